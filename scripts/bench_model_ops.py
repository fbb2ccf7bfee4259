"""The [model] tensor operations' launches on one GPU (informational; bench.py is the project's
benchmark): pkc_combine_fwd / pkc_combine_bwd for CONCAT and MULT, exact fp32, at
  * B = 128 rows x N = 1024 (a frame batch: launch latency is expected to dominate), and
  * M = 2400 rows x N = 1100 (the T * B rows of a sequence batch),
each timed with HIP events around single launches (median over many) and around groups of
back-to-back launches (median over groups), with the GB/s their algorithmic bytes come to against
the 8 TB/s HBM rate:  forward CONCAT 8 M N (one read and one write of every element), MULT 12 M N;
backward (one slab) CONCAT 8 M N, MULT 20 M N (g, a and b read, da and db written).
The same elementwise operations on torch-ROCm in the same process, for comparison.

Then one training step of a two-branch model at B = 128 (MLP 440 -> 1024 BatchNorm relu on each of
two streams, out = mult(a, b), 1928-way head, bf16 operands as in bench.py): the eager step, the
captured step, and the captured step with and without the combine node's two launches
(Engine.step_cost_of: the launches timed where they run, inside the step).
Writes profiles/model_ops_step.json.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-kaldi-cgs_amd"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

HBM_GBS = 8000.0
SHAPES = [("B128_N1024", 128, 512, 512), ("M2400_N1100", 2400, 548, 552)]


def timed(fn, steps, reps):
    """Median / min ms per call over `reps` event-bracketed groups of `steps` calls."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(steps)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return dict(median_ms=statistics.median(out), min_ms=min(out), max_ms=max(out), groups=reps,
                steps_per_group=steps)


def launch_times(fn, nbytes, singles, group, reps):
    """One launch: events around single launches (median of `singles`) and around groups."""
    fn(10)
    torch.cuda.synchronize()
    one = []
    for _ in range(singles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(1)
        e1.record()
        torch.cuda.synchronize()
        one.append(e0.elapsed_time(e1) * 1e3)
    b2b = timed(fn, group, reps)
    us = 1e3 * b2b["median_ms"]
    return dict(algorithmic_bytes=nbytes, single_us_median=statistics.median(one),
                single_us_min=min(one), single_samples=singles, back_to_back_us_median=us,
                back_to_back_us_min=1e3 * b2b["min_ms"], back_to_back_group=group,
                back_to_back_gbs=nbytes / (us * 1e-6) / 1e9,
                back_to_back_frac_hbm=nbytes / (us * 1e-6) / 1e9 / HBM_GBS)


def kernel_section(a, L):
    dev = "cuda"
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for tag, M, Na, Nb in SHAPES:
        for op in ("concatenate", "mult"):
            na, nb = (Na, Nb) if op == "concatenate" else (Na + Nb, Na + Nb)
            N = Na + Nb
            ta, tb = torch.randn(M, na, device=dev), torch.randn(M, nb, device=dev)
            out, g = torch.empty(M, N, device=dev), torch.randn(M, N, device=dev)
            da, db = torch.empty(M, na, device=dev), torch.empty(M, nb, device=dev)
            ca = L.CombineArgs(op=L.COMBINE[op], M=M, Na=na, Nb=nb, a=ta.data_ptr(), lda=na,
                               b=tb.data_ptr(), ldb=nb, out=out.data_ptr(), nslab=1,
                               gslab=g.data_ptr(), slab_stride=M * N, da=da.data_ptr(),
                               db=db.data_ptr())

            def fwd(n):
                for _ in range(n):
                    L.call("pkc_combine_fwd", C.byref(ca), s)

            def bwd(n):
                for _ in range(n):
                    L.call("pkc_combine_bwd", C.byref(ca), s)

            cat = op == "concatenate"
            if cat:
                def t_fwd(n):
                    for _ in range(n):
                        torch.cat((ta, tb), 1, out=out)

                def t_bwd(n):
                    for _ in range(n):
                        da.copy_(g[:, :na])
                        db.copy_(g[:, na:])
            else:
                def t_fwd(n):
                    for _ in range(n):
                        torch.mul(ta, tb, out=out)

                def t_bwd(n):
                    for _ in range(n):
                        torch.mul(g, tb, out=da)
                        torch.mul(g, ta, out=db)
            fb, bb = 4.0 * M * N * (2 if cat else 3), 4.0 * M * N * (2 if cat else 5)
            key = "%s_%s" % (tag, "concat" if cat else "mult")
            res[key] = dict(M=M, N=N, Na=na, Nb=nb,
                            pkc_combine_fwd=launch_times(fwd, fb, a.singles, a.group, a.reps),
                            pkc_combine_bwd=launch_times(bwd, bb, a.singles, a.group, a.reps),
                            torch_fwd=launch_times(t_fwd, fb, a.singles, a.group, a.reps),
                            torch_bwd=launch_times(t_bwd, bb, a.singles, a.group, a.reps))
    return res


def step_section(a, L):
    import pkc.neural_networks as NN
    from cases import MLP_DEF
    from pkc.engine import Engine, parse_model
    dev, B, F, H, NC = "cuda", 128, 440, 1024, 1928
    opt = dict(arch_opt="rmsprop", arch_lr="0.0004", opt_momentum="0.0", opt_alpha="0.95",
               opt_eps="1e-8", opt_centered="False", opt_weight_decay="0.0", arch_freeze="False")
    body = dict(MLP_DEF, **opt, dnn_lay=str(H), dnn_act="relu", dnn_use_batchnorm="True",
                dnn_use_laynorm="False", dnn_drop="0.0")
    archs = {"MLP_a": dict(body, arch_name="MLP_a"), "MLP_b": dict(body, arch_name="MLP_b"),
             "MLP_h": dict(body, arch_name="MLP_h", dnn_lay=str(NC), dnn_act="softmax",
                           dnn_use_batchnorm="False")}
    model = ("out_a=compute(MLP_a,fa)\nout_b=compute(MLP_b,fb)\nout_m=mult(out_a,out_b)\n"
             "out_h=compute(MLP_h,out_m)\nloss_final=cost_nll(out_h,lab)\n"
             "err_final=cost_err(out_h,lab)")
    nets = {}
    for k, inp in (("MLP_a", F), ("MLP_b", F), ("MLP_h", H)):
        torch.manual_seed(1)
        np.random.seed(1)
        nets[k] = NN.MLP(archs[k], inp).to(dev).train()
    rs = np.random.RandomState(0)
    nb = 64
    X = torch.from_numpy(rs.randn(nb * B, 2 * F).astype(np.float32)).to(dev)
    lab = torch.from_numpy(rs.randint(0, NC, size=(nb * B, 1)).astype(np.int32)).to(dev)
    eng = Engine(nets, archs, parse_model(model), {"fa": (0, F), "fb": (F, 2 * F)}, ["lab"], batch=B,
                 seed=1, prec=L.PREC_BF16)
    eng.bind_chunk(X, lab, nb * B)

    def steps(n):
        for _ in range(n):              # (the device batch counter wraps over the chunk)
            eng.train_step()

    steps(a.warmup)
    torch.cuda.synchronize()
    res = dict(model="2 x (440 -> 1024 BN relu) -> mult -> 1928 softmax", batch=B, prec="bf16",
               eager=timed(steps, a.steps, a.reps))
    eng.prof = []
    eng.train_step()
    torch.cuda.synchronize()
    res["launches_per_eager_step"] = len(eng.prof)
    res["combine_in_eager_step_us"] = {lbl.split(" ")[0]: e0.elapsed_time(e1) * 1e3
                                       for (lbl, fn, _, _, e0, e1, _) in eng.prof
                                       if fn.startswith("pkc_combine")}
    eng.prof = None
    node = eng.produced["out_m"]
    labels = ["combine_fwd %s %dx%d" % (node.name, B, node.N),
              "combine_bwd %s %dx%d" % (node.name, B, node.N)]
    cost, full = eng.step_cost_of(labels, reps=a.graph_reps)
    res["captured_step_us"] = full
    res["captured_step_without_combine_us"] = full - cost
    res["combine_launches_in_step_us"] = cost
    res["note"] = ("captured_*: best of 3 groups of %d replays (Engine.step_cost_of); without the "
                   "combine launches the head reads a stale product, the launch sequence is "
                   "otherwise the same" % a.graph_reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--singles", type=int, default=100)
    ap.add_argument("--group", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--graph-reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_ops_step.json"))
    a = ap.parse_args()
    from pkc import _lib as L
    L.lib()
    res = dict(device=torch.cuda.get_device_name(0), hbm_gbs_reference=HBM_GBS,
               launches=kernel_section(a, L), two_branch_step=step_section(a, L))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

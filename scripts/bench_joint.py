"""One training step of the joint speech-enhancement + recognition recipe
(cfg/TIMIT_baselines/TIMIT_joint_training_liGRU_fbank.cfg) on one GPU (informational; bench.py is
the project's benchmark): two 40-dim fbank streams, liGRU_SE 3 x 55 bidirectional -> MLP_SE 40
linear -> liGRU_SR 4 x 55 bidirectional -> 1928-way cd and 48-way mono heads, loss_final = loss_cd
+ loss_mono + mse(out_dnn_SE, fbank_clean), RMSprop, B = 8 sentences, exact fp32.

Times, in this process and in this order, with HIP events around groups of steps:
  1. the pkc Engine step, eager and replayed from the captured sequence graph;
  2. the pkc_mse_fused launch: inside an eager step (events around the single launch, several
     steps) and back to back on the step's own buffers (groups of launches), with the GB/s its
     12 * M * N bytes of algorithmic traffic come to;
  3. the same step of the restatement tests/joint_ref.py on torch-ROCm (oracle.nets modules on the
     GPU, torch autograd and torch.optim.RMSprop).
Writes profiles/joint_se_step.json.
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-kaldi-cgs_amd"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

RMS = dict(arch_opt="rmsprop", arch_lr="0.0004", opt_momentum="0.0", opt_alpha="0.95",
           opt_eps="1e-8", opt_centered="False", opt_weight_decay="0.0", arch_freeze="False")
MODEL = ("out_dnn1=compute(liGRU_SE,fbank_rev)\nout_dnn_SE=compute(MLP_SE,out_dnn1)\n"
         "out_dnn2=compute(liGRU_SR,out_dnn_SE)\nout_dnn3=compute(MLP_layers,out_dnn2)\n"
         "out_dnn4=compute(MLP_layers2,out_dnn2)\nloss_mono=cost_nll(out_dnn4,lab_mono)\n"
         "loss_mono_w=mult_constant(loss_mono,1.0)\nloss_se=mse(out_dnn_SE,fbank_clean)\n"
         "loss_se_w=mult_constant(loss_se,1.0)\nloss_cd=cost_nll(out_dnn3,lab_cd)\n"
         "loss_sum1=sum(loss_cd,loss_mono_w)\nloss_final=sum(loss_sum1,loss_se_w)\n"
         "err_final=cost_err(out_dnn3,lab_cd)")
FD, N_CD, N_MONO = 40, 1928, 48
HBM_GBS = 8000.0


def timed(fn, steps, reps):
    """Median / min ms per step over `reps` event-bracketed groups of `steps` calls."""
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


def sections():
    from cases import LIGRU_DEF

    def rec(name, n):
        return dict(LIGRU_DEF, arch_name=name, ligru_lay=",".join(["55"] * n),
                    ligru_drop=",".join(["0.2"] * n), ligru_use_laynorm=",".join(["False"] * n),
                    ligru_use_batchnorm=",".join(["True"] * n), ligru_act=",".join(["relu"] * n),
                    **RMS)
    mlp = dict(dnn_use_laynorm_inp="False", dnn_use_batchnorm_inp="False", to_do="train",
               dnn_drop="0.0", dnn_use_batchnorm="False", dnn_use_laynorm="False", **RMS)
    return [(rec("liGRU_SE", 3), "liGRU", FD), (dict(mlp, arch_name="MLP_SE", dnn_lay=str(FD),
                                                     dnn_act="linear"), "MLP", 110),
            (rec("liGRU_SR", 4), "liGRU", FD),
            (dict(mlp, arch_name="MLP_layers", dnn_lay=str(N_CD), dnn_act="softmax"), "MLP", 110),
            (dict(mlp, arch_name="MLP_layers2", dnn_lay=str(N_MONO), dnn_act="softmax"), "MLP", 110)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=300, help="padded length T of every batch (<= 1000)")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--torch-steps", type=int, default=2)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_se_step.json"))
    a = ap.parse_args()
    import joint_ref as JR
    import pkc.neural_networks as NN
    from oracle import nets as ON
    from oracle import run as OR
    from pkc import _lib as L
    from pkc.engine import Engine, parse_model

    B, T, dev = a.batch, min(a.frames, 1000), "cuda"
    nets, tnets, opts, seq = {}, {}, {}, {}
    for o, cls, inp in sections():
        torch.manual_seed(1)
        np.random.seed(1)
        k = o["arch_name"]
        nets[k], tnets[k], opts[k], seq[k] = getattr(NN, cls)(o, inp), getattr(ON, cls)(o, inp), o, cls == "liGRU"
        tnets[k].load_state_dict(nets[k].state_dict())
        nets[k].to(dev).train()
        tnets[k].to(dev).train()
    rs = np.random.RandomState(0)
    nb = 4                                       # batches in the chunk, every one padded to T
    lens = np.concatenate([np.sort(rs.randint(T // 2, T, size=B - 1)).tolist() + [T]
                           for _ in range(nb)]).astype(np.int64)
    end = np.cumsum(lens)
    clean = rs.randn(end[-1], FD).astype(np.float32)
    rev = (clean + 0.5 * np.roll(clean, 1, 0) + 0.3 * rs.randn(end[-1], FD)).astype(np.float32)
    X = torch.from_numpy(np.concatenate([rev, clean], 1)).to(dev)
    lab = torch.from_numpy(np.stack([rs.randint(0, N_CD, end[-1]), rs.randint(0, N_MONO, end[-1])],
                                    1).astype(np.int32)).to(dev)
    fea_cols = {"fbank_rev": (0, FD), "fbank_clean": (FD, 2 * FD)}
    M = T * B
    res = dict(shape=dict(batch=B, frames=T, rows=M, streams="2 x %d" % FD, liGRU_SE="3 x 55 bidir",
                          liGRU_SR="4 x 55 bidir", heads="%d / %d" % (N_CD, N_MONO)),
               device=torch.cuda.get_device_name(0), prec="fp32")

    def make_engine():
        eng = Engine(nets, opts, parse_model(MODEL), fea_cols, ["lab_cd", "lab_mono"], batch=B,
                     max_len=T, seed=1)
        eng.bind_chunk(X, lab, end[-1], end_index=end)
        return eng

    eng = make_engine()
    rng = random.Random(7)

    def pkc_steps(n):
        for _ in range(n):
            if eng.snt + B > len(lens):
                eng.snt = 0
            eng.train_step(batch=eng.next_seq_batch(rng))

    pkc_steps(a.warmup)
    torch.cuda.synchronize()
    res["pkc_eager"] = timed(pkc_steps, a.steps, a.reps)
    # the mse launch inside eager steps: events around every launch of a step (Engine._k)
    in_step = []
    for _ in range(a.reps):
        if eng.snt + B > len(lens):
            eng.snt = 0
        eng.prof = []
        eng.train_step(batch=eng.next_seq_batch(rng))
        torch.cuda.synchronize()
        in_step += [e0.elapsed_time(e1) * 1e3 for (lbl, fn, _, _, e0, e1, _) in eng.prof
                    if fn == "pkc_mse_fused"]
        res["pkc_launches_per_step"] = len(eng.prof)
        eng.prof = None
    # ... and back to back on the step's own buffers (y = MLP_SE's output, the target a column
    # range of the batch buffer, dy the slab in front of liGRU_SR's layer-0 dX slabs)
    se = eng.produced["out_dnn_SE"]
    t = eng.mse_terms[0]
    buf, st = eng._mse_slabs(se)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def mse_launches(n):
        for _ in range(n):
            L.call("pkc_mse_fused", M, FD, L.ptr(se.out), FD, C.c_void_p(eng.x.data_ptr() + 4 * t.c0),
                   eng.F, C.c_float(1.0), L.ptr(buf), FD, L.ptr(t.row_loss), s)

    mse_launches(20)
    torch.cuda.synchronize()
    b2b = timed(mse_launches, 200, a.reps)
    nbytes = 12.0 * M * FD
    us_step, us_b2b = statistics.median(in_step), 1e3 * b2b["median_ms"]
    res["pkc_mse_fused"] = dict(
        M=M, N=FD, algorithmic_bytes=nbytes, in_step_us_median=us_step, in_step_us_min=min(in_step),
        in_step_samples=len(in_step), in_step_gbs=nbytes / (us_step * 1e-6) / 1e9,
        back_to_back_us_median=us_b2b, back_to_back_us_min=1e3 * b2b["min_ms"],
        back_to_back_gbs=nbytes / (us_b2b * 1e-6) / 1e9,
        back_to_back_frac_hbm=nbytes / (us_b2b * 1e-6) / 1e9 / HBM_GBS)
    if eng.capture():
        pkc_steps(2 * nb)                        # every batch has the same T: one graph
        torch.cuda.synchronize()
        res["pkc_graph"] = timed(pkc_steps, a.steps, a.reps)
        res["pkc_graph"]["captures"] = eng.seq_captures

    # the restatement on torch-ROCm: same data, torch autograd, torch.optim.RMSprop
    lines = OR.parse_model(MODEL)
    oopt = {k: ON.make_optimizer(tnets[k].parameters(), opts[k]) for k in tnets}
    ds = torch.cat([X, lab.float()], 1)
    lab_cols = {"lab_cd": 2 * FD, "lab_mono": 2 * FD + 1}
    state = dict(i=0)
    rng_t = random.Random(7)
    endl = end.tolist()

    def torch_steps(n):
        with torch.device(dev):
            for _ in range(n):
                i = state["i"] % nb
                state["i"] += 1
                inp = torch.zeros(T, B, ds.shape[1])
                for k in range(B):
                    ln = int(lens[i * B + k])
                    left = rng_t.randint(0, T - ln)
                    b0 = endl[i * B + k] - ln
                    inp[left:left + ln, k] = ds[b0:b0 + ln]
                JR.train_step(lines, tnets, oopt, seq, fea_cols, lab_cols, inp, T, B)

    torch_steps(1)
    torch.cuda.synchronize()
    res["torch_rocm"] = timed(torch_steps, a.torch_steps, a.torch_reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

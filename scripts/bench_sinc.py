"""One training step of the TIMIT_SincNet_raw body on one GPU (informational; bench.py is the
project's benchmark): SincNet 3200 -> 128/60/60/60 filters, len 128 (129 taps)/5/5/3, pool 3/3/3/2,
LayerNorm on the input and every layer, relu, B = 128 -> MLP 4 x 1024 (BatchNorm, relu) + a
1928-way softmax head, exact fp32, SGD.

Times, in this process and in this order, with HIP events around groups of steps:
  1. the pkc Engine step, eager and as captured multi-step graphs, plus a per-launch breakdown of
     one eager step (Engine.profile_step) with each conv / sinc kernel's TF/s and GB/s;
  2. the same step of the CPU restatement tests/sinc_ref.py moved to the GPU (torch's own sin /
     conv1d / max_pool1d / autograd / torch.optim.SGD).
Writes profiles/sinc_raw_step.json.
"""
import argparse
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

SGD = dict(arch_lr="0.001", arch_opt="sgd", opt_momentum="0.0", opt_weight_decay="0.0",
           opt_dampening="0.0", opt_nesterov="False", arch_freeze="False")
SINC_OPTS = dict(sinc_N_filt="128,60,60,60", sinc_len_filt="128,5,5,3",
                 sinc_max_pool_len="3,3,3,2", sinc_use_laynorm_inp="True",
                 sinc_use_batchnorm_inp="False", sinc_use_laynorm="True,True,True,True",
                 sinc_use_batchnorm="False,False,False,False", sinc_act="relu,relu,relu,relu",
                 sinc_drop="0.0,0.0,0.0,0.0", sinc_sample_rate="16000", sinc_min_low_hz="50",
                 sinc_min_band_hz="50", arch_name="sinc", **SGD)
MODEL = ("out1=compute(sinc,fea)\nout2=compute(head,out1)\nloss_final=cost_nll(out2,lab)\n"
         "err_final=cost_err(out2,lab)")
FP32_MFMA_TFLOPS, HBM_GBS = 157.0, 8000.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sinc_raw_step.json"))
    a = ap.parse_args()
    import sinc_ref
    from cases import MLP_DEF
    from oracle import nets as ON
    from pkc.engine import Engine, parse_model
    from pkc.neural_networks import MLP, SincNet

    B, F_, nout, dev = a.batch, 3200, 1928, "cuda"
    hopts = dict(MLP_DEF, arch_name="head", dnn_lay="1024,1024,1024,1024,%d" % nout,
                 dnn_act="relu,relu,relu,relu,softmax", dnn_drop="0.0,0.0,0.0,0.0,0.0",
                 dnn_use_batchnorm="True,True,True,True,False",
                 dnn_use_laynorm="False,False,False,False,False", **SGD)
    torch.manual_seed(1)
    nets = {"sinc": SincNet(SINC_OPTS, F_)}
    nets["head"] = MLP(hopts, nets["sinc"].out_dim)
    tnets = {"sinc": sinc_ref.RefSincNet(SINC_OPTS, F_),
             "head": ON.MLP(hopts, nets["sinc"].out_dim)}
    for k in nets:
        tnets[k].load_state_dict(nets[k].state_dict())
        nets[k].to(dev).train()
        tnets[k].to(dev).train()
    rs = np.random.RandomState(0)
    nb = 16
    X = torch.from_numpy(rs.randn(B * nb, F_).astype(np.float32)).to(dev)
    lab = torch.from_numpy(rs.randint(0, nout, size=(B * nb, 1)).astype(np.int32)).to(dev)

    res = dict(shape=dict(batch=B, inp=F_, sinc=SINC_OPTS["sinc_N_filt"], mlp=hopts["dnn_lay"]),
               device=torch.cuda.get_device_name(0), prec="fp32")
    eng = Engine(nets, {"sinc": SINC_OPTS, "head": hopts}, parse_model(MODEL), {"fea": (0, F_)},
                 ["lab"], batch=B)
    eng.bind_chunk(X, lab, B * nb)
    eng.train_steps(a.warmup)
    torch.cuda.synchronize()
    res["pkc_eager"] = timed(lambda n: eng.train_steps(n), a.steps, a.reps)
    prof = eng.profile_step()
    rows = []
    for label, fn, flops, nbytes, ms in prof:
        r = dict(label=label, fn=fn, us=1e3 * ms)
        if flops:
            r["tflops"] = flops / (ms * 1e-3) / 1e12
            r["frac_fp32_mfma_peak"] = r["tflops"] / FP32_MFMA_TFLOPS
        if nbytes:
            r["gbs"] = nbytes / (ms * 1e-3) / 1e9
            r["frac_hbm"] = r["gbs"] / HBM_GBS
        rows.append(r)
    res["pkc_launches"] = rows
    res["pkc_conv_us"] = sum(r["us"] for r in rows if r["fn"].startswith("pkc_conv"))
    res["pkc_sinc_us"] = sum(r["us"] for r in rows if r["fn"].startswith("pkc_sinc"))
    # layer 0 (C_in = 1, 129 taps, 128 filters over 3072 positions): 2 x 13 GFLOP per step
    res["pkc_layer0_conv_us"] = sum(r["us"] for r in rows if r["fn"].startswith("pkc_conv1d")
                                    and r["label"].endswith("sinc.conv0"))
    res["pkc_step_sum_us"] = sum(r["us"] for r in rows)
    if eng.capture(steps_per_graph=8):
        eng.train_steps(a.warmup)
        torch.cuda.synchronize()
        res["pkc_graph"] = timed(lambda n: eng.train_steps(n), a.steps, a.reps)

    # torch-ROCm's own sin / conv1d: the restatement on the GPU, same data, torch.optim.SGD
    params = [p for k in tnets for p in tnets[k].parameters()]
    opt = torch.optim.SGD(params, lr=float(SGD["arch_lr"]))
    labl = lab.long().view(-1)
    state = dict(i=0)

    def torch_steps(n):
        for _ in range(n):
            i = state["i"] % nb
            state["i"] += 1
            y = tnets["head"](tnets["sinc"](X[i * B:(i + 1) * B]))
            loss = torch.nn.functional.nll_loss(y, labl[i * B:(i + 1) * B])
            opt.zero_grad()
            loss.backward()
            opt.step()

    torch_steps(a.warmup)
    torch.cuda.synchronize()
    res["torch_rocm"] = timed(torch_steps, a.steps, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in res if k != "pkc_launches"}))
    for r in rows:
        print("%-40s %8.1f us %s" % (r["label"], r["us"],
                                      "%.2f TF/s" % r["tflops"] if "tflops" in r else ""))


if __name__ == "__main__":
    main()

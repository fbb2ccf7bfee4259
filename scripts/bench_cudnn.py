"""One training step of the *_cudnn architectures on one GPU (informational; bench.py is the
project's benchmark): a 4-layer bidirectional LSTM_cudnn / GRU_cudnn / RNN_cudnn stack over 440-wide
features with a 1928-way softmax head, batches padded to T = 300, exact fp32, inter-layer dropout
0.2, SGD — at hidden 550 with B = 8 and at hidden 1024 with B = 16.

Times, in this process and per shape and class, with HIP events around groups of steps:
  1. the pkc Engine step, eager and replayed from the captured per-T graph, in ms per step and in
     us per time step and layer (forward + BPTT), plus the per-launch breakdown of one eager step;
  2. torch-ROCm's own nn.LSTM / GRU / RNN (MIOpen) + Linear + log_softmax, autograd and
     torch.optim.SGD on the same shapes;
  3. for GRU_cudnn, pkc's two-phase reference `GRU` (no BatchNorm, tanh) at the same shape.
Writes profiles/cudnn_step.json.
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

SGD = dict(arch_lr="0.01", arch_opt="sgd", opt_momentum="0.0", opt_weight_decay="0.0",
           opt_dampening="0.0", opt_nesterov="False", arch_freeze="False")
MODEL = ("out1=compute(rnn,fea)\nout2=compute(head,out1)\nloss_final=cost_nll(out2,lab)\n"
         "err_final=cost_err(out2,lab)")
F_, NOUT, T, LAYERS, DROP = 440, 1928, 300, 4, 0.2


def timed(fn, steps, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(steps)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    med = statistics.median(out)
    return dict(median_ms=med, min_ms=min(out), max_ms=max(out), groups=reps, steps_per_group=steps,
                us_per_step_layer=1e3 * med / (T * LAYERS))


def pkc_run(cls, opts, H, B, a):
    import pkc.engine as E
    import pkc.neural_networks as NN
    from cases import MLP_DEF
    from pkc.engine import Engine, parse_model
    hopts = dict(MLP_DEF, arch_name="head", dnn_lay=str(NOUT), dnn_act="softmax", dnn_drop="0.0",
                 dnn_use_batchnorm="False", dnn_use_laynorm="False", **SGD)
    torch.manual_seed(1)
    nets = {"rnn": getattr(NN, cls)(opts, F_)}
    nets["head"] = NN.MLP(hopts, nets["rnn"].out_dim)
    for n in nets.values():
        n.to("cuda").train()
    nb = 4
    rs = np.random.RandomState(0)
    end = np.cumsum(np.full(B * nb, T))
    X = torch.from_numpy(rs.randn(end[-1], F_).astype(np.float32)).cuda()
    lab = torch.from_numpy(rs.randint(0, NOUT, size=(end[-1], 1)).astype(np.int32)).cuda()
    res = {}
    for graphs in (False, True):
        eng = Engine(nets, {"rnn": opts, "head": hopts}, parse_model(MODEL), {"fea": (0, F_)},
                     ["lab"], batch=B, max_len=T, seed=1)
        if graphs and not eng.capture():
            break
        eng.bind_chunk(X, lab, end[-1], end_index=end)

        def steps(n, eng=eng):
            for _ in range(n):
                if eng.snt + B > len(eng.sent_beg):
                    eng.snt = 0
                eng.train_step()
        steps(a.warmup)
        torch.cuda.synchronize()
        res["graph" if graphs else "eager"] = timed(steps, a.steps, a.reps)
        if not graphs:
            res["rec_forms"] = eng.rec_forms()
            eng.prof = []
            steps(1)
            torch.cuda.synchronize()
            agg = {}
            for (label, fn, fl, nbytes, e0, e1, _) in eng.prof:
                key = label.split(" T=")[0] if "loop" in label else fn
                c = agg.setdefault(key, dict(us=0.0, launches=0))
                c["us"] += 1e3 * e0.elapsed_time(e1)
                c["launches"] += 1
            eng.prof = None
            res["entry_points"] = dict(sorted(agg.items(), key=lambda kv: -kv[1]["us"]))
        del eng
    return res


def torch_run(cls, H, B, a):
    kind = cls.split("_")[0]
    rnn = getattr(torch.nn, kind)(F_, H, LAYERS, dropout=DROP, bidirectional=True).cuda()
    head = torch.nn.Linear(2 * H, NOUT).cuda()
    params = list(rnn.parameters()) + list(head.parameters())
    opt = torch.optim.SGD(params, lr=float(SGD["arch_lr"]))
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.randn(T, B, F_).astype(np.float32)).cuda()
    lab = torch.from_numpy(rs.randint(0, NOUT, size=(T * B,))).cuda()

    def steps(n):
        for _ in range(n):
            y = torch.log_softmax(head(rnn(x)[0]).view(T * B, NOUT), dim=1)
            loss = torch.nn.functional.nll_loss(y, lab)
            opt.zero_grad()
            loss.backward()
            opt.step()
    steps(a.warmup)
    torch.cuda.synchronize()
    return timed(steps, a.steps, a.reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cudnn_step.json"))
    a = ap.parse_args()
    from cases import GRU_DEF
    res = dict(device=torch.cuda.get_device_name(0), prec="fp32", T=T, layers=LAYERS, inp=F_,
               head=NOUT, dropout=DROP, shapes=[])
    for H, B in ((550, 8), (1024, 16)):
        row = dict(hidden=H, batch=B)
        for cls in ("LSTM_cudnn", "GRU_cudnn", "RNN_cudnn"):
            opts = dict(arch_name="rnn", hidden_size=str(H), num_layers=str(LAYERS), bias="True",
                        batch_first="False", dropout=str(DROP), bidirectional="True", **SGD)
            if cls == "RNN_cudnn":
                opts["nonlinearity"] = "tanh"
            row[cls] = dict(pkc=pkc_run(cls, opts, H, B, a), torch_rocm=torch_run(cls, H, B, a))
            print(H, B, cls, json.dumps({k: (v["median_ms"] if "median_ms" in v else None)
                                         for k, v in row[cls]["pkc"].items() if isinstance(v, dict)}),
                  "torch", row[cls]["torch_rocm"]["median_ms"], flush=True)
        lay = ",".join([str(H)] * LAYERS)
        rep = lambda v: ",".join([v] * LAYERS)          # noqa: E731
        gopts = dict(GRU_DEF, arch_name="rnn", gru_lay=lay, gru_drop=rep(str(DROP)),
                     gru_use_batchnorm=rep("False"), gru_use_laynorm=rep("False"),
                     gru_act=rep("tanh"), gru_bidir="True", gru_orthinit="False", **SGD)
        row["pkc_GRU_two_phase"] = pkc_run("GRU", gopts, H, B, a)
        print(H, B, "GRU two-phase", row["pkc_GRU_two_phase"]["eager"]["median_ms"], flush=True)
        res["shapes"].append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()

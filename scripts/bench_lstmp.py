"""One training step of the projected LSTM (LSTM_cudnn with proj_size = P) on one GPU, beside the
plain LSTM_cudnn (proj_size = 0) at the same hidden size in the same process (informational; bench.py
is the project's benchmark): 4 bidirectional layers over 440-wide features with a 1928-way softmax
head, batches padded to T = 300, exact fp32, inter-layer dropout 0.2, SGD — hidden 1024 with
P in {256, 512} at B = 16, and hidden 550 with P = 160 at B = 8.

Times per shape, with HIP events around groups of steps, the variants' groups interleaved (one group
of each per round): the pkc Engine step, eager and replayed from the captured per-T graph, in ms per
step and in us per time step and layer (forward + BPTT), plus the per-launch breakdown of one eager
step.  Writes profiles/lstmp_step.json.
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


def group(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(steps)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def summary(out, steps):
    med = statistics.median(out)
    return dict(median_ms=med, min_ms=min(out), max_ms=max(out), groups=len(out),
                steps_per_group=steps, us_per_step_layer=1e3 * med / (T * LAYERS))


def make_engine(H, P, B, graphs):
    import pkc.neural_networks as NN
    from cases import MLP_DEF
    from pkc.engine import Engine, parse_model
    opts = dict(arch_name="rnn", hidden_size=str(H), proj_size=str(P), num_layers=str(LAYERS),
                bias="True", batch_first="False", dropout=str(DROP), bidirectional="True", **SGD)
    hopts = dict(MLP_DEF, arch_name="head", dnn_lay=str(NOUT), dnn_act="softmax", dnn_drop="0.0",
                 dnn_use_batchnorm="False", dnn_use_laynorm="False", **SGD)
    torch.manual_seed(1)
    nets = {"rnn": NN.LSTM_cudnn(opts, F_)}
    nets["head"] = NN.MLP(hopts, nets["rnn"].out_dim)
    for n in nets.values():
        n.to("cuda").train()
    rs = np.random.RandomState(0)
    end = np.cumsum(np.full(B * 4, T))
    X = torch.from_numpy(rs.randn(end[-1], F_).astype(np.float32)).cuda()
    lab = torch.from_numpy(rs.randint(0, NOUT, size=(end[-1], 1)).astype(np.int32)).cuda()
    eng = Engine(nets, {"rnn": opts, "head": hopts}, parse_model(MODEL), {"fea": (0, F_)}, ["lab"],
                 batch=B, max_len=T, seed=1)
    if graphs and not eng.capture():
        return None, None
    eng.bind_chunk(X, lab, end[-1], end_index=end)

    def steps(n):
        for _ in range(n):
            if eng.snt + B > len(eng.sent_beg):
                eng.snt = 0
            eng.train_step()
    return eng, steps


def breakdown(eng, steps):
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
    return dict(sorted(agg.items(), key=lambda kv: -kv[1]["us"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstmp_step.json"))
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), prec="fp32", T=T, layers=LAYERS, inp=F_,
               head=NOUT, dropout=DROP, shapes=[])
    for H, B, projs in ((1024, 16, (256, 512)), (550, 8, (160,))):
        row = dict(hidden=H, batch=B, variants={})
        for graphs in (False, True):
            runs = {}
            for P in (0,) + projs:                  # P = 0: the plain LSTM_cudnn, the parent's path
                eng, steps = make_engine(H, P, B, graphs)
                if eng is None:
                    continue
                steps(a.warmup)
                torch.cuda.synchronize()
                runs[P] = (eng, steps, [])
            for _ in range(a.reps):                 # interleaved rounds: one group of each variant
                for P, (eng, steps, out) in runs.items():
                    out.append(group(steps, a.steps))
            for P, (eng, steps, out) in runs.items():
                v = row["variants"].setdefault("proj_size=%d" % P, {})
                v["graph" if graphs else "eager"] = summary(out, a.steps)
                if not graphs:
                    v["rec_forms"] = eng.rec_forms()
                    v["entry_points"] = breakdown(eng, steps)
            del runs
        for k, v in row["variants"].items():
            print(H, B, k, json.dumps({m: round(v[m]["median_ms"], 2) for m in ("eager", "graph")
                                       if m in v}),
                  "us/step/layer", {m: round(v[m]["us_per_step_layer"], 1) for m in ("eager", "graph")
                                    if m in v}, flush=True)
        res["shapes"].append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()

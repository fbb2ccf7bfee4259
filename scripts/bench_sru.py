"""One training step of the SRU architecture on one GPU (informational; bench.py is the project's
benchmark; nothing is gated on these numbers): a 4-layer SRU over 440-wide features with a 1928-way
softmax head, batches padded to T = 300 (the sentence length of scripts/bench_cudnn.py), dropout 0.2
and rnn-dropout 0.1, SGD — 4 x 550 bidirectional with B = 8 and 4 x 1024 (uni-directional) with
B = 16, in fp32 and in bf16 (the projection and dX / dW matmuls; the recurrence is fp32 in both).

In the same session it times, with the same harness, the liGRU C3 body (4 x 550 bidirectional, B = 8,
BatchNorm, relu) and LSTM_cudnn 4 x 1024 (B = 16), so the figures compare like with like.  Per run:
ms per step eager and replayed from the captured graph, us per time step and layer (forward + BPTT),
and the per-launch split of one eager step; for the SRU also the achieved bytes per second of the two
loop launches against their algorithmic bytes, 4 T B n_out (k + 2) forward and
4 T B n_out (2 k + 2) backward (u, c and dy read, dU written), plus the highway input (and its
gradient) of a k = 3 layer.
Writes profiles/sru_step.json.
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
F_, NOUT, T, LAYERS = 440, 1928, 300, 4
HBM_PEAK = 8.0e12          # bytes / s, MI355X


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


def pkc_run(cls, opts, B, prec, a):
    import pkc.neural_networks as NN
    from cases import MLP_DEF
    from pkc import _lib as L
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
                     ["lab"], batch=B, max_len=T, seed=1,
                     prec=L.PREC_BF16 if prec == "bf16" else L.PREC_FP32)
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
                c = agg.setdefault(key, dict(us=0.0, launches=0, bytes=0.0))
                c["us"] += 1e3 * e0.elapsed_time(e1)
                c["launches"] += 1
                c["bytes"] += nbytes
            eng.prof = None
            for key, c in agg.items():
                if key.startswith("sru_") and "loop" in key:
                    c["bytes_per_s"] = c["bytes"] / (1e-6 * c["us"])
                    c["of_hbm_peak"] = c["bytes_per_s"] / HBM_PEAK
            res["entry_points"] = dict(sorted(agg.items(), key=lambda kv: -kv[1]["us"]))
        del eng
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sru_step.json"))
    a = ap.parse_args()
    from cases import LIGRU_DEF
    res = dict(device=torch.cuda.get_device_name(0), T=T, layers=LAYERS, inp=F_, head=NOUT, runs=[])
    rep = lambda v: ",".join([v] * LAYERS)          # noqa: E731

    def sru(H, bidir):
        return dict(arch_name="rnn", sru_hidden_size=str(H), sru_num_layers=str(LAYERS),
                    sru_dropout="0.2", sru_rnn_dropout="0.1", sru_use_tanh="True", sru_use_relu="False",
                    sru_use_selu="False", sru_weight_norm="False", sru_layer_norm="False",
                    sru_bidirectional=str(bidir), sru_is_input_normalized="False",
                    sru_has_skip_term="True", sru_rescale="True", sru_highway_bias="-2.0",
                    sru_n_proj="0", **SGD)
    ligru = dict(LIGRU_DEF, arch_name="rnn", ligru_lay=rep("550"), ligru_drop=rep("0.2"),
                 ligru_use_batchnorm=rep("True"), ligru_use_laynorm=rep("False"),
                 ligru_act=rep("relu"), ligru_bidir="True", **SGD)
    lstm = dict(arch_name="rnn", hidden_size="1024", num_layers=str(LAYERS), bias="True",
                batch_first="False", dropout="0.2", bidirectional="False", **SGD)
    plan = [("SRU 4x550 bidirectional", "SRU", sru(550, True), 8),
            ("liGRU C3 4x550 bidirectional", "liGRU", ligru, 8),
            ("SRU 4x1024", "SRU", sru(1024, False), 16),
            ("LSTM_cudnn 4x1024", "LSTM_cudnn", lstm, 16)]
    for name, cls, opts, B in plan:
        for prec in ("fp32", "bf16"):
            if cls == "LSTM_cudnn" and prec == "bf16":
                continue                      # its step products are exact fp32 in every mode
            row = dict(name=name, cls=cls, batch=B, prec=prec, pkc=pkc_run(cls, opts, B, prec, a))
            print(name, prec, json.dumps({k: round(v["median_ms"], 3) for k, v in row["pkc"].items()
                                          if isinstance(v, dict) and "median_ms" in v}), flush=True)
            res["runs"].append(row)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()

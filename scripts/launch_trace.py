"""The engine's launch sequence as text: for each model, every launch's (label, entry point) of a
few eager training steps, in order, and the step's launch count (Engine.n_launches).  No timing: two
trees that print the same text issue the same launches in the same order with the same labels —
the check of a refactor of pkc.engine (profiles/engine_types_launch_trace_*.txt).

Models, at their benchmarks' smallest sizes and built with the benchmarks' own builders: the C2 MLP
(bench.build) at B = 128 in bf16 and fp32 and at B = 4096 in bf16, the C3 liGRU and C5 LSTM
(scripts/bench_seq.py), LSTM_cudnn (scripts/bench_cudnn.py), the CNN (scripts/bench_cnn.py),
SincNet (scripts/bench_sinc.py) and the HCGS GRU (scripts/bench_gru_hcgs.py).  The B = 128 MLPs
also print graph_launches_per_step after capture().

Frame models go through Engine.profile_step(); sequence models, whose step needs a sentence batch,
through the profile mode profile_step itself uses (Engine.prof) around train_step(batch=...).

Usage: python scripts/launch_trace.py [--models mlp128_bf16,ligru,...] [--steps 3]
"""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "scripts"), os.path.join(ROOT, "pytorch-kaldi-cgs_amd"), ROOT):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def frame_trace(eng, steps):
    out = []
    for _ in range(steps):
        n0 = eng.n_launches
        prof = eng.profile_step()
        out.append(([(label, fn) for label, fn, _, _, _ in prof], eng.n_launches - n0))
    return out


def seq_trace(eng, steps):
    rng = random.Random(7)
    out = []
    for _ in range(steps):
        batch = eng.next_seq_batch(rng)
        n0 = eng.n_launches
        eng.prof = []
        eng.train_step(batch=batch)
        torch.cuda.synchronize()
        prof, eng.prof = eng.prof, None
        out.append(([(e[0], e[1]) for e in prof], eng.n_launches - n0))
    return out


def mlp(prec, batch):
    def run(steps):
        import bench
        from pkc import _lib as L
        eng = bench.build(getattr(L, "PREC_" + prec.upper()), batch, 0, 1)[0]
        tr = frame_trace(eng, steps)
        extra = []
        if batch == 128:
            assert eng.capture()
            extra.append("graph_launches_per_step %r" % eng.graph_launches_per_step)
        return tr, extra
    return run


def seq(cfg_name):
    def run(steps):
        import bench_seq
        eng = bench_seq.build(cfg_name)[0]
        return seq_trace(eng, steps), ["rec_forms %r" % (eng.rec_forms(),)]
    return run


def cudnn(steps):
    import bench_cudnn as BC
    import pkc.neural_networks as NN
    from cases import MLP_DEF
    from pkc.engine import Engine, parse_model
    H, B, nb = 550, 8, 2
    opts = dict(arch_name="rnn", hidden_size=str(H), num_layers=str(BC.LAYERS), bias="True",
                batch_first="False", dropout=str(BC.DROP), bidirectional="True", **BC.SGD)
    hopts = dict(MLP_DEF, arch_name="head", dnn_lay=str(BC.NOUT), dnn_act="softmax", dnn_drop="0.0",
                 dnn_use_batchnorm="False", dnn_use_laynorm="False", **BC.SGD)
    torch.manual_seed(1)
    nets = {"rnn": NN.LSTM_cudnn(opts, BC.F_)}
    nets["head"] = NN.MLP(hopts, nets["rnn"].out_dim)
    for n in nets.values():
        n.to("cuda").train()
    rs = np.random.RandomState(0)
    end = np.cumsum(np.full(B * nb, BC.T))
    X = torch.from_numpy(rs.randn(end[-1], BC.F_).astype(np.float32)).cuda()
    lab = torch.from_numpy(rs.randint(0, BC.NOUT, size=(end[-1], 1)).astype(np.int32)).cuda()
    eng = Engine(nets, {"rnn": opts, "head": hopts}, parse_model(BC.MODEL), {"fea": (0, BC.F_)},
                 ["lab"], batch=B, max_len=BC.T, seed=1)
    eng.bind_chunk(X, lab, end[-1], end_index=end)
    out = []
    for _ in range(steps):
        if eng.snt + B > len(eng.sent_beg):
            eng.snt = 0
        out += seq_trace(eng, 1)
    return out, ["rec_forms %r" % (eng.rec_forms(),)]


def conv(kind):
    def run(steps):
        BM = __import__("bench_" + kind)
        from cases import MLP_DEF
        from pkc.engine import Engine, parse_model
        from pkc.neural_networks import CNN, MLP, SincNet
        B, nout, nb = 128, 1928, 4
        copts, F_, cls = (BM.CNN_OPTS, 440, CNN) if kind == "cnn" else (BM.SINC_OPTS, 3200, SincNet)
        hopts = dict(MLP_DEF, arch_name="head", dnn_lay="1024,1024,1024,1024,%d" % nout,
                     dnn_act="relu,relu,relu,relu,softmax", dnn_drop="0.0,0.0,0.0,0.0,0.0",
                     dnn_use_batchnorm="True,True,True,True,False",
                     dnn_use_laynorm="False,False,False,False,False", **BM.SGD)
        torch.manual_seed(1)
        nets = {kind: cls(copts, F_)}
        nets["head"] = MLP(hopts, nets[kind].out_dim)
        for n in nets.values():
            n.to("cuda").train()
        rs = np.random.RandomState(0)
        X = torch.from_numpy(rs.randn(B * nb, F_).astype(np.float32)).cuda()
        lab = torch.from_numpy(rs.randint(0, nout, size=(B * nb, 1)).astype(np.int32)).cuda()
        eng = Engine(nets, {kind: copts, "head": hopts}, parse_model(BM.MODEL), {"fea": (0, F_)},
                     ["lab"], batch=B)
        eng.bind_chunk(X, lab, B * nb)
        return frame_trace(eng, steps), []
    return run


def gru_hcgs(steps):
    import bench_gru_hcgs as BG
    nets, opts = BG.make_nets("GRU", "[32,2]/[75,75]")
    rs = np.random.RandomState(2234)
    lens = np.sort(rs.randint(150, 451, size=(steps + 1) * BG.B))
    end = np.cumsum(lens)
    N = int(end[-1])
    g = torch.Generator(device="cuda")
    g.manual_seed(2234)
    feats = torch.randn(N, 440, device="cuda", generator=g)
    labs = torch.stack([torch.randint(0, 1928, (N,), device="cuda", generator=g),
                        torch.randint(0, 48, (N,), device="cuda", generator=g)],
                       1).to(torch.int32).contiguous()
    eng = BG.make_engine(nets, opts, "auto", (feats, labs, end, int(lens.max())))
    return seq_trace(eng, steps), ["rec_forms %r" % (eng.rec_forms(),)]


MODELS = {"mlp128_bf16": mlp("bf16", 128), "mlp128_fp32": mlp("fp32", 128),
          "mlp4096_bf16": mlp("bf16", 4096), "ligru": seq("c3"), "lstm": seq("c5"),
          "lstm_cudnn": cudnn, "cnn": conv("cnn"), "sinc": conv("sinc"), "gru_hcgs": gru_hcgs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    for name in a.models.split(","):
        trace, extra = MODELS[name](a.steps)
        print("== model %s" % name)
        for i, (launches, count) in enumerate(trace):
            print("-- step %d: %d launches" % (i, count))
            for label, fn in launches:
                print("%s\t%s" % (fn, label))
        for line in extra:
            print(line)
        sys.stdout.flush()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

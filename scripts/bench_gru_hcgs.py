"""Time-loop cost of HCGS-masked GRU / minimalGRU / RNN layers: block-sparse step kernels
(PKC_RNN_SPARSE=auto) against the dense step kernels on the same masked weights (off), and the
unmasked layer for context.

Shape: config C3's (4 x 550 bidirectional, B = 8 sentences, ReLU, BN, dropout 0.2, heads 1100 ->
1928 cd + 48 mono; synthetic TIMIT-shaped chunk, utterance lengths U[150, 450], 440-dim features)
with the two HCGS settings of SURVEY 8d on W and U: [32,2] / [75,75] and [128,4] / [25,62.5].

Method: the three engines of a cell and setting live in one process and train the same batches in
turn (auto, off, unmasked; the order rotates per group); every layer's forward and BPTT time loop
is bracketed by device events inside its training step (Engine.prof), after its real producers.
Reported: microseconds per time step and layer (mean over the 4 layers), median over the groups
with min / max, and the sparse / dense ratio per group.

Usage: python scripts/bench_gru_hcgs.py [--groups 6] [--warmup 2] [--out profiles/gru_hcgs_step.json]
"""
import argparse
import configparser
import copy
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-kaldi-cgs_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OPT = dict(arch_opt="rmsprop", arch_lr="0.0016", opt_momentum="0.0", opt_alpha="0.95",
           opt_eps="1e-8", opt_centered="False", opt_weight_decay="0.0", arch_freeze="False",
           to_do="train", skip_regularization="True")
SETTINGS = {"[32,2]/[75,75]": ("32,2", "75,75"), "[128,4]/[25,62.5]": ("128,4", "25,62.5")}
CELLS = {"GRU": "gru", "minimalGRU": "minimalgru", "RNN": "rnn"}
MODEL = ("o1=compute(rnn,fea)\no2=compute(head,o1)\no3=compute(mono,o1)\n"
         "lm=cost_nll(o3,lab_mono)\nlmw=mult_constant(lm,1.0)\nlc=cost_nll(o2,lab_cd)\n"
         "loss_final=sum(lc,lmw)\nerr_final=cost_err(o2,lab_cd)")
B, NL, H = 8, 4, 550


def make_nets(cls, setting, seed=2234):
    import pkc.neural_networks as NN
    p = CELLS[cls]
    d = {p + "_lay": ",".join([str(H)] * NL), p + "_drop": ",".join(["0.2"] * NL),
         p + "_use_laynorm_inp": "False", p + "_use_batchnorm_inp": "False",
         p + "_use_laynorm": ",".join(["False"] * NL), p + "_use_batchnorm": ",".join(["True"] * NL),
         p + "_bidir": "True", p + "_act": ",".join(["relu"] * NL), p + "_orthinit": "True"}
    if setting is not None:
        blk, sp = SETTINGS[setting]
        d.update({p + "_hcgs": "True", "hcgsx_block": blk, "hcgsx_sparse": sp, "hcgsh_block": blk,
                  "hcgsh_sparse": sp})
    cfg = configparser.ConfigParser()
    cfg["a1"] = dict(d, arch_name="rnn", **OPT)
    head = dict(dnn_use_laynorm_inp="False", dnn_use_batchnorm_inp="False", arch_name="head",
                dnn_lay="1928", dnn_drop="0.0", dnn_use_batchnorm="False", dnn_use_laynorm="False",
                dnn_act="softmax", **dict(OPT, arch_lr="0.0004"))
    cfg["a2"] = head
    cfg["a3"] = dict(head, arch_name="mono", dnn_lay="48")
    torch.manual_seed(seed)
    np.random.seed(seed)
    rnn = getattr(NN, cls)(cfg["a1"], 440)
    nets = {"rnn": rnn, "head": NN.MLP(cfg["a2"], rnn.out_dim), "mono": NN.MLP(cfg["a3"], rnn.out_dim)}
    for n in nets.values():
        n.cuda().train()
    return nets, {"rnn": cfg["a1"], "head": cfg["a2"], "mono": cfg["a3"]}


def make_engine(nets, opts, sparse, data):
    import pkc.engine as E
    feats, labs, end, max_len = data
    old = E.RNN_SPARSE
    E.RNN_SPARSE = sparse
    try:
        eng = E.Engine(nets, opts, E.parse_model(MODEL), {"fea": (0, 440)}, ["lab_cd", "lab_mono"],
                       batch=B, max_len=max_len, seed=2234)
    finally:
        E.RNN_SPARSE = old
    eng.bind_chunk(feats, labs, int(end[-1]), end_index=end)
    return eng


def timed_step(eng, rng):
    """One training step in profile mode: (us per time step and layer of the forward loops, of the
    BPTT loops), means over the layers"""
    batch = eng.next_seq_batch(rng)
    T = batch[3]
    eng.prof = []
    eng.train_step(batch=batch)
    torch.cuda.synchronize()
    prof, eng.prof = eng.prof, None
    f = [e0.elapsed_time(e1) for (l, _, _, _, e0, e1, _) in prof if l.startswith("rnn_fwd_loop")]
    b = [e0.elapsed_time(e1) for (l, _, _, _, e0, e1, _) in prof if l.startswith("rnn_bwd_loop")]
    assert len(f) == NL and len(b) == NL, (len(f), len(b))
    return 1e3 * sum(f) / (NL * T), 1e3 * sum(b) / (NL * T)


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3),
            "max": round(float(max(v)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", default="GRU,minimalGRU,RNN")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_hcgs_step.json"))
    a = ap.parse_args()
    rs = np.random.RandomState(2234)
    lens = np.sort(rs.randint(150, 451, size=(a.groups + a.warmup) * B))
    end = np.cumsum(lens)
    N = int(end[-1])
    g = torch.Generator(device="cuda")
    g.manual_seed(2234)
    feats = torch.randn(N, 440, device="cuda", generator=g)
    labs = torch.stack([torch.randint(0, 1928, (N,), device="cuda", generator=g),
                        torch.randint(0, 48, (N,), device="cuda", generator=g)],
                       1).to(torch.int32).contiguous()
    data = (feats, labs, end, int(lens.max()))
    out = {"shape": "4x550 bidirectional, B=8, T U[150,450] (length-sorted), fp32 steps",
           "unit": "us per time step and layer", "groups": a.groups, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "results": {}}
    for cls in a.cells.split(","):
        for setting in SETTINGS:
            nets, opts = make_nets(cls, setting)
            plain, popts = make_nets(cls, None)
            engs = {"auto": make_engine(copy.deepcopy(nets), opts, "auto", data),
                    "off": make_engine(copy.deepcopy(nets), opts, "off", data),
                    "unmasked": make_engine(plain, popts, "off", data)}
            forms = {k: e.rec_forms() for k, e in engs.items()}
            slots = [(lb.get("kmap_s_fwd") if lb.get("kmap_fwd") is not None else None,
                      lb.get("kmap_s_bwd") if lb.get("kmap_bwd") is not None else None)
                     for lb in engs["auto"].nodes[0].lbuf]
            rngs = {k: random.Random(7) for k in engs}
            t = {k: {"fwd": [], "bwd": []} for k in engs}
            order = list(engs)
            for i in range(a.warmup + a.groups):
                for k in order:
                    fw, bw = timed_step(engs[k], rngs[k])
                    if i >= a.warmup:
                        t[k]["fwd"].append(fw)
                        t[k]["bwd"].append(bw)
                order = order[1:] + order[:1]
            res = {k: {d: stats(v[d]) for d in v} for k, v in t.items()}
            for d in ("fwd", "bwd"):
                res["sparse/dense " + d] = stats([s / o for s, o in zip(t["auto"][d], t["off"][d])])
            res["forms"] = forms
            res["kmap_slots_per_layer"] = slots
            res["U_density"] = round(float(nets["rnn"].hcgsh[0].mask.detach().mean()), 4)
            out["results"]["%s %s" % (cls, setting)] = res
            print(cls, setting, json.dumps({k: v for k, v in res.items() if k != "forms"}), flush=True)
            del engs, nets, plain
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"wrote": a.out}))


if __name__ == "__main__":
    main()

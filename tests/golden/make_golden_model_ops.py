"""Golden vectors of the [model] tensor operations on produced outputs: the reference's own
utils.model_init + utils.forward_model + loss_final.backward() on the two tiny models of
model_ops_cfg.py — the feed-forward one (sum / mult / avg / sum_constant / mult_constant /
concatenate with a feature operand, dropout 0) and the sequence one (two bidirectional liGRUs on
two streams concatenated into an MLP head) — on the CPU with make_golden's shims.  Runs only where
the reference is present; only data leaves (tests/golden/model_ops/ff.npz, seq.npz: the input
batch, the initial state dicts, every named output, loss, err and every parameter gradient).

It also reruns both with the tests' restatement (tests/model_ops_ref.py) in fp32 from the same
initial state and stores per tensor whether that reproduces the reference's bits (equal/<key>;
eager torch on both sides runs the same operations in the same order — at the time of writing all
23 + 24 tensors are reproduced bit for bit, so the tests ask for torch.equal throughout).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_model_ops.py
"""
import configparser
import os
import sys

import numpy as np
import torch

import make_golden as MG               # the shims (CPU .cuda(), conn_mat) and the helpers
from make_golden import sd_np, utils

sys.path.insert(0, os.path.dirname(MG.OUT))            # tests/: model_ops_ref
sys.path.insert(0, os.path.dirname(os.path.dirname(MG.OUT)))   # the repository root: oracle
import model_ops_cfg as MC  # noqa: E402

SUB = os.path.join(MG.OUT, "model_ops")


def reference_run(archs, model, fea_cols, lab_cols, inp, T, B):
    cfg = configparser.ConfigParser()
    cfg["exp"] = {"use_cuda": "False", "to_do": "train", "seed": "2234"}
    arch_dict = {}
    for i, (a, o) in enumerate(archs.items()):
        sec = "architecture%d" % (i + 1)
        cfg[sec] = {k: str(v) for k, v in o.items()}
        arch_dict[a] = [sec, a, int(o["arch_seq_model"] == "True")]
    fea_dict = {f: [f, "x.scp", "", "0", "0", c0, c1, c1 - c0] for f, (c0, c1) in fea_cols.items()}
    lab_dict = {l: [l, "a", "ali-to-pdf", c] for l, c in lab_cols.items()}
    lines = model.split("\n")
    torch.manual_seed(2234)
    np.random.seed(2234)
    inp_out = dict(fea_dict)
    nns, costs = utils.model_init(inp_out, lines, cfg, arch_dict, False, False, "train")
    out = {}
    for n, net in nns.items():
        sd_np(net, "init/%s/" % n, out)
    outs = utils.forward_model(fea_dict, lab_dict, arch_dict, lines, nns, costs, inp, inp_out, T, B,
                               "train", ["out_h"])
    outs["loss_final"].backward()
    for k, v in outs.items():
        if k not in fea_cols:
            out["out/" + k] = v.detach().numpy().copy()
    for n, net in nns.items():
        for pn, p in net.named_parameters():
            if p.grad is not None:
                out["grad/%s/%s" % (n, pn)] = p.grad.numpy().copy()
    return out


def restated(out, archs, dims, model, fea_cols, lab_cols, inp, T, B, dtype):
    import model_ops_ref as MR
    from oracle.run import parse_model
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)         # (the oracle's recurrent layers start from torch.zeros)
    try:
        state = {a: {k[len("init/%s/" % a):]: torch.from_numpy(v) for k, v in out.items()
                     if k.startswith("init/%s/" % a)} for a in archs}
        nets, _, seq = MR.build(archs, dims, dtype, state=state)
        outs = MR.forward_model(parse_model(model), nets, seq, fea_cols, lab_cols, inp.to(dtype), T, B)
        outs["loss_final"].backward()
    finally:
        torch.set_default_dtype(old)
    res = {"out/" + k: v.detach() for k, v in outs.items() if k not in fea_cols}
    for a, net in nets.items():
        for pn, p in net.named_parameters():
            if p.grad is not None:
                res["grad/%s/%s" % (a, pn)] = p.grad
    return res


def one(tag, archs, dims, model, fea_cols, lab_cols, inp, T, B, extra=None):
    out = {"inp": inp.numpy().copy()}
    out.update(extra or {})
    out.update(reference_run(archs, model, fea_cols, lab_cols, inp, T, B))
    r32 = restated(out, archs, dims, model, fea_cols, lab_cols, inp, T, B, torch.float32)
    keys = [k for k in out if k.startswith(("out/", "grad/"))]
    for k in keys:
        ref = torch.from_numpy(out[k])
        eq = bool(torch.equal(ref.reshape(-1), r32[k].reshape(-1)))
        out["equal/" + k] = np.bool_(eq)
        if not eq:
            d = (ref.reshape(-1).double() - r32[k].reshape(-1).double()).abs().max()
            print("%s %-40s NOT bit-equal: the fp32 restatement is off by %.3g of the tensor's "
                  "scale" % (tag, k, float(d / ref.abs().max().clamp_min(1e-30))))
    print("%s: %d tensors, %d reproduced bit for bit by the fp32 restatement" % (
        tag, len(keys), sum(int(out["equal/" + k]) for k in keys)))
    os.makedirs(SUB, exist_ok=True)
    path = os.path.join(SUB, tag + ".npz")
    np.savez_compressed(path, **out)
    print("written %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


def gen():
    rs = np.random.RandomState(12)
    # feed-forward: B_FF rows of [fa | fb | fc | label]
    B = MC.B_FF
    X = rs.normal(size=(B, 23)).astype(np.float32)
    X[:, 22] = rs.randint(0, MC.N_LAB, size=B)
    archs, dims = MC.ff_archs(drop="0.0")
    one("ff", archs, dims, MC.MODEL_FF, MC.FEA_FF, MC.LAB_FF, torch.from_numpy(X), 0, B)
    # sequence: (T, B, [fa | fb | label]) with left padding (core.py:183-200)
    T, B = max(MC.SEQ_LENS), MC.B_SEQ
    lefts = (0, 2, 1)
    inp = np.zeros((T, B, 18), dtype=np.float32)
    for k, (n, left) in enumerate(zip(MC.SEQ_LENS, lefts)):
        inp[left:left + n, k, :17] = rs.normal(size=(n, 17))
        inp[left:left + n, k, 17] = rs.randint(0, MC.N_LAB, size=n)
    archs, dims = MC.seq_cat_archs()
    one("seq", archs, dims, MC.MODEL_SEQ_CAT, MC.FEA_SEQ, MC.LAB_SEQ, torch.from_numpy(inp), T, B,
        extra=dict(lefts=np.array(lefts), lens=np.array(MC.SEQ_LENS)))


if __name__ == "__main__":
    gen()

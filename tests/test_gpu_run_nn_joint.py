"""pkc.core.run_nn on the joint speech-enhancement + recognition recipe (two feature streams,
liGRU_SE -> MLP_SE -> liGRU_SR -> cd / mono heads, the mse cost) against the reference's own
core.run_nn over a chunk lifecycle: tests/golden/run_nn_joint (make_golden_joint.py, the reference
on CPU with the Kaldi reads shimmed) — train ck0 from the cfg seed, train ck1 resumed from the
REFERENCE-written ck0 checkpoints, valid and forward from the reference's ck1 model, forward
writing two arks (the normalised posteriors to decode and the enhanced features).

Tolerances: those tests/test_gpu_run_nn_parity.py applies to its non-quantised liGRU case — .info
loss 1e-5 relative, err 1e-6, ck1 parameters and RMSprop state 1e-4 relative Frobenius (+ 1e-6
absolute RMS), the posterior ark 1e-4 relative on the log-posterior.  The generator measured the
reference's own fp32 ck1 result 1.9e-6 (worst tensor) from an fp64 rerun of the same steps, far
inside a quarter of 1e-4, so nothing is loosened.  The enhanced-feature ark holds signed linear
outputs (zero crossings make an elementwise relative error meaningless): it is held to 1e-4 of
each utterance's largest magnitude, the measure tests/test_gpu_joint.py uses for out_dnn_SE.

pkc takes forward_out in any order; the reference stops at the LAST name (utils.py:1932), so its
run lists out_dnn_SE first.  Here the cfg lists out_dnn3 first.

The reference's enhanced-feature ark has a header slip: by the time it is written, liGRU_SR's
compute line has re-viewed out_dnn_SE to (T, 1, 13) (utils.py:1927-1928), and write_mat puts
shape[1] = 1 into the column field in front of the T * 13 floats.  pkc writes the (T, 13) matrix
Kaldi can read; the reference's records are parsed here by their known width, and the payloads
(the same floats in the same order) are compared."""
import configparser
import os
import struct

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from joint_cfg import FEA_DIM, SECS, joint_cfg
from joint_ref import unpack
from test_gpu_run_nn_parity import parse_ark, read_info

pytestmark = pytest.mark.gpu
SRC = os.path.join(GOLDEN, "run_nn_joint")


def write_chunk(d, tag, g):
    """The golden utterances as the binary arks pkc's loader reads: <tag>_rev / <tag>_clean scp +
    ark, <tag>.ali/ali_{pdf,phones}.ark."""
    from pkc import data_io as D
    base = os.path.join(d, tag)
    for s in ("rev", "clean"):
        fea = unpack(g, "%s_%s" % (tag, s))
        scp = "%s_%s" % (base, s)
        with open(scp, "w") as f:
            for i, (k, m) in enumerate(fea.items()):
                D.write_mat_path(scp + ".ark", m.reshape(-1, FEA_DIM), k, append=i > 0)
                f.write("%s %s\n" % (k, scp + ".ark"))
    os.makedirs(base + ".ali", exist_ok=True)
    cd, mono = unpack(g, tag + "_cd"), unpack(g, tag + "_mono")
    for i, k in enumerate(cd):
        D.write_vec_int_path(os.path.join(base + ".ali", "ali_pdf.ark"), cd[k], k, append=i > 0)
        D.write_vec_int_path(os.path.join(base + ".ali", "ali_phones.ark"), mono[k], k, append=i > 0)
    return base


def parse_ref_se_ark(buf):
    """(key, (T, 13) matrix) records of the reference's enhanced-feature ark: its header says
    T x 1 (see the module docstring), T * 13 floats follow."""
    out, pos = [], 0
    while pos < len(buf):
        sp = buf.index(b" ", pos)
        key = buf[pos:sp].decode()
        hdr = buf[sp + 1:sp + 1 + 15]
        assert hdr[:5] == b"\0BFM " and hdr[5:6] == b"\x04" and hdr[10:11] == b"\x04", hdr
        rows, cols = struct.unpack("<i", hdr[6:10])[0], struct.unpack("<i", hdr[11:15])[0]
        assert cols == 1, "the reference's header slip is gone: regenerate and compare headers"
        beg = sp + 1 + 15
        n = 4 * rows * FEA_DIM
        out.append((key, np.frombuffer(buf[beg:beg + n], dtype=np.float32).reshape(rows, FEA_DIM)))
        pos = beg + n
    return out


def test_run_nn_joint_lifecycle_vs_reference(tmp_path):
    from pkc.core import run_nn
    g = np.load(os.path.join(SRC, "expected.npz"), allow_pickle=False)
    d = str(tmp_path)
    b0, b1 = write_chunk(d, "ck0", g), write_chunk(d, "ck1", g)
    counts = os.path.join(d, "counts")
    with open(counts, "w") as f:
        f.write("[ " + " ".join(str(int(c)) for c in g["counts"]) + " ]\n")
    ref_ck0 = {s: os.path.join(SRC, "train_ck0_%s.pkl" % s) for s in SECS}
    ref_ck1 = {s: os.path.join(d, "ref_ck1_%s.pkl" % s) for s in SECS}
    c_tr0 = joint_cfg(d, "train_ck0", "train", b0)
    c_tr1 = joint_cfg(d, "train_ck1", "train", b1, pretrain=ref_ck0)
    c_va = joint_cfg(d, "valid", "valid", b0, pretrain=ref_ck1)
    c_fw = joint_cfg(d, "forward", "forward", b0, pretrain=ref_ck1, counts=counts,
                     forward_out="out_dnn3,out_dnn_SE", normalize="True,False")
    nxt, pats, pms = run_nn(None, None, None, None, None, None, c_tr0, True, c_tr1)
    nxt, pats, pms = run_nn(*nxt, c_tr1, False, c_va, patterns=pats, pattern_masks=pms)
    for s in SECS:          # the reference's ck1 model in the reference's checkpoint layout
        like = torch.load(ref_ck0[s], weights_only=True)
        sd = {k: torch.from_numpy(g["ck1/%s/model/%s" % (s, k)].copy()) for k in like["model_par"]}
        torch.save({"model_par": sd, "optimizer_par": like["optimizer_par"]}, ref_ck1[s])
    nxt, pats, pms = run_nn(*nxt, c_va, False, c_fw, patterns=pats, pattern_masks=pms)
    run_nn(*nxt, c_fw, False, c_fw, patterns=pats, pattern_masks=pms)

    l0, e0 = read_info(os.path.join(d, "train_ck0.info"))
    print("train_ck0 (from the cfg seed) loss %r err %r, reference %r" % (l0, e0, g["info_train_ck0"]))
    for tag in ("train_ck1", "valid"):
        loss, err = read_info(os.path.join(d, tag + ".info"))
        rl, re_ = g["info_" + tag]
        print("%s loss %r (reference %r) err %r (%r)" % (tag, loss, rl, err, re_))
        assert abs(loss - rl) <= 1e-5 * abs(rl), "%s loss %r vs reference %r" % (tag, loss, rl)
        assert abs(err - re_) <= 1e-6, "%s err %r vs reference %r" % (tag, err, re_)

    errs = {}

    def check(tag, got, ref):
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        dist = np.linalg.norm(got - ref)
        errs[tag] = (dist / max(np.linalg.norm(ref), 1e-30),
                     dist <= 1e-4 * np.linalg.norm(ref) + 1e-6 * np.sqrt(ref.size))

    for s in SECS:
        ref0 = torch.load(ref_ck0[s], weights_only=True, map_location="cpu")
        got1 = torch.load(os.path.join(d, "train_ck1_%s.pkl" % s), weights_only=True,
                          map_location="cpu")
        assert set(got1["model_par"]) == set(ref0["model_par"])
        assert got1["optimizer_par"]["param_groups"][0].keys() == \
            ref0["optimizer_par"]["param_groups"][0].keys()
        for k, v in got1["model_par"].items():
            ref = g["ck1/%s/model/%s" % (s, k)]
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(ref), (s, k)
                continue
            check("ck1 %s %s" % (s, k), v.numpy(), ref)
        st = got1["optimizer_par"]["state"]
        ref_keys = [k for k in g.files if k.startswith("ck1/%s/opt/" % s)]
        assert ref_keys
        for key in ref_keys:
            _, _, _, pi, name = key.split("/")
            assert int(pi) in st, (s, key)
            if name == "step":
                assert float(st[int(pi)][name]) == float(g[key]), key
                continue
            check(key, st[int(pi)][name].numpy(), g[key])
    bad = {k: "%.3g" % v[0] for k, v in errs.items() if not v[1]}
    print("worst ck1 checkpoint rel err %.3g" % max(v[0] for v in errs.values()))
    assert not bad, "checkpoint tensors off the reference: %s" % bad

    # forward mode: the posteriors to decode (log-softmax - log prior) ...
    with open(os.path.join(d, "forward_out_dnn3_to_decode.ark"), "rb") as f:
        got = parse_ark(f.read())
    with open(os.path.join(SRC, "forward_out_dnn3_to_decode.ark"), "rb") as f:
        ref = parse_ark(f.read())
    assert [k for k, _, _ in got] == [k for k, _, _ in ref] and len(ref) == 10
    c = g["counts"].astype(np.float32)
    lp = np.log(c / np.sum(c)).astype(np.float64)
    worst = 0.0
    for (k, h, m), (_, rh, rm) in zip(got, ref):
        assert h == rh, k
        a, b = m.astype(np.float64) + lp, rm.astype(np.float64) + lp
        worst = max(worst, float((np.abs(a - b) / np.maximum(np.abs(b), 1e-3)).max()))
    print("forward log-posterior max rel err %.3g" % worst)
    assert worst <= 1e-4, "forward log-posterior max rel err %.3g" % worst
    # ... and the enhanced features, not normalised, in a plain .ark
    with open(os.path.join(d, "forward_out_dnn_SE.ark"), "rb") as f:
        got = parse_ark(f.read())
    with open(os.path.join(SRC, "forward_out_dnn_SE.ark"), "rb") as f:
        ref = parse_ref_se_ark(f.read())
    assert [k for k, _, _ in got] == [k for k, _ in ref] and len(ref) == 10
    worst = 0.0
    for (k, h, m), (_, rm) in zip(got, ref):
        assert m.shape == rm.shape, k
        worst = max(worst, float(np.abs(m.astype(np.float64) - rm).max() / np.abs(rm).max()))
    print("forward enhanced features max diff / utterance scale %.3g" % worst)
    assert worst <= 1e-4, "enhanced features off by %.3g of the utterance's scale" % worst

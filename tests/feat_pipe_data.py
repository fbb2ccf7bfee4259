"""Synthetic inputs of the splice-feats / transform-feats tests: 9 utterances of 1 to 60 frames
(about 300 in all, D = 13) of 3 speakers — one of a single frame, several shorter than the splice
context, two longer than a max_seq_length of 40 — with per-speaker cmvn statistics, and the Kaldi
byte forms of transform matrices and tables."""
import os
import struct

import numpy as np

import frontend_data as FD

LENS = [1, 2, 4, 7, 41, 52, 58, 60, 60, 30]      # 285 frames of 9 utterances, and spkX's 30


def make(seed=0, D=13):
    """fea {utt: (T, D) f32}, utt2spk, cmvn stats per speaker, labels.  The tenth utterance's
    speaker spkX has neither statistics nor a transform."""
    rs = np.random.RandomState(seed)
    fea, u2s, lab = {}, {}, {}
    for i, T in enumerate(LENS):
        spk = "spk%d" % (i % 3) if i < 9 else "spkX"
        k = "%s_u%02d" % (spk, i)
        fea[k] = (rs.randn(T, D) * rs.uniform(0.5, 4) + rs.randn(1, D) * 3).astype(np.float32)
        u2s[k] = spk
        lab[k] = rs.randint(0, 40, T).astype(np.int32)
    return fea, u2s, stats_of(fea, u2s, ("spk0", "spk1", "spk2")), lab


def stats_of(fea, u2s, speakers):
    """compute-cmvn-stats per speaker: (2, D+1) float64 [sum x, count; sum x^2, 0]."""
    stats = {}
    for spk in speakers:
        x = np.concatenate([m for k, m in fea.items() if u2s[k] == spk]).astype(np.float64)
        s = np.zeros((2, x.shape[1] + 1))
        s[0, :-1], s[1, :-1], s[0, -1] = x.sum(0), (x * x).sum(0), len(x)
        stats[spk] = s
    return stats


def matrices(seed, rows, cols, keys=("spk0", "spk1", "spk2")):
    """{key: (rows, cols) float32} random transforms of the size an LDA / fMLLR has (O(1) rows)."""
    rs = np.random.RandomState(seed)
    return {k: (rs.randn(rows, cols) / np.sqrt(cols)).astype(np.float32) for k in keys}


def mat_bytes(m, form):
    """One Kaldi matrix: form 'FM' / 'DM' (binary) or 'text'."""
    m = np.asarray(m)
    if form == "text":
        rows = ["  " + " ".join(repr(float(v)) for v in r) for r in m]
        return (" [\n" + "\n".join(rows) + " ]\n").encode()
    dt = {"FM": "<f4", "DM": "<f8"}[form]
    return (b"\0B" + form.encode() + b" \x04" + struct.pack("<i", m.shape[0]) + b"\x04"
            + struct.pack("<i", m.shape[1]) + np.ascontiguousarray(m, dtype=dt).tobytes())


def write_matrix(path, m, form="FM"):
    with open(path, "wb") as f:
        f.write(mat_bytes(m, form))
    return path


def write_table(path, mats, form="FM"):
    with open(path, "wb") as f:
        for k, m in mats.items():
            f.write((k + " ").encode() + mat_bytes(m, form))
    return path


def write_cmvn(d, stats, u2s, name="cmvn.ark"):
    """The stats archive and the utt2spk table -> (cmvn path, utt2spk path)."""
    cm, us = os.path.join(d, name), os.path.join(d, "utt2spk")
    with open(cm, "wb") as f:
        for k, m in stats.items():
            f.write(FD.dm_bytes(k, m))
    with open(us, "w") as f:
        for k, s in u2s.items():
            f.write("%s %s\n" % (k, s))
    return cm, us


def fmllr_pipe(cm, us, final_mat, trans, cm2):
    """make_fmllr_feats.sh's pipe, then the cfg's own apply-cmvn | add-deltas --delta-order=0."""
    return ("apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | "
            "splice-feats --left-context=3 --right-context=3 ark:- ark:- | "
            "transform-feats %s ark:- ark:- | "
            "transform-feats --utt2spk=ark:%s ark:%s ark:- ark:- | "
            "apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | "
            "add-deltas --delta-order=0 ark:- ark:- |" % (us, cm, final_mat, us, trans, us, cm2))


def delta_pipe(cm, us, trans, cm2):
    """The delta recipe: add-deltas in place of the splice and LDA stages."""
    return ("apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | add-deltas ark:- ark:- | "
            "transform-feats --utt2spk=ark:%s ark:%s ark:- ark:- | "
            "apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | "
            "add-deltas --delta-order=0 ark:- ark:- |" % (us, cm, us, trans, us, cm2))

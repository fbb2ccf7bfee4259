"""numpy restatement of Kaldi's splice-feats (feat/feature-functions.cc SpliceFrames) and
transform-feats (featbin/transform-feats.cc: AddMatMat, then AddVecToRows), and of a whole stage
list of the feature pipe, for the tests of pkc_feat_transform.  Parity unpinned against Kaldi
itself (third-party, absent), as oracle/kaldi_feat.c is; the apply-cmvn / add-deltas groups are
that oracle's.

Two forms: float64 (the reference value) and float32 sequential (one multiplication and one
addition, each rounded, per term in ascending k: what the plainest float32 code loses).

The bound every kernel output is held to is the standard one for a K-term float32 sum in any order
plus one addition (Higham, Accuracy and Stability of Numerical Algorithms, §3.1, with
gamma_n ~ n u, u = 2^-24):

    |got - ref64| <= (K + 2) * 2^-24 * (sum_k |A[o][k]| |x[k]| + |b[o]|)
"""
import numpy as np

from oracle import kaldi_feat as OK

U = 2.0 ** -24


def splice(x, left, right):
    """SpliceFrames: row t = frames t-left .. t+right (clamped to the utterance), past first."""
    x = np.asarray(x)
    T = len(x)
    idx = np.clip(np.arange(T)[:, None] + np.arange(-left, right + 1)[None, :], 0, T - 1)
    return x[idx].reshape(T, -1)


def _split(A, K):
    A = np.asarray(A)
    if A.shape[1] not in (K, K + 1):
        raise ValueError("transform of %d x %d over features of dimension %d" % (A.shape + (K,)))
    return A[:, :K], (A[:, K] if A.shape[1] == K + 1 else None)


def transform64(x, A):
    """x (T, K) @ A[:, :K].T + A[:, K] in float64."""
    x = np.asarray(x, np.float64)
    W, b = _split(A, x.shape[1])
    y = x @ W.astype(np.float64).T
    return y if b is None else y + b.astype(np.float64)[None, :]


def transform32(x, A):
    """The same in float32, term after term in ascending k, every product and sum rounded."""
    x = np.asarray(x, np.float32)
    W, b = _split(np.asarray(A, np.float32), x.shape[1])
    acc = np.zeros((len(x), len(W)), np.float32)
    for k in range(x.shape[1]):
        acc = (acc + (x[:, k][:, None] * W[:, k][None, :]).astype(np.float32)).astype(np.float32)
    return acc if b is None else (acc + b[None, :]).astype(np.float32)


def magnitude(x, A):
    """sum_k |A[o][k]| |x[k]| + |b[o]| in float64."""
    x = np.abs(np.asarray(x, np.float64))
    W, b = _split(A, x.shape[1])
    m = x @ np.abs(W.astype(np.float64)).T
    return m if b is None else m + np.abs(b.astype(np.float64))[None, :]


def bound(x, A):
    """The bound of the module docstring for exact float32 inputs x."""
    return (np.asarray(x).shape[1] + 2) * U * magnitude(x, A)


def _key(utt, u2s):
    return utt if u2s is None else u2s.get(utt)


def run_stages(fea, stages):
    """fea {utt: (T, D) float32} through stages, a list of
        ("cmvn", stats {key: (2, D+1) f64}, utt2spk or None, norm_vars)
        ("deltas", order, window)
        ("splice", left, right)
        ("transform", matrix or {key: matrix}, utt2spk or None)
    -> {utt: (ref64, ref32, bound)}: the float64 value, the float32 sequential value and the bound
    on |float32 result - ref64| of a kernel that keeps the module's bound in each transform.
    Utterances without statistics / without a transform are dropped.

    cmvn and deltas in front of the first transform are exact float32 operations of the oracle
    (ref64 = ref32, bound 0).  Behind a transform the bound is carried on: through a transform as
    |A| bound_in plus the transform's own (K + 2) u (|A| (|x| + bound_in) + |b|); through
    apply-cmvn (got = fl(fl(x s) + o), s the oracle's float32 scale, 1 without --norm-vars) as
    bound_in |s| (1 + 2^-22) + 2^-23 (|x s| + |o|); through add-deltas of order 0, a copy."""
    out = {}
    for utt, x in fea.items():
        r32 = np.asarray(x, np.float32)
        r64, bnd = r32.astype(np.float64), np.zeros(r32.shape)
        for st in stages:
            if st[0] == "cmvn":
                _, stats, u2s, norm_vars = st
                sk = _key(utt, u2s)
                if sk is None or sk not in stats:
                    break
                off, sc = OK.cmvn_norm(stats[sk], norm_vars)
                r32 = OK.apply_cmvn(r32, stats[sk], norm_vars)
                if bnd.any():
                    s, o = sc.astype(np.float64)[None, :], off.astype(np.float64)[None, :]
                    bnd = bnd * np.abs(s) * (1 + 4 * U) + 2 * U * (np.abs(r64 * s) + np.abs(o))
                    r64 = r64 * s + o
                else:
                    r64 = r32.astype(np.float64)
            elif st[0] == "deltas":
                if bnd.any() and st[1] != 0:
                    raise NotImplementedError("add-deltas of order > 0 behind a transform")
                r32 = OK.add_deltas(r32, st[1], st[2])
                if not bnd.any():
                    r64, bnd = r32.astype(np.float64), np.zeros(r32.shape)
            elif st[0] == "splice":
                r32, r64, bnd = (splice(a, st[1], st[2]) for a in (r32, r64, bnd))
            else:
                _, mats, u2s = st
                A = mats if not isinstance(mats, dict) else mats.get(_key(utt, u2s))
                if A is None:
                    break
                K = r64.shape[1]
                W, _ = _split(A, K)
                absW = np.abs(W.astype(np.float64)).T
                own = (K + 2) * U * (magnitude(r64, A) + bnd @ absW)
                bnd = bnd @ absW + own
                r64, r32 = transform64(r64, A), transform32(r32, A)
        else:
            out[utt] = (r64, r32, bnd)
    return out

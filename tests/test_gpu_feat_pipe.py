"""splice-feats / transform-feats on the GPU (pkc_feat_transform) against the numpy restatement
(tests/feat_pipe_ref.py): splice alone and selection matrices bit for bit, random transforms
within the derived bound of a K-term float32 sum, determinism, the supported range, the fMLLR and
delta-recipe pipes through the chunk staging, and end to end through the writer, read_lab_fea and
run_nn.

The bound (feat_pipe_ref): |got - ref64| <= (K + 2) * 2^-24 * (sum_k |A||x| + |b|), the standard
bound of a K-term float32 sum in any order plus one addition; derived, not measured.  For the
record, on these inputs the float32 sequential restatement reaches 0.21 of it at K = 13 and 0.06
or less at K >= 91, and the kernel (one fused multiply-add per term) 0.21 and 0.05; each test
prints its own figures."""
import configparser
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feat_pipe_data as PD
import feat_pipe_ref as R
from oracle import loader as OL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "pytorch-kaldi-cgs_amd")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def data():
    """The shared inputs (never modified): 9 utterances of 3 speakers, 285 frames, D = 13."""
    fea, u2s, stats, lab = PD.make()
    fea = {k: v for k, v in fea.items() if not k.startswith("spkX")}
    for v in fea.values():
        v.setflags(write=False)
    return fea, u2s, stats, lab


def _frontend(stages):
    from pkc import frontend as F
    fe = F.FeaFrontend()
    fe.stages = stages
    return fe


def _transform(mats, u2s=None):
    """F.Transform of one matrix (global) or of a {speaker: matrix} table."""
    from pkc import frontend as F
    return F.Transform(mats if isinstance(mats, dict) else {None: mats}, u2s)


def _stage(fea, lab, stages, max_seq):
    """stage_chunk through the given stage list -> (StagedChunk, (rows, Dout) float32)."""
    from pkc import data_io as D
    st = D.stage_chunk(fea, [lab], max_seq, frontend=_frontend(stages))
    torch.cuda.current_stream().wait_event(st.done)
    return st, st.raw_d.cpu().numpy()


def _ordered(per_utt, fea, lab, max_seq):
    """Per-utterance matrices laid out in the sorted / split order of the chunk."""
    from pkc import data_io as D
    _, pieces, _, _ = D.dataset_pieces({k: len(v) for k, v in fea.items()}, [lab], max_seq)
    return np.concatenate([per_utt[k][a:b] for k, a, b in pieces])


def _by_utt(rows, fea, lab, max_seq):
    """The inverse of _ordered: {utt: (T, C)} from the rows of a chunk."""
    from pkc import data_io as D
    _, pieces, _, _ = D.dataset_pieces({k: len(v) for k, v in fea.items()}, [lab], max_seq)
    out = {k: np.empty((len(v), rows.shape[1]), rows.dtype) for k, v in fea.items()}
    r = 0
    for k, a, b in pieces:
        out[k][a:b] = rows[r:r + b - a]
        r += b - a
    assert r == len(rows)
    return out


@pytest.mark.parametrize("left, right", [(3, 3), (4, 2), (0, 5)])
def test_splice_alone_is_numpy_indexing_bit_for_bit(data, left, right):
    fea, _, _, lab = data
    proc = {k: R.splice(v, left, right) for k, v in fea.items()}
    got = {}
    for max_seq in (-1, 40):
        st, got[max_seq] = _stage(fea, lab, [("splice-feats", left, right)], max_seq)
        names, ref, _, end = OL.load_dataset(proc, lab, max_seq)
        assert st.names == names and np.array_equal(st.end_index, end)
        assert got[max_seq].shape == ref.shape == (285, 13 * (left + right + 1))
        assert np.array_equal(_bits(got[max_seq]), _bits(ref))
    assert any("_split" in n for n in names)
    # a split piece splices across its cut: its rows are the rows of the unsplit run
    whole, cut = _by_utt(got[-1], fea, lab, -1), _by_utt(got[40], fea, lab, 40)
    for k in fea:
        assert np.array_equal(_bits(whole[k]), _bits(cut[k])), k


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("per_speaker", [False, True])
def test_selection_matrices_select_bit_for_bit(data, affine, per_speaker):
    """0 / 1 matrices with one 1 per row, small integer offsets: the output is the selected spliced
    column, plus the offset in one float32 addition."""
    fea, u2s, _, lab = data
    rs = np.random.RandomState(11)
    K, Dout = 91, 40
    mats, sel, off = {}, {}, {}
    for spk in ("spk0", "spk1", "spk2") if per_speaker else (None,):
        sel[spk] = rs.randint(0, K, Dout)
        off[spk] = rs.randint(-8, 9, Dout).astype(np.float32)
        A = np.zeros((Dout, K + int(affine)), np.float32)
        A[np.arange(Dout), sel[spk]] = 1.0
        if affine:
            A[:, K] = off[spk]
        mats[spk] = A
    tr = _transform(mats, u2s if per_speaker else None)
    st, got = _stage(fea, lab, [("splice-feats", 3, 3), ("transform-feats", tr)], 40)
    want = {}
    for k, v in fea.items():
        spk = u2s[k] if per_speaker else None
        want[k] = R.splice(v, 3, 3)[:, sel[spk]]
        if affine:
            want[k] = (want[k] + off[spk][None, :]).astype(np.float32)
    assert got.shape == (285, 40)
    assert np.array_equal(_bits(got), _bits(_ordered(want, fea, lab, 40)))


def _check_bound(got, ref64, ref32, bnd, what):
    """Every element within the bound; the message carries the largest ratio and the kernel's
    maximum error over the float32 restatement's."""
    err = np.abs(got.astype(np.float64) - ref64)
    e32 = np.abs(ref32.astype(np.float64) - ref64)
    ratio = float((err / np.maximum(bnd, 1e-300)).max())
    vs32 = float(err.max() / e32.max()) if e32.max() > 0 else float("inf")
    print("%s: max |got - ref64| / bound = %.4f, float32 restatement / bound = %.4f, "
          "kernel max error / restatement max error = %.3f"
          % (what, ratio, float((e32 / np.maximum(bnd, 1e-300)).max()), vs32))
    assert np.isfinite(got).all() and (err <= bnd).all(), (
        "%s: largest |got - ref64| / bound = %.4f (must be <= 1); kernel max error / float32 "
        "restatement max error = %.3f" % (what, ratio, vs32))


# (D, left, right, Dout): K = 91, 143, 13 of the issue, and K = 200 -> 70 outputs, which takes
# three k-chunks and two output chunks of the matrix in LDS (the others take one of each)
SHAPES = {"91x40": (13, 3, 3, 40), "143x7": (13, 5, 5, 7), "13x40": (13, 0, 0, 40),
          "200x70": (40, 2, 2, 70)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("per_speaker", [False, True])
def test_random_transforms_within_the_float32_sum_bound(data, shape, affine, per_speaker):
    fea, u2s, _, lab = data
    Din, left, right, Dout = SHAPES[shape]
    if Din != 13:
        rs = np.random.RandomState(2)
        fea = {k: (rs.randn(len(v), Din) * 3 + 1).astype(np.float32) for k, v in fea.items()}
    K = Din * (left + right + 1)
    mats = PD.matrices(K + Dout, Dout, K + int(affine))
    if affine:
        for m in mats.values():
            m[:, K] *= 10
    tr = _transform(mats if per_speaker else mats["spk1"], u2s if per_speaker else None)
    stages = ([("splice-feats", left, right)] if left or right else []) + [("transform-feats", tr)]
    st, got = _stage(fea, lab, stages, 40)
    ref64, ref32, bnd = {}, {}, {}
    for k, v in fea.items():
        A = mats[u2s[k]] if per_speaker else mats["spk1"]
        spl = R.splice(v, left, right)
        ref64[k], ref32[k], bnd[k] = R.transform64(spl, A), R.transform32(spl, A), R.bound(spl, A)
    assert got.shape == (285, Dout)
    _check_bound(got, *(_ordered(x, fea, lab, 40) for x in (ref64, ref32, bnd)),
                 what="%s affine=%d per_speaker=%d" % (shape, affine, per_speaker))


def test_edge_of_the_supported_range(data):
    """K = 4096 (D = 1024, 1 + 2 frames of context) to Dout = 512, affine: tiles of 5 rows, eight
    output chunks and 43 k-chunks of the matrix.  Three short utterances keep it quick."""
    _, _, _, lab = data
    rs = np.random.RandomState(4)
    fea = {k: rs.randn(T, 1024).astype(np.float32) for k, T in (("a", 1), ("b", 7), ("c", 23))}
    lab = {k: np.zeros(len(v), np.int32) for k, v in fea.items()}
    A = PD.matrices(5, 512, 4097, keys=("m",))["m"]
    st, got = _stage(fea, lab, [("splice-feats", 1, 2), ("transform-feats", _transform(A))], -1)
    spl = {k: R.splice(v, 1, 2) for k, v in fea.items()}
    ref64 = _ordered({k: R.transform64(s, A) for k, s in spl.items()}, fea, lab, -1)
    bnd = _ordered({k: R.bound(s, A) for k, s in spl.items()}, fea, lab, -1)
    err = np.abs(got.astype(np.float64) - ref64)
    assert got.shape == (31, 512) and (err <= bnd).all(), float((err / bnd).max())


def _launch(fea, pieces, groups):
    """One pipe_maps plan over `pieces` run on the current stream -> (rows, Dout) float32."""
    from pkc import data_io as D
    fa = D.pipe_maps({k: len(v) for k, v in fea.items()}, 13, pieces, groups)
    raw = np.ascontiguousarray(np.concatenate([fea[k] for k in fa["keys"]]), dtype=np.float32)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in [raw] + fa["arrays"]]
    out, keep = D.feat_pipe_device(dev[0], dev[1:], fa, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_reruns_and_row_orders_give_equal_bits(data):
    """Two runs are bit-equal, and a row computed in identity order (whole utterances, as an
    intermediate launch writes them) equals the same row in the sorted / split order."""
    from pkc import data_io as D
    from pkc import frontend as F
    fea, u2s, _, lab = data
    mats = PD.matrices(21, 40, 92)
    groups = [F.SpliceTransform(3, 3, _transform(mats, u2s))]
    ident = [(k, 0, len(v)) for k, v in fea.items()]
    _, split, _, _ = D.dataset_pieces({k: len(v) for k, v in fea.items()}, [lab], 40)
    a, a2, b = _launch(fea, ident, groups), _launch(fea, ident, groups), _launch(fea, split, groups)
    assert a.shape == b.shape == (285, 40) and np.array_equal(_bits(a), _bits(a2))
    by_utt, r = {}, 0
    for k, _, T in ident:
        by_utt[k] = a[r:r + T]
        r += T
    assert np.array_equal(_bits(b), _bits(np.concatenate([by_utt[k][s:e] for k, s, e in split])))
    assert not np.array_equal(_bits(a), _bits(b))             # the two orders do differ


def test_shapes_outside_the_range_are_reported_and_launch_nothing():
    from pkc import _lib as L
    lib = L.lib()
    for args in ((31, 64, 64, 512, 1), (4096, 0, 0, 512, 1), (13, 3, 3, 91, 0), (1, 0, 0, 1, 1)):
        assert lib.pkc_feat_transform_ok(*args) == 1, args
        assert lib.pkc_feat_transform_tile(*args) >= 1
    for args, text in (((13, 65, 0, 40, 1), "context"), ((13, 0, 65, 40, 1), "context"),
                       ((64, 32, 32, 40, 1), "4096"), ((13, 3, 3, 513, 1), "Dout"),
                       ((13, 3, 3, 0, 1), "Dout"), ((13, 3, 3, 40, 0), "Dout = K"),
                       ((0, 0, 0, 1, 1), "D >= 1")):
        assert lib.pkc_feat_transform_ok(*args) == 0, args
        assert text in lib.pkc_last_error().decode(), (args, lib.pkc_last_error())
        assert lib.pkc_feat_transform_tile(*args) == 0
    x = torch.ones(8, 13, device="cuda")
    maps = [torch.arange(8, dtype=torch.int32, device="cuda"),
            torch.zeros(8, dtype=torch.int32, device="cuda"),
            torch.tensor([0], dtype=torch.int32, device="cuda"),
            torch.tensor([8], dtype=torch.int32, device="cuda")]
    tiles = torch.tensor([[0, 8]], dtype=torch.int32, device="cuda")
    A = torch.ones(1, 40, 13 * 66, device="cuda")
    out = torch.full((8, 40), float("nan"), device="cuda")
    rc = lib.pkc_feat_transform(L.ptr(x), 13, 65, 0, 8, *[L.ptr(m) for m in maps], 1, None, L.ptr(A),
                                1, 40, 0, L.ptr(tiles), 1, L.ptr(out),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == L.PKC_ERR_UNSUPPORTED and "context" in lib.pkc_last_error().decode()
    assert torch.isnan(out).all()


def _pipe_files(d, fea, u2s, stats, kind):
    """The files of the fMLLR pipe (kind 'fmllr') or the delta-recipe pipe ('delta'), the second
    cmvn's statistics taken over the float32 restatement of the transformed features.
    Returns (fea_opts, restatement stage list)."""
    cm, us = PD.write_cmvn(d, stats, u2s)
    lda = PD.matrices(31, 40, 91)["spk0"]
    fm = PD.matrices(32, 40, 41) if kind == "fmllr" else PD.matrices(33, 39, 40)
    for m in fm.values():
        m[:, -1] *= 5
    head = [("cmvn", stats, u2s, False)]
    head += [("splice", 3, 3), ("transform", lda, None)] if kind == "fmllr" else [("deltas", 2, 2)]
    head += [("transform", fm, u2s)]
    mid = {k: v[1] for k, v in R.run_stages(fea, head).items()}
    stats2 = PD.stats_of(mid, u2s, ("spk0", "spk1", "spk2"))
    cm2, _ = PD.write_cmvn(d, stats2, u2s, "cmvn2.ark")
    trans = PD.write_table(os.path.join(d, "trans.ark"), fm, "FM")
    if kind == "fmllr":
        final = PD.write_matrix(os.path.join(d, "final.mat"), lda, "FM")
        opts = PD.fmllr_pipe(cm, us, final, trans, cm2)
    else:
        opts = PD.delta_pipe(cm, us, trans, cm2)
    return opts, head + [("cmvn", stats2, u2s, False), ("deltas", 0, 2)]


@pytest.mark.parametrize("kind, Dout", [("fmllr", 40), ("delta", 39)])
def test_whole_pipe_through_stage_chunk(tmp_path, kind, Dout):
    """names, end_index and values of the staged chunk against the restatement's stage list; the
    utterance of the speaker without statistics or transform is dropped."""
    from pkc import data_io as D
    from pkc import frontend as F
    fea, u2s, stats, lab = PD.make()
    opts, stages = _pipe_files(str(tmp_path), {k: v for k, v in fea.items() if u2s[k] != "spkX"},
                               u2s, stats, kind)
    fe = F.FeaFrontend.parse(opts)
    st = D.stage_chunk(fea, [lab], 40, frontend=fe)
    torch.cuda.current_stream().wait_event(st.done)
    got = st.raw_d.cpu().numpy()
    ref = R.run_stages(fea, stages)
    assert sorted(ref) == sorted(k for k in fea if u2s[k] != "spkX")
    kept = {k: fea[k] for k in ref}
    names, _, _, end = OL.load_dataset({k: v[1] for k, v in ref.items()}, lab, 40)
    assert st.names == names and np.array_equal(st.end_index, end)
    assert got.shape == (285, Dout) and st.shape == (285, Dout)
    r64, r32, bnd = ({k: v[i] for k, v in ref.items()} for i in range(3))
    _check_bound(got, *(_ordered(x, kept, lab, 40) for x in (r64, r32, bnd)), what=kind + " pipe")


def _wav_set(d):
    """Nine utterances of three speakers as wavs (1 to 97 MFCC frames), their wav list, utt2spk."""
    import wave
    rs = np.random.RandomState(17)
    lst, us = os.path.join(d, "wav.lst"), os.path.join(d, "utt2spk")
    with open(lst, "w") as fl, open(us, "w") as fu:
        for i, nf in enumerate([55, 31, 97, 12, 40, 23, 1, 3, 64]):
            n = 400 + (nf - 1) * 160 + rs.randint(0, 160)
            t = np.arange(n)
            s = rs.normal(0, 400 + 100 * i, n) + 3000 * np.sin(2 * np.pi * (200.0 + 90 * i) * t / 16000)
            k, path = "spk%d_u%02d" % (i % 3, i), os.path.join(d, "u%02d.wav" % i)
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes(np.round(s).astype("<i2").tobytes())
            fl.write("%s %s\n" % (k, path))
            fu.write("%s spk%d\n" % (k, i % 3))
    return lst, us


def test_end_to_end_writer_read_lab_fea_and_run_nn(tmp_path):
    """MFCC scp -> python -m pkc.feat_pipe writes the fMLLR features and their cmvn statistics;
    a cfg whose fea_opts is the full pipe and a cfg that reads the written ark through
    apply-cmvn | add-deltas --delta-order=0 then load bit-equal chunks and train to the same loss;
    pkc-mfcc over the wav list in front of the same pipe stages the MFCC-scp path's chunk."""
    from pkc import core
    from pkc import data_io as D
    from pkc import frontend as F
    from pkc.kaldi_feats import write_feats
    from test_gpu_run_nn import chunk_cfg
    d = str(tmp_path)
    lst, us = _wav_set(d)
    mfcc_ark, mfcc_scp, cm = (os.path.join(d, n) for n in ("mfcc.ark", "mfcc.scp", "cmvn.ark"))
    mfcc = write_feats(lst, F.KaldiFeats("mfcc"), mfcc_ark, mfcc_scp, us, cm)
    assert len(mfcc) == 9 and sum(len(m) for m in mfcc.values()) == 326
    final = PD.write_matrix(os.path.join(d, "final.mat"), PD.matrices(41, 40, 91)["spk0"], "DM")
    trans = PD.write_table(os.path.join(d, "trans.ark"), PD.matrices(42, 40, 41), "text")
    head = ("apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | "
            "splice-feats --left-context=3 --right-context=3 ark:- ark:- | "
            "transform-feats %s ark:- ark:- | transform-feats --utt2spk=ark:%s ark:%s ark:- ark:- |"
            % (us, cm, final, us, trans))
    ark, scp, cm2 = (os.path.join(d, n) for n in ("fmllr.ark", "fmllr.scp", "cmvn_fmllr.ark"))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [PKG] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    subprocess.run([sys.executable, "-m", "pkc.feat_pipe", "--fea-lst", mfcc_scp, "--fea-opts", head,
                    "--ark-out", ark, "--scp-out", scp, "--utt2spk", us, "--cmvn-out", cm2],
                   check=True, env=env, timeout=120)
    # what it wrote: the pipe's own rows, in the scp's order, and their statistics
    written = dict(D.read_mat_ark_path(ark))
    assert list(written) == list(mfcc) == [l.split()[0] for l in open(scp).read().splitlines()]
    fea, fe = core._read_features(mfcc_scp, head, d)
    st = D.stage_chunk(fea, [], -1, frontend=fe)
    torch.cuda.current_stream().wait_event(st.done)
    rows, beg = st.raw_d.cpu().numpy(), 0
    for k, e in zip(st.names, st.end_index):
        assert written[k].shape == (len(mfcc[k]), 40)
        assert np.array_equal(_bits(written[k]), _bits(rows[beg:e])), k
        beg = e
    with open(cm2, "rb") as f:
        stats2 = F.parse_stats_ark(f.read())
    u2s = F.read_utt2spk(us)
    assert sorted(stats2) == ["spk0", "spk1", "spk2"]
    for spk in stats2:
        assert np.array_equal(stats2[spk], F.cmvn_stats([written[k] for k in written if u2s[k] == spk]))
    # against the restatement, within the bound (the first transform's error carried through)
    with open(cm, "rb") as f:
        stats = F.parse_stats_ark(f.read())
    ref = R.run_stages(mfcc, [("cmvn", stats, u2s, False), ("splice", 3, 3),
                              ("transform", fe.stages[2][1].mats[None], None),
                              ("transform", fe.stages[3][1].mats, u2s)])
    for k in written:
        assert (np.abs(written[k].astype(np.float64) - ref[k][0]) <= ref[k][2]).all(), k

    tail = "apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | add-deltas --delta-order=0 ark:- ark:- |" \
        % (us, cm2)
    ali = os.path.join(d, "ali")
    os.makedirs(ali)
    rs = np.random.RandomState(0)
    for i, (k, m) in enumerate(mfcc.items()):
        D.write_vec_int_path(os.path.join(ali, "ali_pdf.ark"), rs.randint(0, 64, len(m)), k, append=i > 0)
        D.write_vec_int_path(os.path.join(ali, "ali_phones.ark"), rs.randint(1, 9, len(m)), k,
                             append=i > 0)
    block = "fea_name=fmllr\nfea_lst=%s\nfea_opts=%s\ncw_left=2\ncw_right=2\n"
    variants = {"pipe": block % (mfcc_scp, head + " " + tail), "ark": block % (scp, tail),
                "wav": block % (lst, "pkc-mfcc ark:- ark:- | " + head + " " + tail)}
    chunks, loss = {}, {}
    for tag, fea_block in variants.items():
        path = chunk_cfg(d, "train_" + tag, "train", "unused", ali)
        cfg = configparser.ConfigParser()
        cfg.read(path)
        cfg["data_chunk"]["fea"] = fea_block
        cfg["architecture1"]["dnn_drop"] = "0.0,0.0"
        cfg["batches"]["max_seq_length_train"] = "40"
        with open(path, "w") as f:
            cfg.write(f)
        shared = []
        np.random.seed(2234)
        core.read_lab_fea(path, False, shared, d)
        ch = core._finish_chunk(shared)[1]
        chunks[tag] = (ch.names, np.asarray(ch.end_index), ch.feats.clone(), ch.labels.clone())
        if tag != "wav":
            core.run_nn(None, None, None, None, None, None, path, True, path)
            info = configparser.ConfigParser()
            info.read(os.path.join(d, "train_%s.info" % tag))
            loss[tag] = info["results"]["loss"]
    names, end, feats, labels = chunks["pipe"]
    assert feats.shape == (326 - 4, 40 * 5) and torch.isfinite(feats).all()
    assert any("_split" in n for n in names)
    for tag in ("ark", "wav"):
        assert chunks[tag][0] == names and np.array_equal(chunks[tag][1], end), tag
        assert torch.equal(chunks[tag][2], feats) and torch.equal(chunks[tag][3], labels), tag
    assert np.isfinite(float(loss["pipe"])) and loss["pipe"] == loss["ark"]

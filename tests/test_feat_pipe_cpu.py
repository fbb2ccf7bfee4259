"""splice-feats / transform-feats in the fea_opts pipe, host side (no GPU): the grammar and the
stage list FeaFrontend.parse returns, the matrix and table readers, linear against affine, the
refusals, the dropped utterances, and the unchanged tables of the pipes accepted before."""
import os

import numpy as np
import pytest

from pkc import data_io as D
from pkc import frontend as F

import feat_pipe_data as PD
import frontend_data as FD


def _files(d, D_in=13, lda_rows=40, lda_cols=91, fmllr_cols=41):
    fea, u2s, stats, lab = PD.make()
    cm, us = PD.write_cmvn(d, stats, u2s)
    final = PD.write_matrix(os.path.join(d, "final.mat"), PD.matrices(1, lda_rows, lda_cols)["spk0"])
    trans = PD.write_table(os.path.join(d, "trans.ark"), PD.matrices(2, lda_rows, fmllr_cols))
    rs = np.random.RandomState(3)
    st2 = {}
    for spk in ("spk0", "spk1", "spk2"):
        s = np.zeros((2, lda_rows + 1))
        s[0, :-1], s[1, :-1], s[0, -1] = rs.randn(lda_rows) * 50, 400 + rs.rand(lda_rows), 100
        st2[spk] = s
    cm2, _ = PD.write_cmvn(d, st2, u2s, "cmvn_fmllr.ark")
    return dict(fea=fea, u2s=u2s, stats=stats, lab=lab, cm=cm, us=us, final=final, trans=trans,
                cm2=cm2)


def test_fmllr_pipe_parses_to_its_stage_list(tmp_path):
    f = _files(str(tmp_path))
    opts = PD.fmllr_pipe(f["cm"], f["us"], f["final"], f["trans"], f["cm2"])
    assert F.is_native_pipe(opts)
    fe = F.FeaFrontend.parse(opts)
    assert [s[0] for s in fe.stages] == ["apply-cmvn", "splice-feats", "transform-feats",
                                         "transform-feats", "apply-cmvn", "add-deltas"]
    assert fe.stages[1][1:] == (3, 3) and fe.stages[5][1:] == (0, 2)
    lda, fm = fe.stages[2][1], fe.stages[3][1]
    assert (lda.rows, lda.cols) == (40, 91) and list(lda.mats) == [None] and lda.utt2spk is None
    assert (fm.rows, fm.cols) == (40, 41) and sorted(fm.mats) == ["spk0", "spk1", "spk2"]
    assert fm.utt2spk == f["u2s"]
    groups = fe.groups()
    assert [type(g).__name__ for g in groups] == ["CmvnDeltas", "SpliceTransform", "SpliceTransform",
                                                  "CmvnDeltas"]
    assert (groups[1].left, groups[1].right, groups[1].transform) == (3, 3, lda)
    assert (groups[2].left, groups[2].right, groups[2].transform) == (0, 0, fm)
    assert groups[0].order == 0 and groups[3].order == 0 and groups[3].cmvn is fe.stages[4][1]
    assert fe.out_dim(13) == 40
    assert fe.feats is None and fe.wav is None
    front = F.FeaFrontend.parse("pkc-mfcc ark:- ark:- | " + opts)
    assert front.feats.D == 13 and len(front.stages) == 6 and front.out_dim(13) == 40


def test_delta_recipe_pipe_parses_to_its_stage_list(tmp_path):
    d = str(tmp_path)
    f = _files(d)
    trans = PD.write_table(os.path.join(d, "trans39.ark"), PD.matrices(4, 39, 40))
    rs = np.random.RandomState(5)
    st2 = {spk: np.concatenate([rs.randn(2, 39) + [[0], [300]], [[100], [0]]], 1)
           for spk in ("spk0", "spk1", "spk2")}
    cm2, _ = PD.write_cmvn(d, st2, f["u2s"], "cmvn39.ark")
    opts = PD.delta_pipe(f["cm"], f["us"], trans, cm2)
    assert F.is_native_pipe(opts)
    fe = F.FeaFrontend.parse(opts)
    assert [s[0] for s in fe.stages] == ["apply-cmvn", "add-deltas", "transform-feats", "apply-cmvn",
                                         "add-deltas"]
    assert fe.stages[1][1:] == (2, 2)
    groups = fe.groups()
    assert [type(g).__name__ for g in groups] == ["CmvnDeltas", "SpliceTransform", "CmvnDeltas"]
    assert groups[0].order == 2 and groups[1].transform.cols == 40 and groups[2].order == 0
    assert fe.out_dim(13) == 39


def test_splice_defaults_are_4_4_and_lone_stages_group():
    fe = F.FeaFrontend.parse("add-deltas --delta-order=0 ark:- ark:- | splice-feats ark:- ark:- |")
    assert fe.stages == [("add-deltas", 0, 2), ("splice-feats", 4, 4)] and fe.out_dim(13) == 117
    assert [type(x).__name__ for x in fe.groups()] == ["CmvnDeltas", "SpliceTransform"]
    # a pipe of splice-feats alone stays what it was: not native (Kaldi's), refused by parse
    for alone in ("splice-feats ark:- ark:- |", "splice-feats ark:- ark:- | splice-feats ark:- ark:-"):
        assert not F.is_native_pipe(alone)
        with pytest.raises(NotImplementedError, match="splice-feats alone"):
            F.FeaFrontend.parse(alone)
    assert F.is_native_pipe("add-deltas ark:- ark:- | splice-feats ark:- ark:- |")
    fe = F.FeaFrontend.parse("splice-feats --left_context=2 ark:- ark:- | add-deltas ark:- ark:- | "
                             "splice-feats --right-context=0 ark:- ark:- |")
    assert fe.stages == [("splice-feats", 2, 4), ("add-deltas", 2, 2), ("splice-feats", 4, 0)]
    g = fe.groups()
    assert [type(x).__name__ for x in g] == ["SpliceTransform", "CmvnDeltas", "SpliceTransform"]
    assert g[0].transform is None and g[1].cmvn is None and fe.out_dim(2) == 2 * 7 * 3 * 5


@pytest.mark.parametrize("form", ["FM", "DM", "text"])
def test_matrix_and_table_readers_decode_every_form(tmp_path, form):
    d = str(tmp_path)
    mats = PD.matrices(7, 5, 14)
    one = F.Transform.read(PD.write_matrix(os.path.join(d, "m"), mats["spk1"], form))
    assert list(one.mats) == [None] and one.mats[None].dtype == np.float32
    assert np.array_equal(one.mats[None], mats["spk1"])
    tab = F.Transform.read("ark:" + PD.write_table(os.path.join(d, "t.ark"), mats, form))
    assert sorted(tab.mats) == sorted(mats)
    for k in mats:
        assert np.array_equal(tab.mats[k], mats[k]), k
    assert (tab.rows, tab.cols) == (5, 14)


def test_linear_and_affine_are_told_apart_by_width(tmp_path):
    d = str(tmp_path)
    t = F.Transform.read(PD.write_matrix(os.path.join(d, "m"), PD.matrices(7, 5, 14)["spk0"]))
    assert t.shape(14) == (5, 0) and t.shape(13) == (5, 1)
    for K in (12, 15):
        with pytest.raises(ValueError, match=r"transform-feats .*5 x 14.* dimension %d\b" % K):
            t.shape(K)
    fe = F.FeaFrontend.parse("splice-feats --left-context=0 --right-context=1 ark:- ark:- | "
                             "transform-feats %s ark:- ark:- |" % os.path.join(d, "m"))
    assert fe.out_dim(7) == 5                             # K = 14: linear
    with pytest.raises(ValueError, match="5 x 14.* dimension 16"):
        fe.out_dim(8)
    with pytest.raises(ValueError, match="5 x 14.* dimension 26"):
        fe.kept_keys(["a"], 13)


def test_refusals_by_name(tmp_path):
    d = str(tmp_path)
    f = _files(d)
    m, t, us = f["final"], f["trans"], f["us"]
    nie = [
        ("add-deltas ark:- ark:- | splice-feats --bogus=1 ark:- ark:- |", "splice-feats options"),
        ("add-deltas ark:- ark:- | splice-feats ark:- ark:out.ark |", "expected ark:- ark:-"),
        ("transform-feats --utt2spk=ark:%s --verbose=2 ark:%s ark:- ark:- |" % (us, t),
         "transform-feats options"),
        ("transform-feats %s ark:- |" % m, "transform-feats"),
        ('transform-feats --utt2spk=ark:%s "ark:cat %s |" ark:- ark:- |' % (us, t), "piped"),
        ("transform-feats scp:%s ark:- ark:- |" % t, "scp:"),
        ("transform-feats --utt2spk=scp:%s ark:%s ark:- ark:- |" % (us, t), "ark:"),
        ("add-deltas ark:- ark:- | pkc-mfcc ark:- ark:- |", "first stage"),
        ("pkc-wav-frames ark:- ark:- | splice-feats ark:- ark:- |", "only stage"),
        ("compose-transforms a b c |", "no native pkc implementation"),
        (" | ".join(["add-deltas --delta-order=0 ark:- ark:-"] * 9) + " |", "9 stages"),
    ]
    for opts, what in nie:
        with pytest.raises(NotImplementedError, match=what):
            F.FeaFrontend.parse(opts)
    # a piped table is a native stage name: it is refused by name, never handed to a shell
    assert F.is_native_pipe('transform-feats "ark:cat %s |" ark:- ark:- |' % t)
    with pytest.raises(ValueError, match="utt2spk"):
        F.FeaFrontend.parse("transform-feats --utt2spk=ark:%s %s ark:- ark:- |" % (us, m))
    with pytest.raises(ValueError, match="left-context"):
        F.FeaFrontend.parse("add-deltas ark:- ark:- | splice-feats --left-context=-1 ark:- ark:- |")
    # eight stages, and the two groups more than once and in any position, are accepted
    fe = F.FeaFrontend.parse(" | ".join(
        ["add-deltas --delta-order=1 ark:- ark:-", "apply-cmvn ark:%s ark:- ark:-" % f["cm"]] * 4))
    assert len(fe.stages) == 8 and len(fe.groups()) == 5 and fe.out_dim(1) == 16


def test_utterances_without_a_transform_are_dropped(tmp_path):
    f = _files(str(tmp_path))
    fe = F.FeaFrontend.parse("transform-feats --utt2spk=ark:%s ark:%s ark:- ark:- |"
                             % (f["us"], f["trans"]))
    with pytest.raises(ValueError, match="40 x 41.* dimension 13"):
        fe.kept_keys(sorted(f["fea"]), 13)
    keys = sorted(f["fea"])
    assert fe.kept_keys(keys, 40) == [k for k in keys if not k.startswith("spkX")]
    assert len(fe.kept_keys(keys, 40)) == 9
    # keyed by utterance without --utt2spk
    d = str(tmp_path)
    per_utt = PD.write_table(os.path.join(d, "u.ark"), PD.matrices(9, 3, 13, keys=keys[2:5]))
    fe = F.FeaFrontend.parse("transform-feats ark:%s ark:- ark:- |" % per_utt)
    assert fe.kept_keys(keys, 13) == keys[2:5]
    # through the whole pipe: the cmvn filter and the transform filter are one filter
    fe = F.FeaFrontend.parse(PD.fmllr_pipe(f["cm"], f["us"], f["final"], f["trans"], f["cm2"]))
    assert fe.kept_keys(keys, 13) == [k for k in keys if not k.startswith("spkX")]


def test_pipe_maps_tables(tmp_path):
    """The launch plan of the fMLLR pipe: identity maps for every launch but the last, the
    sorted / split maps for the last, and tiles that stay inside one utterance."""
    f = _files(str(tmp_path))
    fe = F.FeaFrontend.parse(PD.fmllr_pipe(f["cm"], f["us"], f["final"], f["trans"], f["cm2"]))
    fea = {k: v for k, v in f["fea"].items() if not k.startswith("spkX")}
    names, pieces, _, end = D.dataset_pieces({k: len(v) for k, v in fea.items()}, [f["lab"]], 40)
    fa = D.frontend_args(fea, pieces, fe)
    assert fa["out_shape"] == (285, 40) and fa["D"] == 13 and fa["raw"].shape == (285, 13)
    kinds = [(ln["kind"], ln["D"], ln["Dout"], ln["rows"], ln["map"]) for ln in fa["launches"]]
    assert kinds == [("frontend", 13, 13, 285, 0), ("transform", 13, 40, 285, 0),
                     ("transform", 40, 40, 285, 0), ("frontend", 40, 40, 285, 2)]
    id_s, id_u, fin_s, fin_u, ubeg, uend = fa["arrays"][:6]
    assert np.array_equal(id_s, np.arange(285)) and np.all(np.diff(id_u) >= 0)
    assert np.array_equal(fa["raw"][fin_s], D.load_dataset(fea, [f["lab"]], 40)[1])
    lda, fm = fa["launches"][1], fa["launches"][2]
    assert (lda["left"], lda["right"], lda["affine"], lda["n_mats"]) == (3, 3, 0, 1)
    assert (fm["left"], fm["right"], fm["affine"], fm["n_mats"]) == (0, 0, 1, 3)
    for ln in (lda, fm):
        midx, mats, tiles = fa["arrays"][ln["at"]:ln["at"] + 3]
        assert mats.shape == (ln["n_mats"], 40, ln["D"] * (ln["left"] + ln["right"] + 1) + ln["affine"])
        assert len(midx) == len(fa["keys"]) and tiles.shape == (ln["n_tiles"], 2)
        covered = np.concatenate([np.arange(a, a + n) for a, n in tiles])
        assert np.array_equal(covered, np.arange(285))
        for a, n in tiles:
            assert len(set(id_u[a:a + n])) == 1 and n >= 1
    spk = [f["u2s"][k] for k in fa["keys"]]
    midx = fa["arrays"][fm["at"]]
    assert all((midx[i] == midx[j]) == (spk[i] == spk[j]) for i in range(9) for j in range(9))


def test_feat_tiles_break_at_utterances_and_cuts():
    srow = np.array([0, 1, 2, 3, 4, 10, 11, 12, 5, 6, 7, 8, 9], np.int32)
    urow = np.array([0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1], np.int32)
    assert D.feat_tiles(srow, urow, 3).tolist() == [[0, 3], [3, 2], [5, 3], [8, 3], [11, 1], [12, 1]]
    assert D.feat_tiles(srow, urow, 100).tolist() == [[0, 5], [5, 3], [8, 4], [12, 1]]
    assert D.feat_tiles(srow[:0], urow[:0], 4).shape == (0, 2)


@pytest.mark.parametrize("max_seq", [-1, 40])
def test_pipes_accepted_before_keep_their_tables(tmp_path, max_seq):
    """apply-cmvn --utt2spk | add-deltas --delta-order=2: the tables of the one pkc_feat_frontend
    launch, against the expectation spelled out here.  It uses nothing the earlier front-end did
    not have, so it holds before and after the stage list came."""
    from oracle import kaldi_feat as OK
    fea, u2s, stats, lab = FD.make()
    cm, us = FD.write_files(str(tmp_path), stats, u2s)
    fe = F.FeaFrontend.parse(FD.fea_opts(cm, us, order=2))
    assert (fe.order, fe.window, fe.cmvn["norm_vars"]) == (2, 2, False)
    fea ={k: v for k, v in fea.items() if k != "spkX_u999"}
    names, pieces, _, end = D.dataset_pieces({k: len(v) for k, v in fea.items()}, [lab], max_seq)
    fa = D.frontend_maps({k: len(v) for k, v in fea.items()}, 13, pieces, fe)
    assert sorted(fa) == ["D", "arrays", "cmvn_mode", "keys", "maxoff", "order", "out_shape"]
    keys = list(dict.fromkeys(k for k, _, _ in pieces))
    beg, pos = {}, 0
    for k in keys:
        beg[k] = pos
        pos += len(fea[k])
    srow = [beg[k] + t for k, a, b in pieces for t in range(a, b)]
    urow = [keys.index(k) for k, a, b in pieces for _ in range(a, b)]
    spks = list(dict.fromkeys(u2s[k] for k in keys))
    norm = np.stack([np.stack(OK.cmvn_norm(stats[s], False)) for s in spks])
    want = [np.array(srow, np.int32), np.array(urow, np.int32),
            np.array([beg[k] for k in keys], np.int32),
            np.array([beg[k] + len(fea[k]) for k in keys], np.int32),
            np.array([spks.index(u2s[k]) for k in keys], np.int32), norm.astype(np.float32),
            OK.delta_scales(2, 2)]
    assert fa["keys"] == keys and (fa["D"], fa["cmvn_mode"], fa["order"], fa["maxoff"]) == (13, 1, 2, 4)
    assert fa["out_shape"] == (len(srow), 39) and len(fa["arrays"]) == 7
    for got, exp in zip(fa["arrays"], want):
        assert got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()
    # a front-end built by hand and one parsed from add-deltas alone plan the same single launch
    hand = F.FeaFrontend()
    hand.order = 2
    parsed = F.FeaFrontend.parse("add-deltas --delta-order=2 ark:- ark:- |")
    a, b = (D.frontend_maps({k: len(v) for k, v in fea.items()}, 13, pieces, x) for x in (hand, parsed))
    assert a["cmvn_mode"] == b["cmvn_mode"] == 0 and a["out_shape"] == b["out_shape"]
    for x, y in zip(a["arrays"], b["arrays"]):
        assert x.tobytes() == y.tobytes()

"""SyncBN over the recurrent gate BatchNorms, host side: what the Engine accepts and still refuses
with sync_bn, and pkc.dist.frame_rows (every batch's global row count beside the loss scales) on a
world-2 gloo group."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_dist_cpu import _run

sys.path.insert(0, os.path.join(ROOT, "tests"))


class World:
    world, rank = 2, 1


@pytest.mark.parametrize("family", ["lstm", "ligru", "gru", "minimalgru", "rnn"])
def test_recurrent_batchnorm_accepted_with_sync_bn(family):
    """Each rank's row of the per-layer [R][G][3H] state buffer and the [G][2H] sums buffer exist
    for every BatchNorm'd recurrent layer; without sync_bn neither does."""
    import dp_seq_syncbn_worker as W
    eng, _ = W.build_engine(family, 2, W.B, sync_bn=World(), device="cpu")
    rec = next(n for n in eng.nodes if n.rec)
    assert len(rec.lbuf) == 2
    for lb in rec.lbuf:
        assert lb["bn_states"].numel() == 2 * rec.G * 3 * W.H
        assert lb["bn_sums"].numel() == rec.G * 2 * W.H
    eng, _ = W.build_engine(family, 2, W.B, device="cpu")
    assert all("bn_states" not in lb for n in eng.nodes if n.rec for lb in n.lbuf)


def test_mlp_layer_in_a_sequence_engine_accepted():
    import dp_seq_syncbn_worker as W
    eng, _ = W.build_engine("ligru", 2, W.B, sync_bn=World(), device="cpu", body="mlp")
    body = next(n for n in eng.nodes if not n.rec and n.bn)
    assert body.bn_states.numel() == 2 * 3 * body.N and body.bn_sums is not None


@pytest.mark.parametrize("family", ["lstm", "ligru", "gru", "minimalgru", "rnn"])
def test_input_batchnorm_still_refused(family):
    import dp_seq_syncbn_worker as W
    with pytest.raises(NotImplementedError, match="input BatchNorm"):
        W.build_engine(family, 2, W.B, sync_bn=World(), device="cpu", inp_bn=True)
    W.build_engine(family, 2, W.B, device="cpu", inp_bn=True)      # fine without sync_bn


def test_sequence_step_needs_global_rows():
    """On more than one rank a sequence engine does not guess the global row count."""
    import dp_seq_syncbn_worker as W
    eng, _ = W.build_engine("lstm", 2, W.B, sync_bn=World(), device="cpu")
    assert eng.global_rows is None
    with pytest.raises(ValueError, match="global_rows"):
        eng.train_step(batch=W_batch(eng))


def W_batch(eng):
    from pkc.graph import SeqBatch
    z = np.zeros(eng.B, dtype=np.int64)
    return SeqBatch((z, z + 7, z, 7), 0)


def _frame_rows(rank, ws, lens, B):
    from pkc import dist as DP
    scales, rows = DP.frame_rows(lens[rank], B, 2)
    return scales.tolist(), rows.tolist(), DP.frame_weights(lens[rank], B, 2).tolist()


def test_frame_rows_totals_beside_the_scales():
    """The totals are sum_r T_r * B per batch, the same on every rank; the scales are
    frame_weights's; one rank: its own T * B and scales of 1."""
    lens = [[5, 6, 9, 11, 12, 14, 99], [5, 7, 8, 11, 13, 15, 99]]
    B = 3
    T = np.array([[9, 14], [8, 15]])
    (s0, r0, w0), (s1, r1, w1) = _run(_frame_rows, 2, lens, B)
    assert r0 == r1 == (T.sum(0) * B).tolist()
    assert s0 == w0 and s1 == w1
    np.testing.assert_allclose(s0, T[0] / T.sum(0), rtol=1e-12)
    np.testing.assert_allclose(s1, T[1] / T.sum(0), rtol=1e-12)
    s, r, w = _frame_rows(0, 1, lens, B)
    assert s == w == [1.0, 1.0] and r == (T[0] * B).tolist()

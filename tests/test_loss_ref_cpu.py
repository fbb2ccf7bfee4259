"""What tests/test_gpu_loss.py rests on, checked without a GPU: its float64 reference against
torch's log_softmax + nll_loss autograd, its error bound against a float32 log_softmax of the same
inputs (something that is not the kernel), and the conditions its inputs are drawn to meet."""
import numpy as np
import pytest
import torch

import loss_cases as LC

EVERY = (LC.CASES + LC.ALIGNED + [h for launch in LC.MULTI for h in launch] + LC.MULTI_FALLBACK)
IDS = [LC.case_id(c) for c in EVERY]


def _torch64(i, weight):
    z = (i.slabs.double().sum(0) + (i.bias.double() if i.bias is not None else 0.0)).requires_grad_()
    lp = torch.log_softmax(z, 1)
    y = torch.from_numpy(i.y)
    loss = torch.nn.functional.nll_loss(lp, y)
    (weight * loss).backward()
    rows = torch.nn.functional.nll_loss(lp, y, reduction="none")
    return lp.detach(), z.grad, loss.detach(), rows.detach()


@pytest.mark.parametrize("c", EVERY, ids=IDS)
def test_reference_is_torch_float64(c):
    i, ref = LC.inputs(c), LC.reference(c)
    lp, grad, loss, rows = _torch64(i, c.weight)
    prior = i.prior.double() if i.prior is not None else 0.0
    t = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(torch.from_numpy(ref.logp), lp - prior, **t)
    torch.testing.assert_close(torch.from_numpy(ref.dlogits), grad, **t)
    torch.testing.assert_close(torch.from_numpy(ref.row_loss), rows, **t)
    torch.testing.assert_close(torch.tensor(ref.row_loss.mean()), loss, **t)
    assert np.isfinite(ref.logp).all() and np.isfinite(ref.dlogits).all()
    assert ((0 <= i.y) & (i.y < c.N)).all()
    assert i.lab.shape == (c.M, c.lstride) and bool((i.lab[:, -1].numpy() == i.y).all())


@pytest.mark.parametrize("c", EVERY, ids=IDS)
def test_float32_log_softmax_stays_inside_the_bound(c):
    """The slabs summed in order in fp32, + bias, torch.log_softmax in fp32, - prior: inside the
    bound the kernel is held to; and its autograd gradient inside the dlogits tolerance."""
    i, ref = LC.inputs(c), LC.reference(c)
    z = i.slabs[0].clone()
    for s in range(1, c.S):
        z += i.slabs[s]
    if i.bias is not None:
        z += i.bias
    z.requires_grad_()
    lp = torch.log_softmax(z, 1)
    (c.weight * torch.nn.functional.nll_loss(lp, torch.from_numpy(i.y))).backward()
    out = (lp - i.prior if i.prior is not None else lp).detach()
    b = LC.bound(c.S, ref.z)
    err = np.abs(out.double().numpy() - ref.logp).max()
    assert err <= b, "float32 log_softmax misses the bound: %.3g > %.3g" % (err, b)
    torch.testing.assert_close(z.grad.double(), torch.from_numpy(ref.dlogits), **LC.T_DLOGITS)


@pytest.mark.parametrize("c", [c for c in EVERY if c.kind == "rand"],
                         ids=[LC.case_id(c) for c in EVERY if c.kind == "rand"])
def test_random_rows_have_a_clear_maximum(c):
    """row_err is compared exactly, so the two largest logits of every row lie further apart than
    the error allowed on a logit (every row: a seed that violates this is to be changed)."""
    ref = LC.reference(c)
    gap = LC.top2_gap(ref.z)
    assert gap.min() > LC.bound(c.S, ref.z), (gap.min(), LC.bound(c.S, ref.z))


def test_labels_reach_the_edges_and_both_outcomes():
    """Over the random cases: labels at column 0, at N - 1 and in the last 16-byte chunk; rows
    with error 0 and rows with error 1."""
    for c in LC.NARROW + LC.WIDE + LC.FALLBACK:
        i, ref = LC.inputs(c), LC.reference(c)
        if c.M >= 3:
            assert i.y[0] == 0 and i.y[1] == c.N - 1 and i.y[2] == max(c.N - 3, 0)
        if c.M >= 5 and c.N >= 48:
            assert set(ref.row_err.tolist()) == {0.0, 1.0}, LC.case_id(c)


@pytest.mark.parametrize("c", LC.TIES, ids=[LC.case_id(c) for c in LC.TIES])
def test_tie_cases_are_exact_ties(c):
    i, ref = LC.inputs(c), LC.reference(c)
    assert bool((i.slabs == i.slabs.round()).all()) and ref.z.max() == 8.0
    assert np.abs(i.slabs.numpy()).max() * c.S < 2 ** 20            # every fp32 partial sum is exact
    pairs = LC.tie_pairs(c)
    for k, (a, b) in enumerate(pairs):
        for r in (2 * k, 2 * k + 1):
            assert np.flatnonzero(ref.z[r] == ref.z[r].max()).tolist() == [a, b]
    assert (ref.z[-2:] == 2.0).all()
    assert ref.row_err.tolist() == i.expect_err.tolist() == [0.0, 1.0] * (len(pairs) + 1)


@pytest.mark.parametrize("c", LC.RANGE, ids=[LC.case_id(c) for c in LC.RANGE])
def test_range_cases_underflow_in_float32(c):
    i, ref = LC.inputs(c), LC.reference(c)
    assert np.float32(np.exp(np.float32(-170.0))) == 0.0
    assert ref.z.max() > 1e4 and np.sort(ref.z, 1)[:, -2].max() < 1e4 - 80
    assert (ref.z.max(1) - np.sort(ref.z, 1)[:, -2] > 170).all()
    assert (ref.row_loss[[2, 3, 5]] > 170).all() and np.isfinite(ref.row_loss).all()
    assert (i.slabs.double().sum(0).float().double().numpy() == ref.z).all()   # exact in fp32


def test_the_tables_cover_every_form():
    assert {c.form for c in LC.CASES} == LC.ALL_FORMS
    for forms in ({0, 1, 2, 3, 4, 5, 6, 7}, {8, 9, 10, 11, 12, 13, 14, 15}):
        for S in (3, 5, 7):                         # slab counts below the capacity, in both bodies
            assert any(c.S == S and c.form in forms for c in LC.CASES)
    assert {h.form for launch in LC.MULTI for h in launch} == set(range(16))
    assert {len(launch) for launch in LC.MULTI} == {1, 2, 3, 4}
    assert any(len({h.M for h in launch}) > 1 for launch in LC.MULTI)
    assert any(h.form < 0 for h in LC.MULTI_FALLBACK)
    assert {c.N for c in LC.NARROW} >= {1, 2, 3, 4, 5, 48, 63, 64, 65, 100, 257, 508, 511}
    assert {c.M for c in LC.NARROW} >= {1, 3, 4, 5, 7, 130}
    assert {c.N for c in LC.WIDE} >= {512, 513, 1028, 1928, 2044, 2047, 2048}
    assert {c.M for c in LC.WIDE} >= {1, 3, 5}
    assert {c.N for c in LC.FALLBACK} >= {2049, 2052, 4100, 48, 600}
    assert {c.S for c in LC.CASES} >= {1, 2, 3, 4, 5, 7, 8, 9}
    assert max(c.M for c in LC.CASES) <= 130

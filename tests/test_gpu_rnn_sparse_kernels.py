"""The block-sparse step kernels (rnn_fwd_mm / rnn_bwd_mm with SP = true, read through
pkc_rnn_args.kmap_*) and the persistent liGRU loops (pkc_rnn_persist.hip, form 1) through the C ABI
(tests/rnn_kernel.py), per time step against the float64 step oracle with the masked U — the method
and the bound of tests/test_gpu_rnn_kernels.py: every tensor of a step against the restatement of
that ONE step from the run's own saved state, max|got - ref| / max|ref| <= 2e-5 per tensor, no
outliers, plus the exact checks, the sentinel guards and a bit-identical rerun of _run.

  a. fp32 block-sparse steps, all five cells: 16 / 32 / 64 slots x 16-row / one 32-row / two row
     tiles x load width 4 / 2 / 1, a table with an all -1 forward and BPTT row, T = 1, dy in 3 slabs;
  b. bf16 step products over a kmap (liGRU, LSTM), one case per slot count;
  c. sparse liGRU in the grid-synchronised loops (default environment);
  d. the persistent liGRU loops at every plan class tests/test_rnn_tables_cpu.py names (no cut
     tile, 7 cuts, a tile without a block, a run fixed by the longest tile, register-only, LDS
     slots, both slot limits, fewer fragments than waves), H = 576, ragged H, odd and large B2, one
     direction, T = 1 and 2, dy in two slabs (bwd_loop<true>), mixed forms, the generated mask;
  e. unlisted blocks are never read: U poisoned outside the listed (tile, block) pairs.

The tables come from pkc.engine.rnn_kmaps / persist_plans (checked on the CPU by
tests/test_rnn_tables_cpu.py, which also shows the float32 evaluation of every case here under a
quarter of the bound).  Per-tensor maxima are printed (pytest -s;
profiles/rnn_sparse_kernels_pytest_gpu.txt: the largest measured on an MI355X were 4.2e-7 for the
fp32 block-sparse steps, 2.1e-7 for the bf16 block-sparse steps against their bf16 operands, 1.5e-7
for the sparse liGRU in the grid-synchronised loops and 1.8e-7 for the persistent loops; 89 cases
in 3.6 s, 5.3 s of wall time for the whole module)."""
import pytest
import torch

import rnn_kernel as RK
from test_gpu_rnn_kernels import _run, per_step  # noqa: F401  (per_step: a fixture)

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.id for c in cases]


def _go(c):
    inp = RK.sparse_inputs(c)
    kmaps, plans = RK.case_tables(c, inp["umask"])
    if kmaps is not None:
        assert kmaps[1] == c.slots and kmaps[3] == c.slots, (kmaps[1], kmaps[3])
        assert bool((kmaps[0] == -1).any()) and bool((kmaps[2] == -1).any())
    assert plans is not None or 1 not in c.form, "no plan for a persistent case"
    return _run(c, bf16=c.bf16, form=c.form, inp=inp, mask=c.mask, umask=inp["umask"],
                kmaps=kmaps, plans=plans)


@pytest.mark.parametrize("c", RK.sparse_fp32_cases(), ids=_ids(RK.sparse_fp32_cases()))
def test_sparse_fp32_steps(c, per_step):
    _go(c)


@pytest.mark.parametrize("c", RK.sparse_bf16_cases(), ids=_ids(RK.sparse_bf16_cases()))
def test_sparse_bf16_steps(c, per_step):
    _go(c)


@pytest.mark.parametrize("c", RK.sparse_grid_cases(), ids=_ids(RK.sparse_grid_cases()))
def test_sparse_ligru_grid_loops(c):
    """Default environment: form 2 with a kmap set (a 0 is a failure)."""
    _go(c)


@pytest.mark.parametrize("c", RK.persist_cases(), ids=_ids(RK.persist_cases()))
def test_persistent_ligru_loops(c):
    """Form (1, 1) from pkc_rnn_persist_form itself; the mixed case (1, 0)."""
    _go(c)


# --------------------------------------------------------------------- unlisted blocks are not read
def _kmap_cover(c, kmaps, bwd):
    """(G, H, H) bool: the elements of U the listed (tile, block) pairs of a step table cover, from
    the layout text of include/pkc.h."""
    H, G = c.H, RK.CELLS[c.cell][1]
    cov = torch.zeros(G, H, H, dtype=torch.bool)
    nb = -(-H // 16)
    if bwd:
        tab = kmaps[2].view(G, nb, -1)
        for g in range(G):
            for kt in range(nb):
                for j in tab[g, kt].tolist():
                    if j >= 0:
                        cov[g, 16 * j:16 * j + 16, 16 * kt:16 * kt + 16] = True
        return cov
    cand = RK.CAND.get(c.cell)
    phases = [(list(range(G)), 0)] if cand is None else [([g for g in range(G) if g != cand], 0)]
    if cand is not None:
        nu0 = 16 // (G - 1)
        phases.append(([cand], -(-H // nu0)))
    for gates, row0 in phases:
        nu = 16 // len(gates)
        for i in range(-(-H // nu)):
            for b in kmaps[0][row0 + i].tolist():
                if b >= 0:
                    for g in gates:
                        cov[g, nu * i:nu * i + nu, 16 * b:16 * b + 16] = True
    return cov


def _plan_cover(c, plan, bwd):
    """The elements both gates' U the valid fragments of a persistent plan cover."""
    cov = torch.zeros(2, c.H, c.H, dtype=torch.bool)
    for e in plan.tolist():
        if (e >> 17) & 1 and (e >> 8) & 255:
            t, b = e & 255, ((e >> 8) & 255) - 1
            if bwd:
                cov[:, 32 * b:32 * b + 32, 16 * t:16 * t + 16] = True
            else:
                cov[:, 16 * t:16 * t + 16, 32 * b:32 * b + 32] = True
    return cov


POISON = [RK.make_scase("gru", 3, 322, 17, "tanh", 32, seed=79000),
          RK.make_scase("ligru", 3, 40, 6, "relu", 16, "emptyrow", seed=79001, bf16=True),
          RK.make_scase("ligru", 3, 96, 6, "tanh", 0, "empty_tile", seed=79002, bf16=True,
                        form=(1, 1), bidir=True)]


@pytest.mark.parametrize("c", POISON, ids=_ids(POISON))
def test_unlisted_blocks_are_not_read(c, monkeypatch):
    """include/pkc.h: "-1 = empty slot: never read".  Every element of U / U_h that no listed
    (tile, block) of the forward table covers holds FILL during the forward, every element the BPTT
    table does not cover during the BPTT (U rewritten between the two calls): every output is
    bit-identical to the clean run's.  (A refused lane's load of element 0 of its row is discarded by
    a select: "read" is about values, which is what a bit-identical output shows.)"""
    if c.form == (0, 0):
        monkeypatch.setenv("PKC_RNN_LIGRU_GRID", "0")
        monkeypatch.setenv("PKC_RNN_LSTM_PERSIST", "0")
    inp = RK.sparse_inputs(c)
    kmaps, plans = RK.case_tables(c, inp["umask"])
    if c.form[0] == 1:
        cover = [_plan_cover(c, plans[0], False), _plan_cover(c, plans[1], True)]
    else:
        cover = [_kmap_cover(c, kmaps, False), _kmap_cover(c, kmaps, True)]
    for cv in cover:
        assert bool((cv | ~inp["umask"]).all()), "the table does not cover the mask"
        assert int((~cv).sum()) > 0, "nothing to poison"

    def layer():
        lay = RK.Layer(c.cell, c.T, c.B, c.H, c.bidir, c.act, inp, bf16=c.bf16, umask=inp["umask"],
                       kmaps=kmaps, plans=plans)
        assert (lay.form(0), lay.form(1)) == c.form
        return lay

    def put(lay, cv):
        U = torch.where(cv, inp["U"], torch.full_like(inp["U"], RK.FILL))
        lay.U.copy_(U)
        if c.bf16:
            lay.U_h.copy_(U.to(torch.bfloat16))

    clean = layer()
    clean.forward()
    clean.backward()
    dirty = layer()
    put(dirty, cover[0])
    dirty.forward()
    torch.cuda.synchronize()
    put(dirty, cover[1])
    dirty.backward()
    names = ["hs", "gates", "y", "dgates", "dpre"] + (["rh"] if c.cell in RK.CAND else []) + \
        (["hs_h", "dgates_h"] if c.bf16 else [])
    for k in names:
        assert torch.equal(clean.get(k, True), dirty.get(k, True)), \
            "%s: %s changes with the unlisted blocks of U" % (c.id, k)
    dirty.check_guards()

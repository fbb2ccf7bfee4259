"""The host-built tables of the recurrent kernels, without a GPU: the block-sparse step tables
(pkc.engine.rnn_kmaps -> pkc_rnn_args.kmap_*) and the fragment plans of the persistent liGRU loops
(pkc.engine.persist_plans -> pkc_rnn_args.persist_*), each decoded here from the layout text of
include/pkc.h alone and compared with the mask; then what the case tables of
tests/test_gpu_rnn_sparse_kernels.py reach (tests/rnn_kernel.py), and that its 2e-5 bound rests on
fp32 arithmetic: the float32 evaluation of every new case's restatement stays under a quarter."""
import numpy as np
import pytest
import torch

import rnn_kernel as RK
from pkc import engine as E


def _geo():
    """(waves, forward slots, BPTT slots, largest H) from pkc_rnn_persist_geometry, read where it is
    used: the kmap tests need no library."""
    nw, nsf, nsb, _, hmax = E.persist_geometry()
    return nw, nsf, nsb, hmax


# --------------------------------------------------------------------------------- the mask sweep
def _band_mask(H, G, seed):
    m = RK.block_mask(H, 0.7, seed, G)
    m[:, 16:32, :] = False          # an empty 16-row band
    m[:, :, 32:48] = False          # an empty 16-column band
    return m


def _sweep():
    """[(name, (G, H, H) bool)] for G = 1 .. 4: HCGS-style, random blocks, empty bands."""
    out = []
    for G in (1, 2, 3, 4):
        for H in (40, 96, 550):
            out.append(("hcgs-H%d-G%d" % (H, G), RK.hcgs_mask(H, 100 + H).expand(G, H, H).clone()))
        for H, keep in ((22, 0.6), (25, 0.5), (100, 0.4), (321, 0.85)):
            out.append(("blocks-H%d-G%d" % (H, G), RK.block_mask(H, keep, 200 + H + G, G)))
        for H in (50, 96):
            out.append(("bands-H%d-G%d" % (H, G), _band_mask(H, G, 300 + H + G)))
    return out


def _cell_masks():
    """[(name, cell, masks)]: the sweep for every cell of its gate count, and every mask of the
    GPU case tables."""
    out = []
    for name, m in _sweep():
        for cell, (_, G) in RK.CELLS.items():
            if G == m.shape[0]:
                out.append((name + "-" + cell, cell, m))
    for c in RK.sparse_fp32_cases() + RK.sparse_bf16_cases() + RK.sparse_grid_cases():
        out.append((c.id, c.cell, RK.case_mask(c)))
    return out


# ------------------------------------------------------------------------------------- kmap tables
def _blocks16(rows):
    """The 16-wide column blocks of a (n, H) bool slab that hold a True."""
    cols = np.nonzero(rows.any(0).numpy())[0]
    return sorted({int(k) // 16 for k in cols})


def _check_row(row, want, where):
    row = row.tolist()
    listed = [b for b in row if b != -1]
    assert row[:len(listed)] == listed, "%s: a -1 in front of a listed block" % (where,)
    assert all(b >= 0 for b in listed), where
    assert len(set(listed)) == len(listed), "%s: a block listed twice" % (where,)
    assert sorted(listed) == want, "%s: lists %s, the mask has %s" % (where, sorted(listed), want)
    return len(listed)


def _check_kmaps(cell, m):
    G, H = m.shape[0], m.shape[1]
    cand = RK.CAND.get(cell)
    kf, sf, kb, sb = E.rnn_kmaps(list(m), cand, "force")
    nb = -(-H // 16)
    # forward: one-phase tiles of 16 / G units x G gates; two-phase: the tiles of the NG = G - 1
    # gates that read h_{t-1} (16 / NG units each), then the candidate's 16-unit tiles
    if cand is None:
        phases = [list(range(G))]
    else:
        phases = [[g for g in range(G) if g != cand], [cand]]
    want = []
    for gates in phases:
        nu = 16 // len(gates)
        for i in range(-(-H // nu)):
            want.append(_blocks16(torch.cat([m[g, nu * i:nu * i + nu] for g in gates])))
    fullest = max(len(w) for w in want)
    S = next((s for s in (16, 32, 64) if s >= fullest), None)
    if S is None:
        assert kf is None and sf == 0
    else:
        assert sf == S and kf.dtype == torch.int32 and tuple(kf.shape) == (len(want), S)
        assert not kf.is_cuda
        for i, w in enumerate(want):
            _check_row(kf[i], w, (cell, "fwd", i))
    # BPTT: [G][ceil(H / 16)] rows, the 16-row blocks j with a nonzero in columns 16 kt .. + 15
    wantb = [_blocks16(m[g, :, 16 * kt:16 * kt + 16].t()) for g in range(G) for kt in range(nb)]
    fullest = max(len(w) for w in wantb)
    S = next((s for s in (16, 32, 64) if s >= fullest), None)
    if S is None:
        assert kb is None and sb == 0
    else:
        assert sb == S and tuple(kb.shape) == (G * nb, S)
        for i, w in enumerate(wantb):
            _check_row(kb[i], w, (cell, "bwd", divmod(i, nb)))
    return sf, sb


def test_kmap_tables_list_exactly_the_nonzero_blocks():
    seen = set()
    for name, cell, m in _cell_masks():
        seen.update(_check_kmaps(cell, m))
    assert {16, 32, 64} <= seen


def test_kmap_tables_past_64_slots_and_modes():
    m = torch.ones(1, 1056, 1056, dtype=torch.bool)            # 66 blocks in every row
    assert E.rnn_kmaps(list(m), None, "force") == (None, 0, None, 0)
    m[0, :, 1024:] = False                                     # 64 forward blocks, 66 / 64 BPTT
    m[0, 1024:, :] = False
    kf, sf, kb, sb = E.rnn_kmaps(list(m), None, "force")
    assert sf == 64 and sb == 64 and bool((kf[:64] >= 0).all()) and bool((kf[64:] == -1).all())
    # "auto": a table only under the dense strip (16 at H <= 256, 32 <= 512, 48 <= 768, 64 <= 1024)
    small = RK.block_mask(40, 0.6, 1, 2)
    assert E.rnn_kmaps(list(small), None, "auto") == (None, 0, None, 0)
    assert E.rnn_kmaps(list(small), None, "off") == (None, 0, None, 0)
    thin = RK.hcgs_mask(550, 7).expand(2, 550, 550)
    kf, sf, kb, sb = E.rnn_kmaps(list(thin), None, "auto")
    assert kf is not None and kb is not None and 0 < sf < 48 and 0 < sb < 48     # dense strip: 48
    ff, sff, bb, sbb = E.rnn_kmaps(list(thin), None, "force")
    assert (sf, sb) == (sff, sbb) and torch.equal(kf, ff) and torch.equal(kb, bb)
    _check_kmaps("ligru", thin)


# ------------------------------------------------------------------------------- persistent plans
def _fragments(mask, bwd):
    """{(tile, block)}: forward tiles of 16 units x 32-wide blocks of k with a nonzero; BPTT tiles
    of 16 columns k x 32-wide blocks of units j."""
    m = mask.numpy().T if bwd else mask.numpy()
    H = m.shape[0]
    return {(t, b) for t in range(-(-H // 16)) for b in range(-(-H // 32))
            if m[16 * t:16 * t + 16, 32 * b:32 * b + 32].any()}


def _want_run(mask, bwd):
    """The documented run: ceil(fragments / waves), at least the longest tile (a tile is cut once
    at the most), at least 1."""
    NW, NSF, NSB, HMAX = _geo()
    frs = _fragments(mask, bwd)
    per = {}
    for t, _ in frs:
        per[t] = per.get(t, 0) + 1
    return max(1, -(-len(frs) // NW), max(per.values(), default=0))


def _register_slots():
    """(forward, BPTT) register-resident slots per wave, from the kernel source (the geometry
    call reports the slot counts only)."""
    NW, NSF, NSB, HMAX = _geo()
    import os
    import re
    src = open(os.path.join(os.path.dirname(E.__file__), "..", "csrc", "pkc_rnn_persist.hip")).read()
    f = re.search(r"FNF = (\d+), FNFR = (\d+);", src)
    b = re.search(r"BNF = (\d+), BNFR = (\d+);", src)
    assert f and b, "pkc_rnn_persist.hip no longer declares 'FNF = .., FNFR = ..;' / 'BNF = .., BNFR = ..;'"
    assert (int(f.group(1)), int(b.group(1))) == (NSF, NSB)
    return int(f.group(2)), int(b.group(2))


def _walk(plan, nslots):
    """The host simulator: every wave's slots in order.  Returns the flushes [(tile, spill index or
    None, [(tile, block)])] and the plan's statistics."""
    NW, NSF, NSB, HMAX = _geo()
    tab = np.asarray(plan).reshape(NW, nslots)
    flushes, runs = [], []
    for w in range(NW):
        acc, done, ended = [], set(), False
        n = 0
        for f in range(nslots):
            e = int(tab[w, f])
            if not (e >> 17) & 1:
                ended = True
                continue
            assert not ended, "wave %d: a valid slot behind an empty one" % w
            n += 1
            t, b = e & 255, ((e >> 8) & 255) - 1
            assert b >= 0, "a valid slot without a block"
            assert t not in done, "wave %d: tile %d comes back after its flush" % (w, t)
            assert not acc or acc[-1][0] == t, "wave %d: tile %d cut by another tile" % (w, t)
            acc.append((t, b))
            spill = (e >> 18) & 1
            if (e >> 16) & 1:
                flushes.append((t, (e >> 19) & 7 if spill else None, acc))
                done.add(t)
                acc = []
            else:
                assert not spill, "the spill-over bit on a slot that does not flush"
        assert not acc, "wave %d ends with unflushed fragments of tile %d" % (w, acc[-1][0] if acc else -1)
        runs.append(n)
    return flushes, runs


def _check_plan(mask2d, plan, nslots, bwd):
    NW, NSF, NSB, HMAX = _geo()
    flushes, runs = _walk(plan, nslots)
    frags = [tb for _, _, acc in flushes for tb in acc]
    want = _fragments(mask2d, bwd)
    assert len(frags) == len(set(frags)), "a fragment dealt twice"
    assert set(frags) == want, "the plan's fragments are not the mask's"
    own = [t for t, sp, _ in flushes if sp is None]
    cut = [(t, sp) for t, sp, _ in flushes if sp is not None]
    assert len(own) == len(set(own)), "a tile flushed to itself twice"
    assert len({t for t, _ in cut}) == len(cut), "a tile with two spill-over parts"
    assert len({sp for _, sp in cut}) == len(cut), "two tiles share a spill-over tile"
    assert all(sp < NW - 1 for _, sp in cut)
    return flushes, runs


def _simulate_products(U, v, flushes, bwd):
    """What the loop's cell update sees: each tile's stored products plus its spill-over tile's."""
    H = U.shape[0]
    nt = -(-H // 16)
    Up = np.zeros((nt * 32, nt * 32), dtype=np.int64)
    Up[:H, :H] = U.T if bwd else U
    vp = np.zeros(nt * 32, dtype=np.int64)
    vp[:H] = v
    tile, spill, where = np.zeros((nt, 16), np.int64), {}, {}
    for t, sp, acc in flushes:
        s = sum(Up[16 * t:16 * t + 16, 32 * b:32 * b + 32] @ vp[32 * b:32 * b + 32] for _, b in acc)
        if sp is None:
            tile[t] = s
        else:
            spill[sp], where[t] = s, sp
    for t, sp in where.items():
        tile[t] = tile[t] + spill[sp]
    return tile.reshape(-1)[:H]


def _plan_masks():
    NW, NSF, NSB, HMAX = _geo()
    out = [(name, m.any(0)) for name, m in _sweep() if m.shape[0] == 1 and m.shape[1] % 2 == 0
           and m.shape[1] <= HMAX]
    for c in RK.persist_cases():
        out.append((c.id, RK.case_mask(c).any(0)))
    for c in RK.sparse_fp32_cases():
        if c.cell == "rnn" and c.H % 2 == 0 and c.H <= HMAX:
            out.append((c.id, RK.case_mask(c).any(0)))
    return out


def test_persist_plans_deal_every_fragment_once_and_multiply_right():
    NW, NSF, NSB, HMAX = _geo()
    g = np.random.RandomState(5)
    checked = 0
    for name, m in _plan_masks():
        plans = E.persist_plans(m.numpy())
        fits = _want_run(m, False) <= NSF and _want_run(m, True) <= NSB
        assert (plans is not None) == fits, name
        if plans is None:
            continue
        checked += 1
        H = m.shape[0]
        U = g.randint(-3, 4, size=(H, H)) * m.numpy()
        v = g.randint(-4, 5, size=H)
        for plan, nslots, bwd in ((plans[0], NSF, False), (plans[1], NSB, True)):
            assert plan.dtype == np.int32 and plan.shape == (NW * nslots,), name
            flushes, runs = _check_plan(m, plan, nslots, bwd)
            assert max(runs) <= nslots
            got = _simulate_products(U, v, flushes, bwd)
            want = (U.T if bwd else U) @ v
            assert np.array_equal(got, want), "%s %s: the plan's products" % (name, "bwd" if bwd else "fwd")
    assert checked >= len(RK.persist_cases())


def test_persist_plans_refusals():
    NW, NSF, NSB, HMAX = _geo()
    assert E.persist_plans(np.ones((97, 97), bool)) is None                    # odd H
    assert E.persist_plans(np.ones((HMAX + 2, HMAX + 2), bool)) is None        # H above hmax
    assert E.persist_plans(np.ones((HMAX, HMAX), bool)) is None                # 648 fragments
    # a run above one slot count alone: seeded searches over random block masks at H = hmax
    def runs(m):
        return _want_run(m, False), _want_run(m, True)
    fwd_over = RK._search(lambda s: RK.block_mask(HMAX, 0.15, 900 + s)[0],
                          lambda m: runs(m)[0] == NSF + 1 and runs(m)[1] <= NSB)
    assert E.persist_plans(fwd_over.numpy()) is None
    bwd_over = RK._search(lambda s: RK.block_mask(HMAX, 0.15, 900 + s)[0],
                          lambda m: runs(m)[0] <= NSF and runs(m)[1] == NSB + 1)
    assert E.persist_plans(bwd_over.numpy()) is None
    ok = RK._search(lambda s: RK.block_mask(HMAX, 0.15, 900 + s)[0],
                    lambda m: runs(m)[0] <= NSF and runs(m)[1] <= NSB)
    assert E.persist_plans(ok.numpy()) is not None


# ------------------------------------------------------------------------- what the tables reach
def test_sparse_table_reaches_every_instantiation():
    cases = RK.sparse_fp32_cases()
    allc = cases + RK.sparse_bf16_cases() + RK.sparse_grid_cases() + RK.persist_cases()
    assert len({c.id for c in allc}) == len(allc) and len({c.seed for c in allc}) == len(allc)
    for cell in RK.CELLS:
        mine = [c for c in cases if c.cell == cell]
        assert 9 <= len(mine) <= 12
        forms = [RK.sparse_step_form(cell, c.H, c.B2, c.slots) for c in mine]
        main = [(f, c) for f, c in zip(forms, mine) if c.T == 3 and c.nslab == 1 and c.kind == "blocks"]
        tiling = {(f[0], RK.row_class(c.B2)) for f, c in main}
        loads = {(f[0], f[4]) for f, c in main}
        for S in (16, 32, 64):
            for rc in ("16-row", "one 32-row tile", "two tiles"):
                assert (S, rc) in tiling, (cell, S, rc)
            for vw in (4, 2, 1):
                assert (S, vw) in loads, (cell, S, vw)
        assert {f[1] for f in forms} == {4}
        assert {c.B2 for c in mine} == {6, 17, 34}
        assert any(c.T == 1 for c in mine) and any(c.nslab == 3 for c in mine)
        assert any(c.kind == "emptyrow" for c in mine)
        assert {c.act for c in mine} == ({"tanh"} if cell == "lstm" else {"relu", "tanh"}), cell
    bf = RK.sparse_bf16_cases()
    for cell in ("ligru", "lstm"):
        got = {(c.slots, RK.row_class(c.B2), RK.sparse_step_form(cell, c.H, c.B2, c.slots, True)[4])
               for c in bf if c.cell == cell}
        assert got == {(16, "16-row", "h8"), (32, "one 32-row tile", "h2"), (64, "two tiles", "h1")}
    assert {(c.H, c.form) for c in RK.sparse_grid_cases()} == {(48, (2, 2)), (550, (2, 2))}
    assert all(c.B2 <= 16 and not c.bf16 for c in RK.sparse_grid_cases())


def test_sparse_cases_have_the_slot_count_they_were_chosen_for():
    for c in RK.sparse_fp32_cases() + RK.sparse_bf16_cases() + RK.sparse_grid_cases():
        m = RK.case_mask(c)
        (kf, sf, kb, sb), _ = RK.case_tables(c, m)
        assert (sf, sb) == (c.slots, c.slots), (c.id, sf, sb)
        assert bool((kf == -1).any()) and bool((kb == -1).any()), c.id
        fullest = max(int((kf >= 0).sum(1).max()), int((kb >= 0).sum(1).max()))
        assert fullest > c.slots // 2 or c.slots == 16, (c.id, fullest)    # (more than S / 2 kept)
        if c.kind == "emptyrow":
            assert bool((kf == -1).all(1).any()) and bool((kb == -1).all(1).any()), c.id
            G, nb = RK.CELLS[c.cell][1], -(-c.H // 16)
            assert bool((kb.view(G, nb, -1)[:, 0] == -1).all())


def test_persist_table_reaches_every_plan_class():
    NW, NSF, NSB, HMAX = _geo()
    seen, regs = set(), _register_slots()
    for c in RK.persist_cases():
        m = RK.case_mask(c).any(0)
        kmaps, plans = RK.case_tables(c, RK.case_mask(c))
        assert plans is not None, c.id
        assert c.form[0] == 1 and c.bf16 and c.cell == "ligru"
        (ff, fr), (bf_, br) = (_check_plan(m, plans[0], NSF, False), _check_plan(m, plans[1], NSB, True))
        for tag, flushes, runs, nslots, nreg, bwd in (("fwd", ff, fr, NSF, regs[0], False),
                                                       ("bwd", bf_, br, NSB, regs[1], True)):
            frs = _fragments(m, bwd)
            total, run = len(frs), max(runs)
            cuts = sum(1 for _, sp, _ in flushes if sp is not None)
            nt = -(-c.H // 16)
            longest = max(sum(1 for t, _ in frs if t == i) for i in range(nt))
            if cuts == 0:
                seen.add("no cut")
            if cuts == NW - 1:
                seen.add("%d cuts %s" % (NW - 1, tag))
            if any(all(t != i for t, _ in frs) for i in range(nt)):
                seen.add("tile without a block " + tag)
            if run == longest and run > -(-total // NW):
                seen.add("longest tile " + tag)
            if run == nslots:
                seen.add("slot limit " + tag)
            if total < NW:
                seen.add("fewer fragments than waves")
            if min(runs) == 0:
                seen.add("empty wave")
            seen.add(("registers only" if run <= nreg else "LDS slots") + " " + tag)
            assert run == _want_run(m, bwd), (c.id, tag)
    for need in ("no cut", "%d cuts fwd" % (NW - 1), "%d cuts bwd" % (NW - 1),
                 "tile without a block fwd", "tile without a block bwd", "longest tile fwd",
                 "longest tile bwd", "slot limit fwd", "slot limit bwd", "fewer fragments than waves",
                 "empty wave", "registers only fwd", "registers only bwd", "LDS slots fwd",
                 "LDS slots bwd"):
        assert need in seen, need
    shapes = {(c.H, c.B2, c.bidir, c.T, c.nslab, c.form, c.mask) for c in RK.persist_cases()}
    assert {c.H for c in RK.persist_cases()} >= {2, 18, 32, 34, 46, 96, 550, HMAX}
    assert any(c.B2 > 16 and c.B2 % 2 for c in RK.persist_cases())               # odd, above 16
    assert any(not c.bidir and c.H == 96 for c in RK.persist_cases())            # one direction
    assert {1, 2, 3, 4} <= {c.T for c in RK.persist_cases()}
    assert {h for h, _, _, _, ns, f, _ in shapes if ns == 2 and f == (1, 1)} == {96, 550}
    assert any(ns == 3 and f == (1, 0) for _, _, _, _, ns, f, _ in shapes)
    assert any(mk == "gen" for *_, mk in shapes)
    assert {c.act for c in RK.persist_cases()} == {"relu", "tanh"}


# ---------------------------------------------------------------------------- float32 headroom
GAP_BOUND = 2e-5 / 4       # a quarter of tests/test_gpu_rnn_sparse_kernels.py's bound


def _gap(c):
    inp = RK.sparse_inputs(c)
    s, _ = RK.simulate(c, inp)
    ref = RK.restate(c.cell, c.act, s)
    lo = RK.restate(c.cell, c.act, RK.cast_state(s, torch.float32))
    worst = ("", 0.0)
    for (name, _, r64), (_, _, r32) in zip(ref, lo):
        err = float((r32.double() - r64).abs().max()) / max(float(r64.abs().max()), 1e-30)
        assert np.isfinite(err), (c.id, name)
        if err > worst[1]:
            worst = (name, err)
    return worst


@pytest.mark.parametrize("group", ["fp32", "bf16", "grid", "persist"])
def test_float32_restatement_gap_is_a_quarter_of_the_gpu_bound(group):
    """A condition on the cases, not a measurement of the kernels: the float32 evaluation of each
    step of every new case (masked U) against the float64 one, from the same float64 states."""
    cases = {"fp32": RK.sparse_fp32_cases, "bf16": RK.sparse_bf16_cases,
             "grid": RK.sparse_grid_cases, "persist": RK.persist_cases}[group]()
    worst = ("", "", 0.0)
    for c in cases:
        name, err = _gap(c)
        assert err <= GAP_BOUND, "%s %s: float32 gap %.3g" % (c.id, name, err)
        if err > worst[2]:
            worst = (c.id, name, err)
    print("%s: largest float32-vs-float64 gap %.3g (%s, %s)" % (group, worst[2], worst[0], worst[1]))

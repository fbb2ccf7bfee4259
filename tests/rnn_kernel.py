"""Kernel-level harness of the recurrent time loops (pkc_rnn_fwd / pkc_rnn_bwd): one layer through
the C ABI, every buffer in the layout include/pkc.h documents (fields as Engine._rnn_args fills
them), every buffer the kernels write between sentinel guards.  Also the host-side mirror of the
step kernels' dispatch (step_form) and the table of cases tests/test_gpu_rnn_kernels.py runs, so the
CPU suite can check what the table reaches without a GPU (tests/test_oracle_steps_cpu.py).  The
block-sparse step kernels and the persistent liGRU loops take a U mask and the tables of
pkc.engine.rnn_kmaps / persist_plans (Layer's umask / kmaps / plans); their dispatch mirror
(sparse_step_form), masks and case tables are the second half of the tables section, run by
tests/test_gpu_rnn_sparse_kernels.py and checked on the CPU by tests/test_rnn_tables_cpu.py."""
import collections
import ctypes as C
import functools

import torch

from pkc import _lib as L

DEV = "cuda"
CELLS = {"ligru": (L.CELL_LIGRU, 2), "lstm": (L.CELL_LSTM, 4), "gru": (L.CELL_GRU, 3),
         "mingru": (L.CELL_MINGRU, 2), "rnn": (L.CELL_RNN, 1)}
GUARD = 64                # elements in front of and behind every guarded buffer (16-byte multiples)
FILL = -24576.0           # sentinel: exact in fp32 and bf16, outside every tensor's range here
NAN = float("nan")


# ------------------------------------------------------------------------------ dispatch mirror
def strip_width(H):
    """PKC_S_DISPATCH: the contraction strip per lane group (16 lane groups x S >= H)."""
    return 16 if H <= 256 else 32 if H <= 512 else 48 if H <= 768 else 64 if H <= 1024 else 128


def step_form(cell, H, B2, bf16=False, ln=False):
    """Which per-step instantiation fwd_impl_s / bwd_impl_s select for a dense U:
    (S, waves, rows per tile, row tiles, load form).  waves: of the forward step (the dense
    one-phase cells run 8-wave tiles at S >= 32; the two-phase cells and every one-gate BPTT
    product keep 4).  load form: pick_vw's 4 / 2 / 1 floats per load, or for the bf16 strips
    "h8" / "h2" / "h1" (load_strip_h: 8-wide when H % 8 == 0, pairs when H is even, elements)."""
    assert cell in CELLS and 0 < H <= 2048 and B2 > 0
    assert not bf16 or (cell in ("ligru", "lstm", "rnn") and not ln)
    S = strip_width(H)
    waves = 8 if cell in ("ligru", "lstm", "rnn") and S >= 32 else 4
    rows = 16 if B2 <= 16 else 32
    vw = 4 if H % 4 == 0 else 2 if H % 2 == 0 else 1
    load = ("h8" if H % 8 == 0 else "h2" if H % 2 == 0 else "h1") if bf16 else vw
    return S, waves, rows, (B2 + rows - 1) // rows, load


def row_class(B2):
    rows = 16 if B2 <= 16 else 32
    return "16-row" if rows == 16 else "one 32-row tile" if B2 <= 32 else "two tiles"


# ------------------------------------------------------------------------------ the case tables
Case = collections.namedtuple("Case", "cell T B bidir H act nslab seed")
Case.B2 = property(lambda c: 2 * c.B if c.bidir else c.B)
Case.id = property(lambda c: "%s-T%d-H%d-B2_%d-%s%s" % (
    c.cell, c.T, c.H, c.B2, c.act, "-slabs%d" % c.nslab if c.nslab > 1 else ""))

ROWS_OF = {1: (1, False), 2: (1, True), 3: (3, False), 6: (3, True), 12: (6, True),
           16: (16, False), 17: (17, False), 20: (10, True), 32: (16, True),
           34: (17, True)}                                        # B2 -> (B, bidir)
H_CLASSES = {16: (5, 250, 256), 32: (257, 510, 512), 48: (513, 550, 768), 64: (769, 770, 1024),
             128: (1025, 1030, 2048)}
# per strip class: the B2 of its three H values (vw 1, 2, 4) — one of each row-tiling class, in an
# order that changes from class to class
_B2_ROT = ((6, 17, 34), (16, 32, 34), (34, 6, 17), (17, 34, 16), (32, 34, 6))


def make_case(cell, T, H, B2, act, nslab=1, seed=0):
    B, bidir = ROWS_OF[B2]
    return Case(cell, T, B, bidir, H, "tanh" if cell == "lstm" else act, nslab, seed)


def fp32_cases():
    """The per-step exact-fp32 table: per cell, 15 (H, B2) pairs at T = 3, then T = 1, T = 2 and a
    dy in 3 slabs."""
    out = []
    for ci, cell in enumerate(CELLS):
        for si, (S, Hs) in enumerate(H_CLASSES.items()):
            for hi, H in enumerate(Hs):
                act = ("relu", "tanh")[(ci + si + hi) % 2]
                out.append(make_case(cell, 3, H, _B2_ROT[si][hi], act, seed=1000 * ci + 10 * si + hi))
        out.append(make_case(cell, 1, 250, 17, "relu", seed=1000 * ci + 900))
        out.append(make_case(cell, 2, 257, 6, "tanh", seed=1000 * ci + 901))
        out.append(make_case(cell, 3, 510, 34, "relu", nslab=3, seed=1000 * ci + 902))
    return out


def ln_cases():
    """LayerNorm of h: all five cells x H in {5, 64, 65, 130, 550} x B2 in {3, 6, 34}, T = 3."""
    out = []
    for ci, cell in enumerate(CELLS):
        for hi, H in enumerate((5, 64, 65, 130, 550)):
            for bi, B2 in enumerate((3, 6, 34)):
                act = ("relu", "tanh")[(ci + hi + bi) % 2]
                out.append(make_case(cell, 3, H, B2, act, seed=20000 + 100 * ci + 10 * hi + bi))
    return out


def bf16_cases():
    """bf16 step products: liGRU, LSTM, RNN x H in {24, 264, 510, 513, 768, 1024, 1032} x B2 in
    {6, 17, 34}, T = 3."""
    out = []
    for ci, cell in enumerate(("ligru", "lstm", "rnn")):
        for hi, H in enumerate((24, 264, 510, 513, 768, 1024, 1032)):
            for bi, B2 in enumerate((6, 17, 34)):
                act = ("relu", "tanh")[(ci + hi + bi) % 2]
                out.append(make_case(cell, 3, H, B2, act, seed=30000 + 100 * ci + 10 * hi + bi))
    return out


def grid_cases():
    """The grid-synchronised loops (default environment), T = 4: [(case, bf16)]."""
    out = [(make_case("ligru", 4, H, B2, ("relu", "tanh")[i % 2], seed=40000 + i), False)
           for i, (H, B2) in enumerate(((24, 6), (257, 16), (550, 6), (768, 12)))]
    for bf in (False, True):
        out += [(make_case("lstm", 4, H, B2, "tanh", seed=40100 + 10 * bf + i), bf)
                for i, (H, B2) in enumerate(((512, 6), (768, 20), (1024, 32)))]
    return out


# ------------------------------------------------------------------ block-sparse and persistent
def sparse_step_form(cell, H, B2, slots, bf16=False):
    """fwd_impl_s / bwd_impl_s with SP = true (a kmap table of `slots` slots per tile): S = slots
    whatever H is, 4 waves always (step_waves<S, true>), 16-row tiles up to B2 = 16, the load width
    from H alone.  bf16 (BF && SP): liGRU and LSTM only (check() refuses the RNN, the two-phase
    cells have no bf16 steps)."""
    assert cell in CELLS and 0 < H <= 2048 and B2 > 0 and slots in (16, 32, 64)
    assert not bf16 or cell in ("ligru", "lstm")
    rows = 16 if B2 <= 16 else 32
    vw = 4 if H % 4 == 0 else 2 if H % 2 == 0 else 1
    load = ("h8" if H % 8 == 0 else "h2" if H % 2 == 0 else "h1") if bf16 else vw
    return slots, 4, rows, (B2 + rows - 1) // rows, load


CAND = {"gru": 2, "mingru": 1}          # the two-phase cells' candidate gate


def block_mask(H, keep, seed, G=1, thin=0.5, bs=16):
    """G masks (G, H, H) bool of random bs x bs blocks, each kept with probability `keep`; inside a
    kept block every element but the first stays with probability `thin` (the tables must list a
    block for one nonzero)."""
    g = torch.Generator().manual_seed(seed)
    nb = -(-H // bs)
    blocks = torch.rand(G, nb, nb, generator=g) < keep
    m = blocks.repeat_interleave(bs, 1).repeat_interleave(bs, 2)[:, :H, :H].clone()
    first = torch.zeros(G, H, H, dtype=torch.bool)
    first[:, ::bs, ::bs] = True
    return m & ((torch.rand(G, H, H, generator=g) < thin) | first)


def hcgs_mask(H, seed, blocks=(32, 2), drops=(75, 75)):
    """(1, H, H) bool HCGS mask (oracle.masks.hcgs_conn_mat, C3's [32, 2] / [75, 75] by default)."""
    import numpy as np
    from oracle import masks as OM
    m = OM.hcgs_conn_mat(H, H, list(blocks), list(drops), np.random.RandomState(seed))
    return torch.from_numpy(m != 0)[None]


def _plans(mask):
    from pkc import engine as E
    return E.persist_plans(mask.any(0).numpy())


def plan_stats(plan, nw):
    """(fragments, run = the longest wave's valid slots, cut tiles, waves with no slot) of one plan."""
    tab = plan.reshape(nw, -1)
    valid = (tab >> 17) & 1
    return (int(valid.sum()), int(valid.sum(1).max()), int((valid & (tab >> 18) & 1).sum()),
            int((valid.sum(1) == 0).sum()))


def _search(make, ok, tries=4000):
    for s in range(tries):
        m = make(s)
        if ok(m):
            return m
    raise AssertionError("no mask found in %d seeds" % tries)


@functools.lru_cache(maxsize=None)
def _persist_mask(kind, H, seed):
    """(1, H, H) bool masks for the persistent liGRU loops' plan classes (one mask for both gates, as
    the plan is the union's).  Seeded searches take the first seed whose plans (pkc.engine.
    persist_plans) have the property; the searches read the geometry, never a kernel's output."""
    from pkc import engine as E
    nw, nsf, nsb = E.persist_geometry()[:3]
    if kind == "dense":
        return torch.ones(1, H, H, dtype=torch.bool)
    if kind == "blocks":
        return _search(lambda s: block_mask(H, 0.6, seed + s), lambda m: _plans(m) is not None)
    if kind == "c3":            # a C3-like HCGS mask whose plans fit the slots
        return _search(lambda s: hcgs_mask(H, seed + s), lambda m: _plans(m) is not None)

    def run_is(which, want):
        def ok(m):
            p = _plans(m)               # (once per mask)
            return p is not None and plan_stats(p[which], nw)[1] == want
        return ok
    if kind == "slots_fwd":     # forward run == the forward slot count
        return _search(lambda s: block_mask(H, 0.15, seed + s), run_is(0, nsf))
    if kind == "slots_bwd":     # BPTT run == the BPTT slot count
        return _search(lambda s: block_mask(H, 0.15, seed + s), run_is(1, nsb))
    if kind == "cuts":          # nwaves - 1 cut tiles in both plans
        def ok(m):
            p = _plans(m)
            return p is not None and all(plan_stats(x, nw)[2] == nw - 1 for x in p)
        return _search(lambda s: block_mask(H, 0.5, seed + s), ok)
    if kind == "longest":       # one full unit band and one full column band over a thin diagonal
        m = torch.zeros(1, H, H, dtype=torch.bool)
        m[0, :16, :] = True
        m[0, :, :16] = True
        for i in range(0, H, 16):
            m[0, i:i + 16, i:i + 16] = True
        return m & block_mask(H, 1.0, seed)
    if kind == "empty_tile":    # unit tile 1 and column tile 2 without a block
        m = block_mask(H, 0.7, seed)
        m[0, 16:32, :] = False
        m[0, :, 32:48] = False
        return m
    raise ValueError(kind)


def persist_mask(kind, H, seed=0):
    """A fresh copy of the mask _persist_mask finds (cached per (kind, H, seed): the searches are
    deterministic, and both the CPU reach test and the GPU cases ask for the same masks)."""
    return _persist_mask(kind, H, seed).clone()


SCase = collections.namedtuple("SCase", "cell T B bidir H act nslab seed slots kind bf16 form mask")
SCase.B2 = property(lambda c: 2 * c.B if c.bidir else c.B)
SCase.id = property(lambda c: "%s-%s%s-T%d-H%d-B2_%d-%s%s%s%s" % (
    c.cell, c.kind, "-S%d" % c.slots if c.slots else "", c.T, c.H, c.B2, c.act,
    "-slabs%d" % c.nslab if c.nslab > 1 else "", "-bf16" if c.bf16 else "",
    "-gen" if c.mask == "gen" else ""))

SPARSE_H = {16: (40, 22, 25), 32: (320, 322, 321), 64: (560, 562, 561)}      # vw 4, 2, 1 each
SPARSE_KEEP = {16: 0.6, 32: 0.85, 64: 0.92}     # block keep rate: the fullest row needs S slots
_SB2_ROT = ((6, 17, 34), (34, 6, 17), (17, 34, 6))


def make_scase(cell, T, H, B2, act, slots=0, kind="blocks", nslab=1, seed=0, bf16=False,
               form=(0, 0), mask="inject", bidir=None):
    B, bd = ROWS_OF[B2] if bidir is None else ((B2 // 2, True) if bidir else (B2, False))
    return SCase(cell, T, B, bd, H, "tanh" if cell == "lstm" else act, nslab, seed, slots, kind,
                 bf16, form, mask)


def sparse_fp32_cases():
    """fp32 block-sparse steps: per cell 9 (H, B2) pairs at T = 3 — slots 16 / 32 / 64 x the three
    load widths, the row classes rotating — then a table with an all -1 forward row and an all -1
    BPTT row, T = 1, and dy in 3 slabs."""
    out = []
    for ci, cell in enumerate(CELLS):
        for si, (S, Hs) in enumerate(SPARSE_H.items()):
            for hi, H in enumerate(Hs):
                act = ("relu", "tanh")[(ci + si + hi) % 2]
                out.append(make_scase(cell, 3, H, _SB2_ROT[(si + ci) % 3][hi], act, S,
                                      seed=70000 + 1000 * ci + 10 * si + hi))
        out.append(make_scase(cell, 3, 40, 17, "relu", 16, "emptyrow", seed=70000 + 1000 * ci + 900))
        out.append(make_scase(cell, 1, 25, 17, "tanh", 16, seed=70000 + 1000 * ci + 901))
        out.append(make_scase(cell, 3, 322, 34, "relu", 32, nslab=3, seed=70000 + 1000 * ci + 902))
    return out


def sparse_bf16_cases():
    """bf16 step products over a kmap (BF && SP): liGRU and LSTM, one case per slot count, each at
    another row class; H a multiple of 8, even, odd (load_strip_h's three forms)."""
    out = []
    for ci, cell in enumerate(("ligru", "lstm")):
        for i, (S, H, B2) in enumerate(((16, 40, 6), (32, 322, 17), (64, 561, 34))):
            out.append(make_scase(cell, 3, H, B2, ("relu", "tanh")[(ci + i) % 2], S,
                                  seed=76000 + 100 * ci + i, bf16=True))
    return out


def sparse_grid_cases():
    """Sparse liGRU in the grid-synchronised loops (default environment, fp32, B2 <= 16)."""
    return [make_scase("ligru", 3, 48, 6, "relu", 16, seed=77000, form=(2, 2)),
            make_scase("ligru", 3, 550, 16, "tanh", 64, seed=77001, form=(2, 2))]


def persist_cases():
    """The persistent liGRU loops (bf16 steps, form 1), relu and tanh in turn: a C3-like HCGS plan,
    H = 576 at either slot limit, register-only and tiny plans, ragged H with 34 workgroups, 7 cut
    tiles, a run fixed by the longest tile, a tile without a block, T = 1 and 2, dy in 2 slabs, the
    mixed forms (1, 0) and the generated dropout mask (tests/test_gpu_rnn_sparse_kernels.py, d)."""
    P = dict(cell="ligru", bf16=True, form=(1, 1))
    rows = [  # (kind, T, H, B2, bidir, extra)
        ("c3", 4, 550, 16, True, {}),
        ("slots_fwd", 3, 576, 3, False, {}),
        ("slots_bwd", 3, 576, 3, False, {}),
        ("dense", 3, 96, 17, False, {}),
        ("dense", 3, 32, 6, True, {}),
        ("dense", 3, 2, 1, False, {}),
        ("blocks", 3, 18, 34, True, {}),
        ("blocks", 3, 34, 34, True, {}),
        ("blocks", 3, 46, 34, True, {}),
        ("cuts", 3, 160, 6, True, {}),
        ("longest", 3, 256, 3, False, {}),
        ("empty_tile", 3, 96, 6, True, {}),
        ("dense", 1, 96, 6, True, {}),
        ("dense", 2, 96, 6, True, {}),
        ("dense", 3, 96, 6, True, dict(nslab=2)),
        ("c3", 3, 550, 6, True, dict(nslab=2)),
        ("dense", 3, 96, 12, True, dict(nslab=3, slots=16, form=(1, 0))),
        ("blocks", 3, 96, 6, True, dict(mask="gen")),
    ]
    out = []
    for i, (kind, T, H, B2, bidir, extra) in enumerate(rows):
        kw = dict(P, kind=kind, seed=78000 + i, bidir=bidir)
        kw.update(extra)
        cell = kw.pop("cell")
        out.append(make_scase(cell, T, H, B2, ("relu", "tanh")[i % 2], **kw))
    return out


def case_mask(c):
    """The case's U masks (G, H, H) bool: per-gate masks for the step tables, one shared mask for
    the persistent loops."""
    G = CELLS[c.cell][1]
    if c.form[0] == 1:
        return persist_mask(c.kind, c.H, c.seed).expand(G, c.H, c.H).clone()
    m = block_mask(c.H, SPARSE_KEEP[c.slots], c.seed + 3, G)
    if c.kind == "emptyrow":
        m[:, 16:32, :] = False      # forward tiles of units 16..31: no block (all gates)
        m[:, :, :16] = False        # BPTT tiles of columns 0..15: no block
    return m


def case_tables(c, umask):
    """(kmaps, plans) of a case: the step tables of pkc.engine.rnn_kmaps ("force": a table whenever
    it fits) when the case has a slot count, the persistent plans when it expects form 1."""
    from pkc import engine as E
    kmaps = E.rnn_kmaps(list(umask), CAND.get(c.cell), "force") if c.slots else None
    plans = E.persist_plans(umask.any(0).numpy()) if 1 in c.form else None
    return kmaps, plans


def sparse_inputs(c):
    """make_inputs with the masked U (the kernels' contract: unlisted entries are zero) and the mask."""
    inp = make_inputs(c)
    inp["umask"] = case_mask(c)
    inp["U"] = inp["U"] * inp["umask"]
    return inp


def make_inputs(c, ln=False):
    """The layer's inputs as fp32 CPU tensors (the values both the GPU run and the float64
    restatements read): U_g = randn / sqrt(H), wpre and dy = randn, a Bernoulli(0.8) mask, and for
    LayerNorm random gamma / beta."""
    g = torch.Generator().manual_seed(c.seed)
    G = CELLS[c.cell][1]
    D = 2 * c.H if c.bidir else c.H
    d = dict(U=torch.randn(G, c.H, c.H, generator=g) / c.H ** 0.5,
             wpre=torch.randn(G, c.T, c.B, c.H, generator=g),
             dy=torch.randn(c.T, c.B, D, generator=g),
             mask=(torch.rand(c.B2, c.H, generator=g) < 0.8).float())
    if ln:
        d["gamma"] = 1 + 0.5 * torch.randn(c.H, generator=g)
        d["beta"] = 0.5 * torch.randn(c.H, generator=g)
    return d


def dy_slabs(dy, nslab, seed):
    """dy as nslab partial slabs whose sum is dy (slab s < nslab - 1 random), fp32 CPU."""
    g = torch.Generator().manual_seed(seed + 7)
    parts = [torch.randn(dy.shape, generator=g) for _ in range(nslab - 1)]
    last = dy.clone()
    for p in parts:
        last = last - p
    return torch.stack(parts + [last])


# ------------------------------------------------------------------------------ the harness
class Guarded:
    """A device buffer of n elements the kernels own, GUARD sentinel elements in front and behind,
    the owned part filled with the sentinel too (or with `init`)."""

    def __init__(self, n, dtype=torch.float32, init=None):
        self.n = int(n)
        assert self.n > 0
        self.buf = torch.full((self.n + 2 * GUARD,), FILL, dtype=dtype, device=DEV)
        self.own = self.buf[GUARD:GUARD + self.n]
        assert self.own.data_ptr() % 16 == 0
        if init is not None:
            self.own.copy_(init.reshape(-1))

    @property
    def p(self):
        return self.own.data_ptr()

    def get(self, written=False):
        """The owned region on the CPU; guards intact, and (written) no sentinel left in it."""
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert bool((b[:GUARD] == FILL).all()), "a kernel wrote in front of its buffer"
        assert bool((b[GUARD + self.n:] == FILL).all()), "a kernel wrote behind its buffer"
        own = b[GUARD:GUARD + self.n].clone()
        if written:
            left = int((own == FILL).sum())
            assert left == 0, "%d of %d elements were never written" % (left, self.n)
        return own

    def untouched(self):
        assert bool((self.get() == FILL).all()), "a refused call wrote memory"


def _dev(t, dtype=None):
    t = t.to(DEV).contiguous() if dtype is None else t.to(DEV, dtype).contiguous()
    assert t.data_ptr() % 16 == 0
    return t


class Layer:
    """One layer's buffers and the argument struct of both entry points.
    mask: "inject" (inp["mask"] through drop_mask_in), "gen" (the library's generator) or None
    (drop_p = 0); ln: LayerNorm of h with inp["gamma"] / inp["beta"]; bf16: bf16 step products.
    umask: (G, H, H) U mask — U and U_h are multiplied by it (the block-sparse kernels' contract:
    unlisted entries are zero); kmaps: (kmap_fwd, s_fwd, kmap_bwd, s_bwd) of pkc.engine.rnn_kmaps;
    plans: (persist_fwd, persist_bwd) of pkc.engine.persist_plans (persist_kb from the geometry).
    The tables live in ordinary device tensors."""

    def __init__(self, cell, T, B, H, bidir, act, inp, ln=False, bf16=False, mask="inject",
                 train=True, drop_p=0.2, nslab=1, slab_seed=0, step=0, seed=1234, stream_id=77,
                 umask=None, kmaps=None, plans=None):
        self.cell, self.T, self.B, self.H, self.bidir = cell, T, B, H, bool(bidir)
        cid, G = CELLS[cell]
        self.G, self.B2 = G, 2 * B if bidir else B
        B2, D = self.B2, (2 * H if bidir else H)
        self.D = D
        n = B2 * H
        self.wpre = _dev(inp["wpre"])
        self.U_cpu = inp["U"] if umask is None else inp["U"] * umask
        self.U = _dev(self.U_cpu)
        self.bufs = {}
        mk = self._mk
        mk("drop_mask", n)
        mk("hs", (T + 1) * n)
        if cell == "lstm":
            mk("cs", (T + 1) * n)
        mk("gates", G * T * n)
        mk("y", T * B * D)
        if cell in ("gru", "mingru"):
            mk("rh", T * n)
        mk("dgates", G * T * n)
        mk("work", 8 * n)
        mk("ut", G * H * H)
        mk("dpre", G * T * B * H)
        a = L.RnnArgs()
        a.cell, a.T, a.B, a.H, a.bidir = cid, T, B, H, int(bool(bidir))
        a.act, a.train = L.ACT[act], int(train)
        a.wpre = self.wpre.data_ptr()
        for g in range(G):
            a.U[g] = self.U[g].data_ptr()
        a.drop_p = drop_p if mask else 0.0
        a.seed, a.stream_id = seed, stream_id
        self.ctr = torch.tensor([step], dtype=torch.int64, device=DEV)
        a.step_ctr = self.ctr.data_ptr()
        self.mask_in = _dev(inp["mask"]) if mask == "inject" else None
        a.drop_mask_in = self.mask_in.data_ptr() if self.mask_in is not None else None
        for k in ("drop_mask", "hs", "cs", "gates", "y", "rh", "dgates", "work", "ut"):
            if k in self.bufs:
                setattr(a, k, self.bufs[k].p)
        if ln:
            self.gamma, self.beta = _dev(inp["gamma"]), _dev(inp["beta"])
            a.ln_gamma, a.ln_beta, a.ln_eps = self.gamma.data_ptr(), self.beta.data_ptr(), 1e-6
            for k, sz in (("ln_xhat", T * n), ("ln_stat", T * B2 * 2), ("ln_g", T * n),
                          ("ln_dgamma", H), ("ln_dbeta", H)):
                mk(k, sz)
                setattr(a, k, self.bufs[k].p)
        if bf16:
            # U_h = RNE(U), made with torch (the caller keeps these copies current)
            self.U_h = _dev(self.U_cpu, torch.bfloat16)
            a.step_bf16 = 1
            for k, sz in (("hs_h", (T + 1) * n), ("ut_h", G * H * H), ("dgates_h", G * T * n)):
                mk(k, sz, torch.bfloat16)
                setattr(a, k, self.bufs[k].p)
            for g in range(G):
                a.U_h[g] = self.U_h[g].data_ptr()
        # dy: nslab slabs at a padded stride, NaN in the padding
        self.dy_parts = dy_slabs(inp["dy"], nslab, slab_seed) if nslab > 1 else inp["dy"][None]
        cnt = T * B * D
        stride = cnt + 12 if nslab > 1 else cnt
        flat = torch.full((nslab * stride,), NAN)
        for s in range(nslab):
            flat[s * stride:s * stride + cnt] = self.dy_parts[s].reshape(-1)
        self.dy = _dev(flat)
        a.dy, a.dy_nslab, a.dy_slab_stride = self.dy.data_ptr(), nslab, stride if nslab > 1 else 0
        self.tables = {}
        if kmaps is not None:
            for name, tab, S in (("kmap_fwd", kmaps[0], kmaps[1]), ("kmap_bwd", kmaps[2], kmaps[3])):
                if tab is not None:
                    self.tables[name] = _dev(tab.to(torch.int32))
                    setattr(a, name, self.tables[name].data_ptr())
                    setattr(a, name.replace("kmap_", "kmap_s_"), S)
        if plans is not None:
            from pkc import engine as E
            for name, tab in zip(("persist_fwd", "persist_bwd"), plans):
                self.tables[name] = _dev(torch.as_tensor(tab, dtype=torch.int32))
                setattr(a, name, self.tables[name].data_ptr())
            a.persist_kb = E.persist_geometry()[1]
        self.a = a

    def _mk(self, name, n, dtype=torch.float32):
        self.bufs[name] = Guarded(n, dtype)

    def form(self, bwd):
        return L.lib().pkc_rnn_persist_form(C.byref(self.a), int(bwd))

    def forward(self):
        L.call("pkc_rnn_fwd", C.byref(self.a), None)

    def backward(self):
        L.call("pkc_rnn_bwd", C.byref(self.a), C.c_void_p(self.bufs["dpre"].p), None)

    def raw(self, name):
        """Status of an entry point without raising (the refusal tests)."""
        if name == "pkc_rnn_fwd":
            return L.lib().pkc_rnn_fwd(C.byref(self.a), None)
        return L.lib().pkc_rnn_bwd(C.byref(self.a), C.c_void_p(self.bufs["dpre"].p), None)

    def get(self, name, written=False):
        """Buffer `name` on the CPU in its documented shape (guards checked)."""
        T, B, B2, H, G, D = self.T, self.B, self.B2, self.H, self.G, self.D
        shape = {"drop_mask": (B2, H), "hs": (T + 1, B2, H), "cs": (T + 1, B2, H),
                 "gates": (G, T, B2, H), "y": (T, B, D), "rh": (T, B2, H), "dgates": (G, T, B2, H),
                 "work": (8, B2, H), "ut": (G, H, H), "dpre": (G, T, B, H), "ln_xhat": (T, B2, H),
                 "ln_stat": (T, B2, 2), "ln_g": (T, B2, H), "ln_dgamma": (H,), "ln_dbeta": (H,),
                 "hs_h": (T + 1, B2, H), "ut_h": (G, H, H), "dgates_h": (G, T, B2, H)}[name]
        return self.bufs[name].get(written).view(*shape)

    def check_guards(self):
        for b in self.bufs.values():
            b.get()

    def snapshot(self):
        """Every guarded buffer but work (scratch), for the bit-identical rerun."""
        torch.cuda.synchronize()
        return {k: b.own.clone() for k, b in self.bufs.items() if k != "work"}


# ------------------------------------------------------------------------------ the step oracle
def proc_inputs(c, inp, dtype=torch.float64):
    """wpre per gate and dL/dh from the layer output, in processing time (T, R, H)."""
    from oracle import steps as S
    G = CELLS[c.cell][1]
    wproc = [S.to_proc_time(inp["wpre"][g].to(dtype), c.B, c.bidir) for g in range(G)]
    dh_y = S.out_grad_proc_time(inp["dy"].to(dtype), c.B, c.H, c.bidir)
    return wproc, dh_y


def restate(cell, act, s, ln=None):
    """Every step of a run restated from the state the run had before it (oracle/steps.py), in
    the dtype of s.  s: hs, gates, dgates [, cs, rh] as saved; hA / dgA / UA the product operands
    (the fp32 tensors, or their bf16 copies); wproc, mask (R, H), dh_y.  ln: dict(gamma, beta, eps)
    with s holding ln_xhat, ln_stat, ln_g.  Returns [(name, got, ref)] forward then backward."""
    from oracle import steps as S
    hs, gates, dgates = s["hs"], s["gates"], s["dgates"]
    hA, dgA, UA, wproc, mask, dh_y = s["hA"], s["dgA"], s["UA"], s["wproc"], s["mask"], s["dh_y"]
    out = []
    if cell == "ligru":
        z, hcr, h = S.steps_ligru_fwd(hA[:-1], hs[:-1], UA, wproc, mask, act)
        out += [("z", gates[0], z), ("act(a)", gates[1], hcr)]
    elif cell == "lstm":
        f, i, o, cc, cn, h = S.steps_lstm_fwd(hA[:-1], hs[:-1], s["cs"][:-1], UA, wproc, mask, act)
        out += [("f", gates[0], f), ("i", gates[1], i), ("o", gates[2], o),
                ("act(cand)", gates[3], cc), ("c", s["cs"][1:], cn)]
    elif cell == "gru":
        z, r, rh, hcr, h = S.steps_gru_fwd(hA[:-1], hs[:-1], UA, wproc, mask, act, rhA=s["rh"])
        out += [("z", gates[0], z), ("r", gates[1], r), ("rh", s["rh"], rh),
                ("act(a)", gates[2], hcr)]
    elif cell == "mingru":
        z, zh, hcr, h = S.steps_mingru_fwd(hA[:-1], hs[:-1], UA, wproc, mask, act, zhA=s["rh"])
        out += [("z", gates[0], z), ("zh", s["rh"], zh), ("act(a)", gates[1], hcr)]
    else:
        hcr, h = S.steps_rnn_fwd(hA[:-1], hs[:-1], UA, wproc, mask, act)
        out += [("act(a)", gates[0], hcr)]
    lnb = None
    if ln is not None:
        xhat, den, sd, h = S.ln_h_fwd(h, ln["gamma"], ln["beta"], ln["eps"])
        out += [("ln_xhat", s["ln_xhat"], xhat), ("ln den", s["ln_stat"][..., 0:1], den),
                ("ln std", s["ln_stat"][..., 1:2], sd)]
        lnb = dict(gamma=ln["gamma"], xhat=s["ln_xhat"], den=s["ln_stat"][..., 0:1],
                   std=s["ln_stat"][..., 1:2], g_post=s["ln_g"])
    out.append(("h", hs[1:], h))
    if cell == "ligru":
        r_ = S.steps_ligru_bwd(dh_y, dgA, UA, gates[0], gates[1], hs[:-1], mask, act, ln=lnb)
        ref, gp = [r_[0], r_[1]], (r_[3] if lnb else None)
    elif cell == "lstm":
        r_ = S.steps_lstm_bwd(dh_y, dgA, UA, gates[0], gates[1], gates[2], gates[3], s["cs"][1:],
                              s["cs"][:-1], mask, act, ln=lnb)
        ref, gp = r_[:4], (r_[4] if lnb else None)
    elif cell == "gru":
        ref, gp = S.steps_gru_bwd(dh_y, dgA, UA, gates[0], gates[1], gates[2], hs[:-1], mask, act,
                                  ln=lnb)
    elif cell == "mingru":
        ref, gp = S.steps_mingru_bwd(dh_y, dgA, UA, gates[0], gates[1], hs[:-1], mask, act, ln=lnb)
    else:
        ref, gp = S.steps_rnn_bwd(dh_y, dgA, UA, gates[0], mask, act, ln=lnb)
    if lnb is not None:
        out.append(("ln_g", s["ln_g"], gp))
    out += [("dgates[%d]" % q, dgates[q], ref[q]) for q in range(len(ref))]
    if lnb is not None:
        lg = s["ln_g"] if s["ln_g"] is not None else gp
        _, dgam, dbet = S.ln_h_bwd(lg, ln["gamma"], s["ln_xhat"], lnb["den"], lnb["std"])
        out += [("ln_dgamma", s["ln_dgamma"], dgam), ("ln_dbeta", s["ln_dbeta"], dbet)]
    return out


def simulate(c, inp, ln=False):
    """The layer run sequentially through its own states in float64 (forward, then the BPTT as the
    fixed point of the per-step restatement): the state dict restate() reads."""
    from oracle import steps as S
    T, R, H = c.T, c.B2, c.H
    G = CELLS[c.cell][1]
    f64 = torch.float64
    U = [inp["U"][g].to(f64) for g in range(G)]
    wproc, dh_y = proc_inputs(c, inp)
    mask = inp["mask"].to(f64)
    lnp = dict(gamma=inp["gamma"].to(f64), beta=inp["beta"].to(f64), eps=1e-6) if ln else None
    h, cst = torch.zeros(R, H, dtype=f64), torch.zeros(R, H, dtype=f64)
    hs, cs, gl, rhl, xh, st = [h], [cst], [], [], [], []
    for t in range(T):
        w1 = [w[t:t + 1] for w in wproc]
        if c.cell == "ligru":
            z, hcr, hn = S.steps_ligru_fwd(h[None], h[None], U, w1, mask, c.act)
            gl.append(torch.stack([z[0], hcr[0]]))
        elif c.cell == "lstm":
            f, i, o, cc, cn, hn = S.steps_lstm_fwd(h[None], h[None], cst[None], U, w1, mask, c.act)
            gl.append(torch.stack([f[0], i[0], o[0], cc[0]]))
            cst = cn[0]
            cs.append(cst)
        elif c.cell == "gru":
            z, r, rh, hcr, hn = S.steps_gru_fwd(h[None], h[None], U, w1, mask, c.act)
            gl.append(torch.stack([z[0], r[0], hcr[0]]))
            rhl.append(rh[0])
        elif c.cell == "mingru":
            z, zh, hcr, hn = S.steps_mingru_fwd(h[None], h[None], U, w1, mask, c.act)
            gl.append(torch.stack([z[0], hcr[0]]))
            rhl.append(zh[0])
        else:
            hcr, hn = S.steps_rnn_fwd(h[None], h[None], U, w1, mask, c.act)
            gl.append(hcr[0][None])
        h = hn[0]
        if ln:
            xhat, den, sd, h = S.ln_h_fwd(h, lnp["gamma"], lnp["beta"], lnp["eps"])
            xh.append(xhat)
            st.append(torch.cat([den, sd], -1))
        hs.append(h)
    s = dict(hs=torch.stack(hs), gates=torch.stack(gl, 1), wproc=wproc, mask=mask, dh_y=dh_y, UA=U)
    if c.cell == "lstm":
        s["cs"] = torch.stack(cs)
    if rhl:
        s["rh"] = torch.stack(rhl)
    if ln:
        s["ln_xhat"], s["ln_stat"] = torch.stack(xh), torch.stack(st)
        s["ln_g"] = None
        s["ln_dgamma"] = s["ln_dbeta"] = torch.zeros(H, dtype=f64)
    s["hA"] = s["hs"]
    s["dgates"] = s["dgA"] = torch.zeros(G, T, R, H, dtype=f64)
    for _ in range(2 * T + 2):            # (two dependent products per step: GRU's da -> dr)
        res = [x for x in restate(c.cell, c.act, s, lnp) if x[0].startswith("dgates")]
        s["dgates"] = s["dgA"] = torch.stack([x[2] for x in res])
    if ln:
        fin = dict((x[0], x[2]) for x in restate(c.cell, c.act, s, lnp))
        s["ln_g"] = fin["ln_g"]
        fin = dict((x[0], x[2]) for x in restate(c.cell, c.act, s, lnp))
        s["ln_dgamma"], s["ln_dbeta"] = fin["ln_dgamma"], fin["ln_dbeta"]
    return s, lnp


def cast_state(s, dtype):
    return {k: ([x.to(dtype) for x in v] if isinstance(v, list) else
                v.to(dtype) if torch.is_tensor(v) else v) for k, v in s.items()}

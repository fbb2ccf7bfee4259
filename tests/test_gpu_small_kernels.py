"""Kernel-level parity of the unfused elementwise, norm and gather entry points (through the C ABI)
against plain CPU references: LayerNorm, the regularisers, fake quantisation, pkc_apply_mask,
pkc_cast_bf16, pkc_colsum, pkc_logsoftmax_bwd, pkc_batch_gather, pkc_seq_gather and
pkc_cw_apply_rows.  Every output buffer sits between two sentinel-filled guard regions (Guarded):
the guards must come back unchanged, and no sentinel may be left where the kernel is meant to write.
Inputs with a slab stride or a leading dimension are passed padded, the padding filled with NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
G = 64                  # guard elements on either side (a multiple of 16 bytes for every dtype here)
I32_SENT = 0x7fffffff


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    from pkc import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return _lib


class Guarded:
    """A device buffer of n elements the kernel owns, G guard elements in front and behind, all of
    it filled with a sentinel (or the owned part with `init`)."""

    def __init__(self, n, dtype=torch.float32, fill=7.0, init=None):
        self.n, self.fill = int(n), fill
        assert self.n > 0
        self.buf = torch.full((self.n + 2 * G,), fill, dtype=dtype, device=DEV)
        self.own = self.buf[G:G + self.n]
        if init is not None:
            self.own.copy_(init.reshape(-1))

    @property
    def p(self):
        return C.c_void_p(self.own.data_ptr())

    def get(self, written=True):
        """The owned region on the CPU; guards unchanged, and (written) no sentinel left in it."""
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert bool((b[:G] == self.fill).all()), "the kernel wrote in front of its buffer"
        assert bool((b[G + self.n:] == self.fill).all()), "the kernel wrote behind its buffer"
        own = b[G:G + self.n].clone()
        if written:
            left = int((own == self.fill).sum())
            assert left == 0, "%d of %d elements were never written" % (left, self.n)
        return own

    def untouched(self):
        assert bool((self.get(False) == self.fill).all()), "a refused call wrote memory"


def _slabs(t, stride):
    """(S, ...) CPU tensor -> flat device buffer, slab s at s * stride, NaN in the padding."""
    n = t[0].numel()
    assert stride >= n
    buf = torch.full((t.shape[0] * stride,), NAN, dtype=t.dtype)
    for s in range(t.shape[0]):
        buf[s * stride:s * stride + n] = t[s].reshape(-1)
    return buf.to(DEV)


def _refused(L, name, *args):
    """The entry point returns a status and names itself in pkc_last_error()."""
    rc = getattr(L.lib(), name)(*args)
    assert rc != 0, "%s accepted bad arguments" % name
    assert name in L.lib().pkc_last_error().decode()
    with pytest.raises(L.PkcError):
        L.call(name, *args)


def _close(got, ref, rtol, atol, what=""):
    torch.testing.assert_close(got.double(), ref.double(), rtol=rtol, atol=atol, msg=lambda m: what + ": " + m)


# ------------------------------------------------------------------------------------ LayerNorm

LN_EPS = 1e-6
# M, N, nslab, bias, dy slabs, only dbias
LN_CASES = [(1, 2, 1, False, 1, False), (3, 65, 3, True, 2, False), (5, 63, 1, True, 1, False),
            (5, 64, 3, False, 2, False), (130, 130, 1, True, 2, False), (3, 1024, 1, False, 1, True),
            (130, 1030, 3, True, 2, False), (1, 1030, 3, False, 1, False), (130, 2, 3, True, 1, False),
            (5, 1024, 3, True, 2, False), (3, 130, 1, False, 1, True)]


def _ln_ref(xs, bias, gamma, beta, dys):
    """oracle.nets.LayerNorm in float64 with autograd on x = sum of the slabs + bias."""
    from oracle.nets import LayerNorm
    N = gamma.numel()
    ln = LayerNorm(N, eps=LN_EPS).double()
    with torch.no_grad():
        ln.gamma.copy_(gamma)
        ln.beta.copy_(beta)
    b = (torch.zeros(N) if bias is None else bias).double().requires_grad_()
    x = xs.double().sum(0) + b
    x.retain_grad()
    y = ln(x)
    y.backward(dys.double().sum(0))
    xd = x.detach()
    sd = xd.std(-1, keepdim=True)
    return dict(y=y.detach(), xhat=(xd - xd.mean(-1, keepdim=True)) / (sd + LN_EPS),
                rowstat=torch.cat([sd + LN_EPS, sd], 1), dx=x.grad, dgamma=ln.gamma.grad,
                dbeta=ln.beta.grad, dbias=b.grad)


def _ln_run(L, xs, bias, gamma, beta, dys, only_dbias=False):
    S, M, N = xs.shape
    ss = M * N + 64
    xd, dyd = _slabs(xs, ss), _slabs(dys, ss)
    bd = None if bias is None else bias.to(DEV)
    gd, betd = gamma.to(DEV), beta.to(DEV)
    y, xhat, stat, dx = Guarded(M * N), Guarded(M * N), Guarded(2 * M), Guarded(M * N)
    L.call("pkc_layernorm_fwd", M, N, S, L.ptr(xd), ss, L.ptr(bd), L.ptr(gd), L.ptr(betd), LN_EPS,
           y.p, xhat.p, stat.p, _s())
    out = dict(y=y.get().view(M, N), xhat=xhat.get().view(M, N), rowstat=stat.get().view(M, 2))
    dg, db, dbi = Guarded(N), Guarded(N), Guarded(N)
    L.call("pkc_layernorm_bwd", M, N, dys.shape[0], L.ptr(dyd), ss, xhat.p, L.ptr(gd), stat.p, dx.p,
           None if only_dbias else dg.p, None if only_dbias else db.p, dbi.p, _s())
    out.update(dx=dx.get().view(M, N), dbias=dbi.get())
    if only_dbias:
        dg.untouched()
        db.untouched()
    else:
        out.update(dgamma=dg.get(), dbeta=db.get())
    # the backward reads, never writes, what the forward saved
    assert torch.equal(xhat.get().view(M, N), out["xhat"])
    assert torch.equal(stat.get().view(M, 2), out["rowstat"])
    return out


def _ln_compare(got, ref):
    # tolerances of the sibling BatchNorm kernel (test_dense_bn_fwd_bwd in test_gpu_kernels.py)
    for k in ("y", "xhat", "rowstat"):
        _close(got[k], ref[k], 1e-4, 1e-5, k)
    _close(got["dx"], ref["dx"], 1e-3, 1e-5, "dx")
    for k in ("dgamma", "dbeta", "dbias"):
        if k in got:
            _close(got[k], ref[k], 1e-4, 1e-4, k)


@pytest.mark.parametrize("M,N,nslab,bias,dyslabs,only_dbias", LN_CASES)
def test_layernorm_fwd_bwd(L, M, N, nslab, bias, dyslabs, only_dbias):
    """Rows of 1 .. 17 strides of the 64-lane wave with ragged tails, a ragged last group of 4 rows,
    1 and 3 input slabs on a padded stride, the bias present and absent, 1 and 2 gradient slabs,
    the column sums at M off a multiple of 4, optional outputs left NULL.

    dx is the difference of two terms of size |dy gamma| / std each, so in fp32 it carries a
    rounding error of about 1e-7 |dy gamma| / std whatever the kernel does (at N = 2 the two terms
    cancel entirely).  The rows are therefore drawn with std >= 0.5: rows of 2 random features
    otherwise come with std of 1e-2 and less, where that error alone passes the atol of 1e-5."""
    g = torch.Generator().manual_seed(1000 * M + N + nslab)
    xs = torch.randn(nslab, M, N, generator=g)
    bi = torch.randn(N, generator=g) * 0.3 if bias else None
    x = xs.sum(0) + (bi if bias else 0.0)
    mu, sd = x.mean(-1, keepdim=True), x.std(-1, keepdim=True)
    xs[0] += (x - mu) * ((0.5 / sd).clamp_min(1.0) - 1.0)        # stretch the rows with std < 0.5
    gamma = torch.rand(N, generator=g) + 0.5
    beta = torch.randn(N, generator=g) * 0.1
    dys = torch.randn(dyslabs, M, N, generator=g)
    _ln_compare(_ln_run(L, xs, bi, gamma, beta, dys, only_dbias), _ln_ref(xs, bi, gamma, beta, dys))


@pytest.mark.parametrize("N", [65, 1030])
def test_layernorm_constant_row(L, N):
    """A row that is exactly 0.5 everywhere: the fp32 mean is exact, std is exactly 0, so y == beta
    and xhat == 0 exactly; dx takes the std == 0 branch (torch masks d std to 0 there) and is the
    float64 autograd value (gh - mean(gh)) / eps, of order 1e6."""
    M = 3
    g = torch.Generator().manual_seed(N)
    xs = torch.randn(1, M, N, generator=g)
    xs[0, 1] = 0.5
    gamma = torch.rand(N, generator=g) + 0.5
    beta = torch.randn(N, generator=g) * 0.1
    dys = torch.randn(1, M, N, generator=g)
    got, ref = _ln_run(L, xs, None, gamma, beta, dys), _ln_ref(xs, None, gamma, beta, dys)
    assert torch.equal(got["y"][1], beta)
    assert bool((got["xhat"][1] == 0).all())
    assert got["rowstat"][1, 1].item() == 0.0
    assert got["rowstat"][1, 0].item() == np.float32(LN_EPS)
    assert bool(torch.isfinite(got["dx"]).all()) and bool(torch.isfinite(ref["dx"]).all())
    assert ref["dx"][1].abs().max() > 1e5
    _close(got["dx"][1], ref["dx"][1], 1e-3, 1e-5, "dx of the constant row")
    _ln_compare(got, ref)


def test_layernorm_refusals(L):
    x = torch.ones(16, device=DEV)
    outs = [Guarded(16) for _ in range(7)]
    y, xhat, stat, dx, dg, db, dbi = outs
    for M, N in ((4, 1), (0, 4)):
        _refused(L, "pkc_layernorm_fwd", M, N, 1, L.ptr(x), 16, None, L.ptr(x), L.ptr(x), LN_EPS,
                 y.p, xhat.p, stat.p, _s())
        _refused(L, "pkc_layernorm_bwd", M, N, 1, L.ptr(x), 16, L.ptr(x), L.ptr(x), L.ptr(x), dx.p,
                 dg.p, db.p, dbi.p, _s())
    for o in outs:
        o.untouched()


# --------------------------------------------------------------------------------- regularisers

def _reg_pack(L, items, assign=()):
    """The item list of RegTerm.items as Engine._build_reg packs it for the device."""
    arr = (L.RegItem * len(items))()
    for i, (p, g, ld, r0, r1, c0, c1, blk) in enumerate(items):
        arr[i] = L.RegItem(p=p.data_ptr(), g=None if g is None else g.data_ptr(), ld=ld, r0=r0,
                           r1=r1, c0=c0, c1=c1, block=blk, assign=1 if id(p) in assign else 0)
    return torch.frombuffer(bytearray(C.string_at(arr, C.sizeof(arr))), dtype=torch.uint8).to(DEV)


def _reg_run(L, kind, items, bstart, lam, nrows, assign=()):
    """pkc_reg_partial -> pkc_reg_finalize -> pkc_reg_grad; returns (partial, coef, loss_rows)."""
    dev = _reg_pack(L, items, assign)
    nit, nb = len(items), len(bstart) - 1
    bs = torch.tensor(bstart, dtype=torch.int32, device=DEV)
    partial, coef = Guarded(nit), Guarded(nb)
    rows = Guarded(nrows) if nrows else None
    L.call("pkc_reg_partial", kind, L.ptr(dev), nit, partial.p, _s())
    L.call("pkc_reg_finalize", kind, L.ptr(bs), nb, partial.p, lam, coef.p,
           rows.p if rows else None, nrows, _s())
    L.call("pkc_reg_grad", kind, L.ptr(dev), nit, coef.p, _s())
    return partial.get(), coef.get(), rows.get() if rows else None


def _reg_ref(op, lam, nblk, params):
    """float64: lam * sum ||p||_1, lam * sum ||p||_2, or lam * sum over the torch.chunk blocks."""
    ps = [p.double().requires_grad_() for p in params]
    tot = torch.zeros((), dtype=torch.float64)
    for p in ps:
        if op == "cost_l1":
            tot = tot + p.abs().sum()
        elif op == "cost_l2":
            tot = tot + p.norm(2)
        else:
            for col in torch.chunk(p, nblk, 1):
                for blk in torch.chunk(col, nblk, 0):
                    tot = tot + blk.norm(2)
    loss = lam * tot
    loss.backward()
    return loss.item(), [p.grad for p in ps]


LOSS_RTOL = 2e-5                      # the loss tolerance of test_engine_matches_reference_golden_steps
GRAD_TOL = dict(rtol=1e-4, atol=1e-6)  # its tolerance for updated weights


def _reg_term_case(L, op, lam, nblk, params, nrows, mode="assign"):
    """One term over `params` (CPU tensors) through the real host path.  mode: 'assign' (g = the
    term), 'add' (g += the term, onto a pre-filled gradient); a parameter given as (tensor, None)
    takes no gradient.  Returns (coef, per-parameter gradients or None)."""
    from pkc.engine import RegTerm
    want_g = [not (isinstance(p, tuple) and p[1] is None) for p in params]
    cpu = [p[0] if isinstance(p, tuple) else p for p in params]
    dev = [p.to(DEV) for p in cpu]
    gen = torch.Generator().manual_seed(5)
    before = [torch.randn(p.shape, generator=gen) for p in cpu]
    gbuf = [Guarded(p.numel(), init=b if mode == "add" else None) if w else None
            for p, b, w in zip(cpu, before, want_g)]
    term = RegTerm(op, lam, nblk, dev)
    items, bstart = term.items({id(p): g.own for p, g in zip(dev, gbuf) if g is not None})
    assign = {id(p) for p in dev} if mode == "assign" else set()
    partial, coef, rows = _reg_run(L, term.kind, items, bstart, lam, nrows, assign)
    loss, grads = _reg_ref(op, lam, nblk, cpu)
    assert bool(torch.isfinite(partial).all()) and bool(torch.isfinite(coef).all())
    assert bool((rows == rows[0]).all()), "loss_rows is not one value broadcast"
    _close(rows[:1], torch.tensor([loss]), LOSS_RTOL, 0.0, "loss")
    got = []
    for p, d, g, b, r in zip(cpu, dev, gbuf, before, grads):
        assert torch.equal(d.cpu(), p), "the parameter was written"
        if g is None:
            got.append(None)
            continue
        gg = g.get(written=(mode == "assign")).view(p.shape)
        _close(gg, r + b.double() if mode == "add" else r, what="gradient", **GRAD_TOL)
        got.append(gg)
    return coef, got


@pytest.mark.parametrize("op", ["cost_l1", "cost_l2"])
def test_reg_one_block_of_100_items(L, op):
    """300 x 1030: 3 rows per item, pkc_reg_finalize sums 100 partials of one block."""
    p = torch.randn(300, 1030, generator=torch.Generator().manual_seed(1)) * 0.05
    coef, _ = _reg_term_case(L, op, 1e-3, None, [p], 16)
    assert coef.numel() == 1


def test_reg_l2_row_wider_than_an_item(L):
    """5 x 5000: per = 1, every row an item of 5000 elements."""
    p = torch.randn(5, 5000, generator=torch.Generator().manual_seed(2))
    _reg_term_case(L, "cost_l2", 0.01, None, [p], 300, mode="add")


@pytest.mark.parametrize("R,Cc,nblk", [(100, 70, 3), (9, 10, 4)])
def test_reg_gl_ragged_chunks(L, R, Cc, nblk):
    """cost_gl on ragged torch.chunk grids: 100 x 70 in 3 x 3 blocks of 34 / 24 rows and columns
    (the last chunks shorter); 9 x 10 with nblk = 4, which gives 3 row chunks and 4 column chunks."""
    p = torch.randn(R, Cc, generator=torch.Generator().manual_seed(R))
    coef, _ = _reg_term_case(L, "cost_gl", 0.02, nblk, [p], 16)
    assert coef.numel() == len(torch.chunk(p, nblk, 0)) * len(torch.chunk(p, nblk, 1))


def test_reg_gl_zero_block(L):
    """A whole block of zeros: coef 0, gradient exactly 0 there, no NaN anywhere."""
    p = torch.randn(12, 12, generator=torch.Generator().manual_seed(3))
    p[:6, 6:] = 0.0                     # column chunk 1, row chunk 0: block 1 * 2 + 0
    coef, (g,) = _reg_term_case(L, "cost_gl", 0.5, 2, [p], 16)
    assert coef[2].item() == 0.0 and bool((coef[[0, 1, 3]] > 0).all())
    assert bool((g[:6, 6:] == 0).all()) and bool(torch.isfinite(g).all())


def test_reg_l1_zeros_take_no_gradient(L):
    p = torch.randn(33, 47, generator=torch.Generator().manual_seed(4))
    p[0, :5] = 0.0
    p[7, 3] = -0.0
    p[32, 46] = -0.0
    p[5] = 0.0
    lam = 0.125
    _, (g,) = _reg_term_case(L, "cost_l1", lam, None, [p], 16)
    assert bool((g[p == 0] == 0).all())
    assert torch.equal(g, lam * torch.sign(p))


@pytest.mark.parametrize("mode", ["add", "assign"])
def test_reg_two_parameters_one_without_gradient(L, mode):
    """One term over two parameters: the first counts in the loss only (g = NULL), the second takes
    g += term (assign = 0, onto a pre-filled gradient) or g = term (assign = 1)."""
    g = torch.Generator().manual_seed(6)
    a, b = torch.randn(40, 50, generator=g), torch.randn(33, 470, generator=g)
    _reg_term_case(L, "cost_l2", 0.03, None, [(a, None), b], 16, mode=mode)


def test_reg_item_with_ld_above_its_width(L):
    """A hand-made item: rows 2..7, columns 3..12 of a 10 x 20 matrix (ld = 20, width 9)."""
    gen = torch.Generator().manual_seed(7)
    p = torch.randn(10, 20, generator=gen)
    before = torch.randn(10, 20, generator=gen)
    pd, lam = p.to(DEV), 0.25
    for kind, norm in ((L.REG_L1, lambda t: t.abs().sum()), (L.REG_L2, lambda t: t.norm(2))):
        gb = Guarded(200, init=before)
        items = [(pd, gb.own, 20, 2, 7, 3, 12, 0)]
        _, coef, rows = _reg_run(L, kind, items, [0, 1], lam, 16)
        sub = p[2:7, 3:12].double().requires_grad_()
        loss = lam * norm(sub)
        loss.backward()
        assert bool((rows == rows[0]).all())
        _close(rows[:1], loss.detach().reshape(1), LOSS_RTOL, 0.0, "loss")
        want = before.double().clone()
        want[2:7, 3:12] += sub.grad
        got = gb.get(written=False).view(10, 20)
        _close(got, want, what="gradient", **GRAD_TOL)
        outside = torch.ones(10, 20, dtype=torch.bool)
        outside[2:7, 3:12] = False
        assert torch.equal(got[outside], before[outside]), "the gradient outside the item changed"


def test_reg_finalize_without_loss_rows(L):
    """nrows = 0 with loss_rows = NULL is accepted and still writes the coefficients."""
    partial = torch.tensor([4.0, 5.0, 16.0], device=DEV)
    bs = torch.tensor([0, 2, 3], dtype=torch.int32, device=DEV)
    coef = Guarded(2)
    L.call("pkc_reg_finalize", L.REG_L2, L.ptr(bs), 2, L.ptr(partial), 0.5, coef.p, None, 0, _s())
    assert coef.get().tolist() == [float(np.float32(0.5) / np.float32(3.0)), 0.125]


# ----------------------------------------------------------------------------- fake quantisation

@pytest.mark.parametrize("bits", [2, 8, 16])
def test_fakequant_weight(L, bits):
    """Bit for bit oracle.masks.quantize on weights already inside [-1, 1]: both sides run the same
    IEEE fp32 operations in the same order, and only exact ones (x 2^(b-1), ceil, / 2^(b-1), sign)."""
    from oracle.masks import quantize
    g = torch.Generator().manual_seed(bits)
    q = 2.0 ** (bits - 1)
    grid = torch.arange(-q, q + 1, max(1.0, q / 64)) / q            # values exactly on the grid
    special = torch.tensor([1.0, -1.0, 0.0, -0.0, 1e-30, -1e-30, 0.5, -0.5, 1.0 / q, -1.0 / q])
    for w in (torch.cat([special, grid, torch.rand(301, generator=g) * 2 - 1]),
              torch.rand(2048 * 256 + 1, generator=g) * 2 - 1):      # the grid-stride tail
        ref = quantize(w, bits)[1]
        out, wd = Guarded(w.numel()), w.to(DEV)
        L.call("pkc_fakequant_weight", L.ptr(wd), out.p, w.numel(), bits, _s())
        got = out.get()
        assert torch.equal(got, ref), "%d elements differ" % int((got != ref).sum())
        assert ref.abs().max() <= 1.0
    out = Guarded(8)
    L.call("pkc_fakequant_weight", L.ptr(wd), out.p, 0, bits, _s())     # n = 0: accepted
    out.untouched()


def test_fakequant_weight_special_values(L):
    """+-1 stay, +-0 stay 0, 1e-30 rounds up to one quantum."""
    w = torch.tensor([1.0, -1.0, 0.0, -0.0, 1e-30, -1e-30])
    for bits in (2, 8, 16):
        out, wd = Guarded(6), w.to(DEV)
        L.call("pkc_fakequant_weight", L.ptr(wd), out.p, 6, bits, _s())
        u = 2.0 ** -(bits - 1)
        assert out.get().tolist() == [1.0, -1.0, 0.0, 0.0, u, -u]


def _qinp_chain(x, bits, reps):
    """oracle.masks.quantize_inp applied reps times, each on a clone of the previous result."""
    from oracle.masks import quantize_inp
    outs, cur = [], x
    for _ in range(reps):
        cur = quantize_inp(cur.clone(), bits)
        outs.append(cur)
    return torch.stack(outs)


def _qinp_check(L, x, bits, reps):
    n = x.numel()
    ref = _qinp_chain(x, bits, reps)
    out, work = Guarded(reps * n), Guarded(136)
    xd = x.to(DEV)
    L.call("pkc_fakequant_input", L.ptr(xd), out.p, n, bits, reps, work.p, _s())
    got = out.get().view(reps, n)
    work.get(written=False)
    assert torch.equal(xd.cpu(), x), "the input was written"
    for r in range(reps):                   # every q_r, not only the last
        assert torch.equal(got[r], ref[r]), "q%d of %d at %d bits, n = %d: %d elements differ" % (
            r + 1, reps, bits, n, int((got[r] != ref[r]).sum()))
    return got


@pytest.mark.parametrize("bits", [2, 8, 16])
@pytest.mark.parametrize("n", [1, 255, 16385, 524289])
def test_fakequant_input_chain(L, bits, n):
    """q1..q_reps bit for bit against the reference chain, each of which takes its own max-abs:
    the kernel's reuse of q1's max-abs for q2..q_reps is exact, not approximate.  n = 16385 takes
    a second grid-stride pass of the 64-partial max / min reduction, n = 524289 the 2048-block cap."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(n + bits)) * 1.7
    for reps in (1, 4, 8):
        got = _qinp_check(L, x, bits, reps)
    if n >= 16385 and bits >= 8:            # the chain is no no-op a wrong kernel could pass by accident
        assert bool((got[1] != got[0]).any())    # (hundreds to thousands of elements at these seeds)


@pytest.mark.parametrize("bits", [2, 8, 16])
def test_fakequant_input_sign_and_position_of_the_maximum(L, bits):
    g = torch.Generator().manual_seed(bits)
    n = 1000
    neg_max = torch.randn(n, generator=g)
    neg_max[417] = -9.25                                # the max-abs element is negative
    all_neg = -torch.rand(n, generator=g) - 0.01        # max x < 0: var = |min x|
    last = torch.randn(n, generator=g)
    last[-1] = 11.5                                     # the max-abs element in the last position
    last_neg = torch.randn(16385, generator=g)
    last_neg[-1] = -11.5
    for x in (neg_max, all_neg, last, last_neg):
        _qinp_check(L, x, bits, 4)
    zero = torch.zeros(n)
    assert torch.equal(_qinp_check(L, zero, bits, 4), torch.zeros(4, n))   # var == 0: output = input


def test_fakequant_input_refusals(L):
    x = torch.ones(16, device=DEV)
    out, work = Guarded(9 * 16), Guarded(136)
    for bits, reps in ((8, 0), (8, 9), (0, 1)):
        _refused(L, "pkc_fakequant_input", L.ptr(x), out.p, 16, bits, reps, work.p, _s())
    out.untouched()
    work.untouched()


# --------------------------------------------------------------- pkc_apply_mask / pkc_cast_bf16

@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 1])
def test_apply_mask(L, n):
    """p <- clamp(p * mask), bit exact: mask only, clamp only (NULL mask), both, clampv <= 0 off."""
    g = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g) * 1.5
    mask = (torch.rand(n, generator=g) > 0.4).float()
    mask[::7] = 0.5                       # the multiply is a multiply, not a select
    for m, c in ((mask, 0.0), (None, 1.0), (mask, 1.0), (mask, -1.0), (None, 0.0), (mask, 0.25)):
        ref = p if m is None else p * m
        if c > 0:
            ref = ref.clamp(-c, c)
        buf, md = Guarded(n, init=p), None if m is None else m.to(DEV)
        L.call("pkc_apply_mask", buf.p, L.ptr(md), n, c, _s())
        assert torch.equal(buf.get(written=False), ref), (m is None, c)


@pytest.mark.parametrize("n", [1, 4096 * 256 + 1])
def test_cast_bf16(L, n):
    """Round to nearest even, compared as bit patterns with x.to(torch.bfloat16)."""
    bits = [0x3F808000, 0x3F818000,               # ties: even upper half stays, odd rounds up
            0xBF808000 - (1 << 32), 0xBF818000 - (1 << 32), 0x3F808001, 0x3F807FFF, 0x3F817FFF,
            0x00400000, 0x00012345, 0x80400000 - (1 << 32),      # subnormals
            0x7F800000, 0xFF800000 - (1 << 32),                  # +-inf
            0x00000000, 0x80000000 - (1 << 32)]
    special = torch.cat([torch.tensor(bits, dtype=torch.int32).view(torch.float32),
                         torch.tensor([3.4e38, -3.4e38, 1.0, -2.5, 1e-20, 65504.0])])   # 3.4e38 -> inf
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    if n > special.numel():
        x[-special.numel():] = special       # the grid-stride tail carries the special values
        xs = [x]
    else:
        xs = [x] + [v.reshape(1) for v in special]
    for v in xs:
        out, vd = Guarded(v.numel(), dtype=torch.bfloat16), v.to(DEV)
        L.call("pkc_cast_bf16", L.ptr(vd), out.p, v.numel(), _s())
        got, ref = out.get(written=False).view(torch.int16), v.to(torch.bfloat16).view(torch.int16)
        bad = (got != ref).nonzero().flatten()[:4].tolist()
        assert torch.equal(got, ref), [(hex(v.view(torch.int32)[i].item() & 0xffffffff),
                                        hex(got[i].item() & 0xffff), hex(ref[i].item() & 0xffff))
                                       for i in bad]
    assert torch.isinf(torch.tensor([3.4e38]).to(torch.bfloat16)).all()


# -------------------------------------------------------------------------------------- pkc_colsum

@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nslab", [1, 2, 4, 5, 16])
def test_colsum(L, nslab, accumulate):
    """The three instantiations (1, <= 4, <= 16 slabs) with slab counts below their capacity, on a
    padded slab stride; rows off the 32-row step, columns off the 64-column workgroup."""
    g = torch.Generator().manual_seed(nslab * 2 + accumulate)
    for M in (1, 5, 33, 100):
        for N in (1, 63, 64, 65, 200):
            x = torch.randn(nslab, M, N, generator=g)
            pre = torch.randn(N, generator=g)
            out = Guarded(N, init=pre if accumulate else None)
            ss = M * N + 64
            xd = _slabs(x, ss)
            L.call("pkc_colsum", M, N, nslab, L.ptr(xd), ss, out.p, accumulate, _s())
            ref = x.double().sum((0, 1)) + (pre.double() if accumulate else 0.0)
            _close(out.get(written=not accumulate), ref, 1e-4, 1e-4, "M=%d N=%d" % (M, N))


def test_colsum_refuses_17_slabs(L):
    x = torch.ones(17 * 8, device=DEV)
    out = Guarded(4)
    _refused(L, "pkc_colsum", 2, 4, 17, L.ptr(x), 8, out.p, 0, _s())
    out.untouched()


# ------------------------------------------------------------------------------ pkc_logsoftmax_bwd

@pytest.mark.parametrize("M", [1, 5, 130])
def test_logsoftmax_bwd(L, M):
    """dz = dy - exp(logp) rowsum(dy) against float64 autograd of log_softmax, out of place and in
    place (dz == dy); N = 1 gives exactly 0."""
    g = torch.Generator().manual_seed(M)
    for N in (1, 48, 63, 65, 1928):
        z = (torch.randn(M, N, generator=g) * 2).double().requires_grad_()
        dy = torch.randn(M, N, generator=g)
        lp = torch.log_softmax(z, 1)
        lp.backward(dy.double())
        lpd, dyd = lp.detach().float().to(DEV), dy.to(DEV)
        out = Guarded(M * N)
        L.call("pkc_logsoftmax_bwd", M, N, L.ptr(lpd), L.ptr(dyd), out.p, _s())
        inplace = Guarded(M * N, init=dy)
        L.call("pkc_logsoftmax_bwd", M, N, L.ptr(lpd), inplace.p, inplace.p, _s())
        a, b = out.get().view(M, N), inplace.get(written=False).view(M, N)
        assert torch.equal(a, b), "in place differs from out of place"
        if N == 1:
            assert bool((a == 0).all())
        _close(a, z.grad, 1e-4, 1e-5, "N=%d" % N)      # the dense-forward tolerance


# -------------------------------------------------------------------------------- pkc_batch_gather

I64_SENT = 0x7ffffffffffffff1
NB = 3          # batches in the chunk
# F, ld_feats, column offset of the source in a (rows x (off + ld)) matrix, takes the 16-byte path
GATHER_VARIANTS = [(440, 440, 0, True), (4, 4, 0, True), (441, 441, 0, False), (39, 39, 0, False),
                   (440, 442, 0, False), (440, 444, 1, False)]


def _gather_source(F, ld, off, B, nlab, g):
    rows = NB * B
    wide = torch.randn(rows, ld, generator=g)
    labels = torch.randint(0, 1928, (rows, max(nlab, 1)), generator=g, dtype=torch.int32)
    wd = wide.to(DEV)
    src = C.c_void_p(wd.data_ptr() + 4 * off)       # off = 1: a source 4 bytes off 16-byte alignment
    return wide[:, off:off + F], labels, wd, src


@pytest.mark.parametrize("B", [1, 16, 128])
@pytest.mark.parametrize("F,ld,off,vec", GATHER_VARIANTS)
def test_batch_gather(L, F, ld, off, vec, B):
    """Rows [i B, (i + 1) B) with i = counter % n_batches, copied exactly (features, labels, bf16
    copy), on the 16-byte and the scalar path; advance = 0 leaves the counter pair alone."""
    g = torch.Generator().manual_seed(F + B)
    assert (F % 4 == 0 and ld % 4 == 0 and off == 0) == vec
    for nlab in (1, 2):
        feats, labels, wd, src = _gather_source(F, ld, off, B, nlab, g)
        ld_d = labels.to(DEV)
        for with_bf16 in (False, True):
            for ctr in (0, 2, 3, 7):
                i = ctr % NB
                pair = Guarded(2, dtype=torch.int64, fill=I64_SENT, init=torch.tensor([ctr, 0]))
                x, lab = Guarded(B * F), Guarded(B * nlab, dtype=torch.int32, fill=I32_SENT)
                xb = Guarded(B * F, dtype=torch.bfloat16)
                L.call("pkc_batch_gather", src, ld, F, L.ptr(ld_d), nlab, B, NB, pair.p, x.p, lab.p, 0,
                       xb.p if with_bf16 else None, _s())
                want = feats[i * B:(i + 1) * B]
                assert torch.equal(x.get().view(B, F), want), (nlab, with_bf16, ctr)
                assert torch.equal(lab.get().view(B, nlab), labels[i * B:(i + 1) * B])
                if with_bf16:
                    assert torch.equal(xb.get().view(torch.int16).view(B, F),
                                       want.to(torch.bfloat16).view(torch.int16))
                else:
                    xb.untouched()
                assert pair.get(False).tolist() == [ctr, 0]
        assert torch.equal(wd.cpu()[:, off:off + F], feats)


@pytest.mark.parametrize("B", [1, 16, 128])
@pytest.mark.parametrize("ctr", [0, 2, 7])
def test_batch_gather_advances_its_counter(L, B, ctr):
    """advance = 1 twice: two consecutive batches (wrapping modulo n_batches), the counter + 2 and
    the completion word back at 0 after each call."""
    F, nlab = 40, 2
    g = torch.Generator().manual_seed(B + ctr)
    feats, labels, wd, src = _gather_source(F, F, 0, B, nlab, g)
    ld_d = labels.to(DEV)
    pair = Guarded(2, dtype=torch.int64, fill=I64_SENT, init=torch.tensor([ctr, 0]))
    for k in range(2):
        i = (ctr + k) % NB
        x, lab = Guarded(B * F), Guarded(B * nlab, dtype=torch.int32, fill=I32_SENT)
        L.call("pkc_batch_gather", src, F, F, L.ptr(ld_d), nlab, B, NB, pair.p, x.p, lab.p, 1, None,
               _s())
        assert torch.equal(x.get().view(B, F), feats[i * B:(i + 1) * B]), k
        assert torch.equal(lab.get().view(B, nlab), labels[i * B:(i + 1) * B]), k
        assert pair.get(False).tolist() == [ctr + k + 1, 0]


# ---------------------------------------------------------------------------------- pkc_seq_gather

@pytest.mark.parametrize("F", [1, 40, 300])
@pytest.mark.parametrize("max_len", [1, 7, 20])
def test_seq_gather(L, max_len, F):
    """The padded (max_len, B, F) batch: a sentence filling it (left = 0), one frame at the last
    time step, one in the middle; padded frames come back 0.0 and padded labels 0, from
    sentinel-filled outputs; ld_feats > F; nlab = 2 and nlab = 0 with NULL label pointers."""
    g = torch.Generator().manual_seed(max_len * 1000 + F)
    rows, ld = 64, F + 3
    feats = torch.randn(rows, ld, generator=g)
    labels = torch.randint(1, 1928, (rows, 2), generator=g, dtype=torch.int32)
    mid = max(1, max_len // 2)
    sents = [(3, max_len, 0), (40, 1, max_len - 1), (27, mid, (max_len - mid) // 2)]   # beg, len, left
    fd, ld_d = feats.to(DEV), labels.to(DEV)
    for ks in ([0], [1], [2], [0, 1, 2]):                  # B = 1 (each kind of sentence) and B = 3
        B = len(ks)
        beg, ln, left = (torch.tensor([sents[k][j] for k in ks], dtype=dt, device=DEV)
                         for j, dt in ((0, torch.int64), (1, torch.int32), (2, torch.int32)))
        wx = torch.zeros(max_len, B, F)
        wl = torch.zeros(max_len, B, 2, dtype=torch.int32)
        for col, k in enumerate(ks):
            b0, n, l0 = sents[k]
            wx[l0:l0 + n, col] = feats[b0:b0 + n, :F]
            wl[l0:l0 + n, col] = labels[b0:b0 + n]
        for nlab in (2, 0):
            x = Guarded(max_len * B * F)
            lab = Guarded(max_len * B * 2, dtype=torch.int32, fill=I32_SENT)
            L.call("pkc_seq_gather", L.ptr(fd), ld, F, L.ptr(ld_d) if nlab else None, nlab,
                   L.ptr(beg), L.ptr(ln), L.ptr(left), B, max_len, x.p, lab.p if nlab else None, _s())
            assert torch.equal(x.get().view(max_len, B, F), wx), (ks, nlab)
            if nlab:
                assert torch.equal(lab.get().view(max_len, B, 2), wl), ks
            else:
                lab.untouched()


# ------------------------------------------------------------------------------- pkc_cw_apply_rows

def _cw_ref(raw, Lc, Rc):
    """oracle.loader.context_window in float64, normalised by its own column mean / std."""
    from oracle.loader import context_window
    exp = context_window(raw, Lc, Rc)
    mean, std = np.mean(exp, axis=0), np.std(exp, axis=0)
    return (exp - mean) / std, mean, std


@pytest.mark.parametrize("perm", [False, True])
@pytest.mark.parametrize("row0", [0, 2])
def test_cw_apply_rows(L, row0, perm):
    """A row range of one stream's expansion, optionally permuted, written into columns
    [5, 5 + C) of a wider chunk matrix: the columns on either side and the rows around stay at
    the sentinel.  Tolerance of test_context_window_chunk_prep."""
    N, D, Lc, Rc = 50, 3, 2, 1
    rs = np.random.RandomState(row0 * 2 + perm)
    raw = (rs.randn(N, D) * 2 + rs.randn(1, D)).astype(np.float32)
    ref, mean, std = _cw_ref(raw, Lc, Rc)
    Nexp, Cw = N - Lc - Rc, D * (Lc + Rc + 1)
    nrows, W = Nexp - 3, Cw + 11
    order = rs.permutation(nrows) if perm else np.arange(nrows)
    rd = torch.from_numpy(raw).to(DEV)
    md, sd = torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV)
    pd = torch.from_numpy(order.astype(np.int64)).to(DEV) if perm else None
    chunk = torch.full((nrows + 2, W), 7.0, device=DEV)          # a guard row above and below
    out = C.c_void_p(chunk.data_ptr() + 4 * (W + 5))
    args = [L.ptr(rd), N, D, Lc, Rc, L.ptr(md), L.ptr(sd), L.ptr(pd)]
    L.call("pkc_cw_apply_rows", *args, row0, nrows, out, W, _s())
    torch.cuda.synchronize()
    got = chunk.cpu().numpy()
    np.testing.assert_allclose(got[1:-1, 5:5 + Cw], ref[row0 + order].astype(np.float32), rtol=1e-6,
                               atol=1e-6)
    assert (got[:, :5] == 7.0).all() and (got[:, 5 + Cw:] == 7.0).all()
    assert (got[0] == 7.0).all() and (got[-1] == 7.0).all()
    # one row past the end of the expansion is refused, and nothing is written
    chunk.fill_(7.0)
    _refused(L, "pkc_cw_apply_rows", *args, row0, Nexp - row0 + 1, out, W, _s())
    torch.cuda.synchronize()
    assert bool((chunk == 7.0).all())


def test_cw_apply_beyond_65535_rows(L):
    """pkc_cw_apply on 70 001 output rows (the row count is a grid dimension): every row against
    the reference, those beyond 65 535 included."""
    N, D, Lc, Rc = 70003, 1, 1, 1
    rs = np.random.RandomState(9)
    raw = (rs.randn(N, D) * 3 + 1.5).astype(np.float32)
    ref, mean, std = _cw_ref(raw, Lc, Rc)
    Nexp, Cw = N - Lc - Rc, 3
    out = Guarded(Nexp * Cw)
    rd, md, sd = (torch.from_numpy(a).to(DEV) for a in (raw, mean, std))
    L.call("pkc_cw_apply", L.ptr(rd), N, D, Lc, Rc, L.ptr(md), L.ptr(sd), None, out.p, Cw, _s())
    got = out.get().view(Nexp, Cw).numpy()
    np.testing.assert_allclose(got, ref.astype(np.float32), rtol=1e-6, atol=1e-6)

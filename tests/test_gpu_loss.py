"""pkc_nll_fused in each of its 18 kernel forms, pkc_nll_fused_multi in each of its 16 bodies and
pkc_loss_finalize with 1 to 8 heads, through the C ABI, against the float64 reference of
tests/loss_cases.py (itself checked against torch on the CPU by tests/test_loss_ref_cpu.py).

Every case asserts the form pkc_nll_form reports for the very pointers it passes.  Every output
(logp, dlogits, dlogits_bf16, row_loss, row_err, out, acc, the counter) sits between sentinel
guards (Guarded, as in tests/test_gpu_small_kernels.py): the guards must come back intact, no
sentinel may be left where the kernel must write, and an output that is not asked for stays
untouched.  The padding between slabs on a padded stride, and in front of an input passed one
element off its alignment, is NaN.

Bounds (loss_cases.bound, T_DLOGITS, T_MEAN): logp and row_loss within (nslab + 4) 2^-23
max(1, max |z|) of the reference; dlogits rtol 1e-4 atol 1e-7; the mean loss rtol 1e-5 atol 1e-6;
dlogits_bf16 the bits of the stored dlogits rounded by .bfloat16(); row_err exact; a second run
the same bits."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
G = 64                  # guard elements on either side (a multiple of 16 bytes for every dtype here)
I64_SENT = 0x7ffffffffffffff1
OUTS = ("logp", "dlogits", "bf16", "row_loss", "row_err")


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    from pkc import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return _lib


class Guarded:
    """A device buffer of n elements the kernel owns, G guard elements in front and behind (and
    `off` more in front, which move the owned part off its alignment), all of it filled with a
    sentinel (or the owned part with `init`)."""

    def __init__(self, n, dtype=torch.float32, fill=7.0, init=None, off=0):
        self.n, self.fill, self.lo = int(n), fill, G + int(off)
        assert self.n > 0
        self.buf = torch.full((self.lo + self.n + G,), fill, dtype=dtype, device=DEV)
        self.own = self.buf[self.lo:self.lo + self.n]
        if init is not None:
            self.own.copy_(init.reshape(-1))

    @property
    def ptr(self):
        return self.own.data_ptr()

    @property
    def p(self):
        return C.c_void_p(self.own.data_ptr())

    def get(self, written=True):
        """The owned region on the CPU; guards unchanged, and (written) no sentinel left in it."""
        torch.cuda.synchronize()
        b = self.buf.cpu()
        assert bool((b[:self.lo] == self.fill).all()), "the kernel wrote in front of its buffer"
        assert bool((b[self.lo + self.n:] == self.fill).all()), "the kernel wrote behind its buffer"
        own = b[self.lo:self.lo + self.n].clone()
        if written:
            left = int((own == self.fill).sum())
            assert left == 0, "%d of %d elements were never written" % (left, self.n)
        return own

    def untouched(self):
        assert bool((self.get(False) == self.fill).all()), "memory that was not to be written was"


def _refused(L, name, *args):
    """The entry point returns a status and names itself in pkc_last_error()."""
    rc = getattr(L.lib(), name)(*args)
    assert rc != 0, "%s accepted bad arguments" % name
    assert name in L.lib().pkc_last_error().decode()
    with pytest.raises(L.PkcError):
        L.call(name, *args)


def _dev(t, off=0):
    """A CPU vector on the device, `off` elements into a NaN-filled allocation."""
    buf = torch.full((off + t.numel(),), NAN, dtype=t.dtype)
    buf[off:] = t.reshape(-1)
    d = buf.to(DEV)
    return d[off:]


def _slabs(t, stride, off=0):
    """(S, M, N) CPU tensor -> flat device buffer, slab s at off + s * stride, NaN in the padding
    (in front, between the slabs and behind the last one)."""
    S, n = t.shape[0], t[0].numel()
    assert stride >= n or (S == 1 and stride == 0)
    buf = torch.full((off + (S - 1) * stride + n + 8,), NAN, dtype=t.dtype)
    for s in range(S):
        buf[off + s * stride:off + s * stride + n] = t[s].reshape(-1)
    d = buf.to(DEV)
    return d[off:]


def _setup(L, c):
    """Device inputs, guarded outputs and the argument struct of one case."""
    i = LC.inputs(c)
    M, N = c.M, c.N
    stride = LC.slab_stride(c)
    off = lambda k: 1 if c.off == k else 0
    z = _slabs(i.slabs, stride, off("zslab"))
    b = None if i.bias is None else _dev(i.bias, off("bias"))
    pr = None if i.prior is None else _dev(i.prior, off("log_prior"))
    lab = i.lab.to(DEV)
    o = NS(logp=Guarded(M * N, off=off("logp")), dlogits=Guarded(M * N, off=off("dlogits")),
           bf16=Guarded(M * N, dtype=torch.bfloat16, off=off("dlogits_bf16")),
           row_loss=Guarded(M), row_err=Guarded(M))
    labelled, train = c.mode != "fwd", c.mode == "train"
    a = L.NllArgs(M=M, N=N, nslab=c.S, zslab=z.data_ptr(), slab_stride=stride,
                  bias=None if b is None else b.data_ptr(),
                  labels=lab.data_ptr() + 4 * (c.lstride - 1) if labelled else None,
                  label_stride=c.lstride, weight=c.weight, logp=o.logp.ptr,
                  log_prior=None if pr is None else pr.data_ptr(),
                  dlogits=o.dlogits.ptr if train else None,
                  row_loss=o.row_loss.ptr if labelled and not c.no_loss else None,
                  row_err=o.row_err.ptr if labelled and not c.no_err else None,
                  dlogits_bf16=o.bf16.ptr if c.bf16 else None)
    want = dict(logp=True, dlogits=train, bf16=train and c.bf16,
                row_loss=labelled and not c.no_loss, row_err=labelled and not c.no_err)
    return NS(a=a, o=o, want=want, keep=(z, b, pr, lab), z=z, form=L.lib().pkc_nll_form(C.byref(a)))


def _collect(st):
    """The outputs on the CPU (None where none was asked for, and nothing was written there)."""
    got = {}
    for k in OUTS:
        buf = getattr(st.o, k)
        if st.want[k]:
            got[k] = buf.get()
        else:
            buf.untouched()
            got[k] = None
    assert bool(torch.isnan(st.z[-8:]).all().item())
    return got


def _run(L, c):
    st = _setup(L, c)
    assert st.form == c.form, "%s takes form %d, not %d" % (LC.case_id(c), st.form, c.form)
    L.call("pkc_nll_fused", C.byref(st.a), _s())
    return _collect(st)


def _same_bits(a, b, what):
    for k in OUTS:
        if a[k] is None:
            assert b[k] is None
            continue
        x, y = a[k].view(torch.int16 if k == "bf16" else torch.int32), b[k].view(
            torch.int16 if k == "bf16" else torch.int32)
        assert torch.equal(x, y), "%s: %s differs in %d elements" % (what, k, int((x != y).sum()))


def _check(c, got):
    """One call's outputs against the float64 reference; prints each figure before it asserts."""
    i, ref = LC.inputs(c), LC.reference(c)
    M, N = c.M, c.N
    b = LC.bound(c.S, ref.z)
    name = LC.case_id(c)
    for k in ("logp", "dlogits", "row_loss", "row_err"):
        if got[k] is not None:
            assert bool(torch.isfinite(got[k]).all()), "%s: inf or NaN in %s" % (name, k)
    e = np.abs(got["logp"].double().numpy().reshape(M, N) - ref.logp).max()
    print("%s: max|z| %.4g bound %.3g logp err %.3g" % (name, np.abs(ref.z).max(), b, e), end="")
    assert e <= b, "%s: logp off by %.3g > %.3g" % (name, e, b)
    if got["row_loss"] is not None:
        rl = got["row_loss"].double().numpy()
        e = np.abs(rl - ref.row_loss).max()
        print(" row_loss err %.3g" % e, end="")
        assert e <= b, "%s: row_loss off by %.3g > %.3g" % (name, e, b)
        torch.testing.assert_close(torch.tensor(rl.mean()), torch.tensor(ref.row_loss.mean()),
                                   **LC.T_MEAN)
    if got["row_err"] is not None:
        bad = np.flatnonzero(got["row_err"].numpy() != ref.row_err)
        assert bad.size == 0, "%s: row_err differs in rows %s" % (name, bad[:8].tolist())
    if got["dlogits"] is not None:
        d = got["dlogits"].view(M, N)
        e = (d.double() - torch.from_numpy(ref.dlogits)).abs().max().item()
        print(" dlogits err %.3g" % e, end="")
        torch.testing.assert_close(d.double(), torch.from_numpy(ref.dlogits), **LC.T_DLOGITS)
        if got["bf16"] is not None:
            x, y = got["bf16"].view(torch.int16), got["dlogits"].bfloat16().view(torch.int16)
            assert torch.equal(x, y), "%s: dlogits_bf16 is not dlogits rounded, in %d elements" % (
                name, int((x != y).sum()))
    print()


# ------------------------------------------------------------------------------- pkc_nll_fused

@pytest.mark.parametrize("c", LC.CASES, ids=[LC.case_id(c) for c in LC.CASES])
def test_nll_fused_form(L, c):
    """Each form at its smallest and edge shapes (loss_cases.CASES), run twice."""
    got = _run(L, c)
    _same_bits(got, _run(L, c), "second run")
    _check(c, got)
    i = LC.inputs(c)
    if c.kind == "tie":
        # the label on the lower / the higher of two tied maxima: error 0 / 1 (rows 2k, 2k + 1);
        # the last two rows are all-equal, with the label at column 0 / 3
        assert got["row_err"].tolist() == i.expect_err.tolist()
    if c.kind == "range":
        rl = got["row_loss"]
        assert bool(torch.isfinite(rl).all()) and bool((rl[[2, 3, 5]] > 170).all())
        assert bool((rl[[0, 1, 4]] == 0).all())        # the tail underflows: softmax is one-hot


@pytest.mark.parametrize("what", LC.OFFS)
@pytest.mark.parametrize("base", LC.ALIGNED, ids=["narrow", "wide"])
def test_nll_fused_scalar_twin(L, base, what):
    """One pointer one element off its alignment (or a slab stride off a multiple of 4) at
    N % 4 == 0: the scalar form of the same width and slab capacity, the same errors, everything
    else within the bound of the aligned run (the sum-exp order differs: not the same bits)."""
    c = LC.misaligned(base, what)
    assert base.form >= 8 and c.form == base.form - 8
    ga, gs = _run(L, base), _run(L, c)
    _same_bits(gs, _run(L, c), "second run")
    _check(base, ga)
    _check(c, gs)
    ref = LC.reference(base)
    b = LC.bound(base.S, ref.z)
    assert torch.equal(ga["row_err"], gs["row_err"])
    for k in ("logp", "row_loss"):
        assert (ga[k].double() - gs[k].double()).abs().max().item() <= b, k
    torch.testing.assert_close(gs["dlogits"].double(), ga["dlogits"].double(), **LC.T_DLOGITS)


def test_nll_fused_refusals(L):
    """M = 0, N = 0, nslab = 0, NULL zslab, NULL logp, dlogits without labels: a status, the entry
    named in pkc_last_error(), nothing written."""
    c = LC.case(5, 48, 2, 9, bias=True, bf16=True)
    st = _setup(L, c)
    assert st.form == 9
    good = {k: getattr(st.a, k) for k, _ in L.NllArgs._fields_}
    for bad in (dict(M=0), dict(N=0), dict(nslab=0), dict(zslab=None), dict(logp=None),
                dict(labels=None)):
        a = L.NllArgs(**dict(good, **bad))
        _refused(L, "pkc_nll_fused", C.byref(a), _s())
        for k in OUTS:
            getattr(st.o, k).untouched()
    L.call("pkc_nll_fused", C.byref(st.a), _s())            # the unmodified arguments are accepted
    _check(c, _collect(st))


def test_every_form_is_reached(L):
    """pkc_nll_form over the case table, on the pointers the cases pass: all of -2, -1 and 0..15
    for the single call, and every code 0..15 among the multi launches."""
    single = set()
    for c in LC.CASES:
        f = _setup(L, c).form
        assert f == c.form, LC.case_id(c)
        single.add(f)
    assert single == LC.ALL_FORMS, "forms never reached: %s" % sorted(LC.ALL_FORMS - single)
    multi = set()
    for launch in LC.MULTI:
        for h in launch:
            f = _setup(L, h).form
            assert f == h.form, LC.case_id(h)
            multi.add(f)
    assert multi == set(range(16)), "multi codes never reached: %s" % sorted(set(range(16)) - multi)
    a = L.NllArgs(M=0, N=4, nslab=1)
    assert L.lib().pkc_nll_form(C.byref(a)) == -3 and L.lib().pkc_nll_form(None) == -3


# -------------------------------------------------------------------------- pkc_nll_fused_multi

def _multi_vs_single(L, heads, in_one_launch):
    n = len(heads)
    single = [_setup(L, h) for h in heads]
    multi = [_setup(L, h) for h in heads]
    for h, s, m in zip(heads, single, multi):
        assert s.form == m.form == h.form, LC.case_id(h)
    assert all(h.form >= 0 for h in heads) == in_one_launch
    for s in single:
        L.call("pkc_nll_fused", C.byref(s.a), _s())
    args = (L.NllArgs * n)(*[m.a for m in multi])
    L.call("pkc_nll_fused_multi", args, n, _s())
    for k, (h, s, m) in enumerate(zip(heads, single, multi)):
        gs, gm = _collect(s), _collect(m)
        _same_bits(gs, gm, "head %d (%s)" % (k, LC.case_id(h)))
        _check(h, gm)


@pytest.mark.parametrize("k", range(len(LC.MULTI)))
def test_nll_fused_multi_equals_single_calls(L, k):
    """1 to 4 heads in one launch (narrow and wide, scalar and 16-byte, every slab capacity,
    unequal M): every head has the bits of its own pkc_nll_fused call."""
    _multi_vs_single(L, LC.MULTI[k], True)


def test_nll_fused_multi_falls_back_for_all_heads(L):
    """One head of 2052 columns: no head runs in the multi kernel, the results are the same."""
    _multi_vs_single(L, LC.MULTI_FALLBACK, False)


def test_nll_fused_multi_refuses_0_and_5_heads(L):
    sts = [_setup(L, LC.case(3, 48, 1, 8, seed=k)) for k in range(5)]
    args = (L.NllArgs * 5)(*[st.a for st in sts])
    for n in (0, 5):
        _refused(L, "pkc_nll_fused_multi", args, n, _s())
    for st in sts:
        for k in OUTS:
            getattr(st.o, k).untouched()


# ---------------------------------------------------------------------------- pkc_loss_finalize

def _finalize_inputs(nheads, M):
    g = torch.Generator().manual_seed(100 * nheads + M)
    rl = torch.rand(nheads, M, generator=g) * 5 + 0.1
    err = (torch.rand(M, generator=g) > 0.6).float()
    w = torch.tensor([0.3 + 0.2 * h for h in range(nheads)])
    means = rl.double().mean(1)
    want = torch.cat([torch.stack([(w.double() * means).sum(), err.double().mean()]), means])
    return rl, err, w, want


@pytest.mark.parametrize("M", [1, 7, 255, 256, 257, 1000])
@pytest.mark.parametrize("nheads", [1, 2, 3, 8])
def test_loss_finalize(L, nheads, M):
    """out = [sum_h w_h mean_h, mean err, mean_0 ..] in exactly 2 + nheads floats, against float64;
    acc and the counter left out, and accumulated over two calls; the OP_LOSS operation of
    pkc_gemm_grouped gives the same bits."""
    rl, err, w, want = _finalize_inputs(nheads, M)
    rld = [rl[h].clone().to(DEV) for h in range(nheads)]
    ptrs = torch.tensor([t.data_ptr() for t in rld], dtype=torch.int64, device=DEV)
    errd, wd = err.to(DEV), w.to(DEV)
    t = dict(rtol=1e-5, atol=1e-6)
    # acc and advance_ctr NULL
    out = Guarded(2 + nheads)
    L.call("pkc_loss_finalize", nheads, L.ptr(ptrs), L.ptr(wd), M, L.ptr(errd), out.p, None, None,
           _s())
    o1 = out.get()
    print("nheads %d M %d: max err %.3g" % (nheads, M, (o1.double() - want).abs().max().item()))
    torch.testing.assert_close(o1.double(), want, **t)
    # accumulated and counted over two calls
    acc = Guarded(2, init=torch.zeros(2))
    ctr = Guarded(1, dtype=torch.int64, fill=I64_SENT, init=torch.tensor([5]))
    for k in (1, 2):
        out2 = Guarded(2 + nheads)
        L.call("pkc_loss_finalize", nheads, L.ptr(ptrs), L.ptr(wd), M, L.ptr(errd), out2.p, acc.p,
               ctr.p, _s())
        assert torch.equal(out2.get().view(torch.int32), o1.view(torch.int32))
        assert torch.equal(acc.get(False), o1[:2] * k)          # 0 + x, then x + x: exact in fp32
        assert ctr.get(False).item() == 5 + k
    torch.testing.assert_close(acc.get(False).double(), 2 * want[:2], **t)
    # the same reduction as an operation of a grouped launch, beside a column sum
    out3, acc3 = Guarded(2 + nheads), Guarded(2, init=torch.zeros(2))
    ctr3 = Guarded(1, dtype=torch.int64, fill=I64_SENT, init=torch.tensor([5]))
    cs, ones = Guarded(3), torch.ones(2, 3, device=DEV)
    ops = (L.GemmProblem * 2)(
        L.GemmProblem(kind=L.OP_LOSS, M=nheads, N=M, A=ptrs.data_ptr(), B=wd.data_ptr(), C=out3.ptr,
                      X1=errd.data_ptr(), X2=acc3.ptr, X3=ctr3.ptr),
        L.GemmProblem(kind=L.OP_COLSUM, M=2, N=3, A=ones.data_ptr(), C=cs.ptr))
    L.call("pkc_gemm_grouped", 0, ops, 2, _s())
    assert torch.equal(out3.get().view(torch.int32), o1.view(torch.int32))
    assert torch.equal(acc3.get(False), o1[:2]) and ctr3.get(False).item() == 6
    assert cs.get().tolist() == [2.0, 2.0, 2.0]
    for h in range(nheads):
        assert torch.equal(rld[h].cpu(), rl[h]), "an input was written"


def test_loss_finalize_refuses_0_and_9_heads(L):
    rl, err, w, _ = _finalize_inputs(9, 7)
    rld = [rl[h].clone().to(DEV) for h in range(9)]
    ptrs = torch.tensor([t.data_ptr() for t in rld], dtype=torch.int64, device=DEV)
    errd, wd = err.to(DEV), w.to(DEV)
    out, acc = Guarded(11), Guarded(2)
    ctr = Guarded(1, dtype=torch.int64, fill=I64_SENT)
    for nheads in (0, 9):
        _refused(L, "pkc_loss_finalize", nheads, L.ptr(ptrs), L.ptr(wd), 7, L.ptr(errd), out.p, acc.p,
                 ctr.p, _s())
    for b in (out, acc, ctr):
        b.untouched()

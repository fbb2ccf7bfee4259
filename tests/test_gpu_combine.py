"""pkc_combine_fwd / pkc_combine_bwd through the C ABI against torch on the CPU doing the stated
fp32 arithmetic in the stated order: every comparison is torch.equal (bit-exact) — each output is
one rounded fp32 operation of its inputs (two for avg: the sum, then the exact halving), the slab
sum runs left to right, and the bf16 copy is the round-to-nearest-even of the fp32 result, which is
what .to(torch.bfloat16) does.

Shapes: one element; odd widths in one workgroup; (33, 64, 64), whose tight case takes the 16-byte
form; (130, 100, 28), more than one workgroup of the 16-byte form (N % 4 == 0) and, padded or
offset, of the scalar form.  Operand settings: tight, leading dimensions padded by 3 floats, and b
(a for the constant forms) as a column range that starts at column 1 of a wider matrix (the odd
feature column).  Every output has canary rows behind it.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
OPS = ["concatenate", "sum", "mult", "avg", "sum_constant", "mult_constant"]
SHAPES = [(1, 1, 1), (5, 7, 3), (33, 64, 64), (130, 100, 28)]
SETTINGS = ["tight", "padded", "offset"]
CONST = 0.3
NAN = float("nan")


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    from pkc import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return _lib


def _binary(op):
    return op in ("concatenate", "sum", "mult", "avg")


def _operands(op, M, Na, Nb, setting, seed):
    """Host buffers and (column offset, ld) of a and b; b is None for the constant forms."""
    g = torch.Generator().manual_seed(seed)
    if not _binary(op):
        Nb = 0
    elif op != "concatenate":
        Nb = Na
    pad = 3 if setting == "padded" else 0
    a_off, b_off = 0, 0
    lda, ldb = Na + pad, Nb + pad
    if setting == "offset":
        if _binary(op):
            b_off, ldb = 1, Nb + 5
        else:
            a_off, lda = 1, Na + 5
    abuf = torch.randn(M, lda, generator=g)
    bbuf = torch.randn(M, max(1, ldb), generator=g) if _binary(op) else None
    return dict(M=M, Na=Na, Nb=Nb, N=Na + Nb if op == "concatenate" else Na, abuf=abuf, bbuf=bbuf,
                a_off=a_off, b_off=b_off, lda=lda, ldb=ldb,
                a=abuf[:, a_off:a_off + Na].contiguous(),
                b=bbuf[:, b_off:b_off + Nb].contiguous() if bbuf is not None else None)


def _fwd_ref(op, a, b):
    c = torch.tensor(CONST, dtype=torch.float32)
    if op == "concatenate":
        return torch.cat((a, b), 1)
    if op == "sum":
        return a + b
    if op == "mult":
        return a * b
    if op == "avg":
        return (a + b) * torch.tensor(0.5, dtype=torch.float32)
    if op == "sum_constant":
        return a + c
    return a * c


def _bwd_ref(op, a, b, slabs, Na):
    g = slabs[0].clone()
    for s in slabs[1:]:
        g = g + s
    c = torch.tensor(CONST, dtype=torch.float32)
    if op == "concatenate":
        return g[:, :Na].contiguous(), g[:, Na:].contiguous()
    if op == "sum":
        return g, g
    if op == "avg":
        h = g * torch.tensor(0.5, dtype=torch.float32)
        return h, h
    if op == "mult":
        return g * b, g * a
    if op == "sum_constant":
        return g, None
    return g * c, None


def _args(L, op, o, dev):
    return L.CombineArgs(
        op=L.COMBINE[op], M=o["M"], Na=o["Na"], Nb=o["Nb"],
        a=dev["a"].data_ptr() + 4 * o["a_off"], lda=o["lda"],
        b=(dev["b"].data_ptr() + 4 * o["b_off"]) if dev["b"] is not None else None, ldb=o["ldb"],
        c=CONST)


def _dev(o):
    return dict(a=o["abuf"].to(DEV), b=o["bbuf"].to(DEV) if o["bbuf"] is not None else None)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("M,Na,Nb", SHAPES)
@pytest.mark.parametrize("op", OPS)
def test_combine_fwd(L, op, M, Na, Nb, setting):
    o = _operands(op, M, Na, Nb, setting, seed=M * 1000 + Na)
    N, dev = o["N"], _dev(o)
    ref = _fwd_ref(op, o["a"], o["b"])
    assert ref.dtype == torch.float32 and ref.shape == (M, N)
    for with_h in (True, False):
        out = torch.full((M + 2, N), NAN, device=DEV)
        out_h = torch.full((M + 2, N), NAN, device=DEV, dtype=torch.bfloat16)
        a = _args(L, op, o, dev)
        a.out = out.data_ptr()
        a.out_bf16 = out_h.data_ptr() if with_h else None
        assert L.lib().pkc_combine_ok(C.byref(a), 0) == 1, L.lib().pkc_last_error()
        L.call("pkc_combine_fwd", C.byref(a), _s())
        torch.cuda.synchronize()
        assert torch.equal(out[:M].cpu(), ref)
        assert torch.isnan(out[M:]).all(), "out written past row M"
        if with_h:
            assert torch.equal(out_h[:M].cpu(), ref.to(torch.bfloat16))
            assert torch.isnan(out_h[M:]).all(), "out_bf16 written past row M"
        else:
            assert torch.isnan(out_h).all(), "out_bf16 == NULL still wrote a copy"
    # the inputs are untouched
    assert torch.equal(dev["a"].cpu(), o["abuf"])


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("M,Na,Nb", SHAPES)
@pytest.mark.parametrize("op", OPS)
def test_combine_bwd(L, op, M, Na, Nb, setting):
    o = _operands(op, M, Na, Nb, setting, seed=M * 1000 + Na + 7)
    N, Nb, dev = o["N"], o["Nb"], _dev(o)
    gen = torch.Generator().manual_seed(M + N)
    for nslab in (1, 3):
        # slab_stride > M * N; a multiple of 4 floats where M * N is one (the 16-byte form)
        stride = M * N + (8 if (M * N) % 4 == 0 else 5)
        gbuf = torch.randn(nslab, stride, generator=gen)
        slabs = [gbuf[s, :M * N].view(M, N) for s in range(nslab)]
        gd = gbuf.to(DEV)
        ra, rb = _bwd_ref(op, o["a"], o["b"], slabs, Na)
        for which in (("both", "a", "b") if _binary(op) else ("a",)):
            runs = []
            for _ in range(2):                  # twice: identical bits
                da = torch.full((M + 2, Na), NAN, device=DEV)
                db = torch.full((M + 2, max(1, Nb)), NAN, device=DEV)
                a = _args(L, op, o, dev)
                a.nslab, a.gslab, a.slab_stride = nslab, gd.data_ptr(), stride
                a.da = da.data_ptr() if which in ("both", "a") else None
                a.db = db.data_ptr() if which in ("both", "b") else None
                assert L.lib().pkc_combine_ok(C.byref(a), 1) == 1, L.lib().pkc_last_error()
                L.call("pkc_combine_bwd", C.byref(a), _s())
                torch.cuda.synchronize()
                runs.append((da.cpu(), db.cpu()))
            da, db = runs[0]
            if which in ("both", "a"):
                assert torch.equal(da[:M], ra), (nslab, which)
                assert torch.isnan(da[M:]).all(), "da written past row M"
            else:
                assert torch.isnan(da).all(), "da == NULL still wrote a gradient"
            if which in ("both", "b"):
                assert torch.equal(db[:M], rb), (nslab, which)
                assert torch.isnan(db[M:]).all(), "db written past row M"
            else:
                assert torch.isnan(db).all(), "db == NULL still wrote a gradient"
            for x, y in zip(runs[0], runs[1]):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "rerun differs"
        assert torch.equal(gd.cpu(), gbuf), "the gradient slabs were written"


def test_combine_refused_arguments(L):
    """Every ABI refusal: pkc_combine_ok says 0, the entry point returns a status and names itself
    in pkc_last_error(), and nothing is written."""
    M, N = 4, 8
    lib = L.lib()
    a_t = torch.ones(M, N, device=DEV)
    b_t = torch.ones(M, N, device=DEV)
    g_t = torch.ones(3, M * N, device=DEV)

    def fresh():
        return [torch.full((M + 2, 2 * N), NAN, device=DEV) for _ in range(3)]

    def base(name, **kw):
        d = dict(op=L.COMBINE[name], M=M, Na=N, Nb=N, a=a_t.data_ptr(), lda=N, b=b_t.data_ptr(),
                 ldb=N, c=1.0, nslab=1, gslab=g_t.data_ptr(), slab_stride=M * N)
        d.update(kw)
        return d

    fwd_bad = [base("sum", Nb=N - 1), base("mult", Nb=N + 1), base("avg", Na=N - 4),
               base("sum", M=0), base("sum", M=-2), base("sum", Na=0, Nb=0),
               base("concatenate", Nb=0), base("concatenate", Na=-1), base("mult_constant", Na=0),
               base("sum", lda=N - 1), base("sum", ldb=N - 1), base("sum", a=None),
               base("sum", b=None), base("sum", op=6), base("sum", op=-1), base("sum", out=None)]
    bwd_bad = [base("sum", nslab=0), base("sum", nslab=-1), base("sum", da=None, db=None),
               base("mult_constant", da=None, db=None), base("sum_constant", da=None, db=None),
               base("sum_constant"),          # a constant operand takes no db
              
               base("mult", Nb=N - 1), base("concatenate", M=0), base("sum", gslab=None),
               base("sum", nslab=3, slab_stride=M * N - 1), base("mult", b=None),
               base("mult", lda=N - 1)]
    for bwd, cases in ((0, fwd_bad), (1, bwd_bad)):
        fn = lib.pkc_combine_bwd if bwd else lib.pkc_combine_fwd
        name = "pkc_combine_bwd" if bwd else "pkc_combine_fwd"
        for kw in cases:
            out, da, db = fresh()
            d = dict(out=out.data_ptr(), out_bf16=None, da=da.data_ptr(), db=db.data_ptr())
            d.update(kw)
            a = L.CombineArgs(**d)
            assert lib.pkc_combine_ok(C.byref(a), bwd) == 0, "pkc_combine_ok accepted %s" % kw
            rc = fn(C.byref(a), _s())
            assert rc != 0, "%s accepted %s" % (name, kw)
            assert name in lib.pkc_last_error().decode(), kw
            with pytest.raises(L.PkcError):
                L.call(name, C.byref(a), _s())
            torch.cuda.synchronize()
            for t in (out, da, db):
                assert torch.isnan(t).all(), "refused call wrote memory: %s" % kw
    # the same arguments without the fault are taken
    out, da, db = fresh()
    a = L.CombineArgs(out=out.data_ptr(), da=da.data_ptr(), db=db.data_ptr(), **base("sum"))
    assert lib.pkc_combine_ok(C.byref(a), 0) == 1 and lib.pkc_combine_ok(C.byref(a), 1) == 1
    L.call("pkc_combine_fwd", C.byref(a), _s())
    L.call("pkc_combine_bwd", C.byref(a), _s())
    torch.cuda.synchronize()
    assert (out.view(-1)[:M * N] == 2).all() and (da.view(-1)[:M * N] == 1).all()

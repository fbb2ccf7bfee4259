"""The dense epilogue (pkc_dense.hip) mode by mode and form by form, through the C ABI, against
float64 references computed on the CPU from the same fp32 inputs.

pkc_dense_fwd / pkc_dense_bwd run in three forms, chosen by shape and pointer alignment:
  small : M <= 128, N % 4 == 0, at most 8 slabs, every pointer aligned — one launch; template
          variants RI (rows per thread), G (column groups) and XM (column mapping);
  v4    : 16-byte accesses, aligned pointers, at least 1024 workgroups on the 256-column grid;
  scalar: everything else.
_form() restates those conditions and every call asserts the form it is meant to take, so a shape
list that stops reaching a form fails.  A small or v4 shape is forced into the scalar form by
passing `out` (forward) or `dz` (backward) one float into a larger allocation.

Every output lives inside a NaN-filled (masks: 0xAA) allocation one row longer than needed; what
lies around the M x N (or N) elements must still hold the sentinel after each call.

Tolerances are test_dense_bn_fwd_bwd's (tests/test_gpu_kernels.py): out / xhat rtol 1e-4 atol 1e-5,
running statistics rtol 1e-4 atol 1e-6, dz rtol 1e-3 atol 1e-5, parameter gradients rtol 1e-4
atol 1e-4.  "Same bits" means assert_array_equal on the raw words.
"""
import ctypes as C
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
ACTS = ["linear", "relu", "tanh", "sigmoid", "htanh", "leaky_relu", "elu"]
V4_MIN_WG = 1024
T_OUT = dict(rtol=1e-4, atol=1e-5)
T_RUN = dict(rtol=1e-4, atol=1e-6)
T_DZ = dict(rtol=1e-3, atol=1e-5)
T_PAR = dict(rtol=1e-4, atol=1e-4)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    from pkc import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return _lib


# ------------------------------------------------------------------ which form a call takes
def _form(M, N, nslab, stride, p16=(), p8=(), p4=(), small=True):
    """The form pkc_dense.hip's entry points choose (small_ok + its call sites, v4_fwd / v4_bwd,
    V4_MIN_WG).  p16 / p8 / p4: addresses that must be 16 / 8 / 4-byte aligned (None = NULL,
    aligned).  small=False: the SyncBN entry points, which never take the small form."""
    ok = N % 4 == 0 and (nslab == 1 or stride % 4 == 0)
    for ptrs, al in ((p16, 16), (p8, 8), (p4, 4)):
        ok = ok and all(x is None or x % al == 0 for x in ptrs)
    if small and ok and M <= 128 and nslab <= 8:
        return "small"
    if ok and ((N + 255) // 256) * ((M + 15) // 16) >= V4_MIN_WG:
        return "v4"
    return "scalar"


def _variant(M, N):
    """(RI, G, XM) of the small form (PKC_SMALL_LAUNCH*)."""
    G = 2 if N >= 512 else 4
    return (1 if M <= 256 // G else 2, G, 2 if N % 512 == 0 else 1)


def test_shape_table_reaches_every_form_and_variant():
    got = {(M, N): _variant(M, N) for M, N in [(16, 48), (7, 12), (100, 64), (128, 520), (128, 1024)]}
    assert got == {(16, 48): (1, 4, 1), (7, 12): (1, 4, 1), (100, 64): (2, 4, 1),
                   (128, 520): (1, 2, 1), (128, 1024): (1, 2, 2)}
    assert _form(128, 1024, 8, 128 * 1024) == "small" and _form(100, 64, 9, 6400) == "scalar"
    assert _form(50, 70, 1, 0) == "scalar" and _form(129, 40, 1, 0) == "scalar"
    assert _form(1024, 4096, 1, 0) == "v4" and _form(1030, 4096, 9, 1030 * 4096) == "v4"
    assert _form(1008, 4096, 1, 0) == "scalar"                  # 63 x 16 workgroups: below V4_MIN_WG
    assert _form(1024, 4096, 1, 0, p16=[4]) == "scalar" and _form(100, 64, 1, 0, p4=[1]) == "scalar"
    assert _form(1024, 4096, 1, 0, small=False) == "v4" and _form(17, 4096, 1, 0, small=False) == "scalar"


# ------------------------------------------------------------------ guarded device buffers
class _G:
    """n elements inside a sentinel-filled allocation: `off` elements in front, `pad` behind."""

    def __init__(self, n, pad, dtype=torch.float32, off=0, src=None):
        self.sent = 0xAA if dtype == torch.uint8 else float("nan")
        self.full = torch.full((off + n + pad,), self.sent, dtype=dtype, device=DEV)
        self.t = self.full[off:off + n]
        self.off, self.n = off, n
        if src is not None:
            self.t.copy_(src.reshape(-1))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def cpu(self, *shape):
        return self.t.cpu().view(*shape) if shape else self.t.cpu()

    def guard_ok(self):
        g = torch.cat([self.full[:self.off], self.full[self.off + self.n:]])
        return bool(torch.isnan(g).all()) if g.dtype != torch.uint8 else bool((g == 0xAA).all())

    def untouched(self):
        f = self.full
        return bool(torch.isnan(f).all()) if f.dtype != torch.uint8 else bool((f == 0xAA).all())


def _check_guards(o):
    for k, v in vars(o).items():
        if isinstance(v, _G):
            assert v.guard_ok(), "%s: written outside its M x N / N elements" % k


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy()
    return t.numpy()


def _same_bits(a, b, what=""):
    np.testing.assert_array_equal(_bits(a).ravel(), _bits(b).ravel(), err_msg=what)


def _rne(t):
    """bf16 round-to-nearest-even of an fp32 tensor (torch's CPU conversion)."""
    return t.detach().cpu().float().to(torch.bfloat16)


def _p(x):
    return None if x is None else (x.ptr if isinstance(x, _G) else x.data_ptr())


# ------------------------------------------------------------------ float64 references
def _act(act, y):
    return {"linear": lambda t: t, "relu": lambda t: t.clamp_min(0), "tanh": torch.tanh,
            "sigmoid": torch.sigmoid, "htanh": lambda t: t.clamp(-1, 1),
            "leaky_relu": lambda t: torch.where(t > 0, t, 0.2 * t),
            "elu": lambda t: torch.where(t > 0, t, torch.expm1(t))}[act](y)


def _dact(act, y):
    one = torch.ones_like(y)
    return {"linear": lambda t: one, "relu": lambda t: (t > 0).double(),
            "tanh": lambda t: 1 - torch.tanh(t) ** 2,
            "sigmoid": lambda t: torch.sigmoid(t) * (1 - torch.sigmoid(t)),
            "htanh": lambda t: ((t > -1) & (t < 1)).double(),
            "leaky_relu": lambda t: torch.where(t > 0, one, 0.2 * one),
            "elu": lambda t: torch.where(t > 0, one, torch.exp(t))}[act](y)


def _ref_fwd(z, norm, act, gamma=None, beta=None, rm=None, rv=None, keep=None, p=0.0):
    """z: float64 [M, N] (slab sum + bias).  norm: 'none' | 'train' | 'eval'."""
    r = NS(mean=None, var=None)
    if norm == "none":
        r.xh = r.y = z
    else:
        if norm == "train":
            r.mean, r.var = z.mean(0), z.var(0, unbiased=False)
        else:
            r.mean, r.var = rm.double(), rv.double()
        r.xh = (z - r.mean) / (r.var + EPS).sqrt()
        r.y = r.xh * gamma.double() + beta.double()
    r.out = _act(act, r.y)
    if p > 0:
        r.out = r.out * keep.double() / (1 - p)
    return r


def _ref_bwd(g, r, norm, act, gamma=None, keep=None, p=0.0):
    """g: float64 dL/d out; r: the forward reference (or NS(xh=, y=, var=))."""
    if p > 0:
        g = g * keep.double() / (1 - p)
    dy = g * _dact(act, r.y)
    if norm == "none":
        return NS(dz=dy, dbias=dy.sum(0))
    k = gamma.double() / (r.var + EPS).sqrt()
    return NS(dz=k * (dy - dy.mean(0) - r.xh * (dy * r.xh).mean(0)), dgamma=(dy * r.xh).sum(0),
              dbeta=dy.sum(0))


def _kink_free_cols(act, y):
    """A pre-activation within rounding of ReLU's kink may take the other branch on the GPU, and
    through the BatchNorm mean terms that moves its whole column: the backward is compared on the
    columns whose reference |y| > 1e-5 in every row (as test_dense_bn_fwd_bwd does).  At least 95 %
    of the columns must remain: y's density at 0 is at most 0.8 for gamma >= 0.5, so 1241 rows
    leave out under 2 %."""
    cols = (y.abs() > 1e-5).all(0) if act == "relu" else torch.ones(y.shape[1], dtype=torch.bool)
    assert cols.double().mean() >= 0.95, "ReLU kink filter keeps %.3f of the columns" % cols.double().mean()
    return cols


def _close(got, ref, tol, what=""):
    torch.testing.assert_close(got.double(), ref.double(), msg=lambda m: "%s: %s" % (what, m), **tol)


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=3)
def _data(M, N, S, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 4099 * M + 17 * N + S)
    d = NS(M=M, N=N, S=S)
    d.slabs = torch.randn(S, M, N, generator=g)
    d.gout = torch.randn(S, M, N, generator=g)
    d.bias = torch.randn(N, generator=g) * 0.1
    d.gamma = torch.rand(N, generator=g) + 0.5
    d.beta = torch.randn(N, generator=g) * 0.1
    d.rm = torch.randn(N, generator=g) * 0.3
    d.rv = torch.rand(N, generator=g) + 0.5
    d.keep = (torch.rand(M, N, generator=g) > 0.15).to(torch.uint8)
    d.z = d.slabs.double().sum(0) + d.bias.double()
    d.g = d.gout.double().sum(0)
    return d


def _dev(d, names=("slabs", "gout", "bias", "gamma", "beta", "rm", "rv", "keep")):
    return NS(**{k: getattr(d, k).to(DEV) for k in names})


NORMS = {"none": 0, "train": 1, "eval": 2}


def _fwd(L, d, M, N, norm, act, *, expect, small=True, bias=True, p=0.0, keep_in=None, keep_out=False,
         xhat=True, out=True, bf16=False, count_n=0, momentum=0.05, seed=1, step_ctr=None,
         stream_id=0, off_out=0, off_kin=0, off_kout=0):
    """Argument block + guarded outputs of one forward call on the device inputs d (slabs [S, M, N],
    bias, gamma, beta, rm, rv); asserts the form the call will take."""
    S = d.slabs.shape[0]
    o = NS()
    o.out = _G(M * N, N, off=off_out) if out else None
    o.xhat = _G(M * N, N) if xhat else None
    o.h = _G(M * N, N, dtype=torch.bfloat16) if bf16 else None
    o.kin = _G(M * N, N, dtype=torch.uint8, off=off_kin, src=keep_in.to(DEV)) if keep_in is not None else None
    o.kout = _G(M * N, N, dtype=torch.uint8, off=off_kout) if keep_out else None
    bn = norm != "none"
    o.rm = _G(N, 4, src=d.rm) if bn else None
    o.rv = _G(N, 4, src=d.rv) if bn else None
    o.sm = _G(N, 4) if bn else None
    o.si = _G(N, 4) if bn else None
    o.work = _G(L.lib().pkc_dense_work_size(M, N), 64) if norm == "train" else None
    b = d.bias if bias else None
    stride = M * N
    p16 = [_p(t) for t in (d.slabs, o.out, o.xhat, b)] + ([_p(t) for t in (d.gamma, d.beta, o.rm, o.rv, o.sm, o.si)] if bn else [])
    form = _form(M, N, S, stride, p16, [_p(o.h)], [_p(o.kin), _p(o.kout)], small=small)
    assert form == expect, "this case is meant to take the %s form, its shape / pointers give %s" % (expect, form)
    o.args = L.DenseFwdArgs(M=M, N=N, nslab=S, zslab=_p(d.slabs), slab_stride=stride, bias=_p(b),
                            norm=NORMS[norm], gamma=_p(d.gamma) if bn else None,
                            beta=_p(d.beta) if bn else None, running_mean=_p(o.rm),
                            running_var=_p(o.rv), momentum=momentum, eps=EPS, save_mean=_p(o.sm),
                            save_invstd=_p(o.si), act=L.ACT[act], drop_p=p, seed=seed,
                            step_ctr=_p(step_ctr), stream_id=stream_id, keep_in=_p(o.kin),
                            keep_out=_p(o.kout), xhat=_p(o.xhat), out=_p(o.out), count_n=count_n,
                            out_bf16=_p(o.h))
    return o


def _run_fwd(L, d, M, N, norm, act, **kw):
    o = _fwd(L, d, M, N, norm, act, **kw)
    L.call("pkc_dense_fwd", C.byref(o.args), _p(o.work), _s())
    return o


def _bwd(L, d, M, N, norm, act, *, expect, xhat, si=None, small=True, p=0.0, keep=None, bf16=False,
         scratch=0, off_dz=0, off_keep=0, pgrads=True):
    """Argument block + guarded outputs of one backward call; xhat / si / keep: device tensors."""
    S = d.gout.shape[0]
    bn = norm == "train"
    o = NS()
    o.dz = _G(M * N, N, off=off_dz)
    o.h = _G(M * N, N, dtype=torch.bfloat16) if bf16 else None
    o.keep = _G(M * N, N, dtype=torch.uint8, off=off_keep, src=keep) if keep is not None else None
    o.dgamma = _G(N, 4) if bn and pgrads else None
    o.dbeta = _G(N, 4) if bn and pgrads else None
    o.dbias = _G(N, 4)
    o.work = _G(L.lib().pkc_dense_work_size(M, N), 64)
    stride = M * N
    p16 = [_p(t) for t in (d.gout, xhat, o.dz, o.dbias)] + ([_p(t) for t in (d.gamma, d.beta, si, o.dgamma, o.dbeta)] if bn else [])
    form = _form(M, N, S, stride, p16, [_p(o.h)], [_p(o.keep)], small=small)
    assert form == expect, "this case is meant to take the %s form, its shape / pointers give %s" % (expect, form)
    o.args = L.DenseBwdArgs(M=M, N=N, nslab=S, gslab=_p(d.gout), slab_stride=stride, norm=NORMS[norm],
                            act=L.ACT[act], gamma=_p(d.gamma) if bn else None,
                            beta=_p(d.beta) if bn else None, save_invstd=_p(si) if bn else None,
                            xhat=_p(xhat), keep=_p(o.keep), drop_p=p, dz=_p(o.dz), dgamma=_p(o.dgamma),
                            dbeta=_p(o.dbeta), dbias=_p(o.dbias), dz_bf16=_p(o.h), dz_scratch=scratch)
    return o


def _run_bwd(L, d, M, N, norm, act, **kw):
    o = _bwd(L, d, M, N, norm, act, **kw)
    L.call("pkc_dense_bwd", C.byref(o.args), _p(o.work), _s())
    return o


# (M, N, slabs, forced into the scalar form, form)
SMALL = [(16, 48, 1, 0, "small"), (7, 12, 2, 0, "small"), (100, 64, 3, 0, "small"),
         (128, 520, 5, 0, "small"), (128, 1024, 8, 0, "small")]
SCALAR = [(50, 70, 3, 0, "scalar"), (129, 40, 9, 0, "scalar"), (300, 64, 2, 0, "scalar"),
          (100, 64, 9, 0, "scalar"), (128, 1024, 2, 1, "scalar")]
V4 = [(1024, 4096, 1, 0, "v4"), (1030, 4096, 2, 0, "v4"), (1024, 4096, 1, 1, "scalar")]


# ------------------------------------------------------------------ 1. eval BatchNorm
@pytest.mark.parametrize("p", [0.0, 0.15])
@pytest.mark.parametrize("M,N,S,force,form", SMALL + SCALAR + V4)
def test_eval_bn(L, M, N, S, force, form, p):
    """out = drop(act((z - running_mean) / sqrt(running_var + eps) * gamma + beta)) for every
    activation; running statistics and save_* untouched bit for bit; xhat NULL accepted."""
    dat = _data(M, N, S)
    d = _dev(dat)
    keep = dat.keep if p > 0 else None
    # every activation in every form: at the 4M-element shapes once per form (the dropout cases),
    # three of them in the other cases, to keep each case to a few seconds
    acts = ACTS if M * N < (1 << 20) or (p > 0 and M == 1024) else ["relu", "tanh", "elu"]
    for i, act in enumerate(acts):
        r = _ref_fwd(dat.z, "eval", act, dat.gamma, dat.beta, dat.rm, dat.rv, keep, p)
        o = _run_fwd(L, d, M, N, "eval", act, expect=form, p=p, keep_in=keep, off_out=force)
        _close(o.out.cpu(M, N), r.out, T_OUT, "out " + act)
        if i == 0:                              # xhat does not depend on the activation
            _close(o.xhat.cpu(M, N), r.xh, T_OUT, "xhat")
        else:
            _same_bits(o.xhat.t, xhat0, "xhat " + act)
        xhat0 = o.xhat.t
        if p > 0:
            assert (o.out.cpu(M, N)[dat.keep == 0] == 0).all()
        _same_bits(o.rm.t, dat.rm, "running_mean written in eval mode")
        _same_bits(o.rv.t, dat.rv, "running_var written in eval mode")
        assert o.sm.untouched() and o.si.untouched(), "save_* written in eval mode"
        _check_guards(o)
        if i < 2:
            o2 = _run_fwd(L, d, M, N, "eval", act, expect=form, p=p, keep_in=keep, off_out=force,
                          xhat=False)
            _same_bits(o2.out.t, o.out.t, "out with xhat == NULL")
            _check_guards(o2)


# ------------------------------------------------------------------ 2. no norm
@pytest.mark.parametrize("p", [0.0, 0.15])
@pytest.mark.parametrize("M,N,S,force,form", SMALL + SCALAR + [(1024, 4096, 1, 0, "v4"),
                                                               (1030, 4096, 5, 0, "v4")])
def test_no_norm_fwd_bwd(L, M, N, S, force, form, p):
    """forward act(z + bias) with dropout from keep_in; backward dz = g keep / (1 - p) act'(y),
    dbias = colsum(dz), no dgamma / dbeta, dz_bf16 written by the stats pass.  The backward's y is
    its own input (xhat), so the reference takes act' at the same fp32 value: no kink ambiguity."""
    dat = _data(M, N, S)
    d = _dev(dat)
    keep = dat.keep if p > 0 else None
    for act in (ACTS if M * N < (1 << 20) else ["relu", "tanh", "elu"]):
        r = _ref_fwd(dat.z, "none", act, keep=keep, p=p)
        o = _run_fwd(L, d, M, N, "none", act, expect=form, p=p, keep_in=keep, off_out=force)
        _close(o.out.cpu(M, N), r.out, T_OUT, "out " + act)
        _close(o.xhat.cpu(M, N), r.xh, T_OUT, "xhat " + act)
        _check_guards(o)
        y = o.xhat.cpu(M, N).double()
        rb = _ref_bwd(dat.g, NS(y=y), "none", act, keep=keep, p=p)
        b = _run_bwd(L, d, M, N, "none", act, expect=form, xhat=o.xhat, p=p,
                     keep=d.keep if p > 0 else None, bf16=True, off_dz=force)
        _close(b.dz.cpu(M, N), rb.dz, T_DZ, "dz " + act)
        _close(b.dbias.cpu(), rb.dbias, T_PAR, "dbias " + act)
        _same_bits(b.h.t, _rne(b.dz.t), "dz_bf16 " + act)
        _check_guards(b)


# ------------------------------------------------------------------ 3. bf16 copies
def _ties(shape, g):
    """fp32 values exactly half-way between two bf16 neighbours, upper mantissa bit even and odd."""
    x = torch.randn(*shape, generator=g)
    b = (x.view(torch.int32) & ~0xFFFF) | 0x8000
    return b.view(torch.float32)


@pytest.mark.parametrize("mode", ["bn", "ties"])
@pytest.mark.parametrize("M,N,S,form", [(100, 64, 2, "small"), (128, 1024, 4, "small"),
                                        (50, 70, 3, "scalar"), (300, 64, 1, "scalar"),
                                        (1030, 4096, 2, "v4")])
def test_bf16_copies(L, M, N, S, form, mode):
    """out_bf16 / dz_bf16 are the round-to-nearest-even bf16 of the same call's fp32 out / dz; the
    same bits with out == NULL and with dz_scratch = 1.  'bn': training BatchNorm, gamma 1, beta 0,
    linear; 'ties': no norm, no bias, linear, every value on a rounding tie."""
    dat = _data(M, N, S, seed=3)
    d = _dev(dat)
    if mode == "bn":
        norm = "train"
        d.gamma, d.beta = torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    else:
        norm = "none"
        g = torch.Generator().manual_seed(M + N)
        z, gg = torch.zeros(S, M, N), torch.zeros(S, M, N)
        z[0], gg[0] = _ties((M, N), g), _ties((M, N), g)
        lo = _bits(z[0]) & 0x1FFFF
        assert (lo == 0x18000).any() and (lo == 0x08000).any()
        d.slabs, d.gout = z.to(DEV), gg.to(DEV)
    o = _run_fwd(L, d, M, N, norm, "linear", expect=form, bias=mode == "bn", bf16=True)
    if mode == "ties":
        _same_bits(o.out.t, z[0], "linear, no norm: out is the input")
    _same_bits(o.h.t, _rne(o.out.t), "out_bf16 is not the RNE of out")
    o2 = _run_fwd(L, d, M, N, norm, "linear", expect=form, bias=mode == "bn", bf16=True, out=False)
    _same_bits(o2.h.t, o.h.t, "out_bf16 with out == NULL")
    _check_guards(o)
    _check_guards(o2)
    b = _run_bwd(L, d, M, N, norm, "linear", expect=form, xhat=o.xhat, si=o.si, bf16=True)
    if mode == "ties":
        _same_bits(b.dz.t, gg[0], "linear, no norm: dz is the input")
    _same_bits(b.h.t, _rne(b.dz.t), "dz_bf16 is not the RNE of dz")
    _check_guards(b)
    if mode == "bn":
        b2 = _run_bwd(L, d, M, N, norm, "linear", expect=form, xhat=o.xhat, si=o.si, bf16=True,
                      scratch=1)
        _same_bits(b2.h.t, b.h.t, "dz_bf16 with dz_scratch = 1")
        _check_guards(b2)


def test_dz_scratch_argument_errors(L):
    M, N = 16, 48
    d = _dev(_data(M, N, 1))
    xhat = torch.randn(M, N, device=DEV)
    si = torch.ones(N, device=DEV)
    for norm, bf16 in (("train", False), ("none", True)):
        b = _bwd(L, d, M, N, norm, "relu", expect="small", xhat=xhat, si=si, bf16=bf16, scratch=1)
        st = L.lib().pkc_dense_bwd(C.byref(b.args), _p(b.work), _s())
        assert st == L.PKC_ERR_ARG
        assert b"dz_scratch" in L.lib().pkc_last_error()
        torch.cuda.synchronize()
        assert b.dz.untouched() and b.dbias.untouched() and (b.h is None or b.h.untouched())


# ------------------------------------------------------------------ 4. count_n
@pytest.mark.parametrize("cn_mult", [0, 1, 2])
@pytest.mark.parametrize("M,N,S,force,form", [(16, 48, 1, 0, "small"), (128, 1024, 2, 0, "small"),
                                              (50, 70, 3, 0, "scalar"), (129, 40, 1, 0, "scalar"),
                                              (16, 48, 1, 1, "scalar")])
def test_count_n_running_var(L, M, N, S, force, form, cn_mult):
    """running_var = (1 - m) rv + m var_biased cn / (cn - 1), cn = count_n or M when 0 (the small
    kernel and dense_finalize_kernel).  Momentum 0.5, so that cn = 2M against M moves running_var
    by far more than the tolerance at every M here."""
    dat = _data(M, N, S, seed=4)
    m, cn = 0.5, (cn_mult * M or M)
    o = _run_fwd(L, _dev(dat), M, N, "train", "tanh", expect=form, count_n=cn_mult * M, momentum=m,
                 off_out=force)
    mean, var = dat.z.mean(0), dat.z.var(0, unbiased=False)
    _close(o.rv.cpu(), (1 - m) * dat.rv.double() + m * var * cn / (cn - 1), T_RUN, "running_var")
    _close(o.rm.cpu(), (1 - m) * dat.rm.double() + m * mean, T_RUN, "running_mean")
    _close(o.sm.cpu(), mean, T_OUT, "save_mean")
    _close(o.si.cpu(), 1 / (var + EPS).sqrt(), T_OUT, "save_invstd")
    _check_guards(o)


@pytest.mark.parametrize("N,form", [(12, "small"), (10, "scalar")])
@pytest.mark.parametrize("count_n", [0, 1])
def test_count_n_one_row(L, N, form, count_n):
    """M = 1, cn = 1: the cn > 1 guard keeps the biased variance (0), no division by zero."""
    dat = _data(1, N, 1, seed=5)
    o = _run_fwd(L, _dev(dat), 1, N, "train", "linear", expect=form, count_n=count_n, momentum=0.5)
    assert torch.isfinite(o.rv.cpu()).all()
    _close(o.rv.cpu(), 0.5 * dat.rv.double(), T_RUN, "running_var")
    _close(o.rm.cpu(), 0.5 * dat.rm.double() + 0.5 * dat.z[0], T_RUN, "running_mean")
    _close(o.out.cpu(1, N), dat.beta.double().view(1, N), T_OUT, "out")
    _check_guards(o)


# ------------------------------------------------------------------ 5. generated dropout
@pytest.mark.parametrize("M,N,natural", [(128, 1024, "small"), (1024, 4096, "v4")])
def test_generated_dropout(L, M, N, natural):
    """keep_in == NULL: the mask is a function of (seed, stream_id, step, flat index) alone — the
    same bytes in the natural form and the forced scalar form, with step_ctr NULL or a device
    counter of 0, other bytes at counter 5; out and the backward follow the written keep_out."""
    p, act = 0.15, "relu"
    dat = _data(M, N, 1, seed=6)
    d = _dev(dat)
    c0 = torch.tensor([0, 0], dtype=torch.int64, device=DEV)
    c5 = torch.tensor([5, 0], dtype=torch.int64, device=DEV)
    kw = dict(p=p, keep_out=True, seed=7, stream_id=5)
    a = _run_fwd(L, d, M, N, "train", act, expect=natural, **kw)
    s = _run_fwd(L, d, M, N, "train", act, expect="scalar", off_out=1, **kw)
    z0 = _run_fwd(L, d, M, N, "train", act, expect=natural, step_ctr=c0, **kw)
    z5 = _run_fwd(L, d, M, N, "train", act, expect=natural, step_ctr=c5, **kw)
    s5 = _run_fwd(L, d, M, N, "train", act, expect="scalar", off_out=1, step_ctr=c5, **kw)
    for o in (a, s, z0, z5, s5):
        _check_guards(o)
    keep = a.kout.cpu(M, N)
    assert ((keep == 0) | (keep == 1)).all()
    assert abs(1 - keep.float().mean().item() - p) < 0.01
    _same_bits(s.kout.t, a.kout.t, "mask of the %s and the scalar form" % natural)
    _same_bits(z0.kout.t, a.kout.t, "mask with step_ctr NULL and with a counter holding 0")
    _same_bits(s5.kout.t, z5.kout.t, "mask of the %s and the scalar form at step 5" % natural)
    k5 = z5.kout.cpu(M, N)
    assert 0.2 < (k5 != keep).float().mean().item() < 0.3     # 2 p (1 - p) = 0.255 if independent
    r = _ref_fwd(dat.z, "train", act, dat.gamma, dat.beta, keep=keep, p=p)
    for o in (a, s):
        out = o.out.cpu(M, N)
        assert (out[keep == 0] == 0).all()
        _close(out, r.out, T_OUT, "out")
    rb = _ref_bwd(dat.g, r, "train", act, dat.gamma, keep, p)
    cols = _kink_free_cols(act, r.y)
    for o, form, off in ((a, natural, 0), (s, "scalar", 1)):
        b = _run_bwd(L, d, M, N, "train", act, expect=form, xhat=o.xhat, si=o.si, p=p, keep=o.kout.t,
                     off_dz=off)
        _close(b.dz.cpu(M, N)[:, cols], rb.dz[:, cols], T_DZ, "dz")
        _close(b.dgamma.cpu()[cols], rb.dgamma[cols], T_PAR, "dgamma")
        _close(b.dbeta.cpu()[cols], rb.dbeta[cols], T_PAR, "dbeta")
        assert (b.dbias.cpu() == 0).all()
        _check_guards(b)


# ------------------------------------------------------------------ 6. the forms agree
AGREE = [(100, 64, 3, "small"), (128, 520, 1, "small"), (128, 1024, 2, "small"), (1030, 4096, 5, "v4")]


def _agree(x, y, exact, tol, what, check=True):
    """Same bits, or (exact False) within tol.  check False: print how far the bits are apart
    instead of asserting."""
    if not exact:
        return _close(x.cpu(), y.cpu(), tol, what)
    if check:
        return _same_bits(x.t, y.t, what + ": natural and scalar form")
    bx, by = _bits(x.t).astype(np.int64), _bits(y.t).astype(np.int64)
    fx, fy = x.cpu().double(), y.cpu().double()
    print("%s: %d of %d words differ, max |difference| %.3g at values up to %.3g, max word distance %d"
          % (what, (bx != by).sum(), bx.size, (fx - fy).abs().max(), fy.abs().max(), np.abs(bx - by).max()))


@pytest.mark.parametrize("norm", ["eval", "none", "train"])
@pytest.mark.parametrize("M,N,S,natural", AGREE)
def test_forms_agree_forward(L, M, N, S, natural, norm):
    """Eval and no-norm have no column reduction: the natural form and the forced scalar form give
    the same bits (up to 3 slabs the small form adds them in the scalar order; the v4 form always
    does).  Training BatchNorm: v4 is the scalar kernels "operation for operation" — same bits in
    out, xhat, save_* and the running statistics; the small form sums the rows in another order
    and stays within the fp32 tolerances."""
    p, act = 0.15, "tanh"
    dat = _data(M, N, S, seed=7)
    d = _dev(dat)
    exact = not (norm == "train" and natural == "small")
    a = _run_fwd(L, d, M, N, norm, act, expect=natural, p=p, keep_in=dat.keep)
    s = _run_fwd(L, d, M, N, norm, act, expect="scalar", p=p, keep_in=dat.keep, off_out=1)
    _agree(a.out, s.out, exact, T_OUT, "out")
    _agree(a.xhat, s.xhat, exact, T_OUT, "xhat")
    if norm == "train":
        for k, tol in (("sm", T_OUT), ("si", T_OUT), ("rm", T_RUN), ("rv", T_RUN)):
            _agree(getattr(a, k), getattr(s, k), exact, tol, k)
    for o in (a, s):
        _check_guards(o)


@pytest.mark.parametrize("norm", ["none", "train"])
@pytest.mark.parametrize("M,N,S,natural", AGREE)
def test_forms_agree_backward(L, M, N, S, natural, norm):
    """Both backwards read one forward's outputs, so only the backward's form differs.  No norm:
    dz and dz_bf16 have the same bits in every form (dbias is a column sum: tolerance).  Training
    BatchNorm: the small form within the fp32 tolerances of the scalar form; v4 the same bits.

    (Left to itself the compiler contracts other products in the two backward pairs; the v4
    kernels spell out the scalar kernels' compiled arithmetic.  Before they did, 24 % of the dz
    words at 1030 x 4096 differed, by one unit in the last place of the largest elements.)"""
    p, act = 0.15, "tanh"
    dat = _data(M, N, S, seed=7)
    d = _dev(dat)
    exact = not (norm == "train" and natural == "small")
    f = _run_fwd(L, d, M, N, norm, act, expect="scalar", p=p, keep_in=dat.keep, off_out=1)
    kwb = dict(xhat=f.xhat, si=f.si, p=p, keep=d.keep, bf16=True)
    ba = _run_bwd(L, d, M, N, norm, act, expect=natural, **kwb)
    bs = _run_bwd(L, d, M, N, norm, act, expect="scalar", off_dz=1, **kwb)
    for o in (ba, bs):
        _check_guards(o)
    names = ("dz", "dbias") + (("dgamma", "dbeta") if norm == "train" else ())
    tols = dict(dz=T_DZ, dbias=T_PAR, dgamma=T_PAR, dbeta=T_PAR)
    for k in names:
        _close(getattr(ba, k).cpu(), getattr(bs, k).cpu(), tols[k], k)
    if exact:
        same = ("dz", "h") + (("dgamma", "dbeta", "dbias") if norm == "train" else ())
        for check in (False, True):             # every output's figures first, then the assertions
            for k in same:
                _agree(getattr(ba, k), getattr(bs, k), True, None, "dz_bf16" if k == "h" else k, check)



# ------------------------------------------------------------------ masks at odd addresses
@pytest.mark.parametrize("M,N,natural", [(100, 64, "small"), (1024, 4096, "v4")])
def test_masks_at_odd_addresses_take_the_scalar_form(L, M, N, natural):
    """The small and v4 forms move 4 mask bytes as one word: a keep_in / keep_out / keep that
    starts one byte into its allocation must take the scalar form, give the reference's results
    and write the bytes of the aligned run."""
    p, act = 0.15, "tanh"
    dat = _data(M, N, 1, seed=8)
    d = _dev(dat)
    r = _ref_fwd(dat.z, "train", act, dat.gamma, dat.beta, keep=dat.keep, p=p)
    o = _run_fwd(L, d, M, N, "train", act, expect="scalar", p=p, keep_in=dat.keep, off_kin=1)
    _close(o.out.cpu(M, N), r.out, T_OUT, "out, keep_in at an odd address")
    a = _run_fwd(L, d, M, N, "train", act, expect=natural, p=p, keep_in=dat.keep, keep_out=True)
    u = _run_fwd(L, d, M, N, "train", act, expect="scalar", p=p, keep_in=dat.keep, keep_out=True,
                 off_kout=1)
    _same_bits(a.kout.t, dat.keep, "keep_out copies keep_in")
    _same_bits(u.kout.t, a.kout.t, "keep_out at an odd address")
    ga = _run_fwd(L, d, M, N, "train", act, expect=natural, p=p, keep_out=True, seed=3)
    gu = _run_fwd(L, d, M, N, "train", act, expect="scalar", p=p, keep_out=True, seed=3, off_kout=1)
    _same_bits(gu.kout.t, ga.kout.t, "generated keep_out at an odd address")
    _close(gu.out.cpu(M, N), _ref_fwd(dat.z, "train", act, dat.gamma, dat.beta,
                                      keep=gu.kout.cpu(M, N), p=p).out, T_OUT, "out, generated mask")
    rb = _ref_bwd(dat.g, r, "train", act, dat.gamma, dat.keep, p)
    b = _run_bwd(L, d, M, N, "train", act, expect="scalar", xhat=o.xhat, si=o.si, p=p, keep=d.keep,
                 off_keep=1)
    _close(b.dz.cpu(M, N), rb.dz, T_DZ, "dz, keep at an odd address")
    _close(b.dgamma.cpu(), rb.dgamma, T_PAR, "dgamma")
    _close(b.dbeta.cpu(), rb.dbeta, T_PAR, "dbeta")
    for x in (o, a, u, ga, gu, b):
        _check_guards(x)


# ------------------------------------------------------------------ the SyncBN halves
@functools.lru_cache(maxsize=2)
def _sync_data(splits, N, seed=0):
    """A global batch whose rank r rows are scaled by 1 + 0.25 r and shifted by 0.5 r: the ranks'
    means and variances differ, so the between-rank term of the merge carries most of the global
    variance."""
    Mt = sum(splits)
    g = torch.Generator().manual_seed(7919 * seed + 31 * Mt + N + len(splits))
    d = NS(M=Mt, N=N, S=2)
    d.slabs = torch.randn(2, Mt, N, generator=g)
    r0 = 0
    for r, m in enumerate(splits):
        d.slabs[:, r0:r0 + m] *= 1 + 0.25 * r
        d.slabs[0, r0:r0 + m] += 0.5 * r
        r0 += m
    d.gout = torch.randn(2, Mt, N, generator=g)
    d.bias = torch.randn(N, generator=g) * 0.1
    d.gamma = torch.rand(N, generator=g) + 0.5
    d.beta = torch.randn(N, generator=g) * 0.1
    d.rm = torch.randn(N, generator=g) * 0.3
    d.rv = torch.rand(N, generator=g) + 0.5
    d.keep = (torch.rand(Mt, N, generator=g) > 0.15).to(torch.uint8)
    d.z = d.slabs.double().sum(0) + d.bias.double()
    d.g = d.gout.double().sum(0)
    return d


def _rank_inputs(dat, splits):
    shared = {k: getattr(dat, k).to(DEV) for k in ("bias", "gamma", "beta", "rm", "rv")}
    out, r0 = [], 0
    for m in splits:
        out.append(NS(slabs=dat.slabs[:, r0:r0 + m].contiguous().to(DEV),
                      gout=dat.gout[:, r0:r0 + m].contiguous().to(DEV),
                      keep=dat.keep[r0:r0 + m].contiguous(), **shared))
        r0 += m
    return out


def _sync_forward(L, dat, ranks, splits, forms, act, p, zero_row=None):
    """pkc_dense_fwd_stats of every rank into its row of one zero-filled states buffer, then
    pkc_dense_fwd_sync_apply of every rank with it.  zero_row: an all-zero row inserted there."""
    N, R = dat.N, len(splits)
    rows = R + (zero_row is not None)
    states = torch.zeros(rows, 3 * N, device=DEV)
    row = [r if zero_row is None or r < zero_row else r + 1 for r in range(R)]
    fs = []
    for r, m in enumerate(splits):
        f = _fwd(L, ranks[r], m, N, "train", act, expect=forms[r], small=False, p=p,
                 keep_in=ranks[r].keep if p > 0 else None)
        L.call("pkc_dense_fwd_stats", C.byref(f.args), _p(f.work), C.c_void_p(states[row[r]].data_ptr()),
               _s())
        fs.append(f)
    for f in fs:
        L.call("pkc_dense_fwd_sync_apply", C.byref(f.args), _p(f.work), L.ptr(states), rows, _s())
    return fs, states, row


def _sync_backward(L, dat, ranks, splits, forms, act, p, fs, scratch=0):
    """pkc_dense_bwd_stats per rank, an fp32 sum of the ranks' sums[2N] on the device in place of
    the all-reduce, pkc_dense_bwd_sync_apply per rank with the global row count."""
    N = dat.N
    bs, sums = [], []
    for r, m in enumerate(splits):
        b = _bwd(L, ranks[r], m, N, "train", act, expect=forms[r], small=False, xhat=fs[r].xhat,
                 si=fs[r].si, p=p, keep=ranks[r].keep.to(DEV) if p > 0 else None, bf16=True,
                 scratch=scratch)
        b.sums = _G(2 * N, 4)
        L.call("pkc_dense_bwd_stats", C.byref(b.args), _p(b.work), _p(b.sums), _s())
        bs.append(b)
        sums.append(b.sums.t)
    total = sums[0].clone()
    for t in sums[1:]:
        total += t
    for b in bs:
        L.call("pkc_dense_bwd_sync_apply", C.byref(b.args), _p(b.work), L.ptr(total), sum(splits), _s())
    return bs


SYNC = [((17, 200, 1024), 4096, ("scalar", "scalar", "v4")), ((1,), 48, ("scalar",)),
        ((33, 31), 70, ("scalar", "scalar")), ((16, 16, 16, 16, 1), 48, ("scalar",) * 5)]


@pytest.mark.parametrize("act", ["relu", "tanh", "linear"])
@pytest.mark.parametrize("splits,N,forms", SYNC)
def test_syncbn_halves_equal_whole_batch(L, splits, N, forms, act):
    """R emulated ranks with different row counts, means and variances against float64 BatchNorm
    of the whole batch, forward and backward."""
    p = 0.0 if act == "tanh" else 0.15
    dat = _sync_data(splits, N)
    Mt, R = dat.M, len(splits)
    ranks = _rank_inputs(dat, splits)
    keep = dat.keep if p > 0 else None
    ref = _ref_fwd(dat.z, "train", act, dat.gamma, dat.beta, keep=keep, p=p)
    fs, states, row = _sync_forward(L, dat, ranks, splits, forms, act, p)
    _close(torch.cat([f.out.cpu(m, N) for f, m in zip(fs, splits)]), ref.out, T_OUT, "out")
    _close(torch.cat([f.xhat.cpu(m, N) for f, m in zip(fs, splits)]), ref.xh, T_OUT, "xhat")
    unb = ref.var * Mt / (Mt - 1) if Mt > 1 else ref.var
    _close(fs[0].sm.cpu(), ref.mean, T_OUT, "save_mean")
    _close(fs[0].si.cpu(), 1 / (ref.var + EPS).sqrt(), T_OUT, "save_invstd")
    _close(fs[0].rm.cpu(), 0.95 * dat.rm.double() + 0.05 * ref.mean, T_RUN, "running_mean")
    _close(fs[0].rv.cpu(), 0.95 * dat.rv.double() + 0.05 * unb, T_RUN, "running_var")
    for f in fs[1:]:
        for k in ("sm", "si", "rm", "rv"):
            _same_bits(getattr(f, k).t, getattr(fs[0], k).t, "%s differs between ranks" % k)
    # rank r's row of states: (rows, mean, M2) of its block.  Mean as save_mean; M2 = rows x the
    # block's variance, so the running-variance tolerance scaled by the rows
    st, r0 = states.cpu().double(), 0
    for r, m in enumerate(splits):
        zr = dat.z[r0:r0 + m]
        r0 += m
        assert (st[row[r], :N] == m).all()
        _close(st[row[r], N:2 * N], zr.mean(0), T_OUT, "state mean of rank %d" % r)
        _close(st[row[r], 2 * N:], zr.var(0, unbiased=False) * m, dict(rtol=1e-4, atol=1e-6 * m),
               "state M2 of rank %d" % r)
    for f in fs:
        _check_guards(f)
    # an all-zero state row (a rank without rows) changes no bit
    fz, _, _ = _sync_forward(L, dat, ranks, splits, forms, act, p, zero_row=min(1, R))
    for f, g in zip(fs, fz):
        for k in ("out", "xhat", "sm", "si", "rm", "rv"):
            _same_bits(getattr(g, k).t, getattr(f, k).t, "%s with a zero state row" % k)
    # backward
    rb = _ref_bwd(dat.g, ref, "train", act, dat.gamma, keep, p)
    cols = _kink_free_cols(act, ref.y)
    bs = _sync_backward(L, dat, ranks, splits, forms, act, p, fs)
    _close(torch.cat([b.dz.cpu(m, N) for b, m in zip(bs, splits)])[:, cols], rb.dz[:, cols], T_DZ, "dz")
    _close(sum(b.dgamma.cpu().double() for b in bs)[cols], rb.dgamma[cols], T_PAR, "sum of dgamma")
    _close(sum(b.dbeta.cpu().double() for b in bs)[cols], rb.dbeta[cols], T_PAR, "sum of dbeta")
    for b in bs:
        assert (b.dbias.cpu() == 0).all()
        _same_bits(b.h.t, _rne(b.dz.t), "dz_bf16")
        _check_guards(b)
    b1 = _sync_backward(L, dat, ranks, splits, forms, act, p, fs, scratch=1)
    for b, c in zip(bs, b1):
        _same_bits(c.h.t, b.h.t, "dz_bf16 with dz_scratch = 1")
        _check_guards(c)


@pytest.mark.parametrize("M,N,form", [(300, 64, "scalar"), (1030, 4096, "v4")])
def test_syncbn_single_rank_equals_plain_entry_points(L, M, N, form):
    """R = 1: the split entry points against pkc_dense_fwd / pkc_dense_bwd on the same rows.  (Not
    the same bits: the one-state merge computes mean * n / n.)"""
    p, act = 0.15, "relu"
    dat = _sync_data((M,), N, seed=1)
    ranks = _rank_inputs(dat, (M,))
    d = ranks[0]
    fs, _, _ = _sync_forward(L, dat, ranks, (M,), (form,), act, p)
    o = _run_fwd(L, d, M, N, "train", act, expect=form, p=p, keep_in=dat.keep)
    for k, tol in (("out", T_OUT), ("xhat", T_OUT), ("sm", T_OUT), ("si", T_OUT), ("rm", T_RUN),
                   ("rv", T_RUN)):
        _close(getattr(fs[0], k).cpu(), getattr(o, k).cpu(), tol, k)
    # both backwards from the plain forward's outputs
    bs = _sync_backward(L, dat, ranks, (M,), (form,), act, p, [o])
    b = _run_bwd(L, d, M, N, "train", act, expect=form, xhat=o.xhat, si=o.si, p=p, keep=d.keep.to(DEV))
    _close(bs[0].dz.cpu(), b.dz.cpu(), T_DZ, "dz")
    _close(bs[0].dgamma.cpu(), b.dgamma.cpu(), T_PAR, "dgamma")
    _close(bs[0].dbeta.cpu(), b.dbeta.cpu(), T_PAR, "dbeta")
    assert (bs[0].dbias.cpu() == 0).all() and (b.dbias.cpu() == 0).all()
    for x in (fs[0], o, bs[0], b):
        _check_guards(x)


def test_syncbn_entry_checks(L):
    """nranks = 0, states == NULL, sums == NULL and total_rows < M are refused with a message before
    any launch: every output still holds its sentinel."""
    M, N = 33, 70
    dat = _sync_data((M,), N, seed=2)
    d = _rank_inputs(dat, (M,))[0]
    lib = L.lib()
    states = torch.zeros(1, 3 * N, device=DEV)
    sums = torch.zeros(2 * N, device=DEV)

    def refused(st):
        assert st == L.PKC_ERR_ARG
        msg = lib.pkc_last_error()
        assert msg and b"pkc_dense_" in msg
        torch.cuda.synchronize()

    f = _fwd(L, d, M, N, "train", "relu", expect="scalar", small=False)
    refused(lib.pkc_dense_fwd_stats(C.byref(f.args), _p(f.work), None, _s()))
    refused(lib.pkc_dense_fwd_sync_apply(C.byref(f.args), _p(f.work), None, 1, _s()))
    refused(lib.pkc_dense_fwd_sync_apply(C.byref(f.args), _p(f.work), L.ptr(states), 0, _s()))
    for k in ("out", "xhat", "sm", "si", "work"):
        assert getattr(f, k).untouched(), k
    _same_bits(f.rm.t, dat.rm)
    _same_bits(f.rv.t, dat.rv)
    assert (states == 0).all()
    xhat, si = torch.randn(M, N, device=DEV), torch.ones(N, device=DEV)
    b = _bwd(L, d, M, N, "train", "relu", expect="scalar", small=False, xhat=xhat, si=si, bf16=True)
    refused(lib.pkc_dense_bwd_stats(C.byref(b.args), _p(b.work), None, _s()))
    refused(lib.pkc_dense_bwd_sync_apply(C.byref(b.args), _p(b.work), None, M, _s()))
    refused(lib.pkc_dense_bwd_sync_apply(C.byref(b.args), _p(b.work), L.ptr(sums), M - 1, _s()))
    for k in ("dz", "h", "dgamma", "dbeta", "dbias", "work"):
        assert getattr(b, k).untouched(), k

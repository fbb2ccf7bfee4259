"""GPU parity of the CNN kernels (pkc_conv1d_fwd / _bwd, pkc_conv_post_fwd / _bwd) through the C
ABI against tests/cnn_ref.py.

Exact cases: integer-valued x, W, b, dy in [-2, 2] keep every sum below 2^24, so fp32 is exact in
any summation order and z, the first-max offsets, dX, dW and db must EQUAL the reference's, ties
included.  Real-valued cases: per-element bound 2 (K + 2) 2^-24 (|W| (*) |x| + |b|) against the fp64
reference, K the contraction depth (C_in len forward, B L_conv for dW, C_out len for dX); the
factor 2 covers a product rounded before it is accumulated.  The backward is fed the GPU forward's
own offset map, so a rounding-level near-tie cannot reroute a gradient."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cnn_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    from pkc import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return _lib


# (B, C_in, len, C_out, L_in, pool): the edges of the tiling
SHAPES = {
    "k10_tail": (3, 1, 10, 8, 47, 3),        # K = 10 (not a multiple of 4), pool tail of 2
    "k240_odd": (2, 80, 3, 60, 143, 2),      # C_out % 16 != 0, L_conv 141 > 128 (partial tile)
    "pool1": (2, 3, 4, 5, 21, 1),
    "b1": (1, 8, 3, 6, 30, 2),
    "b130": (130, 8, 3, 6, 30, 2),           # more samples than dW partial slabs
    "len129": (2, 1, 129, 7, 300, 3),        # a long filter (raw-waveform layers)
}


def _data(shape, exact, seed=0):
    B, Ci, ln, Co, Li, pool = shape
    g = torch.Generator().manual_seed(seed)
    Lo = (Li - ln + 1) // pool
    if exact:
        r = lambda *s: torch.randint(-2, 3, s, generator=g).float()      # noqa: E731
    else:
        r = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
    return r(B, Ci, Li), r(Co, Ci, ln), r(Co), r(B, Co, Lo)


def run_fwd(L, x, W, b, pool):
    B, Ci, Li = x.shape
    Co, _, ln = W.shape
    Lo = (Li - ln + 1) // pool
    xd, Wd, bd = x.to(DEV).contiguous(), W.to(DEV).contiguous(), b.to(DEV)
    z = torch.full((B, Co, Lo), float("nan"), device=DEV)
    off = torch.full((B, Co, Lo), 255, dtype=torch.uint8, device=DEV)
    a = L.Conv1dArgs(B=B, C_in=Ci, L_in=Li, C_out=Co, len=ln, pool=pool, x=xd.data_ptr(),
                     ldx=Ci * Li, W=Wd.data_ptr(), bias=bd.data_ptr(), z=z.data_ptr(),
                     off=off.data_ptr())
    assert L.lib().pkc_conv1d_ok(C.byref(a)) == 1
    L.call("pkc_conv1d_fwd", C.byref(a), _s())
    torch.cuda.synchronize()
    return z, off, (xd, Wd, bd)


def run_bwd(L, dev, off, dz, pool, want_dx=True):
    xd, Wd, bd = dev
    B, Ci, Li = xd.shape
    Co, _, ln = Wd.shape
    dzd = dz.to(DEV).contiguous()
    dx = torch.full((B, Ci, Li), float("nan"), device=DEV) if want_dx else None
    dW = torch.full_like(Wd, float("nan"))
    db = torch.full_like(bd, float("nan"))
    a = L.Conv1dArgs(B=B, C_in=Ci, L_in=Li, C_out=Co, len=ln, pool=pool, x=xd.data_ptr(),
                     ldx=Ci * Li, W=Wd.data_ptr(), bias=bd.data_ptr(), off=off.data_ptr(),
                     dz=dzd.data_ptr(), dx=dx.data_ptr() if want_dx else None, lddx=Ci * Li,
                     dW=dW.data_ptr(), dbias=db.data_ptr())
    nw = L.lib().pkc_conv1d_bwd_work_size(C.byref(a))
    assert nw > 0
    work = torch.full((nw,), float("nan"), device=DEV)
    L.call("pkc_conv1d_bwd", C.byref(a), L.ptr(work), _s())
    torch.cuda.synchronize()
    return dx, dW, db


def ref_bwd(x, W, b, off, dz, pool, dtype):
    """Gradients of conv + pool with the routing given by `off` (not re-derived from values)."""
    x = x.to(dtype).requires_grad_(True)
    W = W.to(dtype).requires_grad_(True)
    b = b.to(dtype).requires_grad_(True)
    c = F.conv1d(x, W, b)
    Lo = off.shape[-1]
    idx = off.long() + torch.arange(Lo) * pool
    (c.gather(2, idx) * dz.to(dtype)).sum().backward()
    dconv = torch.zeros(c.shape, dtype=dtype).scatter_(2, idx, dz.to(dtype))
    return x.grad, W.grad, b.grad, dconv


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_exact(L, name):
    shape = SHAPES[name]
    pool = shape[5]
    x, W, b, dz = _data(shape, True)
    z, off, dev = run_fwd(L, x, W, b, pool)
    zr, offr = cnn_ref.conv_pool(x, W, b, pool)
    assert torch.equal(z.cpu(), zr)
    assert torch.equal(off.cpu(), offr), "first-max offsets (ties included)"
    dx, dW, db = run_bwd(L, dev, off, dz, pool)
    dxr, dWr, dbr, _ = ref_bwd(x, W, b, offr, dz, pool, torch.float64)
    assert torch.equal(dx.cpu().double(), dxr)
    assert torch.equal(dW.cpu().double(), dWr)
    assert torch.equal(db.cpu().double(), dbr)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_real(L, name):
    shape = SHAPES[name]
    B, Ci, ln, Co, Li, pool = shape
    x, W, b, dz = _data(shape, False, seed=1)
    z, off, dev = run_fwd(L, x, W, b, pool)
    off_c = off.cpu()
    Lo = z.shape[-1]
    idx = off_c.long() + torch.arange(Lo) * pool
    c64 = F.conv1d(x.double(), W.double(), b.double())
    mag = F.conv1d(x.abs().double(), W.abs().double(), b.abs().double())
    # the value at the GPU's chosen position is the conv output there, within the bound ...
    bound = 2 * (Ci * ln + 2) * U * mag.gather(2, idx)
    err = (z.cpu().double() - c64.gather(2, idx)).abs()
    print("fwd max err/bound", float((err / bound).max()))
    assert bool((err <= bound).all())
    # ... and no element of its window exceeds it by more than the two bounds
    win = c64[..., :Lo * pool].reshape(B, Co, Lo, pool)
    wb = 2 * (Ci * ln + 2) * U * mag[..., :Lo * pool].reshape(B, Co, Lo, pool)
    assert bool((win <= (z.cpu().double() + bound).unsqueeze(-1) + wb).all())
    dx, dW, db = run_bwd(L, dev, off, dz, pool)
    dxr, dWr, dbr, dconv = ref_bwd(x, W, b, off_c, dz, pool, torch.float64)
    Lc = Li - ln + 1
    mW = torch.zeros_like(dWr)
    for k in range(ln):                        # |dconv| (*) |x| per (co, ci, k)
        mW[:, :, k] = torch.einsum("bol,bil->oi", dconv.abs(), x.abs().double()[:, :, k:k + Lc])
    mX = F.conv_transpose1d(dconv.abs(), W.abs().double())
    for nm, got, ref, mag_, K in (("dW", dW, dWr, mW, B * Lc), ("dX", dx, dxr, mX, Co * ln),
                                  ("db", db, dbr, dconv.abs().sum((0, 2)), B * Lc)):
        bd = 2 * (K + 2) * U * mag_
        e = (got.cpu().double() - ref).abs()
        print(nm, "max err/bound", float((e / bd.clamp_min(1e-300)).max()))
        assert bool((e <= bd).all()), nm


def test_no_dx_and_strided_rows(L):
    """dx == NULL (a first layer reading features) and x / dx rows inside a wider matrix."""
    B, Ci, ln, Co, Li, pool = 4, 1, 5, 6, 33, 2
    x, W, b, dz = _data((B, Ci, ln, Co, Li, pool), True, seed=2)
    z, off, dev = run_fwd(L, x, W, b, pool)
    dx0, dW0, db0 = run_bwd(L, dev, off, dz, pool)
    dx1, dW1, db1 = run_bwd(L, dev, off, dz, pool, want_dx=False)
    assert dx1 is None and torch.equal(dW0, dW1) and torch.equal(db0, db1)
    F_ = 50                                    # columns 7 .. 39 of a 50-wide feature matrix
    wide = torch.full((B, F_), float("nan"))
    wide[:, 7:7 + Li] = x[:, 0]
    wd = wide.to(DEV)
    dxw = torch.full((B, F_), float("nan"), device=DEV)
    Lo = z.shape[-1]
    z2 = torch.empty_like(z)
    off2 = torch.empty_like(off)
    dzd = dz.to(DEV)
    dW2, db2 = torch.empty_like(dW0), torch.empty_like(db0)
    a = L.Conv1dArgs(B=B, C_in=Ci, L_in=Li, C_out=Co, len=ln, pool=pool, x=wd.data_ptr() + 4 * 7,
                     ldx=F_, W=dev[1].data_ptr(), bias=dev[2].data_ptr(), z=z2.data_ptr(),
                     off=off2.data_ptr(), dz=dzd.data_ptr(), dx=dxw.data_ptr() + 4 * 7, lddx=F_,
                     dW=dW2.data_ptr(), dbias=db2.data_ptr())
    L.call("pkc_conv1d_fwd", C.byref(a), _s())
    work = torch.empty(L.lib().pkc_conv1d_bwd_work_size(C.byref(a)), device=DEV)
    L.call("pkc_conv1d_bwd", C.byref(a), L.ptr(work), _s())
    torch.cuda.synchronize()
    assert torch.equal(z2, z) and torch.equal(off2, off)
    assert torch.equal(dW2, dW0) and torch.equal(db2, db0)
    assert torch.equal(dxw[:, 7:7 + Li], dx0[:, 0])
    assert bool(torch.isnan(dxw[:, :7]).all()) and bool(torch.isnan(dxw[:, 7 + Li:]).all())


def test_deterministic(L):
    shape = SHAPES["b130"]
    x, W, b, dz = _data(shape, False, seed=3)
    z, off, dev = run_fwd(L, x, W, b, shape[5])
    a1 = run_bwd(L, dev, off, dz, shape[5])
    a2 = run_bwd(L, dev, off, dz, shape[5])
    for u, v in zip(a1, a2):
        assert torch.equal(u, v)


def test_refused_shapes(L):
    a = L.Conv1dArgs(B=1, C_in=1, L_in=20, C_out=4, len=30, pool=1)
    assert L.lib().pkc_conv1d_ok(C.byref(a)) == 0
    a = L.Conv1dArgs(B=1, C_in=1, L_in=400, C_out=4, len=3, pool=100, ldx=400)
    assert L.lib().pkc_conv1d_ok(C.byref(a)) == 0
    with pytest.raises(L.PkcError):
        L.call("pkc_conv1d_fwd", C.byref(a), _s())


# ------------------------------------------------------------------ post kernels
def _post(L, z, norm, gamma, beta, act, eps, p=0.0, keep_in=None, rm=None, rv=None, nslab=1,
          dy=None):
    """Forward (+ backward when dy is given: (nslab, B, C * L)) of pkc_conv_post_*."""
    B, Cc, Ln = z.shape
    zd = z.to(DEV).contiguous()
    t = lambda v: None if v is None else v.to(DEV).contiguous()          # noqa: E731
    gd, bd, kin = t(gamma), t(beta), t(keep_in)
    rmd, rvd = t(rm), t(rv)
    out = torch.full((B, Cc * Ln), float("nan"), device=DEV)
    out_h = torch.zeros(B, Cc * Ln, dtype=torch.bfloat16, device=DEV)
    xhat = torch.zeros(B, Cc, Ln, device=DEV)
    keep = torch.zeros(B, Cc * Ln, dtype=torch.uint8, device=DEV)
    sm, si = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    stat = torch.zeros(B * Cc, 2, device=DEV)
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    a = L.ConvPostArgs(B=B, C=Cc, L=Ln, norm=norm, z=zd.data_ptr(), gamma=L.ptr(gd), beta=L.ptr(bd),
                       running_mean=L.ptr(rmd), running_var=L.ptr(rvd), momentum=0.05, eps=eps,
                       save_mean=sm.data_ptr(), save_invstd=si.data_ptr(), ln_stat=stat.data_ptr(),
                       act=L.ACT[act], drop_p=p, seed=5, step_ctr=ctr.data_ptr(), stream_id=9,
                       keep_in=L.ptr(kin), keep=keep.data_ptr(), xhat=xhat.data_ptr(),
                       out=out.data_ptr(), out_bf16=out_h.data_ptr())
    L.call("pkc_conv_post_fwd", C.byref(a), _s())
    res = dict(out=out, out_h=out_h, keep=keep, rm=rmd, rv=rvd)
    if dy is not None:
        dyd = dy.to(DEV).contiguous()
        dz = torch.full((B, Cc, Ln), float("nan"), device=DEV)
        dg = torch.full_like(gd, float("nan")) if gd is not None else None
        db = torch.full_like(bd, float("nan")) if bd is not None else None
        a.nslab, a.gslab, a.slab_stride = nslab, dyd.data_ptr(), B * Cc * Ln
        a.dz, a.dgamma, a.dbeta = dz.data_ptr(), L.ptr(dg), L.ptr(db)
        L.call("pkc_conv_post_bwd", C.byref(a), _s())
        res.update(dz=dz, dgamma=dg, dbeta=db)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("kind", ["ln", "bn", "none"])
@pytest.mark.parametrize("B,Cc,Ln", [(5, 8, 15), (130, 6, 70), (3, 60, 143)])
def test_post(L, kind, B, Cc, Ln):
    g = torch.Generator().manual_seed(B + Cc)
    z = torch.randn(B, Cc, Ln, generator=g) * 1.5 + 0.3
    shp = (Cc, Ln) if kind == "ln" else (Cc,)
    gamma = torch.rand(shp, generator=g) + 0.5
    beta = torch.randn(shp, generator=g) * 0.1
    dy = torch.randn(2, B, Cc * Ln, generator=g)
    act = "tanh"
    zz = z.double().requires_grad_(True)
    gg, bb = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = torch.zeros(Cc).double(), torch.ones(Cc).double()
    if kind == "ln":
        y = cnn_ref.layer_norm(zz, gg, bb)
    elif kind == "bn":
        y = F.batch_norm(zz, rm, rv, gg, bb, True, 0.05, float(Ln))     # eps = L_out
    else:
        y = zz
    o = cnn_ref.act(act, y).reshape(B, -1)
    (o * dy.double().sum(0)).sum().backward()
    norm = {"ln": L.CONV_NORM_LN, "bn": L.NORM_BN_TRAIN, "none": L.NORM_NONE}[kind]
    r = _post(L, z, norm, gamma if kind != "none" else None, beta if kind != "none" else None, act,
              1e-6 if kind == "ln" else float(Ln), rm=torch.zeros(Cc), rv=torch.ones(Cc), nslab=2,
              dy=dy)
    # the tolerances of the LayerNorm / BatchNorm kernel tests in test_gpu_kernels.py
    torch.testing.assert_close(r["out"].cpu(), o.detach().float(), rtol=1e-4, atol=2e-5)
    torch.testing.assert_close(r["out_h"].cpu().float(), r["out"].cpu().bfloat16().float(), rtol=0,
                               atol=0)
    torch.testing.assert_close(r["dz"].cpu(), zz.grad.float(), rtol=1e-3, atol=1e-5)
    if kind != "none":
        torch.testing.assert_close(r["dgamma"].cpu(), gg.grad.float(), rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(r["dbeta"].cpu(), bb.grad.float(), rtol=1e-4, atol=1e-4)
    if kind == "bn":
        torch.testing.assert_close(r["rm"].cpu(), rm.float(), rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(r["rv"].cpu(), rv.float(), rtol=1e-4, atol=1e-6)


def test_post_bn_running_stats_golden(L):
    """BatchNorm running statistics after one training step against the recorded reference run:
    layer 0 of the golden 'bn' case (eps = L_out = 15, momentum 0.05)."""
    G = np.load(os.path.join(HERE, "golden", "cnn.npz"))
    opts = json.loads(str(G["cases"]))["bn"]
    sd = {k[len("bn/sd/"):]: torch.from_numpy(G[k].copy()) for k in G.files if k.startswith("bn/sd/")}
    x = torch.from_numpy(G["bn/x"].copy())
    pool = int(opts["cnn_max_pool_len"].split(",")[0])
    z, _ = cnn_ref.conv_pool(x.view(x.shape[0], 1, -1), sd["conv.0.weight"], sd["conv.0.bias"], pool)
    r = _post(L, z, L.NORM_BN_TRAIN, sd["bn.0.weight"], sd["bn.0.bias"], "relu", float(z.shape[-1]),
              rm=sd["bn.0.running_mean"].clone(), rv=sd["bn.0.running_var"].clone())
    torch.testing.assert_close(r["rm"].cpu(), torch.from_numpy(G["bn/after/bn.0.running_mean"]),
                               rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(r["rv"].cpu(), torch.from_numpy(G["bn/after/bn.0.running_var"]),
                               rtol=1e-4, atol=1e-6)


def test_post_eval_bn(L):
    g = torch.Generator().manual_seed(4)
    z = torch.randn(4, 5, 9, generator=g)
    gamma, beta = torch.rand(5, generator=g) + 0.5, torch.randn(5, generator=g)
    rm, rv = torch.randn(5, generator=g), torch.rand(5, generator=g) + 0.5
    r = _post(L, z, L.NORM_BN_EVAL, gamma, beta, "relu", 9.0, rm=rm.clone(), rv=rv.clone())
    ref = torch.relu(F.batch_norm(z, rm.clone(), rv.clone(), gamma, beta, False, 0.05, 9.0))
    torch.testing.assert_close(r["out"].cpu(), ref.reshape(4, -1), rtol=1e-4, atol=2e-5)
    assert torch.equal(r["rm"].cpu(), rm) and torch.equal(r["rv"].cpu(), rv)


def test_post_dropout(L):
    """An injected keep mask at p = 0.15 (forward and backward), and the generated stream: mask
    written, rate near 1 - p, output consistent with it."""
    p, B, Cc, Ln = 0.15, 16, 6, 40
    g = torch.Generator().manual_seed(8)
    z = torch.randn(B, Cc, Ln, generator=g)
    keep = (torch.rand(B, Cc * Ln, generator=g) >= p).to(torch.uint8)
    dy = torch.randn(1, B, Cc * Ln, generator=g)
    r = _post(L, z, L.NORM_NONE, None, None, "relu", 0.0, p=p, keep_in=keep, dy=dy)
    ref = torch.relu(z).reshape(B, -1) * keep / (1 - p)
    torch.testing.assert_close(r["out"].cpu(), ref, rtol=1e-6, atol=1e-7)
    assert torch.equal(r["keep"].cpu(), keep)
    dref = (dy[0] * keep / (1 - p) * (z.reshape(B, -1) > 0)).view(B, Cc, Ln)
    torch.testing.assert_close(r["dz"].cpu(), dref, rtol=1e-6, atol=1e-7)
    r2 = _post(L, z, L.NORM_NONE, None, None, "linear", 0.0, p=p)
    k2 = r2["keep"].cpu()
    assert abs(float(k2.float().mean()) - (1 - p)) < 0.03
    torch.testing.assert_close(r2["out"].cpu(), z.reshape(B, -1) * k2 / (1 - p), rtol=1e-6, atol=1e-7)


def test_work_buffer_serves_every_smaller_batch(L):
    """A caller sizes `work` once, for its largest row count, and then runs smaller ones.  The slab
    count of a call is not monotone in B (130 rows: 44 slabs, 128 rows: 64), so the size must not
    depend on B: a buffer of the size asked for B = 130 takes B = 128, 120 and 65 without a write
    past its end (a sentinel region behind it stays untouched) and with the right gradients."""
    Bmax, Ci, ln, Co, Li, pool = 130, 8, 3, 6, 30, 2
    x, W, b, dz = _data((Bmax, Ci, ln, Co, Li, pool), True, seed=5)
    a0 = L.Conv1dArgs(B=Bmax, C_in=Ci, L_in=Li, C_out=Co, len=ln, pool=pool, ldx=Ci * Li)
    nw = L.lib().pkc_conv1d_bwd_work_size(C.byref(a0))
    for B in (128, 120, 65, 1):
        a1 = L.Conv1dArgs(B=B, C_in=Ci, L_in=Li, C_out=Co, len=ln, pool=pool, ldx=Ci * Li)
        assert L.lib().pkc_conv1d_bwd_work_size(C.byref(a1)) == nw
    guard = 1 << 16
    work = torch.full((nw + guard,), -7.0, device=DEV)
    for B in (128, 120, 65):
        z, off, dev = run_fwd(L, x[:B], W, b, pool)
        dzd = dz[:B].to(DEV).contiguous()
        dx = torch.empty(B, Ci, Li, device=DEV)
        dW, db = torch.empty_like(dev[1]), torch.empty_like(dev[2])
        a = L.Conv1dArgs(B=B, C_in=Ci, L_in=Li, C_out=Co, len=ln, pool=pool, x=dev[0].data_ptr(),
                         ldx=Ci * Li, W=dev[1].data_ptr(), bias=dev[2].data_ptr(),
                         off=off.data_ptr(), dz=dzd.data_ptr(), dx=dx.data_ptr(), lddx=Ci * Li,
                         dW=dW.data_ptr(), dbias=db.data_ptr())
        L.call("pkc_conv1d_bwd", C.byref(a), L.ptr(work), _s())
        torch.cuda.synchronize()
        assert bool((work[nw:] == -7.0).all()), "B=%d wrote past the work buffer" % B
        dxr, dWr, dbr, _ = ref_bwd(x[:B], W, b, off.cpu(), dz[:B], pool, torch.float64)
        assert torch.equal(dW.cpu().double(), dWr) and torch.equal(db.cpu().double(), dbr)
        assert torch.equal(dx.cpu().double(), dxr)


def test_post_ln_constant_row(L):
    """LayerNorm over a row that is constant along L (a zero-padded frame: the conv output is the
    bias at every position): std == 0, xhat == 0, and torch masks the std term of the backward to
    0, so the gradients stay finite and equal cnn_ref's.  0.5 * L sums exactly in any order, so the
    mean and std == 0 are exact on both sides."""
    B, Cc, Ln = 6, 5, 15
    g = torch.Generator().manual_seed(12)
    z = torch.randn(B, Cc, Ln, generator=g)
    z[1] = 0.5                                  # every channel row of sample 1
    z[4, 2] = -2.0                              # one row of sample 4
    gamma = torch.rand(Cc, Ln, generator=g) + 0.5
    beta = torch.randn(Cc, Ln, generator=g) * 0.1
    dy = torch.randn(1, B, Cc * Ln, generator=g)
    zz = z.double().requires_grad_(True)
    gg, bb = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    o = cnn_ref.act("tanh", cnn_ref.layer_norm(zz, gg, bb)).reshape(B, -1)
    (o * dy[0].double()).sum().backward()
    assert bool(torch.isfinite(zz.grad).all())
    r = _post(L, z, L.CONV_NORM_LN, gamma, beta, "tanh", 1e-6, dy=dy)
    for k in ("out", "dz", "dgamma", "dbeta"):
        assert bool(torch.isfinite(r[k]).all()), k
    torch.testing.assert_close(r["out"].cpu(), o.detach().float(), rtol=1e-4, atol=2e-5)
    const = torch.zeros(B, Cc, dtype=torch.bool)
    const[1], const[4, 2] = True, True
    dz, dzr = r["dz"].cpu(), zz.grad.float()
    torch.testing.assert_close(dz[~const], dzr[~const], rtol=1e-3, atol=1e-5)
    # a constant row's dz is (dxh - mean(dxh)) / eps, eps = 1e-6: the fp32 rounding of that
    # difference, (L + 2) 2^-24 max |dxh| with |dxh| <= |dy| gamma (tanh' <= 1), times 1e6
    tol = 1e6 * (Ln + 2) * U * float(dy.abs().max() * gamma.max())
    assert float((dz[const] - dzr[const]).abs().max()) <= tol
    assert float(dzr[const].abs().max()) > 1e3 * tol       # (the check has teeth)
    torch.testing.assert_close(r["dgamma"].cpu(), gg.grad.float(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(r["dbeta"].cpu(), bb.grad.float(), rtol=1e-4, atol=1e-4)

"""GPU parity of the sinc filter-bank kernels (pkc_sinc_filters_fwd / _bwd) through the C ABI
against tests/sinc_ref.py.

The yardstick is the reference's own distance: the fp32 restatement (bit-identical to the
reference's filters, test_sinc_cpu.py) against the same formula in fp64 from the same fp32
parameters and constants.  The error arises in the cancellation of lp(high) - lp(low), amplified by
1 / max_ (down to 0.008 at init): a different but correctly rounded sin moves it by a small factor,
a wrong formula by orders of magnitude.  So the kernels are asked to be within 4 x that distance of
the fp64 result: max |.| for the filters (max |f| = 1), relative L2 for the two gradients."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sinc_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SR, MIN_LOW, MIN_BAND = 16000, 50, 50
# N below and above a 64 tile and no multiple of 16; K below and above a wave
SHAPES = [(10, 9), (10, 17), (70, 129), (128, 129)]


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    from pkc import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return _lib


def _params(N, variant):
    """The reference's initial parameters; neg: some entries negated, one of each exactly 0."""
    lo, bd = sinc_ref.mel_init(N, SR, MIN_LOW, MIN_BAND)
    if variant == "neg":
        lo[1] *= -1
        lo[3] = 0.0
        lo[N - 1] *= -1
        bd[2] *= -1
        bd[5] = 0.0
        bd[N - 1] *= -1
    return lo, bd


_REF = {}


def _reference(N, K, variant):
    """Computed once per case and shared: fp32 and fp64 filters, a fixed dW, and the gradients of
    (filters * dW).sum() in both precisions."""
    key = (N, K, variant)
    if key not in _REF:
        lo, bd = _params(N, variant)
        dW = torch.randn(N, K, generator=torch.Generator().manual_seed(100 * N + K))
        out = {"lo": lo, "bd": bd, "dW": dW}
        for name, dt in (("32", torch.float32), ("64", torch.float64)):
            l_, b_ = lo.clone().to(dt).requires_grad_(True), bd.clone().to(dt).requires_grad_(True)
            parts = {}
            f = sinc_ref.sinc_filters(l_, b_, K, SR, MIN_LOW, MIN_BAND, parts)
            (f * dW.to(dt)).sum().backward()
            out["f" + name], out["dlo" + name], out["dbd" + name] = f.detach(), l_.grad, b_.grad
            out["max" + name], out["idx" + name] = parts["max_"].view(-1), parts["idx"].view(-1)
        _REF[key] = out
    return _REF[key]


def _args(L, lo, bd, K, **kw):
    n_, window = sinc_ref.sinc_consts(K, SR)
    t = dict(lo=lo.reshape(-1).to(DEV).contiguous(), bd=bd.reshape(-1).to(DEV).contiguous(),
             n_=n_.reshape(-1).to(DEV).contiguous(), window=window.to(DEV).contiguous())
    a = L.SincArgs(N=lo.numel(), K=K, low_hz=t["lo"].data_ptr(), band_hz=t["bd"].data_ptr(),
                   n_=t["n_"].data_ptr(), window=t["window"].data_ptr(), sr=float(SR),
                   min_low_hz=float(MIN_LOW), min_band_hz=float(MIN_BAND), **kw)
    return a, t


def run_fwd(L, lo, bd, K):
    N = lo.numel()
    f = torch.full((N, K), float("nan"), device=DEV)
    mx = torch.full((N,), float("nan"), device=DEV)
    idx = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    a, keep = _args(L, lo, bd, K, filters=f.data_ptr(), max_=mx.data_ptr(), max_idx=idx.data_ptr())
    assert L.lib().pkc_sinc_ok(C.byref(a)) == 1
    L.call("pkc_sinc_filters_fwd", C.byref(a), _s())
    torch.cuda.synchronize()
    return f, mx, idx


def run_bwd(L, lo, bd, K, dW, idx):
    N = lo.numel()
    dWd = dW.to(DEV).contiguous()
    dlo = torch.full((N,), float("nan"), device=DEV)
    dbd = torch.full((N,), float("nan"), device=DEV)
    a, keep = _args(L, lo, bd, K, max_idx=idx.data_ptr(), dW=dWd.data_ptr(), dlow=dlo.data_ptr(),
                    dband=dbd.data_ptr())
    L.call("pkc_sinc_filters_bwd", C.byref(a), _s())
    torch.cuda.synchronize()
    return dlo.cpu(), dbd.cpu()


@pytest.mark.parametrize("variant", ["init", "neg"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_filters(L, N, K, variant):
    R = _reference(N, K, variant)
    f, mx, idx = run_fwd(L, R["lo"], R["bd"], K)
    f, mx, idx = f.cpu(), mx.cpu(), idx.cpu()
    assert bool(torch.isfinite(f).all())
    d_ref = (R["f32"].double() - R["f64"]).abs().max().item()
    d_gpu = (f.double() - R["f64"]).abs().max().item()
    print("filters N=%d K=%d %s: gpu-fp64 %.3g, fp32-fp64 (d_ref) %.3g" % (N, K, variant, d_gpu, d_ref))
    assert d_gpu <= 4 * d_ref, "max|gpu - fp64| = %.3g > 4 x d_ref = 4 x %.3g" % (d_gpu, d_ref)
    # the right half is the flip of the left before the (asymmetric) window
    window = sinc_ref.sinc_consts(K, SR)[1]
    bp = f.double() / window.double() * mx.double().view(-1, 1)
    assert (bp - torch.flip(bp, dims=[1])).abs().max().item() <= 4e-7 * bp.abs().max().item()
    # the saved maximum: the centre tap (mathematically always the largest), max_ = 2 (high - low)
    assert torch.equal(idx.long(), R["idx64"]) and bool((idx == (K - 1) // 2).all())
    assert (mx.double() - R["max64"]).abs().max().item() <= 4 * max(
        (R["max32"].double() - R["max64"]).abs().max().item(), 2.0 ** -24)


@pytest.mark.parametrize("variant", ["init", "neg"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_gradients(L, N, K, variant):
    R = _reference(N, K, variant)
    _, _, idx = run_fwd(L, R["lo"], R["bd"], K)
    dlo, dbd = run_bwd(L, R["lo"], R["bd"], K, R["dW"], idx)
    for what, got, k in (("dlow", dlo, "dlo"), ("dband", dbd, "dbd")):
        want = R[k + "64"].view(-1)
        d_ref = ((R[k + "32"].view(-1).double() - want).norm() / want.norm()).item()
        d_gpu = ((got.double() - want).norm() / want.norm()).item()
        print("%s N=%d K=%d %s: gpu rel L2 %.3g, fp32 restatement's %.3g" % (what, N, K, variant,
                                                                           d_gpu, d_ref))
        assert d_gpu <= 4 * d_ref, "%s rel L2 %.3g > 4 x %.3g" % (what, d_gpu, d_ref)
    # sign and zero entries: d|p|/dp = sign(p), exactly 0 at p == 0
    lo, bd = R["lo"].view(-1), R["bd"].view(-1)
    assert bool((dlo[lo == 0] == 0).all()) and bool((dbd[bd == 0] == 0).all())
    if variant == "neg":
        assert int((lo == 0).sum()) == 1 and int((bd == 0).sum()) == 1
        P = _reference(N, K, "init")            # the same |p| except at the zeroed entries
        same = (lo != 0) & (bd != 0)
        flip = torch.sign(bd)[same] * torch.sign(P["bd"].view(-1))[same]
        g0 = P["dbd64"].view(-1)[same]
        assert bool((torch.sign(R["dbd64"].view(-1)[same]) == torch.sign(g0) * flip).all())
        assert bool((torch.sign(dbd[same].double()) == torch.sign(R["dbd64"].view(-1)[same])).all())


def test_backward_is_deterministic(L):
    N, K = 128, 129
    R = _reference(N, K, "neg")
    _, _, idx = run_fwd(L, R["lo"], R["bd"], K)
    a = run_bwd(L, R["lo"], R["bd"], K, R["dW"], idx)
    b = run_bwd(L, R["lo"], R["bd"], K, R["dW"], idx)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    f1, f2 = run_fwd(L, R["lo"], R["bd"], K)[0], run_fwd(L, R["lo"], R["bd"], K)[0]
    assert torch.equal(f1, f2)


def test_refused_shapes(L):
    lo, bd = _params(10, "init")
    for bad in (dict(K=16), dict(K=4035), dict(N=0), dict(sr=0.0)):
        a, keep = _args(L, lo, bd, 17)
        for k, v in bad.items():
            setattr(a, k, v)
        assert L.lib().pkc_sinc_ok(C.byref(a)) == 0
        assert L.lib().pkc_last_error().decode() != ""
        with pytest.raises(L.PkcError):
            L.call("pkc_sinc_filters_fwd", C.byref(a), _s())
        with pytest.raises(L.PkcError):
            L.call("pkc_sinc_filters_bwd", C.byref(a), _s())
    a, keep = _args(L, lo, bd, 17)              # a supported shape with null outputs
    assert L.lib().pkc_sinc_ok(C.byref(a)) == 1
    with pytest.raises(L.PkcError):
        L.call("pkc_sinc_filters_fwd", C.byref(a), _s())

"""pkc_mse_fused through the C ABI against fp64 torch on the same fp32 inputs: the mse cost's
per-row loss row_loss[r] = (1/N) sum_j (y - t)^2 and its gradient dy = weight * 2/(M N) * (y - t).

Tolerances (u = 2^-24, the fp32 unit roundoff):
  * row_loss: relative error <= (N + 4) u — every term is non-negative, so any summation order of
    N rounded squares of rounded differences, and the final division, stays inside it;
  * dy: |got - ref| <= 4 u |ref| elementwise — one rounded difference, one rounded constant, one
    product — which is exactly 0 where y == t.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SHAPES = [(1, 1), (5, 40), (3, 63), (3, 65), (70, 257), (2, 1030)]
# whole float4 chunks of aligned rows (the 16-byte path): more than one 256-column sweep, and a
# sweep only some lanes take
VEC_SHAPES = [(5, 40), (70, 260), (2, 1028), (3, 512)]


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    from pkc import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return _lib


def _case(M, N, variant, seed):
    """(y buffer, ldy, target pointer offset in elements, target buffer, ldt, dy buffer, lddy)."""
    g = torch.Generator().manual_seed(seed)
    ldy = lddy = N + 3 if variant == "padded_y" else N
    ldt, c0 = (N + 7, 5) if variant == "odd_target" else (N, 0)
    ybuf = torch.randn(M, ldy, generator=g)
    tbuf = torch.randn(M, ldt, generator=g)
    # some elements with y == t exactly: their gradient is exactly 0
    tbuf[0, c0:c0 + N:3] = ybuf[0, 0:N:3]
    return ybuf, ldy, c0, tbuf, ldt, lddy


def _run(L, M, N, variant, weight, with_dy, seed=0):
    ybuf, ldy, c0, tbuf, ldt, lddy = _case(M, N, variant, seed)
    yd, td = ybuf.to(DEV), tbuf.to(DEV)
    dyd = torch.full((M, lddy), float("nan"), device=DEV)
    rl = torch.full((M + 2,), float("nan"), device=DEV)
    L.call("pkc_mse_fused", M, N, L.ptr(yd), ldy, C.c_void_p(td.data_ptr() + 4 * c0), ldt,
           C.c_float(weight), L.ptr(dyd) if with_dy else None, lddy, L.ptr(rl), _s())
    torch.cuda.synchronize()
    y64 = ybuf[:, :N].double()
    t64 = tbuf[:, c0:c0 + N].double()
    return dict(rl=rl.cpu(), dy=dyd.cpu(), y64=y64, t64=t64, same=(ybuf[:, :N] == tbuf[:, c0:c0 + N]))


def _check(r, M, N, weight, with_dy):
    d = r["y64"] - r["t64"]
    rl_ref = (d * d).mean(1)
    got = r["rl"][:M].double()
    err = ((got - rl_ref).abs() / rl_ref.clamp_min(1e-300)).max().item()
    print("M=%d N=%d row_loss max rel err %.3g (bound %.3g)" % (M, N, err, (N + 4) * U))
    assert ((got - rl_ref).abs() <= (N + 4) * U * rl_ref).all(), "row_loss rel err %.3g" % err
    assert torch.isnan(r["rl"][M:]).all(), "row_loss written past row M"
    if not with_dy:
        assert torch.isnan(r["dy"]).all(), "dy == NULL still wrote a gradient"
        return
    w = float(torch.tensor(weight, dtype=torch.float32))
    ref = w * 2.0 / (M * N) * d
    gdy = r["dy"][:, :N].double()
    derr = ((gdy - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    print("M=%d N=%d dy max rel err %.3g (bound %.3g)" % (M, N, derr, 4 * U))
    assert ((gdy - ref).abs() <= 4 * U * ref.abs()).all(), "dy rel err %.3g" % derr
    assert (gdy[r["same"]] == 0).all() and bool(r["same"].any()) == (N >= 1)
    assert torch.isnan(r["dy"][:, N:]).all(), "dy written past column N"


@pytest.mark.parametrize("mode", ["loss_only", "w1", "w_eighth"])
@pytest.mark.parametrize("variant", ["odd_target", "padded_y", "aligned"])
@pytest.mark.parametrize("M,N", SHAPES)
def test_mse_fused(L, M, N, variant, mode):
    weight = {"loss_only": 1.0, "w1": 1.0, "w_eighth": 0.5 * 0.25}[mode]
    with_dy = mode != "loss_only"
    _check(_run(L, M, N, variant, weight, with_dy, seed=M * 131 + N), M, N, weight, with_dy)


@pytest.mark.parametrize("variant", ["aligned", "odd_target"])
@pytest.mark.parametrize("M,N", VEC_SHAPES)
def test_mse_fused_vector_path_shapes(L, M, N, variant):
    """N % 4 == 0: the aligned variant takes the 16-byte path, the odd target column the scalar one."""
    _check(_run(L, M, N, variant, 0.5 * 0.25, True, seed=M + N), M, N, 0.5 * 0.25, True)


@pytest.mark.parametrize("M,N,variant", [(70, 257, "odd_target"), (70, 260, "aligned")])
def test_mse_fused_bit_identical(L, M, N, variant):
    a = _run(L, M, N, variant, 0.5, True, seed=3)
    b = _run(L, M, N, variant, 0.5, True, seed=3)
    assert torch.equal(a["rl"][:M], b["rl"][:M])
    assert torch.equal(a["dy"][:, :N], b["dy"][:, :N])


def test_mse_fused_refused_arguments(L):
    M, N = 4, 10
    y = torch.zeros(M, N, device=DEV)
    t = torch.zeros(M, N, device=DEV)
    dy = torch.zeros(M, N, device=DEV)
    rl = torch.zeros(M, device=DEV)
    good = dict(M=M, N=N, y=L.ptr(y), ldy=N, t=L.ptr(t), ldt=N, dy=L.ptr(dy), lddy=N, rl=L.ptr(rl))
    bad = [dict(M=0), dict(M=-3), dict(N=0), dict(ldy=N - 1), dict(ldt=N - 1), dict(lddy=N - 1),
           dict(y=None), dict(t=None), dict(rl=None)]
    lib = L.lib()
    for change in bad:
        a = dict(good, **change)
        rc = lib.pkc_mse_fused(a["M"], a["N"], a["y"], a["ldy"], a["t"], a["ldt"], C.c_float(1.0),
                               a["dy"], a["lddy"], a["rl"], _s())
        assert rc < 0, "accepted %s" % change
        msg = lib.pkc_last_error().decode()
        assert "pkc_mse_fused" in msg, (change, msg)
        with pytest.raises(L.PkcError):
            L.call("pkc_mse_fused", a["M"], a["N"], a["y"], a["ldy"], a["t"], a["ldt"],
                   C.c_float(1.0), a["dy"], a["lddy"], a["rl"], _s())
    L.call("pkc_mse_fused", M, N, good["y"], N, good["t"], N, C.c_float(1.0), good["dy"], N,
           good["rl"], _s())
    torch.cuda.synchronize()

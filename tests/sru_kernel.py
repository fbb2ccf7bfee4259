"""Kernel-level harness of the SRU entry points (pkc_sru_fwd / pkc_sru_bwd / pkc_sru_mask_x /
pkc_sru_dx) through the C ABI.  The projections — plain matmuls over the T*B rows, outside the entry
points under test — are done by torch on the device."""
import ctypes as C

import torch

from pkc import _lib as L


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


class Layer:
    """One layer's buffers and the argument struct of the two loop entry points."""

    def __init__(self, T, B, d, D, k, n_in, act="linear", skip=True, alpha=1.0, train=True,
                 drop_p=0.0, keep_in=None):
        self.T, self.B, self.d, self.D, self.k = T, B, d, D, k
        n = d * D
        self.n = n
        self.cs, self.y = _z(T, B, n), _z(T, B, n)
        self.keep = _z(B, n, dtype=torch.uint8)
        self.du, self.dxh = _z(T, B, n * k), _z(T, B, n)
        self.dwc, self.dbias, self.work = _z(2 * n), _z(2 * n), _z(B, 4, n)
        self.keep_in = keep_in
        a = L.SruArgs()
        a.T, a.B, a.d, a.ndir, a.k, a.n_in = T, B, d, D, k, n_in
        a.act, a.train, a.skip, a.alpha = L.ACT[act], int(train), int(skip), alpha
        a.cs, a.y, a.keep = self.cs.data_ptr(), self.y.data_ptr(), self.keep.data_ptr()
        a.drop_p = drop_p
        a.keep_in = keep_in.data_ptr() if keep_in is not None else None
        a.du, a.dxh = self.du.data_ptr(), self.dxh.data_ptr()
        a.dwc, a.dbias, a.work = self.dwc.data_ptr(), self.dbias.data_ptr(), self.work.data_ptr()
        self.a = a

    def forward(self, U, wc, bias, x=None, ldx=0):
        """U (T, B, n*k), wc / bias (2n), x: the rows of the k = 3 skip term (leading dimension
        ldx), all contiguous fp32 on the device."""
        self.hold = (U, wc, bias, x)
        self.a.u, self.a.weight_c, self.a.bias = U.data_ptr(), wc.data_ptr(), bias.data_ptr()
        self.a.x, self.a.ldx = (x.data_ptr() if x is not None else None), ldx
        L.call("pkc_sru_fwd", C.byref(self.a), None)
        return self.y

    def backward(self, dy):
        """dy (T, B, n) or (slabs, T, B, n): partial slabs of dL/dy."""
        self.dy = dy.contiguous()
        ns = dy.shape[0] if dy.dim() == 4 else 1
        self.a.dy, self.a.dy_nslab = self.dy.data_ptr(), ns
        self.a.dy_slab_stride = self.T * self.B * self.n
        L.call("pkc_sru_bwd", C.byref(self.a), None)
        return self.du, self.dxh, self.dwc, self.dbias


def mask_x(x, ld_view, p, keep_in=None, seed=0, stream_id=0):
    """pkc_sru_mask_x on x (T, B, n_in) stored with leading dimension ld_view.shape[-1] (ld_view:
    the (T, B, ld) tensor x is a column slice of).  Returns xt (T, B, n_in), keep (B, n_in)."""
    T, B, n_in = x.shape
    xt, keep = _z(T, B, n_in), _z(B, n_in, dtype=torch.uint8)
    L.call("pkc_sru_mask_x", T, B, n_in, L.ptr(x), ld_view.shape[-1], p, seed, None, stream_id,
           L.ptr(keep_in), L.ptr(keep), L.ptr(xt), None)
    return xt, keep


def fold_dx(slabs, keep=None, p=0.0, dxh=None, B=1):
    """pkc_sru_dx on slabs (ns, T*B, n_in)."""
    ns, rows, n_in = slabs.shape
    dx = _z(rows, n_in)
    L.call("pkc_sru_dx", rows // B, B, n_in, L.ptr(slabs), ns, rows * n_in, L.ptr(keep), p,
           L.ptr(dxh), L.ptr(dx), None)
    return dx

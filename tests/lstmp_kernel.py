"""Kernel-level harness of the projected LSTM's time loops (pkc_lstmp_fwd / pkc_lstmp_bwd): a whole
layer stack through the C ABI, with the input projections and the weight-gradient matmuls — plain
matmuls over the T*B rows, outside the entry points under test — done by torch on the device."""
import ctypes as C

import torch

from pkc import _lib as L


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


class Layer:
    """One layer's buffers and the argument struct of both entry points."""

    def __init__(self, T, B, H, P, nd, train=True, drop_p=0.0, keep_in=None):
        self.T, self.B, self.H, self.P, self.nd = T, B, H, P, nd
        D = nd * P
        self.hs, self.cs = _z(nd, T + 1, B, P), _z(nd, T + 1, B, H)
        self.gates, self.ht = _z(nd, T, B, 4 * H), _z(nd, T, B, H)
        self.y = _z(T, B, D)
        self.keep = _z(T, B, D, dtype=torch.uint8)
        self.dgates, self.dhp = _z(nd, T, B, 4 * H), _z(nd, T, B, P)
        self.ut, self.wt, self.work = _z(nd, P, 4 * H), _z(nd, H, P), _z(nd, B, H)
        self.keep_in = keep_in
        a = L.LstmpArgs()
        a.T, a.B, a.H, a.P, a.ndir, a.train = T, B, H, P, nd, int(train)
        a.hs, a.cs, a.gates = self.hs.data_ptr(), self.cs.data_ptr(), self.gates.data_ptr()
        a.ht, a.y, a.keep = self.ht.data_ptr(), self.y.data_ptr(), self.keep.data_ptr()
        a.drop_p = drop_p
        a.keep_in = keep_in.data_ptr() if keep_in is not None else None
        a.dgates, a.dhp = self.dgates.data_ptr(), self.dhp.data_ptr()
        a.ut, a.wt, a.work = self.ut.data_ptr(), self.wt.data_ptr(), self.work.data_ptr()
        self.a = a

    def forward(self, wpre, U, bhh, Whr):
        """wpre[d] (T, B, 4H), U[d] (4H, P), bhh[d] (4H) or None, Whr[d] (P, H): contiguous fp32 on
        the device."""
        self.hold = (wpre, U, bhh, Whr)
        for d in range(self.nd):
            self.a.wpre[d], self.a.U[d] = wpre[d].data_ptr(), U[d].data_ptr()
            self.a.bhh[d] = bhh[d].data_ptr() if bhh[d] is not None else None
            self.a.Whr[d] = Whr[d].data_ptr()
        L.call("pkc_lstmp_fwd", C.byref(self.a), None)
        return self.y

    def backward(self, dy):
        self.dy = dy.contiguous()
        self.a.dy, self.a.dy_nslab, self.a.dy_slab_stride = self.dy.data_ptr(), 1, 0
        L.call("pkc_lstmp_bwd", C.byref(self.a), None)
        return self.dgates

    def dA(self, d):
        """(T*B, 4H) gradient of direction d's pre-activations."""
        return self.dgates[d].reshape(self.T * self.B, -1)

    def h_prev(self, d):
        """(T*B, P): h_{t-1} of every step of direction d, rows in natural time."""
        hs = self.hs[d]
        return (hs[1:] if d else hs[:-1]).reshape(self.T * self.B, self.P)


def run_stack(sd, prefix, x, r, layers, bidir, bias, train=True, drop_p=0.0, keep=None,
              backward=True):
    """Forward (and backward under loss = (y * r).sum()) of a layer stack with the state dict sd
    (torch's names under prefix).  Returns y, dx, {name: grad}, the layers."""
    T, B, _ = x.shape
    nd = 2 if bidir else 1
    P, H = sd[prefix + "weight_hr_l0"].shape
    p = lambda n, l, d: sd.get("%s%s_l%d%s" % (prefix, n, l, "_reverse" if d else ""))   # noqa: E731
    lays, xs = [], [x.contiguous()]
    for l in range(layers):
        last = l == layers - 1
        kin = keep[l] if (keep is not None and not last) else None
        lay = Layer(T, B, H, P, nd, train, 0.0 if last else drop_p, kin)
        x2 = xs[-1].reshape(T * B, -1)
        wpre = []
        for d in range(nd):
            w = x2 @ p("weight_ih", l, d).t()
            if bias:
                w = w + p("bias_ih", l, d)
            wpre.append(w.view(T, B, 4 * H).contiguous())
        y = lay.forward(wpre, [p("weight_hh", l, d).contiguous() for d in range(nd)],
                        [p("bias_hh", l, d) if bias else None for d in range(nd)],
                        [p("weight_hr", l, d).contiguous() for d in range(nd)])
        lays.append(lay)
        xs.append(y)
    torch.cuda.synchronize()
    if not backward:
        return xs[-1], None, None, lays
    grads, dy = {}, r
    for l in reversed(range(layers)):
        lay = lays[l]
        lay.backward(dy)
        x2 = xs[l].reshape(T * B, -1)
        dx = torch.zeros_like(x2)
        for d in range(nd):
            sfx = "_l%d%s" % (l, "_reverse" if d else "")
            dA = lay.dA(d)
            grads[prefix + "weight_ih" + sfx] = dA.t() @ x2
            grads[prefix + "weight_hh" + sfx] = dA.t() @ lay.h_prev(d)
            grads[prefix + "weight_hr" + sfx] = (lay.dhp[d].reshape(T * B, P).t()
                                                 @ lay.ht[d].reshape(T * B, H))
            if bias:
                grads[prefix + "bias_ih" + sfx] = dA.sum(0)
                grads[prefix + "bias_hh" + sfx] = dA.sum(0)
            dx = dx + dA @ p("weight_ih", l, d)
        dy = dx.view(T, B, -1)
    torch.cuda.synchronize()
    return xs[-1], dy, grads, lays

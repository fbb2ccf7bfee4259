"""Kernel-level harness of the standard-cell time loops (pkc_rnn_std_fwd / pkc_rnn_std_bwd): a whole
layer stack through the C ABI, with the input projections and the weight-gradient matmuls — plain
matmuls over the T*B rows, outside the entry points under test — done by torch on the device."""
import ctypes as C

import torch

from pkc import _lib as L

CELL = {"lstm": (L.STD_LSTM, 4), "gru": (L.STD_GRU, 3), "rnn": (L.STD_RNN, 1)}


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


class Layer:
    """One layer's buffers and the argument struct of both entry points."""

    def __init__(self, cell, T, B, H, nd, act="tanh", train=True, drop_p=0.0, keep_in=None):
        self.cell, self.T, self.B, self.H, self.nd = cell, T, B, H, nd
        cid, G = CELL[cell]
        self.G, self.GD = G, 4 if cell == "gru" else G
        D = nd * H
        self.hs, self.cs = _z(nd, T + 1, B, H), _z(nd, T + 1, B, H)
        self.gates, self.un = _z(nd, T, B, G * H), _z(nd, T, B, H)
        self.y = _z(T, B, D)
        self.keep = _z(T, B, D, dtype=torch.uint8)
        self.dgates = _z(nd, T, B, self.GD * H)
        self.ut, self.work = _z(nd, H, G * H), _z(nd, 2, B, H)
        self.keep_in = keep_in
        a = L.RnnStdArgs()
        a.cell, a.T, a.B, a.H, a.ndir = cid, T, B, H, nd
        a.act, a.train = L.ACT[act], int(train)
        a.hs, a.cs, a.gates = self.hs.data_ptr(), self.cs.data_ptr(), self.gates.data_ptr()
        a.un, a.y, a.keep = self.un.data_ptr(), self.y.data_ptr(), self.keep.data_ptr()
        a.drop_p = drop_p
        a.keep_in = keep_in.data_ptr() if keep_in is not None else None
        a.dgates, a.ut, a.work = self.dgates.data_ptr(), self.ut.data_ptr(), self.work.data_ptr()
        self.a = a

    def forward(self, wpre, U, bhh):
        """wpre[d] (T, B, G*H), U[d] (G*H, H), bhh[d] (G*H) or None, contiguous fp32 on the device."""
        self.hold = (wpre, U, bhh)
        for d in range(self.nd):
            self.a.wpre[d], self.a.U[d] = wpre[d].data_ptr(), U[d].data_ptr()
            self.a.bhh[d] = bhh[d].data_ptr() if bhh[d] is not None else None
        L.call("pkc_rnn_std_fwd", C.byref(self.a), None)
        return self.y

    def backward(self, dy):
        self.dy = dy.contiguous()
        self.a.dy, self.a.dy_nslab, self.a.dy_slab_stride = self.dy.data_ptr(), 1, 0
        L.call("pkc_rnn_std_bwd", C.byref(self.a), None)
        return self.dgates

    def dA(self, d):
        """(T*B, G*H) gradient of direction d's input-side pre-activations."""
        H, g = self.H, self.dgates[d].reshape(self.T * self.B, -1)
        return torch.cat([g[:, :2 * H], g[:, 3 * H:]], 1) if self.cell == "gru" else g

    def dR(self, d):
        """(T*B, G*H) gradient of direction d's recurrent-side pre-activations."""
        return self.dgates[d].reshape(self.T * self.B, -1)[:, :self.G * self.H]

    def h_prev(self, d):
        """(T*B, H): h_{t-1} of every step of direction d, rows in natural time."""
        hs = self.hs[d]
        return (hs[1:] if d else hs[:-1]).reshape(self.T * self.B, self.H)


def run_stack(cell, sd, prefix, x, r, layers, bidir, bias, act="tanh", train=True, drop_p=0.0,
              keep=None, backward=True):
    """Forward (and backward under loss = (y * r).sum()) of a layer stack with the state dict sd
    (torch's names under prefix).  Returns y, dx, {name: grad}."""
    T, B, _ = x.shape
    nd = 2 if bidir else 1
    G = CELL[cell][1]
    H = sd[prefix + "weight_hh_l0"].shape[1]
    p = lambda n, l, d: sd.get("%s%s_l%d%s" % (prefix, n, l, "_reverse" if d else ""))   # noqa: E731
    lays, xs = [], [x.contiguous()]
    for l in range(layers):
        last = l == layers - 1
        kin = keep[l] if (keep is not None and not last) else None
        lay = Layer(cell, T, B, H, nd, act, train, 0.0 if last else drop_p, kin)
        x2 = xs[-1].reshape(T * B, -1)
        wpre = []
        for d in range(nd):
            w = x2 @ p("weight_ih", l, d).t()
            if bias:
                w = w + p("bias_ih", l, d)
            wpre.append(w.view(T, B, G * H).contiguous())
        y = lay.forward(wpre, [p("weight_hh", l, d).contiguous() for d in range(nd)],
                        [p("bias_hh", l, d) if bias else None for d in range(nd)])
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
            dA, dR = lay.dA(d), lay.dR(d)
            grads[prefix + "weight_ih" + sfx] = dA.t() @ x2
            grads[prefix + "weight_hh" + sfx] = dR.t() @ lay.h_prev(d)
            if bias:
                grads[prefix + "bias_ih" + sfx] = dA.sum(0)
                grads[prefix + "bias_hh" + sfx] = dR.sum(0)
            dx = dx + dA @ p("weight_ih", l, d)
        dy = dx.view(T, B, -1)
    torch.cuda.synchronize()
    return xs[-1], dy, grads, lays

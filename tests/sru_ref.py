"""Plain-torch restatement of the Simple Recurrent Unit as pkc runs it (Lei et al., "Simple Recurrent
Units for Highly Parallelizable Recurrence", EMNLP 2018: the v2 cell with the highway scaling alpha;
the contract of include/pkc.h, pkc_sru_args): sequential over time, float64 or float32, with autograd
and injected dropout masks.  It is what the GPU path is compared with; nothing pins it to another
implementation (the reference's SRU class is commented out), so it restates the equations only.

Per layer, X (T, B, n_in), n_out = D * d, column j of direction j // d (direction 1 walks
t = T-1 .. 0), k = 4 when the skip term is on and n_in != n_out, else 3:
  U = (X * m_x) @ weight,  u_g = U[t, b, j * k + g]
  f = sig(u1 + v_f c_{t-1} + b_f),  r = sig(u2 + v_r c_{t-1} + b_r),  c = f c_{t-1} + (1 - f) u0
  x' = u3 (k = 4) | alpha X[t, b, j] (k = 3, skip; the UNdropped input) | 0 (no skip term)
  h = r g(c) m_c + (1 - r) x'
m_x (B, n_in) and m_c (B, n_out) are keep / (1 - p), one mask for all t, in training only.
"""
import math

import torch
import torch.nn as nn


def _b(v):
    return str(v).strip().lower() in ("true", "1", "yes", "y", "t", "on")


def g_act(act, c):
    return torch.tanh(c) if act == "tanh" else torch.relu(c) if act == "relu" else c


def g_grad(act, c):
    if act == "tanh":
        return 1 - torch.tanh(c) ** 2
    return (c > 0).to(c.dtype) if act == "relu" else torch.ones_like(c)


def cell_fwd(U, X, wc, bias, d, D, k, act="linear", skip=True, alpha=1.0, m_c=None):
    """The recurrence of one layer on a given projection U (T, B, n_out*k); X: the layer's input
    (read for the k = 3 skip term only).  Returns y, c, both (T, B, n_out)."""
    T, B, _ = U.shape
    n = d * D
    u = U.view(T, B, n, k)
    vf, vr, bf, br = wc[:n], wc[n:], bias[:n], bias[n:]
    mc = m_c if m_c is not None else torch.ones(B, n, dtype=U.dtype, device=U.device)
    ys, cs = [], []
    for dd in range(D):
        sl = slice(dd * d, (dd + 1) * d)
        c = U.new_zeros(B, d)
        yd, cd = [None] * T, [None] * T
        for t in (range(T - 1, -1, -1) if dd else range(T)):
            f = torch.sigmoid(u[t, :, sl, 1] + vf[sl] * c + bf[sl])
            r = torch.sigmoid(u[t, :, sl, 2] + vr[sl] * c + br[sl])
            c = f * c + (1 - f) * u[t, :, sl, 0]
            if k == 4:
                xp = u[t, :, sl, 3]
            elif skip:
                xp = alpha * X[t, :, sl]
            else:
                xp = torch.zeros_like(c)
            yd[t] = r * g_act(act, c) * mc[:, sl] + (1 - r) * xp
            cd[t] = c
        ys.append(torch.stack(yd))
        cs.append(torch.stack(cd))
    return torch.cat(ys, -1), torch.cat(cs, -1)


def cell_bwd(U, X, wc, bias, cs, dy, d, D, k, act="linear", skip=True, alpha=1.0, m_c=None):
    """The hand-written backward of cell_fwd (the formulas of the kernel), gates recomputed from U
    and the saved c.  Returns dU, dXh (the k = 3 skip gradient, else None), dwc, dbias."""
    T, B, _ = U.shape
    n = d * D
    u = U.view(T, B, n, k)
    vf, vr, bf, br = wc[:n], wc[n:], bias[:n], bias[n:]
    mc = m_c if m_c is not None else torch.ones(B, n, dtype=U.dtype, device=U.device)
    dU = torch.zeros_like(u)
    hw = k == 3 and skip
    dXh = torch.zeros(T, B, n, dtype=U.dtype, device=U.device) if hw else None
    dwc, dbias = torch.zeros_like(wc), torch.zeros_like(bias)
    for dd in range(D):
        sl = slice(dd * d, (dd + 1) * d)
        order = list(range(T - 1, -1, -1) if dd else range(T))
        dc = U.new_zeros(B, d)
        for s in range(T - 1, -1, -1):
            t = order[s]
            cp = cs[order[s - 1], :, sl] if s > 0 else U.new_zeros(B, d)
            c = cs[t, :, sl]
            f = torch.sigmoid(u[t, :, sl, 1] + vf[sl] * cp + bf[sl])
            r = torch.sigmoid(u[t, :, sl, 2] + vr[sl] * cp + br[sl])
            xp = u[t, :, sl, 3] if k == 4 else (alpha * X[t, :, sl] if skip else torch.zeros_like(c))
            dh = dy[t, :, sl]
            dr = dh * (g_act(act, c) * mc[:, sl] - xp)
            dxp = dh * (1 - r)
            dc = dc + dh * r * mc[:, sl] * g_grad(act, c)
            daf = dc * (cp - u[t, :, sl, 0]) * f * (1 - f)
            dar = dr * r * (1 - r)
            dU[t, :, sl, 0] = dc * (1 - f)
            dU[t, :, sl, 1] = daf
            dU[t, :, sl, 2] = dar
            if k == 4:
                dU[t, :, sl, 3] = dxp
            elif hw:
                dXh[t, :, sl] = alpha * dxp
            dwc[sl] += (daf * cp).sum(0)
            dwc[n + dd * d:n + (dd + 1) * d] += (dar * cp).sum(0)
            dbias[sl] += daf.sum(0)
            dbias[n + dd * d:n + (dd + 1) * d] += dar.sum(0)
            dc = dc * f + daf * vf[sl] + dar * vr[sl]
    return dU.view(T, B, n * k), dXh, dwc, dbias


class Cell(nn.Module):
    def __init__(self, n_in, n_out, k, rescale, highway_bias):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n_in, n_out * k))
        self.weight_c = nn.Parameter(torch.empty(2 * n_out))
        self.bias = nn.Parameter(torch.zeros(2 * n_out))
        nn.init.uniform_(self.weight, -math.sqrt(3.0 / n_in), math.sqrt(3.0 / n_in))
        nn.init.uniform_(self.weight_c, -math.sqrt(3.0), math.sqrt(3.0))
        with torch.no_grad():
            if rescale:
                self.weight_c.mul_(math.sqrt(0.5))
            self.bias[n_out:].fill_(highway_bias)


class Holder(nn.Module):
    def __init__(self, cells):
        super().__init__()
        self.rnn_lst = nn.ModuleList(cells)


class SRU(nn.Module):
    """The architecture: parameters sru.rnn_lst.<l>.{weight, weight_c, bias}, pkc's own draws."""

    proj = None         # hook of the bf16-operand oracle: proj(x2, weight) -> x2 @ weight

    def __init__(self, options, inp_dim):
        super().__init__()
        o = options
        self.d = int(o["sru_hidden_size"])
        self.num_layers = int(o["sru_num_layers"])
        self.dropout, self.rnn_dropout = float(o["sru_dropout"]), float(o["sru_rnn_dropout"])
        self.act = "tanh" if _b(o["sru_use_tanh"]) else "relu" if _b(o["sru_use_relu"]) else "linear"
        self.D = 2 if _b(o["sru_bidirectional"]) else 1
        self.skip, self.rescale = _b(o["sru_has_skip_term"]), _b(o["sru_rescale"])
        self.highway_bias = float(o["sru_highway_bias"])
        self.alpha = math.sqrt(1 + 2 * math.exp(self.highway_bias)) if (self.rescale and self.skip) else 1.0
        self.out_dim = self.d * self.D
        cells, n_in = [], inp_dim
        for _ in range(self.num_layers):
            k = 4 if (self.skip and n_in != self.out_dim) else 3
            cells.append(Cell(n_in, self.out_dim, k, self.rescale, self.highway_bias))
            n_in = self.out_dim
        self.sru = Holder(cells)

    def forward(self, x, masks=None):
        """x (T, B, F).  masks (training): {(l, "c"): keep (B, n_out), (l, "x"): keep (B, n_in)} of
        {0, 1}; a missing one is drawn with torch.bernoulli."""
        T, B, _ = x.shape
        for l, cell in enumerate(self.sru.rnn_lst):
            k = cell.weight.shape[1] // self.out_dim

            def scale(key, p, width):
                if not (self.training and p > 0):
                    return None
                keep = masks[key] if (masks is not None and key in masks) else torch.bernoulli(
                    torch.full((B, width), 1 - p))
                return keep.to(x.dtype).to(x.device) / (1 - p)
            mx, mc = scale((l, "x"), self.rnn_dropout, x.shape[2]), scale((l, "c"), self.dropout,
                                                                        self.out_dim)
            xt = x * mx if mx is not None else x
            x2 = xt.reshape(T * B, -1)
            U = (self.proj(x2, cell.weight) if self.proj is not None else x2 @ cell.weight)
            x, _ = cell_fwd(U.view(T, B, -1), x, cell.weight_c, cell.bias, self.d, self.D, k, self.act,
                            self.skip, self.alpha, mc)
        return x

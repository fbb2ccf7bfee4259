"""Plain-torch restatement of the projected LSTM (LSTMP; Sak et al., Interspeech 2014), i.e. of
torch.nn.LSTM(input, H, num_layers, bias, dropout, bidirectional, proj_size=P) with a zero initial
state and 0 < P < H: explicit loops over layers, directions and time in the cell's formulas, with
explicit inter-layer dropout masks, in the style of tests/cudnn_ref.py.  It is what the GPU path of
LSTM_cudnn with proj_size = P is compared with (tests/test_lstmp_cpu.py checks it against torch.nn.LSTM
itself and against the golden torch.nn.LSTM wrote, tests/golden/lstmp.npz).

Parameters carry torch's names, shapes, registration order and init draws (lstm.0.weight_ih_l0
(4H, K), weight_hh_l0 (4H, P), bias_ih_l0, bias_hh_l0, weight_hr_l0 (P, H), ..._l0_reverse, ..._l1,
...; K = the input width for layer 0 and ndir * P above; every tensor U(+-1/sqrt(H)) in that order),
so state dicts go both ways.  Cell (gate rows i,f,g,o; a = W_ih x + b_ih, u = W_hh h_{t-1} + b_hh):
  c = sig(f) c + sig(i) tanh(g),  ht = sig(o) tanh(c)  (H wide),  h = W_hr ht  (P wide, no bias)
h is both the layer output and the recurrent state; a bidirectional layer's output is
[h_fwd, h_bwd], 2P wide.  Dropout: in training with p > 0 the output of every layer but the last is
multiplied by keep / (1 - p); keep[l] (T, B, ndir * P) of {0, 1} is given by the caller or drawn with
torch.bernoulli.
"""
import math

import torch
import torch.nn as nn


def _b(v):
    return str(v).strip().lower() in ("true", "1", "yes", "y", "t", "on")


class Packed(nn.Module):
    """The parameters of a torch.nn.LSTM(proj_size=P) as plain Parameters under torch's names."""

    def __init__(self, inp, H, P, layers, bias, bidir):
        super().__init__()
        nd = 2 if bidir else 1
        for l in range(layers):
            K = inp if l == 0 else P * nd
            for d in range(nd):
                sfx = "_l%d%s" % (l, "_reverse" if d else "")
                self.register_parameter("weight_ih" + sfx, nn.Parameter(torch.empty(4 * H, K)))
                self.register_parameter("weight_hh" + sfx, nn.Parameter(torch.empty(4 * H, P)))
                if bias:
                    self.register_parameter("bias_ih" + sfx, nn.Parameter(torch.empty(4 * H)))
                    self.register_parameter("bias_hh" + sfx, nn.Parameter(torch.empty(4 * H)))
                self.register_parameter("weight_hr" + sfx, nn.Parameter(torch.empty(P, H)))
        stdv = 1.0 / math.sqrt(H)
        for p in self.parameters():              # nn.RNNBase.reset_parameters: the same draws
            nn.init.uniform_(p, -stdv, stdv)


class LSTMP(nn.Module):
    cell = "lstm"

    def __init__(self, options, inp_dim):
        super().__init__()
        o = options
        self.input_dim = inp_dim
        self.hidden_size = int(o["hidden_size"])
        self.proj_size = int(o["proj_size"])
        assert 0 < self.proj_size < self.hidden_size
        self.num_layers = int(o["num_layers"])
        self.bias = _b(o["bias"])
        self.dropout = float(o["dropout"])
        self.bidirectional = _b(o["bidirectional"])
        self.lstm = nn.ModuleList([Packed(inp_dim, self.hidden_size, self.proj_size, self.num_layers,
                                          self.bias, self.bidirectional)])
        self.out_dim = self.proj_size * (2 if self.bidirectional else 1)

    def _p(self, name, l, d):
        return getattr(self.lstm[0], "%s_l%d%s" % (name, l, "_reverse" if d else ""), None)

    # hooks of the bf16-operand oracle (tests): proj(x2, W_ih, b_ih) for the input projection,
    # recur(h, W_hh) for the recurrent product and hproj(ht, W_hr) for the ht -> h product (the
    # last two: exact forward and data gradient, weight gradient on bf16-rounded operands), all
    # autograd Functions; None: plain fp matmuls
    proj = None
    recur = None
    hproj = None

    def _direction(self, x, l, d):
        T, B, _ = x.shape
        H, P = self.hidden_size, self.proj_size
        Wi, Wh, Wr = self._p("weight_ih", l, d), self._p("weight_hh", l, d), self._p("weight_hr", l, d)
        bi, bh = self._p("bias_ih", l, d), self._p("bias_hh", l, d)
        if self.proj is not None:
            a_all = self.proj(x.reshape(T * B, -1), Wi, bi).view(T, B, -1)
        else:
            a_all = (x.reshape(T * B, -1) @ Wi.t()).view(T, B, -1)
            if bi is not None:
                a_all = a_all + bi
        h = x.new_zeros(B, P)
        c = x.new_zeros(B, H)
        ys = [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            u = self.recur(h, Wh) if self.recur is not None else h @ Wh.t()
            if bh is not None:
                u = u + bh
            s = a_all[t] + u
            i, f = torch.sigmoid(s[:, :H]), torch.sigmoid(s[:, H:2 * H])
            g, og = torch.tanh(s[:, 2 * H:3 * H]), torch.sigmoid(s[:, 3 * H:])
            c = f * c + i * g
            ht = og * torch.tanh(c)
            h = self.hproj(ht, Wr) if self.hproj is not None else ht @ Wr.t()
            ys[t] = h
        return torch.stack(ys)

    def forward(self, x, keep=None):
        """x (T, B, F); keep: {layer: (T, B, ndir * P) mask} for the layers below the last
        (training)."""
        nd = 2 if self.bidirectional else 1
        for l in range(self.num_layers):
            x = torch.cat([self._direction(x, l, d) for d in range(nd)], dim=-1)
            if self.training and self.dropout > 0 and l < self.num_layers - 1:
                k = keep[l] if keep is not None else torch.bernoulli(
                    torch.full_like(x, 1 - self.dropout))
                x = x * k.to(x.dtype) / (1 - self.dropout)
        return x


def LSTM_cudnn(options, inp_dim):
    return LSTMP(options, inp_dim)


def torch_module(net):
    """The torch.nn.LSTM(proj_size=P) with net's parameters (for the CPU cross-check)."""
    m = nn.LSTM(net.input_dim, net.hidden_size, num_layers=net.num_layers, bias=net.bias, dropout=0.0,
                bidirectional=net.bidirectional, proj_size=net.proj_size)
    m.load_state_dict(net.lstm[0].state_dict(), strict=True)
    return m

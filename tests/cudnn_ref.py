"""Plain-torch restatement of the reference's LSTM_cudnn / GRU_cudnn / RNN_cudnn
(neural_networks.py:364-465, i.e. torch.nn.LSTM / GRU / RNN with a zero initial state): explicit loops
over layers, directions and time in the cells' formulas, with explicit inter-layer dropout masks.
It is what the GPU path is compared with (tests/test_cudnn_cpu.py checks it against torch.nn itself
and against the golden recorded from the reference).

Parameters carry torch's names, shapes, registration order and init draws
(<lstm|gru|rnn>.0.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, ..._l0_reverse, ..._l1, ...), so
state dicts go both ways.  Cells (a = W_ih x + b_ih, u = W_hh h_{t-1} + b_hh):
  LSTM  rows i,f,g,o: c = sig(f) c + sig(i) tanh(g), h = sig(o) tanh(c)
  GRU   rows r,z,n:   r, z = sig(a + u); n = tanh(a_n + r * u_n); h = (1 - z) n + z h_{t-1}
  RNN   h = act(a + u), act tanh or relu
Dropout: in training with p > 0 the output of every layer but the last is multiplied by
keep / (1 - p); keep[l] (T, B, D) of {0, 1} is given by the caller or drawn with torch.bernoulli.
"""
import math

import torch
import torch.nn as nn

GATES = {"lstm": 4, "gru": 3, "rnn": 1}


def _b(v):
    return str(v).strip().lower() in ("true", "1", "yes", "y", "t", "on")


class Packed(nn.Module):
    """The parameters of a torch.nn.LSTM / GRU / RNN as plain Parameters under torch's names."""

    def __init__(self, G, inp, H, layers, bias, bidir):
        super().__init__()
        nd = 2 if bidir else 1
        for l in range(layers):
            K = inp if l == 0 else H * nd
            for d in range(nd):
                sfx = "_l%d%s" % (l, "_reverse" if d else "")
                self.register_parameter("weight_ih" + sfx, nn.Parameter(torch.empty(G * H, K)))
                self.register_parameter("weight_hh" + sfx, nn.Parameter(torch.empty(G * H, H)))
                if bias:
                    self.register_parameter("bias_ih" + sfx, nn.Parameter(torch.empty(G * H)))
                    self.register_parameter("bias_hh" + sfx, nn.Parameter(torch.empty(G * H)))
        stdv = 1.0 / math.sqrt(H)
        for p in self.parameters():              # nn.RNNBase.reset_parameters: the same draws
            nn.init.uniform_(p, -stdv, stdv)


class StdRec(nn.Module):
    def __init__(self, cell, options, inp_dim):
        super().__init__()
        o = options
        self.cell = cell
        self.input_dim = inp_dim
        self.hidden_size = int(o["hidden_size"])
        self.num_layers = int(o["num_layers"])
        self.bias = _b(o["bias"])
        self.dropout = float(o["dropout"])
        self.bidirectional = _b(o["bidirectional"])
        self.nonlinearity = o.get("nonlinearity", "tanh")
        setattr(self, cell, nn.ModuleList([Packed(GATES[cell], inp_dim, self.hidden_size,
                                                  self.num_layers, self.bias, self.bidirectional)]))
        self.out_dim = self.hidden_size * (2 if self.bidirectional else 1)

    def _p(self, name, l, d):
        return getattr(getattr(self, self.cell)[0], "%s_l%d%s" % (name, l, "_reverse" if d else ""),
                       None)

    # hooks of the bf16-operand oracle (tests): proj(x2, W_ih, b_ih) for the input projection and
    # recur(h, W_hh) for the recurrent product, both autograd Functions; None: plain fp matmuls
    proj = None
    recur = None

    def _direction(self, x, l, d):
        T, B, _ = x.shape
        H = self.hidden_size
        Wi, Wh = self._p("weight_ih", l, d), self._p("weight_hh", l, d)
        bi, bh = self._p("bias_ih", l, d), self._p("bias_hh", l, d)
        if self.proj is not None:
            a_all = self.proj(x.reshape(T * B, -1), Wi, bi).view(T, B, -1)
        else:
            a_all = (x.reshape(T * B, -1) @ Wi.t()).view(T, B, -1)
            if bi is not None:
                a_all = a_all + bi
        h = x.new_zeros(B, H)
        c = x.new_zeros(B, H)
        ys = [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            a = a_all[t]
            u = self.recur(h, Wh) if self.recur is not None else h @ Wh.t()
            if bh is not None:
                u = u + bh
            if self.cell == "lstm":
                s = a + u
                i, f = torch.sigmoid(s[:, :H]), torch.sigmoid(s[:, H:2 * H])
                g, og = torch.tanh(s[:, 2 * H:3 * H]), torch.sigmoid(s[:, 3 * H:])
                c = f * c + i * g
                h = og * torch.tanh(c)
            elif self.cell == "gru":
                r = torch.sigmoid(a[:, :H] + u[:, :H])
                z = torch.sigmoid(a[:, H:2 * H] + u[:, H:2 * H])
                n = torch.tanh(a[:, 2 * H:] + r * u[:, 2 * H:])
                h = (1 - z) * n + z * h
            else:
                s = a + u
                h = torch.tanh(s) if self.nonlinearity == "tanh" else torch.relu(s)
            ys[t] = h
        return torch.stack(ys)

    def forward(self, x, keep=None):
        """x (T, B, F); keep: {layer: (T, B, D) mask} for the layers below the last (training)."""
        nd = 2 if self.bidirectional else 1
        for l in range(self.num_layers):
            x = torch.cat([self._direction(x, l, d) for d in range(nd)], dim=-1)
            if self.training and self.dropout > 0 and l < self.num_layers - 1:
                k = keep[l] if keep is not None else torch.bernoulli(
                    torch.full_like(x, 1 - self.dropout))
                x = x * k.to(x.dtype) / (1 - self.dropout)
        return x


def LSTM_cudnn(options, inp_dim):
    return StdRec("lstm", options, inp_dim)


def GRU_cudnn(options, inp_dim):
    return StdRec("gru", options, inp_dim)


def RNN_cudnn(options, inp_dim):
    return StdRec("rnn", options, inp_dim)


def torch_module(net):
    """The torch.nn.LSTM / GRU / RNN with net's parameters (for the CPU cross-check)."""
    kw = dict(num_layers=net.num_layers, bias=net.bias, dropout=0.0,
              bidirectional=net.bidirectional)
    if net.cell == "rnn":
        kw["nonlinearity"] = net.nonlinearity
    m = {"lstm": nn.LSTM, "gru": nn.GRU, "rnn": nn.RNN}[net.cell](net.input_dim, net.hidden_size, **kw)
    m.load_state_dict(getattr(net, net.cell)[0].state_dict())
    return m

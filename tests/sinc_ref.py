"""CPU restatement of the reference SincNet (neural_networks.py:2036-2143) and of its SincConv
filter bank (:2146-2283) with torch, against a state dict, in the manner of tests/cnn_ref.py.

Not the reference's code: the same computation, so the tests can run it in fp64, inject dropout
masks and look at the pooling windows and the generated filters.

  layers 1.. : CNN's (cnn_ref.py) with sinc_* option names
  layer 0    : conv1d with the (N, 1, K) filters below, no bias; K = len, or len + 1 when len is
               even (:2193-2194), while ln[0] / bn[0] are sized with len as configured (:2094)
  filters    : low = min_low_hz / sr + |low_hz_|, high = low + min_band_hz / sr + |band_hz_|,
               lp(f) = 2 f sinc(2 pi (f n_) sr) with sinc = sin(x) / x on the left half, 1 at the
               centre and the right half the flip of the left, bp = lp(high) - lp(low),
               filters = bp / max_k bp * window_
  n_, window_: plain fp32 attributes of the module (:2226-2232), not parameters: computed here
               in fp32 by the same expressions and cast, so the fp64 run is "the same constants,
               exact arithmetic" (what the reference's own module gives after .double())

In fp32 the filters equal the reference's conv[0].filters bit for bit (tests/golden/sinc.npz).
"""
import math

import torch
import torch.nn.functional as F

import cnn_ref
from cnn_ref import _lst, strtobool


def odd_len(length):
    return length + 1 if length % 2 == 0 else length


def sinc_consts(K, sr):
    """(n_ (1, K), window_ (K)) in fp32 (neural_networks.py:2226-2232)."""
    n_lin = torch.linspace(0, K, steps=K)
    window = 0.54 - 0.46 * torch.cos(2 * math.pi * n_lin / K)
    n = (K - 1) / 2
    return torch.arange(-n, n + 1).view(1, -1) / sr, window


def sinc_filters(low_hz_, band_hz_, K, sr, min_low_hz, min_band_hz, parts=None):
    """(N, K) filters in the dtype of low_hz_ (N, 1) (neural_networks.py:2261-2279).
    parts: a dict that receives band_pass before the normalisation and max_."""
    n_, window = sinc_consts(K, sr)
    n_, window = n_.to(low_hz_), window.to(low_hz_)            # its dtype and device

    def sinc(x):
        left = x[:, 0:int((x.shape[1] - 1) / 2)]
        y = torch.sin(left) / left
        one = torch.ones([x.shape[0], 1], dtype=x.dtype, device=x.device)
        return torch.cat([y, one, torch.flip(y, dims=[1])], 1)

    low = min_low_hz / sr + torch.abs(low_hz_)
    high = low + min_band_hz / sr + torch.abs(band_hz_)
    lp1 = 2 * low * sinc(2 * math.pi * torch.matmul(low, n_) * sr)
    lp2 = 2 * high * sinc(2 * math.pi * torch.matmul(high, n_) * sr)
    bp = lp2 - lp1
    mx, idx = torch.max(bp, dim=1, keepdim=True)
    if parts is not None:
        parts.update(bp=bp.detach(), max_=mx.detach(), idx=idx.detach())
    return bp / mx * window


def mel_init(N, sr, min_low_hz, min_band_hz):
    """Initial (low_hz_, band_hz_), each (N, 1) fp32 (neural_networks.py:2210-2222)."""
    import numpy as np
    to_mel = lambda hz: 2595 * np.log10(1 + hz / 700)           # noqa: E731
    to_hz = lambda mel: 700 * (10 ** (mel / 2595) - 1)          # noqa: E731
    hz = to_hz(np.linspace(to_mel(30), to_mel(sr / 2 - (min_low_hz + min_band_hz)), N + 1)) / sr
    return (torch.tensor(hz[:-1], dtype=torch.float32).view(-1, 1),
            torch.tensor(np.diff(hz), dtype=torch.float32).view(-1, 1))


def geometry(opts, inp_dim):
    """[(C_in, C_out, taps, pool, L_in, L_out)] per layer (neural_networks.py:2079-2110): taps is
    the convolution's length (layer 0: made odd), L_out the size the reference gives the norms."""
    nf, lf, mp = _lst(opts, "sinc_N_filt", int), _lst(opts, "sinc_len_filt", int), \
        _lst(opts, "sinc_max_pool_len", int)
    out, cur, cin = [], inp_dim, 1
    for i in range(len(nf)):
        lo = int((cur - lf[i] + 1) / mp[i])
        out.append((cin, nf[i], odd_len(lf[i]) if i == 0 else lf[i], mp[i], cur, lo))
        cur, cin = lo, nf[i]
    return out


def _sinc_opts(opts):
    return int(opts["sinc_sample_rate"]), int(opts["sinc_min_low_hz"]), int(opts["sinc_min_band_hz"])


def sincnet_forward(sd, opts, x, train=True, keep=None, gaps=None, parts=None):
    """The reference forward from a state dict sd (name -> tensor; running statistics are updated
    in place in training mode).  keep / gaps: as cnn_ref.cnn_forward.  parts: a dict that receives
    layer 0's filters (and sinc_filters' parts)."""
    B, inp = x.shape
    geo = geometry(opts, inp)
    sr, min_low, min_band = _sinc_opts(opts)
    acts, drops = _lst(opts, "sinc_act"), _lst(opts, "sinc_drop", float)
    use_ln = _lst(opts, "sinc_use_laynorm", strtobool)
    use_bn = _lst(opts, "sinc_use_batchnorm", strtobool)
    if strtobool(opts["sinc_use_laynorm_inp"]):
        x = cnn_ref.layer_norm(x, sd["ln0.gamma"], sd["ln0.beta"])
    if strtobool(opts["sinc_use_batchnorm_inp"]):
        x = F.batch_norm(x, sd["bn0.running_mean"], sd["bn0.running_var"], sd["bn0.weight"],
                         sd["bn0.bias"], train, 0.05, 1e-5)
    x = x.view(B, 1, inp)
    for i, (cin, cout, taps, pool, Li, Lo) in enumerate(geo):
        if use_ln[i] and use_bn[i]:
            raise NotImplementedError("layer %d: LN and BN both set (two convolutions)" % i)
        if i == 0:
            filt = sinc_filters(sd["conv.0.low_hz_"], sd["conv.0.band_hz_"], taps, sr, min_low,
                                min_band, parts)
            if parts is not None:
                parts["filters"] = filt.detach()
            c = F.conv1d(x, filt.view(cout, 1, taps))
        else:
            c = F.conv1d(x, sd["conv.%d.weight" % i], sd["conv.%d.bias" % i])
        if gaps is not None:
            gaps.append(cnn_ref.window_gaps(c.detach(), pool))
        z = F.max_pool1d(c, pool)
        if use_ln[i]:
            z = cnn_ref.layer_norm(z, sd["ln.%d.gamma" % i], sd["ln.%d.beta" % i])
        elif use_bn[i]:
            z = F.batch_norm(z, sd["bn.%d.running_mean" % i], sd["bn.%d.running_var" % i],
                             sd["bn.%d.weight" % i], sd["bn.%d.bias" % i], train, 0.05, float(Lo))
        z = cnn_ref.act(acts[i], z)
        if train and drops[i] > 0:
            if keep is None or keep[i] is None:
                raise ValueError("layer %d has dropout: pass its keep mask" % i)
            z = z * keep[i].to(z.dtype) / (1.0 - drops[i])
        x = z
    return x.reshape(B, -1)


leaf_state = cnn_ref.leaf_state


class _Sinc(torch.nn.Module):
    def __init__(self, N, sr, min_low_hz, min_band_hz):
        super().__init__()
        low, band = mel_init(N, sr, min_low_hz, min_band_hz)
        self.low_hz_, self.band_hz_ = torch.nn.Parameter(low), torch.nn.Parameter(band)


class RefSincNet(torch.nn.Module):
    """sincnet_forward behind the reference's module interface (same state-dict keys and order),
    so the oracle's training loop (oracle/run.py) and torch.optim can drive it."""

    def __init__(self, options, inp_dim, dtype=torch.float32):
        super().__init__()
        self.opts, self.keep, self.gaps, self.parts = options, None, None, None
        self.skip_regularization = strtobool(options.get("skip_regularization", "False"))
        nn = torch.nn
        self.conv, self.bn, self.ln = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        if strtobool(options["sinc_use_laynorm_inp"]):
            self.ln0 = cnn_ref._LN(inp_dim)
        if strtobool(options["sinc_use_batchnorm_inp"]):
            self.bn0 = nn.BatchNorm1d(inp_dim, momentum=0.05)
        geo = geometry(options, inp_dim)
        for i, (cin, cout, taps, pool, Li, Lo) in enumerate(geo):
            self.ln.append(cnn_ref._LN([cout, Lo]))
            self.bn.append(nn.BatchNorm1d(cout, eps=Lo, momentum=0.05))
            self.conv.append(_Sinc(cout, *_sinc_opts(options)) if i == 0
                             else nn.Conv1d(cin, cout, taps))
        self.out_dim = geo[-1][5] * geo[-1][1]
        self.to(dtype)

    def forward(self, x):
        sd = self.state_dict(keep_vars=True)
        if self.training:
            for k, v in sd.items():
                used = (k.startswith("bn0.") or
                        (k.startswith("bn.") and _lst(self.opts, "sinc_use_batchnorm",
                                                      strtobool)[int(k.split(".")[1])]))
                if k.endswith("num_batches_tracked") and used:
                    v.add_(1)
        return sincnet_forward(sd, self.opts, x, train=self.training, keep=self.keep,
                               gaps=self.gaps, parts=self.parts)

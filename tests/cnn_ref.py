"""CPU restatement of the reference CNN (neural_networks.py:1934-2033) with torch.nn.functional.

Not the reference's code: the same computation written against a state dict, so the tests can run
it in fp64, inject dropout masks and look at the pooling windows.

  per layer (neural_networks.py:2017-2029): x = drop(act(norm(max_pool1d(conv(x), pool))))
  conv   : nn.Conv1d(C_in, C_out, len): stride 1, no padding, bias (:1992-1997)
  pool   : F.max_pool1d(., pool): stride = kernel, floor mode, first maximal index on ties
  LN     : the reference's own LayerNorm (:40-51) over the LAST dimension (L_out) of (B, C, L):
           gamma * (x - mean) / (std + 1e-6) + beta, unbiased std, gamma / beta of shape (C, L)
  BN     : nn.BatchNorm1d(N_filt, <L_out>, momentum=0.05) (:1988-1990): the second positional
           argument is eps, so eps = L_out
  output : x.view(batch, -1) (:2031), channel-major
"""
import torch
import torch.nn.functional as F


def strtobool(v):
    return str(v).strip().lower() in ("y", "yes", "t", "true", "on", "1")


def _lst(o, k, f=str):
    return [f(v) for v in o[k].split(",")]


def geometry(opts, inp_dim):
    """[(C_in, C_out, len, pool, L_in, L_out)] per layer (neural_networks.py:1971-2002)."""
    nf, lf, mp = _lst(opts, "cnn_N_filt", int), _lst(opts, "cnn_len_filt", int), \
        _lst(opts, "cnn_max_pool_len", int)
    out, cur, cin = [], inp_dim, 1
    for i in range(len(nf)):
        lo = int((cur - lf[i] + 1) / mp[i])
        out.append((cin, nf[i], lf[i], mp[i], cur, lo))
        cur, cin = lo, nf[i]
    return out


def act(name, x):
    """act_fun (neural_networks.py:54-78)."""
    if name == "relu":
        return torch.relu(x)
    if name == "tanh":
        return torch.tanh(x)
    if name == "htanh":
        return F.hardtanh(x)
    if name == "sigmoid":
        return torch.sigmoid(x)
    if name == "leaky_relu":
        return F.leaky_relu(x, 0.2)
    if name == "elu":
        return F.elu(x)
    if name == "linear":
        return x
    raise ValueError(name)


def layer_norm(x, gamma, beta, eps=1e-6):
    """neural_networks.py:48-51."""
    mean = x.mean(-1, keepdim=True)
    std = x.std(-1, keepdim=True)
    return gamma * (x - mean) / (std + eps) + beta


def conv_pool(x, W, b, pool):
    """max_pool1d(conv1d(x)) -> (z (B, C, L_out), first-max offset inside each window (uint8))."""
    c = F.conv1d(x, W, b)
    z, idx = F.max_pool1d(c, pool, return_indices=True)
    off = idx - torch.arange(z.shape[-1], device=idx.device) * pool
    return z, off.to(torch.uint8)


def window_gaps(c, pool):
    """Per pooling window of the conv output c (B, C, L_conv): (top1 - top2) / max |window|
    (inf where pool == 1)."""
    Lo = c.shape[-1] // pool
    w = c[..., :Lo * pool].reshape(c.shape[0], c.shape[1], Lo, pool)
    if pool == 1:
        return torch.full(w.shape[:-1], float("inf"), dtype=c.dtype)
    top = w.topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]) / w.abs().amax(-1).clamp_min(1e-30)


def cnn_forward(sd, opts, x, train=True, keep=None, gaps=None):
    """The reference forward from a state dict sd (name -> tensor; running statistics are updated
    in place in training mode).  keep: optional per-layer list of (B, C, L_out) 0/1 dropout masks
    (None entries / p == 0: no dropout); without it a layer with cnn_drop > 0 in training raises.
    gaps: a list that receives each layer's window_gaps."""
    B, inp = x.shape
    geo = geometry(opts, inp)
    acts, drops = _lst(opts, "cnn_act"), _lst(opts, "cnn_drop", float)
    use_ln, use_bn = _lst(opts, "cnn_use_laynorm", strtobool), _lst(opts, "cnn_use_batchnorm", strtobool)
    if strtobool(opts["cnn_use_laynorm_inp"]):
        x = layer_norm(x, sd["ln0.gamma"], sd["ln0.beta"])
    if strtobool(opts["cnn_use_batchnorm_inp"]):
        x = F.batch_norm(x, sd["bn0.running_mean"], sd["bn0.running_var"], sd["bn0.weight"],
                         sd["bn0.bias"], train, 0.05, 1e-5)
    x = x.view(B, 1, inp)
    for i, (cin, cout, ln_, pool, Li, Lo) in enumerate(geo):
        if use_ln[i] and use_bn[i]:
            raise NotImplementedError("layer %d: LN and BN both set (two convolutions)" % i)
        c = F.conv1d(x, sd["conv.%d.weight" % i], sd["conv.%d.bias" % i])
        if gaps is not None:
            gaps.append(window_gaps(c.detach(), pool))
        z = F.max_pool1d(c, pool)
        if use_ln[i]:
            z = layer_norm(z, sd["ln.%d.gamma" % i], sd["ln.%d.beta" % i])
        elif use_bn[i]:
            z = F.batch_norm(z, sd["bn.%d.running_mean" % i], sd["bn.%d.running_var" % i],
                             sd["bn.%d.weight" % i], sd["bn.%d.bias" % i], train, 0.05, float(Lo))
        z = act(acts[i], z)
        if train and drops[i] > 0:
            if keep is None or keep[i] is None:
                raise ValueError("layer %d has dropout: pass its keep mask" % i)
            z = z * keep[i].to(z.dtype) / (1.0 - drops[i])
        x = z
    return x.reshape(B, -1)


def leaf_state(sd, dtype=torch.float32):
    """A copy of a state dict whose floating parameters are autograd leaves of dtype."""
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(v).clone()
        if t.is_floating_point():
            t = t.to(dtype)
            if "running_" not in k:
                t.requires_grad_(True)
        out[k] = t
    return out


class _LN(torch.nn.Module):
    def __init__(self, shape):
        super().__init__()
        self.gamma = torch.nn.Parameter(torch.ones(shape))
        self.beta = torch.nn.Parameter(torch.zeros(shape))


class RefCNN(torch.nn.Module):
    """cnn_forward behind the reference's module interface (same state-dict keys and order), so
    the oracle's training loop (oracle/run.py) and torch.optim can drive it.  Load the weights
    with load_state_dict; `keep` holds the injected dropout masks of cnn_forward."""

    def __init__(self, options, inp_dim, dtype=torch.float32):
        super().__init__()
        self.opts, self.keep, self.gaps = options, None, None      # (a cfg section or a dict)
        nn = torch.nn
        self.conv, self.bn, self.ln = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        if strtobool(options["cnn_use_laynorm_inp"]):
            self.ln0 = _LN(inp_dim)
        if strtobool(options["cnn_use_batchnorm_inp"]):
            self.bn0 = nn.BatchNorm1d(inp_dim, momentum=0.05)
        for cin, cout, ln_, pool, Li, Lo in geometry(options, inp_dim):
            self.ln.append(_LN([cout, Lo]))
            self.bn.append(nn.BatchNorm1d(cout, eps=Lo, momentum=0.05))
            self.conv.append(nn.Conv1d(cin, cout, ln_))
        self.out_dim = geometry(options, inp_dim)[-1][5] * geometry(options, inp_dim)[-1][1]
        self.to(dtype)

    def forward(self, x):
        sd = self.state_dict(keep_vars=True)
        if self.training:
            for k, v in sd.items():
                used = (k.startswith("bn0.") or
                        (k.startswith("bn.") and _lst(self.opts, "cnn_use_batchnorm", strtobool)[int(k.split(".")[1])]))
                if k.endswith("num_batches_tracked") and used:
                    v.add_(1)
        return cnn_forward(sd, self.opts, x, train=self.training, keep=self.keep, gaps=self.gaps)

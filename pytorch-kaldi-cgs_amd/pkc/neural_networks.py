"""Drop-in architecture plug-ins: ``arch_library = pkc.neural_networks``, ``arch_class = MLP``.

Loaded exactly like the reference's classes (utils.py:1766-1779:
``getattr(importlib.import_module(arch_library), arch_class)(options, inp_dim)``) and exposing the
same contract: ``.out_dim``, ``forward(x)``, ``parameters()/state_dict()/load_state_dict()``,
``train()/eval()``, and the attributes core.run_nn reads (``prune``, ``prune_parameters()``,
``guided_hcgs``, ``apply_guided_hcgs``, ``if_pattern``, ``skip_regularization``).

Parameter names, shapes and the construction-time RNG consumption follow neural_networks.py:81-243
so a state_dict / .pkl checkpoint moves between the reference and this package unchanged and the
same seed gives the same initial weights and HCGS masks.

The math is NOT executed here: training and forward passes run through pkc.engine (HIP kernels in
libpkc.so), driven by pkc.core.run_nn, or by ``forward()`` below — an autograd Function over the
same kernels (pkc.plugin), so the reference's own forward_model + loss.backward() + torch.optim
loop (utils.py:1884-2050, core.py:216-232) trains these classes too.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from .cgs import guided_hcgs_mask, hcgs_mask
from .plugin import arch_forward


def strtobool(v):
    v = str(v).strip().lower()
    if v in ("y", "yes", "t", "true", "on", "1"):
        return 1
    if v in ("n", "no", "f", "false", "off", "0"):
        return 0
    raise ValueError("invalid truth value %r" % v)


def _lst(opts, key, f=str):
    return [f(x) for x in opts[key].split(",")]


class LayerNorm(nn.Module):
    """Parameter holder with the reference's names (neural_networks.py:40-51)."""

    def __init__(self, features, eps=1e-6):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(features))
        self.beta = nn.Parameter(torch.zeros(features))
        self.eps = eps


def _prune_params(params, perc):
    """quantized_modules.prune + W.mul_(mask) on each parameter, on the GPU (pkc_prune)."""
    import ctypes as C
    from . import _lib as L
    work = torch.zeros(L.lib().pkc_prune_work_size(), dtype=torch.uint8, device=params[0].device)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for p in params:
        L.call("pkc_prune", L.ptr(p.data), p.numel(), C.c_double(perc), None, L.ptr(work), s)
    torch.cuda.synchronize()


def _input_norm_specs(net, ln, bn):
    """ln0 (per row) then bn0 (over all rows; T*B rows, padding included, for a recurrent
    architecture: neural_networks.py:826-831) as engine NormLayer specs."""
    out = []
    if ln:
        out.append(dict(kind="ln", gamma=net.ln0.gamma, beta=net.ln0.beta))
    if bn:
        out.append(dict(kind="bn", gamma=net.bn0.weight, beta=net.bn0.bias,
                        rm=net.bn0.running_mean, rv=net.bn0.running_var,
                        nbt=net.bn0.num_batches_tracked))
    return out


class _PatternSet:
    """Pattern-set plumbing shared by MLP and LSTM (neural_networks.py:115-131, 513-529).
    A set comes from ``pattern_from_file`` / ``pattern_file`` (an (P*ph, pw) .npy such as
    pattern_file/b08b08_k04_n16_pattern.npy; a pkc option, shared by every weight), from
    ``pattern_kernels = ...``, or from the ``patterns`` dict run_nn carries between chunks
    (core.py:129-131, 304-306).  Without one, each weight's set is searched as the reference does
    (update_patterns -> sparsity.find_top_k_by_kmeans with pattern_num / pattern_nnz per layer,
    neural_networks.py:339-348, 1162-1172; ``pkc.cgs.kmeans_patterns``): sklearn KMeans with no
    random_state, so parity is unpinned unless ``pattern_seed`` is given."""

    def _pattern_opts(self, o):
        self.if_pattern = strtobool(o["if_pattern"]) if "if_pattern" in o else False
        self.pattern_shape = _lst(o, "pattern_shape", int) if "pattern_shape" in o else [8, 8]
        self.pattern_from_file = o.get("pattern_from_file", o.get("pattern_file", None))
        self.pattern_nnz = _lst(o, "pattern_nnz", int) if "pattern_nnz" in o else []
        self.pattern_num = _lst(o, "pattern_num", int) if "pattern_num" in o else []
        self.pattern_seed = int(o["pattern_seed"]) if "pattern_seed" in o else None

    def can_search_patterns(self):
        return bool(self.pattern_nnz) and bool(self.pattern_num)

    def pattern_search_args(self, layer):
        """(pattern_num, pattern_shape, pattern_nnz) of layer ``layer`` (neural_networks.py:344)."""
        return (self.pattern_num[min(layer, len(self.pattern_num) - 1)], list(self.pattern_shape),
                self.pattern_nnz[min(layer, len(self.pattern_nnz) - 1)])

    @property
    def pattern_kernels(self):
        """(P, ph, pw) float32 pattern set, or None."""
        k = getattr(self, "_pattern_kernels", None)
        if k is None and self.if_pattern:
            pat = self.pattern
            first = (pat[0] if isinstance(pat, list) and pat else
                     next((v[0] for v in pat.values() if v), None) if isinstance(pat, dict) else None)
            if first is not None:                   # (P, 1, ph, pw) kernel, as the reference keeps
                t = first.detach().cpu().numpy() if torch.is_tensor(first) else np.asarray(first)
                k = t.reshape(t.shape[0], t.shape[-2], t.shape[-1]).astype(np.float32)
            elif self.pattern_from_file:
                arr = np.load(self.pattern_from_file, allow_pickle=False).astype(np.float32)
                ph, pw = self.pattern_shape
                k = arr.reshape(-1, ph, pw)
            self._pattern_kernels = k
        return k

    @pattern_kernels.setter
    def pattern_kernels(self, v):
        self._pattern_kernels = None if v is None else np.asarray(v, dtype=np.float32)


class _Mask(nn.Module):
    """HCGS.HCGS / HCGS.guidedHCGS: a ``mask`` Parameter of shape (out, in) (HCGS.py:24-28, 55-59)."""

    def __init__(self, mask):
        super().__init__()
        self.mask = nn.Parameter(torch.from_numpy(mask))


def _mask_product(*ms):
    """Effective in-place mask of several masks multiplied into W one after the other."""
    ms = [m for m in ms if m is not None]
    if not ms:
        return None
    out = ms[0]
    for m in ms[1:]:
        out = out * m
    return out.detach() if len(ms) > 1 else out


def _set_mask(module, arr):
    module.mask.data.copy_(torch.from_numpy(arr).to(module.mask.device))


class _QLinear(nn.Module):
    """Parameter layout + init draws of QuantizeLinear (quantized_modules.py:184-205)."""

    def __init__(self, fin, fout, bits, bias, inp_bits=None):
        super().__init__()
        self.weight = nn.Parameter(torch.Tensor(fout, fin))
        self.bias = nn.Parameter(torch.Tensor(fout)) if bias else None
        s = 1.0 / math.sqrt(fin)
        self.weight.data.uniform_(-s, s)
        if self.bias is not None:
            self.bias.data.uniform_(-s, s)
        self.numBits = bits
        self.inp_quant = inp_bits


class MLP(_PatternSet, nn.Module):
    """neural_networks.py:81-361 (options per proto/MLP.proto + the CGS keys)."""

    seq_model = False

    def __init__(self, options, inp_dim):
        super().__init__()
        o = options
        self.input_dim = inp_dim
        self.dnn_lay = _lst(o, "dnn_lay", int)
        self.dnn_drop = _lst(o, "dnn_drop", float)
        self.dnn_use_batchnorm = _lst(o, "dnn_use_batchnorm", strtobool)
        self.dnn_use_laynorm = _lst(o, "dnn_use_laynorm", strtobool)
        self.dnn_use_laynorm_inp = strtobool(o["dnn_use_laynorm_inp"])
        self.dnn_use_batchnorm_inp = strtobool(o["dnn_use_batchnorm_inp"])
        self.dnn_act = _lst(o, "dnn_act")
        self.to_do = o.get("to_do", "train")
        self.mlp_hcgs = strtobool(o.get("mlp_hcgs", "False"))
        self.hcgs_block = _lst(o, "hcgs_block", int) if "hcgs_block" in o else []
        self.hcgs_sparse = _lst(o, "hcgs_sparse", float) if "hcgs_sparse" in o else []
        self.mlp_quant = strtobool(o.get("mlp_quant", "False"))
        self.param_quant = _lst(o, "param_quant", int) if "param_quant" in o else [8]
        self.mlp_quant_inp = strtobool(o.get("mlp_quant_inp", "False"))
        self.inp_quant = _lst(o, "inp_quant", int) if "inp_quant" in o else [16]
        self.prune = strtobool(o.get("mlp_prune", "False"))
        self.prune_perc = _lst(o, "mlp_prune_perc", float) if "mlp_prune_perc" in o else [0.0]
        self.skip_regularization = strtobool(o.get("skip_regularization", "False"))
        self.guided_hcgs = strtobool(o.get("guided_hcgs", "False"))
        self.apply_guided_hcgs = strtobool(o.get("apply_guided_hcgs", "False"))
        self._pattern_opts(o)
        self.arch_name = o.get("arch_name", "MLP")
        if self.if_pattern:                  # per-layer kernels / masks (neural_networks.py:159-161)
            self.pattern, self.pattern_mask = [], []

        if self.mlp_hcgs:                    # registered first, as neural_networks.py:151-156
            self.hcgs = nn.ModuleList()
        if self.guided_hcgs:
            self.ghcgs = nn.ModuleList()
        self.wx, self.bn, self.ln = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        if self.dnn_use_laynorm_inp:
            self.ln0 = LayerNorm(inp_dim)
        if self.dnn_use_batchnorm_inp:
            self.bn0 = nn.BatchNorm1d(inp_dim, momentum=0.05)
        cur = inp_dim
        for i, n in enumerate(self.dnn_lay):
            self.ln.append(LayerNorm(n))
            self.bn.append(nn.BatchNorm1d(n, momentum=0.05))
            add_bias = not (self.dnn_use_laynorm[i] or self.dnn_use_batchnorm[i])
            if self.mlp_quant:
                lin = _QLinear(cur, n, self.param_quant[i], add_bias,
                               self.inp_quant[0] if self.mlp_quant_inp else None)
            else:
                lin = nn.Linear(cur, n, bias=add_bias)          # consumes the torch RNG as the ref
            self.wx.append(lin)
            if self.mlp_hcgs:
                self.hcgs.append(_Mask(hcgs_mask(n, cur, self.hcgs_block, self.hcgs_sparse)))
            s = np.sqrt(0.01 / (cur + n))                        # neural_networks.py:233-235
            lin.weight = nn.Parameter(torch.Tensor(n, cur).uniform_(-s, s))
            lin.bias = nn.Parameter(torch.zeros(n))
            if self.guided_hcgs:             # from the initial W (neural_networks.py:237-239)
                self.ghcgs.append(_Mask(guided_hcgs_mask(n, cur, self.hcgs_block, self.hcgs_sparse,
                                                         lin.weight.data)))
            cur = n
        self.out_dim = cur

    # --------------------------------------------------------------------- reference hooks
    def prune_parameters(self):
        """Chunk-end pruning (neural_networks.py:321-327, called at core.py:291-296): every
        layer's W pruned at prune_perc[0] (the reference uses the first entry for all layers)."""
        _prune_params([self.wx[i].weight for i in range(len(self.dnn_lay))], self.prune_perc[0])
        return 1

    def apply_ghcgs(self):
        """Chunk-end regeneration of the guided masks from the current W (neural_networks.py:
        329-337, called at core.py:298-300 while apply_guided_hcgs is off)."""
        cur = self.input_dim
        for i, n in enumerate(self.dnn_lay):
            _set_mask(self.ghcgs[i], guided_hcgs_mask(n, cur, self.hcgs_block, self.hcgs_sparse,
                                                      self.wx[i].weight.data))
            cur = n
        return 20.0

    def _wmask(self, i):
        """Masks multiplied into wx[i] before each forward: HCGS, then guided HCGS when applied
        (neural_networks.py:256-262)."""
        return _mask_product(self.hcgs[i].mask if self.mlp_hcgs else None,
                             self.ghcgs[i].mask if (self.guided_hcgs and self.apply_guided_hcgs)
                             else None)

    def layer_specs(self):
        """Per-layer description consumed by pkc.engine."""
        specs = []
        for i, n in enumerate(self.dnn_lay):
            specs.append(dict(out=n, act=self.dnn_act[i], bn=bool(self.dnn_use_batchnorm[i]),
                              ln=bool(self.dnn_use_laynorm[i]), drop=self.dnn_drop[i],
                              W=self.wx[i].weight, b=self.wx[i].bias, gamma=self.bn[i].weight,
                              beta=self.bn[i].bias, rm=self.bn[i].running_mean,
                              rv=self.bn[i].running_var, nbt=self.bn[i].num_batches_tracked,
                              mask=self._wmask(i),
                              quant=self.param_quant[i] if self.mlp_quant else 0,
                              inp_quant=self.inp_quant[0] if (self.mlp_quant and self.mlp_quant_inp) else 0,
                              ln_gamma=self.ln[i].gamma, ln_beta=self.ln[i].beta,
                              prune=self.prune_perc[i] if self.prune else None,
                              pattern=bool(self.if_pattern)))
        return specs

    def pattern_params(self):
        """[(store key, layer, W, HCGS mask)] in the reference's update_mask order."""
        return [((None, i), i, self.wx[i].weight, self._wmask(i)) for i in range(len(self.dnn_lay))]

    def input_norm_specs(self):
        """Input normalisations in the reference's order: ln0 then bn0 (neural_networks.py:246-251)."""
        return _input_norm_specs(self, self.dnn_use_laynorm_inp, self.dnn_use_batchnorm_inp)

    def check_supported(self):
        if self.if_pattern and self.pattern_kernels is None and not self.can_search_patterns():
            raise NotImplementedError("pattern MLP needs a pattern set (pattern_from_file option, "
                                      "pattern_kernels, patterns injected by run_nn) or "
                                      "pattern_num / pattern_nnz for the KMeans search")

    def forward(self, x):
        """(B, F) -> (B, out_dim) on the pkc kernels, trainable under autograd (pkc.plugin)."""
        return arch_forward(self, x)


class _ConvArch(nn.Module):
    """What CNN (neural_networks.py:1934-2033) and SincNet (:2036-2143) share: Conv1d + max-pool
    layers over the (B, 1, inp_dim) input, x = drop(act(norm(max_pool1d(conv(x), pool)))) per
    layer, output (B, C_out * L_out) channel-major.  The two differ in the prefix of their option
    names and in layer 0.  Parameters conv.i, bn.i, ln.i (both norm holders are always registered,
    as the reference does), then ln0 / bn0."""

    seq_model = False
    _prefix = None              # option names: <prefix>_N_filt, ...
    _cgs_suffixes = ("hcgs", "quant", "quant_inp", "prune")

    def _opt(self, key):
        return getattr(self, "%s_%s" % (self._prefix, key))

    def __init__(self, options, inp_dim):
        super().__init__()
        o, p = options, self._prefix
        self.input_dim = inp_dim
        for key, f in (("N_filt", int), ("len_filt", int), ("max_pool_len", int), ("act", str),
                       ("drop", float), ("use_laynorm", strtobool), ("use_batchnorm", strtobool)):
            setattr(self, "%s_%s" % (p, key), _lst(o, "%s_%s" % (p, key), f))
        for key in ("use_laynorm_inp", "use_batchnorm_inp"):
            setattr(self, "%s_%s" % (p, key), strtobool(o["%s_%s" % (p, key)]))
        self.to_do = o.get("to_do", "train")
        # core.run_nn / utils read these on every architecture; the reference class has no CGS hooks
        self.prune = False
        self.guided_hcgs = False
        self.apply_guided_hcgs = False
        self.if_pattern = False
        self.skip_regularization = strtobool(o.get("skip_regularization", "False"))
        # the reference class has no masks, quantisation or pruning: such keys are refused, not ignored
        self._cgs_keys = [k for k in tuple("%s_%s" % (p, s) for s in self._cgs_suffixes) +
                          ("guided_hcgs", "apply_guided_hcgs", "if_pattern")
                          if strtobool(o.get(k, "False"))]
        self._read_options(o)
        N_filt, len_filt, pool = self._opt("N_filt"), self._opt("len_filt"), self._opt("max_pool_len")
        setattr(self, "N_%s_lay" % p, len(N_filt))
        self.conv, self.bn, self.ln = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        if self._opt("use_laynorm_inp"):
            self.ln0 = LayerNorm(inp_dim)
        if self._opt("use_batchnorm_inp"):
            self.bn0 = nn.BatchNorm1d(inp_dim, momentum=0.05)
        cur, cin = inp_dim, 1
        self.L_in, self.L_out = [], []
        for i, n in enumerate(N_filt):
            lout = int((cur - len_filt[i] + 1) / pool[i])
            self.ln.append(LayerNorm([n, lout]))
            # neural_networks.py:1988-1990 (:2096-2098): nn.BatchNorm1d(N_filt, <L_out>,
            # momentum=0.05) puts L_out into the second positional parameter, eps: reproduced
            self.bn.append(nn.BatchNorm1d(n, eps=lout, momentum=0.05))
            self.conv.append(self._make_conv(i, cin, n, len_filt[i], o))
            self.L_in.append(cur)
            self.L_out.append(lout)
            cur, cin = lout, n
        self.out_dim = cur * N_filt[-1]

    def _read_options(self, o):
        """Options of the subclass's own, read before the layers are built."""

    def _make_conv(self, i, cin, n, length, o):
        return nn.Conv1d(cin, n, length)            # the only RNG draws

    def _conv_len(self, i):
        """Taps of layer i's convolution."""
        return self._opt("len_filt")[i]

    def prune_parameters(self):
        raise NotImplementedError("the reference %s has no prune hook" % type(self).__name__)

    def forward(self, x):
        """(B, F) -> (B, out_dim) on the pkc kernels, trainable under autograd (pkc.plugin)."""
        return arch_forward(self, x)

    def check_supported(self):
        name, p = type(self).__name__, self._prefix
        if self._cgs_keys:
            raise NotImplementedError("%s: %s (the reference %s has no weight masks, "
                                      "quantisation or pruning)" % (name, ", ".join(self._cgs_keys), name))
        for i in range(len(self._opt("N_filt"))):
            if self._opt("use_laynorm")[i] and self._opt("use_batchnorm")[i]:
                raise NotImplementedError(
                    "%s layer %d has %s_use_laynorm and %s_use_batchnorm both set: the "
                    "reference then applies the convolution twice (neural_networks.py:2019-2025, "
                    ":2129-2135)" % (name, i, p, p))
            if self._opt("act")[i] == "softmax":
                raise NotImplementedError("%s layer %d: softmax on a convolution layer" % (name, i))
            if self.L_out[i] < 1:
                raise ValueError("%s layer %d has no output (L_out = %d)" % (name, i, self.L_out[i]))

    def input_norm_specs(self):
        return _input_norm_specs(self, self._opt("use_laynorm_inp"), self._opt("use_batchnorm_inp"))

    def conv_specs(self):
        """Per-layer description consumed by pkc.engine (ConvNode)."""
        specs = []
        N_filt = self._opt("N_filt")
        for i, n in enumerate(N_filt):
            conv = self.conv[i]
            specs.append(dict(C_in=1 if i == 0 else N_filt[i - 1], C_out=n,
                              L_in=self.L_in[i], L_out=self.L_out[i], len=self._conv_len(i),
                              pool=self._opt("max_pool_len")[i], act=self._opt("act")[i],
                              drop=self._opt("drop")[i], bn=bool(self._opt("use_batchnorm")[i]),
                              ln=bool(self._opt("use_laynorm")[i]), W=getattr(conv, "weight", None),
                              b=getattr(conv, "bias", None), gamma=self.bn[i].weight,
                              beta=self.bn[i].bias,
                              rm=self.bn[i].running_mean, rv=self.bn[i].running_var,
                              nbt=self.bn[i].num_batches_tracked, bn_eps=float(self.bn[i].eps),
                              bn_momentum=float(self.bn[i].momentum),
                              ln_gamma=self.ln[i].gamma, ln_beta=self.ln[i].beta,
                              ln_eps=float(self.ln[i].eps)))
        return specs


class CNN(_ConvArch):
    """neural_networks.py:1934-2033 (options per proto/CNN.proto).  Per layer only the Conv1d
    draws from the RNG."""

    _prefix = "cnn"


class SincConv(nn.Module):
    """Parameter holder of the reference's SincConv (neural_networks.py:2146-2283): N band-pass
    filters described by low_hz_ and band_hz_ (N, 1), initialised mel-spaced in units of the
    sample rate (:2210-2222, no RNG draw).  window_ (K) and n_ (1, K) are plain attributes, not in
    the state dict; the filters themselves are generated on the GPU (pkc_sinc_filters_fwd)."""

    def __init__(self, out_channels, kernel_size, sample_rate=16000, min_low_hz=50, min_band_hz=50):
        super().__init__()
        self.out_channels = out_channels
        # :2193-2194: an even length is made odd
        self.kernel_size = kernel_size + 1 if kernel_size % 2 == 0 else kernel_size
        self.sample_rate, self.min_low_hz, self.min_band_hz = sample_rate, min_low_hz, min_band_hz
        to_mel = lambda hz: 2595 * np.log10(1 + hz / 700)           # noqa: E731
        to_hz = lambda mel: 700 * (10 ** (mel / 2595) - 1)          # noqa: E731
        high_hz = sample_rate / 2 - (min_low_hz + min_band_hz)
        hz = to_hz(np.linspace(to_mel(30), to_mel(high_hz), out_channels + 1)) / sample_rate
        self.low_hz_ = nn.Parameter(torch.tensor(hz[:-1], dtype=torch.float32).view(-1, 1))
        self.band_hz_ = nn.Parameter(torch.tensor(np.diff(hz), dtype=torch.float32).view(-1, 1))
        K = self.kernel_size
        # :2226-2232 in torch's fp32, so the rounding is the reference's (the window is the
        # reference's own: linspace(0, K, K), not a symmetric Hamming window)
        self.window_ = 0.54 - 0.46 * torch.cos(2 * math.pi * torch.linspace(0, K, steps=K) / K)
        n = (K - 1) / 2
        self.n_ = torch.arange(-n, n + 1).view(1, -1) / sample_rate


class SincNet(_ConvArch):
    """neural_networks.py:2036-2143 (options per proto/SincNet.proto): CNN's layers with sinc_*
    option names, except that layer 0 is a SincConv: its (N, 1, K) weight is a band-pass filter
    bank regenerated before every forward from conv.0.low_hz_ / conv.0.band_hz_, without bias.
    No RNG draw in layer 0."""

    _prefix = "sinc"

    def _read_options(self, o):
        self.sinc_sample_rate = int(o["sinc_sample_rate"])
        self.sinc_min_low_hz = int(o["sinc_min_low_hz"])
        self.sinc_min_band_hz = int(o["sinc_min_band_hz"])

    def _make_conv(self, i, cin, n, length, o):
        if i > 0:
            return nn.Conv1d(cin, n, length)
        return SincConv(n, length, sample_rate=self.sinc_sample_rate,
                        min_low_hz=self.sinc_min_low_hz, min_band_hz=self.sinc_min_band_hz)

    def _conv_len(self, i):
        return self.conv[0].kernel_size if i == 0 else self.sinc_len_filt[i]

    def check_supported(self):
        super().check_supported()
        # neural_networks.py:2094 sizes ln[0] / bn[0] with sinc_len_filt[0] as configured while the
        # convolution runs with the length :2193-2194 made odd
        K, pool = self.conv[0].kernel_size, self.sinc_max_pool_len[0]
        conv_out = int((self.input_dim - K + 1) / pool)
        if conv_out != self.L_out[0]:
            raise ValueError(
                "SincNet: sinc_len_filt[0] = %d is even, so SincConv convolves with %d taps "
                "(neural_networks.py:2193-2194) and layer 0 yields %d positions, but its "
                "LayerNorm / BatchNorm are sized for %d (neural_networks.py:2094): the "
                "reference's forward fails on this shape" % (self.sinc_len_filt[0], K, conv_out,
                                                             self.L_out[0]))

    def conv_specs(self):
        specs = super().conv_specs()
        c = self.conv[0]
        specs[0]["sinc"] = dict(low=c.low_hz_, band=c.band_hz_, n_=c.n_, window=c.window_,
                                sr=float(c.sample_rate), min_low_hz=float(c.min_low_hz),
                                min_band_hz=float(c.min_band_hz))
        return specs


def _hcgs_hook_opts(net, o, key):
    """The LSTM's HCGS hook on a cell the reference gives none (GRU, minimalGRU, RNN; the liGRU's
    ``ligru_hcgs`` is the same extension): with ``key`` set, the keys hcgsx_* / hcgsh_* and the
    mask lists hcgsx / hcgsh, registered before the layer lists as the LSTM's are
    (neural_networks.py:548-550).  One W mask and one U mask per layer, shared by its gates
    (:858-861, 980-983).  Without the key nothing is registered and nothing is drawn."""
    net.hcgs_on = bool(strtobool(o.get(key, "False")))
    setattr(net, key, net.hcgs_on)
    if net.hcgs_on:
        net.hcgsx_block = _lst(o, "hcgsx_block", int)
        net.hcgsh_block = _lst(o, "hcgsh_block", int)
        net.hcgsx_sparse = _lst(o, "hcgsx_sparse", float)
        net.hcgsh_sparse = _lst(o, "hcgsh_sparse", float)
        net.hcgsx, net.hcgsh = nn.ModuleList(), nn.ModuleList()


class liGRU(nn.Module):
    """neural_networks.py:1429-1599 (options per proto/liGRU.proto).  Parameters: wh, wz (input
    Linear), uh, uz (recurrent Linear, no bias), bn_wh, bn_wz, ln; same names and init draws."""

    seq_model = True
    cell = "ligru"
    GATES = ("z", "h")

    def __init__(self, options, inp_dim):
        super().__init__()
        o = options
        self.input_dim = inp_dim
        self.ligru_lay = _lst(o, "ligru_lay", int)
        self.ligru_drop = _lst(o, "ligru_drop", float)
        self.ligru_use_batchnorm = _lst(o, "ligru_use_batchnorm", strtobool)
        self.ligru_use_laynorm = _lst(o, "ligru_use_laynorm", strtobool)
        self.ligru_use_laynorm_inp = strtobool(o["ligru_use_laynorm_inp"])
        self.ligru_use_batchnorm_inp = strtobool(o["ligru_use_batchnorm_inp"])
        self.ligru_orthinit = strtobool(o["ligru_orthinit"])
        self.ligru_act = _lst(o, "ligru_act")
        self.bidir = strtobool(o["ligru_bidir"])
        self.to_do = o.get("to_do", "train")
        self.prune = False
        self.guided_hcgs = False
        self.apply_guided_hcgs = False
        self.if_pattern = False
        self.skip_regularization = strtobool(o.get("skip_regularization", "False"))
        # pkc extension for config C3: the reference liGRU has no CGS hook; with
        # ligru_hcgs the LSTM's HCGS hook is reused (same keys hcgsx_* / hcgsh_*, masks drawn
        # after each layer's W and U Linears, applied in place every forward)
        self.ligru_hcgs = strtobool(o.get("ligru_hcgs", "False"))
        if self.ligru_hcgs:
            self.hcgsx_block = _lst(o, "hcgsx_block", int)
            self.hcgsh_block = _lst(o, "hcgsh_block", int)
            self.hcgsx_sparse = _lst(o, "hcgsx_sparse", float)
            self.hcgsh_sparse = _lst(o, "hcgsh_sparse", float)
            self.hcgsx, self.hcgsh = nn.ModuleList(), nn.ModuleList()
        self.wh, self.uh = nn.ModuleList(), nn.ModuleList()
        self.wz, self.uz = nn.ModuleList(), nn.ModuleList()
        self.ln, self.bn_wh, self.bn_wz = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        if self.ligru_use_laynorm_inp:
            self.ln0 = LayerNorm(inp_dim)
        if self.ligru_use_batchnorm_inp:
            self.bn0 = nn.BatchNorm1d(inp_dim, momentum=0.05)
        cur = inp_dim
        for i, n in enumerate(self.ligru_lay):
            add_bias = not (self.ligru_use_laynorm[i] or self.ligru_use_batchnorm[i])
            self.wh.append(nn.Linear(cur, n, bias=add_bias))
            self.wz.append(nn.Linear(cur, n, bias=add_bias))
            if self.ligru_hcgs:
                self.hcgsx.append(_Mask(hcgs_mask(n, cur, self.hcgsx_block, self.hcgsx_sparse)))
            self.uh.append(nn.Linear(n, n, bias=False))
            self.uz.append(nn.Linear(n, n, bias=False))
            if self.ligru_hcgs:
                self.hcgsh.append(_Mask(hcgs_mask(n, n, self.hcgsh_block, self.hcgsh_sparse)))
            if self.ligru_orthinit:
                nn.init.orthogonal_(self.uh[i].weight)
                nn.init.orthogonal_(self.uz[i].weight)
            self.bn_wh.append(nn.BatchNorm1d(n, momentum=0.05))
            self.bn_wz.append(nn.BatchNorm1d(n, momentum=0.05))
            self.ln.append(LayerNorm(n))
            cur = 2 * n if self.bidir else n
        self.out_dim = cur

    def prune_parameters(self):
        raise NotImplementedError("the reference liGRU has no prune hook")

    def forward(self, x):
        """(T, B, F) -> (T, B, out_dim) on the pkc kernels (the shared-weight bidirectional
        convention when bidir), trainable under autograd (pkc.plugin)."""
        return arch_forward(self, x)

    def check_supported(self):
        pass

    def input_norm_specs(self):
        return _input_norm_specs(self, self.ligru_use_laynorm_inp, self.ligru_use_batchnorm_inp)

    def layer_specs(self):
        specs = []
        for i, n in enumerate(self.ligru_lay):
            specs.append(dict(H=n, act=self.ligru_act[i], bn=bool(self.ligru_use_batchnorm[i]),
                              drop=self.ligru_drop[i], bidir=bool(self.bidir),
                              W=[self.wz[i].weight, self.wh[i].weight],
                              b=[self.wz[i].bias, self.wh[i].bias],
                              U=[self.uz[i].weight, self.uh[i].weight],
                              bnm=[self.bn_wz[i], self.bn_wh[i]],
                              Wmask=self.hcgsx[i].mask if self.ligru_hcgs else None,
                              Umask=self.hcgsh[i].mask if self.ligru_hcgs else None,
                              ln=bool(self.ligru_use_laynorm[i]), ln_gamma=self.ln[i].gamma,
                              ln_beta=self.ln[i].beta))
        return specs


class GRU(nn.Module):
    """neural_networks.py:1240-1426 (options per proto/GRU.proto).  Parameters: wh, uh, wz, uz, wr,
    ur, ln, bn_wh, bn_wz, bn_wr (registration order and init draws of the reference).  pkc adds the
    optional HCGS hook ``gru_hcgs`` (_hcgs_hook_opts); without the key nothing else is registered."""

    seq_model = True
    cell = "gru"
    GATES = ("z", "r", "h")

    def __init__(self, options, inp_dim):
        super().__init__()
        o = options
        self.input_dim = inp_dim
        self.gru_lay = _lst(o, "gru_lay", int)
        self.gru_drop = _lst(o, "gru_drop", float)
        self.gru_use_batchnorm = _lst(o, "gru_use_batchnorm", strtobool)
        self.gru_use_laynorm = _lst(o, "gru_use_laynorm", strtobool)
        self.gru_use_laynorm_inp = strtobool(o["gru_use_laynorm_inp"])
        self.gru_use_batchnorm_inp = strtobool(o["gru_use_batchnorm_inp"])
        self.gru_orthinit = strtobool(o["gru_orthinit"])
        self.gru_act = _lst(o, "gru_act")
        self.bidir = strtobool(o["gru_bidir"])
        self.to_do = o.get("to_do", "train")
        # core.run_nn / utils read these on every architecture; the reference GRU has no CGS hooks
        self.prune = False
        self.guided_hcgs = False
        self.apply_guided_hcgs = False
        self.if_pattern = False
        self.skip_regularization = strtobool(o.get("skip_regularization", "False"))
        # pkc extension (as ligru_hcgs; no reference counterpart): the LSTM's HCGS hook on the GRU
        _hcgs_hook_opts(self, o, "gru_hcgs")
        self.wh, self.uh = nn.ModuleList(), nn.ModuleList()
        self.wz, self.uz = nn.ModuleList(), nn.ModuleList()
        self.wr, self.ur = nn.ModuleList(), nn.ModuleList()
        self.ln = nn.ModuleList()
        self.bn_wh, self.bn_wz, self.bn_wr = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        if self.gru_use_laynorm_inp:
            self.ln0 = LayerNorm(inp_dim)
        if self.gru_use_batchnorm_inp:
            self.bn0 = nn.BatchNorm1d(inp_dim, momentum=0.05)
        cur = inp_dim
        for i, n in enumerate(self.gru_lay):
            add_bias = not (self.gru_use_laynorm[i] or self.gru_use_batchnorm[i])
            self.wh.append(nn.Linear(cur, n, bias=add_bias))
            self.wz.append(nn.Linear(cur, n, bias=add_bias))
            self.wr.append(nn.Linear(cur, n, bias=add_bias))
            if self.hcgs_on:
                self.hcgsx.append(_Mask(hcgs_mask(n, cur, self.hcgsx_block, self.hcgsx_sparse)))
            self.uh.append(nn.Linear(n, n, bias=False))
            self.uz.append(nn.Linear(n, n, bias=False))
            self.ur.append(nn.Linear(n, n, bias=False))
            if self.hcgs_on:
                self.hcgsh.append(_Mask(hcgs_mask(n, n, self.hcgsh_block, self.hcgsh_sparse)))
            if self.gru_orthinit:
                nn.init.orthogonal_(self.uh[i].weight)
                nn.init.orthogonal_(self.uz[i].weight)
                nn.init.orthogonal_(self.ur[i].weight)
            self.bn_wh.append(nn.BatchNorm1d(n, momentum=0.05))
            self.bn_wz.append(nn.BatchNorm1d(n, momentum=0.05))
            self.bn_wr.append(nn.BatchNorm1d(n, momentum=0.05))
            self.ln.append(LayerNorm(n))
            cur = 2 * n if self.bidir else n
        self.out_dim = cur

    def prune_parameters(self):
        raise NotImplementedError("the reference GRU has no prune hook")

    def forward(self, x):
        """(T, B, F) -> (T, B, out_dim) on the pkc kernels (the shared-weight bidirectional
        convention when bidir), trainable under autograd (pkc.plugin)."""
        return arch_forward(self, x)

    def check_supported(self):
        pass

    def input_norm_specs(self):
        return _input_norm_specs(self, self.gru_use_laynorm_inp, self.gru_use_batchnorm_inp)

    def layer_specs(self):
        specs = []
        for i, n in enumerate(self.gru_lay):
            specs.append(dict(H=n, act=self.gru_act[i], bn=bool(self.gru_use_batchnorm[i]),
                              drop=self.gru_drop[i], bidir=bool(self.bidir),
                              W=[self.wz[i].weight, self.wr[i].weight, self.wh[i].weight],
                              b=[self.wz[i].bias, self.wr[i].bias, self.wh[i].bias],
                              U=[self.uz[i].weight, self.ur[i].weight, self.uh[i].weight],
                              bnm=[self.bn_wz[i], self.bn_wr[i], self.bn_wh[i]],
                              Wmask=self.hcgsx[i].mask if self.hcgs_on else None,
                              Umask=self.hcgsh[i].mask if self.hcgs_on else None,
                              ln=bool(self.gru_use_laynorm[i]),
                              ln_gamma=self.ln[i].gamma, ln_beta=self.ln[i].beta))
        return specs


class _PlainRec(nn.Module):
    """Shared construction of the reference's hook-free recurrent families (minimalGRU, RNN;
    pkc adds the optional HCGS hook minimalgru_hcgs / rnn_hcgs, see _hcgs_hook_opts):
    option keys <prefix>_lay/_drop/_use_batchnorm/..., input Linears w<g> (bias only without
    BN/LN), recurrent Linears u<g> (no bias, optional orthogonal init), bn_w<g>, ln."""

    seq_model = True
    PREFIX = ""
    GATES = ()
    INIT_ORDER = ()         # reference registration / init order of the gate letters

    def __init__(self, options, inp_dim):
        super().__init__()
        o, p = options, self.PREFIX
        self.input_dim = inp_dim
        self.lay = _lst(o, p + "_lay", int)
        self.drop = _lst(o, p + "_drop", float)
        self.use_bn = _lst(o, p + "_use_batchnorm", strtobool)
        self.use_ln = _lst(o, p + "_use_laynorm", strtobool)
        self.ln_inp = strtobool(o[p + "_use_laynorm_inp"])
        self.bn_inp = strtobool(o[p + "_use_batchnorm_inp"])
        self.orthinit = strtobool(o[p + "_orthinit"])
        self.acts = _lst(o, p + "_act")
        self.bidir = strtobool(o[p + "_bidir"])
        self.to_do = o.get("to_do", "train")
        self.prune = False
        self.guided_hcgs = False
        self.apply_guided_hcgs = False
        self.if_pattern = False
        self.skip_regularization = strtobool(o.get("skip_regularization", "False"))
        # pkc extension (as ligru_hcgs; no reference counterpart): minimalgru_hcgs / rnn_hcgs
        _hcgs_hook_opts(self, o, p + "_hcgs")
        for g in self.INIT_ORDER:
            setattr(self, "w" + g, nn.ModuleList())
            setattr(self, "u" + g, nn.ModuleList())
        self.ln = nn.ModuleList()
        for g in self.INIT_ORDER:
            setattr(self, "bn_w" + g, nn.ModuleList())
        if self.ln_inp:
            self.ln0 = LayerNorm(inp_dim)
        if self.bn_inp:
            self.bn0 = nn.BatchNorm1d(inp_dim, momentum=0.05)
        cur = inp_dim
        for i, n in enumerate(self.lay):
            add_bias = not (self.use_ln[i] or self.use_bn[i])
            for g in self.INIT_ORDER:
                getattr(self, "w" + g).append(nn.Linear(cur, n, bias=add_bias))
            if self.hcgs_on:
                self.hcgsx.append(_Mask(hcgs_mask(n, cur, self.hcgsx_block, self.hcgsx_sparse)))
            for g in self.INIT_ORDER:
                getattr(self, "u" + g).append(nn.Linear(n, n, bias=False))
            if self.hcgs_on:
                self.hcgsh.append(_Mask(hcgs_mask(n, n, self.hcgsh_block, self.hcgsh_sparse)))
            if self.orthinit:
                for g in self.INIT_ORDER:
                    nn.init.orthogonal_(getattr(self, "u" + g)[i].weight)
            for g in self.INIT_ORDER:
                getattr(self, "bn_w" + g).append(nn.BatchNorm1d(n, momentum=0.05))
            self.ln.append(LayerNorm(n))
            cur = 2 * n if self.bidir else n
        self.out_dim = cur

    def prune_parameters(self):
        raise NotImplementedError("the reference %s has no prune hook" % type(self).__name__)

    def forward(self, x):
        """(T, B, F) -> (T, B, out_dim) on the pkc kernels (the shared-weight bidirectional
        convention when bidir), trainable under autograd (pkc.plugin)."""
        return arch_forward(self, x)

    def check_supported(self):
        pass

    def input_norm_specs(self):
        return _input_norm_specs(self, self.ln_inp, self.bn_inp)

    def layer_specs(self):
        specs = []
        for i, n in enumerate(self.lay):
            specs.append(dict(H=n, act=self.acts[i], bn=bool(self.use_bn[i]), drop=self.drop[i],
                              bidir=bool(self.bidir),
                              W=[getattr(self, "w" + g)[i].weight for g in self.GATES],
                              b=[getattr(self, "w" + g)[i].bias for g in self.GATES],
                              U=[getattr(self, "u" + g)[i].weight for g in self.GATES],
                              bnm=[getattr(self, "bn_w" + g)[i] for g in self.GATES],
                              Wmask=self.hcgsx[i].mask if self.hcgs_on else None,
                              Umask=self.hcgsh[i].mask if self.hcgs_on else None,
                              ln=bool(self.use_ln[i]),
                              ln_gamma=self.ln[i].gamma, ln_beta=self.ln[i].beta))
        return specs


class minimalGRU(_PlainRec):
    """neural_networks.py:1602-1777: z = sig(wz + Uz h); h = z h + (1-z) act(wh + Uh (z*h))*drop.
    Reference attribute names (minimalgru_lay, ...) are aliased below."""

    PREFIX = "minimalgru"
    cell = "minimalgru"
    GATES = ("z", "h")
    INIT_ORDER = ("h", "z")

    def __init__(self, options, inp_dim):
        super().__init__(options, inp_dim)
        self.minimalgru_lay, self.minimalgru_drop = self.lay, self.drop


class RNN(_PlainRec):
    """neural_networks.py:1780-1931: h = act(wh + Uh h) * drop."""

    PREFIX = "rnn"
    cell = "rnn"
    GATES = ("h",)
    INIT_ORDER = ("h",)

    def __init__(self, options, inp_dim):
        super().__init__(options, inp_dim)
        self.rnn_lay, self.rnn_drop = self.lay, self.drop


class LSTM(_PatternSet, nn.Module):
    """neural_networks.py:468-1237.  The reference forces bidir off inside forward (:835), so a
    bidirectional cfg crashes there on layer 2; pkc runs bidirectional LSTMs with the liGRU
    shared-weight convention (BASELINE C4) and uni-directional ones exactly as the reference."""

    seq_model = True
    cell = "lstm"
    GATES = ("f", "i", "o", "c")

    def __init__(self, options, inp_dim):
        super().__init__()
        o = options
        self.input_dim = inp_dim
        self.lstm_lay = _lst(o, "lstm_lay", int)
        self.lstm_drop = _lst(o, "lstm_drop", float)
        self.lstm_use_batchnorm = _lst(o, "lstm_use_batchnorm", strtobool)
        self.lstm_use_laynorm = _lst(o, "lstm_use_laynorm", strtobool)
        self.lstm_use_laynorm_inp = strtobool(o["lstm_use_laynorm_inp"])
        self.lstm_use_batchnorm_inp = strtobool(o["lstm_use_batchnorm_inp"])
        self.lstm_act = _lst(o, "lstm_act")
        self.lstm_orthinit = strtobool(o["lstm_orthinit"])
        self.bidir = strtobool(o["lstm_bidir"])
        self.to_do = o.get("to_do", "train")
        self.lstm_hcgs = strtobool(o.get("lstm_hcgs", "False"))
        self.hcgsx_block = _lst(o, "hcgsx_block", int) if "hcgsx_block" in o else []
        self.hcgsh_block = _lst(o, "hcgsh_block", int) if "hcgsh_block" in o else []
        self.hcgsx_sparse = _lst(o, "hcgsx_sparse", float) if "hcgsx_sparse" in o else []
        self.hcgsh_sparse = _lst(o, "hcgsh_sparse", float) if "hcgsh_sparse" in o else []
        self.lstm_quant = strtobool(o.get("lstm_quant", "False"))
        self.param_quant = _lst(o, "param_quant", int) if "param_quant" in o else [8] * len(self.lstm_lay)
        self.lstm_quant_inp = strtobool(o.get("lstm_quant_inp", "False"))
        self.inp_quant = _lst(o, "inp_quant", int) if "inp_quant" in o else [16]
        self.prune = strtobool(o.get("lstm_prune", "False"))
        self.prune_perc = _lst(o, "lstm_prune_perc", float) if "lstm_prune_perc" in o else [0.0]
        self.skip_regularization = strtobool(o.get("skip_regularization", "False"))
        self.guided_hcgs = strtobool(o.get("guided_hcgs", "False"))
        self.apply_guided_hcgs = strtobool(o.get("apply_guided_hcgs", "False"))
        self._pattern_opts(o)
        self.arch_name = o.get("arch_name", "LSTM")
        if self.lstm_hcgs:                      # registered first, as neural_networks.py:548-550
            self.hcgsx, self.hcgsh = nn.ModuleList(), nn.ModuleList()
        if self.guided_hcgs:                    # then the guided lists (553-564)
            for g in self.GATES:
                setattr(self, "ghcgs_w%sx" % g, nn.ModuleList())
                setattr(self, "ghcgs_u%sh" % g, nn.ModuleList())
        if self.if_pattern:
            self.pattern = {k: [] for k in ("pattern_w%sx" % g for g in self.GATES)}
            self.pattern.update({k: [] for k in ("pattern_u%sh" % g for g in self.GATES)})
            self.pattern_mask = {k: [] for k in ("pattern_mask_w%sx" % g for g in self.GATES)}
            self.pattern_mask.update({k: [] for k in ("pattern_mask_u%sh" % g for g in self.GATES)})
        for g in self.GATES:
            setattr(self, "w%sx" % g, nn.ModuleList())
            setattr(self, "u%sh" % g, nn.ModuleList())
        # registration order above = the reference's wfx, ufh, wix, uih, wox, uoh, wcx, uch
        # (neural_networks.py:606-616), so parameters() / optimizer indices line up
        self.ln = nn.ModuleList()
        for g in self.GATES:
            setattr(self, "bn_w%sx" % g, nn.ModuleList())
        if self.lstm_use_laynorm_inp:
            self.ln0 = LayerNorm(inp_dim)
        if self.lstm_use_batchnorm_inp:
            self.bn0 = nn.BatchNorm1d(inp_dim, momentum=0.05)
        cur = inp_dim
        for i, n in enumerate(self.lstm_lay):
            if not (self.lstm_use_laynorm[i] or self.lstm_use_batchnorm[i]):
                raise IndexError("the reference LSTM creates its W/U layers only with BN or LN "
                                 "(neural_networks.py:681-791)")
            for g in self.GATES:
                if self.lstm_quant:
                    lin = _QLinear(cur, n, self.param_quant[i], False,
                                   self.inp_quant[0] if self.lstm_quant_inp else None)
                else:
                    lin = nn.Linear(cur, n, bias=False)
                getattr(self, "w%sx" % g).append(lin)
            if self.lstm_hcgs:
                self.hcgsx.append(_Mask(hcgs_mask(n, cur, self.hcgsx_block, self.hcgsx_sparse)))
            if self.guided_hcgs:                # from the initial W (neural_networks.py:727-735)
                for g in self.GATES:
                    getattr(self, "ghcgs_w%sx" % g).append(_Mask(guided_hcgs_mask(
                        n, cur, self.hcgsx_block, self.hcgsx_sparse,
                        getattr(self, "w%sx" % g)[i].weight.data)))
            for g in self.GATES:
                if self.lstm_quant:
                    lin = _QLinear(n, n, self.param_quant[i], False,
                                   self.inp_quant[0] if self.lstm_quant_inp else None)
                else:
                    lin = nn.Linear(n, n, bias=False)
                getattr(self, "u%sh" % g).append(lin)
            if self.lstm_hcgs:
                self.hcgsh.append(_Mask(hcgs_mask(n, n, self.hcgsh_block, self.hcgsh_sparse)))
            if self.lstm_orthinit:
                for g in self.GATES:
                    nn.init.orthogonal_(getattr(self, "u%sh" % g)[i].weight)
            if self.guided_hcgs:                # from the initial U (neural_networks.py:797-806)
                for g in self.GATES:
                    getattr(self, "ghcgs_u%sh" % g).append(_Mask(guided_hcgs_mask(
                        n, n, self.hcgsh_block, self.hcgsh_sparse,
                        getattr(self, "u%sh" % g)[i].weight.data)))
            for g in self.GATES:
                getattr(self, "bn_w%sx" % g).append(nn.BatchNorm1d(n, momentum=0.05))
            self.ln.append(LayerNorm(n))
            cur = 2 * n if self.bidir else n
        self.out_dim = cur

    def prune_parameters(self):
        """Chunk-end pruning (neural_networks.py:1114-1135): every gate W and U at prune_perc[0]."""
        _prune_params([getattr(self, "%s" % nm)[i].weight for i in range(len(self.lstm_lay))
                       for nm in ("wfx", "wix", "wox", "wcx", "ufh", "uih", "uoh", "uch")],
                      self.prune_perc[0])
        return 1

    def apply_ghcgs(self):
        """Chunk-end regeneration of the guided masks from the current W / U (neural_networks.py:
        1137-1160, core.py:298-300)."""
        cur = self.input_dim
        for i, n in enumerate(self.lstm_lay):
            for g in self.GATES:
                _set_mask(getattr(self, "ghcgs_w%sx" % g)[i], guided_hcgs_mask(
                    n, cur, self.hcgsx_block, self.hcgsx_sparse, getattr(self, "w%sx" % g)[i].weight.data))
                _set_mask(getattr(self, "ghcgs_u%sh" % g)[i], guided_hcgs_mask(
                    n, n, self.hcgsh_block, self.hcgsh_sparse, getattr(self, "u%sh" % g)[i].weight.data))
            cur = 2 * n if self.bidir else n
        return 1

    def _gmask(self, kind, g, i):
        """Masks multiplied into w<g>x[i] / u<g>h[i] before use: HCGS, then guided HCGS when
        applied (neural_networks.py:858-873, 980-994)."""
        h = (self.hcgsx if kind == "w" else self.hcgsh)[i].mask if self.lstm_hcgs else None
        gm = None
        if self.guided_hcgs and self.apply_guided_hcgs:
            nm = ("ghcgs_w%sx" if kind == "w" else "ghcgs_u%sh") % g
            gm = getattr(self, nm)[i].mask
        return _mask_product(h, gm)

    def input_norm_specs(self):
        return _input_norm_specs(self, self.lstm_use_laynorm_inp, self.lstm_use_batchnorm_inp)

    def forward(self, x):
        """(T, B, F) -> (T, B, out_dim) on the pkc kernels (the shared-weight bidirectional
        convention when bidir), trainable under autograd (pkc.plugin)."""
        return arch_forward(self, x)

    def check_supported(self):
        if self.if_pattern and self.pattern_kernels is None and not self.can_search_patterns():
            raise NotImplementedError("pattern LSTM needs a pattern set (pattern_file option, "
                                      "patterns injected by run_nn) or pattern_num / pattern_nnz "
                                      "for the KMeans search")

    def pattern_params(self):
        """[(store key, layer, W or U, HCGS mask)] in the reference's update_mask order
        (neural_networks.py:1202-1223)."""
        out = []
        for i in range(len(self.lstm_lay)):
            for kind in ("w", "u"):
                for g in self.GATES:
                    nm = ("w%sx" if kind == "w" else "u%sh") % g
                    out.append((("pattern_mask_" + nm, i), i, getattr(self, nm)[i].weight,
                                self._gmask(kind, g, i)))
        return out

    def layer_specs(self):
        specs = []
        for i, n in enumerate(self.lstm_lay):
            specs.append(dict(H=n, act=self.lstm_act[i], bn=bool(self.lstm_use_batchnorm[i]),
                              drop=self.lstm_drop[i], bidir=bool(self.bidir),
                              W=[getattr(self, "w%sx" % g)[i].weight for g in self.GATES],
                              b=[None] * 4,
                              U=[getattr(self, "u%sh" % g)[i].weight for g in self.GATES],
                              bnm=[getattr(self, "bn_w%sx" % g)[i] for g in self.GATES],
                              Wmask=self.hcgsx[i].mask if self.lstm_hcgs else None,
                              Umask=self.hcgsh[i].mask if self.lstm_hcgs else None,
                              Wmasks=[self._gmask("w", g, i) for g in self.GATES],
                              Umasks=[self._gmask("u", g, i) for g in self.GATES],
                              qbits=self.param_quant[i] if self.lstm_quant else 0,
                              ibits=self.inp_quant[0] if (self.lstm_quant and self.lstm_quant_inp) else 0,
                              prune=self.prune_perc[i] if self.prune else None,
                              pattern=bool(self.if_pattern), ln=bool(self.lstm_use_laynorm[i]),
                              ln_gamma=self.ln[i].gamma, ln_beta=self.ln[i].beta))
        return specs


class _StdParams(nn.Module):
    """The parameters of a torch.nn.LSTM / GRU / RNN as plain Parameters under torch's names, in
    torch's registration order (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0, ..._l0_reverse,
    ..._l1, ...) and with nn.RNNBase.reset_parameters' draws (U(-1/sqrt(H), 1/sqrt(H)) in that
    order).  Plain Parameters, not a wrapped nn.LSTM: its flatten_parameters() may re-seat the
    parameter storage on .to(device), while the engine keeps device pointers, and its own forward
    (MIOpen) must never run.  proj > 0 (nn.LSTM's proj_size): weight_hh is (G*H, proj), the layers
    above the first read ndir * proj inputs and weight_hr (proj, H) follows the biases."""

    def __init__(self, G, inp, H, layers, bias, ndir, proj=0):
        super().__init__()
        R = proj if proj > 0 else H              # the width of the recurrent state
        for l in range(layers):
            K = inp if l == 0 else R * ndir
            for d in range(ndir):
                sfx = "_l%d%s" % (l, "_reverse" if d else "")
                self.register_parameter("weight_ih" + sfx, nn.Parameter(torch.empty(G * H, K)))
                self.register_parameter("weight_hh" + sfx, nn.Parameter(torch.empty(G * H, R)))
                if bias:
                    self.register_parameter("bias_ih" + sfx, nn.Parameter(torch.empty(G * H)))
                    self.register_parameter("bias_hh" + sfx, nn.Parameter(torch.empty(G * H)))
                if proj > 0:
                    self.register_parameter("weight_hr" + sfx, nn.Parameter(torch.empty(proj, H)))
        stdv = 1.0 / math.sqrt(H) if H > 0 else 0
        for p in self.parameters():
            nn.init.uniform_(p, -stdv, stdv)


class _StdRec(nn.Module):
    """LSTM_cudnn / GRU_cudnn / RNN_cudnn (neural_networks.py:364-465; options per
    proto/{LSTM,GRU,RNN}_cudnn.proto): torch.nn.LSTM / GRU / RNN with a zero initial state.  Each
    direction has its own weights, the GRU is torch's cell (the reset gate multiplies after the
    recurrent product), and dropout acts between layers — the standard-cell time loops of
    pkc_rnn_std_fwd / _bwd, not the cells of the reference's own LSTM / GRU / RNN classes.
    LSTM_cudnn also reads torch's own keyword proj_size (default 0): with 0 < proj_size <
    hidden_size it is the projected LSTM, torch.nn.LSTM(..., proj_size=P), on the time loops of
    pkc_lstmp_fwd / _bwd (the reference class forwards no proj_size; the pin is torch's)."""

    seq_model = True
    std_cell = ""           # "lstm" | "gru" | "rnn": also the attribute holding the parameters
    STD_GATES = 0

    def __init__(self, options, inp_dim):
        super().__init__()
        o, name = options, type(self).__name__
        for k in o:
            if any(w in k for w in ("hcgs", "quant", "prune", "pattern")):
                raise NotImplementedError("%s: the key %s (CGS / quantisation / pruning) is not "
                                          "supported, the reference class has no such hook" % (name, k))
            if "laynorm" in k or "batchnorm" in k:
                raise NotImplementedError("%s: the input normalisation key %s is not supported, the "
                                          "reference class has none" % (name, k))
        self.input_dim = inp_dim
        self.hidden_size = int(o["hidden_size"])
        self.num_layers = int(o["num_layers"])
        self.bias = strtobool(o["bias"])
        self.batch_first = strtobool(o["batch_first"])     # parsed and ignored, as the reference
        self.dropout = float(o["dropout"])
        self.bidirectional = strtobool(o["bidirectional"])
        if not 0.0 <= self.dropout < 1.0:
            raise ValueError("%s: dropout = %s is outside [0, 1)" % (name, o["dropout"]))
        self.proj_size = int(o.get("proj_size", 0))
        if self.proj_size < 0 or self.proj_size >= self.hidden_size:
            raise ValueError("%s: proj_size = %s has to be a non-negative integer smaller than "
                             "hidden_size = %d" % (name, o["proj_size"], self.hidden_size))
        if self.proj_size != 0 and self.std_cell != "lstm":
            raise ValueError("%s: proj_size = %s, but proj_size is only supported by LSTM_cudnn"
                             % (name, o["proj_size"]))
        self.nonlinearity = "tanh"
        if self.std_cell == "rnn":
            self.nonlinearity = o["nonlinearity"]
            if self.nonlinearity not in ("tanh", "relu"):
                raise NotImplementedError("%s: nonlinearity = %s (tanh or relu)" % (name, self.nonlinearity))
        self.to_do = o.get("to_do", "train")
        self.prune = False
        self.guided_hcgs = False
        self.apply_guided_hcgs = False
        self.if_pattern = False
        self.skip_regularization = strtobool(o.get("skip_regularization", "False"))
        nd = 2 if self.bidirectional else 1
        setattr(self, self.std_cell, nn.ModuleList([_StdParams(
            self.STD_GATES, inp_dim, self.hidden_size, self.num_layers, self.bias, nd,
            self.proj_size)]))
        self.out_dim = (self.proj_size or self.hidden_size) * nd

    def prune_parameters(self):
        raise NotImplementedError("the reference %s has no prune hook" % type(self).__name__)

    def forward(self, x):
        """(T, B, F) -> (T, B, out_dim) on the pkc kernels, trainable under autograd (pkc.plugin)."""
        return arch_forward(self, x)

    def check_supported(self):
        pass

    def input_norm_specs(self):
        return []

    def layer_specs(self):
        """Per layer: the packed per-direction weights (one projection matmul per direction gives
        all gates) and the inter-layer dropout of its output (none after the last layer)."""
        P = getattr(self, self.std_cell)[0]
        nd = 2 if self.bidirectional else 1
        specs = []
        for l in range(self.num_layers):
            sfx = ["_l%d%s" % (l, "_reverse" if d else "") for d in range(nd)]
            get = lambda n: [getattr(P, n + s, None) for s in sfx]      # noqa: E731
            specs.append(dict(std=self.std_cell, H=self.hidden_size, act=self.nonlinearity,
                              bidir=bool(self.bidirectional), ndir=nd, bn=False, bnm=[], ln=False,
                              drop=self.dropout if l < self.num_layers - 1 else 0.0,
                              W=get("weight_ih"), U=get("weight_hh"), bih=get("bias_ih"),
                              bhh=get("bias_hh"), Wmask=None, Umask=None, ibits=0, qbits=0))
            if self.proj_size:
                specs[-1].update(P=self.proj_size, Whr=get("weight_hr"))
        return specs


class LSTM_cudnn(_StdRec):
    """neural_networks.py:364-397 (nn.LSTM; gate rows i, f, g, o).  Parameters lstm.0.*."""
    std_cell = "lstm"
    STD_GATES = 4


class GRU_cudnn(_StdRec):
    """neural_networks.py:400-430 (nn.GRU; gate rows r, z, n).  Parameters gru.0.*."""
    std_cell = "gru"
    STD_GATES = 3


class RNN_cudnn(_StdRec):
    """neural_networks.py:433-465 (nn.RNN, nonlinearity tanh | relu).  Parameters rnn.0.*."""
    std_cell = "rnn"
    STD_GATES = 1


class _SruCell(nn.Module):
    """One SRU layer's parameters under the names of the published `sru` package's state dict
    (weight, weight_c, bias, in that order).  The draws are pkc's own, per layer with torch's
    generator and in this order: weight ~ U(+-sqrt(3 / n_in)); weight_c ~ U(+-sqrt(3)), times
    sqrt(0.5) with rescale; bias = 0 with the b_r half set to highway_bias."""

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


class _SruHolder(nn.Module):
    def __init__(self, cells):
        super().__init__()
        self.rnn_lst = nn.ModuleList(cells)


class SRU(nn.Module):
    """The Simple Recurrent Unit (Lei et al., EMNLP 2018, the v2 cell with the highway scaling
    alpha; options per proto/SRU.proto).  A pkc extension: the reference keeps its SRU class
    commented out and the package it wraps is not runnable here, so the semantics are fixed from the
    paper (include/pkc.h, pkc_sru_args) and pinned against nothing.  Parameters
    sru.rnn_lst.<l>.weight (n_in, n_out*k), .weight_c (2 n_out) = [v_f | v_r], .bias (2 n_out) =
    [b_f | b_r]; k = 4 when the skip term is on and n_in != n_out (layer 0 only), else 3."""

    seq_model = True
    REFUSED = ("sru_use_selu", "sru_weight_norm", "sru_layer_norm", "sru_is_input_normalized")

    def __init__(self, options, inp_dim):
        super().__init__()
        o = options
        for k in o:
            if any(w in k for w in ("hcgs", "quant", "prune", "pattern")):
                raise NotImplementedError("SRU: the key %s (CGS / quantisation / pruning) is not "
                                          "supported" % k)
            if "laynorm" in k or "batchnorm" in k:
                raise NotImplementedError("SRU: the input normalisation key %s is not supported" % k)
        for k in self.REFUSED:
            if strtobool(o.get(k, "False")):
                raise NotImplementedError("SRU: %s = True is not on the pkc path" % k)
        if int(o.get("sru_n_proj", "0")) != 0:
            raise NotImplementedError("SRU: sru_n_proj = %s (only 0) is not on the pkc path"
                                      % o["sru_n_proj"])
        self.input_dim = inp_dim
        self.hidden_size = int(o["sru_hidden_size"])
        self.num_layers = int(o["sru_num_layers"])
        self.dropout = float(o["sru_dropout"])
        self.rnn_dropout = float(o["sru_rnn_dropout"])
        for key, p in (("sru_dropout", self.dropout), ("sru_rnn_dropout", self.rnn_dropout)):
            if not 0.0 <= p < 1.0:
                raise ValueError("SRU: %s = %s is outside [0, 1)" % (key, o[key]))
        # tanh wins if both are set
        self.act = ("tanh" if strtobool(o["sru_use_tanh"]) else
                    "relu" if strtobool(o["sru_use_relu"]) else "linear")
        self.bidirectional = strtobool(o["sru_bidirectional"])
        self.has_skip_term = strtobool(o["sru_has_skip_term"])
        self.rescale = strtobool(o["sru_rescale"])
        self.highway_bias = float(o["sru_highway_bias"])
        self.alpha = (math.sqrt(1.0 + 2.0 * math.exp(self.highway_bias))
                      if (self.rescale and self.has_skip_term) else 1.0)
        self.to_do = o.get("to_do", "train")
        self.prune = False
        self.guided_hcgs = False
        self.apply_guided_hcgs = False
        self.if_pattern = False
        self.skip_regularization = False
        self.out_dim = self.hidden_size * (2 if self.bidirectional else 1)
        cells, n_in = [], inp_dim
        for _ in range(self.num_layers):
            k = 4 if (self.has_skip_term and n_in != self.out_dim) else 3
            cells.append(_SruCell(n_in, self.out_dim, k, self.rescale, self.highway_bias))
            n_in = self.out_dim
        self.sru = _SruHolder(cells)

    def prune_parameters(self):
        raise NotImplementedError("SRU has no prune hook")

    def forward(self, x):
        """(T, B, F) -> (T, B, out_dim) on the pkc kernels, trainable under autograd (pkc.plugin)."""
        return arch_forward(self, x)

    def check_supported(self):
        pass

    def input_norm_specs(self):
        return []

    def layer_specs(self):
        """Per layer: the one projection weight of both directions, the recurrence vectors, the
        dropout of the layer's g(c) term (drop) and of the projection's input (rnn_drop)."""
        specs = []
        for cell in self.sru.rnn_lst:
            n_in, nk = cell.weight.shape
            specs.append(dict(sru=True, H=self.hidden_size, ndir=2 if self.bidirectional else 1,
                              bidir=bool(self.bidirectional), k=nk // self.out_dim, n_in=n_in,
                              act=self.act, skip=bool(self.has_skip_term), alpha=self.alpha,
                              drop=self.dropout, rnn_drop=self.rnn_dropout,
                              weight=cell.weight, weight_c=cell.weight_c, bias=cell.bias,
                              W=[cell.weight], U=[], bn=False, bnm=[], ln=False, Wmask=None,
                              Umask=None, ibits=0, qbits=0))
        return specs

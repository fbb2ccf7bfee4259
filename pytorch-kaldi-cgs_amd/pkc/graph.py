"""pkc.graph — the vocabulary of the cfg [model] graph that pkc.engine executes: the line grammar
(parse_model, resolve_concat), the loss terms that are not heads (RegTerm, MseTerm), a sentence
batch (SeqBatch), the graph nodes (Node and its seven kinds), the convolution / sinc argument structs
and an architecture's pattern masks.  Nothing here launches a step or reads a kernel-form switch;
it imports nothing from pkc.engine, which re-exports these names.
"""
import ctypes as C
import re

import numpy as np
import torch

from . import _lib as L
from ._lib import call, ptr
from .cgs import kmeans_patterns

_PAT = re.compile(r"(.*)=(.*)\((.*),(.*)\)")
_PAT3 = re.compile(r"(.*)=(.*)\((.*),(.*),(.*)\)")


def parse_model(text):
    """utils.py:1888-1903 line grammar: out=op(in1,in2), split at the LAST comma (greedy); a line
    whose output name starts with 'loss_gl' is re-read as out=op(in1,in2,in3) (1904-1906), and
    in3 rides in in2 as "in2,in3"."""
    rows = []
    for line in text.split("\n"):
        if not line.strip():
            continue
        row = list(_PAT.findall(line)[0])
        if row[0][:7] == "loss_gl":
            o, op, a, b, c = _PAT3.findall(line)[0]
            row = [o, op, a, b + "," + c]
        rows.append(row)
    return rows


class RegTerm:
    """One cost_l1 / cost_l2 / cost_gl line of the [model] (utils.py:24-60): a pseudo loss head
    whose per-row 'loss' is the regulariser value (pkc_reg_finalize broadcasts it)."""
    head = False

    def __init__(self, op, lam, nblk, params):
        self.op, self.lam, self.nblk, self.params = op, float(lam), nblk, params
        self.kind = L.REG_L1 if op == "cost_l1" else L.REG_L2
        self.loss_weight = 0.0

    def items(self, grads):
        """Row-slice items of every block, blocks in parameter order (gl: the torch.chunk grid
        along dim 1, then dim 0 — utils.py:49-54)."""
        items, bstart = [], [0]
        for p in self.params:
            R, Cc = p.shape[0], int(np.prod(p.shape[1:]))
            if self.op == "cost_gl":
                cs, rs = -(-Cc // self.nblk), -(-R // self.nblk)
                cgrid = [(c, min(c + cs, Cc)) for c in range(0, Cc, cs)]
                rgrid = [(r, min(r + rs, R)) for r in range(0, R, rs)]
                rects = [(r0, r1, c0, c1) for c0, c1 in cgrid for r0, r1 in rgrid]
            else:
                rects = [(0, R, 0, Cc)]
            g = grads.get(id(p))
            for r0, r1, c0, c1 in rects:
                per = max(1, 4096 // max(1, c1 - c0))
                for a in range(r0, r1, per):
                    items.append((p, g, Cc, a, min(a + per, r1), c0, c1, len(bstart) - 1))
                bstart.append(len(items))
        return items, bstart


class MseTerm:
    """One mse line of the [model] (utils.py:2045-2048: torch.mean((a - b) ** 2)) between a
    feed-forward node's output and a feature stream of the chunk: a loss term whose per-row loss
    is the row's mean square (pkc_mse_fused), and one more gradient source of its node."""
    head = False

    def __init__(self, node, c0, name):
        self.node, self.c0, self.name = node, c0, name
        self.loss_weight = 0.0


def resolve_concat(lines, fea_cols):
    """[model] concatenate(a, b) (utils.py:2014-2016: torch.cat along the feature axis) of feature
    streams — or of earlier such concatenations — whose column ranges are adjacent in the chunk
    matrix: read_lab_fea stacks the streams in fea_dict order (data_io.py:235-240), which is the
    order the [model] first names them, so the result is the column range spanning both, a
    zero-copy view of the chunk.  Returns fea_cols with those names added; every other
    concatenate (a produced output on either side, streams that are not adjacent) is left to the
    graph, where it becomes a CombineNode."""
    cols = dict(fea_cols)
    for out, op, a, b in lines:
        if op != "concatenate":
            continue
        if a in cols and b in cols and cols[a][1] == cols[b][0]:
            cols[out] = (cols[a][0], cols[b][1])
        # (any other concatenate is a CombineNode of the graph, Engine._build_graph)
    return cols


class SeqBatch(tuple):
    """(begin rows, lengths, left pads, T) of one sentence batch, plus .index: the batch's
    position in the bound chunk (its data-parallel frame weight, Engine.frame_scales)."""

    def __new__(cls, items, index):
        t = tuple.__new__(cls, items)
        t.index = index
        return t


def _f32(n, dev):
    return torch.zeros(int(max(1, n)), dtype=torch.float32, device=dev)


def _b(v):
    return str(v).strip().lower() in ("1", "true", "yes", "y", "on", "t")


class Node:
    """What the engine may read on ANY graph node, stated once: class-level defaults for what a
    node kind does not have (so the dense code paths fall through: `n.W is None` is an input norm,
    a combine, a conv or a recurrent node) or the engine sets later, for some nodes only.  A plain
    class: nodes are dictionary keys by identity (Engine.needs_grad, ...): no __eq__ / __hash__."""
    # --- kind flags: a subclass sets its own
    rec = False             # RecNode / StdRecNode: a whole recurrent architecture
    conv = False            # ConvNode: Conv1d + max-pool
    combine = False         # CombineNode: a [model] tensor operation
    std = False             # StdRecNode: torch.nn.LSTM / GRU / RNN cells
    sru = False             # SruNode: Simple Recurrent Unit layers (one-launch time loops)
    head = False            # a Layer ending in LogSoftmax
    # --- dense fall-through: what a Layer has and the other kinds do not
    W = None                # weight of the engine's own matmul (None: the node has none)
    b = None                # its bias
    mask = None             # HCGS (x pattern) mask of W
    Wq = None               # fake-quantised copy of W the matmuls multiply with (qbits)
    W_h = None              # bf16 copy of W (Engine._build_h16)
    qbits = 0               # weight fake-quantisation bits (0: off)
    ibits = 0               # input fake-quantisation bits (0: off)
    reads = 0               # in-place quantisations of its input that the node applies
    bn = False              # BatchNorm after the matmul / convolution
    ln = False              # LayerNorm after the matmul / convolution
    act = "linear"          # activation
    drop = 0.0              # dropout probability of the output
    arch = None             # architecture name (None: no parameters, no optimizer section)
    # --- set later by the engine, for some nodes only
    rec_consumer = None     # the recurrent node reading this output (_build_graph)
    gsrc = None             # (buffer, slabs, stride) of the output gradient when it is not gslab
    out_h = None            # bf16 copy of the output for bf16 consumer matmuls (_build_h16)
    dz_h = None             # bf16 copy of dL/dz (_build_h16)
    bn_states = None        # SyncBN: every rank's forward column state (_alloc)
    bn_sums = None          # SyncBN: backward column sums (_alloc)
    bnb_epi = None          # BnBwdEpi of the consumer's dX matmul epilogue (_bnb_ok)
    keep = None             # dropout keep mask (_alloc, drop > 0)
    sdw = 1                 # split-K slabs of dW (_alloc)
    f32_dead = False        # a training step stores no fp32 output (_build_h16)
    dz_scratch = False      # fp32 dz is scratch, the bf16 copy the result (_build_h16)
    bnb_now = False         # this step's BatchNorm-backward statistics came with a dX matmul
    mse_grad = ()           # weighted mse terms on the output (a list, _build_graph)
    qv0 = 0                 # input version current when the node runs (_build_quant)

    def _wire(self):
        """Per-instance wiring, filled in by Engine._build_graph."""
        self.src = None          # ("fea", c0, c1) or ("node", producer)
        self.consumers = []
        self.label_col = None
        self.loss_weight = 0.0

    def quant_of(self, p):
        return (None, 0)

    def _norm_params(self):
        """(parameter, gradient name, mask) of the node's LayerNorm, then of its BatchNorm."""
        ln = [(self.ln_gamma, "dgamma_ln", None), (self.ln_beta, "dbeta_ln", None)]
        bn = [(self.gamma, "dgamma", None), (self.beta, "dbeta", None)]
        return (ln if self.ln else []) + (bn if self.bn else [])


class Layer(Node):
    """One dense layer of an MLP architecture inside the graph."""

    def __init__(self, arch, idx, spec, K):
        self._wire()
        self.arch, self.idx, self.K = arch, idx, K
        self.N = spec["out"]
        self.spec = spec
        self.act = spec["act"]
        self.head = self.act == "softmax"
        self.bn = spec["bn"]
        self.drop = float(spec["drop"])
        self.W, self.b = spec["W"], spec["b"]
        self.gamma, self.beta, self.rm, self.rv = spec["gamma"], spec["beta"], spec["rm"], spec["rv"]
        self.mask = spec["mask"]
        self.nbt0 = int(spec["nbt"].item()) if spec.get("nbt") is not None else 0
        self.name = "%s.%d" % (arch, idx)
        if self.head and self.bn:
            raise NotImplementedError("%s: BatchNorm before LogSoftmax is not on the pkc path" % self.name)
        self.ln = bool(spec["ln"])                # LayerNorm between the Linear and BN / act
        self.ln_gamma, self.ln_beta = spec.get("ln_gamma"), spec.get("ln_beta")
        if self.act not in L.ACT and not self.head:
            raise NotImplementedError("%s: activation %s" % (self.name, self.act))
        self.qbits = int(spec["quant"] or 0)      # QuantizeLinear weight bits (0: nn.Linear)
        self.ibits = int(spec["inp_quant"] or 0)  # QuantizeLinear input bits (0: off)
        self.reads = 1 if self.ibits else 0       # in-place input quantisations this layer applies

    def params(self):
        return [(self.W, "dW", self.mask), (self.b, "db", None)] + self._norm_params()

    def quant_of(self, p):
        return (self.Wq, self.qbits) if (p is self.W and self.qbits) else (None, 0)


class NormLayer(Layer):
    """An MLP's input LayerNorm / BatchNorm (dnn_use_laynorm_inp / dnn_use_batchnorm_inp,
    neural_networks.py:246-251): a node with no matmul, normalising the arch's input."""

    def __init__(self, arch, idx, spec, K):
        self._wire()             # (not Layer.__init__: no matmul, so none of its spec keys)
        self.arch, self.idx, self.K, self.N = arch, idx, K, K
        self.spec = spec
        self.kind = spec["kind"]
        self.bn, self.ln = self.kind == "bn", self.kind == "ln"
        self.gamma, self.beta = spec["gamma"], spec["beta"]
        self.ln_gamma, self.ln_beta = spec["gamma"], spec["beta"]
        self.rm, self.rv = spec.get("rm"), spec.get("rv")
        self.nbt0 = int(spec["nbt"].item()) if spec.get("nbt") is not None else 0
        self.name = "%s.inp_%s%d" % (arch, self.kind, idx)

    def params(self):
        return self._norm_params()         # (ln_gamma / ln_beta are gamma / beta here)


TENSOR_OPS = ("concatenate", "mult", "sum", "avg", "sum_constant", "mult_constant")


class CombineNode(Node):
    """One [model] tensor operation on produced outputs (utils.py:2014-2043: concatenate, mult,
    sum, mult_constant, sum_constant, avg) as a graph node.  For its neighbours it is a node with
    no matmul and no parameters (W is None, like an input norm): N, out (rows, N), its consumers'
    dX slabs (or a recurrent consumer's layer-0 dX slabs) as its output gradient.  It has two
    sources, each ("node", P) or ("fea", c0, c1) — one for the constant forms, whose second
    operand is the float `c` — and writes each producer's gradient into ONE slab of that
    producer's gradient slabs (cons_idx: its positions in the producers' consumer lists)."""
    combine = True

    def __init__(self, out, op, srcs, widths, c=0.0):
        self._wire()             # (src stays None: its sources are srcs)
        self.op, self.srcs, self.c = op, srcs, float(c)
        self.name = "%s=%s" % (out, op)
        self.Na, self.Nb = widths[0], (widths[1] if len(widths) > 1 else 0)
        if op not in ("concatenate", "sum_constant", "mult_constant") and self.Na != self.Nb:
            raise NotImplementedError("%s: operands %d and %d wide (only concatenate takes "
                                      "unequal widths)" % (self.name, self.Na, self.Nb))
        self.N = self.Na + self.Nb if op == "concatenate" else self.Na
        self.K = self.N
        self.cons_idx = []
        self.heads_in = any(s[0] == "node" and s[1].head for s in srcs)

    def params(self):
        return []


class ConvNode(Node):
    """One Conv1d + max-pool layer of a CNN / SincNet architecture (neural_networks.py:2017-2029,
    :2127-2139) as a graph node.  For its neighbours it is a dense node with no matmul of the
    engine's own (W is None): N = C_out * L_out, out (rows, N) channel-major, consumers' dX slabs
    (or a recurrent consumer's) as its output gradient, dX into its producer's slab.  The
    convolution products are exact fp32 in every pkc_prec mode.  A sinc layer (SincNet's layer 0)
    convolves with an engine-owned filter buffer regenerated from low_hz_ / band_hz_ at the start
    of every forward; those two are its parameters, its dW a work buffer."""
    conv = True

    def __init__(self, arch, idx, spec, K):
        self._wire()
        self.arch, self.idx, self.spec = arch, idx, spec
        self.C_in, self.C_out, self.L_in, self.L_out = (spec["C_in"], spec["C_out"], spec["L_in"],
                                                        spec["L_out"])
        self.len, self.pool = spec["len"], spec["pool"]
        if K != self.C_in * self.L_in:
            raise ValueError("%s.conv%d: input width %d != C_in * L_in = %d"
                             % (arch, idx, K, self.C_in * self.L_in))
        self.K, self.N = K, self.C_out * self.L_out
        self.name = "%s.conv%d" % (arch, idx)
        self.act, self.drop = spec["act"], float(spec["drop"])
        self.bn, self.ln = bool(spec["bn"]), bool(spec["ln"])
        if self.bn and self.ln:
            raise NotImplementedError("%s: LayerNorm and BatchNorm both set (the reference then "
                                      "convolves twice, neural_networks.py:2019-2025)" % self.name)
        if self.act not in L.ACT:
            raise NotImplementedError("%s: activation %s on a convolution layer" % (self.name, self.act))
        self.sinc = spec.get("sinc")
        if self.sinc is not None:
            sinc_bind(spec)
        self.cW, self.cb = spec["W"], spec["b"]
        self.gamma, self.beta, self.rm, self.rv = spec["gamma"], spec["beta"], spec["rm"], spec["rv"]
        self.ln_gamma, self.ln_beta = spec["ln_gamma"], spec["ln_beta"]
        self.nbt0 = int(spec["nbt"].item()) if spec.get("nbt") is not None else 0

    def params(self):
        if self.sinc is not None:
            out = [(self.sinc["low"], "dlow", None), (self.sinc["band"], "dband", None)]
        else:
            out = [(self.cW, "dW", None), (self.cb, "db", None)]
        return out + self._norm_params()


def conv_args(sp, rows, x_ptr, ldx, z, off):
    """pkc_conv1d_args of a conv_specs() entry over `rows` samples."""
    a = L.Conv1dArgs(B=rows, C_in=sp["C_in"], L_in=sp["L_in"], C_out=sp["C_out"], len=sp["len"],
                     pool=sp["pool"], x=x_ptr, ldx=ldx, W=sp["W"].data_ptr(),
                     bias=sp["b"].data_ptr(), z=z.data_ptr(), off=off.data_ptr())
    if L.lib().pkc_conv1d_ok(C.byref(a)) != 1:
        raise NotImplementedError("convolution shape not on the pkc path: %s"
                                  % L.lib().pkc_last_error().decode())
    return a


def sinc_bind(sp):
    """Buffers of a sinc layer's conv_specs() entry: the generated filters as its W, a zero bias
    (SincConv has none), the maximum and its index per filter, n_ and window_ on the device."""
    sn = sp["sinc"]
    dev, N, K = sn["low"].device, sp["C_out"], sp["len"]
    sp["W"], sp["b"] = _f32(N * K, dev).view(N, 1, K), _f32(N, dev)
    sn["max_"], sn["idx"] = _f32(N, dev), torch.zeros(N, dtype=torch.int32, device=dev)
    sn["n_dev"] = sn["n_"].detach().reshape(-1).to(dev, torch.float32).contiguous()
    sn["window_dev"] = sn["window"].detach().reshape(-1).to(dev, torch.float32).contiguous()
    sinc_args(sp)


def sinc_args(sp, **kw):
    """pkc_sinc_args of a bound sinc layer."""
    sn = sp["sinc"]
    a = L.SincArgs(N=sp["C_out"], K=sp["len"], low_hz=sn["low"].data_ptr(),
                   band_hz=sn["band"].data_ptr(), n_=sn["n_dev"].data_ptr(),
                   window=sn["window_dev"].data_ptr(), sr=sn["sr"], min_low_hz=sn["min_low_hz"],
                   min_band_hz=sn["min_band_hz"], filters=sp["W"].data_ptr(),
                   max_=sn["max_"].data_ptr(), max_idx=sn["idx"].data_ptr(), **kw)
    if (sn["n_dev"].numel() != a.K or sn["window_dev"].numel() != a.K
            or L.lib().pkc_sinc_ok(C.byref(a)) != 1):
        raise NotImplementedError("sinc filter bank not on the pkc path: %s"
                                  % L.lib().pkc_last_error().decode())
    return a


def conv_post_args(sp, rows, z, train, out, **kw):
    """pkc_conv_post_args of a conv_specs() entry (norm / activation / dropout after the pool)."""
    if sp["ln"]:
        norm, g, b, eps = L.CONV_NORM_LN, sp["ln_gamma"], sp["ln_beta"], sp.get("ln_eps", 1e-6)
    elif sp["bn"]:
        # eps = L_out: neural_networks.py:1988-1990 passes it as BatchNorm1d's second argument
        norm, g, b, eps = (L.NORM_BN_TRAIN if train else L.NORM_BN_EVAL, sp["gamma"], sp["beta"],
                           sp["bn_eps"])
    else:
        norm, g, b, eps = L.NORM_NONE, None, None, 0.0
    return L.ConvPostArgs(B=rows, C=sp["C_out"], L=sp["L_out"], norm=norm, z=z.data_ptr(),
                          gamma=ptr(g), beta=ptr(b), running_mean=sp["rm"].data_ptr(),
                          running_var=sp["rv"].data_ptr(), momentum=sp.get("bn_momentum", 0.05),
                          eps=eps, act=L.ACT[sp["act"]], out=out.data_ptr(), **kw)


class RecNode(Node):
    """A whole liGRU / LSTM architecture (all its layers) as one graph node."""
    rec = True

    def __init__(self, arch, net, K):
        self._wire()
        self.arch, self.net, self.K = arch, net, K
        self.name = arch
        self.cell = {"lstm": L.CELL_LSTM, "gru": L.CELL_GRU, "ligru": L.CELL_LIGRU,
                     "minimalgru": L.CELL_MINGRU, "rnn": L.CELL_RNN}[net.cell]
        self.G = {L.CELL_LSTM: 4, L.CELL_GRU: 3, L.CELL_LIGRU: 2, L.CELL_MINGRU: 2,
                  L.CELL_RNN: 1}[self.cell]
        # two-phase cells: the candidate gate's U multiplies r*h (GRU) / z*h (minimalGRU)
        self.cand = {L.CELL_GRU: 2, L.CELL_MINGRU: 1}.get(self.cell)
        self.layers = net.layer_specs()
        self.N = net.out_dim
        for sp in self.layers:
            if sp["act"] not in L.ACT:
                raise NotImplementedError("%s: activation %s" % (arch, sp["act"]))
            sp["nbt0"] = [int(bn.num_batches_tracked.item()) for bn in sp["bnm"]]
            sp.setdefault("qbits", 0)
            sp.setdefault("ibits", 0)
            if sp["ibits"] and sp["bidir"]:
                raise NotImplementedError("%s: input quantisation of a bidirectional layer" % arch)
        # in-place quantisations of the node's input (gate linears of layer 0)
        self.ibits = self.layers[0]["ibits"]
        self.reads = self.G if self.ibits else 0
        self.qw = {}            # id(param) -> fake-quantised copy
        self.emask = {}         # id(param) -> effective (HCGS x pattern) mask

    def params(self):
        out = []
        for li, sp in enumerate(self.layers):
            for g in range(self.G):
                W = sp["W"][g]
                wm = sp["Wmasks"][g] if sp.get("Wmasks") else sp["Wmask"]
                out.append((W, ("dW", li, g), self.emask.get(id(W), wm)))
                if sp["b"][g] is not None:
                    out.append((sp["b"][g], ("db", li, g), None))
            for g in range(self.G):
                U = sp["U"][g]
                um = sp["Umasks"][g] if sp.get("Umasks") else sp["Umask"]
                out.append((U, ("dU", li, g), self.emask.get(id(U), um)))
            if sp["bn"]:
                for g in range(self.G):
                    out.append((sp["bnm"][g].weight, ("dgamma", li, g), None))
                    out.append((sp["bnm"][g].bias, ("dbeta", li, g), None))
            if sp.get("ln"):
                out.append((sp["ln_gamma"], ("dgamma_ln", li, 0), None))
                out.append((sp["ln_beta"], ("dbeta_ln", li, 0), None))
        return out

    def quant_of(self, p):
        return self.qw.get(id(p), (None, 0))

    def wq(self, li, kind, g):
        """The weight a GEMM / the time loop multiplies with (fake-quantised when quantised)."""
        p = self.layers[li][kind][g]
        q = self.qw.get(id(p))
        return q[0] if q is not None else p


class StdRecNode(RecNode):
    """A whole LSTM_cudnn / GRU_cudnn / RNN_cudnn architecture (torch.nn.LSTM / GRU / RNN) as one
    graph node: per layer and direction a packed weight_ih (G*H, K), weight_hh (G*H, H) and the two
    biases, the standard-cell time loops of pkc_rnn_std_fwd / _bwd, dropout between layers.
    layer_specs() contract: dict(std, H, act, bidir, ndir, drop (of the layer's output; 0 on the
    last), W / U / bih / bhh: one entry per direction (biases None without bias)).  The projected
    LSTM (LSTM_cudnn with proj_size = P) adds P and Whr (weight_hr (P, H) per direction): its
    weight_hh is (4H, P), its output ndir * P wide and its time loops pkc_lstmp_fwd / _bwd."""
    std = True

    def __init__(self, arch, net, K):
        self._wire()             # (not RecNode.__init__: packed per-direction layer specs)
        self.arch, self.net, self.K = arch, net, K
        self.name = arch
        self.std_cell = net.std_cell
        self.cell = None                 # none of the pkc_rnn_args cells
        self.cid = {"lstm": L.STD_LSTM, "gru": L.STD_GRU, "rnn": L.STD_RNN}[net.std_cell]
        self.G = net.STD_GATES
        # gate-gradient slabs per row: the GRU keeps r * da_n (recurrent side) beside da_n
        self.GD = 4 if net.std_cell == "gru" else self.G
        self.cand = None
        self.layers = net.layer_specs()
        self.N = net.out_dim
        for sp in self.layers:
            if sp["act"] not in ("tanh", "relu"):
                raise NotImplementedError("%s: nonlinearity %s (tanh or relu)" % (arch, sp["act"]))
            if not 0.0 <= sp["drop"] < 1.0:
                raise ValueError("%s: dropout %s outside [0, 1)" % (arch, sp["drop"]))
            if sp.get("P") and not (net.std_cell == "lstm" and 0 < sp["P"] < sp["H"]):
                raise ValueError("%s: proj_size %s (LSTM only, 0 < proj_size < hidden_size = %d)"
                                 % (arch, sp["P"], sp["H"]))
        self.qw = {}
        self.emask = {}

    def params(self):
        out = []
        for li, sp in enumerate(self.layers):
            for d in range(sp["ndir"]):
                out.append((sp["W"][d], ("dW", li, d), None))
                out.append((sp["U"][d], ("dU", li, d), None))
                if sp["bih"][d] is not None:
                    out.append((sp["bih"][d], ("dbih", li, d), None))
                    out.append((sp["bhh"][d], ("dbhh", li, d), None))
                if sp.get("P"):
                    out.append((sp["Whr"][d], ("dWhr", li, d), None))
        return out


class SruNode(RecNode):
    """A whole SRU architecture as one graph node: per layer ONE projection weight (n_in, n_out*k)
    of both directions, the recurrence vectors weight_c and bias, and the one-launch time loops of
    pkc_sru_fwd / _bwd.  layer_specs() contract: dict(sru, H, ndir, k, n_in, act, skip, alpha, drop
    (of the g(c) term), rnn_drop (of the projection's input), weight, weight_c, bias)."""
    sru = True

    def __init__(self, arch, net, K):
        self._wire()             # (not RecNode.__init__: no gates of pkc_rnn_args)
        self.arch, self.net, self.K = arch, net, K
        self.name = arch
        self.cell = None                 # none of the pkc_rnn_args cells
        self.G, self.cand = 1, None
        self.layers = net.layer_specs()
        self.N = net.out_dim
        for sp in self.layers:
            if sp["act"] not in ("linear", "relu", "tanh"):
                raise NotImplementedError("%s: activation %s" % (arch, sp["act"]))
            for key in ("drop", "rnn_drop"):
                if not 0.0 <= sp[key] < 1.0:
                    raise ValueError("%s: dropout %s outside [0, 1)" % (arch, sp[key]))
        if self.layers[0]["n_in"] != K:
            raise ValueError("%s: built for %d inputs, reads %d" % (arch, self.layers[0]["n_in"], K))
        self.qw = {}
        self.emask = {}

    def params(self):
        out = []
        for li, sp in enumerate(self.layers):
            out += [(sp["weight"], ("dweight", li, 0), None), (sp["weight_c"], ("dwc", li, 0), None),
                    (sp["bias"], ("dbias", li, 0), None)]
        return out


def pattern_effective_masks(net, s):
    """Pattern masks (neural_networks.py:263-272, 876-884; sparsity.py:1112-1146) of one
    architecture: computed once, at the first layer call, from |W| of every pattern-masked weight —
    layer 0's input weights already multiplied by their HCGS mask, every other weight raw — and
    then multiplied into all of them once per layer call (L times per forward; {0,1} except on
    tied tiles).  Masks already held in ``net.pattern_mask`` (carried between chunks by run_nn,
    core.py:129-131, 304-306) are reused, as the reference does; new ones are stored there in the
    reference's structure.  Each weight's pattern set is, in order: the one carried in
    ``net.pattern``; the shared set (``pattern_kernels`` / ``pattern_from_file``); or a KMeans
    search of that weight (update_patterns, neural_networks.py:339-348, 1162-1172), stored back
    into ``net.pattern``.  Returns {id(param): HCGS x pattern^L effective mask}."""
    if not getattr(net, "if_pattern", False):
        return {}
    dev = next(net.parameters()).device
    entries = net.pattern_params()
    nl = 1 + max(e[1] for e in entries)
    store, pstore = net.pattern_mask, net.pattern
    have = all(_pm_get(store, key) is not None for key, _, _, _ in entries)
    shared = net.pattern_kernels
    if shared is None and not have and not net.can_search_patterns():
        raise NotImplementedError("%s: pattern masks need a pattern set" % net.arch_name)
    out = {}
    for key, li, p, hmask in entries:
        rows, cols = p.shape
        if have:
            pm = _pm_get(store, key).to(dev, torch.float32).contiguous()
        else:
            pre = li == 0 and hmask is not None and _is_input_weight(key)
            src = (p * hmask if pre else p).contiguous()
            pk = _pm_get(pstore, _pattern_key(key))
            if pk is not None:
                t = pk.detach().cpu().numpy() if torch.is_tensor(pk) else np.asarray(pk)
                pk = t.reshape(t.shape[0], t.shape[-2], t.shape[-1]).astype(np.float32)
            elif shared is not None:
                pk = shared
            else:                               # update_patterns: one KMeans search per weight
                pn, shape, nnz = net.pattern_search_args(li)
                pk = kmeans_patterns(src, pn, shape, nnz, random_state=net.pattern_seed)
            P, ph, pw = pk.shape
            if rows % ph or cols % pw:
                raise NotImplementedError("%s: %dx%d weight not tiled by %dx%d patterns"
                                          % (net.arch_name, rows, cols, ph, pw))
            pat = torch.from_numpy(np.ascontiguousarray(pk, dtype=np.float32)).to(dev)
            pm = torch.empty_like(p)
            call("pkc_pattern_mask", ptr(src), rows, cols, ptr(pat), P, ph, pw, ptr(pm), s)
            _pm_set(store, key, pm)
            if _pm_get(pstore, _pattern_key(key)) is None:
                _pm_set(pstore, _pattern_key(key), pat.view(P, 1, ph, pw))
        e = pm.pow(nl) if nl > 1 else pm.clone()
        out[id(p)] = e * hmask if hmask is not None else e
    return out


def _pattern_key(key):
    """net.pattern key of a net.pattern_mask key: (None, i) for an MLP layer, ('pattern_wfx', i)
    for ('pattern_mask_wfx', i) of an LSTM (neural_networks.py:1162-1172)."""
    name, i = key
    return (None if name is None else name.replace("pattern_mask_", "pattern_"), i)


def _is_input_weight(key):
    name, _ = key
    return name is None or name.startswith("pattern_mask_w")


def _pm_get(store, key):
    name, i = key
    lst = store if name is None else store.get(name, [])
    return lst[i] if i < len(lst) else None


def _pm_set(store, key, v):
    name, i = key
    lst = store if name is None else store.setdefault(name, [])
    while len(lst) <= i:
        lst.append(None)
    lst[i] = v

"""Restatement of the HCGS hook on the GRU, minimalGRU and RNN layers (gru_hcgs / minimalgru_hcgs /
rnn_hcgs): a pkc extension with no reference counterpart, pinned on the LSTM hook's semantics
(reference neural_networks.py:858-861, 980-983) exactly as ligru_hcgs is in oracle.nets.liGRU.

Subclasses of oracle.nets.GRU / minimalGRU / RNN: per layer one W mask hcgsx[i] (n x cur), drawn
after the layer's input Linears, and one U mask hcgsh[i] (n x n), drawn after its recurrent
Linears, layers in order, from numpy's global RNG (oracle.masks.hcgs_conn_mat) — the Linears draw
from torch's RNG, so drawing the masks after the parent constructor gives the same draws.  The
masks are Parameters (state-dict names hcgsx.<i>.mask, hcgsh.<i>.mask, registered in front of the
layer lists) and are multiplied into every gate's .weight.data before each forward."""
import torch
import torch.nn as nn

from oracle import masks as M
from oracle import nets as ON

KEYS = {"GRU": "gru_hcgs", "minimalGRU": "minimalgru_hcgs", "RNN": "rnn_hcgs"}


def _ints(o, k, f=int):
    return [f(v) for v in str(o[k]).split(",")]


class _HookMixin:
    HOOK_KEY = ""
    HOOK_GATES = ()

    def _init_hook(self, o, inp_dim):
        self.hcgs_on = str(o.get(self.HOOK_KEY, "False")).lower() in ("true", "1", "yes")
        if not self.hcgs_on:
            return
        bx, dx = _ints(o, "hcgsx_block"), _ints(o, "hcgsx_sparse", float)
        bh, dh = _ints(o, "hcgsh_block"), _ints(o, "hcgsh_sparse", float)
        self.hcgsx, self.hcgsh = nn.ModuleList(), nn.ModuleList()
        cur = inp_dim
        for n in self.lay:
            for lst, shape, b, d in ((self.hcgsx, (n, cur), bx, dx), (self.hcgsh, (n, n), bh, dh)):
                hm = nn.Module()
                hm.mask = nn.Parameter(torch.from_numpy(M.hcgs_conn_mat(shape[0], shape[1], b, d)))
                lst.append(hm)
            cur = 2 * n if self.bidir else n
        mods = dict(self._modules)               # registered first, as the LSTM's lists are
        self._modules.clear()
        for name in ["hcgsx", "hcgsh"] + [k for k in mods if not k.startswith("hcgs")]:
            self._modules[name] = mods[name]

    def apply_masks(self):
        if not self.hcgs_on:
            return
        for i in range(len(self.lay)):
            for g in self.HOOK_GATES:
                getattr(self, "w" + g)[i].weight.data.mul_(self.hcgsx[i].mask.data)
                getattr(self, "u" + g)[i].weight.data.mul_(self.hcgsh[i].mask.data)

    def forward(self, x, drop_masks=None):
        self.apply_masks()
        return super().forward(x, drop_masks=drop_masks)


class GRU(_HookMixin, ON.GRU):
    HOOK_KEY, HOOK_GATES = "gru_hcgs", ("h", "z", "r")

    def __init__(self, o, inp_dim):
        super().__init__(o, inp_dim)
        self._init_hook(o, inp_dim)


class minimalGRU(_HookMixin, ON.minimalGRU):
    HOOK_KEY, HOOK_GATES = "minimalgru_hcgs", ("h", "z")

    def __init__(self, o, inp_dim):
        super().__init__(o, inp_dim)
        self._init_hook(o, inp_dim)


class RNN(_HookMixin, ON.RNN):
    HOOK_KEY, HOOK_GATES = "rnn_hcgs", ("h",)

    def __init__(self, o, inp_dim):
        super().__init__(o, inp_dim)
        self._init_hook(o, inp_dim)


GATES = {"GRU": ("h", "z", "r"), "minimalGRU": ("h", "z"), "RNN": ("h",)}
HOOK = dict(hcgsx_block="8,4", hcgsx_sparse="50,50", hcgsh_block="8,4", hcgsh_sparse="25,50")

# (tag, class, lay, bidir, seed) of tests/golden/gru_hcgs.npz (make_golden_gru_hcgs.py): T = 6,
# B = 3, F = 20, masks [8,4] / [50,50] on W and U
GOLDEN_T, GOLDEN_B, GOLDEN_F = 6, 3, 20
GOLDEN_HOOK = dict(hcgsx_block="8,4", hcgsx_sparse="50,50", hcgsh_block="8,4", hcgsh_sparse="50,50")
GOLDEN_CASES = [("gru_hcgs_bidir", "GRU", "24,16", True, 41),
                ("mingru_hcgs_uni", "minimalGRU", "24,16", False, 42),
                ("rnn_hcgs_uni", "RNN", "24,16", False, 43)]


def golden_opts(cls, lay, bidir):
    from cases import GRU_DEF, MINGRU_DEF, RNN_DEF
    base, p = {"GRU": (GRU_DEF, "gru"), "minimalGRU": (MINGRU_DEF, "minimalgru"),
               "RNN": (RNN_DEF, "rnn")}[cls]
    return dict(base, **{p + "_lay": lay, p + "_bidir": str(bidir), KEYS[cls]: "True"},
                **GOLDEN_HOOK)


def hook_opts(cls, base, **kw):
    """`base` options of class `cls` with its HCGS key set and the four hcgs* lists"""
    return dict(base, **{KEYS[cls]: "True"}, **dict(HOOK, **kw))

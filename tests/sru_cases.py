"""The cases of the SRU tests, shared by tests/test_sru_cpu.py and tests/test_gpu_sru.py.

Kernel level: operands of one layer's time loop (the projection U given) and their float64 /
float32 restatement results (computed once per case, cached).  Engine level: `o1=compute(rnn,fea)`
into two softmax heads (the [model], data and padded batches of tests/cudnn_cases.py) with an SRU of
2 x 32 bidirectional, B = 4, T <= 12."""
import configparser
import functools

import torch

import cudnn_cases as CC
import sru_ref as R

# name: (d, T, B, D, k, act, skip, alpha, extra leading dimension of x, dy slabs)
KERNEL_CASES = {
    "d8_T1_B1_uni_k3": (8, 1, 1, 1, 3, "linear", True, 1.0, 0, 1),
    "d8_T7_B3_bi_k4_tanh": (8, 7, 3, 2, 4, "tanh", True, 1.0, 0, 1),
    "d40_T7_B3_bi_k3_relu_alpha_ldx_3slabs": (40, 7, 3, 2, 3, "relu", True, 1.3, 5, 3),
    "d40_T33_B8_uni_k4_3slabs": (40, 33, 8, 1, 4, "linear", True, 1.0, 0, 3),
    "d96_T33_B3_bi_k3_tanh_alpha": (96, 33, 3, 2, 3, "tanh", True, 1.27, 0, 1),
    "d96_T7_B8_bi_k4_relu": (96, 7, 8, 2, 4, "relu", True, 1.0, 0, 1),
    "d40_T33_B1_bi_k3_tanh_noskip": (40, 33, 1, 2, 3, "tanh", False, 1.0, 0, 1),
    "d96_T1_B8_uni_k3_alpha_ldx": (96, 1, 8, 1, 3, "linear", True, 1.3, 7, 1),
    "d8_T33_B8_bi_k3_relu_noskip_3slabs": (8, 33, 8, 2, 3, "relu", False, 1.0, 0, 3),
    "d40_T1_B3_uni_k4_tanh": (40, 1, 3, 1, 4, "tanh", True, 1.0, 0, 1),
    "d8_T7_B1_bi_k4_3slabs": (8, 7, 1, 2, 4, "linear", True, 1.0, 0, 3),
    "d96_T33_B8_bi_k4_tanh": (96, 33, 8, 2, 4, "tanh", True, 1.0, 0, 1),
    # the C3 width: 18 column groups of 64 lanes per sentence (the last one 12 lanes wide), the
    # 16-byte loads of k = 4 and the element loads of k = 3
    "d550_T20_B8_bi_k4_tanh": (550, 20, 8, 2, 4, "tanh", True, 1.0, 0, 1),
    "d550_T20_B8_bi_k3_relu_alpha": (550, 20, 8, 2, 3, "relu", True, 1.27, 0, 1),
}
RTOL, ATOL = 1e-4, 1e-5        # the project's bound for this kind of kernel (tests/test_gpu_cudnn.py)
QUANT = ("y", "c", "dU", "dXh", "dwc", "dbias")


def kernel_operands(name):
    """float32 operands of a case: U (T, B, n*k), xw (T, B, n + extra) whose first n columns are
    the skip term's input, wc, bias (2n), dy (slabs, T, B, n)."""
    d, T, B, D, k, act, skip, alpha, extra, slabs = KERNEL_CASES[name]
    n = d * D
    g = torch.Generator().manual_seed(1 + sorted(KERNEL_CASES).index(name))
    r = lambda *s: torch.randn(*s, generator=g)                                     # noqa: E731
    U, xw = r(T, B, n * k), r(T, B, n + extra)
    wc = (torch.rand(2 * n, generator=g) * 2 - 1) * 1.5 ** 0.5
    bias = torch.cat([0.3 * r(n), -1.0 + 0.3 * r(n)])
    dy = r(slabs, T, B, n) / slabs ** 0.5
    return U, xw, wc, bias, dy


def _restate(name, dtype):
    d, T, B, D, k, act, skip, alpha, extra, slabs = KERNEL_CASES[name]
    U, xw, wc, bias, dy = (t.to(dtype) for t in kernel_operands(name))
    X = xw[:, :, :d * D].contiguous()
    leaves = [t.clone().requires_grad_(True) for t in (U, X, wc, bias)]
    y, c = R.cell_fwd(*leaves, d, D, k, act, skip, alpha)
    (y * dy.sum(0)).sum().backward()
    out = dict(y=y.detach(), c=c.detach(), dU=leaves[0].grad, dwc=leaves[2].grad,
               dbias=leaves[3].grad)
    if k == 3 and skip:
        out["dXh"] = leaves[1].grad
    return out


@functools.lru_cache(maxsize=None)
def kernel_reference(name):
    """({quantity: float64 result}, {quantity: d_ref = max |float32 restatement - float64|},
    {quantity: float32 result})."""
    r64, r32 = _restate(name, torch.float64), _restate(name, torch.float32)
    return r64, {q: float((r32[q].double() - r64[q]).abs().max()) for q in r64}, r32


# ------------------------------------------------------------------------------- engine level
F, B, MAX_LEN, HID, LAYERS = CC.F, CC.B, CC.MAX_LEN, 32, 2
MODEL = CC.MODEL
SRU_OPTS = dict(sru_hidden_size=str(HID), sru_num_layers=str(LAYERS), sru_dropout="0.2",
                sru_rnn_dropout="0.1", sru_use_tanh="True", sru_use_relu="False",
                sru_use_selu="False", sru_weight_norm="False", sru_layer_norm="False",
                sru_bidirectional="True", sru_is_input_normalized="False",
                sru_has_skip_term="True", sru_rescale="True", sru_highway_bias="-1.0",
                sru_n_proj="0")


def make_cfg(optk="rmsprop", **over):
    """cudnn_cases' cfg (two softmax heads, the optimizer sections) with an SRU as the body."""
    cfg = CC.make_cfg("LSTM_cudnn", optk)
    opt = {k: v for k, v in cfg["a1"].items() if k.startswith(("arch_opt", "arch_lr", "opt_",
                                                               "arch_freeze"))}
    a1 = dict(arch_name="rnn", arch_class="SRU", to_do="train", **opt)
    a1.update(SRU_OPTS)
    a1.update(over)
    out = configparser.ConfigParser()
    out["a1"] = a1
    for sec in ("a2", "a3", "model"):
        out[sec] = dict(cfg[sec])
    return out


def build(cfg, mods, dtype=torch.float32):
    return CC.build(cfg, mods, dtype)


def oracle_nets(cfg, dtype=torch.float32):
    from oracle import nets as ON
    nets, opts = build(cfg, (R, ON), dtype)
    for n in nets.values():
        n.train()
    oopt = {k: ON.make_optimizer(nets[k].parameters(), opts[k]) for k in nets}
    return nets, opts, oopt


def make_data():
    lens, end, X, lab, _ = CC.make_data()
    return lens, end, X, lab


def oracle_step(nets, oopt, inp, T, masks, train=True):
    """One run_nn training step (train=False: the forward alone) of the restatement side with the
    SRU's dropout masks {(layer, "c" | "x"): keep (B, width)} given."""
    from oracle import run as OR
    body = nets["rnn"]
    f = body.forward
    body.forward = lambda x, _f=f: _f(x, masks)
    try:
        lines = OR.parse_model(MODEL)
        seq = {"rnn": True, "head": False, "mono": False}
        cols = ({"fea": (0, F)}, {"lab_cd": F, "lab_mono": F + 1})
        if train:
            return OR.train_step(lines, nets, oopt, seq, cols[0], cols[1], inp, T, B)
        with torch.no_grad():
            return OR.forward_model(lines, nets, seq, cols[0], cols[1], inp, T, B)
    finally:
        body.forward = f


def engine_masks(eng):
    """The keep masks the engine's last training step drew, in the restatement's keys."""
    node = next(n for n in eng.nodes if n.rec)
    out = {}
    for l, lb in enumerate(node.lbuf):
        if lb["keep"] is not None:
            out[(l, "c")] = lb["keep"].view(eng.B, lb["D"]).cpu().float()
        if lb["keep_x"] is not None:
            out[(l, "x")] = lb["keep_x"].view(eng.B, lb["K"]).cpu().float()
    return out

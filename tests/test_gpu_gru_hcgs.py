"""HCGS-masked GRU / minimalGRU / RNN layers on the GPU (gru_hcgs / minimalgru_hcgs / rnn_hcgs, a pkc
extension like ligru_hcgs with no reference counterpart, pinned on the LSTM hook's semantics):

* the block-sparse step kernels (two-phase and one-gate forms of rnn_fwd_mm / rnn_bwd_mm reading
  only the 16-wide contraction blocks of their kmap rows) against the dense kernels on the same
  masked weights, and both against tests/golden/gru_hcgs.npz (recorded from the reference's own
  classes with the masks multiplied into .weight.data);
* the engine (training steps, bf16 mode, graph replay, eval / forward mode, the plug-in forward)
  against the restatement tests/gru_hcgs_ref.py;
* one run_nn train -> train -> valid -> forward pass carrying the masks in the .pkl files."""
import configparser
import copy
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from cases import GRU_DEF, MINGRU_DEF, RNN_DEF
from test_gpu_rnn import dx0, run_block, section

import gru_hcgs_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
PREFIX = {"GRU": "gru", "minimalGRU": "minimalgru", "RNN": "rnn"}


def rec_opts(cls, lay, bidir, act="relu", **hook):
    """Options of class `cls` with layers `lay` (BatchNorm on the gates, no dropout) and the hook"""
    p, n = PREFIX[cls], len(lay.split(","))
    rep = lambda v: ",".join([v] * n)      # noqa: E731
    o = {p + "_lay": lay, p + "_drop": rep("0.0"), p + "_use_laynorm_inp": "False",
         p + "_use_batchnorm_inp": "False", p + "_use_laynorm": rep("False"),
         p + "_use_batchnorm": rep("True"), p + "_bidir": str(bidir), p + "_act": rep(act),
         p + "_orthinit": "True", "use_cuda": "False", "to_do": "train"}
    return R.hook_opts(cls, o, **hook)


def sparse_vs_dense(cls, opts, T, B, F, edit=None):
    """y, dx, dU, dW of run_block with PKC_RNN_SPARSE off and force on the same net and data; the
    bound of tests/test_gpu_rnn.py::test_block_sparse_u_matches_dense, unchanged."""
    import pkc.engine as E
    import pkc.neural_networks as NN
    res = []
    for mode in ("off", "force"):
        torch.manual_seed(7)
        np.random.seed(7)
        net = getattr(NN, cls)(section(opts), F)
        if edit:
            edit(net)
        net.to(DEV).train()
        g = torch.Generator().manual_seed(3)
        x = torch.randn(T, B, F, generator=g).to(DEV)
        r = torch.randn(T, B, net.out_dim, generator=g).to(DEV)
        old = E.RNN_SPARSE
        E.RNN_SPARSE = mode
        try:
            eng, node, y = run_block(net, x, r)
        finally:
            E.RNN_SPARSE = old
        if mode == "force":
            maps = [lb[k] for lb in node.lbuf for k in ("kmap_fwd", "kmap_bwd")]
            assert all(m is not None for m in maps)
            assert any(bool((m < 0).any()) for m in maps), "no block skipped: the case tests nothing"
            assert all("block-sparse U" in f for f in eng.rec_forms().values()), eng.rec_forms()
        else:
            assert all(lb["kmap_fwd"] is None and lb["kmap_bwd"] is None for lb in node.lbuf)
            assert all(f == "fp32 steps" for f in eng.rec_forms().values()), eng.rec_forms()
        res.append([y, dx0(eng, node)] + [u for lb in node.lbuf for u in lb["dU"]] +
                   [w for lb in node.lbuf for w in lb["dW"]])
        info = [(lb["kmap_s_fwd"], lb["kmap_s_bwd"]) for lb in node.lbuf] if mode == "force" else None
    for i, (a, b) in enumerate(zip(*res)):
        # fp32 sums in another order: differences relative to the tensor's scale
        err = (b - a).abs().max().item()
        assert err <= 2e-5 * a.abs().max().item() + 1e-7, "tensor %d: %.3g" % (i, err)
    return info, node


# widths 24,40: ragged 16-blocks, 8-unit (GRU phase 0) against 16-unit tiles; 22,25: H % 4 == 2 and
# odd H (the 2- and 1-wide loads); rows: 6 (16-row tiles), 20 (one 32-row tile), 34 (two row tiles)
WIDTH_CASES = [(c, lay, B, bidir) for c in ("GRU", "minimalGRU", "RNN")
               for lay, B, bidir in (("24,40", 3, True), ("24,40", 10, True), ("24,40", 34, False),
                                     ("22,25", 3, True))]


@pytest.mark.parametrize("cls,lay,B,bidir", WIDTH_CASES,
                         ids=["%s-%s-B%d" % (c, l, b) for c, l, b, _ in WIDTH_CASES])
def test_block_sparse_matches_dense_widths_and_rows(cls, lay, B, bidir):
    info, _ = sparse_vs_dense(cls, rec_opts(cls, lay, bidir, hcgsh_sparse="50,50"), 5, B, 20)
    assert info == [(16, 16), (16, 16)]


@pytest.mark.parametrize("cls,H,S,T,B", [("GRU", 320, 32, 5, 3), ("RNN", 320, 32, 5, 3),
                                         ("GRU", 640, 64, 3, 2)])
def test_block_sparse_matches_dense_slot_counts(cls, H, S, T, B):
    """[16] / [10]: 18 of 20 (36 of 40) 16-blocks kept per 16-row band — more than 16 (32) blocks
    per tile, so the tables take S = 32 (64) slots."""
    opts = rec_opts(cls, str(H), True, hcgsx_block="16", hcgsx_sparse="10", hcgsh_block="16",
                    hcgsh_sparse="10")
    info, node = sparse_vs_dense(cls, opts, T, B, 20)
    assert info == [(S, S)]
    kept = (node.lbuf[0]["kmap_fwd"] >= 0).sum(1)
    assert int(kept.max()) > S // 2


@pytest.mark.parametrize("cls", ["GRU", "minimalGRU", "RNN"])
def test_block_sparse_empty_kmap_rows(cls):
    """A 16-unit band of U with no nonzero (forward tiles without a block) and a 16-column band with
    none (BPTT tiles without a block): zero products, the dense result."""
    def edit(net):
        for m in net.hcgsh:
            m.mask.data[16:32, :] = 0
            m.mask.data[:, 32:48] = 0

    info, node = sparse_vs_dense(cls, rec_opts(cls, "48,48", True, hcgsh_sparse="50,50"), 5, 3, 20,
                                 edit)
    for lb in node.lbuf:
        assert bool((lb["kmap_fwd"] < 0).all(1).any()), "no empty forward row"
        assert bool((lb["kmap_bwd"] < 0).all(1).any()), "no empty BPTT row"


@pytest.mark.parametrize("mode", ["off", "force"])
@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=[c[0] for c in R.GOLDEN_CASES])
def test_kernels_match_reference_golden(case, mode):
    """tests/golden/gru_hcgs.npz at the bounds tests/test_gpu_rnn.py holds gru.npz to."""
    import pkc.engine as E
    import pkc.neural_networks as NN
    tag, cls, lay, bidir, seed = case
    g = np.load(os.path.join(GOLDEN, "gru_hcgs.npz"), allow_pickle=False)
    torch.manual_seed(seed)
    np.random.seed(seed)
    net = getattr(NN, cls)(section(R.golden_opts(cls, lay, bidir)), R.GOLDEN_F)
    net.load_state_dict({k: torch.from_numpy(g[tag + "/init/" + k]) for k in net.state_dict()})
    net.to(DEV).train()
    x = torch.from_numpy(g[tag + "/x"]).to(DEV)
    r = torch.from_numpy(g[tag + "/r"]).to(DEV)
    old = E.RNN_SPARSE
    E.RNN_SPARSE = mode
    try:
        eng, node, y = run_block(net, x, r)
    finally:
        E.RNN_SPARSE = old
    assert all((lb["kmap_fwd"] is not None) == (mode == "force") for lb in node.lbuf)
    np.testing.assert_allclose(y.cpu().numpy(), g[tag + "/y"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(dx0(eng, node).cpu().numpy().reshape(g[tag + "/dx"].shape),
                               g[tag + "/dx"], rtol=1e-3, atol=1e-5)
    n = 0
    for li, lb in enumerate(node.lbuf):
        for gi, gate in enumerate(net.GATES):
            grads = {"w%s.%d.weight" % (gate, li): lb["dW"][gi],
                     "u%s.%d.weight" % (gate, li): lb["dU"][gi],
                     "bn_w%s.%d.weight" % (gate, li): lb["dgamma"][gi],
                     "bn_w%s.%d.bias" % (gate, li): lb["dbeta"][gi]}
            for k, v in grads.items():
                np.testing.assert_allclose(v.cpu().numpy(), g[tag + "/grad/" + k], rtol=1e-3,
                                           atol=1e-5, err_msg=k)
                n += 1
    assert n == len([k for k in g.files if k.startswith(tag + "/grad/")])


# ------------------------------------------------------------------------------- engine level
OPT = dict(arch_opt="rmsprop", arch_lr="0.0016", opt_momentum="0.0", opt_alpha="0.95",
           opt_eps="1e-8", opt_centered="False", opt_weight_decay="0.0", arch_freeze="False")
SGD = dict(OPT, arch_opt="sgd", opt_dampening="0.0", opt_nesterov="False")
BODIES = {"gru": ("GRU", GRU_DEF, {}, OPT),
          # input LayerNorm + BatchNorm: SGD, as tests/test_gpu_seq.py's *_inpnorm bodies
          "mingru": ("minimalGRU", MINGRU_DEF, dict(minimalgru_use_laynorm_inp="True",
                                                    minimalgru_use_batchnorm_inp="True"), SGD),
          "rnn": ("RNN", RNN_DEF, dict(rnn_act="tanh,relu"), OPT)}
MODEL = ("o1=compute(rnn,fea)\no2=compute(head,o1)\no3=compute(mono,o1)\n"
         "lm=cost_nll(o3,lab_mono)\nlmw=mult_constant(lm,1.0)\nlc=cost_nll(o2,lab_cd)\n"
         "loss_final=sum(lc,lmw)\nerr_final=cost_err(o2,lab_cd)")
F, B = 20, 4


def make_cfg(body, sgd=False, drop="0.2,0.2"):
    cls, base, extra, opt = BODIES[body]
    p = PREFIX[cls]
    cfg = configparser.ConfigParser()
    cfg["a1"] = R.hook_opts(cls, dict(base, arch_name="rnn", **{p + "_lay": "32,24",
                                                               p + "_drop": drop}, **extra, **opt))
    head = dict(dnn_use_laynorm_inp="False", dnn_use_batchnorm_inp="False", to_do="train",
                arch_name="head", dnn_lay="64", dnn_drop="0.0", dnn_use_batchnorm="False",
                dnn_use_laynorm="False", dnn_act="softmax", **OPT)
    cfg["a2"] = head
    cfg["a3"] = dict(head, arch_name="mono", dnn_lay="8", arch_lr="0.0004")
    if sgd:
        for sec in ("a1", "a2", "a3"):
            cfg[sec].update(arch_opt="sgd", arch_lr="0.08", opt_momentum="0.0",
                            opt_dampening="0.0", opt_nesterov="False")
    return cfg


def build_nets(cfg, body, oracle=True):
    import pkc.neural_networks as NN
    from oracle import nets as ON
    nets, onets, opts = {}, {}, {}
    for sec in ("a1", "a2", "a3"):
        o = cfg[sec]
        inp = F if sec == "a1" else nets["rnn"].out_dim
        torch.manual_seed(3)
        np.random.seed(3)
        cls = BODIES[body][0] if sec == "a1" else "MLP"
        name = o["arch_name"]
        nets[name] = getattr(NN, cls)(o, inp)
        if oracle:
            onets[name] = getattr(R if sec == "a1" else ON, cls)(o, inp)
            onets[name].load_state_dict(nets[name].state_dict())
        opts[name] = o
    return nets, onets, opts


def make_data():
    rs = np.random.RandomState(0)
    lens = np.sort(rs.randint(5, 13, size=12))
    end = np.cumsum(lens)
    X = rs.randn(end[-1], F).astype(np.float32)
    lab = np.stack([rs.randint(0, 64, end[-1]), rs.randint(0, 8, end[-1])], 1).astype(np.int32)
    return rs, lens, end, X, lab


def oracle_batch(lens, end, X, lab, snt, T, rng_o, lefts):
    """The padded batch exactly as core.py:183-200 assembles it"""
    inp = torch.zeros(T, B, F + 2)
    for k in range(B):
        n = int(lens[snt + k])
        left = rng_o.randint(0, T - n)
        b0 = int(end[snt + k] - n)
        inp[left:left + n, k, :F] = torch.from_numpy(X[b0:b0 + n])
        inp[left:left + n, k, F:] = torch.from_numpy(lab[b0:b0 + n].astype(np.float32))
        assert left == lefts[k]
    return inp


def masked_ref(name, sd_o):
    """The restatement's W / U times its mask: it re-masks at the next forward, pkc stores W * mask"""
    ref = sd_o[name].double()
    parts = name.split(".")
    if name.endswith("weight") and len(parts[0]) == 2 and parts[0][0] in "wu":
        ref = ref * sd_o[("hcgsx" if parts[0][0] == "w" else "hcgsh") + ".%s.mask" % parts[1]].double()
    return ref


def check_update(step, bf16, nets, onets, opts, report):
    """The step's parameters from the common start: tests/test_gpu_seq.py's rule, unchanged"""
    from flipcheck import assert_counted, step_outliers
    for k in nets:
        sd_o = onets[k].state_dict()
        for name, v in nets[k].state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            ref = masked_ref(name, sd_o) if k == "rnn" else sd_o[name].double()
            scale = float(ref.abs().max())
            if name.endswith("running_mean") and opts[k].get("minimalgru_use_batchnorm_inp") == "True":
                scale = float(sd_o[name.replace("running_mean", "running_var")].double().sqrt().max())
            lr = float(opts[k]["arch_lr"])
            scale = max(scale, lr)
            n, dmax, rest = step_outliers(v.cpu(), ref, 1e-4, scale)
            report["%d %s/%s" % (step, k, name)] = (n, round(dmax / scale, 6))
            sgd = opts[k]["arch_opt"] == "sgd"
            frac = (0.005 if bf16 else 0.0) if sgd else 0.02
            bound = (1e-3 if bf16 else 1e-4) * scale if sgd else 2 * 4.48 * lr
            assert_counted("step %d %s %s" % (step, k, name), n, ref.numel(), frac, dmax,
                           bound + 1e-7, str({a: b for a, b in report.items() if b[0]}))


def assert_masked_zero(net):
    sd = net.state_dict()
    for name, v in sd.items():
        parts = name.split(".")
        if name.endswith("weight") and len(parts[0]) == 2 and parts[0][0] in "wu":
            m = sd[("hcgsx" if parts[0][0] == "w" else "hcgsh") + ".%s.mask" % parts[1]]
            assert bool((v[m == 0] == 0).all()), "%s: a masked entry is not exactly 0" % name


def train_vs_restatement(body, sparse, bf16=False):
    from flipcheck import assert_counted, resync
    from oracle import nets as ON
    from oracle import run as OR
    from pkc import _lib as L
    import pkc.engine as E
    cfg = make_cfg(body, sgd=bf16)
    nets, onets, opts = build_nets(cfg, body)
    if bf16:
        ON.use_bf16_rec_matmuls(onets["rnn"], steps=body == "rnn")
        ON.use_bf16_matmuls(onets["head"])
        ON.use_bf16_matmuls(onets["mono"])
    for k in nets:
        nets[k].to(DEV).train()
        onets[k].train()
    rs, lens, end, X, lab = make_data()
    specs = nets["rnn"].layer_specs()
    bid = 2 if specs[0]["bidir"] else 1
    masks = {("rnn", li): torch.from_numpy((rs.rand(bid * B, sp["H"]) > 0.2).astype(np.float32))
             for li, sp in enumerate(specs)}
    old = E.RNN_SPARSE
    E.RNN_SPARSE = sparse
    try:
        eng = E.Engine(nets, opts, E.parse_model(MODEL), {"fea": (0, F)}, ["lab_cd", "lab_mono"],
                       batch=B, max_len=16, seed=1, prec=L.PREC_BF16 if bf16 else L.PREC_FP32,
                       rnn_drop_in={k: v.to(DEV) for k, v in masks.items()})
    finally:
        E.RNN_SPARSE = old
    lbufs = next(n for n in eng.nodes if n.rec).lbuf
    forms = eng.rec_forms()
    if bf16 and body == "rnn":          # masked RNN in bf16 mode: dense bf16 steps on the masked U
        assert all(lb["kmap_fwd"] is None for lb in lbufs)
        assert forms == {"rnn.0": "bf16 steps", "rnn.1": "bf16 steps"}, forms
    elif sparse == "force":
        assert all(lb["kmap_fwd"] is not None and lb["kmap_bwd"] is not None for lb in lbufs)
        assert forms == {"rnn.0": "fp32 steps, block-sparse U", "rnn.1": "fp32 steps, block-sparse U"}
    else:
        assert all(lb["kmap_fwd"] is None for lb in lbufs)
        assert forms == {"rnn.0": "fp32 steps", "rnn.1": "fp32 steps"}, forms
    assert_masked_zero(nets["rnn"])                  # masks applied at build
    eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), end[-1], end_index=end)
    oopt = {k: ON.make_optimizer(onets[k].parameters(), opts[k]) for k in onets}
    lines = OR.parse_model(MODEL)
    rng_e, rng_o = random.Random(7), random.Random(7)
    report = {}
    for step in range(3):
        eng.sync_state()
        resync(nets, onets, {k: eng.optimizer_state_dict(k) for k in nets} if step else None, oopt)
        batch = eng.next_seq_batch(rng_e)
        T = batch[3]
        inp = oracle_batch(lens, end, X, lab, step * B, T, rng_o, batch[2])
        body_net = onets["rnn"]
        f = body_net.forward
        body_net.forward = lambda x, _f=f: _f(x, drop_masks=[masks[("rnn", i)]
                                                             for i in range(len(specs))])
        outs = OR.train_step(lines, onets, oopt, {"rnn": True, "head": False, "mono": False},
                             {"fea": (0, F)}, {"lab_cd": F, "lab_mono": F + 1}, inp, T, B)
        body_net.forward = f
        eng.train_step(batch=batch)
        loss, err = eng.loss_values()
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-3 if bf16 else 1e-4)
        if not bf16:
            np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
        post, ref = eng.head_output("o2").cpu(), outs["o2"].detach()
        relm = (post - ref).abs() / ref.abs().clamp_min(1e-3)
        rel, nout = relm.max().item(), int((relm > 1e-4).sum().item())
        print("%s %s%s step %d posterior rel err %.3g, %d of %d above 1e-4" % (
            body, sparse, " bf16" if bf16 else "", step, rel, nout, relm.numel()))
        if bf16:
            assert_counted("step %d posteriors" % step, nout, relm.numel(), 0.01, rel, 1e-3)
        else:
            assert rel < 1e-4, "step %d posterior rel err %.3g" % (step, rel)
        eng.sync_state()
        assert_masked_zero(nets["rnn"])
        check_update(step, bf16, nets, onets, opts, report)


@pytest.mark.parametrize("sparse", ["off", "force"])
@pytest.mark.parametrize("body", ["gru", "mingru", "rnn"])
def test_engine_trains_like_restatement(body, sparse):
    """3 training steps (32,24 wide, bidirectional, injected dropout masks, two heads) against the
    restatement, each from the engine's state (flipcheck.resync), at tests/test_gpu_seq.py's fp32
    bounds; masked entries of W and U exactly 0 after every step."""
    train_vs_restatement(body, sparse)


def test_engine_bf16_mode_rnn():
    """pkc_prec = bf16 with masks: the RNN keeps its dense bf16 steps on the masked U (no kmap);
    tests/test_gpu_seq.py's bf16 bounds against the restatement with that rounding."""
    train_vs_restatement("rnn", "auto", bf16=True)


def test_engine_graph_replay_equals_eager():
    """Captured sequence graphs of a masked GRU (block-sparse steps) replay the eager steps bit for
    bit (as tests/test_gpu_seq_graph.py)."""
    import pkc.engine as E
    cfg = make_cfg("gru")
    nets0, _, opts = build_nets(cfg, "gru", oracle=False)
    for n in nets0.values():
        n.to(DEV).train()
    rs = np.random.RandomState(0)
    lens = np.array([5, 7, 12, 9, 6, 9, 8, 9, 12, 12, 10, 5, 7, 9, 9, 6])
    end = np.cumsum(lens)
    X = torch.from_numpy(rs.randn(end[-1], F).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(np.stack([rs.randint(0, 64, end[-1]), rs.randint(0, 8, end[-1])],
                                    1).astype(np.int32)).to(DEV)
    runs = []
    old = E.RNN_SPARSE
    E.RNN_SPARSE = "force"
    try:
        for graphs in (False, True):
            nets = copy.deepcopy(nets0)
            eng = E.Engine(nets, opts, E.parse_model(MODEL), {"fea": (0, F)},
                           ["lab_cd", "lab_mono"], batch=B, max_len=16, seed=1)
            assert all(lb["kmap_fwd"] is not None for lb in eng.nodes[0].lbuf)
            if graphs:
                assert eng.capture()
            eng.bind_chunk(X, lab, end[-1], end_index=end)
            rng = random.Random(7)
            trace = []
            for _ in range(4):
                eng.train_step(batch=eng.next_seq_batch(rng))
                trace.append((eng.loss_values(), eng.head_output("o2").cpu().clone()))
            if graphs:
                assert eng.seq_captures == 2 and sorted(eng.seq_graphs) == [9, 12]
            eng.sync_state()
            runs.append((trace, {k: {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
                                 for k, m in nets.items()}))
    finally:
        E.RNN_SPARSE = old
    (te, se), (tg, sg) = runs
    for step, ((le, pe), (lg, pg)) in enumerate(zip(te, tg)):
        assert le == lg, (step, le, lg)
        assert torch.equal(pe, pg), step
    for k in se:
        for n in se[k]:
            assert torch.equal(se[k][n], sg[k][n]), (k, n)


@pytest.mark.parametrize("body", ["gru", "rnn"])
def test_engine_eval_and_forward_mode(body):
    """Validation (B = 4, padded) and forward mode (one utterance per batch): eval-mode posteriors
    and loss against the restatement, < 1e-4 relative (as tests/test_gpu_cudnn.py)."""
    import pkc.engine as E
    from oracle import run as OR
    cfg = make_cfg(body)
    for batch in (4, 1):
        nets, onets, opts = build_nets(cfg, body)
        for k in nets:
            nets[k].to(DEV).eval()
            onets[k].eval()
        rs, lens, end, X, lab = make_data()
        old = E.RNN_SPARSE
        E.RNN_SPARSE = "force"
        try:
            eng = E.Engine(nets, opts, E.parse_model(MODEL), {"fea": (0, F)},
                           ["lab_cd", "lab_mono"], batch=batch, max_len=16, seed=1, train=False)
        finally:
            E.RNN_SPARSE = old
        assert all(lb["kmap_fwd"] is not None for lb in eng.nodes[0].lbuf)
        eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), end[-1],
                       end_index=end)
        if batch == 4:
            b = eng.next_seq_batch(random.Random(7))
            T, nb = b[3], B
            inp = oracle_batch(lens, end, X, lab, 0, T, random.Random(7), b[2])
            eng.eval_step(batch=b)
        else:
            T, nb = int(lens[0]), 1
            inp = torch.zeros(T, 1, F + 2)
            inp[:, 0, :F] = torch.from_numpy(X[:T])
            inp[:, 0, F:] = torch.from_numpy(lab[:T].astype(np.float32))
            eng.eval_step()
        with torch.no_grad():
            outs = OR.forward_model(OR.parse_model(MODEL), onets,
                                    {"rnn": True, "head": False, "mono": False}, {"fea": (0, F)},
                                    {"lab_cd": F, "lab_mono": F + 1}, inp, T, nb)
        post, ref = eng.head_output("o2").cpu(), outs["o2"].detach().float()
        rel = ((post - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
        assert rel < 1e-4, "batch %d posterior rel err %.3g" % (batch, rel)
        np.testing.assert_allclose(eng.loss_values()[0], outs["loss_final"].item(), rtol=1e-4)


def test_plugin_forward_trains_like_restatement():
    """net(x) of the masked GRU under autograd (pkc.plugin), trained by the reference's loop with
    torch.optim against the restatement: tests/test_gpu_plugin.py's run and bounds."""
    from oracle import run as OR
    from test_gpu_plugin import _run
    cfg = make_cfg("gru", drop="0.0,0.0")
    cfg["model"] = {"model": MODEL}
    nets, onets, opts = build_nets(cfg, "gru")
    for k in nets:
        nets[k].to(DEV).train()
        onets[k].train()
    rs = np.random.RandomState(1)
    batches = []
    for T in (9, 13, 6):
        x = rs.randn(T, B, F).astype(np.float32)
        lab = np.stack([rs.randint(0, 64, (T, B)), rs.randint(0, 8, (T, B))], 2).astype(np.float32)
        batches.append((torch.from_numpy(np.concatenate([x, lab], 2)), T))
    assert OR.parse_model(MODEL)[0][1] == "compute"
    _run(cfg, nets, onets, opts, {"rnn": True, "head": False, "mono": False}, {"fea": (0, F)},
         {"lab_cd": F, "lab_mono": F + 1}, batches, B=B, out="o2")


# ------------------------------------------------------------------------------- run_nn lifecycle
def test_run_nn_lifecycle(tmp_path):
    """pkc.core.run_nn on a masked GRU cfg: train -> train (resumed) -> valid -> forward.  The
    .pkl files carry the masks (the second chunk's are the first chunk's), and the valid loss /
    err and the posterior ark match the restatement loaded from the second chunk's .pkl."""
    from oracle import loader as OL
    from oracle import nets as ON
    from pkc.core import run_nn
    from test_gpu_run_nn import chunk_cfg, write_data
    d = str(tmp_path)
    scp, ali = write_data(d, 0, n_utt=8)
    counts = os.path.join(d, "counts")
    with open(counts, "w") as f:
        f.write("[ " + " ".join(str(i + 3) for i in range(64)) + " ]\n")
    a1 = R.hook_opts("GRU", dict(GRU_DEF, arch_library="pkc.neural_networks", arch_class="GRU",
                                 arch_seq_model="True", arch_name="MLP_layers1", gru_lay="24,24",
                                 gru_drop="0.2,0.2", **OPT))

    def make(name, to_do, pretrain=None, batch="4", **kw):
        path = chunk_cfg(d, name, to_do, scp, ali, **kw)
        cfg = configparser.ConfigParser()
        cfg.read(path)
        cfg["architecture1"] = dict(a1, arch_pretrain_file="none")
        cfg["batches"]["batch_size_train"] = cfg["batches"]["batch_size_valid"] = batch
        if pretrain:
            for i in (1, 2, 3):
                cfg["architecture%d" % i]["arch_pretrain_file"] = os.path.join(
                    d, "%s_architecture%d.pkl" % (pretrain, i))
        with open(path, "w") as f:
            cfg.write(f)
        return path

    def ckpt(name):
        return torch.load(os.path.join(d, name + "_architecture1.pkl"), map_location="cpu",
                          weights_only=True)

    c0 = make("train_ck0", "train")
    c1 = make("train_ck1", "train", pretrain="train_ck0")
    run_nn(None, None, None, None, None, None, c0, True, c1)
    info = configparser.ConfigParser()
    info.read(os.path.join(d, "train_ck0.info"))
    assert 0 < float(info["results"]["loss"]) < 20
    ck = ckpt("train_ck0")
    torch.manual_seed(0)
    np.random.seed(0)
    ref = R.GRU(a1, 440)
    assert list(ck["model_par"].keys()) == list(ref.state_dict().keys())
    assert list(ck["model_par"])[:4] == ["hcgsx.0.mask", "hcgsx.1.mask", "hcgsh.0.mask", "hcgsh.1.mask"]
    c_va = make("valid", "valid", pretrain="train_ck1", batch="1")
    run_nn(None, None, None, None, None, None, c1, True, c_va)          # resumes from the .pkl
    ck1 = ckpt("train_ck1")
    # 2 batches per chunk: the second chunk continued the first one's optimizer state
    st0, st1 = ck["optimizer_par"]["state"], ck1["optimizer_par"]["state"]
    assert int(float(st0[min(st0)]["step"])) == 2 and int(float(st1[min(st1)]["step"])) == 4
    sd0, sd1 = ck["model_par"], ck1["model_par"]
    for k in sd0:
        if "mask" in k:              # the second chunk kept the first chunk's masks
            assert torch.equal(sd0[k], sd1[k]), k
            assert 0 < sd1[k].mean().item() < 1
        parts = k.split(".")
        if k.endswith("weight") and len(parts[0]) == 2 and parts[0][0] in "wu":
            m = sd1[("hcgsx" if parts[0][0] == "w" else "hcgsh") + ".%s.mask" % parts[1]]
            assert bool((sd1[k][m == 0] == 0).all()), k
            assert not torch.equal(sd0[k], sd1[k]), k
    c_fw = make("forward", "forward", pretrain="train_ck1", counts=counts)
    run_nn(None, None, None, None, None, None, c_va, True, c_fw)
    info.read(os.path.join(d, "valid.info"))
    va_loss, va_err = float(info["results"]["loss"]), float(info["results"]["err"])
    nxt, _, _ = run_nn(None, None, None, None, None, None, c_fw, True, c_fw)
    with open(os.path.join(d, "forward_out_dnn2_to_decode.ark"), "rb") as f:
        mats = OL.parse_mat_ark(f.read())
    assert len(mats) == 8
    ref.load_state_dict(sd1, strict=True)
    ref.eval()
    fcfg = configparser.ConfigParser()
    fcfg.read(c_fw)
    heads = []
    for i in (2, 3):
        h = ON.MLP(fcfg["architecture%d" % i], ref.out_dim)
        h.load_state_dict(torch.load(os.path.join(d, "train_ck1_architecture%d.pkl" % i),
                                     map_location="cpu", weights_only=True)["model_par"])
        heads.append(h.eval())
    chunk = nxt[1]                      # the forward chunk again: the same utterances as valid
    feats, labs = chunk.feats.cpu(), chunk.labels.cpu().long()
    ends, names = list(chunk.end_index), list(chunk.names)
    icd, imono = chunk.lab_names.index("lab_cd"), chunk.lab_names.index("lab_mono")
    c = np.arange(3, 67, dtype=np.float64)
    prior = torch.from_numpy(np.log(c / c.sum()).astype(np.float32))
    got = dict(mats)
    beg, losses, errs = 0, [], []
    for name, e in zip(names, ends):
        with torch.no_grad():
            hid = ref(feats[beg:e, :440].unsqueeze(1)).squeeze(1)
            logp, logm = heads[0](hid), heads[1](hid)
        m = torch.from_numpy(np.array(got[name]))
        assert m.shape == logp.shape
        dabs = (m - (logp - prior)).abs().max().item()
        rel = ((m + prior - logp).abs() / logp.abs().clamp_min(1e-3)).max().item()
        assert dabs <= 1e-4 and rel <= 1e-4, (name, dabs, rel)
        nll = torch.nn.functional.nll_loss
        losses.append((nll(logp, labs[beg:e, icd]) + nll(logm, labs[beg:e, imono])).item())
        errs.append((logp.argmax(1) != labs[beg:e, icd]).float().mean().item())
        beg = e
    # valid ran one utterance per batch: the chunk's loss / err are the means over the utterances
    np.testing.assert_allclose(va_loss, np.mean(losses), rtol=1e-4)
    np.testing.assert_allclose(va_err, np.mean(errs), atol=1e-6)

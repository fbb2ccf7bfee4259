"""The *_cudnn architectures (LSTM_cudnn, GRU_cudnn, RNN_cudnn: torch.nn.LSTM / GRU / RNN) on the HIP
path: the standard-cell time loops at kernel level against the golden recorded from the reference
(tests/golden/cudnn.npz), then the architecture classes through the engine, the plug-in and run_nn
against the plain-torch restatement (tests/cudnn_ref.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"

G = np.load(os.path.join(GOLDEN, "cudnn.npz"))
CASES = json.loads(str(G["cases"]))
INP = int(G["inp_dim"])


def _case(name):
    c = CASES[name]
    o = c["opts"]
    cell = c["cls"].split("_")[0].lower()
    keys = json.loads(str(G[name + "/keys"]))
    sd = {k: torch.from_numpy(G["%s/sd/%s" % (name, k)]).to(DEV) for k in keys}
    kw = dict(cell=cell, sd=sd, prefix=cell + ".0.", layers=int(o["num_layers"]),
              bidir=o["bidirectional"] == "True", bias=o["bias"] == "True",
              act=o.get("nonlinearity", "tanh"))
    x = torch.from_numpy(G[name + "/x"]).to(DEV)
    r = torch.from_numpy(G[name + "/r"]).to(DEV)
    return kw, x, r, keys


@pytest.mark.parametrize("name", sorted(CASES))
def test_std_kernels_vs_golden(name):
    """pkc_rnn_std_fwd / _bwd on the golden cases: y to rtol 1e-4 / atol 1e-5, dL/dx and every
    parameter gradient (b_hn, inside bias_hh, included) to rtol 1e-3 / atol 1e-5 — the bounds of
    tests/test_gpu_rnn.py; a rerun is bit-identical."""
    from cudnn_kernel import run_stack
    kw, x, r, keys = _case(name)
    y, dx, grads, _ = run_stack(x=x, r=r, **kw)
    np.testing.assert_allclose(y.cpu().numpy(), G[name + "/y"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(dx.cpu().numpy(), G[name + "/dx"], rtol=1e-3, atol=1e-5)
    assert sorted(grads) == sorted(keys)
    for k in keys:
        np.testing.assert_allclose(grads[k].cpu().numpy(), G["%s/grad/%s" % (name, k)], rtol=1e-3,
                                   atol=1e-5, err_msg=k)
    y2, dx2, grads2, _ = run_stack(x=x, r=r, **kw)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    assert all(torch.equal(grads[k], grads2[k]) for k in keys)
    # eval mode: the same forward (dropout is the only difference, and it is 0 here)
    ye, _, _, _ = run_stack(x=x, r=r, train=False, backward=False, **kw)
    np.testing.assert_allclose(ye.cpu().numpy(), G[name + "/y_eval"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("cls,H", [("LSTM_cudnn", 19), ("GRU_cudnn", 22), ("RNN_cudnn", 19),
                                   ("LSTM_cudnn", 256), ("GRU_cudnn", 550), ("RNN_cudnn", 512)])
def test_std_kernels_other_paths(cls, H):
    """The paths the golden's H = 20 / 48 (16-byte loads, 4-wave tiles) do not take, against the
    restatement on the CPU at the kernel-level bounds: element loads (H = 19), 8-byte loads (H = 22,
    550), the 8-wave forward tiles (H >= 512) and the 8-wave BPTT tiles (G * H >= 1024: LSTM 256).
    One bidirectional layer, B = 5, T = 3."""
    import cudnn_ref as R
    from cudnn_kernel import run_stack
    o = dict(hidden_size=str(H), num_layers="1", bias="True", batch_first="False", dropout="0.0",
             bidirectional="True", nonlinearity="relu")
    torch.manual_seed(H)
    net = getattr(R, cls)(o, 7).train()
    x = torch.randn(3, 5, 7, requires_grad=True)
    r = torch.randn(3, 5, 2 * H)
    y = net(x)
    (y * r).sum().backward()
    cell = net.cell
    sd = {k: v.detach().to(DEV) for k, v in net.state_dict().items()}
    gy, gdx, grads, _ = run_stack(cell=cell, sd=sd, prefix=cell + ".0.", x=x.detach().to(DEV),
                                  r=r.to(DEV), layers=1, bidir=True, bias=True, act="relu")
    np.testing.assert_allclose(gy.cpu().numpy(), y.detach().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(gdx.cpu().numpy(), x.grad.numpy(), rtol=1e-3, atol=1e-5)
    for k, p in net.named_parameters():
        np.testing.assert_allclose(grads[k].cpu().numpy(), p.grad.numpy(), rtol=1e-3, atol=1e-5,
                                   err_msg=k)


@pytest.mark.parametrize("name", ["lstm_c", "gru_c", "rnn_c"])
def test_std_bidirectional_equals_two_unidirectional(name):
    """Layer 0 of the bidirectional B = 17 cases: the two directions of one call against two
    one-direction calls, the second on the time-flipped operands — bit for bit, forward (y, saved
    states) and backward (gate gradients)."""
    from cudnn_kernel import CELL, Layer
    kw, x, r, _ = _case(name)
    cell, sd, pre = kw["cell"], kw["sd"], kw["prefix"]
    T, B, _ = x.shape
    H, Gn = sd[pre + "weight_hh_l0"].shape[1], CELL[cell][1]
    x2 = x.reshape(T * B, -1)
    wpre, U, bhh = [], [], []
    for sfx in ("", "_reverse"):
        w = x2 @ sd[pre + "weight_ih_l0" + sfx].t() + sd[pre + "bias_ih_l0" + sfx]
        wpre.append(w.view(T, B, Gn * H).contiguous())
        U.append(sd[pre + "weight_hh_l0" + sfx].contiguous())
        bhh.append(sd[pre + "bias_hh_l0" + sfx])
    dy = r[:, :, :2 * H].contiguous()
    both = Layer(cell, T, B, H, 2, kw["act"])
    y = both.forward(wpre, U, bhh).clone()
    dg = both.backward(dy).clone()
    fw = Layer(cell, T, B, H, 1, kw["act"])
    y0 = fw.forward(wpre[:1], U[:1], bhh[:1]).clone()
    dg0 = fw.backward(dy[:, :, :H].contiguous()).clone()
    bw = Layer(cell, T, B, H, 1, kw["act"])
    y1 = bw.forward([wpre[1].flip(0).contiguous()], U[1:], bhh[1:]).clone()
    dg1 = bw.backward(dy[:, :, H:].flip(0).contiguous()).clone()
    torch.cuda.synchronize()
    assert torch.equal(y[:, :, :H], y0) and torch.equal(y[:, :, H:], y1.flip(0))
    assert torch.equal(dg[0], dg0[0]) and torch.equal(dg[1], dg1[0].flip(0))
    assert y1.abs().sum() > 0 and dg1.abs().sum() > 0


def test_std_kernel_dropout_and_entry_checks():
    """Inter-layer dropout at kernel level: an injected keep mask gives y = h keep / (1 - p) and
    gates the backward; a generated mask is {0, 1} with a keep rate near 1 - p, is written for the
    backward, and a rerun at the same step counter repeats it.  Bad arguments give a negative
    status and a message."""
    from cudnn_kernel import Layer
    from pkc import _lib as L
    kw, x, r, _ = _case("gru_c")
    sd, pre = kw["sd"], kw["prefix"]
    T, B, _ = x.shape
    H = sd[pre + "weight_hh_l0"].shape[1]
    x2 = x.reshape(T * B, -1)
    ops = ([(x2 @ sd[pre + "weight_ih_l0" + s].t() + sd[pre + "bias_ih_l0" + s]).view(T, B, 3 * H)
            .contiguous() for s in ("", "_reverse")],
           [sd[pre + "weight_hh_l0" + s].contiguous() for s in ("", "_reverse")],
           [sd[pre + "bias_hh_l0" + s] for s in ("", "_reverse")])
    plain = Layer("gru", T, B, H, 2)
    h = plain.forward(*ops).clone()
    dy = r[:, :, :2 * H].contiguous()
    rs = np.random.RandomState(2)
    keep = torch.from_numpy((rs.rand(T, B, 2 * H) > 0.3).astype(np.uint8)).to(DEV)
    inj = Layer("gru", T, B, H, 2, drop_p=0.3, keep_in=keep)
    y = inj.forward(*ops)
    want = torch.where(keep.bool(), h * (1.0 / (1.0 - 0.3)), torch.zeros_like(h))
    torch.testing.assert_close(y, want, rtol=1e-6, atol=0)
    assert torch.equal(inj.keep, keep) and torch.equal(inj.hs, plain.hs)
    dgi = inj.backward(dy).clone()
    dgp = plain.backward(torch.where(keep.bool(), dy * (1.0 / (1.0 - 0.3)), torch.zeros_like(dy)))
    torch.testing.assert_close(dgi, dgp, rtol=1e-6, atol=1e-9)
    gen = Layer("gru", T, B, H, 2, drop_p=0.3)
    gen.a.seed, gen.a.stream_id = 7, 11
    yg = gen.forward(*ops).clone()
    k1 = gen.keep.clone()
    assert set(k1.unique().tolist()) <= {0, 1}
    assert abs(k1.float().mean().item() - 0.7) < 0.05
    torch.testing.assert_close(yg, torch.where(k1.bool(), h / 0.7, torch.zeros_like(h)), rtol=1e-6,
                               atol=0)
    gen.forward(*ops)
    assert torch.equal(gen.keep, k1)
    ev = Layer("gru", T, B, H, 2, train=False, drop_p=0.3)       # eval: no dropout
    assert torch.equal(ev.forward(*ops), h)
    # entry checks
    lib = L.lib()
    bad = Layer("gru", T, B, H, 2)
    bad.forward(*ops)
    for field, value, word in (("H", 4096, "2048"), ("cell", 9, "cell"), ("ndir", 3, "ndir"),
                               ("drop_p", 1.0, "drop_p"), ("hs", None, "null")):
        old = getattr(bad.a, field)
        setattr(bad.a, field, value)
        assert lib.pkc_rnn_std_fwd(C.byref(bad.a), None) < 0
        assert word in lib.pkc_last_error().decode()
        setattr(bad.a, field, old)
    bad.a.dy = None
    assert lib.pkc_rnn_std_bwd(C.byref(bad.a), None) < 0


# ------------------------------------------------------------------------------- engine level
def _engine_setup(cls, optk, bf16=False, train=True, batch=None):
    import cudnn_cases as CC
    import pkc.neural_networks as NN
    from pkc import _lib as L
    from pkc.engine import Engine, parse_model
    cfg = CC.make_cfg(cls, optk)
    nets, opts = CC.build(cfg, (NN, NN))
    for n in nets.values():
        n.to(DEV)
        n.train() if train else n.eval()
    lens, end, X, lab, masks = CC.make_data()
    eng = Engine(nets, opts, parse_model(CC.MODEL), {"fea": (0, CC.F)}, ["lab_cd", "lab_mono"],
                 batch=batch or CC.B, max_len=CC.MAX_LEN, seed=1, train=train,
                 prec=L.PREC_BF16 if bf16 else L.PREC_FP32,
                 rnn_drop_in={k: v.to(DEV) for k, v in masks.items()})
    eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), end[-1], end_index=end)
    return CC, cfg, nets, opts, eng, (lens, end, X, lab, masks)


def _posterior_rel(eng, outs):
    post = eng.head_output("o2").cpu()
    ref = outs["o2"].detach().float()
    return (post - ref).abs() / ref.abs().clamp_min(1e-3)


@pytest.mark.parametrize("optk", ["sgd", "rmsprop"])
@pytest.mark.parametrize("cls", ["LSTM_cudnn", "GRU_cudnn", "RNN_cudnn"])
def test_engine_vs_restatement(cls, optk):
    """Three training steps through the engine (2 bidirectional layers of 32, dropout 0.2 with
    injected masks, the padded batches of next_seq_batch, two softmax heads) against the
    restatement, each step from the engine's state (flipcheck.resync): tests/test_gpu_seq.py's fp32
    rule — loss rtol 1e-4, posteriors < 1e-4 relative (denominator clamped at 1e-3), parameters
    within 1e-4 of the tensor's scale (no outlier under SGD; RMSprop: at most 2 % counted sign
    steps, each <= 2 * 4.48 lr)."""
    import random
    from flipcheck import resync
    CC, cfg, nets, opts, eng, (lens, end, X, lab, masks) = _engine_setup(cls, optk)
    assert eng.rec_forms() == {"rnn.0": "fp32 steps", "rnn.1": "fp32 steps"}
    onets, _, oopt = CC.oracle_nets(cfg)
    rng = random.Random(7)
    report = {}
    for step, (inp, T, lefts) in enumerate(CC.batches(lens, end, X, lab)):
        eng.sync_state()
        resync(nets, onets, {k: eng.optimizer_state_dict(k) for k in nets} if step else None, oopt)
        batch = eng.next_seq_batch(rng)
        assert batch[3] == T and list(batch[2]) == lefts
        outs = CC.oracle_step(onets, oopt, inp, T, masks)
        eng.train_step(batch=batch)
        loss, err = eng.loss_values()
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
        np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
        rel = _posterior_rel(eng, outs).max().item()
        print("%s %s step %d loss %.6f posterior rel err %.3g" % (cls, optk, step, loss, rel))
        assert rel < 1e-4, "step %d posterior rel err %.3g" % (step, rel)
        eng.sync_state()
        CC.check_update(step, optk, opts, {k: nets[k].state_dict() for k in nets},
                        {k: onets[k].state_dict() for k in onets}, report)
    print("%s %s parameter outliers: %s" % (cls, optk, {k: v for k, v in report.items() if v[0]}))


@pytest.mark.parametrize("cls", ["LSTM_cudnn", "GRU_cudnn", "RNN_cudnn"])
def test_engine_eval_and_forward_mode(cls):
    """Validation (B = 4) and forward mode (one utterance per batch) apply no dropout: posteriors
    against the restatement in eval, < 1e-4 relative."""
    import random
    for batch in (4, 1):
        CC, cfg, nets, opts, eng, (lens, end, X, lab, masks) = _engine_setup(
            cls, "sgd", train=False, batch=batch)
        onets, _, oopt = CC.oracle_nets(cfg)
        for k in onets:
            onets[k].load_state_dict({n: v.cpu() for n, v in nets[k].state_dict().items()})
            onets[k].eval()
        if batch == 4:
            inp, T, _ = CC.batches(lens, end, X, lab, steps=1)[0]
            eng.eval_step(batch=eng.next_seq_batch(random.Random(7)))
            B = 4
        else:
            T, B = int(lens[0]), 1
            inp = torch.zeros(T, 1, CC.F + 2)
            inp[:, 0, :CC.F] = torch.from_numpy(X[:T])
            inp[:, 0, CC.F:] = torch.from_numpy(lab[:T].astype(np.float32))
            eng.eval_step()
        from oracle import run as OR
        with torch.no_grad():
            outs = OR.forward_model(OR.parse_model(CC.MODEL), onets,
                                    {"rnn": True, "head": False, "mono": False}, {"fea": (0, CC.F)},
                                    {"lab_cd": CC.F, "lab_mono": CC.F + 1}, inp, T, B)
        rel = _posterior_rel(eng, outs).max().item()
        assert rel < 1e-4, "batch %d posterior rel err %.3g" % (batch, rel)
        loss, _ = eng.loss_values()
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)


@pytest.mark.parametrize("cls", ["LSTM_cudnn", "GRU_cudnn", "RNN_cudnn"])
def test_engine_bf16_mode(cls):
    """pkc_prec = bf16: the input projections, their dX / dW and the weight_hh gradient matmuls on
    bf16-rounded operands, the step products exact fp32 (rec_forms "fp32 steps") — against the
    restatement with exactly that rounding (SGD, as tests/test_gpu_seq.py's bf16 test): loss rtol
    1e-3, at most 1 % of the posteriors above 1e-4 relative, none above 1e-3."""
    import random
    from flipcheck import assert_counted, resync
    from oracle import nets as ON
    CC, cfg, nets, opts, eng, (lens, end, X, lab, masks) = _engine_setup(cls, "sgd", bf16=True)
    assert eng.rec_forms() == {"rnn.0": "fp32 steps", "rnn.1": "fp32 steps"}
    onets, _, oopt = CC.oracle_nets(cfg)
    onets["rnn"].proj = lambda x, w, b: ON._BF16Linear.apply(x, w, b)
    onets["rnn"].recur = lambda h, w: ON._BF16dWLinear.apply(h, w)
    ON.use_bf16_matmuls(onets["head"])
    ON.use_bf16_matmuls(onets["mono"])
    rng = random.Random(7)
    for step, (inp, T, _) in enumerate(CC.batches(lens, end, X, lab)):
        eng.sync_state()
        resync(nets, onets, None, oopt)
        batch = eng.next_seq_batch(rng)
        outs = CC.oracle_step(onets, oopt, inp, T, masks)
        eng.train_step(batch=batch)
        loss, _ = eng.loss_values()
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-3)
        relm = _posterior_rel(eng, outs)
        nout, rel = int((relm > 1e-4).sum().item()), relm.max().item()
        print("%s bf16 step %d posterior rel err %.3g, %d of %d above 1e-4" % (
            cls, step, rel, nout, relm.numel()))
        assert_counted("step %d posteriors" % step, nout, relm.numel(), 0.01, rel, 1e-3)


def test_engine_graph_replay_equals_eager():
    """GRU_cudnn sequence steps replayed from captured graphs (one per padded length) against the
    same steps issued eagerly, with generated inter-layer dropout: bit-identical losses,
    posteriors and trained parameters."""
    import copy
    import random
    import cudnn_cases as CC
    import pkc.neural_networks as NN
    from pkc.engine import Engine, parse_model
    cfg = CC.make_cfg("GRU_cudnn", "rmsprop")
    nets0, opts = CC.build(cfg, (NN, NN))
    for n in nets0.values():
        n.to(DEV).train()
    rs = np.random.RandomState(0)
    lens = np.array([5, 7, 12, 9, 6, 9, 8, 9, 12, 12, 10, 5, 7, 9, 9, 6])
    end = np.cumsum(lens)
    X = torch.from_numpy(rs.randn(end[-1], CC.F).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(np.stack([rs.randint(0, 64, end[-1]), rs.randint(0, 8, end[-1])],
                                    1).astype(np.int32)).to(DEV)
    runs = []
    for graphs in (False, True):
        nets = copy.deepcopy(nets0)
        eng = Engine(nets, opts, parse_model(CC.MODEL), {"fea": (0, CC.F)}, ["lab_cd", "lab_mono"],
                     batch=CC.B, max_len=16, seed=1)
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
        keep = next(n for n in eng.nodes if n.rec).lbuf[0]["keep"]
        assert 0.7 < keep[:9 * CC.B * 64].float().mean().item() < 0.9     # dropout did act
        runs.append((trace, {k: {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
                             for k, m in nets.items()}))
    (te, se), (tg, sg) = runs
    for step, ((le, pe), (lg, pg)) in enumerate(zip(te, tg)):
        assert le == lg, (step, le, lg)
        assert torch.equal(pe, pg), step
    for k in se:
        for n in se[k]:
            assert torch.equal(se[k][n], sg[k][n]), (k, n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plugin_forward_backward_vs_golden(name):
    """net(x) of the architecture class under autograd (pkc.plugin) on the golden cases: y, dL/dx
    and every parameter's .grad to the kernel-level bounds; eval mode too."""
    import pkc.neural_networks as NN
    c = CASES[name]
    net = getattr(NN, c["cls"])(c["opts"], INP)
    keys = json.loads(str(G[name + "/keys"]))
    net.load_state_dict({k: torch.from_numpy(G["%s/sd/%s" % (name, k)]) for k in keys}, strict=True)
    net.to(DEV).train()
    x = torch.from_numpy(G[name + "/x"]).to(DEV).requires_grad_(True)
    r = torch.from_numpy(G[name + "/r"]).to(DEV)
    y = net(x)
    (y * r).sum().backward()
    np.testing.assert_allclose(y.detach().cpu().numpy(), G[name + "/y"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(x.grad.cpu().numpy(), G[name + "/dx"], rtol=1e-3, atol=1e-5)
    for k, p in net.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), G["%s/grad/%s" % (name, k)], rtol=1e-3,
                                   atol=1e-5, err_msg=k)
    net.eval()
    with torch.no_grad():
        ye = net(x.detach())
    np.testing.assert_allclose(ye.cpu().numpy(), G[name + "/y_eval"], rtol=1e-4, atol=1e-5)


def test_engine_refusals():
    import cudnn_cases as CC
    import pkc.neural_networks as NN
    from pkc.engine import Engine, parse_model

    def engine(cfg, model=CC.MODEL, **kw):
        nets, opts = CC.build(cfg, (NN, NN))
        for n in nets.values():
            n.to(DEV).train()
        return Engine(nets, opts, parse_model(model), {"fea": (0, CC.F)}, ["lab_cd", "lab_mono"],
                      batch=CC.B, max_len=CC.MAX_LEN, seed=1, **kw)

    gl = CC.MODEL.replace("loss_final=sum(lc,lmw)", "lt=sum(lc,lmw)\nloss_gl=cost_gl(o2,0.01,4)\n"
                          "loss_final=sum(lt,loss_gl)")
    with pytest.raises(NotImplementedError, match="cost_gl over the GRU_cudnn architecture rnn"):
        engine(CC.make_cfg("GRU_cudnn", skip_regularization="False"), gl)

    class World:            # sync_bn: nothing to synchronise in these classes, accepted and ignored
        world = 2
    assert engine(CC.make_cfg("LSTM_cudnn"), sync_bn=World()).rec_forms()["rnn.0"] == "fp32 steps"
    with pytest.raises(NotImplementedError, match="input normalisation key gru_use_laynorm_inp"):
        engine(CC.make_cfg("GRU_cudnn", gru_use_laynorm_inp="True"))
    with pytest.raises(NotImplementedError, match="nonlinearity = elu"):
        engine(CC.make_cfg("RNN_cudnn", nonlinearity="elu"))
    with pytest.raises(ValueError, match="dropout = 1.0 is outside"):
        engine(CC.make_cfg("LSTM_cudnn", dropout="1.0"))
    with pytest.raises(NotImplementedError, match="key lstm_quant"):
        engine(CC.make_cfg("LSTM_cudnn", lstm_quant="True"))


def test_run_nn_lifecycle(tmp_path):
    """pkc.core.run_nn with arch_class = GRU_cudnn on a tiny synthetic chunk: train -> .info and
    .pkl files under torch's parameter names, resume from the .pkl, valid, forward -> the posterior
    ark, which matches the restatement's log-posteriors (loaded from the .pkl with strict=True) to
    1e-4."""
    import configparser
    import cudnn_ref as R
    from oracle import loader as OL
    from oracle import nets as ON
    from pkc.core import run_nn
    from test_gpu_run_nn import chunk_cfg, write_data
    d = str(tmp_path)
    scp, ali = write_data(d, 0, n_utt=8)
    counts = os.path.join(d, "counts")
    with open(counts, "w") as f:
        f.write("[ " + " ".join(str(i + 3) for i in range(64)) + " ]\n")
    a1 = dict(arch_library="pkc.neural_networks", arch_class="GRU_cudnn", arch_seq_model="True",
              arch_name="MLP_layers1", arch_freeze="False", arch_lr="0.0016", arch_opt="rmsprop",
              opt_momentum="0.0", opt_alpha="0.95", opt_eps="1e-8", opt_centered="False",
              opt_weight_decay="0.0", hidden_size="24", num_layers="2", bias="True",
              batch_first="False", dropout="0.2", bidirectional="True")

    def make(name, to_do, pretrain=None, **kw):
        path = chunk_cfg(d, name, to_do, scp, ali, **kw)
        cfg = configparser.ConfigParser()
        cfg.read(path)
        cfg["architecture1"] = dict(a1, arch_pretrain_file="none")
        cfg["batches"]["batch_size_train"] = cfg["batches"]["batch_size_valid"] = "4"
        if pretrain:
            for i in (1, 2, 3):
                cfg["architecture%d" % i]["arch_pretrain_file"] = os.path.join(
                    d, "%s_architecture%d.pkl" % (pretrain, i))
        with open(path, "w") as f:
            cfg.write(f)
        return path

    c0 = make("train_ck0", "train")
    c1 = make("train_ck1", "train", pretrain="train_ck0")
    run_nn(None, None, None, None, None, None, c0, True, c1)
    info = configparser.ConfigParser()
    info.read(os.path.join(d, "train_ck0.info"))
    loss0 = float(info["results"]["loss"])
    assert 0 < loss0 < 20
    ck = torch.load(os.path.join(d, "train_ck0_architecture1.pkl"), map_location="cpu",
                    weights_only=True)
    torch.manual_seed(0)
    ref = R.GRU_cudnn(a1, 440)
    assert list(ck["model_par"].keys()) == list(ref.state_dict().keys())
    assert list(ck["model_par"])[:5] == ["gru.0.weight_ih_l0", "gru.0.weight_hh_l0", "gru.0.bias_ih_l0",
                                         "gru.0.bias_hh_l0", "gru.0.weight_ih_l0_reverse"]
    assert ck["optimizer_par"]["state"], "no optimizer state in the checkpoint"
    c_va = make("valid", "valid", pretrain="train_ck0")
    run_nn(None, None, None, None, None, None, c1, True, c_va)          # resumes from the .pkl
    info.read(os.path.join(d, "train_ck1.info"))
    assert 0 < float(info["results"]["loss"]) < 20
    c_fw = make("forward", "forward", pretrain="train_ck1", counts=counts)
    run_nn(None, None, None, None, None, None, c_va, True, c_fw)
    info.read(os.path.join(d, "valid.info"))
    assert 0 < float(info["results"]["loss"]) < 20
    nxt, _, _ = run_nn(None, None, None, None, None, None, c_fw, True, c_fw)
    with open(os.path.join(d, "forward_out_dnn2_to_decode.ark"), "rb") as f:
        mats = OL.parse_mat_ark(f.read())
    assert len(mats) == 8
    ck1 = torch.load(os.path.join(d, "train_ck1_architecture1.pkl"), map_location="cpu",
                     weights_only=True)
    # 2 batches per chunk: the second chunk continued the first one's optimizer state
    assert int(float(ck["optimizer_par"]["state"][0]["step"])) == 2
    assert int(float(ck1["optimizer_par"]["state"][0]["step"])) == 4
    ref.load_state_dict(ck1["model_par"], strict=True)
    ref.eval()
    fcfg = configparser.ConfigParser()
    fcfg.read(c_fw)
    head = ON.MLP(fcfg["architecture2"], ref.out_dim)
    head.load_state_dict(torch.load(os.path.join(d, "train_ck1_architecture2.pkl"),
                                    map_location="cpu", weights_only=True)["model_par"])
    head.eval()
    chunk = nxt[1]                      # the forward chunk again (the next cfg is the same one)
    feats, ends, names = chunk.feats.cpu(), list(chunk.end_index), list(chunk.names)
    c = np.arange(3, 67, dtype=np.float64)
    prior = torch.from_numpy(np.log(c / c.sum()).astype(np.float32))
    got = dict(mats)
    beg = 0
    for name, e in zip(names, ends):
        with torch.no_grad():
            logp = head(ref(feats[beg:e, :440].unsqueeze(1)).squeeze(1))
        m = torch.from_numpy(np.array(got[name]))
        assert m.shape == logp.shape
        # the ark holds log-posteriors minus the log prior, which can cancel to ~0: absolute on the
        # ark's values, relative (the engine tests' clamped form) on the log-posteriors themselves
        dabs = (m - (logp - prior)).abs().max().item()
        rel = ((m + prior - logp).abs() / logp.abs().clamp_min(1e-3)).max().item()
        assert dabs <= 1e-4 and rel <= 1e-4, (name, dabs, rel)
        beg = e

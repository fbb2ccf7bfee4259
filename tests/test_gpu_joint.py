"""The joint speech-enhancement + recognition model (cfg/TIMIT_baselines/
TIMIT_joint_training_liGRU_fbank.cfg at test size: liGRU_SE -> MLP_SE (linear) -> liGRU_SR -> cd /
mono heads, loss_final = loss_cd + loss_mono + w * mse(out_dnn_SE, fbank_clean)) through the pkc
engine against its restatement (tests/joint_ref.py, pinned to the reference by
tests/test_joint_cpu.py): the mse loss term (pkc_mse_fused) and the way its gradient joins the
recurrent consumer's layer-0 dX slabs of the node it is taken on.

Built like tests/test_gpu_seq.py: two 13-dim streams in one chunk, B = 4, max_len 16, 12 sentences
of 5-12 frames with the reference's random left padding, injected recurrent dropout masks, three
RMSprop steps each compared from a common start, the project's tolerances unchanged."""
import configparser
import copy
import random

import numpy as np
import pytest
import torch

from cases import LIGRU_DEF

pytestmark = pytest.mark.gpu
DEV = "cuda"
FD, B = 13, 4
FEA_COLS = {"fbank_rev": (0, FD), "fbank_clean": (FD, 2 * FD)}
LAB_COLS = {"lab_cd": 2 * FD, "lab_mono": 2 * FD + 1}
SEQ = {"liGRU_SE": True, "MLP_SE": False, "liGRU_SR": True, "MLP_layers": False,
       "MLP_layers2": False}
RMS = dict(arch_opt="rmsprop", arch_lr="0.0016", opt_momentum="0.0", opt_alpha="0.95",
           opt_eps="1e-8", opt_centered="False", opt_weight_decay="0.0", arch_freeze="False")
SGD = dict(RMS, arch_opt="sgd", arch_lr="0.08", opt_dampening="0.0", opt_nesterov="False")


def model_text(w="0.5", mse="loss_se=mse(out_dnn_SE,fbank_clean)"):
    """w None: the model without the mse line."""
    head = ("out_dnn1=compute(liGRU_SE,fbank_rev)\nout_dnn_SE=compute(MLP_SE,out_dnn1)\n"
            "out_dnn2=compute(liGRU_SR,out_dnn_SE)\nout_dnn3=compute(MLP_layers,out_dnn2)\n"
            "out_dnn4=compute(MLP_layers2,out_dnn2)\nloss_mono=cost_nll(out_dnn4,lab_mono)\n"
            "loss_mono_w=mult_constant(loss_mono,1.0)\n")
    if w is None:
        return head + ("loss_cd=cost_nll(out_dnn3,lab_cd)\nloss_final=sum(loss_cd,loss_mono_w)\n"
                       "err_final=cost_err(out_dnn3,lab_cd)")
    return head + (mse + "\nloss_se_w=mult_constant(loss_se,%s)\nloss_cd=cost_nll(out_dnn3,lab_cd)\n"
                   "loss_sum1=sum(loss_cd,loss_mono_w)\nloss_final=sum(loss_sum1,loss_se_w)\n"
                   "err_final=cost_err(out_dnn3,lab_cd)" % w)


def make_cfg(opt=RMS, sr_bidir=True):
    cfg = configparser.ConfigParser()
    mlp = dict(dnn_use_laynorm_inp="False", dnn_use_batchnorm_inp="False", to_do="train",
               dnn_drop="0.0", dnn_use_batchnorm="False", dnn_use_laynorm="False", **opt)
    cfg["a1"] = dict(LIGRU_DEF, arch_name="liGRU_SE", ligru_lay="12,12", ligru_drop="0.2,0.2", **opt)
    cfg["a2"] = dict(mlp, arch_name="MLP_SE", dnn_lay=str(FD), dnn_act="linear")
    cfg["a3"] = dict(LIGRU_DEF, arch_name="liGRU_SR", ligru_lay="16,12", ligru_drop="0.2,0.2",
                     **dict(opt, ligru_bidir=str(sr_bidir)))
    cfg["a4"] = dict(mlp, arch_name="MLP_layers", dnn_lay="24", dnn_act="softmax")
    cfg["a5"] = dict(mlp, arch_name="MLP_layers2", dnn_lay="6", dnn_act="softmax")
    if opt is RMS:
        cfg["a5"]["arch_lr"] = "0.0004"
    return cfg


def build_nets(cfg, oracle=False, bf16=False):
    import pkc.neural_networks as NN
    from oracle import nets as ON
    nets, onets, opts = {}, {}, {}
    sr_out = 24 if cfg["a3"]["ligru_bidir"] == "True" else 12
    inp = {"a1": FD, "a2": 24, "a3": FD, "a4": sr_out, "a5": sr_out}
    for sec in ("a1", "a2", "a3", "a4", "a5"):
        o = cfg[sec]
        a = o["arch_name"]
        cls = "liGRU" if SEQ[a] else "MLP"
        torch.manual_seed(3)
        np.random.seed(3)
        nets[a] = getattr(NN, cls)(o, inp[sec])
        opts[a] = o
        if oracle:
            onets[a] = getattr(ON, cls)(o, inp[sec])
            onets[a].load_state_dict(nets[a].state_dict())
            if bf16 and SEQ[a]:
                ON.use_bf16_rec_matmuls(onets[a], steps=True)
            elif bf16:
                ON.use_bf16_matmuls(onets[a])
            onets[a].train()
    for n in nets.values():
        n.to(DEV).train()
    return nets, onets, opts


@pytest.fixture(scope="module")
def data():
    rs = np.random.RandomState(0)
    lens = np.sort(rs.randint(5, 13, size=12))
    end = np.cumsum(lens)
    clean = rs.randn(end[-1], FD).astype(np.float32)
    rev = (clean + 0.5 * np.roll(clean, 1, 0) + 0.3 * rs.randn(end[-1], FD)).astype(np.float32)
    X = np.concatenate([rev, clean], 1)
    lab = np.stack([rs.randint(0, 24, end[-1]), rs.randint(0, 6, end[-1])], 1).astype(np.int32)
    masks = {(a, li): torch.from_numpy((rs.rand(2 * B, H) > 0.2).astype(np.float32))
             for a, hs in (("liGRU_SE", (12, 12)), ("liGRU_SR", (16, 12))) for li, H in enumerate(hs)}
    uni = {("liGRU_SR", li): m[:B].clone() for li, m in enumerate((masks[("liGRU_SR", 0)],
                                                                    masks[("liGRU_SR", 1)]))}
    return dict(lens=lens, end=end, X=X, lab=lab, masks=masks, masks_uni={**masks, **uni})


def make_engine(nets, opts, model, data, masks="masks", **kw):
    from pkc.engine import Engine, parse_model
    kw.setdefault("rnn_drop_in", {k: v.to(DEV) for k, v in data[masks].items()})
    eng = Engine(nets, opts, parse_model(model), FEA_COLS, ["lab_cd", "lab_mono"], batch=B,
                 max_len=16, seed=1, **kw)
    eng.bind_chunk(torch.from_numpy(data["X"]).to(DEV), torch.from_numpy(data["lab"]).to(DEV),
                   data["end"][-1], end_index=data["end"])
    return eng


def oracle_batch(data, snt, T, lefts, rng_o):
    """core.py:183-200 with the engine's draws checked."""
    lens, end, X, lab = data["lens"], data["end"], data["X"], data["lab"]
    inp = torch.zeros(T, B, 2 * FD + 2)
    for k in range(B):
        n = int(lens[snt + k])
        left = rng_o.randint(0, T - n)
        b0 = int(end[snt + k] - n)
        inp[left:left + n, k, :2 * FD] = torch.from_numpy(X[b0:b0 + n])
        inp[left:left + n, k, 2 * FD:] = torch.from_numpy(lab[b0:b0 + n].astype(np.float32))
        assert left == lefts[k]
    return inp


def oracle_step(lines, onets, oopt, data, inp, T, masks="masks"):
    import joint_ref as JR
    saved = {}
    for a, hs in (("liGRU_SE", 2), ("liGRU_SR", 2)):
        f = saved[a] = onets[a].forward
        onets[a].forward = lambda x, _f=f, _a=a, _n=hs: _f(
            x, drop_masks=[data[masks][(_a, i)] for i in range(_n)])
    try:
        return JR.train_step(lines, onets, oopt, SEQ, FEA_COLS, LAB_COLS, inp, T, B)
    finally:
        for a, f in saved.items():
            onets[a].forward = f


def _vs_restatement(data, bf16, sr_bidir=True):
    from flipcheck import assert_counted, resync
    from oracle import nets as ON
    from oracle import run as OR
    from pkc import _lib as L
    from test_gpu_seq import _seq_check_update
    cfg = make_cfg(SGD if bf16 else RMS, sr_bidir)
    model = model_text()
    masks = "masks" if sr_bidir else "masks_uni"
    nets, onets, opts = build_nets(cfg, oracle=True, bf16=bf16)
    eng = make_engine(nets, opts, model, data, masks, prec=L.PREC_BF16 if bf16 else L.PREC_FP32)
    se = eng.produced["out_dnn_SE"]
    assert se.mse_grad and se.rec_consumer.dx_res == 1     # the slab in front of the rec dX slabs
    oopt = {k: ON.make_optimizer(onets[k].parameters(), opts[k]) for k in onets}
    lines = OR.parse_model(model)
    rng_e, rng_o = random.Random(7), random.Random(7)
    report, post_out = {}, []
    for step in range(3):
        eng.sync_state()
        resync(nets, onets, {k: eng.optimizer_state_dict(k) for k in nets} if step else None, oopt)
        batch = eng.next_seq_batch(rng_e)
        _, _, lefts, T = batch
        inp = oracle_batch(data, step * B, T, lefts, rng_o)
        outs = oracle_step(lines, onets, oopt, data, inp, T, masks)
        eng.train_step(batch=batch)
        loss, err = eng.loss_values()
        print("step %d loss %.6f (restatement %.6f) loss_se %.6f (%.6f)" % (
            step, loss, outs["loss_final"].item(), eng.loss_term_mean("loss_se"),
            outs["loss_se"].item()))
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-3 if bf16 else 1e-4)
        np.testing.assert_allclose(eng.loss_term_mean("loss_se"), outs["loss_se"].item(),
                                   rtol=1e-3 if bf16 else 1e-4)
        if not bf16:
            np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
        post = eng.head_output("out_dnn3").cpu()
        ref = outs["out_dnn3"].detach()
        relm = (post - ref).abs() / ref.abs().clamp_min(1e-3)
        rel, nout = relm.max().item(), int((relm > 1e-4).sum().item())
        post_out.append(nout)
        enh = eng.head_output("out_dnn_SE").cpu()
        eref = outs["out_dnn_SE"].detach().reshape(enh.shape)
        ed = (enh - eref).abs()
        escale = eref.abs().max().item()
        print("step %d posterior rel err %.3g (%d above 1e-4), out_dnn_SE max diff / scale %.3g" % (
            step, rel, nout, ed.max().item() / escale))
        if bf16:
            assert_counted("step %d posteriors" % step, nout, relm.numel(), 0.01, rel, 1e-3)
            assert_counted("step %d out_dnn_SE" % step, int((ed > 1e-4 * escale).sum()), ed.numel(),
                           0.01, ed.max().item(), 1e-3 * escale)
        else:
            assert rel < 1e-4, "step %d posterior rel err %.3g" % (step, rel)
            assert ed.max().item() <= 1e-4 * escale, "step %d out_dnn_SE off by %.3g of its scale" % (
                step, ed.max().item() / escale)
        _seq_check_update("joint", bf16, step, eng, nets, onets, opts, report, post_out)
    print("parameter outliers per step and tensor: %s" % {k: v for k, v in report.items() if v[0]})


def test_joint_engine_vs_restatement(data):
    _vs_restatement(data, bf16=False)


def test_joint_engine_bf16_vs_bf16_restatement(data):
    """bf16 matmul operands (oracle.nets.use_bf16_rec_matmuls / use_bf16_matmuls on the
    restatement), the mse on the fp32 kernel; SGD and the counted bounds of
    test_seq_engine_bf16_vs_bf16_oracle.

    liGRU_SR is unidirectional here.  The gradient that reaches out_dnn_SE through a recurrent
    layer 0 is dX = bf16(dz) bf16(W): pkc sums a bidirectional layer's two directions into one dz
    over the T*B input rows in fp32 and rounds that sum once, the restatement's cat / flip rounds
    each direction's dz and adds the two products.  Neither is wrong, and they differ by a bf16
    rounding of every element (measured on this model with a bidirectional liGRU_SR: dz of
    out_dnn_SE rms 3.8e-5 apart on an rms of 1.3e-2, i.e. 2^-8.4, while pkc's own dX equals
    bf16(dz_g) bf16(W_g) of its dz_g to 3e-9) — past the 1e-4 counted bound, which is sized for
    last-bit flips between two runs that round the SAME values (MLP_SE's weights: 125 of 312
    elements off by up to 1.4e-3 of the scale).  No earlier bf16 case has a trained layer in
    front of a recurrent one.  With one direction both sides round the same dz, and the bounds
    hold; the bidirectional model's bf16 forward and loss are held by the test below, its fp32
    step by test_joint_engine_vs_restatement."""
    _vs_restatement(data, bf16=True, sr_bidir=False)


def test_joint_bf16_bidirectional_forward(data):
    """The bidirectional model in bf16 mode: loss (rtol 1e-3), the mse term and the posteriors'
    counted bound after one step from the common start (forward products round the same rows on
    both sides)."""
    from flipcheck import assert_counted
    from oracle import nets as ON
    from oracle import run as OR
    from pkc import _lib as L
    nets, onets, opts = build_nets(make_cfg(SGD), oracle=True, bf16=True)
    eng = make_engine(nets, opts, model_text(), data, prec=L.PREC_BF16)
    oopt = {k: ON.make_optimizer(onets[k].parameters(), opts[k]) for k in onets}
    batch = eng.next_seq_batch(random.Random(7))
    inp = oracle_batch(data, 0, batch[3], batch[2], random.Random(7))
    outs = oracle_step(OR.parse_model(model_text()), onets, oopt, data, inp, batch[3])
    eng.train_step(batch=batch)
    np.testing.assert_allclose(eng.loss_values()[0], outs["loss_final"].item(), rtol=1e-3)
    np.testing.assert_allclose(eng.loss_term_mean("loss_se"), outs["loss_se"].item(), rtol=1e-3)
    post, ref = eng.head_output("out_dnn3").cpu(), outs["out_dnn3"].detach()
    relm = (post - ref).abs() / ref.abs().clamp_min(1e-3)
    assert_counted("posteriors", int((relm > 1e-4).sum()), relm.numel(), 0.01, relm.max().item(), 1e-3)


def _one_run(data, model, steps=2, opt=RMS, capture=False, nets0=None, **kw):
    """Train `steps` batches (the engine's own dropout streams); returns (engine, state dicts,
    [(loss, err)])."""
    cfg = make_cfg(opt)
    nets, _, opts = build_nets(cfg)
    if nets0 is not None:
        nets = copy.deepcopy(nets0)
    eng = make_engine(nets, opts, model, data, rnn_drop_in={}, **kw)
    if capture:
        assert eng.capture()
    rng = random.Random(7)
    trace = []
    for _ in range(steps):
        eng.train_step(batch=eng.next_seq_batch(rng))
        trace.append(eng.loss_values())
    eng.sync_state()
    sd = {k: {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
          for k, m in nets.items()}
    return eng, sd, trace


def _same_state(a, b):
    for k in a:
        for n in a[k]:
            assert torch.equal(a[k][n], b[k][n]), (k, n)


def test_mse_argument_order(data):
    _, sa, ta = _one_run(data, model_text())
    _, sb, tb = _one_run(data, model_text(mse="loss_se=mse(fbank_clean,out_dnn_SE)"))
    assert ta == tb
    _same_state(sa, sb)


def test_mse_weight_zero_is_the_model_without_it(data):
    e0, s0, t0 = _one_run(data, model_text(w="0.0"))
    e1, s1, t1 = _one_run(data, model_text(w=None))
    se = e0.produced["out_dnn_SE"]
    assert not se.mse_grad and se.rec_consumer.dx_res == 0 and len(e0.mse_terms) == 1
    assert e0.loss_term_mean("loss_se") > 0            # the loss is still launched and reported
    _same_state(s0, s1)
    for (la, ea), (lb, eb) in zip(t0, t1):
        np.testing.assert_allclose(la, lb, rtol=1e-6)
        assert ea == eb
    # and the weight does matter: 0.5 trains another model
    _, s2, _ = _one_run(data, model_text(w="0.5"))
    assert not torch.equal(s2["MLP_SE"]["wx.0.weight"], s0["MLP_SE"]["wx.0.weight"])


def test_grad_scale_scales_the_mse_gradient(data):
    """Engine(grad_scale=0.5): every gradient is exactly half (SGD: a power of two is exact
    through every product), the mse slab included."""
    e1, _, _ = _one_run(data, model_text(), steps=1, opt=SGD)
    e2, _, _ = _one_run(data, model_text(), steps=1, opt=SGD, grad_scale=0.5)
    g1, g2 = e1.gflat.cpu(), e2.gflat.cpu()
    assert g1.abs().max() > 0
    assert torch.equal(g2, 0.5 * g1)


def test_valid_mode_loss(data):
    """A valid-mode engine (dy = NULL) and the training engine's evaluation forward from equal
    state report the same loss_final."""
    cfg = make_cfg()
    nets, _, opts = build_nets(cfg)
    for n in nets.values():
        n.eval()
    tr = make_engine(nets, opts, model_text(), data, rnn_drop_in={})
    va = make_engine(copy.deepcopy(nets), opts, model_text(), data, rnn_drop_in={}, train=False)
    assert not any(n.mse_grad for n in va.nodes) and len(va.mse_terms) == 1
    bt, bv = tr.next_seq_batch(random.Random(7)), va.next_seq_batch(random.Random(7))
    tr.eval_step(bt)
    va.eval_step(bv)
    (lt, et), (lv, ev) = tr.loss_values(), va.loss_values()
    np.testing.assert_allclose(lv, lt, rtol=1e-6)
    assert et == ev
    np.testing.assert_allclose(va.loss_term_mean("loss_se"), tr.loss_term_mean("loss_se"), rtol=1e-6)


def test_joint_graph_replay_equals_eager():
    """Captured sequence graphs hold the mse launch: replayed steps equal eager ones bitwise."""
    rs = np.random.RandomState(0)
    lens = np.array([5, 7, 12, 9, 6, 9, 8, 9, 12, 12, 10, 5, 7, 9, 9, 6])   # longest 12, 9, 12, 9
    end = np.cumsum(lens)
    d = dict(lens=lens, end=end, X=rs.randn(end[-1], 2 * FD).astype(np.float32),
             lab=np.stack([rs.randint(0, 24, end[-1]), rs.randint(0, 6, end[-1])], 1).astype(np.int32),
             masks={})
    ee, se, te = _one_run(d, model_text(), steps=4)
    eg, sg, tg = _one_run(d, model_text(), steps=4, capture=True)
    assert eg.seq_captures == 2 and sorted(eg.seq_graphs) == [9, 12]
    assert te == tg
    _same_state(se, sg)


def test_refused_forms(data):
    from pkc.engine import Engine, parse_model
    cfg = make_cfg()
    nets, _, opts = build_nets(cfg)

    def eng(model, fea_cols=FEA_COLS):
        return Engine(nets, opts, parse_model(model), fea_cols, ["lab_cd", "lab_mono"], batch=B,
                      max_len=16)

    with pytest.raises(NotImplementedError, match="two produced outputs"):
        eng(model_text(mse="loss_se=mse(out_dnn_SE,out_dnn_SE)"))
    with pytest.raises(NotImplementedError, match="LogSoftmax head"):
        eng(model_text(mse="loss_se=mse(out_dnn4,fbank_clean)"))
    with pytest.raises(NotImplementedError, match="recurrent, convolution"):
        eng(model_text(mse="loss_se=mse(out_dnn1,fbank_clean)"))
    with pytest.raises(ValueError, match="13 wide, the feature stream 26"):
        eng(model_text(mse="loss_se=mse(out_dnn_SE,both)"), dict(FEA_COLS, both=(0, 2 * FD)))
    # a node read by a recurrent arch and by a second compute stays refused
    import pkc.neural_networks as NN
    nets["extra"], opts["extra"] = NN.MLP(cfg["a5"], FD).to(DEV), cfg["a5"]
    with pytest.raises(NotImplementedError, match="read by a recurrent arch and by other archs"):
        eng(model_text().replace("out_dnn4=compute(MLP_layers2,out_dnn2)",
                                 "out_dnn4=compute(MLP_layers2,out_dnn2)\n"
                                 "out_x=compute(extra,out_dnn_SE)"))


def test_mse_on_a_feed_forward_chain(data):
    """The other slab placement: a node without a recurrent consumer takes the mse gradient as
    slab 0 of its own gradient slabs, in front of its consumers' dX slabs.  Frame batches of 32
    rows, body MLP (16 relu, 13 linear) -> softmax head, mse on the body's output, three RMSprop
    steps from a common start against the restatement.  (No BatchNorm: the bias in front of one
    has a gradient that is 0 up to rounding, which RMSprop's first steps blow up to full-size
    sign steps on either side — tests/test_gpu_seq.py trains such layers with SGD.)"""
    import joint_ref as JR
    import pkc.neural_networks as NN
    from flipcheck import resync
    from oracle import nets as ON
    from oracle import run as OR
    from pkc.engine import Engine, parse_model
    from test_gpu_seq import _seq_check_update
    mlp = dict(dnn_use_laynorm_inp="False", dnn_use_batchnorm_inp="False", to_do="train", **RMS)
    cfgs = {"body": dict(mlp, arch_name="body", dnn_lay="16,%d" % FD, dnn_drop="0.0,0.0",
                         dnn_use_batchnorm="False,False", dnn_use_laynorm="False,False",
                         dnn_act="relu,linear"),
            "head": dict(mlp, arch_name="head", dnn_lay="24", dnn_drop="0.0",
                         dnn_use_batchnorm="False", dnn_use_laynorm="False", dnn_act="softmax")}
    model = ("o1=compute(body,fbank_rev)\no2=compute(head,o1)\nlc=cost_nll(o2,lab_cd)\n"
             "ls=mse(o1,fbank_clean)\nlsw=mult_constant(ls,0.5)\nloss_final=sum(lc,lsw)\n"
             "err_final=cost_err(o2,lab_cd)")
    nets, onets = {}, {}
    for k, inp in (("body", FD), ("head", FD)):
        torch.manual_seed(3)
        np.random.seed(3)
        nets[k], onets[k] = NN.MLP(cfgs[k], inp), ON.MLP(cfgs[k], inp)
        onets[k].load_state_dict(nets[k].state_dict())
        nets[k].to(DEV).train()
        onets[k].train()
    R = 32
    X, lab = data["X"][:3 * R], data["lab"][:3 * R]
    eng = Engine(nets, cfgs, parse_model(model), FEA_COLS, ["lab_cd", "lab_mono"], batch=R, seed=1)
    node = eng.produced["o1"]
    assert node.mse_grad and node.gslab is not None and getattr(node, "rec_consumer", None) is None
    eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), 3 * R)
    oopt = {k: ON.make_optimizer(onets[k].parameters(), cfgs[k]) for k in onets}
    lines = OR.parse_model(model)
    full = torch.from_numpy(np.concatenate([X, lab.astype(np.float32)], 1))
    report, post_out = {}, []
    for step in range(3):
        eng.sync_state()
        resync(nets, onets, {k: eng.optimizer_state_dict(k) for k in nets} if step else None, oopt)
        outs = JR.train_step(lines, onets, oopt, {"body": False, "head": False}, FEA_COLS,
                             LAB_COLS, full[step * R:(step + 1) * R])
        eng.train_step()
        loss, err = eng.loss_values()
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
        np.testing.assert_allclose(eng.loss_term_mean("ls"), outs["ls"].item(), rtol=1e-4)
        np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
        post, ref = eng.head_output("o2").cpu(), outs["o2"].detach()
        rel = ((post - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
        assert rel < 1e-4, "step %d posterior rel err %.3g" % (step, rel)
        post_out.append(0)
        _seq_check_update("ff", False, step, eng, nets, onets, cfgs, report, post_out)

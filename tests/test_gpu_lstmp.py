"""The projected LSTM (LSTM_cudnn with proj_size = P: torch.nn.LSTM(..., proj_size=P)) on the HIP path:
the time loops pkc_lstmp_fwd / _bwd at kernel level against the golden torch.nn.LSTM wrote
(tests/golden/lstmp.npz), then the class through the engine, the plug-in and run_nn against the
plain-torch restatement (tests/lstmp_ref.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"

G = np.load(os.path.join(GOLDEN, "lstmp.npz"))
CASES = json.loads(str(G["cases"]))
INP = int(G["inp_dim"])
PRE = "lstm.0."


def _case(name):
    o = CASES[name]["opts"]
    keys = json.loads(str(G[name + "/keys"]))
    sd = {k: torch.from_numpy(G["%s/sd/%s" % (name, k)]).to(DEV) for k in keys}
    kw = dict(sd=sd, prefix=PRE, layers=int(o["num_layers"]), bidir=o["bidirectional"] == "True",
              bias=o["bias"] == "True")
    x = torch.from_numpy(G[name + "/x"]).to(DEV)
    r = torch.from_numpy(G[name + "/r"]).to(DEV)
    return kw, x, r, keys


@pytest.mark.parametrize("name", sorted(CASES))
def test_lstmp_kernels_vs_golden(name):
    """pkc_lstmp_fwd / _bwd on the four golden cases: y to rtol 1e-4 / atol 1e-5, dL/dx and every
    parameter gradient (weight_hr included) to rtol 1e-3 / atol 1e-5 — the bounds
    tests/test_gpu_cudnn.py holds the plain cells to; equal key sets; a rerun is bit-identical; eval
    matches y_eval."""
    from lstmp_kernel import run_stack
    kw, x, r, keys = _case(name)
    y, dx, grads, _ = run_stack(x=x, r=r, **kw)

    def share(got, ref, rtol, atol=1e-5):       # the largest share of the bound in use
        return float((np.abs(got.cpu().numpy() - ref) / (atol + rtol * np.abs(ref))).max())
    print("%s: share of the bound in use: y %.3f, dx %.3f, gradients %.3f" % (
        name, share(y, G[name + "/y"], 1e-4), share(dx, G[name + "/dx"], 1e-3),
        max(share(grads[k], G["%s/grad/%s" % (name, k)], 1e-3) for k in keys if k in grads)))
    np.testing.assert_allclose(y.cpu().numpy(), G[name + "/y"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(dx.cpu().numpy(), G[name + "/dx"], rtol=1e-3, atol=1e-5)
    assert sorted(grads) == sorted(keys)
    assert any("weight_hr" in k for k in keys)
    for k in keys:
        np.testing.assert_allclose(grads[k].cpu().numpy(), G["%s/grad/%s" % (name, k)], rtol=1e-3,
                                   atol=1e-5, err_msg=k)
    y2, dx2, grads2, _ = run_stack(x=x, r=r, **kw)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    assert all(torch.equal(grads[k], grads2[k]) for k in keys)
    ye, _, _, _ = run_stack(x=x, r=r, train=False, backward=False, **kw)
    np.testing.assert_allclose(ye.cpu().numpy(), G[name + "/y_eval"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("H,P,B,bidir", [(19, 7, 5, True), (22, 10, 5, True), (550, 160, 5, True),
                                         (256, 64, 3, False), (512, 128, 3, False),
                                         (1024, 256, 3, False)])
def test_lstmp_kernels_other_paths(H, P, B, bidir):
    """The paths the golden's shapes (16-byte loads, 4-wave tiles in all four kernels) do not take,
    against the restatement computed on the CPU here, at the kernel-level bounds; one layer, T = 3.
    A kernel takes 8 waves where its contraction is >= 256 long, else 4; the contractions are
    P (cell step), H (projection step), 4H (BPTT A: dhp) and P (BPTT B: the gate gradients).
      (19, 7)     element loads in all contractions; 4 waves in all four kernels
      (22, 10)    8-byte loads in all contractions (4H = 88: 16-byte); 4 waves
      (550, 160)  8-byte loads over H, 16-byte over P and 4H; 8 waves in the projection and A
      (256, 64)   the smallest H on the 8-wave projection (H = 256) and A (4H = 1024 >= 256)
      (512, 128)  as (256, 64): cell step and B still on 4 waves (P = 128)
      (1024, 256) P = 256: the 8-wave cell step and B, so all four kernels on 8 waves."""
    import lstmp_ref as R
    from lstmp_kernel import run_stack
    nd = 2 if bidir else 1
    o = dict(hidden_size=str(H), proj_size=str(P), num_layers="1", bias="True", batch_first="False",
             dropout="0.0", bidirectional=str(bidir))
    torch.manual_seed(H)
    net = R.LSTM_cudnn(o, 7).train()
    x = torch.randn(3, B, 7, requires_grad=True)
    r = torch.randn(3, B, nd * P)
    y = net(x)
    (y * r).sum().backward()
    sd = {k: v.detach().to(DEV) for k, v in net.state_dict().items()}
    gy, gdx, grads, _ = run_stack(sd=sd, prefix=PRE, x=x.detach().to(DEV), r=r.to(DEV), layers=1,
                                  bidir=bidir, bias=True)
    np.testing.assert_allclose(gy.cpu().numpy(), y.detach().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(gdx.cpu().numpy(), x.grad.numpy(), rtol=1e-3, atol=1e-5)
    assert sorted(grads) == sorted(k for k, _ in net.named_parameters())
    for k, p in net.named_parameters():
        np.testing.assert_allclose(grads[k].cpu().numpy(), p.grad.numpy(), rtol=1e-3, atol=1e-5,
                                   err_msg=k)


def _layer0_ops(name):
    kw, x, r, _ = _case(name)
    sd = kw["sd"]
    T, B, _ = x.shape
    P, H = sd[PRE + "weight_hr_l0"].shape
    x2 = x.reshape(T * B, -1)
    wpre, U, bhh, Whr = [], [], [], []
    for sfx in ("", "_reverse"):
        w = x2 @ sd[PRE + "weight_ih_l0" + sfx].t() + sd[PRE + "bias_ih_l0" + sfx]
        wpre.append(w.view(T, B, 4 * H).contiguous())
        U.append(sd[PRE + "weight_hh_l0" + sfx].contiguous())
        bhh.append(sd[PRE + "bias_hh_l0" + sfx])
        Whr.append(sd[PRE + "weight_hr_l0" + sfx].contiguous())
    return (T, B, H, P), (wpre, U, bhh, Whr), r[:, :, :2 * P].contiguous()


def test_lstmp_bidirectional_equals_two_unidirectional():
    """Layer 0 of case (c) (B = 17, H = 48, P = 20): the two directions of one call against two
    one-direction calls, the second on the time-flipped operands — bit for bit, forward (y, hs, cs,
    ht) and backward (dgates, dhp); both halves non-zero."""
    from lstmp_kernel import Layer
    (T, B, H, P), (wpre, U, bhh, Whr), dy = _layer0_ops("lstmp_c")
    both = Layer(T, B, H, P, 2)
    y = both.forward(wpre, U, bhh, Whr).clone()
    both.backward(dy)
    fw = Layer(T, B, H, P, 1)
    y0 = fw.forward(wpre[:1], U[:1], bhh[:1], Whr[:1]).clone()
    fw.backward(dy[:, :, :P].contiguous())
    bw = Layer(T, B, H, P, 1)
    y1 = bw.forward([wpre[1].flip(0).contiguous()], U[1:], bhh[1:], Whr[1:]).clone()
    bw.backward(dy[:, :, P:].flip(0).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y[:, :, :P], y0) and torch.equal(y[:, :, P:], y1.flip(0))
    # states: direction 0 keeps the state after time t in slot t + 1; direction 1 in slot t, which
    # for the flipped one-direction run is slot T - t of ITS forward layout
    for name in ("hs", "cs"):
        s2, s0, s1 = getattr(both, name), getattr(fw, name), getattr(bw, name)
        assert torch.equal(s2[0], s0[0]) and torch.equal(s2[1], s1[0].flip(0)), name
    for name in ("ht", "dgates", "dhp"):
        s2, s0, s1 = getattr(both, name), getattr(fw, name), getattr(bw, name)
        assert torch.equal(s2[0], s0[0]) and torch.equal(s2[1], s1[0].flip(0)), name
        assert s0.abs().sum() > 0 and s1.abs().sum() > 0, name
    assert y0.abs().sum() > 0 and y1.abs().sum() > 0


def test_lstmp_kernel_dropout_and_entry_checks():
    """Inter-layer dropout at kernel level: an injected keep mask gives y = h keep / (1 - p) and
    gates dhp; a generated mask is {0, 1} with a keep rate within 0.05 of 1 - p and repeats at the
    same step counter; eval applies none.  Each bad argument gives a negative status with its word
    in pkc_last_error()."""
    from lstmp_kernel import Layer
    from pkc import _lib as L
    (T, B, H, P), ops, dy = _layer0_ops("lstmp_c")
    plain = Layer(T, B, H, P, 2)
    h = plain.forward(*ops).clone()
    rs = np.random.RandomState(2)
    keep = torch.from_numpy((rs.rand(T, B, 2 * P) > 0.3).astype(np.uint8)).to(DEV)
    inj = Layer(T, B, H, P, 2, drop_p=0.3, keep_in=keep)
    y = inj.forward(*ops)
    want = torch.where(keep.bool(), h * (1.0 / (1.0 - 0.3)), torch.zeros_like(h))
    torch.testing.assert_close(y, want, rtol=1e-6, atol=0)
    assert torch.equal(inj.keep, keep) and torch.equal(inj.hs, plain.hs)
    dgi = inj.backward(dy).clone()
    dgp = plain.backward(torch.where(keep.bool(), dy * (1.0 / (1.0 - 0.3)), torch.zeros_like(dy)))
    # the two runs differ by the rounding of 1 / (1 - p) on dy (one ulp, 6e-8 relative), carried
    # through contractions of up to 4H = 192 terms of magnitude <= 1: 1e-7 absolute, 1e-5 relative
    torch.testing.assert_close(dgi, dgp, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(inj.dhp, plain.dhp, rtol=1e-5, atol=1e-7)
    # at the first BPTT step (no recurrent part) dhp is the masked, scaled dy itself
    last = dy[T - 1, :, :P]
    torch.testing.assert_close(inj.dhp[0, T - 1], torch.where(keep[T - 1, :, :P].bool(), last / 0.7,
                                                              torch.zeros_like(last)),
                               rtol=1e-6, atol=0)
    gen = Layer(T, B, H, P, 2, drop_p=0.3)
    gen.a.seed, gen.a.stream_id = 7, 11
    yg = gen.forward(*ops).clone()
    k1 = gen.keep.clone()
    assert set(k1.unique().tolist()) <= {0, 1}
    assert abs(k1.float().mean().item() - 0.7) < 0.05
    torch.testing.assert_close(yg, torch.where(k1.bool(), h / 0.7, torch.zeros_like(h)), rtol=1e-6,
                               atol=0)
    gen.forward(*ops)
    assert torch.equal(gen.keep, k1)
    ev = Layer(T, B, H, P, 2, train=False, drop_p=0.3)       # eval: no dropout
    assert torch.equal(ev.forward(*ops), h)
    # entry checks
    lib = L.lib()
    bad = Layer(T, B, H, P, 2)
    bad.forward(*ops)
    for field, value, word in (("hs", None, "null"), ("ht", None, "null"), ("P", 0, "P=0"),
                               ("P", -3, "P=-3"), ("P", H, "P=%d" % H), ("H", 4096, "2048"),
                               ("ndir", 3, "ndir"), ("ndir", 0, "ndir"), ("drop_p", 1.0, "drop_p"),
                               ("drop_p", -0.5, "drop_p")):
        old = getattr(bad.a, field)
        setattr(bad.a, field, value)
        assert lib.pkc_lstmp_fwd(C.byref(bad.a), None) < 0, (field, value)
        assert word in lib.pkc_last_error().decode(), (field, value, lib.pkc_last_error())
        setattr(bad.a, field, old)
    old = bad.a.Whr[1]
    bad.a.Whr[1] = None
    assert lib.pkc_lstmp_fwd(C.byref(bad.a), None) < 0 and "null" in lib.pkc_last_error().decode()
    bad.a.Whr[1] = old
    assert lib.pkc_lstmp_fwd(None, None) < 0 and "null" in lib.pkc_last_error().decode()
    for field in ("dy", "dhp", "wt"):
        bad.backward(dy)
        setattr(bad.a, field, None)
        assert lib.pkc_lstmp_bwd(C.byref(bad.a), None) < 0, field
        assert "null" in lib.pkc_last_error().decode()
        setattr(bad.a, field, getattr(bad, field).data_ptr())


# ------------------------------------------------------------------------------- engine level
def _engine_setup(optk, bf16=False, train=True, batch=None, proj=None):
    import lstmp_cases as LC
    import pkc.neural_networks as NN
    from pkc import _lib as L
    from pkc.engine import Engine, parse_model
    proj = LC.PROJ if proj is None else proj
    cfg = LC.make_cfg(optk, proj=proj)
    nets, opts = LC.build(cfg, (NN, NN))
    for n in nets.values():
        n.to(DEV)
        n.train() if train else n.eval()
    lens, end, X, lab, masks = LC.make_data(proj or LC.HID)     # masks as wide as a layer's output
    eng = Engine(nets, opts, parse_model(LC.MODEL), {"fea": (0, LC.F)}, ["lab_cd", "lab_mono"],
                 batch=batch or LC.B, max_len=LC.MAX_LEN, seed=1, train=train,
                 prec=L.PREC_BF16 if bf16 else L.PREC_FP32,
                 rnn_drop_in={k: v.to(DEV) for k, v in masks.items()})
    eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), end[-1], end_index=end)
    return LC, cfg, nets, opts, eng, (lens, end, X, lab, masks)


def _posterior_rel(eng, outs):
    post = eng.head_output("o2").cpu()
    ref = outs["o2"].detach().float()
    return (post - ref).abs() / ref.abs().clamp_min(1e-3)


@pytest.mark.parametrize("optk", ["sgd", "rmsprop"])
def test_engine_vs_restatement(optk):
    """Three training steps through the engine (2 bidirectional layers of 32 projected to 12,
    dropout 0.2 with injected masks, the padded batches of next_seq_batch, two softmax heads)
    against the restatement, each step from the engine's state (flipcheck.resync): loss rtol 1e-4,
    posteriors < 1e-4 relative (denominator clamped at 1e-3), parameters by
    cudnn_cases.check_update."""
    import random
    from flipcheck import resync
    LC, cfg, nets, opts, eng, (lens, end, X, lab, masks) = _engine_setup(optk)
    assert eng.rec_forms() == {"rnn.0": "fp32 steps", "rnn.1": "fp32 steps"}
    assert nets["rnn"].out_dim == 2 * LC.PROJ
    assert "lstm.0.weight_hr_l1_reverse" in nets["rnn"].state_dict()
    onets, _, oopt = LC.oracle_nets(cfg)
    rng = random.Random(7)
    report = {}
    for step, (inp, T, lefts) in enumerate(LC.batches(lens, end, X, lab)):
        eng.sync_state()
        resync(nets, onets, {k: eng.optimizer_state_dict(k) for k in nets} if step else None, oopt)
        batch = eng.next_seq_batch(rng)
        assert batch[3] == T and list(batch[2]) == lefts
        outs = LC.oracle_step(onets, oopt, inp, T, masks)
        eng.train_step(batch=batch)
        loss, err = eng.loss_values()
        rel = _posterior_rel(eng, outs).max().item()
        print("lstmp %s step %d loss %.6f (ref %.6f) posterior rel err %.3g" % (
            optk, step, loss, outs["loss_final"].item(), rel))
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
        np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
        assert rel < 1e-4, "step %d posterior rel err %.3g" % (step, rel)
        eng.sync_state()
        LC.check_update(step, optk, opts, {k: nets[k].state_dict() for k in nets},
                        {k: onets[k].state_dict() for k in onets}, report)
    print("lstmp %s parameter outliers: %s" % (optk, {k: v for k, v in report.items() if v[0]}))


def test_engine_eval_and_forward_mode():
    """Validation (B = 4) and forward mode (one utterance per batch) apply no dropout: posteriors
    against the restatement in eval, < 1e-4 relative."""
    import random
    from oracle import run as OR
    for batch in (4, 1):
        LC, cfg, nets, opts, eng, (lens, end, X, lab, masks) = _engine_setup(
            "sgd", train=False, batch=batch)
        onets, _, oopt = LC.oracle_nets(cfg)
        for k in onets:
            onets[k].load_state_dict({n: v.cpu() for n, v in nets[k].state_dict().items()})
            onets[k].eval()
        if batch == 4:
            inp, T, _ = LC.batches(lens, end, X, lab, steps=1)[0]
            eng.eval_step(batch=eng.next_seq_batch(random.Random(7)))
            B = 4
        else:
            T, B = int(lens[0]), 1
            inp = torch.zeros(T, 1, LC.F + 2)
            inp[:, 0, :LC.F] = torch.from_numpy(X[:T])
            inp[:, 0, LC.F:] = torch.from_numpy(lab[:T].astype(np.float32))
            eng.eval_step()
        with torch.no_grad():
            outs = OR.forward_model(OR.parse_model(LC.MODEL), onets,
                                    {"rnn": True, "head": False, "mono": False}, {"fea": (0, LC.F)},
                                    {"lab_cd": LC.F, "lab_mono": LC.F + 1}, inp, T, B)
        rel = _posterior_rel(eng, outs).max().item()
        assert rel < 1e-4, "batch %d posterior rel err %.3g" % (batch, rel)
        loss, _ = eng.loss_values()
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)


def test_engine_bf16_mode():
    """pkc_prec = bf16: the input projections, their dX / dW and the weight_hh and weight_hr
    gradient matmuls on bf16-rounded operands, the products inside both step kernels exact fp32
    (rec_forms "fp32 steps") — against the restatement with exactly that rounding (SGD): loss rtol
    1e-3, at most 1 % of the posteriors above 1e-4 relative, none above 1e-3."""
    import random
    from flipcheck import assert_counted, resync
    from oracle import nets as ON
    LC, cfg, nets, opts, eng, (lens, end, X, lab, masks) = _engine_setup("sgd", bf16=True)
    assert eng.rec_forms() == {"rnn.0": "fp32 steps", "rnn.1": "fp32 steps"}
    onets, _, oopt = LC.oracle_nets(cfg)
    onets["rnn"].proj = lambda x, w, b: ON._BF16Linear.apply(x, w, b)
    onets["rnn"].recur = lambda h, w: ON._BF16dWLinear.apply(h, w)
    onets["rnn"].hproj = lambda h, w: ON._BF16dWLinear.apply(h, w)
    ON.use_bf16_matmuls(onets["head"])
    ON.use_bf16_matmuls(onets["mono"])
    rng = random.Random(7)
    for step, (inp, T, _) in enumerate(LC.batches(lens, end, X, lab)):
        eng.sync_state()
        resync(nets, onets, None, oopt)
        batch = eng.next_seq_batch(rng)
        outs = LC.oracle_step(onets, oopt, inp, T, masks)
        eng.train_step(batch=batch)
        loss, _ = eng.loss_values()
        relm = _posterior_rel(eng, outs)
        nout, rel = int((relm > 1e-4).sum().item()), relm.max().item()
        print("lstmp bf16 step %d loss %.6f (ref %.6f) posterior rel err %.3g, %d of %d above 1e-4" % (
            step, loss, outs["loss_final"].item(), rel, nout, relm.numel()))
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-3)
        assert_counted("step %d posteriors" % step, nout, relm.numel(), 0.01, rel, 1e-3)


def test_engine_graph_replay_equals_eager():
    """Sequence steps replayed from captured graphs (one per padded length) against the same steps
    issued eagerly, with generated inter-layer dropout: bit-identical losses, posteriors and
    trained parameters over 4 steps."""
    import copy
    import random
    import lstmp_cases as LC
    import pkc.neural_networks as NN
    from pkc.engine import Engine, parse_model
    cfg = LC.make_cfg("rmsprop")
    nets0, opts = LC.build(cfg, (NN, NN))
    for n in nets0.values():
        n.to(DEV).train()
    rs = np.random.RandomState(0)
    lens = np.array([5, 7, 12, 9, 6, 9, 8, 9, 12, 12, 10, 5, 7, 9, 9, 6])
    end = np.cumsum(lens)
    X = torch.from_numpy(rs.randn(end[-1], LC.F).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(np.stack([rs.randint(0, 64, end[-1]), rs.randint(0, 8, end[-1])],
                                    1).astype(np.int32)).to(DEV)
    runs = []
    for graphs in (False, True):
        nets = copy.deepcopy(nets0)
        eng = Engine(nets, opts, parse_model(LC.MODEL), {"fea": (0, LC.F)}, ["lab_cd", "lab_mono"],
                     batch=LC.B, max_len=16, seed=1)
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
        assert 0.7 < keep[:9 * LC.B * 2 * LC.PROJ].float().mean().item() < 0.9   # dropout did act
        runs.append((trace, {k: {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
                             for k, m in nets.items()}))
    (te, se), (tg, sg) = runs
    for step, ((le, pe), (lg, pg)) in enumerate(zip(te, tg)):
        assert le == lg, (step, le, lg)
        assert torch.equal(pe, pg), step
    for k in se:
        for n in se[k]:
            assert torch.equal(se[k][n], sg[k][n]), (k, n)
    assert not torch.equal(se["rnn"]["lstm.0.weight_hr_l0"],
                           nets0["rnn"].state_dict()["lstm.0.weight_hr_l0"].cpu())   # it trained


def test_engine_proj_size_zero_builds_todays_buffers():
    """proj_size = 0 is the plain LSTM_cudnn: out_dim 2 * HID, the buffers of pkc_rnn_std_args and
    none of the projected ones."""
    LC, cfg, nets, opts, eng, _ = _engine_setup("sgd", proj=0)
    assert nets["rnn"].out_dim == 2 * LC.HID
    n = next(n for n in eng.nodes if n.rec)
    assert n.N == 2 * LC.HID and eng.rec_forms() == {"rnn.0": "fp32 steps", "rnn.1": "fp32 steps"}
    for lb in n.lbuf:
        assert lb["D"] == 2 * LC.HID and lb["P"] == 0
        assert lb["ht"] is None and lb["dhp"] is None and lb["wt"] is None
        assert lb["hs"].numel() == 2 * (LC.MAX_LEN + 1) * LC.B * LC.HID
        assert lb["ut"].numel() == 2 * LC.HID * 4 * LC.HID
    assert not any(k[0] == "dWhr" for _, k, _ in n.params())


@pytest.mark.parametrize("name", sorted(CASES))
def test_plugin_forward_backward_vs_golden(name):
    """net(x) of the class under autograd (pkc.plugin) on the golden cases: y, dL/dx and every
    parameter's .grad to the kernel-level bounds; eval mode too."""
    import pkc.neural_networks as NN
    c = CASES[name]
    net = NN.LSTM_cudnn(c["opts"], INP)
    keys = json.loads(str(G[name + "/keys"]))
    net.load_state_dict({k: torch.from_numpy(G["%s/sd/%s" % (name, k)]) for k in keys}, strict=True)
    net.to(DEV).train()
    x = torch.from_numpy(G[name + "/x"]).to(DEV).requires_grad_(True)
    r = torch.from_numpy(G[name + "/r"]).to(DEV)
    y = net(x)
    (y * r).sum().backward()
    np.testing.assert_allclose(y.detach().cpu().numpy(), G[name + "/y"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(x.grad.cpu().numpy(), G[name + "/dx"], rtol=1e-3, atol=1e-5)
    assert sorted(k for k, _ in net.named_parameters()) == sorted(keys)
    for k, p in net.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), G["%s/grad/%s" % (name, k)], rtol=1e-3,
                                   atol=1e-5, err_msg=k)
    net.eval()
    with torch.no_grad():
        ye = net(x.detach())
    np.testing.assert_allclose(ye.cpu().numpy(), G[name + "/y_eval"], rtol=1e-4, atol=1e-5)


def test_run_nn_lifecycle(tmp_path):
    """pkc.core.run_nn with arch_class = LSTM_cudnn and proj_size = 10 on a tiny synthetic chunk:
    train -> .info and .pkl files under torch's parameter names (weight_hr included), resume from
    the .pkl, valid, forward -> the posterior ark, which matches the restatement's log-posteriors
    (loaded from the .pkl with strict=True) to 1e-4.  The .pkl loads strictly into
    torch.nn.LSTM(proj_size=10)."""
    import configparser
    import lstmp_ref as R
    from oracle import loader as OL
    from oracle import nets as ON
    from pkc.core import run_nn
    from test_gpu_run_nn import chunk_cfg, write_data
    d = str(tmp_path)
    scp, ali = write_data(d, 0, n_utt=8)
    counts = os.path.join(d, "counts")
    with open(counts, "w") as f:
        f.write("[ " + " ".join(str(i + 3) for i in range(64)) + " ]\n")
    a1 = dict(arch_library="pkc.neural_networks", arch_class="LSTM_cudnn", arch_seq_model="True",
              arch_name="MLP_layers1", arch_freeze="False", arch_lr="0.0016", arch_opt="rmsprop",
              opt_momentum="0.0", opt_alpha="0.95", opt_eps="1e-8", opt_centered="False",
              opt_weight_decay="0.0", hidden_size="24", proj_size="10", num_layers="2", bias="True",
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
    assert 0 < float(info["results"]["loss"]) < 20
    ck = torch.load(os.path.join(d, "train_ck0_architecture1.pkl"), map_location="cpu",
                    weights_only=True)
    torch.manual_seed(0)
    ref = R.LSTM_cudnn(a1, 440)
    assert list(ck["model_par"].keys()) == list(ref.state_dict().keys())
    assert list(ck["model_par"])[:6] == ["lstm.0.weight_ih_l0", "lstm.0.weight_hh_l0",
                                         "lstm.0.bias_ih_l0", "lstm.0.bias_hh_l0",
                                         "lstm.0.weight_hr_l0", "lstm.0.weight_ih_l0_reverse"]
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
    assert int(float(ck["optimizer_par"]["state"][0]["step"])) == 2
    assert int(float(ck1["optimizer_par"]["state"][0]["step"])) == 4
    tm = torch.nn.LSTM(440, 24, num_layers=2, bias=True, bidirectional=True, proj_size=10)
    tm.load_state_dict({k[len("lstm.0."):]: v for k, v in ck1["model_par"].items()}, strict=True)
    assert not torch.equal(ck1["model_par"]["lstm.0.weight_hr_l0"],
                           ck["model_par"]["lstm.0.weight_hr_l0"])       # weight_hr trains
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
        dabs = (m - (logp - prior)).abs().max().item()
        rel = ((m + prior - logp).abs() / logp.abs().clamp_min(1e-3)).max().item()
        assert dabs <= 1e-4 and rel <= 1e-4, (name, dabs, rel)
        beg = e

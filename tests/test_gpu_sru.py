"""The SRU architecture on the HIP path: the one-launch time loops at kernel level against the float64
restatement (tests/sru_ref.py; cases and references in tests/sru_cases.py), then the architecture class
through the engine, the plug-in and run_nn against the same restatement.  Nothing here is pinned to
the reference project: its SRU class is commented out.

Kernel rule, per case and quantity (y, c, dU, dXh, dweight_c, dbias):
  * |kernel - ref64| <= 1e-5 + 1e-4 |ref64| elementwise (tests/test_gpu_cudnn.py's bound), and
  * max|kernel - ref64| <= 4 * d_ref, d_ref = max|ref32 - ref64| being what the restatement itself
    loses in float32 on that case (the rule of tests/test_gpu_kaldi_feats.py).
Engine rule: INTEGRATION's plug-in parity bounds — posteriors and loss within 1e-4 relative, trained
parameters within 1e-3 of their norm."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sru_cases as SC
import sru_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run_case(name):
    """The case through pkc_sru_fwd / _bwd.  Returns {quantity: tensor} and the Layer."""
    from sru_kernel import Layer
    d, T, B, D, k, act, skip, alpha, extra, slabs = SC.KERNEL_CASES[name]
    U, xw, wc, bias, dy = (t.to(DEV).contiguous() for t in SC.kernel_operands(name))
    n = d * D
    lay = Layer(T, B, d, D, k, n if k == 3 else n + 1, act, skip, alpha)
    y = lay.forward(U, wc, bias, xw if (k == 3 and skip) else None, n + extra)
    du, dxh, dwc, dbias = lay.backward(dy if slabs > 1 else dy[0])
    torch.cuda.synchronize()
    out = dict(y=y, c=lay.cs, dU=du, dwc=dwc, dbias=dbias)
    if k == 3 and skip:
        out["dXh"] = dxh
    return {q: v.clone() for q, v in out.items()}, lay


@pytest.mark.parametrize("name", sorted(SC.KERNEL_CASES))
def test_sru_kernels_vs_float64_restatement(name):
    """Measured on an MI355X over these cases (largest ratio max|kernel - ref64| / d_ref per
    quantity): see DESIGN 5, "SRU"."""
    got, _ = _run_case(name)
    r64, d_ref, _ = SC.kernel_reference(name)
    assert sorted(got) == sorted(r64)
    bad = []
    for q in SC.QUANT:
        if q not in got:
            continue
        g, ref = got[q].cpu().double().reshape(r64[q].shape), r64[q]
        err = (g - ref).abs()
        d_gpu = float(err.max())
        share = float((err / (SC.ATOL + SC.RTOL * ref.abs())).max())
        print("%s / %s: gpu-fp64 %.3g, fp32-fp64 (d_ref) %.3g, ratio %.2f, share of rtol/atol %.3f"
              % (name, q, d_gpu, d_ref[q], d_gpu / d_ref[q] if d_ref[q] else float(d_gpu > 0) * np.inf,
                 share))
        if share > 1.0:
            bad.append("%s: %.3f of the rtol 1e-4 / atol 1e-5 bound" % (q, share))
        if d_gpu > 4 * d_ref[q]:
            bad.append("%s: max|gpu - fp64| = %.3g against 4 x d_ref = 4 x %.3g" % (q, d_gpu, d_ref[q]))
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("name", ["d8_T7_B3_bi_k4_tanh", "d550_T20_B8_bi_k3_relu_alpha"])
def test_sru_kernels_rerun_bit_identical(name):
    a, _ = _run_case(name)
    b, _ = _run_case(name)
    assert all(torch.equal(a[q], b[q]) for q in a)


@pytest.mark.parametrize("name", ["d96_T33_B3_bi_k3_tanh_alpha", "d96_T7_B8_bi_k4_relu",
                                  "d550_T20_B8_bi_k4_tanh"])
def test_sru_bidirectional_equals_two_unidirectional(name):
    """One bidirectional call against two one-direction calls, the second on the time-flipped
    operands: bit for bit, forward (y, c) and backward (dU, dXh, dweight_c, dbias)."""
    from sru_kernel import Layer
    d, T, B, D, k, act, skip, alpha, extra, slabs = SC.KERNEL_CASES[name]
    assert D == 2
    both, _ = _run_case(name)
    U, xw, wc, bias, dy = (t.to(DEV) for t in SC.kernel_operands(name))
    u4, dy = U.view(T, B, 2 * d, k), dy[0]
    half = lambda v, h: torch.cat([v[h * d:(h + 1) * d], v[(2 + h) * d:(3 + h) * d]]).contiguous()  # noqa: E731
    for h in (0, 1):
        fl = (lambda t: t.flip(0)) if h else (lambda t: t)
        sl = slice(h * d, (h + 1) * d)
        lay = Layer(T, B, d, 1, k, d if k == 3 else d + 1, act, skip, alpha)
        xh = fl(xw[:, :, sl]).contiguous()
        y = lay.forward(fl(u4[:, :, sl]).reshape(T, B, -1).contiguous(), half(wc, h), half(bias, h),
                        xh if k == 3 else None, d)
        du, dxh, dwc, dbias = lay.backward(fl(dy[:, :, sl]).contiguous())
        torch.cuda.synchronize()
        assert torch.equal(both["y"][:, :, sl], fl(y)) and torch.equal(both["c"][:, :, sl], fl(lay.cs))
        assert torch.equal(both["dU"].view(T, B, 2 * d, k)[:, :, sl], fl(du).view(T, B, d, k))
        if k == 3:
            assert torch.equal(both["dXh"][:, :, sl], fl(dxh))
        assert torch.equal(half(both["dwc"], h), dwc) and torch.equal(half(both["dbias"], h), dbias)
        assert y.abs().sum() > 0 and du.abs().sum() > 0


def test_sru_kernel_dropout():
    """m_c: an injected keep mask gives the restatement's values (forward and backward); a
    generated one is {0, 1} with a keep rate near 1 - p, one mask for all t, written for the
    backward and repeated at the same step counter; eval applies none."""
    from sru_kernel import Layer
    name = "d96_T7_B8_bi_k4_relu"
    d, T, B, D, k, act, skip, alpha, extra, slabs = SC.KERNEL_CASES[name]
    n, p = d * D, 0.3
    ops = SC.kernel_operands(name)
    U, xw, wc, bias, dy = (t.to(DEV) for t in ops)
    rs = np.random.RandomState(2)
    keep = torch.from_numpy((rs.rand(B, n) > p).astype(np.uint8))
    m_c = keep.double() / (1 - p)
    leaves = [t.double().requires_grad_(True) for t in (ops[0], ops[1][:, :, :n], ops[2], ops[3])]
    y64, c64 = R.cell_fwd(*leaves, d, D, k, act, skip, alpha, m_c)
    (y64 * ops[4][0].double()).sum().backward()
    inj = Layer(T, B, d, D, k, n + 1, act, skip, alpha, drop_p=p, keep_in=keep.to(DEV))
    y = inj.forward(U, wc, bias)
    du, _, dwc, dbias = inj.backward(dy[0])
    torch.cuda.synchronize()
    assert torch.equal(inj.keep.cpu(), keep)
    for got, ref in ((y, y64), (inj.cs, c64), (du, leaves[0].grad), (dwc, leaves[2].grad),
                     (dbias, leaves[3].grad)):
        torch.testing.assert_close(got.cpu().double().reshape(ref.shape), ref.detach(), rtol=SC.RTOL,
                                   atol=SC.ATOL)
    gen = Layer(T, B, d, D, k, n + 1, act, skip, alpha, drop_p=p)
    gen.a.seed, gen.a.stream_id = 7, 11
    yg = gen.forward(U, wc, bias).clone()
    k1 = gen.keep.clone()
    assert set(k1.unique().tolist()) <= {0, 1}
    assert abs(k1.float().mean().item() - (1 - p)) < 0.05           # 1536 draws: sigma 0.012
    # one mask for all t: y - (1 - r) x' = r g(c) m_c vanishes on the dropped columns at every t
    plain = Layer(T, B, d, D, k, n + 1, act, skip, alpha)
    yp = plain.forward(U, wc, bias).clone()
    torch.testing.assert_close(plain.cs, gen.cs, rtol=0, atol=0)     # c does not see the mask
    ev = Layer(T, B, d, D, k, n + 1, act, skip, alpha, train=False, drop_p=p)
    assert torch.equal(ev.forward(U, wc, bias), yp)                  # eval: no mask
    y0 = Layer(T, B, d, D, k, n + 1, act, skip, alpha, drop_p=p,
               keep_in=torch.zeros(B, n, dtype=torch.uint8, device=DEV)).forward(U, wc, bias)
    kb = k1.bool().unsqueeze(0).expand(T, B, n)
    torch.testing.assert_close(yg[~kb], y0[~kb], rtol=0, atol=0)
    torch.testing.assert_close((yg - y0)[kb], ((yp - y0) / (1 - p))[kb], rtol=1e-5, atol=1e-6)
    gen.forward(U, wc, bias)
    assert torch.equal(gen.keep, k1)


def test_sru_input_mask_and_dx_fold():
    """pkc_sru_mask_x (injected and generated m_x, an input with a leading dimension wider than
    n_in) and pkc_sru_dx (the slab sum, the mask and the highway gradient into one slab)."""
    from sru_kernel import fold_dx, mask_x
    T, B, n_in, ld, p = 7, 3, 37, 45, 0.25
    g = torch.Generator().manual_seed(0)
    wide = torch.randn(T, B, ld, generator=g).to(DEV)
    x = wide[:, :, 4:4 + n_in]
    keep = (torch.rand(B, n_in, generator=g) > p).to(torch.uint8).to(DEV)
    xt, kout = mask_x(x, wide, p, keep_in=keep)
    assert torch.equal(kout, keep)
    want = torch.where(keep.bool(), x * (1.0 / (1.0 - p)), torch.zeros_like(x))
    torch.testing.assert_close(xt, want, rtol=1e-6, atol=0)
    xg, kg = mask_x(x, wide, p, seed=5, stream_id=9)
    assert set(kg.unique().tolist()) <= {0, 1} and 0.5 < kg.float().mean().item() < 0.95
    torch.testing.assert_close(xg, torch.where(kg.bool(), x * (1.0 / (1.0 - p)), torch.zeros_like(x)),
                               rtol=1e-6, atol=0)
    assert torch.equal(mask_x(x, wide, p, seed=5, stream_id=9)[1], kg)
    assert not torch.equal(mask_x(x, wide, p, seed=5, stream_id=10)[1], kg)
    slabs = torch.randn(3, T * B, n_in, generator=g).to(DEV)
    dxh = torch.randn(T * B, n_in, generator=g).to(DEV)
    m = (keep.float() / (1 - p)).repeat(T, 1)
    s3 = (slabs[0] + slabs[1]) + slabs[2]
    torch.testing.assert_close(fold_dx(slabs, keep, p, dxh, B), s3 * m + dxh, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(fold_dx(slabs, None, 0.0, dxh, B), s3 + dxh, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(fold_dx(slabs[:1], keep, p, None, B), slabs[0] * m, rtol=1e-6, atol=1e-7)


def test_sru_entry_point_refusals():
    from pkc import _lib as L
    from sru_kernel import Layer
    lib = L.lib()
    d, T, B = 8, 3, 2
    U = torch.randn(T, B, 2 * d * 3, device=DEV)
    x = torch.randn(T, B, 2 * d, device=DEV)
    wc, bias = torch.randn(4 * d, device=DEV), torch.randn(4 * d, device=DEV)
    lay = Layer(T, B, d, 2, 3, 2 * d)
    lay.forward(U, wc, bias, x, 2 * d)
    lay.backward(torch.randn(T, B, 2 * d, device=DEV))
    for field, value, word in (("k", 2, "k=2"), ("k", 5, "k=5"), ("u", None, "null"),
                               ("weight_c", None, "null"), ("cs", None, "null"), ("x", None, "null x"),
                               ("n_in", 2 * d + 1, "n_in == n_out"), ("ndir", 3, "ndir"),
                               ("act", L.ACT["sigmoid"], "activation"), ("drop_p", 1.0, "drop_p"),
                               ("T", 0, "T=0"), ("ldx", d, "ldx")):
        old = getattr(lay.a, field)
        setattr(lay.a, field, value)
        assert lib.pkc_sru_fwd(C.byref(lay.a), None) == L.PKC_ERR_ARG, field
        assert word in lib.pkc_last_error().decode(), (field, lib.pkc_last_error().decode())
        setattr(lay.a, field, old)
    for field in ("dy", "du", "dxh", "dwc", "dbias", "work"):
        old = getattr(lay.a, field)
        setattr(lay.a, field, None)
        assert lib.pkc_sru_bwd(C.byref(lay.a), None) == L.PKC_ERR_ARG, field
        assert "null" in lib.pkc_last_error().decode()
        setattr(lay.a, field, old)
    lay.a.k, lay.a.n_in = 4, 2 * d                     # k = 4 needs n_in != n_out
    assert lib.pkc_sru_fwd(C.byref(lay.a), None) == L.PKC_ERR_ARG
    assert lib.pkc_sru_mask_x(T, B, 4, None, 4, 0.5, 0, None, 0, None, None, None, None) == L.PKC_ERR_ARG
    assert lib.pkc_sru_dx(T, B, 4, None, 1, 0, None, 0.0, None, None, None) == L.PKC_ERR_ARG
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- engine level
def _engine_setup(optk, bf16=False, train=True, batch=None, **over):
    import pkc.neural_networks as NN
    from pkc import _lib as L
    from pkc.engine import Engine, parse_model
    cfg = SC.make_cfg(optk, **over)
    nets, opts = SC.build(cfg, (NN, NN))
    for n in nets.values():
        n.to(DEV)
        n.train() if train else n.eval()
    lens, end, X, lab = SC.make_data()
    eng = Engine(nets, opts, parse_model(SC.MODEL), {"fea": (0, SC.F)}, ["lab_cd", "lab_mono"],
                 batch=batch or SC.B, max_len=SC.MAX_LEN, seed=1, train=train,
                 prec=L.PREC_BF16 if bf16 else L.PREC_FP32)
    eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), end[-1], end_index=end)
    return cfg, nets, opts, eng, (lens, end, X, lab)


def _posterior_rel(eng, outs):
    post = eng.head_output("o2").cpu()
    ref = outs["o2"].detach().float()
    return (post - ref).abs() / ref.abs().clamp_min(1e-3)


def _check_params(step, nets, onets):
    """Every trained tensor within 1e-3 of its norm (INTEGRATION's plug-in parity bound)."""
    for k in nets:
        ref_sd = onets[k].state_dict()
        for name, v in nets[k].state_dict().items():
            ref = ref_sd[name].double()
            dn = float((v.cpu().double() - ref).norm())       # (the form of tests/test_gpu_plugin.py)
            assert dn <= 1e-3 * float(ref.norm()) + 1e-7, "step %d %s/%s: |d| = %.3g, |ref| = %.3g" % (
                step, k, name, dn, float(ref.norm()))


@pytest.mark.parametrize("optk", ["sgd", "rmsprop"])
def test_engine_vs_restatement(optk):
    """Three training steps (SRU 2 x 32 bidirectional: layer 0 k = 4, layer 1 k = 3 with the
    highway term; both dropouts on, their masks read back from the engine's buffers and fed to the
    restatement), each step from the engine's state."""
    import random
    from flipcheck import resync
    cfg, nets, opts, eng, (lens, end, X, lab) = _engine_setup(optk)
    assert eng.rec_forms() == {"rnn.0": "one-launch scan", "rnn.1": "one-launch scan"}
    assert [sp["k"] for sp in nets["rnn"].layer_specs()] == [4, 3]
    onets, _, oopt = SC.oracle_nets(cfg)
    rng = random.Random(7)
    for step, (inp, T, lefts) in enumerate(SC.CC.batches(lens, end, X, lab)):
        eng.sync_state()
        resync(nets, onets, {k: eng.optimizer_state_dict(k) for k in nets} if step else None, oopt)
        batch = eng.next_seq_batch(rng)
        assert batch[3] == T and list(batch[2]) == lefts
        eng.train_step(batch=batch)
        loss, err = eng.loss_values()
        masks = SC.engine_masks(eng)
        assert sorted(masks) == [(0, "c"), (0, "x"), (1, "c"), (1, "x")]
        assert all(0.4 < m.mean().item() < 1.0 for m in masks.values())
        outs = SC.oracle_step(onets, oopt, inp, T, masks)
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
        np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
        rel = _posterior_rel(eng, outs).max().item()
        print("SRU %s step %d loss %.6f posterior rel err %.3g" % (optk, step, loss, rel))
        assert rel < 1e-4, "step %d posterior rel err %.3g" % (step, rel)
        eng.sync_state()
        _check_params(step, nets, onets)


def test_engine_eval_and_forward_mode():
    """Validation (B = 4) and forward mode (one utterance per batch) apply no dropout."""
    import random
    from oracle import run as OR
    for batch in (4, 1):
        cfg, nets, opts, eng, (lens, end, X, lab) = _engine_setup("sgd", train=False, batch=batch)
        onets, _, oopt = SC.oracle_nets(cfg)
        for k in onets:
            onets[k].load_state_dict({n: v.cpu() for n, v in nets[k].state_dict().items()})
            onets[k].eval()
        if batch == 4:
            inp, T, _ = SC.CC.batches(lens, end, X, lab, steps=1)[0]
            eng.eval_step(batch=eng.next_seq_batch(random.Random(7)))
            B = 4
        else:
            T, B = int(lens[0]), 1
            inp = torch.zeros(T, 1, SC.F + 2)
            inp[:, 0, :SC.F] = torch.from_numpy(X[:T])
            inp[:, 0, SC.F:] = torch.from_numpy(lab[:T].astype(np.float32))
            eng.eval_step()
        with torch.no_grad():
            outs = OR.forward_model(OR.parse_model(SC.MODEL), onets,
                                    {"rnn": True, "head": False, "mono": False}, {"fea": (0, SC.F)},
                                    {"lab_cd": SC.F, "lab_mono": SC.F + 1}, inp, T, B)
        rel = _posterior_rel(eng, outs).max().item()
        assert rel < 1e-4, "batch %d posterior rel err %.3g" % (batch, rel)
        loss, _ = eng.loss_values()
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)


def test_engine_bf16_mode():
    """pkc_prec = bf16: the projection and its dX / dW matmuls on bf16-rounded operands, the
    recurrence fp32 — against the restatement with exactly that rounding (SGD), at the engine
    bounds."""
    import random
    from flipcheck import resync
    from oracle import nets as ON
    cfg, nets, opts, eng, (lens, end, X, lab) = _engine_setup("sgd", bf16=True)
    assert eng.rec_forms() == {"rnn.0": "one-launch scan", "rnn.1": "one-launch scan"}
    onets, _, oopt = SC.oracle_nets(cfg)
    onets["rnn"].proj = lambda x, w: ON._BF16Linear.apply(x, w.t(), None)
    ON.use_bf16_matmuls(onets["head"])
    ON.use_bf16_matmuls(onets["mono"])
    rng = random.Random(7)
    for step, (inp, T, _) in enumerate(SC.CC.batches(lens, end, X, lab)):
        eng.sync_state()
        resync(nets, onets, None, oopt)
        batch = eng.next_seq_batch(rng)
        eng.train_step(batch=batch)
        loss, _ = eng.loss_values()
        outs = SC.oracle_step(onets, oopt, inp, T, SC.engine_masks(eng))
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
        rel = _posterior_rel(eng, outs).max().item()
        print("SRU bf16 step %d posterior rel err %.3g" % (step, rel))
        assert rel < 1e-4, "step %d posterior rel err %.3g" % (step, rel)
        eng.sync_state()
        _check_params(step, nets, onets)


def test_engine_graph_replay_equals_eager():
    """Sequence steps replayed from captured graphs (one per padded length) against the same steps
    issued eagerly, with generated dropout masks: bit-identical losses, posteriors and trained
    parameters."""
    import copy
    import random
    import pkc.neural_networks as NN
    from pkc.engine import Engine, parse_model
    cfg = SC.make_cfg("rmsprop")
    nets0, opts = SC.build(cfg, (NN, NN))
    for n in nets0.values():
        n.to(DEV).train()
    rs = np.random.RandomState(0)
    lens = np.array([5, 7, 12, 9, 6, 9, 8, 9, 12, 12, 10, 5, 7, 9, 9, 6])
    end = np.cumsum(lens)
    X = torch.from_numpy(rs.randn(end[-1], SC.F).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(np.stack([rs.randint(0, 64, end[-1]), rs.randint(0, 8, end[-1])],
                                    1).astype(np.int32)).to(DEV)
    runs = []
    for graphs in (False, True):
        nets = copy.deepcopy(nets0)
        eng = Engine(nets, opts, parse_model(SC.MODEL), {"fea": (0, SC.F)}, ["lab_cd", "lab_mono"],
                     batch=SC.B, max_len=16, seed=1)
        if graphs:
            assert eng.capture()
        eng.bind_chunk(X, lab, end[-1], end_index=end)
        rng = random.Random(7)
        trace = []
        for _ in range(4):
            eng.train_step(batch=eng.next_seq_batch(rng))
            trace.append((eng.loss_values(), eng.head_output("o2").cpu().clone(),
                          {k: v.clone() for k, v in SC.engine_masks(eng).items()}))
        if graphs:
            assert eng.seq_captures == 2 and sorted(eng.seq_graphs) == [9, 12]
        eng.sync_state()
        runs.append((trace, {k: {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
                             for k, m in nets.items()}))
    (te, se), (tg, sg) = runs
    for step, ((le, pe, me), (lg, pg, mg)) in enumerate(zip(te, tg)):
        assert le == lg, (step, le, lg)
        assert torch.equal(pe, pg), step
        assert all(torch.equal(me[k], mg[k]) for k in me), step
    assert not torch.equal(te[0][2][(0, "c")], te[1][2][(0, "c")])      # a new mask every step
    for k in se:
        for n in se[k]:
            assert torch.equal(se[k][n], sg[k][n]), (k, n)


@pytest.mark.parametrize("optk,over", [
    ("rmsprop", dict()),
    ("sgd", dict(sru_has_skip_term="False", sru_use_tanh="False", sru_use_relu="True",
                 sru_bidirectional="False"))])
def test_plugin_trains_like_restatement(optk, over):
    """net(x) of the class under autograd (pkc.plugin) in the reference's own loop — forward_model's
    calls, NLLLoss, loss.backward() and torch.optim, as restated in oracle/run.py — with the two
    softmax heads, 3 steps (T = 9, 13, 6: the second outgrows the first engine) against the
    restatement run by the same loop on the CPU; no dropout (the restatement would draw its own
    masks).  The loop and bounds of tests/test_gpu_plugin.py: posteriors within 1e-4 relative, the
    loss within 1e-4, the parameters after the 3 steps within 1e-3 of their norm.  Then eval mode."""
    import pkc.neural_networks as NN
    from oracle import nets as ON
    from test_gpu_plugin import _run
    cfg = SC.make_cfg(optk, sru_dropout="0.0", sru_rnn_dropout="0.0", **over)
    nets, opts = SC.build(cfg, (NN, NN))
    onets, _ = SC.build(cfg, (R, ON))
    for k in nets:
        onets[k].load_state_dict(nets[k].state_dict())
        nets[k].to(DEV).train()
        onets[k].train()
    rs = np.random.RandomState(1)
    batches = []
    for T in (9, 13, 6):
        x = rs.randn(T, SC.B, SC.F).astype(np.float32)
        lab = np.stack([rs.randint(0, 64, (T, SC.B)), rs.randint(0, 8, (T, SC.B))], 2).astype(np.float32)
        batches.append((torch.from_numpy(np.concatenate([x, lab], 2)), T))
    _run(cfg, nets, onets, opts, {"rnn": True, "head": False, "mono": False}, {"fea": (0, SC.F)},
         {"lab_cd": SC.F, "lab_mono": SC.F + 1}, batches, B=SC.B, out="o2")
    net, ref = nets["rnn"].eval(), onets["rnn"].eval()
    x = torch.from_numpy(rs.randn(7, 3, SC.F).astype(np.float32))
    with torch.no_grad():
        ye, yr = net(x.to(DEV)).cpu(), ref(x)
    assert ye.shape == (7, 3, net.out_dim)
    torch.testing.assert_close(ye, yr, rtol=1e-4, atol=1e-5)      # test_gpu_plugin.py's eval bound


def test_engine_refusals():
    import pkc.neural_networks as NN
    from pkc.engine import Engine, parse_model

    def engine(cfg, model=SC.MODEL, **kw):
        nets, opts = SC.build(cfg, (NN, NN))
        for n in nets.values():
            n.to(DEV).train()
        return Engine(nets, opts, parse_model(model), {"fea": (0, SC.F)}, ["lab_cd", "lab_mono"],
                      batch=SC.B, max_len=SC.MAX_LEN, seed=1, **kw)

    gl = SC.MODEL.replace("loss_final=sum(lc,lmw)", "lt=sum(lc,lmw)\nloss_gl=cost_gl(o2,0.01,4)\n"
                          "loss_final=sum(lt,loss_gl)")
    with pytest.raises(NotImplementedError, match="cost_gl over the SRU architecture rnn"):
        engine(SC.make_cfg(), gl)
    with pytest.raises(NotImplementedError, match="mse on the output of rnn"):
        engine(SC.make_cfg(sru_hidden_size="10"),
               SC.MODEL.replace("loss_final=sum(lc,lmw)", "lt=sum(lc,lmw)\nlm2=mse(o1,fea)\n"
                                "loss_final=sum(lt,lm2)"))

    class World:            # sync_bn: no BatchNorm in this class, accepted and ignored
        world = 2
    assert engine(SC.make_cfg(), sync_bn=World()).rec_forms()["rnn.0"] == "one-launch scan"
    with pytest.raises(NotImplementedError, match="sru_layer_norm"):
        engine(SC.make_cfg(sru_layer_norm="True"))
    with pytest.raises(ValueError, match="sru_dropout = 1.0 is outside"):
        engine(SC.make_cfg(sru_dropout="1.0"))
    with pytest.raises(NotImplementedError, match="key sru_quant"):
        engine(SC.make_cfg(sru_quant="True"))


def test_run_nn_lifecycle(tmp_path):
    """pkc.core.run_nn with arch_class = SRU on a tiny synthetic chunk: train -> .info and .pkl files
    under the state-dict names, resume from the .pkl, valid, forward -> the posterior ark, which
    matches the restatement's log-posteriors (loaded from the .pkl with strict=True) to 1e-4."""
    import configparser
    from oracle import loader as OL
    from oracle import nets as ON
    from pkc.core import run_nn
    from test_gpu_run_nn import chunk_cfg, write_data
    d = str(tmp_path)
    scp, ali = write_data(d, 0, n_utt=8)
    counts = os.path.join(d, "counts")
    with open(counts, "w") as f:
        f.write("[ " + " ".join(str(i + 3) for i in range(64)) + " ]\n")
    a1 = dict(arch_library="pkc.neural_networks", arch_class="SRU", arch_seq_model="True",
              arch_name="MLP_layers1", arch_freeze="False", arch_lr="0.0016", arch_opt="rmsprop",
              opt_momentum="0.0", opt_alpha="0.95", opt_eps="1e-8", opt_centered="False",
              opt_weight_decay="0.0", **dict(SC.SRU_OPTS, sru_hidden_size="24"))

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
    ref = R.SRU(a1, 440)
    assert list(ck["model_par"].keys()) == list(ref.state_dict().keys())
    assert list(ck["model_par"])[:4] == ["sru.rnn_lst.0.weight", "sru.rnn_lst.0.weight_c",
                                         "sru.rnn_lst.0.bias", "sru.rnn_lst.1.weight"]
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
    assert not torch.equal(ck["model_par"]["sru.rnn_lst.1.weight_c"],
                           ck1["model_par"]["sru.rnn_lst.1.weight_c"])
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

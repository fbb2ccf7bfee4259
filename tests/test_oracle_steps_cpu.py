"""oracle/steps.py (one recurrent step from a given state, vectorised over t) pinned against the
autograd of oracle.nets' reference loops (liGRU neural_networks.py:1576-1584, LSTM :1087-1092, GRU
:1390-1396, minimalGRU :1751-1755, RNN :1905-1907, each with and without the LayerNorm of h),
which tests/test_oracle_golden.py pins to the reference's own outputs: run sequentially through
its own states, the per-step restatement must reproduce the loop's outputs, its dL/dU, the gradient
of the gate pre-activations, dL/dx and the LayerNorm's dgamma / dbeta.

Then the table of tests/test_gpu_rnn_kernels.py (tests/rnn_kernel.py): that it reaches every
instantiation of the step kernels it claims to (through the host-side mirror of the dispatch), and
that the bound the GPU test holds the kernels to rests on fp32 arithmetic, not on the kernels: the
same restatement evaluated in float32 stays under a quarter of it for every case."""
import configparser

import numpy as np
import pytest
import torch

import rnn_kernel as RK
from cases import GRU_DEF, LIGRU_DEF, LSTM_DEF, MINGRU_DEF, RNN_DEF

# kind -> (oracle.nets class, default options, option prefix, gate letters in pkc's order, act)
KINDS = {"ligru": ("liGRU", LIGRU_DEF, "ligru", "zh", "relu"),
         "lstm": ("LSTM", LSTM_DEF, "lstm", "fioc", "tanh"),
         "gru": ("GRU", GRU_DEF, "gru", "zrh", "tanh"),
         "mingru": ("minimalGRU", MINGRU_DEF, "minimalgru", "zh", "relu"),
         "rnn": ("RNN", RNN_DEF, "rnn", "h", "tanh")}


def _net(kind, bidir, H=12, F=8, ln=False):
    from oracle import nets as ON
    cls, base, p, _, act = KINDS[kind]
    cfg = configparser.ConfigParser()
    # the reference LSTM builds W/U only with BN or LN (:681-791); BN is a separate node upstream of
    # the steps, so its output (wpre) is read back from the forward below
    opt = {p + "_lay": str(H), p + "_drop": "0.3", p + "_bidir": str(bidir), p + "_act": act,
           p + "_use_batchnorm": str(kind == "lstm"), p + "_use_laynorm": str(ln)}
    cfg["a"] = dict(base, **opt)
    net = getattr(ON, cls)(cfg["a"], F).double()
    if ln:
        with torch.no_grad():
            net.ln[0].gamma.copy_(1 + 0.5 * torch.randn(H))
            net.ln[0].beta.copy_(0.5 * torch.randn(H))
    return net


def _f64(fn, *a):
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)      # (the loops' h_init = torch.zeros(...))
    try:
        fn(*a)
    finally:
        torch.set_default_dtype(old)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("bidir", [False, True])
def test_steps_match_reference_loop_autograd(kind, bidir):
    _f64(_check, kind, bidir, False)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("bidir", [False, True])
def test_steps_with_laynorm_match_reference_loop_autograd(kind, bidir):
    _f64(_check, kind, bidir, True)


def _step(S, kind, act, h, c, U, w1, mask):
    """One step of the restatement from (h, c): (gates of the step, r h / z h or None, c', h')."""
    if kind == "ligru":
        z, hcr, hn = S.steps_ligru_fwd(h[None], h[None], U, w1, mask, act)
        return [z[0], hcr[0]], None, c, hn[0]
    if kind == "lstm":
        f, i, o, cc, cn, hn = S.steps_lstm_fwd(h[None], h[None], c[None], U, w1, mask, act)
        return [f[0], i[0], o[0], cc[0]], None, cn[0], hn[0]
    if kind == "gru":
        z, r, rh, hcr, hn = S.steps_gru_fwd(h[None], h[None], U, w1, mask, act)
        return [z[0], r[0], hcr[0]], rh[0], c, hn[0]
    if kind == "mingru":
        z, zh, hcr, hn = S.steps_mingru_fwd(h[None], h[None], U, w1, mask, act)
        return [z[0], hcr[0]], zh[0], c, hn[0]
    hcr, hn = S.steps_rnn_fwd(h[None], h[None], U, w1, mask, act)
    return [hcr[0]], None, c, hn[0]


def _check(kind, bidir, ln):
    from oracle import steps as S
    torch.manual_seed(5)
    H, F, T, B = 12, 8, 7, 3
    _, _, _, letters, act = KINDS[kind]
    G = len(letters)
    net = _net(kind, bidir, H, F, ln)
    net.train()
    R = 2 * B if bidir else B
    mask = (torch.rand(R, H) > 0.3).double()
    x = torch.randn(T, B, F, dtype=torch.float64, requires_grad=True)
    # capture the projections the loop adds (post-BN for the LSTM) with forward hooks
    if kind == "lstm":
        mods = [getattr(net, "bn_w%sx" % g)[0] for g in letters]
        Us = [getattr(net, "u%sh" % g)[0] for g in letters]
    else:
        mods = [getattr(net, "w" + g)[0] for g in letters]
        Us = [getattr(net, "u" + g)[0] for g in letters]
    pre = {}

    def keep(k):
        def hook(m_, i_, o_):
            o_.retain_grad()
            pre[k] = o_
        return hook
    hooks = [m.register_forward_hook(keep(k)) for k, m in enumerate(mods)]
    y = net(x, drop_masks=[mask])
    for h_ in hooks:
        h_.remove()
    dy = torch.randn_like(y)
    (y * dy).sum().backward()
    wpre = [pre[k].detach().reshape(T, R, H) for k in range(G)]
    U = [u.weight.detach() for u in Us]
    lnp = dict(gamma=net.ln[0].gamma.detach(), beta=net.ln[0].beta.detach(), eps=1e-6) if ln else None
    # sequential run of the one-step restatement through its own states
    h = torch.zeros(R, H, dtype=torch.float64)
    c = torch.zeros(R, H, dtype=torch.float64)
    hs, cs, gates, rhs, xh, den, sd = [h], [c], [], [], [], [], []
    for t in range(T):
        g_, rh, c, h = _step(S, kind, act, h, c, U, [w[t:t + 1] for w in wpre], mask)
        if ln:
            xhat, d_, s_, h = S.ln_h_fwd(h, lnp["gamma"], lnp["beta"], lnp["eps"])
            xh.append(xhat), den.append(d_), sd.append(s_)
        gates.append(g_), rhs.append(rh), cs.append(c), hs.append(h)
    hs_t, cst = torch.stack(hs), torch.stack(cs)
    gt = [torch.stack([g_[k] for g_ in gates]) for k in range(G)]
    yp = hs_t[1:]
    yp = torch.cat([yp[:, :B], torch.flip(yp[:, B:], [0])], 2) if bidir else yp
    np.testing.assert_allclose(yp.numpy(), y.detach().numpy(), rtol=1e-12, atol=1e-12)
    dh = S.out_grad_proc_time(dy, B, H, bidir)
    lnb = dict(gamma=lnp["gamma"], xhat=torch.stack(xh), den=torch.stack(den),
               std=torch.stack(sd)) if ln else None
    # the BPTT products read the gate gradients the function itself produces: iterate to the fixed
    # point (a step's gradients depend on step t + 1's through at most two products: 2 T passes
    # make the sequential chain exact)
    dg = [torch.zeros(T, R, H, dtype=torch.float64) for _ in range(G)]
    gp = None
    for _ in range(2 * T + 2):
        if kind == "ligru":
            r_ = S.steps_ligru_bwd(dh, dg, U, gt[0], gt[1], hs_t[:-1], mask, act, ln=lnb)
            dg, gp = [r_[0], r_[1]], (r_[3] if ln else None)
        elif kind == "lstm":
            r_ = S.steps_lstm_bwd(dh, dg, U, gt[0], gt[1], gt[2], gt[3], cst[1:], cst[:-1], mask,
                                  act, ln=lnb)
            dg, gp = r_[:4], (r_[4] if ln else None)
        elif kind == "gru":
            dg, gp = S.steps_gru_bwd(dh, dg, U, gt[0], gt[1], gt[2], hs_t[:-1], mask, act, ln=lnb)
        elif kind == "mingru":
            dg, gp = S.steps_mingru_bwd(dh, dg, U, gt[0], gt[1], hs_t[:-1], mask, act, ln=lnb)
        else:
            dg, gp = S.steps_rnn_bwd(dh, dg, U, gt[0], mask, act, ln=lnb)
    # the gradient of every gate's pre-activation, dL/dU (the candidate of the two-phase cells
    # contracts with r h / z h)
    for q, u in enumerate(Us):
        np.testing.assert_allclose(dg[q].numpy(), pre[q].grad.reshape(T, R, H).numpy(),
                                   rtol=1e-10, atol=1e-12)
        src = torch.stack(rhs) if kind in ("gru", "mingru") and q == G - 1 else hs_t[:-1]
        np.testing.assert_allclose(S.weight_grad(dg[q], src).numpy(), u.weight.grad.numpy(),
                                   rtol=1e-10, atol=1e-12)
    # dL/dx through the projections (Linear, with a bias unless LayerNorm; the LSTM's go through
    # BatchNorm, whose input gradient the pre-activation check above stands for)
    if kind != "lstm":
        W = [m.weight.detach() for m in mods]
        dx = sum(S.pre_grad_input_time(dg[q], B, bidir) @ W[q] for q in range(G))
        np.testing.assert_allclose(dx.numpy(), x.grad.numpy(), rtol=1e-10, atol=1e-12)
    if ln:
        _, dgam, dbet = S.ln_h_bwd(gp, lnp["gamma"], lnb["xhat"], lnb["den"], lnb["std"])
        np.testing.assert_allclose(dgam.numpy(), net.ln[0].gamma.grad.numpy(), rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(dbet.numpy(), net.ln[0].beta.grad.numpy(), rtol=1e-10, atol=1e-12)


def test_ln_h_bwd_is_autograd_of_ln_h_fwd_and_masks_zero_std():
    from oracle import steps as S
    torch.manual_seed(11)
    h = torch.randn(4, 3, 9, dtype=torch.float64, requires_grad=True)
    gam = torch.randn(9, dtype=torch.float64, requires_grad=True)
    bet = torch.randn(9, dtype=torch.float64, requires_grad=True)
    xhat, den, sd, y = S.ln_h_fwd(h, gam, bet, 1e-6)
    g = torch.randn_like(y)
    (y * g).sum().backward()
    dh, dgam, dbet = S.ln_h_bwd(g, gam.detach(), xhat.detach(), den.detach(), sd.detach())
    np.testing.assert_allclose(dh.numpy(), h.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(dgam.numpy(), gam.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(dbet.numpy(), bet.grad.numpy(), rtol=1e-10, atol=1e-12)
    # a zero row: std = 0, xhat = 0, and the backward keeps only (gh - mean gh) / eps
    z = torch.zeros(2, 9, dtype=torch.float64)
    xhat, den, sd, y = S.ln_h_fwd(z, gam.detach(), bet.detach(), 1e-6)
    assert float(sd.abs().max()) == 0 and float(xhat.abs().max()) == 0
    assert torch.equal(y, bet.detach().expand(2, 9))
    g = torch.randn(2, 9, dtype=torch.float64)
    dh, _, _ = S.ln_h_bwd(g, gam.detach(), xhat, den, sd)
    gh = g * gam.detach()
    assert bool(torch.isfinite(dh).all())
    np.testing.assert_allclose(dh.numpy(), ((gh - gh.mean(-1, keepdim=True)) / 1e-6).numpy(),
                               rtol=1e-12)


# ----------------------------------------------------------------- the GPU test's table and bound
def test_fp32_table_reaches_every_step_instantiation():
    """tests/test_gpu_rnn_kernels.py's per-step table, through the host-side mirror of the dispatch:
    every (cell, strip width, row-tiling class), every (cell, strip width, load width), B2 = 16, 17
    and 32 per cell, both activations per cell (the LSTM: tanh), T = 1 and T = 2, dy in slabs."""
    cases = RK.fp32_cases()
    assert len({c.id for c in cases}) == len(cases) and len({c.seed for c in cases}) == len(cases)
    for cell in RK.CELLS:
        mine = [c for c in cases if c.cell == cell]
        forms = [RK.step_form(cell, c.H, c.B2) for c in mine]
        tiling = {(f[0], RK.row_class(c.B2)) for f, c in zip(forms, mine) if c.T == 3}
        loads = {(f[0], f[4]) for f, c in zip(forms, mine) if c.T == 3}
        for S in (16, 32, 48, 64, 128):
            for rc in ("16-row", "one 32-row tile", "two tiles"):
                assert (S, rc) in tiling, (cell, S, rc)
            for vw in (1, 2, 4):
                assert (S, vw) in loads, (cell, S, vw)
        assert {16, 17, 32} <= {c.B2 for c in mine}, cell
        assert {c.act for c in mine} == ({"tanh"} if cell == "lstm" else {"relu", "tanh"}), cell
        assert {1, 2, 3} == {c.T for c in mine} and any(c.nslab == 3 for c in mine), cell
        # the dense one-phase cells' 8-wave tiles and the two-phase cells' 4-wave tiles
        assert {f[1] for f in forms} == ({4} if cell in ("gru", "mingru") else {4, 8}), cell
    # both edges of every strip class's H range, and the H range's own
    Hs = {c.H for c in cases}
    assert {5, 256, 257, 512, 513, 768, 769, 1024, 1025, 2048} <= Hs
    assert RK.step_form("lstm", 2048, 34) == (128, 8, 32, 2, 4)
    assert RK.step_form("gru", 5, 6) == (16, 4, 16, 1, 1)
    assert RK.step_form("rnn", 510, 17, bf16=True) == (32, 8, 32, 1, "h2")
    bf = {(RK.step_form(c.cell, c.H, c.B2, bf16=True)[4], RK.row_class(c.B2), c.cell)
          for c in RK.bf16_cases()}
    for cell in ("ligru", "lstm", "rnn"):
        for load in ("h8", "h2", "h1"):
            for rc in ("16-row", "one 32-row tile", "two tiles"):
                assert (load, rc, cell) in bf
    assert len(RK.ln_cases()) == 5 * 5 * 3 and len(RK.grid_cases()) == 4 + 3 + 3


GAP_BOUND = 2e-5 / 4       # a quarter of tests/test_gpu_rnn_kernels.py's bound


def _gap(c, ln):
    """max over the restated tensors of |float32 restatement - float64 restatement| / max|float64|,
    both from the same float64 states of the case."""
    inp = RK.make_inputs(c, ln)
    s, lnp = RK.simulate(c, inp, ln)
    ref = RK.restate(c.cell, c.act, s, lnp)
    f32 = torch.float32
    lo = RK.restate(c.cell, c.act, RK.cast_state(s, f32),
                    {k: (v.to(f32) if torch.is_tensor(v) else v) for k, v in lnp.items()} if ln else None)
    worst = ("", 0.0)
    for (name, _, r64), (_, _, r32) in zip(ref, lo):
        scale = float(r64.abs().max())
        err = float((r32.double() - r64).abs().max()) / max(scale, 1e-30)
        assert np.isfinite(err), (c.id, name)
        if err > worst[1]:
            worst = (name, err)
    return worst


@pytest.mark.parametrize("cell", list(RK.CELLS))
def test_float32_restatement_gap_is_a_quarter_of_the_gpu_bound(cell):
    """The GPU test's 2e-5 is about 40x fp32 rounding: the float32 evaluation of each step of every
    table case (per-step table and LayerNorm table) stays under a quarter of it."""
    worst = ("", "", 0.0)
    for ln, cases in ((False, RK.fp32_cases()), (True, RK.ln_cases())):
        for c in cases:
            if c.cell != cell:
                continue
            name, err = _gap(c, ln)
            assert err <= GAP_BOUND, "%s%s %s: float32 gap %.3g" % (c.id, " LN" if ln else "", name, err)
            if err > worst[2]:
                worst = (c.id + (" LN" if ln else ""), name, err)
    print("%s: largest float32-vs-float64 gap %.3g (%s, %s)" % (cell, worst[2], worst[0], worst[1]))

"""pkc_rnn_fwd / pkc_rnn_bwd through the C ABI (tests/rnn_kernel.py) against the float64 step
oracle (oracle/steps.py): every instantiation fwd_impl_s / bwd_impl_s select — five cells x strip
width S = 16 / 32 / 48 / 64 / 128 x 16-row, one 32-row and two row tiles x load width 4 / 2 / 1 —
at the smallest shapes that reach it, then the LayerNorm of h, the bf16 step products, the
grid-synchronised loops in the default environment, the dropout mask and the check() refusals.

Each tensor is compared with the restatement of that ONE step from the run's own saved hs / cs /
gates / dgates, so nothing compounds and a ReLU kink cannot flip.  Bound: max|got - ref| / max|ref|
<= 2e-5 per tensor, no outliers — the bound tests/test_gpu_steps.py holds these kernels to, about 40x
fp32 rounding; tests/test_oracle_steps_cpu.py shows the float32 evaluation of the same restatement
under a quarter of it for every case of the tables here, so it does not rest on the kernels.  The
per-tensor maxima of a run are printed (pytest -s; profiles/rnn_kernels_pytest_gpu.txt: the largest
measured on an MI355X were 7.8e-7 for the fp32 steps, 1.3e-6 with LayerNorm, 3.2e-7 for the bf16
steps against their bf16 operands and 2.2e-7 for the grid-synchronised loops)."""
import ctypes as C

import pytest
import torch

import rnn_kernel as RK

pytestmark = pytest.mark.gpu
TOL = 2e-5


def _ids(cases):
    return [c.id for c in cases]


def _state(lay, c, inp, bf16, ln, mask):
    """The run's saved tensors as restate() reads them (float64, CPU)."""
    f64 = torch.float64
    s = dict(hs=lay.get("hs", True), gates=lay.get("gates", True), dgates=lay.get("dgates", True))
    if c.cell == "lstm":
        s["cs"] = lay.get("cs", True)
    if c.cell in ("gru", "mingru"):
        s["rh"] = lay.get("rh", True)
    if ln:
        for k in ("ln_xhat", "ln_stat", "ln_g", "ln_dgamma", "ln_dbeta"):
            s[k] = lay.get(k, True)
    s = {k: v.to(f64) for k, v in s.items()}
    U = inp["U"]
    if bf16:
        s["hA"], s["dgA"] = lay.get("hs_h", True).to(f64), lay.get("dgates_h", True).to(f64)
        s["UA"] = [U[g].to(torch.bfloat16).to(f64) for g in range(lay.G)]
    else:
        s["hA"], s["dgA"], s["UA"] = s["hs"], s["dgates"], [U[g].to(f64) for g in range(lay.G)]
    s["wproc"], _ = RK.proc_inputs(c, inp)
    # dL/dh from the output: the float64 sum of the dy slabs
    from oracle import steps as S
    s["dh_y"] = S.out_grad_proc_time(lay.dy_parts.to(f64).sum(0), c.B, c.H, c.bidir)
    s["mask"] = mask.to(f64)
    return s


def _compare(tag, items, report):
    for name, got, ref in items:
        assert bool(torch.isfinite(got).all()), "%s %s: not finite" % (tag, name)
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max()) / max(scale, 1e-30)
        report.append("%s %.2e" % (name, err))
    print("%s: max|diff| / max|ref|: %s" % (tag, "; ".join(report)))
    for name, got, ref in items:
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max()) / max(scale, 1e-30)
        assert err <= TOL, "%s %s: max|diff| / max|ref| = %.3g (> %.1g)" % (tag, name, err, TOL)


def _exact_checks(lay, c, inp, bf16, injected=True):
    B = c.B
    hs, y = lay.get("hs", True), lay.get("y", True)
    assert bool((hs[0] == 0).all()), "hs[0] is not zero"
    if c.cell == "lstm":
        assert bool((lay.get("cs", True)[0] == 0).all()), "cs[0] is not zero"
    yref = torch.cat([hs[1:, :B], torch.flip(hs[1:, B:], [0])], 2) if c.bidir else hs[1:]
    assert torch.equal(y, yref), "y is not the hidden states under the output mapping"
    if injected:
        assert torch.equal(lay.get("drop_mask", True), inp["mask"]), "drop_mask != injected mask"
    dg, dpre = lay.get("dgates", True), lay.get("dpre", True)
    fold = dg[:, :, :B] + torch.flip(dg[:, :, B:], [1]) if c.bidir else dg
    assert torch.equal(dpre, fold), "dpre is not the one fp32 add of the directions' dgates"
    assert torch.equal(lay.get("ut", True), inp["U"].transpose(1, 2)), "ut != U^T"
    if bf16:
        bf = torch.bfloat16
        assert torch.equal(lay.get("hs_h", True), hs.to(bf)), "hs_h != RNE(hs)"
        assert torch.equal(lay.get("dgates_h", True), dg.to(bf)), "dgates_h != RNE(dgates)"
        assert torch.equal(lay.get("ut_h", True), inp["U"].transpose(1, 2).to(bf)), "ut_h != RNE(U^T)"


def _run(c, ln=False, bf16=False, form=0, inp=None, mask="inject", **tables):
    """Forward + backward of one case, every check of the module docstring; returns the layer.
    form: the expected pkc_rnn_persist_form, one number or a (forward, BPTT) pair; tables: the
    Layer's umask / kmaps / plans; mask "gen": the library's own dropout mask."""
    inp = RK.make_inputs(c, ln) if inp is None else inp
    lay = RK.Layer(c.cell, c.T, c.B, c.H, c.bidir, c.act, inp, ln=ln, bf16=bf16, nslab=c.nslab,
                   slab_seed=c.seed, mask=mask, **tables)
    forms = (form, form) if isinstance(form, int) else tuple(form)
    assert (lay.form(0), lay.form(1)) == forms, \
        "pkc_rnn_persist_form %d / %d, expected %d / %d" % ((lay.form(0), lay.form(1)) + forms)
    lay.forward()
    lay.backward()
    n4 = 4 * c.B2 * c.H
    if 2 in forms:
        word = lay.get("work").reshape(-1)[n4 + 1:n4 + 2].view(torch.int32)
        assert int(word[0]) == 0, "a grid-synchronised loop timed out"
    _exact_checks(lay, c, inp, bf16, injected=mask == "inject")
    drop = inp["mask"] if mask == "inject" else lay.get("drop_mask", True)
    s = _state(lay, c, inp, bf16, ln, drop)
    lnp = dict(gamma=inp["gamma"].double(), beta=inp["beta"].double(), eps=1e-6) if ln else None
    tag = c.id + (" LN" if ln else "") + (" bf16" if bf16 else "") + (" grid" if 2 in forms else "")
    _compare(tag, RK.restate(c.cell, c.act, s, lnp), [])
    lay.check_guards()
    first = lay.snapshot()
    lay.forward()
    lay.backward()
    second = lay.snapshot()
    for k, v in first.items():
        assert torch.equal(v, second[k]), "%s: the rerun's %s is not bit-identical" % (tag, k)
    lay.check_guards()
    return lay, s


@pytest.fixture
def per_step(monkeypatch):
    monkeypatch.setenv("PKC_RNN_LIGRU_GRID", "0")
    monkeypatch.setenv("PKC_RNN_LSTM_PERSIST", "0")


@pytest.mark.parametrize("c", RK.fp32_cases(), ids=_ids(RK.fp32_cases()))
def test_per_step_fp32(c, per_step):
    _run(c)


@pytest.mark.parametrize("c", RK.ln_cases(), ids=_ids(RK.ln_cases()))
def test_layernorm_of_h(c, per_step):
    _run(c, ln=True)


def test_layernorm_of_h_zero_row(per_step):
    """A batch row whose wpre is zero for the first two steps: relu liGRU, h_0 = 0.5 * 0 + 0.5 *
    relu(0) = 0 for the whole row, std = 0.  xhat = 0, h = beta, everything finite, and the
    backward takes the masked form (the unmasked 0 / 0 would be a NaN in dgates)."""
    c = RK.make_case("ligru", 3, 65, 6, "relu", seed=29001)
    inp = RK.make_inputs(c, True)
    inp["wpre"][:, :2, 0] = 0
    lay, s = _run(c, ln=True, inp=inp)
    assert float(s["ln_stat"][0, 0, 1]) == 0 and float(s["ln_stat"][0, 0, 0]) == pytest.approx(1e-6)
    assert bool((s["ln_xhat"][0, 0] == 0).all())
    assert torch.equal(s["hs"][1, 0].float(), inp["beta"])
    assert bool((s["dgates"][:, 0, 0] == 0).all())
    for k in ("hs", "gates", "y", "dgates", "dpre", "ln_g", "ln_dgamma", "ln_dbeta", "ln_xhat"):
        assert bool(torch.isfinite(lay.get(k)).all()), k


@pytest.mark.parametrize("c", RK.bf16_cases(), ids=_ids(RK.bf16_cases()))
def test_bf16_step_products(c, per_step):
    _run(c, bf16=True)


@pytest.mark.parametrize("c,bf16", RK.grid_cases(),
                         ids=[c.id + ("-bf16" if b else "") for c, b in RK.grid_cases()])
def test_grid_synchronised_loops(c, bf16):
    """Default environment: the library must take form 2 for these shapes (a 0 is a failure, not a
    reason to pick another shape)."""
    _run(c, bf16=bf16, form=2)


# ------------------------------------------------------------------------------------- dropout
def test_generated_mask(per_step):
    c = RK.make_case("rnn", 2, 256, 16, "tanh", seed=50001)        # B2 * H = 4096
    inp = RK.make_inputs(c)

    def mask_of(step, seed=1234, stream_id=77):
        lay = RK.Layer(c.cell, c.T, c.B, c.H, c.bidir, c.act, inp, mask="gen", step=step,
                       seed=seed, stream_id=stream_id)
        lay.forward()
        lay.backward()
        lay.check_guards()
        return lay, lay.get("drop_mask", True)
    lay, m = mask_of(3)
    assert bool(((m == 0) | (m == 1)).all())
    assert abs(float(m.mean()) - 0.8) <= 0.05, float(m.mean())
    assert torch.equal(mask_of(3)[1], m), "not repeated at the same step_ctr / seed / stream_id"
    assert not torch.equal(mask_of(4)[1], m), "the same mask at step_ctr + 1"
    assert not torch.equal(mask_of(3, seed=1235)[1], m) and not torch.equal(
        mask_of(3, stream_id=78)[1], m)
    # and the steps use it
    _exact_checks(lay, c, inp, False, injected=False)
    _compare(c.id + " generated mask", RK.restate(c.cell, c.act, _state(lay, c, inp, False, False, m)), [])


@pytest.mark.parametrize("cell", list(RK.CELLS))
def test_eval_dropout_is_the_keep_rate(cell, per_step):
    """train = 0, drop_p = 0.2: m = 1 - p everywhere, no mask drawn."""
    c = RK.make_case(cell, 3, 65, 6, "relu", seed=51000 + RK.CELLS[cell][0])
    inp = RK.make_inputs(c)
    lay = RK.Layer(c.cell, c.T, c.B, c.H, c.bidir, c.act, inp, train=False)
    assert lay.form(0) == 0 and lay.form(1) == 0
    lay.forward()
    lay.backward()
    lay.bufs["drop_mask"].untouched()
    _exact_checks(lay, c, inp, False, injected=False)
    keep = (torch.tensor(1.0) - torch.tensor(0.2)).double() * torch.ones(c.B2, c.H, dtype=torch.float64)
    _compare(c.id + " eval", RK.restate(c.cell, c.act, _state(lay, c, inp, False, False, keep)), [])
    lay.check_guards()


# ------------------------------------------------------------------------------------ refusals
def _small(cell, **kw):
    c = RK.make_case(cell, 2, 24, 6, "tanh", seed=60000)
    return RK.Layer(c.cell, c.T, c.B, c.H, c.bidir, c.act, RK.make_inputs(c, kw.get("ln", False)), **kw)


def _set(**fields):
    def f(lay):
        for k, v in fields.items():
            setattr(lay.a, k, v)
    return f


def _null_gate(name, g):
    def f(lay):
        getattr(lay.a, name)[g] = None
    return f


def _kmap(field, width):
    def f(lay):
        lay.kmap = torch.zeros(4096, dtype=torch.int32, device=RK.DEV)
        setattr(lay.a, field, lay.kmap.data_ptr())
        lay.a.kmap_s_fwd, lay.a.kmap_s_bwd = 16, 16
        setattr(lay.a, field.replace("kmap_", "kmap_s_"), width)
    return f


# (id, cell, Layer options, mutation, entry point, word of pkc_last_error())
REFUSALS = [
    ("H0", "ligru", {}, _set(H=0), "pkc_rnn_fwd", "bad shape"),
    ("H2049", "ligru", {}, _set(H=2049), "pkc_rnn_fwd", "bad shape"),
    ("T0", "ligru", {}, _set(T=0), "pkc_rnn_fwd", "bad shape"),
    ("bad_cell", "ligru", {}, _set(cell=5), "pkc_rnn_fwd", "bad cell"),
    ("gru_no_rh", "gru", {}, _set(rh=None), "pkc_rnn_fwd", "need rh"),
    ("mingru_no_rh_bwd", "mingru", {}, _set(rh=None), "pkc_rnn_bwd", "need rh"),
    ("qbits_ligru", "ligru", {}, _set(qbits=8), "pkc_rnn_fwd", "only for LSTM"),
    ("null_wpre", "rnn", {}, _set(wpre=None), "pkc_rnn_fwd", "null buffer"),
    ("lstm_no_cs", "lstm", {}, _set(cs=None), "pkc_rnn_fwd", "needs cs"),
    ("null_U", "lstm", {}, _null_gate("U", 3), "pkc_rnn_fwd", "null U[3]"),
    ("dropout_no_mask", "ligru", {}, _set(drop_mask=None), "pkc_rnn_fwd", "needs drop_mask"),
    ("bwd_no_ut", "lstm", {}, _set(ut=None), "pkc_rnn_bwd", "null buffer"),
    ("ln_no_stat", "rnn", {"ln": True}, _set(ln_stat=None), "pkc_rnn_fwd", "LayerNorm needs"),
    ("ln_bwd_no_g", "gru", {"ln": True}, _set(ln_g=None), "pkc_rnn_bwd", "LayerNorm needs"),
    ("lstm_qbits_no_hq", "lstm", {}, _set(qbits=8), "pkc_rnn_fwd", "quantised h needs"),
    ("bf16_gru", "gru", {}, _set(step_bf16=1), "pkc_rnn_fwd", "bf16 steps only"),
    ("bf16_ln", "ligru", {"ln": True}, _set(step_bf16=1), "pkc_rnn_fwd", "bf16 steps only"),
    ("bf16_no_hs_h", "ligru", {"bf16": True}, _set(hs_h=None), "pkc_rnn_fwd", "need hs_h"),
    ("bf16_no_U_h", "lstm", {"bf16": True}, _null_gate("U_h", 2), "pkc_rnn_fwd", "need U_h[2]"),
    ("bf16_bwd_no_dgates_h", "rnn", {"bf16": True}, _set(dgates_h=None), "pkc_rnn_bwd",
     "need ut_h, dgates_h"),
    ("qh_exact_no_qbits", "lstm", {}, _set(qh_exact=1), "pkc_rnn_fwd", "qh_exact needs"),
    ("kmap_s_fwd_24", "ligru", {}, _kmap("kmap_fwd", 24), "pkc_rnn_fwd", "kmap_s_fwd 24"),
    ("kmap_s_bwd_24", "gru", {}, _kmap("kmap_bwd", 24), "pkc_rnn_bwd", "kmap_s_bwd 24"),
    ("kmap_rnn_bf16", "rnn", {"bf16": True}, _kmap("kmap_fwd", 16), "pkc_rnn_fwd",
     "fp32 step products only"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(case):
    from pkc import _lib as L
    _, cell, opts, mutate, entry, word = case
    lay = _small(cell, **opts)
    mutate(lay)
    rc = lay.raw(entry)
    assert rc < 0, "%s accepted bad arguments" % entry
    msg = L.lib().pkc_last_error().decode()
    assert word in msg and "pkc_rnn" in msg, msg
    for b in lay.bufs.values():
        b.untouched()


def test_refusal_null_dpre():
    from pkc import _lib as L
    lay = _small("ligru")
    rc = L.lib().pkc_rnn_bwd(C.byref(lay.a), None, None)
    assert rc < 0
    assert "null dpre" in L.lib().pkc_last_error().decode()
    for b in lay.bufs.values():
        b.untouched()

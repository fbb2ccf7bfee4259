"""The SincNet architecture end to end on the GPU: the plug-in forward / backward against the
recorded reference runs (tests/golden/sinc.npz), and Engine training steps against
tests/sinc_ref.py + the oracle MLP + torch.optim on the CPU.  The mirror of test_gpu_cnn.py.

Tolerances are that file's: posteriors 1e-4 relative, loss 1e-4, parameters after the steps within
1e-3 of their norm, and the same precondition on the pooling windows (top-two gap above 1e-5 of the
window's largest magnitude, asserted on the CPU reference at the fixed seed).

The gradients of low_hz_ / band_hz_ are cancelling sums of cosines at arguments up to ~200 rad
divided by a maximum as small as 0.008, so the reference's own fp32 values sit 1e-7 .. 1e-5
(relative L2) from the exact ones.  They are bounded by that distance: the relative L2 to the
reference's fp32 value may be at most 4 x the relative L2 of that fp32 value to the fp64
restatement, computed in the test."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cnn_ref  # noqa: E402
import sinc_ref  # noqa: E402
from cases import LSTM_DEF, MLP_DEF  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = np.load(os.path.join(HERE, "golden", "sinc.npz"))
CASES = json.loads(str(G["cases"]))
INPS = json.loads(str(G["inp_dims"]))
INP = 64
SINC = ("conv.0.low_hz_", "conv.0.band_hz_")

SGD = dict(arch_lr="0.05", arch_opt="sgd", opt_momentum="0.0", opt_weight_decay="0.0",
           opt_dampening="0.0", opt_nesterov="False", arch_freeze="False")
# The sinc vectors' gradients are large for a loss taken on the filters' output (1e2 .. 7e3 at init
# under the golden's (y * r).sum()) while low_hz_ starts at 0.002.  Behind a normalisation and a
# mean NLL they are ~3e-3 here, so the head's rate also keeps every low_hz_ / band_hz_ positive over
# the steps, and moves them by ~1e-4; both are asserted (on the CPU reference, resp. after the steps)
SINC_LR = "0.05"
MODEL = ("out1=compute(sinc,fea)\nout2=compute(head,out1)\nloss_final=cost_nll(out2,lab)\n"
         "err_final=cost_err(out2,lab)")


def _golden_sd(name):
    keys = json.loads(str(G[name + "/keys"]))
    return {k: torch.from_numpy(G["%s/sd/%s" % (name, k)].copy()) for k in keys}


def _rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _sinc_rule(got, ref32, ref64, what):
    """got within 4 x (the fp32 reference's own relative L2 to fp64) of the fp32 reference."""
    own, d = _rel(ref32, ref64), _rel(got, ref32)
    print("%s: rel L2 to the fp32 reference %.3g; that reference's own to fp64 %.3g" % (what, d, own))
    assert d <= 4 * own, "%s: rel L2 %.3g > 4 x %.3g" % (what, d, own)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plugin_forward_backward_golden(name):
    """net(x) and .backward() of pkc.neural_networks.SincNet loaded from each golden case.  Bound:
    1e-4 of each tensor's largest magnitude for y, dx and the conv / norm parameters (as
    test_gpu_cnn.py), the module docstring's rule for low_hz_ / band_hz_."""
    from pkc.neural_networks import SincNet
    opts, inp = CASES[name], INPS[name]
    net = SincNet(opts, inp)
    net.load_state_dict(_golden_sd(name))
    net.to(DEV).train()
    x = torch.from_numpy(G[name + "/x"].copy()).to(DEV).requires_grad_(True)
    r = torch.from_numpy(G[name + "/r"]).to(DEV)
    y = net(x)
    assert tuple(y.shape) == (x.shape[0], net.out_dim)
    (y * r).sum().backward()

    def close(got, want, what, scale=0.0):
        want = torch.from_numpy(np.asarray(want)).double()
        err = (got.detach().cpu().double() - want).abs().max().item()
        assert err <= 1e-4 * max(want.abs().max().item(), scale, 1e-6), "%s: %.3g" % (what, err)

    # the filters the forward generated: the engine-owned W of layer 0
    filt = net._pkc_runner.eng.nodes[-len(net.conv)].cW.cpu().view(G[name + "/filters"].shape)
    close(filt, G[name + "/filters"], "filters")
    close(y, G[name + "/y"], "y")
    close(x.grad, G[name + "/dx"], "dx")
    # the fp64 restatement of the same run, for the sinc vectors' rule
    sd64 = sinc_ref.leaf_state(_golden_sd(name), torch.float64)
    y64 = sinc_ref.sincnet_forward(sd64, opts, torch.from_numpy(G[name + "/x"]).double(), train=True)
    (y64 * torch.from_numpy(G[name + "/r"]).double()).sum().backward()
    for k, p in net.named_parameters():
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        want = G["%s/grad/%s" % (name, k)]
        if k in SINC:
            _sinc_rule(g.cpu(), want, sd64[k].grad, "%s %s" % (name, k))
            v = G["%s/sd/%s" % (name, k)]
            assert bool((g.cpu().numpy()[v == 0] == 0).all()), "%s: gradient at an exact 0" % k
            continue
        # a conv bias in front of a normalisation cancels: measured on its weight gradient's scale
        scale = 0.0
        if k.startswith("conv.") and k.endswith("bias"):
            i = int(k.split(".")[1])
            if (cnn_ref.strtobool(opts["sinc_use_laynorm"].split(",")[i]) or
                    cnn_ref.strtobool(opts["sinc_use_batchnorm"].split(",")[i])):
                scale = float(np.abs(G["%s/grad/%s" % (name, k.replace("bias", "weight"))]).max())
        close(g, want, k, scale)
    for k, v in net.state_dict().items():
        if "running_" in k:
            torch.testing.assert_close(v.cpu(), torch.from_numpy(G["%s/after/%s" % (name, k)]),
                                       rtol=1e-4, atol=1e-6)
        if "num_batches" in k:
            assert int(v.item()) == int(G["%s/after/%s" % (name, k)]), k
    # eval forward: running statistics, no state kept
    net.eval()
    ref = sinc_ref.RefSincNet(opts, inp)
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    ref.eval()
    with torch.no_grad():
        ye, yr = net(x.detach()), ref(x.detach().cpu())
    close(ye, yr.numpy(), "eval y")


def _sinc_opts(kind, drop="0.0,0.0", lr=SINC_LR):
    o = dict(CASES["none"], sinc_drop=drop, arch_name="sinc", **dict(SGD, arch_lr=lr))
    if kind == "ln":
        o.update(sinc_use_laynorm="True,True", sinc_use_laynorm_inp="True")
    elif kind == "bn":
        o.update(sinc_use_batchnorm="True,True", sinc_use_batchnorm_inp="True")
    return o


def _head_opts(out="20", lay="32,"):
    n = len((lay + out).split(","))
    return dict(MLP_DEF, arch_name="head", dnn_lay=lay + out,
                dnn_act=",".join(["relu"] * (n - 1) + ["softmax"]), dnn_drop=",".join(["0.0"] * n),
                dnn_use_batchnorm=",".join(["False"] * n), dnn_use_laynorm=",".join(["False"] * n),
                **SGD)


def _build(sopts, hopts, inp, seed=3, dev=DEV):
    from oracle import nets as ON
    from pkc.neural_networks import MLP, SincNet
    torch.manual_seed(seed)
    np.random.seed(seed)
    nets = {"sinc": SincNet(sopts, inp)}
    nets["head"] = MLP(hopts, nets["sinc"].out_dim)
    onets = {"sinc": sinc_ref.RefSincNet(sopts, inp), "head": ON.MLP(hopts, nets["sinc"].out_dim)}
    for k in nets:
        onets[k].load_state_dict(nets[k].state_dict())
        nets[k].to(dev).train()
        onets[k].train()
    return nets, onets, {"sinc": sopts, "head": hopts}


def _compare_state(nets, onets, tol=1e-3):
    for k in nets:
        for name, v in nets[k].state_dict().items():
            ref = onets[k].state_dict()[name]
            if name.endswith("num_batches_tracked"):
                assert int(v.item()) == int(ref.item()), (k, name)
                continue
            d = (v.cpu().double() - ref.double()).norm().item()
            assert d <= tol * ref.double().norm().item() + 1e-7, "%s %s %.3g" % (k, name, d)


def _sinc_stays_positive(onets):
    c = onets["sinc"].conv[0]
    assert bool((c.low_hz_ > 0).all()) and bool((c.band_hz_ > 0).all()), \
        "the step moved a low_hz_ / band_hz_ entry across 0: lower SINC_LR"


def _steps_case(kind, dev=DEV):
    """Nets, data and injected masks of test_engine_three_sgd_steps."""
    B, steps, nout, p = 16, 3, 20, 0.15
    sopts = _sinc_opts("ln" if kind == "drop" else kind, "%g,%g" % (p, p) if kind == "drop"
                       else "0.0,0.0")
    nets, onets, opts = _build(sopts, _head_opts(str(nout)), INP, dev=dev)
    rs = np.random.RandomState(8)
    X = rs.randn(B * steps, INP).astype(np.float32)
    lab = rs.randint(0, nout, size=(B * steps, 1)).astype(np.int32)
    masks = None
    if kind == "drop":
        geo = sinc_ref.geometry(sopts, INP)
        masks = [torch.from_numpy((rs.rand(B, g[1], g[5]) >= p).astype(np.uint8)) for g in geo]
    return B, steps, nets, onets, opts, X, lab, masks


def _reference_steps(B, steps, onets, opts, X, lab, masks, model=MODEL, inp_dim=INP):
    from oracle import nets as ON
    from oracle import run as OR
    onets["sinc"].keep, onets["sinc"].gaps = masks, []
    oopt = {k: ON.make_optimizer(onets[k].parameters(), opts[k]) for k in onets}
    inp = torch.from_numpy(np.concatenate([X, lab.astype(np.float32)], 1))
    refs = [OR.train_step(OR.parse_model(model), onets, oopt, {k: False for k in onets},
                          {"fea": (0, inp_dim)}, {"lab": inp_dim}, inp[s * B:(s + 1) * B])
            for s in range(steps)]
    # the preconditions, on the CPU reference: unambiguous pooling routes in every step, and the
    # sinc vectors on the positive side of |.|
    worst = min(float(g.min()) for g in onets["sinc"].gaps)
    assert worst > 1e-5, "seed gives a near-tie (gap %.3g): pick another" % worst
    _sinc_stays_positive(onets)
    return refs


@pytest.mark.parametrize("kind", ["ln", "bn", "drop"])
def test_engine_three_sgd_steps(kind):
    from pkc.engine import Engine, parse_model
    B, steps, nets, onets, opts, X, lab, masks = _steps_case(kind)
    keep_in = {}
    if masks is not None:
        keep_in = {"sinc.conv%d" % i: m.reshape(B, -1).contiguous().to(DEV)
                   for i, m in enumerate(masks)}
    eng = Engine(nets, opts, parse_model(MODEL), {"fea": (0, INP)}, ["lab"], batch=B,
                 drop_keep_in=keep_in)
    eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), B * steps)
    head = [l for l in eng.layers if l.arch == "head"][-1]
    got = []
    for s in range(steps):
        eng.train_step()
        got.append((eng.loss_values()[0], head.out.view(B, -1).cpu().clone()))
    refs = _reference_steps(B, steps, onets, opts, X, lab, masks)
    for s in range(steps):
        loss, post = got[s]
        ref = refs[s]["out2"].detach()
        rel = ((post - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
        assert rel < 1e-4, "step %d posterior rel err %.3g" % (s, rel)
        np.testing.assert_allclose(loss, refs[s]["loss_final"].item(), rtol=1e-4)
    eng.sync_state()
    _compare_state(nets, onets)
    # the sinc vectors did move, and by the reference's amount: 1e-3 of the movement's norm would
    # ask more than fp32 holds (the parameters are ~1e3 x the movement), 1e-2 does not
    init = sinc_ref.mel_init(10, 16000, 50, 50)
    for k, p0 in zip(SINC, init):
        mv_ref = onets["sinc"].state_dict()[k] - p0
        mv = nets["sinc"].state_dict()[k].cpu() - p0
        assert mv_ref.abs().max().item() > 0
        assert _rel(mv, mv_ref) <= 1e-2, "%s movement rel L2 %.3g" % (k, _rel(mv, mv_ref))


def test_capture_replays_to_the_same_weights():
    """Engine.capture() with a SincNet: graph replays and eager steps end at bit-identical weights
    and filters, so the filter regeneration is inside the graph (stale filters from the capture
    would give other outputs, gradients and weights from the second step on)."""
    from pkc.engine import Engine, parse_model
    B, steps = 16, 4
    rs = np.random.RandomState(2)
    X = torch.from_numpy(rs.randn(B * steps, INP).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(rs.randint(0, 20, size=(B * steps, 1)).astype(np.int32)).to(DEV)
    out, filt = [], []
    for graph in (False, True):
        nets, _, opts = _build(_sinc_opts("bn"), _head_opts(), INP)
        eng = Engine(nets, opts, parse_model(MODEL), {"fea": (0, INP)}, ["lab"], batch=B)
        eng.bind_chunk(X, lab, B * steps)
        node = [n for n in eng.nodes if getattr(n, "sinc", None) is not None][0]
        if graph:
            assert eng.capture(steps_per_graph=2)
            first = node.cW.detach().cpu().clone()     # the filters of the initial parameters
        eng.train_steps(steps)
        torch.cuda.synchronize()
        out.append({k + "." + n: v.detach().cpu().clone() for k in nets
                    for n, v in nets[k].state_dict().items()})
        filt.append(node.cW.detach().cpu().clone())
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
    assert torch.equal(filt[0], filt[1])
    assert not torch.equal(filt[1], first), "the filters never changed: the steps did not move them"


def test_plugin_smaller_batch_after_larger():
    """The plug-in's engine is built for the first row count (130) and then runs a smaller one
    (128): the buffers sized at 130 rows serve it, and the gradients are the reference's."""
    from pkc.neural_networks import SincNet
    opts = CASES["ln"]
    net = SincNet(opts, INP)
    net.load_state_dict(_golden_sd("ln"))
    net.to(DEV).train()
    ref = sinc_ref.RefSincNet(opts, INP)
    ref.load_state_dict(_golden_sd("ln"))
    ref.train()
    ref64 = sinc_ref.RefSincNet(opts, INP, dtype=torch.float64)
    ref64.load_state_dict(_golden_sd("ln"))
    ref64.train()
    rs = np.random.RandomState(9)
    for rows in (130, 128):
        x = torch.from_numpy(rs.randn(rows, INP).astype(np.float32))
        r = torch.from_numpy(rs.randn(rows, net.out_dim).astype(np.float32))
        for m in (net, ref, ref64):
            m.zero_grad()
        xg = x.to(DEV).requires_grad_(True)
        (net(xg) * r.to(DEV)).sum().backward()
        xr = x.clone().requires_grad_(True)
        (ref(xr) * r).sum().backward()
        (ref64(x.double()) * r.double()).sum().backward()
        assert net._pkc_runner.eng.Mmax == 130
        refp, refp64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
        for k, p in list(net.named_parameters()) + [("x", xg)]:
            want = (xr if k == "x" else refp[k]).grad
            if want is None:
                continue
            if k in SINC:
                _sinc_rule(p.grad.cpu(), want, refp64[k].grad, "rows %d %s" % (rows, k))
                continue
            scale = want.abs().max().item()
            if k.startswith("conv.") and k.endswith("bias"):       # cancelled by the LayerNorm
                scale = max(scale, refp[k.replace("bias", "weight")].grad.abs().max().item())
            err = (p.grad.cpu() - want).abs().max().item()
            assert err <= 1e-4 * max(scale, 1e-6), "rows %d %s: %.3g" % (rows, k, err)


def test_bf16_step_uses_the_bf16_copy_of_the_conv_output():
    """pkc_prec = bf16: the filters and the conv products stay exact fp32; the consumer matmul reads
    the bf16 copy of the last conv node's output.  One step against the fp32 run from the same
    weights, with test_gpu_cnn.py's bounds (2^-7 of the largest log-posterior; 2^-5 of the flat
    gradient's norm)."""
    from pkc import _lib as L
    from pkc.engine import Engine, parse_model
    B = 16
    rs = np.random.RandomState(6)
    X = torch.from_numpy(rs.randn(B, INP).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(rs.randint(0, 20, size=(B, 1)).astype(np.int32)).to(DEV)
    res = {}
    for prec in (L.PREC_FP32, L.PREC_BF16):
        nets, _, opts = _build(_sinc_opts("ln"), _head_opts(), INP)
        eng = Engine(nets, opts, parse_model(MODEL), {"fea": (0, INP)}, ["lab"], batch=B, prec=prec)
        conv = [n for n in eng.nodes if getattr(n, "conv", False)]
        assert conv[0].sinc is not None and conv[1].sinc is None
        if prec == L.PREC_BF16:
            assert eng.h16 and conv[-1].out_h is not None and conv[0].out_h is None
        eng.bind_chunk(X, lab, B)
        eng.train_step()
        head = [l for l in eng.layers if l.arch == "head"][-1]
        res[prec] = (eng.loss_values()[0], head.out.view(B, -1).cpu().clone(),
                     conv[-1].out[:B * conv[-1].N].cpu().clone(),
                     None if conv[-1].out_h is None else conv[-1].out_h[:B * conv[-1].N].cpu().clone(),
                     eng.gflat.cpu().clone(), conv[0].cW.cpu().clone())
    (l0, p0, c0, _, g0, f0), (l1, p1, c1, h1, g1, f1) = res[L.PREC_FP32], res[L.PREC_BF16]
    assert torch.equal(f0, f1), "filters differ between fp32 and bf16 mode"
    assert torch.equal(c0, c1), "conv output differs between fp32 and bf16 mode"
    assert torch.equal(h1.float(), c1.bfloat16().float())
    tol = 2.0 ** -7 * p0.abs().max().item()
    assert (p0 - p1).abs().max().item() <= tol
    assert abs(l0 - l1) <= tol
    assert bool(torch.isfinite(g1).all())
    assert (g0.double() - g1.double()).norm().item() <= 2.0 ** -5 * g0.double().norm().item()


def test_sincnet_into_lstm_over_padded_rows():
    """SincNet(40: 6,4; len 5,3; pool 2,1; BatchNorm) -> LSTM 1 x 16 -> softmax head through the
    Engine, 2 SGD steps: the SincNet runs over the T * B rows, padding included
    (utils.py:1905-1930); its output gradient is the LSTM's layer-0 dX slabs.  A padded (all-zero)
    row convolves to exact zeros in layer 0 (no bias): an exact tie, routed to the first index by
    both sides."""
    import random
    from oracle import nets as ON
    from oracle import run as OR
    from pkc.engine import Engine, parse_model
    from pkc.neural_networks import LSTM, MLP, SincNet
    F_, B, nout = 40, 4, 12
    sopts = dict(_sinc_opts("none"), sinc_N_filt="6,4", sinc_len_filt="5,3", sinc_max_pool_len="2,1",
                 sinc_use_batchnorm="True,True")
    ropts = dict(LSTM_DEF, arch_name="rnn", lstm_lay="16", lstm_drop="0.0", lstm_bidir="False",
                 lstm_use_batchnorm="True", lstm_use_laynorm="False", lstm_act="tanh", **SGD)
    hopts = _head_opts(str(nout), "")
    model = ("o0=compute(sinc,fea)\no1=compute(rnn,o0)\no2=compute(head,o1)\n"
             "loss_final=cost_nll(o2,lab)\nerr_final=cost_err(o2,lab)")
    torch.manual_seed(3)
    np.random.seed(3)
    nets = {"sinc": SincNet(sopts, F_)}
    nets["rnn"] = LSTM(ropts, nets["sinc"].out_dim)
    nets["head"] = MLP(hopts, nets["rnn"].out_dim)
    onets = {"sinc": sinc_ref.RefSincNet(sopts, F_), "rnn": ON.LSTM(ropts, nets["sinc"].out_dim),
             "head": ON.MLP(hopts, nets["rnn"].out_dim)}
    opts = {"sinc": sopts, "rnn": ropts, "head": hopts}
    for k in nets:
        onets[k].load_state_dict(nets[k].state_dict())
        nets[k].to(DEV).train()
        onets[k].train()
    rs = np.random.RandomState(0)
    lens = np.sort(rs.randint(5, 13, size=8))             # unequal sentence lengths, T <= 12
    end = np.cumsum(lens)
    X = rs.randn(end[-1], F_).astype(np.float32)
    lab = rs.randint(0, nout, size=(end[-1], 1)).astype(np.int32)
    eng = Engine(nets, opts, parse_model(model), {"fea": (0, F_)}, ["lab"], batch=B, max_len=16,
                 seed=1)
    eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), end[-1], end_index=end)
    oopt = {k: ON.make_optimizer(onets[k].parameters(), opts[k]) for k in onets}
    lines = OR.parse_model(model)
    rng_e, rng_o = random.Random(7), random.Random(7)
    snt = 0
    for step in range(2):
        batch = eng.next_seq_batch(rng_e)
        begs, blens, lefts, T = batch
        inp = torch.zeros(T, B, F_ + 1)                    # batch assembly as core.py:183-200
        real = torch.zeros(T, B, dtype=torch.bool)
        for k in range(B):
            n = int(lens[snt])
            left = rng_o.randint(0, T - n)
            b0 = int(end[snt] - n)
            inp[left:left + n, k, :F_] = torch.from_numpy(X[b0:b0 + n])
            inp[left:left + n, k, F_:] = torch.from_numpy(lab[b0:b0 + n].astype(np.float32))
            assert left == lefts[k]
            real[left:left + n, k] = True
            snt += 1
        onets["sinc"].gaps = []
        outs = OR.train_step(lines, onets, oopt, {"sinc": False, "rnn": True, "head": False},
                             {"fea": (0, F_)}, {"lab": F_}, inp, T, B)
        worst = min(float(g[real.reshape(-1)].min()) for g in onets["sinc"].gaps)
        assert worst > 1e-5, "seed gives a near-tie (gap %.3g): pick another" % worst
        _sinc_stays_positive(onets)
        eng.train_step(batch=batch)
        loss, err = eng.loss_values()
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
        post, ref = eng.head_output("o2").cpu(), outs["o2"].detach()
        rel = ((post.reshape(ref.shape) - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
        assert rel < 1e-4, "step %d posterior rel err %.3g" % (step, rel)
    eng.sync_state()
    _compare_state(nets, onets)


L2_MODEL = ("out1=compute(sinc,fea)\nout2=compute(head,out1)\nloss_nll=cost_nll(out2,lab)\n"
            "loss_l2=cost_l2(out2,0.05)\nloss_final=sum(loss_nll,loss_l2)\n"
            "err_final=cost_err(out2,lab)")


def test_cost_l2_includes_the_sinc_vectors():
    """cost_l2 sums the 2-norms of every parameter with dim > 1 (utils.py:29-39): low_hz_ and
    band_hz_ are (N, 1), so they are in it.  One step with and without the term from the same
    weights: the loss is the reference's, and the term's gradient 0.05 p / |p| arrives in both
    vectors' gradients (read as the difference of the two runs' gradients, to the fp32 rounding of
    forming and adding the term)."""
    from oracle import run as OR
    from pkc.engine import Engine, parse_model
    B = 16
    rs = np.random.RandomState(5)
    X = rs.randn(B, INP).astype(np.float32)
    lab = rs.randint(0, 20, size=(B, 1)).astype(np.int32)
    grads = {}
    for model in (MODEL, L2_MODEL):
        sopts = dict(_sinc_opts("ln"), skip_regularization="False")
        nets, onets, opts = _build(sopts, _head_opts(), INP)
        eng = Engine(nets, opts, parse_model(model), {"fea": (0, INP)}, ["lab"], batch=B)
        eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), B)
        p0 = {k: v.detach().cpu().clone() for k, v in nets["sinc"].named_parameters()}
        eng.train_step()
        names = {id(p): k for k, p in nets["sinc"].named_parameters()}
        grads[model] = {names[id(p)]: g.detach().cpu().clone() for p, g in eng.param_grads
                        if id(p) in names}
        loss = eng.loss_values()[0]
        outs = OR.forward_model(OR.parse_model(model), onets, {k: False for k in onets},
                                {"fea": (0, INP)}, {"lab": INP},
                                torch.from_numpy(np.concatenate([X, lab.astype(np.float32)], 1)))
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
        if model is L2_MODEL:
            term = outs["loss_l2"].item()
            want = 0.05 * sum(p.norm().item() for n_ in onets.values() for p in n_.parameters()
                              if p.dim() > 1 and not n_.skip_regularization)
            np.testing.assert_allclose(term, want, rtol=1e-5)
            assert 0.05 * (p0[SINC[0]].norm() + p0[SINC[1]].norm()).item() > 1e-3 * abs(loss), \
                "the sinc vectors' share of the loss is below the comparison's resolution"
    for k in SINC:
        g0, g1 = grads[MODEL][k].double(), grads[L2_MODEL][k].double()
        want = 0.05 * p0[k].double() / p0[k].double().norm()
        # the term p lam / |p| is formed in fp32 (a norm, a division, a product: 8 ulp of the term
        # at most) and added to the gradient in fp32 (half an ulp of the sum)
        tol = 2.0 ** -24 * (g1.abs() + 8 * want.abs())
        assert bool(((g1 - g0 - want).abs() <= tol).all()), k
        assert bool((want.abs() > 4 * tol).any()), "%s: the term is below the rounding" % k


def test_cost_gl_over_a_sincnet_is_refused():
    from pkc.engine import Engine, parse_model
    model = ("out1=compute(sinc,fea)\nout2=compute(head,out1)\nloss_nll=cost_nll(out2,lab)\n"
             "loss_gl=cost_gl(out2,0.02,3)\nloss_final=sum(loss_nll,loss_gl)\n"
             "err_final=cost_err(out2,lab)")
    for sopts in (dict(_sinc_opts("ln"), skip_regularization="False"),
                  # one layer: no 3-D parameter at all, still a convolution architecture
                  dict(_sinc_opts("none"), sinc_N_filt="10", sinc_len_filt="17",
                       sinc_max_pool_len="2", sinc_use_laynorm="False", sinc_use_batchnorm="False",
                       sinc_act="relu", sinc_drop="0.0", skip_regularization="False")):
        nets, _, opts = _build(sopts, _head_opts(), INP)
        with pytest.raises(NotImplementedError, match="cost_gl"):
            Engine(nets, opts, parse_model(model), {"fea": (0, INP)}, ["lab"], batch=16)


def test_full_geometry_small_batch_step():
    """The TIMIT_SincNet_raw body (3200 -> 128/60/60/60 filters, len 128 (129 taps)/5/5/3, pool
    3/3/3/2, LayerNorm on the input and every layer, relu) + MLP at B = 16, one RMSprop step
    against the restatement on the CPU: the only place where K = 129, two channel tiles and ~49
    position tiles meet.  Bounds as test_gpu_cnn.py::test_full_size_fbank_step: posteriors 1e-4
    relative; conv / norm parameter gradients within 1e-4 of their norm (relative L2); the conv
    biases in front of a LayerNorm zero within the fp32 bound of their sum, on both sides.  The two
    sinc vectors: the module docstring's rule, the fp64 restatement run here.  (Measured: pkc sits
    2.9e-6 / 4.4e-6 from the fp32 reference.  That reference's own distance to fp64 is 7.4e-3 at
    this seed, on ln.2.beta and every gradient below it but not on ln.2.gamma: what one of layer
    2's 108 k relu inputs at a rounding-level 0, gating differently in fp64, would give.)"""
    from oracle import nets as ON
    from oracle import run as OR
    from pkc.engine import Engine, parse_model
    B, F_, nout = 16, 3200, 48
    rms = dict(arch_opt="rmsprop", opt_momentum="0.0", opt_alpha="0.95", opt_eps="1e-8",
               opt_centered="False", opt_weight_decay="0.0", arch_freeze="False")
    sopts = dict(sinc_N_filt="128,60,60,60", sinc_len_filt="128,5,5,3", sinc_max_pool_len="3,3,3,2",
                 sinc_use_laynorm_inp="True", sinc_use_batchnorm_inp="False",
                 sinc_use_laynorm="True,True,True,True",
                 sinc_use_batchnorm="False,False,False,False", sinc_act="relu,relu,relu,relu",
                 sinc_drop="0.0,0.0,0.0,0.0", sinc_sample_rate="16000", sinc_min_low_hz="50",
                 sinc_min_band_hz="50", arch_name="sinc", arch_lr="0.0008", **rms)
    hopts = dict(_head_opts(str(nout), "256,"), arch_lr="0.0004", **rms)
    nets, onets, opts = _build(sopts, hopts, F_)
    assert nets["sinc"].out_dim == 55 * 60 and nets["sinc"].conv_specs()[0]["len"] == 129
    onets64 = {k: copy.deepcopy(v).double() for k, v in onets.items()}
    rs = np.random.RandomState(4)
    X = rs.randn(B, F_).astype(np.float32)
    lab = rs.randint(0, nout, size=(B, 1)).astype(np.int32)
    eng = Engine(nets, opts, parse_model(MODEL), {"fea": (0, F_)}, ["lab"], batch=B)
    eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), B)
    eng.train_step()
    head = [l for l in eng.layers if l.arch == "head"][-1]
    post = head.out.view(B, -1).cpu()
    grads = {id(p): g.detach().cpu().clone() for p, g in eng.param_grads}
    inp = torch.from_numpy(np.concatenate([X, lab.astype(np.float32)], 1))
    lines = OR.parse_model(MODEL)
    seq = {k: False for k in onets}
    oopt = {k: ON.make_optimizer(onets[k].parameters(), opts[k]) for k in onets}
    outs = OR.train_step(lines, onets, oopt, seq, {"fea": (0, F_)}, {"lab": F_}, inp)
    outs64 = OR.forward_model(lines, onets64, seq, {"fea": (0, F_)}, {"lab": F_}, inp.double())
    outs64["loss_final"].backward()
    ref = outs["out2"].detach()
    rel = ((post - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
    assert rel < 1e-4, "posterior rel err %.3g" % rel
    convs = [n for n in eng.nodes if getattr(n, "conv", False)]
    for k in nets:
        refp, refp64 = dict(onets[k].named_parameters()), dict(onets64[k].named_parameters())
        for name, p in nets[k].named_parameters():
            if id(p) not in grads:
                continue                      # the unused norm holders receive no gradient
            rg = refp[name].grad
            if k == "sinc" and name in SINC:
                _sinc_rule(grads[id(p)], rg, refp64[name].grad, name)
                continue
            if k == "sinc" and name.startswith("conv.") and name.endswith(".bias"):
                nd = convs[int(name.split(".")[1])]
                dz = nd.dz[:B * nd.N].view(B, nd.C_out, nd.L_out).abs().double().sum((0, 2)).cpu()
                bound = 2 * (B * nd.L_out + 2) * 2.0 ** -24 * dz
                for what, v in (("pkc", grads[id(p)]), ("reference", rg)):
                    assert bool((v.double().abs() <= bound).all()), "%s %s not ~0" % (what, name)
                continue
            d = (grads[id(p)].double() - rg.double()).norm().item()
            assert d <= 1e-4 * rg.double().norm().item(), "%s.%s grad rel L2 %.3g" % (
                k, name, d / max(rg.double().norm().item(), 1e-30))
    eng.sync_state()
    _compare_state(nets, onets)


def _write_raw(d, n_utt, dim):
    """A `raw` feature stream: dim samples per frame, plus the two alignments of chunk_cfg."""
    from pkc import data_io as D
    rs = np.random.RandomState(0)
    ark, scp = os.path.join(d, "raw.ark"), os.path.join(d, "raw.scp")
    ali = os.path.join(d, "ali")
    os.makedirs(ali, exist_ok=True)
    with open(scp, "w") as f:
        for i in range(n_utt):
            k = "spk0_u%03d" % i
            T = rs.randint(30, 90)
            D.write_mat_path(ark, rs.randn(T, dim).astype(np.float32), k, append=i > 0)
            D.write_vec_int_path(os.path.join(ali, "ali_pdf.ark"), rs.randint(0, 64, T), k, append=i > 0)
            D.write_vec_int_path(os.path.join(ali, "ali_phones.ark"), rs.randint(1, 9, T), k,
                                 append=i > 0)
            f.write("%s %s\n" % (k, ark))
    return scp, ali


def test_run_nn_sincnet_train_and_forward(tmp_path):
    """run_nn end to end with arch_class = SincNet over a `raw` stream (fea_opts empty, no context
    window, as TIMIT_SincNet_raw.cfg): train one chunk, reload the .pkl files into the restatement,
    forward-mode the posterior ark; the ark equals the posteriors of sinc_ref + the oracle MLP
    loaded from those .pkl files."""
    import configparser
    from oracle import loader as OL
    from oracle import nets as ON
    from pkc.core import run_nn
    from test_gpu_run_nn import chunk_cfg
    d = str(tmp_path)
    scp, ali = _write_raw(d, 6, INP)
    counts = os.path.join(d, "counts")
    with open(counts, "w") as f:
        f.write("[ " + " ".join(str(i + 3) for i in range(64)) + " ]\n")
    sinc = dict(CASES["none"], arch_library="pkc.neural_networks", arch_class="SincNet",
                arch_name="MLP_layers1", arch_pretrain_file="none", arch_seq_model="False",
                sinc_use_laynorm_inp="True", sinc_use_laynorm="True,False",
                sinc_use_batchnorm="False,True", sinc_act="relu,leaky_relu", sinc_drop="0.15,0.0",
                **dict(SGD, arch_lr=SINC_LR))

    def make(name, to_do, pre=None, counts=None):
        path = chunk_cfg(d, name, to_do, scp, ali, counts=counts)
        cfg = configparser.ConfigParser()
        cfg.read(path)
        cfg["architecture1"] = dict(sinc)
        cfg["data_chunk"]["fea"] = "fea_name=raw\nfea_lst=%s\nfea_opts=\ncw_left=0\ncw_right=0\n" % scp
        cfg["model"]["model"] = cfg["model"]["model"].replace("fmllr", "raw")
        for i in (1, 2, 3):
            if pre:
                cfg["architecture%d" % i]["arch_pretrain_file"] = os.path.join(
                    d, "%s_architecture%d.pkl" % (pre, i))
        with open(path, "w") as f:
            cfg.write(f)
        return path, cfg

    c_tr, _ = make("train_ck0", "train")
    run_nn(None, None, None, None, None, None, c_tr, True, c_tr)
    info = configparser.ConfigParser()
    info.read(os.path.join(d, "train_ck0.info"))
    assert 0 < float(info["results"]["loss"]) < 20
    c_fw, cfg = make("forward", "forward", pre="train_ck0", counts=counts)
    data, _, _ = run_nn(None, None, None, None, None, None, c_fw, True, c_fw)
    with open(os.path.join(d, "forward_out_dnn2_to_decode.ark"), "rb") as f:
        mats = dict(OL.parse_mat_ark(f.read()))
    names, chunk, end = data[0], data[1], np.asarray(data[2])
    assert len(mats) == 6
    feats = chunk.feats.cpu()
    inp = feats.shape[1]
    assert inp == INP
    ref_c = sinc_ref.RefSincNet(cfg["architecture1"], inp)
    ref_h = ON.MLP(dict(MLP_DEF, **cfg["architecture2"]), ref_c.out_dim)
    for net, i in ((ref_c, 1), (ref_h, 2)):
        ck = torch.load(os.path.join(d, "train_ck0_architecture%d.pkl" % i), weights_only=True,
                        map_location="cpu")
        net.load_state_dict(ck["model_par"])           # strict: the reference's keys
        net.eval()
    init = sinc_ref.mel_init(10, 16000, 50, 50)
    assert not torch.equal(ref_c.conv[0].low_hz_.detach(), init[0]), "low_hz_ was not trained"
    assert not torch.equal(ref_c.conv[0].band_hz_.detach(), init[1]), "band_hz_ was not trained"
    c = np.arange(3, 67, dtype=np.float64)
    prior = torch.from_numpy(np.log(c / c.sum()).astype(np.float32))
    beg = 0
    # as test_gpu_cnn.py: the relative error is taken on the network's log-posterior (ark + log
    # prior) and the ark itself is held to 1e-4 of that magnitude
    for name, e in zip(names, end):
        with torch.no_grad():
            ref = ref_h(ref_c(feats[beg:e])).double()
        ark = torch.from_numpy(np.array(mats[name])).double()
        got = ark + prior.double()
        rel = ((got - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
        assert rel < 1e-4, "%s log-posterior rel err %.3g" % (name, rel)
        assert float((ark - (ref - prior.double())).abs().max()) <= 1e-4 * float(ref.abs().max())
        beg = e

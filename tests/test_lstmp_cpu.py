"""The projected LSTM (LSTM_cudnn with proj_size = P: torch.nn.LSTM(..., proj_size=P)) without a GPU:
the class's parameters against torch.nn.LSTM's, the plain-torch restatement (tests/lstmp_ref.py)
against the golden torch.nn.LSTM wrote (tests/golden/lstmp.npz) and a live torch.nn.LSTM, the ctypes
layout of pkc_lstmp_args against the header, the class's refusals, and the RMSprop cap of the engine
case (tests/lstmp_cases.py)."""
import copy
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

G = np.load(os.path.join(GOLDEN, "lstmp.npz"))
CASES = json.loads(str(G["cases"]))
INP = int(G["inp_dim"])


def _torch_lstm(o, inp=INP):
    return torch.nn.LSTM(inp, int(o["hidden_size"]), num_layers=int(o["num_layers"]),
                         bias=o["bias"] == "True", dropout=0.0,
                         bidirectional=o["bidirectional"] == "True",
                         proj_size=int(o.get("proj_size", 0)))


def test_golden_cases_are_the_issues():
    got = {n: (int(c["opts"]["hidden_size"]), int(c["opts"]["proj_size"]),
               int(c["opts"]["num_layers"]), c["opts"]["bidirectional"], c["opts"]["bias"], c["B"],
               c["T"]) for n, c in CASES.items()}
    assert got == {"lstmp_a": (20, 8, 1, "False", "True", 5, 6),
                   "lstmp_b": (20, 8, 2, "True", "True", 5, 6),
                   "lstmp_c": (48, 20, 2, "True", "True", 17, 6),
                   "lstmp_d": (20, 8, 1, "True", "False", 5, 6)}
    # case (c) alone holds 40 320 parameters: their float32 values and gradients are 315 KiB that
    # do not compress, so the four cases take about 500 KiB; the limit of a committed file is 1 MiB
    assert os.path.getsize(os.path.join(GOLDEN, "lstmp.npz")) < 1024 * 1024


@pytest.mark.parametrize("name", sorted(CASES))
def test_pkc_state_dict_is_torchs(name):
    """Under the same seed the class's state dict equals nn.LSTM(proj_size)'s bit for bit, keys in
    the same order (under lstm.0.), and loads strictly both ways."""
    import pkc.neural_networks as NN
    c = CASES[name]
    o = c["opts"]
    torch.manual_seed(int(G["seed"]))
    net = NN.LSTM_cudnn(o, INP)
    torch.manual_seed(int(G["seed"]))
    tm = _torch_lstm(o)
    sd, tsd = net.state_dict(), tm.state_dict()
    keys = json.loads(str(G[name + "/keys"]))
    assert list(sd.keys()) == ["lstm.0." + k for k in tsd.keys()] == keys
    assert any(k.startswith("lstm.0.weight_hr_l0") for k in keys)
    for k, v in tsd.items():
        assert sd["lstm.0." + k].shape == v.shape and torch.equal(sd["lstm.0." + k], v), k
        assert np.array_equal(v.numpy(), G["%s/sd/lstm.0.%s" % (name, k)]), k
    H, P = int(o["hidden_size"]), int(o["proj_size"])
    nd = 2 if o["bidirectional"] == "True" else 1
    assert tuple(sd["lstm.0.weight_hh_l0"].shape) == (4 * H, P)
    assert tuple(sd["lstm.0.weight_hr_l0"].shape) == (P, H)
    if int(o["num_layers"]) > 1:
        assert tuple(sd["lstm.0.weight_ih_l1"].shape) == (4 * H, nd * P)
    assert net.out_dim == nd * P == int(G[name + "/out_dim"])
    tm.load_state_dict({k[len("lstm.0."):]: v + 1 for k, v in sd.items()}, strict=True)
    net.load_state_dict({"lstm.0." + k: v for k, v in tm.state_dict().items()}, strict=True)
    assert all(torch.equal(net.state_dict()["lstm.0." + k], v) for k, v in tm.state_dict().items())
    specs = net.layer_specs()
    assert all(sp["P"] == P and len(sp["Whr"]) == nd for sp in specs)
    assert specs[0]["Whr"][0] is net.lstm[0].weight_hr_l0
    net.check_supported()


def test_proj_size_zero_is_todays_class():
    """proj_size = 0 (and the key left out) keeps the parameters, the state dict, the draws and
    out_dim of the plain LSTM_cudnn."""
    import pkc.neural_networks as NN
    o = dict(hidden_size="20", num_layers="2", bias="True", batch_first="False", dropout="0.0",
             bidirectional="True")
    sds = []
    for opts in (o, dict(o, proj_size="0")):
        torch.manual_seed(3)
        net = NN.LSTM_cudnn(opts, INP)
        assert net.out_dim == 40 and net.proj_size == 0
        assert all("P" not in sp and "Whr" not in sp for sp in net.layer_specs())
        sds.append(net.state_dict())
    torch.manual_seed(3)
    tsd = _torch_lstm(o).state_dict()
    for sd in sds:
        assert list(sd.keys()) == ["lstm.0." + k for k in tsd.keys()]
        assert not any("weight_hr" in k for k in sd)
        assert all(torch.equal(sd["lstm.0." + k], v) for k, v in tsd.items())
    for cls in (NN.GRU_cudnn, NN.RNN_cudnn):
        assert cls(dict(o, proj_size="0", nonlinearity="tanh"), INP).out_dim == 40


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_vs_golden_and_torch(name):
    """The restatement against the golden and a live torch.nn.LSTM(proj_size) at the CPU bounds of
    tests/test_cudnn_cpu.py: outputs (train and eval) rtol 1e-5 / atol 1e-6, dL/dx and every
    gradient (weight_hr included) rtol 4e-4 / atol 4e-6."""
    import lstmp_ref as R
    c = CASES[name]
    torch.manual_seed(int(G["seed"]))
    net = R.LSTM_cudnn(c["opts"], INP)
    keys = json.loads(str(G[name + "/keys"]))
    assert list(net.state_dict().keys()) == keys
    for k in keys:                      # the restatement's own draws are torch's too
        assert np.array_equal(net.state_dict()[k].numpy(), G["%s/sd/%s" % (name, k)]), k
    net.load_state_dict({k: torch.from_numpy(G["%s/sd/%s" % (name, k)]) for k in keys}, strict=True)
    tm = R.torch_module(net)
    r = torch.from_numpy(G[name + "/r"])
    got = {}
    for tag, mod in (("restatement", net), ("torch", lambda x: tm(x)[0])):
        x = torch.from_numpy(G[name + "/x"]).requires_grad_(True)
        net.train(), tm.train()
        y = mod(x)
        (y * r).sum().backward()
        ps = list((net if tag == "restatement" else tm).parameters())
        got[tag] = (y.detach(), x.grad.clone(), [p.grad.clone() for p in ps])
        for p in ps:
            p.grad = None
    y, dx, gr = got["restatement"]
    assert len(gr) == len(keys)
    for ref_y, ref_dx, ref_g in ((torch.from_numpy(G[name + "/y"]), torch.from_numpy(G[name + "/dx"]),
                                  [torch.from_numpy(G["%s/grad/%s" % (name, k)]) for k in keys]),
                                 got["torch"]):
        torch.testing.assert_close(y, ref_y, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(dx, ref_dx, rtol=4e-4, atol=4e-6)
        for k, a, b in zip(keys, gr, ref_g):
            torch.testing.assert_close(a, b, rtol=4e-4, atol=4e-6, msg=lambda m, k=k: k + ": " + m)
    net.eval()
    with torch.no_grad():
        ye = net(torch.from_numpy(G[name + "/x"]))
    torch.testing.assert_close(ye, torch.from_numpy(G[name + "/y_eval"]), rtol=1e-5, atol=1e-6)


def test_restatement_dropout_is_between_layers():
    """Training with dropout > 0 multiplies each layer's 2P-wide output below the last by its keep
    mask / (1 - p); the last layer has no mask; eval applies none."""
    import lstmp_ref as R
    o = dict(hidden_size="6", proj_size="4", num_layers="3", bias="True", batch_first="False",
             dropout="0.5", bidirectional="True")
    torch.manual_seed(0)
    net = R.LSTM_cudnn(o, 5).train()
    x = torch.randn(4, 2, 5)
    ones = {l: torch.ones(4, 2, 8) for l in range(2)}
    y1 = net(x, keep=ones)
    ye = net.eval()(x)
    net.train()
    # all-ones masks scale every inner layer output by 1 / (1 - p); eval applies nothing
    assert not torch.allclose(y1, ye)
    net.dropout = 0.0
    plain = copy.deepcopy(net)
    net.dropout = 0.5
    rs = np.random.RandomState(1)
    keep = {l: torch.from_numpy((rs.rand(4, 2, 8) > 0.5).astype(np.float32)) for l in range(2)}
    h = x
    for l in range(3):                  # layer by layer: mask / (1 - p) on the 2P-wide output
        h = torch.cat([plain._direction(h, l, d) for d in range(2)], -1)
        assert h.shape[-1] == 8
        if l < 2:
            h = h * keep[l] / 0.5
    torch.testing.assert_close(net(x, keep=keep), h)
    # a zero mask below the last layer cuts the output off from x; the last layer has no mask
    zero = {0: torch.ones(4, 2, 8), 1: torch.zeros(4, 2, 8)}
    torch.testing.assert_close(net(x, keep=zero), net(torch.randn(4, 2, 5), keep=zero))
    net.dropout = 0.0
    torch.testing.assert_close(net(x), ye)
    torch.testing.assert_close(net.eval()(x), ye)


@pytest.mark.parametrize("proj", [12, 20])
def test_engine_case_seeds_stay_inside_the_rmsprop_cap(proj):
    """The 2 % of the GPU test's RMSprop variant is a cap, not a measurement: with the seeds of
    tests/lstmp_cases.py the restatement's three fp32 training steps, each from the fp32 run's
    state, stay inside it against the same steps in fp64 (at most 2 % of a tensor's elements
    counted sign steps, each <= 2 * 4.48 lr), and the SGD variant has no outlier at all."""
    import lstmp_cases as LC
    lens, end, X, lab, masks = LC.make_data(proj)
    for optk in ("rmsprop", "sgd"):
        cfg = LC.make_cfg(optk, proj=proj)
        n32, opts, o32 = LC.oracle_nets(cfg)
        n64, _, o64 = LC.oracle_nets(cfg, torch.float64)
        assert n32["rnn"].out_dim == 2 * proj
        report = {}
        for step, (inp, T, _) in enumerate(LC.batches(lens, end, X, lab)):
            for k in n32:                   # the common start of the step
                n64[k].load_state_dict({a: b.double() for a, b in n32[k].state_dict().items()})
                sd = copy.deepcopy(o32[k].state_dict())
                for st in sd["state"].values():
                    for a, b in st.items():
                        if torch.is_tensor(b) and b.is_floating_point():
                            st[a] = b.double()
                o64[k].load_state_dict(sd)
            out32 = LC.oracle_step(n32, o32, inp, T, masks)
            out64 = LC.oracle_step(n64, o64, inp.double(), T, masks)
            np.testing.assert_allclose(out32["loss_final"].item(), out64["loss_final"].item(),
                                       rtol=1e-4)
            LC.check_update(step, optk, opts, {k: n32[k].state_dict() for k in n32},
                            {k: n64[k].state_dict() for k in n64}, report)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_lstmp_args_layout_matches_header(tmp_path):
    from pkc import _lib as L
    cls, cname = L.LstmpArgs, "pkc_lstmp_args"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pkc.h"', "int main(void) {",
             'printf("%%zu\\n", sizeof(%s));' % cname]
    expect = [("sizeof " + cname, C.sizeof(cls))]
    for f in cls._fields_:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f[0]))
        expect.append(("%s.%s" % (cname, f[0]), getattr(cls, f[0]).offset))
    lines.append('printf("%d\\n", (int)PKC_ABI_VERSION);')
    expect.append(("PKC_ABI_VERSION", 9))
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert len(got) == len(expect)
    bad = [(k, v, g) for (k, v), g in zip(expect, got) if v != g]
    assert not bad, bad
    lib = L.lib()                       # both entry points are exported
    assert lib.pkc_lstmp_fwd and lib.pkc_lstmp_bwd
    assert lib.pkc_abi_version() == 9


def test_class_refusals():
    import pkc.neural_networks as NN
    base = dict(hidden_size="8", num_layers="2", bias="True", batch_first="False", dropout="0.0",
                bidirectional="True")
    for bad in ("-1", "8", "9"):        # torch: 0 <= proj_size < hidden_size
        with pytest.raises(ValueError, match="proj_size = %s" % bad):
            NN.LSTM_cudnn(dict(base, proj_size=bad), 5)
        with pytest.raises(ValueError):
            torch.nn.LSTM(5, 8, proj_size=int(bad))
    for cls, tcls in ((NN.GRU_cudnn, torch.nn.GRU), (NN.RNN_cudnn, torch.nn.RNN)):
        with pytest.raises(ValueError, match="proj_size = 3"):
            cls(dict(base, nonlinearity="tanh", proj_size="3"), 5)
        with pytest.raises(ValueError):
            tcls(5, 8, proj_size=3)
    o = dict(base, proj_size="3")
    assert NN.LSTM_cudnn(o, 5).out_dim == 6
    # the existing refusals stay with proj_size set
    for key in ("lstm_hcgs", "hcgsx_block", "lstm_quant", "param_quant", "lstm_prune", "if_pattern"):
        with pytest.raises(NotImplementedError, match=key):
            NN.LSTM_cudnn(dict(o, **{key: "True"}), 5)
    with pytest.raises(NotImplementedError, match="input normalisation key lstm_use_laynorm_inp"):
        NN.LSTM_cudnn(dict(o, lstm_use_laynorm_inp="False"), 5)
    with pytest.raises(ValueError, match="dropout"):
        NN.LSTM_cudnn(dict(o, dropout="1.0"), 5)

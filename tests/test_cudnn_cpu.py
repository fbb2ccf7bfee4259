"""CPU checks of the *_cudnn architectures (LSTM_cudnn, GRU_cudnn, RNN_cudnn): no GPU, no HIP.

(a) the pkc classes register torch's parameter names, shapes and order and draw the reference's
    initial values: their state dict equals the golden's (tests/golden/cudnn.npz) bit for bit;
(b) the plain-torch restatement (tests/cudnn_ref.py) — what the GPU tests compare with — against the
    golden recorded from the reference and against torch.nn.LSTM / GRU / RNN called directly;
(c) the seeds of the engine-level GPU test keep the RMSprop sign-step count inside its 2 % cap:
    the restatement in fp32 against itself in fp64;
(d) the RnnStdArgs ctypes mirror has the layout of pkc_rnn_std_args; the refusals of the classes.
"""
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

G = np.load(os.path.join(GOLDEN, "cudnn.npz"))
CASES = json.loads(str(G["cases"]))
INP = int(G["inp_dim"])


def test_golden_cases_cover_the_grid():
    vals = {k: set() for k in ("H", "B", "T", "L", "bidir", "bias", "nl")}
    for c in CASES.values():
        o = c["opts"]
        vals["H"].add(int(o["hidden_size"])), vals["B"].add(c["B"]), vals["T"].add(c["T"])
        vals["L"].add(int(o["num_layers"])), vals["bidir"].add(o["bidirectional"])
        vals["bias"].add(o["bias"]), vals["nl"].add(o.get("nonlinearity"))
        if o["bidirectional"] == "True" and o["num_layers"] == "2":
            assert c["B"] == 17
        assert int(o["hidden_size"]) <= 48
    assert vals == dict(H={20, 48}, B={3, 17}, T={1, 7}, L={1, 2}, bidir={"True", "False"},
                        bias={"True", "False"}, nl={None, "tanh", "relu"})
    assert {c["cls"] for c in CASES.values()} == {"LSTM_cudnn", "GRU_cudnn", "RNN_cudnn"}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pkc_state_dict_is_the_references(name):
    import pkc.neural_networks as NN
    c = CASES[name]
    torch.manual_seed(int(G["seed"]))
    np.random.seed(int(G["seed"]))
    net = getattr(NN, c["cls"])(c["opts"], INP)
    keys = json.loads(str(G[name + "/keys"]))
    sd = net.state_dict()
    assert list(sd.keys()) == keys
    for k in keys:
        ref = G["%s/sd/%s" % (name, k)]
        assert tuple(sd[k].shape) == ref.shape and np.array_equal(sd[k].numpy(), ref), k
    H, nd = int(c["opts"]["hidden_size"]), 2 if c["opts"]["bidirectional"] == "True" else 1
    assert net.out_dim == H * nd == int(G[name + "/out_dim"])
    assert net.seq_model and not (net.prune or net.guided_hcgs or net.apply_guided_hcgs
                                  or net.if_pattern or net.skip_regularization)
    net.check_supported()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_vs_golden_and_torch(name):
    """Outputs (train and eval): rtol 1e-5, atol 1e-6 (tests/test_gpu_rnn.py:82's bound; measured
    max |dy| 1.0e-7 over these cases, GRU).  Gradients (dL/dx and every parameter), measured here
    against the golden = torch autograd through the reference class, which agreed with
    torch.nn.LSTM / GRU / RNN called directly to the last bit: max |d| 2.9e-6 (LSTM, GRU 2-layer
    bidirectional weight_ih), 0 (RNN) — at most 0.040 of the GPU tests' bound rtol 1e-3 / atol 1e-5.
    Allowed: 10x that share of the GPU bound, rtol 4e-4 / atol 4e-6 (never more than the GPU
    bound)."""
    import cudnn_ref as R
    c = CASES[name]
    torch.manual_seed(int(G["seed"]))
    net = getattr(R, c["cls"])(c["opts"], INP)
    keys = json.loads(str(G[name + "/keys"]))
    assert list(net.state_dict().keys()) == keys
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
    import cudnn_ref as R
    o = dict(hidden_size="6", num_layers="3", bias="True", batch_first="False", dropout="0.5",
             bidirectional="True")
    torch.manual_seed(0)
    net = R.GRU_cudnn(o, 5).train()
    x = torch.randn(4, 2, 5)
    ones = {l: torch.ones(4, 2, 12) for l in range(2)}
    y1 = net(x, keep=ones)
    ye = net.eval()(x)
    net.train()
    # all-ones masks scale every inner layer output by 1 / (1 - p); eval applies nothing
    assert not torch.allclose(y1, ye)
    # a zero mask below the last layer cuts the output off from x; the last layer has no mask
    zero = {0: torch.ones(4, 2, 12), 1: torch.zeros(4, 2, 12)}
    torch.testing.assert_close(net(x, keep=zero), net(torch.randn(4, 2, 5), keep=zero))
    net.dropout = 0.0
    torch.testing.assert_close(net(x), ye)


@pytest.mark.parametrize("cls", ["LSTM_cudnn", "GRU_cudnn", "RNN_cudnn"])
def test_engine_case_seeds_stay_inside_the_rmsprop_cap(cls):
    """The 2 % of tests/test_gpu_cudnn.py's RMSprop variant is a cap, not a measurement: with the
    seeds of tests/cudnn_cases.py the restatement's three fp32 training steps, each from the fp32
    run's state, stay inside it against the same steps in fp64 (and the SGD variant has no
    outlier at all)."""
    import cudnn_cases as CC
    lens, end, X, lab, masks = CC.make_data()
    for optk in ("rmsprop", "sgd"):
        cfg = CC.make_cfg(cls, optk)
        n32, opts, o32 = CC.oracle_nets(cfg)
        n64, _, o64 = CC.oracle_nets(cfg, torch.float64)
        report = {}
        for step, (inp, T, _) in enumerate(CC.batches(lens, end, X, lab)):
            for k in n32:                   # the common start of the step
                n64[k].load_state_dict({a: b.double() for a, b in n32[k].state_dict().items()})
                sd = copy.deepcopy(o32[k].state_dict())
                for st in sd["state"].values():
                    for a, b in st.items():
                        if torch.is_tensor(b) and b.is_floating_point():
                            st[a] = b.double()
                o64[k].load_state_dict(sd)
            out32 = CC.oracle_step(n32, o32, inp, T, masks)
            out64 = CC.oracle_step(n64, o64, inp.double(), T, masks)
            np.testing.assert_allclose(out32["loss_final"].item(), out64["loss_final"].item(),
                                       rtol=1e-4)
            CC.check_update(step, optk, opts, {k: n32[k].state_dict() for k in n32},
                            {k: n64[k].state_dict() for k in n64}, report)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_rnn_std_args_layout_matches_header(tmp_path):
    from pkc import _lib as L
    cls, cname = L.RnnStdArgs, "pkc_rnn_std_args"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pkc.h"', "int main(void) {",
             'printf("%%zu\\n", sizeof(%s));' % cname]
    expect = [("sizeof " + cname, C.sizeof(cls))]
    for f in cls._fields_:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f[0]))
        expect.append(("%s.%s" % (cname, f[0]), getattr(cls, f[0]).offset))
    for cn, v in (("PKC_STD_LSTM", L.STD_LSTM), ("PKC_STD_GRU", L.STD_GRU), ("PKC_STD_RNN", L.STD_RNN),
                  ("PKC_ABI_VERSION", 9)):
        lines.append('printf("%%d\\n", (int)%s);' % cn)
        expect.append((cn, v))
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


def test_class_refusals():
    import pkc.neural_networks as NN
    base = dict(hidden_size="8", num_layers="2", bias="True", batch_first="False", dropout="0.0",
                bidirectional="True")
    for cls in (NN.LSTM_cudnn, NN.GRU_cudnn, NN.RNN_cudnn):
        o = dict(base, nonlinearity="tanh")
        for key in ("lstm_hcgs", "hcgsx_block", "lstm_quant", "param_quant", "lstm_prune",
                    "if_pattern"):
            with pytest.raises(NotImplementedError, match=key):
                cls(dict(o, **{key: "True"}), 5)
        for key in ("lstm_use_laynorm_inp", "gru_use_batchnorm_inp"):
            with pytest.raises(NotImplementedError, match="input normalisation key " + key):
                cls(dict(o, **{key: "False"}), 5)
        for bad in ("1.0", "-0.1"):
            with pytest.raises(ValueError, match="dropout"):
                cls(dict(o, dropout=bad), 5)
        with pytest.raises(NotImplementedError, match="prune hook"):
            cls(o, 5).prune_parameters()
    with pytest.raises(NotImplementedError, match="nonlinearity = sigmoid"):
        NN.RNN_cudnn(dict(base, nonlinearity="sigmoid"), 5)
    assert NN.LSTM_cudnn(dict(base, batch_first="True"), 5).out_dim == 16     # parsed and ignored

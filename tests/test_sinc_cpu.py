"""SincNet on CPU: the restatement tests/sinc_ref.py against the recorded reference runs
(tests/golden/sinc.npz, written by make_golden_sinc.py), and the parameter layout / initial values
/ refusals of pkc.neural_networks.SincNet.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sinc_ref  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "sinc.npz"))
CASES = json.loads(str(G["cases"]))
INP = json.loads(str(G["inp_dims"]))
NAMES = sorted(CASES)


def golden_sd(name):
    keys = json.loads(str(G[name + "/keys"]))
    return {k: torch.from_numpy(G["%s/sd/%s" % (name, k)].copy()) for k in keys}


def _close(got, want, rel=1e-6):
    """1e-6 relative to the tensor's largest magnitude (fp32 reassociation of an identical
    computation; the golden was written by the same torch build)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    tol = rel * max(float(np.abs(want).max()), 1e-30)
    assert float(np.abs(got - want).max()) <= tol, (float(np.abs(got - want).max()), tol)


def test_golden_cases_present():
    assert set(NAMES) == {"ln", "bn", "none", "even", "neg", "k129"}
    assert INP == dict(ln=64, bn=64, none=64, even=57, neg=64, k129=200) and int(G["seed"]) == 3
    lo, bd = G["neg/sd/conv.0.low_hz_"], G["neg/sd/conv.0.band_hz_"]
    assert (lo < 0).any() and (bd < 0).any() and (lo == 0).sum() == 1 and (bd == 0).sum() == 1


@pytest.mark.parametrize("name", NAMES)
def test_sinc_ref_reproduces_golden(name):
    opts = CASES[name]
    sd = sinc_ref.leaf_state(golden_sd(name))
    x = torch.from_numpy(G[name + "/x"].copy()).requires_grad_(True)
    r = torch.from_numpy(G[name + "/r"])
    parts = {}
    y = sinc_ref.sincnet_forward(sd, opts, x, train=True, parts=parts)
    (y * r).sum().backward()
    # the generated filters: the same fp32 operations in the same order, bit for bit
    want = G[name + "/filters"]
    assert np.array_equal(parts["filters"].numpy().reshape(want.shape), want)
    _close(y.detach(), G[name + "/y"])
    _close(x.grad, G[name + "/dx"])
    for k in G.files:
        if k.startswith(name + "/grad/"):
            p = k[len(name) + 6:]
            g = sd[p].grad
            _close(torch.zeros_like(sd[p]) if g is None else g, G[k])
        if k.startswith(name + "/after/") and "running_" in k:
            _close(sd[k[len(name) + 7:]], G[k])


def test_zero_parameters_have_zero_gradient_in_the_golden():
    """torch.abs has gradient 0 at 0: the recorded reference run shows it (case neg)."""
    for p in ("low_hz_", "band_hz_"):
        v, g = G["neg/sd/conv.0." + p], G["neg/grad/conv.0." + p]
        assert (g[v == 0] == 0).all() and (g[v != 0] != 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_pkc_sincnet_layout_and_init(name):
    from pkc.neural_networks import SincNet
    opts = CASES[name]
    torch.manual_seed(int(G["seed"]))
    np.random.seed(int(G["seed"]))
    net = SincNet(opts, INP[name])
    want = golden_sd(name)
    sd = net.state_dict()
    assert list(sd.keys()) == list(want.keys())
    assert list(sd.keys())[:2] == ["conv.0.low_hz_", "conv.0.band_hz_"]
    init = golden_sd("ln") if name == "neg" else want     # neg: changed after the construction
    for k in want:
        assert tuple(sd[k].shape) == tuple(want[k].shape), k
        ref = init[k] if k in ("conv.0.low_hz_", "conv.0.band_hz_") else want[k]
        assert torch.equal(sd[k], ref), "initial %s differs from the reference's" % k
    assert net.out_dim == int(G[name + "/out_dim"])
    assert [n for n, _ in net.named_parameters()] == [k for k in want
                                                      if "running_" not in k and "num_batches" not in k]
    net.load_state_dict(want)          # strict
    net.check_supported()
    for a in ("prune", "guided_hcgs", "apply_guided_hcgs", "if_pattern", "skip_regularization"):
        assert not getattr(net, a)
    # window_ and n_: plain attributes with the reference's fp32 values, not in the state dict
    K = sinc_ref.geometry(opts, INP[name])[0][2]
    n_, window = sinc_ref.sinc_consts(K, 16000)
    assert net.conv[0].kernel_size == K
    assert torch.equal(net.conv[0].n_, n_) and torch.equal(net.conv[0].window_, window)
    sp = net.conv_specs()[0]
    assert sp["len"] == K and sp["C_in"] == 1 and sp["W"] is None and sp["b"] is None
    assert sp["sinc"]["low"] is net.conv[0].low_hz_ and sp["sinc"]["band"] is net.conv[0].band_hz_


def test_even_length_geometry():
    """neural_networks.py:2094 against :2193-2194: len 8 convolves with 9 taps; at inp_dim 57 and
    pool 3 both lengths give 16 positions, at inp_dim 55 they give 16 against 15 and the reference's
    own forward fails, so the shape is refused with the two line references."""
    from pkc.neural_networks import SincNet
    net = SincNet(CASES["even"], 57)
    net.check_supported()
    assert net.L_out[0] == 16 and net.conv_specs()[0]["len"] == 9
    assert [bn.eps for bn in net.bn] == [16, 7]
    bad = SincNet(CASES["even"], 55)
    with pytest.raises(ValueError, match="2094") as e:
        bad.check_supported()
    assert "2193-2194" in str(e.value)


def test_refusals():
    from pkc.neural_networks import SincNet
    both = dict(CASES["none"], sinc_use_laynorm="True,False", sinc_use_batchnorm="True,False")
    with pytest.raises(NotImplementedError):
        SincNet(both, 64).check_supported()
    with pytest.raises(NotImplementedError):
        SincNet(dict(CASES["none"], sinc_act="relu,softmax"), 64).check_supported()
    with pytest.raises(ValueError):
        SincNet(CASES["none"], 20).check_supported()       # 20 - 17 + 1 = 4 -> 2, then 2 - 3 + 1 = 0
    assert SincNet(dict(CASES["none"], skip_regularization="True"), 64).skip_regularization


def test_cgs_keys_are_refused():
    """The reference SincNet has no masks, quantisation or pruning: such keys raise."""
    from pkc.neural_networks import SincNet
    for k in ("sinc_quant", "sinc_quant_inp", "sinc_prune", "sinc_hcgs", "if_pattern",
              "guided_hcgs", "apply_guided_hcgs"):
        with pytest.raises(NotImplementedError):
            SincNet(dict(CASES["none"], **{k: "True"}), 64).check_supported()


def test_sinc_struct_matches_header(tmp_path):
    """The new ctypes mirror against include/pkc.h (as test_conv_structs_match_header)."""
    import ctypes as C
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    from pkc import _lib as L
    root = os.path.dirname(HERE)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pkc.h"', "int main(void) {"]
    expect = []
    cls, cname = L.SincArgs, "pkc_sinc_args"
    lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
    expect.append(C.sizeof(cls))
    for f in cls._fields_:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f[0]))
        expect.append(getattr(cls, f[0]).offset)
    lines += ["return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o",
                    str(tmp_path / "probe")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == expect
    for fn in ("pkc_sinc_ok", "pkc_sinc_filters_fwd", "pkc_sinc_filters_bwd"):
        assert fn in L._SIGS

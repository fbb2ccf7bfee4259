"""CNN on CPU: the restatement tests/cnn_ref.py against the recorded reference runs
(tests/golden/cnn.npz, written by make_golden_cnn.py), and the parameter layout / init draws /
refusals of pkc.neural_networks.CNN.  No GPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cnn_ref  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "cnn.npz"))
CASES = json.loads(str(G["cases"]))
INP = int(G["inp_dim"])
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
    assert set(NAMES) == {"ln", "bn", "none", "ln0", "bn0", "leaky"}
    assert INP == 55 and int(G["seed"]) == 3


@pytest.mark.parametrize("name", NAMES)
def test_cnn_ref_reproduces_golden(name):
    opts = CASES[name]
    sd = cnn_ref.leaf_state(golden_sd(name))
    x = torch.from_numpy(G[name + "/x"].copy()).requires_grad_(True)
    r = torch.from_numpy(G[name + "/r"])
    y = cnn_ref.cnn_forward(sd, opts, x, train=True)
    (y * r).sum().backward()
    _close(y.detach(), G[name + "/y"])
    _close(x.grad, G[name + "/dx"])
    for k in G.files:
        if k.startswith(name + "/grad/"):
            p = k[len(name) + 6:]
            g = sd[p].grad
            _close(torch.zeros_like(sd[p]) if g is None else g, G[k])
        if k.startswith(name + "/after/") and "running_" in k:
            _close(sd[k[len(name) + 7:]], G[k])


@pytest.mark.parametrize("name", NAMES)
def test_pkc_cnn_layout_and_init(name):
    from pkc.neural_networks import CNN
    opts = CASES[name]
    torch.manual_seed(int(G["seed"]))
    np.random.seed(int(G["seed"]))
    net = CNN(opts, INP)
    want = golden_sd(name)
    sd = net.state_dict()
    assert list(sd.keys()) == list(want.keys())
    for k in want:
        assert tuple(sd[k].shape) == tuple(want[k].shape), k
        assert torch.equal(sd[k], want[k]), "initial %s differs from the reference's" % k
    assert net.out_dim == int(G[name + "/out_dim"])
    assert [n for n, _ in net.named_parameters()] == [k for k in want
                                                      if "running_" not in k and "num_batches" not in k]
    net.load_state_dict(want)
    net.check_supported()
    for a in ("prune", "guided_hcgs", "apply_guided_hcgs", "if_pattern", "skip_regularization"):
        assert not getattr(net, a)


def test_bn_eps_is_l_out():
    """neural_networks.py:1988-1990: the second positional argument of BatchNorm1d is eps."""
    from pkc.neural_networks import CNN
    net = CNN(CASES["bn"], INP)
    assert [bn.eps for bn in net.bn] == [15, 6, 4]
    assert [bn.momentum for bn in net.bn] == [0.05] * 3
    assert [sp["L_out"] for sp in net.conv_specs()] == [15, 6, 4]


def test_refusals():
    from pkc.neural_networks import CNN
    both = dict(CASES["none"], cnn_use_laynorm="True,False,False",
                cnn_use_batchnorm="True,False,False")
    with pytest.raises(NotImplementedError):
        CNN(both, INP).check_supported()
    with pytest.raises(NotImplementedError):
        CNN(dict(CASES["none"], cnn_act="relu,softmax,relu"), INP).check_supported()
    assert CNN(dict(CASES["none"], skip_regularization="True"), INP).skip_regularization


def test_conv_structs_match_header(tmp_path):
    """The two new ctypes mirrors against include/pkc.h (the check test_abi_layout.py makes for
    the nine older structs)."""
    import ctypes as C
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("needs gcc")
    from pkc import _lib as L
    root = os.path.dirname(HERE)
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pkc.h"', "int main(void) {"]
    expect = []
    for py, cname in (("Conv1dArgs", "pkc_conv1d_args"), ("ConvPostArgs", "pkc_conv_post_args")):
        cls = getattr(L, py)
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
    assert L.CONV_NORM_LN == 3


def test_cgs_keys_are_refused():
    """The reference CNN has no masks, quantisation or pruning: such keys raise, not pass silently."""
    from pkc.neural_networks import CNN
    for k in ("cnn_quant", "cnn_prune", "cnn_hcgs", "if_pattern"):
        with pytest.raises(NotImplementedError):
            CNN(dict(CASES["none"], **{k: "True"}), INP).check_supported()

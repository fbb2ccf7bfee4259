"""CPU checks of the SRU architecture (no GPU, no HIP):

(a) the hand-written backward of the cell (tests/sru_ref.py cell_bwd: the kernel's formulas) equals
    autograd of the restatement in float64;
(b) a bidirectional restatement equals two unidirectional ones, the second time-flipped;
(c) the pkc class: state-dict names, shapes and order, out_dim, the init facts, every refusal by key,
    a state-dict round trip;
(d) the SruArgs ctypes mirror has the layout of pkc_sru_args; the header still says ABI 9.
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

import sru_ref as R

OPTS = dict(sru_hidden_size="8", sru_num_layers="2", sru_dropout="0.0", sru_rnn_dropout="0.0",
            sru_use_tanh="False", sru_use_relu="False", sru_use_selu="False",
            sru_weight_norm="False", sru_layer_norm="False", sru_bidirectional="True",
            sru_is_input_normalized="False", sru_has_skip_term="True", sru_rescale="True",
            sru_highway_bias="-1.5", sru_n_proj="0")


def make_case(seed, T, B, d, D, k, skip=True, mask=False, dtype=torch.float64):
    """Random operands of one layer at kernel level (U given, not a projection)."""
    g = torch.Generator().manual_seed(seed)
    n = d * D
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dtype)      # noqa: E731
    U, X, dy = r(T, B, n * k), r(T, B, n), r(T, B, n)
    wc, bias = r(2 * n), 0.5 * r(2 * n)
    m_c = None
    if mask:
        m_c = (torch.rand(B, n, generator=g) > 0.3).to(dtype) / 0.7
    return U, X, wc, bias, dy, m_c


CELL_CASES = [(k, D, act, skip, mask)
              for k in (3, 4) for D in (1, 2) for act in ("linear", "tanh", "relu")
              for skip, mask in ((True, False), (True, True))] + [
             (3, 2, "tanh", False, True), (3, 1, "linear", False, False)]


@pytest.mark.parametrize("k,D,act,skip,mask", CELL_CASES)
def test_hand_backward_equals_autograd(k, D, act, skip, mask):
    T, B, d, alpha = 6, 3, 5, 1.3
    U, X, wc, bias, dy, m_c = make_case(11 * k + D, T, B, d, D, k, skip, mask)
    leaves = [t.clone().requires_grad_(True) for t in (U, X, wc, bias)]
    y, c = R.cell_fwd(leaves[0], leaves[1], leaves[2], leaves[3], d, D, k, act, skip, alpha, m_c)
    (y * dy).sum().backward()
    dU, dXh, dwc, dbias = R.cell_bwd(U, X, wc, bias, c.detach(), dy, d, D, k, act, skip, alpha, m_c)
    kw = dict(rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dU, leaves[0].grad, **kw)
    torch.testing.assert_close(dwc, leaves[2].grad, **kw)
    torch.testing.assert_close(dbias, leaves[3].grad, **kw)
    if k == 3 and skip:
        torch.testing.assert_close(dXh, leaves[1].grad, **kw)
    else:
        assert dXh is None and leaves[1].grad is None


@pytest.mark.parametrize("both", [False, True])
def test_architecture_backward_through_projection_and_input_mask(both):
    """dweight = Xt^T dU and dX = (dU weight^T) * m_x + dXh around the cell's hand backward equal
    autograd of the whole architecture restatement (2 layers: k = 4 then k = 3, both masks)."""
    torch.manual_seed(3)
    o = dict(OPTS, sru_dropout="0.3", sru_rnn_dropout="0.25" if both else "0.0", sru_use_tanh="True")
    net = R.SRU(o, 5).double().train()
    T, B = 5, 3
    x = torch.randn(T, B, 5, dtype=torch.float64, requires_grad=True)
    r = torch.randn(T, B, 16, dtype=torch.float64)
    masks = {(l, "c"): (torch.rand(B, 16) > 0.3).double() for l in range(2)}
    masks.update({(0, "x"): (torch.rand(B, 5) > 0.25).double(),
                  (1, "x"): (torch.rand(B, 16) > 0.25).double()})
    (net(x, masks) * r).sum().backward()
    # by hand, top layer first
    xs, saved = [x.detach()], []
    for l, cell in enumerate(net.sru.rnn_lst):
        k = cell.weight.shape[1] // 16
        mx = masks[(l, "x")] / (1 - net.rnn_dropout) if both else torch.ones(B, xs[-1].shape[2],
                                                                              dtype=torch.float64)
        mc = masks[(l, "c")] / (1 - net.dropout)
        xt = xs[-1] * mx
        U = (xt.reshape(T * B, -1) @ cell.weight.detach()).view(T, B, -1)
        y, c = R.cell_fwd(U, xs[-1], cell.weight_c.detach(), cell.bias.detach(), 8, 2, k, "tanh", True,
                          net.alpha, mc)
        saved.append((U, xt, c, mx, mc, k))
        xs.append(y)
    dy = r
    for l in (1, 0):
        cell = net.sru.rnn_lst[l]
        U, xt, c, mx, mc, k = saved[l]
        dU, dXh, dwc, dbias = R.cell_bwd(U, xs[l], cell.weight_c.detach(), cell.bias.detach(), c, dy, 8,
                                         2, k, "tanh", True, net.alpha, mc)
        kw = dict(rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(xt.reshape(T * B, -1).t() @ dU.view(T * B, -1), cell.weight.grad, **kw)
        torch.testing.assert_close(dwc, cell.weight_c.grad, **kw)
        torch.testing.assert_close(dbias, cell.bias.grad, **kw)
        dy = (dU.view(T * B, -1) @ cell.weight.detach().t()).view(T, B, -1) * mx
        if dXh is not None:
            dy = dy + dXh
    torch.testing.assert_close(dy, x.grad, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("k", [3, 4])
def test_bidirectional_equals_two_unidirectional(k):
    T, B, d = 7, 3, 5
    U, X, wc, bias, dy, m_c = make_case(5, T, B, d, 2, k, mask=True)
    y, c = R.cell_fwd(U, X, wc, bias, d, 2, k, "tanh", True, 1.2, m_c)
    u4 = U.view(T, B, 2 * d, k)
    half = lambda v, h: torch.cat([v[h * d:(h + 1) * d], v[2 * d + h * d:2 * d + (h + 1) * d]])  # noqa: E731
    y0, c0 = R.cell_fwd(u4[:, :, :d].reshape(T, B, -1), X[:, :, :d], half(wc, 0), half(bias, 0), d, 1, k,
                        "tanh", True, 1.2, m_c[:, :d])
    y1, c1 = R.cell_fwd(u4[:, :, d:].flip(0).reshape(T, B, -1), X[:, :, d:].flip(0), half(wc, 1),
                        half(bias, 1), d, 1, k, "tanh", True, 1.2, m_c[:, d:])
    assert torch.equal(y[:, :, :d], y0) and torch.equal(y[:, :, d:], y1.flip(0))
    assert torch.equal(c[:, :, :d], c0) and torch.equal(c[:, :, d:], c1.flip(0))


def test_class_state_dict_and_init():
    import pkc.neural_networks as NN
    torch.manual_seed(4)
    net = NN.SRU(OPTS, 5)
    sd = net.state_dict()
    assert list(sd.keys()) == ["sru.rnn_lst.%d.%s" % (l, n) for l in range(2)
                               for n in ("weight", "weight_c", "bias")]
    assert [tuple(v.shape) for v in sd.values()] == [(5, 64), (32,), (32,), (16, 48), (32,), (32,)]
    assert net.out_dim == 16 and net.seq_model
    assert not (net.prune or net.guided_hcgs or net.apply_guided_hcgs or net.if_pattern
                or net.skip_regularization)
    assert net.alpha == pytest.approx(math.sqrt(1 + 2 * math.exp(-1.5)))
    for l, n_in in ((0, 5), (1, 16)):
        w, wc, b = (sd["sru.rnn_lst.%d.%s" % (l, n)] for n in ("weight", "weight_c", "bias"))
        assert w.abs().max() <= math.sqrt(3.0 / n_in) and w.abs().max() > 0.8 * math.sqrt(3.0 / n_in)
        assert wc.abs().max() <= math.sqrt(1.5) and wc.abs().max() > 0.8 * math.sqrt(1.5)
        assert torch.equal(b[:16], torch.zeros(16)) and torch.equal(b[16:], torch.full((16,), -1.5))
    # the same draws, in the same order, as the restatement's
    torch.manual_seed(4)
    ref = R.SRU(OPTS, 5)
    assert all(torch.equal(sd[k], v) for k, v in ref.state_dict().items())
    # without rescale: weight_c over the whole +-sqrt(3), alpha 1; without the skip term k = 3
    torch.manual_seed(4)
    n2 = NN.SRU(dict(OPTS, sru_rescale="False", sru_has_skip_term="False"), 5)
    assert n2.alpha == 1.0 and n2.sru.rnn_lst[0].weight.shape == (5, 48)
    assert n2.sru.rnn_lst[0].weight_c.abs().max() > math.sqrt(1.5)
    specs = n2.layer_specs()
    assert [sp["k"] for sp in specs] == [3, 3] and [sp["n_in"] for sp in specs] == [5, 16]
    assert NN.SRU(dict(OPTS, sru_use_tanh="True", sru_use_relu="True"), 5).act == "tanh"
    assert NN.SRU(dict(OPTS, sru_use_relu="True"), 5).act == "relu"
    # round trip
    other = NN.SRU(OPTS, 5)
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(other.state_dict()[k], v) for k, v in sd.items())
    # 1-D recurrence vectors: what cost_l1 / cost_l2 skip
    assert [p.dim() for p in net.parameters()] == [2, 1, 1, 2, 1, 1]


def test_class_refusals():
    import pkc.neural_networks as NN
    for key in ("sru_use_selu", "sru_weight_norm", "sru_layer_norm", "sru_is_input_normalized"):
        with pytest.raises(NotImplementedError, match=key):
            NN.SRU(dict(OPTS, **{key: "True"}), 5)
    with pytest.raises(NotImplementedError, match="sru_n_proj"):
        NN.SRU(dict(OPTS, sru_n_proj="4"), 5)
    for key in ("sru_hcgs", "hcgsx_block", "sru_quant", "param_quant", "sru_prune", "if_pattern",
                "sru_use_laynorm_inp", "sru_use_batchnorm_inp"):
        with pytest.raises(NotImplementedError, match=key):
            NN.SRU(dict(OPTS, **{key: "False"}), 5)
    for key in ("sru_dropout", "sru_rnn_dropout"):
        for bad in ("1.0", "-0.1"):
            with pytest.raises(ValueError, match=key):
                NN.SRU(dict(OPTS, **{key: bad}), 5)
    with pytest.raises(NotImplementedError, match="prune hook"):
        NN.SRU(OPTS, 5).prune_parameters()


def test_graph_node_contract():
    """SruNode declares kind flags only (the Node contract of tests/test_engine_types_cpu.py) and
    lists weight, weight_c and bias per layer."""
    import pkc.graph as G
    import pkc.neural_networks as NN
    assert G.Node.sru is False
    own = {k for c in G.SruNode.__mro__ if c not in (G.Node, object)
           for k, v in vars(c).items() if not k.startswith("__") and not callable(v)}
    assert own <= {"rec", "std", "sru"} and G.SruNode.rec and G.SruNode.sru and not G.SruNode.std
    assert not (G.RecNode.sru or G.StdRecNode.sru or G.Layer.sru)
    net = NN.SRU(OPTS, 5)
    node = G.SruNode("a", net, 5)
    ps = node.params()
    assert [p for p, _, _ in ps] == list(net.parameters())
    assert [key for _, key, _ in ps] == [(g, l, 0) for l in range(2)
                                          for g in ("dweight", "dwc", "dbias")]
    with pytest.raises(ValueError, match="built for 5 inputs"):
        G.SruNode("a", net, 7)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_sru_args_layout_matches_header(tmp_path):
    from pkc import _lib as L
    cls, cname = L.SruArgs, "pkc_sru_args"
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
    assert L.ABI_VERSION == 9


def test_kernel_cases_cover_the_grid():
    import sru_cases as SC
    v = list(SC.KERNEL_CASES.values())
    assert {c[0] for c in v} == {8, 40, 96, 550} and {c[1] for c in v} == {1, 7, 33, 20}
    assert {c[2] for c in v} == {1, 3, 8} and {c[3] for c in v} == {1, 2}
    assert {c[4] for c in v} == {3, 4} and {c[5] for c in v} == {"linear", "tanh", "relu"}
    assert {c[6] for c in v} == {True, False} and any(c[7] != 1.0 for c in v)
    assert any(c[8] for c in v) and {c[9] for c in v} == {1, 3}
    assert (550, 20, 8, 2) in {c[:4] for c in v}


def test_kernel_case_seeds_sit_inside_the_bound():
    """The float32 restatement's own error against the float64 one, per case and quantity, is at
    most a quarter of the kernel bound rtol 1e-4 / atol 1e-5 (so 4 x d_ref, the second bound of
    tests/test_gpu_sru.py, is the tighter of the two), and it is not zero where the result is not."""
    import sru_cases as SC
    for name in sorted(SC.KERNEL_CASES):
        r64, d_ref, r32 = SC.kernel_reference(name)
        for q in r64:
            share = ((r32[q].double() - r64[q]).abs() / (SC.ATOL + SC.RTOL * r64[q].abs())).max().item()
            assert share <= 0.25, (name, q, share)
            # (T = 1: dweight_c = sum da c_{t-1} is exactly zero in every precision)
            assert d_ref[q] > 0 or not r64[q].any(), (name, q)

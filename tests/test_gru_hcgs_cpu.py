"""The HCGS hook on the GRU, minimalGRU and RNN classes (gru_hcgs / minimalgru_hcgs / rnn_hcgs; a pkc
extension like ligru_hcgs, pinned on the LSTM hook's semantics), without a GPU: the product classes
against the restatement (tests/gru_hcgs_ref.py), and the restatement against
tests/golden/gru_hcgs.npz, recorded from the reference's own classes with masks from the
reference's hcgs.conn_mat multiplied into .weight.data."""
import configparser
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from cases import GRU_CASES, GRU_DEF, MINGRU_DEF, PLAIN_CASES, RNN_DEF

import gru_hcgs_ref as R

BASE = {"GRU": (GRU_DEF, "gru"), "minimalGRU": (MINGRU_DEF, "minimalgru"), "RNN": (RNN_DEF, "rnn")}


def section(d):
    cp = configparser.ConfigParser()
    cp["s"] = {k: str(v) for k, v in d.items()}
    return cp["s"]


def pair(cls, opts, F, seed):
    import pkc.neural_networks as NN
    nets = []
    for c in (getattr(NN, cls), getattr(R, cls)):
        torch.manual_seed(seed)
        np.random.seed(seed)
        nets.append(c(section(opts), F))
    return nets


@pytest.mark.parametrize("bidir", [True, False])
@pytest.mark.parametrize("cls", ["GRU", "minimalGRU", "RNN"])
def test_class_matches_restatement(cls, bidir):
    """Equal state dicts (names, order, values) at equal seeds; the masks are Parameters hcgsx.<i> /
    hcgsh.<i> of shapes (n, cur) / (n, n) with the density the block lists give."""
    base, p = BASE[cls]
    opts = R.hook_opts(cls, dict(base, **{p + "_lay": "32,24", p + "_bidir": str(bidir)}))
    net, ref = pair(cls, opts, 20, 9)
    assert net.hcgs_on and getattr(net, R.KEYS[cls]) is True
    sd, rsd = net.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd)
    assert list(sd)[:4] == ["hcgsx.0.mask", "hcgsx.1.mask", "hcgsh.0.mask", "hcgsh.1.mask"]
    for k in sd:
        assert torch.equal(sd[k], rsd[k]), k
    assert [n for n, _ in net.named_parameters()] == [n for n, _ in ref.named_parameters()]
    cur = 20
    for i, n in enumerate((32, 24)):
        mx, mh = sd["hcgsx.%d.mask" % i], sd["hcgsh.%d.mask" % i]
        assert tuple(mx.shape) == (n, cur) and tuple(mh.shape) == (n, n)
        assert set(mx.unique().tolist()) <= {0.0, 1.0} and set(mh.unique().tolist()) <= {0.0, 1.0}
        # [8,4] / [25,50] on an n x n matrix of whole 8-blocks: round(0.75 n/8) of n/8 block
        # columns kept per block row, half of each kept block's 4-blocks
        nb = n // 8
        assert mh.double().mean().item() == pytest.approx(round(0.75 * nb) / nb * 0.5)
        cur = 2 * n if bidir else n
    specs = net.layer_specs()
    for i, sp in enumerate(specs):
        assert sp["Wmask"] is net.hcgsx[i].mask and sp["Umask"] is net.hcgsh[i].mask
    with pytest.raises(NotImplementedError):
        net.prune_parameters()


def test_draw_order_across_layers():
    """numpy's RNG is consumed W mask 0, U mask 0, W mask 1, U mask 1 — the LSTM hook's order."""
    from pkc.cgs import hcgs_mask
    opts = R.hook_opts("GRU", dict(GRU_DEF, gru_lay="32,24"))
    net, _ = pair("GRU", opts, 20, 11)
    np.random.seed(11)
    cur = 20
    for i, n in enumerate((32, 24)):
        np.testing.assert_array_equal(net.hcgsx[i].mask.detach().numpy(),
                                      hcgs_mask(n, cur, [8, 4], [50, 50]))
        np.testing.assert_array_equal(net.hcgsh[i].mask.detach().numpy(),
                                      hcgs_mask(n, n, [8, 4], [25, 50]))
        cur = 2 * n


ALL = [(t, "GRU", o, F, sd) for t, o, T, B, F, sd in GRU_CASES] + \
      [(t, c, o, F, sd) for t, c, o, T, B, F, sd in PLAIN_CASES]


@pytest.mark.parametrize("case", ALL, ids=[c[0] for c in ALL])
def test_without_the_key_nothing_moves(case):
    """Key absent, or False with the hcgs* lists present: the same state-dict keys in the same
    order and the same bytes as the hook-free restatement (oracle.nets) at the same seeds, the
    pinned reference init (tests/golden/gru.npz), no mask drawn (numpy's RNG untouched),
    layer_specs() without masks."""
    import pkc.neural_networks as NN
    from oracle import nets as ON
    tag, cls, opts, F, seed = case
    g = np.load(os.path.join(GOLDEN, "gru.npz"), allow_pickle=False)
    for o in (opts, dict(opts, **{R.KEYS[cls]: "False"}, **R.HOOK)):
        torch.manual_seed(seed)
        np.random.seed(seed)
        net = getattr(NN, cls)(section(o), F)
        probe = np.random.rand()
        np.random.seed(seed)
        assert probe == np.random.rand(), "the constructor consumed numpy's RNG"
        sd = net.state_dict()
        torch.manual_seed(seed)
        today = getattr(ON, cls)(section(opts), F).state_dict()    # the hook-free restatement
        assert list(sd) == list(today)
        for k, v in sd.items():
            assert v.numpy().tobytes() == today[k].numpy().tobytes(), k
            # (the pinned init itself: bit-exact where the fixture was recorded, test_host_cpu; another
            # host's LAPACK may round the orthogonal init's QR differently in the last bit)
            np.testing.assert_allclose(v.numpy(), g[tag + "/init/" + k], rtol=1e-5, atol=1e-6,
                                       err_msg=k)
        assert not hasattr(net, "hcgsx") and not net.hcgs_on
        assert all(sp["Wmask"] is None and sp["Umask"] is None for sp in net.layer_specs())


@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=[c[0] for c in R.GOLDEN_CASES])
def test_restatement_reproduces_reference_golden(case):
    """y, dL/dx and every parameter gradient of sum(y * r) recorded from the reference's classes
    (masks multiplied into .weight.data), at tests/test_gpu_rnn.py's bounds for gru.npz; the
    product class at the golden's seeds draws the golden's masks."""
    tag, cls, lay, bidir, seed = case
    g = np.load(os.path.join(GOLDEN, "gru_hcgs.npz"), allow_pickle=False)
    net, ref = pair(cls, R.golden_opts(cls, lay, bidir), R.GOLDEN_F, seed)
    keys = sorted(k[len(tag) + 6:] for k in g.files if k.startswith(tag + "/init/"))
    assert sorted(ref.state_dict()) == keys
    for k, v in net.state_dict().items():
        if "mask" in k:     # numpy's RNG: the same draws on every host (the weights' orthogonal
            # init goes through the host's LAPACK; the classes' draws are pinned on each other above)
            np.testing.assert_array_equal(v.numpy(), g[tag + "/init/" + k], err_msg=k)
    ref.load_state_dict({k: torch.from_numpy(g[tag + "/init/" + k]) for k in keys})
    ref.train()
    x = torch.from_numpy(g[tag + "/x"]).requires_grad_(True)
    y = ref(x)
    (y * torch.from_numpy(g[tag + "/r"])).sum().backward()
    np.testing.assert_allclose(y.detach().numpy(), g[tag + "/y"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(x.grad.numpy(), g[tag + "/dx"], rtol=1e-3, atol=1e-5)
    n = 0
    for k, p in ref.named_parameters():
        if "mask" in k or p.grad is None:      # (unused here: the LayerNorm of h)
            assert p.grad is None and tag + "/grad/" + k not in g.files, k
            continue
        np.testing.assert_allclose(p.grad.numpy(), g[tag + "/grad/" + k], rtol=1e-3, atol=1e-5,
                                   err_msg=k)
        n += 1
    assert n == len([k for k in g.files if k.startswith(tag + "/grad/")])
    # the forward left W and U masked in place
    for k, v in ref.state_dict().items():
        parts = k.split(".")
        if parts[0][0] in "wu" and k.endswith("weight"):
            m = g[tag + "/init/%s.%s.mask" % ("hcgsx" if parts[0][0] == "w" else "hcgsh", parts[1])]
            assert bool((v.numpy()[m == 0] == 0).all()), k

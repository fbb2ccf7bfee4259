"""Generate tests/golden/gru_hcgs.npz from the *reference*'s own GRU / minimalGRU / RNN classes.

The reference gives these classes no HCGS hook, so the fixture pins the hook pkc adds (gru_hcgs /
minimalgru_hcgs / rnn_hcgs) on the LSTM hook's semantics: per layer a W mask and a U mask from the
reference's hcgs.conn_mat (numpy's global RNG; W mask then U mask, layers in order), multiplied
into every gate's .weight.data before the forward (neural_networks.py:858-861, 980-983).  Runs only
where the reference is present; only data leaves (inputs, masks, expected outputs and gradients).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gru_hcgs.py
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as MG  # noqa: E402  (the reference imports and the CPU shims)

sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
import gru_hcgs_ref as R  # noqa: E402  (the cases; none of its classes is used here)


def run_case(tag, cls, lay, bidir, seed, out):
    o = R.golden_opts(cls, lay, bidir)
    torch.manual_seed(seed)
    np.random.seed(seed)
    opts = {k: v for k, v in o.items() if "hcgs" not in k}
    net = getattr(MG.neural_networks, cls)(MG.section(opts), R.GOLDEN_F)
    ints = lambda k, f=int: [f(v) for v in o[k].split(",")]      # noqa: E731
    masks, cur = {}, R.GOLDEN_F
    for i, n in enumerate(ints(R.KEYS[cls].replace("_hcgs", "_lay"))):
        # conn_mat consumes the lists it is given: fresh ones per call
        masks["hcgsx.%d.mask" % i] = MG.hcgs.conn_mat(n, cur, ints("hcgsx_block"),
                                                      ints("hcgsx_sparse", float)).float()
        masks["hcgsh.%d.mask" % i] = MG.hcgs.conn_mat(n, n, ints("hcgsh_block"),
                                                      ints("hcgsh_sparse", float)).float()
        cur = 2 * n if bidir else n
    MG.sd_np(net, tag + "/init/", out)
    for k, m in masks.items():
        out[tag + "/init/" + k] = m.numpy().copy()
    for k, m in masks.items():
        kind, i, _ = k.split(".")
        for g in R.GATES[cls]:
            lin = getattr(net, ("w" if kind == "hcgsx" else "u") + g)[int(i)]
            lin.weight.data.mul_(m)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(R.GOLDEN_T, R.GOLDEN_B, R.GOLDEN_F, generator=gen)
    r = torch.randn(R.GOLDEN_T, R.GOLDEN_B, net.out_dim, generator=gen)
    out[tag + "/x"], out[tag + "/r"] = x.numpy().copy(), r.numpy().copy()
    xi = x.clone().requires_grad_(True)
    y = net(xi)
    (y * r).sum().backward()
    out[tag + "/y"] = y.detach().numpy().copy()
    out[tag + "/dx"] = xi.grad.numpy().copy()
    for pn, p in net.named_parameters():
        if p.grad is not None:
            out[tag + "/grad/" + pn] = p.grad.numpy().copy()


if __name__ == "__main__":
    res = {}
    for case in R.GOLDEN_CASES:
        run_case(*case, res)
    np.savez_compressed(os.path.join(OUT, "gru_hcgs.npz"), **res)
    print("wrote gru_hcgs.npz: %d arrays" % len(res))

"""Regenerate tests/golden/sinc.npz from the reference's neural_networks.SincNet on CPU.

Usage: python tests/golden/make_golden_sinc.py <path of the reference checkout>

Data only: for every case the options, the initial state dict (seed 3; case `neg` after some
low_hz_ / band_hz_ entries were negated or zeroed), an input, the training-mode output, the
gradients of every parameter and of x under loss = (y * r).sum() with a recorded r, layer 0's
generated filters, and the BatchNorm running statistics after that one training forward.  The
reference is imported the way make_golden.py does (CPU-only: Tensor.cuda is the identity).
"""
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SEED = 3
BATCH = 5
BASE = dict(sinc_N_filt="10,6", sinc_len_filt="17,3", sinc_max_pool_len="2,1",
            sinc_use_laynorm_inp="False", sinc_use_batchnorm_inp="False",
            sinc_use_laynorm="False,False", sinc_use_batchnorm="False,False",
            sinc_act="relu,relu", sinc_drop="0.0,0.0", sinc_sample_rate="16000",
            sinc_min_low_hz="50", sinc_min_band_hz="50")
LN = dict(BASE, sinc_use_laynorm_inp="True", sinc_use_laynorm="True,True")
CASES = {
    "ln": dict(LN),
    "bn": dict(BASE, sinc_use_batchnorm_inp="True", sinc_use_batchnorm="True,True"),
    "none": dict(BASE),
    "even": dict(LN, sinc_len_filt="8,3", sinc_max_pool_len="3,2"),
    "neg": dict(LN),
    "k129": dict(LN, sinc_N_filt="10", sinc_len_filt="129", sinc_max_pool_len="3",
                 sinc_use_laynorm="True", sinc_act="relu", sinc_drop="0.0"),
}
INP = {"ln": 64, "bn": 64, "none": 64, "even": 57, "neg": 64, "k129": 200}


def main(ref):
    sys.path.insert(0, ref)
    torch.Tensor.cuda = lambda t, *a, **k: t          # noqa: E731  (CPU-only)
    import neural_networks                             # noqa: E402
    out = {"cases": np.array(json.dumps(CASES)), "seed": np.int64(SEED),
           "inp_dims": np.array(json.dumps(INP))}
    for name, opts in CASES.items():
        inp = INP[name]
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        net = neural_networks.SincNet(opts, inp)
        net.train()
        if name == "neg":
            with torch.no_grad():
                lo, bd = net.conv[0].low_hz_, net.conv[0].band_hz_
                lo[1] *= -1
                lo[4] = 0.0
                lo[8] *= -1
                bd[2] *= -1
                bd[7] = 0.0
                bd[8] *= -1
        sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
        out[name + "/keys"] = np.array(json.dumps(list(sd0.keys())))
        for k, v in sd0.items():
            out["%s/sd/%s" % (name, k)] = v.numpy()
        rs = np.random.RandomState(11)
        x = torch.from_numpy(rs.randn(BATCH, inp).astype(np.float32)).requires_grad_(True)
        r = torch.from_numpy(rs.randn(BATCH, net.out_dim).astype(np.float32))
        y = net(x)
        (y * r).sum().backward()
        out[name + "/out_dim"] = np.int64(net.out_dim)
        out[name + "/x"], out[name + "/r"] = x.detach().numpy(), r.numpy()
        out[name + "/y"], out[name + "/dx"] = y.detach().numpy(), x.grad.numpy()
        out[name + "/filters"] = net.conv[0].filters.detach().numpy()
        for k, p in net.named_parameters():
            out["%s/grad/%s" % (name, k)] = (p.grad if p.grad is not None
                                             else torch.zeros_like(p)).numpy()
        for k, v in net.state_dict().items():          # after the one training forward
            if "running_" in k or "num_batches" in k:
                out["%s/after/%s" % (name, k)] = v.numpy()
    path = os.path.join(OUT, "sinc.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

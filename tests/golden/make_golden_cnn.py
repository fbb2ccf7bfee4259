"""Regenerate tests/golden/cnn.npz from the reference's neural_networks.CNN on CPU.

Usage: python tests/golden/make_golden_cnn.py <path of the reference checkout>

Data only: for every case the options, the initial state dict (seed 3), an input, the training-mode
output, the gradients of every parameter and of x under loss = (y * r).sum() with a recorded r, and
the BatchNorm running statistics after that one training forward.  The reference is imported the
way make_golden.py does (CPU-only: Tensor.cuda is the identity).
"""
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SEED = 3
INP = 55
BATCH = 5
BASE = dict(cnn_N_filt="8,6,6", cnn_len_filt="10,3,3", cnn_max_pool_len="3,2,1",
            cnn_use_laynorm_inp="False", cnn_use_batchnorm_inp="False",
            cnn_use_laynorm="False,False,False", cnn_use_batchnorm="False,False,False",
            cnn_act="relu,relu,relu", cnn_drop="0.0,0.0,0.0")
CASES = {
    "ln": dict(BASE, cnn_use_laynorm="True,True,True"),
    "bn": dict(BASE, cnn_use_batchnorm="True,True,True"),
    "none": dict(BASE),
    "ln0": dict(BASE, cnn_use_laynorm_inp="True", cnn_use_laynorm="True,True,True"),
    "bn0": dict(BASE, cnn_use_batchnorm_inp="True", cnn_use_batchnorm="True,True,True"),
    "leaky": dict(BASE, cnn_act="leaky_relu,leaky_relu,leaky_relu",
                  cnn_use_laynorm="True,True,True"),
}


def main(ref):
    sys.path.insert(0, ref)
    torch.Tensor.cuda = lambda t, *a, **k: t          # noqa: E731  (CPU-only)
    import neural_networks                             # noqa: E402
    out = {"cases": np.array(json.dumps(CASES)), "seed": np.int64(SEED), "inp_dim": np.int64(INP)}
    for name, opts in CASES.items():
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        net = neural_networks.CNN(opts, INP)
        net.train()
        sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
        out[name + "/keys"] = np.array(json.dumps(list(sd0.keys())))
        for k, v in sd0.items():
            out["%s/sd/%s" % (name, k)] = v.numpy()
        rs = np.random.RandomState(11)
        x = torch.from_numpy(rs.randn(BATCH, INP).astype(np.float32)).requires_grad_(True)
        r = torch.from_numpy(rs.randn(BATCH, net.out_dim).astype(np.float32))
        y = net(x)
        (y * r).sum().backward()
        out[name + "/out_dim"] = np.int64(net.out_dim)
        out[name + "/x"], out[name + "/r"] = x.detach().numpy(), r.numpy()
        out[name + "/y"], out[name + "/dx"] = y.detach().numpy(), x.grad.numpy()
        for k, p in net.named_parameters():
            out["%s/grad/%s" % (name, k)] = (p.grad if p.grad is not None
                                             else torch.zeros_like(p)).numpy()
        for k, v in net.state_dict().items():          # after the one training forward
            if "running_" in k or "num_batches" in k:
                out["%s/after/%s" % (name, k)] = v.numpy()
    path = os.path.join(OUT, "cnn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

"""Regenerate tests/golden/cudnn.npz from the reference's LSTM_cudnn / GRU_cudnn / RNN_cudnn on CPU.

Usage: python tests/golden/make_golden_cudnn.py <path of the reference checkout>

Data only: for every case the options, the initial state dict (seed 5), an input x (T, B, 11), the
training-mode output (dropout = 0), the gradients of every parameter and of x under the fixed linear
loss (y * r).sum() with a recorded r, and the eval-mode output.  The reference is imported the way
make_golden_cnn.py does (CPU-only: Tensor.cuda is the identity).

The reference classes hand strtobool's ints to nn.LSTM(bias=..., bidirectional=...), which current
torch refuses inside _VF.lstm; the generator coerces bias, bidirectional and batch_first of the
wrapped nn.* INSTANCE to bool — the least the reference needs to run at all.
"""
import json
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

SEED = 5
INP = 11


def _case(cls, H, B, T, layers, bidir, bias, nonlinearity=None):
    o = dict(hidden_size=str(H), num_layers=str(layers), bias=str(bias), batch_first="False",
             dropout="0.0", bidirectional=str(bidir))
    if nonlinearity is not None:
        o["nonlinearity"] = nonlinearity
    return dict(cls=cls, B=B, T=T, opts=o)


# every value of the issue's grid appears: H 20 (a partial 16-column tile) and 48 (three tiles),
# B 3 and 17 (crosses the 16-row tile), T 1 and 7, 1 and 2 layers, both directions, with and
# without bias, tanh and relu; both bidirectional 2-layer cases of a cell at B = 17
CASES = {}
for _c, _nl in (("LSTM_cudnn", (None, None, None, None)), ("GRU_cudnn", (None, None, None, None)),
                ("RNN_cudnn", ("tanh", "relu", "tanh", "relu"))):
    _p = _c.split("_")[0].lower()
    CASES[_p + "_a"] = _case(_c, 20, 3, 7, 1, False, True, _nl[0])
    CASES[_p + "_b"] = _case(_c, 48, 3, 7, 1, False, False, _nl[1])
    CASES[_p + "_c"] = _case(_c, 20, 17, 7, 2, True, True, _nl[2])
    CASES[_p + "_d"] = _case(_c, 20, 17, 1, 2, True, False, _nl[3])


def main(ref):
    sys.path.insert(0, ref)
    torch.Tensor.cuda = lambda t, *a, **k: t          # noqa: E731  (CPU-only)
    import neural_networks                             # noqa: E402
    out = {"cases": np.array(json.dumps(CASES)), "seed": np.int64(SEED), "inp_dim": np.int64(INP)}
    for name, case in CASES.items():
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        net = getattr(neural_networks, case["cls"])(case["opts"], INP)
        inner = getattr(net, case["cls"].split("_")[0].lower())[0]
        for k in ("bias", "bidirectional", "batch_first"):
            setattr(inner, k, bool(getattr(inner, k)))
        net.train()
        sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
        out[name + "/keys"] = np.array(json.dumps(list(sd0.keys())))
        for k, v in sd0.items():
            out["%s/sd/%s" % (name, k)] = v.numpy()
        rs = np.random.RandomState(13)
        T, B = case["T"], case["B"]
        x = torch.from_numpy(rs.randn(T, B, INP).astype(np.float32)).requires_grad_(True)
        r = torch.from_numpy(rs.randn(T, B, int(net.out_dim)).astype(np.float32))
        y = net(x)
        (y * r).sum().backward()
        out[name + "/out_dim"] = np.int64(net.out_dim)
        out[name + "/x"], out[name + "/r"] = x.detach().numpy(), r.numpy()
        out[name + "/y"], out[name + "/dx"] = y.detach().numpy(), x.grad.numpy()
        for k, p in net.named_parameters():
            out["%s/grad/%s" % (name, k)] = p.grad.numpy()
        net.eval()
        with torch.no_grad():
            out[name + "/y_eval"] = net(x.detach()).numpy()
    path = os.path.join(OUT, "cudnn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

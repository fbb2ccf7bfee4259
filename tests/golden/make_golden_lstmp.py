"""Regenerate tests/golden/lstmp.npz from torch.nn.LSTM(proj_size=P) in float32 on the CPU.

Usage: python tests/golden/make_golden_lstmp.py

Data only, and nothing but torch is needed: the reference's LSTM_cudnn is a bare nn.LSTM call that
forwards no proj_size, so the pin of the projected LSTM is torch.nn.LSTM itself.  For every case the
options, the initial state dict (seed 5, keys under the class's prefix lstm.0.), an input x
(T, B, 11), the training-mode output (dropout = 0), the gradients of every parameter and of x under
the fixed linear loss (y * r).sum() with a recorded r, and the eval-mode output.
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
PREFIX = "lstm.0."


def _case(H, P, B, T, layers, bidir, bias):
    o = dict(hidden_size=str(H), proj_size=str(P), num_layers=str(layers), bias=str(bias),
             batch_first="False", dropout="0.0", bidirectional=str(bidir))
    return dict(cls="LSTM_cudnn", B=B, T=T, opts=o)


# (c): B = 17 makes two row tiles and P = 20 is ragged against the 16-column tile
CASES = {"lstmp_a": _case(20, 8, 5, 6, 1, False, True),
         "lstmp_b": _case(20, 8, 5, 6, 2, True, True),
         "lstmp_c": _case(48, 20, 17, 6, 2, True, True),
         "lstmp_d": _case(20, 8, 5, 6, 1, True, False)}


def main():
    out = {"cases": np.array(json.dumps(CASES)), "seed": np.int64(SEED), "inp_dim": np.int64(INP)}
    for name, case in CASES.items():
        o = case["opts"]
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        bidir = o["bidirectional"] == "True"
        net = torch.nn.LSTM(INP, int(o["hidden_size"]), num_layers=int(o["num_layers"]),
                            bias=o["bias"] == "True", dropout=0.0, bidirectional=bidir,
                            proj_size=int(o["proj_size"]))
        net.train()
        sd0 = {PREFIX + k: v.detach().clone() for k, v in net.state_dict().items()}
        out[name + "/keys"] = np.array(json.dumps(list(sd0.keys())))
        for k, v in sd0.items():
            out["%s/sd/%s" % (name, k)] = v.numpy()
        rs = np.random.RandomState(13)
        T, B = case["T"], case["B"]
        D = int(o["proj_size"]) * (2 if bidir else 1)
        x = torch.from_numpy(rs.randn(T, B, INP).astype(np.float32)).requires_grad_(True)
        r = torch.from_numpy(rs.randn(T, B, D).astype(np.float32))
        y = net(x)[0]
        (y * r).sum().backward()
        out[name + "/out_dim"] = np.int64(D)
        out[name + "/x"], out[name + "/r"] = x.detach().numpy(), r.numpy()
        out[name + "/y"], out[name + "/dx"] = y.detach().numpy(), x.grad.numpy()
        for k, p in net.named_parameters():
            out["%s/grad/%s%s" % (name, PREFIX, k)] = p.grad.numpy()
        net.eval()
        with torch.no_grad():
            out[name + "/y_eval"] = net(x.detach())[0].numpy()
    path = os.path.join(OUT, "lstmp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

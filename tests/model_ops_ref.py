"""The reference's forward_model (utils.py:1884-2050) restated WITH its tensor operations on
produced outputs, on oracle.nets modules: tests/joint_ref.py's forward_model extended with
concatenate, mult, avg, sum_constant and the tensor meanings of sum / mult_constant (the scalar
ones, over cost names, are the same Python expressions).  tests/test_model_ops_cpu.py pins this
file against the reference's own run (tests/golden/model_ops/*.npz); the GPU tests lean on it.
Test infrastructure only."""
import numpy as np
import torch

from oracle.nets import nll_err


def forward_model(lines, nets, seq, fea_cols, lab_cols, inp, max_len=0, batch=0, forward_outs=None):
    """utils.py:1884-2050.  seq: {arch: bool}; fea_cols: {fea: (c0, c1)}; lab_cols: {lab: col};
    forward_outs: forward mode, stop after the last of these names (utils.py:1932, 2017, ...)."""
    outs = {}
    for fea, (c0, c1) in fea_cols.items():         # utils.py:1891-1896
        outs[fea] = inp[..., c0:c1]
    for out_name, op, a, b in lines:
        if op == "compute":
            x = outs[b]
            if not seq[a] and x.dim() == 3:        # utils.py:1912-1913, 1924-1925
                x = x.reshape(max_len * batch, -1)
            if seq[a] and x.dim() == 2:            # utils.py:1917-1918, 1927-1928
                x = x.reshape(max_len, batch, -1)
            if b not in fea_cols:
                outs[b] = x                        # (the reference re-views the stored output)
            outs[out_name] = nets[a](x)
        elif op in ("cost_nll", "cost_err"):
            if forward_outs is not None:
                continue
            lab = inp[..., lab_cols[b]].reshape(-1)
            o = outs[a]
            o = o.reshape(-1, o.shape[-1])
            loss, err = nll_err(o, lab)
            outs[out_name] = loss if op == "cost_nll" else err
        elif op == "concatenate":                  # utils.py:2014-2016: along the last axis
            outs[out_name] = torch.cat((outs[a], outs[b]), outs[a].dim() - 1)
        elif op == "mult":                         # utils.py:2020-2021
            outs[out_name] = outs[a] * outs[b]
        elif op == "sum":                          # utils.py:2025-2026
            outs[out_name] = outs[a] + outs[b]
        elif op == "mult_constant":                # utils.py:2030-2031
            outs[out_name] = outs[a] * float(b)
        elif op == "sum_constant":                 # utils.py:2035-2036
            outs[out_name] = outs[a] + float(b)
        elif op == "avg":                          # utils.py:2040-2041
            outs[out_name] = (outs[a] + outs[b]) / 2
        else:
            raise NotImplementedError(op)
        if forward_outs is not None and out_name == forward_outs[-1]:
            break
    return outs


def train_step(lines, nets, opts, seq, fea_cols, lab_cols, inp, max_len=0, batch=0):
    """core.py:216-232."""
    outs = forward_model(lines, nets, seq, fea_cols, lab_cols, inp, max_len, batch)
    for o in opts.values():
        o.zero_grad()
    outs["loss_final"].backward()
    for o in opts.values():
        o.step()
    return outs


def build(archs, dims, dtype=torch.float32, train=True, state=None):
    """({arch: oracle net}, {arch: optimizer}, {arch: seq?}) of a model_ops_cfg architecture set;
    state: {arch: state dict} to start from."""
    from oracle import nets as ON
    nets, opts, seq = {}, {}, {}
    for a, o in archs.items():
        torch.manual_seed(11)
        np.random.seed(11)
        net = getattr(ON, o["arch_class"])(o, dims[a])
        if state is not None:
            net.load_state_dict(state[a])
        net = net.to(dtype)
        net.train() if train else net.eval()
        nets[a], seq[a] = net, o["arch_seq_model"] == "True"
        opts[a] = ON.make_optimizer(net.parameters(), o)
    return nets, opts, seq


def golden_state(g, archs):
    """{arch: state dict} stored by make_golden_model_ops.py under init/<arch>/<key>."""
    out = {}
    for a in archs:
        pre = "init/%s/" % a
        out[a] = {k[len(pre):]: torch.from_numpy(np.asarray(g[k])) for k in g.files
                  if k.startswith(pre)}
    return out

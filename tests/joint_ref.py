"""The joint speech-enhancement + recognition model restated for the tests: the reference's
forward_model (utils.py:1884-2050) WITH the mse operation (utils.py:2045-2048), on oracle.nets
modules — oracle.run.forward_model covers the operations of the other recipes and raises on mse.
Plus the batch body and the sentence-batch loop of core.run_nn (core.py:157-252) for a sequence
model, so a whole chunk can be replayed on the CPU (tests/test_joint_cpu.py pins this file against
the reference's own run; the GPU tests lean on it).  Test infrastructure only."""
import numpy as np
import torch

from oracle.nets import nll_err


def forward_model(lines, nets, seq, fea_cols, lab_cols, inp, max_len=0, batch=0, forward_outs=None):
    """utils.py:1884-2050.  seq: {arch: bool}; fea_cols: {fea: (c0, c1)}; lab_cols: {lab: col};
    forward_outs: forward mode, stop after the last of these names (utils.py:1932)."""
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
        elif op == "sum":
            outs[out_name] = outs[a] + outs[b]
        elif op == "mult_constant":
            outs[out_name] = outs[a] * float(b)
        elif op == "mse":                          # utils.py:2045-2046: over every element
            ya, yb = outs[a], outs[b]
            outs[out_name] = torch.mean((ya.reshape(-1, ya.shape[-1]) -
                                         yb.reshape(-1, yb.shape[-1])) ** 2)
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


def seq_batch(data_set, end_index, snt, B, rng):
    """core.py:183-200: sentences snt .. snt+B-1 of the chunk matrix padded to the longest, each
    after a random number of leading zero rows (rng: python's random, in the reference's draw
    order).  Returns (inp (T, B, cols), T, left pads)."""
    end = np.asarray(end_index)
    lens = np.diff(np.concatenate([[0], end]))
    T = int(lens[snt:snt + B].max())
    inp = torch.zeros(T, B, data_set.shape[1], dtype=data_set.dtype)
    lefts = []
    for k in range(B):
        n = int(lens[snt + k])
        left = rng.randint(0, T - n)
        b0 = int(end[snt + k]) - n
        inp[left:left + n, k] = data_set[b0:b0 + n]
        lefts.append(left)
    return inp, T, lefts


def unpack(g, prefix):
    """{key: rows} of a pack_dict'ed group of the golden npz."""
    keys, lens, data = g[prefix + "_keys"], g[prefix + "_lens"], g[prefix + "_data"]
    out, pos = {}, 0
    for k, n in zip(keys, lens):
        out[str(k)] = data[pos:pos + n]
        pos += n
    return out


def golden_chunk(g, tag):
    """The chunk matrix the reference's read_lab_fea builds from the golden utterances of chunk
    `tag` (streams in the order the [model] first names them): (names, end_index, fea_cols,
    lab_cols, float32 matrix as core.py:96 casts it)."""
    from oracle import loader as OL
    streams = [("fbank_rev", unpack(g, tag + "_rev"), 0, 0),
               ("fbank_clean", unpack(g, tag + "_clean"), 0, 0)]
    labels = [("lab_cd", unpack(g, tag + "_cd")), ("lab_mono", unpack(g, tag + "_mono"))]
    names, end, fea_cols, lab_cols, ds = OL.read_lab_fea(streams, labels, True)
    return names, end, fea_cols, lab_cols, torch.from_numpy(ds).float()


def build_nets(dtype=torch.float32, to_do="train"):
    """The recipe's five oracle.nets modules and their optimizers: ({arch: net}, {arch: opt},
    {arch: seq?}, {arch: options})."""
    from joint_cfg import FEA_DIM, arch_sections
    from oracle import nets as ON
    nets, opts, seq, o_by = {}, {}, {}, {}
    dims = {"liGRU_SE": FEA_DIM, "MLP_SE": 24, "liGRU_SR": FEA_DIM, "MLP_layers": 24,
            "MLP_layers2": 24}
    for sec, o in arch_sections(to_do=to_do).items():
        a = o["arch_name"]
        torch.manual_seed(5)
        np.random.seed(5)
        net = getattr(ON, o["arch_class"])(o, dims[a]).to(dtype)
        net.train() if to_do == "train" else net.eval()
        nets[a], seq[a], o_by[a] = net, o["arch_seq_model"] == "True", o
        opts[a] = ON.make_optimizer(net.parameters(), o)
    return nets, opts, seq, o_by


def load_checkpoints(nets, opts, o_by, pkls, pnames):
    """core.py:114-121 from reference-written checkpoints: pkls {arch: path}, pnames {arch:
    parameter names in the checkpoint's optimizer order} (the oracle classes may register their
    parameters in another order)."""
    for a, net in nets.items():
        ck = torch.load(pkls[a], weights_only=True, map_location="cpu")
        net.load_state_dict(ck["model_par"])
        if opts is None:
            continue
        sd = ck["optimizer_par"]
        where = {n: i for i, (n, _) in enumerate(net.named_parameters())}
        state = {where[str(pnames[a][i])]: {k: (v.detach().clone() if torch.is_tensor(v) else v)
                                            for k, v in st.items()}
                 for i, st in sd["state"].items()}
        group = dict(sd["param_groups"][0])
        group["params"] = list(range(len(where)))
        opts[a].load_state_dict({"state": state, "param_groups": [group]})
        opts[a].param_groups[0]["lr"] = float(o_by[a]["arch_lr"])


def replay_ck1(g, pkls, dtype=torch.float32, seed=2234):
    """The reference's `train ck1 resumed from the ck0 checkpoints` call restated: returns
    ({arch: net}, {arch: opt}, (loss, err)) after the chunk."""
    import random

    from joint_cfg import ARCHS, MODEL
    from oracle.run import parse_model
    _, end, fea_cols, lab_cols, ds = golden_chunk(g, "ck1")
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)         # (the oracle's recurrent layers start from torch.zeros)
    try:
        nets, opts, seq, o_by = build_nets(dtype)
        load_checkpoints(nets, opts, o_by, pkls, {a: g["pnames/" + a] for a in ARCHS})
        info = run_chunk(parse_model(MODEL), nets, opts, seq, fea_cols, lab_cols, ds.to(dtype), end,
                         3, "train", random.Random(seed))
    finally:
        torch.set_default_dtype(old)
    return nets, opts, info


def run_chunk(lines, nets, opts, seq, fea_cols, lab_cols, data_set, end_index, B, to_do, rng):
    """The sentence-batch loop of core.run_nn over one chunk (core.py:157-252): returns the
    chunk's (mean loss_final, mean err_final) as the .info reports them (core.py:338-345)."""
    n_batches = len(end_index) // B
    loss_sum = err_sum = 0.0
    for i in range(n_batches):
        inp, T, _ = seq_batch(data_set, end_index, i * B, B, rng)
        if to_do == "train":
            outs = train_step(lines, nets, opts, seq, fea_cols, lab_cols, inp, T, B)
        else:
            with torch.no_grad():
                outs = forward_model(lines, nets, seq, fea_cols, lab_cols, inp, T, B)
        loss_sum += float(outs["loss_final"].detach())
        err_sum += float(outs["err_final"].detach())
    return loss_sum / n_batches, err_sum / n_batches

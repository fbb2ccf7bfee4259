"""The engine-level case of the *_cudnn architectures, shared by tests/test_cudnn_cpu.py and
tests/test_gpu_cudnn.py: `o1=compute(rnn,fea)` into two softmax heads (the [model] of
tests/test_gpu_seq.py::make_cfg), hidden 32, 2 bidirectional layers, dropout 0.2 with injected masks,
F = 20, B = 4, max_len 16, the padded batches of Engine.next_seq_batch, three training steps; and the
CPU side of it — the plain-torch restatement (tests/cudnn_ref.py) with the oracle's MLP heads."""
import configparser
import random

import numpy as np
import torch

import cudnn_ref as R

F, B, MAX_LEN, HID, LAYERS, DROP = 20, 4, 16, 32, 2, 0.2
CLASSES = ("LSTM_cudnn", "GRU_cudnn", "RNN_cudnn")
SEED = 3            # parameter init; DATA_SEED: sentences, labels and dropout masks
DATA_SEED = 0
MODEL = ("o1=compute(rnn,fea)\no2=compute(head,o1)\no3=compute(mono,o1)\n"
         "lm=cost_nll(o3,lab_mono)\nlmw=mult_constant(lm,1.0)\nlc=cost_nll(o2,lab_cd)\n"
         "loss_final=sum(lc,lmw)\nerr_final=cost_err(o2,lab_cd)")


def make_cfg(cls, optk="rmsprop", dropout=DROP, **over):
    cfg = configparser.ConfigParser()
    if optk == "rmsprop":
        opt = dict(arch_opt="rmsprop", arch_lr="0.0016", opt_momentum="0.0", opt_alpha="0.95",
                   opt_eps="1e-8", opt_centered="False", opt_weight_decay="0.0", arch_freeze="False")
    else:
        opt = dict(arch_opt="sgd", arch_lr="0.08", opt_momentum="0.0", opt_weight_decay="0.0",
                   opt_dampening="0.0", opt_nesterov="False", arch_freeze="False")
    a1 = dict(arch_name="rnn", arch_class=cls, hidden_size=str(HID), num_layers=str(LAYERS),
              bias="True", batch_first="False", dropout=str(dropout), bidirectional="True",
              to_do="train", **opt)
    if cls == "RNN_cudnn":
        a1["nonlinearity"] = "tanh"
    a1.update(over)
    cfg["a1"] = a1
    head = dict(dnn_use_laynorm_inp="False", dnn_use_batchnorm_inp="False", to_do="train",
                arch_name="head", dnn_lay="64", dnn_drop="0.0", dnn_use_batchnorm="False",
                dnn_use_laynorm="False", dnn_act="softmax", **opt)
    cfg["a2"] = head
    cfg["a3"] = dict(head, arch_name="mono", dnn_lay="8",
                     arch_lr="0.0004" if optk == "rmsprop" else "0.08")
    cfg["model"] = {"model": MODEL}
    return cfg


def make_data():
    rs = np.random.RandomState(DATA_SEED)
    lens = np.sort(rs.randint(5, 13, size=12))
    end = np.cumsum(lens)
    X = rs.randn(end[-1], F).astype(np.float32)
    lab = np.stack([rs.randint(0, 64, end[-1]), rs.randint(0, 8, end[-1])], 1).astype(np.int32)
    # keep masks of the layers below the last, (MAX_LEN, B, D): a batch padded to T reads [:T]
    masks = {("rnn", l): torch.from_numpy((rs.rand(MAX_LEN, B, 2 * HID) > DROP).astype(np.uint8))
             for l in range(LAYERS - 1)}
    return lens, end, X, lab, masks


def build(cfg, mods, dtype=torch.float32):
    """{arch: net} from the module set `mods` (a pkc.neural_networks-like namespace for the
    architecture and the heads), the reference's init draws under SEED."""
    nets, opts = {}, {}
    for sec in ("a1", "a2", "a3"):
        o = cfg[sec]
        inp = F if sec == "a1" else nets["rnn"].out_dim
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        cls = o["arch_class"] if sec == "a1" else "MLP"
        nets[o["arch_name"]] = getattr(mods[0] if sec == "a1" else mods[1], cls)(o, inp).to(dtype)
        opts[o["arch_name"]] = o
    return nets, opts


def oracle_nets(cfg, dtype=torch.float32):
    from oracle import nets as ON
    nets, opts = build(cfg, (R, ON), dtype)
    for n in nets.values():
        n.train()
    oopt = {k: ON.make_optimizer(nets[k].parameters(), opts[k]) for k in nets}
    return nets, opts, oopt


def batches(lens, end, X, lab, steps=3):
    """The first `steps` padded batches as core.py:183-200 assembles them (python Random(7))."""
    rng, snt, out = random.Random(7), 0, []
    for _ in range(steps):
        T = int(lens[snt:snt + B].max())
        inp = torch.zeros(T, B, F + 2)
        lefts = []
        for k in range(B):
            n = int(lens[snt])
            left = rng.randint(0, T - n)
            b0 = int(end[snt] - n)
            inp[left:left + n, k, :F] = torch.from_numpy(X[b0:b0 + n])
            inp[left:left + n, k, F:] = torch.from_numpy(lab[b0:b0 + n].astype(np.float32))
            lefts.append(left)
            snt += 1
        out.append((inp, T, lefts))
    return out


def oracle_step(nets, oopt, inp, T, masks, train=True):
    """One run_nn training step (or, train=False, the forward alone) of the restatement side."""
    from oracle import run as OR
    body = nets["rnn"]
    f = body.forward
    keep = {l: masks[("rnn", l)][:T].to(inp.device) for l in range(LAYERS - 1)}
    body.forward = lambda x, _f=f: _f(x, keep=keep)
    try:
        lines = OR.parse_model(MODEL)
        seq = {"rnn": True, "head": False, "mono": False}
        cols = ({"fea": (0, F)}, {"lab_cd": F, "lab_mono": F + 1})
        if train:
            return OR.train_step(lines, nets, oopt, seq, cols[0], cols[1], inp, T, B)
        with torch.no_grad():
            return OR.forward_model(lines, nets, seq, cols[0], cols[1], inp, T, B)
    finally:
        body.forward = f


def check_update(step, optk, opts, got_sd, ref_sd, report):
    """tests/test_gpu_seq.py's fp32 rule on one step's parameters: within 1e-4 of the tensor's
    scale, with no outlier under SGD; under RMSprop at most 2 % of a tensor's elements counted as
    sign steps, each <= 2 * 4.48 lr."""
    from flipcheck import assert_counted, step_outliers
    for k in got_sd:
        lr = float(opts[k]["arch_lr"])
        for name, v in got_sd[k].items():
            ref = ref_sd[k][name].double()
            scale = max(float(ref.abs().max()), lr)
            n, dmax, _ = step_outliers(v.cpu(), ref, 1e-4, scale)
            report["%d %s/%s" % (step, k, name)] = (n, round(dmax / scale, 6))
            if optk == "sgd":
                assert n == 0, "step %d %s %s: %d of %d elements beyond 1e-4 of the scale (max %.3g)" % (
                    step, k, name, n, ref.numel(), dmax / scale)
            else:
                assert_counted("step %d %s %s" % (step, k, name), n, ref.numel(), 0.02, dmax,
                               2 * 4.48 * lr + 1e-7)

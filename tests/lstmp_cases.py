"""The engine-level case of the projected LSTM (LSTM_cudnn with proj_size = 12), shared by
tests/test_lstmp_cpu.py and tests/test_gpu_lstmp.py: the case of tests/cudnn_cases.py — `o1=compute(rnn,
fea)` into two softmax heads, hidden 32, 2 bidirectional layers, dropout 0.2 with injected masks,
F = 20, B = 4, max_len 16, the same seeds, sentences and padded batches, three training steps — with
the keep masks cut to the 2 P columns of a layer's output, and the plain-torch restatement
tests/lstmp_ref.py on the CPU side."""
import torch

import cudnn_cases as CC
import lstmp_ref as R

F, B, MAX_LEN, HID, LAYERS, DROP = CC.F, CC.B, CC.MAX_LEN, CC.HID, CC.LAYERS, CC.DROP
PROJ = 12
MODEL = CC.MODEL
build, batches, oracle_step, check_update = CC.build, CC.batches, CC.oracle_step, CC.check_update


def make_cfg(optk="rmsprop", dropout=DROP, proj=PROJ, **over):
    return CC.make_cfg("LSTM_cudnn", optk, dropout, proj_size=str(proj), **over)


def make_data(proj=PROJ):
    lens, end, X, lab, masks = CC.make_data()
    return lens, end, X, lab, {k: v[:, :, :2 * proj].contiguous() for k, v in masks.items()}


def oracle_nets(cfg, dtype=torch.float32):
    from oracle import nets as ON
    nets, opts = build(cfg, (R, ON), dtype)
    for n in nets.values():
        n.train()
    oopt = {k: ON.make_optimizer(nets[k].parameters(), opts[k]) for k in nets}
    return nets, opts, oopt

"""Worker and shared builders of tests/test_gpu_seq_syncbn.py (not collected by pytest): one rank
of sequence-model data parallelism with SyncBN over the recurrent layers' gate BatchNorms,
launched by torch.distributed.run with the gloo backend (the ranks share the one GPU; on a node the
same code runs over RCCL).

The rank builds the small recurrent model of make_cfg (F = 24, two layers of H = 48 — no multiple
of the 64-column tile —, cd head 11, mono head 5, dropout 0, RMSprop) from the common seeds, takes
its round-robin share of the chunk of `chunk` (pkc.dist.shard_sentences, as pkc.core.run_nn does),
gets the chunk's loss scales and global row counts in ONE collective (pkc.dist.frame_rows) and
trains STEPS sentence batches of B sentences with the gradient all-reduce.  It saves its
parameters and buffers, its summed loss, the collective counts and, per BatchNorm'd layer and gate
of the last step, save_mean / save_invstd / xhat / dz.

argv: out_dir family (lstm | ligru | gru | minimalgru | rnn) mode (sync | nosync) lens (equal |
unequal) prec (fp32 | bf16) body (rec | mlp)
"""
import configparser
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-kaldi-cgs_amd"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

F, H, B, STEPS, NCD, NMONO = 24, 48, 2, 3, 11, 5
FAMILIES = {"lstm": "LSTM", "ligru": "liGRU", "gru": "GRU", "minimalgru": "minimalGRU",
            "rnn": "RNN"}


def make_cfg(family, body="rec", inp_bn=False):
    """lstm / minimalgru: unidirectional; ligru / gru / rnn: the shared-weight bidirectional form.
    body="mlp": a BatchNorm'd MLP layer of 40 units between the recurrent arch and the heads."""
    from cases import GRU_DEF, LIGRU_DEF, LSTM_DEF, MINGRU_DEF, RNN_DEF
    opt = dict(arch_opt="rmsprop", arch_lr="0.0016", opt_momentum="0.0", opt_alpha="0.95",
               opt_eps="1e-8", opt_centered="False", opt_weight_decay="0.0", arch_freeze="False")
    lay = "%d,%d" % (H, H)
    cfg = configparser.ConfigParser()
    if family == "lstm":
        a1 = dict(LSTM_DEF, lstm_lay=lay, lstm_drop="0.0,0.0", lstm_bidir="False")
    elif family == "ligru":
        a1 = dict(LIGRU_DEF, ligru_lay=lay, ligru_drop="0.0,0.0", ligru_bidir="True")
    elif family == "gru":
        a1 = dict(GRU_DEF, gru_lay=lay, gru_drop="0.0,0.0", gru_bidir="True")
    elif family == "minimalgru":
        a1 = dict(MINGRU_DEF, minimalgru_lay=lay, minimalgru_drop="0.0,0.0",
                  minimalgru_bidir="False")
    else:
        a1 = dict(RNN_DEF, rnn_lay=lay, rnn_drop="0.0,0.0", rnn_bidir="True", rnn_act="tanh,relu")
    if inp_bn:
        a1[family + "_use_batchnorm_inp"] = "True"
    cfg["a1"] = dict(a1, arch_name="rnn", **opt)
    head = dict(dnn_use_laynorm_inp="False", dnn_use_batchnorm_inp="False", to_do="train",
                arch_name="head", dnn_lay=str(NCD), dnn_drop="0.0", dnn_use_batchnorm="False",
                dnn_use_laynorm="False", dnn_act="softmax", **opt)
    cfg["a2"] = head
    cfg["a3"] = dict(head, arch_name="mono", dnn_lay=str(NMONO), arch_lr="0.0004")
    src = "o1"
    model = "o1=compute(rnn,fea)\n"
    if body == "mlp":
        cfg["a4"] = dict(head, arch_name="body", dnn_lay="40", dnn_use_batchnorm="True",
                         dnn_act="relu")
        model += "ob=compute(body,o1)\n"
        src = "ob"
    model += ("o2=compute(head,%s)\no3=compute(mono,%s)\nlm=cost_nll(o3,lab_mono)\n"
              "lc=cost_nll(o2,lab_cd)\nloss_final=sum(lc,lm)\nerr_final=cost_err(o2,lab_cd)"
              % (src, src))
    cfg["model"] = {"model": model}
    return cfg


def build_nets(cfg, family, device="cuda"):
    """The architectures of cfg from the common seed, on `device` in training mode."""
    import pkc.neural_networks as NN
    nets, opts = {}, {}
    order = ["a1"] + (["a4"] if "a4" in cfg else []) + ["a2", "a3"]
    for sec in order:
        o = cfg[sec]
        name = o["arch_name"]
        inp = F if sec == "a1" else (nets["rnn"].out_dim if sec == "a4" or "a4" not in cfg
                                     else nets["body"].out_dim)
        torch.manual_seed(3)
        np.random.seed(3)
        nets[name] = getattr(NN, FAMILIES[family] if sec == "a1" else "MLP")(o, inp)
        opts[name] = o
    for n in nets.values():
        n.to(device).train()
    return nets, opts


def chunk(world, lens_mode):
    """world * STEPS * B sentences; sentence i belongs to rank i % world (round-robin).  equal:
    every sentence 7 frames, rank 0's features offset by +1 and rank 1's by -1 in every column
    (per-rank and global statistics differ grossly).  unequal: rank 0's sentences 7 frames, rank
    1's 5 (unequal padded T per rank in every step)."""
    rs = np.random.RandomState(29)
    n = world * STEPS * B
    owner = np.arange(n) % world
    lens = np.full(n, 7) if lens_mode == "equal" else np.where(owner == 0, 7, 5)
    end = np.cumsum(lens)
    X = rs.randn(end[-1], F).astype(np.float32)
    off = np.repeat(np.where(owner == 0, 1.0, -1.0), lens).astype(np.float32)
    X += off[:, None] * (1.0 if lens_mode == "equal" else 0.25)
    lab = np.stack([rs.randint(0, NCD, end[-1]), rs.randint(0, NMONO, end[-1])], 1).astype(np.int32)
    return lens, end, X, lab


def build_engine(family, world, batch, sync_bn=None, prec="fp32", body="rec", seed=1,
                 device="cuda", inp_bn=False):
    from pkc import _lib as L
    from pkc.engine import Engine, parse_model
    cfg = make_cfg(family, body, inp_bn)
    nets, opts = build_nets(cfg, family, device)
    eng = Engine(nets, opts, parse_model(cfg["model"]["model"]), {"fea": (0, F)},
                 ["lab_cd", "lab_mono"], batch=batch, max_len=8, seed=seed,
                 grad_scale=1.0 / world, sync_bn=sync_bn, device=device,
                 prec=L.PREC_BF16 if prec == "bf16" else L.PREC_FP32)
    return eng, nets


def state(nets):
    return {a + "/" + k: v.detach().cpu().numpy() for a in nets
            for k, v in nets[a].state_dict().items()}


def bn_gammas(eng):
    """Every BatchNorm's gamma as it stands (called before the last step: what its backward
    multiplies by), keyed as bn_tensors."""
    out = {}
    for n in eng.nodes:
        if n.rec:
            for li, sp in enumerate(n.layers):
                if sp["bn"]:
                    for g in range(n.G):
                        out["bn:%s.%d.%d:gamma" % (n.arch, li, g)] = sp["bnm"][g].weight
        elif n.bn and not n.head and n.W is not None:
            out["bn:%s:gamma" % n.name] = n.gamma
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def bn_tensors(eng):
    """save_mean / save_invstd / xhat / dz of every BatchNorm of the last step and, with SyncBN,
    the all-reduced column sums (sum dy, sum dy * xhat over all ranks' rows) its backward
    applied: recurrent layers per gate ("rnn.<layer>.<gate>"), MLP layers by name."""
    out = {}
    M = eng.M
    for n in eng.nodes:
        if n.rec:
            for li, (sp, lb) in enumerate(zip(n.layers, n.lbuf)):
                if not sp["bn"]:
                    continue
                Hh = lb["H"]
                for g in range(n.G):
                    k = "bn:%s.%d.%d:" % (n.arch, li, g)
                    out[k + "mean"] = lb["sm"][g * Hh:(g + 1) * Hh]
                    out[k + "invstd"] = lb["si"][g * Hh:(g + 1) * Hh]
                    out[k + "xhat"] = lb["xhat"][g * M * Hh:(g + 1) * M * Hh].view(M, Hh)
                    out[k + "dz"] = lb["dz"][g * M * Hh:(g + 1) * M * Hh].view(M, Hh)
                    if lb.get("bn_sums") is not None:
                        out[k + "sums"] = lb["bn_sums"][g * 2 * Hh:(g + 1) * 2 * Hh].view(2, Hh)
        elif n.bn and not n.head and n.W is not None:
            k = "bn:%s:" % n.name
            out[k + "mean"], out[k + "invstd"] = n.save_mean, n.save_invstd
            out[k + "xhat"] = n.xhat[:M * n.N].view(M, n.N)
            out[k + "dz"] = n.dz[:M * n.N].view(M, n.N)
            if n.bn_sums is not None:
                out[k + "sums"] = n.bn_sums.view(2, n.N)
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def main():
    import torch.distributed as dist
    out, family, mode, lens_mode, prec, body = sys.argv[1:7]
    from pkc import dist as DP
    dist.init_process_group("gloo")
    rank, world = DP.world()
    torch.cuda.set_device(0)
    lens, end, X, lab = chunk(world, lens_mode)
    sbn = DP.SyncBatchNorm() if mode == "sync" else None
    eng, nets = build_engine(family, world, B, sync_bn=sbn, prec=prec, body=body)
    eng.bind_chunk(torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda(), end[-1],
                   end_index=end, sentences=DP.shard_sentences(end, rank, world))
    eng.n_batches = DP.agree_min(eng.n_batches, device=eng.dev)
    eng.frame_scales, eng.global_rows = DP.frame_rows(eng.sent_len, eng.B, eng.n_batches,
                                                      device=eng.dev)
    ar = DP.GradAllReduce()
    rng = random.Random(7 + rank)
    T = []
    for step in range(STEPS):
        if step == STEPS - 1:
            torch.cuda.synchronize()
            gammas = bn_gammas(eng)
        b = eng.next_seq_batch(rng)
        T.append(b[3])
        eng.train_step(ar, batch=b)
    torch.cuda.synchronize()
    eng.sync_state()
    # this rank's sum over the steps of its batch-mean loss (with equal row counts the ranks'
    # average is the mean over the global batch's rows)
    loss, err = eng.chunk_totals()
    np.savez(os.path.join(out, "rank%d.npz" % rank), loss=loss, T=np.array(T),
             scales=eng.frame_scales, rows=eng.global_rows,
             bn_calls=0 if sbn is None else sbn.calls, ar_calls=ar.calls,
             **state(nets), **bn_tensors(eng), **gammas)
    dist.destroy_process_group()


def main_run_nn():
    """argv: out_dir run_nn cfg_path — one rank of pkc.core.run_nn on a train chunk cfg, with a
    spy on the Engine it builds (what sync_bn it was given)."""
    import json

    import torch.distributed as dist
    out, cfg_path = sys.argv[1], sys.argv[3]
    import pkc.core as core
    from pkc import dist as DP
    dist.init_process_group("gloo")
    rank, world = DP.world()
    torch.cuda.set_device(0)
    seen = []
    real = core.Engine

    def spy(*a, **kw):
        eng = real(*a, **kw)
        seen.append(eng)
        return eng

    core.Engine = spy
    core.run_nn(None, None, None, None, None, None, cfg_path, True, cfg_path)
    sbn = seen[0].sync_bn
    with open(os.path.join(out, "run_nn_rank%d.json" % rank), "w") as f:
        json.dump({"world": world, "sync_bn": type(sbn).__name__ if sbn is not None else None,
                   "bn_calls": 0 if sbn is None else sbn.calls,
                   "steps": seen[0].steps_done, "seq": bool(seen[0].seq)}, f)
    dist.destroy_process_group()


if __name__ == "__main__":
    main_run_nn() if sys.argv[2] == "run_nn" else main()

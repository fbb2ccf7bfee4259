"""SyncBN over the recurrent layers' gate BatchNorms under sequence data parallelism (SURVEY 8e's
parity recipe: R = 1 vs R > 1 on the same global batch with SyncBN on and dropout 0).

Two gloo ranks share the one GPU (tests/dp_seq_syncbn_worker.py; on a node the same code runs over
RCCL).  F = 24, two layers of H = 48 (no multiple of the 64-column tile), B = 2 sentences per rank,
dropout 0, RMSprop, cd head 11, mono head 5, three training steps.
"""
import configparser
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKER = os.path.join(ROOT, "tests", "dp_seq_syncbn_worker.py")
EPS = 1e-5                       # the engine's BatchNorm eps
U = 2.0 ** -23                   # float32 unit roundoff of a sum's term (the issue's bound)
_FAILED = []                     # a launch that exited non-zero: nothing more is started


def _launch(out, *args, port=0):
    """One two-rank launch under its own time limit; after a non-zero exit no further launch."""
    if _FAILED:
        pytest.fail("not started: an earlier two-rank launch failed (%s)" % _FAILED[0])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run",
           "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(29500 + (os.getpid() * 7 + port) % 1000), WORKER, str(out)] + [str(a) for a in args]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        _FAILED.append("%s: exit %d" % (" ".join(str(a) for a in args), r.returncode))
    assert r.returncode == 0, r.stderr[-4000:]


def _ranks(out):
    return [np.load(os.path.join(out, "rank%d.npz" % k)) for k in range(2)]


@functools.lru_cache(maxsize=None)
def _one_process(family, prec, split=False):
    """The single-process Engine on the whole global batch (2B sentences per step, the two ranks'
    union), three steps: (summed loss, state).  split: the same run with a one-rank SyncBN armed —
    its only change is the gate BatchNorms' summation split (statistics pass, merge, apply in
    place of the fused small-batch launch)."""
    import random

    import dp_seq_syncbn_worker as W
    lens, end, X, lab = W.chunk(2, "equal")
    eng, nets = W.build_engine(family, 1, 2 * W.B, prec=prec, sync_bn=_World1() if split else None)
    eng.bind_chunk(torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda(), end[-1], end_index=end)
    rng = random.Random(7)
    for _ in range(W.STEPS):
        eng.train_step(batch=eng.next_seq_batch(rng))
    torch.cuda.synchronize()
    eng.sync_state()
    return eng.chunk_totals()[0], W.state(nets)


# Families that need more than rtol 1e-4 / atol 1e-6 on the weights: in units of
# atol + rtol |ref|, the worst (two ranks vs one process, one process with only the gate summation
# split changed vs one process) as measured on an MI355X; the bound is twice the larger.  In both
# runs 1 or 2 elements of a layer-1 input weight (of 2304 / 4608) exceed 1: RMSprop's first steps
# divide a near-zero gradient element by its own magnitude, so its rounding shows at full size.
MEASURED = {("lstm", "fp32"): (2.0104, 0.9973), ("ligru", "fp32"): (1.5573, 2.7516)}


def _bounds(family, prec):
    # test_dp_engine_two_ranks_equal_full_batch's: (weights rtol, atol, loss rtol)
    rtol, atol, ltol = (1e-2, 1e-3, 1e-3) if prec == "bf16" else (1e-4, 1e-6, 1e-5)
    widen = 2 * max(MEASURED.get((family, prec), (0.5, 0.5)))
    return rtol * widen, atol * widen, ltol


CASES = [("lstm", "fp32"), ("ligru", "fp32"), ("gru", "fp32"), ("minimalgru", "fp32"),
         ("rnn", "fp32"), ("ligru", "bf16")]


@pytest.mark.parametrize("family,prec", CASES, ids=["%s-%s" % c for c in CASES])
def test_two_ranks_equal_one_process(family, prec, tmp_path):
    """Every sentence 7 frames (no padding), the ranks' shards offset by +1 / -1 per feature
    column: two ranks with sync_bn equal the single-process Engine on the whole batch after three
    steps — summed loss rtol 1e-5, every weight / BatchNorm gamma, beta and running statistic
    rtol 1e-4, atol 1e-6 (bf16: 1e-3, and 1e-2 / 1e-3), the bounds of
    test_dp_engine_two_ranks_equal_full_batch[syncbn] — and the replicas, running statistics
    included, are bit-identical.

    lstm and ligru (fp32) need more on the weights.  Measured, in units of atol + rtol |ref|:
    two ranks vs one process 2.01 (lstm) and 1.56 (ligru); one process with only the gate
    summation split changed (_one_process(split=True)) vs one process 1.00 (lstm) and 2.75
    (ligru).  Their weight bounds are twice the larger: 4.02 and 5.50 times 1e-4 / 1e-6 (MEASURED
    above).  gru 0.91, minimalgru 0.67, rnn 0.17, ligru bf16 0.02 keep the bounds as they are."""
    import dp_seq_syncbn_worker as W
    _launch(tmp_path, family, "sync", "equal", prec, "rec", port=CASES.index((family, prec)))
    g = _ranks(tmp_path)
    assert int(g[0]["bn_calls"]) == 2 * 2 * W.STEPS      # one collective per layer and pass
    assert (g[0]["T"] == 7).all() and (g[1]["T"] == 7).all()
    np.testing.assert_array_equal(g[0]["rows"], np.full(W.STEPS, 2 * 7 * W.B))
    loss, ref = _one_process(family, prec)
    rtol, atol, ltol = _bounds(family, prec)
    rtol0, atol0, _ = _bounds(None, prec)
    worst = {}
    for k, v in ref.items():
        np.testing.assert_array_equal(g[0][k], g[1][k], err_msg="replicas differ: " + k)
        if k.endswith("num_batches_tracked"):
            continue
        d = np.abs(g[0][k] - v)
        worst[k] = float((d / (atol0 + rtol0 * np.abs(v))).max()) if d.size else 0.0
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print("%s %s: worst |diff| / (atol + rtol |ref|): %s" % (family, prec, top))
    two = (float(g[0]["loss"]) + float(g[1]["loss"])) / 2
    print("%s %s: loss two ranks %.8g one process %.8g" % (family, prec, two, loss))
    np.testing.assert_allclose(two, loss, rtol=ltol)
    for k, v in ref.items():
        if not k.endswith("num_batches_tracked"):
            np.testing.assert_allclose(g[0][k], v, rtol=rtol, atol=atol, err_msg=k)


@pytest.mark.parametrize("family", ["lstm", "ligru"])
def test_two_ranks_without_sync_bn_miss_the_bound(family, tmp_path):
    """The control: the same two ranks WITHOUT sync_bn miss the bound of
    test_two_ranks_equal_one_process on the layer-0 gate BatchNorms' running means (each rank
    normalises by its own shard's statistics, offset by +1 / -1)."""
    _launch(tmp_path, family, "nosync", "equal", "fp32", "rec", port=11 + (family == "ligru"))
    g = _ranks(tmp_path)
    _, ref = _one_process(family, "fp32")
    rtol, atol, _ = _bounds(family, "fp32")
    keys = [k for k in ref if re.match(r"rnn/bn_w\w+\.0\.running_mean$", k)]
    assert keys
    for k in keys:
        assert not np.allclose(g[0][k], ref[k], rtol=rtol, atol=atol), k
        assert not np.array_equal(g[0][k], g[1][k]), k


def _union_checks(g, key):
    """The BatchNorm `key` of the last step over the UNION of both ranks' rows, per column, summed
    in float64; each bound is n * 2^-23 * sum |term| (float32 summation error, derived).

    sum dz xhat: a BatchNorm backward over n rows gives dz = k (dy - S1 / n - xhat S2 / n) with
    k = gamma invstd, S1 = sum dy, S2 = sum dy xhat, so with sum xhat^2 = n (1 - eps invstd^2)
    (the identity checked just above) sum dz xhat = k S2 eps invstd^2 - k (S1 / n) sum xhat: zero
    only up to eps.  The eps term is no rounding error (measured here, as |sum dz xhat| over the
    bound: liGRU 14.6, LSTM 10.8, the MLP layer 1.5e3), so it is taken out exactly — gamma as it
    stood before the step, S2 the all-reduced sum the backward applied — and what is left is held
    to the same bound.  A backward over rows * world instead of the global count misses it."""
    mean, invstd = g[0][key + "mean"], g[0][key + "invstd"]
    np.testing.assert_array_equal(mean, g[1][key + "mean"], err_msg=key + "save_mean")
    np.testing.assert_array_equal(invstd, g[1][key + "invstd"], err_msg=key + "save_invstd")
    xh = np.concatenate([g[0][key + "xhat"], g[1][key + "xhat"]]).astype(np.float64)
    dz = np.concatenate([g[0][key + "dz"], g[1][key + "dz"]]).astype(np.float64)
    n = xh.shape[0]
    assert n == g[0][key + "xhat"].shape[0] + g[1][key + "xhat"].shape[0]
    assert g[0][key + "xhat"].shape[0] != g[1][key + "xhat"].shape[0]       # unequal T_r
    iv2 = EPS * invstd.astype(np.float64) ** 2
    np.testing.assert_array_equal(g[0][key + "sums"], g[1][key + "sums"])
    eps_term = (g[0][key + "gamma"].astype(np.float64) * invstd * g[0][key + "sums"][1] * iv2)
    print("%s sum dz xhat before the eps term is taken out: max |value| / bound = %.3g" % (
        key, (np.abs((dz * xh).sum(0)) / np.maximum(n * U * np.abs(dz * xh).sum(0),
                                                     np.finfo(np.float64).tiny)).max()))
    checks = [("sum xhat", xh.sum(0), n * U * np.abs(xh).sum(0)),
              # (the right side's eps * invstd^2 carries invstd's own float32 rounding, twice)
              ("sum xhat^2 - n (1 - eps invstd^2)", (xh * xh).sum(0) - n * (1.0 - iv2),
               n * U * (xh * xh).sum(0) + n * iv2 * 2 * U),
              ("sum dz", dz.sum(0), n * U * np.abs(dz).sum(0)),
              # (the eps term's own float32 factors: gamma, invstd three times, S2)
              ("sum dz xhat - k S2 eps invstd^2", (dz * xh).sum(0) - eps_term,
               n * U * np.abs(dz * xh).sum(0) + 5 * U * np.abs(eps_term))]
    for name, val, bound in checks:
        ratio = np.abs(val) / np.maximum(bound, np.finfo(np.float64).tiny)
        print("%s %s: max |value| / bound = %.3g" % (key, name, ratio.max()))
    for name, val, bound in checks:
        bad = np.abs(val) > bound
        assert not bad.any(), "%s %s: column %d value %.3g bound %.3g" % (
            key, name, int(np.argmax(np.abs(val) - bound)), np.abs(val)[bad].max(),
            bound[bad].min())


def _unequal(tmp_path, family, body, port):
    import dp_seq_syncbn_worker as W
    _launch(tmp_path, family, "sync", "unequal", "fp32", body, port=port)
    g = _ranks(tmp_path)
    assert (g[0]["T"] == 7).all() and (g[1]["T"] == 5).all()
    np.testing.assert_array_equal(g[0]["rows"], np.full(W.STEPS, (7 + 5) * W.B))
    np.testing.assert_array_equal(g[0]["rows"], g[1]["rows"])
    keys = sorted({k[:k.rindex(":") + 1] for k in g[0].files if k.startswith("bn:")})
    for k in g[0].files:       # running statistics (and every parameter) bit-identical
        if "/" in k:
            np.testing.assert_array_equal(g[0][k], g[1][k], err_msg="replicas differ: " + k)
    return g, keys


@pytest.mark.parametrize("family", ["ligru", "lstm"])
def test_unequal_padded_lengths_global_population(family, tmp_path):
    """Rank 0 pads to T = 7, rank 1 to T = 5 in every step.  Per layer and gate: save_mean /
    save_invstd bit-identical on the ranks; over the union of the ranks' rows sum xhat = 0,
    sum xhat^2 / n = 1 - eps invstd^2, sum dz = 0, sum dz xhat = 0 (a BatchNorm forward and
    backward over the global population with the global count); running statistics bit-identical
    after three steps; exactly 2 L collectives per step."""
    import dp_seq_syncbn_worker as W
    g, keys = _unequal(tmp_path, family, "rec", port=21 + (family == "lstm"))
    G = {"ligru": 2, "lstm": 4}[family]
    assert len(keys) == 2 * G, keys
    assert int(g[0]["bn_calls"]) == int(g[1]["bn_calls"]) == 2 * 2 * W.STEPS
    for key in keys:
        _union_checks(g, key)


def test_mlp_layer_behind_ligru_uses_global_rows(tmp_path):
    """A BatchNorm'd MLP layer between the liGRU and the heads, unequal padded lengths: its
    synchronised backward runs over sum_r T_r * B rows, not rows * world."""
    import dp_seq_syncbn_worker as W
    g, keys = _unequal(tmp_path, "ligru", "mlp", port=25)
    assert "bn:body.0:" in keys and len(keys) == 2 * 2 + 1
    assert int(g[0]["bn_calls"]) == 2 * 3 * W.STEPS
    for key in keys:
        _union_checks(g, key)


class _World1:
    """A one-rank SyncBN: the collective is the identity."""
    world, rank = 1, 0

    def __init__(self):
        self.calls = 0

    def __call__(self, t):
        self.calls += 1


def _profiled_step(family, sync_bn):
    import random

    import dp_seq_syncbn_worker as W
    lens, end, X, lab = W.chunk(1, "equal")
    eng, nets = W.build_engine(family, 1, W.B, sync_bn=sync_bn)
    eng.bind_chunk(torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda(), end[-1], end_index=end)
    eng.prof = []
    eng.train_step(batch=eng.next_seq_batch(random.Random(7)))
    torch.cuda.synchronize()
    names = [p[1] for p in eng.prof]
    eng.prof = None
    return names, W.state(nets), eng


def test_refusals_kept_and_launches_unchanged():
    import cudnn_cases as CC
    import dp_seq_syncbn_worker as W
    import pkc.neural_networks as NN
    from pkc.engine import Engine, parse_model

    class World:
        world, rank = 2, 0

    for family in W.FAMILIES:
        with pytest.raises(NotImplementedError, match="input BatchNorm"):
            W.build_engine(family, 2, W.B, sync_bn=World(), inp_bn=True)
    nets, opts = CC.build(CC.make_cfg("LSTM_cudnn"), (NN, NN))
    for n in nets.values():
        n.cuda().train()
    eng = Engine(nets, opts, parse_model(CC.MODEL), {"fea": (0, CC.F)}, ["lab_cd", "lab_mono"],
                 batch=CC.B, max_len=CC.MAX_LEN, seed=1, sync_bn=World())
    assert eng.rec_forms()["rnn.0"] == "fp32 steps"
    eng = W.build_engine("ligru", 2, W.B, sync_bn=World())[0]
    assert eng.capture() is False                  # eager steps only with sync_bn
    bn_fns = ("pkc_dense_fwd", "pkc_dense_bwd")
    sync_fns = ("pkc_dense_fwd_stats", "pkc_dense_fwd_sync_apply_packed", "pkc_dense_bwd_stats",
                "pkc_dense_bwd_sync_apply")
    for family, G in (("lstm", 4), ("ligru", 2)):
        plain, sd0, eng0 = _profiled_step(family, None)
        sbn = _World1()
        armed, sd1, eng1 = _profiled_step(family, sbn)
        # without sync_bn: no SyncBN launch, one fused BatchNorm launch per layer, gate and pass
        assert not [f for f in plain if f in sync_fns]
        assert plain.count("pkc_dense_fwd") == plain.count("pkc_dense_bwd") == 2 * G
        # armed: those launches become the stats / apply halves, every other launch as it was
        assert [f for f in plain if f not in bn_fns] == [f for f in armed if f not in sync_fns]
        assert [armed.count(f) for f in sync_fns] == [2 * G] * 4
        assert sbn.calls == 2 * 2
        # one rank synchronised with itself: the same forward up to the summation split
        np.testing.assert_allclose(eng1.loss_values()[0], eng0.loss_values()[0], rtol=1e-5)


def _run_nn_cfg(d):
    """A tiny liGRU train chunk cfg on synthetic arks ([exp] sync_bn = True), after the builders
    of test_gpu_run_nn.py."""
    from pkc import data_io as D
    rs = np.random.RandomState(0)
    fea_ark, scp = os.path.join(d, "feats.ark"), os.path.join(d, "feats.scp")
    ali = os.path.join(d, "ali")
    os.makedirs(ali, exist_ok=True)
    with open(scp, "w") as f:
        for i in range(16):
            k = "spk0_u%03d" % i
            T = rs.randint(8, 20)
            D.write_mat_path(fea_ark, (rs.randn(T, 24) + rs.randn(1, 24)).astype(np.float32), k,
                             append=i > 0)
            D.write_vec_int_path(os.path.join(ali, "ali_pdf.ark"), rs.randint(0, 11, T), k,
                                 append=i > 0)
            D.write_vec_int_path(os.path.join(ali, "ali_phones.ark"), rs.randint(1, 6, T), k,
                                 append=i > 0)
            f.write("%s %s\n" % (k, fea_ark))
    cfg = configparser.ConfigParser()
    cfg["exp"] = {"seed": "2234", "out_folder": d, "use_cuda": "True", "multi_gpu": "False",
                  "to_do": "train", "out_info": os.path.join(d, "train_ck0.info"),
                  "save_gpumem": "False", "production": "False", "run_nn_script": "run_nn.py",
                  "sync_bn": "True"}
    cfg["batches"] = {"batch_size_train": "2", "batch_size_valid": "2",
                      "max_seq_length_train": "1000", "max_seq_length_valid": "1000"}
    cfg["data_chunk"] = {
        "fea": "fea_name=fmllr\nfea_lst=%s\nfea_opts=\ncw_left=0\ncw_right=0\n" % scp,
        "lab": "lab_name=lab_cd\nlab_folder=%s\nlab_opts=ali-to-pdf\n\n"
               "lab_name=lab_mono\nlab_folder=%s\nlab_opts=ali-to-phones --per-frame=true\n" % (ali, ali)}
    base = dict(arch_library="pkc.neural_networks", arch_pretrain_file="none", arch_freeze="False",
                arch_opt="rmsprop", opt_momentum="0.0", opt_alpha="0.95", opt_eps="1e-8",
                opt_centered="False", opt_weight_decay="0.0")
    cfg["architecture1"] = dict(base, arch_name="liGRU_layers", arch_class="liGRU",
                                arch_seq_model="True", arch_lr="0.0016", ligru_lay="48,48",
                                ligru_drop="0.0,0.0", ligru_use_laynorm_inp="False",
                                ligru_use_batchnorm_inp="False", ligru_use_laynorm="False,False",
                                ligru_use_batchnorm="True,True", ligru_bidir="True",
                                ligru_act="relu,relu", ligru_orthinit="True")
    cfg["architecture2"] = dict(base, arch_name="MLP_layers2", arch_class="MLP",
                                arch_seq_model="False", dnn_use_laynorm_inp="False",
                                dnn_use_batchnorm_inp="False", dnn_lay="11", dnn_drop="0.0",
                                dnn_use_batchnorm="False", dnn_use_laynorm="False",
                                dnn_act="softmax", arch_lr="0.0004")
    cfg["architecture3"] = dict(cfg["architecture2"], arch_name="MLP_layers3", dnn_lay="6")
    cfg["model"] = {"model": "out_dnn1=compute(liGRU_layers,fmllr)\n"
                             "out_dnn2=compute(MLP_layers2,out_dnn1)\n"
                             "out_dnn3=compute(MLP_layers3,out_dnn1)\n"
                             "loss_mono=cost_nll(out_dnn3,lab_mono)\n"
                             "loss_mono_w=mult_constant(loss_mono,1.0)\n"
                             "loss_cd=cost_nll(out_dnn2,lab_cd)\n"
                             "loss_final=sum(loss_cd,loss_mono_w)\n"
                             "err_final=cost_err(out_dnn2,lab_cd)"}
    cfg["forward"] = {"forward_out": "out_dnn2", "normalize_posteriors": "False",
                      "normalize_with_counts_from": "none", "save_out_file": "False",
                      "require_decoding": "False"}
    path = os.path.join(d, "train_ck0.cfg")
    with open(path, "w") as f:
        cfg.write(f)
    return path


def test_run_nn_sync_bn_reaches_the_sequence_engine(tmp_path):
    """[exp] sync_bn = True on two ranks: pkc.core.run_nn hands the sequence Engine a
    SyncBatchNorm; both ranks finish, rank 0 writes the .info (finite loss) and the .pkl files."""
    d = str(tmp_path)
    _launch(d, "run_nn", _run_nn_cfg(d), port=31)
    rec = [json.load(open(os.path.join(d, "run_nn_rank%d.json" % k))) for k in range(2)]
    for r in rec:
        assert r["world"] == 2 and r["seq"] and r["sync_bn"] == "SyncBatchNorm"
        assert r["steps"] == 16 // 2 // 2
        assert r["bn_calls"] == 2 * 2 * r["steps"]
    info = configparser.ConfigParser()
    info.read(os.path.join(d, "train_ck0.info"))
    assert np.isfinite(float(info["results"]["loss"])) and 0 < float(info["results"]["loss"]) < 20
    for i in (1, 2, 3):
        assert os.path.exists(os.path.join(d, "train_ck0_architecture%d.pkl" % i))

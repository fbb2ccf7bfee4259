"""tests/joint_ref.py (forward_model with the mse operation, the batch body and the sentence-batch
loop of core.run_nn on oracle.nets modules) against the reference's own run: the golden `train
ck1 resumed from the ck0 checkpoints` call of tests/golden/run_nn_joint (make_golden_joint.py)
replayed on the CPU.  This pins the restatement the GPU tests of the joint recipe lean on.

Both sides are fp32 torch on the CPU running the same expressions, so they agree to summation
order inside torch's own kernels: parameters and RMSprop state within 1e-5 relative Frobenius (the
generator measured 0 on its machine, and 1.9e-6 between the reference and an fp64 rerun), the
chunk's .info loss within 1e-6 relative."""
import os

import numpy as np
import pytest
import torch

import joint_ref as JR
from conftest import GOLDEN
from joint_cfg import ARCHS, MODEL, SE_WEIGHT, SECS

SRC = os.path.join(GOLDEN, "run_nn_joint")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(SRC, "expected.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def replay(golden):
    pkls = {a: os.path.join(SRC, "train_ck0_%s.pkl" % s) for s, a in zip(SECS, ARCHS)}
    return JR.replay_ck1(golden, pkls)


def rel_frob(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b), np.linalg.norm(b)


def test_restatement_reproduces_reference_ck1(golden, replay):
    nets, opts, (loss, err) = replay
    rl, re_ = golden["info_train_ck1"]
    assert abs(loss - rl) <= 1e-6 * abs(rl), (loss, rl)
    assert abs(err - re_) <= 1e-6, (err, re_)
    bad = {}
    for s, a in zip(SECS, ARCHS):
        for k, v in nets[a].state_dict().items():
            ref = golden["ck1/%s/model/%s" % (s, k)]
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(ref), (s, k)
                continue
            d, n = rel_frob(v.numpy(), ref)
            if d > 1e-5 * n + 1e-7 * np.sqrt(ref.size):
                bad["%s %s" % (s, k)] = d / max(n, 1e-30)
        names = [str(x) for x in golden["pnames/" + a]]
        mine = {n: p for n, p in nets[a].named_parameters()}
        keys = [k for k in golden.files if k.startswith("ck1/%s/opt/" % s)]
        assert keys
        for key in keys:
            _, _, _, pi, name = key.split("/")
            st = opts[a].state[mine[names[int(pi)]]][name]
            d, n = rel_frob(torch.as_tensor(st).numpy(), golden[key])
            if d > 1e-5 * n + 1e-7 * np.sqrt(golden[key].size):
                bad[key] = d / max(n, 1e-30)
    assert not bad, "restatement off the reference: %s" % bad


def test_mse_term_is_weighted_mean_over_all_elements(golden):
    """The restated mse is torch.mean over every element, padded rows included, and enters
    loss_final with the [model]'s weight."""
    import random

    from oracle.run import parse_model
    nets, _, seq, _ = JR.build_nets(to_do="valid")
    _, end, fea_cols, lab_cols, ds = JR.golden_chunk(golden, "ck0")
    inp, T, _ = JR.seq_batch(ds, end, 6, 3, random.Random(1))
    with torch.no_grad():
        outs = JR.forward_model(parse_model(MODEL), nets, seq, fea_cols, lab_cols, inp, T, 3)
    c0, c1 = fea_cols["fbank_clean"]
    se = outs["out_dnn_SE"].reshape(T * 3, -1).double()
    want = ((se - inp[..., c0:c1].reshape(T * 3, -1).double()) ** 2).sum() / se.numel()
    np.testing.assert_allclose(outs["loss_se"].item(), want.item(), rtol=1e-6)
    np.testing.assert_allclose(
        outs["loss_final"].item(),
        (outs["loss_cd"] + outs["loss_mono"] + float(SE_WEIGHT) * outs["loss_se"]).item(), rtol=1e-6)

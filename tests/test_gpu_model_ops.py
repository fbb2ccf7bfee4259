"""The [model] tensor operations on produced outputs (CombineNode, pkc_combine_fwd / _bwd) through
the pkc engine against their restatement (tests/model_ops_ref.py, pinned to the reference's own run
by tests/test_model_ops_cpu.py) and against the reference-written fixtures
(tests/golden/model_ops/*.npz).  The models are those of tests/golden/model_ops_cfg.py.

Bounds, unchanged from test_mse_on_a_feed_forward_chain (tests/test_gpu_joint.py): loss rtol 1e-4,
err atol 1e-6, posteriors relative < 1e-4 with the denominator clamped at 1e-3, every parameter by
test_gpu_seq._seq_check_update at its bound; a combine node's output within 1e-4 of its scale.
The bit-level tests ask for torch.equal."""
import os
import random

import numpy as np
import pytest
import torch

import model_ops_cfg as MC
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"


def build_nets(archs, dims, state=None, train=True):
    """({arch: pkc net on the GPU}, {arch: oracle net from the same state})."""
    import model_ops_ref as MR
    import pkc.neural_networks as NN
    nets = {}
    for a, o in archs.items():
        torch.manual_seed(3)
        np.random.seed(3)
        nets[a] = getattr(NN, o["arch_class"])(o, dims[a])
        if state is not None:
            nets[a].load_state_dict(state[a])
    onets, _, seq = MR.build(archs, dims, train=train,
                             state={a: n.state_dict() for a, n in nets.items()})
    for n in nets.values():
        n.to(DEV)
        n.train() if train else n.eval()
    return nets, onets, seq


def oracle_opts(onets, archs):
    from oracle import nets as ON
    return {a: ON.make_optimizer(onets[a].parameters(), archs[a]) for a in onets
            if archs[a]["arch_freeze"] != "True"}


def ff_data(steps=3):
    rs = np.random.RandomState(21)
    n = steps * MC.B_FF
    X = rs.randn(n, 22).astype(np.float32)
    lab = rs.randint(0, MC.N_LAB, size=(n, 1)).astype(np.int32)
    keep = torch.from_numpy((rs.rand(MC.B_FF, 24) > 0.1).astype(np.uint8))
    return X, lab, keep


def ff_engine(nets, archs, X, lab, keep=None, model=MC.MODEL_FF, **kw):
    from pkc.engine import Engine, parse_model
    if keep is not None:
        kw["drop_keep_in"] = {"MLP_a.0": keep.to(DEV)}
    eng = Engine(nets, archs, parse_model(model), MC.FEA_FF, ["lab"], batch=MC.B_FF, seed=1, **kw)
    eng.bind_chunk(torch.from_numpy(X).to(DEV), torch.from_numpy(lab).to(DEV), X.shape[0])
    return eng


def check_outputs(eng, outs, names, head="out_h", what=""):
    """Posteriors at the relative bound, every other named output within 1e-4 of its scale."""
    post, ref = eng.head_output(head).cpu(), outs[head].detach().reshape(-1, outs[head].shape[-1])
    rel = ((post - ref).abs() / ref.abs().clamp_min(1e-3)).max().item()
    print("%s posterior rel err %.3g" % (what, rel))
    assert rel < 1e-4, "%s posterior rel err %.3g" % (what, rel)
    for name in names:
        got = eng.head_output(name).cpu()
        r = outs[name].detach().reshape(got.shape)
        d, scale = (got - r).abs().max().item(), r.abs().max().item()
        print("%s %s max diff / scale %.3g" % (what, name, d / scale))
        assert d <= 1e-4 * scale, "%s %s off by %.3g of its scale" % (what, name, d / scale)


def ff_steps(archs, dims, steps, check_frozen=None):
    """`steps` SGD steps of the feed-forward model, each from a common start, against the
    restatement (injected dropout mask on MLP_a)."""
    import model_ops_ref as MR
    from flipcheck import resync
    from oracle.run import parse_model as oparse
    from test_gpu_seq import _seq_check_update
    X, lab, keep = ff_data(steps)
    nets, onets, seq = build_nets(archs, dims)
    eng = ff_engine(nets, archs, X, lab, keep)
    assert sum(1 for n in eng.nodes if getattr(n, "combine", False)) == 6
    oopt = oracle_opts(onets, archs)
    body = onets["MLP_a"]
    f = body.forward
    body.forward = lambda x, _f=f: _f(x, drop_masks=[keep.float()])
    lines = oparse(MC.MODEL_FF)
    full = torch.from_numpy(np.concatenate([X, lab.astype(np.float32)], 1))
    frozen0 = ({k: v.detach().cpu().clone() for k, v in nets[check_frozen].state_dict().items()}
               if check_frozen else None)
    report, post_out, B = {}, [], MC.B_FF
    live = {a: n for a, n in nets.items() if a in oopt}
    for step in range(steps):
        eng.sync_state()
        resync(live, onets, {k: eng.optimizer_state_dict(k) for k in live} if step else None, oopt)
        outs = MR.train_step(lines, onets, oopt, seq, MC.FEA_FF, MC.LAB_FF,
                             full[step * B:(step + 1) * B])
        eng.train_step()
        loss, err = eng.loss_values()
        print("step %d loss %.6f (restatement %.6f)" % (step, loss, outs["loss_final"].item()))
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
        np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
        check_outputs(eng, outs, ("out_a", "out_b") + MC.COMBINE_FF, what="step %d" % step)
        post_out.append(0)
        _seq_check_update("ff", False, step, eng, live, onets, archs, report, post_out)
    if check_frozen:
        for k, v in nets[check_frozen].state_dict().items():
            assert torch.equal(v.cpu(), frozen0[k]), "frozen %s.%s moved" % (check_frozen, k)
    return eng


def test_feed_forward_engine_vs_restatement():
    archs, dims = MC.ff_archs()
    ff_steps(archs, dims, 3)


def test_feed_forward_first_step_vs_reference_golden():
    import model_ops_ref as MR
    g = np.load(os.path.join(GOLDEN, "model_ops", "ff.npz"))
    archs, dims = MC.ff_archs(drop="0.0")
    nets, _, _ = build_nets(archs, dims, state=MR.golden_state(g, archs))
    inp = g["inp"]
    eng = ff_engine(nets, archs, inp[:, :22].copy(), inp[:, 22:].astype(np.int32))
    eng.train_step()
    loss, err = eng.loss_values()
    outs = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("out/")}
    np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
    np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
    check_outputs(eng, outs, ("out_a", "out_b") + MC.COMBINE_FF, what="golden")
    # and the gradients the reference's backward wrote, at the parameter bound's 1e-4 of scale
    gview = {id(p): gr for p, gr in eng.param_grads}
    checked = 0
    for a, net in nets.items():
        for pn, p in net.named_parameters():
            if "grad/%s/%s" % (a, pn) not in g.files:      # (a parameter the model never uses)
                continue
            checked += 1
            ref = torch.from_numpy(g["grad/%s/%s" % (a, pn)]).double()
            got = gview[id(p)].detach().cpu().double().reshape(ref.shape)
            scale = max(float(ref.abs().max()), 1e-6)
            assert float((got - ref).abs().max()) <= 1e-4 * scale + 1e-7, (a, pn)
    assert checked == sum(1 for k in g.files if k.startswith("grad/"))


# ------------------------------------------------------------------ sequence models
def seq_data(n_batches=2):
    rs = np.random.RandomState(4)
    lens = np.array(list(MC.SEQ_LENS) * n_batches)
    end = np.cumsum(lens)
    X = rs.randn(end[-1], 17).astype(np.float32)
    lab = rs.randint(0, MC.N_LAB, size=(end[-1], 1)).astype(np.int32)
    return dict(lens=lens, end=end, X=X, lab=lab)


def seq_engine(nets, archs, model, d, **kw):
    from pkc.engine import Engine, parse_model
    eng = Engine(nets, archs, parse_model(model), MC.FEA_SEQ, ["lab"], batch=MC.B_SEQ, max_len=8,
                 seed=1, **kw)
    eng.bind_chunk(torch.from_numpy(d["X"]).to(DEV), torch.from_numpy(d["lab"]).to(DEV),
                   d["end"][-1], end_index=d["end"])
    return eng


def padded(d, snt, T, lefts):
    """core.py:183-200: (T, B, [features | label]) of sentences snt .. snt + B - 1."""
    B = MC.B_SEQ
    inp = torch.zeros(T, B, 18)
    for k in range(B):
        n = int(d["lens"][snt + k])
        b0 = int(d["end"][snt + k] - n)
        inp[lefts[k]:lefts[k] + n, k, :17] = torch.from_numpy(d["X"][b0:b0 + n])
        inp[lefts[k]:lefts[k] + n, k, 17] = torch.from_numpy(d["lab"][b0:b0 + n, 0].astype(np.float32))
    return inp


@pytest.mark.parametrize("which", ["concatenate_of_two_ligrus", "sum_into_one_ligru"])
def test_sequence_engine_vs_restatement(which):
    import model_ops_ref as MR
    from flipcheck import resync
    from oracle.run import parse_model as oparse
    from pkc.engine import CombineNode
    from test_gpu_seq import _seq_check_update
    cat = which == "concatenate_of_two_ligrus"
    (archs, dims), model = (MC.seq_cat_archs(), MC.MODEL_SEQ_CAT) if cat else (
        MC.seq_sum_archs(), MC.MODEL_SEQ_SUM)
    d = seq_data(2)
    nets, onets, seq = build_nets(archs, dims)
    eng = seq_engine(nets, archs, model, d)
    node = eng.produced["out_c" if cat else "out_x"]
    assert isinstance(node, CombineNode)
    if cat:         # each liGRU's output gradient: the combine node's one slab
        assert all(p.gslab is not None and p.rec for _, p in node.srcs)
    else:           # the combine node's gradient: the recurrent layer-0 dX slabs
        assert node.rec_consumer is eng.produced["out_r"] and node.gslab is None
    oopt = oracle_opts(onets, archs)
    lines = oparse(model)
    rng = random.Random(7)
    report, post_out = {}, []
    names = ("out_r1", "out_r2", "out_c") if cat else ("out_m1", "out_m2", "out_x", "out_r")
    for step in range(2):
        eng.sync_state()
        resync(nets, onets, {k: eng.optimizer_state_dict(k) for k in nets} if step else None, oopt)
        batch = eng.next_seq_batch(rng)
        _, _, lefts, T = batch
        inp = padded(d, step * MC.B_SEQ, T, lefts)
        outs = MR.train_step(lines, onets, oopt, seq, MC.FEA_SEQ, MC.LAB_SEQ, inp, T, MC.B_SEQ)
        eng.train_step(batch=batch)
        loss, err = eng.loss_values()
        print("step %d loss %.6f (restatement %.6f)" % (step, loss, outs["loss_final"].item()))
        np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
        np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
        check_outputs(eng, outs, names, what="%s step %d" % (which, step))
        post_out.append(0)
        _seq_check_update("model_ops", False, step, eng, nets, onets, archs, report, post_out)


def test_sequence_first_step_vs_reference_golden():
    import model_ops_ref as MR
    from pkc.engine import SeqBatch
    g = np.load(os.path.join(GOLDEN, "model_ops", "seq.npz"))
    archs, dims = MC.seq_cat_archs()
    nets, _, _ = build_nets(archs, dims, state=MR.golden_state(g, archs))
    inp, lens, lefts = g["inp"], g["lens"], g["lefts"]
    T = inp.shape[0]
    rows = np.concatenate([inp[lefts[k]:lefts[k] + lens[k], k] for k in range(MC.B_SEQ)])
    d = dict(lens=lens, end=np.cumsum(lens), X=rows[:, :17].copy(),
             lab=rows[:, 17:].astype(np.int32))
    eng = seq_engine(nets, archs, MC.MODEL_SEQ_CAT, d)
    begs = np.concatenate([[0], d["end"][:-1]]).astype(np.int64)
    eng.train_step(batch=SeqBatch((begs, lens.astype(np.int64), lefts.astype(np.int64), T), 0))
    loss, err = eng.loss_values()
    outs = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("out/")}
    np.testing.assert_allclose(loss, outs["loss_final"].item(), rtol=1e-4)
    np.testing.assert_allclose(err, outs["err_final"].item(), atol=1e-6)
    check_outputs(eng, outs, ("out_r1", "out_r2", "out_c"), what="golden seq")


# ------------------------------------------------------------------ bit-level self-consistency
def _stated(node, eng):
    """The node's stated fp32 arithmetic applied on the GPU to its operands' buffers."""
    M = eng.M
    ops = []
    for src in node.srcs:
        if src[0] == "fea":
            ops.append(eng.x[:M * eng.F].view(M, eng.F)[:, src[1]:src[2]])
        else:
            ops.append(src[1].out[:M * src[1].N].view(M, src[1].N))
    c = torch.tensor(node.c, dtype=torch.float32, device=DEV)
    half = torch.tensor(0.5, dtype=torch.float32, device=DEV)
    return {"concatenate": lambda: torch.cat(ops, 1), "sum": lambda: ops[0] + ops[1],
            "mult": lambda: ops[0] * ops[1], "avg": lambda: (ops[0] + ops[1]) * half,
            "sum_constant": lambda: ops[0] + c, "mult_constant": lambda: ops[0] * c}[node.op]()


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_combine_outputs_are_the_stated_arithmetic_of_their_operands(prec):
    from pkc import _lib as L
    archs, dims = MC.ff_archs()
    X, lab, keep = ff_data(1)
    nets, _, _ = build_nets(archs, dims)
    eng = ff_engine(nets, archs, X, lab, keep,
                    prec=L.PREC_BF16 if prec == "bf16" else L.PREC_FP32)
    eng.eval_step()
    torch.cuda.synchronize()
    nodes = [n for n in eng.nodes if getattr(n, "combine", False)]
    assert [n.op for n in nodes] == ["sum", "mult", "avg", "sum_constant", "mult_constant",
                                     "concatenate"]
    for n in nodes:
        out = n.out[:eng.M * n.N].view(eng.M, n.N)
        assert torch.equal(out, _stated(n, eng)), n.name
        if n.out_h is not None:
            assert torch.equal(n.out_h[:eng.M * n.N].view(eng.M, n.N), out.to(torch.bfloat16)), n.name
    cat = eng.produced["out_c"]
    # only the node a matmul reads keeps a bf16 copy, and only in the bf16-operand mode
    assert (cat.out_h is not None) == (prec == "bf16")
    assert all(n.out_h is None for n in nodes if n is not cat)


# ------------------------------------------------------------------ graph replay
def test_graph_replay_equals_eager():
    """The comparison of test_joint_graph_replay_equals_eager: the captured step holds the combine
    launches, and three replayed steps leave the same bits as three eager ones."""
    archs, dims = MC.ff_archs()
    X, lab, _ = ff_data(3)
    res = []
    for capture in (False, True):
        nets, _, _ = build_nets(archs, dims)
        eng = ff_engine(nets, archs, X, lab)
        if capture:
            assert eng.capture()
        trace = []
        for _ in range(3):
            eng.train_step()
            trace.append(eng.loss_values())
        eng.sync_state()
        res.append((trace, {k: {n: v.detach().cpu().clone() for n, v in m.state_dict().items()}
                            for k, m in nets.items()}))
    (te, se), (tg, sg) = res
    assert te == tg
    for k in se:
        for n in se[k]:
            assert torch.equal(se[k][n], sg[k][n]), (k, n)
    assert not torch.equal(se["MLP_b"]["wx.0.weight"],
                           build_nets(archs, dims)[0]["MLP_b"].state_dict()["wx.0.weight"].cpu())


# ------------------------------------------------------------------ frozen branch
def test_frozen_branch():
    archs, dims = MC.ff_archs()
    archs["MLP_b"] = dict(archs["MLP_b"], arch_freeze="True")
    ff_steps(archs, dims, 2, check_frozen="MLP_b")


# ------------------------------------------------------------------ forward mode
def _post_rel(got, ref, prior):
    """Relative error of prior-normalised log posteriors the way
    tests/test_gpu_run_nn_parity.py measures it: on the log posteriors, the log prior added back
    in fp64 (logp - prior crosses zero, where a last-bit difference of logp, 2^-22 at |logp| in
    [2, 4), is any multiple of the difference), denominator clamped at 1e-3."""
    lp = torch.from_numpy(prior).double()
    a, b = got.double() + lp, ref.double() + lp
    return ((a - b).abs() / b.abs().clamp_min(1e-3)).max().item()


def test_forward_mode_posterior_ensemble():
    import model_ops_ref as MR
    from oracle.run import parse_model as oparse
    from pkc.engine import Engine, parse_model
    from pkc.runners import ForwardRunner
    archs, dims = MC.ens_archs()
    nets, onets, seq = build_nets(archs, dims, train=False)
    rs = np.random.RandomState(9)
    lens = [9, 14]
    X = rs.randn(sum(lens), 17).astype(np.float32)
    lab = rs.randint(0, MC.N_LAB, size=(sum(lens), 1)).astype(np.int32)
    counts = rs.randint(1, 500, size=MC.N_LAB)
    prior = np.log(counts / counts.sum()).astype(np.float32)
    feats = torch.from_numpy(X).to(DEV)
    runner = ForwardRunner(nets, parse_model(MC.MODEL_ENS), MC.FEA_SEQ, ["out_e"])
    lines = oparse(MC.MODEL_ENS)
    full = torch.from_numpy(np.concatenate([X, lab.astype(np.float32)], 1))

    def ref_post(b, e):
        with torch.no_grad():
            outs = MR.forward_model(lines, onets, seq, MC.FEA_SEQ, MC.LAB_SEQ, full[b:e],
                                    forward_outs=["out_e"])
        return outs["out_e"] - torch.from_numpy(prior)        # core.py:242-245

    beg = 0
    for n in lens:
        got = torch.from_numpy(runner.forward(feats, beg, beg + n, {"out_e": prior})["out_e"])
        ref = ref_post(beg, beg + n)
        assert got.shape == (n, MC.N_LAB)
        rel = _post_rel(got, ref, prior)
        print("utterance of %d frames: posterior rel err %.3g, largest difference of the "
              "normalised values %.3g" % (n, rel, (got - ref).abs().max().item()))
        assert rel < 1e-4, "utterance of %d frames: posterior rel err %.3g" % (n, rel)
        beg += n
    # the same model through the engine: eval_step + head_output, the prior on the host
    eng = Engine(nets, archs, parse_model(MC.MODEL_ENS), MC.FEA_SEQ, ["lab"], batch=lens[0],
                 train=False)
    eng.bind_chunk(feats, torch.from_numpy(lab).to(DEV), sum(lens))
    node = eng.produced["out_e"]
    assert node.heads_in and not eng.needs_grad[node]
    eng.eval_step()
    got = eng.head_output("out_e").cpu() - torch.from_numpy(prior)
    ref = ref_post(0, lens[0])
    rel = _post_rel(got, ref, prior)
    assert rel < 1e-4, "engine posterior rel err %.3g" % rel


# ------------------------------------------------------------------ what stays refused
def test_refused_forms():
    import pkc.neural_networks as NN
    from pkc.engine import Engine, parse_model
    archs, dims = MC.ff_archs()
    nets, _, _ = build_nets(archs, dims)

    def eng(model, nets=nets, archs=archs, fea=MC.FEA_FF, **kw):
        return Engine(nets, archs, parse_model(model), fea, ["lab"], batch=MC.B_FF, **kw)

    tail = "\nout_h=compute(MLP_h,out_c)\nloss_final=cost_nll(out_h,lab)\nerr_final=cost_err(out_h,lab)"
    head = "out_a=compute(MLP_a,fa)\nout_b=compute(MLP_b,fb)\n"
    # a feature stream as the first argument of the five non-concatenate operations
    for line in ("x=sum(fa,fa)", "x=mult(fa,fa)", "x=avg(fa,fa)", "x=sum_constant(fa,1.0)",
                 "x=mult_constant(fa,2.0)"):
        with pytest.raises(NotImplementedError, match="feature stream as the first argument"):
            eng(head + line + "\nout_c=concatenate(out_a,fc)" + tail)
    # (a feature as the second argument is fine, and on either side of concatenate)
    a5 = dict(archs["MLP_a"], arch_name="MLP_a5", dnn_lay="5")
    w22 = dict(archs["MLP_h"], arch_name="MLP_w")
    e = eng("o5=compute(MLP_a5,fa)\ns5=sum(o5,fc)\nc1=concatenate(fb,s5)\nc2=concatenate(c1,fa)\n"
            "out_h=compute(MLP_w,c2)\nloss_final=cost_nll(out_h,lab)\nerr_final=cost_err(out_h,lab)",
            nets={"MLP_a5": NN.MLP(a5, 11).to(DEV), "MLP_w": NN.MLP(w22, 22).to(DEV)},
            archs={"MLP_a5": a5, "MLP_w": w22})
    assert e.produced["c2"].N == 22 and e.produced["s5"].srcs[1] == ("fea", 17, 22)
    assert e.produced["c1"].srcs[0] == ("fea", 11, 17)
    # a cost on a combine output
    model = head + "out_s=sum(out_a,out_b)\nout_c=concatenate(out_s,fc)" + tail
    with pytest.raises(NotImplementedError, match="cost_nll on the combine output"):
        eng(model.replace("cost_nll(out_h,lab)", "cost_nll(out_c,lab)"))
    with pytest.raises(NotImplementedError, match="cost_err on the combine output"):
        eng(model.replace("cost_err(out_h,lab)", "cost_err(out_c,lab)"))
    with pytest.raises(NotImplementedError, match="mse on the combine output"):
        eng(model.replace("loss_final=cost_nll(out_h,lab)",
                          "l1=cost_nll(out_h,lab)\nl2=mse(out_c,out_c)\nloss_final=sum(l1,l2)"))
    # a combine of LogSoftmax heads that has a consumer
    e_archs, e_dims = MC.ens_archs()
    e_nets, _, _ = build_nets(e_archs, e_dims)
    e_nets["MLP_h"], e_archs["MLP_h"] = NN.MLP(dict(archs["MLP_h"]), MC.N_LAB).to(DEV), archs["MLP_h"]
    with pytest.raises(NotImplementedError, match="combine of LogSoftmax heads that has a consumer"):
        eng(MC.MODEL_ENS.replace("loss_final=", "out_z=compute(MLP_h,out_e)\nloss_final="),
            nets=e_nets, archs=e_archs, fea=MC.FEA_SEQ)
    # in-place input quantisation: a quantising consumer of a combine output, and a combine operand
    # that another consumer quantises in place
    q = dict(archs["MLP_h"], mlp_quant="True", mlp_quant_inp="True", param_quant="8,8")
    q_nets = dict(nets, MLP_h=NN.MLP(q, 29).to(DEV))
    q_archs = dict(archs, MLP_h=q)
    with pytest.raises(NotImplementedError, match="in-place input quantisation"):
        eng(model, nets=q_nets, archs=q_archs)
    q24 = dict(q, arch_name="MLP_q24")
    q_nets2 = dict(nets, MLP_q24=NN.MLP(q24, 24).to(DEV))
    with pytest.raises(NotImplementedError, match="in-place input quantisation"):
        eng(model.replace("out_h=compute(MLP_h,out_c)", "out_h=compute(MLP_h,out_c)\n"
                          "out_y=compute(MLP_q24,out_a)"),
            nets=q_nets2, archs=dict(archs, MLP_q24=q24))
    # unequal widths outside concatenate
    with pytest.raises(NotImplementedError, match="only concatenate takes unequal widths"):
        eng(head + "out_c=concatenate(out_a,fc)\nbad=sum(out_c,out_a)" + tail)
    # a node read by a recurrent arch and by another consumer; by two recurrent archs
    s_archs, s_dims = MC.seq_sum_archs()
    s_nets, _, _ = build_nets(s_archs, s_dims)

    def seng(model, nets=s_nets, archs=s_archs):
        return Engine(nets, archs, parse_model(model), MC.FEA_SEQ, ["lab"], batch=MC.B_SEQ, max_len=8)

    with pytest.raises(NotImplementedError, match="read by a recurrent arch and by other archs"):
        seng(MC.MODEL_SEQ_SUM.replace("out_h=compute(MLP_h,out_r)",
                                      "res=concatenate(out_x,out_r)\nout_h=compute(MLP_h,out_r)"))
    y = dict(s_archs["liGRU_x"], arch_name="liGRU_y")
    with pytest.raises(NotImplementedError, match="read by two recurrent archs"):
        seng(MC.MODEL_SEQ_SUM.replace("out_h=compute", "out_r2=compute(liGRU_y,out_x)\nout_h=compute"),
             nets=dict(s_nets, liGRU_y=NN.liGRU(y, 12).to(DEV)), archs=dict(s_archs, liGRU_y=y))


# ------------------------------------------------------------------ nothing moved
def test_adjacent_feature_concatenate_is_still_a_column_range():
    from pkc.engine import Engine, parse_model, resolve_concat
    model = ("ab=concatenate(fa,fb)\nabc=concatenate(ab,fc)\nout_h=compute(MLP_w,abc)\n"
             "loss_final=cost_nll(out_h,lab)\nerr_final=cost_err(out_h,lab)")
    assert resolve_concat(parse_model(model), MC.FEA_FF)["abc"] == (0, 22)
    archs, _ = MC.ff_archs()
    w = dict(archs["MLP_h"], arch_name="MLP_w")
    nets, _, _ = build_nets({"MLP_w": w}, {"MLP_w": 22})
    eng = Engine(nets, {"MLP_w": w}, parse_model(model), MC.FEA_FF, ["lab"], batch=MC.B_FF)
    assert not any(getattr(n, "combine", False) for n in eng.nodes)
    assert eng.nodes[0].src == ("fea", 0, 22) and eng.fea_cols["abc"] == (0, 22)

"""The tiny models of the [model] tensor operations (concatenate / mult / sum / avg / sum_constant /
mult_constant on produced outputs, utils.py:2014-2043), in the reference's cfg schema.  Shared by
make_golden_model_ops.py (the reference's own model_init + forward_model + backward) and by
tests/test_model_ops_cpu.py / tests/test_gpu_model_ops.py (the restatement's and pkc's).

Feed-forward model, B = 12: three streams fa (11 columns), fb (6) and fc (5) in that order, so fc
starts at an odd column; one label stream of 10 classes.  out_a and out_b each feed two combine
nodes; the concatenate is 29 wide with a feature operand.

Sequence models, B = 3 sentences of 7, 5 and 4 frames: two bidirectional liGRUs (H = 8) on two
streams concatenated into an MLP head; and the sum of two MLPs feeding one liGRU."""
from cases import LIGRU_DEF, MLP_DEF

B_FF, N_LAB = 12, 10
FEA_FF = {"fa": (0, 11), "fb": (11, 17), "fc": (17, 22)}
LAB_FF = {"lab": 22}
B_SEQ, SEQ_LENS = 3, (7, 5, 4)
FEA_SEQ = {"fa": (0, 11), "fb": (11, 17)}
LAB_SEQ = {"lab": 17}

SGD = dict(arch_opt="sgd", arch_lr="0.05", opt_momentum="0.0", opt_weight_decay="0.0",
           opt_dampening="0.0", opt_nesterov="False", arch_freeze="False",
           arch_library="neural_networks", arch_pretrain_file="none")

MODEL_FF = ("out_a=compute(MLP_a,fa)\n"
            "out_b=compute(MLP_b,fb)\n"
            "out_s=sum(out_a,out_b)\n"
            "out_m=mult(out_a,out_b)\n"
            "out_v=avg(out_s,out_m)\n"
            "out_k=sum_constant(out_v,0.25)\n"
            "out_q=mult_constant(out_k,-1.5)\n"
            "out_c=concatenate(out_q,fc)\n"
            "out_h=compute(MLP_h,out_c)\n"
            "loss_final=cost_nll(out_h,lab)\n"
            "err_final=cost_err(out_h,lab)")
COMBINE_FF = ("out_s", "out_m", "out_v", "out_k", "out_q", "out_c")

MODEL_SEQ_CAT = ("out_r1=compute(liGRU_1,fa)\n"
                 "out_r2=compute(liGRU_2,fb)\n"
                 "out_c=concatenate(out_r1,out_r2)\n"
                 "out_h=compute(MLP_h,out_c)\n"
                 "loss_final=cost_nll(out_h,lab)\n"
                 "err_final=cost_err(out_h,lab)")
MODEL_SEQ_SUM = ("out_m1=compute(MLP_1,fa)\n"
                 "out_m2=compute(MLP_2,fb)\n"
                 "out_x=sum(out_m1,out_m2)\n"
                 "out_r=compute(liGRU_x,out_x)\n"
                 "out_h=compute(MLP_h,out_r)\n"
                 "loss_final=cost_nll(out_h,lab)\n"
                 "err_final=cost_err(out_h,lab)")
# the posterior ensemble of forward mode: the average of two heads' log posteriors
MODEL_ENS = ("out_h1=compute(MLP_e1,fa)\n"
             "out_h2=compute(MLP_e2,fb)\n"
             "out_e=avg(out_h1,out_h2)\n"
             "loss_final=cost_nll(out_h1,lab)\n"
             "err_final=cost_err(out_h1,lab)")


def _mlp(name, lay, act, drop=None, bn=None, ln=None, **kw):
    n = len(lay.split(","))
    return dict(MLP_DEF, **SGD, arch_name=name, arch_class="MLP", arch_seq_model="False",
                dnn_lay=lay, dnn_act=act, dnn_drop=drop or ",".join(["0.0"] * n),
                dnn_use_batchnorm=bn or ",".join(["False"] * n),
                dnn_use_laynorm=ln or ",".join(["False"] * n),
                param_quant=",".join(["8"] * n), mlp_prune_perc=",".join(["70"] * n), **kw)


def _ligru(name, **kw):
    return dict(LIGRU_DEF, **SGD, arch_name=name, arch_class="liGRU", arch_seq_model="True",
                ligru_lay="8", ligru_drop="0.0", ligru_use_laynorm="False",
                ligru_use_batchnorm="True", ligru_act="relu", **kw)


def ff_archs(drop="0.1"):
    """({arch: options}, {arch: input width}) of the feed-forward model."""
    return ({"MLP_a": _mlp("MLP_a", "24", "relu", drop=drop, bn="True"),
             "MLP_b": _mlp("MLP_b", "24", "tanh", ln="True"),
             "MLP_h": _mlp("MLP_h", "16,%d" % N_LAB, "relu,softmax")},
            {"MLP_a": 11, "MLP_b": 6, "MLP_h": 29})


def seq_cat_archs():
    return ({"liGRU_1": _ligru("liGRU_1"), "liGRU_2": _ligru("liGRU_2"),
             "MLP_h": _mlp("MLP_h", str(N_LAB), "softmax")},
            {"liGRU_1": 11, "liGRU_2": 6, "MLP_h": 32})


def seq_sum_archs():
    return ({"MLP_1": _mlp("MLP_1", "12", "relu"), "MLP_2": _mlp("MLP_2", "12", "tanh"),
             "liGRU_x": _ligru("liGRU_x"), "MLP_h": _mlp("MLP_h", str(N_LAB), "softmax")},
            {"MLP_1": 11, "MLP_2": 6, "liGRU_x": 12, "MLP_h": 16})


def ens_archs():
    return ({"MLP_e1": _mlp("MLP_e1", "14,%d" % N_LAB, "relu,softmax"),
             "MLP_e2": _mlp("MLP_e2", str(N_LAB), "softmax")},
            {"MLP_e1": 11, "MLP_e2": 6})

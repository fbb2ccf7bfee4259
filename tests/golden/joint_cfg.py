"""The tiny joint speech-enhancement + recognition recipe of the run_nn_joint golden case: the
chunk-cfg schema of cfg/TIMIT_baselines/TIMIT_joint_training_liGRU_fbank.cfg (two feature streams,
liGRU_SE -> MLP_SE (linear) -> liGRU_SR -> cd / mono heads, an mse between the enhanced features
and the clean stream) at test size.  Shared by make_golden_joint.py (the reference's run) and
tests/test_gpu_run_nn_joint.py / tests/test_joint_cpu.py (pkc's and the restatement's)."""
import configparser
import os

from cases import LIGRU_DEF, MLP_DEF

SECS = ("architecture1", "architecture2", "architecture3", "architecture4", "architecture5")
ARCHS = ("liGRU_SE", "MLP_SE", "liGRU_SR", "MLP_layers", "MLP_layers2")
FEA_DIM, N_CD, N_MONO = 13, 24, 6
SE_WEIGHT = "0.5"          # not 1.0, so a dropped weight shows

MODEL = ("out_dnn1=compute(liGRU_SE,fbank_rev)\n"
         "out_dnn_SE=compute(MLP_SE,out_dnn1)\n"
         "out_dnn2=compute(liGRU_SR,out_dnn_SE)\n"
         "out_dnn3=compute(MLP_layers,out_dnn2)\n"
         "out_dnn4=compute(MLP_layers2,out_dnn2)\n"
         "loss_mono=cost_nll(out_dnn4,lab_mono)\n"
         "loss_mono_w=mult_constant(loss_mono,1.0)\n"
         "loss_se=mse(out_dnn_SE,fbank_clean)\n"
         "loss_se_w=mult_constant(loss_se," + SE_WEIGHT + ")\n"
         "loss_cd=cost_nll(out_dnn3,lab_cd)\n"
         "loss_sum1=sum(loss_cd,loss_mono_w)\n"
         "loss_final=sum(loss_sum1,loss_se_w)\n"
         "err_final=cost_err(out_dnn3,lab_cd)")

OPT = dict(arch_opt="rmsprop", arch_lr="0.0004", opt_momentum="0.0", opt_alpha="0.95",
           opt_eps="1e-8", opt_centered="False", opt_weight_decay="0.0")


def arch_sections(d="/tmp", to_do="train"):
    """{section: options} of the five architectures."""
    common = dict(arch_library="neural_networks", arch_freeze="False", out_folder=d,
                  arch_pretrain_file="none", use_cuda="False", to_do=to_do, **OPT)
    rec = dict(LIGRU_DEF, **common, arch_class="liGRU", arch_seq_model="True", ligru_lay="12,12")
    mlp = dict(MLP_DEF, **common, arch_class="MLP", arch_seq_model="False",
               dnn_use_batchnorm="False")
    return {"architecture1": dict(rec, arch_name="liGRU_SE"),
            "architecture2": dict(mlp, arch_name="MLP_SE", dnn_lay=str(FEA_DIM), dnn_act="linear"),
            "architecture3": dict(rec, arch_name="liGRU_SR"),
            "architecture4": dict(mlp, arch_name="MLP_layers", dnn_lay=str(N_CD),
                                  dnn_act="softmax"),
            "architecture5": dict(mlp, arch_name="MLP_layers2", dnn_lay=str(N_MONO),
                                  dnn_act="softmax")}


def joint_cfg(d, name, to_do, base, pretrain=None, counts="none",
              forward_out="out_dnn_SE,out_dnn3", normalize="False,True"):
    """A chunk cfg of the joint recipe.  base: the chunk's path stem — the streams' lists are
    <base>_rev and <base>_clean, the alignments <base>.ali; pretrain: {section: pkl path}.
    (The reference's forward_model stops at the LAST name of forward_out, utils.py:1932, so with
    the reference that one must be the output computed last.)"""
    cfg = configparser.ConfigParser()
    cfg["exp"] = {"seed": "2234", "out_folder": d, "use_cuda": "False", "multi_gpu": "False",
                  "to_do": to_do, "out_info": os.path.join(d, name + ".info"),
                  "save_gpumem": "False", "production": "False", "run_nn_script": "run_nn.py"}
    cfg["batches"] = {"batch_size_train": "3", "batch_size_valid": "3",
                      "max_seq_length_train": "1000", "max_seq_length_valid": "1000"}
    cfg["data_chunk"] = {
        "fea": "fea_name=fbank_clean\nfea_lst=%s_clean\nfea_opts=\ncw_left=0\ncw_right=0\n\n"
               "fea_name=fbank_rev\nfea_lst=%s_rev\nfea_opts=\ncw_left=0\ncw_right=0\n"
               % (base, base),
        "lab": "lab_name=lab_cd\nlab_folder=%s\nlab_opts=ali-to-pdf\n\n"
               "lab_name=lab_mono\nlab_folder=%s\nlab_opts=ali-to-phones --per-frame=true\n"
               % (base + ".ali", base + ".ali")}
    for sec, a in arch_sections(d, to_do).items():
        cfg[sec] = a
        if pretrain:
            cfg[sec]["arch_pretrain_file"] = pretrain[sec]
    cfg["model"] = {"model": MODEL}
    n = len(forward_out.split(","))
    cfg["forward"] = {"forward_out": forward_out, "normalize_posteriors": normalize,
                      "normalize_with_counts_from": ",".join(
                          counts if s == "True" else "none" for s in normalize.split(",")),
                      "save_out_file": ",".join(["True"] * n),
                      "require_decoding": ",".join(
                          "True" if s == "True" else "False" for s in normalize.split(","))}
    path = os.path.join(d, name + ".cfg")
    with open(path, "w") as f:
        cfg.write(f)
    return path

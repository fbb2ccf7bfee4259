"""CPU checks of the [model] tensor operations: (a) the tests' restatement (tests/model_ops_ref.py)
reproduces what the reference's own model_init + forward_model + backward wrote into
tests/golden/model_ops/*.npz — every named output, the loss and every parameter gradient, bit for
bit: eager torch on both sides runs the same fp32 operations in the same order, and the generator
recorded that every tensor was reproduced exactly (equal/<key>); (b) the CombineArgs ctypes mirror
has the layout of pkc_combine_args (the gcc probe of tests/test_abi_layout.py for this one struct,
which that file's fixed list does not hold).  No GPU, no HIP."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT


def _restated(tag):
    import model_ops_cfg as MC
    import model_ops_ref as MR
    from oracle.run import parse_model
    g = np.load(os.path.join(GOLDEN, "model_ops", tag + ".npz"))
    if tag == "ff":
        (archs, dims), model = MC.ff_archs(drop="0.0"), MC.MODEL_FF
        fea, lab, T, B = MC.FEA_FF, MC.LAB_FF, 0, MC.B_FF
    else:
        (archs, dims), model = MC.seq_cat_archs(), MC.MODEL_SEQ_CAT
        fea, lab, T, B = MC.FEA_SEQ, MC.LAB_SEQ, max(MC.SEQ_LENS), MC.B_SEQ
    nets, _, seq = MR.build(archs, dims, state=MR.golden_state(g, archs))
    outs = MR.forward_model(parse_model(model), nets, seq, fea, lab, torch.from_numpy(g["inp"]), T, B)
    outs["loss_final"].backward()
    got = {"out/" + k: v.detach() for k, v in outs.items() if k not in fea}
    for a, net in nets.items():
        for pn, p in net.named_parameters():
            if p.grad is not None:
                got["grad/%s/%s" % (a, pn)] = p.grad
    return g, got


@pytest.mark.parametrize("tag", ["ff", "seq"])
def test_restatement_reproduces_the_reference(tag):
    g, got = _restated(tag)
    keys = [k for k in g.files if k.startswith(("out/", "grad/"))]
    assert len(keys) >= 20 and "out/loss_final" in keys and "out/out_c" in keys
    assert sorted(keys) == sorted(got)
    for k in keys:
        assert bool(g["equal/" + k]), "%s was not bit-equal when the fixture was written" % k
        ref = torch.from_numpy(g[k])
        assert got[k].dtype == torch.float32
        assert torch.equal(got[k].reshape(ref.shape), ref), k
    if tag == "ff":         # every operation of the DSL is in the fixture
        for name in ("out_s", "out_m", "out_v", "out_k", "out_q", "out_c"):
            assert "out/" + name in keys
        a, b = torch.from_numpy(g["out/out_a"]), torch.from_numpy(g["out/out_b"])
        assert torch.equal(torch.from_numpy(g["out/out_v"]), ((a + b) + a * b) / 2)
        assert g["out/out_c"].shape == (12, 29)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_combine_args_layout_matches_header(tmp_path):
    from pkc import _lib as L
    cls, cname = L.CombineArgs, "pkc_combine_args"
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "pkc.h"', "int main(void) {",
             'printf("%%zu\\n", sizeof(%s));' % cname]
    expect = [("sizeof " + cname, C.sizeof(cls))]
    for f in cls._fields_:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, f[0]))
        expect.append(("%s.%s" % (cname, f[0]), getattr(cls, f[0]).offset))
    for name, v in L.COMBINE.items():
        cn = {"concatenate": "CONCAT", "sum_constant": "SUM_CONST",
              "mult_constant": "MULT_CONST"}.get(name, name.upper())
        lines.append('printf("%%d\\n", (int)PKC_COMBINE_%s);' % cn)
        expect.append(("PKC_COMBINE_" + cn, v))
    lines += ["return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert len(got) == len(expect)
    bad = [(k, v, g) for (k, v), g in zip(expect, got) if v != g]
    assert not bad, "ctypes vs C (name, ctypes, C): %s" % bad


def test_resolve_concat_keeps_adjacent_streams_and_leaves_the_rest():
    from pkc.engine import parse_model, resolve_concat
    cols = {"fa": (0, 11), "fb": (11, 17), "fc": (17, 22)}
    lines = parse_model("ab=concatenate(fa,fb)\nabc=concatenate(ab,fc)\nac=concatenate(fa,fc)\n"
                        "o=compute(net,abc)\nco=concatenate(o,fc)")
    got = resolve_concat(lines, cols)
    assert got["ab"] == (0, 17) and got["abc"] == (0, 22)
    assert "ac" not in got and "co" not in got        # nodes of the graph, not column ranges

"""The engine's explicit types (no GPU): the Node contract of pkc.graph (one base class whose
class-level defaults are what the engine may read on any node), the Op launch operation of
pkc.engine, and the module layout — the graph vocabulary in pkc.graph (importable without
pkc.engine), the forward runners in pkc.runners, and every kernel-form switch that the tests assign
still an attribute of pkc.engine and of no other module."""
import ast
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-kaldi-cgs_amd")
sys.path.insert(0, PKG)

KINDS = ("rec", "conv", "combine")
# module globals of pkc.engine that tests and scripts assign to flip a kernel form
SWITCHES = ("BN_BWD_EPI", "DW_SPLIT_ROWS", "FUSED_FWD", "OPT_DIRECT", "OPT_FWD", "RNN_BF16_SPARSE",
            "RNN_PERSIST", "RNN_QH_EXACT", "RNN_SPARSE", "SEQ_CAPTURE_AFTER", "W_SPARSE",
            "W_SPARSE_MAX_FRAC")
# what tests, scripts and bench.py imported from pkc.engine before the graph vocabulary moved out
ENGINE_NAMES = ("CombineNode", "Engine", "MAX_SPLITS", "RegTerm", "SeqBatch", "_splits",
                "ktile_table", "parse_model", "resolve_concat", "torch_optimizer", "MseTerm",
                "Layer", "NormLayer", "ConvNode", "RecNode", "StdRecNode", "Node", "TENSOR_OPS",
                "conv_args", "sinc_bind", "sinc_args", "conv_post_args", "pattern_effective_masks",
                "persist_plans", "persist_geometry", "Op")


def _declared(cls):
    return {k: v for k, v in vars(cls).items() if not k.startswith("__") and not callable(v)}


def _classes():
    import pkc.graph as G
    return G, (G.Layer, G.NormLayer, G.CombineNode, G.ConvNode, G.RecNode, G.StdRecNode)


def test_node_classes_share_one_base_and_its_defaults():
    G, classes = _classes()
    decl = _declared(G.Node)
    for group in (("rec", "conv", "combine", "std", "head"),
                  ("W", "b", "mask", "Wq", "W_h", "qbits", "ibits", "reads", "bn", "ln", "act",
                   "drop", "arch"),
                  ("rec_consumer", "gsrc", "out_h", "dz_h", "bn_states", "bn_sums", "bnb_epi",
                   "keep", "sdw", "f32_dead", "dz_scratch", "bnb_now", "mse_grad")):
        assert set(group) <= set(decl), set(group) - set(decl)
    assert all(decl[k] is False for k in ("rec", "conv", "combine", "std", "head", "bn", "ln",
                                          "f32_dead", "dz_scratch", "bnb_now"))
    assert all(decl[k] is None for k in ("W", "b", "mask", "Wq", "W_h", "arch", "rec_consumer",
                                         "gsrc", "out_h", "dz_h", "bn_states", "bn_sums", "bnb_epi",
                                         "keep"))
    assert (decl["qbits"], decl["ibits"], decl["reads"], decl["sdw"]) == (0, 0, 0, 1)
    assert (decl["act"], decl["drop"], decl["mse_grad"]) == ("linear", 0.0, ())
    for cls in classes:
        assert issubclass(cls, G.Node)
        own = {k for c in cls.__mro__ if c not in (G.Node, object) for k in _declared(c)}
        assert own <= {"rec", "conv", "combine", "std"}, (cls.__name__, own)   # kind flags only
        for k, v in decl.items():
            if k not in own:
                assert getattr(cls, k) is v, (cls.__name__, k)


def test_kind_flags():
    G, _ = _classes()
    want = {G.Layer: (), G.NormLayer: (), G.RecNode: ("rec",), G.StdRecNode: ("rec",),
            G.ConvNode: ("conv",), G.CombineNode: ("combine",)}
    for cls, kinds in want.items():
        assert tuple(k for k in KINDS if getattr(cls, k)) == kinds, cls.__name__
        assert cls.std is (cls is G.StdRecNode), cls.__name__


def test_wiring_is_per_instance_and_nodes_are_identity_keys():
    G, classes = _classes()
    for cls in (G.Node,) + classes:
        assert not hasattr(cls, "consumers"), cls.__name__       # never a shared class-level list
    a = G.CombineNode("o1", "sum", [("fea", 0, 4), ("fea", 4, 8)], [4, 4])
    b = G.CombineNode("o1", "sum", [("fea", 0, 4), ("fea", 4, 8)], [4, 4])
    assert a.consumers == [] and a.consumers is not b.consumers
    assert (a.src, a.label_col, a.loss_weight) == (None, None, 0.0)
    a.consumers.append(b)
    assert b.consumers == []
    for cls in (G.Node,) + classes:
        assert cls.__eq__ is object.__eq__ and cls.__hash__ is object.__hash__, cls.__name__
    assert a != b and a == a and hash(a) != hash(b)
    d = {a: 1, b: 2}
    assert d[a] == 1 and d[b] == 2 and len(d) == 2


def test_op_is_a_five_field_tuple():
    from pkc.engine import Op
    prob = object()
    op = Op("x", 1.0, 2.0, None)
    assert op.half is None and len(op) == 5
    op = Op("x", 1.0, 2.0, prob)
    assert tuple(op)[3] is op.prob is prob and op[0] == op.label and op[2] == op.nbytes == 2.0
    assert Op._fields == ("label", "flops", "nbytes", "prob", "half")


def test_op_on_half_substitutes_the_bf16_problem():
    from pkc.engine import Op
    prob, hprob = object(), object()
    op = Op("fwd 8x8x8", 1024.0, 768.0, prob, (384.0, hprob))
    h = op.on_half()
    assert (h.label, h.flops, h.nbytes) == ("fwd 8x8x8", 1024.0, 384.0)
    assert h.prob is hprob and h.half is None
    assert op.prob is prob and op.nbytes == 768.0          # the original is unchanged


def _engine_imports(path):
    with open(path) as f:
        tree = ast.parse(f.read())
    return {a.name for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)
            and n.module == "pkc.engine" for a in n.names}


def test_names_still_resolve_on_pkc_engine():
    import pkc.engine as E
    import pkc.graph as G
    import pkc.runners as R
    files = (glob.glob(os.path.join(ROOT, "tests", "*.py"))
             + glob.glob(os.path.join(ROOT, "scripts", "*.py"))
             + [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")])
    names = set(ENGINE_NAMES) | set(SWITCHES)
    for f in files:
        names |= _engine_imports(f)
    assert len(names) > len(ENGINE_NAMES)
    for name in sorted(names):
        assert hasattr(E, name), name
    for name in ("ForwardRunner", "ModuleRunner", "ConvRunner", "torch_optimizer"):
        assert hasattr(R, name), name
    assert R.torch_optimizer is E.torch_optimizer
    for name in ("Node", "Layer", "CombineNode", "RegTerm", "SeqBatch", "parse_model"):
        assert getattr(E, name) is getattr(G, name), name      # re-exported, not copied


def test_switches_live_in_pkc_engine_only():
    """A switch copied into another module at import would leave `E.<SWITCH> = ...` in a two-form
    parity test without effect there."""
    import pkc.engine as E
    import pkc.graph as G
    import pkc.runners as R
    upper = {k for k in vars(E) if k.isupper() and not k.startswith("_")
             and isinstance(getattr(E, k), (bool, int, float, str))}
    assert set(SWITCHES) <= upper
    for k in upper:
        assert not hasattr(G, k), k
        assert not hasattr(R, k) or k == "MAX_SPLITS", k       # a buffer size no test assigns


def test_graph_imports_without_engine():
    code = ("import sys; sys.path.insert(0, %r); import pkc.graph; "
            "assert 'pkc.engine' not in sys.modules and 'pkc.runners' not in sys.modules; "
            "import pkc.engine; assert 'pkc.runners' not in sys.modules" % PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

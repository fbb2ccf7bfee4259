"""The streams of the B = 128 step's gradient and update launches: how the optimizer work items and
the small matmul body's fp32 tile epilogue move their bytes (store widths, cache policies) must not
change a bit of what they store, nor touch a byte next to it.  Every output buffer here sits between
canary regions that are compared afterwards."""
import configparser
import ctypes as C

import numpy as np
import pytest
import torch

from cases import MLP_DEF

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64                      # canary elements on each side (keeps the 16-byte alignment)
CANARY = {torch.float32: (torch.int32, 0x7FC0ABCD), torch.bfloat16: (torch.int16, 0x7FCD)}
ITEM = 2048                   # elements per optimizer work item (pkc_optim_chunks)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    from pkc import _lib
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _lib.lib()
    return _lib


class Guarded:
    """n elements at an element offset `shift` from a 16-byte boundary, between two canary regions."""

    def __init__(self, n, dtype=torch.float32, shift=0, init=None):
        it, self.can = CANARY[dtype]
        self.lo, self.n = PAD + shift, n
        self.buf = torch.empty(self.lo + n + PAD, dtype=dtype, device=DEV)
        self.bits = self.buf.view(it)
        self.bits.fill_(self.can)
        self.v = self.buf[self.lo:self.lo + n]
        if init is not None:
            self.v.copy_(init)

    def ptr(self):
        return self.v.data_ptr()

    def check(self, what):
        assert bool((self.bits[:self.lo] == self.can).all()), "%s: bytes in front touched" % what
        assert bool((self.bits[self.lo + self.n:] == self.can).all()), "%s: bytes behind touched" % what

    def host(self):
        return self.v.cpu().clone()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------
# update items

OPTS = {
    "sgd": dict(kind=0, lr=0.08),
    "sgd_mom": dict(kind=0, lr=0.05, momentum=0.9, nesterov=1, wd=1e-3),
    "rmsprop": dict(kind=1, lr=4e-4, alpha=0.95, eps=1e-8),
    "rmsprop_centered_mom": dict(kind=1, lr=4e-4, alpha=0.95, eps=1e-8, centered=1, momentum=0.9),
    "adam_amsgrad": dict(kind=2, lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-8, amsgrad=1),
}
STATES = {"sgd": (), "sgd_mom": (1,), "rmsprop": (1,), "rmsprop_centered_mom": (1, 2, 3),
          "adam_amsgrad": (1, 2, 3)}


def torch_opt(kind, params):
    if kind == "sgd":
        return torch.optim.SGD(params, lr=0.08)
    if kind == "sgd_mom":
        return torch.optim.SGD(params, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-3)
    if kind == "rmsprop":
        return torch.optim.RMSprop(params, lr=4e-4, alpha=0.95, eps=1e-8)
    if kind == "rmsprop_centered_mom":
        return torch.optim.RMSprop(params, lr=4e-4, alpha=0.95, eps=1e-8, centered=True, momentum=0.9)
    return torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.98), eps=1e-8, amsgrad=True)


# (n, mask, qbits, bout: None / element offset of the bf16 copy from a 16-byte boundary)
#   8: one thread's 8 elements; 2048: one whole item; 2056: one item + 8; 6140: n % 8 == 4, the last
#   thread's half-filled tail; 2052: the same tail in an item's first vectors; 4099: n % 4 != 0,
#   the scalar path.  bout offset 4: 8-byte but not 16-byte aligned.
CASES = [(8, True, 8, 0), (2048, False, 0, 0), (2056, True, 0, 0), (6140, False, 8, 0),
         (4099, True, 8, 0), (2056, False, 0, 4), (6140, True, 0, 4), (6140, False, 0, None),
         (2048, True, 8, None), (8, False, 0, 4), (2052, False, 0, 0)]
NSTEP = 2


def run_updates(L, kind, form, pshift):
    """Every case through NSTEP steps of the update, form = "map" (pkc_optim_step) or "direct"
    (PKC_OP_OPTIM runs of pkc_gemm_grouped); pshift = 1 puts p one element off the 16-byte boundary
    (the scalar path) on the same values.  Returns per case {name: host tensor}."""
    g = torch.Generator().manual_seed(5)
    T = []
    for n, mask, qbits, bo in CASES:
        p0 = torch.randn(n, generator=g)
        m = (torch.rand(n, generator=g) > 0.5).float() if mask else None
        gr = [torch.randn(n, generator=g) for _ in range(NSTEP)]
        if m is not None:
            p0 = p0 * m
        t = dict(n=n, qbits=qbits, p0=p0, m=m, gr=gr,
                 p=Guarded(n, shift=pshift, init=p0), g=Guarded(n),
                 mask=Guarded(n, init=m) if mask else None,
                 q=Guarded(n) if qbits else None,
                 b=Guarded(n, torch.bfloat16, shift=bo) if bo is not None else None)
        # the map form reads the first state from the kind alone; every form gets a buffer there
        for k in (1, 2, 3):
            keep = k in STATES[kind] or (k == 1 and form == "map")
            t["s%d" % k] = Guarded(n, init=torch.zeros(n)) if keep else None
        T.append(t)
    nt = len(T)
    sizes = (C.c_int64 * nt)(*[t["n"] for t in T])
    nch = L.lib().pkc_optim_chunks(sizes, nt, None, 0)
    cmap = (C.c_int32 * (2 * nch))()
    L.lib().pkc_optim_chunks(sizes, nt, cmap, nch)
    dmap = torch.from_numpy(np.frombuffer(cmap, dtype=np.int32).copy()).to(DEV)

    def opt_ptr(x):
        return x.ptr() if x is not None else None

    for step in range(NSTEP):
        arr = (L.OptTensor * nt)()
        for i, t in enumerate(T):
            d = arr[i]
            d.p, d.g, d.n, d.step = t["p"].ptr(), t["g"].ptr(), t["n"], step + 1
            d.s1, d.s2, d.s3 = opt_ptr(t["s1"]), opt_ptr(t["s2"]), opt_ptr(t["s3"])
            d.mask, d.qout, d.qbits, d.bout = (opt_ptr(t["mask"]), opt_ptr(t["q"]), t["qbits"],
                                               opt_ptr(t["b"]))
            for k, v in OPTS[kind].items():
                setattr(d, k, v)
            t["g"].v.copy_(t["gr"][step])
        desc = torch.frombuffer(bytearray(C.string_at(arr, C.sizeof(arr))), dtype=torch.uint8).to(DEV)
        if form == "map":
            L.call("pkc_optim_step", L.ptr(desc), nt, L.ptr(dmap), nch, _s())
        else:
            for i0 in range(0, nt, L.OPT_SEGS_MAX):          # one launch per 8 single-tensor runs
                grp = T[i0:i0 + L.OPT_SEGS_MAX]
                segs = (L.OptSeg * len(grp))()
                for k, t in enumerate(grp):
                    sg = segs[k]
                    sg.tensor, sg.chunk0, sg.nchunks = i0 + k, 0, (t["n"] + ITEM - 1) // ITEM
                    sg.p, sg.g, sg.n = t["p"].ptr(), t["g"].ptr(), t["n"]
                    sg.s1 = opt_ptr(t["s1"]) if 1 in STATES[kind] else None
                    sg.s2, sg.s3, sg.mask = opt_ptr(t["s2"]), opt_ptr(t["s3"]), opt_ptr(t["mask"])
                    sg.qout, sg.bout = opt_ptr(t["q"]), opt_ptr(t["b"])
                pr = L.GemmProblem(kind=L.OP_OPTIM, M=sum(s.nchunks for s in segs),
                                   A=desc.data_ptr(), X1=C.addressof(segs), N=len(grp))
                L.call("pkc_gemm_grouped", L.PREC_BF16IN, C.byref(pr), 1, _s())
        torch.cuda.synchronize()
    out = []
    for i, t in enumerate(T):
        r = {}
        for name in ("p", "s1", "s2", "s3", "q", "b", "g", "mask"):
            if t[name] is not None:
                t[name].check("%s %s case %d %s" % (kind, form, i, name))
                if name not in ("g", "mask") and not (name == "s1" and 1 not in STATES[kind]):
                    r[name] = t[name].host()
        out.append(r)
    return out, T


@pytest.fixture(scope="module")
def update_refs():
    """torch.optim on the CPU over the cases' values, once per optimizer."""
    cache = {}

    def get(kind, T):
        if kind not in cache:
            ref = [t["p0"].clone().requires_grad_(True) for t in T]
            opt = torch_opt(kind, ref)
            for step in range(NSTEP):
                for r, t in zip(ref, T):
                    r.grad = t["gr"][step].clone()
                opt.step()
                with torch.no_grad():
                    for r, t in zip(ref, T):
                        if t["m"] is not None:
                            r.mul_(t["m"])
            cache[kind] = [r.detach() for r in ref]
        return cache[kind]
    return get


@pytest.fixture(scope="module")
def update_runs(L):
    """Every case through both forms and both paths, once per optimizer."""
    cache = {}

    def get(kind):
        if kind not in cache:
            runs = {}
            for form in ("map", "direct"):
                for pshift in (0, 1):
                    runs[form, pshift], T = run_updates(L, kind, form, pshift)
            cache[kind] = (runs, T)
        return cache[kind]
    return get


def assert_same_bits(kind, a_key, b_key, runs):
    for i, (a, b) in enumerate(zip(runs[a_key], runs[b_key])):
        assert a.keys() == b.keys()
        for name in a:
            assert torch.equal(bits(a[name]), bits(b[name])), (kind, a_key, b_key, CASES[i], name)


@pytest.mark.parametrize("kind", list(OPTS))
def test_update_items(L, update_runs, update_refs, kind):
    """Map form and direct form, on the vector path and on the scalar path (p one element off): p,
    the optimizer states, the quantised copy and the bf16 operand copy are bitwise equal between
    the forms, p is within test_optimizer_step_matches_torch's bound of torch.optim, the quantised
    copy is Quantize(p) and the bf16 copy is the rounding of the stored fp32 p; no canary byte is
    touched (checked in run_updates)."""
    runs, T = update_runs(kind)
    ref = update_refs(kind, T)
    for pshift in (0, 1):
        assert_same_bits(kind, ("map", pshift), ("direct", pshift), runs)
        for i, r in enumerate(runs["map", pshift]):
            torch.testing.assert_close(r["p"], ref[i], rtol=1e-5, atol=1e-6)
            if "b" in r:
                assert torch.equal(bits(r["b"]), bits(r["p"].bfloat16())), (kind, CASES[i], "bout")
            if "q" in r:
                sc = 2.0 ** (CASES[i][2] - 1)
                q = torch.ceil(r["p"].abs() * sc) / sc * torch.sign(r["p"])
                assert torch.equal(bits(r["q"]), bits(q)), (kind, CASES[i], "qout")
            for k in STATES[kind]:
                assert "s%d" % k in r and bool(torch.isfinite(r["s%d" % k]).all())


@pytest.mark.parametrize("kind", list(OPTS))
def test_update_items_vector_equals_scalar(L, update_runs, kind):
    """The vector path (16-byte accesses) and the scalar path (p one element off the 16-byte
    boundary) on the same values: p, states, quantised and bf16 copies bitwise equal.  (RMSprop's
    two-product sums are spelled as one fused form in opt_update for this: left to the compiler,
    the two paths rounded square_avg differently by one unit in the last place.)"""
    runs, _ = update_runs(kind)
    for form in ("map", "direct"):
        assert_same_bits(kind, (form, 0), (form, 1), runs)


# ---------------------------------------------------------------------------------------------
# tile epilogue

def _tol(prec, K):      # test_gemm_grouped's bound (tests/test_gpu_kernels.py)
    return {0: 2e-5, 1: 1e-3, 2: 1e-3, 3: 6e-5}[prec] * K ** 0.5


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("M,N,K", [(72, 40, 24), (128, 120, 128), (64, 64, 32)])
def test_tile_epilogue(L, prec, M, N, K):
    """The 64x64 body's fp32 tile store: 16-byte row stores where ldc and C allow them (ldc = N,
    N + 4) against the 4-byte form (ldc = N + 3, C one float off), grouped and standalone, forward
    (nt) and dW (tn) orientation, with and without split-K slabs: bitwise equal to each other,
    within test_gemm_grouped's bound of the fp64 product of the rounded operands, and nothing
    stored outside the M x N block of each slab."""
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g)
    if prec == 2:
        A, B = A.bfloat16().float(), B.bfloat16().float()
    ref = (A.double() @ B.double().t()).float()
    _, can = CANARY[torch.float32]
    outs = {}
    for orient in ("nt", "tn"):
        akc, bkc = {"nt": (1, 1), "tn": (0, 0)}[orient]
        Ast = A if akc else A.t().contiguous()
        Bst = B if bkc else B.t().contiguous()
        Ad, Bd = Ast.to(DEV), Bst.to(DEV)
        if prec == 2:
            Ad, Bd = Ad.bfloat16().contiguous(), Bd.bfloat16().contiguous()
        for splits in (1, 2):
            layouts = [(N, 0), (N + 4, 0), (N + 3, 0), (N, 1)]       # (ldc, C offset in floats)
            bufs, probs = [], []
            for ldc, off in layouts:
                gd = Guarded(splits * M * ldc, shift=off)
                bufs.append(gd)
                probs.append(L.GemmProblem(a_kcontig=akc, b_kcontig=bkc, M=M, N=N, K=K, splits=splits,
                                           A=Ad.data_ptr(), lda=Ast.shape[1], B=Bd.data_ptr(),
                                           ldb=Bst.shape[1], C=gd.ptr(), ldc=ldc,
                                           slab_stride=M * ldc))
            arr = (L.GemmProblem * len(probs))(*probs)
            L.call("pkc_gemm_grouped", prec, arr, len(probs), _s())
            for ldc, off in layouts:                                  # the same, standalone
                gd = Guarded(splits * M * ldc, shift=off)
                bufs.append(gd)
                L.call("pkc_gemm", prec, akc, bkc, M, N, K, L.ptr(Ad), Ast.shape[1], L.ptr(Bd),
                       Bst.shape[1], C.c_void_p(gd.ptr()), ldc, splits, M * ldc, _s())
            torch.cuda.synchronize()
            for j, gd in enumerate(bufs):
                ldc, off = layouts[j % len(layouts)]
                what = "%s splits=%d %s ldc=%d off=%d" % (orient, splits, "grouped" if j < 4 else
                                                          "standalone", ldc, off)
                gd.check(what)
                full = gd.v.view(splits, M, ldc)
                pad = bits(full[:, :, N:].cpu())
                assert bool((pad == can).all()), what + ": columns >= N touched"
                outs[orient, splits, j] = full[:, :, :N].cpu().contiguous()
    # the four layouts of one launch form hold the same bits (the forms themselves may order their
    # k-tiles differently), and every one is within the bound
    for (orient, sp, j), o in outs.items():
        base = outs[orient, sp, j - j % 4]
        assert torch.equal(bits(o), bits(base)), (orient, sp, j)
        torch.testing.assert_close(o.sum(0), ref, rtol=1e-4, atol=_tol(prec, K))


# ---------------------------------------------------------------------------------------------
# engine

def toy_config():
    """C2-shaped toy: 24 -> 2 x 64 BatchNorm / relu / dropout -> heads 40 + 8; SGD body, RMSprop
    heads."""
    cfg = configparser.ConfigParser()
    body = dict(MLP_DEF, arch_name="MLP_layers1", dnn_lay="64,64", dnn_drop="0.15,0.15",
                dnn_use_batchnorm="True,True", dnn_use_laynorm="False,False", dnn_act="relu,relu",
                param_quant="8,8", arch_lr="0.08", arch_opt="sgd", opt_momentum="0.0",
                opt_weight_decay="0.0", opt_dampening="0.0", opt_nesterov="False", arch_freeze="False")
    head = dict(MLP_DEF, arch_name="MLP_layers2", dnn_lay="40", dnn_act="softmax",
                dnn_use_batchnorm="False", arch_lr="0.0004", arch_opt="rmsprop", opt_momentum="0.0",
                opt_alpha="0.95", opt_eps="1e-8", opt_centered="False", opt_weight_decay="0.0",
                arch_freeze="False")
    mono = dict(head, arch_name="MLP_layers3", dnn_lay="8")
    cfg["architecture1"], cfg["architecture2"], cfg["architecture3"] = body, head, mono
    cfg["model"] = {"model": "out_dnn1=compute(MLP_layers1,fmllr)\n"
                             "out_dnn2=compute(MLP_layers2,out_dnn1)\n"
                             "out_dnn3=compute(MLP_layers3,out_dnn1)\n"
                             "loss_mono=cost_nll(out_dnn3,lab_mono)\n"
                             "loss_mono_w=mult_constant(loss_mono,1.0)\n"
                             "loss_cd=cost_nll(out_dnn2,lab_cd)\n"
                             "loss_final=sum(loss_cd,loss_mono_w)\n"
                             "err_final=cost_err(out_dnn2,lab_cd)"}
    return cfg


def test_engine_toy_graphs_equal_eager(L):
    """12 bf16 steps of the toy: multi-step graphs (4 steps each) against eager steps, bit-identical
    weights, BatchNorm statistics, optimizer state and loss totals; afterwards every layer's bf16
    operand copy is the rounding of its fp32 weights."""
    from pkc.engine import Engine, parse_model
    from pkc.neural_networks import MLP
    cfg = toy_config()
    B, NB, STEPS = 16, 4, 12
    rs = np.random.RandomState(4)
    X = torch.from_numpy(rs.randn(B * NB, 24).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(np.stack([rs.randint(0, 40, B * NB), rs.randint(0, 8, B * NB)], 1)
                           .astype(np.int32)).to(DEV)
    res = []
    for graphs in (False, True):
        torch.manual_seed(2234)
        np.random.seed(2234)
        nets, opts = {}, {}
        for sec, inp in (("architecture1", 24), ("architecture2", 64), ("architecture3", 64)):
            o = cfg[sec]
            nets[o["arch_name"]] = MLP(o, inp)
            opts[o["arch_name"]] = o
            nets[o["arch_name"]].to(DEV).train()
        eng = Engine(nets, opts, parse_model(cfg["model"]["model"]), {"fmllr": (0, 24)},
                     ["lab_cd", "lab_mono"], batch=B, prec=L.PREC_BF16, seed=3)
        eng.bind_chunk(X, lab, B * NB)
        if graphs:
            assert eng.capture(steps_per_graph=4)
            eng.ctr.zero_()
            eng.loss_acc.zero_()
            eng.train_steps(STEPS)
        else:
            for _ in range(STEPS):
                eng.train_step()
        torch.cuda.synchronize()
        eng.sync_state()
        st = {"loss_totals": torch.tensor(eng.chunk_totals(), dtype=torch.float64)}
        for a, net in nets.items():
            for k, v in net.state_dict().items():
                st["%s/%s" % (a, k)] = v.detach().cpu().clone()
            for pi, d in eng.optimizer_state_dict(a)["state"].items():
                for k, v in d.items():
                    st["%s/opt%d/%s" % (a, pi, k)] = torch.as_tensor(v).cpu().clone()
        copies = 0
        for e in eng.opt_entries:
            if e.get("bout") is not None:
                copies += 1
                want = e["p"].detach().reshape(-1).bfloat16()
                assert torch.equal(bits(e["bout"].reshape(-1)), bits(want)), e["arch"]
        assert copies == 4, copies              # two body layers and two heads
        res.append(st)
    assert res[0].keys() == res[1].keys()
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k

"""Cases, inputs and the float64 reference for the kernel-level tests of pkc_nll_fused
(tests/test_gpu_loss.py on the GPU, tests/test_loss_ref_cpu.py for what can be checked without one).

pkc_loss.hip dispatches pkc_nll_fused to 18 kernels.  pkc_nll_form names the one a call takes:
  0..15  register-resident: 8 * (16-byte accesses) + 4 * (four waves per row) + log2(slab capacity)
  -1     the general form, one wave per row   (more than 8 slabs, N < 512)
  -2     the general form, four waves per row (more than 8 slabs or N > 2048, N >= 512)
Every case below states the form it is meant to take, and the GPU test asserts it on the real
pointers, so the table cannot stop reaching a form without a test failing.

Everything here runs on the CPU; nothing imports the library."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch

EPS23 = 2.0 ** -23
T_DLOGITS = dict(rtol=1e-4, atol=1e-7)      # test_nll_fused (tests/test_gpu_kernels.py)
T_MEAN = dict(rtol=1e-5, atol=1e-6)         # its tolerance for the mean loss

ALL_FORMS = set(range(16)) | {-1, -2}


def bound(nslab, z):
    """|logp - ref| and |row_loss - ref| per case: (nslab + 4) 2^-23 max(1, max |z|).

    In units of u = 2^-24 times Z = max(1, max |z|): the slab sum and the bias take nslab roundings
    of partial sums of size <= Z; lse = mx + logf(se) one rounding of a value <= Z + log N plus
    logf's and the sum-exp's error (a few u, not scaled by Z); z - lse one rounding of a value
    <= 2 Z + log N, and the prior one more: about nslab + 4 in all, doubled for margin."""
    return (nslab + 4) * EPS23 * max(1.0, float(np.abs(z).max()))


def case(M, N, S, form, stride="tight", bias=False, prior=False, bf16=False, lstride=1, weight=1.0,
         mode="train", no_loss=False, no_err=False, off=None, kind="rand", scale=3.0, seed=0):
    """stride: 'tight' (M N), 'pad' (M N + 64), 'odd' (M N + 3), 'zero' (0: one slab only).
    mode: 'train' (labels, dlogits), 'valid' (labels, dlogits NULL), 'fwd' (labels NULL, and with
    them dlogits, row_loss, row_err).  off: the one pointer passed one element off 16-byte (bf16:
    8-byte) alignment.  kind: 'rand', 'tie', 'range'."""
    assert stride in ("tight", "pad", "odd", "zero") and mode in ("train", "valid", "fwd")
    assert kind in ("rand", "tie", "range")
    assert off in (None, "zslab", "logp", "dlogits", "bias", "log_prior", "dlogits_bf16")
    return NS(M=M, N=N, S=S, form=form, stride=stride, bias=bias, prior=prior, bf16=bf16,
              lstride=lstride, weight=weight, mode=mode, no_loss=no_loss, no_err=no_err, off=off,
              kind=kind, scale=scale, seed=seed)


def case_id(c):
    s = "%s-M%d-N%d-S%d-%s-form%d" % (c.kind, c.M, c.N, c.S, c.stride, c.form)
    s += "".join("-" + k for k in ("bias", "prior", "bf16", "no_loss", "no_err") if getattr(c, k))
    if c.mode != "train":
        s += "-" + c.mode
    if c.lstride != 1:
        s += "-ls%d" % c.lstride
    if c.weight != 1.0:
        s += "-w%g" % c.weight
    if c.off:
        s += "-off_" + c.off
    return s


def slab_stride(c):
    return {"tight": c.M * c.N, "pad": c.M * c.N + 64, "odd": c.M * c.N + 3, "zero": 0}[c.stride]


# --------------------------------------------------------------------------------- the case table
# narrow heads (N < 512): one wave per row, four rows per workgroup; M = 1, 3, 5, 7, 130 leave the
# last workgroup partly filled (its spare waves read row M - 1)
NARROW = [
    case(1, 1, 1, 0, scale=1.0),
    case(3, 2, 2, 1, stride="odd", bias=True, scale=1.0),
    case(4, 3, 3, 2, stride="pad", prior=True, scale=1.0),
    case(5, 4, 1, 8, scale=1.0),
    case(7, 5, 4, 2, scale=1.0, bf16=True),
    case(130, 48, 2, 9, bias=True, bf16=True, lstride=2),
    case(5, 63, 5, 3, stride="odd", bias=True, prior=True),
    case(4, 64, 3, 10, stride="pad"),
    case(3, 65, 8, 3, weight=0.7),
    case(7, 100, 1, 8, stride="zero"),                       # a layer-normed head: no bias, stride 0
    case(5, 100, 5, 11, stride="pad", prior=True, bf16=True, weight=0.7, lstride=3),
    case(130, 257, 7, 3, stride="pad", bf16=True),
    case(5, 508, 7, 11, bias=True),
    case(1, 511, 1, 0, bias=True),
    case(5, 48, 4, 10, mode="valid", bias=True, bf16=True),  # bf16 passed without dlogits: untouched
    case(3, 100, 2, 9, mode="fwd", prior=True),
    case(7, 63, 1, 0, mode="fwd", bias=True),
    case(5, 65, 2, 1, no_loss=True),
    case(5, 64, 8, 11, no_err=True, bias=True),
    case(4, 257, 4, 2, mode="valid", prior=True, lstride=2),
    case(5, 5, 5, 3, scale=1.0, bias=True, prior=True),
]
# wide heads (512 <= N <= 2048): four waves per row, one row per workgroup
WIDE = [
    case(1, 512, 1, 12),
    case(3, 513, 2, 5, bias=True),
    case(5, 1028, 3, 14, stride="pad", prior=True, bf16=True),
    case(3, 1928, 5, 15, bias=True, weight=0.7, lstride=2),
    case(3, 2044, 2, 13, prior=True),
    case(5, 2047, 7, 7, stride="odd", bias=True, prior=True, bf16=True),
    case(1, 2048, 8, 15, bias=True),
    case(1, 2047, 1, 4),
    case(5, 513, 3, 6, mode="valid"),
    case(3, 1028, 7, 15, mode="fwd", stride="pad", bias=True, prior=True),
    case(5, 2048, 4, 14, bf16=True, no_err=True),
    case(3, 2047, 5, 7, mode="fwd"),
    case(5, 1928, 1, 12, stride="zero", no_loss=True, lstride=3),
]
# the general form: N > 2048 or more than 8 slabs
FALLBACK = [
    case(3, 2049, 1, -2, bias=True, prior=True),
    case(5, 2052, 2, -2, bf16=True, prior=True, weight=0.7),
    case(1, 4100, 3, -2, stride="pad"),
    case(5, 48, 9, -1, bias=True, prior=True, bf16=True),    # narrow, a partly filled workgroup
    case(3, 600, 9, -2, prior=True, stride="pad"),
    case(3, 2052, 1, -2, mode="fwd", prior=True),
    case(7, 100, 9, -1, mode="valid", lstride=2, stride="odd"),
    case(130, 63, 9, -1, bias=True, no_err=True),
]
# ties of the maximum (integer logits: every summation order is exact), in each kind of body
TIES = [
    case(16, 301, 1, 0, kind="tie"),
    case(16, 300, 2, 9, kind="tie", bias=True),
    case(20, 1101, 1, 4, kind="tie"),
    case(20, 1100, 1, 12, kind="tie"),
    case(20, 1100, 3, 6, kind="tie", stride="odd", bias=True),
    case(16, 300, 9, -1, kind="tie"),
    case(20, 2052, 1, -2, kind="tie", bias=True),
]
# one logit near +90 above a tail near -90, two of the rows shifted by 1e4
RANGE = [
    case(6, 100, 1, 8, kind="range", bf16=True),
    case(6, 1029, 2, 5, kind="range"),
    case(6, 2052, 1, -2, kind="range"),
]
CASES = NARROW + WIDE + FALLBACK + TIES + RANGE

# the aligned runs whose scalar twins (one pointer one element off, or an odd slab stride) must take
# the scalar form of the same width and slab capacity: code - 8
ALIGNED = [case(5, 100, 2, 9, bias=True, prior=True, bf16=True, weight=0.7, seed=1),
           case(3, 1028, 3, 14, bias=True, prior=True, bf16=True, seed=1)]
OFFS = ["zslab", "logp", "dlogits", "bias", "log_prior", "dlogits_bf16", "stride"]


def misaligned(base, what):
    c = NS(**vars(base))
    c.form = base.form - 8
    if what == "stride":
        c.stride = "odd"
    else:
        c.off = what
    return c


# pairs of tied columns, by what separates them in the bodies (T = 64 or 256 threads per row; the
# scalar bodies give thread t the columns t + T q, the 16-byte body the chunks 4 (t + T q) .. + 3)
TIE_PAIRS_NARROW = [(5, 69),        # scalar: one thread (q = 0, 1); 16-byte: two lanes
                    (21, 276),      # 16-byte: one thread (chunks 20.., 276..); scalar: two lanes
                    (8, 10),        # 16-byte: inside one float4
                    (3, 40),        # two lanes either way
                    (63, 64),       # scalar: lane 63 (q = 0) below lane 0 (q = 1)
                    (255, 256),     # 16-byte: lane 63's chunk below lane 0's second chunk
                    (2, None)]      # column 2 and the last column (the clamped chunk)
TIE_PAIRS_WIDE = [(5, 261),         # scalar: one thread
                  (21, 1044),       # 16-byte: one thread
                  (8, 10),          # inside one float4
                  (10, 50),         # two lanes of one wave either way
                  (10, 100),        # scalar: waves 0 and 1
                  (40, 400),        # 16-byte: waves 0 and 1; scalar: waves 0 and 2
                  (255, 256),       # scalar: wave 3 holds the lower index, wave 0 the higher
                  (1023, 1024),     # 16-byte: the same
                  (2, None)]


def tie_pairs(c):
    pairs = TIE_PAIRS_NARROW if c.N < 512 else TIE_PAIRS_WIDE
    return [(a, c.N - 1 if b is None else b) for a, b in pairs]


def _split_exact(z, S, g, step):
    """S slabs of multiples of `step` that sum to z exactly in any order (z a multiple of step)."""
    parts = [torch.randint(-8, 9, z.shape, generator=g).float() * step for _ in range(S - 1)]
    return torch.stack([z - sum(parts)] + parts) if parts else z[None].clone()


@functools.lru_cache(maxsize=None)
def _inputs(key):
    c = NS(**dict(key))
    M, N, S = c.M, c.N, c.S
    g = torch.Generator().manual_seed(1000003 * c.seed + 7919 * M + 31 * N + S)
    bias = prior = None
    expect_err = None
    if c.kind == "rand":
        slabs = torch.randn(S, M, N, generator=g) * (c.scale / S ** 0.5)
        if c.bias:
            bias = torch.randn(N, generator=g) * 0.5
    elif c.kind == "tie":
        pairs = tie_pairs(c)
        assert M == 2 * len(pairs) + 2 and all(0 <= a < b < N for a, b in pairs)
        z = torch.randint(-6, 4, (M, N), generator=g).float()
        if c.bias:
            bias = torch.randint(-2, 3, (N,), generator=g).float()
        for i, (a, b) in enumerate(pairs):
            for r in (2 * i, 2 * i + 1):
                z[r, a] = z[r, b] = 8.0
        z[M - 2:] = 2.0                                         # two rows of all-equal logits
        slabs = _split_exact(z - (bias if c.bias else 0.0), S, g, 1.0)
    else:
        z = -90.0 + torch.randint(-16, 17, (M, N), generator=g).float() / 8
        top = [0, N - 1, 37, 50, 3, N - 2]
        for r in range(M):
            z[r, top[r]] = 90.0 + r / 8
        z[3:5] += 1e4
        slabs = _split_exact(z, S, g, 0.125)
    if c.prior:
        counts = torch.rand(N, generator=g) + 0.05
        prior = torch.log(counts / counts.sum())
    z64 = slabs.double().sum(0).numpy() + (bias.double().numpy() if bias is not None else 0.0)
    # labels: column 0, the last column, the last (clamped) 16-byte chunk, then alternately the
    # row's argmax (error 0) and a random column
    y = torch.randint(0, N, (M,), generator=g).numpy()
    am = z64.argmax(1)
    if c.kind == "rand":
        fixed = [0, N - 1, max(N - 3, 0)]
        for r in range(M):
            if M >= 3 and r < 3:
                y[r] = fixed[r]
            elif M < 3 and r == 0:
                y[r] = fixed[(N + c.S) % 3]
            elif r % 2:
                y[r] = am[r]
    elif c.kind == "tie":
        pairs = tie_pairs(c)
        for i, (a, b) in enumerate(pairs):
            y[2 * i], y[2 * i + 1] = a, b                      # the lower, then the higher tied index
        y[M - 2], y[M - 1] = 0, min(3, N - 1)
        expect_err = np.array([0.0, 1.0] * (len(pairs) + 1), dtype=np.float32)
    else:
        top = [0, N - 1, 37, 50, 3, N - 2]
        y[:] = [top[0], top[1], 0, N - 1, top[4], 5]           # rows 2, 3, 5: a label in the tail
    lab = torch.empty(M, c.lstride, dtype=torch.int32)
    for k in range(c.lstride):                                  # the other columns: other labels
        lab[:, k] = torch.from_numpy((y + c.lstride - 1 - k) % N)
    assert bool((lab[:, c.lstride - 1].numpy() == y).all())
    return NS(slabs=slabs, bias=bias, prior=prior, lab=lab, y=y.astype(np.int64),
              expect_err=expect_err)


def _key(c):
    """What the inputs depend on (not the form, the layout in memory or which outputs are asked)."""
    return tuple(sorted((k, getattr(c, k)) for k in ("M", "N", "S", "bias", "prior", "lstride", "kind",
                                                     "scale", "seed")))


def inputs(c):
    """The case's CPU inputs (computed once, shared, never modified): slabs (S, M, N), bias (N) or
    None, prior (N) or None, lab (M, lstride) int32 with the label in the last column, y (M)."""
    return _inputs(_key(c))


def nll_ref(slabs, bias, prior, y, weight):
    """float64, from the fp32 inputs: z = sum of the slabs + bias; logp = z - logsumexp(z) (- prior);
    dlogits = weight / M (softmax - onehot); row_loss = -logp[y] before the prior; row_err = the
    first index of the row's maximum (numpy.argmax) is not y."""
    z = np.asarray(slabs, dtype=np.float64).sum(0)
    if bias is not None:
        z = z + np.asarray(bias, dtype=np.float64)
    M = z.shape[0]
    mx = z.max(1, keepdims=True)
    lse = mx + np.log(np.exp(z - mx).sum(1, keepdims=True))
    lp = z - lse
    onehot = np.zeros_like(z)
    onehot[np.arange(M), y] = 1.0
    return NS(z=z, logp=lp - (np.asarray(prior, dtype=np.float64) if prior is not None else 0.0),
              dlogits=weight / M * (np.exp(lp) - onehot), row_loss=-lp[np.arange(M), y],
              row_err=(np.argmax(z, 1) != y).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _reference(key, weight):
    i = _inputs(key)
    return nll_ref(i.slabs.numpy(), None if i.bias is None else i.bias.numpy(),
                   None if i.prior is None else i.prior.numpy(), i.y, weight)


def reference(c):
    """nll_ref of the case's inputs (computed once, shared, never modified)."""
    return _reference(_key(c), c.weight)


def top2_gap(z):
    s = np.sort(z, 1)
    return s[:, -1] - s[:, -2] if z.shape[1] > 1 else np.full(z.shape[0], np.inf)


# -------------------------------------------------------------------- pkc_nll_fused_multi launches
# (M, N, S, code, options) per head; `code` is the form of the head's own pkc_nll_fused call
def head(M, N, S, code, **kw):
    return case(M, N, S, code, seed=2, **kw)


MULTI = [
    [head(3, 1928, 5, 15, bias=True)],
    [head(5, 63, 1, 0), head(7, 65, 2, 1, bias=True), head(3, 5, 3, 2, scale=1.0),
     head(4, 257, 7, 3, stride="odd", prior=True)],
    [head(3, 513, 1, 4), head(1, 2047, 2, 5, bias=True, bf16=True), head(5, 513, 4, 6),
     head(3, 1029, 5, 7, prior=True)],
    [head(5, 4, 1, 8, scale=1.0), head(5, 48, 2, 9, bias=True), head(5, 100, 3, 10, stride="pad"),
     head(5, 508, 8, 11, bf16=True)],
    [head(3, 512, 1, 12, mode="valid"), head(5, 2044, 2, 13, bias=True),
     head(1, 1028, 4, 14, prior=True, bf16=True)],
    [head(130, 48, 2, 9, lstride=2), head(3, 2048, 7, 15, bias=True)],
    [head(5, 1028, 3, 14, mode="fwd"), head(7, 65, 2, 1, weight=0.7), head(3, 100, 5, 11, bf16=True),
     head(1, 2047, 1, 4, bias=True, prior=True)],
]
# one head outside the register-resident forms: every head falls back to its own launch
MULTI_FALLBACK = [head(5, 48, 2, 9, bias=True), head(3, 2052, 1, -2, prior=True),
                  head(3, 513, 1, 4, bf16=True)]

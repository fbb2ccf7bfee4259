"""numpy restatement of Kaldi's fbank / MFCC computation (feature-window.cc, mel-computations.cc,
feature-fbank.cc, feature-mfcc.cc as published; snip-edges, no dither, no VTLN), the algorithm of
the `pkc-fbank` / `pkc-mfcc` fea_opts stages.  `features(..., dtype=np.float64)` is the reference;
`dtype=np.float32` is the same code with every array and every table in float32, whose distance
from the float64 result is the size of error a float32 implementation may show."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
FLT_MIN = float(np.finfo(np.float32).tiny)

DEFAULTS = dict(sample_frequency=16000.0, frame_length=25.0, frame_shift=10.0,
                preemphasis_coefficient=0.97, remove_dc_offset=True, window_type="povey",
                num_mel_bins=23, low_freq=20.0, high_freq=0.0, energy_floor=0.0, raw_energy=True,
                use_power=True, num_ceps=13, cepstral_lifter=22.0)


def options(kind, **kw):
    o = dict(DEFAULTS, use_energy=(kind == "mfcc"))
    unknown = set(kw) - set(o)
    assert not unknown, unknown
    o.update(kw)
    return o


def geometry(o):
    """(L, S, N): frame length and shift in samples, the padded FFT length."""
    L = int(o["sample_frequency"] * 0.001 * o["frame_length"])
    S = int(o["sample_frequency"] * 0.001 * o["frame_shift"])
    N = 1
    while N < L:
        N *= 2
    return L, S, N


def n_frames(n, L, S):
    return 0 if n < L else 1 + (n - L) // S


def window(kind, L):
    a = 2.0 * np.pi / (L - 1)
    i = np.arange(L, dtype=np.float64)
    if kind == "povey":
        return (0.5 - 0.5 * np.cos(a * i)) ** 0.85
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(a * i)
    if kind == "hanning":
        return 0.5 - 0.5 * np.cos(a * i)
    assert kind == "rectangular", kind
    return np.ones(L)


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_banks(B, N, fs, low, high):
    """(B, N/2) triangular weights in the mel domain; the band edge tests are strict."""
    nyq = 0.5 * fs
    if high <= 0.0:
        high += nyq
    assert 0.0 <= low < nyq and 0.0 < high <= nyq and low < high
    ml, mh = float(mel(low)), float(mel(high))
    delta = (mh - ml) / (B + 1)
    m = mel(fs / N * np.arange(N // 2))
    W = np.zeros((B, N // 2))
    for b in range(B):
        left, center, right = ml + b * delta, ml + (b + 1) * delta, ml + (b + 2) * delta
        up = (m - left) / (center - left)
        down = (right - m) / (right - center)
        W[b] = np.where((m > left) & (m < right), np.where(m <= center, up, down), 0.0)
    return W


def dct_matrix(B, C):
    n = np.arange(B, dtype=np.float64)
    M = np.sqrt(2.0 / B) * np.cos(np.pi / B * (n[None, :] + 0.5) * np.arange(C)[:, None])
    M[0] = np.sqrt(1.0 / B)
    return M


def lifter(C, Q):
    if Q == 0.0:
        return np.ones(C)
    return 1.0 + 0.5 * Q * np.sin(np.pi * np.arange(C) / Q)


def out_dim(kind, o):
    return o["num_ceps"] if kind == "mfcc" else o["num_mel_bins"] + int(o["use_energy"])


def features(sig, kind, dtype=np.float64, **kw):
    """(frames, D) of one int16 signal; kind is 'fbank' or 'mfcc'."""
    o = options(kind, **kw)
    t = np.dtype(dtype).type
    L, S, N = geometry(o)
    F = n_frames(len(sig), L, S)
    B = o["num_mel_bins"]
    win = window(o["window_type"], L).astype(t)
    banks = mel_banks(B, N, o["sample_frequency"], o["low_freq"], o["high_freq"]).astype(t)
    c = t(o["preemphasis_coefficient"])
    eps = t(FLT_EPSILON)
    out = np.zeros((F, out_dim(kind, o)), dtype=t)
    if kind == "mfcc":
        dct = dct_matrix(B, o["num_ceps"]).astype(t)
        lift = lifter(o["num_ceps"], o["cepstral_lifter"]).astype(t)
    for f in range(F):
        x = np.asarray(sig[f * S:f * S + L]).astype(t)
        if o["remove_dc_offset"]:
            x = x - x.sum(dtype=t) / t(L)
        energy = np.log(max(np.dot(x, x), eps))
        y = x.copy()
        y[1:] = x[1:] - c * x[:-1]
        y[0] = x[0] - c * x[0]
        y = y * win
        if not o["raw_energy"]:
            energy = np.log(max(np.dot(y, y), t(FLT_MIN)))
        pad = np.zeros(N, dtype=t)
        pad[:L] = y
        X = np.fft.rfft(pad)
        assert X.real.dtype == t
        p = X.real * X.real + X.imag * X.imag
        if not o["use_power"]:
            p = np.sqrt(p)
        m = np.log(np.maximum(banks @ p[:N // 2], eps))
        if o["energy_floor"] > 0.0:
            energy = max(energy, t(np.log(o["energy_floor"])))
        if kind == "mfcc":
            row = (dct @ m) * lift
            if o["use_energy"]:
                row[0] = energy
        elif o["use_energy"]:
            row = np.concatenate([[energy], m])
        else:
            row = m
        out[f] = row
    assert out.dtype == t
    return out

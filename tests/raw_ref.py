"""numpy restatement of the raw-waveform framing the `pkc-wav-frames` stage computes (the formula
of include/pkc.h pkc_wav_frames, itself restated from the reference's save_raw_fea.py:73-104),
with the refusals of what the script cannot frame.  tests/golden/raw_fea.npz pins it to the
script's own output; it serves the shapes that have no fixture."""
import numpy as np


def geometry(fs, sig_wlen=200, lab_wlen=25, lab_wshift=10):
    """(W, Lw, S) in samples: int(fs*ms/1000) as save_raw_fea.py:49-51."""
    return int((fs * sig_wlen) / 1000), int((fs * lab_wlen) / 1000), int((fs * lab_wshift) / 1000)


def n_frames(n, Lw, S):
    """The count of f >= 0 with f*S + Lw < n."""
    f = 0
    while f * S + Lw < n:
        f += 1
    return f


def frames(s, W, Lw, S, utt="utt"):
    """int16 signal -> float64 (frames, W): out[f][j] = s[b+j]/peak inside the signal, 0 outside,
    b = (2*f*S + Lw - 2)//2 - W//2."""
    s = np.asarray(s)
    assert s.dtype == np.int16 and s.ndim == 1
    n = len(s)
    if W % 2:
        raise ValueError("%s: odd window %d" % (utt, W))
    F = n_frames(n, Lw, S)
    if F == 0:
        raise ValueError("%s: no frame in %d samples" % (utt, n))
    peak = int(np.abs(s.astype(np.int64)).max())
    if peak == 0:
        raise ValueError("%s: all-zero signal" % utt)
    sig = s.astype(np.float64) / np.float64(peak)
    out = np.zeros((F, W), np.float64)
    for f in range(F):
        b = (2 * f * S + Lw - 2) // 2 - W // 2
        if b < 0 and b + W > n:
            raise ValueError("%s: frame %d overflows the %d samples on both sides" % (utt, f, n))
        lo, hi = max(b, 0), min(b + W, n)
        out[f, lo - b:hi - b] = sig[lo:hi]
    return out

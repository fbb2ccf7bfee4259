"""Writes tests/golden/kaldi_feats.npz: short int16 signals and their Kaldi-compatible log-mel
filter-bank matrices as computed by transformers.audio_utils (a third-party implementation with a
povey window, mel_scale="kaldi", triangularize_in_mel_space and remove_dc_offset), the arithmetic
the `pkc-fbank` stage is pinned to.  Needs the `transformers` package; run by hand:

    python tests/golden/make_golden_kaldi_feats.py

Per case <name>: <name>/signal (int16), <name>/fbank (float32, frames x bins) and the settings
<name>/fs, /bins, /low, /high (as given to --high-freq), /window, /preemph, /frame_length,
/frame_shift (ms)."""
import os

import numpy as np
from transformers.audio_utils import mel_filter_bank, spectrogram, window_function

HERE = os.path.dirname(os.path.abspath(__file__))
MEL_FLOOR = 1.192092955078125e-07          # FLT_EPSILON


def fbank(sig, fs, bins, low, high, window, preemph, frame_length=25.0, frame_shift=10.0):
    L = int(fs * 0.001 * frame_length)
    S = int(fs * 0.001 * frame_shift)
    N = 1
    while N < L:
        N *= 2
    win = window_function(L, window, periodic=False)
    filters = mel_filter_bank(num_frequency_bins=N // 2 + 1, num_mel_filters=bins,
                              min_frequency=low, max_frequency=high if high > 0 else fs / 2 + high,
                              sampling_rate=fs, norm=None, mel_scale="kaldi",
                              triangularize_in_mel_space=True)
    out = spectrogram(sig.astype(np.float64), win, frame_length=L, hop_length=S, fft_length=N,
                      power=2.0, center=False, preemphasis=preemph, mel_filters=filters,
                      mel_floor=MEL_FLOOR, log_mel="log", remove_dc_offset=True)
    return np.ascontiguousarray(out.T, dtype=np.float32)


def signals():
    rs = np.random.RandomState(20241)
    t = np.arange(6000)
    tone = 8000.0 * np.sin(2 * np.pi * 440.0 * t / 16000.0)
    return {
        "noise3000": np.clip(rs.normal(0, 3000, 6000), -32768, 32767),
        "tone_noise50": tone[:5000] + rs.normal(0, 50, 5000),
        "noise3": rs.normal(0, 3, 4000),
        "dc4000": 4000.0 + rs.normal(0, 300, 4500),
    }


CASES = [
    # name, signal, fs, bins, low, high, window, preemph
    ("fs16k_b40_noise3000", "noise3000", 16000, 40, 20.0, 0.0, "povey", 0.97),
    ("fs16k_b40_tone", "tone_noise50", 16000, 40, 20.0, 0.0, "povey", 0.97),
    ("fs16k_b40_noise3", "noise3", 16000, 40, 20.0, 0.0, "povey", 0.97),
    ("fs16k_b40_dc4000", "dc4000", 16000, 40, 20.0, 0.0, "povey", 0.97),
    ("fs8k_b23_noise3000", "noise3000", 8000, 23, 20.0, 0.0, "povey", 0.97),
    ("fs8k_b23_dc4000_hamming", "dc4000", 8000, 23, 20.0, 0.0, "hamming", 0.97),
    ("fs16k_b40_high-400_tone", "tone_noise50", 16000, 40, 20.0, -400.0, "povey", 0.97),
    ("fs16k_b23_low0_high-400_hamming", "noise3000", 16000, 23, 0.0, -400.0, "hamming", 0.95),
]


def main():
    sig = {k: np.round(v).astype(np.int16) for k, v in signals().items()}
    out = {}
    for name, s, fs, bins, low, high, window, preemph in CASES:
        out[name + "/signal"] = sig[s]
        out[name + "/fbank"] = fbank(sig[s], fs, bins, low, high, window, preemph)
        for k, v in (("fs", fs), ("bins", bins), ("low", low), ("high", high), ("window", window),
                     ("preemph", preemph), ("frame_length", 25.0), ("frame_shift", 10.0)):
            out[name + "/" + k] = np.array(v)
    path = os.path.join(HERE, "kaldi_feats.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

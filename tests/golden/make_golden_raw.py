"""Regenerate tests/golden/raw_fea.npz by running the reference's save_raw_fea.py.

Usage: python tests/golden/make_golden_raw.py <path of the reference checkout>   (needs scipy)

Data only: per case the int16 signal, its sampling rate and the float64 matrix the script hands to
write_mat.  The script is executed at run time, never copied: its text is read from the checkout,
its path and rate assignments are replaced by substitution (one run per case, over a wav written
to a temporary folder), and a stub `data_io` module stands in for the reference's — its write_mat
captures (key, matrix) under whatever signature the script calls it with (this fork's
data_io.write_mat takes (output_folder, file_or_fd, m, key), so the script's own call cannot run
against it) and its read_vec_int_ark yields nothing (the labels are read and never used).
"""
import os
import re
import sys
import tempfile
import types
import wave

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def _sig(seed, n, lo=-32768, hi=32768):
    return np.random.RandomState(seed).randint(lo, hi, size=n).astype(np.int16)


def cases():
    """name -> (fs, int16 signal).  At fs 1600 the script's windows are W 320, Lw 40, S 16; at
    fs 1000 W 200, Lw 25 (odd), S 10; at fs 16000 the recipe's own W 3200, Lw 400, S 160."""
    neg = _sig(14, 777, -32000, 32000)
    neg[413] = -32768                     # the peak is the one sample -32768
    return {
        "fs1600_n307": (1600, _sig(11, 307)),       # smallest framable length
        "fs1600_n360": (1600, _sig(12, 360)),       # Lw + 20*S: the strict <
        "fs1600_n777": (1600, _sig(13, 777)),
        "fs1600_n777_negpeak": (1600, neg),
        "fs1600_n777_quiet": (1600, _sig(15, 777, -1000, 1001)),
        "fs1000_n900": (1000, _sig(16, 900)),
        "fs16000_n3079": (16000, _sig(17, 3079)),
    }


def run_script(ref, fs, signals):
    """{utt: int16 signal} at rate fs -> {utt: float64 matrix} from one run of the script."""
    captured = {}
    stub = types.ModuleType("data_io")

    def write_mat(*args, **kw):
        mats = [a for a in args if isinstance(a, np.ndarray)]
        captured[kw["key"]] = np.array(mats[0])
    stub.write_mat = write_mat
    stub.read_vec_int_ark = lambda *a, **k: iter(())
    with open(os.path.join(ref, "save_raw_fea.py")) as f:
        text = f.read()
    with tempfile.TemporaryDirectory() as d:
        lst = os.path.join(d, "wav_lst.scp")
        with open(lst, "w") as f:
            for utt, s in signals.items():
                path = os.path.join(d, utt + ".wav")
                with wave.open(path, "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(fs)
                    w.writeframes(s.astype("<i2").tobytes())
                f.write("%s %s\n" % (utt, path))
        subst = {"lab_folder": repr(d), "out_folder": repr(os.path.join(d, "out")),
                 "wav_lst": repr(lst), "scp_file_out": repr(os.path.join(d, "feats_raw.scp")),
                 "sig_fs": str(fs), "lab_fs": str(fs)}
        for name, value in subst.items():
            text, n = re.subn(r"^%s=.*$" % name, "%s=%s" % (name, value), text, count=1, flags=re.M)
            assert n == 1, name
        saved = sys.modules.get("data_io")
        sys.modules["data_io"] = stub
        try:
            exec(compile(text, "save_raw_fea.py", "exec"), {"__name__": "__main__"})
        finally:
            if saved is None:
                del sys.modules["data_io"]
            else:
                sys.modules["data_io"] = saved
    return captured


def main(ref):
    out = {}
    cs = cases()
    for fs in sorted({fs for fs, _ in cs.values()}):
        sigs = {k: s for k, (f, s) in cs.items() if f == fs}
        mats = run_script(ref, fs, sigs)
        for k, s in sigs.items():
            assert mats[k].dtype == np.float64 and mats[k].ndim == 2
            out[k + "/fs"] = np.int64(fs)
            out[k + "/signal"] = s
            out[k + "/frames"] = mats[k]
            print(k, mats[k].shape)
    path = os.path.join(OUT, "raw_fea.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])

"""The `pkc-wav-frames` fea_opts stage without a GPU: the numpy restatement of the framing
(tests/raw_ref.py) equals what the reference's save_raw_fea.py wrote for every fixture
(tests/golden/raw_fea.npz, float64, bit for bit), the fea_opts parser accepts the stage alone and
refuses everything else, and the wav reader refuses what the reference cannot frame."""
import os
import wave

import numpy as np
import pytest

import raw_ref

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "raw_fea.npz"))
CASES = sorted({k.split("/")[0] for k in G.files})
ROWS = {"fs1600_n307": (17, 320), "fs1600_n360": (20, 320), "fs1600_n777": (47, 320),
        "fs1600_n777_negpeak": (47, 320), "fs1600_n777_quiet": (47, 320),
        "fs1000_n900": (88, 200), "fs16000_n3079": (17, 3200)}
STAGE = "pkc-wav-frames --sig-wlen=200 --lab-wlen=25 --lab-wshift=10 --fs=%d ark:- ark:- |"


def test_fixture_has_every_case():
    assert CASES == sorted(ROWS)
    sig = G["fs1600_n777_negpeak/signal"]
    assert sig.min() == -32768 and (sig == -32768).sum() == 1 and sig.max() < 32768 - 700
    assert np.abs(G["fs1600_n777_quiet/signal"]).max() <= 1000


@pytest.mark.parametrize("name", CASES)
def test_raw_ref_equals_the_reference_script(name):
    W, Lw, S = raw_ref.geometry(int(G[name + "/fs"]))
    want = G[name + "/frames"]
    got = raw_ref.frames(G[name + "/signal"], W, Lw, S)
    assert want.dtype == np.float64 and got.dtype == np.float64
    assert want.shape == ROWS[name]
    assert np.array_equal(got, want)


def test_parser_accepts_the_stage_and_applies_the_defaults():
    from pkc import frontend as F
    assert F.is_native_pipe("pkc-wav-frames ark:- ark:- |")
    assert F.is_native_pipe(STAGE % 16000)
    fe = F.FeaFrontend.parse("pkc-wav-frames ark:- ark:- |")
    assert (fe.wav.sig_wlen, fe.wav.lab_wlen, fe.wav.lab_wshift, fe.wav.fs) == (200, 25, 10, 16000)
    assert (fe.wav.W, fe.wav.Lw, fe.wav.S) == (3200, 400, 160)
    assert fe.cmvn is None and fe.order == 0
    fe = F.FeaFrontend.parse(STAGE % 1600)
    assert (fe.wav.W, fe.wav.Lw, fe.wav.S) == (320, 40, 16) == raw_ref.geometry(1600)
    fe = F.FeaFrontend.parse("pkc-wav-frames --sig_wlen=100 --fs=1000 ark:- ark:-")
    assert (fe.wav.W, fe.wav.Lw, fe.wav.S) == (100, 25, 10)
    # the other pipes parse as before
    assert F.FeaFrontend.parse("add-deltas --delta-order=2 ark:- ark:- |").wav is None
    assert not F.is_native_pipe("splice-feats ark:- ark:- |")


@pytest.mark.parametrize("opts, word", [
    ("pkc-wav-frames --window=hamming ark:- ark:- |", "window"),
    ("pkc-wav-frames --fs=16000 ark:- ark:- | add-deltas --delta-order=2 ark:- ark:- |", "only stage"),
    ("apply-cmvn --norm-vars=false ark:/nonexistent ark:- ark:- | pkc-wav-frames ark:- ark:- |",
     "only stage"),
    ("add-deltas ark:- ark:- | pkc-wav-frames ark:- ark:- |", "only stage"),
    ("pkc-wav-frames ark:- ark:- | pkc-wav-frames ark:- ark:- |", "only stage"),
    ("pkc-wav-frames scp:x ark:- |", "ark:- ark:-"),
])
def test_parser_refuses(opts, word):
    from pkc import frontend as F
    with pytest.raises(NotImplementedError, match=word):
        F.FeaFrontend.parse(opts)


def _wav(path, s, fs=1600, channels=1, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(fs)
        w.writeframes(np.asarray(s).tobytes())
    return str(path)


def _noise(n, seed=0):
    return np.random.RandomState(seed).randint(-32768, 32768, size=n).astype(np.int16)


def test_wav_reader_reads_pcm16(tmp_path):
    from pkc.frontend import WavFrames
    s = _noise(777)
    got, peak = WavFrames(fs=1600).read("u1", _wav(tmp_path / "a.wav", s))
    assert got.dtype == np.int16 and np.array_equal(got, s)
    assert peak == int(np.abs(s.astype(np.int64)).max())
    neg = np.zeros(500, np.int16)
    neg[7] = -32768
    assert WavFrames(fs=1600).read("u2", _wav(tmp_path / "b.wav", neg))[1] == 32768


def test_wav_reader_refusals(tmp_path):
    from pkc.frontend import WavFrames
    wf = WavFrames(fs=1600)
    s = _noise(777)
    bad = [
        ("stereo", wf, _wav(tmp_path / "st.wav", np.stack([s, s], 1), channels=2)),
        ("eightbit", wf, _wav(tmp_path / "u8.wav", (s >> 8).astype(np.uint8), width=1)),
        ("rate", wf, _wav(tmp_path / "r.wav", s, fs=16000)),
        ("silent", wf, _wav(tmp_path / "z.wav", np.zeros(777, np.int16))),
        ("oddw", WavFrames(sig_wlen=201, fs=1000), _wav(tmp_path / "o.wav", s, fs=1000)),
        ("short", wf, _wav(tmp_path / "s.wav", _noise(40))),        # n == Lw
        ("shorter", wf, _wav(tmp_path / "s2.wav", _noise(17))),
        ("n306", wf, _wav(tmp_path / "n306.wav", _noise(306))),
    ]
    for utt, w, path in bad:
        with pytest.raises(ValueError, match=utt):
            w.read(utt, path)
    assert WavFrames(sig_wlen=201, fs=1000).W == 201
    got, _ = wf.read("n307", _wav(tmp_path / "n307.wav", _noise(307)))
    assert len(got) == 307 and wf.n_frames(307) == 17


def test_unframable_lengths_match_the_restatement():
    """Every length around the two-sided overflow at one-tenth scale and at the real geometry:
    WavFrames.check refuses exactly what raw_ref refuses (n <= Lw, then Lw < n < 307 / 3079)."""
    from pkc.frontend import WavFrames
    for fs, first_ok in ((1600, 307), (16000, 3079)):
        wf = WavFrames(fs=fs)
        W, Lw, S = raw_ref.geometry(fs)
        for n in list(range(Lw - 1, Lw + 3)) + list(range(first_ok - 3, first_ok + 3)):
            try:
                want = len(raw_ref.frames(np.ones(n, np.int16), W, Lw, S))
            except ValueError:
                want = None
            assert (want is not None) == (n >= first_ok)
            if want is None:
                with pytest.raises(ValueError, match="uttX"):
                    wf.check("uttX", n)
            else:
                assert wf.check("uttX", n) == want


def test_frame_count_is_strict():
    from pkc.frontend import WavFrames
    for fs in (1600, 1000, 16000):
        wf = WavFrames(fs=fs)
        for k in (1, 2, 20, 331):
            n = wf.Lw + k * wf.S
            assert wf.n_frames(n) == k == raw_ref.n_frames(n, wf.Lw, wf.S)
            assert wf.n_frames(n + 1) == k + 1
            assert wf.n_frames(n - 1) == k
        assert wf.n_frames(wf.Lw) == 0 and wf.n_frames(wf.Lw + 1) == 1


def test_entry_point_is_declared_and_bound():
    import re
    from pkc import _lib as L
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "pkc.h")).read()
    assert re.search(r"^int pkc_wav_frames\(", hdr, re.M)
    assert len(L._SIGS["pkc_wav_frames"][1]) == 13
    assert int(re.search(r"#define PKC_ABI_VERSION (\d+)", hdr).group(1)) == 9 == L.ABI_VERSION

"""The `pkc-fbank` / `pkc-mfcc` fea_opts stages without a GPU: the float64 restatement of Kaldi's
algorithm (tests/kaldi_feats_ref.py) against the log-mel matrices transformers.audio_utils computed
for the fixtures (tests/golden/kaldi_feats.npz), the host tables of the kernel against the
restatement's, the option parser with its defaults, conf file, refusals and stage-order rules, the
snip-edges frame count, and the cmvn statistics writer."""
import os
import wave

import numpy as np
import pytest

import kaldi_feats_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "kaldi_feats.npz"))
CASES = sorted({k.split("/")[0] for k in G.files})


def case_opts(name):
    return dict(sample_frequency=float(G[name + "/fs"]), num_mel_bins=int(G[name + "/bins"]),
                low_freq=float(G[name + "/low"]), high_freq=float(G[name + "/high"]),
                window_type=str(G[name + "/window"]),
                preemphasis_coefficient=float(G[name + "/preemph"]))


def test_fixture_has_every_case():
    assert len(CASES) == 8
    assert {(int(G[k + "/fs"]), int(G[k + "/bins"])) for k in CASES} >= {(16000, 40), (8000, 23)}
    assert any(float(G[k + "/high"]) < 0 for k in CASES)
    for k in CASES:
        assert G[k + "/signal"].dtype == np.int16 and 4000 <= len(G[k + "/signal"]) <= 6000
        assert G[k + "/fbank"].dtype == np.float32


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_third_party_fbank(name):
    """The library returns float32: half an ulp below 32 is 9.5e-7, and 1.01e-6 was the largest
    distance measured.  1e-5 is a condition, not a tolerance: a miss is another algorithm."""
    want = G[name + "/fbank"]
    got = R.features(G[name + "/signal"], "fbank", np.float64, **case_opts(name))
    assert got.shape == want.shape and got.dtype == np.float64
    d = np.abs(got - want).max()
    print("%s: max |ref64 - golden| = %.3g" % (name, d))
    assert d <= 1e-5


def test_float32_restatement_is_float32_and_close():
    name = "fs16k_b40_noise3000"
    r32 = R.features(G[name + "/signal"], "mfcc", np.float32, **case_opts(name))
    r64 = R.features(G[name + "/signal"], "mfcc", np.float64, **case_opts(name))
    assert r32.dtype == np.float32 and r32.shape == r64.shape == (36, 13)
    assert 0 < np.abs(r32 - r64).max() < 1e-3


def test_defaults_are_kaldis():
    from pkc import frontend as F
    fb = F.FeaFrontend.parse("pkc-fbank ark:- ark:- |")
    assert fb.wav is None and fb.cmvn is None and fb.order == 0
    o = fb.feats.opts
    assert fb.feats.kind == "fbank" and fb.feats.stage == "pkc-fbank"
    assert (o["sample-frequency"], o["frame-length"], o["frame-shift"]) == (16000.0, 25.0, 10.0)
    assert (o["preemphasis-coefficient"], o["remove-dc-offset"], o["window-type"]) == (0.97, True,
                                                                                       "povey")
    assert (o["num-mel-bins"], o["low-freq"], o["high-freq"]) == (23, 20.0, 0.0)
    assert (o["use-energy"], o["energy-floor"], o["raw-energy"], o["use-power"]) == (False, 0.0,
                                                                                     True, True)
    assert (fb.feats.L, fb.feats.S, fb.feats.N, fb.feats.B, fb.feats.D) == (400, 160, 512, 23, 23)
    assert fb.feats.high == 8000.0
    mf = F.FeaFrontend.parse("pkc-mfcc ark:- ark:- |").feats
    assert mf.kind == "mfcc" and mf.opts["use-energy"] is True
    assert (mf.opts["num-ceps"], mf.opts["cepstral-lifter"], mf.B, mf.C, mf.D) == (13, 22.0, 23, 13, 13)
    assert dict(mf.opts, **{"use-energy": False}) == dict(o, **{"num-ceps": 13, "cepstral-lifter": 22.0})
    e = F.FeaFrontend.parse("pkc-fbank --use-energy=true --num_mel_bins=40 --high-freq=-400 "
                            "--sample-frequency=8000 ark:- ark:- |").feats
    assert (e.B, e.D, e.L, e.S, e.N, e.high) == (40, 41, 200, 80, 256, 3600.0)
    assert F.FeaFrontend.parse("pkc-mfcc --num-ceps=23 --cepstral-lifter=0 ark:- ark:-").feats.D == 23
    # what may be said without changing anything
    F.FeaFrontend.parse("pkc-fbank --dither=0 --snip-edges=true --htk-compat=false "
                        "--use-log-fbank=true --round-to-power-of-two=true ark:- ark:- |")


def test_stage_order_and_native_pipe(tmp_path):
    from pkc import frontend as F
    from pkc.kaldi_feats import write_stats_ark
    cm = str(tmp_path / "cmvn.ark")
    write_stats_ark(cm, {"u": np.ones((2, 24))})
    pipe = ("pkc-fbank ark:- ark:- | apply-cmvn ark:%s ark:- ark:- | "
            "add-deltas --delta-order=2 ark:- ark:- |" % cm)
    assert F.is_native_pipe(pipe) and F.is_native_pipe("pkc-mfcc ark:- ark:- |")
    assert not F.is_native_pipe("pkc-plp ark:- ark:- |")
    fe = F.FeaFrontend.parse(pipe)
    assert fe.feats.kind == "fbank" and fe.order == 2 and sorted(fe.cmvn["stats"]) == ["u"]
    assert fe.out_dim(fe.feats.D) == 69
    for bad in ("add-deltas ark:- ark:- | pkc-fbank ark:- ark:- |",
                "apply-cmvn ark:%s ark:- ark:- | pkc-mfcc ark:- ark:- |" % cm,
                "pkc-fbank ark:- ark:- | pkc-mfcc ark:- ark:- |",
                "pkc-fbank ark:- ark:- | pkc-wav-frames ark:- ark:- |",
                "pkc-wav-frames ark:- ark:- | pkc-fbank ark:- ark:- |",
                "pkc-fbank scp:x ark:- |"):
        with pytest.raises(NotImplementedError):
            F.FeaFrontend.parse(bad)
    # pkc-wav-frames keeps its rule and its message
    with pytest.raises(NotImplementedError, match="only stage"):
        F.FeaFrontend.parse("pkc-wav-frames ark:- ark:- | add-deltas ark:- ark:- |")


@pytest.mark.parametrize("stage, opt", [
    ("pkc-fbank", "--dither=1.0"), ("pkc-mfcc", "--dither=0.5"),
    ("pkc-fbank", "--snip-edges=false"), ("pkc-mfcc", "--snip-edges=false"),
    ("pkc-fbank", "--htk-compat=true"), ("pkc-mfcc", "--htk-compat=true"),
    ("pkc-fbank", "--use-log-fbank=false"),
    ("pkc-fbank", "--round-to-power-of-two=false"),
    ("pkc-fbank", "--vtln-low=100"), ("pkc-mfcc", "--vtln-high=-500"),
    ("pkc-fbank", "--vtln-map=ark:x"), ("pkc-fbank", "--vtln-warp=1.1"),
    ("pkc-fbank", "--window-type=blackman"), ("pkc-mfcc", "--window-type=blackman"),
    ("pkc-fbank", "--subtract-mean=true"), ("pkc-fbank", "--channel=0"),
    ("pkc-fbank", "--blackman-coeff=0.42"), ("pkc-fbank", "--min-duration=1"),
    ("pkc-fbank", "--num-ceps=13"), ("pkc-fbank", "--cepstral-lifter=22"),
    ("pkc-mfcc", "--allow-downsample=true"), ("pkc-mfcc", "--utt2spk=ark:x"),
])
def test_refusals_name_the_option(stage, opt):
    from pkc import frontend as F
    with pytest.raises(NotImplementedError, match=opt.split("=")[0]):
        F.FeaFrontend.parse("%s %s ark:- ark:- |" % (stage, opt))


def test_bad_values_are_errors():
    from pkc import frontend as F
    for bad in ("pkc-mfcc --num-ceps=24 ark:- ark:- |", "pkc-fbank --low-freq=9000 ark:- ark:- |",
                "pkc-fbank --high-freq=-8000 ark:- ark:- |", "pkc-fbank --use-energy=maybe ark:- ark:-",
                "pkc-fbank --num-mel-bins=400 ark:- ark:- |"):
        with pytest.raises(ValueError):
            F.FeaFrontend.parse(bad).feats.tables()


def test_conf_file_and_command_line_override(tmp_path):
    from pkc import frontend as F
    conf = str(tmp_path / "fbank.conf")
    with open(conf, "w") as f:
        f.write("# a Kaldi conf file\n--num-mel-bins=40   # TIMIT recipe\n\n--use_energy=true\n"
                "--sample-frequency=8000\n--window-type=hamming\n")
    kf = F.FeaFrontend.parse("pkc-fbank --config=%s ark:- ark:- |" % conf).feats
    assert (kf.B, kf.D, kf.L, kf.opts["window-type"], kf.opts["use-energy"]) == (40, 41, 200,
                                                                                  "hamming", True)
    kf = F.FeaFrontend.parse("pkc-fbank --num-mel-bins=30 --config=%s --use-energy=false ark:- ark:- |"
                             % conf).feats
    assert (kf.B, kf.D, kf.L) == (30, 30, 200)
    with open(conf, "a") as f:
        f.write("--dither=1.0\n")
    with pytest.raises(NotImplementedError, match="dither"):
        F.FeaFrontend.parse("pkc-fbank --config=%s ark:- ark:- |" % conf)
    F.FeaFrontend.parse("pkc-fbank --config=%s --dither=0 ark:- ark:- |" % conf)
    with open(conf, "a") as f:
        f.write("num-mel-bins=3\n")
    with pytest.raises(ValueError, match="fbank.conf:8"):
        F.FeaFrontend.parse("pkc-fbank --config=%s --dither=0 ark:- ark:- |" % conf)


def test_frame_counts():
    from pkc import frontend as F
    for kf in (F.KaldiFeats("fbank"), F.KaldiFeats("mfcc", sample_frequency=8000.0),
               F.KaldiFeats("fbank", frame_length=32.0, frame_shift=7.0)):
        L, S = kf.L, kf.S
        assert [kf.n_frames(n) for n in (L - 1, L, L + S - 1, L + S)] == [0, 1, 1, 2]
        assert [R.n_frames(n, L, S) for n in (0, L - 1, L, L + S - 1, L + S, L + 10 * S)] == \
            [kf.n_frames(n) for n in (0, L - 1, L, L + S - 1, L + S, L + 10 * S)]
    assert (F.KaldiFeats("fbank", frame_length=32.0).L, F.KaldiFeats("fbank", frame_length=32.0).N) \
        == (512, 512)


@pytest.mark.parametrize("kind, kw", [
    ("fbank", dict(num_mel_bins=40)),
    ("mfcc", dict(sample_frequency=8000.0, window_type="hamming", low_freq=0.0, high_freq=-400.0)),
    ("mfcc", dict(num_mel_bins=80, num_ceps=80, cepstral_lifter=0.0, window_type="hanning")),
    ("fbank", dict(frame_length=20.0, window_type="rectangular")),
])
def test_host_tables_equal_the_restatement(kind, kw):
    """Evaluated in float64, stored as float32: the float32 cast of the restatement's tables."""
    from pkc import frontend as F
    kf = F.KaldiFeats(kind, **kw)
    o = R.options(kind, **kw)
    L, S, N = R.geometry(o)
    assert (kf.L, kf.S, kf.N, kf.D) == (L, S, N, R.out_dim(kind, o))
    t = kf.tables()
    assert all(v.dtype == (np.float64 if k == "twiddle" else np.int32 if k in
               ("mel_first", "mel_count", "mel_offset") else np.float32) for k, v in t.items())
    assert np.array_equal(t["window"], R.window(o["window_type"], L).astype(np.float32))
    W = R.mel_banks(kf.B, N, o["sample_frequency"], o["low_freq"], o["high_freq"]).astype(np.float32)
    dense = np.zeros_like(W)
    for b in range(kf.B):
        f, c, off = t["mel_first"][b], t["mel_count"][b], t["mel_offset"][b]
        assert c > 0 and f + c <= N // 2
        dense[b, f:f + c] = t["mel_weight"][off:off + c]
    assert np.array_equal(dense, W)
    k = np.arange(N // 2)
    assert np.allclose(t["twiddle"][:, 0] + 1j * t["twiddle"][:, 1], np.exp(-2j * np.pi * k / N),
                       rtol=0, atol=1e-15)
    if kind == "mfcc":
        assert np.array_equal(t["dct"], R.dct_matrix(kf.B, kf.C).astype(np.float32))
        assert np.array_equal(t["lifter"], R.lifter(kf.C, o["cepstral_lifter"]).astype(np.float32))


def test_library_enforces_the_shape_limits():
    """pkc_kaldi_feats_ok: N a power of two up to 4096, D and the mel bins up to 256, the widths
    consistent with the kind; every refusal leaves a message."""
    import ctypes as C
    from pkc import _lib as L
    lib = L.lib()
    ok = dict(L=400, S=160, N=512, num_bins=40, num_ceps=0, D=40, mfcc=0, use_energy=0)

    def verdict(**kw):
        a = L.KaldiFeatsArgs(**dict(ok, **kw))
        return lib.pkc_kaldi_feats_ok(C.byref(a)), lib.pkc_last_error().decode()
    assert verdict()[0] == 1
    assert verdict(L=4096, N=4096)[0] == 1 and verdict(num_bins=256, D=256)[0] == 1
    assert verdict(mfcc=1, num_ceps=13, D=13)[0] == 1 and verdict(use_energy=1, D=41)[0] == 1
    for kw, word in ((dict(N=8192, L=8000), "power of two"), (dict(N=500), "power of two"),
                     (dict(L=513), "frame length"), (dict(L=1), "frame length"),
                     (dict(S=0), "frame shift"), (dict(num_bins=257, D=257), "mel bins"),
                     (dict(num_bins=256, D=257, use_energy=1), "output columns"),
                     (dict(D=41), "fbank"), (dict(mfcc=1, num_ceps=41, D=41), "cepstra"),
                     (dict(mfcc=1, num_ceps=13, D=14), "cepstra"), (dict(rows=-1), "rows")):
        got, msg = verdict(**kw)
        assert got == 0 and word in msg, (kw, msg)
    assert lib.pkc_kaldi_feats_ok(None) == 0
    # rows == 0 launches nothing and needs no pointer
    assert lib.pkc_kaldi_feats(C.byref(L.KaldiFeatsArgs(**ok)), None) == L.PKC_OK
    assert lib.pkc_kaldi_feats(C.byref(L.KaldiFeatsArgs(**dict(ok, N=8192))), None) == L.PKC_ERR_ARG


def test_wav_reader_names_the_utterance(tmp_path):
    from pkc import frontend as F
    kf = F.KaldiFeats("fbank")

    def wav(name, ch, width, rate):
        p = str(tmp_path / name)
        with wave.open(p, "wb") as w:
            w.setnchannels(ch)
            w.setsampwidth(width)
            w.setframerate(rate)
            w.writeframes(b"\1\0" * 64 * ch * (width // 2 or 1))
        return p
    s = kf.read("ok", wav("ok.wav", 1, 2, 16000))
    assert s.dtype == np.int16 and len(s) == 64 and (s == 1).all()     # the int16 scale, unscaled
    for name, ch, width, rate in (("st", 2, 2, 16000), ("b8", 1, 1, 16000), ("r8k", 1, 2, 8000)):
        with pytest.raises(ValueError, match="utterance utt_" + name):
            kf.read("utt_" + name, wav(name + ".wav", ch, width, rate))


def test_cmvn_stats_writer_round_trips(tmp_path):
    from pkc import frontend as F
    from pkc.kaldi_feats import write_stats_ark
    rs = np.random.RandomState(3)
    feats = {"spkA": [rs.randn(17, 23).astype(np.float32) * 5 - 12, rs.randn(1, 23).astype(np.float32)],
             "spkB": [rs.randn(40, 23).astype(np.float32)]}
    stats = {k: F.cmvn_stats(v) for k, v in feats.items()}
    path = str(tmp_path / "cmvn.ark")
    write_stats_ark(path, stats)
    with open(path, "rb") as f:
        back = F.parse_stats_ark(f.read())
    assert sorted(back) == ["spkA", "spkB"]
    for k, ms in feats.items():
        m = np.concatenate(ms).astype(np.float64)
        assert back[k].shape == (2, 24) and back[k].dtype == np.float64
        assert np.array_equal(back[k], stats[k])
        assert back[k][0, 23] == len(m) and back[k][1, 23] == 0.0
        assert np.array_equal(back[k][0, :23], m.sum(0))
        assert np.array_equal(back[k][1, :23], (m * m).sum(0))
    off, scale = F.cmvn_norm(back["spkB"], True)
    assert np.allclose(np.concatenate(feats["spkB"]) .astype(np.float64).mean(0), -off / scale, atol=1e-6)

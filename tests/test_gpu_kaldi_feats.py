"""Kaldi fbank / MFCC features on the GPU (pkc_kaldi_feats, the `pkc-fbank` / `pkc-mfcc` fea_opts
stages) against the float64 restatement of Kaldi's algorithm (tests/kaldi_feats_ref.py, itself
pinned to transformers.audio_utils by tests/test_kaldi_feats_cpu.py): at kernel level, on silence,
row by row independent, through the chunk staging against the writer's arks, and end to end
through run_nn.

Kernel rule (that of test_gpu_sinc.py): per case max|gpu - ref64| <= 4 * d_ref, where
d_ref = max|ref32 - ref64| is what the same algorithm loses in numpy float32 on that case; the
kernel's FFT and sums run in another float32 order, so its error is of like size, not equal.  As a
condition, max|gpu - ref64| <= 1e-3 on every non-silent case."""
import configparser
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import kaldi_feats_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "pytorch-kaldi-cgs_amd")
LOG_EPS = float(np.log(np.float32(R.FLT_EPSILON)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _signals(fs, L, S):
    """Noise-bearing int16 signals of 13 frames each, and noise of exactly 1 and 2 frames."""
    rs = np.random.RandomState(int(fs) + L)
    n = L + 12 * S
    t = np.arange(n)
    sq = np.where((t // 23) % 2 == 0, 32767, -32767)
    sig = {"noise300": rs.normal(0, 300, n),
           "tone_noise50": 8000 * np.sin(2 * np.pi * 440.0 * t / fs) + rs.normal(0, 50, n),
           "dc4000": 4000 + rs.normal(0, 300, n),
           "square": sq,
           "one_frame": rs.normal(0, 1000, L),
           "two_frames": rs.normal(0, 1000, L + S)}
    return {k: np.clip(np.round(v), -32768, 32767).astype(np.int16) for k, v in sig.items()}


def _gpu(sig, kind, **kw):
    """{utt: (frames, D) float32} of one pkc_kaldi_feats call over every frame of `sig`."""
    from pkc import data_io as D
    from pkc import frontend as F
    kf = F.KaldiFeats(kind, **kw)
    out = D.kaldi_features(sig, kf).cpu().numpy()
    res, r = {}, 0
    for k, s in sig.items():
        n = kf.n_frames(len(s))
        res[k] = out[r:r + n]
        r += n
    assert r == len(out) and out.shape[1] == kf.D
    return res


CONFIGS = {
    "fbank_default_23": ("fbank", {}),
    "fbank_40": ("fbank", dict(num_mel_bins=40)),
    "fbank_80": ("fbank", dict(num_mel_bins=80)),
    "fbank_8k_23": ("fbank", dict(sample_frequency=8000.0)),
    "fbank_8k_40": ("fbank", dict(sample_frequency=8000.0, num_mel_bins=40)),
    "fbank_32ms_no_padding": ("fbank", dict(frame_length=32.0, num_mel_bins=40)),
    "fbank_20ms": ("fbank", dict(frame_length=20.0, num_mel_bins=40)),
    "fbank_low0_high-400": ("fbank", dict(num_mel_bins=40, low_freq=0.0, high_freq=-400.0)),
    "fbank_80_low0_high-400_8k": ("fbank", dict(sample_frequency=8000.0, num_mel_bins=80,
                                                low_freq=0.0, high_freq=-400.0)),
    "fbank_hamming": ("fbank", dict(num_mel_bins=40, window_type="hamming")),
    "fbank_hanning": ("fbank", dict(num_mel_bins=40, window_type="hanning")),
    "fbank_rectangular": ("fbank", dict(num_mel_bins=40, window_type="rectangular")),
    "fbank_use_energy": ("fbank", dict(num_mel_bins=40, use_energy=True)),
    "fbank_energy_after_window": ("fbank", dict(use_energy=True, raw_energy=False)),
    "fbank_magnitude": ("fbank", dict(num_mel_bins=40, use_power=False)),
    "fbank_keep_dc_no_preemphasis": ("fbank", dict(num_mel_bins=40, remove_dc_offset=False,
                                                   preemphasis_coefficient=0.0)),
    "mfcc_default": ("mfcc", {}),
    "mfcc_40_8k_hamming": ("mfcc", dict(sample_frequency=8000.0, num_mel_bins=40,
                                        window_type="hamming")),
    "mfcc_c0": ("mfcc", dict(use_energy=False)),
    "mfcc_energy_after_window": ("mfcc", dict(raw_energy=False)),
    "mfcc_c0_raw_energy_false": ("mfcc", dict(use_energy=False, raw_energy=False)),
    "mfcc_no_lifter": ("mfcc", dict(cepstral_lifter=0.0)),
    "mfcc_23_ceps_of_23": ("mfcc", dict(num_ceps=23)),
    "mfcc_magnitude_32ms": ("mfcc", dict(use_power=False, frame_length=32.0, num_mel_bins=40)),
    "mfcc_energy_floor": ("mfcc", dict(energy_floor=1.0e9)),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_kernel_vs_fp64_restatement(name):
    kind, kw = CONFIGS[name]
    L, S, _ = R.geometry(R.options(kind, **kw))
    sig = _signals(R.options(kind, **kw)["sample_frequency"], L, S)
    got = _gpu(sig, kind, **kw)
    assert [len(got[k]) for k in sig] == [13, 13, 13, 13, 1, 2]
    bad = []
    for k, s in sig.items():
        r64 = R.features(s, kind, np.float64, **kw)
        r32 = R.features(s, kind, np.float32, **kw)
        assert got[k].shape == r64.shape and np.isfinite(got[k]).all()
        d_gpu = np.abs(got[k].astype(np.float64) - r64).max()
        d_ref = np.abs(r32.astype(np.float64) - r64).max()
        print("%s / %s: gpu-fp64 %.3g, fp32-fp64 (d_ref) %.3g, ratio %.2f"
              % (name, k, d_gpu, d_ref, d_gpu / d_ref if d_ref else np.inf))
        if not (d_gpu <= 4 * d_ref and d_gpu <= 1e-3):
            bad.append("%s: max|gpu - fp64| = %.3g against 4 x d_ref = 4 x %.3g and 1e-3"
                       % (k, d_gpu, d_ref))
    assert not bad, "; ".join(bad)


def test_energy_floor_is_applied():
    """--energy-floor=1e9 lies above the quiet signals' energy and below the square wave's."""
    sig = _signals(16000.0, 400, 160)
    got = _gpu(sig, "mfcc", energy_floor=1.0e9)
    floor = np.float32(np.log(1.0e9))
    assert (got["noise300"][:, 0] == floor).all() and (got["square"][:, 0] > floor + 1).all()


@pytest.mark.parametrize("kind, kw, e_col, e_val", [
    ("fbank", dict(num_mel_bins=40, use_energy=True), 0, LOG_EPS),
    ("fbank", dict(num_mel_bins=23), None, None),
    ("fbank", dict(use_energy=True, raw_energy=False), 0, float(np.log(np.float32(R.FLT_MIN)))),
    ("fbank", dict(use_energy=True, energy_floor=0.5), 0, float(np.log(0.5))),
    ("mfcc", dict(num_mel_bins=40), 0, LOG_EPS),
])
def test_silence(kind, kw, e_col, e_val):
    """All-zero audio: every mel column is log(FLT_EPSILON) = -15.94 to 4 ulp (4e-6) and the energy
    is at its floor, to 4 ulp of that floor (log(FLT_MIN) = -87.34 for the energy after the window,
    log(--energy-floor) when one is set).  The cepstra above C0 are the DCT of a constant column,
    zero in exact arithmetic: 40 products of at most sqrt(2/40) * 15.94 = 3.6, each rounded to
    2^-24, under a lifter of at most 12 stay below 40 * 3.6 * 6e-8 * 12 = 1e-4."""
    sig = {"silence": np.zeros(400 + 3 * 160, np.int16)}
    got = _gpu(sig, kind, **kw)["silence"]
    assert got.shape[0] == 4
    r64 = R.features(sig["silence"], kind, np.float64, **kw)
    if kind == "fbank":
        mel = got[:, 1:] if e_col is not None else got
        assert mel.shape[1] == kw.get("num_mel_bins", 23)
        assert np.abs(mel.astype(np.float64) - LOG_EPS).max() <= 4e-6
    else:
        assert np.abs(got[:, 1:].astype(np.float64)).max() <= 1e-4
        assert np.abs(r64[:, 1:]).max() <= 1e-4
    if e_col is not None:
        tol = 4 * float(np.spacing(np.float32(abs(e_val))))
        assert np.abs(got[:, e_col].astype(np.float64) - e_val).max() <= tol
        assert np.abs(r64[:, e_col] - e_val).max() <= tol


@pytest.mark.parametrize("kind, kw", [("fbank", dict(num_mel_bins=40, use_energy=True)),
                                      ("mfcc", dict(sample_frequency=8000.0))])
def test_rows_are_independent_and_reruns_identical(kind, kw):
    L, S, _ = R.geometry(R.options(kind, **kw))
    sig = _signals(R.options(kind, **kw)["sample_frequency"], L, S)
    sig = {k: sig[k] for k in ("noise300", "one_frame", "square", "two_frames", "dc4000")}
    whole = _gpu(sig, kind, **kw)
    again = _gpu(sig, kind, **kw)
    for k, s in sig.items():
        assert np.array_equal(_bits(again[k]), _bits(whole[k])), k
        alone = _gpu({k: s}, kind, **kw)[k]
        assert np.array_equal(_bits(alone), _bits(whole[k])), k


def test_rows_in_any_order_and_bad_rows_left_alone():
    """The row maps may name frames in any order; a row naming no whole frame is not written."""
    from pkc import data_io as D
    from pkc import frontend as F
    kf = F.KaldiFeats("fbank", num_mel_bins=40)
    sig = _signals(16000.0, 400, 160)
    sig = {k: sig[k] for k in ("noise300", "two_frames")}
    want = _gpu(sig, "fbank", num_mel_bins=40)
    ka = D.kaldi_feats_args(sig, list(sig), kf)
    dev = [t.to("cuda") for t in ka["pinned"]]
    rs = np.random.RandomState(1)
    perm = rs.permutation(15)
    urow = np.concatenate([dev[3].cpu().numpy()[perm], [0, 1, 2, -1, 1]]).astype(np.int32)
    frow = np.concatenate([dev[4].cpu().numpy()[perm], [13, 2, 0, 0, -1]]).astype(np.int32)
    dev[3], dev[4] = torch.from_numpy(urow).cuda(), torch.from_numpy(frow).cuda()
    out = torch.full((20, 40), float("nan"), dtype=torch.float32, device="cuda")
    D.kaldi_feats_device(dev, kf, torch.cuda.current_stream(), out=out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    flat = np.concatenate([want["noise300"], want["two_frames"]])
    assert np.array_equal(_bits(out[:15]), _bits(flat[perm]))
    assert np.isnan(out[15:]).all()


def _write_wavs(d, sig, fs, name="wav_lst.scp"):
    lst = os.path.join(d, name)
    with open(lst, "w") as f:
        for k, s in sig.items():
            path = os.path.join(d, name + "_" + k + ".wav")
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(fs)
                w.writeframes(s.astype("<i2").tobytes())
            f.write("%s %s\n" % (k, path))
    return lst


def _utts(frames, L, S, seed):
    """{spkX_uNN: int16 noise + tone} with the given frame counts (0: too short for a frame)."""
    rs = np.random.RandomState(seed)
    sig = {}
    for i, nf in enumerate(frames):
        n = L + (nf - 1) * S + rs.randint(0, S) if nf else L - 1
        t = np.arange(n)
        v = rs.normal(0, 400 + 100 * i, n) + 3000 * np.sin(2 * np.pi * (200.0 + 90 * i) * t / 16000)
        sig["spk%d_u%02d" % (i % 2, i)] = np.round(v).astype(np.int16)
    return sig


def _utt2spk(d, sig):
    path = os.path.join(d, "utt2spk")
    with open(path, "w") as f:
        for k in sig:
            f.write("%s %s\n" % (k, k.split("_")[0]))
    return path


def test_pipe_from_wav_list_equals_pipe_from_the_writers_ark(tmp_path):
    """python -m pkc.kaldi_feats writes the fbank ark, scp and per-speaker cmvn stats of seven
    utterances (one too short for a frame); `pkc-fbank | apply-cmvn --utt2spk | add-deltas` from
    the wav list then stages the same chunk, bit for bit, as `apply-cmvn | add-deltas` read from
    that ark.  max_seq_length 40 splits the longer utterances."""
    from pkc import core
    from pkc import data_io as D
    from pkc import frontend as F
    d = str(tmp_path)
    sig = _utts([55, 31, 0, 97, 12, 40, 1], 400, 160, seed=7)
    lst, u2s = _write_wavs(d, sig, 16000), _utt2spk(d, sig)
    ark, scp, cm = (os.path.join(d, n) for n in ("fbank.ark", "fbank.scp", "cmvn.ark"))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [PKG] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    subprocess.run([sys.executable, "-m", "pkc.kaldi_feats", "--wav-lst", lst, "--type", "fbank",
                    "--num-mel-bins=40", "--ark-out", ark, "--scp-out", scp, "--utt2spk", u2s,
                    "--cmvn-out", cm], check=True, env=env, timeout=120)
    kept = [k for k in sig if len(sig[k]) >= 400]
    assert len(kept) == 6
    lines = open(scp).read().splitlines()
    assert [l.split()[0] for l in lines] == kept
    direct = _gpu({k: sig[k] for k in kept}, "fbank", num_mel_bins=40)
    buf = open(ark, "rb").read()
    for k, line in zip(kept, lines):
        path, off = line.split(" ")[1].rsplit(":", 1)
        assert path == ark and buf[int(off) - len(k) - 1:int(off) + 5] == (k + " ").encode() + b"\0BFM "
    arks = dict(D.read_mat_ark_path(ark))
    for k in kept:
        assert np.array_equal(_bits(arks[k]), _bits(direct[k])), k
    with open(cm, "rb") as f:
        stats = F.parse_stats_ark(f.read())
    assert sorted(stats) == ["spk0", "spk1"]
    for spk in stats:
        assert np.array_equal(stats[spk], F.cmvn_stats([arks[k] for k in kept if k.startswith(spk)]))

    tail = "apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | add-deltas --delta-order=2 ark:- ark:- |" \
        % (u2s, cm)
    rs = np.random.RandomState(8)
    lab = {k: rs.randint(0, 50, len(arks[k])).astype(np.int32) for k in kept}
    lab["spk0_u02"] = np.zeros(1, np.int32)           # a label for the utterance without a frame
    staged = []
    for fea_lst, opts in ((lst, "pkc-fbank --num-mel-bins=40 ark:- ark:- | " + tail), (scp, tail)):
        fea, fe = core._read_features(fea_lst, opts, d)
        staged.append(D.stage_chunk(fea, [lab], 40, frontend=fe))
    st, ref = staged
    cur = torch.cuda.current_stream()
    cur.wait_event(st.done)
    cur.wait_event(ref.done)
    assert any("_split" in n for n in ref.names) and any("_split" not in n for n in ref.names)
    assert st.names == ref.names
    assert np.array_equal(np.asarray(st.end_index), np.asarray(ref.end_index))
    assert np.array_equal(st.lab_arrays[0], ref.lab_arrays[0])
    assert st.shape == ref.shape == (sum(len(arks[k]) for k in kept), 120)
    assert st.raw_d.dtype == torch.float32 and torch.equal(st.raw_d, ref.raw_d)
    assert torch.isfinite(st.raw_d).all()
    # the stage alone, no cmvn and no deltas: the features themselves in the sorted / split order
    fea, fe = core._read_features(lst, "pkc-fbank --num-mel-bins=40 ark:- ark:- |", d)
    plain = D.stage_chunk(fea, [lab], 40, frontend=fe)
    ref = D.stage_chunk(arks, [lab], 40)
    cur.wait_event(plain.done)
    cur.wait_event(ref.done)
    assert plain.names == ref.names and torch.equal(plain.raw_d, ref.raw_d)


def _lifecycle(d, streams):
    """Train one chunk and forward one chunk of a tiny MLP whose feature streams come (a) from wav
    lists through the new stages and (b) from the writer's arks.  streams: [(name, kind, options,
    signals)].  Returns nothing; asserts that (a) and (b) agree bit for bit."""
    from oracle import loader as OL
    from pkc import data_io as D
    from pkc import frontend as F
    from pkc.core import run_nn
    from pkc.kaldi_feats import write_feats
    from test_gpu_run_nn import chunk_cfg
    ali = os.path.join(d, "ali")
    os.makedirs(ali)
    fea_wav, fea_ark, nfr = [], [], None
    for name, kind, opts, sig in streams:
        lst, u2s = _write_wavs(d, sig, 16000, name + "_wav.lst"), _utt2spk(d, sig)
        ark, scp, cm = (os.path.join(d, name + e) for e in (".ark", ".scp", "_cmvn.ark"))
        kf = F.KaldiFeats.from_options("pkc-" + kind, dict(o[2:].split("=") for o in opts.split()))
        feats = write_feats(lst, kf, ark, scp, u2s, cm)
        assert nfr is None or nfr == {k: len(m) for k, m in feats.items()}
        nfr = {k: len(m) for k, m in feats.items()}
        tail = ("apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | add-deltas --delta-order=1 "
                "ark:- ark:- |" % (u2s, cm))
        block = "fea_name=%s\nfea_lst=%s\nfea_opts=%s\ncw_left=1\ncw_right=1\n"
        fea_wav.append(block % (name, lst, "pkc-%s %s ark:- ark:- | %s" % (kind, opts, tail)))
        fea_ark.append(block % (name, scp, tail))
    rs = np.random.RandomState(0)
    for i, (k, T) in enumerate(nfr.items()):
        D.write_vec_int_path(os.path.join(ali, "ali_pdf.ark"), rs.randint(0, 64, T), k, append=i > 0)
        D.write_vec_int_path(os.path.join(ali, "ali_phones.ark"), rs.randint(1, 9, T), k, append=i > 0)
    counts = os.path.join(d, "counts")
    with open(counts, "w") as f:
        f.write("[ " + " ".join(str(i + 3) for i in range(64)) + " ]\n")
    names = [s[0] for s in streams]

    def make(cfg_name, to_do, fea, pre=None, counts=None):
        path = chunk_cfg(d, cfg_name, to_do, "unused", ali, counts=counts)
        cfg = configparser.ConfigParser()
        cfg.read(path)
        cfg["data_chunk"]["fea"] = "\n".join(fea)
        model = cfg["model"]["model"]
        if len(names) == 2:
            model = "conc=concatenate(%s,%s)\n" % tuple(names) + model.replace("fmllr", "conc")
        else:
            model = model.replace("fmllr", names[0])
        cfg["model"]["model"] = model
        cfg["architecture1"]["dnn_drop"] = "0.0,0.0"
        cfg["batches"]["max_seq_length_train"] = "40"
        for i in (1, 2, 3):
            if pre:
                cfg["architecture%d" % i]["arch_pretrain_file"] = os.path.join(
                    d, "%s_architecture%d.pkl" % (pre, i))
        with open(path, "w") as f:
            cfg.write(f)
        return path

    res = {}
    for tag, fea in (("wav", fea_wav), ("ark", fea_ark)):
        c_tr = make("train_" + tag, "train", fea)
        run_nn(None, None, None, None, None, None, c_tr, True, c_tr)
        info = configparser.ConfigParser()
        info.read(os.path.join(d, "train_%s.info" % tag))
        pk = [torch.load(os.path.join(d, "train_%s_architecture%d.pkl" % (tag, i)),
                         map_location="cpu", weights_only=True)["model_par"] for i in (1, 2, 3)]
        c_fw = make("forward_" + tag, "forward", fea, pre="train_" + tag, counts=counts)
        run_nn(None, None, None, None, None, None, c_fw, True, c_fw)
        with open(os.path.join(d, "forward_%s_out_dnn2_to_decode.ark" % tag), "rb") as f:
            post = dict(OL.parse_mat_ark(f.read()))
        res[tag] = (info["results"]["loss"], info["results"]["err"], pk, post)
    (l_w, e_w, pk_w, po_w), (l_a, e_a, pk_a, po_a) = res["wav"], res["ark"]
    assert np.isfinite(float(l_w)) and (l_w, e_w) == (l_a, e_a)
    for a, b in zip(pk_w, pk_a):
        assert sorted(a) == sorted(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert sorted(po_w) == sorted(po_a) == sorted(nfr)
    rows = 0
    for k in po_w:
        m = np.asarray(po_w[k])
        # the context window of one frame costs the chunk its first and its last row
        assert m.shape[1] == 64 and nfr[k] - 1 <= m.shape[0] <= nfr[k] and np.isfinite(m).all()
        assert np.array_equal(_bits(m), _bits(np.asarray(po_a[k])))
        rows += m.shape[0]
    assert rows == sum(nfr.values()) - 2


def test_run_nn_fbank_stream_from_a_wav_list(tmp_path):
    sig = _utts([55, 31, 97, 12, 40, 23], 400, 160, seed=11)
    _lifecycle(str(tmp_path), [("fbank", "fbank", "--num-mel-bins=40", sig)])


def test_run_nn_fbank_and_mfcc_streams_from_two_wav_lists(tmp_path):
    """Two streams, each from its own wav list (the same utterance ids, other audio)."""
    a = _utts([55, 31, 97, 12, 40, 23], 400, 160, seed=12)
    b = {k: v[::-1].copy() for k, v in a.items()}
    _lifecycle(str(tmp_path), [("fbank", "fbank", "--num-mel-bins=40 --use-energy=true", a),
                               ("mfcc", "mfcc", "--num-mel-bins=23 --num-ceps=13", b)])

"""Raw-waveform framing on the GPU (pkc_wav_frames, the `pkc-wav-frames` fea_opts stage) against
the reference's save_raw_fea.py output (tests/golden/raw_fea.npz) and its numpy restatement
(tests/raw_ref.py): at kernel level, through the chunk staging of the loader, end to end through
read_lab_fea / run_nn, and through the ark writer.  Everything is compared bit for bit: the path
is exact by construction (an fp64 division of two exactly represented integers, cast to float32
as the ark reader casts the script's float64 rows), so no tolerance appears."""
import configparser
import ctypes as C
import os
import struct
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import raw_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "pytorch-kaldi-cgs_amd")
G = np.load(os.path.join(HERE, "golden", "raw_fea.npz"))
CASES = sorted({k.split("/")[0] for k in G.files})
DEV = "cuda"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _kernel(sigs, W, Lw, S, seed):
    """pkc_wav_frames over every frame of every signal in one call, rows permuted (seed).
    Tables are built here, not by pkc.data_io.  Returns (out (rows, W), utt of row, frame of row)."""
    from pkc._lib import call, ptr
    lens = np.array([len(s) for s in sigs], np.int64)
    ubeg = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    peak = np.array([np.abs(s.astype(np.int64)).max() for s in sigs], np.int32)
    nfr = [raw_ref.n_frames(len(s), Lw, S) for s in sigs]
    urow = np.concatenate([np.full(n, u) for u, n in enumerate(nfr)]).astype(np.int32)
    frow = np.concatenate([np.arange(n) for n in nfr]).astype(np.int32)
    perm = np.random.RandomState(seed).permutation(len(urow))
    urow, frow = urow[perm], frow[perm]
    d = [torch.from_numpy(a).to(DEV) for a in
         (np.concatenate(sigs).astype(np.int16), ubeg, lens.astype(np.int32), peak, urow, frow)]
    out = torch.full((len(urow), W), float("nan"), dtype=torch.float32, device=DEV)
    work = torch.full((int(lens.sum()),), float("nan"), dtype=torch.float32, device=DEV)
    call("pkc_wav_frames", *[ptr(t) for t in d], len(urow), W, Lw, S, ptr(work), ptr(out),
         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy(), urow, frow


def _fixture_run(fs, seed=5):
    names = [k for k in CASES if int(G[k + "/fs"]) == fs]
    W, Lw, S = raw_ref.geometry(fs)
    out, urow, frow = _kernel([G[k + "/signal"] for k in names], W, Lw, S, seed)
    return names, out, urow, frow


@pytest.fixture(scope="module")
def fixture_runs():
    return {fs: _fixture_run(fs) for fs in (1600, 1000, 16000)}


@pytest.mark.parametrize("fs", [1600, 1000, 16000])
def test_kernel_equals_the_reference_script(fixture_runs, fs):
    """Every fixture matrix, cast to float32 as the ark reader casts it, bit for bit; all the
    utterances of one geometry in one call with the rows permuted."""
    names, out, urow, frow = fixture_runs[fs]
    assert sorted(names) == [k for k in CASES if k.startswith("fs%d_" % fs)]
    assert len(out) == sum(len(G[k + "/frames"]) for k in names)
    for u, k in enumerate(names):
        want = G[k + "/frames"].astype(np.float32)
        rows = np.flatnonzero(urow == u)
        assert sorted(frow[rows]) == list(range(len(want)))
        assert np.array_equal(_bits(out[rows]), _bits(want[frow[rows]])), k


def test_kernel_is_deterministic(fixture_runs):
    for fs in (1600, 16000):
        again = _fixture_run(fs)
        assert np.array_equal(_bits(again[1]), _bits(fixture_runs[fs][1]))


def _smallest_framable(W, Lw, S):
    n = Lw + 1
    while True:
        try:
            raw_ref.frames(np.ones(n, np.int16), W, Lw, S)
            return n
        except ValueError:
            n += 1


@pytest.mark.parametrize("fs, W", [(1100, 220), (1010, 202)])
def test_other_geometries_vs_restatement(fs, W):
    """fs 1100: an odd label window with 16-byte rows; fs 1010: W % 4 != 0, the scalar path.
    Several blocks, the last one partial; the shortest framable signal beside longer ones."""
    Wg, Lw, S = raw_ref.geometry(fs)
    assert Wg == W and (W % 4 == 0) == (fs == 1100)
    rs = np.random.RandomState(fs)
    sigs = [rs.randint(-32768, 32768, size=n).astype(np.int16)
            for n in (_smallest_framable(W, Lw, S), 1203, 500, 777)]
    out, urow, frow = _kernel(sigs, W, Lw, S, seed=fs)
    assert len(out) * W > 8 * 1024
    for u, s in enumerate(sigs):
        want = raw_ref.frames(s, W, Lw, S).astype(np.float32)
        rows = np.flatnonzero(urow == u)
        assert np.array_equal(_bits(out[rows]), _bits(want[frow[rows]]))


def test_entry_point_refuses_bad_arguments():
    from pkc import _lib as L
    t = torch.zeros(64, dtype=torch.float32, device=DEV)
    p = L.ptr(t)
    ok = [p, p, p, p, p, p, 1, 320, 40, 16, p, p, None]
    assert L.lib().pkc_wav_frames(*(ok[:6] + [0] + ok[7:])) == L.PKC_OK          # no launch
    for i, v in ((0, None), (10, None), (11, None), (6, -1), (7, 321), (7, 0), (7, -320),
                 (8, 1), (9, 0)):
        args = list(ok)
        args[i] = v
        assert L.lib().pkc_wav_frames(*args) == L.PKC_ERR_ARG, (i, v)
    torch.cuda.synchronize()


def _utts(lengths, seed):
    rs = np.random.RandomState(seed)
    sig = {"spk0_u%03d" % i: rs.randint(-32768, 32768, size=n).astype(np.int16)
           for i, n in enumerate(lengths)}
    return sig


def test_staging_order_matches_the_ark_path():
    """Six utterances at fs 1600, max_seq 40 so that some are split: the wav-staged chunk equals
    stage_chunk fed the restatement's frames as a dict."""
    from pkc import data_io as D
    from pkc import frontend as F
    fe = F.FeaFrontend.parse("pkc-wav-frames --fs=1600 ark:- ark:- |")
    wf = fe.wav
    sig = _utts([1500, 400, 1111, 680, 999, 845], seed=21)
    rs = np.random.RandomState(22)
    fr = {k: raw_ref.frames(s, wf.W, wf.Lw, wf.S).astype(np.float32) for k, s in sig.items()}
    lab = {k: rs.randint(0, 50, len(m)).astype(np.int32) for k, m in fr.items()}
    st = D.stage_chunk({k: wf.signal(k, s) for k, s in sig.items()}, [lab], 40, frontend=fe)
    ref = D.stage_chunk(fr, [lab], 40)
    cur = torch.cuda.current_stream()
    cur.wait_event(st.done)
    cur.wait_event(ref.done)
    assert any("_split" in n for n in ref.names) and any("_split" not in n for n in ref.names)
    assert st.names == ref.names
    assert np.array_equal(np.asarray(st.end_index), np.asarray(ref.end_index))
    assert len(st.lab_arrays) == 1 and np.array_equal(st.lab_arrays[0], ref.lab_arrays[0])
    assert st.shape == ref.shape == (sum(len(m) for m in fr.values()), 320)
    assert st.raw_d.dtype == torch.float32 and torch.equal(st.raw_d, ref.raw_d)


def _write_wavs(d, sig, fs):
    lst = os.path.join(d, "wav_lst.scp")
    with open(lst, "w") as f:
        for k, s in sig.items():
            path = os.path.join(d, k + ".wav")
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(fs)
                w.writeframes(s.astype("<i2").tobytes())
            f.write("%s %s\n" % (k, path))
    return lst


def test_read_lab_fea_and_run_nn_from_a_wav_list(tmp_path):
    """The small SincNet of test_run_nn_sincnet_train_and_forward over a wav list (input 320, the
    fs 1600 geometry): the prepared chunk is bit-equal to the one the same cfg prepares from an FM
    ark of the restatement's frames; train one chunk, then forward mode."""
    from oracle import loader as OL
    from pkc import core
    from pkc import data_io as D
    from pkc.core import run_nn
    from test_gpu_run_nn import chunk_cfg
    from test_gpu_sincnet import CASES as SINC_CASES, SGD, SINC_LR
    d = str(tmp_path)
    W, Lw, S = raw_ref.geometry(1600)
    sig = _utts([1500, 640, 1111, 680, 999, 845], seed=31)
    lst = _write_wavs(d, sig, 1600)
    ark, scp, ali = os.path.join(d, "raw.ark"), os.path.join(d, "raw.scp"), os.path.join(d, "ali")
    os.makedirs(ali)
    rs = np.random.RandomState(0)
    nfr = {}
    with open(scp, "w") as f:
        for i, (k, s) in enumerate(sig.items()):
            m = raw_ref.frames(s, W, Lw, S).astype(np.float32)
            nfr[k] = T = len(m)
            D.write_mat_path(ark, m, k, append=i > 0)
            D.write_vec_int_path(os.path.join(ali, "ali_pdf.ark"), rs.randint(0, 64, T), k, append=i > 0)
            D.write_vec_int_path(os.path.join(ali, "ali_phones.ark"), rs.randint(1, 9, T), k,
                                 append=i > 0)
            f.write("%s %s\n" % (k, ark))
    counts = os.path.join(d, "counts")
    with open(counts, "w") as f:
        f.write("[ " + " ".join(str(i + 3) for i in range(64)) + " ]\n")
    sinc = dict(SINC_CASES["none"], arch_library="pkc.neural_networks", arch_class="SincNet",
                arch_name="MLP_layers1", arch_pretrain_file="none", arch_seq_model="False",
                sinc_use_laynorm_inp="True", sinc_use_laynorm="True,False",
                sinc_use_batchnorm="False,True", sinc_act="relu,leaky_relu", sinc_drop="0.15,0.0",
                **dict(SGD, arch_lr=SINC_LR))
    stage = "pkc-wav-frames --sig-wlen=200 --lab-wlen=25 --lab-wshift=10 --fs=1600 ark:- ark:- |"

    def make(name, to_do, fea_lst, fea_opts, pre=None, counts=None):
        path = chunk_cfg(d, name, to_do, scp, ali, counts=counts)
        cfg = configparser.ConfigParser()
        cfg.read(path)
        cfg["architecture1"] = dict(sinc)
        cfg["data_chunk"]["fea"] = ("fea_name=raw\nfea_lst=%s\nfea_opts=%s\ncw_left=0\ncw_right=0\n"
                                    % (fea_lst, fea_opts))
        cfg["model"]["model"] = cfg["model"]["model"].replace("fmllr", "raw")
        for i in (1, 2, 3):
            if pre:
                cfg["architecture%d" % i]["arch_pretrain_file"] = os.path.join(
                    d, "%s_architecture%d.pkl" % (pre, i))
        with open(path, "w") as f:
            cfg.write(f)
        return path

    c_tr = make("train_ck0", "train", lst, stage)
    c_ark = make("train_ark", "train", scp, "")
    chunks = []
    for c in (c_tr, c_ark):
        shared = []
        np.random.seed(2234)
        core.read_lab_fea(c, False, shared, d)
        chunks.append(core._finish_chunk(shared))
    (n_w, ch_w, e_w, fd_w, ld_w, _), (n_a, ch_a, e_a, fd_a, ld_a, _) = chunks
    assert n_w == n_a and sorted(n_w) == sorted(sig)
    assert np.array_equal(np.asarray(e_w), np.asarray(e_a))
    assert ch_w.feats.shape == (sum(nfr.values()), 320)
    assert torch.equal(ch_w.feats, ch_a.feats)
    assert torch.equal(ch_w.labels, ch_a.labels)
    assert fd_w["raw"][5:] == fd_a["raw"][5:] == [0, 320, 320] and ld_w == ld_a

    run_nn(None, None, None, None, None, None, c_tr, True, c_tr)
    info = configparser.ConfigParser()
    info.read(os.path.join(d, "train_ck0.info"))
    assert np.isfinite(float(info["results"]["loss"]))
    for i in (1, 2, 3):
        assert os.path.getsize(os.path.join(d, "train_ck0_architecture%d.pkl" % i)) > 0
    c_fw = make("forward", "forward", lst, stage, pre="train_ck0", counts=counts)
    run_nn(None, None, None, None, None, None, c_fw, True, c_fw)
    with open(os.path.join(d, "forward_out_dnn2_to_decode.ark"), "rb") as f:
        mats = dict(OL.parse_mat_ark(f.read()))
    assert sorted(mats) == sorted(sig)
    for k, m in mats.items():
        m = np.asarray(m)
        assert m.shape == (nfr[k], 64) and np.isfinite(m).all()


def test_writer_tool_in_a_child_process(tmp_path):
    """python -m pkc.raw_fea on two fixture signals: <out>/<utt>.ark holds the fixture cast to
    float32 under the key <utt>, and the scp offset points at the matrix header."""
    d = str(tmp_path)
    names = ["fs1600_n307", "fs1600_n777_negpeak"]
    lst = _write_wavs(d, {k: G[k + "/signal"] for k in names}, 1600)
    out, scp = os.path.join(d, "raw_200ms"), os.path.join(d, "feats_raw.scp")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [PKG] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    subprocess.run([sys.executable, "-m", "pkc.raw_fea", "--wav-lst", lst, "--out-folder", out,
                    "--scp-out", scp, "--fs", "1600"], check=True, env=env, timeout=120)
    lines = open(scp).read().splitlines()
    assert lines == ["%s %s/%s.ark:%d" % (k, out, k, len(k) + 1) for k in names]
    for k, line in zip(names, lines):
        path, off = line.split(" ")[1].rsplit(":", 1)
        buf = open(path, "rb").read()
        off = int(off)
        assert buf[:off] == (k + " ").encode()
        assert buf[off:off + 6] == b"\0BFM \x04" and buf[off + 10:off + 11] == b"\x04"
        rows, cols = struct.unpack("<i", buf[off + 6:off + 10])[0], struct.unpack(
            "<i", buf[off + 11:off + 15])[0]
        want = G[k + "/frames"].astype(np.float32)
        assert (rows, cols) == want.shape and len(buf) == off + 15 + 4 * rows * cols
        got = np.frombuffer(buf[off + 15:], dtype="<f4").reshape(rows, cols)
        assert np.array_equal(_bits(got), _bits(want))

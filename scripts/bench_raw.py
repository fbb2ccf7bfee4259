"""Loading one `raw` chunk of the TIMIT_SincNet_raw geometry two ways (informational; bench.py is
the project's benchmark): W 3200, Lw 400, S 160 at 16 kHz, about 700 utterances of U[150, 450]
frames of seeded int16 noise, seed 2234.

  (a) ark: fea_lst is an scp over float32 `FM` arks of the framed rows (written by pkc.raw_fea,
      one ark per utterance as save_raw_fea.py lays them out), fea_opts empty;
  (b) wav: fea_lst is the wav list, fea_opts is the pkc-wav-frames stage.

Each leg is core._read_features + data_io.stage_chunk + PendingChunk.finish (chunk z-normalisation
into the chunk matrix) ending in a device synchronise, timed with the host clock; the two legs
alternate in one process after a warm-up of each, and the medians over the repeats are reported
with the bytes each leg reads from disk and uploads.  The files are read through the page cache
(they were just written): the ark leg's disk time on a cold cache is not in these numbers.
pkc_wav_frames alone (both launches) is timed with HIP events over the same chunk; its write rate
is the N x W x 4 bytes of the output over that time, against the HBM peak the project uses.
Writes profiles/raw_frames_chunk.json.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-kaldi-cgs_amd")):
    sys.path.insert(0, p)

HBM_GBS = 8000.0
STAGE = "pkc-wav-frames --sig-wlen=200 --lab-wlen=25 --lab-wshift=10 --fs=16000 ark:- ark:- |"


def make_wavs(d, n_utt, seed, wav):
    rs = np.random.RandomState(seed)
    lst = os.path.join(d, "wav_lst.scp")
    nbytes = 0
    with open(lst, "w") as f:
        for i in range(n_utt):
            frames = rs.randint(150, 451)
            s = rs.randint(-32768, 32768, size=wav.Lw + frames * wav.S).astype("<i2")
            path = os.path.join(d, "u%04d.wav" % i)
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(wav.fs)
                w.writeframes(s.tobytes())
            nbytes += os.path.getsize(path)
            f.write("u%04d %s\n" % (i, path))
    return lst, nbytes


def leg(fea_lst, fea_opts, d):
    """One chunk load; returns (ms of read / stage / finish / total, bytes uploaded, chunk)."""
    from pkc import core
    from pkc import data_io as D
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fea, fe = core._read_features(fea_lst, fea_opts, d)
    t1 = time.perf_counter()
    st = D.stage_chunk(fea, [], 1000, frontend=fe)
    t2 = time.perf_counter()
    ch = D.PendingChunk([(st, 0, 0, "raw")], [], [], 1000, None).finish()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    up = sum(t.numel() * t.element_size() for t in st._pinned)
    ms = dict(read_ms=1e3 * (t1 - t0), stage_ms=1e3 * (t2 - t1), finish_ms=1e3 * (t3 - t2),
              wall_ms=1e3 * (t3 - t0))
    return ms, up, ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=700)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--tmp", default=None, help="folder for the synthetic wavs and arks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_frames_chunk.json"))
    a = ap.parse_args()
    from pkc import data_io as D
    from pkc import raw_fea
    from pkc.frontend import WavFrames, read_wav_list

    assert torch.cuda.is_available(), "bench_raw needs a GPU"
    wav = WavFrames()
    d = tempfile.mkdtemp(prefix="bench_raw_", dir=a.tmp)
    try:
        lst, wav_bytes = make_wavs(d, a.utts, 2234, wav)
        t0 = time.perf_counter()
        scp = os.path.join(d, "feats_raw.scp")
        raw_fea.write_raw_arks(lst, os.path.join(d, "arks"), scp, wav)
        write_s = time.perf_counter() - t0
        ark_bytes = sum(os.path.getsize(os.path.join(d, "arks", f))
                        for f in os.listdir(os.path.join(d, "arks")))
        legs = {"ark": (scp, ""), "wav": (lst, STAGE)}
        runs = {k: [] for k in legs}
        up, same = {}, None
        for rep in range(a.reps + 1):                 # rep 0 warms both legs up
            got = {}
            for k, (fl, fo) in legs.items():
                ms, up[k], ch = leg(fl, fo, d)
                print("rep %d %s %.0f ms" % (rep, k, ms["wall_ms"]), file=sys.stderr, flush=True)
                if rep:
                    runs[k].append(ms)
                elif k == "wav":
                    same = bool(torch.equal(ch.feats, got["ark"]))
                    rows = int(ch.feats.shape[0])
                got[k] = ch.feats if not rep else None
                del ch
            del got
        res = dict(device=torch.cuda.get_device_name(0), utterances=a.utts, rows=rows, W=wav.W,
                   seed=2234, reps=a.reps, chunk_matrices_bit_equal=same,
                   ark_written_by_pkc_raw_fea_s=write_s)
        for k in legs:
            res[k] = {f: statistics.median(r[f] for r in runs[k]) for f in runs[k][0]}
            res[k]["wall_ms_min"] = min(r["wall_ms"] for r in runs[k])
            res[k]["wall_ms_max"] = max(r["wall_ms"] for r in runs[k])
            res[k]["bytes_read_from_disk"] = ark_bytes if k == "ark" else wav_bytes
            res[k]["bytes_uploaded"] = up[k]
        res["disk_byte_ratio"] = ark_bytes / wav_bytes
        res["upload_byte_ratio"] = up["ark"] / up["wav"]
        res["wall_ratio_ark_over_wav"] = res["ark"]["wall_ms"] / res["wav"]["wall_ms"]

        # the kernel alone: the whole chunk, every frame of every utterance, HIP events
        sig = {k: wav.read(k, p) for k, p in read_wav_list(lst)}
        pieces = [(k, 0, wav.n_frames(len(s))) for k, (s, _) in sig.items()]
        dev_t = [t.to("cuda") for t in D.wav_args(sig, pieces, wav)["pinned"]]
        cur = torch.cuda.current_stream()
        for _ in range(3):
            out, work = D.wav_frames_device(dev_t, wav, cur)
        torch.cuda.synchronize()
        us = []
        samples, ubeg, ulen, upeak, urow, frow = dev_t
        for _ in range(a.kernel_reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            D.call("pkc_wav_frames", D.ptr(samples), D.ptr(ubeg), D.ptr(ulen), D.ptr(upeak),
                   D.ptr(urow), D.ptr(frow), urow.numel(), wav.W, wav.Lw, wav.S, D.ptr(work),
                   D.ptr(out), C.c_void_p(cur.cuda_stream))
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1))
        written = out.numel() * 4
        med = statistics.median(us)
        res["kernel"] = dict(us_median=med, us_min=min(us), us_max=max(us), reps=a.kernel_reps,
                             bytes_written=written, samples=int(samples.numel()),
                             write_gbs=written / (med * 1e-6) / 1e9, hbm_peak_gbs=HBM_GBS,
                             frac_hbm_peak=written / (med * 1e-6) / 1e9 / HBM_GBS,
                             note="both launches (normalise + gather); writes only, the "
                                  "normalise pass adds 6 B per sample of traffic")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

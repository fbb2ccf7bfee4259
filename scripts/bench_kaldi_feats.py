"""Loading one fbank chunk of TIMIT's shape two ways (informational; bench.py is the project's
benchmark): 740 utterances of U[150, 450] frames (about 222 k frames) of seeded int16 noise at
16 kHz, 40 mel bins, cmvn per speaker (74 speakers) and delta-order 2, seed 2234.

  (a) ark: fea_lst is an scp over the float32 `FM` ark python -m pkc.kaldi_feats wrote, fea_opts is
      `apply-cmvn --utt2spk | add-deltas` (the existing path);
  (b) wav: fea_lst is the wav list, fea_opts is `pkc-fbank --num-mel-bins=40 |` in front of the
      same two stages (the new path).

Each leg is core._read_features + data_io.stage_chunk + PendingChunk.finish ending in a device
synchronise, timed with the host clock; the legs alternate in one process after a warm-up of each
and the medians over the repeats are reported with the bytes each reads from disk and uploads.
The files are read through the page cache (they were just written).  pkc_kaldi_feats alone is
timed with HIP events over every frame of the chunk, fbank and mfcc; beside its time stand the
bytes it moves through HBM, and its LDS traffic and fp64 operation counts derived from the
kernel's loops, each against the chip's rate, to show which of them is nearest.
Writes profiles/kaldi_feats_chunk.json.
"""
import argparse
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
LDS_GBS = 256 * 128 * 2.4          # 256 CUs x 128 B/clk x 2.4 GHz
FP64_GFLOPS = 78600.0              # vector fp64, datasheet


def make_wavs(d, n_utt, seed, kf):
    rs = np.random.RandomState(seed)
    lst, u2s = os.path.join(d, "wav_lst.scp"), os.path.join(d, "utt2spk")
    nbytes = 0
    with open(lst, "w") as f, open(u2s, "w") as g:
        for i in range(n_utt):
            frames = rs.randint(150, 451)
            s = np.clip(rs.normal(0, 3000, kf.L + (frames - 1) * kf.S), -32768, 32767).astype("<i2")
            path = os.path.join(d, "u%04d.wav" % i)
            with wave.open(path, "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(int(kf.fs))
                w.writeframes(s.tobytes())
            nbytes += os.path.getsize(path)
            f.write("u%04d %s\n" % (i, path))
            g.write("u%04d spk%02d\n" % (i, i % 74))
    return lst, u2s, nbytes


def leg(fea_lst, fea_opts, d):
    from pkc import core
    from pkc import data_io as D
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fea, fe = core._read_features(fea_lst, fea_opts, d)
    t1 = time.perf_counter()
    st = D.stage_chunk(fea, [], 1000, frontend=fe)
    t2 = time.perf_counter()
    ch = D.PendingChunk([(st, 0, 0, "fbank")], [], [], 1000, None).finish()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    up = sum(t.numel() * t.element_size() for t in st._pinned)
    ms = dict(read_ms=1e3 * (t1 - t0), stage_ms=1e3 * (t2 - t1), finish_ms=1e3 * (t3 - t2),
              wall_ms=1e3 * (t3 - t0))
    return ms, up, ch


def kernel_alone(sig, kf, reps):
    from pkc import data_io as D
    ka = D.kaldi_feats_args(sig, list(sig), kf)
    dev_t = [t.to("cuda") for t in ka["pinned"]]
    cur = torch.cuda.current_stream()
    out = torch.empty(ka["rows"], kf.D, dtype=torch.float32, device="cuda")
    for _ in range(3):
        D.kaldi_feats_device(dev_t, kf, cur, out=out)
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        D.kaldi_feats_device(dev_t, kf, cur, out=out)
        e1.record()
        torch.cuda.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    med = statistics.median(us)
    rows, M = ka["rows"], kf.N // 2
    logM = M.bit_length() - 1
    hbm = int(dev_t[0].numel()) * 2 + out.numel() * 4
    # per frame: the bit-reversed store (N doubles), logM radix-2 stages (each reads and writes M
    # complex doubles), the split step (2 M complex reads, M double writes), the mel sums (one
    # double read per weight)
    nw = int(kf.tables()["mel_weight"].size)
    lds = rows * (8 * kf.N + logM * 2 * 16 * M + (2 * 16 + 8) * M + 8 * nw)
    flop = rows * (logM * (M // 2) * 10 + M * 17 + 2 * nw + 2 * kf.C * kf.B)
    s = med * 1e-6
    return dict(kind=kf.kind, D=kf.D, rows=rows, us_median=med, us_min=min(us), us_max=max(us),
                reps=reps, frames_per_s=rows / s, samples=int(dev_t[0].numel()),
                hbm_bytes=hbm, hbm_gbs=hbm / s / 1e9, frac_hbm_peak=hbm / s / 1e9 / HBM_GBS,
                lds_bytes=lds, lds_gbs=lds / s / 1e9, frac_lds_peak=lds / s / 1e9 / LDS_GBS,
                fp64_flop=flop, fp64_gflops=flop / s / 1e9,
                frac_fp64_peak=flop / s / 1e9 / FP64_GFLOPS,
                barriers_per_frame=logM + 3, waves_per_frame=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=740)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--tmp", default=None, help="folder for the synthetic wavs and arks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kaldi_feats_chunk.json"))
    a = ap.parse_args()
    from pkc import kaldi_feats as KF
    from pkc.frontend import KaldiFeats, read_wav_list

    assert torch.cuda.is_available(), "bench_kaldi_feats needs a GPU"
    kf = KaldiFeats("fbank", num_mel_bins=40)
    d = tempfile.mkdtemp(prefix="bench_kf_", dir=a.tmp)
    try:
        lst, u2s, wav_bytes = make_wavs(d, a.utts, 2234, kf)
        ark, scp, cm = (os.path.join(d, n) for n in ("fbank.ark", "fbank.scp", "cmvn.ark"))
        t0 = time.perf_counter()
        KF.write_feats(lst, kf, ark, scp, u2s, cm)
        write_s = time.perf_counter() - t0
        tail = ("apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | add-deltas --delta-order=2 "
                "ark:- ark:- |" % (u2s, cm))
        legs = {"ark": (scp, tail), "wav": (lst, "pkc-fbank --num-mel-bins=40 ark:- ark:- | " + tail)}
        runs = {k: [] for k in legs}
        up, same, rows = {}, None, 0
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
        res = dict(device=torch.cuda.get_device_name(0), utterances=a.utts, rows=rows,
                   columns=120, seed=2234, reps=a.reps, chunk_matrices_bit_equal=same,
                   ark_and_stats_written_by_pkc_kaldi_feats_s=write_s)
        for k in legs:
            res[k] = {f: statistics.median(r[f] for r in runs[k]) for f in runs[k][0]}
            res[k]["wall_ms_min"] = min(r["wall_ms"] for r in runs[k])
            res[k]["wall_ms_max"] = max(r["wall_ms"] for r in runs[k])
            res[k]["bytes_read_from_disk"] = os.path.getsize(ark) if k == "ark" else wav_bytes
            res[k]["bytes_uploaded"] = up[k]
        res["wall_ratio_ark_over_wav"] = res["ark"]["wall_ms"] / res["wav"]["wall_ms"]
        sig = {k: kf.read(k, p) for k, p in read_wav_list(lst)}
        res["kernel_fbank40"] = kernel_alone(sig, kf, a.kernel_reps)
        res["kernel_mfcc13"] = kernel_alone(sig, KaldiFeats("mfcc"), a.kernel_reps)
        res["peaks"] = dict(hbm_gbs=HBM_GBS, lds_gbs=LDS_GBS, fp64_gflops=FP64_GFLOPS)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

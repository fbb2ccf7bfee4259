"""Staging one fMLLR chunk of TIMIT's shape two ways (informational; bench.py is the project's
benchmark): 740 utterances of U[150, 450] frames (about 222 k frames) of seeded 13-dimensional
MFCC-like noise, 74 speakers, seed 2234, through the pipe of make_fmllr_feats.sh and a cfg's own
normalisation:

    apply-cmvn --utt2spk | splice-feats +-3 | transform-feats final.mat (40 x 91) |
    transform-feats --utt2spk trans.ark (40 x 41 per speaker) | apply-cmvn --utt2spk |
    add-deltas --delta-order=0

  (a) dumped: fea_lst is an scp over the 40-dimensional ark python -m pkc.feat_pipe wrote (what
      Kaldi's script would have dumped), fea_opts is the last two stages (the existing path);
  (b) pipe: fea_lst is the MFCC scp, fea_opts is the whole pipe (the new path).

Each leg is core._read_features + data_io.stage_chunk + PendingChunk.finish ending in a device
synchronise, timed with the host clock; the legs alternate in one process after a warm-up of each
and the medians over the repeats are reported with the bytes each reads from disk and uploads.
The files are read through the page cache (they were just written).  The two pkc_feat_transform
launches are timed alone with HIP events around batches of back-to-back launches over every frame
of the chunk (so the inputs are warm in the last-level cache); beside each time stand the bytes
the algorithm must move through HBM (frames in, rows out, the matrices once) against the chip's
bandwidth, its fused multiply-adds against the fp32 vector rate and the LDS bytes its inner loop
reads against the LDS rate, to show which of them is nearest.
Writes profiles/feat_pipe_chunk.json.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-kaldi-cgs_amd")):
    sys.path.insert(0, p)

HBM_GBS = 8000.0
LDS_GBS = 256 * 128 * 2.4          # 256 CUs x 128 B/clk x 2.4 GHz
FP32_GFLOPS = 157300.0             # vector fp32, datasheet


def fm_bytes(m):
    import struct
    m = np.ascontiguousarray(m, dtype="<f4")
    return (b"\0BFM \x04" + struct.pack("<i", m.shape[0]) + b"\x04" + struct.pack("<i", m.shape[1])
            + m.tobytes())


def make_inputs(d, n_utt, seed):
    """MFCC ark / scp / cmvn stats, utt2spk, final.mat and trans.ark -> their paths."""
    from pkc.kaldi_feats import write_matrices
    rs = np.random.RandomState(seed)
    u2s = os.path.join(d, "utt2spk")
    with open(u2s, "w") as g:
        for i in range(n_utt):
            g.write("u%04d spk%02d\n" % (i, i % 74))
    mats = (("u%04d" % i, (rs.randn(rs.randint(150, 451), 13) * 4 + 2).astype(np.float32))
            for i in range(n_utt))
    ark, scp, cm = (os.path.join(d, n) for n in ("mfcc.ark", "mfcc.scp", "cmvn.ark"))
    write_matrices(mats, ark, scp, u2s, cm)
    final, trans = os.path.join(d, "final.mat"), os.path.join(d, "trans.ark")
    with open(final, "wb") as f:
        f.write(fm_bytes(rs.randn(40, 91) / np.sqrt(91)))
    with open(trans, "wb") as f:
        for s in range(74):
            f.write(("spk%02d " % s).encode() + fm_bytes(np.eye(40, 41) + rs.randn(40, 41) * 0.05))
    return dict(ark=ark, scp=scp, cm=cm, u2s=u2s, final=final, trans=trans)


def leg(fea_lst, fea_opts, d):
    from pkc import core
    from pkc import data_io as D
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fea, fe = core._read_features(fea_lst, fea_opts, d)
    t1 = time.perf_counter()
    st = D.stage_chunk(fea, [], 1000, frontend=fe)
    t2 = time.perf_counter()
    ch = D.PendingChunk([(st, 0, 0, "fmllr")], [], [], 1000, None).finish()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    up = sum(t.numel() * t.element_size() for t in st._pinned)
    ms = dict(read_ms=1e3 * (t1 - t0), stage_ms=1e3 * (t2 - t1), finish_ms=1e3 * (t3 - t2),
              wall_ms=1e3 * (t3 - t0))
    return ms, up, ch


def launches_alone(scp, fea_opts, d, reps, batch):
    """Each pkc_feat_transform launch of the pipe alone, over the whole chunk."""
    from pkc import core
    from pkc import data_io as D
    fea, fe = core._read_features(scp, fea_opts, d)
    lens = {k: len(v) for k, v in fea.items()}
    _, pieces, _, _ = D.dataset_pieces(lens, [], 1000)
    fa = D.frontend_args(fea, pieces, fe)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in [fa["raw"]] + fa["arrays"]]
    cur = torch.cuda.current_stream()
    _, srcs = D.feat_pipe_device(dev[0], dev[1:], fa, cur)
    torch.cuda.synchronize()
    res = {}
    for ln, src in zip(fa["launches"], srcs):
        if ln["kind"] != "transform":
            continue
        one = dict(fa, launches=[ln])
        for _ in range(3):
            D.feat_pipe_device(src, dev[1:], one, cur)
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                D.feat_pipe_device(src, dev[1:], one, cur)
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / batch)
        med = statistics.median(us)
        s = med * 1e-6
        rows, K = ln["rows"], ln["D"] * (ln["left"] + ln["right"] + 1)
        mats = dev[1 + ln["at"] + 1]
        hbm = 4 * (rows * ln["D"] + rows * ln["Dout"] + mats.numel())
        fma = rows * K * ln["Dout"]
        # inner loop: per k one 16-byte matrix read and four 4-byte frame reads feed 16 FMAs
        lds = fma * 2
        name = "%dx%d%s" % (ln["Dout"], K + ln["affine"], "_per_speaker" if ln["n_mats"] > 1 else "")
        res[name] = dict(rows=rows, D=ln["D"], left=ln["left"], right=ln["right"], K=K,
                         Dout=ln["Dout"], affine=ln["affine"], matrices=ln["n_mats"],
                         tiles=ln["n_tiles"], us_median=med, us_min=min(us), us_max=max(us),
                         reps=reps, launches_per_rep=batch, frames_per_s=rows / s,
                         hbm_bytes=hbm, hbm_gbs=hbm / s / 1e9, frac_hbm_peak=hbm / s / 1e9 / HBM_GBS,
                         fma=fma, fp32_gflops=2 * fma / s / 1e9,
                         frac_fp32_peak=2 * fma / s / 1e9 / FP32_GFLOPS,
                         lds_bytes=lds, lds_gbs=lds / s / 1e9, frac_lds_peak=lds / s / 1e9 / LDS_GBS)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=740)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=15)
    ap.add_argument("--kernel-batch", type=int, default=20)
    ap.add_argument("--tmp", default=None, help="folder for the synthetic arks")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feat_pipe_chunk.json"))
    a = ap.parse_args()
    from pkc import feat_pipe as FP
    from pkc.kaldi_feats import write_matrices

    assert torch.cuda.is_available(), "bench_feat_pipe needs a GPU"
    d = tempfile.mkdtemp(prefix="bench_fp_", dir=a.tmp)
    try:
        f = make_inputs(d, a.utts, 2234)
        head = ("apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | "
                "splice-feats --left-context=3 --right-context=3 ark:- ark:- | "
                "transform-feats %s ark:- ark:- | "
                "transform-feats --utt2spk=ark:%s ark:%s ark:- ark:- |"
                % (f["u2s"], f["cm"], f["final"], f["u2s"], f["trans"]))
        ark, scp, cm2 = (os.path.join(d, n) for n in ("fmllr.ark", "fmllr.scp", "cmvn_fmllr.ark"))
        t0 = time.perf_counter()
        write_matrices(FP.pipe_matrices(f["scp"], head), ark, scp, f["u2s"], cm2)
        write_s = time.perf_counter() - t0
        tail = ("apply-cmvn --utt2spk=ark:%s ark:%s ark:- ark:- | add-deltas --delta-order=0 "
                "ark:- ark:- |" % (f["u2s"], cm2))
        legs = {"dumped": (scp, tail), "pipe": (f["scp"], head + " " + tail)}
        runs = {k: [] for k in legs}
        up, same, rows = {}, None, 0
        for rep in range(a.reps + 1):                 # rep 0 warms both legs up
            got = {}
            for k, (fl, fo) in legs.items():
                ms, up[k], ch = leg(fl, fo, d)
                print("rep %d %s %.0f ms" % (rep, k, ms["wall_ms"]), file=sys.stderr, flush=True)
                if rep:
                    runs[k].append(ms)
                elif k == "pipe":
                    same = bool(torch.equal(ch.feats, got["dumped"]))
                    rows = int(ch.feats.shape[0])
                got[k] = ch.feats if not rep else None
                del ch
            del got
        res = dict(device=torch.cuda.get_device_name(0), utterances=a.utts, rows=rows, columns=40,
                   seed=2234, reps=a.reps, chunk_matrices_bit_equal=same,
                   ark_and_stats_written_by_pkc_feat_pipe_s=write_s)
        for k in legs:
            res[k] = {fld: statistics.median(r[fld] for r in runs[k]) for fld in runs[k][0]}
            res[k]["wall_ms_min"] = min(r["wall_ms"] for r in runs[k])
            res[k]["wall_ms_max"] = max(r["wall_ms"] for r in runs[k])
            res[k]["bytes_read_from_disk"] = os.path.getsize(ark if k == "dumped" else f["ark"])
            res[k]["bytes_uploaded"] = up[k]
        res["wall_ratio_dumped_over_pipe"] = res["dumped"]["wall_ms"] / res["pipe"]["wall_ms"]
        res["launches"] = launches_alone(f["scp"], head + " " + tail, d, a.kernel_reps,
                                         a.kernel_batch)
        res["peaks"] = dict(hbm_gbs=HBM_GBS, lds_gbs=LDS_GBS, fp32_gflops=FP32_GFLOPS)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

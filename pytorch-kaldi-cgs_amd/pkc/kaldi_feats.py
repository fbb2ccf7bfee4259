"""python -m pkc.kaldi_feats — write Kaldi fbank / MFCC arks (and their cmvn statistics) from a
wav list, without Kaldi.

    python -m pkc.kaldi_feats --wav-lst L --type fbank|mfcc [stage options | --config F]
                              --ark-out A --scp-out S [--utt2spk U --cmvn-out C]

For every ``utt_id /path/file.wav`` line of L: one float32 (``FM``) matrix under the key ``utt_id``
in A and the line ``utt_id A:<offset>`` in S, as ``compute-fbank-feats ... ark,scp:A,S`` /
``compute-mfcc-feats`` write them; an utterance too short for one frame is left out, as Kaldi
leaves it out.  The stage options are those of the ``pkc-fbank`` / ``pkc-mfcc`` fea_opts stages
(Kaldi's names and defaults, --dither=0) and the rows come from the same kernel
(pkc_kaldi_feats).  With --cmvn-out, C is the ``compute-cmvn-stats`` archive the ``apply-cmvn``
stage reads: per speaker of U (per utterance without --utt2spk) a (2, D+1) double matrix
[sum x, count; sum x^2, 0], accumulated in float64 from the float32 features.
"""
import argparse
import os
import struct

import numpy as np

from . import data_io as D
from .frontend import KaldiFeats, cmvn_stats, read_utt2spk, read_wav_list


def write_stats_ark(path, stats):
    """{key: (2, D+1) float64} -> binary ``DM`` archive."""
    with open(path, "wb") as f:
        for key, st in stats.items():
            st = np.ascontiguousarray(st, dtype="<f8")
            f.write((key + " ").encode("latin1") + b"\0BDM " + b"\x04"
                    + struct.pack("<i", st.shape[0]) + b"\x04" + struct.pack("<i", st.shape[1])
                    + st.tobytes())


def write_matrices(mats, ark_out, scp_out, utt2spk=None, cmvn_out=None):
    """mats: iterable of (utt, float32 (frames, D)) -> the ark, its scp and, with cmvn_out, the
    compute-cmvn-stats archive per speaker of utt2spk (per utterance without it).  Returns
    {utt: matrix} of what was written."""
    u2s = read_utt2spk(utt2spk) if utt2spk else None
    feats, by_spk = {}, {}
    open(ark_out, "wb").close()
    with open(scp_out, "w") as scp:
        for utt, m in mats:
            off = os.path.getsize(ark_out) + len(utt.encode("latin1")) + 1
            D.write_mat_path(ark_out, m, utt, append=True)
            scp.write("%s %s:%d\n" % (utt, ark_out, off))
            feats[utt] = m
            spk = utt if u2s is None else u2s.get(utt)
            if spk is not None:
                by_spk.setdefault(spk, []).append(m)
    if cmvn_out:
        write_stats_ark(cmvn_out, {spk: cmvn_stats(ms) for spk, ms in by_spk.items()})
    return feats


def write_feats(wav_lst, kf, ark_out, scp_out, utt2spk=None, cmvn_out=None):
    """Returns {utt: float32 (frames, D)} of what was written."""
    def mats():
        for utt, path in read_wav_list(wav_lst):
            s = kf.read(utt, path)
            if kf.n_frames(len(s)) > 0:
                yield utt, D.kaldi_features({utt: s}, kf).cpu().numpy()
    return write_matrices(mats(), ark_out, scp_out, utt2spk, cmvn_out)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m pkc.kaldi_feats",
                                 description=__doc__.split("\n")[0], allow_abbrev=False)
    ap.add_argument("--wav-lst", required=True)
    ap.add_argument("--config", help="Kaldi conf file of stage options")
    ap.add_argument("--type", required=True, choices=["fbank", "mfcc"])
    ap.add_argument("--ark-out", required=True)
    ap.add_argument("--scp-out", required=True)
    ap.add_argument("--utt2spk")
    ap.add_argument("--cmvn-out")
    a, rest = ap.parse_known_args(argv)
    kv = {"config": a.config} if a.config else {}
    for o in rest:
        if not o.startswith("--"):
            ap.error("unexpected argument %r" % o)
        k, _, v = o[2:].partition("=")
        kv[k.replace("_", "-")] = v
    write_feats(a.wav_lst, KaldiFeats.from_options("pkc-" + a.type, kv), a.ark_out, a.scp_out,
                a.utt2spk, a.cmvn_out)


if __name__ == "__main__":
    main()

"""python -m pkc.raw_fea — write the raw-waveform arks of the reference's save_raw_fea.py.

    python -m pkc.raw_fea --wav-lst L --out-folder D --scp-out F
                          [--sig-wlen 200 --lab-wlen 25 --lab-wshift 10 --fs 16000]

For every ``utt_id /path/file.wav`` line of L: ``D/<utt>.ark`` holding one matrix under the key
``<utt>`` (one row per 10 ms label frame, the 200 ms window around it) and the line
``<utt> D/<utt>.ark:<len(utt)+1>`` of F — what save_raw_fea.py:106-112 writes, which this fork of
the reference cannot run (it calls write_mat(out_file, frame_all, key=...) against a
data_io.write_mat(output_folder, file_or_fd, m, key)).  The rows are cut by the same kernel that
serves the ``pkc-wav-frames`` fea_opts stage and stored as float32 (``FM``): the float32 cast of
the script's float64 rows; the reference reads either matrix type.
"""
import argparse
import os

from . import data_io as D
from .frontend import WavFrames, read_wav_list


def write_raw_arks(wav_lst, out_folder, scp_out, wav):
    os.makedirs(out_folder, exist_ok=True)
    with open(scp_out, "w") as scp:
        for utt, path in read_wav_list(wav_lst):
            m = D.frame_signals({utt: wav.read(utt, path)}, wav).cpu().numpy()
            ark = out_folder + "/" + utt + ".ark"
            D.write_mat_path(ark, m, utt)
            scp.write("%s %s:%d\n" % (utt, ark, len(utt) + 1))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m pkc.raw_fea", description=__doc__.split("\n")[0])
    ap.add_argument("--wav-lst", required=True)
    ap.add_argument("--out-folder", required=True)
    ap.add_argument("--scp-out", required=True)
    ap.add_argument("--sig-wlen", type=int, default=200, help="signal window, ms")
    ap.add_argument("--lab-wlen", type=int, default=25, help="label window, ms")
    ap.add_argument("--lab-wshift", type=int, default=10, help="label shift, ms")
    ap.add_argument("--fs", type=int, default=16000, help="sampling rate, Hz")
    a = ap.parse_args(argv)
    write_raw_arks(a.wav_lst, a.out_folder, a.scp_out,
                   WavFrames(a.sig_wlen, a.lab_wlen, a.lab_wshift, a.fs))


if __name__ == "__main__":
    main()

"""python -m pkc.feat_pipe — run a native fea_opts pipe over a feature scp or a wav list and write
what it produces, without Kaldi.

    python -m pkc.feat_pipe --fea-lst F --fea-opts "<pipe>" --ark-out A --scp-out S
                            [--utt2spk U --cmvn-out C]

<pipe> is any fea_opts pipe pkc runs itself (pkc.frontend: pkc-fbank / pkc-mfcc / pkc-wav-frames
over a wav list F, apply-cmvn, add-deltas, splice-feats, transform-feats over a feature scp F), and
the rows come from the staging and the kernels the loader uses (pkc.data_io.stage_chunk).  For every
utterance the pipe writes — apply-cmvn drops those without statistics, transform-feats those
without a transform — one float32 (``FM``) matrix under its key in A and the line
``utt A:<offset>`` in S, in F's order.  With --cmvn-out, C is the ``compute-cmvn-stats`` archive of
the written features per speaker of U (per utterance without --utt2spk).

The use it was written for: a cfg that trains on fMLLR features ends its pipe in an apply-cmvn
over per-speaker statistics OF the fMLLR features.  Run the pipe up to the per-speaker transform
through this tool with --cmvn-out once, and point that last apply-cmvn at C.
"""
import argparse

import numpy as np
import torch

from . import core
from . import data_io as D
from .kaldi_feats import write_matrices


def pipe_matrices(fea_lst, fea_opts, device="cuda"):
    """[(utt, float32 (frames, Dout))] of the native pipe fea_opts over fea_lst, in its order."""
    from . import frontend as FE
    if not FE.is_native_pipe(fea_opts):
        raise NotImplementedError("fea_opts %r is not a pipe of native pkc stages" % fea_opts)
    fea, frontend = core._read_features(fea_lst, fea_opts, None)
    st = D.stage_chunk(fea, [], -1, device, frontend=frontend)       # unsplit: names are the keys
    torch.cuda.current_stream().wait_event(st.done)
    out = st.raw_d.cpu().numpy()
    beg = np.concatenate([[0], np.asarray(st.end_index)[:-1]])
    where = {k: (int(b), int(e)) for k, b, e in zip(st.names, beg, st.end_index)}
    return [(k, out[where[k][0]:where[k][1]]) for k in fea if k in where]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m pkc.feat_pipe", description=__doc__.split("\n")[0],
                                 allow_abbrev=False)
    ap.add_argument("--fea-lst", required=True, help="feature scp, or wav list for a pkc-* first stage")
    ap.add_argument("--fea-opts", required=True, help="the pipe, as in a cfg's fea_opts")
    ap.add_argument("--ark-out", required=True)
    ap.add_argument("--scp-out", required=True)
    ap.add_argument("--utt2spk")
    ap.add_argument("--cmvn-out")
    a = ap.parse_args(argv)
    write_matrices(pipe_matrices(a.fea_lst, a.fea_opts), a.ark_out, a.scp_out, a.utt2spk, a.cmvn_out)


if __name__ == "__main__":
    main()

"""What SyncBN over the recurrent gate BatchNorms costs per step (a record, not a threshold;
bench.py is the project's benchmark): the C4 layer shape (LSTM 4 x 1024 bidirectional, B = 16
sentences per rank, T U[150, 450], fp32, scripts/bench_seq.py) trained by TWO gloo ranks that share
ONE GPU, with sync_bn off and on, alternating in the same session.

What the number is: wall time per step (host clock between device synchronises and barriers, the
max over ranks) over the mean padded T and the layers, in us per time step and layer.  With
sync_bn on a step adds 2 x layers collectives ([R][G][3H] and [G][2H] floats) — through gloo,
which stages the device buffer through the host and synchronises the stream per collective.  That
is NOT the cost over RCCL / xGMI, which has never run here with more than one rank: not measured.

Both runs use the per-step launches (PKC_RNN_LSTM_PERSIST=0).  The grid-synchronised LSTM loops
spin on peers that must all be resident; two processes on one GPU take CUs from each other, and
the first attempt at this record with the loops on measured 14.7 s per step with sync_bn off and
5.1 s with it on — the loops waiting for each other, nothing about SyncBN.  On a node every rank
has its own GPU and keeps the loops.

Writes profiles/seq_syncbn_step.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-kaldi-cgs_amd"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)


def worker(a):
    import torch
    import torch.distributed as dist

    import bench_seq as BS
    from pkc import dist as DP
    dist.init_process_group("gloo")
    rank, world = DP.world()
    torch.cuda.set_device(0)
    sbn = DP.SyncBatchNorm() if a.worker == "on" else None
    ar = DP.GradAllReduce()
    r = BS.run(a.config, a.steps, a.warmup, allreduce=ar, rank=rank, world=world, sync_bn=sbn)
    r.update(sync_bn=a.worker, bn_collectives=0 if sbn is None else sbn.calls,
             grad_collectives=ar.calls, device=torch.cuda.get_device_name(0))
    if rank == 0:
        with open(a.out, "w") as f:
            json.dump(r, f)
    dist.destroy_process_group()


def commit():
    try:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
        return r.stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="off / on pairs, alternating")
    ap.add_argument("--commit", default=None, help="the commit measured (default: git HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_syncbn_step.json"))
    ap.add_argument("--worker", default=None, choices=["off", "on"])
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    runs = {"off": [], "on": []}
    # per-step launches: the grid-synchronised LSTM loops need every workgroup of a launch
    # co-resident, which two processes sharing one GPU take from each other (see the docstring)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2",
               PKC_RNN_LSTM_PERSIST="0")
    for k in range(a.rounds):
        for mode in ("off", "on"):
            tmp = a.out + ".%s%d.tmp" % (mode, k)
            cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run",
                   "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                   "--master-port", str(29500 + (os.getpid() + 2 * k + (mode == "on")) % 1000),
                   os.path.abspath(__file__), "--worker", mode, "--config", a.config, "--steps",
                   str(a.steps), "--warmup", str(a.warmup), "--out", tmp]
            r = subprocess.run(cmd, env=env)
            if r.returncode != 0:              # nothing more on the GPU after a failed launch
                sys.exit("sync_bn %s, round %d: exit %d" % (mode, k, r.returncode))
            with open(tmp) as f:
                runs[mode].append(json.load(f))
            os.remove(tmp)
            print(mode, k, runs[mode][-1]["us_per_time_step_per_layer_fwd_bwd"],
                  runs[mode][-1]["ms_per_step"], flush=True)

    def summary(rs):
        us = [r["us_per_time_step_per_layer_fwd_bwd"] for r in rs]
        ms = [r["ms_per_step"] for r in rs]
        return {"us_per_step_layer": {"median": statistics.median(us), "min": min(us), "max": max(us)},
                "ms_per_step": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)},
                "mean_T": [r["mean_T"] for r in rs],
                "bn_collectives_per_step": rs[0]["bn_collectives"] / (a.steps + a.warmup),
                "grad_collectives_per_step": rs[0]["grad_collectives"] / (a.steps + a.warmup)}

    off, on = summary(runs["off"]), summary(runs["on"])
    res = {"what": "two gloo ranks sharing ONE GPU, sync_bn off vs on, same session, alternating",
           "commit": a.commit or commit(), "device": runs["off"][0]["device"],
           "config": a.config, "shape": "LSTM 4x1024 bidirectional, B=16 sentences per rank, "
                                        "T U[150,450], fp32" if a.config == "c4" else a.config,
           "unit": "us per time step and layer (forward + backward + update, wall time per step "
                   "/ (mean padded T x layers))",
           "timing": "host clock between barriers, device synchronised on both sides, max over ranks",
           "steps": a.steps, "warmup": a.warmup, "runs_per_mode": a.rounds, "n_ranks": 2, "n_gpus": 1,
           "transport": "gloo (host-staged); RCCL / xGMI with more than one rank: not measured",
           "step_form": "per-step launches (PKC_RNN_LSTM_PERSIST=0: two processes on one GPU "
                        "cannot both keep the grid-synchronised loops resident)",
           "sync_bn_off": off, "sync_bn_on": on,
           "on_over_off": on["us_per_step_layer"]["median"] / off["us_per_step_layer"]["median"],
           "rec_forms": runs["on"][0]["rec_forms"]}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out, "off": off["us_per_step_layer"],
                      "on": on["us_per_step_layer"]}))


if __name__ == "__main__":
    main()

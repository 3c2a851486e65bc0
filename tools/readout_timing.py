"""What does the readout pass cost against the bytes it has to store?  (run on the GPU box)

    python tools/readout_timing.py [--n 4096] [--snaps 256] [--repeats 15] [--out profiles/readout_timing.txt]

Two cases on the handle's stream - the current state of N envs, and a stack of `snaps` snapshots of N envs - each with frames only and
with all four outputs.  The yardstick, timed in the same run and alternating with the pass, is a device-to-device copy of exactly the
number of bytes the pass stores (the pass also reads 232 bytes per env-state, 12 % of its stores at most; the copy reads as much as it
writes).  Times are medians over the repeats after warm-up, taken with events around `inner` back-to-back launches so that a window is
not a single few-microsecond kernel.  A record, not a gate."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jitterbug_amd import model
from jitterbug_amd.vec_env import JitterbugVecEnv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--snaps", type=int, default=256)
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
n, S = args.n, args.snaps
env = JitterbugVecEnv(n, "move_to_pose", seed=0)
stream = torch.cuda.ExternalStream(int(env.stream), device=dev)
g = torch.Generator(device=dev); g.manual_seed(0)
tape = torch.rand((20, n), generator=g, device=dev) * 2 - 1
snaps = torch.zeros((S, env.snapshot_bytes), device=dev, dtype=torch.uint8)
torch.cuda.synchronize()
env.reset_device()
env.step_many_device(20, tape.data_ptr())
for k in range(S):          # the stack: a short trajectory, repeated (what the pass reads does not change what it costs)
    if k < 8:
        env.step_many_device(1, tape[k].data_ptr())
    env.snapshot_device(snaps[k].data_ptr())
env.synchronize()
LEN = dict(frames=model.NFRAME * 12, clearance=model.NGEOM, body_vel=model.NBODY * 6, energy=8)


def timed(bodies, inner):
    """medians (ms per launch) of several bodies, alternated inside every repeat"""
    ms = [[] for _ in bodies]
    for i in range(args.warmup + args.repeats):
        for j, body in enumerate(bodies):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(inner):
                body()
            e1.record(stream)
            e1.synchronize()
            if i >= args.warmup:
                ms[j].append(e0.elapsed_time(e1) / inner)
    return [(float(np.median(m)), float(np.min(m)), float(np.max(m))) for m in ms]


lines = ["readout pass against a device-to-device copy of the bytes it stores; ms per launch: median (min .. max) over %d repeats" % args.repeats,
         "N = %d envs, kernel variant %s" % (n, env.kernel_variant)]
for label, n_snaps, inner in (("current state", 1, 200), ("stack of %d snapshots" % S, S, 5)):
    m = n * n_snaps
    for outs in (("frames",), ("frames", "clearance", "body_vel", "energy")):
        buf = {k: torch.zeros((m, LEN[k]), device=dev, dtype=torch.float32) for k in outs}
        nbytes = 4 * m * sum(LEN[k] for k in outs)
        src, dst = (torch.zeros(nbytes // 4, device=dev, dtype=torch.float32) for _ in range(2))
        torch.cuda.synchronize()
        ptr = [buf[k].data_ptr() if k in buf else None for k in ("frames", "clearance", "body_vel", "energy")]
        sp = None if n_snaps == 1 else snaps.data_ptr()

        def readout():
            env.readout_device(*ptr, snaps_ptr=sp, n_snaps=n_snaps)

        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(src, non_blocking=True)

        (r, rlo, rhi), (c, clo, chi) = timed([readout, copy], inner)
        lines.append("%-24s %-10s %8.1f MB stored: readout %.4f (%.4f .. %.4f)  copy %.4f (%.4f .. %.4f)  ratio %.2f  readout %.0f GB/s stored"
                     % (label, "frames" if len(outs) == 1 else "all four", nbytes / 1e6, r, rlo, rhi, c, clo, chi, r / c, nbytes / r / 1e6))
        del buf, src, dst
env.close()
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")

"""What does the readout pass cost against the bytes it has to store?  (run on the GPU box)

    python tools/readout_timing.py [--n 4096] [--snaps 256] [--repeats 15] [--out profiles/readout_timing.txt]

Two cases on the handle's stream - the current state of N envs, and a stack of `snaps` snapshots of N envs - each with frames only and
with all four outputs.  The yardstick, timed in the same run and alternating with the pass, is a device-to-device copy of exactly the
number of bytes the pass stores (the pass also reads 232 bytes per env-state, 12 % of its stores at most; the copy reads as much as it
writes).  Times are medians over the repeats after warm-up, taken with events around `inner` back-to-back launches so that a window is
not a single few-microsecond kernel.  A record, not a gate."""
import argparse

import pass_timing as pt

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--snaps", type=int, default=256)
args = pt.arguments(ap)

import torch

from jitterbug_amd import model

dev = torch.device("cuda", 0)
n, S = args.n, args.snaps
env, stream, _, snaps, _ = pt.prepared(n, S)          # (what the pass reads does not change what it costs)
LEN = dict(frames=model.NFRAME * 12, clearance=model.NGEOM, body_vel=model.NBODY * 6, energy=8)

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

        (r, rlo, rhi), (c, clo, chi) = pt.timed(args, stream, [readout, copy], inner)
        lines.append("%-24s %-10s %8.1f MB stored: readout %.4f (%.4f .. %.4f)  copy %.4f (%.4f .. %.4f)  ratio %.2f  readout %.0f GB/s stored"
                     % (label, "frames" if len(outs) == 1 else "all four", nbytes / 1e6, r, rlo, rhi, c, clo, chi, r / c, nbytes / r / 1e6))
        del buf, src, dst
env.close()
pt.report(args, lines)

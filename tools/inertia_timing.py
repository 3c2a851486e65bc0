"""What does the inertia pass cost per env-state, against a readout of the same states?  (run on the GPU box)

    python tools/inertia_timing.py [--parent-lib PATH/libjitterbug_hip.so] [--repeats 15] [--out profiles/inertia_timing.txt]

The pass (jb_inertia_device) with all four outputs and with qM + qfrc only, at 4096 and at 65 536 env-states, each as the current state of
that many envs and as a stack of 4 snapshots of a quarter as many, in microseconds per env-state and as achieved store bandwidth (the
full pass writes 6180 bytes per env-state, qM + qfrc 1080; the readout 1944).  The yardstick is a readout with all four outputs over the
same env-states prepared the same way, measured in a child process of its own on the library named by --parent-lib (the build of the
parent commit: JITTERBUG_HIP_LIB; without it, this tree's library, and the report says so).  Times are medians over the repeats after
warm-up, taken with events around `inner` back-to-back launches.  A record, not a gate."""
import argparse
import json
import sys

import pass_timing as pt

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--readout-only", default=None, help="(the child process) N,n_snaps: time readouts with all four outputs over n_snaps snapshots of N envs (1: the current state) and print one JSON line")
args = pt.arguments(ap)

import torch

from jitterbug_amd import model

dev = torch.device("cuda", 0)
NV, NJAC = model.NV, len(model.BODY_NAMES) + model.NLEG
BYTES = dict(qM=4 * NV * NV, qfrc=4 * 3 * NV, qacc_smooth=4 * NV, jac=4 * NJAC * 6 * NV)
RO_BYTES = 4 * (model.NFRAME * 12 + model.NGEOM + model.NBODY * 6 + 8)


def stack_of(snaps, n_snaps):
    """the stack's pointer, or None for the current state (a stack of one would be the same launch on other memory)"""
    return None if n_snaps == 1 else snaps.data_ptr()


if args.readout_only:
    n, n_snaps = (int(x) for x in args.readout_only.split(","))
    env, stream, _, snaps, _ = pt.prepared(n, n_snaps)
    m = n_snaps * n
    out = [torch.zeros((m, w), device=dev, dtype=torch.float32) for w in (model.NFRAME * 12, model.NGEOM, model.NBODY * 6, 8)]
    torch.cuda.synchronize()
    (med, lo, hi), = pt.timed(args, stream, [lambda: env.readout_device(*[o.data_ptr() for o in out], snaps_ptr=stack_of(snaps, n_snaps), n_snaps=n_snaps)], 20 if m <= 4096 else 5)
    print(json.dumps(dict(m=m, ms=med, lo=lo, hi=hi)))
    env.close()
    sys.exit(0)

lines = ["inertia pass against a readout (all four outputs) of %s on the same states; median (min .. max) over %d repeats" % (pt.whose(args.parent_lib), args.repeats),
         "bytes stored per env-state: inertia, all four %d, qM + qfrc %d; readout %d" % (sum(BYTES.values()), BYTES["qM"] + BYTES["qfrc"], RO_BYTES)]
for m in (4096, 65536):
    for n_snaps in (1, 4):
        n = m // n_snaps
        ro = pt.child(__file__, args, "--readout-only", "%d,%d" % (n, n_snaps))
        env, stream, _, snaps, ctrl = pt.prepared(n, n_snaps)
        for keys in (("qM", "qfrc", "qacc_smooth", "jac"), ("qM", "qfrc")):
            t = {k: torch.zeros((m * BYTES[k] // 4,), device=dev, dtype=torch.float32) for k in keys}
            torch.cuda.synchronize()
            ptr = [t[k].data_ptr() if k in t else None for k in ("qM", "qfrc", "qacc_smooth", "jac")]
            (med, lo, hi), = pt.timed(args, stream, [lambda: env.inertia_device(ctrl.data_ptr(), *ptr, snaps_ptr=stack_of(snaps, n_snaps), n_snaps=n_snaps)], 20 if m <= 4096 else 5)
            stored = m * sum(BYTES[k] for k in keys)
            lines.append("%6d env-states (%d x %5d)  %-10s inertia %.4f ms (%.4f .. %.4f) = %.4f us per env-state, %.0f GB/s stored;  readout %.4f ms (%.4f .. %.4f) = %.4f us per env-state, %.0f GB/s;  ratio %.2f"
                         % (m, n_snaps, n, "all four" if len(keys) == 4 else "qM + qfrc", med, lo, hi, 1e3 * med / m, stored / med / 1e6, ro["ms"], ro["lo"], ro["hi"], 1e3 * ro["ms"] / m,
                            m * RO_BYTES / ro["ms"] / 1e6, med / ro["ms"]))
            del t
        env.close()
pt.report(args, lines)

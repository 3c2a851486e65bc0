"""What does the forward-dynamics pass cost per env-state, against one substep's share of a step launch?  (run on the GPU box)

    python tools/forward_timing.py [--parent-lib PATH/libjitterbug_hip.so] [--repeats 15] [--out profiles/forward_timing.txt]

The pass (jb_forward_device: one substep on a copy of the state, then inverse dynamics) at 4096 env-states - the current state of 4096
envs - and at 65 536 - a stack of 16 snapshots of them -, with qacc + qfrc and with all five outputs, in microseconds per env-state.  The
yardstick is a single-step launch of the same number of envs divided by its 50 substeps, measured in a child process of its own on the
library named by --parent-lib (the build of the parent commit: JITTERBUG_HIP_LIB; without it, this tree's library, and the report says
so).  Times are medians over the repeats after warm-up, taken with events around `inner` back-to-back launches.  A record, not a gate:
a pass stages the constant tables and loads the state for ONE substep where a step launch does so for fifty."""
import argparse
import json
import sys

import pass_timing as pt

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--step-only", type=int, default=0, help="(the child process) time single-step launches of this many envs and print one JSON line")
args = pt.arguments(ap)

import torch

dev = torch.device("cuda", 0)

if args.step_only:
    env, stream, tape, _, _ = pt.prepared(args.step_only, 0)
    k = [0]

    def step():
        env.step_many_device(1, tape[20 + k[0] % 4].data_ptr())
        k[0] += 1
    (med, lo, hi), = pt.timed(args, stream, [step], 20)
    print(json.dumps(dict(n=args.step_only, ms=med, lo=lo, hi=hi, variant=env.kernel_variant, substeps=env.substeps)))
    env.close()
    sys.exit(0)

SIZES = ((4096, 1), (4096, 16))
steps = {m: pt.child(__file__, args, "--step-only", m) for m in sorted(set(n * s for n, s in SIZES))}

lines = ["forward pass against one substep's share of a single-step launch (%s); median (min .. max) over %d repeats"
         % (pt.whose(args.parent_lib), args.repeats)]
env, stream, tape, _, _ = pt.prepared(4096, 0)
lines.append("N = 4096 envs, step kernel variant %s" % env.kernel_variant)
for n, n_snaps in SIZES:
    m = n * n_snaps
    ctrl = (torch.rand((m,), device=dev) * 2 - 1).contiguous()
    snaps = pt.snapshots(env, tape, n_snaps)
    s = steps[m]
    sub_us = 1e3 * s["ms"] / s["substeps"] / m
    for outs in (("qacc", "qfrc"), ("qacc", "qfrc", "body_acc", "motor", "unconverged")):
        LEN = dict(qacc=15, qfrc=15, body_acc=60, motor=3)
        buf = {k_: torch.zeros((m, LEN[k_]), device=dev, dtype=torch.float32) for k_ in outs if k_ in LEN}
        un = torch.zeros((m,), device=dev, dtype=torch.uint8) if "unconverged" in outs else None
        torch.cuda.synchronize()
        ptr = [buf[k_].data_ptr() if k_ in buf else None for k_ in ("qacc", "qfrc", "body_acc", "motor")]

        def forward():
            env.forward_device(ctrl.data_ptr(), *ptr, unconverged_ptr=None if un is None else un.data_ptr(), snaps_ptr=snaps.data_ptr(), n_snaps=n_snaps)
        (med, lo, hi), = pt.timed(args, stream, [forward], 20 if m <= 4096 else 3)
        lines.append("%6d env-states (%2d x %d)  %-11s forward %.4f ms (%.4f .. %.4f) = %.4f us per env-state;  step of %d envs (%s) %.4f ms / %d substeps = %.4f us per env-substep;  ratio %.2f"
                     % (m, n_snaps, n, "qacc + qfrc" if len(outs) == 2 else "all five", med, lo, hi, 1e3 * med / m, m, s["variant"], s["ms"], s["substeps"], sub_us, 1e3 * med / m / sub_us))
        del buf
env.close()
pt.report(args, lines)

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
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--step-only", type=int, default=0, help="(the child process) time single-step launches of this many envs and print one JSON line")
args = ap.parse_args()

import torch

from jitterbug_amd.vec_env import JitterbugVecEnv

dev = torch.device("cuda", 0)


def timed(env, stream, body, inner):
    ms = []
    for i in range(args.warmup + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(inner):
            body()
        e1.record(stream)
        e1.synchronize()
        if i >= args.warmup:
            ms.append(e0.elapsed_time(e1) / inner)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def prepared(n):
    """an env of n robots 20 control steps into an episode under random actions, its stream, and an action tape"""
    env = JitterbugVecEnv(n, "move_to_pose", seed=0)
    stream = torch.cuda.ExternalStream(int(env.stream), device=dev)
    g = torch.Generator(device=dev); g.manual_seed(0)
    tape = torch.rand((24, n), generator=g, device=dev) * 2 - 1
    torch.cuda.synchronize()
    env.reset_device()
    env.step_many_device(20, tape.data_ptr())
    env.synchronize()
    return env, stream, tape


if args.step_only:
    env, stream, tape = prepared(args.step_only)
    k = [0]

    def step():
        env.step_many_device(1, tape[20 + k[0] % 4].data_ptr())
        k[0] += 1
    med, lo, hi = timed(env, stream, step, 20)
    print(json.dumps(dict(n=args.step_only, ms=med, lo=lo, hi=hi, variant=env.kernel_variant, substeps=env.substeps)))
    env.close()
    sys.exit(0)

SIZES = ((4096, 1), (4096, 16))
child_env = dict(os.environ)
if args.parent_lib:
    child_env["JITTERBUG_HIP_LIB"] = os.path.abspath(args.parent_lib)
steps = {}
for n in sorted(set(n * s for n, s in SIZES)):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-only", str(n), "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                         env=child_env, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    steps[n] = json.loads(out.strip().splitlines()[-1])

lines = ["forward pass against one substep's share of a single-step launch (%s); median (min .. max) over %d repeats"
         % ("the parent commit's library" if args.parent_lib else "THIS tree's library: no --parent-lib given", args.repeats)]
env, stream, tape = prepared(4096)
lines.append("N = 4096 envs, step kernel variant %s" % env.kernel_variant)
for n, n_snaps in SIZES:
    m = n * n_snaps
    snaps = torch.zeros((n_snaps, env.snapshot_bytes), device=dev, dtype=torch.uint8)
    ctrl = (torch.rand((m,), device=dev) * 2 - 1).contiguous()
    torch.cuda.synchronize()
    for k in range(n_snaps):
        env.step_many_device(1, tape[20 + k % 4].data_ptr())
        env.snapshot_device(snaps[k].data_ptr())
    env.synchronize()
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
        med, lo, hi = timed(env, stream, forward, 20 if m <= 4096 else 3)
        lines.append("%6d env-states (%2d x %d)  %-11s forward %.4f ms (%.4f .. %.4f) = %.4f us per env-state;  step of %d envs (%s) %.4f ms / %d substeps = %.4f us per env-substep;  ratio %.2f"
                     % (m, n_snaps, n, "qacc + qfrc" if len(outs) == 2 else "all five", med, lo, hi, 1e3 * med / m, m, s["variant"], s["ms"], s["substeps"], sub_us, 1e3 * med / m / sub_us))
        del buf
env.close()
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")

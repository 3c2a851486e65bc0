"""What does the contact pass cost per env-state, against a forward pass on the same states?  (run on the GPU box)

    python tools/contacts_timing.py [--parent-lib PATH/libjitterbug_hip.so] [--repeats 15] [--out profiles/contacts_timing.txt]

The pass (jb_contacts_device: one substep on a copy of the state, then the per-slot evaluation) at 4096 env-states - the current state of
4096 envs - and at 65 536 - a stack of 16 snapshots of them -, with geom_frc only and with all four outputs, in microseconds per
env-state.  The yardstick is a forward pass (qacc + qfrc) over the same number of env-states prepared the same way, measured in a child
process of its own on the library named by --parent-lib (the build of the parent commit: JITTERBUG_HIP_LIB; without it, this tree's
library, and the report says so).  Times are medians over the repeats after warm-up, taken with events around `inner` back-to-back
launches.  A record, not a gate."""
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
ap.add_argument("--forward-only", type=int, default=0, help="(the child process) time forward passes over this many snapshots of 4096 envs and print one JSON line")
args = ap.parse_args()

import torch

from jitterbug_amd import model
from jitterbug_amd.vec_env import JitterbugVecEnv

dev = torch.device("cuda", 0)
N = 4096


def timed(stream, body, inner):
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


def prepared(n_snaps):
    """N robots 20 control steps into an episode under random actions, a stack of n_snaps snapshots of the steps that follow, actions for it"""
    env = JitterbugVecEnv(N, "move_to_pose", seed=0)
    stream = torch.cuda.ExternalStream(int(env.stream), device=dev)
    g = torch.Generator(device=dev); g.manual_seed(0)
    tape = torch.rand((24, N), generator=g, device=dev) * 2 - 1
    snaps = torch.zeros((n_snaps, env.snapshot_bytes), device=dev, dtype=torch.uint8)
    ctrl = (torch.rand((n_snaps * N,), generator=g, device=dev) * 2 - 1).contiguous()
    torch.cuda.synchronize()
    env.reset_device()
    env.step_many_device(20, tape.data_ptr())
    for k in range(n_snaps):
        env.step_many_device(1, tape[20 + k % 4].data_ptr())
        env.snapshot_device(snaps[k].data_ptr())
    env.synchronize()
    return env, stream, snaps, ctrl


if args.forward_only:
    n_snaps = args.forward_only
    env, stream, snaps, ctrl = prepared(n_snaps)
    m = n_snaps * N
    qacc, qfrc = (torch.zeros((m, model.NV), device=dev, dtype=torch.float32) for _ in range(2))
    torch.cuda.synchronize()
    med, lo, hi = timed(stream, lambda: env.forward_device(ctrl.data_ptr(), qacc.data_ptr(), qfrc.data_ptr(), snaps_ptr=snaps.data_ptr(), n_snaps=n_snaps), 20 if n_snaps == 1 else 3)
    print(json.dumps(dict(m=m, ms=med, lo=lo, hi=hi, variant=env.kernel_variant)))
    env.close()
    sys.exit(0)

child_env = dict(os.environ)
if args.parent_lib:
    child_env["JITTERBUG_HIP_LIB"] = os.path.abspath(args.parent_lib)
lines = ["contact pass against a forward pass (qacc + qfrc) of %s on the same states; median (min .. max) over %d repeats"
         % ("the parent commit's library" if args.parent_lib else "THIS tree's library: no --parent-lib given", args.repeats)]
for n_snaps in (1, 16):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--forward-only", str(n_snaps), "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                         env=child_env, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    fw = json.loads(out.strip().splitlines()[-1])
    env, stream, snaps, ctrl = prepared(n_snaps)
    m = n_snaps * N
    if n_snaps == 1:
        lines.append("N = %d envs, step kernel variant %s" % (N, env.kernel_variant))
    for all_outputs in (False, True):
        gf = torch.zeros((m, model.NGEOM, 3), device=dev, dtype=torch.float32)
        table = torch.zeros((m, model.NCONTACT, model.CONTACT_WIDTH), device=dev, dtype=torch.float32) if all_outputs else None
        ncon = torch.zeros((m,), device=dev, dtype=torch.int32) if all_outputs else None
        un = torch.zeros((m,), device=dev, dtype=torch.uint8) if all_outputs else None
        torch.cuda.synchronize()

        def contacts():
            env.contacts_device(ctrl.data_ptr(), None if table is None else table.data_ptr(), None if ncon is None else ncon.data_ptr(), gf.data_ptr(),
                                None if un is None else un.data_ptr(), snaps_ptr=snaps.data_ptr(), n_snaps=n_snaps)
        med, lo, hi = timed(stream, contacts, 20 if n_snaps == 1 else 3)
        lines.append("%6d env-states (%2d x %d)  %-13s contacts %.4f ms (%.4f .. %.4f) = %.4f us per env-state;  forward %.4f ms (%.4f .. %.4f) = %.4f us per env-state;  ratio %.2f;  mean ncon %s"
                     % (m, n_snaps, N, "all four" if all_outputs else "geom_frc only", med, lo, hi, 1e3 * med / m, fw["ms"], fw["lo"], fw["hi"], 1e3 * fw["ms"] / m, med / fw["ms"],
                        "%.2f" % ncon.float().mean().item() if ncon is not None else "-"))
        del gf, table, ncon, un
    env.close()
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")

"""What tools/readout_timing.py, forward_timing.py and contacts_timing.py share: the prepared batch, the timing loop, the yardstick measured
in a child process on the parent commit's library, and the report.  (imported by them; run on the GPU box)

Times are medians over the repeats after warm-up, taken with events around `inner` back-to-back launches so that a window is not a single
few-microsecond kernel."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arguments(ap):
    """the options every tool has, on top of the ones it added to `ap` itself"""
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def timed(args, stream, bodies, inner):
    """(median, min, max) in ms per launch of each of `bodies`, alternated inside every repeat"""
    import torch
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


def snapshots(env, tape, n_snaps):
    """a stack of n_snaps snapshots of the steps that follow the env's state (actions: the tape's last four rows in turn)"""
    import torch
    snaps = torch.zeros((n_snaps, env.snapshot_bytes), device=tape.device, dtype=torch.uint8)
    torch.cuda.synchronize()
    for k in range(n_snaps):
        env.step_many_device(1, tape[20 + k % 4].data_ptr())
        env.snapshot_device(snaps[k].data_ptr())
    env.synchronize()
    return snaps


def prepared(n, n_snaps):
    """n robots 20 control steps into an episode under random actions: the env, its stream, the action tape, snapshots(n_snaps) and an
    action for every env-state of them"""
    import torch

    from jitterbug_amd.vec_env import JitterbugVecEnv
    dev = torch.device("cuda", 0)
    env = JitterbugVecEnv(n, "move_to_pose", seed=0)
    stream = torch.cuda.ExternalStream(int(env.stream), device=dev)
    g = torch.Generator(device=dev); g.manual_seed(0)
    tape = torch.rand((24, n), generator=g, device=dev) * 2 - 1
    ctrl = (torch.rand((n_snaps * n,), generator=g, device=dev) * 2 - 1).contiguous()
    torch.cuda.synchronize()
    env.reset_device()
    env.step_many_device(20, tape.data_ptr())
    return env, stream, tape, snapshots(env, tape, n_snaps), ctrl


def whose(parent_lib):
    return "the parent commit's library" if parent_lib else "THIS tree's library: no --parent-lib given"


def child(script, args, option, value):
    """The yardstick: `script option value` in a process of its own on the library named by --parent-lib (the build of the parent commit:
    JITTERBUG_HIP_LIB; without it, this tree's library); the JSON object of its last output line."""
    env = dict(os.environ)
    if args.parent_lib:
        env["JITTERBUG_HIP_LIB"] = os.path.abspath(args.parent_lib)
    out = subprocess.run([sys.executable, os.path.abspath(script), option, str(value), "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                         env=env, stdout=subprocess.PIPE, check=True, timeout=600).stdout.decode()
    return json.loads(out.strip().splitlines()[-1])


def report(args, lines):
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")

"""What does a planner iteration cost on top of the rollout it has to do anyway?  (run on the GPU box)

    python tools/plan_timing.py [--n 4096] [--k 20] [--repeats 15] [--only-a] [--baseline-json A.json] [--out profiles/plan_timing.json]

  (a) step_many_device(K, rewards)                         the fused K-step rollout alone
  (b) restore_device(fork map) + score_tapes_device(K)     one planner iteration: fork, the same rollout, the return kernel

Both start from the same forked state in every repeat (for (a) the restore sits in front of the timed region), so the step kernel does
the same work; times are medians over the repeats after warm-up, taken with events on the handle's stream.  (a) is code this feature
did not touch: --only-a with JITTERBUG_HIP_LIB pointing at a build of the parent commit measures it there (from a set_state of the same
forked positions: that build has no exact restore; the in-tree build reports this variant too), and --baseline-json feeds that
measurement into the criterion:   (b) <= (a) + (a)'s min-to-max spread + 1 %."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jitterbug_amd.vec_env import JitterbugVecEnv

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--group", type=int, default=64)
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only-a", action="store_true")
ap.add_argument("--baseline-json", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.repeats >= 10

dev = torch.device("cuda", 0)
n, K, M = args.n, args.k, args.group
env = JitterbugVecEnv(n, "move_from_origin", seed=0)
stream = torch.cuda.ExternalStream(int(env.stream), device=dev)
g = torch.Generator(device=dev); g.manual_seed(0)
warm = torch.rand((50, n), generator=g, device=dev) * 2 - 1
tapes = torch.rand((K, n), generator=g, device=dev) * 2 - 1
rew = torch.zeros((K, n), device=dev)
ret = torch.zeros(n, device=dev)
torch.cuda.synchronize()
env.reset_device()
env.step_many_device(50, warm.data_ptr())
env.synchronize()
have_snapshot = hasattr(env, "snapshot_device") and hasattr(env._L, "jb_snapshot_device")
# the way back a library from before the feature has: the old surface (same positions, cold solver start) - good enough to time (a), and
# the same on both builds
q, v, t = env.get_state()
grp = M * (np.arange(n) // M)
q, v, t = q[grp], v[grp], t[grp]
go_back_set_state = lambda: env.set_state(q, v, t)
if have_snapshot:
    snap = torch.zeros(env.snapshot_bytes, device=dev, dtype=torch.uint8)
    src = torch.from_numpy(grp.astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    env.snapshot_device(snap.data_ptr())
    go_back = lambda: env.restore_device(snap.data_ptr(), n_src=n, src_ptr=src.data_ptr())

def timed(body, before=None):
    ms = []
    for i in range(args.warmup + args.repeats):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        body()
        e1.record(stream)
        e1.synchronize()
        if i >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), spread_ms=float(ms.max() - ms.min()), repeats=len(ms))


out = dict(n_envs=n, k_steps=K, group=M, kernel_variant=env.kernel_variant, library="JITTERBUG_HIP_LIB" if os.environ.get("JITTERBUG_HIP_LIB") else "in-tree")
rollout = lambda: env.step_many_device(K, tapes.data_ptr(), rewards_ptr=rew.data_ptr())
out["a_step_many_after_set_state"] = timed(rollout, before=go_back_set_state)
if have_snapshot:
    out["a_step_many"] = timed(rollout, before=go_back)
if not args.only_a and have_snapshot:
    def iteration():
        env.restore_device(snap.data_ptr(), n_src=n, src_ptr=src.data_ptr())
        env.score_tapes_device(K, tapes.data_ptr(), 1.0, ret.data_ptr())
    out["b_restore_and_score"] = timed(iteration)
    out["fork_alone"] = timed(go_back)
    base = out["a_step_many"]
    if args.baseline_json:
        out["a_step_many_parent_build"] = json.load(open(args.baseline_json))["a_step_many_after_set_state"]
        base = out["a_step_many_parent_build"]
    limit = base["median_ms"] + base["spread_ms"] + 0.01 * base["median_ms"]
    out["criterion"] = dict(limit_ms=limit, b_median_ms=out["b_restore_and_score"]["median_ms"], met=bool(out["b_restore_and_score"]["median_ms"] <= limit),
                            rule="(b) <= (a) + (a)'s min-to-max spread + 1 %, (a) measured on the parent commit's build when given")
env.close()
text = json.dumps(out, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")

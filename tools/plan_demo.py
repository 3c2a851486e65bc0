"""MPPI on the simulator as its own model, against the reference's heuristic policy, from the same start (run on the GPU box).

    python tools/plan_demo.py [--plants 4] [--candidates 256] [--horizon 20] [--steps 100] [--out FILE.json]

A `move_from_origin` episode prefix of --steps control steps for --plants robots: once with every action chosen by
jitterbug_amd.planning.MPPIPlanner (per step: snapshot the plant, fork it into plants x candidates model lanes, score the candidate
tapes, softmax update, apply the first action), once with the task's heuristic policy, both from one snapshot of the start.  Prints the
mean return of the prefix under each and the planner's decisions per second (one decision = one plan() for all plants)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from jitterbug_amd.planning import MPPIPlanner
from jitterbug_amd.vec_env import JitterbugVecEnv

ap = argparse.ArgumentParser()
ap.add_argument("--plants", type=int, default=4)
ap.add_argument("--candidates", type=int, default=256)
ap.add_argument("--horizon", type=int, default=20)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--temperature", type=float, default=0.02)
ap.add_argument("--sigma", type=float, default=0.5)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
G, T = args.plants, args.steps
plant = JitterbugVecEnv(G, "move_from_origin", seed=args.seed, envs_per_wave=4)
planner = MPPIPlanner("move_from_origin", n_groups=G, n_candidates=args.candidates, horizon=args.horizon, gamma=1.0, temperature=args.temperature,
                      noise_sigma=args.sigma, seed=args.seed, envs_per_wave=4)
start = torch.zeros(plant.snapshot_bytes, device=dev, dtype=torch.uint8)
snap = torch.zeros(plant.snapshot_bytes, device=dev, dtype=torch.uint8)
rew = torch.zeros((T, G), device=dev)
obs = torch.zeros((G, plant.obs_dim), device=dev); done = torch.zeros(G, device=dev, dtype=torch.uint8)
torch.cuda.synchronize()
plant.reset_device()
plant.snapshot_device(start.data_ptr())
plant.synchronize()

# the heuristic policy, evaluated in the step kernel
plant.step_many_device(T, None, rewards_ptr=rew.data_ptr())
plant.synchronize()
ret_heuristic = rew.sum(dim=0).cpu().numpy()

plant.restore_device(start.data_ptr())
plant.synchronize()
t0 = time.perf_counter()
for k in range(T):
    plant.snapshot_device(snap.data_ptr())
    plant.synchronize()
    action = planner.plan(snap.data_ptr())
    torch.cuda.synchronize()
    plant.step_device(action.data_ptr(), obs.data_ptr(), rew[k].data_ptr(), done.data_ptr())
plant.synchronize()
dt = time.perf_counter() - t0
ret_mppi = rew.sum(dim=0).cpu().numpy()
out = dict(task="move_from_origin", plants=G, candidates=args.candidates, horizon=args.horizon, steps=T, temperature=args.temperature, noise_sigma=args.sigma,
           return_heuristic_mean=float(ret_heuristic.mean()), return_mppi_mean=float(ret_mppi.mean()),
           return_heuristic=[float(x) for x in ret_heuristic], return_mppi=[float(x) for x in ret_mppi],
           decisions_per_second=T / dt, model_env_steps_per_second=T * G * args.candidates * args.horizon / dt)
print("move_from_origin, %d plants, first %d steps: return under the heuristic policy %.3f, under MPPI (%d candidates x %d steps) %.3f; %.1f decisions/s" %
      (G, T, out["return_heuristic_mean"], args.candidates, args.horizon, out["return_mppi_mean"], out["decisions_per_second"]))
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(json.dumps(out, indent=1) + "\n")
plant.close(); planner.close()

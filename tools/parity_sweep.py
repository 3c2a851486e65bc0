"""A wider run of the SURVEY 8(d) parity protocol than the test suite affords: teacher-forced (the oracle's state copied into the GPU env every
control step), N envs x 1000 control steps, every task, several seeds; ordinary and LEAN kernels; tipped-over regime; and the per-env-model
kernels PAIR and LEAN + PAIR on augmented_params (N envs x 1000 steps x seeds) and on the mass-touching and thread-touching models of the
tests (64 envs, uniform actions and motor flat out after a lead-in).  Prints what the protocol (tests/parity_protocol.py) asserts on, for the record
(profiles/r07_parity_sweep.txt).   python tools/parity_sweep.py [n_envs] [n_seeds] [blocks: any of ordinary,lean,pair,lean_pair]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.parity_inputs import mass_touching_models, thread_touching_models, tiled
from tests.parity_protocol import teacher_forced, MARGIN_TOL
from jitterbug_amd import model
n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
seeds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
blocks = sys.argv[3].split(",") if len(sys.argv) > 3 else ["ordinary", "lean", "pair", "lean_pair"]
t0 = time.time()
held = []          # worst_reward_held of every line: tests/parity_protocol.py REWARD_HELD_CAP is twice the largest


def rewards(r):
    """the reward columns: env-steps whose reward leaves the derived bound around oracle.reward of the GPU's own state (must be 0), the worst
    such difference and its share of the bound; the worst difference to the ORACLE'S step on env-steps that are not near a switch"""
    held.append(r["worst_reward_held"])
    return " | rewards: outside the derived bound %d (worst %.1e, %.2f of the bound), held against the oracle's step: worst %.2e" % (r["reward_bad"], r["worst_reward_own"], r["worst_reward_ratio"], r["worst_reward_held"])


print("# teacher-forced parity, %d envs x 1000 control steps per (task, seed): entries outside 1e-4 rel + 1e-6 abs on WELL-conditioned env-steps (oracle contact-switch margin >= MARGIN_TOL = %.0f nm) [of those outside 1e-4 rel + 1e-5 abs: must be 0] / worst error there / share of ill-conditioned env-steps / share of ALL entries within tolerance / rewards within tolerance / Newton cap hits / excluded env-steps: worst error, cascade check (next step from the GPU's own state: checked, bad)" % (n, MARGIN_TOL * 1e9))
for flags, name in ((0, "ordinary kernel"), (2, "LEAN kernel")):
    if ("lean" if flags else "ordinary") not in blocks:
        continue
    for task in model.TASKS:
        for sd in range(seeds):
            r = teacher_forced(task, n, 1000, seed=100 + 10 * model.TASKS.index(task) + sd, flags=flags)
            print("%-16s %-18s seed %3d : well-conditioned bad %d [strict %d] (worst %.1e, any > 1e-2: %d) | ill-conditioned env-steps %.5f | all entries %.6f | rewards %.6f | cap hits %.0f | excluded: worst %.1e, cascade %d checked %d bad | largest margin of a flipped env-step %.1f nm | deep env-steps %d"
                  % (name, task, 100 + 10 * model.TASKS.index(task) + sd, r["well_bad"], r["strict_bad"], r["worst_well"], r["well_big"], r["ill_frac"], r["frac"], r["frac_reward"], r["cap"], r["worst_ill"], r["cascade_checked"], r["cascade_bad"], r["flip_margin_max"] * 1e9, r["deep_steps"]) + rewards(r))
            sys.stdout.flush()
        if flags:
            break           # LEAN: one task is enough here (the suite checks it at 8192 envs too)
if "ordinary" in blocks:
    r = teacher_forced("move_to_pose", n, 300, seed=55, flat_out=True, skip=250)
    print("tipped regime (motor flat out, 250 lead-in steps, 300 compared): tipped %.2f | well-conditioned bad %d [strict %d] (worst %.1e) | ill %.5f | all entries %.6f | cap hits %.0f | excluded: worst %.1e, bad env-steps %d, cascade %d checked %d bad"
          % (r["tipped"], r["well_bad"], r["strict_bad"], r["worst_well"], r["ill_frac"], r["frac"], r["cap"], r["worst_ill"], r["ill_bad_steps"], r["cascade_checked"], r["cascade_bad"]) + rewards(r))
    sys.stdout.flush()


def pair_line(name, what, r):
    """the three classes of tests/parity_protocol.py: well | deep (narrow phase converged / unconverged) | near-switch"""
    print("%-9s %-46s: well bad %d [strict %d] (worst %.1e, any > 1e-2: %d) | deep %d env-steps (%.2f %%): bad %d, converged narrow phase [strict %d] (worst %.1e), unconverged %d env-steps [strict %d] (worst %.1e) | near-switch %.5f: worst %.1e, bad env-steps %d, cascade %d checked %d bad | largest switch margin of an env-step outside the strict tolerance, deep or not (flip_margin_max) %.1f nm | unconverged well env-steps %d | all entries %.6f | cap hits %.0f | tipped %.2f | kernel %s"
          % (name, what, r["well_bad"], r["strict_bad"], r["worst_well"], r["well_big"], r["deep_steps"], 100.0 * r["deep_steps"] / r["env_steps"], r["deep_bad"], r["deep_strict_bad"] - r["clamped_strict_bad"], r["worst_deep_converged"],
             r["clamped_steps"], r["clamped_strict_bad"], r["worst_clamped"], r["ill_frac"], r["worst_ill"], r["ill_bad_steps"], r["cascade_checked"], r["cascade_bad"], r["flip_margin_max"] * 1e9, r["unconverged_well"], r["frac"], r["cap"], r["tipped"], r["kernel_variant"]) + rewards(r))
    sys.stdout.flush()


if "pair" in blocks or "lean_pair" in blocks:
    from jitterbug_amd import augmented_jitterbug as aj
    mass, thread = tiled(mass_touching_models(), 64), tiled(thread_touching_models(16, seed=11), 64)
    print("# one model per env: PAIR and LEAN + PAIR kernels.  Classes: well (switch margin >= MARGIN_TOL, not deep) | deep (a pair overlap beyond the leg's radius), split by whether the oracle's fixed-count narrow phase converged | near-switch (switch margin < MARGIN_TOL)")
    for flags, name in ((0, "PAIR"), (2, "LEAN+PAIR")):
        if ("lean_pair" if flags else "pair") not in blocks:
            continue
        # (model seed 5 / env seed 6: the robots of tests/test_gpu_parity.py::test_per_env_randomised_models, two of which reach the multiplier's clamp)
        for msd, sd in [(50 + k, 200 + k) for k in range(seeds)] + [(5, 6)]:
            r = teacher_forced("move_to_pose", n, 1000, seed=sd, params=aj.augmented_params(n, seed=msd), flags=flags)
            pair_line(name, "augmented_params(%d, seed=%d) x 1000, seed %d" % (n, msd, sd), r)
        for what, P in (("mass-touching", mass), ("thread-touching", thread)):
            for sd in range(seeds):
                pair_line(name, "%s 64 x 300 uniform, seed %d" % (what, 210 + sd), teacher_forced("move_to_pose", 64, 300, seed=210 + sd, params=P, flags=flags))
                pair_line(name, "%s 64 x 150 flat out, seed %d" % (what, 220 + sd), teacher_forced("move_from_origin", 64, 150, seed=220 + sd, params=P, flags=flags, flat_out=True))
                pair_line(name, "%s 64 x 150 flat out after 250, seed %d" % (what, 230 + sd), teacher_forced("move_from_origin", 64, 150, seed=230 + sd, params=P, flags=flags, flat_out=True, skip=250))
print("# worst held reward difference over this run (REWARD_HELD_MEASURED): %.3e" % max(held))
print("# %.0f s" % (time.time() - t0))

"""What does the evaluate pass cost, against a readout of the same stack and against the Python loop it replaces?  (run on the GPU box)

    python tools/evaluate_timing.py [--repeats 15] [--out profiles/evaluate_timing.txt]

At N = 4096 envs, for the current state (n_snaps = 1) and for a stack of 100 snapshots: the pass (jb_evaluate_device) with all four
outputs and with `reward` only; a readout (frames + clearance) of the same env-states; and the loop a caller had to write before the pass
existed - restore_device + observe_device (obs and reward) once per snapshot, which also overwrites the env's state.  All in ONE process
on this tree's library, the three alternated inside every repeat.  Times are medians over the repeats after warm-up, taken with events on
the env's stream around `inner` back-to-back launches (the loop: around its n_snaps restore + observe pairs, so its figure holds the
launches' host cost where the host is the slower side).  A record, not a gate."""
import argparse

import pass_timing as pt

ap = argparse.ArgumentParser()
args = pt.arguments(ap)

import torch

from jitterbug_amd import model

dev = torch.device("cuda", 0)
N = 4096
EV_BYTES = dict(obs=4 * 19, reward=4, terms=16, achieved=12)          # move_to_pose: 19 observation entries
RO_BYTES = 4 * (model.NFRAME * 12 + model.NGEOM)

lines = ["evaluate pass at N = %d (move_to_pose), against a readout (frames + clearance) of the same env-states and the loop it replaces "
         "(restore_device + observe_device per snapshot), one process; median (min .. max) over %d repeats" % (N, args.repeats),
         "bytes stored per env-state: evaluate, all four %d, reward only %d; readout %d; the loop's observe %d (and it copies the %d-byte state)"
         % (sum(EV_BYTES.values()), EV_BYTES["reward"], RO_BYTES, EV_BYTES["obs"] + EV_BYTES["reward"], 232),
         "the loop's figure is the time of its 2 x n_snaps launches as the host issues them (events around the whole loop): host-bound, not GPU time "
         "against GPU time; the pass and the readout are events around `inner` back-to-back launches of one kernel"]
for n_snaps in (1, 100):
    m = n_snaps * N
    env, stream, _, snaps, _ = pt.prepared(N, n_snaps)
    D = env.obs_dim
    out = dict(obs=torch.zeros((m, D), device=dev), reward=torch.zeros((m,), device=dev), terms=torch.zeros((m, 4), device=dev), achieved=torch.zeros((m, 3), device=dev))
    frames, clear = torch.zeros((m, model.NFRAME * 12), device=dev), torch.zeros((m, model.NGEOM), device=dev)
    loop_obs, loop_rew = torch.zeros((N, D), device=dev), torch.zeros((N,), device=dev)
    torch.cuda.synchronize()
    stack = None if n_snaps == 1 else snaps.data_ptr()          # (a stack of one would be the same launch on other memory)
    p = {k: v.data_ptr() for k, v in out.items()}

    def everything():
        env.evaluate_device(obs_ptr=p["obs"], reward_ptr=p["reward"], terms_ptr=p["terms"], achieved_ptr=p["achieved"], snaps_ptr=stack, n_snaps=n_snaps)

    def reward_only():
        env.evaluate_device(reward_ptr=p["reward"], snaps_ptr=stack, n_snaps=n_snaps)

    def readout():
        env.readout_device(frames.data_ptr(), clear.data_ptr(), snaps_ptr=stack, n_snaps=n_snaps)

    inner = 20 if n_snaps == 1 else 5
    (ev, ev_lo, ev_hi), (rw, rw_lo, rw_hi), (ro, ro_lo, ro_hi) = pt.timed(args, stream, [everything, reward_only, readout], inner)

    def loop():
        for k in range(n_snaps):
            env.restore_device(snaps[k].data_ptr())
            env.observe_device(loop_obs.data_ptr(), loop_rew.data_ptr())

    (lp, lp_lo, lp_hi), = pt.timed(args, stream, [loop], 1)
    # the pass and the loop give the same rows
    reward_only()
    env.synchronize()
    assert torch.equal(out["reward"][(n_snaps - 1) * N:], loop_rew)
    for name, (med, lo, hi), stored in (("evaluate, all four", (ev, ev_lo, ev_hi), sum(EV_BYTES.values())), ("evaluate, reward only", (rw, rw_lo, rw_hi), EV_BYTES["reward"]),
                                        ("readout, frames + clearance", (ro, ro_lo, ro_hi), RO_BYTES), ("restore + observe loop", (lp, lp_lo, lp_hi), EV_BYTES["obs"] + EV_BYTES["reward"])):
        lines.append("%7d env-states (%3d x %d)  %-28s %.4f ms (%.4f .. %.4f) = %.5f us per env-state, %.0f GB/s stored;  %.2f of the readout, %.3f of the loop"
                     % (m, n_snaps, N, name, med, lo, hi, 1e3 * med / m, m * stored / med / 1e6, med / ro, med / lp))
    env.close()
pt.report(args, lines)

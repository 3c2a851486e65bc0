"""Episode boundaries on the GPU against the CPU fp64 oracle: the step kernel's control-step epilogue (jb_step.hpp control_step_tail: time limit,
terminal reward, in-place reset, new target, counters, first observation of the new episode) and the masked jb_reset_kernel, on every launch
row, every task, per-env tables, shards and the failure counter.

The env under test runs FREE with auto_reset and never gets set_state: what the kernel writes at a reset is what it continues from.  The
cases, their seeds and the driver are tests/episode_inputs.py (its conditions are asserted on the oracle alone by
tests/test_episode_boundary_cpu.py); the tolerance lines are parity_protocol's and test_reset_matches_oracle's, none is new."""
import numpy as np
import pytest

from jitterbug_amd import model
from jitterbug_amd.vec_env import JitterbugVecEnv
from oracle import oracle as O
from tests import episode_inputs as ei
from tests.parity_inputs import LAUNCH_ROWS
from tests.parity_protocol import MARGIN_TOL, REWARD_HELD_CAP, ParityTally, assert_protocol, near_switch_cap, protocol_message, within

pytestmark = pytest.mark.gpu


def make_env(c, lo=0, hi=None, **kw):
    hi = c["n"] if hi is None else hi
    kw.setdefault("time_limit", ei.TIME_LIMIT)
    if c["variant"] is not None:
        kw.update(flags=ei.variant_flags(c["variant"]), envs_per_wave=c["epw"])
    P = None if c["params"] is None else c["params"][lo:hi]
    return JitterbugVecEnv(hi - lo, c["task"], seed=c["seed"], random_pose=c["random_pose"], params=P, env_offset=lo, **kw)


def run_case(c, **kw):
    env, o = make_env(c), ei.make_oracle(c)
    if c["variant"] is not None:
        assert env.kernel_variant == c["variant"] and env.envs_per_wave == c["epw"]
    env.reset(), o.reset()
    r = ei.boundary_run(env, o, c, **kw)
    env.close()
    print(r)
    return r


def assert_boundary_protocol(c, r, steps=ei.STEPS):
    done = ei.clocks(c["n"], steps, c["stagger"])[0]
    assert r["boundaries"] == done.sum() and r["env_steps"] == done.size - done.sum(), r
    # (a terminal step near a contact switch is not held to the reward line - the protocol's rule -; the inputs have none on the oracle alone,
    #  and the share the protocol allows a run of this size is the cap on how many the free run may meet)
    assert r["boundaries"] - r["reward_compared"] <= np.ceil(near_switch_cap(r["boundaries"]) * r["boundaries"]), r
    # random_pose=False: the first control step of every episode starts with the feet ON the floor and is near a switch by construction
    # (episode_inputs.fixed_pose_first_steps): those env-steps on top of the cap, nothing else
    first = ei.fixed_pose_first_steps(c, steps)
    assert_protocol(r, well_bad=0, worst_well=2e-5, near_cap=near_switch_cap(r["env_steps"]) + first.sum() / r["env_steps"])
    if not c["per_env"]:
        assert r["deep_steps"] == 0, protocol_message(r)


@pytest.mark.parametrize("variant,epw", LAUNCH_ROWS, ids=["%s-%d" % r for r in LAUNCH_ROWS])
def test_every_launch_row_across_three_resets(variant, epw):
    """Every row of the launch table, two full waves and a ragged one, 19 control steps of the flat stream (motor angle past pi, hinges at
    0.04 rad when a reset has to clear them), clocks staggered so that the envs of a wave reach their limits on different steps; per-env
    tables with a reset height and a target height of their own per env on the PAIR rows.  move_to_pose: the terminal reward differs from the
    new episode's (reward_moved), so a reward taken after the reset would show."""
    c = ei.row_case(variant, epw)
    r = run_case(c)
    assert_boundary_protocol(c, r)
    assert r["reward_moved"] >= 1, r


@pytest.mark.parametrize("random_pose", [True, False], ids=["random", "fixed"])
@pytest.mark.parametrize("task", model.TASKS)
def test_every_task_across_three_resets(task, random_pose):
    c = ei.task_case(task, random_pose)
    assert_boundary_protocol(c, run_case(c))


MASKED_ROWS = [("ordinary", 4), ("lean", 2), ("lean_pair", 4)]


@pytest.mark.parametrize("variant,epw", MASKED_ROWS, ids=["%s-%d" % r for r in MASKED_ROWS])
def test_masked_reset_mid_episode(variant, epw):
    """reset(mask) after four flat steps (no stagger before it): the drawn pose, the target and the returned rows of the selected envs against
    the oracle's, the others bit-unchanged with their rows the observation of their state, counters equal; then both go on for two steps."""
    c = dict(ei.row_case(variant, epw), stagger=ei.NO_STAGGER)
    n = c["n"]
    env, o = make_env(c), ei.make_oracle(c)
    env.reset(), o.reset()
    r = ei.boundary_run(env, o, c, steps=4)
    mask = (np.arange(n) % 2 == 1).astype(np.uint8)
    q = env.get_state()[0]
    assert (np.abs(q[:, 15]) > 1.0).all() and (np.abs(q[:, 7:15]).max(axis=1) > 1e-3).all()          # there is something to clear
    ei.masked_reset(env, o, c, mask)
    sc, ep, _ = env.counters()
    assert np.array_equal(sc, np.where(mask, 0, 4)) and np.array_equal(ep, np.where(mask, 3, 2))
    act = ei.flat(n)
    for t in range(2):          # ... and the kernel continues from what the reset kernel wrote
        pre = env.get_state()
        og, rg, dg, _ = env.step(act(t))
        o.set_state(*pre)
        oo, ro, do = o.step(act(t), auto_reset=True)
        well = o.conditioning()["switch"] >= MARGIN_TOL
        assert within(og.astype(np.float64), oo)[well].all() and np.array_equal(dg, do.astype(bool)) and np.array_equal(dg, ~mask.astype(bool) & (t == 1))
    env.close()


SHARD_ROWS = [("ordinary", 4), ("lean_pair", 4)]


@pytest.mark.parametrize("variant,epw", SHARD_ROWS, ids=["%s-%d" % r for r in SHARD_ROWS])
def test_two_shards_equal_the_unsplit_run_across_the_resets(variant, epw):
    """The Philox key is (seed, env_offset + env, episode): the launch row's case as one batch and as two shards (5 + 4 envs: the waves are
    composed differently too) gives the same observations, rewards, done flags and states, bit for bit, through the staggered resets."""
    c = ei.row_case(variant, epw)
    n = c["n"]
    act = ei.flat(n)

    def run(parts):
        outs = []
        for lo, hi in parts:
            e = make_env(c, lo, hi)
            rec = [np.concatenate([e.reset()] + [x.reshape(hi - lo, -1) for x in e.get_state()], axis=1)]
            for t in range(ei.STEPS):
                for s, r in c["stagger"]:
                    if s == t:
                        e.reset(ei.stagger_mask(n, r)[lo:hi])
                ob, rw, dn, _ = e.step(act(t)[lo:hi])
                rec.append(np.concatenate([ob, rw[:, None], dn[:, None].astype(np.float64)] + [x.reshape(hi - lo, -1) for x in e.get_state()], axis=1))
            sc, ep, cap = e.counters()
            outs.append((rec[0], np.stack(rec[1:]), sc, ep))
            e.close()
        return [np.concatenate([o_[k] for o_ in outs], axis=-2 if k < 2 else 0) for k in range(4)]

    whole, split = run([(0, n)]), run([(0, 5), (5, n)])
    for a, b in zip(whole, split):
        assert np.array_equal(a, b)
    assert np.isfinite(whole[1]).all() and whole[3].max() == 5          # three in-kernel resets on top of the two explicit ones


def test_without_auto_reset_done_stays_set_and_the_state_goes_on():
    c = dict(ei.row_case("ordinary", 4), stagger=ei.NO_STAGGER)
    env, o = make_env(c, auto_reset=False), ei.make_oracle(c)
    env.reset(), o.reset()
    dones = []
    r = ei.boundary_run(env, o, c, steps=ei.L + 3, auto_reset=False, hook=lambda t, og, rg, dg, post: dones.append(dg.copy()))
    sc, ep, _ = env.counters()
    env.close()
    print(r)
    assert np.array_equal(np.array(dones), np.arange(ei.L + 3)[:, None] >= ei.L - 1 + np.zeros((1, c["n"]), int))
    assert (sc == ei.L + 3).all() and (ep == 2).all()
    assert r["boundaries"] == 0 and r["env_steps"] == c["n"] * (ei.L + 3), r
    assert_protocol(r, well_bad=0, worst_well=2e-5, near_cap=near_switch_cap(r["env_steps"]))
    assert r["deep_steps"] == 0, protocol_message(r)


def test_failure_counter_survives_a_reset_and_the_new_episode_is_clean():
    """One NaN in one env's qpos (the input of test_non_finite_state_is_flagged_in_the_failure_counter) one step before that env's limit: the
    boundary step flags it (+1000, kept across the reset), and the reset leaves that env finite and equal to the oracle's new episode -
    state, observation, target; its wave-mates stay inside the protocol."""
    c = dict(ei.task_case("move_from_origin", True))
    n, bad, P = c["n"], 3, model.default_params()
    env, o = make_env(c), ei.make_oracle(c)
    env.reset(), o.reset()
    r = ei.boundary_run(env, o, c, steps=ei.L - 1)
    assert r["boundaries"] == 0
    q, v, tg = env.get_state()
    qn = q.copy(); qn[bad, 0] = np.nan
    env.set_state(qn, v, tg)
    a = ei.uniform(n, c["seed"])(ei.L - 1)
    og, rg, dg, _ = env.step(a)
    o.set_state(q, v, tg)          # (the oracle takes the step from the finite state: only its reset is compared for that env)
    oo, ro, do = o.step(a, auto_reset=True)
    assert dg.all() and do.all()
    sc, ep, cap = env.counters()
    sco, epo = o.counters()
    assert np.array_equal(sc, sco) and np.array_equal(ep, epo)
    assert cap[bad] >= 1000 and (np.delete(cap, bad) < 1000).all()
    assert np.isfinite(og).all()
    ei.assert_new_episode(np.ones(n, bool), og, oo, env.get_state(), o.get_state(), P, "after the non-finite step")
    held = (np.arange(n) != bad) & (o.conditioning()["switch"] >= MARGIN_TOL)
    assert held.sum() >= n - 2 and (np.abs(rg.astype(np.float64) - ro)[held] <= REWARD_HELD_CAP).all()
    # the new episode: everyone inside the protocol, the flagged env included, and its counter keeps the +1000
    r = boundary_tail(env, o, c, first=ei.L, steps=3)
    assert_protocol(r, well_bad=0, worst_well=2e-5, near_cap=near_switch_cap(r["env_steps"]))
    cap2 = env.counters()[2]
    assert cap2[bad] >= 1000 and (np.delete(cap2, bad) < 1000).all()
    env.close()


def boundary_tail(env, o, c, first, steps):
    """`steps` more control steps of the case's stream from step `first` on, every env-step into a tally (no boundary among them)"""
    n = c["n"]
    act = ei.STREAMS[c["stream"]](n, c["seed"])
    tally = ParityTally(n, c["task"], ei.case_params(c))
    followed = np.zeros(n, bool)
    for t in range(first, first + steps):
        pre = env.get_state()
        og, rg, dg, _ = env.step(act(t))
        o.set_state(*pre)
        oo, ro, do = o.step(act(t), auto_reset=True)
        assert not dg.any() and not do.any()
        tally.cascade(followed, o, og, oo)
        followed = tally.add(o, og, oo, rg, ro, env.get_state())
    return tally.result((env.counters()[2] % 1000).sum())

"""The strict parity protocol's own instrument (tests/parity_protocol.py) on the CPU: an error of a given size planted in an env-step of a
given class must land in the counter that fails the assertion.  The env under test is a stand-in - the oracle itself behind the calls
teacher_forced makes, handed a state rounded through fp32 and answering in fp32 -, so a clean run is clean, and a planted error is the only
thing a run can be caught on.  Because the run is teacher-forced, the class of every env-step is a property of the ORACLE'S trajectory: the
tests find the env-step they want by running an OracleEnv alone on the same seed and action stream and reading conditioning() themselves
(not through classify(), which is under test).

Inputs:  A  nominal model, move_to_pose, 8 envs x 5 steps, seed 3: every env-step well.
         B  mass-touching models, move_to_pose, 16 x 60, seed 4, uniform actions: deep env-steps with a converged narrow phase, one near-switch.
         C  the same models, move_from_origin, 16 x 40, seed 5, motor flat out: a deep env-step whose narrow phase stops short of its root.
Every planted error is sized from the module's constants: s(x) = 1e-4 |x| + 1e-5 is the strict line at an entry of value x."""
import os
import subprocess
import sys

import numpy as np
import pytest

from jitterbug_amd import model
from oracle import oracle as O
from tests import parity_protocol as pp
from tests.parity_inputs import mass_touching_models, tiled

ENTRY = 5                         # the observation entry the errors are planted in
NOT_ASSERTED = 10 ** 9            # `well_bad` on B and C: the fp32 cast of the stand-in's own output can leave the 1e-6 line on a tipped robot, which says nothing about the instrument


def two_s(x):
    return 2 * (1e-4 * abs(x) + 1e-5)


class StandIn:
    """An OracleEnv behind the calls the drivers make of an env under test.  set_state rounds velocities, x / y position and joint angles
    through fp32 (height and quaternion kept: the perturbation of tools/flip_study.py sensitivity()), step answers in fp32.
    plants: {(step, env, entry): size} - size(value) is added to that observation entry (entry "reward": to the reward) of that env at
    that step of THIS instance; step None: at every step."""
    kernel_variant = "stand-in"

    def __init__(self, n, task, P, seed, plants=None, **kw):
        step_limit = 2 ** 31 - 1 if kw.get("time_limit") == float("inf") else 1000
        self.o = O.OracleEnv(n, task, P, seed=seed, per_env_model=np.ndim(P) == 2, step_limit=step_limit)
        self.n, self.t, self.plants = n, 0, plants or {}

    def reset(self):
        return self.o.reset().astype(np.float32)

    def set_state(self, q, v, tg):
        q = q.copy()
        q[:, :2] = q[:, :2].astype(np.float32); q[:, 7:] = q[:, 7:].astype(np.float32)
        self.o.set_state(q, v.astype(np.float32).astype(np.float64), tg)

    def step(self, a):
        ob, rw, dn = self.o.step(np.asarray(a, dtype=np.float32), auto_reset=False)
        for (t, i, entry), size in self.plants.items():
            if t is None or t == self.t:
                if entry == "reward":
                    rw[i] += size(rw[i])
                else:
                    ob[i, entry] += size(ob[i, entry])
        self.t += 1
        return ob.astype(np.float32), rw.astype(np.float32), dn.astype(bool), {}

    def get_state(self):
        return self.o.get_state()

    def counters(self):
        sc, ep = self.o.counters()
        return sc, ep, np.zeros(self.n)

    def close(self):
        pass


@pytest.fixture(scope="module")
def inputs():
    P = tiled(mass_touching_models(), 16)
    return dict(A=dict(task="move_to_pose", n=8, steps=5, seed=3, params=model.default_params()),
                B=dict(task="move_to_pose", n=16, steps=60, seed=4, params=P),
                C=dict(task="move_from_origin", n=16, steps=40, seed=5, params=P, flat_out=True))


def run(inp, plants=None, cascade_plants=None):
    """teacher_forced over the stand-in; the cascade pair's env (made with time_limit=inf) gets plants of its own"""
    def make_env(**extra):
        return StandIn(inp["n"], inp["task"], inp["params"], inp["seed"], plants=cascade_plants if extra else plants, **extra)
    return pp.teacher_forced(make_env=make_env, **inp)


def oracle_classes(inp):
    """[steps, n] masks of the input's env-steps, from the oracle alone: near-switch, deep, deep with an unconverged narrow phase"""
    n, P = inp["n"], inp["params"]
    o = O.OracleEnv(n, inp["task"], P, seed=inp["seed"], per_env_model=P.ndim == 2)
    o.reset()
    rng = np.random.default_rng(inp["seed"])
    near, deep, unconv = [], [], []
    for t in range(inp["steps"]):
        o.step(np.ones(n) if inp.get("flat_out") else rng.uniform(-1, 1, size=n), auto_reset=False)
        c = o.conditioning()
        near.append(c["switch"] < pp.MARGIN_TOL); deep.append(c["deep"].astype(bool)); unconv.append(c["narrow_resid"] >= pp.NARROW_RESID_TOL)
    return np.array(near), np.array(deep), np.array(unconv)


def first(mask):
    """(step, env) of the first env-step of a [steps, n] mask"""
    assert mask.any()
    return tuple(int(x) for x in np.argwhere(mask)[0])


def raises_on(r, key, harmless, **kw):
    """assert_protocol raises on r, and on nothing but `key`: the same result with that one figure made harmless passes"""
    with pytest.raises(AssertionError):
        pp.assert_protocol(r, **kw)
    pp.assert_protocol({**r, key: harmless}, **kw)


def test_tolerance_lines_and_near_switch_cap():
    b = np.array([0.0, 1.0, -200.0])
    for fn, floor in ((pp.within, 1e-6), (pp.strict_within, 1e-5)):
        edge = np.array([0.0, 1e-4, 2e-2]) + floor          # 1e-4 relative, written out
        assert fn(b + 0.99 * edge, b).all() and fn(b - 0.99 * edge, b).all()
        assert not fn(b + 1.01 * edge, b).any() and not fn(b - 1.01 * edge, b).any()
        assert not fn(np.array([np.nan]), b[:1]).any()
    assert pp.near_switch_cap(9600) == pp.NEAR_SWITCH_CAP == pp.near_switch_cap(10 ** 6)
    assert pp.near_switch_cap(2880) == pytest.approx(pp.NEAR_SWITCH_CAP + 3 * np.sqrt(0.0015 * 0.9985 / 2880), rel=1e-12)
    assert pp.near_switch_cap(9599) > pp.NEAR_SWITCH_CAP
    assert pp.REWARD_HELD_CAP == 2 * pp.REWARD_HELD_MEASURED


def test_importing_the_protocol_loads_neither_pytest_nor_torch_nor_the_env():
    code = "import sys, tests.parity_protocol as p; assert p.MARGIN_TOL > 0; print([m for m in ('pytest', 'torch', 'jitterbug_amd.vec_env') if m in sys.modules])"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0 and out.stdout.strip() == "[]", (out.stdout, out.stderr)


def test_clean_runs_are_clean_and_the_inputs_hold_the_classes_they_are_chosen_for(inputs):
    near, deep, unconv = oracle_classes(inputs["A"])
    assert not near.any() and not deep.any()
    r = run(inputs["A"])
    assert r["env_steps"] == 40 and r["ill_steps"] == 0 and r["deep_steps"] == 0 and r["kernel_variant"] == "stand-in"
    pp.assert_protocol(r, well_bad=0)
    for name in ("B", "C"):
        near, deep, unconv = oracle_classes(inputs[name])
        r = run(inputs[name])
        print(name, r)
        # the tally's classes are the oracle's, read here without classify()
        assert r["ill_steps"] == near.sum() and r["deep_steps"] == (deep & ~near).sum() and r["clamped_steps"] == (deep & ~near & unconv).sum()
        assert r["strict_bad"] == r["deep_strict_bad"] == r["cascade_bad"] == r["reward_bad"] == 0, r
        if name == "B":
            assert (deep & ~near & ~unconv).any() and near.any()
        else:
            assert (deep & ~near & unconv).any()


def test_an_error_on_a_well_env_step_fails_the_strict_line(inputs):
    r = run(inputs["A"], {(2, 3, ENTRY): two_s})
    assert r["strict_bad"] == 1 and r["well_bad"] >= 1 and r["flip_margin_max"] > pp.MARGIN_TOL, r
    raises_on(r, "strict_bad", 0, well_bad=1)
    with pytest.raises(AssertionError):
        pp.assert_protocol({**r, "strict_bad": 0}, well_bad=0)          # ... and the counted north-star line on its own


def test_an_error_on_a_converged_deep_env_step_fails_the_deep_line(inputs):
    near, deep, unconv = oracle_classes(inputs["B"])
    t, i = first(deep & ~near & ~unconv)
    r = run(inputs["B"], {(t, i, ENTRY): two_s})
    assert r["deep_strict_bad"] == 1 and r["clamped_strict_bad"] == 0 and r["strict_bad"] == 0, r
    raises_on(r, "deep_strict_bad", 0, well_bad=NOT_ASSERTED)


def test_an_unconverged_deep_env_step_is_bounded_not_held_to_the_strict_line(inputs):
    near, deep, unconv = oracle_classes(inputs["C"])
    t, i = first(deep & ~near & unconv)
    r = run(inputs["C"], {(t, i, ENTRY): two_s})
    assert r["clamped_strict_bad"] == 1 and r["deep_strict_bad"] - r["clamped_strict_bad"] == 0 and r["strict_bad"] == 0, r
    pp.assert_protocol(r, well_bad=NOT_ASSERTED)                        # the deep lines do not fire
    r = run(inputs["C"], {(t, i, ENTRY): lambda x: 2 * pp.DEEP_ERROR_CAP})
    assert r["worst_clamped"] >= pp.DEEP_ERROR_CAP, r
    raises_on(r, "worst_clamped", 0.0, well_bad=NOT_ASSERTED)


def test_a_near_switch_env_step_is_excluded_bounded_and_followed(inputs):
    near, deep, unconv = oracle_classes(inputs["B"])
    t, i = first(near)
    assert 1e-4 * 1 + 1e-5 < 1e-3 < pp.ILL_ERROR_CAP                    # above the strict line of a normalised entry, below the cap
    r = run(inputs["B"], {(t, i, ENTRY): lambda x: 1e-3})
    assert r["ill_bad_steps"] == 1 and r["strict_bad"] == 0 and r["worst_ill"] >= 0.99e-3, r
    assert r["cascade_checked"] >= 1 and r["cascade_bad"] == 0, r      # the cascade pair of envs was made, and its step agrees
    pp.assert_protocol(r, well_bad=NOT_ASSERTED)
    # the same, and the followed env off the strict line in the cascade pair's step
    r = run(inputs["B"], {(t, i, ENTRY): lambda x: 1e-3}, cascade_plants={(None, i, ENTRY): two_s})
    assert r["cascade_bad"] == 1, r
    raises_on(r, "cascade_bad", 0, well_bad=NOT_ASSERTED)
    r = run(inputs["B"], {(t, i, ENTRY): lambda x: 2 * pp.ILL_ERROR_CAP})
    assert r["worst_ill"] >= pp.ILL_ERROR_CAP and r["strict_bad"] == 0, r
    raises_on(r, "worst_ill", 0.0, well_bad=NOT_ASSERTED)


def test_an_error_on_a_returned_reward_fails_both_reward_lines(inputs):
    r = run(inputs["A"], {(2, 3, "reward"): lambda x: 1e-3})
    assert r["worst_reward_held"] >= 0.99e-3 > pp.REWARD_HELD_CAP and r["reward_bad"] == 1, r
    with pytest.raises(AssertionError):
        pp.assert_rewards(r)
    with pytest.raises(AssertionError):
        pp.assert_rewards({**r, "reward_bad": 0})
    with pytest.raises(AssertionError):
        pp.assert_rewards({**r, "worst_reward_held": 0.0})
    pp.assert_rewards({**r, "reward_bad": 0, "worst_reward_held": 0.0})

"""The episode-boundary cases of tests/episode_inputs.py on the CPU.  First the conditions the GPU module (tests/test_gpu_episode_boundary.py)
relies on, asserted on the oracle alone for every case it runs: no env-step near a contact switch (nor, nominal, a deep one), a motor angle
past pi and bent hinges when a reset has to clear them, reset and target heights that differ from env to env, clocks that diverge inside
every wave, done flags as the clocks imply.  Then the driver itself on a stand-in - the oracle behind the calls the driver makes of an env
under test, answering in fp32 -: a clean run is clean, and each mistake a reset can make, planted in the stand-in, fails it."""
import numpy as np
import pytest

from jitterbug_amd import model
from oracle import oracle as O
from tests import episode_inputs as ei, parity_protocol as pp

CASES = ei.all_cases()


@pytest.fixture(scope="module")
def alone():
    """every case on the oracle alone, once"""
    return {name: ei.oracle_alone(c) for name, c in CASES}


@pytest.mark.parametrize("name,c", CASES, ids=[name for name, _ in CASES])
def test_conditions_of_a_case_on_the_oracle_alone(name, c, alone):
    r, n = alone[name], c["n"]
    near = r["switch"] < pp.MARGIN_TOL
    print(name, "smallest switch margin %.3g m over %d env-steps, near-switch %d, deep %d" % (r["switch"][~ei.fixed_pose_first_steps(c)].min(), near.size, near.sum(), r["deep"].sum()))
    # no near-switch env-step - but for the first step of every episode that starts in the rest pose, feet on the floor: exactly those
    assert np.array_equal(near, ei.fixed_pose_first_steps(c))
    if not c["random_pose"]:
        assert near.any() and (r["switch"][near] < 1e-15).all()
    if not c["per_env"]:
        assert not r["deep"].any()
    # done flags and counters are what the clocks imply
    done, sc, ep = ei.clocks(n, ei.STEPS, c["stagger"])
    assert np.array_equal(r["done"], done) and np.array_equal(r["sc"], sc) and np.array_equal(r["ep"], ep)
    assert np.array_equal(r["done"].sum(axis=1), done.sum(axis=1)) and done.sum() > 0
    if not c["stagger"]:
        assert np.array_equal(done.sum(axis=1), np.where((np.arange(ei.STEPS) + 1) % ei.L == 0, n, 0))          # three boundaries of the whole batch
    else:
        assert ep[-1].max() == ep[-1].min() == 5 and (done.sum(axis=0) >= 2).all()
    if c["stream"] == "flat":
        # the state a boundary step starts from (one step before the reset): motor past pi - `turns` and `phi` are non-zero -, every env's hinges bent
        q = r["q"]
        assert (np.abs(q[:, :, 15])[done] > np.pi).all()
        hinge = np.abs(q[:, :, 7:15]).max(axis=2)
        assert (hinge[done] > 1e-3).all() and hinge[done].max() > 0.02, hinge[done]
    if c["per_env"]:
        P = c["params"]
        z0, tz = P[:, model.P_ROOTPOS0 + 2].astype(np.float32), P[:, model.P_TARGETZ].astype(np.float32)
        assert len(np.unique(z0)) == n and len(np.unique(tz)) == n and not np.intersect1d(z0, tz).size          # pairwise different as the kernel holds them
        assert np.abs(np.diff(np.sort(z0))).min() > 1e-5 and np.abs(np.diff(np.sort(tz))).min() > 1e-5          # ... by far more than the 2e-7 m the state is held to
        assert np.all(P[:, model.P_ROOTPOS0:model.P_ROOTPOS0 + 2] == 0)
    if c["stagger"] and c["epw"] >= 2:
        # a wave holds `epw` consecutive envs: whenever one of its envs reaches its limit, another one does not (two step counts in the wave)
        for w0 in range(0, n, c["epw"]):
            wave = slice(w0, min(w0 + c["epw"], n))
            if wave.stop - wave.start < 2:
                continue
            hit = done[:, wave].any(axis=1)
            assert hit.any() and not done[hit][:, wave].all(axis=1).any(), (name, w0)


def test_the_first_stagger_entry_alone_would_leave_one_wave_in_lockstep():
    """why STAGGER has two entries: with `i % 3 == 1` alone, envs 2 and 3 - a whole wave at two envs per wave - share a clock"""
    done = ei.clocks(5, ei.STEPS, ei.STAGGER[:1])[0]
    assert np.array_equal(done[:, 2], done[:, 3])
    done = ei.clocks(5, ei.STEPS, ei.STAGGER)[0]
    assert not (done[:, 2] & done[:, 3]).any()


# ---------------------------------------------------------------------------------------------------------------- the driver, on a stand-in
class StandIn:
    """An OracleEnv behind the calls of a JitterbugVecEnv that the boundary tests make, answering in fp32; a reset leaves the height as the fp32
    number the kernel's table holds.  plant: one mistake of a reset - 'reward_after_reset', 'stale_motor' (the motor angle survives),
    'stale_low_word' (1 nm left on the height), 'neighbours_height' (env i starts at env i+1's height), 'next_episodes_target' (the draw is keyed
    with another episode: the target of a different draw)."""
    kernel_variant, envs_per_wave = "stand-in", 0

    def __init__(self, n, task, seed=0, random_pose=True, params=None, env_offset=0, time_limit=10, auto_reset=True, plant=None, **kw):
        self.P = model.default_params() if params is None else np.asarray(params)
        self.n, self.task, self.auto_reset, self.plant = n, task, auto_reset, plant
        self.seed, self.env_offset, self.random_pose = seed, env_offset, random_pose
        self.o = O.OracleEnv(n, task, self.P, seed=seed, random_pose=random_pose, env_offset=env_offset, per_env_model=self.P.ndim == 2,
                             step_limit=int(np.ceil(time_limit / 0.01 - 1e-9)))

    def _after_reset(self, sel, q_before):
        q, v, tg = self.o.get_state()
        z0 = ei.root_z0(self.P, self.n).astype(np.float32).astype(np.float64)
        q[sel, 2] = z0[sel]
        if self.plant == "stale_motor":
            q[sel, 15] = q_before[sel, 15]
        if self.plant == "stale_low_word":
            q[sel, 2] += 1e-9
        if self.plant == "neighbours_height":
            q[sel, 2] = np.roll(z0, -1)[sel]
        if self.plant == "next_episodes_target":
            ep = self.o.counters()[1]
            for i in np.nonzero(sel)[0]:
                tg[i] = O.reset(self.P[i] if self.P.ndim == 2 else self.P, self.task, self.random_pose, self.seed, self.env_offset + i, int(ep[i]))[2]
        self.o.set_state(q, v, tg)

    def _obs(self):
        q, v, tg = self.o.get_state()
        return np.array([O.observation(self.P[i] if self.P.ndim == 2 else self.P, self.task, q[i], v[i], tg[i]) for i in range(self.n)]).astype(np.float32)

    def reset(self, mask=None):
        q = self.o.get_state()[0]
        self.o.reset(mask)
        self._after_reset(np.ones(self.n, bool) if mask is None else np.asarray(mask).astype(bool), q)
        return self._obs()

    def step(self, a):
        q = self.o.get_state()[0]
        ob, rw, dn = self.o.step(np.asarray(a, dtype=np.float32), auto_reset=self.auto_reset)
        dn = dn.astype(bool)
        if self.auto_reset and dn.any():
            self._after_reset(dn, q)
            ob = self._obs()
            if self.plant == "reward_after_reset":
                qn, vn, tn = self.o.get_state()
                for i in np.nonzero(dn)[0]:
                    rw[i] = O.reward(self.P[i] if self.P.ndim == 2 else self.P, self.task, qn[i], vn[i], tn[i])
        return ob.astype(np.float32), rw.astype(np.float32), dn, {}

    def get_state(self):
        return self.o.get_state()

    def set_state(self, q, v, tg):
        self.o.set_state(q, v, tg)

    def counters(self):
        sc, ep = self.o.counters()
        return sc, ep, np.zeros(self.n, dtype=np.float32)

    def close(self):
        pass


def drive(c, plant=None, **kw):
    env = StandIn(c["n"], c["task"], seed=c["seed"], random_pose=c["random_pose"], params=c["params"], time_limit=ei.TIME_LIMIT, plant=plant)
    o = ei.make_oracle(c)
    env.reset(), o.reset()
    return ei.boundary_run(env, o, c, **kw)


@pytest.mark.parametrize("row", [("ordinary", 4), ("pair", 2)], ids=["nominal", "per-env"])
def test_the_driver_is_clean_on_a_clean_env_and_counts_what_it_compares(row):
    c = ei.row_case(*row)
    r = drive(c)
    done = ei.clocks(c["n"], ei.STEPS, c["stagger"])[0]
    assert r["boundaries"] == r["reward_compared"] == done.sum() and r["env_steps"] == done.size - done.sum(), r
    assert r["reward_moved"] >= 1, r          # move_to_pose under the flat stream: the terminal reward is not the new episode's
    pp.assert_protocol(r, well_bad=0, worst_well=2e-5, near_cap=0)


@pytest.mark.parametrize("plant", ["reward_after_reset", "stale_motor", "stale_low_word", "next_episodes_target"])
def test_a_planted_reset_mistake_fails_the_driver(plant):
    with pytest.raises(AssertionError):
        drive(ei.row_case("ordinary", 2), plant=plant)


def test_a_neighbours_reset_height_fails_the_driver_on_per_env_tables():
    with pytest.raises(AssertionError):
        drive(ei.row_case("pair", 2), plant="neighbours_height")


def test_a_table_that_starts_an_episode_off_the_origin_is_refused_on_the_host():
    """The oracle's reset places the root at P[ROOTPOS0 + 0..2]; the kernel's keeps the height alone and starts at x = y = 0.  The table
    builder (jb_model_build.hpp, compiled for the host) refuses what it would otherwise simulate as if it were zero: code -7, any leg."""
    import ctypes as C
    import tests.build_harness as bh
    lib = C.CDLL(bh.build())
    dp = C.POINTER(C.c_double)
    lib.jbh_lane_table.argtypes = [dp, C.c_int, dp]
    out = np.zeros(lib.jbh_lm_count())
    P = model.default_params()
    assert lib.jbh_lane_table(P.ctypes.data_as(dp), 0, out.ctypes.data_as(dp)) == 0
    for k in (0, 1):
        for leg in range(4):
            bad = P.copy(); bad[model.P_ROOTPOS0 + k] = 1e-3
            assert lib.jbh_lane_table(bad.ctypes.data_as(dp), leg, out.ctypes.data_as(dp)) == -7
    up = P.copy(); up[model.P_ROOTPOS0 + 2] += 1e-3          # the height is the table's to choose
    assert lib.jbh_lane_table(up.ctypes.data_as(dp), 0, out.ctypes.data_as(dp)) == 0


def test_a_selection_keeps_the_tally_to_the_selected_envs():
    """ParityTally.add(sel=...): an error planted in an env outside the selection is not seen, inside it is; env_steps counts the selection"""
    c = ei.task_case("move_to_pose", True)
    n, P = c["n"], model.default_params()
    o = ei.make_oracle(c)
    o.reset()
    a = ei.uniform(n, c["seed"])(0)
    oo, ro, _ = o.step(a, auto_reset=True)
    state = o.get_state()
    sel = np.arange(n) % 2 == 0
    for planted, bad in ((1, 0), (2, 1)):
        og = oo.copy(); og[planted, 5] += 1e-3
        t = pp.ParityTally(n, c["task"], P)
        ill = t.add(o, og.astype(np.float32), oo, ro.astype(np.float32), ro, state, sel=sel)
        r = t.result(0)
        assert ill.shape == (n,) and not ill.any()
        assert r["env_steps"] == sel.sum() and (r["strict_bad"] > 0) == bool(bad), r

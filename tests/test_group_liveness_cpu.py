"""Register-only updates taken out from under their lane-GROUP predicates (jb_sim.hpp JB_GROUP_MERGE: the reload of the group reduction's
totals in contact_sweep, the iterate's update after star_solve and the check's record comparison in newton_phase) against the reference form
that keeps them under `is_main` / `grp == 0 || g1z` (-DJB_GROUP_PREDICATED_MERGES): the host build of the kernel source, compiled both
ways, must give the SAME BITS in fp32 and fp64 - the main lanes and the replica run the same arithmetic on the same operands, and what a
helper lane now computes on whatever it holds reaches no result.

Where the changed code is reached:
  * four lane groups take the transposed reduction whose totals every lane now reloads (the host wave's group distance is 16, as in the
    4-envs-per-wave kernels); two groups take the other branch, one group none: they cover the update after star_solve alone;
  * lying robots: spread rounds, a dozen contacts, rank-one passes between the full ones;
  * PAIR: the reduction carries a 53rd value; LEAN: no reduction hand-over, the state parked in the scratch;
  * max_newton = 1: the line-searched cold solve runs through the changed newton_phase (every lane group comes along there).
No tolerances, no excluded cases: equality only.  The host harness poisons the scratch before every substep, so a helper lane that read a
word nobody wrote in that substep would carry a NaN - harmless only if it really reaches nothing."""
import ctypes as C

import numpy as np
import pytest

from jitterbug_amd import model
from oracle import oracle as O

N_ENVS = 8
N_STEPS = 6          # control steps of 50 substeps from every env's start: 300 substeps per env and case
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _bind(path):
    lib = C.CDLL(path)
    for name in ("jbh_step_groups", "jbh_step_pair", "jbh_step_lean", "jbh_step_pair_lean"):
        getattr(lib, name).argtypes = [DP, DP, DP, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, DP]
    lib.jbh_rollout.argtypes = [DP, DP, DP, DP, IP, C.c_int, DP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, DP, C.c_int, C.c_int, DP]
    lib.jbh_ls_stats.argtypes = [C.POINTER(C.c_long), C.c_int]
    return lib


@pytest.fixture(scope="module")
def libs():
    """(the product form, the reference form under its group predicates)"""
    import tests.build_harness as bh
    return _bind(bh.build()), _bind(bh.build(defines={"JB_GROUP_PREDICATED_MERGES": 1}))


@pytest.fixture(scope="module")
def starts(params):
    """Start states and action sequences of the two regimes, computed once, as tests/test_fused_row_build_cpu.py makes them: upright
    (uniform actions) and lying (motor flat out until robots rest on a leg).  The oracle only supplies states; every comparison below is
    between the two host builds."""
    out = {}
    for regime in ("upright", "lying"):
        env = O.OracleEnv(N_ENVS, "move_from_origin", params, seed=5, step_limit=10 ** 9)
        env.reset()
        rng = np.random.default_rng(2)
        for t in range(260 if regime == "lying" else 30):
            env.step(np.ones(N_ENVS) if regime == "lying" else rng.uniform(-1, 1, size=N_ENVS), auto_reset=False)
        q, v, _ = env.get_state()
        if regime == "lying":
            assert ((1 - 2 * (q[:, 4] ** 2 + q[:, 5] ** 2)) < 0.5).any()      # some robots really lie on the floor
            acts = np.ones((N_STEPS, N_ENVS))
        else:
            acts = np.random.default_rng(7).uniform(-1, 1, size=(N_STEPS, N_ENVS))
        out[regime] = (q.copy(), v.copy(), acts)
    return out


def _states(lib, P, q, v, acts, groups, f32, spread, maxn, fn):
    """every env stepped N_STEPS control steps by one build, feeding its own results back: the first differing bit grows from there on"""
    q, v = q.copy(), v.copy()
    trace = []
    lib.jbh_set_spread(spread)
    try:
        for a in acts:
            for i in range(q.shape[0]):
                qi, vi, fail = np.ascontiguousarray(q[i]), np.ascontiguousarray(v[i]), np.zeros(1)
                assert getattr(lib, fn)(P.ctypes.data_as(DP), qi.ctypes.data_as(DP), vi.ctypes.data_as(DP), float(a[i]), 50, 1, maxn, f32, groups, 1, fail.ctypes.data_as(DP)) == 0
                q[i], v[i] = qi, vi
                trace.append(np.concatenate([qi, vi, fail]))
    finally:
        lib.jbh_set_spread(1)
    return np.array(trace)


def _same_states(libs, params, starts, regime, groups, f32, spread, maxn=20, fn="jbh_step_groups"):
    P = np.ascontiguousarray(params, dtype=np.float64)
    q, v, acts = starts[regime]
    a, b = (_states(lib, P, q, v, acts, groups, f32, spread, maxn, fn) for lib in libs)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert a.tobytes() == b.tobytes(), "first differing row %d of %d" % (int(np.argmax((a != b).any(axis=1))), len(a))


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("spread", [1, 0])
@pytest.mark.parametrize("groups", [1, 2, 4])
@pytest.mark.parametrize("regime", ["upright", "lying"])
def test_states_are_bit_identical_to_the_group_predicated_form(libs, params, starts, regime, groups, spread, f32):
    """(the ordinary kernel's two-group layout - 8 envs per wave - keeps the update after star_solve under its predicate,
    StepLayout::every_lane_update, so with two groups this compares the check's records alone; the PAIR kernel's two-group layout below has both)"""
    _same_states(libs, params, starts, regime, groups, f32, spread)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("fn,groups", [("jbh_step_pair", 1), ("jbh_step_pair", 2), ("jbh_step_pair", 4), ("jbh_step_lean", 1), ("jbh_step_lean", 2), ("jbh_step_lean", 4),
                                       ("jbh_step_pair_lean", 4)])
@pytest.mark.parametrize("regime", ["upright", "lying"])
def test_states_in_the_pair_and_lean_layouts(libs, params, starts, regime, fn, groups, f32):
    """PAIR with four groups: the transposed reduction with its 53rd value, reloaded by every lane.  LEAN: the totals are combined in
    registers (no hand-over), the update after star_solve runs on the main lanes alone in the hot solve and on every group in the cold one."""
    _same_states(libs, params, starts, regime, groups, f32, 1, fn=fn)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("fn,groups", [("jbh_step_groups", 1), ("jbh_step_groups", 2), ("jbh_step_groups", 4), ("jbh_step_pair", 4), ("jbh_step_lean", 4)])
@pytest.mark.parametrize("regime", ["upright", "lying"])
def test_states_with_a_small_newton_cap(libs, params, starts, regime, fn, groups, f32):
    """max_newton = 1: most substeps run into the cap and are solved again by the line-searched cold solve - the helper groups come along
    through its update (the step along the direction, the flags) and its checks on whatever they hold"""
    st = (C.c_long * 4)()
    libs[0].jbh_ls_stats(st, 1)
    _same_states(libs, params, starts, regime, groups, f32, 1, maxn=1, fn=fn)
    libs[0].jbh_ls_stats(st, 0)
    assert st[0] > 50, list(st)      # the cold solve really ran


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("regime", ["upright", "lying"])
def test_observations_rewards_and_states_of_the_rollout_loop(libs, params, starts, regime, groups, f32):
    """the fused rollout's loop (normalise, substeps, control-step tail) on the ordinary layout: observation rows, rewards, done flags and
    the final state of every env"""
    task = "move_from_origin"
    D = model.OBS_DIM[task]
    P = np.ascontiguousarray(params, dtype=np.float64)
    q0, v0, acts = starts[regime]
    out = []
    for lib in libs:
        rows_all = []
        for i in range(N_ENVS):
            q, v = q0[i].copy(), v0[i].copy()          # (the call writes the final state back: never into the shared starts)
            tgt, cnt = np.zeros(3), np.zeros(2, dtype=np.int32)
            a = np.ascontiguousarray(acts[:, i], dtype=np.float64)
            rows = np.full((N_STEPS, D + 2), np.nan)
            rc = lib.jbh_rollout(P.ctypes.data_as(DP), q.ctypes.data_as(DP), v.ctypes.data_as(DP), tgt.ctypes.data_as(DP), cnt.ctypes.data_as(IP), N_STEPS, a.ctypes.data_as(DP),
                                 model.TASKS.index(task), 50, 10 ** 9, 0, 0, 5, i, None, groups, f32, rows.ctypes.data_as(DP))
            assert rc == 0, rc
            rows_all.append(np.concatenate([rows.ravel(), q, v]))
        out.append(np.array(rows_all))
    a, b = out
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert a.tobytes() == b.tobytes(), "first differing env %d" % int(np.argmax((a != b).any(axis=1)))

"""The wave-uniform decisions of the Newton loop's check and the substep's broadphase taken as votes of the main lanes by EVERY lane
(jb_lane.hpp main_vote, StepLayout::scalar_votes) against the reference form that takes them under `is_main` and hands the
answer over with wave_bcast_u (-DJB_VECTOR_VOTES): the host build of the kernel source, compiled both ways, must give the SAME BITS in
fp32 and fp64, and the product form must agree with the oracle as the kernel source always has.

With the scalar votes the helper groups run the records' decode, the rank-one pass and the broadphase on whatever they hold.  The host
harness poisons the scratch before every substep and starts a helper lane from a harmless state, so a helper lane's junk that reached a
store, a vote or the main lanes' arithmetic would show as a NaN or a changed bit.  Four group threads (group distance 16, as in the
4-envs-per-wave kernels) in every case; states as in tests/test_group_liveness_cpu.py: walking robots (uniform actions) and tipped ones
(motor flat out until robots lie on a leg: spread rounds, a dozen contacts, rank-one passes between the full ones).
No tolerance on the comparison of the two builds: equality only."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

N_ENVS = 8
N_STEPS = 6          # control steps of 50 substeps from every env's start: 300 substeps per env and case
GROUPS = 4
DP = C.POINTER(C.c_double)
STEP_FNS = ("jbh_step_groups", "jbh_step_pair", "jbh_step_lean", "jbh_step_pair_lean")


def _bind(path):
    lib = C.CDLL(path)
    for name in STEP_FNS:
        getattr(lib, name).argtypes = [DP, DP, DP, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, DP]
    lib.jbh_ls_stats.argtypes = [C.POINTER(C.c_long), C.c_int]
    return lib


@pytest.fixture(scope="module")
def libs():
    """(the product form, the reference form: every decision under the main lanes' predicate)"""
    import tests.build_harness as bh
    return _bind(bh.build()), _bind(bh.build(defines={"JB_VECTOR_VOTES": 1}))


@pytest.fixture(scope="module")
def starts(params):
    """Start states, action sequences and the oracle's state one control step on, for the two regimes - computed once.  The oracle's
    step is the reference of the agreement test below; the bit comparison is between the two host builds alone."""
    out = {}
    for regime in ("walking", "tipped"):
        env = O.OracleEnv(N_ENVS, "move_from_origin", params, seed=5, step_limit=10 ** 9)
        env.reset()
        rng = np.random.default_rng(2)
        for t in range(260 if regime == "tipped" else 30):
            env.step(np.ones(N_ENVS) if regime == "tipped" else rng.uniform(-1, 1, size=N_ENVS), auto_reset=False)
        q, v, _ = env.get_state()
        if regime == "tipped":
            assert ((1 - 2 * (q[:, 4] ** 2 + q[:, 5] ** 2)) < 0.5).any()      # some robots really lie on the floor
            acts = np.ones((N_STEPS, N_ENVS))
        else:
            acts = np.random.default_rng(7).uniform(-1, 1, size=(N_STEPS, N_ENVS))
        env.step(acts[0], auto_reset=False)
        q1, v1, _ = env.get_state()
        for a in (q, v, acts, q1, v1):
            a.setflags(write=False)
        out[regime] = (q.copy(), v.copy(), acts, q1.copy(), v1.copy())
    return out


def _step(lib, P, q, v, a, f32, maxn, fn):
    qi, vi, fail = np.ascontiguousarray(q).copy(), np.ascontiguousarray(v).copy(), np.zeros(1)
    assert getattr(lib, fn)(P.ctypes.data_as(DP), qi.ctypes.data_as(DP), vi.ctypes.data_as(DP), float(a), 50, 1, maxn, f32, GROUPS, 1, fail.ctypes.data_as(DP)) == 0
    return qi, vi, fail


def _states(lib, P, q, v, acts, f32, maxn, fn):
    """every env stepped N_STEPS control steps by one build, feeding its own results back: the first differing bit grows from there on"""
    q, v = q.copy(), v.copy()
    trace = []
    for a in acts:
        for i in range(q.shape[0]):
            q[i], v[i], fail = _step(lib, P, q[i], v[i], a[i], f32, maxn, fn)
            trace.append(np.concatenate([q[i], v[i], fail]))
    return np.array(trace)


def _same_states(libs, params, starts, regime, f32, maxn=20, fn="jbh_step_groups"):
    P = np.ascontiguousarray(params, dtype=np.float64)
    q, v, acts = starts[regime][:3]
    a, b = (_states(lib, P, q, v, acts, f32, maxn, fn) for lib in libs)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert a.tobytes() == b.tobytes(), "first differing row %d of %d" % (int(np.argmax((a != b).any(axis=1))), len(a))


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("fn", STEP_FNS)
@pytest.mark.parametrize("regime", ["walking", "tipped"])
def test_states_are_bit_identical_to_the_vector_vote_form(libs, params, starts, regime, fn, f32):
    """the ordinary layout (replica and aux lanes: every group holds a state of its own in the broadphase), PAIR (helper groups 2 and 3
    hold the harmless state), LEAN and LEAN + PAIR (no replica: the helper groups load the parked factorisation for the rank-one pass)"""
    _same_states(libs, params, starts, regime, f32, fn=fn)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("regime", ["walking", "tipped"])
def test_states_through_the_line_searched_second_solve(libs, params, starts, regime, f32):
    """max_newton = 1: most substeps run into the cap, which the scalar form reads off the vote itself (`wave_capped`), and are solved
    again by newton_phase<LS = true> - every check of that solve votes too"""
    st = (C.c_long * 4)()
    libs[0].jbh_ls_stats(st, 1)
    _same_states(libs, params, starts, regime, f32, maxn=1)
    libs[0].jbh_ls_stats(st, 0)
    assert st[0] > 50, list(st)      # the second solve really ran


def test_scalar_vote_form_agrees_with_the_oracle(libs, params, starts):
    """One control step from the oracle's states against the oracle's own step, with the bounds the kernel source is held to elsewhere
    (tests/test_kernel_source_host.py): fp64 with four groups, walking and tipped, below 1e-10 (test_helper_groups_fp64_equal_single_group_and_oracle);
    fp32 on the walking states in that file's measure of the root coordinates, median below 1e-6 and 95 % below 1e-5
    (test_contact_rollout_fp64_equals_oracle_and_fp32_is_close)."""
    P = np.ascontiguousarray(params, dtype=np.float64)
    worst64, errs32 = 0.0, []
    for regime in ("walking", "tipped"):
        q0, v0, acts, q1, v1 = starts[regime]
        for i in range(N_ENVS):
            qh, vh, fail = _step(libs[0], P, q0[i], v0[i], acts[0][i], 0, 20, "jbh_step_groups")
            assert fail[0] == 0
            worst64 = max(worst64, np.abs(qh - q1[i]).max(), (np.abs(vh - v1[i]) / (1 + np.abs(v1[i]))).max())
            if regime == "walking":
                qf, vf, _ = _step(libs[0], P, q0[i], v0[i], acts[0][i], 1, 20, "jbh_step_groups")
                errs32.append(max(np.abs(qf[:7] - q1[i][:7]).max(), (np.abs(vf[:6] - v1[i][:6]) / np.array([1, 1, 1, 35, 35, 35])).max()))
    print("scalar votes vs oracle: fp64 %.2e, fp32 median %.2e, 95 %% %.2e" % (worst64, np.median(errs32), np.quantile(errs32, 0.95)))
    assert worst64 < 1e-10
    assert np.median(errs32) < 1e-6 and np.quantile(errs32, 0.95) < 1e-5

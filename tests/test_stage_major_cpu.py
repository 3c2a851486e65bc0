"""The order of independent instructions in the substep loop - the transposed group reduction run stage by stage over batches of quadruples
(jb_lane.hpp row_transpose_swap1 / _add1 / _swap2 / _add2, StepLayout::stage_major) and the packed accumulations run term by term over all
their accumulators (jb_sim.hpp acc_root, row_residuals, StepLayout::term_major) - against the reference order, one quadruple and
one accumulator after the other (-DJB_ELEMENT_MAJOR_ORDER): the host build of the kernel source, compiled both ways, must give the SAME BITS
in fp32 and fp64.

On the host the order of independent operations cannot matter, and no accumulator's own operations changed their order; what this catches
is an index slip in the reordered loops - a quadruple stored to another total's word, a batch boundary that skips or repeats one, a term
multiplied with the wrong row - and a host emulation of the two stages that associates other than (g0 + g2) + (g1 + g3).

Where the changed code is reached (the shapes of tests/test_group_liveness_cpu.py; the host harness binds its scratch by the same
StepLayout as the kernels, so each case runs the order its kernel row runs):
  * the ordinary layout with four lane groups 16 lanes apart takes the stage-major reduction: 13 quadruples in batches of 4, 3, 3, 3; two
    groups and one group take the other reduction and cover the term-major accumulations alone, as LEAN and PAIR do (PAIR keeps the
    element-major reduction);
  * lying robots: a dozen contacts, spread sweeps (contact_apply_leg runs the same acc_root), grouped full sweeps;
  * max_newton = 1: the line-searched cold solve sweeps through the same reduction and the same accumulations.
No tolerances, no excluded cases: equality only."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

N_ENVS = 8
N_STEPS = 6          # control steps of 50 substeps from every env's start: 300 substeps per env and case
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
    """(the product order, the reference order)"""
    import tests.build_harness as bh
    return _bind(bh.build()), _bind(bh.build(defines={"JB_ELEMENT_MAJOR_ORDER": 1}))


@pytest.fixture(scope="module")
def starts(params):
    """Start states and action sequences of the two regimes, computed once: upright (uniform actions) and lying (motor flat out until robots
    rest on a leg).  The oracle only supplies states; every comparison below is between the two host builds."""
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
        for a in (q, v, acts):
            a.setflags(write=False)
        out[regime] = (q, v, acts)
    return out


def _states(lib, P, q, v, acts, groups, f32, maxn, fn):
    """every env stepped N_STEPS control steps by one build, feeding its own results back: the first differing bit grows from there on"""
    q, v = q.copy(), v.copy()
    trace = []
    for a in acts:
        for i in range(q.shape[0]):
            qi, vi, fail = np.ascontiguousarray(q[i]), np.ascontiguousarray(v[i]), np.zeros(1)
            assert getattr(lib, fn)(P.ctypes.data_as(DP), qi.ctypes.data_as(DP), vi.ctypes.data_as(DP), float(a[i]), 50, 1, maxn, f32, groups, 1, fail.ctypes.data_as(DP)) == 0
            q[i], v[i] = qi, vi
            trace.append(np.concatenate([qi, vi, fail]))
    return np.array(trace)


def _same_states(libs, params, starts, regime, groups, f32, maxn=20, fn="jbh_step_groups"):
    P = np.ascontiguousarray(params, dtype=np.float64)
    q, v, acts = starts[regime]
    a, b = (_states(lib, P, q, v, acts, groups, f32, maxn, fn) for lib in libs)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert a.tobytes() == b.tobytes(), "first differing row %d of %d" % (int(np.argmax((a != b).any(axis=1))), len(a))


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("groups", [4, 2, 1])
@pytest.mark.parametrize("regime", ["upright", "lying"])
def test_states_are_bit_identical_to_the_element_major_order(libs, params, starts, regime, groups, f32):
    _same_states(libs, params, starts, regime, groups, f32)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("fn,groups", [("jbh_step_pair", 4), ("jbh_step_pair", 2), ("jbh_step_lean", 4), ("jbh_step_pair_lean", 4)])
@pytest.mark.parametrize("regime", ["upright", "lying"])
def test_states_in_the_pair_and_lean_layouts(libs, params, starts, regime, fn, groups, f32):
    """PAIR: the pair contact's rows (root columns scaled to zero) through the term-major accumulations.  LEAN: the totals are combined in
    registers, the accumulations are the same."""
    _same_states(libs, params, starts, regime, groups, f32, fn=fn)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("fn,groups", [("jbh_step_groups", 4), ("jbh_step_groups", 1), ("jbh_step_pair", 4)])
@pytest.mark.parametrize("regime", ["upright", "lying"])
def test_states_with_a_small_newton_cap(libs, params, starts, regime, fn, groups, f32):
    """max_newton = 1: most substeps run into the cap and are solved again by the line-searched cold solve, whose full sweeps end in the
    same reduction"""
    st = (C.c_long * 4)()
    libs[0].jbh_ls_stats(st, 1)
    _same_states(libs, params, starts, regime, groups, f32, maxn=1, fn=fn)
    libs[0].jbh_ls_stats(st, 0)
    assert st[0] > 50, list(st)      # the cold solve really ran


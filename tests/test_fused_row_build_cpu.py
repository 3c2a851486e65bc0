"""Contact rows built inside the first full Newton sweep (jb_sim.hpp contact_sweep, `build`) against the reference form that builds them
in a pass of their own (-DJB_SEPARATE_ROW_BUILD): the host build of the kernel source, compiled both ways, must give the SAME BITS in fp32
and fp64 - the fusion moves no arithmetic.

The cases that can go wrong, and where they are reached:
  * grouped plans with idle lanes in a round (2 and 4 lane groups, any state with two or more contacts);
  * spread rounds with adopted contacts (robots resting on a leg, spread sweeps on) and the ordinary loop over the same slots (spread off);
  * slots beyond the row cache (the two-entry row-cache build: a few rows are built in the sweep, the rest recomputed per pass);
  * a capped substep that enters the line-searched solve on the cached rows (max_newton = 1)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

N_ENVS = 8
N_STEPS = 6          # control steps of 50 substeps from every env's start: 300 substeps per env and case


def _build_reference(row_k=None):
    """tests/build_harness.py's command line plus the reference switch (and its staleness rule)."""
    import tests.build_harness as bh
    out = bh.OUT.replace(".so", "_seprows%s.so" % ("" if row_k is None else "_rowk%d" % row_k))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not (os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in bh.DEPS + [os.path.abspath(__file__)])):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", "-DJB_SEPARATE_ROW_BUILD"]
                              + (["-DJB_ROW_K=%d" % row_k] if row_k is not None else []) + ["-o", out, bh.SRC])
    return out


def _bind(path):
    lib = C.CDLL(path)
    dp = C.POINTER(C.c_double)
    for name in ("jbh_step_groups", "jbh_step_pair", "jbh_step_lean"):
        getattr(lib, name).argtypes = [dp, dp, dp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    return lib


@pytest.fixture(scope="module")
def libs():
    """(fused, reference) pairs: the default row cache and the two-entry one"""
    import tests.build_harness as bh
    return {None: (_bind(bh.build()), _bind(_build_reference())), 2: (_bind(bh.build(row_k=2)), _bind(_build_reference(row_k=2)))}


@pytest.fixture(scope="module")
def starts(params):
    """Start states and action sequences of the two regimes, computed once: walking (uniform actions) and lying (motor flat out until
    robots rest on a leg).  The oracle only supplies states; every comparison below is between the two host builds."""
    out = {}
    for regime in ("walking", "lying"):
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


def _rollout(lib, P, q, v, acts, groups, f32, spread, maxn, fn="jbh_step_groups"):
    """every env stepped N_STEPS control steps by one build, feeding its own results back: the first differing bit grows from there on"""
    dp = C.POINTER(C.c_double)
    q, v = q.copy(), v.copy()
    trace = []
    lib.jbh_set_spread(spread)
    try:
        for a in acts:
            for i in range(q.shape[0]):
                qi, vi, fail = np.ascontiguousarray(q[i]), np.ascontiguousarray(v[i]), np.zeros(1)
                assert getattr(lib, fn)(P.ctypes.data_as(dp), qi.ctypes.data_as(dp), vi.ctypes.data_as(dp), float(a[i]), 50, 1, maxn, f32, groups, 1, fail.ctypes.data_as(dp)) == 0
                q[i], v[i] = qi, vi
                trace.append(np.concatenate([qi, vi, fail]))
    finally:
        lib.jbh_set_spread(1)
    return np.array(trace)


def _same_bits(libs, params, starts, regime, row_k, groups, f32, spread, maxn=20, fn="jbh_step_groups"):
    P = np.ascontiguousarray(params, dtype=np.float64)
    q, v, acts = starts[regime]
    fused, ref = libs[row_k]
    a = _rollout(fused, P, q, v, acts, groups, f32, spread, maxn, fn)
    b = _rollout(ref, P, q, v, acts, groups, f32, spread, maxn, fn)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert a.tobytes() == b.tobytes(), "first differing row %d of %d" % (int(np.argmax((a != b).any(axis=1))), len(a))
    return a


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("spread", [1, 0])
@pytest.mark.parametrize("groups", [1, 2, 4])
@pytest.mark.parametrize("regime", ["walking", "lying"])
def test_fused_row_build_is_bit_identical_to_the_separate_pass(libs, params, starts, regime, groups, spread, f32):
    _same_bits(libs, params, starts, regime, None, groups, f32, spread)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("fn,groups", [("jbh_step_pair", 2), ("jbh_step_pair", 4), ("jbh_step_lean", 1), ("jbh_step_lean", 4)])
@pytest.mark.parametrize("regime", ["walking", "lying"])
def test_fused_row_build_in_the_pair_and_lean_layouts(libs, params, starts, regime, fn, groups, f32):
    """The two-group layout of the ordinary kernel (8 envs per wave) keeps the separate pass (StepLayout::fused_row_build), so the case above
    with two groups compares that pass with itself; the PAIR kernel's two-group layout builds in the sweep, and so do its four-group
    layout and the LEAN one (state, system and factorisation parked in the scratch around the sweep)."""
    _same_bits(libs, params, starts, regime, None, groups, f32, 1, fn=fn)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("regime", ["walking", "lying"])
def test_fused_row_build_with_slots_beyond_the_row_cache(libs, params, starts, regime, groups, f32):
    """two cached rows: built in the sweep (spread rounds with four groups on lying robots), every other slot recomputed per pass as before"""
    _same_bits(libs, params, starts, regime, 2, groups, f32, 1)


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("regime", ["walking", "lying"])
def test_fused_row_build_feeds_the_line_searched_solve(libs, params, starts, regime, groups, f32):
    """max_newton = 1: most substeps run into the cap and are solved again by the cold solve, which never builds - it reads the rows the hot
    solve's first sweep left in the cache"""
    lib = libs[None][0]
    lib.jbh_ls_stats.argtypes = [C.POINTER(C.c_long), C.c_int]
    st = (C.c_long * 4)()
    lib.jbh_ls_stats(st, 1)
    _same_bits(libs, params, starts, regime, None, groups, f32, 1, maxn=1)
    lib.jbh_ls_stats(st, 0)
    assert st[0] > 50, list(st)      # the cold solve really ran

"""The task layer the kernels inline (jitterbug_amd/csrc/jb_task.hpp) compiled for the host (tests/host_harness.cpp jbh_task_layer) on the
seam states of tests/task_reference.py, without a GPU: in fp64 the source must BE the oracle's formulas, seams included (1e-12); in fp32 it
must stay inside the derived bound of tests/task_reference.py (C roundings of 2^-24 on |y| + sum |dy/dx_i| |x_i|, plus one ulp on every input
word; the counts C are stated there and pinned here), and that bound must respect its own cap on the state set."""
import ctypes as C

import numpy as np
import pytest

from jitterbug_amd import model
from tests import task_reference as tr


@pytest.fixture(scope="module")
def hlib():
    import tests.build_harness as bh
    return C.CDLL(bh.build())


@pytest.fixture(scope="module")
def seams():
    return tr.seam_states()


@pytest.mark.parametrize("task", model.TASKS)
def test_rounding_counts_are_the_stated_ones(task):
    assert tr.roundings(task) == tr.ROUNDINGS[task]


def test_seam_states_are_fp32_words_and_the_bound_respects_its_cap(seams, params):
    q, v, t, fams, nv = seams
    assert np.array_equal(q[:, :15], q[:, :15].astype(np.float32).astype(np.float64)) and np.array_equal(v, v.astype(np.float32).astype(np.float64))
    assert set(fams) == {"heading", "motor", "position", "position_far", "upright", "velocity", "near_vertical"} and 2000 < len(q) < 8000
    for task in model.TASKS:
        b = tr.bounds(params, task, q, v, t)
        tr.assert_cap(b, nv)
        assert b["h"][nv].min() < 1.1e-3 and b["h"][~nv].min() > 0.9


@pytest.mark.parametrize("task", model.TASKS)
def test_fp64_source_equals_the_oracle_on_the_seams(hlib, seams, params, task):
    q, v, t, fams, nv = seams
    obs, rew, terms, _ = tr.host_task_layer(hlib, params, task, q, v, t, use_float=0)
    ref_o, ref_r, ref_t = tr.reference(params, task, q, v, t)
    assert tr.obs_error(task, obs, ref_o).max() < 1e-12
    assert np.abs(rew - ref_r).max() < 1e-12 and np.abs(terms - ref_t).max() < 1e-12


@pytest.mark.parametrize("task", model.TASKS)
def test_fp32_source_stays_inside_the_derived_bound_on_the_seams(hlib, seams, params, task):
    q, v, t, fams, nv = seams
    obs, rew, terms, _ = tr.host_task_layer(hlib, params, task, q, v, t, use_float=1)
    tr.compare(task, params, q, v, t, obs, rew, terms, fams, nv, "host fp32")


@pytest.mark.parametrize("policy", [None, tr.NON_DEFAULT_POLICY], ids=["default", "non_default"])
@pytest.mark.parametrize("task", model.TASKS)
def test_fp32_policy_agrees_with_the_reference_across_its_thresholds(hlib, params, task, policy):
    """heuristic_policy<float> on the rows of task_reference.policy_rows against policy_batch in fp64 on the same fp32 rows: 2e-6 (the line of
    the existing policy tests) on every kept row; at most 1 % of the rows are left out (within 4 ulp of a threshold behind atan2f)."""
    kw = policy or {}
    obs, keep = tr.policy_rows(task, **kw)
    assert (~keep).mean() <= 0.01
    act = _policy_on_rows(hlib, params, task, obs, policy)
    ref = tr.policy_reference(task, obs, **kw)
    assert len(set(np.round(ref[keep], 6))) >= 2
    assert np.abs(act[keep] - ref[keep]).max() <= 2e-6


def _policy_on_rows(lib, P, task, obs, policy):
    dp = C.POINTER(C.c_double)
    lib.jbh_policy_rows.argtypes = [C.c_int, C.c_int, dp, dp, dp]
    n = len(obs)
    o = np.ascontiguousarray(obs, dtype=np.float64)
    out = np.zeros(n)
    pp = None if policy is None else np.array([policy["kick_angle"], policy["speed"], policy["angle_threshold"]])
    lib.jbh_policy_rows(model.TASKS.index(task), n, o.ctypes.data_as(dp), None if pp is None else pp.ctypes.data_as(dp), out.ctypes.data_as(dp))
    return out

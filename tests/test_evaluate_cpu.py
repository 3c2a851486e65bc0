"""No-GPU checks of the evaluate pass (jitterbug_amd/csrc/jb_evaluate.hpp): the element functions the device kernel is made of, compiled
for the host in fp32 and fp64 (tests/evaluate_harness.cpp) and run on the seam batch of tests/task_reference.py packed into a two-deep
snapshot stack (tests/evaluate_inputs.py has the inputs, the references and the bounds); the override logic; the NULL-handle answers of the
new entry points; and one stand-alone sanitizer run of the host code.

The fp64 build must BE the oracle (1e-12, the line tests/test_task_layer_host.py holds jb_task.hpp itself to): that separates a wrong
formula, a wrong word or a wrong index from rounding.  The fp32 build goes through task_reference.compare: the derived bound with its cap."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from jitterbug_amd import model
from tests.build_harness import build_source
from tests import evaluate_inputs as ei
from tests import readout_inputs as ri
from tests import task_reference as tr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "evaluate_harness.cpp")
KEYS = ("obs", "reward", "terms", "achieved")


@pytest.fixture(scope="module")
def he():
    lib = C.CDLL(build_source(SRC, "libjb_evaluate_host.so", ["-Wall", "-O2", "-fPIC", "-shared"]))
    vp = C.c_void_p
    lib.jbe_run_f32.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.jbe_run_f64.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    assert lib.jbe_words_per_env() == ri.WORDS
    assert [lib.jbe_obs_dim(i) for i in range(5)] == [model.OBS_DIM[t] for t in model.TASKS]
    return lib


def run_words(he, snap, n, n_snaps, P, task, targets, dtype, want=KEYS):
    P = np.ascontiguousarray(P, dtype=np.float64)
    t = None if targets is None else np.ascontiguousarray(targets, dtype=dtype)
    shapes = dict(obs=(model.OBS_DIM[task],), reward=(), terms=(4,), achieved=(3,))
    out = {k: np.full((n * n_snaps,) + shapes[k], np.nan, dtype=dtype) for k in want}
    fn = he.jbe_run_f32 if dtype == np.float32 else he.jbe_run_f64
    ptr = lambda a: None if a is None else a.ctypes.data
    assert fn(snap.ctypes.data, n, n_snaps, P.ctypes.data, 1 if P.ndim == 1 else P.shape[0], model.TASKS.index(task), ptr(t), *[ptr(out.get(k)) for k in KEYS]) == 0
    for k in want:
        assert np.isfinite(out[k]).all(), k          # every promised entry was written
    return out


@pytest.mark.parametrize("task", model.TASKS)
def test_fp64_build_is_the_oracle(he, params, task):
    snap, n, (q, v, t, fams, nv), _ = ei.stack()
    o = run_words(he, snap, n, 2, params, task, t, np.float64)
    assert np.array_equal(params, model.default_params())
    ref_o, ref_r, ref_t = ei.reference(task)
    e_o, e_r, e_t = tr.obs_error(task, o["obs"], ref_o).max(), np.abs(o["reward"] - ref_r).max(), np.abs(o["terms"] - ref_t).max()
    ref_a = ei.achieved_reference(q)
    e_p, e_y = np.abs(o["achieved"][:, :2] - ref_a[:, :2]).max(), ei.circular(o["achieved"][:, 2] - ref_a[:, 2]).max()
    print("%s fp64: obs %.2e reward %.2e terms %.2e achieved xy %.2e yaw %.2e" % (task, e_o, e_r, e_t, e_p, e_y))
    assert e_o < ei.FP64_TOL and e_r < ei.FP64_TOL and e_t < ei.FP64_TOL
    assert e_p == 0 and e_y < ei.FP64_TOL
    assert (o["achieved"][:, 2] > -np.pi).all() and (o["achieved"][:, 2] <= np.pi).all()


@pytest.mark.parametrize("task", model.TASKS)
def test_fp32_build_against_the_oracle(he, params, task):
    snap, n, (q, v, t, fams, nv), _ = ei.stack()
    o = run_words(he, snap, n, 2, params, task, t, np.float32)
    ratios = tr.compare(task, params, q, v, t, o["obs"], o["reward"], o["terms"], fams, nv, "host fp32, evaluate")
    assert set(ratios) == set(fams)
    # the achieved goal: the position words themselves, the yaw inside pi times the bound of face_direction's angle entry
    ref_a = ei.achieved_reference(q)
    assert np.array_equal(o["achieved"][:, :2].astype(np.float64), q[:, :2])
    yb, h = ei.yaw_bound(params, q, v, t)
    assert (yb / np.pi <= np.where(nv, tr.STRICT_ABS / h, tr.STRICT_ABS)).all()          # (the cap task_reference gives the entry)
    e_y = ei.circular(o["achieved"][:, 2].astype(np.float64) - ref_a[:, 2])
    print("%s fp32: achieved yaw worst err / bound %.3f" % (task, (e_y / yb).max()))
    assert (e_y <= yb).all(), np.nonzero(e_y > yb)[0][:10]


def test_attaining_the_goal_on_the_host(he, params):
    """The achieved goal fed back as the target under face_direction gives a relative angle of zero up to rounding: |obs[15]| within twice
    the entry's bound wherever that bound is inside its cap; at most the near-vertical family is left out (asserted by attained())."""
    snap, n, (q, v, t, fams, nv), _ = ei.stack()
    # the condition on the inputs, on the fp64 goal (tests/test_gpu_evaluate.py relies on it for the device's goal)
    ei.attained(params, q, v, ei.achieved_reference(q), nv)
    goal = run_words(he, snap, n, 2, params, "face_direction", t, np.float32, want=("achieved",))["achieved"]
    limit, kept = ei.attained(params, q, v, goal.astype(np.float64), nv)
    ang = run_words(he, snap, n, 2, params, "face_direction", goal, np.float32, want=("obs",))["obs"][:, ei.ANGLE_ENTRY].astype(np.float64)
    print("attained: %d of %d kept, worst |obs[15]| / limit %.3f" % (kept.sum(), kept.size, (np.abs(ang[kept]) / limit[kept]).max()))
    assert (np.abs(ang[kept]) <= limit[kept]).all()


def test_override_logic(he, params):
    """targets NULL: the stored target is used; targets given: the stored one is ignored; obs has obs_dim(task) columns for every task
    whatever the snapshot's own task was (a snapshot's blocks do not name one)"""
    snap, n, (q, v, t, fams, nv), stored = ei.stack()
    other = ri.pack(q[:n, :], v[:n], np.full((n, 3), 0.3))          # the same states with another stored target
    for task in model.TASKS:
        given = run_words(he, snap, n, 2, params, task, t, np.float32)
        assert given["obs"].shape == (2 * n, model.OBS_DIM[task])
        from_store = run_words(he, snap, n, 2, params, task, None, np.float32)
        as_given = run_words(he, snap, n, 2, params, task, stored, np.float32)
        again = run_words(he, other, n, 1, params, task, t[:n], np.float32)
        for k in KEYS:
            assert np.array_equal(from_store[k].view(np.uint32), as_given[k].view(np.uint32)), (task, k)
            assert np.array_equal(again[k].view(np.uint32), given[k][:n].view(np.uint32)), (task, k)
        # the decoy is a different goal: the task's reward sees it (move_from_origin and move_to_position through P, the others through tpsi)
        assert not np.array_equal(from_store["reward"], given["reward"]), task
        # what does not depend on the target does not move
        assert np.array_equal(from_store["achieved"].view(np.uint32), given["achieved"].view(np.uint32))
        assert np.array_equal(from_store["obs"][:, :15].view(np.uint32), given["obs"][:, :15].view(np.uint32))
        assert np.array_equal(from_store["terms"][:, 3].view(np.uint32), given["terms"][:, 3].view(np.uint32))


def test_stack_and_single_calls_agree_bit_for_bit(he, params):
    snap, n, (q, v, t, fams, nv), _ = ei.stack()
    both = run_words(he, snap, n, 2, params, "move_to_pose", t, np.float32)
    for k in range(2):
        one = run_words(he, snap[k * ri.WORDS * n:(k + 1) * ri.WORDS * n], n, 1, params, "move_to_pose", t[k * n:(k + 1) * n], np.float32)
        for key in KEYS:
            assert np.array_equal(both[key][k * n:(k + 1) * n].view(np.uint32), one[key].view(np.uint32)), (k, key)
    # snapshot 1 is snapshot 0 reversed
    for key in KEYS:
        assert np.array_equal(both[key][n:].view(np.uint32), both[key][:n][::-1].view(np.uint32)), key


def test_new_entry_points_refuse_a_null_handle():
    from jitterbug_amd import _lib, build
    build.build()
    lib = _lib.load()
    for call in (lambda: lib.jb_evaluate_device(None, None, 1, -1, None, None, None, None, None), lambda: lib.jb_evaluate(None, -1, None, None, None, None, None)):
        assert call() == -1 and b"NULL" in lib.jb_last_error()


def test_host_code_under_address_and_undefined_sanitizers():
    """The one sanitizer run of this code: a stand-alone program (its own main, tests/evaluate_harness.cpp -DJBE_MAIN) over ragged sizes,
    the five tasks, all 14 output masks, targets given and stored, and a 3-snapshot stack, on heap blocks of exactly the promised sizes."""
    # (the sanitizer runtimes are linked statically: the program is complete in itself, whatever else the process environment loads)
    exe = build_source(SRC, "evaluate_harness_san", ["-Wall", "-O1", "-g", "-DJBE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = p.stdout.decode("utf-8", "replace")
    assert p.returncode == 0 and "all ok" in text and "MISMATCH" not in text and "runtime error" not in text, text

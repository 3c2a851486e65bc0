"""No-GPU checks of the contact pass (jitterbug_amd/csrc/jb_contacts.hpp): one substep of jb_sim.hpp with a SolveTap plus the per-slot
function ct_slot on the scratch the substep left, compiled for the host in fp32 and fp64 (tests/contacts_harness.cpp: the step kernels'
lane layout with 1 and 4 lane groups, the PAIR instantiation on and off), fed forward_inputs' five families and held to the oracle's
contact lists (tests/contacts_inputs.py has the references and the bounds); the slot map; the NULL-handle answers of the new entry
points; the Python names; and one stand-alone sanitizer run of the host code.

The fp64 build must agree with the oracle to 1e-9 of each block's scale at the very most (asserted: ten times the measured worst): that
separates a wrong frame, a wrong sign or a wrong row from rounding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from jitterbug_amd import model
from tests.build_harness import build_source
from tests import contacts_inputs as ci
from tests import forward_inputs as fi
from tests import readout_inputs as ri

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "contacts_harness.cpp")


@pytest.fixture(scope="module")
def hc():
    lib = C.CDLL(build_source(SRC, "libjb_contacts_host.so", ["-pthread", "-O2", "-fPIC", "-shared"]))
    vp = C.c_void_p
    lib.jbc_run_f32.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.jbc_run_f64.argtypes = lib.jbc_run_f32.argtypes
    lib.jbc_slot_geoms.argtypes = [vp]
    return lib


def run(hc, name, dtype, ngroups, pair=None, snap=None, n=None, n_snaps=1, ctrl=None, present=(1, 1, 1, 1)):
    f = fi.family(name)
    snap = f.snap if snap is None else snap
    n = f.n if n is None else n
    P = np.ascontiguousarray(f.P)
    ctrl = np.ascontiguousarray(f.ctrl if ctrl is None else ctrl, dtype=np.float64)
    m = n * n_snaps
    outs = [np.full((m, ci.NROW, ci.W), np.nan, dtype=dtype), np.full(m, -1, dtype=np.int32), np.full((m, model.NGEOM, 3), np.nan, dtype=dtype), np.full((m, fi.NV), np.nan, dtype=dtype)]
    outs = [o if on else None for o, on in zip(outs, present)]
    un = np.full(m, 255, dtype=np.uint8)
    fn = hc.jbc_run_f32 if dtype == np.float32 else hc.jbc_run_f64
    assert fn(snap.ctypes.data, n, n_snaps, P.ctypes.data, f.n_models, ctrl.ctypes.data, ngroups, f.pair if pair is None else pair,
              *[None if o is None else o.ctypes.data for o in outs], un.ctypes.data) == 0
    return dict((k, o) for k, o in zip(("contact", "ncon", "geom_frc", "qfrc"), outs) if o is not None), un


_runs = {}          # a family's host run, computed once per (precision, lane groups) and left unchanged


def cached_run(hc, name, dtype, ngroups):
    key = (name, np.dtype(dtype).name, ngroups)
    if key not in _runs:
        _runs[key] = run(hc, name, dtype, ngroups)
    return _runs[key]


def test_reference_covers_what_the_issue_says():
    """with the oracle alone: what the families' contact lists hold"""
    r = ci.reference("rollout")
    codes = np.concatenate([c["code"] for c in r.con])
    print("rollout: %d states, at most %d contacts, geoms %d-%d" % (r.n, r.ncon.max(), codes.min(), codes.max()))
    assert r.n == 960 and r.ncon.max() == 9 and codes.min() >= 6 and codes.max() <= 19
    p = ci.reference("poses-moving")
    codes = np.concatenate([c["code"] for c in p.con])
    print("poses-moving: %d states, at most %d contacts, %d distinct geoms" % (p.n, p.ncon.max(), len(set(codes))))
    assert p.n == 64 and p.ncon.max() >= 50 and set(codes) == set(range(model.NGEOM))
    for name, lo in (("mass-touching", model.NGEOM), ("thread-touching", model.NGEOM + 4)):
        codes = np.concatenate([c["code"] for c in ci.reference(name).con])
        assert ((codes >= lo) & (codes < lo + 4)).sum() >= fi.family(name).n // 2, name


def test_slot_map_agrees_with_the_model(hc):
    from jitterbug_amd import _lib, build
    build.build()
    g = ci.slot_geoms()
    h = np.zeros_like(g)
    hc.jbc_slot_geoms(h.ctypes.data)
    assert np.array_equal(g, h) and g.shape == (ci.NROW, 2)
    names = model.GEOM_NAMES
    floor = g[:, 0] < 0
    assert floor.sum() == ci.NROW - 8 and (g[:, 1] >= 0).all() and (g[:, 1] < model.NGEOM).all()
    assert set(g[floor, 1]) == set(range(model.NGEOM)), "every geom can touch the floor"
    for leg in range(model.NLEG):          # ten leg rows per leg: the foot, four points of each cylinder, the knee tip
        rows = g[10 * leg:10 * leg + 10]
        assert (rows[:, 0] == -1).all()
        assert [names[i] for i in rows[:, 1]] == [names[7 + 4 * leg]] + [names[6 + 4 * leg]] * 4 + [names[4 + 4 * leg]] * 4 + [names[5 + 4 * leg]]
        assert names[7 + 4 * leg].startswith("foot") and names[6 + 4 * leg].endswith("lower_cyl") and names[4 + 4 * leg].endswith("upper_cyl") and names[5 + 4 * leg].endswith("_tip")
    body = g[40:66]
    count = {names[i]: int((body[:, 1] == i).sum()) for i in set(body[:, 1])}
    assert count == {"coreBody1": 8, "coreBody2": 8, "screw1": 4, "screw2": 1, "threadMass": 4, "mass": 1} and (body[:, 0] == -1).all()
    pair = g[66:]
    assert sorted(map(tuple, pair)) == sorted([(4 + 4 * leg, other) for leg in range(model.NLEG) for other in (20, 21)])
    assert all(names[a].endswith("upper_cyl") for a in pair[:, 0]) and {names[b] for b in pair[:, 1]} == {"threadMass", "mass"}


@pytest.mark.parametrize("ngroups", (1, 4))
@pytest.mark.parametrize("name", fi.FAMILIES)
def test_fp64_build_is_the_oracle(hc, name, ngroups):
    out, un = cached_run(hc, name, np.float64, ngroups)
    measured = {}
    ci.check(name, out["contact"], out["ncon"], ci.fp64_bounds(name), "fp64, %d lane groups" % ngroups, measured=measured)
    assert not un.any()
    print("%s: the reference's own error of a pair normal %.2e" % (name, ci.reference(name).normal_err))
    for k, v in measured.items():
        assert k == "normal" or v <= ci.FP64_MEASURED[k], "the measured figure written into contacts_inputs.FP64_MEASURED no longer holds: %s %.3e" % (k, v)
    s = ci.sums(name, out["contact"], out["geom_frc"], out["qfrc"])
    mom = s["moment"][np.isfinite(s["moment"])]          # (the states without an active pair row: none in the two touching families)
    print("%s fp64 sums over all env-states: geom_frc %.2e, force %.2e, moment %.2e (%d states without a pair row)" % (
        name, s["geom_frc"].max(), s["force"].max(), mom.max() if mom.size else 0.0, mom.size))
    assert s["geom_frc"].max() <= fi.FP64_BOUND[("qfrc", "force")] and s["force"].max() <= fi.FP64_BOUND[("qfrc", "force")]
    assert (mom.size > 0) == (name not in ("mass-touching", "thread-touching")) and (mom <= fi.FP64_BOUND[("qfrc", "moment")]).all()


@pytest.mark.parametrize("name", fi.FAMILIES)
def test_fp32_build_within_the_fp32_bounds(hc, name):
    measured = {}
    out, un = cached_run(hc, name, np.float32, 4)
    ci.check(name, out["contact"], out["ncon"], ci.FP32_BOUND[name], "fp32, 4 lane groups", measured=measured)
    assert not un.any()
    for k, v in measured.items():
        assert v <= ci.FP32_MEASURED[name][k], "the measured figure written into contacts_inputs.FP32_MEASURED no longer holds: %s %s %.3e" % (name, k, v)
    out1, _ = cached_run(hc, name, np.float32, 1)
    ci.check(name, out1["contact"], out1["ncon"], ci.FP32_BOUND[name], "fp32, main lanes alone")
    for o in (out, out1):
        s = ci.sums(name, o["contact"], o["geom_frc"], o["qfrc"])
        mom = s["moment"][np.isfinite(s["moment"])]
        print("%s fp32 sums over all env-states: geom_frc %.2e, force %.2e, moment %.2e" % (name, s["geom_frc"].max(), s["force"].max(), mom.max() if mom.size else 0.0))
        assert s["geom_frc"].max() <= fi.FP32_BOUND[("qfrc", "force")] and s["force"].max() <= fi.FP32_BOUND[("qfrc", "force")]
        assert (mom <= fi.FP32_BOUND[("qfrc", "moment")]).all()


def test_stack_absent_outputs_and_single_states_agree_bit_for_bit(hc):
    f = fi.family("rollout")
    q, v, t = ri.raw_states("rollout")
    stack = np.concatenate([ri.pack(q[32 * k:32 * k + 32], v[32 * k:32 * k + 32], t[32 * k:32 * k + 32]) for k in range(3)])
    whole, _ = cached_run(hc, "rollout", np.float32, 4)
    got, un = run(hc, "rollout", np.float32, 4, snap=stack, n=32, n_snaps=3, ctrl=f.ctrl[:96])
    assert whole["ncon"][:96].max() >= 4
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), whole[k][:96].view(np.uint32)), k
    assert not un.any()
    only, _ = run(hc, "rollout", np.float32, 4, snap=stack, n=32, n_snaps=3, ctrl=f.ctrl[:96], present=(0, 0, 1, 0))
    assert list(only) == ["geom_frc"] and np.array_equal(only["geom_frc"].view(np.uint32), got["geom_frc"].view(np.uint32))
    one, _ = run(hc, "rollout", np.float32, 4, snap=ri.pack(q[40:41], v[40:41], t[40:41]), n=1, ctrl=f.ctrl[40:41])
    for k in one:
        assert np.array_equal(one[k].view(np.uint32), whole[k][40:41].view(np.uint32)), k


def test_python_names():
    from jitterbug_amd import _lib, jitterbug, trajectory, vec_env
    import inspect
    assert {"jb_contacts_device", "jb_contacts", "jb_contact_slot_geoms", "jb_contact_rows"} <= set(_lib.EXPORTS)
    for name in ("contacts", "contacts_device", "foot_forces"):
        assert callable(getattr(vec_env.JitterbugVecEnv, name))
    assert "snaps_ptr" in inspect.signature(vec_env.JitterbugVecEnv.contacts_device).parameters
    assert "action" in inspect.signature(jitterbug.Physics.contacts).parameters and callable(jitterbug.Physics.contact_force)
    assert inspect.signature(trajectory.record).parameters["contacts"].default is False
    assert model.NCONTACT == ci.NROW and model.CONTACT_WIDTH == ci.W


def test_new_entry_points_refuse_a_null_handle():
    from jitterbug_amd import _lib, build
    build.build()
    lib = _lib.load()
    for call in (lambda: lib.jb_contacts_device(None, None, 1, None, None, None, None, None), lambda: lib.jb_contacts(None, None, None, None, None, None)):
        assert call() == -1 and b"NULL" in lib.jb_last_error()
    lib.jb_contact_slot_geoms(None)          # a NULL table is ignored
    from jitterbug_amd import model, vec_env
    assert lib.jb_contact_rows() == model.NCONTACT and vec_env.JitterbugVecEnv.contact_slot_geoms().shape == (model.NCONTACT, 2)


def test_host_code_under_address_and_undefined_sanitizers():
    """The one sanitizer run of this code: a stand-alone program (its own main, tests/contacts_harness.cpp -DJBC_MAIN) over ragged sizes,
    absent outputs and a 2-snapshot stack of states in floor contact, with and without the PAIR substep, on heap blocks of exactly the
    promised sizes."""
    # (the sanitizer runtimes are linked statically: the program is complete in itself, whatever else the process environment loads)
    exe = build_source(SRC, "contacts_harness_san", ["-pthread", "-O1", "-g", "-DJBC_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode("utf-8", "replace")
    assert p.returncode == 0 and "all ok" in text and "MISMATCH" not in text and "runtime error" not in text, text

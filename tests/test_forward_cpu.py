"""No-GPU checks of the forward-dynamics pass (jitterbug_amd/csrc/jb_forward.hpp): one substep of jb_sim.hpp plus the element function
fw_lane, compiled for the host in fp32 and fp64 (tests/forward_harness.cpp: the step kernels' lane layout with 1 and 4 lane groups, the
PAIR instantiation on and off), fed states packed into the device's block layout and held to the oracle (tests/forward_inputs.py has the
inputs, the references and the bounds); the NULL-handle answers of the new entry points; the Python names; and one stand-alone sanitizer
run of the host code.

The fp64 build must agree with the oracle to 1e-9 of each block's scale at the very most (asserted: ten times the measured worst, which is
1.4e-11): that separates a wrong sign, a wrong frame or a missing h b term from rounding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from jitterbug_amd import model
from tests.build_harness import build_source
from tests import forward_inputs as fi
from tests import readout_inputs as ri

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "forward_harness.cpp")


@pytest.fixture(scope="module")
def hf():
    lib = C.CDLL(build_source(SRC, "libjb_forward_host.so", ["-pthread", "-O2", "-fPIC", "-shared"]))
    vp = C.c_void_p
    lib.jbf_run_f32.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.jbf_run_f64.argtypes = lib.jbf_run_f32.argtypes
    return lib


def run(hf, name, dtype, ngroups, pair=None, snap=None, n=None, n_snaps=1, ctrl=None, present=(1, 1, 1, 1)):
    f = fi.family(name)
    snap = f.snap if snap is None else snap
    n = f.n if n is None else n
    P = np.ascontiguousarray(f.P)
    ctrl = np.ascontiguousarray(f.ctrl if ctrl is None else ctrl, dtype=np.float64)
    outs = [np.full((n * n_snaps,) + s, np.nan, dtype=dtype) if on else None for s, on in zip(((15,), (15,), (10, 6), (3,)), present)]
    un = np.full(n * n_snaps, 255, dtype=np.uint8)
    fn = hf.jbf_run_f32 if dtype == np.float32 else hf.jbf_run_f64
    assert fn(snap.ctypes.data, n, n_snaps, P.ctypes.data, f.n_models, ctrl.ctypes.data, ngroups, f.pair if pair is None else pair,
              *[None if o is None else o.ctypes.data for o in outs], un.ctypes.data) == 0
    return {k: o for k, o in zip(("qacc", "qfrc", "body_acc", "motor"), outs) if o is not None}, un


def test_inputs_meet_their_conditions():
    """with the oracle alone: the caps on excluded env-states, what the families cover, and that the reference for qacc is the one-substep
    velocity difference while forward_debug's own qacc is not"""
    from oracle import oracle as O
    for name in fi.FAMILIES:
        ref, f = fi.reference(name), fi.family(name)
        excluded = int((~ref.strict).sum())
        print("%s: %d env-states, %d excluded (cap %d), smallest margin kept %.3e m, %d in contact, at most %d contacts" % (
            name, ref.n, excluded, fi.EXCLUDED_CAP[name], ref.margin[ref.strict].min(), (ref.ncon > 0).sum(), ref.ncon.max()))
        assert excluded <= fi.EXCLUDED_CAP[name] and 4 * excluded <= ref.n
        assert np.isfinite(ref.qacc).all() and np.isfinite(ref.qfrc).all() and np.isfinite(ref.body_acc()).all()
        assert np.abs(f.ctrl).max() <= 1 and f.ctrl.min() < -0.5 and f.ctrl.max() > 0.5
    r = fi.reference("rollout")
    assert r.n == 960 and (r.ncon > 0).sum() == 779 and r.ncon.max() == 9 and (r.ncon == 0).sum() > 100
    assert fi.reference("poses-moving").ncon.max() >= 50
    for name in ("mass-touching", "thread-touching"):          # the pair contacts are live: the oracle finds more contacts with its geom-geom pairs on
        f = fi.family(name)
        more = sum(O.forward_debug(f.table(j), f.q[j], f.v[j], 0.0)["ncon"] > O.forward_debug(f.table(j), f.q[j], f.v[j], 0.0, O.default_opts(pair_contacts=0))["ncon"] for j in range(f.n))
        print("%s: pair contact live in %d of %d states" % (name, more, f.n))
        assert more >= f.n // 2
    # qacc's reference is (v1 - v0) / h of one oracle substep; forward_debug's qacc field differs from it wherever there are contacts
    f, worst, other = fi.family("rollout"), 0.0, 0.0
    P = f.P
    for j in range(0, 960, 16):
        _, v1 = O.step_physics(P, f.q[j], f.v[j], f.ctrl[j], nsub=1, opts=O.default_opts(pair_contacts=0))
        acc = (v1 - f.v[j]) / P[model.P_TIMESTEP]
        worst = max(worst, np.abs(acc - r.qacc[j]).max() / np.abs(r.qacc[j]).max())
        if r.ncon[j]:
            other = max(other, np.abs(O.forward_debug(P, f.q[j], f.v[j], f.ctrl[j], O.default_opts(pair_contacts=0))["qacc"] - r.qacc[j]).max())
    print("reference qacc against (v1 - v0) / h: %.2e relative; forward_debug's qacc field differs by up to %.2f rad/s^2" % (worst, other))
    assert worst < 1e-8 and other > 1.0


@pytest.mark.parametrize("ngroups", (1, 4))
@pytest.mark.parametrize("name", fi.FAMILIES)
def test_fp64_build_is_the_oracle(hf, name, ngroups):
    out, un = run(hf, name, np.float64, ngroups)
    ref = fi.reference(name)
    fi.check(name, {k: out[k] for k in ("qacc", "qfrc", "motor")}, fi.FP64_BOUND, "fp64, %d lane groups" % ngroups)
    fi.check(name, {"body_acc": out["body_acc"]}, fi.FP64_BOUND_FD, "fp64, %d lane groups, against the finite difference" % ngroups)
    assert not un.any()
    # the ground reaction is the bodies' inertial forces summed: sum_b m_b (a_b - g), from the body_acc the same call returned
    f = fi.family(name)
    mass = np.array([[f.table(j)[model.P_BODY + b * model.BODY_STRIDE + model.B_MASS] for b in range(fi.NB)] for j in range(f.n)])
    grav = np.array([f.table(j)[model.P_GRAVITY:model.P_GRAVITY + 3] for j in range(f.n)])
    total = (mass[:, :, None] * (out["body_acc"][:, :, 0:3] - grav[:, None, :])).sum(1)
    scale = np.abs(ref.My[:, 0:3]).max(1) + fi.BLOCKS[("qfrc", "force")][1]
    err = (np.abs(total - out["qfrc"][:, 0:3]).max(1) / scale).max()
    print("%s: |sum_b m_b (a_b - g) - qfrc[0:3]| / scale = %.2e" % (name, err))
    assert err <= 1e-12


def test_pair_instantiation_without_a_pair_in_reach_is_the_ordinary_one(hf):
    """nominal model, rollout states: the PAIR substep finds no geom-geom contact and gives the ordinary one's answer (fp64: to rounding)"""
    a, _ = run(hf, "rollout", np.float64, 4, pair=0)
    b, _ = run(hf, "rollout", np.float64, 4, pair=1)
    for k in a:
        assert np.abs(a[k] - b[k]).max() <= 1e-9 * max(1.0, np.abs(a[k]).max()), k


@pytest.mark.parametrize("name", fi.FAMILIES)
def test_fp32_build_within_the_fp32_bounds(hf, name):
    measured = {}
    out, un = run(hf, name, np.float32, 4)
    fi.check(name, out, fi.FP32_BOUND, "fp32, 4 lane groups", measured=measured)
    assert not un.any()
    for k, v in measured.items():
        assert v <= fi.FP32_MEASURED[k], "the measured figure written into forward_inputs.FP32_MEASURED no longer holds: %s %.3e" % (k, v)
    out1, _ = run(hf, name, np.float32, 1)
    fi.check(name, out1, fi.FP32_BOUND, "fp32, main lanes alone")


def test_stack_absent_outputs_and_single_states_agree_bit_for_bit(hf):
    f = fi.family("rollout")
    q, v, t = ri.raw_states("rollout")
    stack = np.concatenate([ri.pack(q[32 * k:32 * k + 32], v[32 * k:32 * k + 32], t[32 * k:32 * k + 32]) for k in range(3)])
    whole, _ = run(hf, "rollout", np.float32, 4)
    got, un = run(hf, "rollout", np.float32, 4, snap=stack, n=32, n_snaps=3, ctrl=f.ctrl[:96])
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), whole[k][:96].view(np.uint32)), k
    assert not un.any()
    only, _ = run(hf, "rollout", np.float32, 4, snap=stack, n=32, n_snaps=3, ctrl=f.ctrl[:96], present=(0, 1, 0, 0))
    assert list(only) == ["qfrc"] and np.array_equal(only["qfrc"].view(np.uint32), got["qfrc"].view(np.uint32))
    one, _ = run(hf, "rollout", np.float32, 4, snap=ri.pack(q[40:41], v[40:41], t[40:41]), n=1, ctrl=f.ctrl[40:41])
    for k in one:
        assert np.array_equal(one[k].view(np.uint32), whole[k][40:41].view(np.uint32)), k


def test_python_names():
    from jitterbug_amd import _lib, jitterbug, trajectory, vec_env
    import inspect
    assert {"jb_forward_device", "jb_forward"} <= set(_lib.EXPORTS)
    for name in ("forward", "forward_device", "ground_reaction"):
        assert callable(getattr(vec_env.JitterbugVecEnv, name))
    assert list(inspect.signature(vec_env.JitterbugVecEnv.forward).parameters)[1:] == ["actions", "qacc", "qfrc", "body_acc", "motor"]
    assert "snaps_ptr" in inspect.signature(vec_env.JitterbugVecEnv.forward_device).parameters
    assert "action" in inspect.signature(jitterbug.Physics.forward).parameters
    assert inspect.signature(trajectory.record).parameters["forces"].default is False


def test_new_entry_points_refuse_a_null_handle():
    from jitterbug_amd import _lib, build
    build.build()
    lib = _lib.load()
    for call in (lambda: lib.jb_forward_device(None, None, 1, None, None, None, None, None, None), lambda: lib.jb_forward(None, None, None, None, None, None, None)):
        assert call() == -1 and b"NULL" in lib.jb_last_error()


def test_host_code_under_address_and_undefined_sanitizers():
    """The one sanitizer run of this code: a stand-alone program (its own main, tests/forward_harness.cpp -DJBF_MAIN) over ragged sizes,
    absent outputs and a 3-snapshot stack, with and without the PAIR substep, on heap blocks of exactly the promised sizes."""
    # (the sanitizer runtimes are linked statically: the program is complete in itself, whatever else the process environment loads)
    exe = build_source(SRC, "forward_harness_san", ["-pthread", "-O1", "-g", "-DJBF_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = p.stdout.decode("utf-8", "replace")
    assert p.returncode == 0 and "all ok" in text and "MISMATCH" not in text and "runtime error" not in text, text

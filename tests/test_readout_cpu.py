"""No-GPU checks of the readout pass (jitterbug_amd/csrc/jb_readout.hpp): the element functions the device kernel is made of, compiled for
the host in fp32 and fp64 (tests/readout_harness.cpp), fed states packed into the device's block layout and held to the oracle
(tests/readout_inputs.py has the inputs, the references and the bounds); the NULL-handle answers of the new entry points; the Python
names; and one stand-alone sanitizer run of the host code.

The fp64 build must agree with the oracle to 1e-12 on everything: that separates a wrong formula from rounding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from jitterbug_amd import model
from tests.build_harness import build_source
from tests import readout_inputs as ri

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "readout_harness.cpp")


@pytest.fixture(scope="module")
def hr():
    lib = C.CDLL(build_source(SRC, "libjb_readout_host.so", ["-Wall", "-O2", "-fPIC", "-shared"]))
    vp = C.c_void_p
    lib.jbr_run_f32.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    lib.jbr_run_f64.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    assert lib.jbr_nframe() == model.NFRAME == 33 and lib.jbr_words_per_env() == ri.WORDS
    return lib


def run(hr, name, dtype):
    snap = ri.snapshot(name)
    n = snap.size // ri.WORDS
    P = np.ascontiguousarray(ri.tables(name), dtype=np.float64)
    out = [np.full((n,) + s, np.nan, dtype=dtype) for s in ((ri.NF, 12), (ri.NG,), (ri.NB, 6), (8,))]
    fn = hr.jbr_run_f32 if dtype == np.float32 else hr.jbr_run_f64
    assert fn(snap.ctypes.data, n, 1, P.ctypes.data, 1 if P.ndim == 1 else P.shape[0], *[o.ctypes.data for o in out]) == 0
    return out


def test_inputs_cover_every_geom_and_type_below_the_floor():
    ref = ri.reference("poses")
    below = ref.clear < 0
    assert below.any(axis=0).all(), np.nonzero(~below.any(axis=0))[0]
    assert set(ref.types[0]) == {0, 1, 2, 3}
    assert len(ri.rollout_states()[0]) == 960 and ri.random_models().shape == (8, model.NPARAM)
    assert np.abs(ri.random_models() - model.default_params()).max() > 1e-4          # the models really differ from the nominal one


def test_oracle_clearance_is_its_own_contact_list():
    """the four formulas on oracle.geom_world against the oracle's contacts: the same touching set, and for spheres, cylinders and
    ellipsoids the smallest contact distance (boxes: the set only - the oracle keeps the first four touching vertices, MuJoCo's rule)"""
    worst = 0.0
    for name in ("poses", "rollout", "models"):
        ref = ri.reference(name)
        for j in range(ref.n):
            assert set(np.nonzero(ref.clear[j] < 0)[0].tolist()) == ref.touching[j], (name, j)
            for g, d in ref.con_min[j].items():
                if ref.types[j, g] != model.GEOM_BOX:
                    worst = max(worst, abs(d - ref.clear[j, g]))
    print("worst |clearance - smallest con_dist| = %.2e" % worst)
    assert worst < 1e-15


@pytest.mark.parametrize("name", ri.NAMES)
def test_fp64_build_is_the_oracle(hr, name):
    fr, cl, bv, en = run(hr, name, np.float64)
    ri.reference(name).check(fr, cl, bv, en, rtol=0.0, atol=1e-12, tol_c=1e-12, tol_e=1e-12, label=name + " fp64")


@pytest.mark.parametrize("name", ri.NAMES)
def test_fp32_build_against_the_oracle(hr, name):
    fr, cl, bv, en = run(hr, name, np.float32)
    dev = ri.reference(name).check(fr, cl, bv, en, label=name + " fp32")
    assert dev <= ri.TOL_C_MEASURED, "the measured figure written next to TOL_C no longer holds: %.3e" % dev


def test_stack_and_single_calls_agree_bit_for_bit(hr):
    snap = ri.snapshot("rollout")           # 30 kept steps x 32 envs: a stack of 30 snapshots of 32 envs is NOT the same word order
    q, v, t = ri.raw_states("rollout")
    P = np.ascontiguousarray(ri.tables("rollout"))
    stack = np.concatenate([ri.pack(q[32 * k:32 * k + 32], v[32 * k:32 * k + 32], t[32 * k:32 * k + 32]) for k in range(3)])
    outs = [np.zeros((96,) + s, dtype=np.float32) for s in ((ri.NF, 12), (ri.NG,), (ri.NB, 6), (8,))]
    assert hr.jbr_run_f32(stack.ctypes.data, 32, 3, P.ctypes.data, 1, *[o.ctypes.data for o in outs]) == 0
    whole = run(hr, "rollout", np.float32)
    for a, b in zip(outs, whole):
        assert np.array_equal(a.view(np.uint32), b[:96].view(np.uint32))
    assert snap.size == 960 * ri.WORDS


def test_names():
    assert len(model.GEOM_NAMES) == 22 and len(set(model.GEOM_NAMES)) == 22
    assert model.GEOM_NAMES[:4] == ("coreBody1", "coreBody2", "screw1", "screw2") and model.GEOM_NAMES[20:] == ("threadMass", "mass")
    assert model.GEOM_NAMES[4:8] == ("leg2upper_cyl", "leg2_tip", "leg2lower_cyl", "foot2")
    assert [model.GEOM_NAMES[g] for g in model.FOOT_GEOMS] == ["foot2", "foot3", "foot1", "foot4"]
    types = ri.geom_types(model.default_params())
    assert all(types[g] == model.GEOM_SPHERE for g in model.FOOT_GEOMS)


def test_new_entry_points_refuse_a_null_handle():
    from jitterbug_amd import _lib, build
    build.build()
    lib = _lib.load()
    for call in (lambda: lib.jb_readout_device(None, None, 1, None, None, None, None), lambda: lib.jb_readout(None, None, None, None, None)):
        assert call() == -1 and b"NULL" in lib.jb_last_error()


def test_host_code_under_address_and_undefined_sanitizers():
    """The one sanitizer run of this code: a stand-alone program (its own main, tests/readout_harness.cpp -DJBR_MAIN) over ragged sizes,
    absent outputs and a 3-snapshot stack, on heap blocks of exactly the promised sizes."""
    # (the sanitizer runtimes are linked statically: the program is complete in itself, whatever else the process environment loads)
    exe = build_source(SRC, "readout_harness_san", ["-Wall", "-O1", "-g", "-DJBR_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = p.stdout.decode("utf-8", "replace")
    assert p.returncode == 0 and "all ok" in text and "MISMATCH" not in text and "runtime error" not in text, text

"""No-GPU checks of the inertia pass (jitterbug_amd/csrc/jb_inertia.hpp): the element functions the device kernel is made of, compiled for
the host in fp32 and fp64 (tests/inertia_harness.cpp), fed states packed into the device's block layout and held to the oracle
(tests/inertia_inputs.py has the inputs, the references and the bounds); the NULL-handle answers of the new entry points; and one
stand-alone sanitizer run of the host code.

The fp64 build must agree with the oracle to 1e-12 of every entry's scale: that separates a wrong formula from rounding."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from jitterbug_amd import model
from tests.build_harness import build_source
from tests import inertia_inputs as ii
from tests import readout_inputs as ri

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "inertia_harness.cpp")
SHAPES = ((ii.NV, ii.NV), (3, ii.NV), (ii.NV,), (ii.NJAC, 6, ii.NV))
KEYS = ("qM", "qfrc", "qacc_smooth", "jac")


@pytest.fixture(scope="module")
def hi():
    lib = C.CDLL(build_source(SRC, "libjb_inertia_host.so", ["-Wall", "-O2", "-fPIC", "-shared"]))
    vp = C.c_void_p
    lib.jbi_run_f32.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.jbi_run_f64.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    assert lib.jbi_njac() == ii.NJAC == len(model.JAC_NAMES) and lib.jbi_words_per_env() == ri.WORDS
    return lib


def run_words(hi, snap, n, n_snaps, P, ctrl, dtype):
    P = np.ascontiguousarray(P, dtype=np.float64)
    a = np.ascontiguousarray(ctrl, dtype=dtype)
    out = [np.full((n * n_snaps,) + s, np.nan, dtype=dtype) for s in SHAPES]
    fn = hi.jbi_run_f32 if dtype == np.float32 else hi.jbi_run_f64
    assert fn(snap.ctypes.data, n, n_snaps, P.ctypes.data, 1 if P.ndim == 1 else P.shape[0], a.ctypes.data, *[o.ctypes.data for o in out]) == 0
    return dict(zip(KEYS, out))


def run(hi, name, dtype):
    snap = ri.snapshot(name)
    return run_words(hi, snap, snap.size // ri.WORDS, 1, ri.tables(name), ii.actions(name), dtype)


@pytest.mark.parametrize("name", ii.NAMES)
def test_references_are_the_oracles(name):
    """the numpy restatement behind the Jacobian reference and the bias scale: its Jacobians sum to forward_debug's M, map qvel to the
    readout reference's body velocities, and its bias recursion is the oracle's"""
    ref, rr = ii.reference(name), ri.reference(name)
    q, v, _ = ri.states(name)
    dg = np.sqrt(np.einsum("nii->ni", ref.qM))
    e_m = (np.abs(ref.M_numpy - ref.qM) / (dg[:, :, None] * dg[:, None, :])).max()
    e_v = np.abs(np.einsum("nbrd,nd->nbr", ref.jac[:, :ii.NB], v) - rr.bvel).max()
    sc = ref.qfrc_scale[:, 0]
    assert (ref.bias_numpy[sc == 0] == 0).all() and (ref.qfrc[:, 0][sc == 0] == 0).all()      # (horizontal gravity on a state at rest)
    e_b = (np.abs(ref.bias_numpy - ref.qfrc[:, 0]) / np.where(sc > 0, sc, 1.0)).max()
    print("%s: numpy M %.2e of sqrt(M_ii M_jj), jac @ qvel %.2e, bias %.2e of its scale" % (name, e_m, e_v, e_b))
    assert e_m <= 1e-12 and e_v <= 1e-12 and e_b <= 1e-12
    # the actions reach beyond the ctrlrange on both sides, and the motor hinge has no spring or damper in any table
    assert ii.actions(name).min() < -1 and ii.actions(name).max() > 1
    for P in np.atleast_2d(ri.tables(name)):
        k, b = ii.hinge_kb(P)
        assert k[8] == 0 and b[8] == 0 and (k[:8] > 0).all()


@pytest.mark.parametrize("name", ii.NAMES)
def test_fp64_build_is_the_oracle(hi, name):
    ii.reference(name).check(ii.FP64, label=name + " fp64", **run(hi, name, np.float64))


@pytest.mark.parametrize("name", ii.NAMES)
def test_fp32_build_against_the_oracle(hi, name):
    dev = ii.reference(name).check(ii.FP32, label=name + " fp32", **run(hi, name, np.float32))
    for key, x in dev.items():
        assert x <= ii.MEASURED[key], "the measured figure written next to the bound of %s no longer holds: %.3e" % (key, x)


def test_stack_and_single_calls_agree_bit_for_bit(hi):
    q, v, t = ri.raw_states("rollout")
    P, a = ri.tables("rollout"), ii.actions("rollout").astype(np.float32)
    snaps = [ri.pack(q[32 * k:32 * k + 32], v[32 * k:32 * k + 32], t[32 * k:32 * k + 32]) for k in range(3)]
    stack = run_words(hi, np.concatenate(snaps), 32, 3, P, a[:96], np.float32)
    for k in range(3):
        one = run_words(hi, snaps[k], 32, 1, P, a[32 * k:32 * k + 32], np.float32)
        for key in KEYS:
            assert np.array_equal(stack[key][32 * k:32 * k + 32].view(np.uint32), one[key].view(np.uint32)), (k, key)
    # an env-state alone equals itself in the batch
    j = 37
    alone = run_words(hi, ri.pack(q[j:j + 1], v[j:j + 1], t[j:j + 1]), 1, 1, P, a[j:j + 1], np.float32)
    for key in KEYS:
        assert np.array_equal(alone[key][0].view(np.uint32), stack[key][j].view(np.uint32)), key


@pytest.mark.parametrize("name", ("rollout", "models-moving"))
def test_exact_structure(hi, name):
    o = run(hi, name, np.float32)
    M, f, jac = o["qM"], o["qfrc"], o["jac"]
    assert np.array_equal(M.view(np.uint32), M.transpose(0, 2, 1).view(np.uint32))
    for l in range(4):
        other = [d for d in range(6, 15) if d not in (6 + 2 * l, 7 + 2 * l)]
        assert (M[:, 6 + 2 * l:8 + 2 * l][:, :, other] == 0).all()           # leg-leg and leg-motor blocks
    assert (M[:, 14, 6:14] == 0).all() and (M[:, 6:14, 14] == 0).all()
    assert (M[:, np.arange(15), np.arange(15)] > 0).all()
    assert (f[:, 1, :6] == 0).all() and (f[:, 1, 14] == 0).all() and (f[:, 2, :14] == 0).all()
    assert (f[:, 1, 6:14] != 0).any() and (f[:, 2, 14] != 0).all()
    # columns of dofs outside a block's chain
    chain = {0: [], 9: [14]}
    for l in range(4):
        chain[1 + 2 * l] = [6 + 2 * l]; chain[2 + 2 * l] = chain[10 + l] = [6 + 2 * l, 7 + 2 * l]
    for r in range(ii.NJAC):
        outside = [d for d in range(6, 15) if d not in chain[r]]
        assert (jac[:, r][:, :, outside] == 0).all(), r
        assert (jac[:, r, 0:3, 0:3] == np.eye(3, dtype=np.float32)).all() and (jac[:, r, 3:6, 0:3] == 0).all(), r
        assert (np.abs(jac[:, r][:, 3:6][:, :, chain[r]]).max(axis=1) > 0).all(), r


def test_names():
    assert model.JAC_NAMES[:10] == model.BODY_NAMES and model.JAC_NAMES[10:] == ("foot2", "foot3", "foot1", "foot4")
    assert [model.GEOM_NAMES[g] for g in model.FOOT_GEOMS] == list(model.JAC_NAMES[10:])


def test_new_entry_points_refuse_a_null_handle():
    from jitterbug_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert _lib.NJAC == ii.NJAC
    for call in (lambda: lib.jb_inertia_device(None, None, 1, None, None, None, None, None), lambda: lib.jb_inertia(None, None, None, None, None, None)):
        assert call() == -1 and b"NULL" in lib.jb_last_error()


def test_host_code_under_address_and_undefined_sanitizers():
    """The one sanitizer run of this code: a stand-alone program (its own main, tests/inertia_harness.cpp -DJBI_MAIN) over ragged sizes,
    all 14 output masks and a 3-snapshot stack, on heap blocks of exactly the promised sizes."""
    # (the sanitizer runtimes are linked statically: the program is complete in itself, whatever else the process environment loads)
    exe = build_source(SRC, "inertia_harness_san", ["-Wall", "-O1", "-g", "-DJBI_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    text = p.stdout.decode("utf-8", "replace")
    assert p.returncode == 0 and "all ok" in text and "MISMATCH" not in text and "runtime error" not in text, text

"""The step kernels' source over the whole range of the leg hinges, on the host (no GPU): the reference XML gives the hinges no range, and four
places of the kernel source change their behaviour with the hinge angle - the sine / cosine routine (|th| > 0.9: jb_lane.hpp vsincos_pi, else
jb_sim.hpp sincos_small), the upper-leg floor broad phase (|th1| > 0.3: the all-geom path), the thread pair's broad phase (|th1| > 0.4: run
whatever the builder's flag says) and the builder's flag itself (sampled over |th1| <= 0.4).  The inputs are tests/parity_inputs.py
hinge_range_states: families of states with the hinges uniform in +-H, H = 0.3, 0.85, 1.5, 2.8, pushed into the floor.
Every line below that was measured is written next to what it was measured against (and in profiles/r11_hinge_range.txt)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from jitterbug_amd import augmented_jitterbug as aj, model
from oracle import oracle as O
from tests.parity_inputs import HINGE_FAMILIES, hinge_range_conditions, hinge_range_inputs

dp = C.POINTER(C.c_double)
fp = C.POINTER(C.c_float)
N = 256
ACTION_SEED = 7
# host entry, lane groups, model set (tests/parity_inputs.py hinge_range_inputs) per instantiation of the substep
ENTRIES = {"ordinary": ("jbh_step", 1, "nominal"), "groups4": ("jbh_step_groups", 4, "nominal"), "lean": ("jbh_step_lean", 4, "nominal"),
           "pair": ("jbh_step_pair", 4, "augmented"), "pair_lean": ("jbh_step_pair_lean", 4, "augmented")}
# the GPU variants (tests/test_gpu_hinge_range.py) and the host instantiation that stands for each in fp32
GPU_VARIANTS = {"ordinary": "groups4", "lean": "lean", "pair": "pair", "lean_pair": "pair_lean"}
GPU_FAMILIES = (0.3, 0.85, 1.5)
# seed of hinge_range_inputs per (family, model set) for the GPU parity test, chosen on the CPU: the first of 0..20 at which the fp32 host
# build stays under HALF of each GPU line on every variant of that model set (test_fp32_host_build_stays_inside_half_the_gpu_lines)
GPU_SEEDS = {(0.3, "nominal"): 0, (0.85, "nominal"): 0, (1.5, "nominal"): 2, (0.3, "augmented"): 0, (0.85, "augmented"): 0, (1.5, "augmented"): 6}


def hinge_range_actions(n=N):
    return np.random.default_rng(ACTION_SEED).uniform(-1, 1, size=n)


def _load(path):
    lib = C.CDLL(path)
    lib.jbh_step.argtypes = [dp, dp, dp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    for e in ("jbh_step_groups", "jbh_step_lean", "jbh_step_pair", "jbh_step_pair_lean"):
        getattr(lib, e).argtypes = [dp, dp, dp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    lib.jbh_hinge_sincos_f32.argtypes = [C.c_int, C.c_int, fp, fp, fp]
    lib.jbh_lane_table.argtypes = [dp, C.c_int, dp]
    return lib


@pytest.fixture(scope="module")
def lib():
    import tests.build_harness as bh
    return _load(bh.build())


@pytest.fixture(scope="module")
def lib_wide():
    """the harness with every hinge through vsincos_pi (fp64: libm): no series anywhere in the fp64 build - and with the mass - leg pair's
    narrow phase cold in every substep, as the oracle runs it (see test_fp64_excess_over_round_off_is_the_series_alone)"""
    import tests.build_harness as bh
    return _load(bh.build(defines={"JB_HINGE_SINCOS_WIDE": 1, "JB_PAIR_NARROW_COLD": 1}))


def host_step(lib, name, P, q, v, u, f32=0, nsub=2):
    """one control step of nsub substeps of every state through the host instantiation `name` -> (q, v, failure counters)"""
    entry, groups, _ = ENTRIES[name]
    n = len(q)
    qo, vo, fail = np.array(q, dtype=np.float64), np.array(v, dtype=np.float64), np.zeros(n)
    P = np.asarray(P, dtype=np.float64)
    for i in range(n):
        Pi = np.ascontiguousarray(P[i] if P.ndim == 2 else P)
        f = np.zeros(1)
        a = (Pi.ctypes.data_as(dp), qo[i].ctypes.data_as(dp), vo[i].ctypes.data_as(dp), float(u[i]), nsub, 1, 20)
        if entry == "jbh_step":
            rc = lib.jbh_step(*a, 1, f32, f.ctypes.data_as(dp))
        else:
            rc = getattr(lib, entry)(*a, f32, groups, 1, f.ctypes.data_as(dp))
        assert rc == 0, (name, i, rc)
        fail[i] = f[0]
    return qo, vo, fail


@functools.lru_cache(maxsize=None)
def oracle_step(family, kind, seed=0, nsub=2):
    """the oracle's control step from hinge_range_inputs(family, kind, seed=seed): pair contacts on with the augmented models (the PAIR
    instantiations), off with the nominal one (the others do not simulate the pairs) -> (q, v), computed once"""
    P, q, v, _ = hinge_range_inputs(family, kind, N, seed)
    u = hinge_range_actions()
    o = O.default_opts(pair_contacts=0 if kind == "nominal" else 3)
    out = [O.step_physics(P[i] if P.ndim == 2 else P, q[i], v[i], u[i], nsub, o) for i in range(N)]
    return np.stack([x[0] for x in out]), np.stack([x[1] for x in out])


def velocity_change_error(v0, v_test, v_ref):
    """test_all_geoms_contact_parity's measure: the error of the root's velocity change relative to the largest component of that change"""
    dv_o, dv_g = v_ref - v0, v_test - v0
    return np.abs(dv_g[:, :6] - dv_o[:, :6]) / (np.abs(dv_o[:, :6]).max(axis=1, keepdims=True) + 1e-3)


# ----------------------------------------------------------------------------------------------- the inputs' own conditions
@pytest.mark.parametrize("kind", ["nominal", "augmented"])
@pytest.mark.parametrize("family", HINGE_FAMILIES)
def test_inputs_reach_the_upper_legs_the_bodies_and_both_sides_of_every_switch(family, kind):
    """Conditions of the input, from the oracle's contact lists alone: at n = 256 each family has at least 40 states with a leg on its upper
    part alone, at least 40 with a root-body or motor-body geom on the floor, and hinges on both sides of every switch below its H."""
    seeds = {0} | ({GPU_SEEDS[family, kind]} if family in GPU_FAMILIES else set())
    for seed in sorted(seeds):
        _, q, _, contacts = hinge_range_inputs(family, kind, N, seed)
        upper, body, both = hinge_range_conditions(family, q, contacts)
        print("H = %.2f %s seed %d: upper leg alone %d, root / motor body %d, most contacts %d" % (family, kind, seed, upper, body, max(len(c) for c in contacts)))
        assert upper >= 40 and body >= 40 and both
        assert np.abs(q[:, 7:15]).max() <= family and np.abs(q[:, 7:15]).max() > 0.95 * family


# ----------------------------------------------------------------------------------------------- 2a: fp64 host build = oracle
# max(|dq|, |dv| / (1 + |v|)) of the fp64 host build against the oracle above H = 0.3, where sincos_small<double> is itself a truncated
# series (0.9^13 / 13! = 4e-11 in the sine): measured worst per family over the five instantiations -> line = 4 x that.
FP64_MEASURED = {0.85: 2.03e-9, 1.5: 8.51e-10, 2.8: 1.90e-9}
FP64_LINE = {H: None if m is None else 4 * m for H, m in FP64_MEASURED.items()}


def _fp64_errors(lib, family, name):
    kind = ENTRIES[name][2]
    P, q, v, _ = hinge_range_inputs(family, kind, N, 0)
    qo, vo = oracle_step(family, kind, 0)
    qh, vh, fail = host_step(lib, name, P, q, v, hinge_range_actions())
    assert (fail == 0).all(), (family, name, np.nonzero(fail)[0])
    return np.abs(qh - qo).max(), (np.abs(vh - vo) / (1 + np.abs(vo))).max()


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("family", HINGE_FAMILIES)
def test_fp64_host_build_equals_oracle_on_every_family(lib, family, name):
    """H = 0.3: the lines of test_every_geom_type_fp64_equals_oracle (1e-12 on q, 1e-10 relative on v).  Above: FP64_LINE, 4 x the measured
    worst of the family over the five instantiations against the oracle's step_physics (two substeps, 256 states): H = 0.85 2.03e-9 ->
    8.12e-9, H = 1.5 8.51e-10 -> 3.40e-9, H = 2.8 1.90e-9 -> 7.60e-9 (the PAIR instantiations are the worst of each; the others stay at
    7.9e-10 or below).  All under 1e-8: lines, not findings."""
    eq, ev = _fp64_errors(lib, family, name)
    print("fp64 host [%s] H = %.2f: q %.2e v %.2e" % (name, family, eq, ev))
    if family == 0.3:
        assert eq < 1e-12 and ev < 1e-10
    else:
        assert max(eq, ev) < FP64_LINE[family]


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("family", HINGE_FAMILIES)
def test_fp64_excess_over_round_off_is_the_series_alone(lib_wide, family, name):
    """With libm in place of the series (-DJB_HINGE_SINCOS_WIDE) the fp64 build is held to the H = 0.3 lines on EVERY family and every
    instantiation: what the test above admits beyond 1e-12 is the truncation of sincos_small - and, in the PAIR instantiations, ONE more
    thing, which the same build switches off (-DJB_PAIR_NARROW_COLD): the warm start of the mass - leg narrow phase.
    Measured (q, v; profiles/r11_hinge_range.txt): at most 1.5e-13, 9.3e-11 over the twenty cases (the worst is H = 2.8, ordinary).
    With libm ALONE the ordinary / four-group / LEAN figures are the same and PAIR and PAIR + LEAN miss the line on v: H = 0.85 4.77e-10
    (9.47e-10 in some runs), H = 1.5 up to 1.06e-10.  The cause, followed on H = 0.85 state 97 (two mass - leg contacts, 0.54 and 0.34 mm deep
    on legs of 0.61 mm radius): from the second substep on pair_narrow_warm runs Newton from the previous substep's solution to the ROOT of
    f(t) to 64 ulp, while the cold fixed-count scheme - the oracle's, the contact's definition - on so deep a contact stops short of it
    (O.pair_geometric, fixed counts against exact, on that leg: normal 1.0e-8 and contact point 1.8e-11 m apart, the distance - second
    order in the axis parameter - 1e-18 m; on the shallower contact 1e-12 and 1e-15 m).  One substep with one
    lane group: 6e-15 against the oracle; two substeps: 4.77e-10; two substeps, cold: 1.1e-12 at worst over the family.  Far below fp32's rounding, which is what the
    warm start was sized for.  (The run-to-run spread is the host emulation's own: the main group and its replica are threads that read and
    write the warm slots with no barrier between them, so a four-group run's FIRST substep may start warm from its twin's solution of the
    same substep; the lanes of a wave do that load before that store in lockstep.)"""
    eq, ev = _fp64_errors(lib_wide, family, name)
    print("fp64 host, libm hinges [%s] H = %.2f: q %.2e v %.2e" % (name, family, eq, ev))
    assert eq < 1e-12 and ev < 1e-10


# ----------------------------------------------------------------------------------------------- 2b: the two routines against libm
def _f32_neighbours(x, k=1):
    x = np.float32(x)
    lo = hi = x
    for _ in range(k):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    return [lo, x, hi]


def _grid(lo, hi):
    """2^20 points of [lo, hi] with the ends, +-0, the switch point 0.9 as the kernel holds it and its neighbours, the multiples of pi/4
    and theirs - whatever of these lies inside [lo, hi]"""
    pts = list(np.linspace(lo, hi, 2 ** 20).astype(np.float32)) + [np.float32(lo), np.float32(hi), np.float32(0.0), np.float32(-0.0)]
    for s in (1, -1):
        pts += _f32_neighbours(s * 0.9)
        for k in range(0, 9):
            pts += _f32_neighbours(s * k * math.pi / 4)
    x = np.array(pts, dtype=np.float32)
    return np.ascontiguousarray(x[(x >= np.float32(lo)) & (x <= np.float32(hi))])


def _routine(lib, which, x):
    s, c = np.zeros_like(x), np.zeros_like(x)
    lib.jbh_hinge_sincos_f32(which, len(x), x.ctypes.data_as(fp), s.ctypes.data_as(fp), c.ctypes.data_as(fp))
    return s, c


# Roundings of each routine as its source writes it (every operation once, fp32, result and intermediates of magnitude <= 1):
#   sincos_small sine:   x2 = x*x (1); five Horner levels, a product and a sum each (10); x * (...) (1)                          = 12
#   sincos_small cosine: x2 (1); six Horner levels (12)                                                                          = 13
#   vsincos_pi sine:     two fused reductions r = x - k*hi - k*lo (2); r2 (1); three Horner levels (6); r*r2 (1); *(...) (1); r + (1) = 12
#   vsincos_pi cosine:   reductions (2); r2 (1); five Horner levels (10)                                                          = 13
# (the coefficients a routine holds in fp32 are on chains no longer than these; choosing k = rint(x * 2/pi) is no rounding of the result:
# a neighbouring k only moves r to pi/4 plus a few ulp).  Bound: C * 2^-24 + the series' truncation + what the two-term pi/2 leaves.
ROUNDINGS = {(0, "sin"): 12, (0, "cos"): 13, (1, "sin"): 12, (1, "cos"): 13}
PI2_HI, PI2_LO = 1.57079625129699707031, float(np.float32(7.54978941586159635336e-08))


def _bounds():
    r = math.pi / 4 + 1e-6
    trunc = {(0, "sin"): 0.9 ** 13 / math.factorial(13), (0, "cos"): 0.9 ** 14 / math.factorial(14),
             (1, "sin"): r ** 11 / math.factorial(11), (1, "cos"): r ** 12 / math.factorial(12)}
    reduction = 4 * abs(math.pi / 2 - (PI2_HI + PI2_LO))          # |k| <= 4 on [-2 pi, 2 pi]
    return {k: ROUNDINGS[k] * 2.0 ** -24 + trunc[k] + (reduction if k[0] else 0.0) for k in ROUNDINGS}


def test_hinge_sine_cosine_routines_against_libm(lib):
    """sincos_small<float> on [-0.9, 0.9] and vsincos_pi<float> on [-2 pi, 2 pi] against fp64 libm of the same fp32 argument, inside the
    bound counted above (7.2e-7 / 7.8e-7: 12 or 13 roundings).  Measured on this grid: see the assertion's comment.  The two routines give
    different bits somewhere in [-0.9, 0.9] - otherwise the wave-mate test on the GPU (tests/test_gpu_hinge_range.py) would prove nothing."""
    assert ROUNDINGS == {(0, "sin"): 12, (0, "cos"): 13, (1, "sin"): 12, (1, "cos"): 13}
    bound = _bounds()
    worst = {}
    for which, (lo, hi) in ((0, (-0.9, 0.9)), (1, (-2 * math.pi, 2 * math.pi))):
        x = _grid(lo, hi)
        assert len(x) >= 2 ** 20 + 10
        s, c = _routine(lib, which, x)
        x64 = x.astype(np.float64)
        worst[which, "sin"] = np.abs(s.astype(np.float64) - np.sin(x64)).max()
        worst[which, "cos"] = np.abs(c.astype(np.float64) - np.cos(x64)).max()
    print("hinge sine / cosine against libm: " + ", ".join("%s %s %.2e (bound %.2e)" % (("sincos_small", "vsincos_pi")[k[0]], k[1], worst[k], bound[k]) for k in sorted(worst)))
    for k in worst:
        assert worst[k] <= bound[k], (k, worst[k], bound[k])
    x = _grid(-0.9, 0.9)
    s0, c0 = _routine(lib, 0, x)
    s1, c1 = _routine(lib, 1, x)
    differ = (s0.view(np.uint32) != s1.view(np.uint32)) | (c0.view(np.uint32) != c1.view(np.uint32))
    small = np.abs(x) <= 0.05
    print("the two routines differ in bits at %d of %d angles of [-0.9, 0.9], %d of %d within 0.05 rad" % (differ.sum(), len(x), (differ & small).sum(), small.sum()))
    assert differ.sum() > len(x) // 100 and (differ & small).sum() > small.sum() // 100


# ----------------------------------------------------------------------------------------------- 2c: the builder's thread flag
def test_thread_flag_is_conservative_over_its_whole_envelope(lib):
    """jb_model_build.hpp samples the thread flag at nine shoulder angles with a 1 mm margin; the kernel trusts it for |th1| <= 0.4.  500 models
    at the reference's sigmas and 500 at twice them, every leg, th1 in steps of 0.01 rad over [-0.4, 0.4] (the thread is coaxial with the
    motor: its angle does not matter): wherever the oracle's thread contact reports a negative distance, the leg's flag is set."""
    nlm = lib.jbh_lm_count()
    rng = np.random.RandomState(21)
    models = list(aj.augmented_params(500, seed=31))
    while len(models) < 1000:
        off = aj.draw_offsets(rng, modify_legs=True, sd_legs=2 * aj.SD_LEGS, modify_mass=True, sd_mass_pos=2 * aj.SD_MASS_POS)
        models.append(model.compile_spec(aj.apply_offsets(off, modify_legs=True, modify_mass=True)))
    thetas = np.linspace(-0.4, 0.4, 81)
    tab = np.zeros(nlm)
    closest_unflagged, flagged, touching = np.inf, 0, 0
    for P in models:
        P = np.ascontiguousarray(P, dtype=np.float64)
        q = model.qpos0(P)
        for leg in range(4):
            assert lib.jbh_lane_table(P.ctypes.data_as(dp), leg, tab.ctypes.data_as(dp)) == 0
            flag = tab[nlm - 11 + 1] < 0          # the sign of LM_PE_IS + 1 (the table ends LM_PE_IS (3), LM_PT_C (3), LM_PT_AX (3), LM_PT_R, LM_PT_H)
            flagged += flag
            dmin = np.inf
            for th in thetas:
                q[7 + 2 * leg] = th
                dmin = min(dmin, O.pair_thread_geometric(P, q, leg)[0])
            q[7 + 2 * leg] = 0.0
            touching += dmin < 0
            assert flag or dmin >= 0, (leg, dmin)
            if not flag:
                closest_unflagged = min(closest_unflagged, dmin)
    print("thread flag: %d of 4000 legs flagged, %d touch somewhere in |th1| <= 0.4; smallest oracle distance of an unflagged leg %.3e m" % (flagged, touching, closest_unflagged))
    assert touching >= 3          # (the check is not empty)


# ----------------------------------------------------------------------------------------------- 2d: fp32 host build on the GPU's inputs
@pytest.mark.parametrize("variant", list(GPU_VARIANTS))
@pytest.mark.parametrize("family", GPU_FAMILIES)
def test_fp32_host_build_stays_inside_half_the_gpu_lines(lib, family, variant):
    """The condition of tests/test_gpu_hinge_range.py's parity test: on its inputs (GPU_SEEDS) the kernel source in fp32 on the host - the
    reference arithmetic alone, no GPU - stays under half of each of the GPU's lines (q99 < 1e-4, max < 1e-3 of the velocity change)."""
    name = GPU_VARIANTS[variant]
    kind = ENTRIES[name][2]
    seed = GPU_SEEDS[family, kind]
    P, q, v, _ = hinge_range_inputs(family, kind, N, seed)
    _, vo = oracle_step(family, kind, seed)
    _, vh, fail = host_step(lib, name, P, q, v, hinge_range_actions(), f32=1)
    rel = velocity_change_error(v, vh, vo)
    print("fp32 host [%s] H = %.2f seed %d: q99 %.2e max %.2e, failure counters %d" % (variant, family, seed, np.quantile(rel, 0.99), rel.max(), (fail != 0).sum()))
    assert np.quantile(rel, 0.99) < 0.5e-4 and rel.max() < 0.5e-3
    assert (fail == 0).all()

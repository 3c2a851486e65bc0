"""The step kernels over the whole range of the leg hinges, on the GPU: parity with the oracle on tests/parity_inputs.py's hinge families
(hinges uniform in +-0.3, +-0.85, +-1.5 rad, pushed into the floor), and the bits of an env's wave-mates across each place where the kernel
source changes its behaviour with a hinge angle.  The CPU side - the same inputs through the kernel source on the host, the conditions the
inputs meet, how the seeds were chosen - is tests/test_hinge_range_cpu.py."""
import numpy as np
import pytest

from jitterbug_amd import _lib, augmented_jitterbug as aj, model
from jitterbug_amd.vec_env import JitterbugVecEnv
from oracle import oracle as O
from tests.parity_inputs import LAUNCH_ROWS, ROOT_MOTOR_GEOMS, hinge_range_inputs
from tests.test_hinge_range_cpu import GPU_FAMILIES, GPU_SEEDS, N, hinge_range_actions, oracle_step, velocity_change_error

pytestmark = pytest.mark.gpu

TWO_SUBSTEPS = dict(auto_reset=False, control_timestep=0.0004, time_limit=1000)


def _env(n, variant, epw, params=None, **kw):
    """a handle on the launch row (variant, envs per wave); the PAIR variants get one model per env (`params` [n, NPARAM])"""
    flags = {"ordinary": 0, "pair": _lib.FLAG_PAIR, "lean": _lib.FLAG_LEAN, "lean_pair": _lib.FLAG_LEAN}[variant]
    g = JitterbugVecEnv(n, "move_from_origin", flags=flags, envs_per_wave=epw, params=params if "pair" in variant else None, **TWO_SUBSTEPS, **kw)
    assert g.kernel_variant == variant and g.envs_per_wave == epw, (g.kernel_variant, g.envs_per_wave)
    return g


# ----------------------------------------------------------------------------------------------- 3a: parity against the oracle
@pytest.mark.parametrize("variant", ["ordinary", "lean", "pair", "lean_pair"])
@pytest.mark.parametrize("family", GPU_FAMILIES)
def test_hinge_range_contact_parity(family, variant):
    """256 states of the family (depth 0.2 - 2 mm under the first floor contact; the PAIR variants: one model per env from augmented_params,
    the oracle's pair contacts on), one control step of 2 substeps, test_all_geoms_contact_parity's measure and lines: q99 < 1e-4,
    max < 1e-3 of the velocity change, no contact solve at its cap.  The seed of each input (GPU_SEEDS) is the first of 0..20 at which the
    fp32 HOST build of the kernel source stays under half of each line; no family's depth range had to be narrowed."""
    kind = "augmented" if "pair" in variant else "nominal"
    seed = GPU_SEEDS[family, kind]
    P, q, v, _ = hinge_range_inputs(family, kind, N, seed)
    _, vo = oracle_step(family, kind, seed)
    g = _env(N, variant, 4, params=P)
    g.set_state(q, v, np.zeros((N, 3)))
    g.step(hinge_range_actions())
    _, vg, _ = g.get_state()
    _, _, cap = g.counters()
    g.close()
    rel = velocity_change_error(v, vg, vo)
    print("hinge-range parity [%s] H = %.2f seed %d: median %.2e q99 %.2e max %.2e, caps %d" % (variant, family, seed, np.median(rel), np.quantile(rel, 0.99), rel.max(), int(cap.sum())))
    assert np.quantile(rel, 0.99) < 1e-4 and rel.max() < 1e-3
    assert cap.sum() == 0


# ----------------------------------------------------------------------------------------------- 3b: wave-mates across each switch
N_MATES, TRIGGERED = 17, 5


def _walking_states(per_env_models):
    """17 plain walking states from an oracle rollout (30 control steps of uniform actions), hinges of a few hundredths of a radian"""
    P = aj.augmented_params(N_MATES, seed=3) if per_env_models else model.default_params()
    env = O.OracleEnv(N_MATES, "move_from_origin", P, seed=5, step_limit=10 ** 9, per_env_model=per_env_models)
    env.reset()
    rng = np.random.default_rng(2)
    for _ in range(30):
        env.step(rng.uniform(-1, 1, size=N_MATES), auto_reset=False)
    q, v, _ = env.get_state()
    assert np.abs(q[:, 7:15]).max() < 0.19
    return P, q, v


def _triggers(P, q, v, pair):
    """env 5 with one trigger at a time -> [(name, q)]: a hinge past the sine / cosine switch (1.2 rad), a shoulder past the upper-leg broad
    phase's slack (0.35) and - PAIR kernels - past the thread flag's envelope (0.45), each on every quad position; upside down with a core box in the floor"""
    out = []
    for leg in range(4):
        for name, j, th in (("knee 1.2 rad", 8, 1.2), ("shoulder 0.35 rad", 7, 0.35)) + ((("shoulder 0.45 rad", 7, 0.45),) if pair else ()):
            qt = q.copy()
            qt[TRIGGERED, j + 2 * leg] = th if leg % 2 == 0 else -th
            out.append(("%s, leg %d" % (name, leg), qt))
    qt = q.copy()
    qt[TRIGGERED, 3:7] = (0, 1, 0, 0)
    Pi = P[TRIGGERED] if np.ndim(P) == 2 else P
    lo, hi = -0.1, 0.2
    for _ in range(30):
        qt[TRIGGERED, 2] = mid = 0.5 * (lo + hi)
        if np.isin(O.forward_debug(Pi, qt[TRIGGERED], v[TRIGGERED], 0.0)["con_geom"], ROOT_MOTOR_GEOMS[:4]).any():
            lo = mid
        else:
            hi = mid
    qt[TRIGGERED, 2] = lo - 0.001
    assert np.isin(O.forward_debug(Pi, qt[TRIGGERED], v[TRIGGERED], 0.0)["con_geom"], ROOT_MOTOR_GEOMS[:4]).any()
    out.append(("upside down, a core box 1 mm in the floor", qt))
    return out


def _run(g, q, v, acts):
    """one control step from (q, v), then a fused 3-step launch from (q, v) -> the raw words of [rows and state of the step, of the launch]"""
    n = len(q)
    words = []
    g.set_state(q, v, np.zeros((n, 3)))
    ob, rw, dn, _ = g.step(acts[0])
    qs, vs, _ = g.get_state()
    words += [ob.view(np.uint32), rw.view(np.uint32), dn.astype(np.uint8), qs.view(np.uint64), vs.view(np.uint64)]
    g.set_state(q, v, np.zeros((n, 3)))
    ob, rw, dn = g.rollout(3, acts)
    qs, vs, _ = g.get_state()
    words += [ob.view(np.uint32).transpose(1, 0, 2), rw.view(np.uint32).T, dn.astype(np.uint8).T, qs.view(np.uint64), vs.view(np.uint64)]
    return [np.ascontiguousarray(w) for w in words]          # (every array env-major)


_ONE_PER_WAVE = {}


def _one_per_wave(variant):
    """what every (trigger, env) gives at ONE env per wave, per kernel variant with such a row: (models, states, actions, raw words by
    trigger).  LEAN+PAIR has no row at 1 env per wave: it shares PAIR's inputs and is compared with its own plain batch alone."""
    pair = "pair" in variant
    base = {"ordinary": "ordinary", "lean": "lean", "pair": "pair", "lean_pair": "pair"}[variant]
    if base not in _ONE_PER_WAVE:
        P, q, v = _walking_states(pair)
        acts = np.random.default_rng(11).uniform(-1, 1, size=(3, N_MATES)).astype(np.float32)
        g = _env(N_MATES, base, 1, params=P)
        ref = {name: _run(g, qt, v, acts) for name, qt in [("plain", q)] + _triggers(P, q, v, pair)}
        g.close()
        _ONE_PER_WAVE[base] = (P, q, v, acts, ref)
    return _ONE_PER_WAVE[base]


@pytest.mark.parametrize("variant,epw", LAUNCH_ROWS, ids=["%s-%d" % r for r in LAUNCH_ROWS])
def test_wave_mates_keep_their_bits_across_every_hinge_switch(variant, epw):
    """An env's bits never depend on its wave-mates: 17 walking envs, env 5 given one trigger at a time (a hinge at 1.2 rad: the wide sine /
    cosine routine; a shoulder at 0.35: the all-geom path; at 0.45 on the PAIR kernels: the thread broad phase whatever the flag says;
    upside down with a core box in the floor), on every quad position, one control step and a fused 3-step launch, on every launch row.
    The other 16 envs' rows and state equal, in the raw words, the same batch with env 5 left plain, and all 17 equal the same envs at
    1 env per wave (so env 5 gives the same bits at every envs-per-wave).  Two rows are held to the first comparison alone: LEAN+PAIR has no
    row at 1 env per wave, and the 8-envs-per-wave kernels run two lane groups where the others run four - another summation order, other
    bits by design (tests/test_gpu_parity.py test_edge_cases_batch_sizes_and_layouts), with or without a trigger."""
    P, q, v, acts, ref = _one_per_wave(variant)
    pair = "pair" in variant
    others = np.arange(N_MATES) != TRIGGERED
    g = _env(N_MATES, variant, epw, params=P)
    plain = _run(g, q, v, acts)
    bad = []
    vs_one = variant != "lean_pair" and epw != 8
    if vs_one:
        bad += ["plain batch != 1 env per wave" for a, b in zip(plain, ref["plain"]) if not np.array_equal(a, b)][:1]
    for name, qt in _triggers(P, q, v, pair):
        got = _run(g, qt, v, acts)
        if any(not np.array_equal(a[others], b[others]) for a, b in zip(got, plain)):
            bad.append("%s: wave-mates differ from the plain batch" % name)
        if vs_one and any(not np.array_equal(a, b) for a, b in zip(got, ref[name])):
            bad.append("%s: differs from 1 env per wave" % name)
        assert all(np.isfinite(w.view(np.float32)).all() for w in got[:2])
    g.close()
    print("wave-mates [%s, %d envs per wave]: %d differences %s" % (variant, epw, len(bad), bad))
    assert not bad, bad

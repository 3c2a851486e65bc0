"""Native model compiler / domain randomiser (csrc/jb_model_compile.hpp) against its golden-checked Python
definition: jitterbug_amd.augmented_jitterbug.augment_spec (same draw order as the reference's augment_Jitterbug,
augmented_jitterbug.py:95-267, pinned by tests/golden/augment_golden.json) + jitterbug_amd.model.compile_spec."""
import numpy as np
import pytest

from jitterbug_amd import _lib, model
from jitterbug_amd import augmented_jitterbug as aj
from tests.parity_protocol import MARGIN_TOL, NARROW_RESID_TOL, ParityTally, assert_protocol, free_running, teacher_forced, within

ALL = dict(modify_legs=True, modify_mass=True, modify_coreBody1=True, modify_coreBody2=True, modify_global_density=True, modify_gear=True)
COMBOS = [dict(), dict(modify_legs=True), dict(modify_mass=True), dict(modify_legs=True, modify_mass=True), dict(modify_coreBody1=True, modify_gear=True), ALL]


def _native(off, flags):
    P = np.zeros(model.NPARAM)
    o = None if off is None else np.ascontiguousarray(off, dtype=np.float64)
    assert _lib.load().jb_model_compile_host(_lib.ptr(o), aj.flags_of(**flags), _lib.ptr(P)) == 0
    return P


def _close(a, b):
    return np.abs(a - b) <= 1e-9 * np.abs(b) + 1e-30 + 1e-12 * np.abs(b).max() * 0


def test_offsets_replay_equals_the_reference_ordered_draws():
    """draw_offsets consumes the generator exactly like augment_spec (the golden-checked twin of the reference function), and
    apply_offsets(draw_offsets(rng)) reproduces augment_spec(rng) bit for bit - for every flag combination."""
    for k, flags in enumerate(COMBOS):
        rng = np.random.RandomState(100 + k)
        st = rng.get_state()
        off = aj.draw_offsets(rng, **flags)
        after_draw = rng.normal()
        rng.set_state(st)
        spec = aj.augment_spec(None, rng, **flags)
        assert rng.normal() == after_draw                                # same number of draws consumed
        assert np.array_equal(model.compile_spec(spec), model.compile_spec(aj.apply_offsets(off, **flags)))
        assert off.shape == (aj.NOFFSET,) and (np.count_nonzero(off) > 0) == bool(flags)


def test_native_compiler_equals_python_compile_spec():
    np.testing.assert_allclose(_native(None, {}), model.default_params(), rtol=1e-8, atol=1e-30)       # nominal model (invweight: Cholesky vs inv)
    worst = 0.0
    for k, flags in enumerate(COMBOS):
        rng = np.random.RandomState(7 + k)
        for _ in range(6):
            off = aj.draw_offsets(rng, **flags)
            ref = model.compile_spec(aj.apply_offsets(off, **flags))
            got = _native(off, flags)
            scale = np.abs(ref) + 1e-12 * (np.abs(ref) > 0) + (ref == 0) * 1e-18
            worst = max(worst, (np.abs(got - ref) / scale).max())
    assert worst < 1e-8, worst


def test_mass_clearance_check_against_exact_gjk_sweep():
    """The generator's validity check (can the eccentric mass turn?) is conservative with respect to the oracle's exact GJK sweep,
    and rejects little more than it must."""
    from oracle import oracle as O
    P = aj.augmented_params(700, seed=12)
    sweep = O.mass_sweep_clearance(P, 144)
    assert 0.02 < (sweep <= 0).mean() < 0.06                                  # the reference's sigmas: ~3.6 % cannot turn the mass
    for margin in (0.0, 1e-3):
        ok = np.array([aj.mass_clearance_ok(p, margin) for p in P])
        assert sweep[ok].min() >= margin - 1e-5                                # never accepts a model that comes closer
        assert ((~ok) & (sweep > margin + 3e-4)).sum() == 0                    # never rejects one that clears it by 0.3 mm more
    assert aj.mass_clearance_ok(model.default_params(), 2.5e-3) and not aj.mass_clearance_ok(model.default_params(), 3.2e-3)   # nominal: 2.99 mm
    # host generator with the option: every model clears the margin
    Q = aj.augmented_params(40, seed=3, min_mass_clearance=1e-3)
    assert O.mass_sweep_clearance(Q, 144).min() >= 1e-3 - 1e-5


def test_native_draws_have_the_reference_distributions():
    L = _lib.load()
    cfg = _lib.RandomiseConfig()
    assert L.jb_default_randomise_config(cfg) == 0
    assert (cfg.flags, list(cfg.sd_legs), list(cfg.sd_mass_pos)) == (3, [0.003, 0.003, 0.002], [0.0015, 0.002, 0.001])       # reference :96, :98
    cfg.flags = 63
    n = 20000
    off = np.zeros((n, aj.NOFFSET))
    for i in range(n):
        assert L.jb_model_draw_offsets_host(5, i, 0, cfg, _lib.ptr(off[i])) == 0
    sd = np.array([200.0, 10.0, 80.0] + [0.003, 0.003, 0.002] * 8 + [0.0015, 0.002, 0.001, 0.001])
    z = off / sd
    unclipped = [i for i in range(aj.NOFFSET) if i not in (28, 29)]
    assert np.abs(z[:, unclipped].mean(0)).max() < 4 / np.sqrt(n) and np.abs(z[:, unclipped].std(0) - 1).max() < 0.03
    assert np.abs(np.corrcoef(z[:, unclipped].T) - np.eye(len(unclipped))).max() < 0.04
    assert off[:, 28].min() == -0.001 and off[:, 29].min() == -0.001 and off[:, 28].max() > 0.004          # clipped below only (reference :219-221)
    assert abs((off[:, 28] == -0.001).mean() - 0.3085) < 0.012 and abs((off[:, 29] == -0.001).mean() - 0.1587) < 0.01   # P(N < -sd/2), P(N < -sd)
    # keyed by (seed, env, attempt): reproducible, and every key gives another draw
    a, b, c, d = (np.zeros(aj.NOFFSET) for _ in range(4))
    L.jb_model_draw_offsets_host(5, 17, 0, cfg, _lib.ptr(a)); L.jb_model_draw_offsets_host(5, 17, 0, cfg, _lib.ptr(b))
    L.jb_model_draw_offsets_host(5, 17, 1, cfg, _lib.ptr(c)); L.jb_model_draw_offsets_host(6, 17, 0, cfg, _lib.ptr(d))
    assert np.array_equal(a, b) and np.array_equal(a, off[17]) and not np.array_equal(a, c) and not np.array_equal(a, d)


# ----------------------------------------------------------------------------------------------- on the GPU
@pytest.mark.gpu
def test_device_compiler_matches_python_on_given_offsets_and_steps_like_the_oracle():
    """jb_randomise_models(offsets_in): the DEVICE compiles exactly the tables model.compile_spec derives from the same offsets, and
    the kernel then simulates those N models like the oracle does (teacher-forced)."""
    from jitterbug_amd.vec_env import JitterbugVecEnv
    from oracle import oracle as O
    n = 96
    rng = np.random.RandomState(4)
    flags = dict(modify_legs=True, modify_mass=True, modify_coreBody1=True, modify_gear=True)
    offs = np.stack([aj.draw_offsets(rng, **flags) for _ in range(n)])
    ref = np.stack([model.compile_spec(aj.apply_offsets(o, **flags)) for o in offs])
    env = JitterbugVecEnv(n, "move_to_pose", seed=6, auto_reset=False)
    out = env.randomise_models(offsets=offs, return_offsets=True, **flags)
    assert np.array_equal(out["offsets"], offs) and (out["attempts"] == 1).all()
    np.testing.assert_allclose(out["params"], ref, rtol=1e-8, atol=1e-30)
    o = O.OracleEnv(n, "move_to_pose", ref, seed=6, per_env_model=True)
    np.testing.assert_allclose(env.reset(), o.reset(), rtol=2e-6, atol=2e-6)
    env.close()

    def device_compiled(**extra):          # (the cascade check's second env too: the same device-compiled models)
        e = JitterbugVecEnv(n, "move_to_pose", seed=6, auto_reset=False, **extra)
        e.randomise_models(offsets=offs, **flags)
        return e
    r = teacher_forced("move_to_pose", n, 30, seed=6, params=ref, make_env=device_compiled, action_seed=0)
    print("device-compiled models, 96 envs x 30 steps:", r)
    # the whole protocol.  2880 env-steps: the near-switch cap is 0.3 % plus three binomial spreads of a run this size (3 x 0.07 %) - this
    # test allowed 3 % of the env-steps outside its own 30 nm before
    assert_protocol(r, well_bad=0)


@pytest.mark.gpu
def test_device_randomiser_at_config5_size():
    """BASELINE config 5 (65 536 envs, one model each): generated in HBM in well under a second, reproducible, independent of how the
    batch is split over ranks, with the reference's distributions; with min_mass_clearance every model can turn its mass."""
    import time
    from jitterbug_amd.vec_env import JitterbugVecEnv
    from oracle import oracle as O
    n = 65536
    env = JitterbugVecEnv(n, "move_to_pose", seed=1)
    env.randomise_models(seed=9, return_params=False)                              # warm-up (module load)
    t0 = time.perf_counter()
    out = env.randomise_models(seed=9, return_params=False, return_offsets=True)
    dt = time.perf_counter() - t0
    print("jb_randomise_models: %d models in %.3f s" % (n, dt))
    assert dt < 1.0
    off = out["offsets"]
    sd = np.array([0.003, 0.003, 0.002] * 8 + [0.0015])
    z = off[:, 3:28] / sd
    assert np.abs(z.mean(0)).max() < 0.02 and np.abs(z.std(0) - 1).max() < 0.02 and (off[:, [0, 1, 2, 30]] == 0).all()
    ob = env.reset()
    for _ in range(3):
        ob, rw, dn, _ = env.step(np.full(n, 0.5, dtype=np.float32))
    assert np.isfinite(ob).all()
    env.close()
    # the same global envs from two shards, and again: identical offsets
    lo = 40000
    e2 = JitterbugVecEnv(3000, "move_to_pose", seed=1, env_offset=lo)
    o2 = e2.randomise_models(seed=9, return_offsets=True)
    assert np.array_equal(o2["offsets"], off[lo:lo + 3000])
    # ... and the compiled tables are those of the Python definition
    flags = dict(modify_legs=True, modify_mass=True)
    for i in (0, 1234, 2999):
        np.testing.assert_allclose(o2["params"][i], model.compile_spec(aj.apply_offsets(o2["offsets"][i], **flags)), rtol=1e-8, atol=1e-30)
    # with the validity check: re-draws happen (attempt > 1 for ~14 % of the envs) and every model clears 1 mm
    o3 = e2.randomise_models(seed=9, min_mass_clearance=1e-3, return_offsets=True)
    assert 0.08 < (o3["attempts"] > 1).mean() < 0.25
    same = o3["attempts"] == 1
    assert np.array_equal(o3["offsets"][same], o2["offsets"][same])               # first draws that were fine are kept
    assert O.mass_sweep_clearance(o3["params"], 144).min() >= 1e-3 - 1e-5
    e2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["ordinary", "lean"])
def test_config5_shard_8192_device_models_against_the_oracle(variant):
    """BASELINE configs[4]'s per-GPU shard as it really runs: 8192 envs, one DEVICE-generated model each (every draw kept: 3.6 % of
    the robots touch a front leg with their eccentric mass, simulated by the PAIR kernel), per-env constant tables staged in LDS by 2048 full waves, 200 control steps of the open-loop rollout.  A 64-env subset
    spread over the batch is held against the oracle every step, from the GPU's own pre-step state (teacher-forced the other way
    round) and with the tables the device generated (return_params=True); the whole batch must stay physical."""
    from jitterbug_amd.vec_env import JitterbugVecEnv
    from oracle import oracle as O
    n, steps, task = 8192, 200, "move_to_pose"
    # variant "lean": JB_FLAG_LEAN - with one model per env that is the LEAN + PAIR kernel (two waves per SIMD, only the common path's
    # table entries staged in LDS, the rest read from the env's table in global memory)
    env = JitterbugVecEnv(n, task, seed=3, auto_reset=False, flags=2 if variant == "lean" else 0)
    out = env.randomise_models(seed=77, return_params=True)                  # the reference's distribution, every draw kept
    P = out["params"]
    assert P.shape == (n, model.NPARAM) and (out["attempts"] == 1).all()
    touching = np.nonzero(O.mass_sweep_clearance(P[:2048], 72) <= 1e-9)[0]
    assert len(touching) >= 30                                               # ~3.6 % of the robots cannot turn their mass without touching a leg
    spread = np.setdiff1d(np.linspace(0, n - 1, 60).astype(int), touching)
    idx = np.sort(np.concatenate([touching[:24], spread[:40]]))                # robots that touch plus a spread of the others
    assert len(idx) == 64 and len(np.unique(idx)) == 64
    o = O.OracleEnv(64, task, P[idx], seed=3, per_env_model=True)
    o.reset()
    env.reset()
    rng = np.random.default_rng(12)
    # Three classes of robots in the subset, by how deep the mass ever gets into a leg during THIS rollout (the oracle's own narrow phase
    # on the pre-step states): 0 never touches; 1 touches by less than the leg's radius (a contact MuJoCo's MPR and the geometric
    # narrow phase agree on); 2 deeper (the leg's axis inside the mass: a robot that could not be built).  The north-star tolerance is asserted
    # on all three; the env-steps of class-2 robots in which the overlap IS that deep are the protocol's deep class (the oracle's own flag,
    # OracleEnv.conditioning()), held to the strict line by the tally below, not merely counted.
    LEG_RADIUS = 0.00061          # reference jitterbug.xml:58-100: every leg cylinder has size 0.00061
    depth = np.zeros(64)
    bad = np.zeros((3,), dtype=np.int64); tot_c = np.zeros((3,), dtype=np.int64); ill_c = np.zeros((3,), dtype=np.int64)
    rew_err = np.zeros(3); worst_c = np.zeros(3)
    per_step = []
    tally = ParityTally(64, task, P[idx])

    def account(t, pre, og, rg, oo, ro, o):
        if t % 4 == 0:
            for j, i in enumerate(idx):
                for leg in range(4):
                    okp, dist, _, _ = O.pair_geometric(P[i], pre[0][i], leg)
                    if okp and dist < 0:
                        depth[j] = max(depth[j], -dist)
        cond = o.conditioning()
        # well and deep classes alike - but for the deep env-steps whose narrow phase stops short of its root, which the tally bounds (DEEP_ERROR_CAP)
        held = (cond["switch"] >= MARGIN_TOL) & ~(cond["deep"] & (cond["narrow_resid"] >= NARROW_RESID_TOL))
        err = np.abs(og - oo)          # (fp32 - fp64: taken in fp64)
        w = within(og, oo)
        per_step.append((held.copy(), (~w).sum(1), err.max(1), np.abs(rg - ro), cond["deep"].copy(), cond["switch"] < MARGIN_TOL))
    og = free_running(env, o, idx, steps, lambda t: rng.uniform(-1, 1, size=n), tally=tally, hook=account)
    cls = np.where(depth <= 0, 0, np.where(depth < LEG_RADIUS, 1, 2))
    deep_of_class = np.zeros(3, dtype=np.int64)
    for well, nbad, emax, rerr, deep, near in per_step:
        for c in range(3):
            deep_of_class[c] += (deep & (cls == c)).sum()
            m = (cls == c) & well
            bad[c] += nbad[m].sum(); tot_c[c] += m.sum() * model.OBS_DIM[task]; ill_c[c] += ((cls == c) & near).sum()
            if m.any():
                worst_c[c] = max(worst_c[c], emax[m].max()); rew_err[c] = max(rew_err[c], rerr[m].max())
    sizes = [int((cls == c).sum()) for c in range(3)]
    print("config-5 shard [%s]: robots never touching / touching < leg radius (%.2f mm) / deeper: %s; entries of well-conditioned env-steps outside the tolerance %s of %s; "
          "worst error %s; worst reward error %s; ill-conditioned env-steps %s of %d"
          % (variant, 1e3 * LEG_RADIUS, sizes, bad.tolist(), tot_c.tolist(), ["%.1e" % x for x in worst_c], ["%.1e" % x for x in rew_err], ill_c.tolist(), 64 * steps))
    r = tally.result(env.counters()[2].sum())
    print("config-5 shard [%s], the protocol over the 64 compared envs:" % variant, r, "deep env-steps per robot class", deep_of_class.tolist())
    assert sizes[0] >= 30 and sizes[1] + sizes[2] >= 10, sizes
    # the whole protocol over the subset (12 800 env-steps): well and deep classes on the strict line, near-switch env-steps capped at 0.3 %,
    # bounded and followed into the GPU's next step; `well_bad` as the per-class count below allows (1 + 2)
    assert_protocol(r, well_bad=3)
    # (the robot classes come from the pre-step states of every fourth control step, the deep flag from every substep: nearly all deep env-steps
    #  belong to class-2 robots - measured 818 of 838 -, and those robots have some)
    assert sizes[2] == 0 or deep_of_class[2] > 0, (deep_of_class, sizes)
    # classes 0 and 1: the north-star tolerance on every entry of every well-conditioned env-step (measured: ONE of 196 574 entries outside
    # it, a near-zero entry off by 3.8e-6 absolute - fp32 rounding, no contact switch involved; the largest ABSOLUTE error of any entry,
    # inside the tolerance or not, 4.7e-6 / 1.0e-5 in the two classes), rewards to 1e-5 (measured 6e-7)
    # (why 3e-5 and not round 4's 1e-5: worst_c is the largest ABSOLUTE error of ANY entry, and with the mass pair live a motor-rate entry of
    #  magnitude 0.1-0.8 carries 1e-4 relative = 1e-5 ... 8e-5 legitimately; the tolerance itself is what `bad` counts)
    assert bad[0] + bad[1] <= 1 and max(worst_c[0], worst_c[1]) < 3e-5, (bad, worst_c, sizes)
    assert rew_err[0] < 1e-5 and rew_err[1] < 1e-5, rew_err
    # class 2 (deeper than the leg's radius): its env-steps, the deep ones included (a third of them), hold the tolerance too
    assert bad[2] <= 2 and worst_c[2] < 1e-4 and rew_err[2] < 1e-4, (bad, worst_c, rew_err)
    # env-steps within MARGIN_TOL of a contact switch: capped over the subset by the protocol above (0.3 %); per robot class, three binomial
    # spreads of the class's own number of env-steps on top (the nominal share is 0.15 %)
    for c in range(3):
        m = sizes[c] * steps
        assert m == 0 or ill_c[c] <= 0.003 * m + 3 * np.sqrt(0.0015 * m), (c, ill_c, sizes)
    q, v, _ = env.get_state()
    sc, ep, cap = env.counters()
    assert np.isfinite(og).all() and np.isfinite(q).all() and np.isfinite(v).all()
    assert np.abs(np.linalg.norm(q[:, 3:7], axis=1) - 1).max() < 1e-5 and q[:, 2].min() > 0.005 and q[:, 2].max() < 0.08
    assert (sc == steps).all() and cap.sum() == 0          # every contact solve converged
    env.close()


@pytest.mark.gpu
def test_model_params_of_unfetched_per_env_models_are_rebuilt_not_defaulted():
    """randomise_models(return_params=False) (the default above 8192 envs) leaves the tables on the device; model_params(i) -
    what the Physics accessors read (root COM, target height) - must then be env i's OWN table, rebuilt on the host from the same draws,
    not the nominal model's."""
    from jitterbug_amd.vec_env import JitterbugVecEnv
    n = 300
    a = JitterbugVecEnv(n, "move_to_pose", seed=1, env_offset=5000)
    b = JitterbugVecEnv(n, "move_to_pose", seed=1, env_offset=5000)
    ref = a.randomise_models(seed=21, min_mass_clearance=1e-3, return_params=True)
    out = b.randomise_models(seed=21, min_mass_clearance=1e-3, return_params=False)
    assert np.array_equal(ref["attempts"], out["attempts"]) and (out["attempts"] > 1).any()
    nominal = model.default_params()
    for i in (0, 7, 123, int(np.argmax(out["attempts"])), n - 1):
        np.testing.assert_allclose(b.model_params(i), ref["params"][i], rtol=1e-9, atol=1e-30)
        assert np.abs(b.model_params(i) - nominal).max() > 1e-5
    # a failed call leaves handle and host copy on the model they had
    with pytest.raises(Exception):
        a.randomise_models(seed=21, sd_mass_pos=(0.02, 0.02, 0.02), min_mass_clearance=0.05, return_params=True)      # nothing clears 5 cm
    np.testing.assert_array_equal(a.model_params(3), ref["params"][3])
    ob = a.reset()
    for _ in range(2):
        ob, _, _, _ = a.step(np.zeros(n, dtype=np.float32))
    ob_b = b.reset()
    for _ in range(2):
        ob_b, _, _, _ = b.step(np.zeros(n, dtype=np.float32))
    assert np.array_equal(ob, ob_b)                                        # still the randomised models, bit for bit
    a.close(); b.close()

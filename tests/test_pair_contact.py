"""The one geom-geom contact randomised models need: the eccentric-mass ellipsoid (motor body) against the upper-leg cylinders
(reference: every jitterbug geom has contype = conaffinity = 1, jitterbug.xml:44-107, so MuJoCo collides them; with the reference's
own sigmas, augmented_jitterbug.py:165-241, 3.6 % of the drawn robots cannot turn their mass without touching a front leg).
CPU tests of the oracle side: the narrow phase against MuJoCo's (MPR, restated in oracle/jb_oracle.c) and the contact in the dynamics."""
import numpy as np
import pytest

from jitterbug_amd import model
from oracle import oracle as O
from tests.parity_inputs import conditioning_inputs, mass_touching_models, tiled
from tests.parity_protocol import MARGIN_TOL, NARROW_RESID_TOL, NEAR_SWITCH_CAP, assert_protocol, host_pair_vs_oracle, protocol_message, teacher_forced


@pytest.fixture(scope="module")
def touching():
    return mass_touching_models()


def test_only_the_mass_against_the_front_upper_legs_ever_touches(touching):
    legs = set()
    for P, hits in touching:
        legs |= set(hits)
        # every other geom pair MuJoCo's filters let through keeps its distance over the whole motor revolution
        for phi in np.linspace(0, 2 * np.pi, 25)[:-1]:
            q = model.qpos0(P); q[15] = phi
            for gi in (20, 21):
                for gj in range(4, 20):
                    if gi == 21 and gj in (4, 8, 12, 16):
                        continue
                    assert O.geom_distance(P, q, gi, gj) > 1e-5, (gi, gj)
    assert legs <= {0, 1}           # legs 0 and 1 (XML leg2 / leg3): the two front legs


def test_geometric_contact_is_what_mujocos_mpr_returns_and_is_smooth(touching):
    """pair_geometric (closest points of the cylinder axis and the ellipsoid, minus the radius) against the restated MPR: at MuJoCo's own
    settings (tolerance 1e-6, 50 iterations) MPR returns the geometric contact's depth (median ratio 1.003, 5-95 % band 0.99-1.16) and, in
    a good part of the configurations, its normal to a fraction of a degree - in the others a normal 5-25 degrees away, jumping from one
    configuration to the next; run towards convergence it drifts AWAY from it (so "converged MPR" is not what MuJoCo computes), and
    it is still 1e-3 from its own limit at tolerance 1e-10.  Separated, the gap is the exact GJK distance."""
    ratio, ang, ang_conv, conv_self = [], [], [], []
    for P, hits in touching[:8]:
        for l, lst in hits.items():
            for phi, d in lst[::3]:
                q = model.qpos0(P); q[15] = phi
                ok, dist, n, pos = O.pair_geometric(P, q, l)
                hit, depth, nm, pm = O.pair_mpr(P, q, l)
                if not hit or dist > -2e-5:
                    continue
                ratio.append(depth / -dist)
                ang.append(np.degrees(np.arccos(np.clip(n @ nm, -1, 1))))
                assert np.linalg.norm(pos - pm) < 1.5e-3
                h2, d2, n2, _ = O.pair_mpr(P, q, l, 1e-10, 400)
                h3, d3, n3, _ = O.pair_mpr(P, q, l, 1e-13, 2000)
                ang_conv.append(np.degrees(np.arccos(np.clip(n @ n3, -1, 1))))
                conv_self.append(np.abs(n2 - n3).max())
    # the fixed-count scheme collide() and the HIP kernel run against the same contact by bracketed iterations run to convergence:
    # identical to round-off on every contact shallower than the cylinder radius
    worst_fixed = 0.0
    for P, hits in touching:
        for l, lst in hits.items():
            for phi, d in lst[::2]:
                q = model.qpos0(P); q[15] = phi
                rad = P[model.P_GEOM + (4 + 4 * l) * model.GEOM_STRIDE + 14]
                ok, dist, n, pos = O.pair_geometric(P, q, l)
                ok2, d2, n2, p2 = O.pair_geometric(P, q, l, exact=True)
                if dist > -0.9 * rad:
                    worst_fixed = max(worst_fixed, abs(dist - d2), np.abs(n - n2).max() * 1e-3, np.abs(pos - p2).max())
    assert worst_fixed < 1e-10, worst_fixed
    ratio, ang, ang_conv = np.array(ratio), np.array(ang), np.array(ang_conv)
    print("MPR(1e-6) depth / geometric: median %.4f p5 %.3f p95 %.3f | normal angle median %.2f deg p90 %.1f max %.1f | converged MPR vs geometric: median %.1f deg | MPR(1e-10) vs MPR(1e-13) normal: max %.1e"
          % (np.median(ratio), np.quantile(ratio, .05), np.quantile(ratio, .95), np.median(ang), np.quantile(ang, .9), ang.max(), np.median(ang_conv), max(conv_self)))
    assert len(ratio) > 40
    assert abs(np.median(ratio) - 1) < 0.02 and np.quantile(ratio, .05) > 0.9 and np.quantile(ratio, .95) < 1.3      # (MPR overshoots by up to ~15-25 % when it stops on a slanted portal)
    assert (ang < 1.0).mean() > 0.25 and np.median(ang) < 8.0      # MPR's normal: on the geometric one in a good part of the configurations, 5-25 degrees off in others
    assert np.median(ang_conv) > np.median(ang) and np.median(ang_conv) > 5.0            # the limit MPR heads for is a different point
    assert max(conv_self) > 1e-4                # ... and it is not reached at any affordable tolerance
    # separated: the signed distance is the exact GJK distance, continuous through zero
    P, hits = touching[0]
    l, lst = next(iter(hits.items()))
    phis = np.linspace(lst[0][0] - 0.4, lst[0][0] + 0.05, 40)
    ds = []
    for phi in phis:
        q = model.qpos0(P); q[15] = phi
        ok, dist, n, pos = O.pair_geometric(P, q, l)
        ds.append(dist)
        if dist > 0:
            assert abs(dist - O.geom_distance(P, q, 21, 4 + 4 * l)) < 1e-9
    ds = np.array(ds)
    assert (ds > 0).any() and (ds < 0).any() and np.abs(np.diff(ds, 2)).max() < 2e-5        # smooth through the switch


def _free(P):
    """the model floating far above the floor without gravity: only the geom-geom contact acts"""
    P = P.copy()
    P[model.P_GRAVITY:model.P_GRAVITY + 3] = 0.0
    q = model.qpos0(P); q[2] = 1.0
    return P, q


def test_pair_contact_is_an_internal_force_momentum_is_conserved(touching):
    """J = jac(leg) - jac(mass) along (n, t1, t2): the contact pushes the two bodies apart with equal and opposite forces.  From rest, in
    free flight, with the mass pressed into the leg, the constraint force has no component on the six root dofs (no net force or torque:
    momentum is the integrator's business, as without the contact) and acts on the hit leg's shoulder and the motor only."""
    o = O.default_opts(pair_contacts=1)
    n_checked = 0
    for P0, hits in touching[:6]:
        P, q = _free(P0)
        l, lst = next(iter(hits.items()))
        q[15] = lst[len(lst) // 2][0]                        # the overlapping motor angle
        v = np.zeros(model.NV)
        d = O.forward_debug(P, q, v, 0.8, o)
        assert d["ncon"] >= 1 and (d["con_geom"] >= 22).all() and d["f"].max() > 0
        # generalised constraint force: nothing on the six root dofs (= no net force, no net torque about the root origin: total linear and
        # angular momentum are untouched), equal work on the shoulder of the leg that is hit and on the motor
        qfc = d["qfrc_constraint"]
        assert np.abs(qfc[:6]).max() <= 1e-14 * np.abs(qfc).max() and abs(qfc[6 + 2 * l]) > 0 and abs(qfc[14]) > 0
        assert np.abs(np.delete(qfc, [6 + 2 * l, 14])).max() <= 1e-14 * np.abs(qfc).max()       # ... and on nothing else (the knee is below the contact)
        # the leg is pushed away from the mass, the mass held back: shoulder and motor accelerations differ from the contact-free ones
        d0 = O.forward_debug(P, q, v, 0.8, O.default_opts(pair_contacts=0))
        assert abs(d["qacc"][14] - d0["qacc"][14]) > 1e-3 * abs(d0["qacc"][14]) and abs(d["qacc"][6 + 2 * l] - d0["qacc"][6 + 2 * l]) > 1.0
        n_checked += 1
    assert n_checked >= 4


def test_pair_contact_holds_the_mass_back(touching):
    """With the contact the mass ploughs past the leg with a smaller overlap and loses motor angle doing so (0.3 s at action 0.5);
    without it the mass sweeps through the leg unhindered.  Both solvers of the oracle agree on the contact forces."""
    held = 0
    for P0, hits in touching[:6]:
        res = {}
        for pair in (1, 0):
            o = O.default_opts(pair_contacts=pair)
            q = model.qpos0(P0); v = np.zeros(model.NV)
            worst = 0.0
            for k in range(150):
                q, v = O.step_physics(P0, q, v, 0.5, 10, o)
                for l in hits:
                    worst = max(worst, -O.pair_geometric(P0, q, l)[1])
            assert np.isfinite(q).all() and np.abs(q[7:15]).max() < 0.2
            res[pair] = (worst, q[15])
        assert res[1][0] < res[0][0] and res[1][1] < res[0][1] + 1e-9, res
        held += res[1][1] < res[0][1] - 0.3
    assert held >= 4
    P0, hits = touching[0]
    l = next(iter(hits))
    # the two solvers (dual PGS to convergence, primal Newton) on a touching state
    q = model.qpos0(P0); q[15] = hits[l][len(hits[l]) // 2][0]
    v = np.zeros(model.NV); v[14] = 30.0
    a = O.forward_debug(P0, q, v, 0.5, O.default_opts(pair_contacts=1, solver=1))
    b = O.forward_debug(P0, q, v, 0.5, O.default_opts(pair_contacts=1, solver=0, warmstart=0))
    assert a["ncon"] == b["ncon"] and (a["con_geom"] >= 22).any()
    np.testing.assert_allclose(a["qacc"], b["qacc"], rtol=1e-6, atol=1e-6)
    assert (a["jar"] + a["R"] * a["f"] > -1e-6 * (1 + np.abs(a["aref"]))).all()         # KKT: the active rows sit on their soft constraint


def test_nominal_model_is_untouched_by_the_pair_contact(params):
    """The nominal robot never brings its mass near a leg: switching the pair contact on changes nothing, bit for bit."""
    rng = np.random.default_rng(0)
    q, v = model.qpos0(params), np.zeros(model.NV)
    qa, va, qb, vb = q.copy(), v.copy(), q.copy(), v.copy()
    for k in range(20):
        u = rng.uniform(-1, 1)
        qa, va = O.step_physics(params, qa, va, u, 50, O.default_opts(pair_contacts=1))
        qb, vb = O.step_physics(params, qb, vb, u, 50, O.default_opts(pair_contacts=0))
    assert np.array_equal(qa, qb) and np.array_equal(va, vb)


# ----------------------------------------------------------------------------------------------- what the oracle reports about an env-step
def test_oracle_reports_deep_overlap_and_switch_margin_separately(touching):
    """jbo_stats.margin_min folds two conditions into one number: how close a contact candidate came to switching (the model's one
    discontinuity) and a pair overlap deeper than the leg's radius, which forces it to 0.  OracleEnv.conditioning() reports them apart:
    margins() == where(deep, 0, switch) EXACTLY on every env-step of every input, the per-source parts make up the switch margin, the nominal
    model is never deep, the mass - leg narrow phase's fixed counts leave a residual (`narrow_resid`) only on deep env-steps, and the deep share of each input is the one the GPU tests' bounds were derived from (+- 20 % relative: it is a
    property of the input, and the touching inputs must really exercise the class - a seventh of their env-steps)."""
    for name, task, P, n, seed, steps, actions, deep_share in conditioning_inputs(touching):
        o = O.OracleEnv(n, task, P, seed=seed, per_env_model=P.ndim == 2)
        o.reset()
        rng = np.random.default_rng(seed)
        deep = near = unconv = 0
        for t in range(steps):
            o.step(actions(rng, n), auto_reset=False)
            c = o.conditioning()
            assert np.array_equal(o.margins(), np.where(c["deep"], 0.0, c["switch"])), (name, t)
            assert np.array_equal(c["switch"], np.minimum(c["floor"], np.minimum(c["mass"], c["thread"]))), (name, t)
            assert (c["switch"] > 0).all() and np.isfinite(c["floor"]).all(), (name, t)
            # a deep overlap is an overlap of a pair: that pair was a candidate of the step, at a distance from switching of its own
            assert np.isfinite(np.minimum(c["mass"], c["thread"])[c["deep"]]).all(), (name, t)
            # the narrow phase's fixed counts reach the root on every live contact that is not deep (the residual they leave: 3.6e-9 at most)
            assert (c["narrow_resid"][~c["deep"]] < NARROW_RESID_TOL).all(), (name, t, c["narrow_resid"][~c["deep"]].max())
            unconv += int((c["narrow_resid"] >= NARROW_RESID_TOL).sum())
            deep += int(c["deep"].sum()); near += int((c["switch"] < MARGIN_TOL).sum())
        share = deep / (n * steps)
        print("%-32s deep %.4f of the env-steps (pinned to %.4f), of which with an unconverged narrow phase %d; within 11 nm of a contact switch %.5f" % (name, share, deep_share, unconv, near / (n * steps)))
        if deep_share == 0:
            assert deep == 0, (name, deep)
        else:
            assert 0.8 * deep_share <= share <= 1.2 * deep_share, (name, share, deep_share)
        # the near-switch share is the nominal model's on every input (0.07-0.18 %): what the GPU tests cap at 0.3 %
        assert near <= NEAR_SWITCH_CAP * n * steps, (name, near)


# ----------------------------------------------------------------------------------------------- the kernel source on the host, fp32
@pytest.mark.parametrize("variant", ["pair", "pair_lean"])
def test_host_fp32_pair_kernels_hold_the_strict_line_on_deep_overlaps(touching, variant):
    """The property the GPU tests hold the PAIR kernels to, on the CPU (so that a change of the kernel source meets it before it reaches a GPU):
    on the mass-touching models - 64 envs x 60 control steps of uniform actions, and 64 x 12 with the motor flat out after a 250-step lead-in
    on the oracle (the robots lie on their legs by then) - the fp32 host build is inside the strict tolerance (1e-4 rel + 1e-5 abs) on EVERY
    entry of EVERY env-step of the well and the deep class; every env-step that is not has a switch margin below MARGIN_TOL (a contact
    that switched a substep earlier or later); and the deep class is really there (>= 5 % of the env-steps).  The deep class is where the
    narrow phase looks for the nearest surface point of the leg's axis INSIDE the mass; fp64 host tests cannot see an fp32-only defect there."""
    P = tiled(touching, 64)
    for name, kw in (("uniform", dict(task="move_to_pose", seed=4, steps=60)), ("flat out", dict(task="move_from_origin", seed=5, steps=12, flat_out=True, skip=250))):
        rows, failed = host_pair_vs_oracle(variant, P, **kw)
        switch, deep, strict, worst = rows[:, 2], rows[:, 3] != 0, rows[:, 5], rows[:, 6]
        held = switch >= MARGIN_TOL
        viol = strict > 0
        print("%s, %s: %d env-steps, deep %d, near a switch %d; strict violations %d (largest switch margin of one %.2f nm); worst error held well %.1e deep %.1e"
              % (variant, name, len(rows), (deep & held).sum(), (~held).sum(), viol.sum(), 1e9 * (switch[viol].max() if viol.any() else 0.0),
                 worst[held & ~deep].max(), worst[held & deep].max() if (held & deep).any() else 0.0))
        assert failed == 0
        assert (deep & held).sum() >= 0.05 * len(rows), (name, int((deep & held).sum()), len(rows))
        assert not (viol & held).any(), (name, rows[viol & held])          # well AND deep: nothing outside the strict tolerance
        assert (switch[viol] < MARGIN_TOL).all()                           # (the same statement, as the issue of the parity protocol puts it)


# ----------------------------------------------------------------------------------------------- the HIP path (PAIR kernel variant)
@pytest.mark.gpu
def test_gpu_touching_models_match_the_oracle(touching):
    """One model per env, every one of them a robot whose mass hits a front leg: the PAIR kernel (chosen automatically for per-env
    models) against the oracle, teacher-forced, 300 control steps with the motor driven both ways and 150 with it flat out - the strict parity
    protocol of tests/parity_protocol.py in full, the env-steps with the leg's axis inside the mass (the deep class) held like the others."""
    P = tiled(touching, 64)
    r = teacher_forced("move_to_pose", 64, 300, seed=4, params=P)
    print("touching models, uniform actions:", r)
    # every model here is a robot whose mass hits a leg, 50 of the 64 by more than the leg's radius at some time: 14.6 % of the env-steps are
    # of the DEEP class (jb_oracle.c collide()), held to the strict line like the well class - these are the env-steps in which the pair
    # contact works hardest.  Near a contact switch: 0.20 % (the oracle alone, test_oracle_reports_deep_overlap_and_switch_margin_separately).
    assert r["kernel_variant"] == "pair", r
    assert_protocol(r, well_bad=2, deep_share_min=0.05)
    assert r["frac"] >= 0.999, protocol_message(r)
    r = teacher_forced("move_from_origin", 64, 150, seed=5, params=P, flat_out=True)
    print("touching models, motor flat out:", r)
    # motor flat out, 89 % of the robots lying on their legs, the mass hitting the leg at 150 rad/s: 11.1 % of the env-steps deep.  The same
    # lines as every other run: no entry of a well-conditioned or deep env-step off by 2e-5.
    assert_protocol(r, well_bad=16, worst_well=2e-5, deep_share_min=0.05)
    assert r["frac"] >= 0.998, protocol_message(r)


@pytest.mark.gpu
def test_gpu_pair_contact_is_really_simulated_and_chosen_by_the_model(touching):
    """(i) the contact acts: with it (default for these models) the motor is held back exactly as in the oracle, without it (JB_FLAG_NO_PAIR)
    it is not; (ii) a SHARED table whose mass touches selects the PAIR kernel by itself; (iii) on the nominal model the PAIR kernel, forced
    by JB_FLAG_PAIR, reproduces the ordinary kernel."""
    from jitterbug_amd.vec_env import JitterbugVecEnv
    P0, hits = touching[0]
    n = 8
    res = {}
    for name, flags in (("auto", 0), ("off", 8)):
        g = JitterbugVecEnv(n, "move_from_origin", seed=1, auto_reset=False, random_pose=False, params=P0, flags=flags)
        g.reset()
        for t in range(30):
            g.step(np.full(n, 0.5, dtype=np.float32))
        q, v, _ = g.get_state()
        res[name] = q[0, 15]
        g.close()
    o = O.OracleEnv(1, "move_from_origin", P0, seed=1, random_pose=False)
    o.reset()
    for t in range(30):
        o.step(np.full(1, 0.5), auto_reset=False)
    qo, _, _ = o.get_state()
    print("motor angle after 30 steps: GPU with the contact %.4f, oracle %.4f, GPU without %.4f" % (res["auto"], qo[0, 15], res["off"]))
    assert abs(res["auto"] - qo[0, 15]) < 2e-3 * abs(qo[0, 15]) and abs(res["off"] - qo[0, 15]) > 0.05
    # nominal model: the forced PAIR kernel never finds the mass near a leg
    a = JitterbugVecEnv(64, "move_to_pose", seed=2, flags=4)
    b = JitterbugVecEnv(64, "move_to_pose", seed=2)
    oa, ob = a.reset(), b.reset()
    rng = np.random.default_rng(0)
    worst = 0.0
    for t in range(40):          # both from the same state every step (the ordinary kernel sums the motor / root terms in another order - its aux
        u = rng.uniform(-1, 1, size=64).astype(np.float32)          # bodies - so the two agree to fp32 rounding per step and drift apart open loop)
        q, v, tg = a.get_state()
        a.set_state(q, v, tg); b.set_state(q, v, tg)
        oa, ra, _, _ = a.step(u); ob, rb, _, _ = b.step(u)
        ok = np.abs(oa - ob) <= 1e-4 * np.abs(ob) + 2e-6          # (a bound of its own on purpose: two kernels against each other, a 2e-6 floor - not the protocol's within())
        worst = max(worst, np.abs(oa - ob).max())
        assert ok.mean() > 0.999, (t, ok.mean())
    print("nominal model, PAIR kernel vs ordinary kernel, step by step from common states: max |diff| %.2e" % worst)
    # ... and OPEN LOOP for a few steps: the per-step check re-synchronises the states, so a drift between the two kernels - an
    # asymmetric lane-group bug, say - would slip through it; five steps from one common state must stay together to 1e-3 relative
    q, v, tg = a.get_state()
    a.set_state(q, v, tg); b.set_state(q, v, tg)
    for t in range(5):
        u = rng.uniform(-1, 1, size=64).astype(np.float32)
        oa, _, _, _ = a.step(u); ob, _, _, _ = b.step(u)
    qa, va, _ = a.get_state()
    qb, vb, _ = b.get_state()
    close = np.abs(oa - ob) <= 1e-3 * np.abs(ob) + 1e-4
    print("five open-loop steps: observation entries together %.4f, max |dq| %.2e" % (close.mean(), np.abs(qa[:, :15] - qb[:, :15]).max()))
    assert close.mean() > 0.995 and np.abs(qa[:, :15] - qb[:, :15]).max() < 2e-3, (close.mean(), np.abs(qa[:, :15] - qb[:, :15]).max())
    a.close(); b.close()

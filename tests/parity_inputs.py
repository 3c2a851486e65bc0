"""The model draws and action streams the parity tests and the record runs under tools/ share: robots whose eccentric mass or motor-axis thread
touches a front leg (why: tests/test_pair_contact.py, test_thread_contact.py), the per-env-model GPU tests' inputs.  Not a conftest: plain helpers."""
import numpy as np

from jitterbug_amd import augmented_jitterbug as aj, model
from oracle import oracle as O


# every row of the launch table (jb_variant.hpp STEP_ROWS: the 12 step-kernel instantiations) as (kernel variant, envs per wave)
LAUNCH_ROWS = [(v, epw) for v, epws in (("ordinary", (1, 2, 4, 8)), ("pair", (1, 2, 4, 8)), ("lean", (1, 2, 4)), ("lean_pair", (4,))) for epw in epws]


def mass_touching_models():
    """randomised models whose mass cannot turn freely (exact GJK sweep), with the leg each one hits"""
    Ps = aj.augmented_params(600, seed=123)
    cl = O.mass_sweep_clearance(Ps, 72)
    bad = np.nonzero(cl <= 1e-9)[0]
    assert 10 <= len(bad) <= 60          # ~3.6 % of the reference's draws
    out = []
    for i in bad[:16]:
        hits = {}
        for phi in np.linspace(0, 2 * np.pi, 145)[:-1]:
            q = model.qpos0(Ps[i]); q[15] = phi
            for l in range(4):
                ok, d, n, pos = O.pair_geometric(Ps[i], q, l)
                if ok and d < 0:
                    hits.setdefault(l, []).append((phi, d))
        assert hits, i
        out.append((Ps[i], hits))
    return out


def thread_touching_models(n, seed=0):
    """draws of the reference's distribution whose motor offset is then moved so that the thread overlaps the upper leg of a front leg by a
    few hundredths of a millimetre to half a millimetre at the rest pose (leg 0 or 1 = XML leg2 / leg3, alternating)"""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        off = aj.draw_offsets(rng, modify_legs=True, modify_mass=True)
        leg = len(out) & 1
        sx = 1.0 if leg == 0 else -1.0
        want = -rng.uniform(2e-5, 5e-4)                    # overlap asked for
        lo, hi = 0.0, 1.0                                  # move the motor axis along the line towards that leg's shoulder end
        base = off[27:29].copy()
        target = np.array([sx * 0.0046, 0.0068])
        ok = False
        for it in range(40):
            mid = 0.5 * (lo + hi)
            off[27:29] = base + mid * (target - base)
            P = model.compile_spec(aj.apply_offsets(off, modify_legs=True, modify_mass=True))
            d = O.pair_thread_geometric(P, model.qpos0(P), leg)[0]
            if d > want:
                lo = mid
            else:
                hi = mid
            if abs(d - want) < 2e-6:
                ok = True
                break
        if ok:
            out.append((P, leg, d))
    return out


def tiled(models, n):
    """[n, NPARAM]: the tables of a list of touching models (either kind), repeated over n envs"""
    return np.stack([models[i % len(models)][0] for i in range(n)])


def small_actions(rng, n):
    """The motor held within a few degrees of its rest angle: on the thread-touching robots - their motor axis sits 7 mm nearer a front leg
    than nominal - a turning mass would strike that leg too (by millimetres: the deep-overlap class of tests/test_pair_contact.py); held
    back, the thread is the only geom-geom contact, which is what tests/test_thread_contact.py is about."""
    return rng.uniform(-0.02, 0.02, size=n)


def conditioning_inputs(touching):
    """The inputs the per-env-model GPU tests run, as those tests build them (task, tables, env / action seed, steps, action stream), with the
    share of env-steps whose deep flag the oracle sets - a property of the input alone (measured with the oracle, fp64, no kernel involved).  touching: mass_touching_models()."""
    uniform = lambda rng, n: rng.uniform(-1, 1, size=n)
    flat_out = lambda rng, n: np.ones(n)
    mass, thread = tiled(touching, 64), tiled(thread_touching_models(16, seed=11), 64)
    return [("nominal", "move_to_pose", model.default_params(), 256, 6, 200, uniform, 0.0),
            ("augmented_params(256, seed=5)", "move_to_pose", aj.augmented_params(256, seed=5), 256, 6, 200, uniform, 0.0078),
            ("mass-touching, uniform", "move_to_pose", mass, 64, 4, 300, uniform, 0.146),
            ("mass-touching, flat out", "move_from_origin", mass, 64, 5, 150, flat_out, 0.111),
            ("thread-touching, uniform", "move_to_pose", thread, 64, 4, 150, uniform, 0.0079),
            ("thread-touching, small actions", "move_to_pose", thread, 64, 4, 150, small_actions, 0.0)]

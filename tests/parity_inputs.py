"""The model draws and action streams the parity tests and the record runs under tools/ share: robots whose eccentric mass or motor-axis thread
touches a front leg (why: tests/test_pair_contact.py, test_thread_contact.py), the per-env-model GPU tests' inputs.  Not a conftest: plain helpers."""
import ctypes
import functools

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


HINGE_FAMILIES = (0.3, 0.85, 1.5, 2.8)      # H: leg hinges uniform in +-H rad.  The kernel source switches at 0.3 (all-geom path), 0.4 (thread broad phase) and 0.9 (sine / cosine routine)
HINGE_SWITCHES = (0.3, 0.4, 0.9)
ROOT_MOTOR_GEOMS = (0, 1, 2, 3, 20, 21)
UPPER_LEG_GEOMS = tuple(g + 4 * l for l in range(4) for g in (4, 5))
HINGE_FIRST_GEOMS = (tuple(range(22)), UPPER_LEG_GEOMS, ROOT_MOTOR_GEOMS)      # whose first floor contact state i starts from: by i % 3


def _contact_geoms(P, q, v, opts, dbg):
    """the geoms of the oracle's contacts at a state (O.forward_debug's con_geom, without the rest of its report: this runs ~10^5 times)"""
    O.lib().jbo_forward_debug(O._p(P), O._p(q), O._p(v), 0.0, ctypes.byref(opts), ctypes.byref(dbg))
    return dbg.con_geom[:dbg.ncon]


def _upper_leg_alone(c):
    return any((4 + 4 * l in c or 5 + 4 * l in c) and 6 + 4 * l not in c and 7 + 4 * l not in c for l in range(4))


@functools.lru_cache(maxsize=None)
def hinge_range_inputs(family, kind, n=256, seed=0, depth=(0.0002, 0.002)):
    """hinge_range_states for the two model sets the hinge-range tests use, computed once per process (seconds each): kind "nominal" (one
    table, the oracle's geom-geom pairs off: the kernels without PAIR) or "augmented" (augmented_params(n, seed=5), one model per state,
    pairs on).  -> (P, q, v, contacts); the arrays are shared: do not write to them."""
    P = model.default_params() if kind == "nominal" else aj.augmented_params(n, seed=5)
    q, v, contacts = hinge_range_states(family, n, seed, P, depth=depth, pair_contacts=0 if kind == "nominal" else 3)
    for a in (P, q, v):
        a.setflags(write=False)
    return P, q, v, contacts


def hinge_range_states(family, n, seed, models, depth=(0.0002, 0.002), pair_contacts=3):
    """n states with the leg hinges anywhere in +-family rad, each pushed into the floor: the construction of test_all_geoms_contact_parity
    (uniform quaternion, motor in +-3 rad, its velocity scales, a bisection on the oracle for the height of the first floor contact) and then
    a depth uniform in `depth` below it.  The first contact is any geom's (state i with i % 3 == 0), an upper-leg geom's (1) or a root-body /
    motor-body geom's (2): a foot reaches the floor first in nearly every pose, and the upper legs and the bodies are what the hinge angle
    moves between the kernel's paths.  The poses of class 1 are drawn on the robot's back (within some 20 degrees, not uniformly), and again
    (at most 100 times) until some leg lies on its upper part alone, its lower leg and foot clear of the floor.
    models: one table, or [n, NPARAM] (one per state).  pair_contacts: the oracle's geom-geom pairs (off for the kernels that do not
    simulate them).  -> (q [n, 16], v [n, 15], per state the list of the oracle's contact geoms).
    Conditions (hinge_range_conditions, checked by tests/test_hinge_range_cpu.py with the oracle alone): at n = 256 every family has at
    least 40 states of each of the two kinds, and hinges on both sides of every switch below its H."""
    assert family in HINGE_FAMILIES
    rng = np.random.default_rng([seed, int(round(family * 100))])
    P = np.asarray(models, dtype=np.float64)
    Pi = (lambda i: P[i]) if P.ndim == 2 else (lambda i: P)
    o = O.default_opts(pair_contacts=pair_contacts)
    q = np.stack([model.qpos0(Pi(i)) for i in range(n)])
    v = np.zeros((n, 15))
    contacts, dbg = [], O.Debug()
    for i in range(n):
        below = rng.uniform(depth[0], depth[1])
        Pm, qi, vi, first = np.ascontiguousarray(Pi(i)), q[i], v[i], set(HINGE_FIRST_GEOMS[i % 3])          # (qi, vi: views of the rows)
        for attempt in range(100):
            quat = rng.normal(size=4)
            q[i, 3:7] = quat / np.linalg.norm(quat)
            q[i, 7:15] = rng.uniform(-family, family, size=8)
            q[i, 15] = rng.uniform(-3, 3)
            v[i] = rng.normal(size=15) * np.array([.05] * 3 + [1] * 3 + [1] * 8 + [20])
            if i % 3 == 1:          # on its back, within some 20 degrees and with any twist: the shortest rotation that takes `down` to -ez, then any angle about ez
                down = np.array([0, 0, 1.0]) + 0.35 * rng.normal(size=3)
                down /= np.linalg.norm(down)
                turn = np.array([1 - down[2], -down[1], down[0], 0.0])
                turn /= np.linalg.norm(turn)
                psi = rng.uniform(-np.pi, np.pi)
                cz, sz = np.cos(psi / 2), np.sin(psi / 2)
                q[i, 3:7] = (cz * turn[0] - sz * turn[3], cz * turn[1] - sz * turn[2], cz * turn[2] + sz * turn[1], cz * turn[3] + sz * turn[0])
            lo, hi = -0.1, 0.2
            for _ in range(30):          # the height at which the first floor contact (of the state's class) appears
                q[i, 2] = mid = 0.5 * (lo + hi)
                if first.intersection(_contact_geoms(Pm, qi, vi, o, dbg)):
                    lo = mid
                else:
                    hi = mid
            q[i, 2] = lo - below
            c = _contact_geoms(Pm, qi, vi, o, dbg)
            if i % 3 != 1 or _upper_leg_alone(c):
                break
        contacts.append(c)
    return q, v, contacts


def hinge_range_conditions(family, q, contacts):
    """What hinge_range_states' doc promises of a family at n = 256, from the oracle's contact lists alone: (states with an upper-leg cylinder
    or knee tip (geoms 4+4l, 5+4l) on the floor and no lower-leg or foot geom (6+4l, 7+4l) of that leg, states with a root-body or
    motor-body geom on the floor, hinges on both sides of every switch below the family's H)."""
    upper_only = sum(_upper_leg_alone(c) for c in contacts)
    root_motor = sum(any(g in ROOT_MOTOR_GEOMS for g in c) for c in contacts)
    a = np.abs(q[:, 7:15])
    both_sides = all((a < s).any() and (a > s).any() for s in HINGE_SWITCHES if s < family)
    return upper_only, root_motor, both_sides


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

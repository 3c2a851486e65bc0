"""Inputs, fp64 references and bounds of the contact-pass tests (tests/test_contacts_cpu.py, tests/test_gpu_contacts*.py) - not a test module.

The inputs are tests/forward_inputs.py's five families as they are (states, tables, controls, the strict set and its caps).  The reference is
the oracle's contact list, oracle.forward_debug with the family's pair option: per contact its geom code, position, distance and four edge
forces f, from which
    fn = f0 + f1 + f2 + f3,   |force|^2 = fn^2 + mu^2 (f0 - f1)^2 + mu^2 (f2 - f3)^2,   mu = friction sqrt(1 / impratio),
and for a floor contact the world force (-mu (f2 - f3), mu (f0 - f1), fn) - the oracle's floor frame is y = (0, 1, 0), z = (-1, 0, 0).  The
oracle's Debug does not carry a pair contact's normal: a pair row is held by fn, |force|, dist, pos, |normal| = 1 and force . normal = fn, and
its normal by oracle.pair_geometric (the mass: the oracle's runs from the mass to the leg, the pass's from geom1 = the leg's cylinder to the mass)
and oracle.pair_thread_geometric (leg -> thread).  Rows are matched to oracle contacts by geom and nearest position, never by order.

Errors per env-state: forces (fn, force) over the env-state's largest fn plus a thousandth of the robot's weight; positions over 1 m;
distances over the env-state's largest |dist| plus 1 um; normals absolute; the two sums (floor forces, their moment about the root origin)
over forward_inputs' scale of qfrc_constraint, the largest inertial term |M y| of the block plus its floor."""
import functools

import numpy as np

from jitterbug_amd import model
from oracle import oracle as O
from tests import forward_inputs as fi

FAMILIES = fi.FAMILIES
NROW, W = model.NCONTACT, model.CONTACT_WIDTH          # (slot_geoms() holds them against the library's own count)
WEIGHT_FLOOR = 1.72e-4          # N: a thousandth of the robot's weight
DIST_FLOOR = 1e-6               # m
BLOCKS = ("pos", "dist", "fn", "force", "normal")

# ---- bounds.  fp64 host build against the oracle: the worst error over all families and both lane layouts (1 and 4 groups), measured by
# tests/test_contacts_cpu.py (it prints every figure); asserted: ten times it.  Above 1e-9 an error is a formula's, not rounding.
# (the worst are models-moving / mass-touching states; on rollout fn and force are within 6e-14, dist within 1.1e-12 - it is solved from the
#  row's reference acceleration, jb_contacts.hpp)
FP64_MEASURED = {"pos": 2.2e-12, "dist": 1.1e-12, "fn": 6.2e-12, "force": 6.0e-12}
# A pair row's normal is held against oracle.pair_geometric / pair_thread_geometric, whose fixed iteration counts are the contact's
# definition but stop where they stop: the reference's own error is its distance from the same contact iterated to convergence
# (Reference.normal_err: 1.2e-9 for the mass, 7.1e-8 for the thread's bisection on these families), and the bound is that plus 1e-9.  Measured: 1.2e-9 (mass-touching).
FP64_NORMAL_ROUNDING = 1e-9
# fp32 host build (4 lane groups, the device's layout), per block and family; asserted - on the host AND on the GPU - three times it (the
# project's allowance for the device contracting multiply-adds differently from g++ -O2).  A floor row's normal is (0, 0, 1) exactly.
FP32_MEASURED = {
    "rollout": {"pos": 1.2e-8, "dist": 2.3e-4, "fn": 3.8e-5, "force": 4.2e-5, "normal": 1e-15},
    "poses-moving": {"pos": 6.2e-8, "dist": 9.4e-7, "fn": 1.5e-4, "force": 1.5e-4, "normal": 1e-15},
    "models-moving": {"pos": 4.1e-8, "dist": 6.1e-7, "fn": 3.2e-5, "force": 3.2e-5, "normal": 3.7e-7},
    "mass-touching": {"pos": 3.8e-9, "dist": 3.0e-5, "fn": 3.0e-6, "force": 3.0e-6, "normal": 2.1e-7},
    "thread-touching": {"pos": 2.9e-9, "dist": 3.2e-6, "fn": 5.7e-6, "force": 5.7e-6, "normal": 8.0e-7},
}
# Measured on the MI355X (tests/test_gpu_contacts.py prints every figure), rollout / poses-moving / models-moving / mass-touching /
# thread-touching: pos 9.2e-9 / 6.1e-8 / 4.0e-8 / 4.3e-9 / 2.8e-9, dist 3.1e-5 / 9.9e-7 / 3.2e-7 / 5.4e-5 / 3.1e-6, fn 3.1e-5 / 6.9e-5 /
# 2.3e-5 / 1.9e-6 / 4.5e-6, force 3.1e-5 / 6.9e-5 / 2.3e-5 / 2.0e-6 / 4.6e-6, pair normal - / - / 3.5e-7 / 2.0e-7 / 1.0e-6: every block
# inside three times the host's figure; the closest are mass-touching's dist (1.8 x) and thread-touching's normal (1.3 x).
# ---- the sum checks (geom_frc against its rows, the floor rows' total against qfrc[0:3], their moment against qfrc[3:6]) compare the pass
# with the forward pass's inverse dynamics, so they are held to THAT quantity's bounds and scale - forward_inputs' FP64_BOUND / FP32_BOUND
# of ("qfrc", "force") and ("qfrc", "moment") over the block's largest |M y| plus its floor - not to the per-contact blocks above: the
# difference is dominated by qfrc's cancellation error, which a bound scaled by one env-state's largest fn does not describe.
FP64_BOUND = {k: 10 * v for k, v in FP64_MEASURED.items()}
FP32_BOUND = {name: {k: 3 * v for k, v in d.items()} for name, d in FP32_MEASURED.items()}
assert max(FP64_MEASURED.values()) <= 1e-9


def fp64_bounds(name):
    """FP64_BOUND and the pair normal's bound for family `name`: rounding plus the reference's own error"""
    return dict(FP64_BOUND, normal=FP64_NORMAL_ROUNDING + reference(name).normal_err)


def mu_of(P):
    return P[model.P_FRICTION] * np.sqrt(1.0 / P[model.P_IMPRATIO])


def slot_code(g1, g2):
    """the oracle's con_geom code of a row's (geom1, geom2): the geom for a floor contact, 22 + leg for the mass pair, 26 + leg for the thread's"""
    if g1 < 0:
        return g2
    return (model.NGEOM if g2 == 21 else model.NGEOM + 4) + (g1 - 4) // 4


class Reference:
    """the oracle's contact lists of a family, computed once and left unchanged"""

    def __init__(self, fam):
        self.n, self._fam = fam.n, fam
        opts = O.default_opts() if fam.pair else O.default_opts(pair_contacts=0)
        self.con = []           # per env-state: dict(code [c], pos [c,3], dist [c], fn [c], fabs [c], force [c,3] (floor rows; nan otherwise), normal [c,3] (pair rows; nan otherwise))
        self.ncon = np.zeros(fam.n, dtype=int)
        self.total = np.zeros((fam.n, 3))
        self.normal_err = 0.0   # the pair normals' own error: the fixed iteration counts against the same contact iterated to convergence
        for j in range(fam.n):
            P, q, v, u = fam.table(j), fam.q[j], fam.v[j], float(fam.ctrl[j])
            d = O.forward_debug(P, q, v, u, opts)
            c, mu = d["ncon"], mu_of(P)
            f = d["f"].reshape(c, 4)
            fn, t1, t2 = f.sum(1), mu * (f[:, 0] - f[:, 1]), mu * (f[:, 2] - f[:, 3])
            code = d["con_geom"].astype(int)
            force = np.stack([-t2, t1, fn], axis=1)
            force[code >= model.NGEOM] = np.nan
            normal = np.full((c, 3), np.nan)
            for i in np.nonzero(code >= model.NGEOM)[0]:
                if code[i] < model.NGEOM + 4:
                    ok, _, nrm, _ = O.pair_geometric(P, q, code[i] - model.NGEOM)
                    assert ok
                    normal[i] = -nrm
                    exact = O.pair_geometric(P, q, code[i] - model.NGEOM, exact=True)[2]
                else:
                    _, nrm, _, _ = O.pair_thread_geometric(P, q, code[i] - model.NGEOM - 4)
                    normal[i] = nrm
                    exact = O.pair_thread_geometric(P, q, code[i] - model.NGEOM - 4, steps=200)[1]
                if fi.reference(fam.name).strict[j]:
                    self.normal_err = max(self.normal_err, float(np.abs(nrm - exact).max()))
            self.con.append(dict(code=code, pos=d["con_pos"], dist=d["con_dist"], fn=fn, fabs=np.sqrt(fn * fn + t1 * t1 + t2 * t2), force=force, normal=normal))
            self.ncon[j] = c
            self.total[j] = np.nansum(force, axis=0)
            # the identity the sum checks lean on holds in the reference
            assert np.abs(self.total[j] - d["qfrc_constraint"][0:3]).max() <= 1e-12 * max(1.0, np.abs(d["qfrc_constraint"][0:3]).max())


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(fi.family(name))


@functools.lru_cache(maxsize=None)
def slot_geoms(lib_path=None):
    """[NROW, 2] (geom1, geom2) of every row, from the library (jb_contact_slot_geoms needs no GPU)"""
    from jitterbug_amd import _lib, build
    build.build()
    assert _lib.load().jb_contact_rows() == NROW == 74
    out = np.zeros((NROW, 2), dtype=np.int32)
    _lib.load().jb_contact_slot_geoms(out.ctypes.data)
    out.setflags(write=False)
    return out


def compare(name, contact, ncon, idx=None):
    """contact [n, NROW, W], ncon [n] of family `name` (states idx, default all) against the oracle's lists.
    -> (errors {block: [n]}, mismatches: the env-states whose active set or ncon is not the oracle's)"""
    ref, geoms = reference(name), slot_geoms()
    idx = np.arange(ref.n) if idx is None else np.asarray(idx).reshape(-1)
    contact = np.asarray(contact, dtype=np.float64).reshape(len(idx), NROW, W)
    codes = np.array([slot_code(g1, g2) for g1, g2 in geoms])
    err = {b: np.zeros(len(idx)) for b in BLOCKS}
    mismatch = []
    for i, j in enumerate(idx):
        c, rows = ref.con[j], contact[i]
        act = np.nonzero(rows[:, 11] != 0)[0]
        assert np.all(rows[rows[:, 11] == 0] == 0), (name, j, "an inactive row is all zeros")
        assert np.all(rows[act, 11] == 1.0) and np.all(rows[act, 10] >= 0)
        if sorted(codes[act]) != sorted(c["code"]) or int(ncon[i]) != len(c["code"]) or int(ncon[i]) != len(act):
            mismatch.append(int(j))
            continue
        if not len(act):
            continue
        fscale, dscale = c["fn"].max() + WEIGHT_FLOOR, np.abs(c["dist"]).max() + DIST_FLOOR
        left = list(range(len(c["code"])))
        for r in act:
            cand = [k for k in left if c["code"][k] == codes[r]]
            k = min(cand, key=lambda k: np.abs(c["pos"][k] - rows[r, 0:3]).max())
            left.remove(k)
            pos, nrm, frc, dist, fn = rows[r, 0:3], rows[r, 3:6], rows[r, 6:9], rows[r, 9], rows[r, 10]
            err["pos"][i] = max(err["pos"][i], np.abs(pos - c["pos"][k]).max())
            err["dist"][i] = max(err["dist"][i], abs(dist - c["dist"][k]) / dscale)
            err["fn"][i] = max(err["fn"][i], abs(fn - c["fn"][k]) / fscale)
            if codes[r] < model.NGEOM:
                e_f, e_n = np.abs(frc - c["force"][k]).max(), np.abs(nrm - (0, 0, 1)).max()
            else:
                e_f = max(abs(np.linalg.norm(frc) - c["fabs"][k]), abs(frc @ nrm - fn))
                e_n = max(abs(np.linalg.norm(nrm) - 1.0), np.abs(nrm - c["normal"][k]).max())
            err["force"][i] = max(err["force"][i], e_f / fscale)
            err["normal"][i] = max(err["normal"][i], e_n)
    return err, mismatch


def check(name, contact, ncon, bounds, label, idx=None, measured=None):
    """every strict env-state: the oracle's active set and ncon, every block within `bounds` {block: bound}.  Prints each figure before it
    asserts.  measured (a dict): takes the worst figure per block (max with what it holds)."""
    fref = fi.reference(name)
    strict = fref.strict if idx is None else fref.strict[np.asarray(idx).reshape(-1)]
    ids = np.arange(fref.n) if idx is None else np.asarray(idx).reshape(-1)
    assert np.isfinite(np.asarray(contact, dtype=np.float64)).all(), (label, name)
    err, mismatch = compare(name, contact, ncon, idx)
    bad_sets = [j for j in mismatch if fref.strict[j]]
    print("%s %s: active set differs from the oracle's in %d strict env-states %s and %d excluded ones" % (label, name, len(bad_sets), bad_sets[:8], len(mismatch) - len(bad_sets)))
    bad = []
    for b in BLOCKS:
        worst = err[b][strict].max() if strict.any() else 0.0
        print("%s %s %s: worst %.3e over %d strict env-states (bound %.3e); over the %d excluded %.3e" % (
            label, name, b, worst, strict.sum(), bounds.get(b, np.nan), (~strict).sum(), err[b][~strict].max() if (~strict).any() else 0.0))
        if b not in bounds:
            continue
        if measured is not None:
            measured[b] = max(measured.get(b, 0.0), worst)
        if not worst <= bounds[b]:
            bad.append((b, worst, int(ids[strict][err[b][strict].argmax()])))
    assert not bad_sets and not bad, (label, name, bad_sets[:8], bad)


def sums(name, contact, geom_frc, qfrc, idx=None):
    """on all env-states -> {"geom_frc" | "force" | "moment": [n] error over forward_inputs' qfrc scale}: geom_frc against the sum of its
    rows, the floor rows' total force against qfrc[0:3], R^T sum (pos - root) x force against qfrc[3:6] (nan where a pair row is active)"""
    fam, fref, geoms = fi.family(name), fi.reference(name), slot_geoms()
    idx = np.arange(fam.n) if idx is None else np.asarray(idx).reshape(-1)
    contact = np.asarray(contact, dtype=np.float64).reshape(len(idx), NROW, W)
    geom_frc = np.asarray(geom_frc, dtype=np.float64).reshape(len(idx), model.NGEOM, 3)
    qfrc = np.asarray(qfrc, dtype=np.float64).reshape(len(idx), fi.NV)
    floor = geoms[:, 0] < 0
    per_geom = np.zeros_like(geom_frc)
    for g in range(model.NGEOM):
        per_geom[:, g] = contact[:, floor & (geoms[:, 1] == g), 6:9].sum(1)
    fscale = np.abs(fref.My[idx, 0:3]).max(1) + fi.BLOCKS[("qfrc", "force")][1]
    mscale = np.abs(fref.My[idx, 3:6]).max(1) + fi.BLOCKS[("qfrc", "moment")][1]
    total = contact[:, floor, 6:9].sum(1)
    out = {"geom_frc": np.abs(geom_frc - per_geom).reshape(len(idx), -1).max(1) / fscale, "force": np.abs(total - qfrc[:, 0:3]).max(1) / fscale}
    mom = np.full(len(idx), np.nan)
    for i, j in enumerate(idx):
        if contact[i, ~floor, 11].any():
            continue
        q = fam.q[j]
        w, x, y, z = q[3:7] / np.linalg.norm(q[3:7])
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        m = np.cross(contact[i, floor, 0:3] - q[0:3], contact[i, floor, 6:9]).sum(0)
        mom[i] = np.abs(R.T @ m - qfrc[i, 3:6]).max() / mscale[i]
    out["moment"] = mom
    return out

"""Inputs and fp64 references of the readout tests (tests/test_readout_cpu.py, tests/test_gpu_readout.py) - not a test module.

Inputs, all seeded:
  (a) 64 constructed poses on the nominal model: arbitrary unit quaternion, z in [-0.01, 0.03], x, y in +-1, leg hinges in +-0.4 rad, motor
      angle in +-20 rad (whole turns included); zero velocities or random ones
  (b) oracle rollout states: 32 envs, move_to_pose, uniform random actions, every fourth of 120 steps
  (c) eight randomised models (jb_model_draw_offsets_host + jb_model_compile_host), one table per env, with the poses of (a)
References: oracle.geom_world (geom frames), the four clearance formulas in fp64 on its output, oracle.forward_debug's contact list,
oracle.momentum_energy, and a short numpy restatement of oracle/jb_oracle.c kinematics() for the body frames and velocities."""
import ctypes as C
import functools

import numpy as np

from jitterbug_amd import _lib, model
from oracle import oracle as O

ROOT_F, LEG_F, WORDS = 32, 6, 58
RF_P, RF_Q, RF_V, RF_W, RF_PHI, RF_PHID, RF_TURNS, RF_TGT, RF_LO = 0, 3, 7, 10, 13, 14, 15, 24, 27
NF, NG, NB = model.NFRAME, model.NGEOM, model.NBODY
# the project's strict entry bound for fp32 against the oracle
RTOL, ATOL = 1e-4, 1e-5
# Clearance: worst deviation of the fp32 HOST build from the oracle over inputs (a) - (c), measured by test_readout_cpu.py (it prints the
# figure per input): 2.678e-8 m on (b), 1.358e-8 on (a), 1.544e-8 on (c) - a few ulps of the heights involved (2^-24 * 0.07 m = 4e-9; the
# constant tables are fp32 too).  Asserted: four times it, headroom for the device's different multiply-add fusion.  Never above 1e-6 m
# (about 130 ulps of the largest height): beyond it the error is a formula's.
TOL_C_MEASURED = 2.7e-8
TOL_C = 4 * TOL_C_MEASURED
assert TOL_C <= 1e-6


def geom_types(P):
    return P[model.P_GEOM + model.G_TYPE:model.P_GEOM + NG * model.GEOM_STRIDE:model.GEOM_STRIDE].astype(int)


# ------------------------------------------------------------------------------------------------ states in the device's block layout
def pack(qpos, qvel, target):
    """[n, 16], [n, 15], [n, 3] fp64 -> one snapshot (uint32 [58 n]) exactly as jb_set_state leaves the blocks: fp32 words, the height and
    the quaternion as hi + lo, the motor angle as wrapped angle + whole turns"""
    q, v, t = (np.asarray(a, dtype=np.float64) for a in (qpos, qvel, target))
    n = q.shape[0]
    root = np.zeros((ROOT_F, n), dtype=np.float32)
    leg = np.zeros((LEG_F, n, 4), dtype=np.float32)
    root[0:7] = q[:, 0:7].T.astype(np.float32)
    root[RF_LO:RF_LO + 5] = (q[:, 2:7] - q[:, 2:7].astype(np.float32).astype(np.float64)).T.astype(np.float32)
    k = np.floor((q[:, 15] + np.pi) / (2 * np.pi))
    root[RF_PHI] = (q[:, 15] - k * 6.283185307179586).astype(np.float32)
    root[RF_TURNS] = k.astype(np.float32)
    root[RF_V:RF_V + 6] = v[:, 0:6].T.astype(np.float32)
    root[RF_PHID] = v[:, 14].astype(np.float32)
    root[RF_TGT:RF_TGT + 3] = t.T.astype(np.float32)
    leg[0] = q[:, 7:15:2].astype(np.float32); leg[1] = q[:, 8:15:2].astype(np.float32)
    leg[2] = v[:, 6:14:2].astype(np.float32); leg[3] = v[:, 7:14:2].astype(np.float32)
    return np.concatenate([root.reshape(-1), leg.reshape(-1), np.zeros(2 * n, dtype=np.float32)]).view(np.uint32)


def unpack(snap, n):
    """the fp64 state jb_get_state returns for these blocks: (qpos [n, 16], qvel [n, 15], target [n, 3])"""
    w = np.asarray(snap, dtype=np.uint32).view(np.float32)
    root = w[:ROOT_F * n].reshape(ROOT_F, n).astype(np.float64)
    leg = w[ROOT_F * n:(ROOT_F + 4 * LEG_F) * n].reshape(LEG_F, n, 4).astype(np.float64)
    q, v = np.zeros((n, 16)), np.zeros((n, 15))
    q[:, 0:7] = root[0:7].T
    q[:, 2:7] += root[RF_LO:RF_LO + 5].T
    q[:, 7:15:2] = leg[0]; q[:, 8:15:2] = leg[1]
    q[:, 15] = root[RF_PHI] + 6.283185307179586 * root[RF_TURNS]
    v[:, 0:6] = root[RF_V:RF_V + 6].T
    v[:, 6:14:2] = leg[2]; v[:, 7:14:2] = leg[3]
    v[:, 14] = root[RF_PHID]
    return q, v, root[RF_TGT:RF_TGT + 3].T.copy()


# ------------------------------------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def poses(with_velocity):
    """input (a): (qpos [64, 16], qvel [64, 15], target [64, 3])"""
    rng = np.random.default_rng(1)
    n = 64
    q = np.zeros((n, 16))
    quat = rng.normal(size=(n, 4))
    q[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    q[:, 2] = rng.uniform(-0.01, 0.03, n)
    q[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    q[:, 7:15] = rng.uniform(-0.4, 0.4, (n, 8))
    q[:, 15] = rng.uniform(-20, 20, n)
    t = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), rng.uniform(-np.pi, np.pi, (n, 1))], axis=1)
    v = np.zeros((n, 15))
    if with_velocity:
        v[:, 0:3] = rng.normal(0, 0.3, (n, 3)); v[:, 3:6] = rng.normal(0, 3.0, (n, 3)); v[:, 6:14] = rng.normal(0, 5.0, (n, 8)); v[:, 14] = rng.normal(0, 60.0, n)
    for a in (q, v, t):
        a.setflags(write=False)
    return q, v, t


@functools.lru_cache(maxsize=None)
def rollout_states():
    """input (b): (qpos [960, 16], qvel [960, 15], target [960, 3]), step-major (32 envs per kept step)"""
    env = O.OracleEnv(32, "move_to_pose", P=model.default_params(), seed=11)
    env.reset()
    rng = np.random.default_rng(2)
    qs, vs, ts = [], [], []
    for k in range(120):
        env.step(rng.uniform(-1, 1, 32))
        if k % 4 == 3:
            q, v, t = env.get_state()
            qs.append(q); vs.append(v); ts.append(t)
    out = tuple(np.concatenate(a) for a in (qs, vs, ts))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def random_models():
    """input (c): eight parameter tables [8, NPARAM] from the project's own randomiser (legs and mass position, the reference's sigmas)"""
    L = _lib.load()
    cfg = _lib.RandomiseConfig()
    assert L.jb_default_randomise_config(C.byref(cfg)) == 0
    P = np.zeros((8, model.NPARAM))
    for i in range(8):
        off = np.zeros(_lib.NOFFSET)
        assert L.jb_model_draw_offsets_host(C.c_uint64(5), C.c_uint64(i), C.c_uint32(0), C.byref(cfg), _lib.ptr(off)) == 0
        assert L.jb_model_compile_host(_lib.ptr(off), int(cfg.flags), _lib.ptr(P[i])) == 0
    P.setflags(write=False)
    return P


# ------------------------------------------------------------------------------------------------ fp64 references
def _quat2mat(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def _rodrigues(e, th):
    K = np.array([[0, -e[2], e[1]], [e[2], 0, -e[0]], [-e[1], e[0], 0]])
    return np.cos(th) * np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * np.outer(e, e)


def bodies(P, q, v):
    """what oracle/jb_oracle.c kinematics() and its Jacobians give, restated: per body the rotation from qpos0 [10, 3, 3], the centre of mass
    [10, 3], its world velocity [10, 3], the world angular velocity [10, 3], the world inertia about the centre of mass [10, 3, 3], the mass [10]"""
    R, t, anchor, axis = [None] * NB, [None] * NB, [None] * NB, [None] * NB
    R[0] = _quat2mat(q[3:7] / np.linalg.norm(q[3:7])); t[0] = q[0:3].copy()
    for b in range(1, NB):
        H = P[model.P_HINGE + (b - 1) * model.HINGE_STRIDE:][:model.HINGE_STRIDE]
        a, e, p = H[model.H_ANCHOR:model.H_ANCHOR + 3], H[model.H_AXIS:model.H_AXIS + 3], model.BODY_PARENT[b]
        Rj = _rodrigues(e, q[7 + b - 1])
        R[b] = R[p] @ Rj
        t[b] = t[p] + R[p] @ (a - Rj @ a)
        anchor[b] = R[p] @ a + t[p]
        axis[b] = R[p] @ e
    com, vc, w, Iw, m = np.zeros((NB, 3)), np.zeros((NB, 3)), np.zeros((NB, 3)), np.zeros((NB, 3, 3)), np.zeros(NB)
    w0 = R[0] @ v[3:6]
    for b in range(NB):
        B = P[model.P_BODY + b * model.BODY_STRIDE:][:model.BODY_STRIDE]
        m[b] = B[model.B_MASS]
        com[b] = R[b] @ B[model.B_COM:model.B_COM + 3] + t[b]
        ii = B[model.B_INERTIA:model.B_INERTIA + 6]
        Iw[b] = R[b] @ np.array([[ii[0], ii[3], ii[4]], [ii[3], ii[1], ii[5]], [ii[4], ii[5], ii[2]]]) @ R[b].T
        vc[b] = v[0:3] + np.cross(w0, com[b] - t[0]); w[b] = w0
        a = b
        while a > 0:
            vc[b] += np.cross(axis[a], com[b] - anchor[a]) * v[5 + a]
            w[b] = w[b] + axis[a] * v[5 + a]
            a = model.BODY_PARENT[a]
    return np.array(R), com, vc, w, Iw, m


def clearance_of(types, c, R, s):
    """the four exact formulas: signed smallest height of a geom's surface above z = 0"""
    if types == model.GEOM_SPHERE:
        return c[2] - s[0]
    if types == model.GEOM_CYLINDER:
        return c[2] - (s[1] * abs(R[2, 2]) + s[0] * np.sqrt(max(0.0, 1 - R[2, 2] ** 2)))
    if types == model.GEOM_BOX:
        return c[2] - sum(s[i] * abs(R[2, i]) for i in range(3))
    return c[2] - np.sqrt(sum((s[i] * R[2, i]) ** 2 for i in range(3)))


class Reference:
    """fp64 answers for states (qpos, qvel, target) [n, ...] with tables P ([NPARAM], or [m, NPARAM]: state j takes table j % m); computed
    once and left unchanged"""

    def __init__(self, P, q, v, t, contacts=True):
        P = np.asarray(P, dtype=np.float64)
        n = q.shape[0]
        tab = (lambda j: P) if P.ndim == 1 else (lambda j: P[j % P.shape[0]])
        self.n = n
        self.frames = np.zeros((n, NF, 12)); self.clear = np.zeros((n, NG)); self.bvel = np.zeros((n, NB, 6)); self.energy = np.zeros((n, 8))
        self.energy_scale = np.zeros((n, 8))          # per component: the sum of the absolute per-body terms it is made of
        self.types = np.array([geom_types(tab(j)) for j in range(n)])
        self.touching, self.con_min = [], []
        for j in range(n):
            Pj = tab(j)
            R, com, vc, w, Iw, m = bodies(Pj, q[j], v[j])
            self.frames[j, :NB, 0:3] = com; self.frames[j, :NB, 3:] = R.reshape(NB, 9)
            self.bvel[j, :, 0:3] = vc; self.bvel[j, :, 3:6] = w
            for g in range(NG):
                c, Rg, s = O.geom_world(Pj, q[j], g)
                self.frames[j, NB + g, 0:3] = c; self.frames[j, NB + g, 3:] = Rg.reshape(9)
                self.clear[j, g] = clearance_of(self.types[j, g], c, Rg, s)
            psi = t[j, 2]
            self.frames[j, NB + NG, 0:3] = (t[j, 0], t[j, 1], Pj[model.P_TARGETZ])
            self.frames[j, NB + NG, 3:] = (np.cos(psi), -np.sin(psi), 0, np.sin(psi), np.cos(psi), 0, 0, 0, 1)
            e = O.momentum_energy(Pj, q[j], v[j])
            self.energy[j] = np.concatenate([e["P"], e["L"], [e["T"], e["V"]]])
            h = np.einsum("bij,bj->bi", Iw, w)
            grav = Pj[model.P_GRAVITY:model.P_GRAVITY + 3]
            k = Pj[model.P_HINGE + model.H_STIFFNESS:model.P_HINGE + model.NHINGE * model.HINGE_STRIDE:model.HINGE_STRIDE]
            sc = self.energy_scale[j]
            sc[0:3] = np.abs(m[:, None] * vc).sum(0)
            sc[3:6] = np.abs(h + m[:, None] * np.cross(com, vc)).sum(0)
            sc[6] = (0.5 * m * (vc * vc).sum(1) + 0.5 * (w * h).sum(1)).sum()
            sc[7] = np.abs(m * (com @ grav)).sum() + np.abs(0.5 * k * q[j, 7:16] ** 2).sum()
            if contacts:
                d = O.forward_debug(Pj, q[j], v[j], 0.0, O.default_opts(pair_contacts=0))
                self.touching.append(set(int(g) for g in d["con_geom"]))
                self.con_min.append({int(g): float(d["con_dist"][d["con_geom"] == g].min()) for g in set(d["con_geom"])})
        for a in (self.frames, self.clear, self.bvel, self.energy, self.energy_scale):
            a.setflags(write=False)

    def subset(self, idx):
        """the reference of states idx (a slice or index list), sharing this one's arrays"""
        import copy
        r = copy.copy(self)
        idx = list(range(self.n))[idx] if isinstance(idx, slice) else list(idx)
        r.n = len(idx)
        r.frames, r.clear, r.bvel, r.energy, r.energy_scale, r.types = (a[idx] for a in (self.frames, self.clear, self.bvel, self.energy, self.energy_scale, self.types))
        r.touching = [self.touching[j] for j in idx] if self.touching else []
        r.con_min = [self.con_min[j] for j in idx] if self.con_min else []
        return r

    def check(self, frames=None, clear=None, bvel=None, energy=None, rtol=RTOL, atol=ATOL, tol_c=TOL_C, tol_e=1e-4, label=""):
        """every given output [n, ...] against the reference; prints each figure before it asserts; returns the clearance deviation"""
        dev = None
        if frames is not None:
            err = np.abs(np.asarray(frames, dtype=np.float64).reshape(self.n, NF, 12) - self.frames) - rtol * np.abs(self.frames)
            print("%s frames: worst |error| - rtol |ref| = %.3e (bound %.1e)" % (label, err.max(), atol))
            assert err.max() <= atol, np.unravel_index(err.argmax(), err.shape)
        if bvel is not None:
            err = np.abs(np.asarray(bvel, dtype=np.float64).reshape(self.n, NB, 6) - self.bvel) - rtol * np.abs(self.bvel)
            print("%s body_vel: worst |error| - rtol |ref| = %.3e (bound %.1e)" % (label, err.max(), atol))
            assert err.max() <= atol, np.unravel_index(err.argmax(), err.shape)
        if clear is not None:
            c = np.asarray(clear, dtype=np.float64).reshape(self.n, NG)
            dev = np.abs(c - self.clear).max()
            print("%s clearance: worst deviation %.3e m (bound %.1e)" % (label, dev, tol_c))
            assert dev <= tol_c
            if self.touching:
                decided = np.abs(self.clear) > tol_c
                share = 1.0 - decided.mean()
                print("%s touching sets: %d of %d (state, geom) entries within the bound of the plane (%.3f %%)" % (label, (~decided).sum(), decided.size, 100 * share))
                assert share < 0.005
                for j in range(self.n):
                    got = set(np.nonzero((c[j] < 0) & decided[j])[0].tolist())
                    want = set(g for g in self.touching[j] if decided[j, g])
                    assert got == want, (j, got ^ want)
        if energy is not None:
            err = np.abs(np.asarray(energy, dtype=np.float64).reshape(self.n, 8) - self.energy) / np.maximum(self.energy_scale, 1e-300)
            print("%s energy: worst error / sum |per-body terms| per component = %s (bound %.1e)" % (label, np.array2string(err.max(0), precision=2), tol_e))
            assert (np.abs(np.asarray(energy, dtype=np.float64).reshape(self.n, 8) - self.energy) <= tol_e * self.energy_scale).all()
        return dev


@functools.lru_cache(maxsize=None)
def reference(name):
    """'poses' (a, zero velocities), 'poses-moving' (a, random velocities), 'rollout' (b), 'models' / 'models-moving' (c)"""
    return Reference(tables(name), *states(name))


def raw_states(name):
    """the states as drawn (fp64): what a test hands to set_state"""
    return rollout_states() if name == "rollout" else poses(name.endswith("moving"))


@functools.lru_cache(maxsize=None)
def snapshot(name):
    s = pack(*raw_states(name))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def states(name):
    """the states as the device holds them (fp32 words, hi + lo) and get_state returns them: where the references are evaluated"""
    out = unpack(snapshot(name), raw_states(name)[0].shape[0])
    for a in out:
        a.setflags(write=False)
    return out


def tables(name):
    return random_models() if name.startswith("models") else model.default_params()


NAMES = ("poses", "poses-moving", "rollout", "models", "models-moving")

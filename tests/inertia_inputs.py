"""Inputs, fp64 references and bounds of the inertia tests (tests/test_inertia_cpu.py, tests/test_gpu_inertia.py) - not a test module.

Inputs: readout_inputs' five sets (poses, poses-moving, rollout, models, models-moving), taken by import, with one action per state drawn
uniformly in [-1.5, 1.5] from a fixed seed (the ctrlrange is [-1, 1]: the clamp is exercised).
References: oracle.forward_debug(P, q, v, ctrl) gives M, bias, tau and qacc_smooth; the passive and actuator rows are split out of
tau + bias with the parameter table.  A numpy restatement of oracle/jb_oracle.c kinematics() / jacobian() gives the Jacobians, and one of
dynamics()' bias recursion the per-body terms of the bias - only for the scale its error is measured against."""
import functools

import numpy as np

from jitterbug_amd import model
from oracle import oracle as O
from tests import readout_inputs as ri

NV, NB, NJAC = model.NV, model.NBODY, 14
NAMES = ri.NAMES
# the project's strict entry bound for fp32 against the oracle: relative to the entry's scale, absolute on dimensionless entries
RTOL, ATOL = ri.RTOL, ri.ATOL

# Worst scaled deviation of the fp32 HOST build from the oracle over the five inputs, per output, measured by test_inertia_cpu.py (it prints
# the figure per input).  Asserted: four times it - headroom for the device's different multiply-add fusion, the readout's margin and
# reason - and never above the strict figure (RTOL of the entry's scale, ATOL on the dimensionless jacr), beyond which the error is a formula's.
#   qM           |error_ij| / sqrt(M_ii M_jj)                                  3.88e-7 rollout, 3.42e-7 models, 3.31e-7 poses
#   qfrc         |error_d| / sum over the bodies of |Jv^T F| + |Jw^T N| of dof d (bias), |k th| + |b th'| (passive), the force's addends
#                (actuator)                                                    4.77e-5 poses, 3.28e-5 rollout, 2.29e-5 models, 1.95e-5 models-moving, 9.5e-6
#                poses-moving.  All of it is the bias of the five dofs with ONE body behind them (the knees 7, 9, 11, 13 and the motor 14),
#                where the scale is the term itself: in some states gravity's lever about the hinge nearly vanishes (the worst, a knee
#                of a pose at rest, keeps 4e-3 of it), and the fp32 rounding of the rotations (eps m g r) is then large against what is
#                left.  Every other entry of the bias stays below 5.7e-6, passive and actuator below 1.6e-7.  Four times the figure is
#                above the cap: the cap is what is asserted.
#                On the MI355X (tests/test_gpu_inertia.py's cases, 158 states): 2.66e-5 (rollout, N = 32), 3.1e-6 poses-moving, below 1.6e-6
#                on every other case - a quarter of the cap; qM 3.1e-7, qacc_smooth 3.8e-7, jacp 2.3e-7, jacr 1.9e-7, all below the host's.
#   qacc_smooth  sqrt(e^T M e) / sqrt(x^T M x)                                 4.28e-7 models, 4.23e-7 rollout
#   jacp         |error| / lever arm (1 for the linear columns)                3.68e-7 rollout
#   jacr         |error| (dimensionless)                                       2.45e-7 rollout
TOL_M_MEASURED, TOL_F_MEASURED, TOL_A_MEASURED, TOL_JP_MEASURED, TOL_JR_MEASURED = 3.9e-7, 4.8e-5, 4.3e-7, 3.7e-7, 2.5e-7
TOL_M, TOL_F, TOL_A, TOL_JP = (min(4 * x, RTOL) for x in (TOL_M_MEASURED, TOL_F_MEASURED, TOL_A_MEASURED, TOL_JP_MEASURED))
TOL_JR = min(4 * TOL_JR_MEASURED, ATOL)
MEASURED = dict(qM=TOL_M_MEASURED, qfrc=TOL_F_MEASURED, qacc_smooth=TOL_A_MEASURED, jacp=TOL_JP_MEASURED, jacr=TOL_JR_MEASURED)
FP32 = dict(qM=TOL_M, qfrc=TOL_F, qacc_smooth=TOL_A, jacp=TOL_JP, jacr=TOL_JR)
FP64 = dict(qM=1e-12, qfrc=1e-12, qacc_smooth=1e-10, jacp=1e-12, jacr=1e-12)


@functools.lru_cache(maxsize=None)
def actions(name):
    """one action per state of input `name`, fp32-exact (what the device is handed), uniform in [-1.5, 1.5]"""
    n = ri.raw_states(name)[0].shape[0]
    a = np.random.default_rng(7 + NAMES.index(name)).uniform(-1.5, 1.5, n).astype(np.float32).astype(np.float64)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------ numpy restatement of the oracle
def kinematics(P, q):
    """oracle/jb_oracle.c kinematics(): per body R, t, hinge anchor and axis (world), centre of mass, world inertia, mass"""
    R, t, anchor, axis = [None] * NB, [None] * NB, [None] * NB, [None] * NB
    R[0] = ri._quat2mat(q[3:7] / np.linalg.norm(q[3:7])); t[0] = q[0:3].copy()
    for b in range(1, NB):
        H = P[model.P_HINGE + (b - 1) * model.HINGE_STRIDE:][:model.HINGE_STRIDE]
        a, e, p = H[model.H_ANCHOR:model.H_ANCHOR + 3], H[model.H_AXIS:model.H_AXIS + 3], model.BODY_PARENT[b]
        Rj = ri._rodrigues(e, q[7 + b - 1])
        R[b] = R[p] @ Rj
        t[b] = t[p] + R[p] @ (a - Rj @ a)
        anchor[b] = R[p] @ a + t[p]
        axis[b] = R[p] @ e
    com, Iw, m = np.zeros((NB, 3)), np.zeros((NB, 3, 3)), np.zeros(NB)
    for b in range(NB):
        B = P[model.P_BODY + b * model.BODY_STRIDE:][:model.BODY_STRIDE]
        m[b] = B[model.B_MASS]
        com[b] = R[b] @ B[model.B_COM:model.B_COM + 3] + t[b]
        ii = B[model.B_INERTIA:model.B_INERTIA + 6]
        Iw[b] = R[b] @ np.array([[ii[0], ii[3], ii[4]], [ii[3], ii[1], ii[5]], [ii[4], ii[5], ii[2]]]) @ R[b].T
    return dict(R=R, t=t, anchor=anchor, axis=axis, com=com, Iw=Iw, m=m)


def jacobian(k, b, x):
    """oracle jacobian(): (Jv [3, 15], Jw [3, 15]) of the world point x on body b, and per column the lever arm its jacp entries scale with"""
    Jv, Jw, lever = np.zeros((3, NV)), np.zeros((3, NV)), np.ones(NV)
    Jv[:, 0:3] = np.eye(3)
    for j in range(3):
        e = k["R"][0][:, j]
        Jw[:, 3 + j] = e; Jv[:, 3 + j] = np.cross(e, x - k["t"][0]); lever[3 + j] = np.linalg.norm(x - k["t"][0])
    a = b
    while a > 0:
        Jw[:, 5 + a] = k["axis"][a]; Jv[:, 5 + a] = np.cross(k["axis"][a], x - k["anchor"][a]); lever[5 + a] = np.linalg.norm(x - k["anchor"][a])
        a = model.BODY_PARENT[a]
    return Jv, Jw, lever


def bias_terms(P, k, J, v):
    """oracle dynamics()' recursion: the velocity-product accelerations at qacc = 0 with gravity folded in as -g at the root; returns the
    per-body terms [10, 2, 15] - the force's Jv^T F and the moment's Jw^T N, the addends of dynamics()' `bias[d] +=` - whose sum is qfrc_bias"""
    g = P[model.P_GRAVITY:model.P_GRAVITY + 3]
    w, al, ref, Aref = np.zeros((NB, 3)), np.zeros((NB, 3)), np.zeros((NB, 3)), np.zeros((NB, 3))
    w[0] = k["R"][0] @ v[3:6]; ref[0] = k["t"][0]; Aref[0] = -g
    terms = np.zeros((NB, 2, NV))
    for b in range(NB):
        if b > 0:
            p, qd = model.BODY_PARENT[b], v[5 + b]
            w[b] = w[p] + k["axis"][b] * qd
            al[b] = al[p] + np.cross(w[p], k["axis"][b]) * qd
            r = k["anchor"][b] - ref[p]; ref[b] = k["anchor"][b]
            Aref[b] = Aref[p] + np.cross(al[p], r) + np.cross(w[p], np.cross(w[p], r))
        r = k["com"][b] - ref[b]
        F = k["m"][b] * (Aref[b] + np.cross(al[b], r) + np.cross(w[b], np.cross(w[b], r)))
        N = k["Iw"][b] @ al[b] + np.cross(w[b], k["Iw"][b] @ w[b])
        terms[b, 0], terms[b, 1] = J[b][0].T @ F, J[b][1].T @ N
    return terms


def hinge_kb(P):
    k = P[model.P_HINGE + model.H_STIFFNESS:model.P_HINGE + model.NHINGE * model.HINGE_STRIDE:model.HINGE_STRIDE]
    b = P[model.P_HINGE + model.H_DAMPING:model.P_HINGE + model.NHINGE * model.HINGE_STRIDE:model.HINGE_STRIDE]
    return k, b


class Reference:
    """fp64 answers for states (qpos, qvel) [n, ...] under actions ctrl [n] with tables P ([NPARAM], or [m, NPARAM]: state j takes table
    j % m); computed once and left unchanged"""

    def __init__(self, P, q, v, ctrl):
        P = np.asarray(P, dtype=np.float64)
        n = q.shape[0]
        tab = (lambda j: P) if P.ndim == 1 else (lambda j: P[j % P.shape[0]])
        self.n = n
        self.qM, self.qfrc, self.qfrc_scale, self.qacc = np.zeros((n, NV, NV)), np.zeros((n, 3, NV)), np.zeros((n, 3, NV)), np.zeros((n, NV))
        self.jac, self.lever = np.zeros((n, NJAC, 6, NV)), np.ones((n, NJAC, NV))
        self.M_numpy, self.bias_numpy = np.zeros((n, NV, NV)), np.zeros((n, NV))
        for j in range(n):
            Pj = tab(j)
            d = O.forward_debug(Pj, q[j], v[j], float(ctrl[j]), O.default_opts(contacts=0))
            self.qM[j], self.qacc[j] = d["M"], d["qacc_smooth"]
            kk, bb = hinge_kb(Pj)
            pas = np.zeros(NV)
            pas[6:15] = -kk * q[j, 7:16] - bb * v[j, 6:15]
            self.qfrc[j, 0], self.qfrc[j, 1] = d["bias"], pas
            self.qfrc[j, 2, 14] = d["tau"][14] + d["bias"][14] - pas[14]      # (the oracle's actuator acts on the motor dof alone)
            assert np.abs(d["tau"] + d["bias"] - pas - self.qfrc[j, 2]).max() <= 1e-15 * np.abs(d["bias"]).max()
            k = kinematics(Pj, q[j])
            J = [jacobian(k, b, k["com"][b]) for b in range(NB)]
            J += [jacobian(k, 2 + 2 * l, O.geom_world(Pj, q[j], model.FOOT_GEOMS[l])[0]) for l in range(model.NLEG)]
            for r in range(NJAC):
                self.jac[j, r, 0:3], self.jac[j, r, 3:6], self.lever[j, r] = J[r]
            self.M_numpy[j] = sum(k["m"][b] * J[b][0].T @ J[b][0] + J[b][1].T @ k["Iw"][b] @ J[b][1] for b in range(NB))
            terms = bias_terms(Pj, k, J, v[j])
            self.bias_numpy[j] = terms.sum((0, 1))
            u = min(max(float(ctrl[j]), Pj[model.P_CTRLRANGE]), Pj[model.P_CTRLRANGE + 1])
            gear, bp = Pj[model.P_GEAR], Pj[model.P_BIASPRM:model.P_BIASPRM + 3]
            self.qfrc_scale[j, 0] = np.abs(terms).sum((0, 1))
            self.qfrc_scale[j, 1, 6:15] = np.abs(kk * q[j, 7:16]) + np.abs(bb * v[j, 6:15])
            self.qfrc_scale[j, 2, 14] = abs(gear) * (abs(Pj[model.P_GAIN] * u) + abs(bp[0]) + abs(bp[1] * gear * q[j, 15]) + abs(bp[2] * gear * v[j, 14]))
        for a in (self.qM, self.qfrc, self.qfrc_scale, self.qacc, self.jac, self.lever, self.M_numpy, self.bias_numpy):
            a.setflags(write=False)

    def subset(self, idx):
        """the reference of states idx (a slice or index list), sharing this one's arrays"""
        import copy
        r = copy.copy(self)
        idx = list(range(self.n))[idx] if isinstance(idx, slice) else list(idx)
        r.n = len(idx)
        r.qM, r.qfrc, r.qfrc_scale, r.qacc, r.jac, r.lever, r.M_numpy, r.bias_numpy = (a[idx] for a in (self.qM, self.qfrc, self.qfrc_scale, self.qacc, self.jac, self.lever, self.M_numpy, self.bias_numpy))
        return r

    def deviations(self, qM=None, qfrc=None, qacc_smooth=None, jac=None):
        """the worst scaled deviation of every given output [n, ...], as a dict keyed like FP32 / FP64.  Where the scale of an entry is 0
        the reference is an exact 0 and so must the output be (asserted here)."""
        n, dev = self.n, {}
        if qM is not None:
            dg = np.sqrt(np.einsum("nii->ni", self.qM))
            dev["qM"] = float((np.abs(np.asarray(qM, dtype=np.float64).reshape(n, NV, NV) - self.qM) / (dg[:, :, None] * dg[:, None, :])).max())
        if qfrc is not None:
            e = np.abs(np.asarray(qfrc, dtype=np.float64).reshape(n, 3, NV) - self.qfrc)
            assert (e[self.qfrc_scale == 0] == 0).all()
            dev["qfrc"] = float((e / np.where(self.qfrc_scale > 0, self.qfrc_scale, 1.0)).max())
        if qacc_smooth is not None:
            e = np.asarray(qacc_smooth, dtype=np.float64).reshape(n, NV) - self.qacc
            num, den = np.sqrt(np.einsum("ni,nij,nj->n", e, self.qM, e)), np.sqrt(np.einsum("ni,nij,nj->n", self.qacc, self.qM, self.qacc))
            dev["qacc_smooth"] = float((num / den).max())
        if jac is not None:
            e = np.abs(np.asarray(jac, dtype=np.float64).reshape(n, NJAC, 6, NV) - self.jac)
            dev["jacp"] = float((e[:, :, 0:3] / self.lever[:, :, None, :]).max())
            dev["jacr"] = float(e[:, :, 3:6].max())
        return dev

    def check(self, bounds, label="", **outputs):
        """every given output against the reference under `bounds` (FP32 or FP64); prints each figure before it asserts; returns them"""
        dev = self.deviations(**outputs)
        for key, x in dev.items():
            print("%s %s: worst scaled deviation %.3e (bound %.1e)" % (label, key, x, bounds[key]))
        for key, x in dev.items():
            assert x <= bounds[key], (label, key, x, bounds[key])
        return dev


@functools.lru_cache(maxsize=None)
def reference(name):
    q, v, _ = ri.states(name)
    return Reference(ri.tables(name), q, v, actions(name))

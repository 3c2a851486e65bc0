"""Inputs, fp64 references and bounds of the forward-dynamics tests (tests/test_forward_cpu.py, tests/test_gpu_forward.py) - not a test module.

Families (states packed into the device's block layout by readout_inputs.pack; the oracle sees the fp64 value of the packed words, so both
sides start from the same state; controls uniform in [-1, 1] from a fixed seed per family):
  rollout          readout_inputs' 960 oracle rollout states on the nominal model, 779 in floor contact, at most 9 contacts
  poses-moving     its 64 constructed poses with velocities: every geom type below the floor, up to 52 contacts
  models-moving    the same poses on its 8 randomised models (state j takes table j % 8), the oracle's geom-geom pairs on
  mass-touching    parity_inputs.mass_touching_models(): the rest pose with the motor turned to where the mass ellipsoid overlaps an upper leg
                   least and most, small random velocities (state j takes model j % m)
  thread-touching  parity_inputs.thread_touching_models(4): the rest pose, where the motor-axis thread overlaps a front leg, at rest and moving
References, all from the oracle (oracle.forward_debug's M, tau, qfrc_constraint; oracle.step_physics(nsub=1) for the contact-switch margin):
  qacc             numpy.linalg.solve(M + h diag(b), tau + qfrc_constraint) - NOT forward_debug's own qacc, which leaves h b out
  qfrc_constraint  forward_debug's
  body_acc         central finite difference (step 1e-6 s) of readout_inputs.bodies' velocities along q' = v, v' = qacc
  motor            the three formulas of include/jitterbug_hip.h on the parameter table
Errors are taken per output block, |x - ref| over (the block's largest |ref| in that env-state + the block's floor); for qfrc_constraint the
scale is the block's largest inertial term |M y| instead: the quantity is what is left when the inertial terms and tau cancel, and its
rounding error scales with what cancels."""
import functools

import numpy as np

from jitterbug_amd import model
from oracle import oracle as O
from tests import parity_inputs as pi
from tests import readout_inputs as ri
from tests.parity_protocol import MARGIN_TOL

NV, NB = model.NV, model.NBODY
FAMILIES = ("rollout", "poses-moving", "models-moving", "mass-touching", "thread-touching")
FD_STEP = 1e-6

# ---- blocks: (output, block) -> index into the output's last axis, and the absolute floor added to the block's scale.  The floors are a
# thousandth of the magnitudes these quantities reach on the oracle's states (root accelerations 3.3e3, hinge accelerations 3.9e4 rad/s^2;
# the robot weighs 0.172 N, hinge torques reach 0.014 N m), so an env-state in free fall is not judged against a zero scale.
BLOCKS = {
    ("qacc", "linear"): (slice(0, 3), 3.0), ("qacc", "angular"): (slice(3, 6), 3.0), ("qacc", "hinges"): (slice(6, 14), 40.0), ("qacc", "motor"): (slice(14, 15), 40.0),
    ("qfrc", "force"): (slice(0, 3), 2e-4), ("qfrc", "moment"): (slice(3, 6), 1e-5), ("qfrc", "hinges"): (slice(6, 14), 1e-5), ("qfrc", "motor"): (slice(14, 15), 1e-5),
    ("body_acc", "linear"): (slice(0, 3), 3.0), ("body_acc", "angular"): (slice(3, 6), 3.0),
    ("motor", "all"): (slice(0, 3), 1e-3),
}

# ---- conditioning: env-states whose one-substep oracle margin is below MARGIN_TOL (a contact within 11 nm of switching, or a deep pair
# overlap: margin 0) are excluded from the strict bounds.  The caps are conditions on the inputs, computed with the oracle alone:
# rollout 0 of 960 (smallest margin 1.07 um); poses-moving at most 12 of 64 (12 with the oracle's geom-geom pairs on: margin 0 from deep
# overlaps; none with the pairs off, which is what the nominal model's kernels simulate and what the family's reference uses); models-moving
# 11 of 64 and mass-touching 5 of 32 (deep overlaps, margin 0; the smallest margin kept is 0.23 um), thread-touching 0 of 8.  No family may
# exclude more than a quarter of its states.
EXCLUDED_CAP = {"rollout": 0, "poses-moving": 12, "models-moving": 11, "mass-touching": 5, "thread-touching": 0}

# ---- bounds.  fp64 host build against the references: the worst error over all families and the lane layouts (1 and 4 groups), measured by
# tests/test_forward_cpu.py (it prints every figure); asserted: ten times it.  Above 1e-9 an error is a formula's, not rounding.
FP64_MEASURED = {
    # (the worst are mass-touching states, where the oracle's and the kernel's pair narrow phase each stop at their own iteration count; on the
    #  nominal model's families every block is below 1e-12)
    ("qacc", "linear"): 6.0e-12, ("qacc", "angular"): 9.3e-12, ("qacc", "hinges"): 1.4e-11, ("qacc", "motor"): 1.2e-11,
    ("qfrc", "force"): 4.4e-12, ("qfrc", "moment"): 7.8e-12, ("qfrc", "hinges"): 3.3e-12, ("qfrc", "motor"): 1.1e-11,
    ("motor", "all"): 1e-15,          # (measured 0: the three formulas are evaluated in the same order)
}
# body_acc against the finite difference: the reference's own error is the difference's rounding, 2^-53 |body_vel| / FD_STEP relative to the
# block's scale plus the truncation, of second order in FD_STEP; measured 1.07e-8 (linear) and 9.8e-11 (angular), both on rollout.
FP64_MEASURED_FD = {("body_acc", "linear"): 1.1e-8, ("body_acc", "angular"): 9.8e-11}
# fp32 host build (4 lane groups, the device's layout; g++ -O2 rounds every operation once), worst over all families; asserted - on the host
# AND on the GPU - three times it: the device contracts multiply-adds differently from the host compiler, which the project's own
# LEAN-against-ordinary history shows is worth a small factor and no more.
# The worst cases are all poses-moving / models-moving (up to 52 contacts, forces of 14 N on a robot of 0.17 N); on rollout every block
# stays below 5e-5.
FP32_MEASURED = {
    ("qacc", "linear"): 5.8e-5, ("qacc", "angular"): 8.3e-5, ("qacc", "hinges"): 3.9e-5, ("qacc", "motor"): 1.8e-4,
    ("qfrc", "force"): 5.8e-5, ("qfrc", "moment"): 2.6e-4, ("qfrc", "hinges"): 1.7e-5, ("qfrc", "motor"): 7.8e-5,
    ("body_acc", "linear"): 2.0e-5, ("body_acc", "angular"): 2.9e-5,
    ("motor", "all"): 2.3e-7,
}
# Measured on the MI355X (tests/test_gpu_forward.py, worst over its cases): qacc 2.5e-5 / 5.5e-5 / 1.2e-5 / 3.0e-4, qfrc 6.0e-5 / 2.6e-4 /
# 1.1e-5 / 1.2e-4, body_acc 9.4e-6 / 1.2e-5, motor 1.4e-7 - every block inside three times the host's figure.
FP64_BOUND = {k: 10 * v for k, v in FP64_MEASURED.items()}
FP64_BOUND_FD = {k: 10 * v for k, v in FP64_MEASURED_FD.items()}
FP32_BOUND = {k: 3 * v for k, v in FP32_MEASURED.items()}
assert max(FP64_MEASURED.values()) <= 1e-9


def _advance(q, v, t):
    """q after time t along q' = v: the free joint's position by its world velocity, its quaternion by the root-frame angular velocity
    (q * exp(t w / 2)), the hinges by their rates"""
    out = q.copy()
    out[0:3] += t * v[0:3]
    w = v[3:6] * t
    a = np.linalg.norm(w)
    s = 0.5 if a < 1e-12 else np.sin(0.5 * a) / a
    d = np.array([np.cos(0.5 * a), s * w[0], s * w[1], s * w[2]])
    p = q[3:7]
    out[3:7] = (p[0] * d[0] - p[1] * d[1] - p[2] * d[2] - p[3] * d[3], p[0] * d[1] + p[1] * d[0] + p[2] * d[3] - p[3] * d[2],
                p[0] * d[2] - p[1] * d[3] + p[2] * d[0] + p[3] * d[1], p[0] * d[3] + p[1] * d[2] - p[2] * d[1] + p[3] * d[0])
    out[7:16] += t * v[6:15]
    return out


def _body_vel(P, q, v):
    _, _, vc, w, _, _ = ri.bodies(P, q, v)
    return np.concatenate([vc, w], axis=1)


class Family:
    """One family's inputs: snap (uint32 words, one snapshot of n envs), P ([NPARAM] or [m, NPARAM]: state j takes table j % m), ctrl [n],
    pair (the kernels' PAIR instantiation / the oracle's geom-geom pairs), and the fp64 states (q, v, t) the words hold"""

    def __init__(self, name, raw, P, pair, seed):
        snap = ri.pack(*raw)
        self.raw = raw          # the states as drawn (fp64): what a test hands to set_state
        self.name, self.snap, self.P, self.pair = name, snap, np.asarray(P, dtype=np.float64), int(pair)
        self.n = snap.size // ri.WORDS
        self.q, self.v, self.t = ri.unpack(snap, self.n)
        self.ctrl = np.random.default_rng(seed).uniform(-1, 1, self.n).astype(np.float32).astype(np.float64)      # (the fp32 value the device is handed)
        self.n_models = 1 if self.P.ndim == 1 else self.P.shape[0]
        for a in (self.snap, self.P, self.q, self.v, self.t, self.ctrl):
            a.setflags(write=False)

    def table(self, j):
        return self.P if self.P.ndim == 1 else self.P[j % self.P.shape[0]]

    def tables_per_env(self):
        """[n, NPARAM]: one table per state, as a handle with one model per env takes them"""
        return np.stack([self.table(j) for j in range(self.n)])


def _touching_states(models, poses_of, seed):
    """states (q, v, t) on `models` (a list of tables): poses_of(i) -> the qpos rows of model i; row r of every model first, so that state
    j sits on model j % m"""
    rng = np.random.default_rng(seed)
    m = len(models)
    rows = [poses_of(i) for i in range(m)]
    q = np.stack([rows[i][r] for r in range(len(rows[0])) for i in range(m)])
    v = rng.normal(size=(q.shape[0], 15)) * np.array([.02] * 3 + [.5] * 3 + [.5] * 8 + [10.0])
    v[:m] = 0.0          # the first pose of every model at rest
    return q, v, np.zeros((q.shape[0], 3))


@functools.lru_cache(maxsize=None)
def family(name):
    if name in ("rollout", "poses-moving", "models-moving"):
        return Family(name, ri.raw_states(name), ri.tables(name), name.startswith("models"), 21 + FAMILIES.index(name))
    if name == "mass-touching":
        ms = pi.mass_touching_models()

        def poses_of(i):
            P, hits = ms[i]
            flat = sorted((d, phi) for l in hits for phi, d in hits[l])          # (d < 0: overlap) most overlap first
            out = []
            for d, phi in (flat[-1], flat[0]):
                q = model.qpos0(P); q[15] = phi
                out.append(q)
            return out
        P = np.stack([m_[0] for m_ in ms])
        q, v, t = _touching_states(list(P), poses_of, 31)
    elif name == "thread-touching":
        ms = pi.thread_touching_models(4)
        P = np.stack([m_[0] for m_ in ms])
        q, v, t = _touching_states(list(P), lambda i: [model.qpos0(P[i]), model.qpos0(P[i])], 32)
    else:
        raise KeyError(name)
    return Family(name, (q, v, t), P, True, 21 + FAMILIES.index(name))


class Reference:
    """the oracle's answers for a family, computed once and left unchanged (body_acc, the one expensive part - two numpy restatements of the
    kinematics per state - row by row when first asked for)"""

    def __init__(self, fam):
        n = fam.n
        self.n, self._fam = n, fam
        self.qacc, self.qfrc, self.My = np.zeros((n, NV)), np.zeros((n, NV)), np.zeros((n, NV))
        self.bacc, self.motor, self.margin = np.zeros((n, NB, 6)), np.zeros((n, 3)), np.zeros(n)
        self.ncon, self._bacc_done = np.zeros(n, dtype=int), np.zeros(n, dtype=bool)
        opts = O.default_opts() if fam.pair else O.default_opts(pair_contacts=0)
        for j in range(n):
            P, q, v, u = fam.table(j), fam.q[j], fam.v[j], float(fam.ctrl[j])
            d = O.forward_debug(P, q, v, u, opts)
            h = P[model.P_TIMESTEP]
            b = np.zeros(NV)
            b[6:15] = P[model.P_HINGE + model.H_DAMPING:model.P_HINGE + model.NHINGE * model.HINGE_STRIDE:model.HINGE_STRIDE]
            y = np.linalg.solve(d["M"] + h * np.diag(b), d["tau"] + d["qfrc_constraint"])
            self.qacc[j], self.qfrc[j], self.My[j], self.ncon[j] = y, d["qfrc_constraint"], d["M"] @ y, d["ncon"]
            st = O.Stats()
            st.margin_min = np.inf
            O.step_physics(P, q, v, u, nsub=1, opts=opts, stats=st)
            self.margin[j] = st.margin_min
            uc = min(max(u, P[model.P_CTRLRANGE]), P[model.P_CTRLRANGE + 1])
            gear, bp = P[model.P_GEAR], P[model.P_BIASPRM:model.P_BIASPRM + 3]
            torque = gear * (P[model.P_GAIN] * uc + bp[0] + bp[1] * gear * q[15] + bp[2] * gear * v[14])
            self.motor[j] = (uc, torque, torque * v[14])
        self.strict = self.margin >= MARGIN_TOL
        for a in (self.qacc, self.qfrc, self.My, self.motor, self.margin, self.strict):
            a.setflags(write=False)

    def body_acc(self, idx=None):
        """the finite-difference reference of body_acc for states idx (default: all)"""
        fam = self._fam
        for j in (range(self.n) if idx is None else np.asarray(idx).reshape(-1)):
            if not self._bacc_done[j]:
                P, q, v, y = fam.table(j), fam.q[j], fam.v[j], self.qacc[j]
                self.bacc[j] = (_body_vel(P, _advance(q, v, FD_STEP), v + FD_STEP * y) - _body_vel(P, _advance(q, v, -FD_STEP), v - FD_STEP * y)) / (2 * FD_STEP)
                self._bacc_done[j] = True
        return self.bacc if idx is None else self.bacc[idx]

    def refs(self, out):
        """(reference, what its blocks are scaled by) of output `out`"""
        return {"qacc": (self.qacc, self.qacc), "qfrc": (self.qfrc, self.My), "body_acc": (self.bacc, self.bacc), "motor": (self.motor, self.motor)}[out]

    def errors(self, out, x, idx=None):
        """{block: [n] worst |x - ref| / (largest |scale| of the block in that env-state + floor)} for output `out` = x [n, ...]; idx: the
        states x holds (default: all)"""
        if out == "body_acc":
            self.body_acc(idx)
        ref, scale = self.refs(out)
        if idx is not None:
            ref, scale = ref[idx], scale[idx]
        x = np.asarray(x, dtype=np.float64).reshape(ref.shape)
        res = {}
        for (o, blk), (sl, floor) in BLOCKS.items():
            if o != out:
                continue
            e, s = np.abs(x[..., sl] - ref[..., sl]), np.abs(scale[..., sl])
            res[blk] = e.reshape(e.shape[0], -1).max(1) / (s.reshape(s.shape[0], -1).max(1) + floor)
        return res


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(family(name))


def check(name, outputs, bounds, label, idx=None, measured=None):
    """outputs {"qacc" | "qfrc" | "body_acc" | "motor": array} of family `name` (states idx, default all) against the oracle: every strict
    env-state within `bounds` {(output, block): bound}, every env-state finite.  Prints each figure before it asserts.  measured (a dict):
    takes the worst figure per block (max with what it holds)."""
    ref = reference(name)
    strict = ref.strict if idx is None else ref.strict[idx]
    bad = []
    for out, x in outputs.items():
        assert np.isfinite(np.asarray(x, dtype=np.float64)).all(), (label, out)
        for blk, e in ref.errors(out, x, idx).items():
            if (out, blk) not in bounds:
                continue
            worst = e[strict].max() if strict.any() else 0.0
            print("%s %s %s/%s: worst %.3e over %d strict env-states (bound %.3e); over the %d excluded %.3e" % (
                label, name, out, blk, worst, strict.sum(), bounds[(out, blk)], (~strict).sum(), e[~strict].max() if (~strict).any() else 0.0))
            if measured is not None:
                measured[(out, blk)] = max(measured.get((out, blk), 0.0), worst)
            if not worst <= bounds[(out, blk)]:
                bad.append((out, blk, worst, int(np.nonzero(strict)[0][e[strict].argmax()])))
    assert not bad, (label, name, bad)

"""Inputs, fp64 references and bounds of the evaluate tests (tests/test_evaluate_cpu.py, tests/test_gpu_evaluate.py) - not a test module.

Inputs: the seam batch of tests/task_reference.py (states placed ON the branches of jb_task.hpp, every word an fp32 number), written
into a synthetic snapshot stack two deep in the device's block layout (tests/readout_inputs.py pack): snapshot 0 is the batch, snapshot 1
the batch REVERSED, so that an indexing slip between snapshots shows.  The targets the tests hand over explicitly are the seam batch's
own; the target STORED in the snapshots is a decoy (decoy() below), so that a pass which reads the stored one where it was given another shows.
References: oracle.observation / reward / reward_terms through task_reference.reference, on the state as the blocks hold it - the wrapped
motor angle, which is what the task layer reads -, and for the achieved goal the formula of jb_evaluate.hpp in fp64:
    (px, py, wrap(atan2(R10, R00) - pi / 2)),   R00 = qw^2 + qx^2 - qy^2 - qz^2,   R10 = 2 (qx qy + qw qz),   wrap into (-pi, pi].
Bounds: task_reference.compare's derived bound with its cap for obs, reward and terms; for the achieved yaw pi times the bound of
face_direction's angle entry obs[15] on the same state (the yaw's chain - R00, atan2f, - pi/2, wrap - is a sub-chain of that entry's:
10 roundings against 12, and the entry's S holds the yaw's), compared by circular distance."""
import functools

import numpy as np

from jitterbug_amd import model
from tests import readout_inputs as ri
from tests import task_reference as tr

PI = np.pi
FP64_TOL = 1e-12          # the line tests/test_task_layer_host.py holds the fp64 build of jb_task.hpp to
ANGLE_ENTRY = 15          # face_direction's angle to the target


@functools.lru_cache(maxsize=None)
def seams():
    q, v, t, fams, nv = tr.seam_states()
    for a in (q, v, t, nv):
        a.setflags(write=False)
    return q, v, t, tuple(fams), nv


def decoy(t):
    """a stored target that is none of the explicit ones: fp32 words, every entry moved"""
    return (np.asarray(t)[::-1] * 0.5 + np.array([0.11, -0.07, 0.9])).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def stack():
    """(snap uint32 [2 * 58 n], n, (q, v, t, families, near_vertical) of the 2 n env-states in launch order, stored targets [2 n, 3]):
    q, v as the blocks hold them with the WRAPPED motor angle, t the explicit targets"""
    q, v, t, fams, nv = seams()
    n = len(q)
    stored = decoy(t)
    snaps = [ri.pack(q, v, stored), ri.pack(q[::-1], v[::-1], stored[::-1])]
    held = [ri.unpack(s, n) for s in snaps]
    qh, vh = np.concatenate([h[0] for h in held]), np.concatenate([h[1] for h in held])
    w = np.concatenate([s.view(np.float32)[ri.RF_PHI * n:(ri.RF_PHI + 1) * n] for s in snaps]).astype(np.float64)
    qh[:, 15] = w                                     # the wrapped word: what the task layer reads (every output is periodic in the angle)
    th = np.concatenate([t, t[::-1]])
    assert np.array_equal(qh[:, :15], np.concatenate([q, q[::-1]])[:, :15]) and np.array_equal(vh, np.concatenate([v, v[::-1]]))
    assert np.array_equal(np.concatenate([h[2] for h in held]), np.concatenate([stored, stored[::-1]]))
    return np.concatenate(snaps), n, (qh, vh, th, fams + fams[::-1], np.concatenate([nv, nv[::-1]])), np.concatenate([stored, stored[::-1]])


@functools.lru_cache(maxsize=None)
def reference(task):
    """the oracle on the stack's 2 n env-states with the explicit targets, computed once: (obs, reward, terms)"""
    _, _, (q, v, t, _, _), _ = stack()
    return tr.reference(model.default_params(), task, q, v, t)


def achieved_reference(q):
    """fp64 [n, 3] of states q [n, 16]"""
    w, x, y, z = (np.asarray(q, dtype=np.float64)[:, 3 + i] for i in range(4))
    a = np.arctan2(2 * (x * y + w * z), w * w + x * x - y * y - z * z) - PI / 2
    a = a + 2 * PI * np.floor((PI - a) / (2 * PI))
    return np.stack([q[:, 0], q[:, 1], a], axis=1)


def circular(d):
    d = np.abs(d) % (2 * PI)
    return np.minimum(d, 2 * PI - d)


def yaw_bound(P, q, v, t):
    """radians, per state: pi times the derived bound of face_direction's angle entry; and hypot(R00, R10)"""
    b = tr.bounds(P, "face_direction", q, v, t)
    return PI * b["obs"][:, ANGLE_ENTRY], b["h"]


def attained(P, q, v, goal, near_vertical):
    """Feeding the achieved goal back as the target under face_direction: (limit [n] on |obs[15]|, kept [n]).  limit = twice the angle
    entry's bound on the state with that target (once for the achieved yaw's own error, once for the entry's); kept = the bound is inside
    its cap (task_reference.assert_cap's: 1e-5, or 1e-5 / hypot(R00, R10) in the near-vertical family).  At most the near-vertical family
    may be left out: asserted here, it is a condition on the inputs."""
    b = tr.bounds(P, "face_direction", q, v, goal)
    b15 = b["obs"][:, ANGLE_ENTRY]
    kept = b15 <= np.where(near_vertical, tr.STRICT_ABS / b["h"], tr.STRICT_ABS)
    assert not (~kept & ~near_vertical).any(), "states outside the near-vertical family leave the cap: %r" % (np.nonzero(~kept & ~near_vertical)[0][:10],)
    assert (~kept).mean() <= near_vertical.mean()
    return 2 * b15, kept


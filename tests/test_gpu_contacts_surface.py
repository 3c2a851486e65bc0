"""The Python surface of the contact pass on the GPU: JitterbugVecEnv.contacts / foot_forces, Physics.contacts / data.ncon / data.contact /
contact_force, trajectory.record(contacts=True)."""
import os

import numpy as np
import pytest

from jitterbug_amd import model
from tests import forward_inputs as fi
from tests.test_gpu_forward import bits, load, make_env

pytestmark = pytest.mark.gpu


def test_a_robot_at_rest_is_carried_by_its_contacts():
    """dropped at rest for 200 steps: the feet's and the other geoms' z forces add up to the ground reaction, which is the weight"""
    env = make_env(4, random_pose=False)
    env.reset()
    for _ in range(200):
        env.step(np.zeros(4, dtype=np.float32))
    ff, c, gr = env.foot_forces(), env.contacts(), env.ground_reaction()
    assert ff.shape == (4, 4, 3) and np.array_equal(bits(ff), bits(c["geom_frc"][:, model.FOOT_GEOMS]))
    others = [g for g in range(model.NGEOM) if g not in model.FOOT_GEOMS]
    total = ff[:, :, 2].astype(np.float64).sum(1) + c["geom_frc"][:, others, 2].astype(np.float64).sum(1)
    # the bound of the sum checks: forward_inputs' fp32 bound of qfrc's force block, over the largest inertial term - at rest the weight
    # itself, M y = tau + J^T f with y ~ 0 - plus the block's floor
    P = model.default_params()
    weight = -P[model.P_GRAVITY + 2] * sum(P[model.P_BODY + b * model.BODY_STRIDE + model.B_MASS] for b in range(model.NBODY))
    bound = fi.FP32_BOUND[("qfrc", "force")] * (weight + fi.BLOCKS[("qfrc", "force")][1])
    print("feet %s N + others = %s N, ground reaction %s N, weight %.4f N, bound %.2e N" % (ff[:, :, 2].sum(1), total, gr[:, 2], weight, bound))
    assert np.abs(total - gr[:, 2]).max() <= bound
    assert np.all(np.abs(gr[:, 2] - weight) < 0.05 * weight) and (c["ncon"] >= 3).all() and not c["unconverged"].any()
    env.close()


def test_contacts_list_and_physics_data():
    from jitterbug_amd.jitterbug import Physics
    env = make_env(5)
    ctrl = load(env, "poses-moving", 20 + np.arange(5))
    c = env.contacts(ctrl)
    assert set(c) == {"ncon", "contact", "geom_frc", "unconverged", "slot_geoms", "list"}
    assert c["contact"].shape == (5, model.NCONTACT, 12) and c["ncon"].dtype == np.int32 and c["unconverged"].dtype == np.bool_
    assert c["slot_geoms"].shape == (model.NCONTACT, 2) and c["ncon"].max() >= 4
    for j in range(5):
        rows = c["list"][j]
        assert len(rows["dist"]) == c["ncon"][j] == int((c["contact"][j, :, 11] != 0).sum())
        assert ((rows["geom2"] >= 0) & (rows["geom2"] < model.NGEOM)).all() and ((rows["geom1"] == -1) | ((rows["geom1"] >= 4) & (rows["geom1"] < 20))).all()
        assert np.array_equal(rows["force"], c["contact"][j, rows["slot"], 6:9]) and (rows["dist"] < 0).all() and (rows["fn"] >= 0).all()
    # physics.data: the current state under a zero action
    zero = env.contacts()
    ph = Physics(env, 3)
    rows = zero["list"][3]
    assert ph.data.ncon == zero["ncon"][3] == len(ph.data.contact) and ph.data.ncon >= 1
    for i, rec in enumerate(ph.data.contact):
        assert rec.dist == float(rows["dist"][i]) and np.array_equal(rec.pos, rows["pos"][i].astype(np.float64))
        assert np.array_equal(rec.frame[0:3], rows["normal"][i].astype(np.float64)) and rec.geom1 == rows["geom1"][i] and rec.geom2 == rows["geom2"][i]
        F = rec.frame.reshape(3, 3)
        assert np.abs(F @ F.T - np.eye(3)).max() < 1e-6
        cf = ph.contact_force(i)
        assert cf.shape == (3,) and abs(cf[0] - rows["fn"][i]) <= 1e-6 * max(1.0, float(rows["fn"][i]))
        assert abs(np.linalg.norm(cf) - np.linalg.norm(rows["force"][i].astype(np.float64))) <= 1e-6 * max(1.0, float(rows["fn"][i]))
    one = ph.contacts(float(ctrl[3]))
    assert np.array_equal(bits(one["force"]), bits(c["list"][3]["force"])) and np.array_equal(one["geom2"], c["list"][3]["geom2"])
    env.close()


def test_record_with_contacts_equals_live_calls_and_survives_save_npz(tmp_path):
    from jitterbug_amd import trajectory
    K = 3
    acts = np.random.default_rng(3).uniform(-1, 1, (K, 5)).astype(np.float32)
    env, twin = make_env(5), make_env(5)
    load(env, "rollout", 100 + np.arange(5))
    load(twin, "rollout", 100 + np.arange(5))
    tr = trajectory.record(env, K, acts, contacts=True)
    assert tuple(tr.geom_frc.shape) == (K, 5, model.NGEOM, 3) and tuple(tr.ncon.shape) == (K, 5)
    for k in range(K):
        live = twin.contacts(acts[k])
        assert np.array_equal(bits(tr.geom_frc[k]), bits(live["geom_frc"])), k
        assert np.array_equal(tr.ncon[k].cpu().numpy(), live["ncon"]), k
        twin.step(acts[k])
    assert tr.ncon.max().item() >= 1
    path = os.path.join(str(tmp_path), "t.npz")
    tr.save_npz(path, [1, 4])
    z = np.load(path)
    assert np.array_equal(z["geom_frc"], tr.geom_frc[:, [1, 4]].cpu().numpy()) and np.array_equal(z["ncon"], tr.ncon[:, [1, 4]].cpu().numpy())
    plain = trajectory.record(env, 1, acts[:1])
    assert plain.geom_frc is None and plain.ncon is None
    with pytest.raises(ValueError):
        trajectory.record(env, 1, None, contacts=True)
    env.close(); twin.close()

"""The Python surface of the inertia pass on the GPU: JitterbugVecEnv.inertia / foot_jacobians and jitterbug.Physics.inertia / jacobian."""
import numpy as np
import pytest

from jitterbug_amd import model
from tests import inertia_inputs as ii
from tests.test_gpu_readout import load, make_env

pytestmark = pytest.mark.gpu


def test_vec_env_surface():
    env = make_env(5)
    load(env, "rollout", 200)
    r = env.inertia()
    assert sorted(r) == ["qM", "qfrc_actuator", "qfrc_bias", "qfrc_passive"]
    assert r["qM"].shape == (5, 15, 15) and all(r[k].shape == (5, 15) and r[k].dtype == np.float32 for k in ("qfrc_bias", "qfrc_passive", "qfrc_actuator"))
    block = r["qfrc_bias"].base
    assert block.shape == (5, 3, 15) and r["qfrc_passive"].base is block and r["qfrc_actuator"].base is block
    a = np.linspace(-1, 1, 5).astype(np.float32)
    full = env.inertia(a, qacc_smooth=True, jac=True)
    assert full["qacc_smooth"].shape == (5, 15) and full["jac"].shape == (5, 14, 6, 15)
    assert np.array_equal(full["qM"], r["qM"]) and np.array_equal(full["qfrc_bias"], r["qfrc_bias"])
    assert not np.array_equal(full["qfrc_actuator"], r["qfrc_actuator"])          # the action reaches the actuator row
    only = env.inertia(qM=False, qfrc=False, jac=True)
    assert sorted(only) == ["jac"] and np.array_equal(only["jac"], full["jac"])
    feet = env.foot_jacobians()
    assert feet.shape == (5, 4, 3, 15) and np.array_equal(feet, full["jac"][:, 10:, 0:3, :])
    assert len(model.JAC_NAMES) == 14 == ii.NJAC
    env.close()


def test_physics_surface():
    from jitterbug_amd.jitterbug import Physics
    env = make_env(5)
    load(env, "rollout", 200)
    ph = Physics(env, index=3)
    a = np.zeros(5, dtype=np.float32); a[3] = 0.7
    batch = env.inertia(a, qacc_smooth=True, jac=True)
    one = ph.inertia(0.7)
    assert sorted(one) == sorted(batch)
    for k in batch:
        assert np.array_equal(one[k], batch[k][3]), k
    jp, jr = ph.jacobian("foot1")
    blk = batch["jac"][3, model.JAC_NAMES.index("foot1")]
    assert model.JAC_NAMES.index("foot1") == 12 and jp.shape == jr.shape == (3, 15)
    assert np.array_equal(jp, blk[0:3]) and np.array_equal(jr, blk[3:6])
    jp0, _ = ph.jacobian("jitterbug")
    assert np.array_equal(jp0, batch["jac"][3, 0, 0:3])
    with pytest.raises(KeyError):
        ph.jacobian("no such body")
    env.close()

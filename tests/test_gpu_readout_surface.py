"""What is built on the readout pass: physics.named.data's geom_xpos / geom_xmat / xipos, JitterbugVecEnv.foot_contacts and
jitterbug_amd.trajectory.record - each against the batch readout itself (tests/test_gpu_readout.py holds that to the oracle)."""
import numpy as np
import pytest

from jitterbug_amd import model
from tests import readout_inputs as ri

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_env(n, **kw):
    from jitterbug_amd.vec_env import JitterbugVecEnv
    return JitterbugVecEnv(n, "move_to_pose", seed=7, **kw)


def test_named_data_gives_the_readout_rows_and_keeps_the_old_keys():
    from jitterbug_amd.jitterbug import Physics, _quat2mat
    env = make_env(64)
    q, v, t = ri.raw_states("poses-moving")
    env.set_state(q, v, t)
    frames = env.readout()["frames"]
    gq, _, gt = env.get_state()
    for i in (0, 41):
        d = Physics(env, i).named.data
        for name in ("foot1", "mass", "leg3upper_cyl", "coreBody1"):
            row = frames[i, model.FRAME_GEOM0 + model.GEOM_NAMES.index(name)]
            assert np.array_equal(d.geom_xpos[name], row[0:3]) and np.array_equal(d.geom_xmat[name], row[3:12])
        assert np.array_equal(d.geom_xmat["target"], frames[i, model.FRAME_TARGET, 3:12])
        for name in ("leg3lower", "jitterbug", "mass"):
            assert np.array_equal(d.xipos[name], frames[i, model.BODY_NAMES.index(name), 0:3])
        # the keys that existed: fp64, from get_state, exactly as before
        tz = model.default_params()[model.P_TARGETZ]
        assert np.array_equal(d.xpos["jitterbug"], gq[i, 0:3]) and np.array_equal(d.xquat["jitterbug"], gq[i, 3:7])
        assert np.array_equal(d.xmat["jitterbug"], _quat2mat(gq[i, 3:7]).reshape(-1))
        assert np.array_equal(d.geom_xpos["target"], np.array([gt[i, 0], gt[i, 1], tz])) and np.array_equal(d.xpos["target"], d.geom_xpos["target"])
        assert d.geom_xpos["target"].dtype == np.float64
        np.testing.assert_allclose(d.geom_xpos["target"], frames[i, model.FRAME_TARGET, 0:3], rtol=1e-6, atol=1e-7)
        for idx, key in ((d.geom_xpos, "foot5"), (d.geom_xmat, "jitterbug"), (d.xipos, "foot1")):
            with pytest.raises(KeyError, match="valid names"):
                idx[key]
    # the cache follows the state
    d = Physics(env, 3).named.data
    a = d.geom_xpos["foot2"]
    env.set_state(q[::-1].copy(), v, t)
    assert not np.array_equal(a, d.geom_xpos["foot2"])
    env.close()


def test_foot_contacts_are_the_foot_clearances():
    env = make_env(64)
    env.set_state(*ri.raw_states("poses"))
    fc = env.foot_contacts()
    cl = env.readout(frames=False, clearance=True)["clearance"]
    assert fc.shape == (64, 4) and fc.dtype == np.bool_
    assert np.array_equal(fc, cl[:, [7, 11, 15, 19]] < 0)
    assert fc.any() and not fc.all()
    ref = ri.reference("poses")
    decided = np.abs(ref.clear[:, [7, 11, 15, 19]]) > ri.TOL_C
    assert np.array_equal(fc[decided], (ref.clear[:, [7, 11, 15, 19]] < 0)[decided])
    env.close()


def test_record_is_the_live_readout_after_every_step_and_perturbs_nothing(tmp_path):
    import torch
    from jitterbug_amd import trajectory
    K, N = 5, 24
    env, twin = make_env(N), make_env(N)
    env.randomise_models(seed=5)
    twin.randomise_models(seed=5)
    actions = np.random.default_rng(4).uniform(-1, 1, (K, N)).astype(np.float32)
    env.reset()
    twin.reset()
    traj = trajectory.record(env, K, actions)
    assert tuple(traj.frames.shape) == (K + 1, N, 33, 12) and tuple(traj.clearance.shape) == (K + 1, N, 22) and tuple(traj.snapshots.shape) == (K + 1, env.snapshot_bytes)
    assert traj.frames.is_cuda and traj.n_steps == K
    dev = torch.device("cuda", 0)
    tape = torch.as_tensor(actions).to(dev)
    rows = torch.zeros((K, N, env.obs_dim + 2), device=dev)
    fr = torch.zeros((N, 33, 12), device=dev)
    cl = torch.zeros((N, 22), device=dev)
    torch.cuda.synchronize()
    for k in range(K + 1):
        if k:
            twin.step_many_device(1, tape[k - 1].data_ptr(), rows_ptr=rows[k - 1].data_ptr())
        twin.readout_device(fr.data_ptr(), cl.data_ptr())
        twin.synchronize()
        assert np.array_equal(bits(traj.frames[k]), bits(fr)), k
        assert np.array_equal(bits(traj.clearance[k]), bits(cl)), k
    assert np.array_equal(bits(traj.rows), bits(rows))
    assert all(np.array_equal(a, b) for a, b in zip(env.get_state() + env.counters(), twin.get_state() + twin.counters()))
    # with the device policy
    t2 = trajectory.record(env, 2)
    twin.step_many_device(2, None, rows_ptr=rows[:2].data_ptr())
    twin.synchronize()
    assert np.array_equal(bits(t2.rows), bits(rows[:2]))
    # the file: names and shapes
    path = str(tmp_path / "traj.npz")
    traj.save_npz(path, [3, 23])
    z = np.load(path)
    assert z["frames"].shape == (K + 1, 2, 33, 12) and z["clearance"].shape == (K + 1, 2, 22)
    assert np.array_equal(z["frames"].view(np.uint32), bits(traj.frames[:, [3, 23]]))
    assert list(z["geom_names"]) == list(model.GEOM_NAMES) and list(z["body_names"]) == list(model.BODY_NAMES)
    assert list(z["frame_names"]) == list(model.BODY_NAMES) + list(model.GEOM_NAMES) + ["target"] and list(z["envs"]) == [3, 23]
    assert z["geom_type"].shape == (2, 22) and z["geom_size"].shape == (2, 22, 3)
    assert np.array_equal(z["geom_type"][0], ri.geom_types(env.model_params(3)))
    g = env.model_params(23)[model.P_GEOM:].reshape(22, model.GEOM_STRIDE)
    assert np.array_equal(z["geom_size"][1], g[:, model.G_SIZE:model.G_SIZE + 3])
    env.close(); twin.close()

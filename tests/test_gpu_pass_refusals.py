"""What the three passes over states (readout, forward dynamics, contacts) refuse - one launch path in jb_api.hip (check_pass), one test:
a refusal names its reason, returns JB_E_INVALID and launches nothing; the same call succeeds once the reason is gone."""
import numpy as np
import pytest

from jitterbug_amd import _lib, model

pytestmark = pytest.mark.gpu
N = 5
# name -> (has a ctrl argument, number of outputs, which output the test asks for, that output's shape per env, its key in the Python method's dict)
PASSES = dict(readout=(False, 4, 0, (model.NFRAME, 12), "frames"), forward=(True, 5, 0, (15,), "qacc"), contacts=(True, 4, 2, (model.NGEOM, 3), "geom_frc"))


@pytest.mark.parametrize("name", sorted(PASSES))
def test_refusals_launch_nothing(name):
    import torch

    from jitterbug_amd.vec_env import JitterbugVecEnv
    has_ctrl, n_out, at, shape, key = PASSES[name]
    env = JitterbugVecEnv(N, "move_to_pose", seed=7)
    L, h = env._L, env._h
    buf = torch.full((N * int(np.prod(shape)),), -7.25, device=torch.device("cuda", 0), dtype=torch.float32)
    host = np.full((N,) + shape, -7.25, dtype=np.float32)
    torch.cuda.synchronize()
    outs = lambda p: [p if i == at else None for i in range(n_out)]
    device = lambda n_snaps, p: getattr(L, "jb_%s_device" % name)(h, None, n_snaps, *([None] if has_ctrl else []), *outs(p))
    on_host = lambda p: getattr(L, "jb_" + name)(h, *([None] if has_ctrl else []), *outs(p))
    p = buf.data_ptr()
    assert device(0, p) == -1 and b"n_snaps" in L.jb_last_error()
    assert device(-3, p) == -1
    assert device(2, p) == -1 and b"ONE state" in L.jb_last_error()
    assert device(1, None) == -1 and b"NULL" in L.jb_last_error()
    assert on_host(None) == -1 and b"NULL" in L.jb_last_error()
    env.step_async(np.zeros(N, dtype=np.float32))
    assert device(1, p) == -1 and b"pending" in L.jb_last_error()
    assert on_host(_lib.ptr(host)) == -1 and b"pending" in L.jb_last_error()
    env.step_wait()
    env.synchronize()
    assert (buf == -7.25).all().item() and (host == -7.25).all()
    assert device(1, p) == 0
    env.synchronize()
    assert torch.isfinite(buf).all().item() and not (buf == -7.25).any().item()
    assert model.NFRAME == 33
    env.release_staging()
    assert np.isfinite(getattr(env, name)()[key]).all()
    env.close()

"""The evaluate pass on the GPU (jb_evaluate_device / jb_evaluate, jitterbug_amd/csrc/jb_evaluate.hpp): bit equality with the observe and
reward-terms kernels and with the step kernels' rows on every kernel variant, a snapshot stack against the live passes, any task and any
target against the fp64 oracle on the seam batch (tests/task_reference.py: the derived bound with its cap, nothing fitted), the achieved
goal fed back as the target, and the refusals."""
import numpy as np
import pytest

from jitterbug_amd import _lib, model
from tests import evaluate_inputs as ei
from tests import task_reference as tr
from tests.test_gpu_task_seams import VARIANTS, _variant_env

pytestmark = pytest.mark.gpu
N = 19          # sixteen quads fill a wave, three are left ragged
TASK = "move_to_pose"


def _dev():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", params=VARIANTS)
def venv(request):
    env = _variant_env(request.param, N, TASK, seed=11)          # auto_reset=False, time_limit=inf; per-env models on the PAIR variants
    yield env
    env.close()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _evaluate_live(env, **kw):
    """one pass on the current state with all four outputs, as device tensors"""
    import torch
    n, D = env.num_envs, env.obs_dim
    out = dict(obs=torch.full((n, D), np.nan, device=_dev()), reward=torch.full((n,), np.nan, device=_dev()), terms=torch.full((n, 4), np.nan, device=_dev()),
               achieved=torch.full((n, 3), np.nan, device=_dev()))
    torch.cuda.synchronize()
    env.evaluate_device(obs_ptr=out["obs"].data_ptr(), reward_ptr=out["reward"].data_ptr(), terms_ptr=out["terms"].data_ptr(), achieved_ptr=out["achieved"].data_ptr(), **kw)
    env.synchronize()
    return out


def test_same_bits_as_the_observe_kernels(venv):
    """After reset() and 5 steps, the pass on the current state with the handle's own task and the stored target gives the words of
    jb_observe_device (obs, reward) and jb_reward_terms_device - on every step-kernel variant, per-env models (c0, target z) included."""
    import torch
    env = venv
    env.reset()
    rng = np.random.default_rng(21)
    for _ in range(5):
        env.step(rng.uniform(-1, 1, size=N).astype(np.float32))
    obs = torch.full((N, env.obs_dim), np.nan, device=_dev())
    rew, terms = torch.full((N,), np.nan, device=_dev()), torch.full((N, 4), np.nan, device=_dev())
    torch.cuda.synchronize()
    env.observe_device(obs.data_ptr(), rew.data_ptr())
    _lib.check(env._L.jb_reward_terms_device(env._h, terms.data_ptr()))
    got = _evaluate_live(env, task=-1)
    assert torch.isfinite(got["obs"]).all().item() and torch.isfinite(got["achieved"]).all().item()
    for key, ref in (("obs", obs), ("reward", rew), ("terms", terms)):
        same = _bits(got[key]) == _bits(ref)
        assert same.all(), "%s: %s differs from the observe kernels in %d words; first %r against %r" % (env.kernel_variant, key, (~same).sum(), got[key].cpu().numpy()[~same][:4], ref.cpu().numpy()[~same][:4])
    # the same through the task's name and through an absent-output launch
    only = torch.full((N,), np.nan, device=_dev())
    torch.cuda.synchronize()
    env.evaluate_device(task=TASK, reward_ptr=only.data_ptr())
    env.synchronize()
    assert np.array_equal(_bits(only), _bits(rew))


def test_a_stack_equals_the_live_passes_and_the_step_rows(venv):
    """Snapshots before and after each of 6 steps in one stack: ONE pass over the 7 snapshots equals the 7 live passes taken along the
    way, and rows 1 .. 6 equal the [obs | reward] columns of the rows the step kernel returned."""
    import torch
    env = venv
    D, K = env.obs_dim, 6
    env.reset()
    rng = np.random.default_rng(22)
    tape = torch.from_numpy(rng.uniform(-1, 1, size=(K, N)).astype(np.float32)).to(_dev())
    snaps = torch.zeros((K + 1, env.snapshot_bytes), dtype=torch.uint8, device=_dev())
    rows = torch.full((K, N, D + 2), np.nan, device=_dev())
    torch.cuda.synchronize()
    live = []
    for k in range(K + 1):
        if k:
            env.step_many_device(1, tape[k - 1].data_ptr(), rows[k - 1].data_ptr())
        env.snapshot_device(snaps[k].data_ptr())
        live.append(_evaluate_live(env))
    M = (K + 1) * N
    out = dict(obs=torch.full((M, D), np.nan, device=_dev()), reward=torch.full((M,), np.nan, device=_dev()), terms=torch.full((M, 4), np.nan, device=_dev()),
               achieved=torch.full((M, 3), np.nan, device=_dev()))
    torch.cuda.synchronize()
    env.evaluate_device(obs_ptr=out["obs"].data_ptr(), reward_ptr=out["reward"].data_ptr(), terms_ptr=out["terms"].data_ptr(), achieved_ptr=out["achieved"].data_ptr(),
                        snaps_ptr=snaps.data_ptr(), n_snaps=K + 1)
    env.synchronize()
    for key in out:
        stack = _bits(out[key]).reshape((K + 1, N) + tuple(out[key].shape[1:]))
        for k in range(K + 1):
            assert np.array_equal(stack[k], _bits(live[k][key])), (env.kernel_variant, key, k)
    r = _bits(rows)
    assert np.array_equal(_bits(out["obs"]).reshape(K + 1, N, D)[1:], r[:, :, :D]) and np.array_equal(_bits(out["reward"]).reshape(K + 1, N)[1:], r[:, :, D])
    assert (rows[:, :, D + 1] == 0).all().item()
    # the robots moved: the seven snapshots are seven different states
    a = out["achieved"].cpu().numpy().reshape(K + 1, N, 3)
    assert (np.abs(a[1:] - a[:-1]).max(axis=(1, 2)) > 0).all()


@pytest.fixture(scope="module")
def seam_env():
    """a handle of move_to_pose holding the seam batch with a decoy target stored; (env, state as the device holds it)"""
    from jitterbug_amd.vec_env import JitterbugVecEnv
    q, v, t, fams, nv = ei.seams()
    env = JitterbugVecEnv(len(q), "move_to_pose", auto_reset=False, time_limit=float("inf"))
    env.set_state(q, v, ei.decoy(t))
    qd, vd, td = env.get_state()
    assert np.array_equal(qd[:, :15], q[:, :15]) and np.array_equal(vd, v) and np.array_equal(td, ei.decoy(t))
    yield env, qd, vd
    env.close()


@pytest.fixture(scope="module")
def seam_env_other():
    """the same on a handle of face_direction (for move_to_pose as the override task)"""
    from jitterbug_amd.vec_env import JitterbugVecEnv
    q, v, t, fams, nv = ei.seams()
    env = JitterbugVecEnv(len(q), "face_direction", auto_reset=False, time_limit=float("inf"))
    env.set_state(q, v, ei.decoy(t))
    qd, vd, _ = env.get_state()
    yield env, qd, vd
    env.close()


@pytest.mark.parametrize("task", model.TASKS)
def test_any_task_any_target_against_fp64(seam_env, seam_env_other, params, task):
    """Each task as the OVERRIDE task on a handle created with another one, explicit targets from the seam batch (the stored target is a
    decoy): obs, reward and terms inside the derived bound around the oracle on the state the device holds, the bound inside its cap;
    achieved: the position words themselves, the yaw inside pi times the bound of face_direction's angle entry."""
    q, v, t, fams, nv = ei.seams()
    env, qd, vd = seam_env_other if task == "move_to_pose" else seam_env
    assert env.task != task
    o = env.evaluate(task, t, terms=True, achieved=True)
    assert o["obs"].shape == (len(q), model.OBS_DIM[task])
    ratios = tr.compare(task, params, qd, vd, t, o["obs"], o["reward"], o["terms"], list(fams), nv, "GPU evaluate")
    assert set(ratios) == set(fams)
    assert np.array_equal(o["achieved"][:, :2].view(np.uint32), qd[:, :2].astype(np.float32).view(np.uint32))
    yb, h = ei.yaw_bound(params, qd, vd, t)
    assert (yb / np.pi <= np.where(nv, tr.STRICT_ABS / h, tr.STRICT_ABS)).all()
    e_y = ei.circular(o["achieved"][:, 2].astype(np.float64) - ei.achieved_reference(qd)[:, 2])
    print("GPU evaluate, %s: achieved yaw worst err / bound %.3f" % (task, (e_y / yb).max()))
    assert (e_y <= yb).all(), np.nonzero(e_y > yb)[0][:10]
    # the state, the stored target included, is as it was
    assert np.array_equal(env.get_state()[2], ei.decoy(t))


def test_attaining_the_goal(seam_env, params):
    """The achieved goal fed back as the target under face_direction: |obs[15]| within twice the angle entry's bound wherever that bound is
    inside its cap; at most the near-vertical family is left out (evaluate_inputs.attained asserts the shares)."""
    q, v, t, fams, nv = ei.seams()
    env, qd, vd = seam_env
    goal = env.achieved_goals()
    limit, kept = ei.attained(params, qd, vd, goal.astype(np.float64), nv)
    ang = env.evaluate("face_direction", goal, reward=False)["obs"][:, ei.ANGLE_ENTRY].astype(np.float64)
    print("GPU attained: %d of %d kept, worst |obs[15]| / limit %.3f" % (kept.sum(), kept.size, (np.abs(ang[kept]) / limit[kept]).max()))
    assert (np.abs(ang[kept]) <= limit[kept]).all()
    # ... and as a position goal under move_to_position only the height difference is left
    tz = np.float32(params[model.P_TARGETZ])
    P = env.evaluate("move_to_position", goal, obs=False, reward=False, terms=True)["terms"][:, 0].astype(np.float64)
    assert np.abs(P - 0.1 ** ((20.0 * np.abs(np.float64(tz) - qd[:, 2])) ** 2)).max() <= tr.STRICT_ABS


def test_refusals_launch_nothing():
    """Every JB_E_INVALID case of the two entry points returns before anything is launched and names the function; after each refusal the
    handle still steps, and its row equals the row of a twin handle that saw no refusal."""
    import torch
    from jitterbug_amd.vec_env import JitterbugVecEnv
    n = 5
    env, twin = (JitterbugVecEnv(n, "move_to_pose", seed=7) for _ in range(2))
    env.reset(); twin.reset()
    L, h = env._L, env._h
    D = env.obs_dim
    buf = torch.full((2 * n * 19,), -7.25, device=_dev(), dtype=torch.float32)
    tg = torch.zeros((2 * n, 3), device=_dev(), dtype=torch.float32)
    host = np.full((n, 19), -7.25, dtype=np.float32)
    torch.cuda.synchronize()
    p, hp = buf.data_ptr(), _lib.ptr(host)
    rng = np.random.default_rng(3)

    def still_steps():
        a = rng.uniform(-1, 1, size=n).astype(np.float32)
        r1, r2 = env.step(a), twin.step(a)
        assert all(np.array_equal(x, y) for x, y in zip(r1[:3], r2[:3]))

    def refused(rc, fn, word):
        msg = L.jb_last_error()
        assert rc == -1 and fn in msg and word in msg, (rc, msg)
        env.synchronize()
        assert (buf == -7.25).all().item() and (host == -7.25).all()
        still_steps()

    dev = lambda snaps, n_snaps, task, t, o: L.jb_evaluate_device(h, snaps, n_snaps, task, t, o, None, None, None)
    refused(dev(None, 0, -1, None, p), b"jb_evaluate_device", b"n_snaps")
    refused(dev(None, -3, -1, None, p), b"jb_evaluate_device", b"n_snaps")
    refused(dev(None, 2, -1, None, p), b"jb_evaluate_device", b"ONE state")
    refused(dev(None, 1, -1, None, None), b"jb_evaluate_device", b"NULL")
    refused(dev(None, 1, -2, tg.data_ptr(), p), b"jb_evaluate_device", b"task_id")
    refused(dev(None, 1, 5, tg.data_ptr(), p), b"jb_evaluate_device", b"task_id")
    for other in (0, 1, 2, 3):
        refused(dev(None, 1, other, None, p), b"jb_evaluate_device", b"explicit targets")
    refused(L.jb_evaluate(h, -1, None, None, None, None, None), b"jb_evaluate:", b"NULL")
    refused(L.jb_evaluate(h, 7, None, hp, None, None, None), b"jb_evaluate:", b"task_id")
    refused(L.jb_evaluate(h, 3, None, hp, None, None, None), b"jb_evaluate:", b"explicit targets")
    # a pending jb_step_async: both forms refuse, and the pending step completes as the twin's ordinary step does
    a = rng.uniform(-1, 1, size=n).astype(np.float32)
    env.step_async(a)
    rc1, m1 = dev(None, 1, -1, None, p), L.jb_last_error()
    rc2, m2 = L.jb_evaluate(h, -1, None, hp, None, None, None), L.jb_last_error()
    r1, r2 = env.step_wait(), twin.step(a)
    assert rc1 == -1 and b"jb_evaluate_device" in m1 and b"pending" in m1 and rc2 == -1 and b"jb_evaluate:" in m2 and b"pending" in m2
    assert all(np.array_equal(x, y) for x, y in zip(r1[:3], r2[:3]))
    env.synchronize()
    assert (buf == -7.25).all().item() and (host == -7.25).all()
    still_steps()
    # the same calls succeed once the reason is gone: the handle's own task by its index without targets, another task with targets
    assert dev(None, 1, 4, None, p) == 0 and dev(None, 1, 1, tg.data_ptr(), p + 4 * n * 19) == 0
    env.synchronize()
    got = buf.cpu().numpy()
    assert np.isfinite(got[:n * D]).all() and not (got[:n * D] == -7.25).any() and (got[n * D:n * 19] == -7.25).all()
    assert not (got[n * 19:n * 19 + n * 16] == -7.25).any() and (got[n * 19 + n * 16:] == -7.25).all()
    assert np.array_equal(got[:n * D].reshape(n, D), env.observe()[0])
    env.release_staging()
    assert np.array_equal(env.evaluate()["obs"], env.observe()[0])
    still_steps()
    env.close(); twin.close()

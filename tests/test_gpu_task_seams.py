"""The task layer on the GPU (jb_task.hpp inlined into the observe, reward-terms, policy and step kernels) on states placed ON its branches -
tests/task_reference.py: seam_states(), the fp64 reference, the derived bound with its rounding counts and its cap - and the header's promise
that an observation and a reward have ONE set of bits whichever kernel computed them."""
import numpy as np
import pytest

from jitterbug_amd import model
from tests import task_reference as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seams():
    return tr.seam_states()


def _env(n, task, **kw):
    from jitterbug_amd.vec_env import JitterbugVecEnv
    return JitterbugVecEnv(n, task, auto_reset=False, time_limit=float("inf"), **kw)


@pytest.mark.parametrize("task", model.TASKS)
def test_seam_states_against_fp64(seams, params, task):
    """One batch of all families: set_state, get_state, observe (observation and reward), reward_terms.  Every observation entry, the task's
    reward and the four terms of EVERY state inside the derived bound around the oracle of the state the device holds; the bound inside its cap."""
    q, v, t, fams, nv = seams
    env = _env(len(q), task)
    env.set_state(q, v, t)
    qd, vd, td = env.get_state()
    assert np.array_equal(qd[:, :15], q[:, :15]) and np.array_equal(vd, v) and np.array_equal(td, t)          # fp32 words: held as given
    assert np.abs(qd[:, 15] - q[:, 15]).max() < 1e-3          # (the motor angle is held wrapped in fp32 next to its whole turns)
    obs, rew = env.observe()
    terms = env.reward_terms()
    env.close()
    ratios = tr.compare(task, params, qd, vd, td, obs, rew, terms, fams, nv, "GPU")
    assert set(ratios) == set(fams)


@pytest.mark.parametrize("policy", [None, tr.NON_DEFAULT_POLICY], ids=["default", "non_default"])
@pytest.mark.parametrize("task", model.TASKS)
def test_policy_across_its_thresholds(task, policy):
    """jb_policy on rows that walk every variable of heuristic_policy across its thresholds (task_reference.policy_rows: +-{3, 4, 8, 64} ulp) against
    policy_batch in fp64 on the same fp32 rows: every kept row to 2e-6, at most 1 % left out (within 4 ulp of a threshold behind atan2f)."""
    kw = policy or {}
    obs, keep = tr.policy_rows(task, **kw)
    assert (~keep).mean() <= 0.01
    env = _env(len(obs), task)
    if policy:
        env.set_policy_params(**policy)
    act = env.policy(obs)
    env.close()
    ref = tr.policy_reference(task, obs, **kw)
    err = np.abs(act.astype(np.float64) - ref)
    print("policy %s (%s): %d rows, %d left out, worst kept %.1e" % (task, "non-default" if policy else "default", len(obs), (~keep).sum(), err[keep].max()))
    assert err[keep].max() <= 2e-6, (np.nonzero(keep & (err > 2e-6))[0][:10], obs[keep & (err > 2e-6)][:4])


# ------------------------------------------------------------------------------------------------ one set of bits whichever kernel computed it
VARIANTS = ["ordinary", "lean", "pair", "lean_pair"]


def _variant_env(variant, n, task, **kw):
    from jitterbug_amd import _lib, augmented_jitterbug as aj
    flags = {"ordinary": 0, "pair": _lib.FLAG_PAIR, "lean": _lib.FLAG_LEAN, "lean_pair": _lib.FLAG_LEAN}[variant]
    params = None
    if variant in ("pair", "lean_pair"):
        pool = aj.augmented_params(16, seed=3)          # one model per env, out of a pool of 16
        params = pool[np.arange(n) % 16]
    env = _env(n, task, params=params, flags=flags, envs_per_wave=4, **kw)
    assert env.kernel_variant == variant
    return env


def _rows_against_observe(env, step):
    """step(rows_ptr) runs step launches that end in packed rows [.., N, D + 2]; returns (last rows, observe kernel's obs, reward) as numpy"""
    import torch
    dev = torch.device("cuda", 0)
    n, D = env.num_envs, env.obs_dim
    obs = torch.zeros((n, D), device=dev, dtype=torch.float32)
    rew = torch.zeros((n,), device=dev, dtype=torch.float32)
    rows = step(dev)
    env.observe_device(obs.data_ptr(), rew.data_ptr())
    env.synchronize()
    return rows.cpu().numpy().reshape(-1, n, D + 2)[-1], obs.cpu().numpy(), rew.cpu().numpy()


def _assert_same_bits(what, rows, obs, rew):
    D = obs.shape[1]
    assert np.isfinite(obs).all() and np.isfinite(rew).all(), what
    same_o, same_r = rows[:, :D].view(np.uint32) == obs.view(np.uint32), rows[:, D].view(np.uint32) == rew.view(np.uint32)
    assert same_o.all() and same_r.all(), "%s: the step kernel's row and the observe kernel differ in %d observation entries (columns %r) and %d rewards; first: %r against %r" % (
        what, (~same_o).sum(), sorted(set(np.nonzero(~same_o)[1].tolist())), (~same_r).sum(), rows[:, :D][~same_o][:4], obs[~same_o][:4])


def _single_and_fused(env, actions7, restart):
    """one control step with packed rows, then the last row of a 7-step launch, each against the observe kernel on the state it left"""
    import torch
    n, D = env.num_envs, env.obs_dim

    def one(dev):
        a = torch.from_numpy(actions7[0]).to(dev)
        rows = torch.zeros((n, D + 2), device=dev, dtype=torch.float32)
        env.step_rows_device(a.data_ptr(), rows.data_ptr())
        env.synchronize()
        return rows

    def seven(dev):
        a = torch.from_numpy(actions7).to(dev)
        rows = torch.zeros((7, n, D + 2), device=dev, dtype=torch.float32)
        env.step_many_device(7, actions_ptr=a.data_ptr(), rows_ptr=rows.data_ptr())
        env.synchronize()
        return rows

    restart()
    _assert_same_bits("%s, one step" % env.kernel_variant, *_rows_against_observe(env, one))
    restart()
    _assert_same_bits("%s, last of 7 fused steps" % env.kernel_variant, *_rows_against_observe(env, seven))


@pytest.mark.parametrize("task", ["move_in_direction", "move_to_pose"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_step_row_and_observe_kernel_have_the_same_bits_from_the_seams(seams, variant, task):
    """jb_task.hpp promises one set of bits whichever kernel computed an observation or a reward.  Contacts off, from the seam batch (the robots stay
    where they were put for a step): the row of one control step, and the last row of a 7-step launch, against jb_observe on the state left."""
    q, v, t, fams, nv = seams
    env = _variant_env(variant, len(q), task, contacts=False)
    rng = np.random.default_rng(4)
    actions = rng.uniform(-1, 1, size=(7, len(q))).astype(np.float32)
    _single_and_fused(env, actions, lambda: env.set_state(q, v, t))
    env.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_step_row_and_observe_kernel_have_the_same_bits_along_a_rollout(variant):
    """The same with contacts on along an ordinary rollout: reset, 30 steps with a third of the robots flat out, two waves and a ragged tail."""
    import torch
    n, task = 2 * 4 + 3, "move_to_pose"
    env = _variant_env(variant, n, task, seed=8)
    env.reset()
    rng = np.random.default_rng(5)
    dev = torch.device("cuda", 0)
    D = env.obs_dim
    for k in range(30):
        a = rng.uniform(-1, 1, size=n).astype(np.float32)
        a[::3] = 1.0

        def one(dev, a=a):
            ad = torch.from_numpy(a).to(dev)
            rows = torch.zeros((n, D + 2), device=dev, dtype=torch.float32)
            env.step_rows_device(ad.data_ptr(), rows.data_ptr())
            env.synchronize()
            return rows
        _assert_same_bits("%s, step %d of the rollout" % (variant, k), *_rows_against_observe(env, one))
    actions = rng.uniform(-1, 1, size=(7, n)).astype(np.float32)
    actions[:, ::3] = 1.0

    def seven(dev):
        ad = torch.from_numpy(actions).to(dev)
        rows = torch.zeros((7, n, D + 2), device=dev, dtype=torch.float32)
        env.step_many_device(7, actions_ptr=ad.data_ptr(), rows_ptr=rows.data_ptr())
        env.synchronize()
        return rows
    _assert_same_bits("%s, last of 7 fused steps after the rollout" % variant, *_rows_against_observe(env, seven))
    _, _, cap = env.counters()
    assert cap.sum() == 0
    env.close()

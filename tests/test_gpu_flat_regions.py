"""Lane predicates taken off register-only work in the substep loop ("no lane predicate on register-only work"): what used to
run under a narrowed exec mask now runs on every lane - idle lanes, helper lanes and lanes of a half-filled wave included - and its
result is kept or dropped by a select.  Nothing an idle lane computes may reach a result, whatever its registers or the scratch hold:

  * 70 envs (seventeen full four-env waves and a half-filled one), motor flat out for 300 control steps - the regime of the spread sweeps,
    rank-one passes and body slots: the same observations bit for bit with the scratch poisoned every third step and without, and with
    1, 2 and 4 envs per wave;
  * a fused launch of 7 control steps equals 7 single steps bit for bit, at 4 and at 8 envs per wave (6 envs: a partly idle wave)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_TIP, STEPS_TIP = 70, 300


def _flat_out(epw, poison):
    from jitterbug_amd.vec_env import JitterbugVecEnv
    env = JitterbugVecEnv(N_TIP, "move_from_origin", seed=5, envs_per_wave=epw)
    try:
        env.reset()
        a = np.ones(N_TIP, dtype=np.float32)
        obs = []
        for t in range(STEPS_TIP):
            if poison and t % 3 == 0:
                env.debug_poison_lds()
            ob = env.step(a)[0]
            if t % 50 == 49:
                obs.append(ob.copy())
        _, _, cap = env.counters()
        return np.stack(obs), int(cap.sum())
    finally:
        env.close()


@pytest.fixture(scope="module")
def reference_run():
    """4 envs per wave, no poison: computed once, compared against by every variant below"""
    obs, cap = _flat_out(4, False)
    obs.setflags(write=False)
    return obs, cap


def test_the_flat_out_run_is_finite_converged_and_tipped(reference_run):
    obs, cap = reference_run
    assert np.isfinite(obs).all()
    assert cap == 0                                       # every contact solve converged
    qt = obs[-1][:, 3:7]                                  # observation entries 3-6 are the root quaternion
    up = 1 - 2 * (qt[:, 1] ** 2 + qt[:, 2] ** 2)
    print("tipped (up < 0.5): %d of %d" % ((up < 0.5).sum(), N_TIP))
    assert (up < 0.5).mean() > 0.05


@pytest.mark.parametrize("epw,poison", [(4, True), (1, False), (2, False)], ids=["poisoned-lds", "one-env-per-wave", "two-envs-per-wave"])
def test_flat_out_bits_do_not_depend_on_the_scratch_or_on_wave_mates(reference_run, epw, poison):
    ref, _ = reference_run
    obs, cap = _flat_out(epw, poison)
    assert np.isfinite(obs).all() and cap == 0
    assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("epw", [4, 8])
def test_fused_launches_of_seven_steps_equal_single_steps(epw):
    import torch
    from jitterbug_amd.vec_env import JitterbugVecEnv
    n, steps, K = 6, 40, 7
    dev = torch.device("cuda", 0)
    a = JitterbugVecEnv(n, "move_from_origin", seed=7, envs_per_wave=epw)
    b = JitterbugVecEnv(n, "move_from_origin", seed=7, envs_per_wave=epw)
    try:
        assert a.envs_per_wave == epw and b.envs_per_wave == epw
        D = a.obs_dim
        g = torch.Generator(device=dev); g.manual_seed(11)
        tape = torch.rand((steps, n), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        a.reset_device(); b.reset_device()
        rows_a = torch.full((steps, n, D + 2), float("nan"), device=dev)
        rows_b = torch.full((steps, n, D + 2), float("nan"), device=dev)
        for k in range(steps):
            a.step_rows_device(tape[k].data_ptr(), rows_a[k].data_ptr())
        for k in range(0, steps, K):
            kk = min(K, steps - k)
            b.step_many_device(kk, tape[k:k + kk].data_ptr(), rows_ptr=rows_b[k:k + kk].data_ptr())
        a.synchronize(); b.synchronize()
        ra, rb = rows_a.cpu().numpy(), rows_b.cpu().numpy()
        assert np.isfinite(ra).all()
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
    finally:
        a.close(); b.close()

"""Contact rows built inside the first full Newton sweep of a substep (jb_sim.hpp contact_sweep, `build`): the lane that sweeps a
row forms it from the candidate, stores it for the later passes and applies the registers it holds.  What must not change:

  * an env's bits do not depend on its wave-mates - 1, 2 and 4 envs per wave share the slots out differently (four lane groups with idle
    lanes in most rounds against a fuller wave), so a row that an idle lane read before its owner built it would show here;
  * one fused launch of all the control steps equals single steps;
  * whatever the scratch holds between steps reaches no result (an idle lane of a building sweep has no built row to read: zeros by selects).

64 envs, motor flat out for 250 control steps: the smallest run in which robots end up lying on a leg - spread rounds with adopted
contacts, the all-geom path, body slots in the ordinary loop, idle lanes in a round."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS = 64, 250


def _flat_out(epw, poison=False):
    from jitterbug_amd.vec_env import JitterbugVecEnv
    env = JitterbugVecEnv(N, "move_from_origin", seed=5, envs_per_wave=epw)
    try:
        assert env.envs_per_wave == epw
        env.reset()
        a = np.ones(N, dtype=np.float32)
        obs = []
        for t in range(STEPS):
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
    """4 envs per wave (the flagship kernel), no poison: computed once, compared against by every case below"""
    obs, cap = _flat_out(4)
    obs.setflags(write=False)
    return obs, cap


def test_the_run_is_finite_and_reaches_the_tipped_regime(reference_run):
    obs, cap = reference_run
    assert np.isfinite(obs).all()
    qt = obs[-1][:, 3:7]                                  # observation entries 3-6 are the root quaternion
    up = 1 - 2 * (qt[:, 1] ** 2 + qt[:, 2] ** 2)
    print("tipped (up < 0.5): %d of %d, cap hits %d" % ((up < 0.5).sum(), N, cap))
    assert (up < 0.5).sum() >= 2


@pytest.mark.parametrize("epw", [1, 2])
def test_bits_do_not_depend_on_the_envs_per_wave(reference_run, epw):
    ref, _ = reference_run
    obs, _ = _flat_out(epw)
    assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32))


def test_poisoned_scratch_stays_finite_and_changes_no_bit(reference_run):
    ref, _ = reference_run
    obs, _ = _flat_out(4, poison=True)
    assert np.isfinite(obs).all()
    assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32))


def test_one_fused_launch_of_all_the_steps_equals_single_steps():
    import torch
    from jitterbug_amd.vec_env import JitterbugVecEnv
    dev = torch.device("cuda", 0)
    a = JitterbugVecEnv(N, "move_from_origin", seed=5, envs_per_wave=4)
    b = JitterbugVecEnv(N, "move_from_origin", seed=5, envs_per_wave=4)
    try:
        D = a.obs_dim
        tape = torch.ones((STEPS, N), device=dev, dtype=torch.float32)
        a.reset_device(); b.reset_device()
        rows_a = torch.full((STEPS, N, D + 2), float("nan"), device=dev)
        rows_b = torch.full((STEPS, N, D + 2), float("nan"), device=dev)
        for k in range(STEPS):
            a.step_rows_device(tape[k].data_ptr(), rows_a[k].data_ptr())
        b.step_many_device(STEPS, tape.data_ptr(), rows_ptr=rows_b.data_ptr())
        a.synchronize(); b.synchronize()
        ra, rb = rows_a.cpu().numpy(), rows_b.cpu().numpy()
        assert np.isfinite(ra).all()
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
    finally:
        a.close(); b.close()

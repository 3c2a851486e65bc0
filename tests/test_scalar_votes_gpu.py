"""Scalar votes (jb_lane.hpp main_vote, StepLayout::scalar_votes): after a check of the active set EVERY lane group decodes the
records, runs the rank-one pass and its selects, and every lane runs the substep's broadphase - the helper groups on whatever they hold -
while the decisions are votes of the main lanes alone.  Nothing a helper lane computes may reach a result.  The build is compared with
itself under perturbation, by the recipe of tests/test_group_liveness_gpu.py:

  * the LDS poisoned every third step against an undisturbed run: a helper lane whose junk records sent its rank-one pass to a word that
    nobody wrote, or whose result reached a store or a vote, would carry the poison on;
  * 4, 2 and 1 envs per wave: the main lanes are lanes 0-15, 0-7 and 0-3 of the wave - the mask main_vote restricts its ballot with - and
    the half-filled wave of the batch has main lanes that retired at the kernel's entry; an env's bits depend on none of that;
  * fused launches against single steps, at 4 and at 8 envs per wave (two lane groups, main lanes 0-31);
  * the PAIR kernel, whose helper groups 2 and 3 hold no state of their own in the broadphase.

Correctness against the oracle stays with the parity suite.  Shapes: 22 envs are five full four-env waves and a half-filled one; motor
flat out for 300 control steps tips a share of the robots (spread sweeps, grouped full sweeps, rank-one passes between the full ones).
One tipped robot puts its wave into that regime for the rest of the run and a helper lane's junk can only travel inside its wave, so the
run is asked for at least one (which robots tip within 300 steps is chaotic: no larger count can be promised for 22 envs without choosing
the seed by the kernel's own result)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, SEED = 22, 300, 5


def _flat_out(n, steps, epw, poison=False, params=None, variant="ordinary", every=50):
    from jitterbug_amd.vec_env import JitterbugVecEnv
    env = JitterbugVecEnv(n, "move_from_origin", seed=SEED, envs_per_wave=epw, params=params)
    try:
        assert env.envs_per_wave == epw and env.kernel_variant == variant
        env.reset()
        a = np.ones(n, dtype=np.float32)
        obs = []
        for t in range(steps):
            if poison and t % 3 == 0:
                env.debug_poison_lds()
            ob = env.step(a)[0]
            if t % every == every - 1:
                obs.append(ob.copy())
        _, _, cap = env.counters()
        return np.stack(obs), int(cap.sum())
    finally:
        env.close()


@pytest.fixture(scope="module")
def reference_run():
    """4 envs per wave (the flagship kernel), no poison: computed once, compared against by every case below"""
    obs, cap = _flat_out(N, STEPS, 4)
    obs.setflags(write=False)
    return obs, cap


def test_the_run_reaches_the_tipped_regime_without_a_cap_hit(reference_run):
    obs, cap = reference_run
    assert np.isfinite(obs).all()
    qt = obs[-1][:, 3:7]                                  # observation entries 3-6 are the root quaternion
    up = 1 - 2 * (qt[:, 1] ** 2 + qt[:, 2] ** 2)
    print("tipped (up < 0.5): %d of %d, cap hits %d" % ((up < 0.5).sum(), N, cap))
    assert (up < 0.5).sum() >= 1
    assert cap == 0


def test_poisoned_scratch_changes_no_bit(reference_run):
    ref, _ = reference_run
    obs, cap = _flat_out(N, STEPS, 4, poison=True)
    assert np.isfinite(obs).all() and cap == 0
    assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("epw", [2, 1])
def test_bits_do_not_depend_on_the_envs_per_wave(reference_run, epw):
    ref, _ = reference_run
    obs, cap = _flat_out(N, STEPS, epw)
    assert cap == 0
    assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("epw", [4, 8])
def test_fused_launches_of_seven_steps_equal_single_steps(epw):
    import torch
    from jitterbug_amd.vec_env import JitterbugVecEnv
    n, steps, k = 6, 40, 7
    dev = torch.device("cuda", 0)
    a = JitterbugVecEnv(n, "move_from_origin", seed=5, envs_per_wave=epw)
    b = JitterbugVecEnv(n, "move_from_origin", seed=5, envs_per_wave=epw)
    try:
        assert a.envs_per_wave == epw and b.envs_per_wave == epw
        D = a.obs_dim
        g = torch.Generator(device=dev); g.manual_seed(11)
        tape = (torch.rand((steps, n), generator=g, device=dev, dtype=torch.float32) * 2 - 1).contiguous()      # a uniform tape
        a.reset_device(); b.reset_device()
        rows_a = torch.full((steps, n, D + 2), float("nan"), device=dev)
        rows_b = torch.full((steps, n, D + 2), float("nan"), device=dev)
        for t in range(steps):
            a.step_rows_device(tape[t].data_ptr(), rows_a[t].data_ptr())
        for t in range(0, steps, k):          # 7, 7, 7, 7, 7 and a last launch of 5
            m = min(k, steps - t)
            b.step_many_device(m, tape[t].data_ptr(), rows_ptr=rows_b[t].data_ptr())
        a.synchronize(); b.synchronize()
        ra, rb = rows_a.cpu().numpy(), rows_b.cpu().numpy()
        assert np.isfinite(ra).all()
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
    finally:
        a.close(); b.close()


@pytest.fixture(scope="module")
def pair_inputs():
    """robots whose eccentric mass touches a front leg, one model per env: the PAIR kernel; the reference run at 4 envs per wave"""
    from tests.parity_inputs import mass_touching_models, tiled
    P = tiled(mass_touching_models(), 12)
    obs, cap = _flat_out(12, 100, 4, params=P, variant="pair", every=25)
    obs.setflags(write=False)
    return P, obs


def test_pair_kernel_poisoned_scratch_changes_no_bit(pair_inputs):
    P, ref = pair_inputs
    assert np.isfinite(ref).all()
    obs, _ = _flat_out(12, 100, 4, poison=True, params=P, variant="pair", every=25)
    assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32))


def test_pair_kernel_bits_do_not_depend_on_the_envs_per_wave(pair_inputs):
    P, ref = pair_inputs
    obs, _ = _flat_out(12, 100, 1, params=P, variant="pair", every=25)
    assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32))

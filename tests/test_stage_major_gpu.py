"""The order of independent instructions in the substep loop (tools/experiments/wait_states.txt): the transposed group reduction of a
full Newton sweep run stage by stage over batches of quadruples (jb_lane.hpp row_transpose_swap1 / _add1 / _swap2 / _add2,
StepLayout::stage_major: the ordinary kernel at 4 envs per wave) and the packed accumulations run term by term over all their accumulators
(jb_sim.hpp acc_root, row_residuals, StepLayout::term_major: every row but the PAIR kernel at 8 envs per wave).  No value may change.  The
library is compared with itself along the seams the reordered code sits on:

  * 4, 2 and 1 envs per wave, bit for bit: only at 4 envs per wave are the four lane groups 16 lanes apart - the stage-major reduction, its
    batches of 4 3 3 3 quadruples and their stores; 2 and 1 envs per wave reduce every value by the butterfly, in the same association.  A
    total that landed in another word, a swap's half read twice, a batch boundary that skipped a quadruple: any of it parts the rows;
  * the LDS poisoned every third step against an undisturbed run: the totals travel through the scratch, and a word of the hand-over that no
    batch stored would carry the poison to the main lanes;
  * fused launches against single steps at 4 and at 8 envs per wave (8: two lane groups, the accumulations alone);
  * the PAIR kernel at 4, 2 and 1 envs per wave: term-major accumulations with the pair contact's rows (its root columns scaled to zero)
    next to the element-major reduction it keeps.

Correctness against the oracle stays with the parity suite.  Shapes: those of tests/test_group_liveness_gpu.py, the smallest that reach the paths -
22 envs are five full four-env waves and a half-filled one; motor flat out for 300 control steps tips a share of the robots (measured there on
MI355X: 1 of 22 with seed 5), and the wave that holds a tipped robot runs grouped full sweeps, spread sweeps and rank-one passes from then on.
One tipped robot is what is asked for, for the reason given there: junk can only travel inside its wave."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, STEPS, SEED = 22, 300, 5


def _flat_out(n, steps, epw, poison=False, params=None, variant="ordinary", every=50):
    """(observations of every `every`-th step [steps / every, n, D], cap hits of the whole run)"""
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


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


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
    assert _same_bits(obs, ref)


@pytest.mark.parametrize("epw", [2, 1])
def test_bits_do_not_depend_on_the_envs_per_wave(reference_run, epw):
    ref, _ = reference_run
    obs, cap = _flat_out(N, STEPS, epw)
    assert cap == 0
    assert _same_bits(obs, ref)


@pytest.mark.parametrize("epw", [4, 8])
def test_fused_launches_of_seven_steps_equal_single_steps(epw):
    import torch
    from jitterbug_amd.vec_env import JitterbugVecEnv
    n, steps, k = 6, 40, 7
    dev = torch.device("cuda", 0)
    a = JitterbugVecEnv(n, "move_from_origin", seed=SEED, envs_per_wave=epw)
    b = JitterbugVecEnv(n, "move_from_origin", seed=SEED, envs_per_wave=epw)
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
            b.step_many_device(min(k, steps - t), tape[t].data_ptr(), rows_ptr=rows_b[t].data_ptr())
        a.synchronize(); b.synchronize()
        ra, rb = rows_a.cpu().numpy(), rows_b.cpu().numpy()
        assert np.isfinite(ra).all()
        assert _same_bits(ra, rb)
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
    assert _same_bits(obs, ref)


@pytest.mark.parametrize("epw", [2, 1])
def test_pair_kernel_bits_do_not_depend_on_the_envs_per_wave(pair_inputs, epw):
    P, ref = pair_inputs
    obs, _ = _flat_out(12, 100, epw, params=P, variant="pair", every=25)
    assert _same_bits(obs, ref)

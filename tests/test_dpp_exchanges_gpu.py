"""The quad and row exchanges of jb_lane.hpp (quad_sum, quad_rot, quad_bcast, quad_pick, the row rotations of xor_sum / xor_get) read
with bound_ctrl set: no lane of a full-mask quad permutation or row rotation lacks a source, so no value may change - only the copy the
tied "old" operand forced after every DPP move goes away (profiles/ab_dpp_forms.txt).  What must not change, on every kernel
variant:

  * an env's bits do not depend on its wave-mates: 1, 2 and 4 envs per wave, and the same envs as a batch that starts three envs later
    (every env then sits in another quad of another wave, next to other envs);
  * whatever the scratch holds between steps reaches no result;
  * one fused launch of 7 control steps equals seven single steps;
  * every contact solve converges (cap == 0) and every output is finite.

70 envs: not a multiple of the envs of a wave at 4 (or 8) envs per wave, so the last wave is a partial one.  The motor runs flat out: after
250 control steps robots lie on a leg, and the 30 recorded steps that follow run the spread sweeps (segmented quad sums, quad_pick, the
rotated tags) and the all-geom path next to walking robots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, SETTLE, STEPS = 70, 250, 30
VARIANTS = ["ordinary", "lean", "pair", "lean_pair"]
OTHER_EPW = {"ordinary": (1, 2), "lean": (1, 2), "pair": (1, 2), "lean_pair": ()}          # (the LEAN + PAIR kernel exists at 4 envs per wave only)


def _make(variant, epw=4, lo=0):
    """envs lo .. N-1 of the batch of N on the kernel `variant` (the PAIR kernels: one model per env out of a pool of 16)"""
    from jitterbug_amd import _lib, augmented_jitterbug as aj
    from jitterbug_amd.vec_env import JitterbugVecEnv
    flags = {"ordinary": 0, "pair": _lib.FLAG_PAIR, "lean": _lib.FLAG_LEAN, "lean_pair": _lib.FLAG_LEAN}[variant]
    params = aj.augmented_params(16, seed=3)[np.arange(lo, N) % 16] if variant in ("pair", "lean_pair") else None
    env = JitterbugVecEnv(N - lo, "move_from_origin", seed=5, env_offset=lo, params=params, flags=flags, envs_per_wave=epw)
    assert env.kernel_variant == variant and env.envs_per_wave == epw
    return env


def _flat_out(variant, epw=4, lo=0, poison=False):
    """(obs [STEPS, n, D], reward, done) as raw words, and the cap hits of the whole run"""
    env = _make(variant, epw, lo)
    try:
        env.reset()
        a = np.ones(N - lo, dtype=np.float32)
        out = []
        for t in range(SETTLE + STEPS):
            if poison and t % 3 == 0:
                env.debug_poison_lds()
            ob, rw, dn, _ = env.step(a)
            if t >= SETTLE:
                out.append(np.concatenate([ob, rw[:, None], dn[:, None].astype(np.float32)], axis=1))
        _, _, cap = env.counters()
        out = np.stack(out)
        assert np.isfinite(out).all()
        assert cap.sum() == 0, "%d contact solves ran into the iteration cap" % int(cap.sum())
        return out
    finally:
        env.close()


_REFERENCE = {}


@pytest.fixture
def reference():
    """4 envs per wave, the whole batch, no poison: computed once per variant, compared against by every case below"""
    def get(variant):
        if variant not in _REFERENCE:
            ref = _flat_out(variant)
            ref.setflags(write=False)
            _REFERENCE[variant] = ref
        return _REFERENCE[variant]
    return get


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_run_reaches_the_tipped_regime(reference, variant):
    rows = reference(variant)
    qt = rows[-1][:, 3:7]                                 # observation entries 3-6 are the root quaternion
    up = 1 - 2 * (qt[:, 1] ** 2 + qt[:, 2] ** 2)
    print("%s: tipped (up < 0.5) %d of %d" % (variant, (up < 0.5).sum(), N))
    assert (up < 0.5).sum() >= 2


@pytest.mark.parametrize("variant,epw", [(v, e) for v in VARIANTS for e in OTHER_EPW[v]])
def test_bits_do_not_depend_on_the_envs_per_wave(reference, variant, epw):
    assert _same_bits(_flat_out(variant, epw), reference(variant))


@pytest.mark.parametrize("variant", VARIANTS)
def test_bits_do_not_depend_on_the_wave_mates(reference, variant):
    """the batch without its first three envs: env i sits in quad i - 3, every wave holds another set of envs, the partial wave another number"""
    assert _same_bits(_flat_out(variant, lo=3), reference(variant)[:, 3:])


def test_poisoned_scratch_changes_no_bit(reference):
    assert _same_bits(_flat_out("ordinary", poison=True), reference("ordinary"))


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_fused_launch_of_seven_steps_equals_seven_single_steps(variant):
    import torch
    dev = torch.device("cuda", 0)
    a, b = _make(variant), _make(variant)
    try:
        D = a.obs_dim
        tape = torch.ones((SETTLE, N), device=dev, dtype=torch.float32)
        a.reset_device(); b.reset_device()
        a.step_many_device(SETTLE, tape.data_ptr()); b.step_many_device(SETTLE, tape.data_ptr())
        rows_a = torch.full((7, N, D + 2), float("nan"), device=dev)
        rows_b = torch.full((7, N, D + 2), float("nan"), device=dev)
        for k in range(7):
            a.step_rows_device(tape[k].data_ptr(), rows_a[k].data_ptr())
        b.step_many_device(7, tape.data_ptr(), rows_ptr=rows_b.data_ptr())
        a.synchronize(); b.synchronize()
        ra, rb = rows_a.cpu().numpy(), rows_b.cpu().numpy()
        assert np.isfinite(ra).all() and np.isfinite(rb).all()
        assert _same_bits(ra, rb)
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
        for env in (a, b):
            assert env.counters()[2].sum() == 0
    finally:
        a.close(); b.close()

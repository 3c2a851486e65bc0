"""The readout pass on the GPU (jb_readout_device / jb_readout; jitterbug_amd/csrc/jb_readout.hpp): every output against the oracle at the
state get_state returns, under the bounds of the fp32 host build (tests/readout_inputs.py); a stack of snapshots against single calls and
an env of a batch against the same state alone, bit for bit; absent outputs; the state left untouched (the refusals: tests/test_gpu_pass_refusals.py).

The kernel gives a quad of lanes to an env-state and 16 env-states to a block: N = 17 is one block plus one, N = 64 four whole blocks."""
import numpy as np
import pytest

from tests import readout_inputs as ri

pytestmark = pytest.mark.gpu

SHAPES = dict(frames=(ri.NF, 12), clearance=(ri.NG,), body_vel=(ri.NB, 6), energy=(8,))
KEYS = tuple(SHAPES)


def _torch():
    import torch
    return torch


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_env(n, **kw):
    from jitterbug_amd.vec_env import JitterbugVecEnv
    return JitterbugVecEnv(n, "move_to_pose", seed=7, **kw)


def load(env, name, first):
    """states first .. first + N of input `name` (wrapping round) into env; what get_state then returns must be the state the references
    were evaluated at"""
    q, v, t = ri.raw_states(name)
    idx = (first + np.arange(env.num_envs)) % q.shape[0]
    env.set_state(q[idx], v[idx], t[idx])
    got = env.get_state()
    for a, b in zip(got, ri.states(name)):
        assert np.array_equal(a, b[idx])
    return idx


def read_all(env, name, count):
    """the four outputs for states 0 .. count of input `name`, batch by batch through the host form"""
    out = {k: np.zeros((count,) + s, dtype=np.float32) for k, s in SHAPES.items()}
    n = env.num_envs
    for first in range(0, count, n):
        load(env, name, first)
        r = env.readout(frames=True, clearance=True, body_vel=True, energy=True)
        m = min(n, count - first)
        for k in KEYS:
            out[k][first:first + m] = r[k][:m]
    return out


CASES = [("poses", 64, 64), ("poses-moving", 17, 64), ("rollout", 64, 960), ("rollout", 17, 51), ("models", 8, 64), ("models-moving", 8, 64), ("models-moving", 1, 8)]


@pytest.mark.parametrize("name,n,count", CASES, ids=["%s-n%d" % (c[0], c[1]) for c in CASES])
def test_outputs_against_the_oracle(name, n, count):
    env = make_env(n)
    ref = ri.reference(name)
    if name.startswith("models"):
        P = ri.random_models()
        if n == 1:          # one env, one model per env: state j with table j, one after the other
            out = {k: np.zeros((count,) + s, dtype=np.float32) for k, s in SHAPES.items()}
            for j in range(count):
                env.set_model_params(P[j])
                load(env, name, j)
                r = env.readout(frames=True, clearance=True, body_vel=True, energy=True)
                for k in KEYS:
                    out[k][j] = r[k][0]
        else:
            env.set_model_params(P)
            out = read_all(env, name, count)
    else:
        out = read_all(env, name, count)
    ref.subset(slice(0, count)).check(out["frames"], out["clearance"], out["body_vel"], out["energy"], label="%s N=%d GPU" % (name, n))
    env.close()


def device_readout(env, mask=15, snaps=None, n_snaps=1, fill=float("nan")):
    """readout_device into fresh tensors filled with `fill`; bit k of mask: output k is present"""
    torch = _torch()
    dev = torch.device("cuda", 0)
    t = {k: torch.full((n_snaps * env.num_envs,) + s, fill, device=dev, dtype=torch.float32) for k, s in SHAPES.items()}
    torch.cuda.synchronize()
    ptr = [t[k].data_ptr() if mask >> i & 1 else None for i, k in enumerate(KEYS)]
    env.readout_device(*ptr, snaps_ptr=None if snaps is None else snaps.data_ptr(), n_snaps=n_snaps)
    env.synchronize()
    return {k: bits(t[k]) for k in KEYS}


def test_a_stack_of_snapshots_equals_single_calls_bit_for_bit():
    torch = _torch()
    env = make_env(17)
    snaps = torch.zeros((3, env.snapshot_bytes), device=torch.device("cuda", 0), dtype=torch.uint8)
    torch.cuda.synchronize()
    live = []
    for k in range(3):
        load(env, "rollout", 300 + 17 * k)
        env.snapshot_device(snaps[k].data_ptr())
        live.append(device_readout(env))
    stack = device_readout(env, snaps=snaps, n_snaps=3)
    for k in range(3):
        one = device_readout(env, snaps=snaps[k], n_snaps=1)
        for key in KEYS:
            assert np.array_equal(stack[key][17 * k:17 * k + 17], one[key]), (k, key)
            assert np.array_equal(one[key], live[k][key]), (k, key)
    assert not np.array_equal(stack["frames"][:17], stack["frames"][17:34])
    env.close()


def test_an_env_of_a_batch_equals_the_same_state_alone_bit_for_bit():
    env, solo = make_env(64), make_env(1)
    load(env, "poses-moving", 0)
    whole = device_readout(env)
    for j in (0, 5, 37, 63):
        load(solo, "poses-moving", j)
        one = device_readout(solo)
        for key in KEYS:
            assert np.array_equal(whole[key][j], one[key][0]), (j, key)
    env.close(); solo.close()


def test_absent_outputs_leave_the_present_ones_unchanged_and_store_nothing():
    env = make_env(17)
    load(env, "poses-moving", 20)
    full = device_readout(env)
    sentinel = bits(np.float32(-7.25))
    for mask in range(1, 15):
        got = device_readout(env, mask=mask, fill=-7.25)
        for i, key in enumerate(KEYS):
            if mask >> i & 1:
                assert np.array_equal(got[key], full[key]), (mask, key)
            else:
                assert (got[key] == sentinel).all(), (mask, key)
    env.close()


def test_the_pass_does_not_touch_the_state():
    torch = _torch()
    env, twin = make_env(64), make_env(64)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(5)
    tape = torch.rand((8, 64), generator=g, device=dev, dtype=torch.float32) * 2 - 1
    before, after = (torch.zeros(env.snapshot_bytes, device=dev, dtype=torch.uint8) for _ in range(2))
    rows = [torch.zeros((3, 64, env.obs_dim + 2), device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for e in (env, twin):
        e.reset_device()
        e.step_many_device(5, tape[:5].data_ptr())
    env.snapshot_device(before.data_ptr())
    device_readout(env)
    env.readout(frames=True, clearance=True, body_vel=True, energy=True)
    env.snapshot_device(after.data_ptr())
    env.synchronize()
    assert torch.equal(before, after)
    for e, r in zip((env, twin), rows):
        e.step_many_device(3, tape[5:].data_ptr(), rows_ptr=r.data_ptr())
        e.synchronize()
    assert np.array_equal(bits(rows[0]), bits(rows[1]))
    env.close(); twin.close()

"""The forward-dynamics pass on the GPU (jb_forward_device / jb_forward; jb_forward_kernel in jitterbug_amd/csrc/jb_api.hip, element function
jb_forward.hpp): every output against the oracle under the bounds of the fp32 host build (tests/forward_inputs.py: three times the host's
measured worst, per output block); the shapes at which the indexing can go wrong, bit for bit; the state, the counters and the solver
statistics left untouched; agreement with the step kernel's own first substep; the Python surface (the refusals: tests/test_gpu_pass_refusals.py).

The kernel gives a wave to four env-states (a quad of lanes each, three mirror groups): N = 1 is one quad with the rest of its wave
repeating it, N = 5 a full wave plus a ragged one, and a stack of snapshots starts a new wave at every snapshot."""
import numpy as np
import pytest

from jitterbug_amd import _lib, model
from tests import forward_inputs as fi

pytestmark = pytest.mark.gpu

SHAPES = dict(qacc=(15,), qfrc=(15,), body_acc=(10, 6), motor=(3,))
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


def load(env, name, idx):
    """states idx of family `name` into env (its tables too where the family has one per state); what get_state then returns must be the
    state the references were evaluated at"""
    f = fi.family(name)
    idx = np.asarray(idx)
    assert len(idx) == env.num_envs
    if f.n_models > 1:
        env.set_model_params(f.tables_per_env()[idx])
    q, v, t = f.raw
    env.set_state(q[idx], v[idx], t[idx])
    got = env.get_state()
    for a, b in zip(got, (f.q, f.v, f.t)):
        assert np.array_equal(a, b[idx])
    return f.ctrl[idx].astype(np.float32)


def host_forward(env, ctrl):
    r = env.forward(ctrl, qacc=True, qfrc=True, body_acc=True, motor=True)
    return {"qacc": r["qacc"], "qfrc": r["qfrc_constraint"], "body_acc": r["body_acc"], "motor": r["motor"]}, r["unconverged"]


def device_forward(env, ctrl=None, mask=31, snaps=None, n_snaps=1, fill=float("nan")):
    """forward_device into fresh tensors filled with `fill`; bit k of mask: output k (qacc, qfrc, body_acc, motor, unconverged) is present.
    ctrl: float32 [n_snaps * N] or None.  -> ({output: bit patterns}, unconverged uint8)"""
    torch = _torch()
    dev = torch.device("cuda", 0)
    m = n_snaps * env.num_envs
    t = {k: torch.full((m,) + s, fill, device=dev, dtype=torch.float32) for k, s in SHAPES.items()}
    un = torch.full((m,), 77, device=dev, dtype=torch.uint8)
    c = None if ctrl is None else torch.as_tensor(np.ascontiguousarray(ctrl, dtype=np.float32)).to(dev)
    torch.cuda.synchronize()
    ptr = [t[k].data_ptr() if mask >> i & 1 else None for i, k in enumerate(KEYS)]
    env.forward_device(None if c is None else c.data_ptr(), *ptr, unconverged_ptr=un.data_ptr() if mask >> 4 & 1 else None,
                       snaps_ptr=None if snaps is None else snaps.data_ptr(), n_snaps=n_snaps)
    env.synchronize()
    return {k: bits(t[k]) for k in KEYS}, un.cpu().numpy()


def rollout_pick():
    """64 rollout states: flight and every contact count 1 .. 9 (up to six of each, in order of appearance), filled up from the front"""
    ncon = fi.reference("rollout").ncon
    pick = [int(j) for c in range(10) for j in np.nonzero(ncon == c)[0][:6]]
    assert set(ncon[pick]) == set(range(10))
    rest = [j for j in range(ncon.size) if j not in set(pick)]
    return np.array(sorted(pick + rest[:64 - len(pick)]))


# ------------------------------------------------------------------------------------------------ (a) parity with the oracle
PARITY = [("rollout", "ordinary"), ("poses-moving", "ordinary"), ("models-moving", "pair"), ("mass-touching", "pair"), ("thread-touching", "pair")]


@pytest.mark.parametrize("name,variant", PARITY, ids=[p[0] for p in PARITY])
def test_outputs_against_the_oracle(name, variant):
    f = fi.family(name)
    idx = rollout_pick() if name == "rollout" else np.arange(f.n)
    env = make_env(len(idx))
    ctrl = load(env, name, idx)
    assert env.kernel_variant == variant
    out, un = host_forward(env, ctrl)
    ref = fi.reference(name)
    print("%s: %d env-states, %d excluded, unconverged %d" % (name, len(idx), (~ref.strict[idx]).sum(), un.sum()))
    assert not un.any()          # (the excluded env-states included)
    fi.check(name, out, fi.FP32_BOUND, "GPU N=%d" % len(idx), idx=idx)
    # the same through device pointers, bit for bit
    dev, un2 = device_forward(env, ctrl)
    for k in KEYS:
        assert np.array_equal(dev[k], bits(out[k])), k
    assert not un2.any()
    gr = env.ground_reaction(ctrl)
    assert np.array_equal(bits(gr), bits(out["qfrc"][:, 0:3]))
    env.close()


# ------------------------------------------------------------------------------------------------ (b) shapes
def test_a_stack_of_snapshots_equals_single_calls_bit_for_bit():
    torch = _torch()
    env = make_env(5)
    snaps = torch.zeros((3, env.snapshot_bytes), device=torch.device("cuda", 0), dtype=torch.uint8)
    torch.cuda.synchronize()
    live, ctrls = [], []
    for k in range(3):
        ctrls.append(load(env, "rollout", 300 + 5 * k + np.arange(5)))
        env.snapshot_device(snaps[k].data_ptr())
        live.append(device_forward(env, ctrls[k]))
    stack, un = device_forward(env, np.concatenate(ctrls), snaps=snaps, n_snaps=3)
    assert not un.any()
    for k in range(3):
        one, un1 = device_forward(env, ctrls[k], snaps=snaps[k], n_snaps=1)
        for key in KEYS:
            assert np.array_equal(stack[key][5 * k:5 * k + 5], one[key]), (k, key)
            assert np.array_equal(one[key], live[k][0][key]), (k, key)
    assert not np.array_equal(stack["qacc"][:5], stack["qacc"][5:10])
    fi.check("rollout", {k: stack[k].view(np.float32) for k in KEYS}, fi.FP32_BOUND, "GPU stack 3 x 5", idx=300 + np.arange(15))
    # no action tape: action 0
    zero, _ = device_forward(env, None, snaps=snaps, n_snaps=3)
    same, _ = device_forward(env, np.zeros(15, dtype=np.float32), snaps=snaps, n_snaps=3)
    for key in KEYS:
        assert np.array_equal(zero[key], same[key])
    assert not np.array_equal(zero["motor"], stack["motor"])
    env.close()


@pytest.mark.parametrize("name,n", [("rollout", 5), ("models-moving", 5)])
def test_an_env_of_a_batch_equals_the_same_state_alone_bit_for_bit(name, n):
    env, solo = make_env(n), make_env(1, flags=_lib.FLAG_PAIR if fi.family(name).pair else 0)      # (one table is a shared model: ask for the batch's kernel)
    first = 200 if name == "rollout" else 10
    idx = first + np.arange(n)
    ctrl = load(env, name, idx)
    whole, _ = device_forward(env, ctrl)
    for j in range(n):
        c1 = load(solo, name, idx[j:j + 1])
        one, un = device_forward(solo, c1)
        for key in KEYS:
            assert np.array_equal(whole[key][j], one[key][0]), (j, key)
        assert un[0] == 0
    fi.check(name, {k: whole[k].view(np.float32) for k in KEYS}, fi.FP32_BOUND, "GPU N=%d" % n, idx=idx)
    env.close(); solo.close()


def test_absent_outputs_and_poisoned_lds_change_nothing():
    env = make_env(5)
    ctrl = load(env, "poses-moving", 20 + np.arange(5))
    full, un = device_forward(env, ctrl)
    sentinel = bits(np.float32(-7.25))
    for mask in (1, 2, 4, 8, 16, 3, 5, 10, 12, 22, 30):
        got, un2 = device_forward(env, ctrl, mask=mask, fill=-7.25)
        for i, key in enumerate(KEYS):
            if mask >> i & 1:
                assert np.array_equal(got[key], full[key]), (mask, key)
            else:
                assert (got[key] == sentinel).all(), (mask, key)
        assert np.array_equal(un2, un) if mask >> 4 & 1 else (un2 == 77).all()
    env.debug_poison_lds()
    again, un3 = device_forward(env, ctrl)
    for key in KEYS:
        assert np.array_equal(again[key], full[key]), key
    assert np.array_equal(un3, un)
    env.close()


# ------------------------------------------------------------------------------------------------ (c) read-only
def test_the_pass_does_not_touch_the_state_the_counters_or_the_solver_statistics():
    torch = _torch()
    env = make_env(64)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev); g.manual_seed(5)
    tape = torch.rand((5, 64), generator=g, device=dev, dtype=torch.float32) * 2 - 1
    before, after = (torch.zeros(env.snapshot_bytes, device=dev, dtype=torch.uint8) for _ in range(2))
    torch.cuda.synchronize()
    env.reset_device()
    env.step_many_device(5, tape.data_ptr())
    env.snapshot_device(before.data_ptr())
    env.synchronize()
    counters, stats = env.counters(), env.solver_stats()
    device_forward(env, tape[0].cpu().numpy())
    host_forward(env, tape[1].cpu().numpy())
    env.snapshot_device(after.data_ptr())
    env.synchronize()
    assert torch.equal(before, after)
    for a, b in zip(counters, env.counters()):
        assert np.array_equal(a, b)
    assert env.solver_stats() == stats
    env.close()


# ------------------------------------------------------------------------------------------------ (d) consistency with the step kernel
# Distance between forward()'s qacc and the warm-start words the step kernel leaves after ONE substep from the same state with the same
# action, in units in the last place of the block's largest entry in that env-state (an entry near zero is a cancellation of entries of
# that size; both sides are fp32 and no integration lies between them).  Measured on the MI355X over the 16 states below: 8.0 - the two
# kernels inline the same substep source, and the compiler contracts its multiply-adds differently in the two; against the oracle the same
# entries are four orders of magnitude further away (test_outputs_against_the_oracle).  Asserted: three times it.
STEP_ULP_MEASURED = 8.0


def _warm_start(env):
    """qacc [N, 15] in qvel order from the warm-start words of the current state's snapshot (save_state: 64-byte header, then the blocks)"""
    n = env.num_envs
    w = env.save_state()[64:].view(np.float32)
    root = w[:32 * n].reshape(32, n)
    leg = w[32 * n:(32 + 24) * n].reshape(6, n, 4)
    y = np.zeros((n, 15), dtype=np.float32)
    y[:, 0:3] = root[19:22].T; y[:, 3:6] = root[16:19].T; y[:, 14] = root[22]
    y[:, 6:14:2] = leg[4]; y[:, 7:14:2] = leg[5]
    return y


def _block_ulps(a, b):
    worst = 0.0
    for (o, blk), (sl, _) in fi.BLOCKS.items():
        if o == "qacc":
            top = np.abs(b[:, sl]).max(1)
            ulp = np.spacing(np.maximum(top, np.float32(1e-30)).astype(np.float32)).astype(np.float64)
            worst = max(worst, (np.abs(a[:, sl].astype(np.float64) - b[:, sl].astype(np.float64)).max(1) / ulp).max())
    return worst


@pytest.mark.parametrize("variant", ("ordinary", "lean"))
def test_qacc_is_what_one_step_of_one_substep_leaves_in_the_warm_start(variant):
    idx = rollout_pick()[::4]
    env = make_env(len(idx), control_timestep=0.0002, variant=variant, envs_per_wave=4, auto_reset=False, time_limit=float("inf"))
    assert env.substeps == 1 and env.kernel_variant == variant and env.envs_per_wave == 4 and len(idx) == 16
    ctrl = load(env, "rollout", idx)
    out, un = host_forward(env, ctrl)
    env.step(ctrl)
    y = _warm_start(env)
    ulps = _block_ulps(out["qacc"], y)
    print("%s handle: forward qacc against the step's warm start: %.1f ulp of the block's largest entry" % (variant, ulps))
    assert np.abs(y).max() > 100.0 and not un.any()
    if variant == "ordinary":
        assert ulps <= 3 * STEP_ULP_MEASURED
    else:          # the LEAN step kernel fuses multiply-adds differently: the fp32 bound of the parity test
        for (o, blk), (sl, floor) in fi.BLOCKS.items():
            if o == "qacc":
                e = np.abs(out["qacc"][:, sl].astype(np.float64) - y[:, sl]).max(1) / (np.abs(y[:, sl]).max(1) + floor)
                print("lean handle qacc/%s: %.3e (bound %.3e)" % (blk, e.max(), fi.FP32_BOUND[(o, blk)]))
                assert e.max() <= fi.FP32_BOUND[(o, blk)]
    env.close()


# (refusals: tests/test_gpu_pass_refusals.py, one test for the three passes)


# ------------------------------------------------------------------------------------------------ (f) surface
def test_python_surface():
    from jitterbug_amd import trajectory
    from jitterbug_amd.jitterbug import Physics
    env = make_env(5)
    ctrl = load(env, "rollout", 100 + np.arange(5))
    r = env.forward(ctrl)
    assert set(r) == {"qacc", "qfrc_constraint", "unconverged"} and r["qacc"].shape == (5, 15) and r["unconverged"].dtype == np.bool_
    full = env.forward(ctrl, body_acc=True, motor=True)
    assert full["body_acc"].shape == (5, model.NBODY, 6) and full["motor"].shape == (5, 3)
    assert np.array_equal(bits(full["qacc"]), bits(r["qacc"]))
    gr = env.ground_reaction(ctrl)
    assert gr.shape == (5, 3) and np.array_equal(bits(gr), bits(r["qfrc_constraint"][:, 0:3]))
    ph = Physics(env, 3)
    one = ph.forward(float(ctrl[3]))
    assert set(one) == {"qacc", "qfrc_constraint"} and np.array_equal(bits(one["qacc"]), bits(r["qacc"][3])) and np.array_equal(bits(one["qfrc_constraint"]), bits(r["qfrc_constraint"][3]))
    # a standing robot is carried by the floor: the ground reaction of the reset pose, once it has settled, is its weight
    rest = make_env(4, random_pose=False)
    rest.reset()
    for _ in range(20):
        rest.step(np.zeros(4, dtype=np.float32))
    P = model.default_params()
    weight = -P[model.P_GRAVITY + 2] * sum(P[model.P_BODY + b * model.BODY_STRIDE + model.B_MASS] for b in range(model.NBODY))
    fz = rest.ground_reaction()[:, 2]
    print("ground reaction of a robot at rest %s N, weight %.4f N" % (fz, weight))
    assert np.all(np.abs(fz - weight) < 0.05 * weight)
    rest.close()
    # record(forces=True): row k is a live forward before step k with action k
    K = 3
    acts = np.random.default_rng(3).uniform(-1, 1, (K, 5)).astype(np.float32)
    twin = make_env(5)
    load(twin, "rollout", 100 + np.arange(5))
    tr = trajectory.record(env, K, acts, forces=True)
    assert tuple(tr.qfrc.shape) == (K, 5, 15)
    for k in range(K):
        live = twin.forward(acts[k])["qfrc_constraint"]
        assert np.array_equal(bits(tr.qfrc[k]), bits(live)), k
        twin.step(acts[k])
    assert trajectory.record(env, 1, acts[:1]).qfrc is None
    with pytest.raises(ValueError):
        trajectory.record(env, 1, None, forces=True)
    env.close(); twin.close()

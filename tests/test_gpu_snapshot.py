"""Exact snapshot / restore / fork of the simulator state and the on-device tape scorer (jb_snapshot_device, jb_restore_device,
jb_snapshot, jb_restore, jb_score_tapes_device; jitterbug_amd/csrc/jb_snapshot.hpp) and the MPPI planner built on them.

A restored handle continues BIT FOR BIT - rows, state and counters, across an in-kernel auto-reset - for a ragged tail wave, the
per-env-model kernels and the LEAN kernels; get_state() / set_state() does not (shown as a control)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [
    # (label, n_envs, kwargs, randomise, kernel variant)
    ("n37-ragged", 37, dict(envs_per_wave=2), False, "ordinary"),
    ("n256-pair", 256, dict(), True, "pair"),
    ("n256-lean", 256, dict(flags=2), False, "lean"),
    ("n1024-lean-pair", 1024, dict(flags=2), True, "lean_pair"),
]
CASE_IDS = [c[0] for c in CASES]
PRE, K = 20, 25          # steps before the snapshot; steps after it (time_limit = 0.3 s = 30 steps: the roll crosses the auto-reset)


def _torch():
    import torch
    return torch


def bits(t):
    """float tensor / array -> uint32 bit patterns (NaN-safe exact comparison)"""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def full_state(env):
    return tuple(env.get_state()) + tuple(env.counters())


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def make_env(label):
    from jitterbug_amd.vec_env import JitterbugVecEnv
    _, n, kw, randomise, variant = CASES[CASE_IDS.index(label)]
    env = JitterbugVecEnv(n, "move_to_pose", seed=7, time_limit=0.3, **kw)
    if randomise:
        env.randomise_models(seed=5, return_params=False)
    assert env.kernel_variant == variant
    return env


class Case:
    """One env per case, built once: PRE steps, a device snapshot and a host blob of that state, then the UNINTERRUPTED continuation -
    K steps with packed rows - which every test compares against after restoring.  The reference is never written again."""

    def __init__(self, label):
        torch = _torch()
        self.dev = dev = torch.device("cuda", 0)
        self.env = env = make_env(label)
        self.n, self.D = n, D = env.num_envs, env.obs_dim
        g = torch.Generator(device=dev); g.manual_seed(3)
        tape = torch.rand((PRE + K, n), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        tape[:, : n // 3] = 1.0          # a third of the robots flat out: some tip over
        self.pre, self.tape = tape[:PRE].contiguous(), tape[PRE:].contiguous()
        self.snap = torch.zeros(env.snapshot_bytes, device=dev, dtype=torch.uint8)
        rows = torch.full((K, n, D + 2), float("nan"), device=dev)
        torch.cuda.synchronize()
        env.reset_device()
        env.step_many_device(PRE, self.pre.data_ptr())
        env.snapshot_device(self.snap.data_ptr())
        self.blob = env.save_state()                 # (synchronous: the same state as the device snapshot)
        self.at_snapshot = full_state(env)
        env.step_many_device(K, self.tape.data_ptr(), rows_ptr=rows.data_ptr())
        env.synchronize()
        self.rows = rows.cpu().numpy()
        self.rows.setflags(write=False)
        self.after = full_state(env)
        assert np.isfinite(self.rows).all()
        done = self.rows[:, :, D + 1]
        assert done[30 - PRE - 1].all() and done.sum() == n, "every env finishes exactly one episode inside the roll"

    def roll(self):
        """K steps of the case's tape from the env's current state -> packed rows (numpy)"""
        torch = _torch()
        rows = torch.full((K, self.n, self.D + 2), float("nan"), device=self.dev)
        torch.cuda.synchronize()
        self.env.step_many_device(K, self.tape.data_ptr(), rows_ptr=rows.data_ptr())
        self.env.synchronize()
        return rows.cpu().numpy()


_cases = {}


@pytest.fixture(scope="module")
def case():
    def get(label):
        if label not in _cases:
            _cases[label] = Case(label)
        return _cases[label]
    yield get
    for c in _cases.values():
        c.env.close()
    _cases.clear()


# ---------------------------------------------------------------------------------------------- 1. rewind
@pytest.mark.parametrize("label", CASE_IDS)
def test_restore_rewinds_bit_for_bit_and_set_state_does_not(case, label):
    c = case(label)
    env = c.env
    env.restore_device(c.snap.data_ptr())
    env.synchronize()
    assert same(full_state(env), c.at_snapshot)
    again = c.roll()
    assert np.array_equal(bits(again), bits(c.rows)), "the roll after restore differs from the uninterrupted one"
    assert same(full_state(env), c.after)
    # control on the surface there was before: get_state / set_state brings qpos, qvel and target back, but neither the episode clocks
    # nor the episode numbers (nor the warm start) - so the same roll resets at other steps and counters() comes out different
    q, v, t = c.at_snapshot[:3]
    env.set_state(q, v, t)
    c.roll()
    sc, ep, _ = env.counters()
    assert not (np.array_equal(sc, c.after[3]) and np.array_equal(ep, c.after[4])), "set_state was expected NOT to reproduce the counters"
    # a snapshot of a restored state is the same bytes
    torch = _torch()
    snap2 = torch.zeros_like(c.snap)
    torch.cuda.synchronize()
    env.restore_device(c.snap.data_ptr())
    env.snapshot_device(snap2.data_ptr())
    env.synchronize()
    assert torch.equal(snap2, c.snap) and np.array_equal(env.save_state(), c.blob)


# ---------------------------------------------------------------------------------------------- 2. host blob
@pytest.mark.parametrize("label", ["n37-ragged", "n256-pair"])
def test_host_blob_moves_the_state_to_a_fresh_handle(case, label):
    c = case(label)
    assert c.blob.dtype == np.uint8 and c.blob.size == 64 + 232 * c.n and c.blob[:4].tobytes() == b"JBSN"
    other = make_env(label)          # freshly created: episode 0, step 0, no warm start
    try:
        other.load_state(c.blob)
        assert same(full_state(other), c.at_snapshot)
        torch = _torch()
        rows = torch.full((K, c.n, c.D + 2), float("nan"), device=c.dev)
        torch.cuda.synchronize()
        other.step_many_device(K, c.tape.data_ptr(), rows_ptr=rows.data_ptr())
        other.synchronize()
        assert np.array_equal(bits(rows), bits(c.rows))
        assert same(full_state(other), c.after)
    finally:
        other.close()


def test_restore_refusals_happen_on_the_host_before_any_launch(case):
    from jitterbug_amd import _lib
    from jitterbug_amd.vec_env import JitterbugVecEnv
    c = case("n37-ragged")
    env, n = c.env, c.n
    env.load_state(c.blob)
    before = env.save_state()
    E = _lib.JitterbugHipError
    with pytest.raises(E, match="size"):
        env.load_state(c.blob[:-232])                      # truncated by one env
    with pytest.raises(E, match="header"):
        env.load_state(c.blob[:10])
    bad = c.blob.copy(); bad[0] ^= 1
    with pytest.raises(E, match="magic"):
        env.load_state(bad)
    src = np.arange(n, dtype=np.int32)
    for j, v in ((5, n), (n - 1, -1)):
        s = src.copy(); s[j] = v
        with pytest.raises(E, match=r"src\[%d\]" % j):
            env.load_state(c.blob, src=s)
    other = JitterbugVecEnv(n, "move_from_origin", seed=7)          # another task: the target means something else
    small = JitterbugVecEnv(5, "move_to_pose", seed=7)
    try:
        with pytest.raises(E, match="task"):
            other.load_state(c.blob)
        with pytest.raises(E, match="index map"):
            small.load_state(c.blob)                                # other env count without a map
        with pytest.raises(E, match="index map"):
            small.restore_device(c.snap.data_ptr(), n_src=n)
        small.load_state(c.blob, src=[0, 1, 36, 3, 3])              # ... with one it is a gather
        q = small.get_state()[0]
        assert np.array_equal(q, c.at_snapshot[0][[0, 1, 36, 3, 3]])
    finally:
        other.close(); small.close()
    # a pending jb_step_async: every form is refused, and the pairing async -> wait is still intact afterwards
    torch = _torch()
    ret = torch.zeros(n, device=c.dev)
    torch.cuda.synchronize()
    env.load_state(c.blob)
    env.step_async(np.zeros(n, np.float32))
    try:
        for call in (lambda: env.save_state(), lambda: env.load_state(c.blob), lambda: env.snapshot_device(c.snap.data_ptr()),
                     lambda: env.restore_device(c.snap.data_ptr()), lambda: env.score_tapes_device(2, c.tape.data_ptr(), 1.0, ret.data_ptr())):
            with pytest.raises(E, match="pending"):
                call()
    finally:
        env.step_wait()
    env.load_state(c.blob)
    assert np.array_equal(env.save_state(), before)


# ---------------------------------------------------------------------------------------------- 3. fork within a handle
def test_fork_within_a_handle_every_lane_follows_its_group_leader():
    from jitterbug_amd.vec_env import JitterbugVecEnv
    torch = _torch()
    dev = torch.device("cuda", 0)
    n, pre, k = 256, 25, 12
    env = JitterbugVecEnv(n, "move_to_pose", seed=11)
    try:
        D = env.obs_dim
        g = torch.Generator(device=dev); g.manual_seed(4)
        mixed = torch.rand((pre, n), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        mixed[:, ::3] = 1.0
        group_tape = (torch.rand((k, n // 8), generator=g, device=dev, dtype=torch.float32) * 2 - 1).repeat_interleave(8, dim=1).contiguous()
        src = (8 * (torch.arange(n, device=dev) // 8)).to(torch.int32)
        snap = torch.zeros(env.snapshot_bytes, device=dev, dtype=torch.uint8)
        rows_f = torch.full((k, n, D + 2), float("nan"), device=dev); rows_u = torch.full((k, n, D + 2), float("nan"), device=dev)
        torch.cuda.synchronize()
        env.reset_device()
        env.step_many_device(pre, mixed.data_ptr())
        env.snapshot_device(snap.data_ptr())
        env.restore_device(snap.data_ptr(), n_src=n, src_ptr=src.data_ptr())
        env.step_many_device(k, group_tape.data_ptr(), rows_ptr=rows_f.data_ptr())
        env.restore_device(snap.data_ptr())                                  # un-forked: every env its own state, the same tape
        env.step_many_device(k, group_tape.data_ptr(), rows_ptr=rows_u.data_ptr())
        env.synchronize()
        f, u = bits(rows_f), bits(rows_u)
        assert np.isfinite(rows_f.cpu().numpy()).all()
        leaders = 8 * (np.arange(n) // 8)
        assert np.array_equal(f, f[:, leaders]), "a forked lane differs from its group leader"
        assert np.array_equal(f[:, ::8], u[:, ::8]), "a leader differs from the same env of the un-forked handle"
        assert not np.array_equal(f, u)                                      # (the other lanes did change state)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 4. plant -> model fan-out
def test_plant_to_model_fan_out_predicts_the_plant_exactly():
    from jitterbug_amd.vec_env import JitterbugVecEnv
    torch = _torch()
    dev = torch.device("cuda", 0)
    G, M, k = 2, 64, 10
    plant = JitterbugVecEnv(G, "move_from_origin", seed=21, envs_per_wave=4)
    model = JitterbugVecEnv(G * M, "move_from_origin", seed=21, envs_per_wave=4)
    try:
        g = torch.Generator(device=dev); g.manual_seed(6)
        warm = torch.rand((15, G), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        tapes = torch.rand((k, G * M), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        src = (torch.arange(G * M, device=dev) // M).to(torch.int32)
        snap = torch.zeros(plant.snapshot_bytes, device=dev, dtype=torch.uint8)
        ret = torch.zeros(G * M, device=dev); alive = torch.zeros(G * M, device=dev, dtype=torch.int32)
        rew_m = torch.zeros((k, G * M), device=dev); rew_p = torch.zeros((k, G), device=dev)
        torch.cuda.synchronize()
        plant.reset_device()
        plant.step_many_device(15, warm.data_ptr())
        plant.snapshot_device(snap.data_ptr())
        plant.synchronize()                                                 # (the model runs on its own stream)
        model.restore_device(snap.data_ptr(), n_src=G, src_ptr=src.data_ptr())
        model.score_tapes_device(k, tapes.data_ptr(), 1.0, ret.data_ptr(), alive.data_ptr())
        model.restore_device(snap.data_ptr(), n_src=G, src_ptr=src.data_ptr())
        model.step_many_device(k, tapes.data_ptr(), rewards_ptr=rew_m.data_ptr())
        model.synchronize()
        assert (alive.cpu().numpy() == k).all()
        best = ret.view(G, M).argmax(dim=1) + torch.arange(G, device=dev) * M
        best_tapes = tapes[:, best].contiguous()
        torch.cuda.synchronize()
        plant.step_many_device(k, best_tapes.data_ptr(), rewards_ptr=rew_p.data_ptr())
        plant.synchronize()
        assert float(rew_p.abs().sum()) > 0
        assert np.array_equal(bits(rew_p), bits(rew_m[:, best])), "the plant did not do what its model predicted for the chosen tape"
    finally:
        plant.close(); model.close()


# ---------------------------------------------------------------------------------------------- 5. scorer
def returns_fp64(rew, done, gamma32):
    """sum_k gamma^k r_k up to and including the first done step, in fp64, with its magnitude sum (for the bound) and the steps counted"""
    Kk, n = rew.shape
    first = np.where(done.any(axis=0), done.argmax(axis=0), Kk - 1)
    alive = first + 1
    counted = np.arange(Kk)[:, None] <= first[None, :]
    gk = (np.float64(gamma32) ** np.arange(Kk))[:, None]
    terms = gk * rew.astype(np.float64) * counted
    return terms.sum(axis=0), np.abs(terms).sum(axis=0), alive


@pytest.mark.parametrize("label", CASE_IDS)
def test_scored_returns_match_fp64_within_the_derived_bound(case, label):
    """|err| <= K * 2^-23 * sum_k gamma^k |r_k|: the k multiplications behind gamma^k contribute a relative error of at most k * 2^-24,
    the K fused multiply-adds at most K * 2^-24 (jb_snapshot.hpp fixes that order of operations).  gamma is the float32 value."""
    torch = _torch()
    c = case(label)
    env, n, D = c.env, c.n, c.D
    rew, done = c.rows[:, :, D], c.rows[:, :, D + 1] > 0.5
    ret = torch.zeros(n, device=c.dev); alive = torch.zeros(n, device=c.dev, dtype=torch.int32)
    torch.cuda.synchronize()
    for gamma in (1.0, 0.97):
        env.restore_device(c.snap.data_ptr())
        env.score_tapes_device(K, c.tape.data_ptr(), gamma, ret.data_ptr(), alive.data_ptr())
        env.synchronize()
        want, mag, want_alive = returns_fp64(rew, done, np.float32(gamma))
        got = ret.cpu().numpy().astype(np.float64)
        err, bound = np.abs(got - want), K * 2.0 ** -23 * mag
        print("%s gamma %.2f: max |err| %.3e, max err / bound %.3f" % (label, gamma, err.max(), (err / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(alive.cpu().numpy(), want_alive) and (want_alive == 30 - PRE).all()
        assert (err <= bound).all()
        assert same(full_state(env), c.after), "scoring leaves the post-rollout state"
    # tapes = NULL: the in-kernel heuristic policy.  The same returns as scoring, as a tape, the actions that policy is recorded to take
    obs = torch.zeros((n, D), device=c.dev); act = torch.zeros((K, n), device=c.dev)
    r1 = torch.zeros(n, device=c.dev); d1 = torch.zeros(n, device=c.dev, dtype=torch.uint8)
    ret_p = torch.zeros(n, device=c.dev); alive_p = torch.zeros(n, device=c.dev, dtype=torch.int32)
    torch.cuda.synchronize()
    env.restore_device(c.snap.data_ptr())
    env.observe_device(obs.data_ptr())
    for k in range(K):
        env.policy_device(obs.data_ptr(), act[k].data_ptr())
        env.step_device(act[k].data_ptr(), obs.data_ptr(), r1.data_ptr(), d1.data_ptr())
    env.restore_device(c.snap.data_ptr())
    env.score_tapes_device(K, None, 0.97, ret_p.data_ptr(), alive_p.data_ptr())
    env.restore_device(c.snap.data_ptr())
    env.score_tapes_device(K, act.data_ptr(), 0.97, ret.data_ptr(), alive.data_ptr())
    env.synchronize()
    assert float(act.abs().sum()) > 0
    assert np.array_equal(bits(ret_p), bits(ret)) and torch.equal(alive_p, alive)


def test_scored_returns_stop_at_each_envs_own_first_done_step():
    """The cases above end every env's episode on the same step.  Here the episode clocks are staggered - a masked reset part-way through the
    lead-in - so `alive` varies over the batch and every return must stop at its OWN env's first done step; same bound as above."""
    from jitterbug_amd.vec_env import JitterbugVecEnv
    torch = _torch()
    dev = torch.device("cuda", 0)
    n, early = 37, 8
    env = JitterbugVecEnv(n, "move_from_origin", seed=7, time_limit=0.3, envs_per_wave=2)          # (a task whose rewards are not near zero: a return that stopped late would show)
    try:
        D = env.obs_dim
        g = torch.Generator(device=dev); g.manual_seed(4)
        tape = torch.rand((PRE + K, n), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        mask = (np.arange(n) % 3 == 1).astype(np.uint8)
        snap = torch.zeros(env.snapshot_bytes, device=dev, dtype=torch.uint8)
        rows = torch.full((K, n, D + 2), float("nan"), device=dev)
        ret = torch.zeros(n, device=dev); alive = torch.zeros(n, device=dev, dtype=torch.int32)
        torch.cuda.synchronize()
        env.reset_device()
        env.step_many_device(early, tape[:early].contiguous().data_ptr())
        env.synchronize()
        env.reset(mask=mask)                                    # these envs' clocks start again, `early` steps behind the others
        env.step_many_device(PRE - early, tape[early:PRE].contiguous().data_ptr())
        env.snapshot_device(snap.data_ptr())
        env.step_many_device(K, tape[PRE:].contiguous().data_ptr(), rows_ptr=rows.data_ptr())
        env.synchronize()
        r = rows.cpu().numpy()
        rew, done = r[:, :, D], r[:, :, D + 1] > 0.5
        for gamma in (1.0, 0.97):
            env.restore_device(snap.data_ptr())
            env.score_tapes_device(K, tape[PRE:].contiguous().data_ptr(), gamma, ret.data_ptr(), alive.data_ptr())
            env.synchronize()
            want, mag, want_alive = returns_fp64(rew, done, np.float32(gamma))
            assert np.array_equal(want_alive, np.where(mask == 1, 30 - PRE + early, 30 - PRE)) and len(set(want_alive)) == 2
            assert np.array_equal(alive.cpu().numpy(), want_alive)
            err, bound = np.abs(ret.cpu().numpy().astype(np.float64) - want), K * 2.0 ** -23 * mag
            print("staggered clocks, gamma %.2f: max |err| %.3e, max err / bound %.3f" % (gamma, err.max(), (err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all()
            # ... and a return that ran on to another env's done step would differ by that env's later rewards
            late = returns_fp64(rew, np.broadcast_to(done[:, mask == 1][:, :1], done.shape), np.float32(gamma))[0]
            assert (np.abs(late - want)[mask == 0] > 10 * bound[mask == 0]).any()
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------- 6. planner plumbing
def test_mppi_planner_is_deterministic_leaves_the_plant_alone_and_applies_its_update():
    from jitterbug_amd.planning import MPPIPlanner
    from jitterbug_amd.vec_env import JitterbugVecEnv
    torch = _torch()
    dev = torch.device("cuda", 0)
    G, M, k = 2, 64, 8
    plant = JitterbugVecEnv(G, "move_from_origin", seed=3, envs_per_wave=4)
    kw = dict(n_groups=G, n_candidates=M, horizon=k, gamma=0.98, temperature=0.05, noise_sigma=0.6, seed=9, envs_per_wave=4)
    p1, p2 = MPPIPlanner("move_from_origin", **kw), MPPIPlanner("move_from_origin", **kw)
    try:
        snap = torch.zeros(plant.snapshot_bytes, device=dev, dtype=torch.uint8)
        g = torch.Generator(device=dev); g.manual_seed(12)
        warm = torch.rand((10, G), generator=g, device=dev, dtype=torch.float32) * 2 - 1
        torch.cuda.synchronize()
        plant.reset_device()
        plant.step_many_device(10, warm.data_ptr())
        plant.snapshot_device(snap.data_ptr())
        blob = plant.save_state()
        snap0 = snap.clone()
        for it in range(2):
            a1, a2 = p1.plan(snap.data_ptr()), p2.plan(blob if it else snap.data_ptr())      # (device snapshot and host blob: the same state)
            torch.cuda.synchronize()
            assert a1.shape == (G,) and torch.equal(a1, a2) and bool((a1.abs() <= 1).all())
            assert torch.equal(p1.returns, p2.returns) and torch.equal(p1.candidates, p2.candidates)
            # the update, restated in fp64 from the planner's own returns and candidate tapes
            R = p1.returns.double().view(G, M)
            e = torch.exp((R - R.max(dim=1, keepdim=True).values) / 0.05)
            w = e / e.sum(dim=1, keepdim=True)
            tape = (p1.candidates.double().view(k, G, M) * w[None]).sum(dim=2)
            assert float((a1.double() - tape[0]).abs().max()) <= 1e-6
            assert float((p1.nominal[:-1].double() - tape[1:]).abs().max()) <= 1e-6 and torch.equal(p1.nominal[-1], p1.nominal[-2])
            best, best_ret = p1.best_tape()
            assert best.shape == (k, G) and torch.equal(best_ret, p1.returns.view(G, M).max(dim=1).values)
        assert float(p1.returns.std()) > 0
        assert torch.equal(snap, snap0) and np.array_equal(plant.save_state(), blob), "plan() touched the plant"
    finally:
        plant.close(); p1.close(); p2.close()

"""The contact pass on the GPU (jb_contacts_device / jb_contacts; jb_contacts_kernel in jitterbug_amd/csrc/jb_api.hip, per-slot function
jb_contacts.hpp): every family through a snapshot stack against the oracle's contact lists under the bounds of the fp32 host build
(tests/contacts_inputs.py: three times the host's measured worst, per block and family); consistency with the forward pass; the shapes at
which the indexing can go wrong, bit for bit; the state, the counters and the solver statistics left untouched (the refusals: tests/test_gpu_pass_refusals.py).

The kernel gives a wave to four env-states (a quad of lanes each, three mirror groups): N = 1 is one quad with the rest of its wave
repeating it, N = 5 a full wave plus a ragged one, and a stack of snapshots starts a new wave at every snapshot."""
import numpy as np
import pytest

from jitterbug_amd import _lib, model
from tests import contacts_inputs as ci
from tests import forward_inputs as fi
from tests.test_gpu_forward import bits, device_forward, load, make_env, rollout_pick

pytestmark = pytest.mark.gpu

KEYS = ("contact", "ncon", "geom_frc")


def _torch():
    import torch
    return torch


def device_contacts(env, ctrl=None, mask=15, snaps=None, n_snaps=1, fill=-7.25):
    """contacts_device into fresh tensors filled with `fill` (ncon: 77); bit k of mask: output k (contact, ncon, geom_frc, unconverged) is
    present.  -> ({output: array, floats as bit patterns}, unconverged uint8)"""
    torch = _torch()
    dev = torch.device("cuda", 0)
    m = n_snaps * env.num_envs
    t = dict(contact=torch.full((m, model.NCONTACT, model.CONTACT_WIDTH), fill, device=dev, dtype=torch.float32),
             ncon=torch.full((m,), 77, device=dev, dtype=torch.int32), geom_frc=torch.full((m, model.NGEOM, 3), fill, device=dev, dtype=torch.float32))
    un = torch.full((m,), 77, device=dev, dtype=torch.uint8)
    c = None if ctrl is None else torch.as_tensor(np.ascontiguousarray(ctrl, dtype=np.float32)).to(dev)
    torch.cuda.synchronize()
    ptr = [t[k].data_ptr() if mask >> i & 1 else None for i, k in enumerate(KEYS)]
    env.contacts_device(None if c is None else c.data_ptr(), *ptr, unconverged_ptr=un.data_ptr() if mask >> 3 & 1 else None,
                        snaps_ptr=None if snaps is None else snaps.data_ptr(), n_snaps=n_snaps)
    env.synchronize()
    return dict(contact=bits(t["contact"]), ncon=t["ncon"].cpu().numpy(), geom_frc=bits(t["geom_frc"])), un.cpu().numpy()


def stack_of(env, name, chunks):
    """the states chunks[k] of family `name` as snapshot k of a device stack (env holds len(chunks[k]) envs) -> (snaps, ctrl [K * N])"""
    torch = _torch()
    snaps = torch.zeros((len(chunks), env.snapshot_bytes), device=torch.device("cuda", 0), dtype=torch.uint8)
    torch.cuda.synchronize()
    ctrl = []
    for k, idx in enumerate(chunks):
        ctrl.append(load(env, name, idx))
        env.snapshot_device(snaps[k].data_ptr())
    env.synchronize()
    return snaps, np.concatenate(ctrl)


# ------------------------------------------------------------------------------------------------ (a) parity with the oracle
PARITY = [("rollout", "ordinary", 16), ("rollout", "lean", 16), ("poses-moving", "ordinary", 16), ("models-moving", "pair", 16), ("mass-touching", "pair", 16), ("thread-touching", "pair", 4)]


@pytest.mark.parametrize("name,variant,n", PARITY, ids=["%s-%s" % p[:2] for p in PARITY])
def test_a_family_through_a_snapshot_stack_against_the_oracle(name, variant, n):
    f = fi.family(name)
    idx = rollout_pick() if name == "rollout" else np.arange(f.n)
    assert len(idx) % n == 0
    chunks = idx.reshape(-1, n)
    env = make_env(n, variant=variant, envs_per_wave=4) if variant == "lean" else make_env(n)
    snaps, ctrl = stack_of(env, name, chunks)
    assert env.kernel_variant == variant
    if name in ("models-moving", "mass-touching", "thread-touching"):
        # one table per env: every snapshot must meet the tables its states were drawn with (state j takes table j % m, and n % m == 0)
        assert f.n_models > 1 and n % f.n_models == 0
    out, un = device_contacts(env, ctrl, snaps=snaps, n_snaps=len(chunks))
    ref = fi.reference(name)
    print("%s on a %s handle: %d env-states in %d snapshots, %d excluded, unconverged %d, at most %d contacts" % (
        name, variant, len(idx), len(chunks), (~ref.strict[idx]).sum(), un.sum(), out["ncon"].max()))
    assert not un.any()
    contact, gf = out["contact"].view(np.float32), out["geom_frc"].view(np.float32)
    ci.check(name, contact, out["ncon"], ci.FP32_BOUND[name], "GPU %d x %d" % (len(chunks), n), idx=idx)
    # consistency with the forward pass on the same handle, states and actions: the floor rows' total against qfrc[0:3], unconverged identical
    torch = _torch()
    dev = torch.device("cuda", 0)
    qfrc = torch.zeros((len(idx), model.NV), device=dev, dtype=torch.float32)
    unf = torch.full((len(idx),), 77, device=dev, dtype=torch.uint8)
    c = torch.as_tensor(ctrl).to(dev)
    torch.cuda.synchronize()
    env.forward_device(c.data_ptr(), qfrc_ptr=qfrc.data_ptr(), unconverged_ptr=unf.data_ptr(), snaps_ptr=snaps.data_ptr(), n_snaps=len(chunks))
    env.synchronize()
    assert np.array_equal(unf.cpu().numpy(), un)
    s = ci.sums(name, contact, gf, qfrc.cpu().numpy(), idx=idx)
    mom = s["moment"][np.isfinite(s["moment"])]
    print("%s sums on the GPU over all env-states: geom_frc %.2e, force against forward's qfrc %.2e, moment %.2e (bounds %.2e, %.2e)" % (
        name, s["geom_frc"].max(), s["force"].max(), mom.max() if mom.size else 0.0, fi.FP32_BOUND[("qfrc", "force")], fi.FP32_BOUND[("qfrc", "moment")]))
    assert s["geom_frc"].max() <= fi.FP32_BOUND[("qfrc", "force")] and s["force"].max() <= fi.FP32_BOUND[("qfrc", "force")]
    assert (mom <= fi.FP32_BOUND[("qfrc", "moment")]).all()
    env.close()


# ------------------------------------------------------------------------------------------------ (b) shapes, bit for bit
@pytest.mark.parametrize("name,n", [("poses-moving", 1), ("poses-moving", 5), ("models-moving", 5)])
def test_stack_single_calls_batch_mates_absent_outputs_and_poisoned_lds(name, n):
    """The states: two sets of n on which the forward pass - the same substep, unchanged by this pass - gives env j of a batch the bits it
    gives the state alone (poses-moving 25 .. 34 with 4 - 47 contacts; models-moving 10 .. 14, tests/test_gpu_forward.py's own, and
    34 .. 38 on the same tables, 13 - 42 contacts).  That is a condition on the inputs: where a wave sweeps its leg slots in spread mode
    and the single env does not, the substep's own sums round differently for some states ("Contacts") and nothing built on it
    can be bit-equal there; test_without_spread_sweeps_an_env_never_depends_on_its_wave_mates holds such states."""
    pair = fi.family(name).pair
    env = make_env(n, flags=_lib.FLAG_PAIR if pair and n == 1 else 0)
    first = 25 if name == "poses-moving" else 10
    chunks = [first + np.arange(n), first + n + np.arange(n)]
    if pair:          # one table per env: snapshot k's states must sit on the tables of snapshot 0's (state j takes table j % 8)
        chunks[1] = chunks[0] + 24
    snaps, ctrl = stack_of(env, name, chunks)
    stack, un = device_contacts(env, ctrl, snaps=snaps, n_snaps=2)
    assert stack["ncon"].max() >= 4 and not un.any()
    ci.check(name, stack["contact"].view(np.float32), stack["ncon"], ci.FP32_BOUND[name], "GPU stack 2 x %d" % n, idx=np.concatenate(chunks))
    # a stack equals single calls, on a snapshot and on the live state
    for k in range(2):
        one, _ = device_contacts(env, ctrl[n * k:n * k + n], snaps=snaps[k], n_snaps=1)
        load(env, name, chunks[k])
        live, _ = device_contacts(env, ctrl[n * k:n * k + n])
        for key in KEYS:
            assert np.array_equal(stack[key][n * k:n * k + n], one[key]), (k, key)
            assert np.array_equal(one[key], live[key]), (k, key)
    # env j of a batch equals the same state alone
    if n > 1:
        solo = make_env(1, flags=_lib.FLAG_PAIR if pair else 0)
        for k in range(2):
            for j in range(n):
                c1 = load(solo, name, chunks[k][j:j + 1])
                alone, un1 = device_contacts(solo, c1)
                for key in KEYS:
                    differ = np.argwhere(np.atleast_1d(stack[key][n * k + j] != alone[key][0]))
                    assert not len(differ), (k, j, key, "first differing entries", differ[:6].tolist())
                assert un1[0] == 0
        solo.close()
    # absent outputs change nothing, and cost no stores
    sentinel = bits(np.float32(-7.25))
    for mask in (1, 2, 4, 8, 3, 5, 6, 12):
        got, un2 = device_contacts(env, ctrl, mask=mask, snaps=snaps, n_snaps=2)
        for i, key in enumerate(KEYS):
            if mask >> i & 1:
                assert np.array_equal(got[key], stack[key]), (mask, key)
            else:
                assert (got[key] == (77 if key == "ncon" else sentinel)).all(), (mask, key)
        assert np.array_equal(un2, un) if mask >> 3 & 1 else (un2 == 77).all()
    # no action tape: action 0
    zero, _ = device_contacts(env, None, snaps=snaps, n_snaps=2)
    same, _ = device_contacts(env, np.zeros(2 * n, dtype=np.float32), snaps=snaps, n_snaps=2)
    for key in KEYS:
        assert np.array_equal(zero[key], same[key])
    env.debug_poison_lds()
    again, un3 = device_contacts(env, ctrl, snaps=snaps, n_snaps=2)
    for key in KEYS:
        assert np.array_equal(again[key], stack[key]), key
    assert np.array_equal(un3, un)
    env.close()


@pytest.mark.parametrize("name,first", [("poses-moving", 20), ("models-moving", 18)])
def test_without_spread_sweeps_an_env_never_depends_on_its_wave_mates(name, first):
    """The public guarantee, on states where the ordinary handle's substep is NOT independent (poses-moving 20 and 22, models-moving 20:
    there the forward pass's qacc differs between the batch and the single env, and the forces follow it): on handles created with
    JB_FLAG_NO_SPREAD env j of a batch equals the same state alone, bit for bit, for the contact pass and for forward's qacc."""
    pair, n = fi.family(name).pair, 5
    idx = first + np.arange(n)
    env, solo = make_env(n, flags=_lib.FLAG_NO_SPREAD), make_env(1, flags=_lib.FLAG_NO_SPREAD | (_lib.FLAG_PAIR if pair else 0))
    ctrl = load(env, name, idx)
    whole, un = device_contacts(env, ctrl)
    fwhole, _ = device_forward(env, ctrl)
    assert whole["ncon"].max() >= 19 and not un.any()
    for j in range(n):
        c1 = load(solo, name, idx[j:j + 1])
        alone, _ = device_contacts(solo, c1)
        assert np.array_equal(fwhole["qacc"][j], device_forward(solo, c1)[0]["qacc"][0]), j
        for key in KEYS:
            assert np.array_equal(whole[key][j], alone[key][0]), (j, key)
    ci.check(name, whole["contact"].view(np.float32), whole["ncon"], ci.FP32_BOUND[name], "GPU without spread sweeps", idx=idx)
    env.close(); solo.close()


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
    out, _ = device_contacts(env, tape[0].cpu().numpy())
    host = env.contacts(tape[0].cpu().numpy())
    for key in KEYS:
        assert np.array_equal(bits(host[key]) if key != "ncon" else host[key], out[key]), key
    env.snapshot_device(after.data_ptr())
    env.synchronize()
    assert torch.equal(before, after)
    for a, b in zip(counters, env.counters()):
        assert np.array_equal(a, b)
    assert env.solver_stats() == stats
    env.close()

"""The line-searched second contact solve (jb_sim.hpp: the cold block of substep_impl, newton_phase<V, PAIR, LS = true>) on the GPU, against
the oracle.  With the default max_newton = 12 the block runs for a few wave-substeps in ten million; max_newton = 1 gives the plain active-set
iteration ONE check, so every substep whose set does not repeat at once is solved again - 11-13 % of the env-substeps on the inputs below
(the kernel source on the host, fp32, four lane groups: 902 of 6800 tipped, 1081 of 6800 walking; none ended at NEWTON_LS_CAP, no entry left
strict_within).  The two solves minimise the same strictly convex cost, so the strict parity protocol (tests/parity_protocol.py) holds
unchanged.  What only the GPU has: group_sum_u of the capped bits across lane groups, the ls_mailbox hand-over (SC_RED; LEAN: the head of the
kept factorisation), contact_sweep mode 3 between wave_syncs, quad_sum's DPP exchanges, LEAN's failure counter in LDS and its spilled
registers, the PAIR instantiations, 1 / 2 / 8 envs per wave, the copy of the block inside the fused jb_step_many_device kernel.

  a  every launch row x (walking, tipped), 17 envs (one ragged wave at every envs-per-wave setting, 17 waves at 1), 8 compared steps
  b  ... and `resolved` (solver_stats()) says the block really ran
  c  max_newton = 3 on the four rows at 4 envs per wave: rank-one passes on the kept factorisation BEFORE the cap (LEAN: the mailbox lies on it)
  d  live geom - geom contacts inside the second solve (PAIR, LEAN + PAIR; robots whose thread rubs a front leg)
  e  an env's bits are its own: a wave-mate that did not cap keeps the first solve's bits while its wave goes through the block

The zero caps (near_cap = 0, deep_steps == 0) are conditions on the INPUTS, checked with OracleEnv.conditioning() on the CPU over the 8
compared steps (teacher-forced: the classes are the oracle's trajectory's); MARGIN_TOL is 1.1e-8 m:
    nominal, env seed 3, walking                       smallest switch margin 1.19e-7 m, none deep
    nominal, env seed 2, tipped                        1.57e-7 m, 3 of 17 tipped, none deep
    augmented_params(17, seed=4), env seed 3, walking  1.26e-7 m, none deep
    augmented_params(17, seed=4), env seed 2, tipped   2.50e-7 m, 6 of 17 tipped, none deep
    thread-touching models cycled with the nominal one, env seed 0, tipped (d)   2.46e-7 m, 15 of 17 tipped, none deep, a geom - geom contact in all 8 steps
augmented seed 4 is the first of a scan of seeds 0-20 with at least 5 x MARGIN_TOL in both regimes and no deep env-step (seed 3, which
test_every_launch_row_against_the_oracle uses at 9 envs, has 2.0e-8 / 1.8e-8 m at 17).
W = 1: the share the suite already allows (4 of ~1.1 M entries walking, 6 of 1.46 M tipped) scaled to these runs rounds to one entry.
`resolved >= 50` is a condition too: the host fp32 build re-solved 900-1080 env-substeps, and a wave of 8 envs cannot count fewer than an
eighth of its envs' re-solves.

measured (MI355X, profiles/r10_line_search_parity.txt): well_bad 0 in all 30 parity cases, worst_well 2.0e-7 - 2.2e-6 (the largest: lean_pair, tipped),
resolved 572 - 1186 wave-substeps per case with max_newton = 1 (1081 walking / 902 tipped at one env per wave: the host build's counts), 73 - 92 with
max_newton = 3; e: 83 021 - 104 219 re-solved wave-substeps per 250-step run with max_newton = 1, 1905 - 2120 with 3, every comparison
bit-identical, failure counter 0 throughout."""
import numpy as np
import pytest

from jitterbug_amd import model
from oracle import oracle as O
from tests.parity_inputs import LAUNCH_ROWS, thread_touching_models
from tests.parity_protocol import assert_protocol, protocol_message, teacher_forced

pytestmark = pytest.mark.gpu

N_ENVS, STEPS, W = 17, 8, 1
REGIMES = {"walking": dict(seed=3), "tipped": dict(seed=2, flat_out=True, skip=250)}
AUGMENTED_SEED = 4


def _row_inputs(variant):
    """(flags, params) of a launch row: `pair` is the nominal model with JB_FLAG_PAIR, `lean_pair` needs one model per env"""
    from jitterbug_amd import _lib, augmented_jitterbug as aj
    flags = {"ordinary": 0, "pair": _lib.FLAG_PAIR, "lean": _lib.FLAG_LEAN, "lean_pair": _lib.FLAG_LEAN}[variant]
    return flags, (aj.augmented_params(N_ENVS, seed=AUGMENTED_SEED) if variant == "lean_pair" else None)


def _hold(r, what, variant, resolved_min):
    print("line-search parity | %s | well_bad %d worst_well %.3e resolved %s | strict_bad %d ill_steps %d deep_steps %d cap %g tipped %.2f"
          % (what, r["well_bad"], r["worst_well"], r["resolved"], r["strict_bad"], r["ill_steps"], r["deep_steps"], r["cap"], r["tipped"]))
    assert r["kernel_variant"] == variant, r
    assert_protocol(r, well_bad=W, near_cap=0)
    assert r["deep_steps"] == 0, protocol_message(r)
    assert r["resolved"] >= resolved_min, protocol_message(r)


@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("variant,epw", LAUNCH_ROWS, ids=["%s-%d" % r for r in LAUNCH_ROWS])
def test_every_launch_row_with_the_second_solve_forced(variant, epw, regime):
    from jitterbug_amd.vec_env import JitterbugVecEnv
    flags, params = _row_inputs(variant)
    g = JitterbugVecEnv(N_ENVS, "move_to_pose", seed=3, params=params, flags=flags, envs_per_wave=epw, max_newton=1)
    assert g.kernel_variant == variant and g.envs_per_wave == epw
    g.close()
    r = teacher_forced("move_to_pose", N_ENVS, STEPS, params=params, flags=flags, envs_per_wave=epw, max_newton=1, **REGIMES[regime])
    _hold(r, "a %s-%d %s" % (variant, epw, regime), variant, 50)
    if regime == "tipped":
        assert r["tipped"] > 0, protocol_message(r)


@pytest.mark.parametrize("variant", ["ordinary", "pair", "lean", "lean_pair"])
def test_rank_one_passes_before_the_cap(variant):
    """max_newton = 3: the hot loop keeps a factorisation and makes rank-one passes on it before it gives up - in LEAN the second solve's
    mailbox then lies over a factorisation that was in use."""
    flags, params = _row_inputs(variant)
    r = teacher_forced("move_to_pose", N_ENVS, STEPS, params=params, flags=flags, envs_per_wave=4, max_newton=3, **REGIMES["tipped"])
    _hold(r, "c %s-4 tipped max_newton=3" % variant, variant, 1)
    assert r["tipped"] > 0, protocol_message(r)


@pytest.mark.parametrize("variant", ["pair", "lean_pair"])
def test_geom_geom_contacts_inside_the_second_solve(variant):
    """One model per env - robots whose thread rubs a front leg (tests/test_thread_contact.py) cycled with the nominal one, as in
    test_all_geoms_contact_parity -, motor flat out: nearly every robot lies on the floor with its thread on a leg, the pair's rows are live
    in the second solve's sweeps."""
    from jitterbug_amd import _lib
    models = [m[0] for m in thread_touching_models(6, seed=11)] + [model.default_params()]
    P = np.stack([models[i % len(models)] for i in range(N_ENVS)])
    pair_steps = set()

    def probe(t, q, v, a):
        for i in range(N_ENVS):
            d = O.forward_debug(P[i], q[i], v[i], a[i])
            if (d["con_geom"][:d["ncon"]] >= model.NGEOM).any():
                pair_steps.add(t)
                return
    r = teacher_forced("move_to_pose", N_ENVS, STEPS, seed=0, flat_out=True, skip=250, params=P, flags=_lib.FLAG_PAIR if variant == "pair" else _lib.FLAG_LEAN,
                       envs_per_wave=4, max_newton=1, probe=probe)
    _hold(r, "d %s-4 thread on a leg, tipped" % variant, variant, 50)
    assert r["tipped"] > 0 and len(pair_steps) >= 1, (sorted(pair_steps), protocol_message(r))


# ---- e: an env's bits are its own (the shape of tests/test_fused_row_build_gpu.py, with the second solve forced)
N, FLAT_STEPS = 64, 250
KERNELS = {"ordinary": 0, "lean": 2}          # JB_FLAG_LEAN


def _tipped(obs):
    qt = obs[:, 3:7]                                  # observation entries 3-6 are the root quaternion
    return int(((1 - 2 * (qt[:, 1] ** 2 + qt[:, 2] ** 2)) < 0.5).sum())


def _flat_out(kernel, max_newton, epw, poison=False):
    from jitterbug_amd.vec_env import JitterbugVecEnv
    env = JitterbugVecEnv(N, "move_from_origin", seed=5, envs_per_wave=epw, flags=KERNELS[kernel], max_newton=max_newton)
    try:
        assert env.envs_per_wave == epw and env.kernel_variant == kernel
        env.reset()
        a = np.ones(N, dtype=np.float32)
        obs = []
        for t in range(FLAT_STEPS):
            if poison and t % 3 == 0:
                env.debug_poison_lds()
            ob = env.step(a)[0]
            if t % 50 == 49:
                obs.append(ob.copy())
        obs = np.stack(obs)
        _, _, cap = env.counters()
        resolved = env.solver_stats()
        print("line-search bits | %s-%d max_newton=%d%s | resolved %d tipped %d cap %g" % (kernel, epw, max_newton, " poisoned" if poison else "", resolved, _tipped(obs[-1]), cap.sum()))
        assert np.isfinite(obs).all() and _tipped(obs[-1]) >= 2 and cap.sum() == 0 and resolved > 0
        return obs
    finally:
        env.close()


# max_newton = 1 AND 3.  With one check an env that did NOT cap has solved one full pass from the warm start, and the second solve's first
# pass is that very pass (full step, no rank-one pass anywhere): it reproduces the first solve's bits, so a per-env select that let a
# wave-mate's second solve through would change nothing (measured: a library whose select was made wave-wide passed every max_newton = 1
# case).  With three checks an env may settle on its second or third check after rank-one passes, which the second solve does not make - its
# two solves then differ in rounding, and whose accelerations it takes shows in the bits.
BITS_RUNS = [(k, mn) for mn in (1, 3) for k in KERNELS]
BITS_IDS = ["%s-max_newton%d" % r for r in BITS_RUNS]


@pytest.fixture(scope="module", params=BITS_RUNS, ids=BITS_IDS)
def reference_run(request):
    """4 envs per wave, no poison: computed once per kernel and cap, compared against by every case below"""
    kernel, max_newton = request.param
    obs = _flat_out(kernel, max_newton, 4)
    obs.setflags(write=False)
    return kernel, max_newton, obs


@pytest.mark.parametrize("epw", [1, 2])
def test_bits_do_not_depend_on_capped_wave_mates(reference_run, epw):
    """With one env per wave an env never has a capped wave-mate; with four, an env that did not cap must keep the first solve's bits while
    its wave goes through the cold block: a leak in the per-env select shows here (at max_newton = 3: see BITS_RUNS)."""
    kernel, max_newton, ref = reference_run
    obs = _flat_out(kernel, max_newton, epw)
    assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32))


def test_poisoned_scratch_changes_no_bit_of_the_second_solve(reference_run):
    kernel, max_newton, ref = reference_run
    obs = _flat_out(kernel, max_newton, 4, poison=True)
    assert np.array_equal(obs.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("kernel,max_newton", BITS_RUNS, ids=BITS_IDS)
def test_the_fused_launch_s_second_solve_equals_single_steps(kernel, max_newton):
    import torch
    from jitterbug_amd.vec_env import JitterbugVecEnv
    dev = torch.device("cuda", 0)
    kw = dict(seed=5, envs_per_wave=4, flags=KERNELS[kernel], max_newton=max_newton)
    a = JitterbugVecEnv(N, "move_from_origin", **kw)
    b = JitterbugVecEnv(N, "move_from_origin", **kw)
    try:
        assert a.kernel_variant == kernel and b.kernel_variant == kernel
        D = a.obs_dim
        tape = torch.ones((FLAT_STEPS, N), device=dev, dtype=torch.float32)
        a.reset_device(); b.reset_device()
        rows_a = torch.full((FLAT_STEPS, N, D + 2), float("nan"), device=dev)
        rows_b = torch.full((FLAT_STEPS, N, D + 2), float("nan"), device=dev)
        for k in range(FLAT_STEPS):
            a.step_rows_device(tape[k].data_ptr(), rows_a[k].data_ptr())
        b.step_many_device(FLAT_STEPS, tape.data_ptr(), rows_ptr=rows_b.data_ptr())
        a.synchronize(); b.synchronize()
        ra, rb = rows_a.cpu().numpy(), rows_b.cpu().numpy()
        res = (a.solver_stats(), b.solver_stats())
        print("line-search bits | %s-4 max_newton=%d fused | resolved single %d fused %d tipped %d" % (kernel, max_newton, res[0], res[1], _tipped(rb[-1])))
        for env, rows in ((a, ra), (b, rb)):
            assert np.isfinite(rows).all() and _tipped(rows[-1]) >= 2 and env.counters()[2].sum() == 0
        assert res[0] > 0 and res[1] == res[0]          # the same waves re-solve the same substeps
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
        for x, y in zip(a.get_state(), b.get_state()):
            assert np.array_equal(x, y)
    finally:
        a.close(); b.close()

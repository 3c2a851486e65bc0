"""The strict parity protocol: how a run of the HIP path (or of the kernel source on the host) is held against the CPU fp64 oracle on identical
inputs - tolerance lines, classes of env-steps and their constants, the tally and its assertions, the drivers that feed it.  Shared by the tests
and the record runs under tools/; not a conftest, not a test file: plain helpers, exercised on the CPU by tests/test_parity_protocol_cpu.py.
Importing it loads numpy and the oracle alone (a tool can read MARGIN_TOL without pytest, torch or the GPU library): jitterbug_amd.model and
tests.task_reference are imported where they are used, since any jitterbug_amd submodule runs the package's __init__, which imports vec_env.

Tolerance (north_star: fp64 -> fp32, 1e-4 relative): an observation / reward entry PASSES when |gpu - oracle| <= 1e-4 * |oracle| + 1e-6
(within), and is inside the STRICT line when |gpu - oracle| <= 1e-4 * |oracle| + 1e-5 (strict_within: fp32 cannot hold 1e-6 absolute on an
entry that is a difference of O(1) terms: eps x 8 roundings).
Teacher-forced comparison: every control step the oracle's (qpos, qvel, target) is copied into the GPU env
(jb_set_state keeps the fp64 height and quaternion as hi + lo fp32 words), both advance one control step (50 substeps) with the
same action.  What is asserted, and why it is conditioned on the oracle's contact-switch margin, is explained above MARGIN_TOL below."""
import numpy as np

from oracle import oracle as O


def within(a, b):          # the two lines entry by entry, b the reference: the only statement of their literals
    return np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-6


def strict_within(a, b):
    return np.abs(a - b) <= 1e-4 * np.abs(b) + 1e-5


# Conditioning of an env-step.  Contact activation (dist < 0, MuJoCo margin 0) is the model's one discontinuity: a candidate point
# that crosses the floor plane within the POSITION ERROR of an fp32 run at a substep boundary switches on one substep earlier or
# later than in fp64, and the two runs then differ by one substep's contact impulse (~1e-3 in the velocities) - in ANY fp32
# implementation, MuJoCo's own included.  The oracle reports how close each env-step came to that (jbo_stats.margin_min: the
# smallest |distance| of any contact candidate at any of the 50 substep boundaries).  tools/flip_study.py (the kernel source on the
# host in fp32 vs the oracle) shows every out-of-tolerance env-step has margin < 1e-8 m (10 nm; fp32 resolves the 35 mm body
# height to 3.7 nm), and none above (on the GPU, whose compiler fuses multiply-adds its own way: 10.5 nm over 3.84 M env-steps); tools/oracle_fp32_study.py shows the same for the oracle's own algorithm compiled in fp32.  So the protocol asserts the north-star tolerance on EVERY entry of every env-step whose
# margin is at least MARGIN_TOL, and separately bounds how many env-steps fall below it and the overall fraction.
#
# ONE constant for every kernel variant and every model: MARGIN_TOL is 3 ulp of the 35 mm body height in fp32 (one ulp of a number in
# [2^-5, 2^-4) m is 2^-28 m = 3.73 nm; 3 x 3.73 nm = 11.2 nm) - the position error an fp32 run carries, not a fitted figure.
#
# Three classes of env-steps (OracleEnv.conditioning(): the switch margin is margins() WITHOUT the zeros a deep pair overlap forces):
#   well         switch margin >= MARGIN_TOL, not deep                the north-star tolerance on every entry
#   deep         switch margin >= MARGIN_TOL, deep                    a mass - leg or thread - leg pair overlaps by more than the leg's radius in some
#                                                                     substep (the leg's axis inside the mass / the thread).  No discontinuity is involved:
#                                                                     the contact is simulated, and held to the same strict line as the well class
#   near-switch  switch margin < MARGIN_TOL (deep or not)             excluded from the tolerance, bounded by ILL_ERROR_CAP, cascade-checked, share capped
# The nominal model never brings the mass or the thread near a leg: deep is never set there (asserted by the nominal tests' callers through
# `deep_steps == 0`), so for it the classes are what they were when the protocol had two.
MARGIN_TOL = 1.1e-8     # metres.  Round 6: tools/parity_sweep.py 256 3 on the GPU (3.84 M env-steps, profiles/r06_parity_sweep.txt) - the LARGEST margin at which an env-step left the strict tolerance is 10.5 nm; tools/flip_study.py (the packed-fp32 source on the host, 6400 env-steps): every one in [1, 10) nm, none of the 24 in [10, 30) nm


# What the excluded env-steps may differ by: a contact that switches on one substep earlier or later than in fp64 leaves the step with one
# substep's contact impulse more or less - for this robot (17.5 g, contact forces up to a few times its weight within 0.2 ms, a motor that
# spins at 150 rad/s) at most a few 1e-2 in a normalised observation entry (measured worst: 2.5e-2, a tipped robot).
ILL_ERROR_CAP = 5e-2

# The deep class has a part of its own.  The mass - leg narrow phase is a FIXED-COUNT iteration (jb_sim.hpp pair_narrow = jb_oracle.c
# pair_geometric: what the counts reach is the contact's definition).  On shallow contacts it reaches the root to round-off; with the leg's
# axis deep inside the flat mass ellipsoid the multiplier runs into its clamp (-0.95 min s^2) and the counts stop short of the root - the
# oracle reports the residual they leave (conditioning()["narrow_resid"]: 3.6e-9 at most on env-steps that are not deep, 0.8-1.0 where the
# clamp holds).  Such a contact is a function of every rounding on the way: the same source in fp64 equals the oracle (1.7e-7), in fp32 it
# is off by up to 1.5e-3 in an observation entry on 6 of 141 such env-steps (tools/flip_study.py, profiles/r07_flip_study_pair.txt), and
# the oracle's own step from the same state rounded to fp32 already differs by up to 2.8e-5 there.
# So: deep env-steps whose narrow phase CONVERGED (residual < NARROW_RESID_TOL) are held to the strict line like the well class; the
# UNCONVERGED ones (`clamped_*` keys) are bounded by DEEP_ERROR_CAP - never unbounded.
NARROW_RESID_TOL = 1e-6      # 8 ulp of 1 in fp32: the root as well as fp32 can state it
# Measured against the oracle on the GPU, profiles/r07_parity_sweep.txt: the largest error on an unconverged deep env-step over the sweep is
# 2.4e-3 (lines "augmented_params(256, seed=5) x 1000, seed 6", PAIR and LEAN + PAIR alike: 434 such env-steps, 47 entries outside the strict
# tolerance; every other line of the sweep - up to 47 such env-steps each - has none outside it, worst 2.1e-6).  Twice that: seeds sample the tail.
DEEP_ERROR_CAP = 5e-3

# Share of near-switch env-steps a per-env-model run may have.  A CAP, not a measurement: the oracle alone gives 0.07-0.20 % on the inputs of
# these tests (tests/test_pair_contact.py::test_oracle_reports_deep_overlap_and_switch_margin_separately prints them), the binomial spread
# at 9600-19 200 env-steps is +- 0.03-0.04 %.  Runs shorter than 9600 env-steps add three binomial spreads of their own size (near_switch_cap).
NEAR_SWITCH_CAP = 0.003


def near_switch_cap(env_steps):
    if env_steps >= 9600:
        return NEAR_SWITCH_CAP
    return NEAR_SWITCH_CAP + 3 * np.sqrt(0.0015 * (1 - 0.0015) / env_steps)          # 0.15 %: the nominal near-switch share


def classify(o, contacts=True):
    """(well, deep, near) masks of the oracle env's last control step - the three classes above"""
    if not contacts:
        return np.ones(o.n, bool), np.zeros(o.n, bool), np.zeros(o.n, bool)
    c = o.conditioning()
    near = c["switch"] < MARGIN_TOL
    return ~near & ~c["deep"], ~near & c["deep"], near


def unconverged(o, contacts=True):
    """env-steps of the oracle env's last control step in which the mass - leg narrow phase's fixed counts stopped short of the root"""
    return o.conditioning()["narrow_resid"] >= NARROW_RESID_TOL if contacts else np.zeros(o.n, bool)


def protocol_message(r):
    """what an assertion of the protocol shows when it fails: the whole result, the figure MARGIN_TOL has to cover first"""
    return "largest switch margin of an env-step outside the strict tolerance (flip_margin_max) %.2f nm, MARGIN_TOL %.1f nm; %r" % (r["flip_margin_max"] * 1e9, MARGIN_TOL * 1e9, r)


def assert_protocol(r, well_bad, worst_well=None, near_cap=None, deep_share_min=None):
    """The strict parity protocol on one result of a ParityTally - every per-env-model test asserts ALL of it: on the well class the
    north-star line counted (`well_bad` entries at most outside within(), none by 1e-2; where the caller bounds it, none by
    `worst_well`) and exact (strict_bad == 0: strict_within() on every entry); on the deep class the same exact line
    (no entry of a deep env-step with a converged narrow phase outside it; the unconverged ones below DEEP_ERROR_CAP) and the same
    `worst_well`; near-switch env-steps bounded in error, never cascading, capped in number
    (NEAR_SWITCH_CAP unless the caller's own bound is tighter); every contact solve converged."""
    msg = protocol_message(r)
    assert r["well_bad"] <= well_bad and r["well_big"] == 0, msg
    assert r["strict_bad"] == 0, msg
    assert r["deep_strict_bad"] - r["clamped_strict_bad"] == 0, msg          # deep, narrow phase converged: the strict line
    assert r["worst_clamped"] < DEEP_ERROR_CAP, msg                          # deep, narrow phase unconverged: bounded
    if worst_well is not None:
        assert r["worst_well"] < worst_well and r["worst_deep_converged"] < worst_well, msg
    assert r["worst_ill"] < ILL_ERROR_CAP and r["cascade_bad"] == 0, msg
    assert r["ill_frac"] <= (near_switch_cap(r["env_steps"]) if near_cap is None else near_cap), msg
    assert r["cap"] == 0, msg
    assert_rewards(r)
    if deep_share_min is not None:
        assert r["deep_steps"] >= deep_share_min * r["env_steps"], msg          # the class really is exercised


# Rewards.  The reward is a CONTINUOUS function of the state - no contact switch is involved -, so it is held on EVERY env-step, the near-switch
# class included: against oracle.reward of the GPU's OWN post-step state, inside the derived bound of tests/task_reference.py (its rounding
# counts are stated there); `reward_bad` counts the env-steps outside it and must be zero.  Next to it the reward the kernel returned against the
# ORACLE'S step (`worst_reward_held`, over the env-steps that are not near a switch: it carries the step's own fp32 error through the reward's
# slope) is capped by a measurement against the oracle: the worst over the full tools/parity_sweep.py run, all four kernels
# (profiles/r09_parity_sweep.txt: REWARD_HELD_MEASURED), times two - seeds sample the tail, the convention of DEEP_ERROR_CAP.
REWARD_HELD_MEASURED = 7.759e-6      # the tipped regime of the ordinary kernel; every other line of the record is below 2.5e-6.  reward_bad is 0 on all 51 lines
REWARD_HELD_CAP = 2 * REWARD_HELD_MEASURED


def assert_rewards(r):
    msg = protocol_message(r)
    assert r["reward_bad"] == 0, msg
    assert r["worst_reward_held"] <= REWARD_HELD_CAP, msg


class ParityTally:
    """The protocol's counters over a run of env-steps, whoever drives the envs (teacher_forced and free_running below).
    add() takes one compared control step - the oracle env just stepped, the GPU's and the oracle's
    observations and rewards, and the GPU's post-step state (q, v, target) of the compared envs - and returns the env-steps of the near-switch
    class that left the tolerance (those the cascade check follows; sel: a bool mask of the envs compared in this step, where not all are); cascade() takes the GPU's NEXT step of such envs from its own state
    against the oracle's from that same state; result() the figures.  task, P: what the rewards are the rewards of (P [NPARAM] or [n, NPARAM])."""

    def __init__(self, n, task, P, contacts=True):
        self.n, self.contacts, self.steps, self.env_steps = n, contacts, 0, 0
        self.task, self.P = task, np.asarray(P, dtype=np.float64)
        self.reward_bad, self.worst_reward_own, self.worst_reward_ratio = 0, 0.0, 0.0
        self.tot = self.ok = self.okr = self.big = 0
        self.well_tot = self.well_ok = self.well_big = self.ill_steps = self.ill_bad_steps = self.strict_bad = self.cascade_checked = self.cascade_bad = 0
        self.deep_steps = self.deep_bad = self.deep_strict_bad = self.far_off = 0
        self.clamped_steps = self.clamped_strict_bad = self.unconverged_well = 0
        self.worst_clamped = self.worst_deep_converged = 0.0
        self.worst = self.worst_well = self.worst_ill = self.worst_deep = self.flip_margin_max = self.worst_reward_held = 0.0

    def add(self, o, og, oo, rg, ro, gstate, sel=None):
        if sel is not None:          # only the envs of this bool mask are compared (a run across episode boundaries leaves out the env-steps that end in a reset)
            return self._add_selected(o, og, oo, rg, ro, gstate, np.asarray(sel, dtype=bool))
        return self._add(classify(o, self.contacts), unconverged(o, self.contacts), o.conditioning()["switch"] if self.contacts else None, self.P, og, oo, rg, ro, gstate)

    def _add_selected(self, o, og, oo, rg, ro, gstate, sel):
        out = np.zeros(self.n, bool)
        if sel.any():
            out[sel] = self._add(tuple(c[sel] for c in classify(o, self.contacts)), unconverged(o, self.contacts)[sel], o.conditioning()["switch"][sel] if self.contacts else None,
                                 self.P[sel] if self.P.ndim == 2 else self.P, og[sel], oo[sel], rg[sel], ro[sel], tuple(x[sel] for x in gstate))
        return out

    def _add(self, classes, unconv, switch, P, og, oo, rg, ro, gstate):
        from tests import task_reference as tr
        well, deep, near = classes
        qg, vg, tg = gstate
        Pi = (lambda i: P[i]) if P.ndim == 2 else (lambda i: P)
        own = np.abs(rg.astype(np.float64) - np.array([O.reward(Pi(i), self.task, qg[i], vg[i], tg[i]) for i in range(len(rg))]))
        rb = tr.reward_bound(P, self.task, qg, vg, tg)
        self.reward_bad += int((own > rb).sum())          # (a non-finite reward counts: the comparison is False only inside the bound)
        self.reward_bad += int((~np.isfinite(own)).sum())
        self.worst_reward_own = max(self.worst_reward_own, float(own.max()))
        self.worst_reward_ratio = max(self.worst_reward_ratio, float((own / rb).max()))
        og = og.astype(np.float64)
        w = within(og, oo)
        err = np.abs(og - oo)
        self.steps += 1; self.env_steps += len(rg)
        self.ok += w.sum(); self.tot += w.size
        self.okr += within(rg.astype(np.float64), ro).sum()
        self.big += (err > 1e-2).sum()
        self.worst = max(self.worst, err.max())
        self.well_tot += w[well].size; self.well_ok += w[well].sum(); self.well_big += (err[well] > 1e-2).sum()
        strict = ~strict_within(og, oo)
        viol = strict.any(axis=1)              # env-steps with an entry outside the strict tolerance, whatever their class
        self.strict_bad += int(strict[well].sum())
        self.far_off += int((err > 1e-3 * np.abs(oo) + 1e-5).any(axis=1).sum())
        flipped = viol & ~(deep & unconv)          # (what leaves the tolerance in the unconverged part of the deep class is no flip: DEEP_ERROR_CAP)
        if self.contacts and flipped.any():
            self.flip_margin_max = max(self.flip_margin_max, float(switch[flipped].max()))      # the LARGEST contact-switch margin at which fp32 still flipped: what MARGIN_TOL must cover
        if well.any():
            self.worst_well = max(self.worst_well, err[well].max())
            self.unconverged_well += int((well & unconv).sum())
        if deep.any():
            self.deep_steps += int(deep.sum()); self.deep_bad += int((~w[deep]).sum())
            self.deep_strict_bad += int(strict[deep].sum())
            self.worst_deep = max(self.worst_deep, float(err[deep].max()))
            cl = deep & unconv
            self.clamped_steps += int(cl.sum()); self.clamped_strict_bad += int(strict[cl].sum())
            if cl.any():
                self.worst_clamped = max(self.worst_clamped, float(err[cl].max()))
            if (deep & ~cl).any():
                self.worst_deep_converged = max(self.worst_deep_converged, float(err[deep & ~cl].max()))
        if (~near).any():
            self.worst_reward_held = max(self.worst_reward_held, float(np.abs(rg.astype(np.float64) - ro)[~near].max()))
        ill_bad = near & ~w.all(axis=1)
        self.ill_steps += near.sum(); self.ill_bad_steps += ill_bad.sum()
        if near.any():
            self.worst_ill = max(self.worst_ill, err[near].max())
        return ill_bad

    def cascade(self, followed, o2, og2, oo2):
        sel = followed & ~classify(o2, self.contacts)[2]          # (that next step is held to the strict line whether it is deep or not)
        self.cascade_checked += int(sel.sum())
        if sel.any():
            self.cascade_bad += int((~strict_within(og2.astype(np.float64)[sel], oo2[sel]).all(axis=1)).sum())

    def result(self, cap, **extra):
        env_steps = self.env_steps          # (n x steps, unless add() was given a selection)
        return dict(well_bad=int(self.well_tot - self.well_ok), frac=self.ok / self.tot, worst=self.worst, frac_reward=self.okr / env_steps, cap=float(cap), frac_big=self.big / self.tot,
                    well_frac=self.well_ok / max(self.well_tot, 1), well_big=int(self.well_big), worst_well=self.worst_well,
                    ill_frac=self.ill_steps / env_steps, ill_steps=int(self.ill_steps), ill_bad_steps=int(self.ill_bad_steps),
                    strict_bad=int(self.strict_bad), worst_ill=float(self.worst_ill), flip_margin_max=self.flip_margin_max, cascade_checked=int(self.cascade_checked), cascade_bad=int(self.cascade_bad),
                    env_steps=env_steps, deep_steps=int(self.deep_steps), deep_bad=int(self.deep_bad), deep_strict_bad=int(self.deep_strict_bad), worst_deep=float(self.worst_deep),
                    clamped_steps=int(self.clamped_steps), clamped_strict_bad=int(self.clamped_strict_bad), worst_clamped=self.worst_clamped, worst_deep_converged=self.worst_deep_converged,
                    unconverged_well=int(self.unconverged_well), far_off=int(self.far_off), worst_reward_held=self.worst_reward_held,
                    reward_bad=int(self.reward_bad), worst_reward_own=self.worst_reward_own, worst_reward_ratio=self.worst_reward_ratio, **extra)


def teacher_forced(task, n, steps, seed, contacts=True, params=None, flat_out=False, skip=0, flags=0, actions=None, probe=None, make_env=None, action_seed=None, **env_kw):
    """Returns, next to the north-star counts (within() per entry): `strict_bad` - entries of well-conditioned env-steps outside
    strict_within() (asserted to be ZERO by the callers, no counting) -, `worst_ill` - the largest error on an excluded env-step (bounded by ILL_ERROR_CAP) - and the CASCADE
    check: whenever an excluded env-step is out of tolerance, the GPU's own NEXT step from its own resulting state is held against the oracle's
    from that same state (`cascade_checked` env-steps, `cascade_bad` of them outside the tolerance where that step is well-conditioned).
    Every `well_*` key, `strict_bad` and `worst_well` are over the WELL class; `deep_steps` / `deep_bad` (entries outside within()) /
    `deep_strict_bad` (outside strict_within()) / `worst_deep` the same figures over the DEEP class, `clamped_*` over its env-steps with an
    unconverged narrow phase and `worst_deep_converged` over the others (see DEEP_ERROR_CAP); `ill_*` and `worst_ill` over the
    NEAR-SWITCH class alone (see MARGIN_TOL).  `flip_margin_max`: the largest SWITCH margin of an env-step outside the strict tolerance.
    `resolved`: the main env's solver_stats() before it is closed - wave-substeps that went to the line-searched second solve (None where the
    env under test has no such counter).
    actions(rng, n): another action stream than uniform / flat out; probe(t, q, v, a): called with the oracle's pre-step state.
    make_env(**extra): builds the env under test in place of the JitterbugVecEnv of these arguments - anything with reset, set_state, step,
    get_state, counters, kernel_variant and close; called for the main env (no keywords) and, when a cascade check is first needed, with the
    cascade pair's own keywords (time_limit=inf).  action_seed: the action streams' seed where it is not the envs'."""
    from jitterbug_amd import model
    P = model.default_params() if params is None else params
    per_env = P.ndim == 2
    if make_env is None:
        from jitterbug_amd.vec_env import JitterbugVecEnv
        make_env = lambda **extra: JitterbugVecEnv(n, task, seed=seed, auto_reset=False, contacts=contacts, params=P if per_env else None, flags=flags, **env_kw, **extra)
    g = make_env()
    okw = dict(opts=O.default_opts(contacts=int(contacts)), per_env_model=per_env)
    o = O.OracleEnv(n, task, P, seed=seed, **okw)
    g.reset(), o.reset()
    g2 = o2 = None          # the cascade check's own pair of envs (made when first needed: their step counters must not disturb the main pair's)
    action_seed = seed if action_seed is None else action_seed
    rng = np.random.default_rng(action_seed)
    rng2 = np.random.default_rng(action_seed + 1000)
    tally = ParityTally(n, task, P, contacts)

    def draw(r):
        return np.ones(n) if flat_out else (r.uniform(-1, 1, size=n) if actions is None else actions(r, n))
    for t in range(-skip, steps):
        a = draw(rng)
        if t < 0:                                       # lead-in on the oracle alone (robots tip over), not compared
            o.step(a, auto_reset=False)
            continue
        q, v, tg = o.get_state()
        if probe is not None:
            probe(t, q, v, a)
        g.set_state(q, v, tg)
        og, rg, dg, _ = g.step(a)
        oo, ro, do = o.step(a, auto_reset=False)
        ill_bad = tally.add(o, og, oo, rg, ro, g.get_state())
        assert np.array_equal(dg, do.astype(bool))
        if ill_bad.any() and contacts and not dg.any():
            # a flipped contact must not cascade: from the GPU's OWN state after that step, its next step agrees with the oracle's
            if g2 is None:
                g2 = make_env(time_limit=float("inf"))
                o2 = O.OracleEnv(n, task, P, seed=seed, **okw)
                g2.reset(), o2.reset()
            q2, v2, t2 = g.get_state()
            g2.set_state(q2, v2, t2); o2.set_state(q2, v2, t2)
            a2 = draw(rng2)
            og2 = g2.step(a2)[0]
            oo2 = o2.step(a2, auto_reset=False)[0]
            tally.cascade(ill_bad, o2, og2, oo2)
    sc, ep, cap = g.counters()
    variant = g.kernel_variant
    stats = getattr(g, "solver_stats", None)          # (an env under test without the counter - a host stand-in - reports None)
    resolved = None if stats is None else int(stats())
    g.close()
    if g2 is not None:
        g2.close()
    q, _, _ = o.get_state()
    tipped = float(((1 - 2 * (q[:, 4] ** 2 + q[:, 5] ** 2)) < 0.5).mean())
    return tally.result(cap.sum(), tipped=tipped, kernel_variant=variant, resolved=resolved)


def free_running(env, o, idx, steps, actions, tally=None, hook=None):
    """Teacher-forced the other way round: the env under test runs FREE (env and o built and reset by the caller; actions(t): the whole batch's),
    and every control step its pre-step state of the subset `idx` is copied into the oracle env `o` of len(idx) envs, which takes the same step.
    A `tally` is fed every compared step, and its cascade check needs no second env: the near-switch env-steps that left the tolerance at step t
    are followed into step t + 1, which IS the env's next step from its own state.  hook(t, pre-step (q, v, target) of the whole batch, the
    subset's og, rg, oo, ro, the oracle env just stepped).  Returns the last observation of the whole batch."""
    followed = np.zeros(len(idx), bool)
    for t in range(steps):
        a = actions(t)
        pre = env.get_state()
        og, rg, _, _ = env.step(a)
        o.set_state(*(x[idx] for x in pre))
        oo, ro, _ = o.step(a[idx], auto_reset=False)
        if tally is not None:
            tally.cascade(followed, o, og[idx], oo)
            followed = tally.add(o, og[idx], oo, rg[idx], ro, tuple(x[idx] for x in env.get_state()))
        if hook is not None:
            hook(t, pre, og[idx], rg[idx], oo, ro, o)
    return og


def host_pair_vs_oracle(variant, P, task, seed, steps, flat_out=False, skip=0, actions=None, f32=1, groups=4, deep_only=False):
    """The PAIR (`pair`) or LEAN + PAIR (`pair_lean`) instantiation of the kernel's substep, built for the host (tests/host_harness.cpp) in
    fp32 with four lane groups, against the oracle, teacher-forced like teacher_forced above: one model per env, the
    oracle's state handed to the host build every control step (split into hi + lo words like jb_set_state), observations compared.
    Returns one row per env-step: env, step, switch margin, deep flag, entries outside within(), entries outside
    strict_within(), largest error, residual of the oracle's narrow phase; and how many steps raised the failure flag.  (tools/flip_study.py prints tables of these.)"""
    import ctypes as C
    import tests.build_harness as bh
    lib = C.CDLL(bh.build())
    dp = C.POINTER(C.c_double)
    fn = getattr(lib, "jbh_step_" + variant)
    fn.argtypes = [dp, dp, dp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    n = len(P)
    o = O.OracleEnv(n, task, P, seed=seed, per_env_model=True)
    o.reset()
    rng = np.random.default_rng(seed)
    rows, failed = [], 0
    for t in range(-skip, steps):
        a = np.ones(n) if flat_out else (rng.uniform(-1, 1, size=n) if actions is None else actions(rng, n))
        if t < 0:                                       # lead-in on the oracle alone (robots tip over), not compared
            o.step(a, auto_reset=False)
            continue
        q0, v0, tg = o.get_state()
        oo, _, _ = o.step(a, auto_reset=False)
        c = o.conditioning()
        for i in range(n):
            if deep_only and not c["deep"][i]:          # (a study of the deep class alone, on inputs where it is rare)
                continue
            Pi = np.ascontiguousarray(P[i]); q, v, fail = q0[i].copy(), v0[i].copy(), np.zeros(1)
            assert fn(Pi.ctypes.data_as(dp), q.ctypes.data_as(dp), v.ctypes.data_as(dp), float(np.float32(a[i])), 50, 1, 20, f32, groups, 1, fail.ctypes.data_as(dp)) == 0
            failed += int(fail[0] != 0)
            q[3:7] /= np.linalg.norm(q[3:7])
            ob = O.observation(Pi, task, q, v, tg[i])
            rows.append((i, t, c["switch"][i], c["deep"][i], (~within(ob, oo[i])).sum(), (~strict_within(ob, oo[i])).sum(), np.abs(ob - oo[i]).max(), c["narrow_resid"][i]))
    return np.array(rows, dtype=np.float64), failed

// host_harness.cpp — TEST INFRASTRUCTURE.  Compiles the simulator source the HIP kernel runs
// (jitterbug_amd/csrc/jb_sim.hpp) for the host, with the 4 lanes of a quad emulated by jb::Quad<T>,
// so tests/ can check that math in fp64 and fp32 against the oracle without a GPU.
// It is never linked into, or loaded by, the product library.
#include "host_run.hpp"

extern "C" void jbh_set_offload(int on) { g_offload = on; }
extern "C" void jbh_set_aux(int on) { g_aux = on; }
extern "C" void jbh_set_spread(int on) { g_spread = on; }

template <typename T> static LaneState<Quad<T>> state_from_qpos(const double* qpos, const double* qvel) {
    using V = Quad<T>;
    LaneState<V> s;
    s.px = V(T(qpos[0])); s.py = V(T(qpos[1])); s.pz = V(T(qpos[2]));
    s.qw = V(T(qpos[3])); s.qx = V(T(qpos[4])); s.qy = V(T(qpos[5])); s.qz = V(T(qpos[6]));
    // low-order words of the compensated position state (what jb_set_state imports): value - (double)(T)value
    auto lo = [](double x) { return V(T(x - (double)T(x))); };
    s.pz_lo = lo(qpos[2]); s.qw_lo = lo(qpos[3]); s.qx_lo = lo(qpos[4]); s.qy_lo = lo(qpos[5]); s.qz_lo = lo(qpos[6]);
    s.vx = V(T(qvel[0])); s.vy = V(T(qvel[1])); s.vz = V(T(qvel[2]));
    s.wx = V(T(qvel[3])); s.wy = V(T(qvel[4])); s.wz = V(T(qvel[5]));
    double ph = qpos[15], k = std::floor((ph + M_PI) / (2 * M_PI));
    s.phi = V(T(ph - k * 2 * M_PI)); s.turns = V(T(k)); s.phid = V(T(qvel[14]));
    s.th1 = V(T(qpos[7]), T(qpos[9]), T(qpos[11]), T(qpos[13]));
    s.th2 = V(T(qpos[8]), T(qpos[10]), T(qpos[12]), T(qpos[14]));
    s.thd1 = V(T(qvel[6]), T(qvel[8]), T(qvel[10]), T(qvel[12]));
    s.thd2 = V(T(qvel[7]), T(qvel[9]), T(qvel[11]), T(qvel[13]));
    for (int i = 0; i < 3; i++) { s.wa[i] = V(T(0)); s.wl[i] = V(T(0)); }
    s.wj[0] = s.wj[1] = V(T(0)); s.wm = V(T(0)); s.fail = V(T(0));
    return s;
}
template <typename T> static void qpos_from_state(const LaneState<Quad<T>>& s, double* qpos, double* qvel) {
    T n = std::sqrt(s.qw.v[0] * s.qw.v[0] + s.qx.v[0] * s.qx.v[0] + s.qy.v[0] * s.qy.v[0] + s.qz.v[0] * s.qz.v[0]);
    qpos[0] = s.px.v[0]; qpos[1] = s.py.v[0]; qpos[2] = (double)s.pz.v[0] + (double)s.pz_lo.v[0];
    qpos[3] = ((double)s.qw.v[0] + (double)s.qw_lo.v[0]) / n; qpos[4] = ((double)s.qx.v[0] + (double)s.qx_lo.v[0]) / n;
    qpos[5] = ((double)s.qy.v[0] + (double)s.qy_lo.v[0]) / n; qpos[6] = ((double)s.qz.v[0] + (double)s.qz_lo.v[0]) / n;
    qvel[0] = s.vx.v[0]; qvel[1] = s.vy.v[0]; qvel[2] = s.vz.v[0]; qvel[3] = s.wx.v[0]; qvel[4] = s.wy.v[0]; qvel[5] = s.wz.v[0];
    for (int l = 0; l < 4; l++) { qpos[7 + 2 * l] = s.th1.v[l]; qpos[8 + 2 * l] = s.th2.v[l]; qvel[6 + 2 * l] = s.thd1.v[l]; qvel[7 + 2 * l] = s.thd2.v[l]; }
    qpos[15] = (double)s.phi.v[0] + 2 * M_PI * (double)s.turns.v[0]; qvel[14] = s.phid.v[0];
}

template <typename T>
static int run(const double* P, double* qpos, double* qvel, double ctrl, int nsub, int contacts, int max_newton, int implicit_damp, double* fail, int ngroups, int rank_one, int lean, int pair) {
    using V = Quad<T>;
    HostRun<T> w;
    if (int rc = w.init(P, ngroups, lean != 0, pair != 0, contacts, max_newton, implicit_damp, rank_one)) return rc;
    LaneState<V> s = state_from_qpos<T>(qpos, qvel);
    normalise_state(s);
    w.run(s, [&](typename HostRun<T>::Group& G) {
        if (G.g == 0 && lean) state_store(G.sc, G.s);
        for (int i = 0; i < nsub; i++) {
            w.before_substep(G, true, i == 0);
            if (pair) substep<V, true>(*G.m, G.sc, G.s, V(T(ctrl)), w.o); else substep<V>(*G.m, G.sc, G.s, V(T(ctrl)), w.o);
        }
        if (G.g == 0) { if (lean) state_load(G.sc, G.s); s = G.s; }
    });
    // replicated quantities must agree across the quad
    for (int l = 1; l < 4; l++) if (s.px.v[l] != s.px.v[0] || s.qw.v[l] != s.qw.v[0] || s.wz.v[l] != s.wz.v[0] || s.phid.v[l] != s.phid.v[0]) return -100;
    qpos_from_state<T>(s, qpos, qvel);
    if (fail) *fail = s.fail.v[0];
    return 0;
}

// fp32 or fp64, with ngroups lane groups (1, 2 or 4)
static int run_as(int use_float, const double* P, double* qpos, double* qvel, double ctrl, int nsub, int contacts, int max_newton, int implicit_damp, double* fail, int ngroups = 1, int rank_one = 1, int lean = 0, int pair = 0) {
    if (ngroups != 1 && ngroups != 2 && ngroups != 4) return -101;
    return use_float ? run<float>(P, qpos, qvel, ctrl, nsub, contacts, max_newton, implicit_damp, fail, ngroups, rank_one, lean, pair)
                     : run<double>(P, qpos, qvel, ctrl, nsub, contacts, max_newton, implicit_damp, fail, ngroups, rank_one, lean, pair);
}
extern "C" int jbh_step(const double* P, double* qpos, double* qvel, double ctrl, int nsub, int contacts, int max_newton, int implicit_damp, int use_float, double* fail) {
    return run_as(use_float, P, qpos, qvel, ctrl, nsub, contacts, max_newton, implicit_damp, fail);
}
// the same with ngroups lane groups and the rank-one Newton passes on or off
extern "C" int jbh_step_groups(const double* P, double* qpos, double* qvel, double ctrl, int nsub, int contacts, int max_newton, int use_float, int ngroups, int rank_one, double* fail) {
    return run_as(use_float, P, qpos, qvel, ctrl, nsub, contacts, max_newton, 1, fail, ngroups, rank_one);
}
// ... and in the LEAN variant (state / system / factorisation parked in the scratch, constants never preloaded)
extern "C" int jbh_step_lean(const double* P, double* qpos, double* qvel, double ctrl, int nsub, int contacts, int max_newton, int use_float, int ngroups, int rank_one, double* fail) {
    return run_as(use_float, P, qpos, qvel, ctrl, nsub, contacts, max_newton, 1, fail, ngroups, rank_one, 1);
}
// ... and with the geom-geom pair contact (mass ellipsoid against the upper-leg cylinders): the PAIR instantiation of the substep
extern "C" int jbh_step_pair(const double* P, double* qpos, double* qvel, double ctrl, int nsub, int contacts, int max_newton, int use_float, int ngroups, int rank_one, double* fail) {
    return run_as(use_float, P, qpos, qvel, ctrl, nsub, contacts, max_newton, 1, fail, ngroups, rank_one, 0, 1);
}
// ... and PAIR in the LEAN layout (parked state / system / factorisation incl. the cross term's share, pair frame behind them)
extern "C" int jbh_step_pair_lean(const double* P, double* qpos, double* qvel, double ctrl, int nsub, int contacts, int max_newton, int use_float, int ngroups, int rank_one, double* fail) {
    return run_as(use_float, P, qpos, qvel, ctrl, nsub, contacts, max_newton, 1, fail, ngroups, rank_one, 1, 1);
}
// ---- K control steps in ONE call, the loop of the fused rollout kernel (jb_api.hip step_body): the state, the step counter, the episode
// number and the target stay in the lane variables between the control steps; every step = normalise + nsub substeps +
// control_step_tail (jb_step.hpp: failure flag, reward, time limit, in-place reset, observation) and, with actions == NULL, the heuristic
// policy evaluated on the observation just produced.  ngroups = 1 (main lanes) or 4 (main + replica + two helper groups, one thread each).
// io: qpos/qvel/target in and out; rows_out [K, D+2] = [obs | reward | done]; counters = [step_count, episode] in and out.
template <typename T>
static int rollout(const double* P, double* qpos, double* qvel, double* target, int* counters, int K, const double* actions, int task, int nsub, int step_limit, int auto_reset,
                   int random_pose, unsigned long long seed, unsigned long long env_global, const double* policy_params, int ngroups, double* rows_out) {
    using V = Quad<T>;
    HostRun<T> w;
    if (int rc = w.init(P, ngroups, false, false, 1, 12, 1, 1)) return rc;
    const int D = obs_dim(task);
    TaskOpts topt; topt.task = task; topt.step_limit = step_limit; topt.auto_reset = auto_reset; topt.random_pose = random_pose; topt.seed = seed; topt.env_global = env_global;
    PolicyParams<T> pp = default_policy_params<T>();
    if (policy_params) { pp.kick_angle = T(policy_params[0]); pp.speed = T(policy_params[1]); pp.angle_threshold = T(policy_params[2]); }
    LaneState<V> s_final;
    EpisodeRegs<T> er_final;
    w.run(state_from_qpos<T>(qpos, qvel), [&](typename HostRun<T>::Group& G) {
        const LaneModel<V>& mg = *G.m;
        LaneState<V>& s = G.s;
        const bool rep = G.rep;
        EpisodeRegs<T> er;
        er.step_count = counters[0]; er.episode = (uint32_t)counters[1];
        er.tgt[0] = T(target[0]); er.tgt[1] = T(target[1]); er.tgt[2] = T(target[2]);
        T ctrl_next = T(0);
        if (!actions && rep) {
            T obs0[19];
            EnvCore<T> e0;
            core_from_lane_state<V>(mg, s, er.tgt, e0);
            observe<T>(task, e0, lane0(mg.c[LM_TARGET_Z]), obs0, 1);
            ctrl_next = heuristic_policy<T>(task, obs0, 1, pp);
        }
        for (int k = 0; k < K; k++) {
            T ctrl = ctrl_next;
            if (actions && rep) ctrl = T(actions[k]);
            if (rep) normalise_state(s);
            for (int i = 0; i < nsub; i++) {
                w.before_substep(G, false, i == 0);      // (no pair contact here: every slot is poisoned before every substep)
                substep<V>(mg, G.sc, s, V(ctrl), w.o);
            }
            if (!rep) continue;
            T obs[19], rew;
            bool done;
            control_step_tail<V>(topt, mg, s, er, obs, rew, done);
            if (!actions) ctrl_next = heuristic_policy<T>(task, obs, 1, pp);
            if (G.g == 0) {
                double* row = rows_out + (size_t)k * (D + 2);
                for (int j = 0; j < D; j++) row[j] = (double)obs[j];
                row[D] = (double)rew; row[D + 1] = done ? 1.0 : 0.0;
            }
        }
        if (G.g == 0) { s_final = s; er_final = er; }
    });
    qpos_from_state<T>(s_final, qpos, qvel);
    target[0] = er_final.tgt[0]; target[1] = er_final.tgt[1]; target[2] = er_final.tgt[2];
    counters[0] = er_final.step_count; counters[1] = (int)er_final.episode;
    return 0;
}
extern "C" int jbh_rollout(const double* P, double* qpos, double* qvel, double* target, int* counters, int K, const double* actions, int task, int nsub, int step_limit,
                           int auto_reset, int random_pose, unsigned long long seed, unsigned long long env_global, const double* policy_params, int ngroups, int use_float, double* rows_out) {
    if (ngroups != 1 && ngroups != 4) return -101;
    return use_float ? rollout<float>(P, qpos, qvel, target, counters, K, actions, task, nsub, step_limit, auto_reset, random_pose, seed, env_global, policy_params, ngroups, rows_out)
                     : rollout<double>(P, qpos, qvel, target, counters, K, actions, task, nsub, step_limit, auto_reset, random_pose, seed, env_global, policy_params, ngroups, rows_out);
}
// ---- the task layer alone (jb_task.hpp observe / reward / reward_terms / heuristic_policy) on n states, T = double or float: each state
// goes through the words the device holds (state_from_qpos: T-rounded root state, wrapped motor angle) and core_from_lane_state, as in the
// kernels.  out [n, 25] = [obs(19, zeros beyond the task's width) | reward | P, H, V, U | action of the heuristic policy on that row]
template <typename T>
static int task_layer(const double* P, int task, int n, const double* qpos, const double* qvel, const double* target, const double* policy_params, double* out) {
    using V = Quad<T>;
    HostRun<T> w;
    if (int rc = w.init(P, 1, false, false, 1, 12, 1, 1)) return rc;
    PolicyParams<T> pp = default_policy_params<T>();
    if (policy_params) { pp.kick_angle = T(policy_params[0]); pp.speed = T(policy_params[1]); pp.angle_threshold = T(policy_params[2]); }
    const T target_z = lane0(w.m.c[LM_TARGET_Z]);
    for (int i = 0; i < n; i++) {
        const LaneState<V> s = state_from_qpos<T>(qpos + (size_t)i * 16, qvel + (size_t)i * 15);
        const T tgt[3] = {T(target[3 * i]), T(target[3 * i + 1]), T(target[3 * i + 2])};
        EnvCore<T> e;
        core_from_lane_state<V>(w.m, s, tgt, e);
        T obs[19], terms[4];
        observe<T>(task, e, target_z, obs, 1);
        reward_terms<T>(e, target_z, terms);
        double* o = out + (size_t)i * 25;
        for (int j = 0; j < 19; j++) o[j] = j < obs_dim(task) ? (double)obs[j] : 0.0;
        o[19] = (double)reward<T>(task, e, target_z);
        for (int j = 0; j < 4; j++) o[20 + j] = (double)terms[j];
        o[24] = (double)heuristic_policy<T>(task, obs, 1, pp);
    }
    return 0;
}
extern "C" int jbh_task_layer(const double* P, int task, int n, const double* qpos, const double* qvel, const double* target, const double* policy_params, int use_float, double* out) {
    return use_float ? task_layer<float>(P, task, n, qpos, qvel, target, policy_params, out) : task_layer<double>(P, task, n, qpos, qvel, target, policy_params, out);
}
// heuristic_policy<float> on n given observation rows [n, obs_dim(task)] (what jb_policy_device computes)
extern "C" void jbh_policy_rows(int task, int n, const double* obs, const double* policy_params, double* action) {
    PolicyParams<float> pp = default_policy_params<float>();
    if (policy_params) { pp.kick_angle = float(policy_params[0]); pp.speed = float(policy_params[1]); pp.angle_threshold = float(policy_params[2]); }
    const int D = obs_dim(task);
    for (int i = 0; i < n; i++) {
        float row[19] = {0};
        for (int j = 0; j < D; j++) row[j] = (float)obs[(size_t)i * D + j];
        action[i] = (double)heuristic_policy<float>(task, row, 1, pp);
    }
}
// ONE substep from a captured fp32 record (jb_sim.hpp SimOpts::capture: the substep's entry state with its warm start, 64 floats), main lanes +
// three helper groups; returns the failure counter's increment.  trace = 1 prints the line-searched iteration.
extern "C" int jbh_substep_record(const double* P, const float* rec, int max_newton, int ngroups, int trace, double* fail_out) {
    using T = float;
    using V = Quad<T>;
    HostRun<T> w;
    if (int rc = w.init(P, ngroups, false, false, 1, max_newton, 1, 1)) return rc;
    LaneState<V> s0;
    const T ctrl = rec[0];
    s0.px = V(rec[1]); s0.py = V(rec[2]); s0.pz = V(rec[3]); s0.qw = V(rec[4]); s0.qx = V(rec[5]); s0.qy = V(rec[6]); s0.qz = V(rec[7]);
    s0.pz_lo = V(rec[8]); s0.qw_lo = V(rec[9]); s0.qx_lo = V(rec[10]); s0.qy_lo = V(rec[11]); s0.qz_lo = V(rec[12]);
    s0.vx = V(rec[13]); s0.vy = V(rec[14]); s0.vz = V(rec[15]); s0.wx = V(rec[16]); s0.wy = V(rec[17]); s0.wz = V(rec[18]);
    s0.phi = V(rec[19]); s0.phid = V(rec[20]); s0.turns = V(rec[21]);
    for (int i = 0; i < 3; i++) { s0.wa[i] = V(rec[22 + i]); s0.wl[i] = V(rec[25 + i]); }
    s0.wm = V(rec[28]);
    const float* l = rec + 32;
    s0.th1 = V(l[0], l[6], l[12], l[18]); s0.th2 = V(l[1], l[7], l[13], l[19]); s0.thd1 = V(l[2], l[8], l[14], l[20]); s0.thd2 = V(l[3], l[9], l[15], l[21]);
    s0.wj[0] = V(l[4], l[10], l[16], l[22]); s0.wj[1] = V(l[5], l[11], l[17], l[23]);
    s0.fail = V(T(0));
    LaneState<V> s_final;
    g_ls_trace = trace;
    w.run(s0, [&](typename HostRun<T>::Group& G) {
        w.sync();
        substep<V>(*G.m, G.sc, G.s, V(ctrl), w.o);
        if (G.g == 0) s_final = G.s;
    });
    g_ls_trace = 0;
    if (fail_out) *fail_out = s_final.fail.v[0];
    return 0;
}
// The two fp32 sine / cosine routines of the hinge angles on n given angles: which = 0 jb_sim.hpp sincos_small (the series, |th| <= 0.9),
// 1 jb_lane.hpp vsincos_pi (the quarter-turn reduction).  As this build compiles them: one rounding per operation, nothing fused.
extern "C" void jbh_hinge_sincos_f32(int which, int n, const float* x, float* s, float* c) {
    for (int i = 0; i < n; i++) { if (which) vsincos_pi(x[i], s[i], c[i]); else sincos_small<float>(x[i], s[i], c[i]); }
}
// jb_variant.hpp for the tests.  out = [JB_VARIANT_* id or -1 (no kernel), bytes of dynamic LDS, main lanes, lane groups, offload, aux, split tables,
// scratch floats per lane, pd, pd2, red_lds, waves per SIMD, floats per lane of the block in global memory]; then, from jb_sim.hpp, what the
// layout is stated in: [SC_PD, SC_PD_LEAN, SC_PD2 - SC_OVC, 4 * (NSLOT - ROW_K), SC_COUNT, SC_COUNT_LEAN, SC_COUNT_LEAN_PAIR].  Returns out[0].
extern "C" int jbh_step_layout(int lean, int pair, int per_env_model, int epw, int* out) {
    const StepLayout l = step_layout(epw, lean != 0, pair != 0);
    const int v[20] = {step_variant(lean != 0, pair != 0, per_env_model != 0, epw), (int)step_lds_bytes(l, per_env_model != 0), l.main_lanes, l.groups, l.offload, l.aux, l.split_tables,
                       l.scratch_floats, l.pd, l.pd2, l.red_lds, l.waves_per_simd, l.ovc_floats,
                       SC_PD, SC_PD_LEAN, SC_PD2 - SC_OVC, 4 * (NSLOT - ROW_K), SC_COUNT, SC_COUNT_LEAN, SC_COUNT_LEAN_PAIR};
    for (int i = 0; i < 20; i++) out[i] = v[i];
    return v[0];
}
// What jb_variant.hpp's helpers hand a lane of group grp in the (lean, pair, epw) wave, with the device's stride (the main lanes).  out = [stride,
// grp, ngrp, gstride, floats from the lane's scratch base to its overflow candidates or -1 (outside the scratch), ovc_stride, pd, pd2, red_lds,
// aux_lane, holds_state, SimOpts lean / offload / aux, SC_OVC]
extern "C" void jbh_lane_binding(int lean, int pair, int epw, int grp, int* out) {
    const StepLayout l = step_layout(epw, lean != 0, pair != 0);
    static Quad<float> lds[1], ext[1];       // (addresses only)
    LaneScratch<Quad<float>> sc;
    bind_scratch(sc, l, lds, l.main_lanes, grp, ext);
    const SimOpts o = sim_opts(l, 1, 12, 1, 1, 1);
    const int v[15] = {sc.stride, sc.grp, sc.ngrp, sc.gstride, sc.ovc == ext ? -1 : (int)(sc.ovc - lds), sc.ovc_stride, sc.pd, sc.pd2, sc.red_lds, sc.aux_lane, holds_state(l, grp),
                       o.lean, o.offload, o.aux, SC_OVC};
    for (int i = 0; i < 15; i++) out[i] = v[i];
}
extern "C" void jbh_wave_order_plan(int grid, int wave_slots, int waves_per_simd, int* out) {
    const WaveOrderPlan p = wave_order_plan(grid, wave_slots, waves_per_simd);
    out[0] = p.reorder; out[1] = p.fold_from;
}
// the line-searched second solve (jb_sim.hpp newton_phase<LS = true>): [substeps solved a second time, outer passes of those solves, passes whose
// line search shortened the step, second solves that ended at NEWTON_LS_CAP]
extern "C" void jbh_ls_stats(long* out, int reset) { for (int i = 0; i < 4; i++) { out[i] = g_ls_stats[i]; if (reset) g_ls_stats[i] = 0; } }
extern "C" void jbh_pair_narrow_stats(long* out, int reset) { out[0] = g_pair_narrow_stats[0]; out[1] = g_pair_narrow_stats[1]; if (reset) g_pair_narrow_stats[0] = g_pair_narrow_stats[1] = 0; }
extern "C" int jbh_lm_count(void) { return LM_COUNT; }
// the per-leg constant table (LM_COUNT doubles) for inspection by tests / tools
extern "C" int jbh_lane_table(const double* P, int leg, double* out) { return build_lane_model<double>(P, leg, out); }

// ---- jb_witness.hpp (the run-time witness for the geom pairs the simulator does not collide) on the host: one configuration, from the
// float constant table the device kernel reads -> smallest distance over the unsimulated pairs and the geoms that attain it
#include "../jitterbug_amd/csrc/jb_witness.hpp"
extern "C" int jbh_witness(const double* P, const double* qpos, int* pair, double* out) {
    static thread_local float tab[LM_TABLE];
    const int rc = build_packed_model<float>(P, tab);
    if (rc) return rc;
    double th1[4], th2[4];
    for (int l = 0; l < 4; l++) { th1[l] = qpos[7 + 2 * l]; th2[l] = qpos[8 + 2 * l]; }
    *out = witness_clearance<float>(tab, th1, th2, qpos[15], pair);
    return 0;
}

// ---- jb_device_guard.hpp against a recording stub of hipGetDevice / hipSetDevice (the library instantiates it with the real ones)
#include "../jitterbug_amd/csrc/jb_device_guard.hpp"
namespace {
struct StubDeviceApi {
    static int cur, fail_set, n_set, last_set;
    static int get(int* d) { *d = cur; return 0; }
    static int set(int d) { n_set++; last_set = d; if (fail_set) return 1; cur = d; return 0; }
};
int StubDeviceApi::cur = 0, StubDeviceApi::fail_set = 0, StubDeviceApi::n_set = 0, StubDeviceApi::last_set = -1;
}
// One "entry point" on a handle of device `target` while the caller's current device is `cur` (early_return: the entry point fails
// half way, like a JB_HIP return).  out = [rc of enter, device current INSIDE the entry point, device current AFTER it, hipSetDevice calls]
extern "C" void jbh_device_guard_probe(int cur, int target, int fail_set, int early_return, int* out) {
    StubDeviceApi::cur = cur; StubDeviceApi::fail_set = fail_set; StubDeviceApi::n_set = 0; StubDeviceApi::last_set = -1;
    out[1] = -1;
    auto entry = [&]() -> int {
        jb::DeviceGuard<StubDeviceApi> g;
        const int rc = g.enter(target);
        if (rc) return rc;
        out[1] = StubDeviceApi::cur;
        if (early_return) return -3;
        return 0;
    };
    out[0] = entry();
    out[2] = StubDeviceApi::cur; out[3] = StubDeviceApi::n_set;
}

// ---- jb_owned.hpp against a stub allocator whose k-th allocation fails (the library instantiates it with hipMalloc / hipFree & co.)
#include <set>
#include "../jitterbug_amd/csrc/jb_owned.hpp"
namespace {
struct StubAllocApi {
    static int n_alloc, fail_at, n_free, bad_free;
    static std::set<void*> live;
    static char arena[64];
    template <typename T> static int alloc(T** p, size_t) {
        if (++n_alloc == fail_at) return 2;                  // (the runtime's "out of memory")
        *p = reinterpret_cast<T*>(arena + n_alloc % 64);      // a distinct fake address per live allocation
        live.insert(*p);
        return 0;
    }
    template <typename T> static void free(T* p) { n_free++; if (!live.erase(p)) bad_free++; }
};
int StubAllocApi::n_alloc = 0, StubAllocApi::fail_at = 0, StubAllocApi::n_free = 0, StubAllocApi::bad_free = 0;
std::set<void*> StubAllocApi::live;
char StubAllocApi::arena[64];
struct StubGroup { jb::Owned<float*, StubAllocApi> a, b; jb::Owned<int*, StubAllocApi> c; };
// what jb_api.hip does for a lazily created group: allocate into a local group, move it into the target only when all went well
int fill_group(StubGroup& target) {
    if (target.a) return 0;
    StubGroup g;
    if (int rc = g.a.alloc(4)) return rc;
    if (int rc = g.b.alloc(8)) return rc;
    if (int rc = g.c.alloc(2)) return rc;
    target = std::move(g);
    return 0;
}
bool group_empty(const StubGroup& g) { return !g.a && !g.b && !g.c && !g.a.size() && !g.b.size() && !g.c.size(); }
}
// The k-th allocation (1..3) of a group fails, then the group is built again with nothing failing, rebuilt over a full target, and
// destroyed.  out = [rc of the failed attempt, target empty after it, live allocations after it, rc of the retry, target filled,
// live after it, live after the rebuild, live after destruction, allocations, frees, frees of an address not live]
extern "C" void jbh_owned_group_probe(int k, int* out) {
    StubAllocApi::n_alloc = StubAllocApi::n_free = StubAllocApi::bad_free = 0;
    StubAllocApi::live.clear();
    {
        StubGroup target;
        StubAllocApi::fail_at = k;
        out[0] = fill_group(target);
        out[1] = group_empty(target);
        out[2] = (int)StubAllocApi::live.size();
        StubAllocApi::fail_at = 0;
        out[3] = fill_group(target);
        out[4] = target.a.size() == 4 && target.b.size() == 8 && target.c.size() == 2 && target.a.get() != target.b.get();
        out[5] = (int)StubAllocApi::live.size();
        StubGroup fresh;
        fresh.a = std::move(target.a);       // the old buffers go through moves...
        target = std::move(fresh);           // ...and a move assignment over a filled target frees what it held
        out[6] = (int)StubAllocApi::live.size();
    }
    out[7] = (int)StubAllocApi::live.size();
    out[8] = StubAllocApi::n_alloc; out[9] = StubAllocApi::n_free; out[10] = StubAllocApi::bad_free;
}

// ---- the pair narrow phase of jb_sim.hpp (mass ellipsoid against the upper cylinder of `leg`) on a posed model, fp64 or fp32, for the
// comparison with the oracle's pair_geometric: inputs are the two geoms in WORLD coordinates, out = [dist, n(3), pos(3)]
extern "C" void jbh_pair_narrow(const double* ce, const double* Re, const double* sz, const double* cc, const double* ua, double rad, double half, int use_float, double* out) {
    auto run1 = [&](auto tag) {
        using T = decltype(tag);
        Vec3<T> c_e = v3<T>(T(ce[0]), T(ce[1]), T(ce[2])), s_z = v3<T>(T(sz[0]), T(sz[1]), T(sz[2])), c_c = v3<T>(T(cc[0]), T(cc[1]), T(cc[2])), u_a = v3<T>(T(ua[0]), T(ua[1]), T(ua[2]));
        Mat3<T> R;
        for (int i = 0; i < 9; i++) R.m[i] = T(Re[i]);
        T dist; Vec3<T> n, pos;
        pair_narrow<T>(c_e, R, s_z, c_c, u_a, T(rad), T(half), dist, n, pos);
        out[0] = dist; out[1] = n.x; out[2] = n.y; out[3] = n.z; out[4] = pos.x; out[5] = pos.y; out[6] = pos.z;
    };
    if (use_float) run1(float(0)); else run1(double(0));
}

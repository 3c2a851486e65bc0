// jb_evaluate.hpp — the evaluate pass: a state (the handle's blocks or a snapshot, jb_snapshot.hpp SnapView) -> the task layer's view of it
// under ANY task and ANY target: the observation row, the task reward, the four reward terms and the goal the state attains.  It reads the
// state and the constant tables and writes nothing but its outputs.
//
// Inputs per env-state: the state words the observe kernel reads (jb_api.hip load_state / core_from_state: the HIGH words of the height and
// the quaternion, the WRAPPED motor angle, never the low words or the whole turns), the env's LM_TARGET_Z and the root body's own centre of
// mass LM_C0 (the point the reference's framelinvel sensor measures at), and the target (tx, ty, tpsi): row es of `targets` when given,
// otherwise the one stored in the state (RF_TGT).  `task` is one value for the whole launch.
//
// Outputs per env-state (each may be absent; an absent output is neither computed nor stored):
//   obs      [obs_dim(task)]  observe<T>(task, ...), dense rows
//   reward   [1]              reward<T>(task, ...)
//   terms    [4]              reward_terms<T>: [P, H, V, U]
//   achieved [3]              (px, py, yaw): the goal this state attains, in the target's own coordinates.  px, py are the state words;
//                             yaw = wrap_pi(atan2(R10, R00) - pi/2),  R00 = qw^2 + qx^2 - qy^2 - qz^2,  R10 = 2 (qx qy + qw qz)
//                             - the heading angle_to_target subtracts from the target's, so a target whose tpsi is this yaw gives a
//                             relative angle of zero up to rounding.
//
// The arithmetic is jb_task.hpp's, called unchanged and compiled without multiply-add contraction like every other user of it: on the same
// words the pass gives the bits jb_observe_device, jb_reward_terms_device and the step kernels' epilogue give.
//
// Lane mapping: FOUR LANES PER ENV-STATE like the other passes over states.  The task layer is replicated work (the four lanes of a quad
// compute the same values, as in the observe kernel); the quad shares the STORES: lane l stores entries j with (j & 3) == l of every row.
// The element function is written once on the real type: the device runs it in fp32 (jb_evaluate_kernel below), tests/evaluate_harness.cpp
// runs the same source on the host in fp32 and fp64.
#pragma once
#include "jb_readout.hpp"
#include "jb_step.hpp"

namespace jb {

constexpr int EV_TERMS = 4, EV_GOAL = 3, EV_OBS_MAX = 19;

// where one env-state's rows go (a null pointer: that output is absent)
template <typename T> struct EvOut { T* obs; T* reward; T* terms; T* achieved; };

// the goal a state attains (see the header of this file)
template <typename T> JB_HD void achieved_goal(const EnvCore<T>& e, T (&g)[3]) {
    JB_NO_CONTRACT
    T R00 = e.qw * e.qw + e.qx * e.qx - e.qy * e.qy - e.qz * e.qz;
    T R10 = T(2) * (e.qx * e.qy + e.qw * e.qz);
    g[0] = e.px; g[1] = e.py;
    g[2] = wrap_pi(vatan2(R10, R00) - T(1.5707963267948966));
}

// What the task layer reads of env-state (v, env), through the step kernels' own loader (jb_step.hpp core_from_lane_state): tab is the env's
// packed constant table (LM_TABLE entries), tgt the caller's target or null (the stored one).  *target_z: the env's LM_TARGET_Z.
template <typename T> JB_HD void ev_core(const SnapView& v, long long env, const T* tab, int leg, const T* tgt, EnvCore<T>& e, T* target_z) {
    const long long N = v.n;
    auto R = [&](int f) { return (T)ro_word(v.root[(long long)f * N + env]); };
    LaneModel<T> m;
    m.c.lean = true;                       // nothing preloaded: every constant is read from the table where it is used
    m.c.inv = tab; m.c.tab = tab + LM_INV + leg;
    LaneState<T> s;
    s.px = R(RO_RF_P); s.py = R(RO_RF_P + 1); s.pz = R(RO_RF_P + 2);
    s.qw = R(RO_RF_Q); s.qx = R(RO_RF_Q + 1); s.qy = R(RO_RF_Q + 2); s.qz = R(RO_RF_Q + 3);
    s.vx = R(RO_RF_V); s.vy = R(RO_RF_V + 1); s.vz = R(RO_RF_V + 2);
    s.wx = R(RO_RF_W); s.wy = R(RO_RF_W + 1); s.wz = R(RO_RF_W + 2);
    s.phi = R(RO_RF_PHI); s.phid = R(RO_RF_PHID);
    T t[3];
    if (tgt) { t[0] = tgt[0]; t[1] = tgt[1]; t[2] = tgt[2]; }
    else { t[0] = R(RO_RF_TGT); t[1] = R(RO_RF_TGT + 1); t[2] = R(RO_RF_TGT + 2); }
    core_from_lane_state<T>(m, s, t, e);
    *target_z = m.c[LM_TARGET_Z];
}

// Lane `leg`'s share of an env-state's rows.  Every value is worked out in full (the task layer is replicated over the quad); the lane
// stores entries j with (j & 3) == leg.  `task` is uniform over the launch: the branches on it inside observe / reward are scalar branches.
template <typename T> JB_HD void ev_lane(int task, const EnvCore<T>& e, const T& target_z, int leg, const EvOut<T>& o) {
    if (o.obs) {
        T row[EV_OBS_MAX];
        observe<T>(task, e, target_z, row, 1);
        const int D = obs_dim(task);
#pragma unroll
        for (int j = 0; j < EV_OBS_MAX; j++) if ((j & 3) == leg && j < D) o.obs[j] = row[j];
    }
    if (o.reward) {
        const T r = reward<T>(task, e, target_z);
        if (leg == 0) o.reward[0] = r;
    }
    if (o.terms) {
        T t[EV_TERMS];
        reward_terms<T>(e, target_z, t);
#pragma unroll
        for (int j = 0; j < EV_TERMS; j++) if (j == leg) o.terms[j] = t[j];
    }
    if (o.achieved) {
        T g[EV_GOAL];
        achieved_goal<T>(e, g);
#pragma unroll
        for (int j = 0; j < EV_GOAL; j++) if (j == leg) o.achieved[j] = g[j];
    }
}

#if defined(__HIPCC__)
// ---- the device pass, on jb_readout_kernel's launch plan: one wave per block, RO_EPB env-states per block (a quad each), env-state
// es = snapshot es / N, env es % N, field-major state loads (a root field is one 64-byte run of the block's 16 envs), a lane past the end
// repeats the last env-state so that its loads stay inside the blocks, and stores nothing.  The rows are short (at most 19 words), so they
// leave the quad directly, spread over its four lanes as the observe kernel's do: no LDS, no row in private memory.
struct EvArgs {
    SnapView first;              // snapshot 0 (or the handle's blocks); first.n = N envs
    long long stride_words;      // distance between consecutive snapshots, in 4-byte words
    long long total;             // n_snaps * N env-states
    const float* tab; int n_tab; // n_tab tables of LM_TABLE floats: one shared, or one per env (taken by env % n_tab)
    int task;
    const float* targets;        // [total, 3] or null: the stored target
    float *obs, *reward, *terms, *achieved;
};
__global__ __launch_bounds__(64) void jb_evaluate_kernel(EvArgs a) {
    const int tid = threadIdx.x, q = tid >> 2, leg = tid & 3;
    const long long at = (long long)blockIdx.x * RO_EPB + q;
    const bool live = at < a.total;
    const long long es = live ? at : a.total - 1;
    const long long k = es / a.first.n, env = es - k * a.first.n;
    SnapView v = a.first;
    v.root += k * a.stride_words;
    EnvCore<float> e;
    float target_z;
    ev_core<float>(v, env, a.tab + (size_t)(env % a.n_tab) * LM_TABLE, leg, a.targets ? a.targets + (size_t)es * EV_GOAL : nullptr, e, &target_z);
    if (!live) return;
    const int D = obs_dim(a.task);
    EvOut<float> o;
    o.obs = a.obs ? a.obs + (size_t)es * D : nullptr;
    o.reward = a.reward ? a.reward + (size_t)es : nullptr;
    o.terms = a.terms ? a.terms + (size_t)es * EV_TERMS : nullptr;
    o.achieved = a.achieved ? a.achieved + (size_t)es * EV_GOAL : nullptr;
    ev_lane<float>(a.task, e, target_z, leg, o);
}
#endif

}  // namespace jb

// pass_harness.hpp — TEST INFRASTRUCTURE: what the host harnesses of the passes over states (readout_harness.cpp, forward_harness.cpp,
// contacts_harness.cpp) share.  For every harness: the synthetic snapshot stacks and the "absent outputs / a stack equals its snapshots"
// check of the stand-alone sanitizer programs.  For the two that run a substep (they define JB_PASS_SUBSTEP before the include): the lane
// state of a snapshot's words, ONE substep on the step kernels' lane layout (tests/host_run.hpp), and jb_forward.hpp's lanes on its result.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../jitterbug_amd/csrc/jb_model_build.hpp"
#include "../jitterbug_amd/csrc/jb_readout.hpp"

using namespace jb;

// A snapshot stack of n_snaps x N plausible states, every env-state different: a unit quaternion turned by
// tilt_e * (tilt_mod ? e % tilt_mod : e + 1) + tilt_k * k about an axis in the plane of x and quaternion component `axis`, the root at height
// z0 + z_step * ((e + k) % 4), speeds that grow with v_mod ? e % v_mod + 1 : e + 1, the motor at 0.5 * (phi_mod ? e % phi_mod : e) - 1 turning
// at phid, hinge angles th1 * (l + 1) and th2 * (l + 1) + 0.01 k; a target only with `target`, k - 1 motor turns only with a field to put them in.
struct SynthSpec { float tilt_e, tilt_k; int tilt_mod, axis; float z0, z_step, z_lo; int v_mod, phi_mod; float phid; bool target; int turns_field; float th1, th2; };
inline std::vector<uint32_t> synth(const SynthSpec& c, int N, int n_snaps) {
    std::vector<uint32_t> s((size_t)SNAP_WORDS * N * n_snaps, 0u);
    auto put = [](uint32_t* p, float x) { std::memcpy(p, &x, 4); };
    for (int k = 0; k < n_snaps; k++) {
        SnapView v = snap_view(s.data() + (size_t)k * SNAP_WORDS * N, N);
        for (int e = 0; e < N; e++) {
            const float a = c.tilt_e * (float)(c.tilt_mod ? e % c.tilt_mod : e + 1) + c.tilt_k * (float)k;
            double q[4] = {std::cos(0.5 * a), 0.6 * std::sin(0.5 * a), 0.0, 0.0};
            q[c.axis] = 0.8 * std::sin(0.5 * a);
            float r[SNAP_ROOT_F] = {0};
            r[RO_RF_P] = 0.1f * (float)e; r[RO_RF_P + 1] = -0.05f * (float)k; r[RO_RF_P + 2] = c.z0 + c.z_step * (float)((e + k) % 4);
            for (int i = 0; i < 4; i++) { r[RO_RF_Q + i] = (float)q[i]; r[RO_RF_LO + 1 + i] = (float)(q[i] - (double)(float)q[i]); }
            r[RO_RF_LO] = c.z_lo;
            for (int i = 0; i < 6; i++) r[RO_RF_V + i] = 0.01f * (float)(i + 1) * (float)((c.v_mod ? e % c.v_mod : e) + 1);
            r[RO_RF_PHI] = 0.5f * (float)(c.phi_mod ? e % c.phi_mod : e) - 1.f; r[RO_RF_PHID] = c.phid;
            if (c.target) { r[RO_RF_TGT] = 0.2f; r[RO_RF_TGT + 1] = -0.1f; r[RO_RF_TGT + 2] = 0.7f; }
            if (c.turns_field >= 0) r[c.turns_field] = (float)(k - 1);
            for (int f = 0; f < SNAP_ROOT_F; f++) put(&v.root[(size_t)f * N + e], r[f]);
            for (int l = 0; l < 4; l++) {
                const float lf[SNAP_LEG_F] = {c.th1 * (float)(l + 1), c.th2 * (float)(l + 1) + 0.01f * (float)k, 0.3f, -0.2f, 0.f, 0.f};
                for (int f = 0; f < SNAP_LEG_F; f++) put(&v.leg[(size_t)f * 4 * N + 4 * e + l], lf[f]);
            }
        }
    }
    return s;
}

// The sanitizer programs' check of a pass with K nullable outputs, output i holding es_bytes[i] bytes per env-state.  `full` are the outputs
// of the whole stack s with every output present; run(snaps, n_snaps, first env-state, out[K]) runs the pass on n_snaps snapshots with the
// outputs out (NULL: absent) and returns its code.  Every run writes into heap blocks of exactly the promised sizes (the sanitizer sees any
// element beyond them).  Counts: absent outputs in every combination leave the present ones unchanged, and the outputs `stack_outputs` (a
// bit mask) of the stack in one call equal those of its snapshots one by one.
template <size_t K, typename Run>
static int absent_and_stack_mismatches(const std::vector<uint32_t>& s, int N, int n_snaps, const void* const (&full)[K], const size_t (&es_bytes)[K], unsigned stack_outputs, Run run) {
    int bad = 0;
    auto compare = [&](const uint32_t* snaps, int ns, size_t es0, unsigned mask) {
        std::vector<char> got[K];
        void* out[K];
        for (size_t i = 0; i < K; i++) { got[i].resize((size_t)ns * N * es_bytes[i]); out[i] = (mask >> i & 1u) ? got[i].data() : nullptr; }
        bad += run(snaps, ns, es0, out) != 0;
        for (size_t i = 0; i < K; i++) if (out[i]) bad += std::memcmp((const char*)full[i] + es0 * es_bytes[i], out[i], got[i].size()) != 0;
    };
    for (unsigned mask = 1; mask + 1 < (1u << K); mask++) compare(s.data(), n_snaps, 0, mask);
    for (int k = 0; k < n_snaps; k++) {
        const std::vector<uint32_t> one(s.begin() + (size_t)k * SNAP_WORDS * N, s.begin() + (size_t)(k + 1) * SNAP_WORDS * N);
        compare(one.data(), 1, (size_t)k * N, stack_outputs);
    }
    return bad;
}

#ifdef JB_PASS_SUBSTEP
#include "host_run.hpp"

#include "../jitterbug_amd/csrc/jb_forward.hpp"

// the lane state the step kernels load from the blocks (jb_api.hip load_state): every word as it is, warm start included
template <typename T> static LaneState<Quad<T>> state_from_words(const SnapView& v, long long env) {
    using V = Quad<T>;
    const long long N = v.n;
    auto R = [&](int f) { return V((T)ro_word(v.root[(long long)f * N + env])); };
    auto L = [&](int f) { const uint32_t* p = v.leg + (long long)f * 4 * N + 4 * env; return V((T)ro_word(p[0]), (T)ro_word(p[1]), (T)ro_word(p[2]), (T)ro_word(p[3])); };
    LaneState<V> s;
    s.px = R(RO_RF_P); s.py = R(RO_RF_P + 1); s.pz = R(RO_RF_P + 2);
    s.qw = R(RO_RF_Q); s.qx = R(RO_RF_Q + 1); s.qy = R(RO_RF_Q + 2); s.qz = R(RO_RF_Q + 3);
    s.pz_lo = R(RO_RF_LO); s.qw_lo = R(RO_RF_LO + 1); s.qx_lo = R(RO_RF_LO + 2); s.qy_lo = R(RO_RF_LO + 3); s.qz_lo = R(RO_RF_LO + 4);
    s.vx = R(RO_RF_V); s.vy = R(RO_RF_V + 1); s.vz = R(RO_RF_V + 2); s.wx = R(RO_RF_W); s.wy = R(RO_RF_W + 1); s.wz = R(RO_RF_W + 2);
    s.phi = R(RO_RF_PHI); s.phid = R(RO_RF_PHID); s.turns = R(FW_RF_TURNS);
    for (int i = 0; i < 3; i++) { s.wa[i] = R(FW_RF_WA + i); s.wl[i] = R(FW_RF_WL + i); }
    s.wm = R(FW_RF_WM); s.fail = V(T(0));
    s.th1 = L(RO_LF_TH1); s.th2 = L(RO_LF_TH2); s.thd1 = L(RO_LF_THD1); s.thd2 = L(RO_LF_THD2); s.wj[0] = L(FW_LF_WJ0); s.wj[1] = L(FW_LF_WJ1);
    return s;
}

// The runs of a substep pass: one per parameter table of P (env j takes table j % n_models), ngroups lane groups (1: the main lanes alone, 4: the
// pass kernels' wave), pair: the PAIR instantiation of the substep.
template <typename T> static int pass_runs(const double* P, int n_models, int ngroups, int pair, std::vector<HostRun<T>>& runs) {
    if (ngroups != 1 && ngroups != 4) return -101;
    runs = std::vector<HostRun<T>>(n_models);
    for (int t = 0; t < n_models; t++)
        if (int rc = runs[t].init(P + (size_t)t * JB_NPARAM, ngroups, false, pair != 0, 1, 12, 1, 1)) return rc;
    return 0;
}
// ONE substep with the action u on a copy of env-state (v, env), as the pass kernels run it: group 0's state, tap and scratch afterwards.
// Tap has a tap() that hands the substep its listener (jb_contacts.hpp CtTap; Untapped: nobody listens).
struct Untapped { NoTap tap() { return NoTap(); } };
template <typename T, typename Tap> struct Substepped { LaneState<Quad<T>> s; Tap tap; LaneScratch<Quad<T>> sc; };
template <typename T, bool PAIR, typename Tap> static Substepped<T, Tap> one_substep(HostRun<T>& w, const SnapView& v, long long env, T u) {
    using V = Quad<T>;
    LaneState<V> s = state_from_words<T>(v, env);
    normalise_state(s);
    Substepped<T, Tap> r;
    w.run(s, [&](typename HostRun<T>::Group& G) {
        w.before_substep(G, true, true);          // the pair narrow phase starts cold: the first substep of a control step
        Tap mine;
        substep<V, PAIR, decltype(mine.tap())>(*G.m, G.sc, G.s, V(u), w.o, mine.tap());
        if (G.g == 0) { r.s = G.s; r.tap = mine; r.sc = G.sc; }
    });
    return r;
}
template <typename T, typename Tap> static Substepped<T, Tap> one_substep(int pair, HostRun<T>& w, const SnapView& v, long long env, T u) {
    return pair ? one_substep<T, true, Tap>(w, v, env, u) : one_substep<T, false, Tap>(w, v, env, u);
}
// jb_forward.hpp's element function on (the untouched input state, the y the substep left in s1), lane by lane as jb_forward_kernel runs it;
// qfrc is the quad total of the four lanes' partial sums
template <typename T> static void fw_qfrc(const SnapView& v, long long env, const LaneState<Quad<T>>& s1, T u, const T* tab, const FwOut<T>& o) {
    T p[4][6];
    for (int leg = 0; leg < 4; leg++) {
        FwAcc<T> y;
        for (int i = 0; i < 3; i++) { y.lin[i] = s1.wl[i].v[leg]; y.ang[i] = s1.wa[i].v[leg]; }
        y.j1 = s1.wj[0].v[leg]; y.j2 = s1.wj[1].v[leg]; y.m = s1.wm.v[leg];
        fw_lane<T>(fw_load<T>(v, env, leg), y, u, tab, leg, o, p[leg]);
    }
    if (o.qfrc) for (int i = 0; i < 6; i++) o.qfrc[i] = ro_quad_total(p[0][i], p[1][i], p[2][i], p[3][i]);
}
#endif

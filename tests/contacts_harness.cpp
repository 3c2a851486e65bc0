// contacts_harness.cpp — the contact pass compiled for the host (test infrastructure): ONE substep of jb_sim.hpp on the lane layout of the
// step kernels (tests/host_harness.cpp HostRun; tests/forward_harness.cpp's state loading, included as they are) with a SolveTap, then the
// per-slot function of jitterbug_amd/csrc/jb_contacts.hpp on the scratch the substep left, slot by slot as jb_contacts_kernel walks them,
// and - for the tests' sum checks - jb_forward.hpp's qfrc from the same y.
//
// Two builds (tests/test_contacts_cpu.py):
//   g++ -shared                                   jbc_run_f32 / jbc_run_f64 below, driven from numpy through ctypes
//   g++ -DJBC_MAIN -fsanitize=address,undefined   a stand-alone program: ragged sizes, absent outputs and a stack on heap blocks of exactly
//                                                 the promised sizes (main lanes only: no threads under the sanitizer)
#include "forward_harness.cpp"

#include "../jitterbug_amd/csrc/jb_contacts.hpp"

// as forward() of forward_harness.cpp; contact [n_snaps * N, CT_NROW, CT_W], ncon [n_snaps * N], gfrc [n_snaps * N, 22, 3], qfrc [n_snaps * N, 15]
// (the forward pass's, from the same substep), unconv: each nullable
template <typename T> static int contacts(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const double* ctrl, int ngroups, int pair,
                                          T* contact, int32_t* ncon, T* gfrc, T* qfrc, unsigned char* unconv) {
    using V = Quad<T>;
    if (ngroups != 1 && ngroups != 4) return -101;
    std::vector<HostRun<T>> runs(n_models);
    for (int t = 0; t < n_models; t++)
        if (int rc = runs[t].init(P + (size_t)t * JB_NPARAM, ngroups, false, pair != 0, 1, 12, 1, 1)) return rc;
    for (long long es = 0; es < (long long)n_snaps * N; es++) {
        const long long k = es / N, env = es - k * N;
        const SnapView v = snap_view(const_cast<uint32_t*>(snaps) + (size_t)k * SNAP_WORDS * N, N);
        HostRun<T>& w = runs[env % n_models];
        const T u = ctrl ? T(ctrl[es]) : T(0);
        LaneState<V> s = state_from_words<T>(v, env), s1;
        normalise_state(s);
        CtTap<V> tap0;
        LaneScratch<V> sc0;
        w.run(s, [&](typename HostRun<T>::Group& G) {
            w.before_substep(G, true, true);          // the pair narrow phase starts cold: the first substep of a control step
            CtTap<V> mine;
            if (pair) substep<V, true, SolveTap<V>>(*G.m, G.sc, G.s, V(u), w.o, mine.tap()); else substep<V, false, SolveTap<V>>(*G.m, G.sc, G.s, V(u), w.o, mine.tap());
            if (G.g == 0) { s1 = G.s; tap0 = mine; sc0 = G.sc; }
        });
        // the pose, as the kernel takes it: the readout's loads of the untouched input state
        const RoState<T> st = ro_load<T>(v, env, 0);
        const Mat3<T> R = ro_quat2mat(st.q, st.ql);
        CtPose<V> pose;
        for (int i = 0; i < 9; i++) pose.R.m[i] = V(R.m[i]);
        pose.px = V(st.px); pose.py = V(st.py); pose.pz = V(st.pz); pose.pz_lo = V(st.pz_lo);
        const unsigned live = tap0.live;
        const CtY<V> y = ct_y<V>(sc0, tap0);
        T* rows = contact ? contact + (size_t)es * CT_TABLE : nullptr;
        T* gf = gfrc ? gfrc + (size_t)es * CT_GEOMF : nullptr;
        if (rows) for (int i = 0; i < CT_TABLE; i++) rows[i] = T(0);
        if (gf) for (int i = 0; i < CT_GEOMF; i++) gf[i] = T(0);
        int count = 0;
        for (unsigned rest = live; rest; rest &= rest - 1u) {
            const int slot = __builtin_ctz(rest);
            CtRowOut<V> r;
            if (pair) ct_slot<V, true>(w.m, sc0, live, slot, pose, y, r); else ct_slot<V, false>(w.m, sc0, live, slot, pose, y, r);
            for (int leg = 0; leg < 4; leg++) {
                if (!ct_has_row(leg, slot)) continue;
                if (rows) for (int i = 0; i < CT_W; i++) rows[ct_row(leg, slot) * CT_W + i] = r.v[i].v[leg];
                if (gf && slot < SLOT_THREAD) for (int i = 0; i < 3; i++) gf[3 * ct_geom(leg, slot) + i] += r.v[CT_FORCE + i].v[leg];
                count += r.on.v[leg] ? 1 : 0;
            }
        }
        if (ncon) ncon[es] = count;
        if (qfrc) {
            FwOut<T> o;
            o.qacc = nullptr; o.qfrc = qfrc + (size_t)es * FW_NV; o.bacc = nullptr; o.motor = nullptr;
            T p[4][6];
            for (int leg = 0; leg < 4; leg++) {
                FwAcc<T> a;
                for (int i = 0; i < 3; i++) { a.lin[i] = s1.wl[i].v[leg]; a.ang[i] = s1.wa[i].v[leg]; }
                a.j1 = s1.wj[0].v[leg]; a.j2 = s1.wj[1].v[leg]; a.m = s1.wm.v[leg];
                fw_lane<T>(fw_load<T>(v, env, leg), a, u, w.tab, leg, o, p[leg]);
            }
            for (int i = 0; i < 6; i++) o.qfrc[i] = ro_quad_total(p[0][i], p[1][i], p[2][i], p[3][i]);
        }
        if (unconv) unconv[es] = s1.fail.v[0] > T(0) ? 1 : 0;
    }
    return 0;
}

extern "C" {
int jbc_run_f32(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const double* ctrl, int ngroups, int pair,
                float* contact, int32_t* ncon, float* gfrc, float* qfrc, unsigned char* unconv) {
    return contacts<float>(snaps, N, n_snaps, P, n_models, ctrl, ngroups, pair, contact, ncon, gfrc, qfrc, unconv);
}
int jbc_run_f64(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const double* ctrl, int ngroups, int pair,
                double* contact, int32_t* ncon, double* gfrc, double* qfrc, unsigned char* unconv) {
    return contacts<double>(snaps, N, n_snaps, P, n_models, ctrl, ngroups, pair, contact, ncon, gfrc, qfrc, unconv);
}
void jbc_slot_geoms(int32_t* out) { ct_slot_geoms(out); }
}  // extern "C"

#ifdef JBC_MAIN
#include "../jitterbug_amd/csrc/jb_default_params.h"

// states on or below the floor, every one different: the robot lowered so that feet and legs touch, tilted further with the env index
static std::vector<uint32_t> synth_low(int N, int n_snaps) {
    std::vector<uint32_t> s((size_t)SNAP_WORDS * N * n_snaps, 0u);
    auto put = [](uint32_t* p, float x) { std::memcpy(p, &x, 4); };
    for (int k = 0; k < n_snaps; k++) {
        SnapView v = snap_view(s.data() + (size_t)k * SNAP_WORDS * N, N);
        for (int e = 0; e < N; e++) {
            const float a = 0.08f * (float)(e % 9) + 0.03f * (float)k;
            const double q[4] = {std::cos(0.5 * a), 0.6 * std::sin(0.5 * a), 0.8 * std::sin(0.5 * a), 0.0};
            float r[SNAP_ROOT_F] = {0};
            r[RO_RF_P] = 0.1f * (float)e; r[RO_RF_P + 1] = -0.05f * (float)k; r[RO_RF_P + 2] = 0.012f + 0.002f * (float)((e + k) % 4);
            for (int i = 0; i < 4; i++) { r[RO_RF_Q + i] = (float)q[i]; r[RO_RF_LO + 1 + i] = (float)(q[i] - (double)(float)q[i]); }
            for (int i = 0; i < 6; i++) r[RO_RF_V + i] = 0.01f * (float)(i + 1) * (float)(e % 5 + 1);
            r[RO_RF_PHI] = 0.5f * (float)(e % 6) - 1.f; r[RO_RF_PHID] = 30.f;
            for (int f = 0; f < SNAP_ROOT_F; f++) put(&v.root[(size_t)f * N + e], r[f]);
            for (int l = 0; l < 4; l++) {
                const float lf[SNAP_LEG_F] = {0.05f * (float)(l + 1), -0.04f * (float)(l + 1) + 0.01f * (float)k, 0.3f, -0.2f, 0.f, 0.f};
                for (int f = 0; f < SNAP_LEG_F; f++) put(&v.leg[(size_t)f * 4 * N + 4 * e + l], lf[f]);
            }
        }
    }
    return s;
}
static int check_case(int N, int n_snaps, int pair) {
    const std::vector<uint32_t> s = synth_low(N, n_snaps);
    const size_t M = (size_t)N * n_snaps;
    std::vector<double> u(M);
    for (size_t i = 0; i < M; i++) u[i] = 0.3 * (double)(i % 7) - 1.0;
    std::vector<float> ct(M * CT_TABLE), gf(M * CT_GEOMF);
    std::vector<int32_t> nc(M);
    int bad = jbc_run_f32(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, u.data(), 1, pair, ct.data(), nc.data(), gf.data(), nullptr, nullptr) != 0;
    long long total = 0;
    for (float x : ct) bad += !std::isfinite(x);
    for (float x : gf) bad += !std::isfinite(x);
    for (size_t e = 0; e < M; e++) {
        int act = 0;
        for (int r = 0; r < CT_NROW; r++) act += ct[(e * CT_NROW + r) * CT_W + CT_ACTIVE] != 0.f;
        bad += act != nc[e];
        total += act;
    }
    // absent outputs leave the present ones unchanged
    for (int mask = 1; mask < 7; mask++) {
        std::vector<float> ct2(M * CT_TABLE), gf2(M * CT_GEOMF);
        std::vector<int32_t> nc2(M);
        bad += jbc_run_f32(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, u.data(), 1, pair, (mask & 1) ? ct2.data() : nullptr, (mask & 2) ? nc2.data() : nullptr,
                           (mask & 4) ? gf2.data() : nullptr, nullptr, nullptr) != 0;
        if (mask & 1) bad += std::memcmp(ct.data(), ct2.data(), 4 * ct.size()) != 0;
        if (mask & 2) bad += std::memcmp(nc.data(), nc2.data(), 4 * nc.size()) != 0;
        if (mask & 4) bad += std::memcmp(gf.data(), gf2.data(), 4 * gf.size()) != 0;
    }
    // a stack in one call equals its snapshots one by one
    for (int k = 0; k < n_snaps; k++) {
        std::vector<uint32_t> one(s.begin() + (size_t)k * SNAP_WORDS * N, s.begin() + (size_t)(k + 1) * SNAP_WORDS * N);
        std::vector<float> ct1((size_t)N * CT_TABLE);
        bad += jbc_run_f32(one.data(), N, 1, JB_DEFAULT_PARAMS, 1, u.data() + (size_t)k * N, 1, pair, ct1.data(), nullptr, nullptr, nullptr, nullptr) != 0;
        bad += std::memcmp(ct1.data(), ct.data() + (size_t)k * N * CT_TABLE, 4 * ct1.size()) != 0;
    }
    std::printf("N %3d  n_snaps %d  pair %d  %lld contacts: %s\n", N, n_snaps, pair, total, bad ? "MISMATCH" : "ok");
    return bad + (total == 0);
}
int main() {
    int bad = 0;
    const int sizes[3] = {1, 5, 17};
    for (int N : sizes) for (int pair = 0; pair < 2; pair++) { bad += check_case(N, 1, pair); bad += check_case(N, 2, pair); }
    std::printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
#endif

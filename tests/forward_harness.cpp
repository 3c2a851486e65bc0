// forward_harness.cpp — the forward-dynamics pass compiled for the host (test infrastructure): ONE substep of jb_sim.hpp on the lane layout
// of the step kernels (tests/host_harness.cpp HostRun, included as it is), then the element function of jitterbug_amd/csrc/jb_forward.hpp
// on (state, y), lane by lane as jb_forward_kernel runs it.
//
// Two builds (tests/test_forward_cpu.py):
//   g++ -shared                                   jbf_run_f32 / jbf_run_f64 below, driven from numpy through ctypes
//   g++ -DJBF_MAIN -fsanitize=address,undefined   a stand-alone program: ragged sizes, absent outputs and a 3-snapshot stack on heap blocks
//                                                 of exactly the promised sizes (main lanes only: no threads under the sanitizer)
#include "host_harness.cpp"

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

// snaps: n_snaps snapshots of N envs back to back (the device's block layout); P: n_models parameter tables, env j takes table j % n_models;
// ctrl [n_snaps * N] nullable (NULL: 0).  ngroups lane groups (1: the main lanes alone, 4: the forward kernel's wave), pair: the PAIR
// instantiation of the substep.  Every output [n_snaps * N, ...] is nullable.
template <typename T> static int forward(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const double* ctrl, int ngroups, int pair,
                                         T* qacc, T* qfrc, T* bacc, T* motor, unsigned char* unconv) {
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
        w.run(s, [&](typename HostRun<T>::Group& G) {
            w.before_substep(G, true, true);          // the pair narrow phase starts cold: the first substep of a control step
            if (pair) substep<V, true>(*G.m, G.sc, G.s, V(u), w.o); else substep<V>(*G.m, G.sc, G.s, V(u), w.o);
            if (G.g == 0) s1 = G.s;
        });
        FwOut<T> o;
        o.qacc = qacc ? qacc + (size_t)es * FW_NV : nullptr;
        o.qfrc = qfrc ? qfrc + (size_t)es * FW_NV : nullptr;
        o.bacc = bacc ? bacc + (size_t)es * FW_BACC : nullptr;
        o.motor = motor ? motor + (size_t)es * FW_MOTOR : nullptr;
        T p[4][6];
        for (int leg = 0; leg < 4; leg++) {
            FwAcc<T> y;
            for (int i = 0; i < 3; i++) { y.lin[i] = s1.wl[i].v[leg]; y.ang[i] = s1.wa[i].v[leg]; }
            y.j1 = s1.wj[0].v[leg]; y.j2 = s1.wj[1].v[leg]; y.m = s1.wm.v[leg];
            fw_lane<T>(fw_load<T>(v, env, leg), y, u, w.tab, leg, o, p[leg]);
        }
        if (o.qfrc) for (int i = 0; i < 6; i++) o.qfrc[i] = ro_quad_total(p[0][i], p[1][i], p[2][i], p[3][i]);
        if (unconv) unconv[es] = s1.fail.v[0] > T(0) ? 1 : 0;
    }
    return 0;
}

extern "C" {
int jbf_run_f32(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const double* ctrl, int ngroups, int pair,
                float* qacc, float* qfrc, float* bacc, float* motor, unsigned char* unconv) {
    return forward<float>(snaps, N, n_snaps, P, n_models, ctrl, ngroups, pair, qacc, qfrc, bacc, motor, unconv);
}
int jbf_run_f64(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const double* ctrl, int ngroups, int pair,
                double* qacc, double* qfrc, double* bacc, double* motor, unsigned char* unconv) {
    return forward<double>(snaps, N, n_snaps, P, n_models, ctrl, ngroups, pair, qacc, qfrc, bacc, motor, unconv);
}
}  // extern "C"

#ifdef JBF_MAIN
#include "../jitterbug_amd/csrc/jb_default_params.h"

// a snapshot stack of n_snaps x N plausible states near the floor (unit quaternion close to upright, small hinge angles), every one different
static std::vector<uint32_t> synth(int N, int n_snaps) {
    std::vector<uint32_t> s((size_t)SNAP_WORDS * N * n_snaps, 0u);
    auto put = [](uint32_t* p, float x) { std::memcpy(p, &x, 4); };
    for (int k = 0; k < n_snaps; k++) {
        SnapView v = snap_view(s.data() + (size_t)k * SNAP_WORDS * N, N);
        for (int e = 0; e < N; e++) {
            const float a = 0.05f * (float)(e + 1) + 0.02f * (float)k;
            const double q[4] = {std::cos(0.5 * a), 0.6 * std::sin(0.5 * a), 0.8 * std::sin(0.5 * a), 0.0};
            float r[SNAP_ROOT_F] = {0};
            r[RO_RF_P] = 0.1f * (float)e; r[RO_RF_P + 1] = -0.05f * (float)k; r[RO_RF_P + 2] = 0.030f + 0.002f * (float)((e + k) % 4);
            for (int i = 0; i < 4; i++) { r[RO_RF_Q + i] = (float)q[i]; r[RO_RF_LO + 1 + i] = (float)(q[i] - (double)(float)q[i]); }
            r[RO_RF_LO] = 1e-10f;
            for (int i = 0; i < 6; i++) r[RO_RF_V + i] = 0.01f * (float)(i + 1) * (float)(e + 1);
            r[RO_RF_PHI] = 0.5f * (float)e - 1.f; r[RO_RF_PHID] = 30.f; r[FW_RF_TURNS] = (float)(k - 1);
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
    const std::vector<uint32_t> s = synth(N, n_snaps);
    const size_t M = (size_t)N * n_snaps;
    std::vector<double> u(M);
    for (size_t i = 0; i < M; i++) u[i] = 0.3 * (double)(i % 7) - 1.0;
    // heap blocks of exactly the promised sizes (the sanitizer sees any element beyond them)
    std::vector<float> qa(M * FW_NV), qf(M * FW_NV), ba(M * FW_BACC), mo(M * FW_MOTOR);
    std::vector<unsigned char> un(M);
    int bad = jbf_run_f32(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, u.data(), 1, pair, qa.data(), qf.data(), ba.data(), mo.data(), un.data()) != 0;
    for (float x : qa) bad += !std::isfinite(x);
    for (float x : qf) bad += !std::isfinite(x);
    for (float x : ba) bad += !std::isfinite(x);
    for (float x : mo) bad += !std::isfinite(x);
    // absent outputs in every combination leave the present ones unchanged
    for (int mask = 1; mask < 15; mask++) {
        std::vector<float> qa2(M * FW_NV), qf2(M * FW_NV), ba2(M * FW_BACC), mo2(M * FW_MOTOR);
        bad += jbf_run_f32(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, u.data(), 1, pair, (mask & 1) ? qa2.data() : nullptr, (mask & 2) ? qf2.data() : nullptr,
                           (mask & 4) ? ba2.data() : nullptr, (mask & 8) ? mo2.data() : nullptr, nullptr) != 0;
        if (mask & 1) bad += std::memcmp(qa.data(), qa2.data(), 4 * qa.size()) != 0;
        if (mask & 2) bad += std::memcmp(qf.data(), qf2.data(), 4 * qf.size()) != 0;
        if (mask & 4) bad += std::memcmp(ba.data(), ba2.data(), 4 * ba.size()) != 0;
        if (mask & 8) bad += std::memcmp(mo.data(), mo2.data(), 4 * mo.size()) != 0;
    }
    // a stack in one call equals its snapshots one by one
    for (int k = 0; k < n_snaps; k++) {
        std::vector<uint32_t> one(s.begin() + (size_t)k * SNAP_WORDS * N, s.begin() + (size_t)(k + 1) * SNAP_WORDS * N);
        std::vector<float> qa1((size_t)N * FW_NV), qf1((size_t)N * FW_NV), ba1((size_t)N * FW_BACC), mo1((size_t)N * FW_MOTOR);
        bad += jbf_run_f32(one.data(), N, 1, JB_DEFAULT_PARAMS, 1, u.data() + (size_t)k * N, 1, pair, qa1.data(), qf1.data(), ba1.data(), mo1.data(), nullptr) != 0;
        bad += std::memcmp(qa1.data(), qa.data() + (size_t)k * N * FW_NV, 4 * qa1.size()) != 0;
        bad += std::memcmp(qf1.data(), qf.data() + (size_t)k * N * FW_NV, 4 * qf1.size()) != 0;
        bad += std::memcmp(ba1.data(), ba.data() + (size_t)k * N * FW_BACC, 4 * ba1.size()) != 0;
        bad += std::memcmp(mo1.data(), mo.data() + (size_t)k * N * FW_MOTOR, 4 * mo1.size()) != 0;
    }
    // fp64 on the same words agrees with fp32 to rounding (accelerations to 1e-3 of the largest entry of the env-state)
    std::vector<double> qad(M * FW_NV);
    bad += jbf_run_f64(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, u.data(), 1, pair, qad.data(), nullptr, nullptr, nullptr, nullptr) != 0;
    for (size_t e = 0; e < M; e++) {
        double top = 1.0;
        for (int i = 0; i < FW_NV; i++) top = std::fmax(top, std::fabs(qad[e * FW_NV + i]));
        for (int i = 0; i < FW_NV; i++) bad += !(std::fabs((double)qa[e * FW_NV + i] - qad[e * FW_NV + i]) < 1e-3 * top);
    }
    std::printf("N %3d  n_snaps %d  pair %d: %s\n", N, n_snaps, pair, bad ? "MISMATCH" : "ok");
    return bad;
}
int main() {
    int bad = 0;
    const int sizes[3] = {1, 5, 17};
    for (int N : sizes) for (int pair = 0; pair < 2; pair++) { bad += check_case(N, 1, pair); bad += check_case(N, 3, pair); }
    std::printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
#endif

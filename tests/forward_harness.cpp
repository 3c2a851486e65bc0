// forward_harness.cpp — the forward-dynamics pass compiled for the host (test infrastructure): ONE substep of jb_sim.hpp on the lane layout
// of the step kernels (tests/pass_harness.hpp one_substep), then the element function of jitterbug_amd/csrc/jb_forward.hpp on (state, y),
// lane by lane as jb_forward_kernel runs it.
//
// Two builds (tests/test_forward_cpu.py):
//   g++ -shared                                   jbf_run_f32 / jbf_run_f64 below, driven from numpy through ctypes
//   g++ -DJBF_MAIN -fsanitize=address,undefined   a stand-alone program: ragged sizes, absent outputs and a 3-snapshot stack on heap blocks
//                                                 of exactly the promised sizes (main lanes only: no threads under the sanitizer)
#define JB_PASS_SUBSTEP
#include "pass_harness.hpp"

// snaps: n_snaps snapshots of N envs back to back (the device's block layout); P: n_models parameter tables, env j takes table j % n_models;
// ctrl [n_snaps * N] nullable (NULL: 0).  ngroups lane groups (1: the main lanes alone, 4: the forward kernel's wave), pair: the PAIR
// instantiation of the substep.  Every output [n_snaps * N, ...] is nullable.
template <typename T> static int forward(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const double* ctrl, int ngroups, int pair,
                                         T* qacc, T* qfrc, T* bacc, T* motor, unsigned char* unconv) {
    std::vector<HostRun<T>> runs;
    if (int rc = pass_runs<T>(P, n_models, ngroups, pair, runs)) return rc;
    for (long long es = 0; es < (long long)n_snaps * N; es++) {
        const long long k = es / N, env = es - k * N;
        const SnapView v = snap_view(const_cast<uint32_t*>(snaps) + (size_t)k * SNAP_WORDS * N, N);
        HostRun<T>& w = runs[env % n_models];
        const T u = ctrl ? T(ctrl[es]) : T(0);
        const auto r = one_substep<T, Untapped>(pair, w, v, env, u);
        FwOut<T> o;
        o.qacc = qacc ? qacc + (size_t)es * FW_NV : nullptr;
        o.qfrc = qfrc ? qfrc + (size_t)es * FW_NV : nullptr;
        o.bacc = bacc ? bacc + (size_t)es * FW_BACC : nullptr;
        o.motor = motor ? motor + (size_t)es * FW_MOTOR : nullptr;
        fw_qfrc<T>(v, env, r.s, u, w.tab, o);
        if (unconv) unconv[es] = r.s.fail.v[0] > T(0) ? 1 : 0;
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

// near the floor: unit quaternions close to upright, small hinge angles, motor turns
static const SynthSpec STATES = {0.05f, 0.02f, 0, 2, 0.030f, 0.002f, 1e-10f, 0, 0, 30.f, false, FW_RF_TURNS, 0.05f, -0.04f};
static int check_case(int N, int n_snaps, int pair) {
    const std::vector<uint32_t> s = synth(STATES, N, n_snaps);
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
    const void* const full[4] = {qa.data(), qf.data(), ba.data(), mo.data()};
    const size_t es_bytes[4] = {4 * FW_NV, 4 * FW_NV, 4 * FW_BACC, 4 * FW_MOTOR};
    bad += absent_and_stack_mismatches(s, N, n_snaps, full, es_bytes, 15u, [&](const uint32_t* snaps, int ns, size_t es0, void* const* o) {
        return jbf_run_f32(snaps, N, ns, JB_DEFAULT_PARAMS, 1, u.data() + es0, 1, pair, (float*)o[0], (float*)o[1], (float*)o[2], (float*)o[3], nullptr);
    });
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

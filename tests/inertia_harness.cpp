// inertia_harness.cpp — the element functions of jitterbug_amd/csrc/jb_inertia.hpp compiled for the host (test infrastructure).
//
// Two builds (tests/test_inertia_cpu.py):
//   g++ -shared                          jbi_run_f32 / jbi_run_f64 below, driven from numpy through ctypes: the device's arithmetic type and
//                                        fp64 (which separates a wrong formula from rounding)
//   g++ -DJBI_MAIN -fsanitize=address,undefined   a stand-alone program: ragged sizes, absent outputs and a 3-snapshot stack on heap
//                                        blocks of exactly the promised sizes, so that an index that leaves a block is reported
#include "pass_harness.hpp"

#include "../jitterbug_amd/csrc/jb_inertia.hpp"

// snaps: n_snaps snapshots of N envs back to back (the device's block layout, hi / lo words included); P: n_models parameter tables
// (include/jitterbug_model.h), env j takes table j % n_models; ctrl [n_snaps * N] or NULL = 0.  Every output [n_snaps * N, ...] is nullable.
// Env-state by env-state, lane by lane, as the device kernel runs it: the first part of the four lanes, the quad totals of their partial
// sums (ro_quad_total's association), the second part, the Jacobian blocks.
template <typename T> static int run(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const T* ctrl, T* qM, T* qfrc, T* qacc, T* jac) {
    std::vector<T> tabs((size_t)n_models * LM_TABLE);
    for (int t = 0; t < n_models; t++) {
        const int rc = build_packed_model<T>(P + (size_t)t * JB_NPARAM, tabs.data() + (size_t)t * LM_TABLE);
        if (rc) return rc;
    }
    for (long long es = 0; es < (long long)n_snaps * N; es++) {
        const long long k = es / N, env = es - k * N;
        const SnapView v = snap_view(const_cast<uint32_t*>(snaps) + (size_t)k * SNAP_WORDS * N, N);
        const T* tab = tabs.data() + (size_t)(env % n_models) * LM_TABLE;
        InOut<T> o;
        o.qM = qM ? qM + (size_t)es * IN_QM : nullptr;
        o.qfrc = qfrc ? qfrc + (size_t)es * IN_QFRC : nullptr;
        o.qacc = qacc ? qacc + (size_t)es * IN_QACC : nullptr;
        o.jac = jac ? jac + (size_t)es * IN_JAC : nullptr;
        InLane<T> L[4];
        T p[4][IN_NP], t[IN_NP];
        for (int leg = 0; leg < 4; leg++) in_lane_a<T>(fw_load<T>(v, env, leg), ctrl ? ctrl[es] : T(0), tab, leg, o, L[leg], p[leg]);
        for (int i = 0; i < IN_NP; i++) t[i] = ro_quad_total(p[0][i], p[1][i], p[2][i], p[3][i]);
        for (int leg = 0; leg < 4; leg++) {
            if (o.qM || o.qfrc || o.qacc) in_lane_b<T>(L[leg], t, leg, o);
            if (o.jac) in_jac<T>(L[leg], leg, o.jac);
        }
    }
    return 0;
}

extern "C" {
int jbi_njac(void) { return IN_NJAC; }
int jbi_words_per_env(void) { return SNAP_WORDS; }
int jbi_run_f32(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const float* ctrl, float* qM, float* qfrc, float* qacc, float* jac) {
    return run<float>(snaps, N, n_snaps, P, n_models, ctrl, qM, qfrc, qacc, jac);
}
int jbi_run_f64(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const double* ctrl, double* qM, double* qfrc, double* qacc, double* jac) {
    return run<double>(snaps, N, n_snaps, P, n_models, ctrl, qM, qfrc, qacc, jac);
}
}  // extern "C"

#ifdef JBI_MAIN
#include "../jitterbug_amd/csrc/jb_default_params.h"

// unit quaternions at any tilt, small hinge angles, whole motor turns
static const SynthSpec STATES = {0.37f, 0.11f, 0, 3, 0.02f, 0.f, 1e-10f, 0, 0, 3.f, true, FW_RF_TURNS, 0.1f, -0.07f};
static int check_case(int N, int n_snaps) {
    const std::vector<uint32_t> s = synth(STATES, N, n_snaps);
    const size_t M = (size_t)N * n_snaps;
    std::vector<float> ctrl(M);
    for (size_t i = 0; i < M; i++) ctrl[i] = 1.5f - 0.4f * (float)(i % 8);      // beyond the ctrlrange at both ends
    // heap blocks of exactly the promised sizes (the sanitizer sees any element beyond them), filled with NaN: every entry is to be written
    const float nan = std::nanf("");
    std::vector<float> qM(M * IN_QM, nan), qf(M * IN_QFRC, nan), qa(M * IN_QACC, nan), ja(M * IN_JAC, nan);
    int bad = jbi_run_f32(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, ctrl.data(), qM.data(), qf.data(), qa.data(), ja.data()) != 0;
    for (float x : qM) bad += !std::isfinite(x);
    for (float x : qf) bad += !std::isfinite(x);
    for (float x : qa) bad += !std::isfinite(x);
    for (float x : ja) bad += !std::isfinite(x);
    // qM is symmetric bit for bit, and M qacc_smooth = passive + actuator - bias to rounding (in fp64 on the fp32 outputs)
    for (size_t e = 0; e < M; e++) {
        const float* A = qM.data() + e * IN_QM;
        for (int i = 0; i < IN_NV; i++) {
            double r = 0, sc = 0;
            for (int j = 0; j < IN_NV; j++) {
                bad += std::memcmp(&A[i * IN_NV + j], &A[j * IN_NV + i], 4) != 0;
                r += (double)A[i * IN_NV + j] * qa[e * IN_QACC + j]; sc += std::fabs((double)A[i * IN_NV + j] * qa[e * IN_QACC + j]);
            }
            const float* f = qf.data() + e * IN_QFRC;
            const double rhs = (double)f[IN_NV + i] + f[2 * IN_NV + i] - f[i];
            bad += !(std::fabs(r - rhs) <= 1e-4 * (sc + std::fabs(rhs)));
        }
    }
    const void* const full[4] = {qM.data(), qf.data(), qa.data(), ja.data()};
    const size_t es_bytes[4] = {4 * IN_QM, 4 * IN_QFRC, 4 * IN_QACC, 4 * IN_JAC};
    bad += absent_and_stack_mismatches(s, N, n_snaps, full, es_bytes, 15u, [&](const uint32_t* snaps, int ns, size_t es0, void* const* o) {
        return jbi_run_f32(snaps, N, ns, JB_DEFAULT_PARAMS, 1, ctrl.data() + es0, (float*)o[0], (float*)o[1], (float*)o[2], (float*)o[3]);
    });
    // fp64 on the same words agrees with fp32 to rounding
    std::vector<double> jad(M * IN_JAC), ctrld(ctrl.begin(), ctrl.end());
    bad += jbi_run_f64(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, ctrld.data(), nullptr, nullptr, nullptr, jad.data()) != 0;
    for (size_t i = 0; i < ja.size(); i++) bad += !(std::fabs((double)ja[i] - jad[i]) < 1e-5);
    std::printf("N %3d  n_snaps %d: %s\n", N, n_snaps, bad ? "MISMATCH" : "ok");
    return bad;
}
int main() {
    int bad = 0;
    const int sizes[3] = {1, 5, 17};
    for (int N : sizes) { bad += check_case(N, 1); bad += check_case(N, 3); }
    std::printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
#endif

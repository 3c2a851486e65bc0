// readout_harness.cpp — the element functions of jitterbug_amd/csrc/jb_readout.hpp compiled for the host (test infrastructure).
//
// Two builds (tests/test_readout_cpu.py):
//   g++ -shared                          jbr_run_f32 / jbr_run_f64 below, driven from numpy through ctypes: the device's arithmetic type and
//                                        fp64 (which separates a wrong formula from rounding)
//   g++ -DJBR_MAIN -fsanitize=address,undefined   a stand-alone program: ragged sizes, absent outputs and a 3-snapshot stack on heap
//                                        blocks of exactly the promised sizes, so that an index that leaves a block is reported
#include "pass_harness.hpp"

// snaps: n_snaps snapshots of N envs back to back (the device's block layout, hi / lo words included); P: n_models parameter tables
// (include/jitterbug_model.h), env j takes table j % n_models.  Every output [n_snaps * N, ...] is nullable.  Env-state by env-state, lane
// by lane, as the device kernel runs it; energy is the quad total of the four lanes' partial sums.
template <typename T> static int run(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, T* frames, T* clear, T* bvel, T* energy) {
    std::vector<T> tabs((size_t)n_models * LM_TABLE);
    for (int t = 0; t < n_models; t++) {
        const int rc = build_packed_model<T>(P + (size_t)t * JB_NPARAM, tabs.data() + (size_t)t * LM_TABLE);
        if (rc) return rc;
    }
    for (long long es = 0; es < (long long)n_snaps * N; es++) {
        const long long k = es / N, env = es - k * N;
        const SnapView v = snap_view(const_cast<uint32_t*>(snaps) + (size_t)k * SNAP_WORDS * N, N);
        RoOut<T> o;
        o.frames = frames ? frames + (size_t)es * RO_FRAMES : nullptr;
        o.clear = clear ? clear + (size_t)es * RO_CLEAR : nullptr;
        o.bvel = bvel ? bvel + (size_t)es * RO_BVEL : nullptr;
        o.energy = energy ? energy + (size_t)es * RO_ENERGY : nullptr;
        T e[4][8];
        for (int leg = 0; leg < 4; leg++) {
            const RoState<T> s = ro_load<T>(v, env, leg);
            ro_lane<T>(s, tabs.data() + (size_t)(env % n_models) * LM_TABLE, leg, o, e[leg]);
        }
        if (o.energy) for (int i = 0; i < 8; i++) o.energy[i] = ro_quad_total(e[0][i], e[1][i], e[2][i], e[3][i]);
    }
    return 0;
}

extern "C" {
int jbr_nframe(void) { return RO_NFRAME; }
int jbr_words_per_env(void) { return SNAP_WORDS; }
int jbr_run_f32(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, float* frames, float* clear, float* bvel, float* energy) {
    return run<float>(snaps, N, n_snaps, P, n_models, frames, clear, bvel, energy);
}
int jbr_run_f64(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, double* frames, double* clear, double* bvel, double* energy) {
    return run<double>(snaps, N, n_snaps, P, n_models, frames, clear, bvel, energy);
}
}  // extern "C"

#ifdef JBR_MAIN
#include "../jitterbug_amd/csrc/jb_default_params.h"

// unit quaternions at any tilt, small hinge angles, a target
static const SynthSpec STATES = {0.37f, 0.11f, 0, 3, 0.02f, 0.f, 1e-10f, 0, 0, 3.f, true, -1, 0.1f, -0.07f};
static int check_case(int N, int n_snaps) {
    const std::vector<uint32_t> s = synth(STATES, N, n_snaps);
    const size_t M = (size_t)N * n_snaps;
    // heap blocks of exactly the promised sizes (the sanitizer sees any element beyond them)
    std::vector<float> fr(M * RO_FRAMES), cl(M * RO_CLEAR), bv(M * RO_BVEL), en(M * RO_ENERGY);
    int bad = jbr_run_f32(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, fr.data(), cl.data(), bv.data(), en.data()) != 0;
    // every rotation is orthonormal and every number finite
    for (size_t i = 0; i < M * RO_NFRAME; i++) {
        const float* R = fr.data() + i * RO_FRAME_W + 3;
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {
            const float d = R[3 * a] * R[3 * b] + R[3 * a + 1] * R[3 * b + 1] + R[3 * a + 2] * R[3 * b + 2];
            bad += !(std::fabs(d - (a == b ? 1.f : 0.f)) < 1e-5f);
        }
    }
    for (float x : cl) bad += !std::isfinite(x);
    for (float x : bv) bad += !std::isfinite(x);
    for (float x : en) bad += !std::isfinite(x);
    const void* const full[4] = {fr.data(), cl.data(), bv.data(), en.data()};
    const size_t es_bytes[4] = {4 * RO_FRAMES, 4 * RO_CLEAR, 4 * RO_BVEL, 4 * RO_ENERGY};
    bad += absent_and_stack_mismatches(s, N, n_snaps, full, es_bytes, 15u, [&](const uint32_t* snaps, int ns, size_t, void* const* o) {
        return jbr_run_f32(snaps, N, ns, JB_DEFAULT_PARAMS, 1, (float*)o[0], (float*)o[1], (float*)o[2], (float*)o[3]);
    });
    // fp64 on the same words agrees with fp32 to rounding
    std::vector<double> frd(M * RO_FRAMES), cld(M * RO_CLEAR);
    bad += jbr_run_f64(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, frd.data(), cld.data(), nullptr, nullptr) != 0;
    for (size_t i = 0; i < cl.size(); i++) bad += !(std::fabs((double)cl[i] - cld[i]) < 1e-6);
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

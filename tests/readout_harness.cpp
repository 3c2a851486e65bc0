// readout_harness.cpp — the element functions of jitterbug_amd/csrc/jb_readout.hpp compiled for the host (test infrastructure).
//
// Two builds (tests/test_readout_cpu.py):
//   g++ -shared                          jbr_run_f32 / jbr_run_f64 below, driven from numpy through ctypes: the device's arithmetic type and
//                                        fp64 (which separates a wrong formula from rounding)
//   g++ -DJBR_MAIN -fsanitize=address,undefined   a stand-alone program: ragged sizes, absent outputs and a 3-snapshot stack on heap
//                                        blocks of exactly the promised sizes, so that an index that leaves a block is reported
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../jitterbug_amd/csrc/jb_model_build.hpp"
#include "../jitterbug_amd/csrc/jb_readout.hpp"

using namespace jb;

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

// a snapshot stack of n_snaps x N plausible states (unit quaternion, small hinge angles), every env-state different
static std::vector<uint32_t> synth(int N, int n_snaps) {
    std::vector<uint32_t> s((size_t)SNAP_WORDS * N * n_snaps, 0u);
    auto put = [](uint32_t* p, float x) { std::memcpy(p, &x, 4); };
    for (int k = 0; k < n_snaps; k++) {
        SnapView v = snap_view(s.data() + (size_t)k * SNAP_WORDS * N, N);
        for (int e = 0; e < N; e++) {
            const float a = 0.37f * (float)(e + 1) + 0.11f * (float)k;
            const double q[4] = {std::cos(0.5 * a), 0.6 * std::sin(0.5 * a), 0.0, 0.8 * std::sin(0.5 * a)};
            float r[SNAP_ROOT_F] = {0};
            r[RO_RF_P] = 0.1f * (float)e; r[RO_RF_P + 1] = -0.05f * (float)k; r[RO_RF_P + 2] = 0.02f;
            for (int i = 0; i < 4; i++) { r[RO_RF_Q + i] = (float)q[i]; r[RO_RF_LO + 1 + i] = (float)(q[i] - (double)(float)q[i]); }
            r[RO_RF_LO] = 1e-10f;
            for (int i = 0; i < 6; i++) r[RO_RF_V + i] = 0.01f * (float)(i + 1) * (float)(e + 1);
            r[RO_RF_PHI] = 0.5f * (float)e - 1.f; r[RO_RF_PHID] = 3.f; r[RO_RF_TGT] = 0.2f; r[RO_RF_TGT + 1] = -0.1f; r[RO_RF_TGT + 2] = 0.7f;
            for (int f = 0; f < SNAP_ROOT_F; f++) put(&v.root[(size_t)f * N + e], r[f]);
            for (int l = 0; l < 4; l++) {
                const float lf[SNAP_LEG_F] = {0.1f * (float)(l + 1), -0.07f * (float)(l + 1) + 0.01f * (float)k, 0.3f, -0.2f, 0.f, 0.f};
                for (int f = 0; f < SNAP_LEG_F; f++) put(&v.leg[(size_t)f * 4 * N + 4 * e + l], lf[f]);
            }
        }
    }
    return s;
}
static int check_case(int N, int n_snaps) {
    const std::vector<uint32_t> s = synth(N, n_snaps);
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
    // absent outputs in every combination leave the present ones unchanged
    for (int mask = 1; mask < 15; mask++) {
        std::vector<float> fr2(M * RO_FRAMES), cl2(M * RO_CLEAR), bv2(M * RO_BVEL), en2(M * RO_ENERGY);
        bad += jbr_run_f32(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, (mask & 1) ? fr2.data() : nullptr, (mask & 2) ? cl2.data() : nullptr, (mask & 4) ? bv2.data() : nullptr,
                           (mask & 8) ? en2.data() : nullptr) != 0;
        if (mask & 1) bad += std::memcmp(fr.data(), fr2.data(), 4 * fr.size()) != 0;
        if (mask & 2) bad += std::memcmp(cl.data(), cl2.data(), 4 * cl.size()) != 0;
        if (mask & 4) bad += std::memcmp(bv.data(), bv2.data(), 4 * bv.size()) != 0;
        if (mask & 8) bad += std::memcmp(en.data(), en2.data(), 4 * en.size()) != 0;
    }
    // a stack read in one call equals its snapshots read one by one
    for (int k = 0; k < n_snaps; k++) {
        std::vector<uint32_t> one(s.begin() + (size_t)k * SNAP_WORDS * N, s.begin() + (size_t)(k + 1) * SNAP_WORDS * N);
        std::vector<float> fr1((size_t)N * RO_FRAMES), cl1((size_t)N * RO_CLEAR), bv1((size_t)N * RO_BVEL), en1((size_t)N * RO_ENERGY);
        bad += jbr_run_f32(one.data(), N, 1, JB_DEFAULT_PARAMS, 1, fr1.data(), cl1.data(), bv1.data(), en1.data()) != 0;
        bad += std::memcmp(fr1.data(), fr.data() + (size_t)k * N * RO_FRAMES, 4 * fr1.size()) != 0;
        bad += std::memcmp(cl1.data(), cl.data() + (size_t)k * N * RO_CLEAR, 4 * cl1.size()) != 0;
        bad += std::memcmp(bv1.data(), bv.data() + (size_t)k * N * RO_BVEL, 4 * bv1.size()) != 0;
        bad += std::memcmp(en1.data(), en.data() + (size_t)k * N * RO_ENERGY, 4 * en1.size()) != 0;
    }
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

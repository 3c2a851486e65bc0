// evaluate_harness.cpp — the element functions of jitterbug_amd/csrc/jb_evaluate.hpp compiled for the host (test infrastructure).
//
// Two builds (tests/test_evaluate_cpu.py):
//   g++ -shared                          jbe_run_f32 / jbe_run_f64 below, driven from numpy through ctypes: the device's arithmetic type and
//                                        fp64 (which separates a wrong formula from rounding)
//   g++ -DJBE_MAIN -fsanitize=address,undefined   a stand-alone program: ragged sizes, every task, absent outputs, targets given and stored,
//                                        and a 3-snapshot stack on heap blocks of exactly the promised sizes, so that an index that leaves
//                                        a block is reported
#include "pass_harness.hpp"

#include "../jitterbug_amd/csrc/jb_evaluate.hpp"

// snaps: n_snaps snapshots of N envs back to back (the device's block layout); P: n_models parameter tables (include/jitterbug_model.h),
// env j takes table j % n_models; task 0 .. 4; targets [n_snaps * N, 3] or NULL = the stored ones.  Every output [n_snaps * N, ...] is
// nullable; obs rows are dense, obs_dim(task) wide.  Env-state by env-state, lane by lane, as the device kernel runs it.
template <typename T> static int run(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, int task, const T* targets, T* obs, T* reward, T* terms, T* achieved) {
    if (task < 0 || task > 4) return -201;
    std::vector<T> tabs((size_t)n_models * LM_TABLE);
    for (int t = 0; t < n_models; t++) {
        const int rc = build_packed_model<T>(P + (size_t)t * JB_NPARAM, tabs.data() + (size_t)t * LM_TABLE);
        if (rc) return rc;
    }
    const int D = obs_dim(task);
    for (long long es = 0; es < (long long)n_snaps * N; es++) {
        const long long k = es / N, env = es - k * N;
        const SnapView v = snap_view(const_cast<uint32_t*>(snaps) + (size_t)k * SNAP_WORDS * N, N);
        const T* tab = tabs.data() + (size_t)(env % n_models) * LM_TABLE;
        EvOut<T> o;
        o.obs = obs ? obs + (size_t)es * D : nullptr;
        o.reward = reward ? reward + (size_t)es : nullptr;
        o.terms = terms ? terms + (size_t)es * EV_TERMS : nullptr;
        o.achieved = achieved ? achieved + (size_t)es * EV_GOAL : nullptr;
        for (int leg = 0; leg < 4; leg++) {
            EnvCore<T> e;
            T target_z;
            ev_core<T>(v, env, tab, leg, targets ? targets + (size_t)es * EV_GOAL : nullptr, e, &target_z);
            ev_lane<T>(task, e, target_z, leg, o);
        }
    }
    return 0;
}

extern "C" {
int jbe_obs_dim(int task) { return obs_dim(task); }
int jbe_words_per_env(void) { return SNAP_WORDS; }
int jbe_run_f32(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, int task, const float* targets, float* obs, float* reward, float* terms, float* achieved) {
    return run<float>(snaps, N, n_snaps, P, n_models, task, targets, obs, reward, terms, achieved);
}
int jbe_run_f64(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, int task, const double* targets, double* obs, double* reward, double* terms, double* achieved) {
    return run<double>(snaps, N, n_snaps, P, n_models, task, targets, obs, reward, terms, achieved);
}
}  // extern "C"

#ifdef JBE_MAIN
#include "../jitterbug_amd/csrc/jb_default_params.h"

// unit quaternions at any tilt, a stored target, the motor anywhere in its turn
static const SynthSpec STATES = {0.37f, 0.11f, 0, 3, 0.02f, 0.f, 1e-10f, 0, 0, 3.f, true, -1, 0.1f, -0.07f};
static int check_case(int N, int n_snaps, int task, bool given) {
    const std::vector<uint32_t> s = synth(STATES, N, n_snaps);
    const size_t M = (size_t)N * n_snaps, D = (size_t)obs_dim(task);
    std::vector<float> tg(M * EV_GOAL);
    for (size_t i = 0; i < tg.size(); i++) tg[i] = 0.3f - 0.11f * (float)(i % 7);
    const float* targets = given ? tg.data() : nullptr;
    // heap blocks of exactly the promised sizes (the sanitizer sees any element beyond them), filled with NaN: every entry is to be written
    const float nan = std::nanf("");
    std::vector<float> ob(M * D, nan), rw(M, nan), tm(M * EV_TERMS, nan), ac(M * EV_GOAL, nan);
    int bad = jbe_run_f32(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, task, targets, ob.data(), rw.data(), tm.data(), ac.data()) != 0;
    for (float x : ob) bad += !std::isfinite(x);
    for (float x : rw) bad += !(x >= 0.f && x <= 1.f);
    for (float x : tm) bad += !(x >= 0.f && x <= 1.f);
    for (float x : ac) bad += !std::isfinite(x);
    const void* const full[4] = {ob.data(), rw.data(), tm.data(), ac.data()};
    const size_t es_bytes[4] = {4 * D, 4, 4 * EV_TERMS, 4 * EV_GOAL};
    bad += absent_and_stack_mismatches(s, N, n_snaps, full, es_bytes, 15u, [&](const uint32_t* snaps, int ns, size_t es0, void* const* o) {
        return jbe_run_f32(snaps, N, ns, JB_DEFAULT_PARAMS, 1, task, targets ? targets + es0 * EV_GOAL : nullptr, (float*)o[0], (float*)o[1], (float*)o[2], (float*)o[3]);
    });
    // fp64 on the same words agrees with fp32 to rounding on the copied entries and the rewards
    std::vector<double> rd(M), tgd(tg.begin(), tg.end());
    bad += jbe_run_f64(s.data(), N, n_snaps, JB_DEFAULT_PARAMS, 1, task, given ? tgd.data() : nullptr, nullptr, rd.data(), nullptr, nullptr) != 0;
    for (size_t i = 0; i < M; i++) bad += !(std::fabs((double)rw[i] - rd[i]) < 1e-4);
    std::printf("N %3d  n_snaps %d  task %d  targets %s: %s\n", N, n_snaps, task, given ? "given " : "stored", bad ? "MISMATCH" : "ok");
    return bad;
}
int main() {
    int bad = 0;
    const int sizes[3] = {1, 5, 17};
    for (int N : sizes)
        for (int task = 0; task < 5; task++) { bad += check_case(N, 1, task, task & 1); bad += check_case(N, 3, task, !(task & 1)); }
    std::printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
#endif

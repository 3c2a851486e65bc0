// contacts_harness.cpp — the contact pass compiled for the host (test infrastructure): ONE substep of jb_sim.hpp on the lane layout of the
// step kernels (tests/pass_harness.hpp one_substep) with a SolveTap, then the
// per-slot function of jitterbug_amd/csrc/jb_contacts.hpp on the scratch the substep left, slot by slot as jb_contacts_kernel walks them,
// and - for the tests' sum checks - jb_forward.hpp's qfrc from the same y.
//
// Two builds (tests/test_contacts_cpu.py):
//   g++ -shared                                   jbc_run_f32 / jbc_run_f64 below, driven from numpy through ctypes
//   g++ -DJBC_MAIN -fsanitize=address,undefined   a stand-alone program: ragged sizes, absent outputs and a stack on heap blocks of exactly
//                                                 the promised sizes (main lanes only: no threads under the sanitizer)
#define JB_PASS_SUBSTEP
#include "pass_harness.hpp"

#include "../jitterbug_amd/csrc/jb_contacts.hpp"

// arguments as forward() of forward_harness.cpp; contact [n_snaps * N, CT_NROW, CT_W], ncon [n_snaps * N], gfrc [n_snaps * N, 22, 3], qfrc [n_snaps * N, 15]
// (the forward pass's, from the same substep), unconv: each nullable
template <typename T> static int contacts(const uint32_t* snaps, int N, int n_snaps, const double* P, int n_models, const double* ctrl, int ngroups, int pair,
                                          T* contact, int32_t* ncon, T* gfrc, T* qfrc, unsigned char* unconv) {
    using V = Quad<T>;
    std::vector<HostRun<T>> runs;
    if (int rc = pass_runs<T>(P, n_models, ngroups, pair, runs)) return rc;
    for (long long es = 0; es < (long long)n_snaps * N; es++) {
        const long long k = es / N, env = es - k * N;
        const SnapView v = snap_view(const_cast<uint32_t*>(snaps) + (size_t)k * SNAP_WORDS * N, N);
        HostRun<T>& w = runs[env % n_models];
        const T u = ctrl ? T(ctrl[es]) : T(0);
        const auto sub = one_substep<T, CtTap<V>>(pair, w, v, env, u);
        const LaneScratch<V>& sc0 = sub.sc;
        // the pose, as the kernel takes it: the readout's loads of the untouched input state
        const RoState<T> st = ro_load<T>(v, env, 0);
        const Mat3<T> R = ro_quat2mat(st.q, st.ql);
        CtPose<V> pose;
        for (int i = 0; i < 9; i++) pose.R.m[i] = V(R.m[i]);
        pose.px = V(st.px); pose.py = V(st.py); pose.pz = V(st.pz); pose.pz_lo = V(st.pz_lo);
        const unsigned live = sub.tap.live;
        const CtY<V> y = ct_y<V>(sc0, sub.tap);
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
            fw_qfrc<T>(v, env, sub.s, u, w.tab, o);
        }
        if (unconv) unconv[es] = sub.s.fail.v[0] > T(0) ? 1 : 0;
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

// on or below the floor: the robot lowered so that feet and legs touch, tilted further with the env index
static const SynthSpec STATES = {0.08f, 0.03f, 9, 2, 0.012f, 0.002f, 0.f, 5, 6, 30.f, false, -1, 0.05f, -0.04f};
static int check_case(int N, int n_snaps, int pair) {
    const std::vector<uint32_t> s = synth(STATES, N, n_snaps);
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
    const void* const full[3] = {ct.data(), nc.data(), gf.data()};
    const size_t es_bytes[3] = {4 * CT_TABLE, 4, 4 * CT_GEOMF};
    bad += absent_and_stack_mismatches(s, N, n_snaps, full, es_bytes, 1u, [&](const uint32_t* snaps, int ns, size_t es0, void* const* o) {
        return jbc_run_f32(snaps, N, ns, JB_DEFAULT_PARAMS, 1, u.data() + es0, 1, pair, (float*)o[0], (int32_t*)o[1], (float*)o[2], nullptr, nullptr);
    });
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

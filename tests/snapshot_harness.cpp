// snapshot_harness.cpp — the element functions of jitterbug_amd/csrc/jb_snapshot.hpp compiled for the host (test infrastructure).
//
// Two builds (tests/test_snapshot_cpu.py):
//   g++ -shared                          the jbs_* functions below, driven from numpy through ctypes
//   g++ -DJBS_MAIN -fsanitize=address,undefined   a stand-alone program: the ragged, fan-out and clamped cases on heap blocks of
//                                        exactly the size the layout promises, so that an index that leaves a block is reported
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../jitterbug_amd/csrc/jb_snapshot.hpp"

using namespace jb;

extern "C" {

int jbs_words_per_env(void) { return SNAP_WORDS; }
int jbs_header_bytes(void) { return SNAP_HEADER_BYTES; }

// every word of a destination of n_dst envs from a flat snapshot of n_src envs; the destination is either flat (root == NULL: dst_flat)
// or four separate blocks, as a handle's state is
void jbs_fork(uint32_t* dst_flat, uint32_t* root, uint32_t* leg, uint32_t* step, uint32_t* episode, int n_dst, const uint32_t* src_flat, int n_src, const int32_t* map) {
    SnapView dst;
    if (root) { dst.root = root; dst.leg = leg; dst.step = step; dst.episode = episode; dst.n = n_dst; }
    else dst = snap_view(dst_flat, n_dst);
    const SnapView src = snap_view(const_cast<uint32_t*>(src_flat), n_src);
    const long long total = (long long)SNAP_WORDS * n_dst;
    // the order a grid-stride launch would not take either: every word exactly once, last to first
    for (long long w = total - 1; w >= 0; w--) fork_word(dst, src, map, w);
}

void jbs_return(const float* rew, const unsigned char* done, int K, int N, float gamma, float* returns, int32_t* alive) {
    for (int env = 0; env < N; env++) {
        int a;
        returns[env] = discounted_return(rew, done, K, N, env, gamma, &a);
        alive[env] = a;
    }
}

void jbs_make_header(void* out, int n_envs, int task_id, int substeps, int step_limit) {
    const SnapHeader hd = snap_make_header(n_envs, task_id, substeps, step_limit);
    std::memcpy(out, &hd, sizeof hd);
}
// 0: the blob can be restored onto a handle of `task_id`; 1: refused (why, if not NULL, receives the message)
int jbs_check_header(const void* blob, long long blob_bytes, int task_id, char* why, int why_len) {
    if (blob_bytes < SNAP_HEADER_BYTES) { if (why) std::snprintf(why, (size_t)why_len, "short"); return 1; }
    SnapHeader hd;
    std::memcpy(&hd, blob, sizeof hd);
    const char* msg = snap_check_header(hd, blob_bytes, task_id);
    if (msg && why) std::snprintf(why, (size_t)why_len, "%s", msg);
    return msg ? 1 : 0;
}
int jbs_first_bad_index(const int32_t* map, int n, int n_src) { return snap_first_bad_index(map, n, n_src); }

}  // extern "C"

#ifdef JBS_MAIN
// word (block, field, env, lane) of a synthetic snapshot: every word of every env is different
static uint32_t tag(int block, int f, int env, int l) { return ((uint32_t)block << 28) | ((uint32_t)f << 20) | ((uint32_t)env << 4) | (uint32_t)l; }
static std::vector<uint32_t> synth(int n) {
    std::vector<uint32_t> s((size_t)SNAP_WORDS * n);
    SnapView v = snap_view(s.data(), n);
    for (int f = 0; f < SNAP_ROOT_F; f++) for (int e = 0; e < n; e++) v.root[(size_t)f * n + e] = tag(1, f, e, 0);
    for (int f = 0; f < SNAP_LEG_F; f++) for (int e = 0; e < n; e++) for (int l = 0; l < 4; l++) v.leg[(size_t)f * 4 * n + 4 * e + l] = tag(2, f, e, l);
    for (int e = 0; e < n; e++) { v.step[e] = tag(3, 0, e, 0); v.episode[e] = tag(4, 0, e, 0); }
    return s;
}
static int check_case(const char* name, int n_dst, int n_src, const std::vector<int32_t>* map) {
    const std::vector<uint32_t> src = synth(n_src);
    // four separate heap blocks of exactly the promised sizes (the sanitizer sees any word beyond them)
    std::vector<uint32_t> root((size_t)SNAP_ROOT_F * n_dst), leg((size_t)SNAP_LEG_F * 4 * n_dst), step((size_t)n_dst), episode((size_t)n_dst);
    jbs_fork(nullptr, root.data(), leg.data(), step.data(), episode.data(), n_dst, src.data(), n_src, map ? map->data() : nullptr);
    int bad = 0;
    for (int j = 0; j < n_dst; j++) {
        int s = map ? (*map)[j] : j;
        s = s < 0 ? 0 : s >= n_src ? n_src - 1 : s;
        for (int f = 0; f < SNAP_ROOT_F; f++) bad += root[(size_t)f * n_dst + j] != tag(1, f, s, 0);
        for (int f = 0; f < SNAP_LEG_F; f++) for (int l = 0; l < 4; l++) bad += leg[(size_t)f * 4 * n_dst + 4 * j + l] != tag(2, f, s, l);
        bad += step[j] != tag(3, 0, s, 0);
        bad += episode[j] != tag(4, 0, s, 0);
    }
    std::printf("%-28s n_dst %4d n_src %4d: %s\n", name, n_dst, n_src, bad ? "MISMATCH" : "ok");
    return bad;
}
int main() {
    int bad = 0;
    bad += check_case("straight copy", 37, 37, nullptr);
    {
        std::vector<int32_t> m(37);
        for (int j = 0; j < 37; j++) m[j] = (j * 7 + 3) % 37;
        bad += check_case("permutation", 37, 37, &m);
    }
    {
        std::vector<int32_t> m(128);
        for (int j = 0; j < 128; j++) m[j] = j / 64;
        bad += check_case("fan-out 2 -> 128", 128, 2, &m);
    }
    {
        std::vector<int32_t> m(5, 0);
        bad += check_case("fan-out 1 -> 5", 5, 1, &m);
    }
    {
        std::vector<int32_t> m = {-1, 3, 2, 0, 3, -2147483647 - 1, 2147483647, 1, 0};      // -1, n_src and far beyond: clamped
        bad += check_case("clamped map", 9, 3, &m);
    }
    bad += check_case("no map, n_src < n_dst (clamped)", 9, 3, nullptr);
    {   // the return recurrence on exactly sized arrays: done at step 0, at step K-1, never
        const int K = 5, N = 3;
        std::vector<float> r((size_t)K * N), out(N);
        std::vector<unsigned char> d((size_t)K * N, 0);
        std::vector<int32_t> alive(N);
        for (int k = 0; k < K; k++) for (int n = 0; n < N; n++) r[(size_t)k * N + n] = 1.f + k;
        d[0 * N + 0] = 1; d[(K - 1) * N + 1] = 1;
        jbs_return(r.data(), d.data(), K, N, 0.5f, out.data(), alive.data());
        const float whole = 1.f + 0.5f * 2.f + 0.25f * 3.f + 0.125f * 4.f + 0.0625f * 5.f;      // exact in fp32
        const bool ok = out[0] == 1.f && alive[0] == 1 && out[1] == whole && alive[1] == K && out[2] == whole && alive[2] == K;
        std::printf("%-28s %s\n", "return recurrence", ok ? "ok" : "MISMATCH");
        bad += ok ? 0 : 1;
    }
    {   // header round trip and the refusals
        std::vector<unsigned char> blob((size_t)snap_blob_bytes(4));
        jbs_make_header(blob.data(), 4, 2, 50, 1000);
        int ok = jbs_check_header(blob.data(), (long long)blob.size(), 2, nullptr, 0) == 0;
        ok &= jbs_check_header(blob.data(), (long long)blob.size() - 1, 2, nullptr, 0) == 1;
        ok &= jbs_check_header(blob.data(), (long long)blob.size(), 3, nullptr, 0) == 1;
        ok &= jbs_check_header(blob.data(), 10, 2, nullptr, 0) == 1;
        blob[0] ^= 1;
        ok &= jbs_check_header(blob.data(), (long long)blob.size(), 2, nullptr, 0) == 1;
        const int32_t m[4] = {0, 3, 4, -1};
        ok &= jbs_first_bad_index(m, 2, 4) == -1 && jbs_first_bad_index(m, 4, 4) == 2 && jbs_first_bad_index(m, 4, 5) == 3;
        std::printf("%-28s %s\n", "blob header / map checks", ok ? "ok" : "MISMATCH");
        bad += ok ? 0 : 1;
    }
    std::printf(bad ? "FAILED\n" : "all ok\n");
    return bad ? 1 : 0;
}
#endif

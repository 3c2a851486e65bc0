// jb_snapshot.hpp — exact snapshot / restore / fork of the simulator state, and the per-env discounted return of a fused rollout.
//
// Everything a handle carries from one launch to the next lives in four device blocks (jb_api.hip, KArgs): root [ROOT_F][N],
// leg [LEG_F][4N], step_count [N], episode [N] - 58 words of 4 bytes = 232 bytes per env (the RNG is stateless: keyed by seed, global
// env, episode, stream).  A SNAPSHOT is those four blocks back to back, in the same field-major layout, for its own env count:
//
//   root [SNAP_ROOT_F][n] | leg [SNAP_LEG_F][4n] | step_count [n] | episode [n]
//
// so snapshot, restore and fork are one copy between two such layouts: word w of the destination comes from the same field of env
// src[j] of the source (a gather; without a map, env j).  The element functions are JB_HD: tests/snapshot_harness.cpp runs the very
// same source on the host.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "jb_lane.hpp"

namespace jb {

constexpr int SNAP_ROOT_F = 32, SNAP_LEG_F = 6;                      // = RootF::ROOT_F, LegF::LEG_F (static_assert in jb_api.hip)
constexpr int SNAP_WORDS = SNAP_ROOT_F + 4 * SNAP_LEG_F + 2;         // 4-byte words per env
constexpr int SNAP_ENV_BYTES = 4 * SNAP_WORDS;                       // 232
constexpr uint32_t SNAP_MAGIC = 0x4E53424Au;                         // "JBSN", little endian
constexpr uint32_t SNAP_VERSION = 1;                                 // layout version of the blocks behind the header
constexpr int SNAP_HEADER_BYTES = 64;

// the four blocks of one side of a copy (a handle's state, or a snapshot), as raw words
struct SnapView {
    uint32_t* root; uint32_t* leg; uint32_t* step; uint32_t* episode;
    int n;
};
JB_HD SnapView snap_view(void* base, int n) {
    uint32_t* p = (uint32_t*)base;
    SnapView v;
    v.n = n; v.root = p; v.leg = p + (size_t)SNAP_ROOT_F * n; v.step = v.leg + (size_t)SNAP_LEG_F * 4 * n; v.episode = v.step + n;
    return v;
}
// every source index is clamped into [0, n): a bad map can select the wrong env, never memory outside the source
JB_HD int snap_clamp(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// Word w of the destination, w in [0, SNAP_WORDS * dst.n), numbered through root | leg | step_count | episode: consecutive w are
// consecutive envs (leg block: consecutive lanes) of one field, so a launch with one thread per word stores coalesced.
// map [dst.n] nullable: destination env j takes source env map[j] (NULL: env j), clamped.
JB_HD void fork_word(const SnapView& dst, const SnapView& src, const int* map, long long w) {
    const long long N = dst.n, S = src.n;
    const long long root_words = (long long)SNAP_ROOT_F * N, leg_words = (long long)SNAP_LEG_F * 4 * N;
    if (w < root_words) {
        const long long f = w / N;
        const int j = (int)(w - f * N), s = snap_clamp(map ? map[j] : j, src.n);
        dst.root[w] = src.root[f * S + s];
    } else if (w < root_words + leg_words) {
        const long long x = w - root_words, f = x / (4 * N), c = x - f * 4 * N;
        const int j = (int)(c >> 2), l = (int)(c & 3), s = snap_clamp(map ? map[j] : j, src.n);
        dst.leg[x] = src.leg[f * 4 * S + 4 * (long long)s + l];
    } else {
        const long long x = w - root_words - leg_words;
        const int j = (int)(x < N ? x : x - N), s = snap_clamp(map ? map[j] : j, src.n);
        if (x < N) dst.step[j] = src.step[s];
        else dst.episode[j] = src.episode[s];
    }
}

// Discounted return of env `env` over a fused rollout's rewards and done flags, both [K, N] row major.  THE ORDER OF OPERATIONS IS
// FIXED (tests/test_gpu_snapshot.py derives its error bound from it), fp32 throughout:
//     acc = 0, g = 1;   for k = 0, 1, ..:   acc = fmaf(g, r[k], acc);   stop if done[k];   g = g * gamma
// i.e. one fused multiply-add per counted step and one multiplication per step after the first.  The step whose done flag is set
// still counts; what follows it (the kernel resets the env in place) belongs to another episode.  *alive = steps counted (K when
// the env was never done).
JB_HD float discounted_return(const float* rew, const unsigned char* done, int K, int N, int env, float gamma, int* alive) {
    float acc = 0.f, g = 1.f;
    int k = 0;
    while (k < K) {
        const size_t i = (size_t)k * (size_t)N + (size_t)env;
        acc = fmaf(g, rew[i], acc);
        k++;
        if (done[i]) break;
        g = g * gamma;
    }
    *alive = k;
    return acc;
}

// ---- the host blob: a 64-byte header in front of the raw blocks
struct SnapHeader {
    uint32_t magic, version;
    int32_t n_envs, task_id, substeps, step_limit, root_f, leg_f;
    uint32_t reserved[8];
};
static_assert(sizeof(SnapHeader) == SNAP_HEADER_BYTES, "the blob header is 64 bytes");
inline long long snap_blob_bytes(long long n) { return SNAP_HEADER_BYTES + (long long)SNAP_ENV_BYTES * n; }
inline SnapHeader snap_make_header(int n_envs, int task_id, int substeps, int step_limit) {
    SnapHeader hd = SnapHeader();
    hd.magic = SNAP_MAGIC; hd.version = SNAP_VERSION; hd.n_envs = n_envs; hd.task_id = task_id; hd.substeps = substeps; hd.step_limit = step_limit;
    hd.root_f = SNAP_ROOT_F; hd.leg_f = SNAP_LEG_F;
    return hd;
}
// why a blob cannot be restored onto a handle of `task_id`, or NULL when it can (the env counts are the caller's to compare)
inline const char* snap_check_header(const SnapHeader& hd, long long blob_bytes, int task_id) {
    if (hd.magic != SNAP_MAGIC) return "not a jitterbug snapshot (wrong magic)";
    if (hd.version != SNAP_VERSION) return "snapshot layout version not supported";
    if (hd.root_f != SNAP_ROOT_F || hd.leg_f != SNAP_LEG_F) return "snapshot field counts differ from this library's state layout";
    if (hd.n_envs < 1 || blob_bytes != snap_blob_bytes(hd.n_envs)) return "blob size does not match the header";
    if (hd.task_id != task_id) return "snapshot of another task (the target's meaning differs by task)";
    return nullptr;
}
// first j with map[j] outside [0, n_src), or -1 when every entry is valid (the host form refuses such a map before anything is launched)
inline int snap_first_bad_index(const int32_t* map, int n, int n_src) {
    for (int j = 0; j < n; j++) if (map[j] < 0 || map[j] >= n_src) return j;
    return -1;
}

#if defined(__HIPCC__)
// snapshot, restore and fork in ONE launch: one thread per destination word (grid-stride), stores coalesced; a map that is constant
// over a group of envs makes the gathered loads broadcasts
__global__ __launch_bounds__(256) void jb_fork_kernel(SnapView dst, SnapView src, const int* __restrict__ map) {
    const long long total = (long long)SNAP_WORDS * dst.n, stride = (long long)gridDim.x * 256;
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < total; w += stride) fork_word(dst, src, map, w);
}
// one thread per env; row k of rewards / done flags is read coalesced across the envs
__global__ __launch_bounds__(256) void jb_return_kernel(const float* __restrict__ rew, const unsigned char* __restrict__ done, int K, int N, float gamma,
                                                        float* __restrict__ returns, int* __restrict__ alive) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= N) return;
    int n_alive;
    returns[env] = discounted_return(rew, done, K, N, env, gamma, &n_alive);
    if (alive) alive[env] = n_alive;
}
#endif

}  // namespace jb

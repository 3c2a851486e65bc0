// jb_api.hip — kernels and host side of the C ABI declared in include/jitterbug_hip.h.
//
// Layout in HBM (all fp32 unless noted), N environments, 4 lanes per environment:
//   root [ROOT_F][N]      root pose/velocity, motor angle/rate/turns, warm-start accelerations, target
//   leg  [LEG_F][4N]      per-leg hinge angles/rates and warm-start accelerations (lane-private, fully coalesced)
//   lane_model [T][LM_TABLE]      packed constant tables (jb_sim.hpp LM_INV; T = 1 shared, or N per-env)
//   step_count[N] (i32), episode[N] (u32)
// One launch of jb_step_kernel advances every env by one control step (cfg.substeps physics substeps),
// then computes reward, done, optional in-kernel episode reset, and the observation row.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/jitterbug_hip.h"
#include "jb_default_params.h"
#include "jb_device_guard.hpp"
#include "jb_forward.hpp"
#include "jb_contacts.hpp"
#include "jb_model_build.hpp"
#include "jb_model_compile.hpp"
#include "jb_nominal_spec.h"
#include "jb_owned.hpp"
#include "jb_readout.hpp"
#include "jb_inertia.hpp"
#include "jb_evaluate.hpp"
#include "jb_sim.hpp"
#include "jb_snapshot.hpp"
#include "jb_step.hpp"
#include "jb_task.hpp"
#include "jb_variant.hpp"
#include "jb_witness.hpp"

using namespace jb;

#ifndef JB_DEFAULT_MAX_NEWTON
#define JB_DEFAULT_MAX_NEWTON 12      // checks of the active set after which a substep's contact problem goes to the line-searched solve (jb_sim.hpp newton_phase)
#endif

namespace {

enum RootF : int { RF_P = 0, RF_Q = 3, RF_V = 7, RF_W = 10, RF_PHI = 13, RF_PHID = 14, RF_TURNS = 15, RF_WA = 16, RF_WL = 19, RF_WM = 22, RF_FAIL = 23, RF_TGT = 24, RF_LO = 27 /*5: low-order words of z and the quaternion*/, ROOT_F = 32 };
enum LegF : int { LF_TH1 = 0, LF_TH2 = 1, LF_THD1 = 2, LF_THD2 = 3, LF_WJ0 = 4, LF_WJ1 = 5, LEG_F = 6 };
static_assert(ROOT_F == SNAP_ROOT_F && LEG_F == SNAP_LEG_F, "jb_snapshot.hpp copies exactly the state blocks declared here");
static_assert(RO_RF_P == RF_P && RO_RF_Q == RF_Q && RO_RF_V == RF_V && RO_RF_W == RF_W && RO_RF_PHI == RF_PHI && RO_RF_PHID == RF_PHID && RO_RF_TGT == RF_TGT && RO_RF_LO == RF_LO &&
              RO_LF_TH1 == LF_TH1 && RO_LF_TH2 == LF_TH2 && RO_LF_THD1 == LF_THD1 && RO_LF_THD2 == LF_THD2, "jb_readout.hpp reads exactly the state fields declared here");
static_assert(RO_NFRAME == JB_NFRAME, "the header promises this many frames");
static_assert(FW_RF_TURNS == RF_TURNS && FW_RF_WA == RF_WA && FW_RF_WL == RF_WL && FW_RF_WM == RF_WM && FW_LF_WJ0 == LF_WJ0 && FW_LF_WJ1 == LF_WJ1, "jb_forward.hpp names exactly the state fields declared here");

struct KArgs {
    int n, task, substeps, step_limit, auto_reset, contacts, max_newton, random_pose, per_env_model;
    int epw;       // environments per wave (= per 64-thread workgroup) of the step kernel
    int rank_one;      // 0: diagnostic, no rank-one Newton passes (jb_config.flags & JB_FLAG_NO_RANK_ONE)
    int spread;        // 0: diagnostic, no spread sweeps (JB_FLAG_NO_SPREAD)
    int lean;          // 1: the LEAN kernel variant (two waves per SIMD; jb_config.flags & JB_FLAG_LEAN)
    int pair;          // 1: the PAIR kernel variant (geom-geom contact mass ellipsoid / upper-leg cylinders; see JB_FLAG_PAIR)
    int packed_rows;   // step kernel output: 0 = obs[N,D] + reward[N] + done[N]; 1 = one float row [obs(D) | reward | done] per env
    unsigned long long seed, env_offset;
    float* root; float* leg; const float* lane_model;
    int* step_count; unsigned* episode;
    float* ovc_buf;    // LEAN variant: per wave, the candidates of the live slots beyond the row cache (global memory: the variant's 20 KB of LDS have no room)
    unsigned long long* wave_stats;   // diagnostic builds (-DJB_WAVE_STATS): [n_waves][4] = cycles, rare-path substeps, Newton sweeps, contact substeps
    float* capture; unsigned* capture_count;      // diagnostic builds (-DJB_CAPTURE): SimOpts::capture
    unsigned long long* resolve_count;   // [1]: wave-substeps whose contact solve ran a second time with the exact line search (jb_sim.hpp newton_phase), since jb_create
};

// What one launch of a step kernel reads and writes besides the state: K control steps in ONE launch (jb_step_many_device; K = 1 is the
// ordinary step - the same kernel, hence the same machine code and the same bits).  A wave owns its environments for all K steps:
// state, step counter, episode and target stay in registers (LEAN: LDS) between the control steps, and no wave waits for another.
struct StepIO {
    int n_steps;                   // K >= 1
    int use_policy;                // 1: the action of every step is the handle's heuristic policy, evaluated in the kernel on the observation the lanes just produced
    const float* actions;          // use_policy = 0: action tape [K, N] (step k reads row k)
    const float* obs_in;           // use_policy = 1, nullable: [N, D] current observation rows for step 0 (NULL: observed from the state in the kernel)
    float* obs_out;                // nullable: obs [.., N, D], or packed rows [.., N, D+2] when KArgs::packed_rows
    float* reward_out;             // nullable [.., N]   (not packed rows)
    unsigned char* done_out;       // nullable [.., N]   (not packed rows)
    int every_step;                // bit 0 / 1 / 2: obs (rows) / reward / done blocks are written for EVERY step ([K, ...] buffers); clear: only the last step's
    PolicyParams<float> pp;
    unsigned long long* wave_clock;      // nullable [n_waves]: how long each wave lived in this launch (s_memrealtime ticks, 100 MHz): the imbalance a fused rollout removes
    const int* wave_order;               // nullable [n_waves]: workgroup b steps wave wave_order[b] - the waves of the PREVIOUS launch, longest first (jb_wave_order_kernel)
};

// Stage the packed constant table(s) of this workgroup (one wave = a.epw envs) into LDS: one LM_TABLE copy for a
// shared model, epw copies for per-env models.  Called by all 64 threads before the idle quads retire.
// aux_grp: -1 = no aux bodies in this kernel; otherwise the caller's lane group (groups 2 and 3 are the aux lanes: SimOpts::aux)
template <bool SPLIT = false>
__device__ __forceinline__ void stage_model(const KArgs& a, float* lds, int lblock, int quad, int leg, LaneModel<float>& m, bool lean = false, bool pair = true, int aux_grp = -1) {
    m.c.lean = lean;
    m.c.split = false;
    const int tsz = pair ? LM_TABLE : LM_TABLE_BASE, gsz = LM_TABLE;      // staged prefix / table pitch in global memory
    if (SPLIT) {
        // split mode (jb_sim.hpp LaneConsts): per env the resident block only - the lane-invariant prefix, the pair's ellipsoid (lane 0's copy)
        // and the five per-lane entries read after phase A; phase A's per-lane entries are re-staged every substep (restage_overlay)
        const int env0 = lblock * a.epw, rsz = LM_SPLIT_RES;
        for (int i = threadIdx.x; i < rsz * a.epw; i += blockDim.x) {
            int e = env0 + i / rsz;
            if (e >= a.n) e = a.n - 1;
            const int k = i % rsz;
            int src = k;
            if (k >= LM_INV + 15) { const int r = (k - LM_INV - 15) >> 2, l = (k - LM_INV - 15) & 3; src = LM_INV + 4 * (lm_split_res_entry(r) - LM_INV) + l; }
            else if (k >= LM_INV) src = LM_INV + 4 * (LM_PE_C + (k - LM_INV) - LM_INV);
            lds[i] = a.lane_model[(size_t)e * gsz + src];
        }
        m.c.inv = lds + quad * rsz;
        m.c.tab = m.c.inv + LM_INV + 15 + leg;
        m.c.split = true;
        const int env = lblock * a.epw + quad;
        m.c.cold = a.lane_model + (size_t)(env < a.n ? env : a.n - 1) * gsz + LM_INV + leg;
        // overlay: scratch entries [SC_SYS, SC_SYS + LM_SPLIT_OVL) of the main lanes (the scratch precedes the resident block in LDS)
        float* const scratch0 = lds - (size_t)SC_COUNT_LEAN_PAIR * LM_SPLIT_STRIDE;
        const int l16 = threadIdx.x % LM_SPLIT_STRIDE, j_sub = threadIdx.x / LM_SPLIT_STRIDE;
        m.c.ovl = scratch0 + SC_SYS * LM_SPLIT_STRIDE + l16;
        int e_src = lblock * a.epw + (l16 >> 2);
        if (e_src >= a.n) e_src = a.n - 1;
        m.c.ovl_src = a.lane_model + (size_t)e_src * gsz + LM_INV + (l16 & 3) + 4 * j_sub;
        m.c.ovl_dst = scratch0 + SC_SYS * LM_SPLIT_STRIDE + threadIdx.x;
        __syncthreads();
        restage_overlay(m.c);             // (preload below reads the per-level weights from it)
        __syncthreads();
    } else if (a.per_env_model) {
        const int env0 = lblock * a.epw;
        for (int i = threadIdx.x; i < tsz * a.epw; i += blockDim.x) {
            int e = env0 + i / tsz;
            if (e >= a.n) e = a.n - 1;
            lds[i] = a.lane_model[(size_t)e * gsz + (i % tsz)];
        }
        if (aux_grp >= 0)          // one aux block per env behind the tables (jb_sim.hpp build_aux_block)
            for (int k = threadIdx.x; k < LM_AUX * a.epw; k += blockDim.x) {
                int e = env0 + k / LM_AUX;
                if (e >= a.n) e = a.n - 1;
                const int kk = k % LM_AUX;
                lds[tsz * a.epw + k] = aux_entry<float>(a.lane_model + (size_t)e * gsz, LM_INV + (kk >> 2), kk & 3);
            }
        __syncthreads();
        m.c.inv = lds + quad * tsz;
        if (aux_grp >= 2) { m.c.tab_rare = m.c.inv + LM_INV + leg; m.c.tab = lds + tsz * a.epw + quad * LM_AUX + leg; }
    } else {
        for (int i = threadIdx.x; i < tsz; i += blockDim.x) lds[i] = a.lane_model[i];
        if (aux_grp >= 0)          // the aux block behind the table (jb_sim.hpp build_aux_block): the motor body and the root body as two "legs"
            for (int k = threadIdx.x; k < LM_AUX; k += blockDim.x) lds[tsz + k] = aux_entry<float>(a.lane_model, LM_INV + (k >> 2), k & 3);
        __syncthreads();
        m.c.inv = lds;
    }
    if (!SPLIT && !(a.per_env_model && aux_grp >= 2)) m.c.tab = m.c.inv + LM_INV + leg;
    if (!SPLIT && !a.per_env_model && aux_grp >= 2) { m.c.tab_rare = m.c.tab; m.c.tab = lds + tsz + leg; }      // an aux lane: hot per-lane entries from the aux block, the rest from the leg it mirrors
    m.c.preload();
}
__device__ __forceinline__ void load_state(const KArgs& a, int env, int lane, LaneState<float>& s) {
    const float* r = a.root + env;
    const int N = a.n;
    s.px = r[(RF_P + 0) * N]; s.py = r[(RF_P + 1) * N]; s.pz = r[(RF_P + 2) * N];
    s.qw = r[(RF_Q + 0) * N]; s.qx = r[(RF_Q + 1) * N]; s.qy = r[(RF_Q + 2) * N]; s.qz = r[(RF_Q + 3) * N];
    s.vx = r[(RF_V + 0) * N]; s.vy = r[(RF_V + 1) * N]; s.vz = r[(RF_V + 2) * N];
    s.wx = r[(RF_W + 0) * N]; s.wy = r[(RF_W + 1) * N]; s.wz = r[(RF_W + 2) * N];
    s.phi = r[RF_PHI * N]; s.phid = r[RF_PHID * N]; s.turns = r[RF_TURNS * N];
#pragma unroll
    for (int i = 0; i < 3; i++) { s.wa[i] = r[(RF_WA + i) * N]; s.wl[i] = r[(RF_WL + i) * N]; }
    s.wm = r[RF_WM * N]; s.fail = r[RF_FAIL * N];
    s.pz_lo = r[(RF_LO + 0) * N]; s.qw_lo = r[(RF_LO + 1) * N]; s.qx_lo = r[(RF_LO + 2) * N]; s.qy_lo = r[(RF_LO + 3) * N]; s.qz_lo = r[(RF_LO + 4) * N];
    const float* l = a.leg + lane;
    const int L = 4 * N;
    s.th1 = l[LF_TH1 * L]; s.th2 = l[LF_TH2 * L]; s.thd1 = l[LF_THD1 * L]; s.thd2 = l[LF_THD2 * L]; s.wj[0] = l[LF_WJ0 * L]; s.wj[1] = l[LF_WJ1 * L];
}
__device__ __forceinline__ void store_state(const KArgs& a, int env, int lane, int leg, const LaneState<float>& s) {
    const int N = a.n, L = 4 * N;
    float* l = a.leg + lane;
    l[LF_TH1 * L] = s.th1; l[LF_TH2 * L] = s.th2; l[LF_THD1 * L] = s.thd1; l[LF_THD2 * L] = s.thd2; l[LF_WJ0 * L] = s.wj[0]; l[LF_WJ1 * L] = s.wj[1];
    // the replicated root block: each of the 4 lanes writes a quarter of the fields
    float* r = a.root + env;
    const float vals[24] = {s.px, s.py, s.pz, s.qw, s.qx, s.qy, s.qz, s.vx, s.vy, s.vz, s.wx, s.wy, s.wz, s.phi, s.phid, s.turns,
                            s.wa[0], s.wa[1], s.wa[2], s.wl[0], s.wl[1], s.wl[2], s.wm, s.fail};
#pragma unroll
    for (int f = 0; f < 24; f++) if ((f & 3) == leg) r[f * N] = vals[f];
    const float los[5] = {s.pz_lo, s.qw_lo, s.qx_lo, s.qy_lo, s.qz_lo};
#pragma unroll
    for (int f = 0; f < 5; f++) if ((f & 3) == leg) r[(RF_LO + f) * N] = los[f];
}
__device__ __forceinline__ void core_from_state(const LaneState<float>& s, const float (&c0)[3], const float (&tgt)[3], EnvCore<float>& e) {
    e.cx = c0[0]; e.cy = c0[1]; e.cz = c0[2];
    e.px = s.px; e.py = s.py; e.pz = s.pz; e.qw = s.qw; e.qx = s.qx; e.qy = s.qy; e.qz = s.qz;
    e.vx = s.vx; e.vy = s.vy; e.vz = s.vz; e.wx = s.wx; e.wy = s.wy; e.wz = s.wz; e.phi = s.phi; e.phid = s.phid;
    e.tx = tgt[0]; e.ty = tgt[1]; e.tpsi = tgt[2];
}
__device__ __forceinline__ void core_from_state(const KArgs& a, int env, const LaneState<float>& s, const float (&c0)[3], EnvCore<float>& e) {
    const float tgt[3] = {a.root[(RF_TGT + 0) * a.n + env], a.root[(RF_TGT + 1) * a.n + env], a.root[(RF_TGT + 2) * a.n + env]};
    core_from_state(s, c0, tgt, e);
}
__device__ __forceinline__ void state_from_reset(const EnvCore<float>& e, LaneState<float>& s) {
    s.px = e.px; s.py = e.py; s.pz = e.pz; s.qw = e.qw; s.qx = e.qx; s.qy = e.qy; s.qz = e.qz;
    s.pz_lo = s.qw_lo = s.qx_lo = s.qy_lo = s.qz_lo = 0.f;
    s.vx = s.vy = s.vz = s.wx = s.wy = s.wz = 0.f; s.phi = 0.f; s.phid = 0.f; s.turns = 0.f;
    s.th1 = s.th2 = s.thd1 = s.thd2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; i++) { s.wa[i] = 0.f; s.wl[i] = 0.f; }
    s.wj[0] = s.wj[1] = 0.f; s.wm = 0.f;
}
__device__ __forceinline__ void write_obs(const KArgs& a, int env, int leg, const EnvCore<float>& e, float target_z, float* obs_out, int row_stride = 0) {
    if (!obs_out) return;
    float obs[19];
    observe<float>(a.task, e, target_z, obs, 1);
    const int D = obs_dim(a.task);
    float* row = obs_out + (size_t)env * (row_stride ? row_stride : D);
#pragma unroll
    for (int j = 0; j < 19; j++) if ((j & 3) == leg && j < D) row[j] = obs[j];
}
__device__ __forceinline__ void store_target(const KArgs& a, int env, const EnvCore<float>& e) {
    a.root[(RF_TGT + 0) * a.n + env] = e.tx; a.root[(RF_TGT + 1) * a.n + env] = e.ty; a.root[(RF_TGT + 2) * a.n + env] = e.tpsi;
}

// ---------------------------------------------------------------------------------------------- step
// The step kernels' arguments (KArgs, StepIO) live in the kernarg segment.  What the control-step epilogue needs of them (output
// pointers, task options, RNG keys: ~60 scalar registers) must not stay in scalar registers across the 50 substeps - the substep loop
// needs them all, and what does not fit is spilled to VGPR lanes and read back with v_readlane inside the hot loop.  The epilogue
// therefore reads its arguments where it uses them, through a pointer to the kernarg segment that the optimiser cannot see through
// (so the loads cannot be hoisted above the substep loop): a handful of s_load per control step.
typedef const __attribute__((address_space(4))) KArgs* KArgsC;
typedef const __attribute__((address_space(4))) StepIO* StepIOC;
// (AMDGPU kernarg ABI: the explicit arguments lie in declaration order, each at its natural alignment - KArgs at 0, StepIO behind it)
constexpr unsigned STEPIO_KERNARG_OFFSET = (unsigned)((sizeof(KArgs) + alignof(StepIO) - 1) / alignof(StepIO) * alignof(StepIO));
static_assert(alignof(KArgs) == 8 && alignof(StepIO) == 8 && std::is_trivially_copyable<KArgs>::value && std::is_trivially_copyable<StepIO>::value, "kernel arguments are plain data with pointer alignment");
__device__ __forceinline__ const __attribute__((address_space(4))) char* kernarg_base() {
    const __attribute__((address_space(4))) char* p = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
// EPW (envs per wave) is a template parameter so that the scratch stride is a compile-time constant and every LDS access
// of the substep uses an immediate offset instead of integer address arithmetic.
template <int EPW, bool LEAN, bool PAIR = false>
__device__ __forceinline__ void step_body(KArgs a, StepIO io) {
    // one wave per workgroup; quad q (4 lanes) of the wave owns env blockIdx*epw + q.  Quads beyond epw (a small batch is
    // spread over all SIMDs with partially filled waves) and beyond the batch retire at once: DPP quad sums and the
    // wave ballots only ever involve complete, active quads.
    extern __shared__ float lds[];           // [SC_COUNT][4*EPW] per-lane scratch, then the lane constant table(s)
    // Lanes 0 .. 4*EPW-1 are the MAIN lanes (quad q = env q of this wave, lane = leg).  A wave with fewer than 16 envs uses
    // its spare lanes as NGRP-1 helper groups: helper lane L + g*4*EPW mirrors main lane L (same env, leg, scratch and
    // constant-table addresses) and takes a share of the live contact slots in every Newton pass (jb_sim.hpp, SlotPlan).
    constexpr StepLayout LAY = step_layout(EPW, LEAN, PAIR);      // jb_variant.hpp: the one description of this variant
    constexpr int MAIN = LAY.main_lanes;
    constexpr int NGRP = LAY.groups;
    static_assert(EPW == 1 || EPW == 2 || EPW == 4 || EPW == 8, "envs per wave");
    const int lane_in_grp = threadIdx.x % MAIN, grp = threadIdx.x / MAIN;
    const int quad = lane_in_grp >> 2, leg = threadIdx.x & 3;
    // XCD-aware workgroup -> env-range map: hardware deals workgroups round-robin over the 8 XCDs (b and b+8 share one),
    // so give XCD x one contiguous range of envs; then every 128-byte line of the SoA state arrays is touched by a single
    // XCD's L2 instead of all eight (placement is a speed/traffic matter only, never correctness).
    const int nb = (int)gridDim.x, b = (int)blockIdx.x, xcd = b & 7, per = nb >> 3, rem = nb & 7;
    // More waves than the device holds at once: the hardware hands out workgroups in index order, so the order decides which waves share
    // a SIMD's time.  Longest-first by the previous launch's measured wave times (a robot that has tipped over, or whose mass rubs a leg,
    // stays slow) keeps the slow waves out of the last round; which workgroup steps which envs never shows in the results.
    const int lblock = io.wave_order ? io.wave_order[b] : xcd * per + (xcd < rem ? xcd : rem) + (b >> 3);
    const int env = lblock * EPW + quad;
    const unsigned long long clock0 = __builtin_amdgcn_s_memrealtime();
    LaneModel<float> m;
    constexpr int SCN = LAY.scratch_floats;      // floats of per-lane scratch
    // AUX bodies (jb_sim.hpp SimOpts::aux): the ordinary kernel with four lane groups and a shared model - groups 2 and 3 run phase A on the
    // motor body and the root body's own mass instead of idling while every leg lane repeats that work
    constexpr bool AUX = LAY.aux;
    constexpr bool aux_on = AUX;
    stage_model<LAY.split_tables>(a, lds + SCN * MAIN, lblock, quad, leg, m, LEAN, LAY.pair_entries, aux_on ? grp : -1);      // (LEAN + PAIR is only launched with one model per env: split tables)
    if (grp >= NGRP || env >= a.n) return;       // whole quads (and their mirrors in every group) retire together
    const int lane = env * 4 + leg;
    LaneScratch<float> scr;
    scr.p = lds + lane_in_grp;
    scr.stride = MAIN;
    scr.grp = grp; scr.ngrp = NGRP; scr.gstride = MAIN;
    // (LEAN: per wave a block in global memory - the overflow candidates, then the second pair contact's frame: rare paths both)
    static_assert(LAY.lean == LEAN && LAY.red_lds == !LEAN && (LAY.ovc_floats != 0) == LEAN, "the LEAN layout: no reduction hand-over, overflow block in global memory");
    if (LEAN) { scr.ovc = a.ovc_buf + (size_t)lblock * (LAY.ovc_floats * MAIN) + lane_in_grp; scr.pd2 = LAY.pd2; scr.red_lds = LAY.red_lds; }
    else { scr.ovc = lds + SC_OVC * MAIN + lane_in_grp; scr.pd2 = LAY.pd2; scr.red_lds = LAY.red_lds; }
    scr.ovc_stride = MAIN;
    scr.pd = LAY.pd;
    scr.stage_major = LAY.stage_major; scr.term_major = LAY.term_major;
    scr.aux_lane = aux_on && grp >= 2;
#ifdef JB_WAVE_STATS
    const unsigned long long t_start = __builtin_amdgcn_s_memtime();
#endif
    LaneState<float> s;
    constexpr bool OFFLOAD = LAY.offload;         // lane group 1 replicates the main lanes (jb_sim.hpp SimOpts::offload)
    // the lanes that hold an env's state: the main lanes, their replica and the aux lanes.  All run everything below that changes the state
    // (substeps, failure flag, episode reset) with the very same instructions; only the main lanes write to memory.
    const bool rep = grp == 0 || (OFFLOAD && grp == 1) || scr.aux_lane;
    if (rep) load_state(a, env, lane, s);
    else {
        s.px = s.py = s.pz = 0.f; s.qw = 1.f; s.qx = s.qy = s.qz = 0.f; s.vx = s.vy = s.vz = s.wx = s.wy = s.wz = 0.f;
        s.pz_lo = s.qw_lo = s.qx_lo = s.qy_lo = s.qz_lo = 0.f;
        s.phi = s.phid = s.turns = 0.f; s.th1 = s.th2 = s.thd1 = s.thd2 = 0.f;
        for (int i = 0; i < 3; i++) { s.wa[i] = 0.f; s.wl[i] = 0.f; }
        s.wj[0] = s.wj[1] = 0.f; s.wm = 0.f; s.fail = 0.f;
    }
#ifdef JB_WAVE_STATS
    s.st_xtra = 0.f; s.st_sweeps = 0.f; s.st_contact = 0.f; s.st_slots = 0.f; s.st_fast = 0.f; s.st_checks = 0.f;
#endif
    SimOpts o; o.contacts = a.contacts; o.max_newton = a.max_newton; o.implicit_damp = 1; o.rank_one = a.rank_one; o.lean = LEAN ? 1 : 0; o.offload = OFFLOAD ? 1 : 0; o.spread = a.spread; o.prof = nullptr; o.hist = nullptr;
    o.aux = aux_on ? 1 : 0; o.fuse_rows = LAY.fused_row_build ? 1 : 0; o.every_lane_update = LAY.every_lane_update ? 1 : 0; o.scalar_votes = LAY.scalar_votes ? 1 : 0;
#ifdef JB_CAPTURE
    o.capture = a.capture; o.capture_count = a.capture_count;
#endif
#ifdef JB_WAVE_STATS
    const unsigned long long rt_start = __builtin_amdgcn_s_memrealtime();
    unsigned long long prof_local[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // accumulated in registers, written once at the end
    o.prof = prof_local;
    o.hist = a.wave_stats ? a.wave_stats + (size_t)16 * a.n + (size_t)64 * lblock : nullptr;
#endif
    if (OFFLOAD && grp == 0) {
#pragma unroll
        for (int i = 0; i < 56; i++) scr.st(SC_ZERO + i, 0.f);
    }
    // per-env bookkeeping that a K-step launch carries in registers: step counter, episode number, target
    EpisodeRegs<float> er;
    er.step_count = a.step_count[env];
    er.episode = a.episode[env];
    er.tgt[0] = a.root[(RF_TGT + 0) * a.n + env]; er.tgt[1] = a.root[(RF_TGT + 1) * a.n + env]; er.tgt[2] = a.root[(RF_TGT + 2) * a.n + env];
    const int n_substeps = a.substeps;
    float ctrl_next = 0.f;           // use_policy: the action of the NEXT step, computed right after the observation it reads
    if (io.use_policy && rep) {      // the observation the first action is computed from: the caller's row, or the state observed here
        const int D = obs_dim(a.task);
        float obs0[19];
#pragma unroll
        for (int j = 0; j < 19; j++) obs0[j] = 0.f;
        if (io.obs_in) {
#pragma unroll
            for (int j = 0; j < 19; j++) if (j < D) obs0[j] = io.obs_in[(size_t)env * D + j];
        } else {
            EnvCore<float> e0;
            core_from_lane_state<float>(m, s, er.tgt, e0);
            observe<float>(a.task, e0, m.c[LM_TARGET_Z], obs0, 1);
        }
        ctrl_next = heuristic_policy<float>(a.task, obs0, 1, io.pp);
    }
    // (from here on the arguments are read through kernarg_base(): see above)
    int k = 0;
#pragma unroll 1
    for (;;) {
        float ctrl = ctrl_next;
        {
            const auto kb = kernarg_base();
            const KArgsC ka = (KArgsC)kb;
            const StepIOC ic = (StepIOC)(kb + STEPIO_KERNARG_OFFSET);
            if (rep && !ic->use_policy) ctrl = ic->actions[(size_t)k * ka->n + env];
        }
        if (rep) normalise_state(s);          // mj_kinematics normalises the free-joint quaternion; phase C keeps it normalised from here on
        if (PAIR && rep) scr.st(scr.pd + 11, 0.f);      // the narrow phase starts cold in every control step (its warm start is not simulator state)
        if (LEAN && grp == 0) state_store(scr, s);                   // LEAN: the state lives in the scratch between substeps
#pragma unroll 1
        for (int i = 0; i < n_substeps; i++) {
            if (__builtin_expect(substep<float, PAIR>(m, scr, s, ctrl, o), false)) {      // rare (a few substeps in ten million): counted for jb_solver_stats
                if (threadIdx.x == 0) atomicAdd(((KArgsC)kernarg_base())->resolve_count, 1ull);
            }
        }
        const auto kb = kernarg_base();
        const KArgsC ka = (KArgsC)kb;
        const StepIOC ic = (StepIOC)(kb + STEPIO_KERNARG_OFFSET);
        const bool last = k == ic->n_steps - 1;
        k++;
        if (!rep) { if (last) break; continue; }      // helper lanes only take part in the substeps
        if (LEAN) state_load(scr, s);
        const int task = ka->task, N = ka->n, D = obs_dim(task), packed = ka->packed_rows, W = packed ? D + 2 : D;
        TaskOpts topt;
        topt.task = task; topt.step_limit = ka->step_limit; topt.auto_reset = ka->auto_reset; topt.random_pose = ka->random_pose;
        topt.seed = ka->seed; topt.env_global = ka->env_offset + (unsigned long long)env;
        float obs[19], rew;
        bool done;
        control_step_tail<float>(topt, m, s, er, obs, rew, done);          // jb_step.hpp: failure flag, reward, time limit, in-place reset, observation
        if (ic->use_policy) {
            PolicyParams<float> pp;
            pp.kick_angle = ic->pp.kick_angle; pp.speed = ic->pp.speed; pp.angle_threshold = ic->pp.angle_threshold;
            ctrl_next = heuristic_policy<float>(task, obs, 1, pp);
        }
        if (grp == 0) {                       // the replica holds the new state and the next action too; only the main lanes write
            const int every = ic->every_step, kk = k - 1;
            float* const obs_out = ic->obs_out;
            if (obs_out && (last || (every & 1))) {
                float* row = obs_out + ((every & 1) ? (size_t)kk * (size_t)N * W : (size_t)0) + (size_t)env * W;
#pragma unroll
                for (int j = 0; j < 19; j++) if ((j & 3) == leg && j < D) row[j] = obs[j];
                if (packed && leg == 0) { row[D] = rew; row[D + 1] = done ? 1.f : 0.f; }
            }
            if (leg == 0 && !packed) {
                float* const reward_out = ic->reward_out;
                unsigned char* const done_out = ic->done_out;
                if (reward_out && (last || (every & 2))) reward_out[((every & 2) ? (size_t)kk * (size_t)N : (size_t)0) + env] = rew;
                if (done_out && (last || (every & 4))) done_out[((every & 4) ? (size_t)kk * (size_t)N : (size_t)0) + env] = done ? 1 : 0;
            }
        }
        if (last) break;
    }
    if (grp != 0) return;
    const auto kb = kernarg_base();
    const KArgsC ka = (KArgsC)kb;
    const StepIOC ic = (StepIOC)(kb + STEPIO_KERNARG_OFFSET);
#ifdef JB_WAVE_STATS
    if (threadIdx.x == 0 && a.wave_stats) {
        unsigned long long* ws = a.wave_stats + (size_t)lblock * 16;
        ws[10] = __builtin_amdgcn_s_memrealtime() - rt_start;
        {   // where the wave ran: [63] = workgroup index << 40 | XCC_ID << 32 | HW_ID (se, sh, cu, simd, wave slot) - tools/debug/placement.py
            const unsigned hw = __builtin_amdgcn_s_getreg(63492), xcc = __builtin_amdgcn_s_getreg(63508);
            a.wave_stats[(size_t)16 * a.n + (size_t)64 * lblock + 63] = ((unsigned long long)blockIdx.x << 40) | ((unsigned long long)(xcc & 0xfu) << 32) | hw;
        }
        ws[0] = __builtin_amdgcn_s_memtime() - t_start;
        for (int i = 0; i < 5; i++) ws[4 + i] = prof_local[i]; ws[1] = (unsigned long long)s.st_xtra; ws[2] = (unsigned long long)s.st_sweeps; ws[3] = (unsigned long long)s.st_contact; ws[11] = (unsigned long long)s.st_slots; ws[15] = (unsigned long long)s.st_fast; ws[9] = (unsigned long long)s.st_checks; ws[12] = prof_local[5]; ws[13] = prof_local[6]; ws[14] = prof_local[7];
    }
#endif
    {
        KArgs af;                 // the fields store_state reads
        af.n = ka->n; af.root = ka->root; af.leg = ka->leg;
        // StepLayout::late_env_index: the env index as a value of its own, so that the addresses below are formed HERE.  Left to itself the
        // compiler keeps the 64-bit byte offset of the loads at the kernel's entry alive through every loop for these stores - a register
        // pair that the substep loop with its scalar votes has no room for (one spill at the entry, one reload here).
        int env_out = env;
        if (LAY.late_env_index) asm volatile("" : "+v"(env_out));
        store_state(af, env_out, env_out * 4 + leg, leg, s);
        if (leg == 0) {
            ka->step_count[env_out] = er.step_count;
            ka->episode[env_out] = er.episode;
            af.root[(RF_TGT + 0) * af.n + env_out] = er.tgt[0]; af.root[(RF_TGT + 1) * af.n + env_out] = er.tgt[1]; af.root[(RF_TGT + 2) * af.n + env_out] = er.tgt[2];
        }
    }
    unsigned long long* const wc = ic->wave_clock;
    if (threadIdx.x == 0 && wc) wc[lblock] = __builtin_amdgcn_s_memrealtime() - clock0;
}

template <int EPW>
__global__ __launch_bounds__(64) void jb_step_kernel(KArgs a, StepIO io) {
    step_body<EPW, false>(a, io);
}
// The LEAN variant: the same substep with the register budget of TWO waves per SIMD (256 registers per lane).  Model constants are read
// from LDS where they are used, and the lane state, the joint-space system and the kept factorisation are parked in the lane's
// scratch between the phases that use them (jb_sim.hpp SimOpts::lean).  The same algorithm, but NOT the same bits as the one-wave kernel:
// the damping factorisation comes from star_factor<false> instead of the replica group's star_solve stream, and the compiler fuses
// multiply-adds differently in the two instantiations - the results agree to fp32 rounding (on the host, without contraction, they are
// identical).  Every shard of one batch must therefore run the same variant (jitterbug_amd.variants resolves it from the global batch).
// A second resident wave doubles the SIMD's VALU issue rate, which pays when a GPU holds >= 2048 waves.
template <int EPW>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void jb_step_kernel_lean(KArgs a, StepIO io) {
    step_body<EPW, true>(a, io);
}

// The PAIR variant: the same step with the one geom-geom contact randomised models need (jb_sim.hpp pair_narrow / pair_rows_build,
// the shoulder - motor cross term in the star solve).  A separate instantiation so that the nominal model's kernel stays exactly
// the code it was; chosen per handle (launch_step).
template <int EPW>
__global__ __launch_bounds__(64) void jb_step_kernel_pair(KArgs a, StepIO io) {
    step_body<EPW, false, true>(a, io);
}

// LEAN + PAIR: one model per env on the two-waves-per-SIMD kernel (BASELINE configs[4]'s 8192-env shard).  Four 3 KB tables per wave do not
// fit next to the scratch, so only the entries of the common path are staged (LaneConsts split mode): 25 KB per wave, six waves per CU.
template <int EPW>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void jb_step_kernel_lean_pair(KArgs a, StepIO io) {
    step_body<EPW, true, true>(a, io);
}

// ---------------------------------------------------------------------------------------------- forward dynamics (jb_forward.hpp)
// One substep on a COPY of a state, then inverse dynamics on (state, y): accelerations and contact forces without advancing time.  The wave is
// the step kernels' at four envs per wave, one wave per SIMD - step_layout(4, false, PAIR): the same scratch binding, helper / replica / aux
// lane groups, table staging, SC_ZERO initialisation and options as step_body, so the substep runs exactly the instruction stream of that
// step kernel's first substep of a control step.  One layout serves every handle (the pass is off the hot path); PAIR follows the handle's
// KArgs::pair.  A handle that STEPS with a LEAN kernel therefore gets forward results that agree with its own steps to fp32 rounding only
// (the two instantiations fuse multiply-adds differently: see jb_step_kernel_lean above).
// Workgroup b = wave b % waves_per_snap of snapshot b / waves_per_snap: a wave never straddles two snapshots, so stage_model works unchanged.
// A quad past the end of a snapshot repeats its last env (loads stay inside the blocks, every quad of the wave stays complete for the quad
// and wave operations; its rows are never copied out).  The main lanes then reload the untouched input state, run fw_lane and write their rows
// into an LDS image of the block's part of each output array (the scratch is dead by then); the wave copies each present image out as one
// contiguous segment, in 16-byte words where the segment starts on one.  Nothing but the outputs is written.
// What both substep passes are told about their launch (jb_forward_device / jb_contacts_device fill it in prepare_pass).
struct PassArgs {
    SnapView first;              // snapshot 0 (or the handle's blocks)
    long long stride_words;      // distance between consecutive snapshots, in 4-byte words
    int waves_per_snap;          // ceil(N / 4)
    const float* ctrl;           // nullable [n_snaps * N]: the action of every env-state (NULL: 0)
    unsigned char* unconv;       // nullable [n_snaps * N]
};
struct FwArgs {
    PassArgs p;
    float *qacc, *qfrc, *bacc, *motor;      // each nullable
};
constexpr int FW_EPW = 4;
// A pass's wave up to its substep: everything step_body does before the first substep of a control step, on the state of env-state
// (k, env) instead of the handle's.  BOTH pass kernels run this one text, which is what makes the contact pass's solve the forward pass's.
// (It names the dynamic LDS itself: handing the pointer in changes the code of the STEP kernels - DESIGN.md, "module coupling".)
template <bool PAIR>
struct PassWave {
    int grp, quad, leg, k, lblock, env;
    bool rep;                    // this lane group holds the state
    LaneModel<float> m;
    LaneScratch<float> scr;
    LaneState<float> s;
    SnapView v;                  // the snapshot of this wave
    float ctrl;
    SimOpts o;
    __device__ __forceinline__ void begin(const KArgs& a, const PassArgs& f) {
        extern __shared__ float lds[];           // [SC_COUNT][16] per-lane scratch, then the lane constant table(s): step_body's layout
        constexpr StepLayout LAY = step_layout(FW_EPW, false, PAIR);
        constexpr int MAIN = LAY.main_lanes, SCN = LAY.scratch_floats;
        static_assert(LAY.groups * MAIN == 64 && LAY.offload && LAY.red_lds && !LAY.split_tables && LAY.ovc_floats == 0, "the one-wave-per-SIMD layout at four envs per wave fills the wave");
        const int lane_in_grp = threadIdx.x % MAIN;
        grp = threadIdx.x / MAIN; quad = lane_in_grp >> 2; leg = threadIdx.x & 3;
        k = (int)blockIdx.x / f.waves_per_snap; lblock = (int)blockIdx.x - k * f.waves_per_snap;
        stage_model<false>(a, lds + SCN * MAIN, lblock, quad, leg, m, false, LAY.pair_entries, LAY.aux ? grp : -1);      // (a.epw == FW_EPW: prepare_pass)
        env = lblock * FW_EPW + quad;
        if (env >= a.n) env = a.n - 1;
        scr.p = lds + lane_in_grp;
        scr.stride = MAIN;
        scr.grp = grp; scr.ngrp = LAY.groups; scr.gstride = MAIN;
        scr.ovc = lds + SC_OVC * MAIN + lane_in_grp; scr.pd2 = LAY.pd2; scr.red_lds = LAY.red_lds;
        scr.ovc_stride = MAIN;
        scr.pd = LAY.pd;
        scr.stage_major = LAY.stage_major; scr.term_major = LAY.term_major;
        scr.aux_lane = LAY.aux && grp >= 2;
        v = f.first;
        v.root += (long long)k * f.stride_words; v.leg += (long long)k * f.stride_words;
        rep = holds_state(LAY, grp);
        if (rep) {
            KArgs av;                 // the fields load_state reads
            av.n = a.n; av.root = (float*)v.root; av.leg = (float*)v.leg;
            load_state(av, env, env * 4 + leg, s);
        } else helper_lane_state(s);
        s.fail = 0.f;                 // counts this substep alone
#ifdef JB_WAVE_STATS
        s.st_xtra = 0.f; s.st_sweeps = 0.f; s.st_contact = 0.f; s.st_slots = 0.f; s.st_fast = 0.f; s.st_checks = 0.f;
#endif
        o = sim_opts(LAY, a.contacts, a.max_newton, 1, a.rank_one, a.spread);
        if (grp == 0) {
#pragma unroll
            for (int i = 0; i < 56; i++) scr.st(SC_ZERO + i, 0.f);
        }
        ctrl = 0.f;
        if (rep && f.ctrl) ctrl = f.ctrl[(size_t)k * a.n + env];
        if (rep) normalise_state(s);
        if (PAIR && rep) scr.st(scr.pd + 11, 0.f);      // the narrow phase starts cold, as in the first substep of a control step
    }
    // this lane's env-state is a real one (not the repeat that fills a ragged last quad) and the lane speaks for it
    __device__ __forceinline__ bool speaks(const KArgs& a) const { return leg == 0 && lblock * FW_EPW + quad < a.n; }
    __device__ __forceinline__ size_t env_state(const KArgs& a) const { return (size_t)k * a.n + env; }
    // the wave copies the block's LDS image of one output array (len floats per env-state) out as one contiguous segment, if the array is wanted
    __device__ __forceinline__ void store(const KArgs& a, float* arr, const float* image, int len) const {
        if (!arr) return;
        const int left = a.n - lblock * FW_EPW, n_es = left < FW_EPW ? left : FW_EPW;
        float* dst = arr + ((size_t)k * a.n + (size_t)lblock * FW_EPW) * len;
        ro_store_segment(dst, image, n_es * len, (((uintptr_t)dst) & 15u) == 0 ? 1 : 0, (int)threadIdx.x);
    }
};
constexpr int FW_LDS_QACC = 0, FW_LDS_QFRC = FW_LDS_QACC + FW_EPW * FW_NV, FW_LDS_BACC = FW_LDS_QFRC + FW_EPW * FW_NV, FW_LDS_MOTOR = FW_LDS_BACC + FW_EPW * FW_BACC,
              FW_LDS_FLOATS = FW_LDS_MOTOR + FW_EPW * FW_MOTOR;
static_assert(FW_LDS_QFRC % 4 == 0 && FW_LDS_BACC % 4 == 0 && FW_LDS_MOTOR % 4 == 0, "every LDS image starts on a 16-byte word");
static_assert(FW_LDS_FLOATS <= SC_COUNT * 4 * FW_EPW, "the images fit into the (dead) scratch");
template <bool PAIR>
__global__ __launch_bounds__(64) void jb_forward_kernel(KArgs a, FwArgs f) {
    extern __shared__ float lds[];
    PassWave<PAIR> w;
    w.begin(a, f.p);
    (void)substep<float, PAIR>(w.m, w.scr, w.s, w.ctrl, w.o);
    __syncthreads();                                // every lane group is done with the scratch: it becomes the output images
    if (w.grp == 0) {
        const int quad = w.quad, leg = w.leg;
        const FwState<float> st = fw_load<float>(w.v, w.env, leg);
        FwAcc<float> y;
#pragma unroll
        for (int i = 0; i < 3; i++) { y.lin[i] = w.s.wl[i]; y.ang[i] = w.s.wa[i]; }
        y.j1 = w.s.wj[0]; y.j2 = w.s.wj[1]; y.m = w.s.wm;
        FwOut<float> out;
        out.qacc = f.qacc ? lds + FW_LDS_QACC + quad * FW_NV : nullptr;
        out.qfrc = f.qfrc ? lds + FW_LDS_QFRC + quad * FW_NV : nullptr;
        out.bacc = f.bacc ? lds + FW_LDS_BACC + quad * FW_BACC : nullptr;
        out.motor = f.motor ? lds + FW_LDS_MOTOR + quad * FW_MOTOR : nullptr;
        float p[6];
        fw_lane<float>(st, y, w.ctrl, w.m.c.inv, leg, out, p);
        if (out.qfrc) {
#pragma unroll
            for (int i = 0; i < 6; i++) { const float t = quad_sum(p[i]); if (leg == (i & 3)) out.qfrc[i] = t; }
        }
        if (f.p.unconv && w.speaks(a)) f.p.unconv[w.env_state(a)] = w.s.fail > 0.f ? 1 : 0;
    }
    __syncthreads();
    w.store(a, f.qacc, lds + FW_LDS_QACC, FW_NV); w.store(a, f.qfrc, lds + FW_LDS_QFRC, FW_NV);
    w.store(a, f.bacc, lds + FW_LDS_BACC, FW_BACC); w.store(a, f.motor, lds + FW_LDS_MOTOR, FW_MOTOR);
}
// ---------------------------------------------------------------------------------------------- contacts (jb_contacts.hpp)
// The forward pass's wave, launch shape and substep - step_layout(4, false, PAIR), n_snaps x ceil(N / 4) workgroups, a ragged last quad
// repeats its last env - so the solve behind the forces is the one behind jb_forward_kernel's qacc, bit for bit.  The substep is handed a
// SolveTap: the scratch entries it leaves are packed by rank among the wave's live slots.  The scratch is NOT dead afterwards - the rows are read from it - so the
// output images have LDS of their own behind the constant tables (CtArgs::img: 15 KB; 51 KB per wave with one model per env).  They are
// zeroed before the substep; the main lanes then walk the live slots (a wave-uniform loop), every lane evaluates the slot for its leg
// (ct_slot) and a lane that can hold a contact there writes its row, adds a floor row's force to its geom's three words - every geom belongs
// to one lane, no exchange - and counts.  The wave copies each present image out as one contiguous segment.  Nothing but the outputs is written.
struct CtArgs {
    PassArgs p;
    int img;                     // where the images start in the dynamic LDS, in floats (a multiple of 4: behind the scratch and the tables)
    float *contact, *geom_frc; int* ncon;      // each nullable
};
constexpr int CT_LDS_TABLE = 0, CT_LDS_GEOM = CT_LDS_TABLE + FW_EPW * CT_TABLE, CT_LDS_FLOATS = CT_LDS_GEOM + FW_EPW * CT_GEOMF;
static_assert(CT_LDS_GEOM % 4 == 0 && CT_LDS_FLOATS % 4 == 0 && CT_TABLE % 4 == 0 && (FW_EPW * CT_GEOMF) % 4 == 0, "every LDS image starts on a 16-byte word and a full block's segment is whole words");
template <bool PAIR>
__global__ __launch_bounds__(64) void jb_contacts_kernel(KArgs a, CtArgs f) {
    extern __shared__ float lds[];           // PassWave's scratch and tables, then the output images
    float* const img = lds + f.img;
    for (int i = threadIdx.x; i < CT_LDS_FLOATS / 4; i += 64) ((float4*)img)[i] = make_float4(0.f, 0.f, 0.f, 0.f);      // an inactive row is all zeros
    PassWave<PAIR> w;
    w.begin(a, f.p);
    CtTap<float> tap;
    (void)substep<float, PAIR, SolveTap<float>>(w.m, w.scr, w.s, w.ctrl, w.o, tap.tap());
    const unsigned live = tap.live;
    __syncthreads();                                // the solve's last scratch writes, and the zeroed images
    if (w.grp == 0) {
        const int quad = w.quad, leg = w.leg;
        const RoState<float> st = ro_load<float>(w.v, w.env, leg);
        CtPose<float> P;
        P.R = ro_quat2mat(st.q, st.ql); P.px = st.px; P.py = st.py; P.pz = st.pz; P.pz_lo = st.pz_lo;
        const CtY<float> y = ct_y<float>(w.scr, tap);
        float* const rows = f.contact ? img + CT_LDS_TABLE + quad * CT_TABLE : nullptr;
        float* const gfrc = f.geom_frc ? img + CT_LDS_GEOM + quad * CT_GEOMF : nullptr;
        unsigned count = 0u;
#pragma unroll 1
        for (unsigned rest = live; rest; rest &= rest - 1u) {
            const int slot = __builtin_ctz(rest);
            CtRowOut<float> r;
            ct_slot<float, PAIR>(w.m, w.scr, live, slot, P, y, r);
            if (ct_has_row(leg, slot)) {
                if (rows) {
                    float* q = rows + ct_row(leg, slot) * CT_W;
#pragma unroll
                    for (int i = 0; i < CT_W; i++) q[i] = r.v[i];
                }
                if (gfrc && slot < SLOT_THREAD) {
                    float* q = gfrc + 3 * ct_geom(leg, slot);
                    q[0] += r.v[CT_FORCE]; q[1] += r.v[CT_FORCE + 1]; q[2] += r.v[CT_FORCE + 2];
                }
                count += r.on ? 1u : 0u;
            }
        }
        count = quad_sum_u(count);
        if (f.ncon && w.speaks(a)) f.ncon[w.env_state(a)] = (int)count;
        if (f.p.unconv && w.speaks(a)) f.p.unconv[w.env_state(a)] = w.s.fail > 0.f ? 1 : 0;
    }
    __syncthreads();
    w.store(a, f.contact, img + CT_LDS_TABLE, CT_TABLE); w.store(a, f.geom_frc, img + CT_LDS_GEOM, CT_GEOMF);
}

// Self-check of the kernarg-segment reads above, run once per process before the first handle is handed out: a kernel with the step kernels'
// argument list compares what it reads through kernarg_base() with the arguments it received by value.
__global__ void jb_kernarg_probe_kernel(KArgs a, StepIO io, int* ok) {
    const auto kb = kernarg_base();
    const KArgsC ka = (KArgsC)kb;
    const StepIOC ic = (StepIOC)(kb + STEPIO_KERNARG_OFFSET);
    *ok = (ka->n == a.n && ka->seed == a.seed && ka->root == a.root && ka->step_limit == a.step_limit && ic->n_steps == io.n_steps && ic->obs_out == io.obs_out &&
           ic->every_step == io.every_step && ic->wave_clock == io.wave_clock && ic->pp.angle_threshold == io.pp.angle_threshold) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- reset / observe
__global__ __launch_bounds__(64) void jb_reset_kernel(KArgs a, const unsigned char* __restrict__ mask, float* __restrict__ obs_out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    int env = t >> 2, leg = t & 3;
    if (env >= a.n) return;
    const int lane = env * 4 + leg;
    const float* tab = a.lane_model + (a.per_env_model ? (size_t)env * LM_TABLE : 0);
    const float target_z = tab[lm_offset(LM_TARGET_Z, leg)], root_z0 = tab[lm_offset(LM_ROOT_Z0, leg)];
    const float c0[3] = {tab[lm_offset(LM_C0, leg)], tab[lm_offset(LM_C0 + 1, leg)], tab[lm_offset(LM_C0 + 2, leg)]};
    LaneState<float> s;
    EnvCore<float> e;
    e.cx = c0[0]; e.cy = c0[1]; e.cz = c0[2];
    if (!mask || mask[env]) {
        unsigned ep = a.episode[env];
        episode_reset<float>(a.task, a.random_pose, a.seed, a.env_offset + (unsigned long long)env, ep, root_z0, e);
        state_from_reset(e, s);
        s.fail = a.root[RF_FAIL * a.n + env];
        store_state(a, env, lane, leg, s);
        if (leg == 0) { a.episode[env] = ep + 1; a.step_count[env] = 0; store_target(a, env, e); }
    } else {
        load_state(a, env, lane, s);
        core_from_state(a, env, s, c0, e);
    }
    write_obs(a, env, leg, e, target_z, obs_out);
}

__global__ __launch_bounds__(64) void jb_observe_kernel(KArgs a, float* __restrict__ obs_out, float* __restrict__ reward_out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    int env = t >> 2, leg = t & 3;
    if (env >= a.n) return;
    const float* tab = a.lane_model + (a.per_env_model ? (size_t)env * LM_TABLE : 0);
    const float target_z = tab[lm_offset(LM_TARGET_Z, leg)];
    const float c0[3] = {tab[lm_offset(LM_C0, leg)], tab[lm_offset(LM_C0 + 1, leg)], tab[lm_offset(LM_C0 + 2, leg)]};
    LaneState<float> s;
    load_state(a, env, env * 4 + leg, s);
    EnvCore<float> e;
    core_from_state(a, env, s, c0, e);
    write_obs(a, env, leg, e, target_z, obs_out);
    if (leg == 0 && reward_out) reward_out[env] = reward<float>(a.task, e, target_z);
}

// ---------------------------------------------------------------------------------------------- heuristic policies
__global__ void jb_policy_kernel(int n, int task, PolicyParams<float> pp, const float* __restrict__ obs, float* __restrict__ action) {
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n) return;
    action[env] = heuristic_policy<float>(task, obs + (size_t)env * obs_dim(task), 1, pp);
}

// the four reward terms [P, H, V, U] of every env (reference jitterbug.py:840-889), whatever the handle's task
__global__ __launch_bounds__(64) void jb_reward_terms_kernel(KArgs a, float* __restrict__ terms_out) {
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    int env = t >> 2, leg = t & 3;
    if (env >= a.n) return;
    const float* tab = a.lane_model + (a.per_env_model ? (size_t)env * LM_TABLE : 0);
    const float target_z = tab[lm_offset(LM_TARGET_Z, leg)];
    const float c0[3] = {tab[lm_offset(LM_C0, leg)], tab[lm_offset(LM_C0 + 1, leg)], tab[lm_offset(LM_C0 + 2, leg)]};
    LaneState<float> s;
    load_state(a, env, env * 4 + leg, s);
    EnvCore<float> e;
    core_from_state(a, env, s, c0, e);
    float out[4];
    reward_terms<float>(e, target_z, out);
    terms_out[(size_t)env * 4 + leg] = out[leg];
}

// ---------------------------------------------------------------------------------------------- witness for the unsimulated geom pairs
// One thread per env (fp64, private memory: a diagnostic pass, jb_witness.hpp): smallest distance over the geom pairs MuJoCo would test and the
// step kernels do not collide, in the env's current state.  clear_out / pair_out: this pass's result; min_acc / count_acc (nullable): running
// minimum and the number of passes that found a pair interpenetrating (JB_FLAG_PAIR_WITNESS: one pass behind every step launch).
__global__ __launch_bounds__(64) void jb_witness_kernel(KArgs a, float* __restrict__ clear_out, int* __restrict__ pair_out, float* __restrict__ min_acc, unsigned* __restrict__ count_acc) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= a.n) return;
    const float* tab = a.lane_model + (a.per_env_model ? (size_t)env * LM_TABLE : 0);
    const int L = 4 * a.n;
    double th1[4], th2[4];
    for (int l = 0; l < 4; l++) { th1[l] = a.leg[LF_TH1 * L + env * 4 + l]; th2[l] = a.leg[LF_TH2 * L + env * 4 + l]; }
    int pair[2];
    const double d = witness_clearance<float>(tab, th1, th2, (double)a.root[RF_PHI * a.n + env], pair);
    if (clear_out) clear_out[env] = (float)d;
    if (pair_out) { pair_out[2 * env] = pair[0]; pair_out[2 * env + 1] = pair[1]; }
    if (min_acc) min_acc[env] = fminf(min_acc[env], (float)d);
    if (count_acc && !(d > 0.0)) count_acc[env] += 1u;
}

// ---------------------------------------------------------------------------------------------- launch order of the waves
// order[0 .. n) = the waves sorted by their last measured lifetime, longest first (a 1024-bin counting sort: exact order inside a bin does
// not matter).  One workgroup; runs on the handle's stream right after a step launch whenever the batch has more waves than the device
// holds at once.  All-zero clocks (nothing measured yet) give the identity.
// fold_from > 0 (two-waves-per-SIMD kernels whose batch fits the device at once, but only with both wave slots of some SIMDs in use): the
// hardware gives workgroups b and b + fold_from the same SIMD (measured, tools/debug/placement.py: all 1024 SIMDs, index distance 1024),
// so the sorted list is FOLDED: with n <= 2 fold_from waves the 2 fold_from - n longest get a SIMD to themselves, and of the others the
// longest shares its SIMD with the shortest, the second longest with the second shortest.
__global__ __launch_bounds__(1024) void jb_wave_order_kernel(const unsigned long long* __restrict__ clock, int* __restrict__ order, int n, int fold_from) {
    __shared__ unsigned long long s_max[1024];
    __shared__ unsigned s_bin[1024], s_pos[1024];
    const int t = threadIdx.x;
    unsigned long long mx = 0;
    for (int i = t; i < n; i += 1024) mx = clock[i] > mx ? clock[i] : mx;
    s_max[t] = mx; s_bin[t] = 0u;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) { if (t < st) s_max[t] = s_max[t] > s_max[t + st] ? s_max[t] : s_max[t + st]; __syncthreads(); }
    mx = s_max[0];
    if (mx == 0ull) { for (int i = t; i < n; i += 1024) order[i] = i; return; }
    const double scale = 1023.0 / (double)mx;
    for (int i = t; i < n; i += 1024) atomicAdd(&s_bin[1023 - (int)((double)clock[i] * scale)], 1u);      // bin 0 = the longest waves
    __syncthreads();
    if (t == 0) { unsigned acc = 0; for (int k = 0; k < 1024; k++) { s_pos[k] = acc; acc += s_bin[k]; } }
    __syncthreads();
    for (int i = t; i < n; i += 1024) {
        int p = (int)atomicAdd(&s_pos[1023 - (int)((double)clock[i] * scale)], 1u);
        if (fold_from > 0) {      // S = fold_from SIMDs, n <= 2 S waves: the 2 S - n longest run alone, the rest pair longest with shortest
            const int S = fold_from, alone = 2 * S - n;
            p = p < alone ? (n - S) + p : p < S ? p - alone : S + (n - 1 - p);
        }
        order[p] = i;
    }
}

// ---------------------------------------------------------------------------------------------- diagnostics
// Fills LDS with NaN bit patterns (LDS keeps its contents between kernels): a step kernel that reads scratch it has not
// written in the same launch then produces NaNs deterministically instead of depending on what ran before it.
__global__ void jb_poison_lds_kernel(int n_floats, float* sink) {
    extern __shared__ float lds[];
    for (int i = threadIdx.x; i < n_floats; i += blockDim.x) lds[i] = __uint_as_float(0x7FC00000u + (unsigned)(i & 0xFFFF));
    __syncthreads();
    if (sink && lds[(threadIdx.x * 97) % n_floats] == 0.f) sink[0] = 1.f;     // keep the stores alive
}

// ---------------------------------------------------------------------------------------------- observation encoder (tiny dense network per row)
struct EncArgs {
    int n, n_layers, vae, in_dim, out_dim;
    int dims[JB_ENC_MAX_LAYERS + 1], acts[JB_ENC_MAX_LAYERS], woff[JB_ENC_MAX_LAYERS], boff[JB_ENC_MAX_LAYERS];
    const float* params;          // weights then biases
    unsigned long long seed, env_offset;
    unsigned call;
};
__global__ void jb_encode_kernel(EncArgs e, const float* __restrict__ obs, float* __restrict__ out) {
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= e.n) return;
    float a[JB_ENC_MAX_WIDTH], b[JB_ENC_MAX_WIDTH];
    for (int i = 0; i < e.in_dim; i++) a[i] = obs[(size_t)env * e.in_dim + i];
    for (int l = 0; l < e.n_layers; l++) {
        const int din = e.dims[l], dout = e.dims[l + 1];
        const float* W = e.params + e.woff[l];
        const float* bias = e.params + e.boff[l];
        for (int j = 0; j < dout; j++) {
            float t = bias[j];
            for (int i = 0; i < din; i++) t = fmaf(a[i], W[i * dout + j], t);
            b[j] = e.acts[l] == JB_ACT_TANH ? tanhf(t) : e.acts[l] == JB_ACT_RELU ? fmaxf(t, 0.f) : t;
        }
        for (int j = 0; j < dout; j++) a[j] = b[j];
    }
    if (e.vae) {   // code = mean + std * eps, eps ~ N(0,1) by Box-Muller on Philox words
        const int L = e.out_dim;
        for (int j0 = 0; j0 < L; j0 += 4) {
            uint32_t r[4];
            philox4x32(e.seed ^ 0x656E636F64657273ull, e.env_offset + (unsigned long long)env, e.call, (uint32_t)(j0 >> 2), r);
            float u0 = ((float)(r[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u1 = ((float)(r[1] >> 8) + 0.5f) * (1.0f / 16777216.0f);
            float u2 = ((float)(r[2] >> 8) + 0.5f) * (1.0f / 16777216.0f), u3 = ((float)(r[3] >> 8) + 0.5f) * (1.0f / 16777216.0f);
            float ra = sqrtf(-2.f * logf(u0)), rb = sqrtf(-2.f * logf(u2));
            float eps[4] = {ra * cosf(6.2831853f * u1), ra * sinf(6.2831853f * u1), rb * cosf(6.2831853f * u3), rb * sinf(6.2831853f * u3)};
            for (int k = 0; k < 4 && j0 + k < L; k++) out[(size_t)env * L + j0 + k] = a[j0 + k] + a[L + j0 + k] * eps[k];
        }
    } else {
        for (int j = 0; j < e.out_dim; j++) out[(size_t)env * e.out_dim + j] = a[j];
    }
}

// ---------------------------------------------------------------------------------------------- state import / export (fp64 MuJoCo layout)
__global__ void jb_export_kernel(KArgs a, double* __restrict__ qpos, double* __restrict__ qvel, double* __restrict__ target) {
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= a.n) return;
    const int N = a.n, L = 4 * N;
    const float* r = a.root + env;
    if (qpos) {
        double* q = qpos + (size_t)env * 16;
        for (int i = 0; i < 7; i++) q[i] = r[i * N];
        for (int i = 0; i < 5; i++) q[2 + i] += (double)r[(RF_LO + i) * N];          // height and quaternion are held as hi + lo
        for (int l = 0; l < 4; l++) { q[7 + 2 * l] = a.leg[LF_TH1 * L + env * 4 + l]; q[8 + 2 * l] = a.leg[LF_TH2 * L + env * 4 + l]; }
        q[15] = (double)r[RF_PHI * N] + 6.283185307179586 * (double)r[RF_TURNS * N];
    }
    if (qvel) {
        double* v = qvel + (size_t)env * 15;
        for (int i = 0; i < 6; i++) v[i] = r[(RF_V + i) * N];
        for (int l = 0; l < 4; l++) { v[6 + 2 * l] = a.leg[LF_THD1 * L + env * 4 + l]; v[7 + 2 * l] = a.leg[LF_THD2 * L + env * 4 + l]; }
        v[14] = r[RF_PHID * N];
    }
    if (target) for (int i = 0; i < 3; i++) target[(size_t)env * 3 + i] = r[(RF_TGT + i) * N];
}
__global__ void jb_import_kernel(KArgs a, const double* __restrict__ qpos, const double* __restrict__ qvel, const double* __restrict__ target) {
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= a.n) return;
    const int N = a.n, L = 4 * N;
    float* r = a.root + env;
    if (qpos) {
        const double* q = qpos + (size_t)env * 16;
        for (int i = 0; i < 7; i++) r[i * N] = (float)q[i];
        for (int i = 0; i < 5; i++) r[(RF_LO + i) * N] = (float)(q[2 + i] - (double)(float)q[2 + i]);
        for (int l = 0; l < 4; l++) { a.leg[LF_TH1 * L + env * 4 + l] = (float)q[7 + 2 * l]; a.leg[LF_TH2 * L + env * 4 + l] = (float)q[8 + 2 * l]; }
        double k = floor((q[15] + 3.141592653589793) / 6.283185307179586);
        r[RF_PHI * N] = (float)(q[15] - k * 6.283185307179586); r[RF_TURNS * N] = (float)k;
    }
    if (qvel) {
        const double* v = qvel + (size_t)env * 15;
        for (int i = 0; i < 6; i++) r[(RF_V + i) * N] = (float)v[i];
        for (int l = 0; l < 4; l++) { a.leg[LF_THD1 * L + env * 4 + l] = (float)v[6 + 2 * l]; a.leg[LF_THD2 * L + env * 4 + l] = (float)v[7 + 2 * l]; }
        r[RF_PHID * N] = (float)v[14];
    }
    if (target) for (int i = 0; i < 3; i++) r[(RF_TGT + i) * N] = (float)target[(size_t)env * 3 + i];
    // a teacher-forced state has no history: clear the contact-solver warm start
    for (int i = 0; i < 7; i++) r[(RF_WA + i) * N] = 0.f;
    for (int l = 0; l < 4; l++) { a.leg[LF_WJ0 * L + env * 4 + l] = 0.f; a.leg[LF_WJ1 * L + env * 4 + l] = 0.f; }
}

// ---------------------------------------------------------------------------------------------- domain randomisation (one thread per env)
static_assert(AO_COUNT == JB_NOFFSET, "offset vector layout: header and compiler disagree");
struct RndArgs {
    int n, flags, max_attempts;
    unsigned long long seed, env_offset;
    AugSigmas sd;
    double min_mass_clearance;
    const JbNominalSpec* spec;            // nominal model, device memory
    const double* offsets_in;             // [n, AO_COUNT] nullable: use these instead of drawing
    float* tables;                        // [n, LM_TABLE] lane constant tables (the kernel's per-env model)
    double* params_out;                   // [n, JB_NPARAM] nullable
    double* offsets_out;                  // [n, AO_COUNT] nullable
    int* attempts_out;                    // [n] nullable
    int* status;                          // [1]: first failure code (0 = ok)
};
__global__ __launch_bounds__(64) void jb_randomise_kernel(RndArgs a) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= a.n) return;
    JbNominalSpec S;
    double P[JB_NPARAM], off[AO_COUNT];
    int attempt = 0, rc = 0;
    for (;;) {
        if (a.offsets_in) for (int i = 0; i < AO_COUNT; i++) off[i] = a.offsets_in[(size_t)env * AO_COUNT + i];
        else draw_offsets(a.seed, a.env_offset + (unsigned long long)env, (uint32_t)attempt, a.flags, a.sd, off);
        apply_offsets(*a.spec, a.flags, off, S);
        rc = compile_model(S, P);
        attempt++;
        if (rc == 0 && (a.offsets_in || a.min_mass_clearance <= 0.0 || mass_sweep_clear(P, a.min_mass_clearance))) break;
        if (a.offsets_in || attempt >= a.max_attempts) { if (rc == 0) rc = -30; break; }      // -30: no acceptable draw within max_attempts
    }
    if (rc == 0) rc = build_packed_model<float>(P, a.tables + (size_t)env * LM_TABLE);
    if (rc != 0) atomicCAS(a.status, 0, rc);
    if (a.params_out) for (int i = 0; i < JB_NPARAM; i++) a.params_out[(size_t)env * JB_NPARAM + i] = P[i];
    if (a.offsets_out) for (int i = 0; i < AO_COUNT; i++) a.offsets_out[(size_t)env * AO_COUNT + i] = off[i];
    if (a.attempts_out) a.attempts_out[env] = attempt;
}

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define JB_HIP(call)                                                                                     \
    do {                                                                                                 \
        hipError_t _e = (call);                                                                          \
        if (_e != hipSuccess) return fail(JB_E_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

// The owners of the handle's memory (jb_owned.hpp): device buffers, pinned host buffers, an event (n = 1)
struct HipDeviceMem {
    template <typename T> static hipError_t alloc(T** p, size_t n) { return hipMalloc((void**)p, n * sizeof(T)); }
    template <typename T> static void free(T* p) { (void)hipFree(p); }
};
struct HipPinnedMem {
    template <typename T> static hipError_t alloc(T** p, size_t n) { return hipHostMalloc((void**)p, n * sizeof(T), hipHostMallocDefault); }
    template <typename T> static void free(T* p) { (void)hipHostFree(p); }
};
struct HipEventApi {
    static hipError_t alloc(hipEvent_t* e, size_t) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }
    static void free(hipEvent_t e) { (void)hipEventDestroy(e); }
};
template <typename T> using Dev = Owned<T*, HipDeviceMem>;
template <typename T> using Pinned = Owned<T*, HipPinnedMem>;
using Event = Owned<hipEvent_t, HipEventApi>;

}  // namespace

// Every member that owns memory is an owner: destroying the handle frees it, and the handle cannot be copied.  The raw pointers in ka
// (and in the StepIO of a launch) are non-owning copies, refreshed wherever an owner is replaced.
struct jb_handle {
    jb_config cfg;
    KArgs ka;
    int D;
    hipStream_t stream;
    bool own_stream;
    Dev<float> d_root, d_leg, d_model, d_ovc;      // d_model: n_tables x LM_TABLE
    Dev<int> d_step; Dev<unsigned> d_episode;
    Dev<float> d_action, d_obs, d_reward; Dev<unsigned char> d_done, d_mask;      // staging for the host-buffer entry points
    Dev<double> d_qpos, d_qvel, d_target;
    Dev<unsigned long long> d_wave_stats, d_wave_clock, d_resolve;      // -DJB_WAVE_STATS builds; the last launch's wave lifetimes; [1]: KArgs::resolve_count
    Dev<float> d_capture; Dev<unsigned> d_capture_count;      // diagnostic builds (-DJB_CAPTURE)
    Dev<float> d_tape, d_rows_stage, d_rew_stage;      // staging of the host-buffer rollouts (jb_step_many, jb_rollout_policy): grow-only
    Dev<unsigned char> d_done_stage;                   // jb_score_tapes_device: the done flags of every step, next to d_rew_stage (grow-only)
    Dev<float> d_readout_stage;                        // jb_readout: the outputs on their way to the host (grow-only)
    Dev<float> d_inertia_stage;                        // jb_inertia: the actions and the outputs on their way (grow-only)
    Dev<float> d_evaluate_stage;                       // jb_evaluate: the targets and the outputs on their way (grow-only)
    Dev<float> d_contacts_stage;                       // jb_contacts: likewise
    Dev<float> d_forward_stage;                        // jb_forward: the actions on their way in, the outputs on their way out (grow-only)
    Dev<uint32_t> d_snap_stage; Dev<int> d_src_stage;  // jb_snapshot / jb_restore: the raw blocks and the index map on their way to / from the host (grow-only)
    Dev<int> d_wave_order;           // launch order of the waves (jb_wave_order_kernel), empty while the device holds the whole batch at once
    int wave_slots;                  // waves the device holds at once with this handle's kernel variant
    EncArgs enc;          // observation encoder (n_layers = 0: none)
    PolicyParams<float> policy;      // keyword arguments of the reference's heuristic policies
    Dev<JbNominalSpec> d_spec;       // nominal (uncompiled) model for the randomiser
    void* comm;                      // RCCL communicator (jb_comm_init), null until asked for
    int comm_ranks, comm_rank, comm_nmax;      // comm_nmax: envs of the longest shard (jb_comm_set_shards); 0: every rank holds cfg.n_envs
    // jb_step_async / jb_step_wait: pinned host staging (allocated at the first jb_step_async) and the event behind the D2H copies
    struct AsyncStage { Pinned<float> action, obs, reward; Pinned<unsigned char> done; Event copied; } async;
    bool async_pending;
    Dev<float> d_terms, d_enc_params, d_code;
    struct Witness { Dev<float> clear, min; Dev<int> pair; Dev<unsigned> count; } wit;      // the pair witness (jb_pair_witness / JB_FLAG_PAIR_WITNESS), allocated at first use
};
static_assert(!std::is_copy_constructible<jb_handle>::value && !std::is_copy_assignable<jb_handle>::value, "the handle owns its memory: never copied");

// ---------------------------------------------------------------------------------------------- RCCL, bound at run time
// The library has no link-time dependency on RCCL: a host that never calls jb_comm_* never loads it, and a process that already
// holds an RCCL (PyTorch-ROCm ships its own copy) keeps exactly that one - dlopen finds the loaded image first.
namespace {
struct RcclApi {
    struct IdBlob { char b[128]; };          // ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128), passed BY VALUE to ncclCommInitRank
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, IdBlob, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
int load_rccl() {
    if (g_rccl.lib) return JB_OK;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* lib = nullptr;
    for (const char* n : names) if ((lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;          // an image the process already holds
    if (!lib) for (const char* n : names) if ((lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!lib) return fail(JB_E_HIP, std::string("RCCL is not available (librccl.so): ") + (dlerror() ? dlerror() : ""));
    auto sym = [&](const char* n) { return dlsym(lib, n); };
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))sym("ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))sym("ncclCommInitRank");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))sym("ncclCommDestroy");
    g_rccl.GroupStart = (decltype(g_rccl.GroupStart))sym("ncclGroupStart");
    g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))sym("ncclGroupEnd");
    g_rccl.Send = (decltype(g_rccl.Send))sym("ncclSend");
    g_rccl.Recv = (decltype(g_rccl.Recv))sym("ncclRecv");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))sym("ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.GroupStart || !g_rccl.GroupEnd || !g_rccl.Send || !g_rccl.Recv)
        return fail(JB_E_HIP, "librccl.so lacks an expected symbol");
    g_rccl.lib = lib;
    return JB_OK;
}
#define JB_NCCL(call)                                                                                                      \
    do {                                                                                                                   \
        int _r = (call);                                                                                                   \
        if (_r != 0) return fail(JB_E_HIP, std::string(#call) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(_r) : "RCCL error")); \
    } while (0)
}  // namespace

// ---------------------------------------------------------------------------------------------- roctx ranges, bound at run time
// Named ranges around step / reset / gather so that a rocprofv3 --marker-trace timeline of the N > 1 path shows where the row gather
// sits relative to the step kernel (tracing row).  Like RCCL the library is bound by dlopen: an image the process
// already holds (the profiler's, or PyTorch's libroctx64) is used as is; otherwise it is loaded only when JB_ROCTX=1 asks for it.
// Without it the ranges cost one predictable branch.
namespace {
struct RoctxApi {
    int state = 0;          // 0: not looked for yet, 1: bound, -1: unavailable
    int (*Push)(const char*) = nullptr;
    int (*Pop)() = nullptr;
};
RoctxApi g_roctx;
void load_roctx() {
    const char* names[] = {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"};
    void* lib = nullptr;
    for (const char* n : names) if ((lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
    const char* want = getenv("JB_ROCTX");
    if (!lib && want && want[0] == '1') for (const char* n : names) if ((lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (lib) {
        g_roctx.Push = (decltype(g_roctx.Push))dlsym(lib, "roctxRangePushA");
        g_roctx.Pop = (decltype(g_roctx.Pop))dlsym(lib, "roctxRangePop");
    }
    g_roctx.state = (g_roctx.Push && g_roctx.Pop) ? 1 : -1;
}
struct RoctxRange {          // RAII: popped on every return path
    bool on;
    explicit RoctxRange(const char* name) {
        if (g_roctx.state == 0) load_roctx();
        on = g_roctx.state == 1;
        if (on) g_roctx.Push(name);
    }
    ~RoctxRange() { if (on) g_roctx.Pop(); }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;
};
}  // namespace

// Every entry point that allocates or launches runs with the handle's device current (a process may hold handles on several
// GPUs, or switch devices with torch.cuda.set_device after jb_create) and hands the caller's current device back on EVERY return
// path (jb_device_guard.hpp): torch reads the current device through hipGetDevice, so a switch that leaked out of an entry
// point would send the caller's next allocation or launch to the wrong GPU.
struct HipDeviceApi {
    static int get(int* d) { return hipGetDevice(d) == hipSuccess ? 0 : 1; }
    static int set(int d) { return hipSetDevice(d) == hipSuccess ? 0 : 1; }
};
#define JB_ENTER(h)                                                                                                   \
    if (!(h)) return fail(JB_E_INVALID, "handle is NULL");                                                            \
    jb::DeviceGuard<HipDeviceApi> _jb_device_guard;                                                                   \
    if (_jb_device_guard.enter((h)->cfg.device_id) != 0) return fail(JB_E_HIP, "hipSetDevice(" + std::to_string((h)->cfg.device_id) + ") failed")

static dim3 grid_lanes(int n) { return dim3((unsigned)(((size_t)n * 4 + 63) / 64)); }

// Which step kernel a handle runs: the row of jb_variant.hpp's launchable set for (LEAN, PAIR, one model per env, envs per wave).  A
// combination without a row is refused (JB_E_INVALID) at the call that creates it - never silently run as another kernel.
typedef void (*StepKernel)(KArgs, StepIO);
template <int I> static StepKernel step_row_kernel() {
    constexpr StepRow r = STEP_ROWS[I];
#ifdef JB_DEV_ONLY4      // development builds: the one instantiation the headline runs (a fifth of the compile time)
    constexpr bool built = r.variant == JB_VARIANT_ORDINARY && r.epw == 4;
#else
    constexpr bool built = true;
#endif
    if constexpr (!built) return nullptr;
    else if constexpr (r.lean && r.pair) return jb_step_kernel_lean_pair<r.epw>;
    else if constexpr (r.pair) return jb_step_kernel_pair<r.epw>;
    else if constexpr (r.lean) return jb_step_kernel_lean<r.epw>;
    else return jb_step_kernel<r.epw>;
}
template <int... I> static const StepKernel* step_kernels(std::integer_sequence<int, I...>) {
    static const StepKernel table[] = {step_row_kernel<I>()...};      // by row of STEP_ROWS
    return table;
}
// ... and a substep pass of a handle (jb_forward_kernel for FwArgs, jb_contacts_kernel for CtArgs), by whether its step kernel has the pair contacts
template <typename Args> using PassKernel = void (*)(KArgs, Args);
template <typename Args, bool PAIR> static PassKernel<Args> pass_kernel() {
#ifdef JB_DEV_ONLY4      // development builds: the ordinary layout only, like the step kernels
    constexpr bool built = !PAIR;
#else
    constexpr bool built = true;
#endif
    if constexpr (!built) return nullptr;
    else if constexpr (std::is_same<Args, FwArgs>::value) return jb_forward_kernel<PAIR>;
    else return jb_contacts_kernel<PAIR>;
}
static int kernel_variant(const KArgs& k) { return step_variant(k.lean, k.pair, k.per_env_model, k.epw); }
static int check_variant(int lean, int pair, int per_env_model, int epw) {
    if (step_row(lean, pair, per_env_model, epw) != STEP_NOT_LAUNCHABLE) return JB_OK;
    if (lean && pair)
        return fail(JB_E_INVALID, "JB_FLAG_LEAN cannot be honoured: the pair-contact kernel has a two-waves-per-SIMD form only for one model per env at 4 envs per wave "
                                  "(this handle: " + std::string(per_env_model ? "one model per env" : "a shared model that needs the pair contact") + ", " + std::to_string(epw) +
                                  " envs per wave); drop JB_FLAG_LEAN, or add JB_FLAG_NO_PAIR for floor contacts only");
    return fail(JB_E_INVALID, "no step kernel for " + std::to_string(epw) + " envs per wave" + (lean ? " with JB_FLAG_LEAN" : ""));
}
// The one way a model becomes the handle's (jb_create, jb_set_model_params, jb_randomise_models): `fresh`, when not empty, replaces the
// table buffer (empty: the tables were rewritten in place), and the kernel arguments follow.  The caller has synchronised the stream.
static void install_model(jb_handle* h, Dev<float> fresh, int per_env_model, int pair) {
    if (fresh) h->d_model = std::move(fresh);
    h->ka.lane_model = h->d_model.get(); h->ka.per_env_model = per_env_model; h->ka.pair = pair;
}
static int upload_model(jb_handle* h, const double* params, int n_tables) {
    std::vector<float> host((size_t)n_tables * LM_TABLE);
    for (int t = 0; t < n_tables; t++) {
        int rc = build_packed_model<float>(params + (size_t)t * JB_NPARAM, host.data() + (size_t)t * LM_TABLE);
        if (rc) return fail(JB_E_MODEL, "parameter table " + std::to_string(t) + " not supported by the kernel (code " + std::to_string(rc) + ")");
    }
    // which step kernel: the PAIR variant whenever the model(s) may bring the mass against a leg (see JB_FLAG_PAIR)
    const int pair = (h->cfg.flags & JB_FLAG_NO_PAIR) ? 0 : ((h->cfg.flags & JB_FLAG_PAIR) || n_tables > 1 || !mass_sweep_clear(params, 5e-4)) ? 1 : 0;
    const int per_env_model = n_tables > 1 ? 1 : 0;
    // a model that JB_FLAG_LEAN cannot run is refused BEFORE anything changes (the handle keeps the model it had)
    { int rc = check_variant(h->ka.lean, pair, per_env_model, h->ka.epw); if (rc) return rc; }
    Dev<float> fresh;      // (a buffer of the same size is rewritten in place)
    if (h->d_model.size() != host.size()) JB_HIP(fresh.alloc(host.size()));
    JB_HIP(hipMemcpyAsync(fresh ? fresh.get() : h->d_model.get(), host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    install_model(h, std::move(fresh), per_env_model, pair);
    return JB_OK;
}
// grow-only device staging owned by the handle, of any element type: (re)allocated only when a call needs more than any call before it
template <typename T> static int grow_stage(jb_handle* h, Dev<T>& buf, size_t n, const char* what) {
    if (n <= buf.size()) return JB_OK;
    if (buf) JB_HIP(hipStreamSynchronize(h->stream));      // (the buffer may still be in use by queued work)
    if (buf.alloc(n) != hipSuccess) return fail(JB_E_HIP, std::string("out of device memory for ") + what);
    return JB_OK;
}

// The host-buffer forms of the passes over states (jb_readout, jb_forward, jb_contacts) stage through one grow-only buffer of the handle, cut into the call's parts back to back in table order (every
// part but a last one of bytes is whole 4-byte words, and the tables put the parts whose lengths are multiples of 16 bytes first).  A part
// whose host pointer is NULL is absent: dev() is NULL and nothing is copied.
struct StagePart {
    void* host; size_t bytes; bool upload;
    char* at;
    template <typename T> T* dev() const { return host ? (T*)at : nullptr; }
};
template <size_t P> static int stage_parts(jb_handle* h, Dev<float>& buf, StagePart (&part)[P], const char* what) {
    size_t total = 0;
    for (const StagePart& q : part) total += q.bytes;
    int rc = grow_stage(h, buf, (total + 3) / 4, what);
    if (rc) return rc;
    char* at = (char*)buf.get();
    for (StagePart& q : part) {
        q.at = at; at += q.bytes;
        if (q.upload && q.host) JB_HIP(hipMemcpyAsync(q.at, q.host, q.bytes, hipMemcpyHostToDevice, h->stream));
    }
    return JB_OK;
}
template <size_t P> static int fetch_parts(jb_handle* h, const StagePart (&part)[P]) {
    for (const StagePart& q : part)
        if (!q.upload && q.host) JB_HIP(hipMemcpyAsync(q.host, q.at, q.bytes, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}

extern "C" {

const char* jb_last_error(void) { return g_err.c_str(); }
int jb_abi_version(void) { return JB_ABI_VERSION; }
// sha256 of the sources (csrc/*, include/*, compiler flags) this library was built from; jitterbug_amd/build.py passes it in and reads it
// back from the file (the tag in front makes it findable without loading the library)
#ifndef JB_SRC_SHA
#define JB_SRC_SHA "0000000000000000000000000000000000000000000000000000000000000000"
#endif
static const char JB_SRC_TAG[] = "JB_SRC_SHA256=" JB_SRC_SHA;
const char* jb_source_sha256(void) { return JB_SRC_TAG + 14; }
const double* jb_default_model_params(void) { return JB_DEFAULT_PARAMS; }
int jb_obs_dim(int32_t task_id) { return (task_id >= 0 && task_id < JB_NTASK) ? obs_dim(task_id) : JB_E_INVALID; }
int jb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int jb_default_config(jb_config* cfg, int32_t n_envs, int32_t task_id) {
    if (!cfg) return fail(JB_E_INVALID, "cfg is NULL");
    std::memset(cfg, 0, sizeof *cfg);
    cfg->n_envs = n_envs; cfg->task_id = task_id; cfg->device_id = 0; cfg->random_pose = 1; cfg->contacts = 1;
    cfg->substeps = 50; cfg->step_limit = 1000; cfg->auto_reset = 1; cfg->max_newton = JB_DEFAULT_MAX_NEWTON; cfg->seed = 0; cfg->env_offset = 0; cfg->stream = nullptr;
    return JB_OK;
}

static int create_impl(jb_handle* h) {      // every failure returns through jb_create, which destroys the partly built handle
    const jb_config* cfg = &h->cfg;
    const size_t N = (size_t)cfg->n_envs;
    if (cfg->use_caller_stream) { h->stream = (hipStream_t)cfg->stream; h->own_stream = false; }
    else { JB_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)); h->own_stream = true; }
    JB_HIP(h->d_root.alloc(ROOT_F * N)); JB_HIP(h->d_leg.alloc(LEG_F * 4 * N)); JB_HIP(h->d_step.alloc(N)); JB_HIP(h->d_episode.alloc(N)); JB_HIP(h->d_resolve.alloc(1));
    JB_HIP(h->d_action.alloc(N)); JB_HIP(h->d_obs.alloc(N * h->D)); JB_HIP(h->d_reward.alloc(N)); JB_HIP(h->d_done.alloc(N)); JB_HIP(h->d_mask.alloc(N));
    JB_HIP(h->d_qpos.alloc(16 * N)); JB_HIP(h->d_qvel.alloc(15 * N)); JB_HIP(h->d_target.alloc(3 * N)); JB_HIP(h->d_terms.alloc(4 * N));
#ifdef JB_CAPTURE
    JB_HIP(h->d_capture.alloc(64 * JB_CAPTURE_SLOTS)); JB_HIP(h->d_capture_count.alloc(1));
    JB_HIP(hipMemsetAsync(h->d_capture_count.get(), 0, sizeof(unsigned), h->stream));
#endif
    JB_HIP(hipMemsetAsync(h->d_resolve.get(), 0, sizeof(unsigned long long), h->stream));
#ifdef JB_WAVE_STATS
    JB_HIP(h->d_wave_stats.alloc((size_t)(16 + 64) * N));
    JB_HIP(hipMemset(h->d_wave_stats.get(), 0, sizeof(unsigned long long) * (size_t)(16 + 64) * N));
#endif
    JB_HIP(hipMemsetAsync(h->d_root.get(), 0, sizeof(float) * ROOT_F * N, h->stream));
    JB_HIP(hipMemsetAsync(h->d_leg.get(), 0, sizeof(float) * LEG_F * 4 * N, h->stream));
    JB_HIP(hipMemsetAsync(h->d_step.get(), 0, sizeof(int) * N, h->stream));
    JB_HIP(hipMemsetAsync(h->d_episode.get(), 0, sizeof(unsigned) * N, h->stream));
    KArgs& k = h->ka;
    k.n = cfg->n_envs; k.task = cfg->task_id; k.substeps = cfg->substeps; k.step_limit = cfg->step_limit; k.auto_reset = cfg->auto_reset;
    k.contacts = cfg->contacts; k.max_newton = h->cfg.max_newton; k.random_pose = cfg->random_pose; k.per_env_model = 0;
    k.seed = cfg->seed; k.env_offset = cfg->env_offset; k.rank_one = (cfg->flags & JB_FLAG_NO_RANK_ONE) ? 0 : 1; k.spread = (cfg->flags & JB_FLAG_NO_SPREAD) ? 0 : 1;
    k.lean = (cfg->flags & JB_FLAG_LEAN) ? 1 : 0;
    {   // envs per wave: fill every SIMD of the device before filling the lanes of a wave.  The kernel holds one wave
        // per SIMD (register budget), so the device runs (CUs x 4) waves at a time; LDS (scratch is per active lane)
        // allows 4 resident waves per CU up to 8 envs per wave.
        int epw = cfg->envs_per_wave;
        if (epw <= 0) {
            hipDeviceProp_t prop;
            JB_HIP(hipGetDeviceProperties(&prop, cfg->device_id));
            const int simds = prop.multiProcessorCount * 4;
            epw = (cfg->n_envs + simds - 1) / simds;
            if (epw > 4) epw = 4;     // LDS: 4 resident waves per CU need <= 40 KB each
        }
        if (epw < 1) epw = 1;
        if (epw > 8) epw = 8;                // (a 16-env wave would need 97 KB of LDS - one wave per CU - and spilled registers: not instantiated)
        while (epw & (epw - 1)) epw++;       // 1, 2, 4 or 8 (the kernel is instantiated for these)
        if (k.lean) { if (cfg->envs_per_wave <= 0) epw = 4; if (epw > 4) epw = 4; }     // LEAN: 4 envs per wave, 20 KB of LDS each: 8 waves per CU, two per SIMD
        k.epw = epw;
    }
    k.root = h->d_root.get(); k.leg = h->d_leg.get(); k.step_count = h->d_step.get(); k.episode = h->d_episode.get(); k.wave_stats = h->d_wave_stats.get();
    k.resolve_count = h->d_resolve.get(); k.capture = h->d_capture.get(); k.capture_count = h->d_capture_count.get();
    {   // the step kernels read part of their arguments through the kernarg segment: make sure that layout is what they assume (once per
        // process; handles created from several threads at once are serialised here)
        static std::mutex probe_mutex;
        static bool probed = false;
        std::lock_guard<std::mutex> lock(probe_mutex);
        if (!probed) {
            Dev<int> d_ok;
            JB_HIP(d_ok.alloc(1));
            KArgs pa = KArgs(); StepIO pio = StepIO();
            pa.n = 0x1234567; pa.seed = 0x0123456789ABCDEFull; pa.root = (float*)0x10002000; pa.step_limit = 777;
            pio.n_steps = 4242; pio.obs_out = (float*)0x30004000; pio.every_step = 5; pio.wave_clock = (unsigned long long*)0x50006000; pio.pp.angle_threshold = 0.625f;
            hipLaunchKernelGGL(jb_kernarg_probe_kernel, dim3(1), dim3(1), 0, h->stream, pa, pio, d_ok.get());
            int ok = 0;
            const hipError_t e1 = hipGetLastError(), e2 = hipMemcpyAsync(&ok, d_ok.get(), sizeof(int), hipMemcpyDeviceToHost, h->stream), e3 = hipStreamSynchronize(h->stream);
            if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return fail(JB_E_HIP, "kernarg probe failed to run");
            if (!ok) return fail(JB_E_HIP, "the step kernels' view of the kernarg segment does not match their arguments (compiler ABI change?): rebuild is needed with the layout fixed");
            probed = true;
        }
    }
    int rc = upload_model(h, JB_DEFAULT_PARAMS, 1);
    if (rc) return rc;
    rc = jb_reset_device(h, nullptr, nullptr);     // every env starts in a valid episode-0 state
    if (rc) return rc;
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}

int jb_create(const jb_config* cfg, jb_handle** out) {
    if (!cfg || !out) return fail(JB_E_INVALID, "cfg/out is NULL");
    *out = nullptr;
    if (cfg->n_envs < 1) return fail(JB_E_INVALID, "n_envs must be >= 1");
    if (cfg->task_id < 0 || cfg->task_id >= JB_NTASK) return fail(JB_E_INVALID, "unknown task_id");
    if (cfg->substeps < 1 || cfg->step_limit < 1) return fail(JB_E_INVALID, "substeps and step_limit must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(JB_E_NODEVICE, "no HIP device available (there is no CPU fallback)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(JB_E_INVALID, "device_id out of range");
    jb::DeviceGuard<HipDeviceApi> guard;              // the caller's current device is restored on every return path
    if (guard.enter(cfg->device_id) != 0) return fail(JB_E_HIP, "hipSetDevice(" + std::to_string(cfg->device_id) + ") failed");
    jb_handle* h = new (std::nothrow) jb_handle();      // (value-initialised: every plain member zero, every owner empty)
    if (!h) return fail(JB_E_INVALID, "out of host memory");
    h->cfg = *cfg;
    if (h->cfg.max_newton <= 0) h->cfg.max_newton = JB_DEFAULT_MAX_NEWTON;
    h->D = obs_dim(cfg->task_id);
    h->policy = default_policy_params<float>();
    const int rc = create_impl(h);
    if (rc) {                               // one cleanup path: the handle with what it holds so far, the stream (keep the message)
        const std::string msg = g_err;
        jb_destroy(h);
        g_err = msg;
        return rc;
    }
    *out = h;
    return JB_OK;
}

int jb_destroy(jb_handle* h) {
    if (!h) return JB_OK;
    jb::DeviceGuard<HipDeviceApi> guard;
    guard.enter(h->cfg.device_id);
    if (h->stream || !h->own_stream) hipStreamSynchronize(h->stream);
    if (h->comm && g_rccl.CommDestroy) { hipDeviceSynchronize(); g_rccl.CommDestroy(h->comm); h->comm = nullptr; }      // (device-wide: exchanges may be queued on streams of the caller's)
    const hipStream_t stream = h->own_stream ? h->stream : nullptr;      // (a caller's stream is never destroyed)
    delete h;                                  // every buffer, the pinned staging and the event
    if (stream) hipStreamDestroy(stream);
    return JB_OK;
}

int jb_set_obs_encoder(jb_handle* h, int32_t n_layers, const int32_t* dims, const int32_t* acts, const float* weights, const float* biases, int32_t vae) {
    JB_ENTER(h);
    JB_HIP(hipStreamSynchronize(h->stream));
    if (n_layers == 0) { h->d_enc_params.reset(); h->d_code.reset(); h->enc = EncArgs(); return JB_OK; }
    if (n_layers < 0 || n_layers > JB_ENC_MAX_LAYERS || !dims || !acts || !weights || !biases) return fail(JB_E_INVALID, "encoder: 1.." + std::to_string(JB_ENC_MAX_LAYERS) + " layers with dims/acts/weights/biases");
    if (dims[0] != h->D) return fail(JB_E_INVALID, "encoder: dims[0] must be the observation width " + std::to_string(h->D));
    size_t nw = 0, nb = 0;
    for (int l = 0; l < n_layers; l++) {
        if (dims[l] < 1 || dims[l] > JB_ENC_MAX_WIDTH || dims[l + 1] < 1 || dims[l + 1] > JB_ENC_MAX_WIDTH) return fail(JB_E_INVALID, "encoder: layer widths must be 1.." + std::to_string(JB_ENC_MAX_WIDTH));
        if (acts[l] < JB_ACT_LINEAR || acts[l] > JB_ACT_RELU) return fail(JB_E_INVALID, "encoder: unknown activation");
        nw += (size_t)dims[l] * dims[l + 1]; nb += (size_t)dims[l + 1];
    }
    if (vae && (dims[n_layers] & 1)) return fail(JB_E_INVALID, "encoder: a VAE head needs an even last width [mean | std]");
    EncArgs e = EncArgs();
    e.n = h->cfg.n_envs; e.n_layers = n_layers; e.vae = vae ? 1 : 0; e.in_dim = dims[0]; e.out_dim = vae ? dims[n_layers] / 2 : dims[n_layers];
    size_t wo = 0, bo = nw;
    for (int l = 0; l < n_layers; l++) {
        e.dims[l] = dims[l]; e.acts[l] = acts[l]; e.woff[l] = (int)wo; e.boff[l] = (int)bo;
        wo += (size_t)dims[l] * dims[l + 1]; bo += (size_t)dims[l + 1];
    }
    e.dims[n_layers] = dims[n_layers];
    e.seed = h->cfg.seed; e.env_offset = h->cfg.env_offset; e.call = 0;
    Dev<float> params, code;          // the handle keeps the encoder it had until every step below has succeeded
    JB_HIP(params.alloc(nw + nb)); JB_HIP(code.alloc((size_t)e.n * e.out_dim));
    JB_HIP(hipMemcpy(params.get(), weights, nw * sizeof(float), hipMemcpyHostToDevice));
    JB_HIP(hipMemcpy(params.get() + nw, biases, nb * sizeof(float), hipMemcpyHostToDevice));
    e.params = params.get();
    h->d_enc_params = std::move(params); h->d_code = std::move(code);
    h->enc = e;
    return JB_OK;
}
int jb_encoded_dim(jb_handle* h) { return h ? h->enc.out_dim * (h->enc.n_layers > 0) : JB_E_INVALID; }
int jb_encode_device(jb_handle* h, const float* d_obs, float* d_code_out) {
    if (!h || !d_obs || !d_code_out) return fail(JB_E_INVALID, "handle/obs/out is NULL");
    JB_ENTER(h);
    if (h->enc.n_layers <= 0) return fail(JB_E_INVALID, "no observation encoder set (jb_set_obs_encoder)");
    const int N = h->cfg.n_envs;
    hipLaunchKernelGGL(jb_encode_kernel, dim3((unsigned)((N + 127) / 128)), dim3(128), 0, h->stream, h->enc, d_obs, d_code_out);
    JB_HIP(hipGetLastError());
    h->enc.call++;
    return JB_OK;
}
int jb_encode(jb_handle* h, const float* obs, float* code_out) {
    if (!h || !obs || !code_out) return fail(JB_E_INVALID, "handle/obs/out is NULL");
    JB_ENTER(h);
    if (h->enc.n_layers <= 0) return fail(JB_E_INVALID, "no observation encoder set (jb_set_obs_encoder)");
    const size_t N = (size_t)h->cfg.n_envs;
    JB_HIP(hipMemcpyAsync(h->d_obs.get(), obs, sizeof(float) * N * h->D, hipMemcpyHostToDevice, h->stream));
    int rc = jb_encode_device(h, h->d_obs.get(), h->d_code.get());
    if (rc) return rc;
    JB_HIP(hipMemcpyAsync(code_out, h->d_code.get(), sizeof(float) * N * h->enc.out_dim, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}
int jb_debug_poison_lds(jb_handle* h) {
    JB_ENTER(h);
    hipDeviceProp_t prop;
    JB_HIP(hipGetDeviceProperties(&prop, h->cfg.device_id));
    const int bytes = 40 * 1024;                                   // 4 resident blocks cover a CU's 160 KB
    hipLaunchKernelGGL(jb_poison_lds_kernel, dim3((unsigned)prop.multiProcessorCount * 8), dim3(256), bytes, h->stream, bytes / 4, (float*)nullptr);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
int jb_num_envs(jb_handle* h) { return h ? h->cfg.n_envs : JB_E_INVALID; }
void* jb_stream(jb_handle* h) { return h ? (void*)h->stream : nullptr; }
int jb_synchronize(jb_handle* h) {
    JB_ENTER(h);
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}

int jb_reset_device(jb_handle* h, const uint8_t* d_mask, float* d_obs_out) {
    JB_ENTER(h);
    RoctxRange range("jb_reset");
    hipLaunchKernelGGL(jb_reset_kernel, grid_lanes(h->cfg.n_envs), dim3(64), 0, h->stream, h->ka, d_mask, d_obs_out);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
static int ensure_witness(jb_handle* h) {
    if (h->wit.clear) return JB_OK;
    const size_t N = (size_t)h->cfg.n_envs;
    jb_handle::Witness w;          // all or nothing: the handle takes the group once every buffer is allocated and initialised
    JB_HIP(w.clear.alloc(N)); JB_HIP(w.min.alloc(N)); JB_HIP(w.pair.alloc(2 * N)); JB_HIP(w.count.alloc(N));
    std::vector<float> inf(N, INFINITY);
    JB_HIP(hipMemcpyAsync(w.min.get(), inf.data(), sizeof(float) * N, hipMemcpyHostToDevice, h->stream));
    JB_HIP(hipMemsetAsync(w.count.get(), 0, sizeof(unsigned) * N, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));          // (`inf` goes out of scope)
    h->wit = std::move(w);
    return JB_OK;
}
static int launch_step(jb_handle* h, StepIO io, int packed_rows) {
    if (!h) return fail(JB_E_INVALID, "handle is NULL");
    if (io.n_steps < 1) return fail(JB_E_INVALID, "n_steps must be >= 1");
    if (!io.use_policy && !io.actions) return fail(JB_E_INVALID, "action buffer is NULL");
    JB_ENTER(h);
    const int row = step_row(h->ka.lean, h->ka.pair, h->ka.per_env_model, h->ka.epw);
    if (row == STEP_NOT_LAUNCHABLE) return check_variant(h->ka.lean, h->ka.pair, h->ka.per_env_model, h->ka.epw);
    const StepKernel kernel = step_kernels(std::make_integer_sequence<int, N_STEP_ROWS>())[row];
    if (!kernel) return fail(JB_E_INVALID, "JB_DEV_ONLY4 build: only the ordinary kernel at 4 envs per wave");
    const StepLayout lay = step_layout(h->ka.epw, STEP_ROWS[row].lean, STEP_ROWS[row].pair);
    RoctxRange range(io.n_steps > 1 ? "jb_step_many" : "jb_step");
    h->ka.packed_rows = packed_rows;
    io.pp = h->policy;
    const dim3 grid((unsigned)((h->cfg.n_envs + h->ka.epw - 1) / h->ka.epw));
    if (!h->d_wave_clock) {
        Dev<unsigned long long> clock;
        JB_HIP(clock.alloc((size_t)h->cfg.n_envs));      // (>= the number of waves for any envs-per-wave)
        JB_HIP(hipMemsetAsync(clock.get(), 0, sizeof(unsigned long long) * (size_t)h->cfg.n_envs, h->stream));
        h->d_wave_clock = std::move(clock);
    }
    io.wave_clock = h->d_wave_clock.get();
    // more waves than the device holds at once -> launch them longest first (the order comes from the previous launch's clocks)
    WaveOrderPlan order_plan = {false, 0};
    if (!(h->cfg.flags & JB_FLAG_NO_REORDER)) {
        if (h->wave_slots == 0) {
            hipDeviceProp_t prop;
            JB_HIP(hipGetDeviceProperties(&prop, h->cfg.device_id));
            h->wave_slots = prop.multiProcessorCount * 4;
        }
        order_plan = wave_order_plan((int)grid.x, h->wave_slots, lay.waves_per_simd);
        if (order_plan.reorder && !h->d_wave_order) {
            Dev<int> order;
            JB_HIP(order.alloc((size_t)h->cfg.n_envs));
            hipLaunchKernelGGL(jb_wave_order_kernel, dim3(1), dim3(1024), 0, h->stream, h->d_wave_clock.get(), order.get(), (int)grid.x, order_plan.fold_from);      // (clocks all zero: identity)
            JB_HIP(hipGetLastError());
            h->d_wave_order = std::move(order);
        }
    }
    io.wave_order = order_plan.reorder ? h->d_wave_order.get() : nullptr;
    const size_t lds_bytes = step_lds_bytes(lay, h->ka.per_env_model != 0);
#ifdef JB_DEBUG
    static const size_t extra_lds = getenv("JB_DEBUG_EXTRA_LDS") ? (size_t)atoi(getenv("JB_DEBUG_EXTRA_LDS")) : 0;      // occupancy experiments (-DJB_DEBUG builds only)
    const size_t lds_bytes_x = lds_bytes + extra_lds;
#else
    const size_t lds_bytes_x = lds_bytes;
#endif
    if (lay.ovc_floats && !h->d_ovc) {      // the LEAN variants' block per wave: overflow candidates (beyond the row cache), the second pair contact's frame
        JB_HIP(h->d_ovc.alloc((size_t)grid.x * lay.ovc_floats * lay.main_lanes));      // (a failed allocation leaves it empty)
        h->ka.ovc_buf = h->d_ovc.get();
    }
    hipLaunchKernelGGL(kernel, grid, dim3(64), lds_bytes_x, h->stream, h->ka, io);
    JB_HIP(hipGetLastError());
    if (order_plan.reorder) {
        hipLaunchKernelGGL(jb_wave_order_kernel, dim3(1), dim3(1024), 0, h->stream, h->d_wave_clock.get(), h->d_wave_order.get(), (int)grid.x, order_plan.fold_from);
        JB_HIP(hipGetLastError());
    }
    if (h->cfg.flags & JB_FLAG_PAIR_WITNESS) {      // one witness pass behind every step launch (the state the launch left)
        int rc = ensure_witness(h);
        if (rc) return rc;
        hipLaunchKernelGGL(jb_witness_kernel, dim3((unsigned)((h->cfg.n_envs + 63) / 64)), dim3(64), 0, h->stream, h->ka, (float*)nullptr, (int*)nullptr, h->wit.min.get(), h->wit.count.get());
        JB_HIP(hipGetLastError());
    }
    return JB_OK;
}
int jb_kernel_variant(jb_handle* h) { return h ? kernel_variant(h->ka) : JB_E_INVALID; }
int jb_envs_per_wave(jb_handle* h) { return h ? h->ka.epw : JB_E_INVALID; }
int jb_step_device(jb_handle* h, const float* d_action, float* d_obs_out, float* d_reward_out, uint8_t* d_done_out) {
    if (!d_action) return fail(JB_E_INVALID, "handle/action is NULL");
    StepIO io = StepIO();
    io.n_steps = 1; io.actions = d_action; io.obs_out = d_obs_out; io.reward_out = d_reward_out; io.done_out = d_done_out;
    return launch_step(h, io, 0);
}
int jb_step_rows_device(jb_handle* h, const float* d_action, float* d_rows_out) {
    if (!d_action) return fail(JB_E_INVALID, "handle/action is NULL");
    if (!d_rows_out) return fail(JB_E_INVALID, "rows buffer is NULL");
    StepIO io = StepIO();
    io.n_steps = 1; io.actions = d_action; io.obs_out = d_rows_out;
    return launch_step(h, io, 1);
}
// K control steps in ONE launch (see StepIO).  d_actions [K, N], or NULL: the handle's heuristic policy, evaluated in the kernel.
// d_rows_out [K, N, D+2] nullable (packed rows of every step); d_rewards [K, N] nullable; d_obs_last [N, D] / d_done_last [N] nullable:
// the last step's observations / done flags.  Rows and the separate outputs exclude each other (one output layout per launch).
int jb_step_many_device(jb_handle* h, int32_t n_steps, const float* d_actions, float* d_rows_out, float* d_rewards, float* d_obs_last, uint8_t* d_done_last) {
    if (!h) return fail(JB_E_INVALID, "handle is NULL");
    if (n_steps < 0) return fail(JB_E_INVALID, "n_steps < 0");
    if (n_steps == 0) return JB_OK;
    if (d_rows_out && (d_rewards || d_obs_last || d_done_last)) return fail(JB_E_INVALID, "jb_step_many_device: either packed rows [K,N,D+2] or rewards / last observations / last done flags, not both");
    StepIO io = StepIO();
    io.n_steps = n_steps; io.use_policy = d_actions ? 0 : 1; io.actions = d_actions;
    if (d_rows_out) {
        io.obs_out = d_rows_out; io.every_step = 1;
        return launch_step(h, io, 1);
    }
    io.obs_out = d_obs_last; io.reward_out = d_rewards; io.done_out = d_done_last;
    io.every_step = 2;
    return launch_step(h, io, 0);
}
// host-buffer form of jb_step_many_device: actions [K, N] (NULL: the in-kernel heuristic policy), rows_out [K, N, D+2] (nullable);
// the device staging belongs to the handle and only ever grows (no allocation after the first call of a given size); the results are valid on return
int jb_step_many(jb_handle* h, int32_t n_steps, const float* actions, float* rows_out) {
    if (!h) return fail(JB_E_INVALID, "handle is NULL");
    if (n_steps < 0) return fail(JB_E_INVALID, "n_steps < 0");
    if (n_steps == 0) return JB_OK;
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs, K = (size_t)n_steps, W = (size_t)h->D + 2;
    int rc = JB_OK;
    if (actions) {
        rc = grow_stage(h, h->d_tape, K * N, "the action tape");
        if (rc) return rc;
        JB_HIP(hipMemcpyAsync(h->d_tape.get(), actions, sizeof(float) * K * N, hipMemcpyHostToDevice, h->stream));
    }
    if (rows_out) { rc = grow_stage(h, h->d_rows_stage, K * N * W, "the rows"); if (rc) return rc; }
    rc = jb_step_many_device(h, n_steps, actions ? h->d_tape.get() : nullptr, rows_out ? h->d_rows_stage.get() : nullptr, nullptr, nullptr, nullptr);
    if (!rc && rows_out && hipMemcpyAsync(rows_out, h->d_rows_stage.get(), sizeof(float) * K * N * W, hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = fail(JB_E_HIP, "jb_step_many: copy of the rows failed");
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (!rc && e != hipSuccess) rc = fail(JB_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
}
int jb_release_staging(jb_handle* h) {
    JB_ENTER(h);
    JB_HIP(hipStreamSynchronize(h->stream));
    h->d_tape.reset(); h->d_rows_stage.reset(); h->d_rew_stage.reset(); h->d_done_stage.reset();
    h->d_snap_stage.reset(); h->d_src_stage.reset(); h->d_readout_stage.reset(); h->d_inertia_stage.reset(); h->d_evaluate_stage.reset(); h->d_forward_stage.reset(); h->d_contacts_stage.reset();
    return JB_OK;
}
// ---------------------------------------------------------------------------------------------- snapshot / restore / fork, tape scoring
// (jb_snapshot.hpp: a snapshot is the four state blocks back to back; every form below is ONE launch of jb_fork_kernel)
static SnapView state_view(jb_handle* h) {
    SnapView v;
    v.root = (uint32_t*)h->d_root.get(); v.leg = (uint32_t*)h->d_leg.get(); v.step = (uint32_t*)h->d_step.get(); v.episode = (uint32_t*)h->d_episode.get();
    v.n = h->cfg.n_envs;
    return v;
}
static int launch_fork(jb_handle* h, const SnapView& dst, const SnapView& src, const int* d_map) {
    const long long total = (long long)SNAP_WORDS * dst.n;
    long long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;      // (grid-stride beyond 2 M words)
    hipLaunchKernelGGL(jb_fork_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, dst, src, d_map);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
int64_t jb_snapshot_bytes(jb_handle* h) {
    if (!h) return fail(JB_E_INVALID, "handle is NULL");
    return (int64_t)SNAP_ENV_BYTES * (int64_t)h->cfg.n_envs;
}
int64_t jb_snapshot_host_bytes(jb_handle* h) {
    if (!h) return fail(JB_E_INVALID, "handle is NULL");
    return (int64_t)snap_blob_bytes(h->cfg.n_envs);
}
int jb_snapshot_device(jb_handle* h, void* d_snap) {
    JB_ENTER(h);
    if (!d_snap) return fail(JB_E_INVALID, "jb_snapshot_device: the snapshot buffer is NULL");
    if (h->async_pending) return fail(JB_E_INVALID, "jb_snapshot_device: a jb_step_async is pending (jb_step_wait first)");
    RoctxRange range("jb_snapshot");
    return launch_fork(h, snap_view(d_snap, h->cfg.n_envs), state_view(h), nullptr);
}
int jb_restore_device(jb_handle* h, const void* d_snap, int32_t n_src, const int32_t* d_src) {
    JB_ENTER(h);
    if (!d_snap) return fail(JB_E_INVALID, "jb_restore_device: the snapshot buffer is NULL");
    if (h->async_pending) return fail(JB_E_INVALID, "jb_restore_device: a jb_step_async is pending (jb_step_wait first)");
    if (n_src < 1) return fail(JB_E_INVALID, "jb_restore_device: n_src must be >= 1");
    if (!d_src && n_src != h->cfg.n_envs)
        return fail(JB_E_INVALID, "jb_restore_device: a snapshot of " + std::to_string(n_src) + " envs onto a handle of " + std::to_string(h->cfg.n_envs) + " needs an index map");
    RoctxRange range("jb_restore");
    return launch_fork(h, state_view(h), snap_view(const_cast<void*>(d_snap), n_src), d_src);      // (const_cast: the source side is only read)
}
int jb_snapshot(jb_handle* h, void* blob) {
    JB_ENTER(h);
    if (!blob) return fail(JB_E_INVALID, "jb_snapshot: blob is NULL");
    if (h->async_pending) return fail(JB_E_INVALID, "jb_snapshot: a jb_step_async is pending (jb_step_wait first)");
    const size_t N = (size_t)h->cfg.n_envs;
    int rc = grow_stage(h, h->d_snap_stage, N * SNAP_WORDS, "the snapshot");
    if (rc) return rc;
    rc = jb_snapshot_device(h, h->d_snap_stage.get());
    if (rc) return rc;
    const SnapHeader hd = snap_make_header(h->cfg.n_envs, h->cfg.task_id, h->cfg.substeps, h->cfg.step_limit);
    std::memcpy(blob, &hd, sizeof hd);
    JB_HIP(hipMemcpyAsync((char*)blob + SNAP_HEADER_BYTES, h->d_snap_stage.get(), N * SNAP_ENV_BYTES, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}
int jb_restore(jb_handle* h, const void* blob, int64_t blob_bytes, const int32_t* src) {
    JB_ENTER(h);
    if (!blob) return fail(JB_E_INVALID, "jb_restore: blob is NULL");
    if (h->async_pending) return fail(JB_E_INVALID, "jb_restore: a jb_step_async is pending (jb_step_wait first)");
    // everything is checked on the host before anything is copied or launched
    if (blob_bytes < (int64_t)SNAP_HEADER_BYTES) return fail(JB_E_INVALID, "jb_restore: blob is shorter than its header");
    SnapHeader hd;
    std::memcpy(&hd, blob, sizeof hd);
    if (const char* why = snap_check_header(hd, (long long)blob_bytes, h->cfg.task_id)) return fail(JB_E_INVALID, std::string("jb_restore: ") + why);
    const int N = h->cfg.n_envs, n_src = hd.n_envs;
    if (!src && n_src != N) return fail(JB_E_INVALID, "jb_restore: a snapshot of " + std::to_string(n_src) + " envs onto a handle of " + std::to_string(N) + " needs an index map");
    if (src) {
        const int bad = snap_first_bad_index(src, N, n_src);
        if (bad >= 0) return fail(JB_E_INVALID, "jb_restore: src[" + std::to_string(bad) + "] = " + std::to_string(src[bad]) + " is outside [0, " + std::to_string(n_src) + ")");
    }
    int rc = grow_stage(h, h->d_snap_stage, (size_t)n_src * SNAP_WORDS, "the snapshot");
    if (rc) return rc;
    if (src) { rc = grow_stage(h, h->d_src_stage, (size_t)N, "the index map"); if (rc) return rc; }
    JB_HIP(hipMemcpyAsync(h->d_snap_stage.get(), (const char*)blob + SNAP_HEADER_BYTES, (size_t)n_src * SNAP_ENV_BYTES, hipMemcpyHostToDevice, h->stream));
    if (src) JB_HIP(hipMemcpyAsync(h->d_src_stage.get(), src, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, h->stream));
    rc = jb_restore_device(h, h->d_snap_stage.get(), n_src, src ? h->d_src_stage.get() : nullptr);
    const hipError_t e = hipStreamSynchronize(h->stream);      // (the caller's blob and map are free again on return)
    if (!rc && e != hipSuccess) rc = fail(JB_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
}
// K fused steps from the current state (the step kernel, through launch_step: rewards and done flags of EVERY step into the handle's
// staging), then one thread per env folds them into the discounted return.  The handle is left in the post-rollout state.
int jb_score_tapes_device(jb_handle* h, int32_t n_steps, const float* d_tapes, float gamma, float* d_returns, int32_t* d_alive) {
    JB_ENTER(h);
    if (n_steps < 1) return fail(JB_E_INVALID, "jb_score_tapes_device: n_steps must be >= 1");
    if (!d_returns) return fail(JB_E_INVALID, "jb_score_tapes_device: the returns buffer is NULL");
    if (!std::isfinite(gamma)) return fail(JB_E_INVALID, "jb_score_tapes_device: gamma must be finite");
    if (h->async_pending) return fail(JB_E_INVALID, "jb_score_tapes_device: a jb_step_async is pending (jb_step_wait first)");
    RoctxRange range("jb_score_tapes");
    const size_t N = (size_t)h->cfg.n_envs, K = (size_t)n_steps;
    int rc = grow_stage(h, h->d_rew_stage, K * N, "the rewards");
    if (!rc) rc = grow_stage(h, h->d_done_stage, K * N, "the done flags");
    if (rc) return rc;
    StepIO io = StepIO();
    io.n_steps = n_steps; io.use_policy = d_tapes ? 0 : 1; io.actions = d_tapes;
    io.reward_out = h->d_rew_stage.get(); io.done_out = h->d_done_stage.get(); io.every_step = 2 | 4;
    rc = launch_step(h, io, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(jb_return_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, (const float*)h->d_rew_stage.get(), (const unsigned char*)h->d_done_stage.get(),
                       (int)n_steps, (int)N, gamma, d_returns, (int*)d_alive);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
// ---------------------------------------------------------------------------------------------- passes over states: readout, forward dynamics, contacts
// What every pass refuses before it touches anything, under the name of the entry point `fn` (`n_out` spells how many outputs it has); then
// `first` is snapshot 0 of the stack, or the handle's own blocks.
static int check_pass(jb_handle* h, const std::string& fn, const void* d_snaps, int n_snaps, bool any_output, const char* n_out, SnapView* first = nullptr) {
    if (n_snaps < 1) return fail(JB_E_INVALID, fn + ": n_snaps must be >= 1");
    if (!any_output) return fail(JB_E_INVALID, fn + ": all " + n_out + " outputs are NULL");
    if (h->async_pending) return fail(JB_E_INVALID, fn + ": a jb_step_async is pending (jb_step_wait first)");
    if (!d_snaps && n_snaps != 1) return fail(JB_E_INVALID, fn + ": the handle's current state is ONE state (n_snaps must be 1 without a snapshot stack)");
    if (first) *first = d_snaps ? snap_view(const_cast<void*>(d_snaps), h->cfg.n_envs) : state_view(h);      // (const_cast: the passes only read)
    return JB_OK;
}
static int check_grid(const std::string& fn, long long blocks) {
    return blocks > 0x7fffffffLL ? fail(JB_E_INVALID, fn + ": too many env-states for one launch") : JB_OK;
}
// The launch of a substep pass (PassWave): n_snaps x ceil(N / 4) waves of the step kernels' layout at four envs per wave, whichever kernel the handle steps with.
struct PassLaunch {
    KArgs a;
    PassArgs p;
    dim3 grid;
    size_t lds_bytes;            // scratch and tables (step_lds_bytes)
};
static int prepare_pass(jb_handle* h, const std::string& fn, const void* d_snaps, int n_snaps, bool any_output, const char* n_out, const float* d_ctrl, uint8_t* d_unconverged, PassLaunch& l) {
    int rc = check_pass(h, fn, d_snaps, n_snaps, any_output, n_out, &l.p.first);
    if (rc) return rc;
    const int N = h->cfg.n_envs;
    l.a = h->ka;
    l.a.epw = FW_EPW; l.a.lean = 0;
    l.p.stride_words = (long long)SNAP_WORDS * N;
    l.p.waves_per_snap = (N + FW_EPW - 1) / FW_EPW;
    l.p.ctrl = d_ctrl; l.p.unconv = d_unconverged;
    const long long blocks = (long long)n_snaps * l.p.waves_per_snap;
    l.grid = dim3((unsigned)blocks);
    l.lds_bytes = step_lds_bytes(step_layout(FW_EPW, false, h->ka.pair != 0), h->ka.per_env_model != 0);
    return check_grid(fn, blocks);
}
// The readout pass (jb_readout.hpp): one launch over n_snaps * N env-states, a quad of lanes each; reads the state, writes only its outputs.
int jb_readout_device(jb_handle* h, const void* d_snaps, int32_t n_snaps, float* d_frames, float* d_clearance, float* d_body_vel, float* d_energy) {
    JB_ENTER(h);
    RoArgs a;
    int rc = check_pass(h, "jb_readout_device", d_snaps, n_snaps, d_frames || d_clearance || d_body_vel || d_energy, "four", &a.first);
    if (rc) return rc;
    RoctxRange range("jb_readout");
    const int N = h->cfg.n_envs;
    a.stride_words = (long long)SNAP_WORDS * N;
    a.total = (long long)n_snaps * N;
    a.tab = h->ka.lane_model; a.n_tab = h->ka.per_env_model ? N : 1;
    a.frames = d_frames; a.clear = d_clearance; a.bvel = d_body_vel; a.energy = d_energy;
    a.vec4 = ((((uintptr_t)d_frames | (uintptr_t)d_clearance | (uintptr_t)d_body_vel | (uintptr_t)d_energy) & 15u) == 0) ? 1 : 0;
    const long long blocks = (a.total + RO_EPB - 1) / RO_EPB;
    rc = check_grid("jb_readout_device", blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(jb_readout_kernel, dim3((unsigned)blocks), dim3(64), 0, h->stream, a);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
int jb_readout(jb_handle* h, float* frames, float* clearance, float* body_vel, float* energy) {
    JB_ENTER(h);
    const size_t F = sizeof(float) * (size_t)h->cfg.n_envs;
    StagePart part[] = {{frames, F * RO_FRAMES}, {body_vel, F * RO_BVEL}, {energy, F * RO_ENERGY}, {clearance, F * RO_CLEAR}};
    int rc = check_pass(h, "jb_readout", nullptr, 1, frames || clearance || body_vel || energy, "four");
    if (!rc) rc = stage_parts(h, h->d_readout_stage, part, "the readout");
    if (!rc) rc = jb_readout_device(h, nullptr, 1, part[0].dev<float>(), part[3].dev<float>(), part[1].dev<float>(), part[2].dev<float>());
    return rc ? rc : fetch_parts(h, part);
}
// The forward-dynamics pass (jb_forward_kernel above): reads the state, writes only its outputs.
int jb_forward_device(jb_handle* h, const void* d_snaps, int32_t n_snaps, const float* d_ctrl, float* d_qacc, float* d_qfrc, float* d_body_acc, float* d_motor, uint8_t* d_unconverged) {
    JB_ENTER(h);
    PassLaunch l;
    int rc = prepare_pass(h, "jb_forward_device", d_snaps, n_snaps, d_qacc || d_qfrc || d_body_acc || d_motor || d_unconverged, "five", d_ctrl, d_unconverged, l);
    if (rc) return rc;
    const PassKernel<FwArgs> kernel = h->ka.pair ? pass_kernel<FwArgs, true>() : pass_kernel<FwArgs, false>();
    if (!kernel) return fail(JB_E_INVALID, "JB_DEV_ONLY4 build: only the forward pass without the pair contacts");
    RoctxRange range("jb_forward");
    FwArgs f;
    f.p = l.p;
    f.qacc = d_qacc; f.qfrc = d_qfrc; f.bacc = d_body_acc; f.motor = d_motor;
    hipLaunchKernelGGL(kernel, l.grid, dim3(64), l.lds_bytes, h->stream, l.a, f);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
int jb_forward(jb_handle* h, const float* ctrl, float* qacc, float* qfrc, float* body_acc, float* motor, uint8_t* unconverged) {
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs, F = sizeof(float) * N;
    StagePart part[] = {{body_acc, F * FW_BACC}, {qacc, F * FW_NV}, {qfrc, F * FW_NV}, {motor, F * FW_MOTOR}, {const_cast<float*>(ctrl), F, true}, {unconverged, N}};
    int rc = check_pass(h, "jb_forward", nullptr, 1, qacc || qfrc || body_acc || motor || unconverged, "five");
    if (!rc) rc = stage_parts(h, h->d_forward_stage, part, "the forward pass");
    if (!rc) rc = jb_forward_device(h, nullptr, 1, part[4].dev<float>(), part[1].dev<float>(), part[2].dev<float>(), part[0].dev<float>(), part[3].dev<float>(), part[5].dev<uint8_t>());
    return rc ? rc : fetch_parts(h, part);
}
// The contact pass (jb_contacts_kernel above): the forward pass's launch with the output images behind the scratch and the tables in LDS.
static_assert(JB_NCONTACT == CT_NROW && JB_CONTACT_WIDTH == CT_W, "the header states the table's shape");
static_assert(step_lds_bytes(step_layout(FW_EPW, false, true), true) + 16 + CT_LDS_FLOATS * sizeof(float) <= 64 * 1024 &&
              step_lds_bytes(step_layout(FW_EPW, false, false), true) + 16 + CT_LDS_FLOATS * sizeof(float) <= 64 * 1024, "scratch, tables and images fit a workgroup's 64 KB of LDS");
int32_t jb_contact_rows(void) { return CT_NROW; }
void jb_contact_slot_geoms(int32_t* out) { if (out) ct_slot_geoms(out); }
int jb_contacts_device(jb_handle* h, const void* d_snaps, int32_t n_snaps, const float* d_ctrl, float* d_contact, int32_t* d_ncon, float* d_geom_frc, uint8_t* d_unconverged) {
    JB_ENTER(h);
    PassLaunch l;
    int rc = prepare_pass(h, "jb_contacts_device", d_snaps, n_snaps, d_contact || d_ncon || d_geom_frc || d_unconverged, "four", d_ctrl, d_unconverged, l);
    if (rc) return rc;
    const PassKernel<CtArgs> kernel = h->ka.pair ? pass_kernel<CtArgs, true>() : pass_kernel<CtArgs, false>();
    if (!kernel) return fail(JB_E_INVALID, "JB_DEV_ONLY4 build: only the contact pass without the pair contacts");
    RoctxRange range("jb_contacts");
    CtArgs f;
    f.p = l.p;
    f.img = (int)((l.lds_bytes + 15) / 16 * 4);
    f.contact = d_contact; f.geom_frc = d_geom_frc; f.ncon = d_ncon;
    hipLaunchKernelGGL(kernel, l.grid, dim3(64), ((size_t)f.img + CT_LDS_FLOATS) * sizeof(float), h->stream, l.a, f);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
int jb_contacts(jb_handle* h, const float* ctrl, float* contact, int32_t* ncon, float* geom_frc, uint8_t* unconverged) {
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs, F = sizeof(float) * N;
    StagePart part[] = {{contact, F * CT_TABLE}, {geom_frc, F * CT_GEOMF}, {const_cast<float*>(ctrl), F, true}, {ncon, sizeof(int32_t) * N}, {unconverged, N}};
    int rc = check_pass(h, "jb_contacts", nullptr, 1, contact || ncon || geom_frc || unconverged, "four");
    if (!rc) rc = stage_parts(h, h->d_contacts_stage, part, "the contact pass");
    if (!rc) rc = jb_contacts_device(h, nullptr, 1, part[2].dev<float>(), part[0].dev<float>(), part[3].dev<int32_t>(), part[1].dev<float>(), part[4].dev<uint8_t>());
    return rc ? rc : fetch_parts(h, part);
}
// The inertia pass (jb_inertia.hpp): the readout's launch - n_snaps * N env-states, a quad of lanes each, one kernel for every handle; reads
// the state and the actions, writes only its outputs.
static_assert(JB_NJAC == IN_NJAC && FW_NV == IN_NV, "the header states the Jacobian's shape");
int jb_inertia_device(jb_handle* h, const void* d_snaps, int32_t n_snaps, const float* d_ctrl, float* d_qM, float* d_qfrc, float* d_qacc_smooth, float* d_jac) {
    JB_ENTER(h);
    InArgs a;
    int rc = check_pass(h, "jb_inertia_device", d_snaps, n_snaps, d_qM || d_qfrc || d_qacc_smooth || d_jac, "four", &a.first);
    if (rc) return rc;
    RoctxRange range("jb_inertia");
    const int N = h->cfg.n_envs;
    a.stride_words = (long long)SNAP_WORDS * N;
    a.total = (long long)n_snaps * N;
    a.tab = h->ka.lane_model; a.n_tab = h->ka.per_env_model ? N : 1;
    a.ctrl = d_ctrl;
    a.qM = d_qM; a.qfrc = d_qfrc; a.qacc = d_qacc_smooth; a.jac = d_jac;
    a.vec4 = ((((uintptr_t)d_qM | (uintptr_t)d_qfrc | (uintptr_t)d_qacc_smooth | (uintptr_t)d_jac) & 15u) == 0) ? 1 : 0;
    const long long blocks = (a.total + RO_EPB - 1) / RO_EPB;
    rc = check_grid("jb_inertia_device", blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(jb_inertia_kernel, dim3((unsigned)blocks), dim3(64), 0, h->stream, a);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
int jb_inertia(jb_handle* h, const float* ctrl, float* qM, float* qfrc, float* qacc_smooth, float* jac) {
    JB_ENTER(h);
    const size_t F = sizeof(float) * (size_t)h->cfg.n_envs;
    StagePart part[] = {{jac, F * IN_JAC}, {qM, F * IN_QM}, {qfrc, F * IN_QFRC}, {qacc_smooth, F * IN_QACC}, {const_cast<float*>(ctrl), F, true}};
    int rc = check_pass(h, "jb_inertia", nullptr, 1, qM || qfrc || qacc_smooth || jac, "four");
    if (!rc) rc = stage_parts(h, h->d_inertia_stage, part, "the inertia pass");
    if (!rc) rc = jb_inertia_device(h, nullptr, 1, part[4].dev<float>(), part[1].dev<float>(), part[2].dev<float>(), part[3].dev<float>(), part[0].dev<float>());
    return rc ? rc : fetch_parts(h, part);
}
// The evaluate pass (jb_evaluate.hpp): the readout's launch - n_snaps * N env-states, a quad of lanes each, one kernel for every handle; reads
// the state and the targets, writes only its outputs.  What it refuses about the task, before anything is launched; *task: the task evaluated.
static int check_evaluate_task(jb_handle* h, const std::string& fn, int task_id, bool has_targets, int* task) {
    if (task_id < -1 || task_id > 4) return fail(JB_E_INVALID, fn + ": task_id " + std::to_string(task_id) + " is outside -1 .. 4");
    if (task_id != -1 && task_id != h->cfg.task_id && !has_targets)
        return fail(JB_E_INVALID, fn + ": a task other than the handle's own needs explicit targets (the stored target's meaning differs by task)");
    *task = task_id < 0 ? h->cfg.task_id : task_id;
    return JB_OK;
}
int jb_evaluate_device(jb_handle* h, const void* d_snaps, int32_t n_snaps, int32_t task_id, const float* d_targets, float* d_obs, float* d_reward, float* d_terms, float* d_achieved) {
    JB_ENTER(h);
    EvArgs a;
    int rc = check_pass(h, "jb_evaluate_device", d_snaps, n_snaps, d_obs || d_reward || d_terms || d_achieved, "four", &a.first);
    if (!rc) rc = check_evaluate_task(h, "jb_evaluate_device", task_id, d_targets != nullptr, &a.task);
    if (rc) return rc;
    RoctxRange range("jb_evaluate");
    const int N = h->cfg.n_envs;
    a.stride_words = (long long)SNAP_WORDS * N;
    a.total = (long long)n_snaps * N;
    a.tab = h->ka.lane_model; a.n_tab = h->ka.per_env_model ? N : 1;
    a.targets = d_targets;
    a.obs = d_obs; a.reward = d_reward; a.terms = d_terms; a.achieved = d_achieved;
    const long long blocks = (a.total + RO_EPB - 1) / RO_EPB;
    rc = check_grid("jb_evaluate_device", blocks);
    if (rc) return rc;
    hipLaunchKernelGGL(jb_evaluate_kernel, dim3((unsigned)blocks), dim3(64), 0, h->stream, a);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
int jb_evaluate(jb_handle* h, int32_t task_id, const float* targets, float* obs, float* reward, float* terms, float* achieved) {
    JB_ENTER(h);
    const size_t F = sizeof(float) * (size_t)h->cfg.n_envs;
    int task = 0;
    int rc = check_pass(h, "jb_evaluate", nullptr, 1, obs || reward || terms || achieved, "four");
    if (!rc) rc = check_evaluate_task(h, "jb_evaluate", task_id, targets != nullptr, &task);
    if (rc) return rc;
    StagePart part[] = {{obs, F * (size_t)obs_dim(task)}, {reward, F}, {terms, F * EV_TERMS}, {achieved, F * EV_GOAL}, {const_cast<float*>(targets), F * EV_GOAL, true}};
    rc = stage_parts(h, h->d_evaluate_stage, part, "the evaluate pass");
    if (!rc) rc = jb_evaluate_device(h, nullptr, 1, task, part[4].dev<float>(), part[0].dev<float>(), part[1].dev<float>(), part[2].dev<float>(), part[3].dev<float>());
    return rc ? rc : fetch_parts(h, part);
}
// how long each wave of the last step launch lived, in seconds (s_memrealtime, 100 MHz): out[0 .. n_waves); returns the number of waves
int jb_wave_clocks(jb_handle* h, double* out, int32_t max_waves) {
    if (!h || !out) return fail(JB_E_INVALID, "handle/out is NULL");
    JB_ENTER(h);
    const int waves = (h->cfg.n_envs + h->ka.epw - 1) / h->ka.epw;
    if (!h->d_wave_clock) return fail(JB_E_INVALID, "no step has been launched yet");
    JB_HIP(hipStreamSynchronize(h->stream));
    std::vector<unsigned long long> t((size_t)waves);
    JB_HIP(hipMemcpy(t.data(), h->d_wave_clock.get(), sizeof(unsigned long long) * (size_t)waves, hipMemcpyDeviceToHost));
    for (int i = 0; i < waves && i < max_waves; i++) out[i] = (double)t[(size_t)i] * 1e-8;
    return waves;
}
int jb_observe_device(jb_handle* h, float* d_obs_out, float* d_reward_out) {
    JB_ENTER(h);
    hipLaunchKernelGGL(jb_observe_kernel, grid_lanes(h->cfg.n_envs), dim3(64), 0, h->stream, h->ka, d_obs_out, d_reward_out);
    JB_HIP(hipGetLastError());
    return JB_OK;
}

int jb_reset(jb_handle* h, const uint8_t* mask, float* obs_out) {
    JB_ENTER(h);
    if (h->async_pending) return fail(JB_E_INVALID, "jb_reset: a jb_step_async is pending (jb_step_wait first)");
    const size_t N = (size_t)h->cfg.n_envs;
    if (mask) JB_HIP(hipMemcpyAsync(h->d_mask.get(), mask, N, hipMemcpyHostToDevice, h->stream));
    int rc = jb_reset_device(h, mask ? h->d_mask.get() : nullptr, obs_out ? h->d_obs.get() : nullptr);
    if (rc) return rc;
    if (obs_out) JB_HIP(hipMemcpyAsync(obs_out, h->d_obs.get(), sizeof(float) * N * h->D, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}
int jb_step(jb_handle* h, const float* action, float* obs_out, float* reward_out, uint8_t* done_out) {
    if (!h || !action) return fail(JB_E_INVALID, "handle/action is NULL");
    JB_ENTER(h);
    if (h->async_pending) return fail(JB_E_INVALID, "jb_step: a jb_step_async is pending (jb_step_wait first)");
    RoctxRange range("jb_step_host_buffers");
    const size_t N = (size_t)h->cfg.n_envs;
    JB_HIP(hipMemcpyAsync(h->d_action.get(), action, sizeof(float) * N, hipMemcpyHostToDevice, h->stream));
    int rc = jb_step_device(h, h->d_action.get(), h->d_obs.get(), h->d_reward.get(), h->d_done.get());
    if (rc) return rc;
    if (obs_out) JB_HIP(hipMemcpyAsync(obs_out, h->d_obs.get(), sizeof(float) * N * h->D, hipMemcpyDeviceToHost, h->stream));
    if (reward_out) JB_HIP(hipMemcpyAsync(reward_out, h->d_reward.get(), sizeof(float) * N, hipMemcpyDeviceToHost, h->stream));
    if (done_out) JB_HIP(hipMemcpyAsync(done_out, h->d_done.get(), N, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}
// jb_step in two halves (header: the VecEnv's step_async / step_wait).  Pinned staging: a copy from or to pageable memory would make
// hipMemcpyAsync wait for the stream; with pinned buffers the call returns as soon as the four operations are queued.
int jb_step_async(jb_handle* h, const float* action) {
    if (!h || !action) return fail(JB_E_INVALID, "handle/action is NULL");
    JB_ENTER(h);
    if (h->async_pending) return fail(JB_E_INVALID, "jb_step_async: the previous step has not been waited for (jb_step_wait)");
    const size_t N = (size_t)h->cfg.n_envs;
    jb_handle::AsyncStage& a = h->async;
    if (!a.copied) {          // all or nothing: the handle takes the staging once every buffer and the event exist
        jb_handle::AsyncStage fresh;
        JB_HIP(fresh.action.alloc(N)); JB_HIP(fresh.obs.alloc(N * h->D)); JB_HIP(fresh.reward.alloc(N)); JB_HIP(fresh.done.alloc(N));
        JB_HIP(fresh.copied.alloc(1));
        a = std::move(fresh);
    }
    RoctxRange range("jb_step_async");
    std::memcpy(a.action.get(), action, sizeof(float) * N);
    JB_HIP(hipMemcpyAsync(h->d_action.get(), a.action.get(), sizeof(float) * N, hipMemcpyHostToDevice, h->stream));
    int rc = jb_step_device(h, h->d_action.get(), h->d_obs.get(), h->d_reward.get(), h->d_done.get());
    if (rc) return rc;
    JB_HIP(hipMemcpyAsync(a.obs.get(), h->d_obs.get(), sizeof(float) * N * h->D, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipMemcpyAsync(a.reward.get(), h->d_reward.get(), sizeof(float) * N, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipMemcpyAsync(a.done.get(), h->d_done.get(), N, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipEventRecord(a.copied.get(), h->stream));
    h->async_pending = true;
    return JB_OK;
}
int jb_step_wait(jb_handle* h, float* obs_out, float* reward_out, uint8_t* done_out) {
    if (!h) return fail(JB_E_INVALID, "handle is NULL");
    if (!h->async_pending) return fail(JB_E_INVALID, "jb_step_wait: no jb_step_async is pending");
    JB_ENTER(h);
    h->async_pending = false;          // (whatever happens below, the pairing async -> wait is used up)
    JB_HIP(hipEventSynchronize(h->async.copied.get()));
    const size_t N = (size_t)h->cfg.n_envs;
    if (obs_out) std::memcpy(obs_out, h->async.obs.get(), sizeof(float) * N * h->D);
    if (reward_out) std::memcpy(reward_out, h->async.reward.get(), sizeof(float) * N);
    if (done_out) std::memcpy(done_out, h->async.done.get(), N);
    return JB_OK;
}
int jb_step_views(jb_handle* h, const float** obs, const float** reward, const uint8_t** done) {
    if (!h) return fail(JB_E_INVALID, "handle is NULL");
    if (!h->async.copied) return fail(JB_E_INVALID, "jb_step_views: no jb_step_async yet (the pinned buffers come into being with the first one)");
    if (obs) *obs = h->async.obs.get();
    if (reward) *reward = h->async.reward.get();
    if (done) *done = h->async.done.get();
    return JB_OK;
}
int jb_observe(jb_handle* h, float* obs_out, float* reward_out) {
    if (!h || !obs_out) return fail(JB_E_INVALID, "handle/obs_out is NULL");
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs;
    int rc = jb_observe_device(h, h->d_obs.get(), reward_out ? h->d_reward.get() : nullptr);
    if (rc) return rc;
    JB_HIP(hipMemcpyAsync(obs_out, h->d_obs.get(), sizeof(float) * N * h->D, hipMemcpyDeviceToHost, h->stream));
    if (reward_out) JB_HIP(hipMemcpyAsync(reward_out, h->d_reward.get(), sizeof(float) * N, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}
int jb_policy_device(jb_handle* h, const float* d_obs, float* d_action) {
    if (!h || !d_obs || !d_action) return fail(JB_E_INVALID, "handle/obs/action is NULL");
    JB_ENTER(h);
    const int N = h->cfg.n_envs;
    hipLaunchKernelGGL(jb_policy_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, N, h->cfg.task_id, h->policy, d_obs, d_action);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
// K control steps of "heuristic policy -> step" (the loop of the reference's benchmarks/evaluate_policy.py:29-33, for every env of the
// batch at once) in ONE launch: the policy is evaluated in the step kernel on the observation the lanes just produced (step 0: on the
// caller's rows).  d_rewards (nullable): [K, N] per-step rewards.
int jb_rollout_policy_device(jb_handle* h, int32_t n_steps, float* d_obs_inout /*[N,D]: current observations in, last out*/,
                             float* d_rewards /*[K,N] nullable*/, uint8_t* d_done_last /*[N] nullable*/) {
    if (!h || !d_obs_inout || n_steps < 0) return fail(JB_E_INVALID, "handle/obs is NULL or n_steps < 0");
    if (n_steps == 0) return JB_OK;
    StepIO io = StepIO();
    io.n_steps = n_steps; io.use_policy = 1; io.obs_in = d_obs_inout;
    io.obs_out = d_obs_inout;
    io.reward_out = d_rewards ? d_rewards : h->d_reward.get(); io.every_step = d_rewards ? 2 : 0;
    io.done_out = d_done_last ? d_done_last : h->d_done.get();
    return launch_step(h, io, 0);
}
int jb_rollout_policy(jb_handle* h, int32_t n_steps, float* rewards_out /*[K,N] host, nullable*/, float* obs_out /*[N,D] host, nullable*/) {
    if (!h || n_steps < 0) return fail(JB_E_INVALID, "handle is NULL or n_steps < 0");
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs;
    const bool want_rew = rewards_out && n_steps > 0;
    if (want_rew) { int rc0 = grow_stage(h, h->d_rew_stage, N * (size_t)n_steps, "the rewards"); if (rc0) return rc0; }
    int rc = jb_observe_device(h, h->d_obs.get(), nullptr);
    if (!rc) rc = jb_rollout_policy_device(h, n_steps, h->d_obs.get(), want_rew ? h->d_rew_stage.get() : nullptr, nullptr);
    if (!rc && want_rew && hipMemcpyAsync(rewards_out, h->d_rew_stage.get(), sizeof(float) * N * (size_t)n_steps, hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = fail(JB_E_HIP, "copy of rewards failed");
    if (!rc && obs_out && hipMemcpyAsync(obs_out, h->d_obs.get(), sizeof(float) * N * h->D, hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = fail(JB_E_HIP, "copy of observations failed");
    hipError_t e = hipStreamSynchronize(h->stream);
    if (!rc && e != hipSuccess) rc = fail(JB_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
}
int jb_policy(jb_handle* h, const float* obs, float* action) {
    if (!h || !obs || !action) return fail(JB_E_INVALID, "handle/obs/action is NULL");
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs;
    JB_HIP(hipMemcpyAsync(h->d_obs.get(), obs, sizeof(float) * N * h->D, hipMemcpyHostToDevice, h->stream));
    int rc = jb_policy_device(h, h->d_obs.get(), h->d_action.get());
    if (rc) return rc;
    JB_HIP(hipMemcpyAsync(action, h->d_action.get(), sizeof(float) * N, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}
int jb_set_policy_params(jb_handle* h, float kick_angle, float speed, float angle_threshold) {
    if (!h) return fail(JB_E_INVALID, "handle is NULL");
    if (!(kick_angle >= 0.f) || !(angle_threshold >= 0.f) || !std::isfinite(speed)) return fail(JB_E_INVALID, "policy parameters: kick_angle, angle_threshold >= 0 and a finite speed");
    h->policy.kick_angle = kick_angle; h->policy.speed = speed; h->policy.angle_threshold = angle_threshold;
    return JB_OK;
}
int jb_reward_terms_device(jb_handle* h, float* d_terms_out) {
    if (!h || !d_terms_out) return fail(JB_E_INVALID, "handle/terms is NULL");
    JB_ENTER(h);
    hipLaunchKernelGGL(jb_reward_terms_kernel, grid_lanes(h->cfg.n_envs), dim3(64), 0, h->stream, h->ka, d_terms_out);
    JB_HIP(hipGetLastError());
    return JB_OK;
}
int jb_reward_terms(jb_handle* h, float* terms_out) {
    if (!h || !terms_out) return fail(JB_E_INVALID, "handle/terms is NULL");
    JB_ENTER(h);
    int rc = jb_reward_terms_device(h, h->d_terms.get());
    if (rc) return rc;
    JB_HIP(hipMemcpyAsync(terms_out, h->d_terms.get(), sizeof(float) * 4 * (size_t)h->cfg.n_envs, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}
int jb_get_state(jb_handle* h, double* qpos, double* qvel, double* target) {
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs;
    hipLaunchKernelGGL(jb_export_kernel, dim3((unsigned)((N + 127) / 128)), dim3(128), 0, h->stream, h->ka, qpos ? h->d_qpos.get() : nullptr, qvel ? h->d_qvel.get() : nullptr,
                       target ? h->d_target.get() : nullptr);
    JB_HIP(hipGetLastError());
    if (qpos) JB_HIP(hipMemcpyAsync(qpos, h->d_qpos.get(), sizeof(double) * 16 * N, hipMemcpyDeviceToHost, h->stream));
    if (qvel) JB_HIP(hipMemcpyAsync(qvel, h->d_qvel.get(), sizeof(double) * 15 * N, hipMemcpyDeviceToHost, h->stream));
    if (target) JB_HIP(hipMemcpyAsync(target, h->d_target.get(), sizeof(double) * 3 * N, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}
int jb_set_state(jb_handle* h, const double* qpos, const double* qvel, const double* target) {
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs;
    if (qpos) JB_HIP(hipMemcpyAsync(h->d_qpos.get(), qpos, sizeof(double) * 16 * N, hipMemcpyHostToDevice, h->stream));
    if (qvel) JB_HIP(hipMemcpyAsync(h->d_qvel.get(), qvel, sizeof(double) * 15 * N, hipMemcpyHostToDevice, h->stream));
    if (target) JB_HIP(hipMemcpyAsync(h->d_target.get(), target, sizeof(double) * 3 * N, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(jb_import_kernel, dim3((unsigned)((N + 127) / 128)), dim3(128), 0, h->stream, h->ka, qpos ? h->d_qpos.get() : nullptr, qvel ? h->d_qvel.get() : nullptr,
                       target ? h->d_target.get() : nullptr);
    JB_HIP(hipGetLastError());
    JB_HIP(hipStreamSynchronize(h->stream));
    return JB_OK;
}
int jb_get_counters(jb_handle* h, int32_t* step_count, uint32_t* episode, float* solver_cap_hits) {
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs;
    JB_HIP(hipStreamSynchronize(h->stream));
    if (step_count) JB_HIP(hipMemcpy(step_count, h->d_step.get(), sizeof(int) * N, hipMemcpyDeviceToHost));
    if (episode) JB_HIP(hipMemcpy(episode, h->d_episode.get(), sizeof(unsigned) * N, hipMemcpyDeviceToHost));
    if (solver_cap_hits) JB_HIP(hipMemcpy(solver_cap_hits, h->d_root.get() + RF_FAIL * N, sizeof(float) * N, hipMemcpyDeviceToHost));
    return JB_OK;
}
// how often the contact solve needed its second, line-searched pass: wave-substeps since jb_create (jb_sim.hpp newton_phase<LS = true>)
int jb_solver_stats(jb_handle* h, uint64_t* resolved_wave_substeps) {
    if (!h || !resolved_wave_substeps) return fail(JB_E_INVALID, "handle/out is NULL");
    JB_ENTER(h);
    JB_HIP(hipStreamSynchronize(h->stream));
    unsigned long long v = 0;
    JB_HIP(hipMemcpy(&v, h->d_resolve.get(), sizeof v, hipMemcpyDeviceToHost));
    *resolved_wave_substeps = (uint64_t)v;
    return JB_OK;
}
#ifdef JB_CAPTURE
// diagnostic builds only: the captured records (SimOpts::capture), out[max_records][64]; returns how many substeps stayed unconverged
int jb_debug_captured(jb_handle* h, float* out, int32_t max_records) {
    if (!h || !out) return fail(JB_E_INVALID, "NULL");
    JB_HIP(hipStreamSynchronize(h->stream));
    unsigned n = 0;
    JB_HIP(hipMemcpy(&n, h->d_capture_count.get(), sizeof n, hipMemcpyDeviceToHost));
    const int m = (int)n < max_records ? (int)n : max_records;
    JB_HIP(hipMemcpy(out, h->d_capture.get(), sizeof(float) * 64 * (size_t)(m < JB_CAPTURE_SLOTS ? m : JB_CAPTURE_SLOTS), hipMemcpyDeviceToHost));
    return (int)n;
}
#endif
#ifdef JB_WAVE_STATS
// diagnostic builds only: per-wave [cycles, rare-path substeps, Newton sweeps, contact substeps] of the last step launch
int jb_debug_wave_stats(jb_handle* h, unsigned long long* out, int32_t n_waves) {
    if (!h || !out) return fail(JB_E_INVALID, "NULL");
    JB_HIP(hipStreamSynchronize(h->stream));
    JB_HIP(hipMemcpy(out, h->d_wave_stats.get(), sizeof(unsigned long long) * 16 * n_waves, hipMemcpyDeviceToHost));
    return h->ka.epw;
}
#endif
// The witness for the geom pairs the step kernels do not collide (header; jb_witness.hpp): one pass over the current state, results on the host.
int jb_pair_witness(jb_handle* h, float* clearance_out, int32_t* pairs_out, int32_t* n_touching) {
    JB_ENTER(h);
    int rc = ensure_witness(h);
    if (rc) return rc;
    const size_t N = (size_t)h->cfg.n_envs;
    hipLaunchKernelGGL(jb_witness_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, h->stream, h->ka, h->wit.clear.get(), h->wit.pair.get(), (float*)nullptr, (unsigned*)nullptr);
    JB_HIP(hipGetLastError());
    std::vector<float> host(N);
    JB_HIP(hipMemcpyAsync(host.data(), h->wit.clear.get(), sizeof(float) * N, hipMemcpyDeviceToHost, h->stream));
    if (pairs_out) JB_HIP(hipMemcpyAsync(pairs_out, h->wit.pair.get(), sizeof(int) * 2 * N, hipMemcpyDeviceToHost, h->stream));
    JB_HIP(hipStreamSynchronize(h->stream));
    int touching = 0;
    for (size_t i = 0; i < N; i++) { if (!(host[i] > 0.f)) touching++; if (clearance_out) clearance_out[i] = host[i]; }
    if (n_touching) *n_touching = touching;
    return JB_OK;
}
int jb_get_pair_witness(jb_handle* h, uint32_t* overlap_passes, float* min_clearance) {
    JB_ENTER(h);
    if (!(h->cfg.flags & JB_FLAG_PAIR_WITNESS)) return fail(JB_E_INVALID, "jb_get_pair_witness: the handle was created without JB_FLAG_PAIR_WITNESS (jb_pair_witness gives one pass on demand)");
    int rc = ensure_witness(h);
    if (rc) return rc;
    const size_t N = (size_t)h->cfg.n_envs;
    JB_HIP(hipStreamSynchronize(h->stream));
    if (overlap_passes) JB_HIP(hipMemcpy(overlap_passes, h->wit.count.get(), sizeof(unsigned) * N, hipMemcpyDeviceToHost));
    if (min_clearance) JB_HIP(hipMemcpy(min_clearance, h->wit.min.get(), sizeof(float) * N, hipMemcpyDeviceToHost));
    return JB_OK;
}
int jb_set_model_params(jb_handle* h, const double* params, int32_t n_tables) {
    if (!h || !params) return fail(JB_E_INVALID, "handle/params is NULL");
    JB_ENTER(h);
    if (n_tables != 1 && n_tables != h->cfg.n_envs) return fail(JB_E_INVALID, "n_tables must be 1 or n_envs");
    JB_HIP(hipStreamSynchronize(h->stream));
    return upload_model(h, params, n_tables);
}


int jb_default_randomise_config(jb_randomise_cfg* c) {
    if (!c) return fail(JB_E_INVALID, "cfg is NULL");
    std::memset(c, 0, sizeof *c);
    c->flags = JB_RND_LEGS | JB_RND_MASS;                 // what the reference's training harness switches on (benchmarks/benchmark.py:130-136)
    c->max_attempts = 64; c->seed = 0;
    c->sd_legs[0] = 0.003; c->sd_legs[1] = 0.003; c->sd_legs[2] = 0.002;                    // reference augmented_jitterbug.py:96
    c->sd_mass_pos[0] = 0.0015; c->sd_mass_pos[1] = 0.002; c->sd_mass_pos[2] = 0.001;      // :98
    c->sd_core1_density = 10.0; c->sd_core2_density = 80.0; c->sd_global_density = 200.0; c->sd_gear = 0.001;     // :100-107
    c->min_mass_clearance = 0.0;
    return JB_OK;
}
int jb_randomise_models(jb_handle* h, const jb_randomise_cfg* cfg, const double* offsets_in, double* params_out, double* offsets_out, int32_t* attempts_out) {
    if (!h || !cfg) return fail(JB_E_INVALID, "handle/cfg is NULL");
    JB_ENTER(h);
    const size_t N = (size_t)h->cfg.n_envs;
    // one model per env runs the PAIR kernel: refuse up front what JB_FLAG_LEAN cannot run (see check_variant)
    const int pair = (h->cfg.flags & JB_FLAG_NO_PAIR) ? 0 : 1;
    { int rc = check_variant(h->ka.lean, pair, 1, h->ka.epw); if (rc) return rc; }
    JB_HIP(hipStreamSynchronize(h->stream));
    if (!h->d_spec) {
        Dev<JbNominalSpec> spec;
        JB_HIP(spec.alloc(1)); JB_HIP(hipMemcpy(spec.get(), &JB_NOMINAL_SPEC, sizeof(JbNominalSpec), hipMemcpyHostToDevice));
        h->d_spec = std::move(spec);
    }
    // The tables are generated into a FRESH buffer and installed only after the kernel succeeded: a failure on the way (the 5 KB x N
    // params_out allocation is the likeliest) leaves the handle on the model it had, never on freed or half-written tables.
    Dev<float> d_tables;
    Dev<double> d_off_in, d_par, d_off_out;
    Dev<int> d_att, d_status;
    JB_HIP(d_tables.alloc(N * LM_TABLE));
    JB_HIP(d_status.alloc(1));
    JB_HIP(hipMemset(d_status.get(), 0, sizeof(int)));
    if (offsets_in) { JB_HIP(d_off_in.alloc(N * AO_COUNT)); JB_HIP(hipMemcpy(d_off_in.get(), offsets_in, sizeof(double) * N * AO_COUNT, hipMemcpyHostToDevice)); }
    if (params_out) JB_HIP(d_par.alloc(N * JB_NPARAM));
    if (offsets_out) JB_HIP(d_off_out.alloc(N * AO_COUNT));
    if (attempts_out) JB_HIP(d_att.alloc(N));
    RndArgs a;
    a.n = (int)N; a.flags = cfg->flags; a.max_attempts = cfg->max_attempts > 0 ? cfg->max_attempts : 64;
    a.seed = cfg->seed; a.env_offset = h->cfg.env_offset;
    for (int i = 0; i < 3; i++) { a.sd.legs[i] = cfg->sd_legs[i]; a.sd.mass_pos[i] = cfg->sd_mass_pos[i]; }
    a.sd.core1_density = cfg->sd_core1_density; a.sd.core2_density = cfg->sd_core2_density; a.sd.global_density = cfg->sd_global_density; a.sd.gear = cfg->sd_gear;
    a.min_mass_clearance = cfg->min_mass_clearance;
    a.spec = h->d_spec.get(); a.offsets_in = d_off_in.get(); a.tables = d_tables.get(); a.params_out = d_par.get(); a.offsets_out = d_off_out.get();
    a.attempts_out = d_att.get(); a.status = d_status.get();
    hipLaunchKernelGGL(jb_randomise_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, h->stream, a);
    JB_HIP(hipGetLastError());
    JB_HIP(hipStreamSynchronize(h->stream));
    int status = 0;
    JB_HIP(hipMemcpy(&status, d_status.get(), sizeof(int), hipMemcpyDeviceToHost));
    if (status != 0)      // the handle keeps the model it had
        return fail(JB_E_MODEL, status == -30 ? "randomise: no draw cleared min_mass_clearance within max_attempts for some env" : "randomise: a generated model is not supported by the kernel (code " + std::to_string(status) + ")");
    if (params_out) JB_HIP(hipMemcpy(params_out, d_par.get(), sizeof(double) * N * JB_NPARAM, hipMemcpyDeviceToHost));
    if (offsets_out) JB_HIP(hipMemcpy(offsets_out, d_off_out.get(), sizeof(double) * N * AO_COUNT, hipMemcpyDeviceToHost));
    if (attempts_out) JB_HIP(hipMemcpy(attempts_out, d_att.get(), sizeof(int) * N, hipMemcpyDeviceToHost));
    install_model(h, std::move(d_tables), 1, pair);      // (the stream is idle: synchronised above)
    return JB_OK;
}
// host-only helpers (no GPU): the native compiler / validity check on ONE model - what the device kernel runs per env
int jb_model_compile_host(const double* offsets, int32_t flags, double* params_out) {
    if (!params_out) return fail(JB_E_INVALID, "params_out is NULL");
    JbNominalSpec S;
    double zero[AO_COUNT] = {0};
    apply_offsets(JB_NOMINAL_SPEC, offsets ? flags : 0, offsets ? offsets : zero, S);
    const int rc = compile_model(S, params_out);
    return rc ? fail(JB_E_MODEL, "model does not compile (code " + std::to_string(rc) + ")") : JB_OK;
}
int jb_model_mass_clearance_ok(const double* params, double margin) {
    if (!params) return fail(JB_E_INVALID, "params is NULL");
    return mass_sweep_clear(params, margin) ? 1 : 0;
}
int jb_model_draw_offsets_host(uint64_t seed, uint64_t env, uint32_t attempt, const jb_randomise_cfg* cfg, double* offsets_out) {
    if (!cfg || !offsets_out) return fail(JB_E_INVALID, "cfg/offsets_out is NULL");
    AugSigmas sd;
    for (int i = 0; i < 3; i++) { sd.legs[i] = cfg->sd_legs[i]; sd.mass_pos[i] = cfg->sd_mass_pos[i]; }
    sd.core1_density = cfg->sd_core1_density; sd.core2_density = cfg->sd_core2_density; sd.global_density = cfg->sd_global_density; sd.gear = cfg->sd_gear;
    draw_offsets(seed, env, attempt, cfg->flags, sd, offsets_out);
    return JB_OK;
}


// ---- rows between GPUs without Python: one RCCL communicator per handle (gather of [N_local, D+2] rows to rank 0;
// on 8 MI355X that is 7 concurrent single-hop xGMI sends, not a ring)
int jb_comm_unique_id(void* id_out) {
    if (!id_out) return fail(JB_E_INVALID, "id_out is NULL");
    int rc = load_rccl();
    if (rc) return rc;
    JB_NCCL(g_rccl.GetUniqueId(id_out));
    return JB_OK;
}
int jb_comm_init(jb_handle* h, int32_t n_ranks, int32_t rank, const void* id) {
    if (!h || !id) return fail(JB_E_INVALID, "handle/id is NULL");
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(JB_E_INVALID, "need 0 <= rank < n_ranks");
    if (h->comm) return fail(JB_E_INVALID, "the handle already has a communicator (jb_comm_destroy first)");
    JB_ENTER(h);
    int rc = load_rccl();
    if (rc) return rc;
    RcclApi::IdBlob blob;
    std::memcpy(blob.b, id, sizeof blob.b);
    JB_NCCL(g_rccl.CommInitRank(&h->comm, n_ranks, blob, rank));
    h->comm_ranks = n_ranks; h->comm_rank = rank; h->comm_nmax = 0;
    return JB_OK;
}
int jb_comm_set_shards(jb_handle* h, const int32_t* shard_envs) {
    if (!h || !shard_envs) return fail(JB_E_INVALID, "handle/shard_envs is NULL");
    if (!h->comm) return fail(JB_E_INVALID, "no communicator (jb_comm_init)");
    int nmax = 0;
    for (int r = 0; r < h->comm_ranks; r++) {
        if (shard_envs[r] < 1) return fail(JB_E_INVALID, "shard_envs[" + std::to_string(r) + "] < 1");
        nmax = shard_envs[r] > nmax ? shard_envs[r] : nmax;
    }
    if (shard_envs[h->comm_rank] != h->cfg.n_envs)
        return fail(JB_E_INVALID, "shard_envs[" + std::to_string(h->comm_rank) + "] = " + std::to_string(shard_envs[h->comm_rank]) + " but this handle steps " + std::to_string(h->cfg.n_envs) +
                                  " envs: the ranks do not agree on the partition");
    h->comm_nmax = nmax;
    return JB_OK;
}
int jb_comm_destroy(jb_handle* h) {
    if (!h) return fail(JB_E_INVALID, "handle is NULL");
    // the exchanges run on streams of the caller's choosing (ShardedJitterbugEnv: a side stream): wait for the whole device, not just the handle's stream
    if (h->comm) { JB_ENTER(h); hipDeviceSynchronize(); JB_NCCL(g_rccl.CommDestroy(h->comm)); h->comm = nullptr; h->comm_nmax = 0; }
    return JB_OK;
}
// The grouped exchange with rank 0 behind the gathers and the scatter, `count` floats per rank: rank 0 exchanges block r of `all`
// [n_ranks, count] with rank r, and every rank its own block `mine` with rank 0 - a gather sends `mine` and rank 0 receives into `all`,
// a scatter the reverse.  A failed Send/Recv must not leave the RCCL group open: the group is closed, then the first error is reported.
static int rccl_exchange(jb_handle* h, bool gather, const float* all, const float* mine, size_t count, void* stream, int32_t use_stream, const char* what) {
    hipStream_t st = use_stream ? (hipStream_t)stream : h->stream;
    JB_NCCL(g_rccl.GroupStart());
    int err = 0;
    if (h->comm_rank == 0)
        for (int r = 0; r < h->comm_ranks && !err; r++)      // (const_cast: the receiving side of a gather)
            err = gather ? g_rccl.Recv(const_cast<float*>(all) + (size_t)r * count, count, 7 /*ncclFloat*/, r, h->comm, st) : g_rccl.Send(all + (size_t)r * count, count, 7 /*ncclFloat*/, r, h->comm, st);
    if (!err) err = gather ? g_rccl.Send(mine, count, 7 /*ncclFloat*/, 0, h->comm, st) : g_rccl.Recv(const_cast<float*>(mine), count, 7 /*ncclFloat*/, 0, h->comm, st);
    const int end = g_rccl.GroupEnd();
    if (err || end) return fail(JB_E_HIP, std::string(what) + (g_rccl.GetErrorString ? g_rccl.GetErrorString(err ? err : end) : "RCCL error"));
    return JB_OK;
}
// the same exchange for a block of `count` floats per rank (equal on every rank): what a fused K-step rollout returns, [K, N_local, D+2]
int jb_gather_block_device(jb_handle* h, const float* d_src, float* d_all, int64_t count, void* stream, int32_t use_stream) {
    if (!h || !d_src || count < 1) return fail(JB_E_INVALID, "handle/src is NULL or count < 1");
    if (!h->comm) return fail(JB_E_INVALID, "no communicator (jb_comm_init)");
    if (h->comm_rank == 0 && !d_all) return fail(JB_E_INVALID, "rank 0 needs the receive buffer [n_ranks, count]");
    JB_ENTER(h);
    RoctxRange range("jb_gather_block");
    return rccl_exchange(h, true, d_all, d_src, (size_t)count, stream, use_stream, "RCCL block gather: ");
}
int jb_gather_rows_device(jb_handle* h, const float* d_rows, float* d_all, void* stream, int32_t use_stream) {
    if (!h || !d_rows) return fail(JB_E_INVALID, "handle/rows is NULL");
    if (!h->comm) return fail(JB_E_INVALID, "no communicator (jb_comm_init)");
    if (h->comm_rank == 0 && !d_all) return fail(JB_E_INVALID, "rank 0 needs the receive buffer [n_ranks, N_local, D+2]");
    JB_ENTER(h);
    RoctxRange range("jb_gather_rows");
    // every rank posts blocks of the longest shard (jb_comm_set_shards; without it the shards are equal by contract)
    const size_t count = (size_t)(h->comm_nmax > 0 ? h->comm_nmax : h->cfg.n_envs) * (size_t)(h->D + 2);
    return rccl_exchange(h, true, d_all, d_rows, count, stream, use_stream, "RCCL row gather: ");
}
int jb_scatter_actions_device(jb_handle* h, const float* d_all, float* d_local, int64_t count, void* stream, int32_t use_stream) {
    if (!h || !d_local || count < 1) return fail(JB_E_INVALID, "handle/local is NULL or count < 1");
    if (!h->comm) return fail(JB_E_INVALID, "no communicator (jb_comm_init)");
    if (h->comm_rank == 0 && !d_all) return fail(JB_E_INVALID, "rank 0 needs the send buffer [n_ranks, count]");
    if (count < (int64_t)h->cfg.n_envs || (h->comm_nmax > 0 && count != (int64_t)h->comm_nmax))
        return fail(JB_E_INVALID, "jb_scatter_actions_device: count must be the longest shard's envs (" + std::to_string(h->comm_nmax > 0 ? h->comm_nmax : h->cfg.n_envs) + "), the same on every rank");
    JB_ENTER(h);
    RoctxRange range("jb_scatter_actions");
    return rccl_exchange(h, false, d_all, d_local, (size_t)count, stream, use_stream, "RCCL action scatter: ");
}

}  // extern "C"

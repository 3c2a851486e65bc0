// jb_variant.hpp — a step-kernel variant, described once.
//
// A variant is (envs per wave, LEAN, PAIR).  Everything that follows from those three - how the wave's lanes are grouped, what the
// per-lane scratch holds and where, the bytes of dynamic LDS, the waves resident per SIMD, which combinations have a kernel at all -
// is stated here and read by the kernel (jb_api.hip step_body), by the launcher (launch_step) and by the host harness of the tests
// (tests/host_harness.cpp).  A new variant, or a change of an existing one's layout, starts in this file.
#pragma once
#include "../../include/jitterbug_hip.h"
#include "jb_sim.hpp"

namespace jb {

// LEAN kernels' per-wave block in global memory, floats per main lane: the overflow candidates, then the second pair contact's frame
constexpr int OVC_FLOATS_PER_LANE = 4 * (NSLOT - ROW_K) + 9;

struct StepLayout {
    int epw;                 // environments per wave
    bool lean, pair;
    int main_lanes;          // lanes 0 .. main_lanes-1: quad q = env q of the wave, lane = leg
    int groups;              // lane groups: the main lanes and groups-1 helper groups that mirror them (jb_sim.hpp SlotPlan)
    bool offload;            // lane group 1 replicates the main lanes (SimOpts::offload)
    bool aux;                // lane groups 2 and 3 run phase A on the motor body and the root body's own mass (SimOpts::aux)
    bool split_tables;       // only the entries of the common path are staged per env (LaneConsts split mode): LEAN + PAIR, one model per env
    int scratch_floats;      // per-lane scratch (SC_COUNT*)
    bool pair_entries;       // the staged constant table carries the pair contact's entries, its tail (without them only where LDS is short: LEAN without PAIR)
    int table_floats;        // the staged prefix of a packed constant table (not with split tables)
    int pd, pd2;             // LaneScratch::pd, ::pd2
    bool red_lds;            // LaneScratch::red_lds; also: the overflow candidates sit in the scratch (false: in the global block below)
    int ovc_floats;          // floats per main lane of the wave's block in global memory (0: none)
    int waves_per_simd;      // resident waves per SIMD (the register budget the kernel is compiled for)
    bool fused_row_build;    // the first full Newton sweep of a substep builds the contact rows it applies (SimOpts::fuse_rows); false: the rows are
                             // built in a pass of their own before the solve - the rows whose register budget the fused sweep does not fit (it
                             // adds scratch operations to their substep loop's hot part: tools/asm_spills.py).  Same bits either way.
    bool every_lane_update;  // the iterate's update after star_solve is made by every lane, not under the main lanes' predicate (SimOpts::every_lane_update,
                             // tools/experiments/group_liveness.txt); false: the two rows whose hot part it would give scratch operations.  Same bits.
    bool scalar_votes;       // the wave-uniform decisions of the Newton loop's check and of the substep's broadphase are votes of the main lanes taken by every
                             // lane (jb_lane.hpp main_vote, SimOpts::scalar_votes, tools/experiments/scalar_votes.txt); false: under the main lanes'
                             // predicate and fetched back from the first lane - the rows that would gain a hot scratch operation or lose occupancy,
                             // and every row with -DJB_VECTOR_VOTES (today no row objects).  Same bits.
    bool stage_major;        // the transposed group reduction of a full Newton sweep runs its quadruples in batches, stage by stage (LaneScratch::stage_major,
                             // jb_sim.hpp contact_sweep, tools/experiments/wait_states.txt): an add is followed by another quadruple's swap, not by the
                             // wait states in front of its own.  Only the rows that take that reduction - four lane groups 16 lanes apart, the totals
                             // handed over through the scratch - have the choice, and the PAIR row among them keeps the old order: with both new orders
                             // its hot part grows by two instructions, with the term-major one alone it is shortest.  False everywhere with
                             // -DJB_ELEMENT_MAJOR_ORDER, the reference form.  Same bits.
    bool term_major;         // the packed accumulations of a contact - the root block's fifteen accumulators (jb_sim.hpp acc_root), the three rows' residuals
                             // (row_residuals) - run term by term over all accumulators, so that no packed multiply-add reads the result of the one in
                             // front of it (LaneScratch::term_major); false: one accumulator after the other - the one row whose hot part the new order
                             // gives scratch operations, and every row with -DJB_ELEMENT_MAJOR_ORDER.  Same bits.
    bool late_env_index;     // the kernel's closing stores form their addresses from a fresh copy of the env index, so that no byte offset of the
                             // entry's loads stays in registers through the loops (jb_api.hip step_body); it comes with the scalar votes - whose
                             // flagship row would otherwise spill that offset once per launch - except on the one row it gives hot scratch operations
};

constexpr StepLayout step_layout(int epw, bool lean, bool pair) {
    StepLayout l = StepLayout();
    l.epw = epw; l.lean = lean; l.pair = pair;
    l.main_lanes = 4 * epw;
    l.groups = epw == 8 ? 2 : 4;
    l.offload = !lean;
    l.aux = !lean && !pair && l.groups == 4;
    l.split_tables = lean && pair;
    l.scratch_floats = lean ? (pair ? SC_COUNT_LEAN_PAIR : SC_COUNT_LEAN) : SC_COUNT;
    l.pair_entries = pair || !lean;
    l.table_floats = l.pair_entries ? LM_TABLE : LM_TABLE_BASE;
    l.pd = lean ? SC_PD_LEAN : SC_PD;
    l.pd2 = lean ? 4 * (NSLOT - ROW_K) : SC_PD2 - SC_OVC;
    l.red_lds = !lean;
    l.ovc_floats = lean ? OVC_FLOATS_PER_LANE : 0;
    l.waves_per_simd = lean ? 2 : 1;
    l.fused_row_build = !(lean && pair) && !(pair && epw == 1) && !(!pair && !lean && epw == 8);
    l.every_lane_update = !(lean && !pair && epw == 2) && !(!pair && !lean && epw == 8);
#ifdef JB_VECTOR_VOTES
    l.scalar_votes = false;
#else
    l.scalar_votes = true;
#endif
#ifdef JB_ELEMENT_MAJOR_ORDER
    l.stage_major = false; l.term_major = false;
#else
    l.stage_major = l.groups == 4 && l.main_lanes == 16 && l.red_lds && !pair;
    l.term_major = !(pair && !lean && epw == 8);
#endif
    l.late_env_index = l.scalar_votes && !(pair && !lean && epw == 8);
    return l;
}

// dynamic LDS of one wave: [scratch_floats][main_lanes] of scratch, then the constant table(s) - one for a shared model, one per env otherwise -
// each with its aux block behind it (split tables: the resident block of every env)
constexpr size_t step_lds_bytes(const StepLayout& l, bool per_env_model) {
    return l.split_tables ? ((size_t)l.scratch_floats * 4 * l.epw + (size_t)LM_SPLIT_RES * l.epw) * sizeof(float)
                          : ((size_t)l.scratch_floats * 4 * l.epw + ((size_t)l.table_floats + (l.aux ? LM_AUX : 0)) * (per_env_model ? l.epw : 1)) * sizeof(float);
}

// ---- the variants that have a kernel.  JB_FLAG_LEAN is honoured where a LEAN instantiation exists: without the pair contact at 1, 2 or 4 envs
// per wave, or - LEAN + PAIR, split tables - with one model per env at four envs per wave.
struct StepRow {
    int variant;             // JB_VARIANT_*
    int epw;
    bool lean, pair;
    bool per_env_only;       // launched only with one model per env
};
constexpr StepRow STEP_ROWS[] = {
    {JB_VARIANT_LEAN_PAIR, 4, true, true, true},
    {JB_VARIANT_PAIR, 1, false, true, false}, {JB_VARIANT_PAIR, 2, false, true, false}, {JB_VARIANT_PAIR, 4, false, true, false}, {JB_VARIANT_PAIR, 8, false, true, false},
    {JB_VARIANT_LEAN, 1, true, false, false}, {JB_VARIANT_LEAN, 2, true, false, false}, {JB_VARIANT_LEAN, 4, true, false, false},
    {JB_VARIANT_ORDINARY, 1, false, false, false}, {JB_VARIANT_ORDINARY, 2, false, false, false}, {JB_VARIANT_ORDINARY, 4, false, false, false}, {JB_VARIANT_ORDINARY, 8, false, false, false},
};
constexpr int N_STEP_ROWS = (int)(sizeof(STEP_ROWS) / sizeof(STEP_ROWS[0]));
constexpr int STEP_NOT_LAUNCHABLE = -1;

// the row of STEP_ROWS that runs (lean, pair, per_env_model, epw), or STEP_NOT_LAUNCHABLE
constexpr int step_row(bool lean, bool pair, bool per_env_model, int epw) {
    for (int i = 0; i < N_STEP_ROWS; i++)
        if (STEP_ROWS[i].lean == lean && STEP_ROWS[i].pair == pair && STEP_ROWS[i].epw == epw && (per_env_model || !STEP_ROWS[i].per_env_only)) return i;
    return STEP_NOT_LAUNCHABLE;
}
// ... and its JB_VARIANT_* id
constexpr int step_variant(bool lean, bool pair, bool per_env_model, int epw) {
    const int i = step_row(lean, pair, per_env_model, epw);
    return i < 0 ? STEP_NOT_LAUNCHABLE : STEP_ROWS[i].variant;
}

// More waves than the device holds at once (wave_slots SIMDs x waves_per_simd): launch them longest first.  Two waves per SIMD and the whole
// batch resident: no launch ORDER to choose, but who shares a SIMD with whom - the waves from fold_from on are paired with the ones before.
struct WaveOrderPlan { bool reorder; int fold_from; };
constexpr WaveOrderPlan wave_order_plan(int grid, int wave_slots, int waves_per_simd) {
    WaveOrderPlan p = {(long long)grid > (long long)wave_slots * waves_per_simd, 0};
    if (waves_per_simd == 2 && grid > wave_slots && !p.reorder) { p.reorder = true; p.fold_from = wave_slots; }
    return p;
}

// ---- what a lane of group `grp` is handed, for callers that emulate a wave (the kernel states the same inline: its statements stay where the
// register allocator has them).  base: the lane's first scratch float, element i at base[i * stride]; ext_ovc: the lane's first float of the
// block outside the scratch (used when the layout keeps the overflow candidates there).
template <typename V> JB_HD void bind_scratch(LaneScratch<V>& sc, const StepLayout& l, V* base, int stride, int grp, V* ext_ovc) {
    sc.p = base; sc.stride = stride;
    sc.grp = grp; sc.ngrp = l.groups; sc.gstride = l.main_lanes;
    sc.ovc = l.red_lds ? base + SC_OVC * stride : ext_ovc; sc.ovc_stride = stride;
    sc.pd = l.pd; sc.pd2 = l.pd2; sc.red_lds = l.red_lds; sc.stage_major = l.stage_major; sc.term_major = l.term_major;
    sc.aux_lane = l.aux && grp >= 2;
}
// the lanes that hold an env's state: the main lanes, their replica and the aux lanes (the other helper lanes only take part in the substeps)
JB_HD bool holds_state(const StepLayout& l, int grp) { return grp == 0 || (l.offload && grp == 1) || (l.aux && grp >= 2); }
// ... and the harmless state those other helper lanes start from
template <typename V> JB_HD void helper_lane_state(LaneState<V>& s) {
    s.px = s.py = s.pz = V(0.f); s.qw = V(1.f); s.qx = s.qy = s.qz = V(0.f); s.vx = s.vy = s.vz = s.wx = s.wy = s.wz = V(0.f);
    s.pz_lo = s.qw_lo = s.qx_lo = s.qy_lo = s.qz_lo = V(0.f);
    s.phi = s.phid = s.turns = V(0.f); s.th1 = s.th2 = s.thd1 = s.thd2 = V(0.f);
    for (int i = 0; i < 3; i++) { s.wa[i] = V(0.f); s.wl[i] = V(0.f); }
    s.wj[0] = s.wj[1] = V(0.f); s.wm = V(0.f); s.fail = V(0.f);
}
// the substep's options: what the layout fixes, plus the run-time switches
JB_HD SimOpts sim_opts(const StepLayout& l, int contacts, int max_newton, int implicit_damp, int rank_one, int spread) {
    SimOpts o;
    o.contacts = contacts; o.max_newton = max_newton; o.implicit_damp = implicit_damp; o.rank_one = rank_one; o.spread = spread;
    o.lean = l.lean ? 1 : 0; o.offload = l.offload ? 1 : 0; o.aux = l.aux ? 1 : 0; o.fuse_rows = l.fused_row_build ? 1 : 0;
    o.every_lane_update = l.every_lane_update ? 1 : 0; o.scalar_votes = l.scalar_votes ? 1 : 0;
    o.prof = nullptr; o.hist = nullptr;
    return o;
}

}  // namespace jb

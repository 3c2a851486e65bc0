// host_run.hpp — TEST INFRASTRUCTURE.  One env's share of a wave on the host (HostRun): what tests/host_harness.cpp and the harnesses of the
// passes over states (tests/pass_harness.hpp) run the simulator source on.  Never linked into, or loaded by, the product library.
#pragma once
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include "../jitterbug_amd/csrc/jb_model_build.hpp"
#include "../jitterbug_amd/csrc/jb_step.hpp"
#include "../jitterbug_amd/csrc/jb_variant.hpp"

using namespace jb;

// ngroups = 4: the wave layout of the 4-envs-per-wave kernel for ONE env - a main group and three helper groups, one host thread each,
// sharing the scratch and exchanging through jb_lane.hpp's HostWave (group_sum, row_transpose_sum, the rank-one pass on rows other groups
// built, the broadcast loop decisions): the same code paths the device takes with helper lanes.  ngroups = 2: the 8-envs-per-wave kernel's
// two groups.  ngroups = 1: the main lanes alone (the harness's own diagnostic shape).  The layout itself is jb_variant.hpp's.
static int g_offload = 1;      // lane group 1 as the main lanes' replica (SimOpts::offload), as the one-wave-per-SIMD kernels run it
static int g_aux = 1;          // aux bodies on lane groups 2 / 3 (SimOpts::aux)
static int g_spread = 1;       // spread contact sweeps (SimOpts::spread)

// One env's share of a wave on the host: the model (and its aux twin), the scratch, and one host thread per lane group.
template <typename T> struct HostRun {
    using V = Quad<T>;
    StepLayout lay;                    // the wave this run stands for, with the harness's overrides (ngroups, g_offload, g_aux) on top
    SimOpts o;
    T tab[LM_TABLE], auxtab[LM_AUX];
    LaneModel<V> m, m_aux;
    V scratch[SC_COUNT];               // (the LEAN variants park state / system / factorisation where the ordinary one has its reduction buffer and overflow candidates)
    V ovcbuf[OVC_FLOATS_PER_LANE];     // LEAN: the candidates beyond the row cache live outside the scratch (global memory on the device), and behind them the thread pair contact's frame
    HostWave wave;
    static_assert(SC_COUNT >= SC_COUNT_LEAN_PAIR && SC_COUNT >= SC_COUNT_LEAN, "the scratch holds every variant's");
    struct Group { int g; LaneScratch<V> sc; const LaneModel<V>* m; bool rep; LaneState<V> s; };      // rep: the lanes that hold the env's state (main, replica, aux)

    int init(const double* P, int ngroups, bool lean, bool pair, int contacts, int max_newton, int implicit_damp, int rank_one) {
        if (int rc = build_packed_model<T>(P, tab)) return rc;
        m.c.inv = tab; m.c.tab = tab + LM_INV; m.c.lean = lean; m.c.preload();
        build_aux_block<T>(tab, auxtab);
        m_aux = m;
        m_aux.c.tab = auxtab; m_aux.c.tab_rare = tab + LM_INV; m_aux.c.preload();
        lay = step_layout(ngroups == 2 ? 8 : 4, lean, pair);
        lay.groups = ngroups;
        lay.offload = lay.offload && g_offload && ngroups >= 2;
        lay.aux = lay.aux && g_aux && lay.offload;          // (rides on the replica's layout)
        o = sim_opts(lay, contacts, max_newton, implicit_damp, rank_one, g_spread);
        wave.ngrp = ngroups; wave.gstride = lay.main_lanes;      // the lane distance between groups selects the reduction (16: the 4-envs-per-wave kernel's transposed one)
        return 0;
    }
    void sync() { if (lay.groups > 1) wave.barrier(); }
    void poison(int count) { for (int k = 0; k < count; k++) scratch[k] = V(std::numeric_limits<T>::quiet_NaN()); }
    // Every lane group runs body(Group&) from the env's state s0 (helper lanes: from a harmless one), group 0 on the caller's thread.
    template <typename F> void run(const LaneState<V>& s0, F body) {
        auto group = [&](int g) {
            if (lay.groups > 1) { g_host_wave = &wave; g_host_grp = g; }
            Group G;
            G.g = g;
            bind_scratch(G.sc, lay, scratch, 1, g, ovcbuf);
            G.m = G.sc.aux_lane ? &m_aux : &m;
            G.rep = holds_state(lay, g);
            G.s = s0;
            if (!G.rep) helper_lane_state(G.s);
            if (g == 0) {
                poison(SC_COUNT);
                if (lay.offload) for (int k = 0; k < 56; k++) scratch[SC_ZERO + k] = V(T(0));       // written once per kernel on the device
            }
            body(G);
            g_host_wave = nullptr;
        };
        std::vector<std::thread> th;
        for (int g = 1; g < lay.groups; g++) th.emplace_back(group, g);
        group(0);
        for (auto& t : th) t.join();
    }
    // Before every substep: poison the scratch - a substep must not read anything it has not written itself (on the device LDS keeps whatever
    // the previous kernel left there).  What carries over: the replica's zeros and, in the LEAN variants, the parked state.  pair_warm_start (the
    // entry points that may run the PAIR substep): the pair narrow phase's warm start too, within a control step - it starts cold in every one.
    // Without it those three slots are poisoned like the rest: a substep without the pair contact must not read them.
    void before_substep(const Group& G, bool pair_warm_start, bool first_of_control_step) {
        sync();
        if (G.g == 0) {
            const int pd = G.sc.pd;
            const bool keep = pair_warm_start && !first_of_control_step;
            for (int k = 0; k < (lay.lean ? SC_LSTATE : lay.offload ? SC_ZERO : SC_COUNT); k++) if (!keep || k < pd + 9 || k > pd + 11) scratch[k] = V(std::numeric_limits<T>::quiet_NaN());
            if (pair_warm_start && first_of_control_step) scratch[pd + 11] = V(T(0));
            for (auto& c : ovcbuf) c = V(std::numeric_limits<T>::quiet_NaN());
        }
        sync();
    }
};

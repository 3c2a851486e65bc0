// jb_contacts.hpp — the contact pass: a state and an action -> the contacts of that state and the force each one carries, without
// advancing time.
//
// Nothing about a contact is computed twice.  ONE substep of the step kernels (jb_sim.hpp substep) runs on a copy of the state: phase A leaves
// the candidates in the per-lane scratch, the contact solve turns them into rows (RowVals: weight D, joint columns, reference accelerations)
// and ends with the accelerations y - the forward pass's qacc.  This file reads those rows back, slot by slot, with the solver's own helpers
// (row_load / row_values for a slot beyond the row cache, row_pairs, row_residuals) and evaluates the pyramid's four edge forces at y:
//     r_e = J_e y - aref_e  for the edges J_n +- mu J_t1, J_n +- mu J_t2,      f_e = D max(0, -r_e)
// (MuJoCo's mj_contactForce on a pyramidal cone); y is the contact problem's minimiser, which the solve leaves in the scratch too (ct_y).  The
// scratch entries are packed by rank among the LIVE slots of the wave, so the caller hands the substep a SolveTap (CtTap) and passes the mask on.
//
// Rows.  A contact is one candidate slot of phase A (jb_sim.hpp SC_ROWS) of one lane; the table below fixes the row of every (lane, slot)
// that can hold one - ct_row - and the geom it belongs to - ct_geom, by jb_model_build.hpp's assignment of the root / motor-body geoms to lanes:
//     0-39   leg l, slot s -> 10 l + s: foot (geom 7 + 4 l), lower cylinder x 4 (6 + 4 l), upper cylinder x 4 (4 + 4 l), knee tip (5 + 4 l)
//     40-44  lane 2, slots 10-14: screw1 x 4 (geom 2), screw2 (3)        45-52 / 53-60  lanes 0 / 1, slots 15-22: the box vertices of coreBody1 / 2
//     61-65  lane 3, slots 23-27: threadMass x 4 (geom 20), mass (21)    66-73  leg l, slots 28 / 29: the leg's upper cylinder against threadMass / mass
// A floor row is (geom1 -1, geom2 the geom); a pair row (geom1 the leg's cylinder, geom2 the thread or the mass).
//
// One row, CT_W floats: [pos(3) | normal(3) | force(3) | dist | fn | active], world axes.  pos: the candidate's point (the midpoint between
// the two surfaces).  normal: from geom1 to geom2, +z for the floor.  force: on geom2 (geom1 receives the opposite), fn n + mu (f0 - f1) t1
// + mu (f2 - f3) t2 along the contact frame; for the floor the frame is (z, y, -x), so force = (-mu (f2 - f3), mu (f0 - f1), fn).  The solver
// keeps a pair's frame with its normal towards the leg: its three directions are negated here.  An inactive row is all zeros.
// dist: phase A's signed distance.  The row build overwrites it with the weight (ROW_F), so it is solved from what the row keeps:
// aref_n = -b v_n - k d(r) r with d(r) = D c / (1 + D c), c the regulariser's constant of the slot - algebra, no geometry restated.
//
// Written once on the lane type V: the device runs it on float, tests/contacts_harness.cpp on Quad<float> and Quad<double>.
#pragma once
#include "jb_readout.hpp"

namespace jb {

constexpr int CT_NROW = 74, CT_W = 12, CT_TABLE = CT_NROW * CT_W, CT_GEOMF = RO_NGEOM * 3;
constexpr int CT_POS = 0, CT_NORMAL = 3, CT_FORCE = 6, CT_DIST = 9, CT_FN = 10, CT_ACTIVE = 11;

// can lane `leg` hold a contact in `slot`, which row is it, and which geom touches (the floor, or the leg's upper cylinder)
JB_HD constexpr bool ct_has_row(int leg, int slot) { return slot < 10 || slot >= SLOT_THREAD || (slot < 15 ? leg == 2 : slot < 23 ? leg < 2 : leg == 3); }
JB_HD constexpr int ct_row(int leg, int slot) {
    return slot < 10 ? 10 * leg + slot : slot < 15 ? 30 + slot : slot < 23 ? (leg == 0 ? 30 : 38) + slot : slot < SLOT_THREAD ? 38 + slot : 66 + 2 * leg + (slot - SLOT_THREAD);
}
JB_HD constexpr int ct_geom(int leg, int slot) {
    return slot == 0 ? 7 + 4 * leg : slot < 5 ? 6 + 4 * leg : slot < 9 ? 4 + 4 * leg : slot == 9 ? 5 + 4 * leg : slot < 14 ? 2 : slot == 14 ? 3 : slot < 23 ? leg
         : slot < 27 ? 20 : slot == 27 ? 21 : slot == SLOT_THREAD ? 20 : 21;
}
constexpr bool ct_rows_are_a_permutation() {
    bool seen[CT_NROW] = {};
    int n = 0;
    for (int leg = 0; leg < 4; leg++) for (int slot = 0; slot < NSLOT; slot++) if (ct_has_row(leg, slot)) {
        const int r = ct_row(leg, slot);
        if (r < 0 || r >= CT_NROW || seen[r]) return false;
        seen[r] = true; n++;
    }
    return n == CT_NROW;
}
static_assert(NSLOT == 30 && SLOT_THREAD == 28 && SLOT_MASS == 29 && ct_rows_are_a_permutation(), "every (lane, slot) that can hold a contact has a row of its own, and every row is one");
// (geom1, geom2) of every row: out [CT_NROW][2]
inline void ct_slot_geoms(int32_t* out) {
    for (int leg = 0; leg < 4; leg++) for (int slot = 0; slot < NSLOT; slot++) if (ct_has_row(leg, slot)) {
        int32_t* o = out + 2 * ct_row(leg, slot);
        o[0] = slot >= SLOT_THREAD ? 4 + 4 * leg : -1; o[1] = ct_geom(leg, slot);
    }
}

// the root's world pose (the readout's hi + lo rotation and height) and y as the solver holds it: root block [angular | linear], both in
// the ROOT frame, the lane's own two hinges, the motor
template <typename V> struct CtPose { Mat3<V> R; V px, py, pz, pz_lo; };
template <typename V> struct CtY { Pk2<V> yr[3]; V yl[2], ym; };
template <typename V> struct CtRowOut { V v[CT_W]; typename lane_traits<V>::mask on; };
// What a SolveTap collects, and the y the env's solve ended with: the minimiser y the Newton iteration left in the scratch (SC_Y) - the
// substep's qacc is y - d with (M + h diag(b)) d = h diag(b) y, the implicit damping's share, which is not part of the contact problem.
// In a wave that solved a second time SC_Y holds the second solve's y for EVERY env; an env that kept its first solve takes that one's.
template <typename V> struct CtTap {
    unsigned live = 0u; bool redone = false; V y1[9]; typename lane_traits<V>::mask re;
    JB_HD SolveTap<V> tap() { return SolveTap<V>{&live, &redone, y1, &re}; }
};
template <typename V> JB_HD CtY<V> ct_y(const LaneScratch<V>& sc, const CtTap<V>& t) {
    V y[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { y[i] = sc.ld(SC_Y + i); if (t.redone) y[i] = sel(t.re, y[i], t.y1[i]); }
    CtY<V> r;
    r.yr[0] = Pk2<V>(y[0], y[1]); r.yr[1] = Pk2<V>(y[2], y[3]); r.yr[2] = Pk2<V>(y[4], y[5]);
    r.yl[0] = y[6]; r.yl[1] = y[7]; r.ym = y[8];
    return r;
}

// The row of `slot` (live in this substep: a bit of `live`) for every lane, from what the substep left in the scratch.  A lane that has no
// contact there - or cannot have one (ct_has_row) - gets zeros and on = false.
template <typename V, bool PAIR>
JB_HD void ct_slot(const LaneModel<V>& m, const LaneScratch<V>& sc, unsigned live, int slot, const CtPose<V>& P, const CtY<V>& y, CtRowOut<V>& o) {
    using MK = typename lane_traits<V>::mask;
    const int rank = __builtin_popcount(live & ((1u << slot) - 1u)), level = slot_level(slot);
    const bool is_pair = PAIR && level == 4, cached = rank < ROW_K;
    const V mu = m.c[LM_MU];
    RowVals<V> rv;
    if (cached) row_load<V>(sc, rank, rv);
    else {      // beyond the cache: the candidate is still there, the row is formed as every pass of the solve forms it
        const int c0 = 4 * (rank - ROW_K) * sc.ovc_stride;
        row_values<V, PAIR>(m, sc, level == 3, slot, v3<V>(sc.ovc[c0], sc.ovc[c0 + sc.ovc_stride], sc.ovc[c0 + 2 * sc.ovc_stride]), sc.ovc[c0 + 3 * sc.ovc_stride], rv);
        // ... and taken as the values a cache entry would hold: a product left open to the sums below would be fused into them, and the row's
        // bits would depend on whether the env's wave-mates pushed the slot beyond the cache (contact_sweep's build pins them likewise)
        rv.D = val_pin(rv.D);
#pragma unroll
        for (int k = 0; k < 3; k++) { rv.jsh[k] = val_pin(rv.jsh[k]); rv.j7[k] = val_pin(rv.j7[k]); rv.ah[k] = val_pin(rv.ah[k]); }
    }
    MK on = gt(rv.D, V(0));
    // (a leg slot's entry of a lane without the contact may never have been built - spread sweeps - and still hold phase A's +1 where the weight goes)
    if (slot < 10) on = mand(on, neq_u(and_u(vtou(sc.ld(SC_OWN)), 1u << slot), zero_u<V>()));
    Vec3<V> dk[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (!is_pair) dk[k] = sc.ld3(SC_DD + 3 * k);
        else if (slot == SLOT_THREAD) dk[k] = v3<V>(sc.ovc[(sc.pd2 + 3 * k) * sc.ovc_stride], sc.ovc[(sc.pd2 + 3 * k + 1) * sc.ovc_stride], sc.ovc[(sc.pd2 + 3 * k + 2) * sc.ovc_stride]);
        else dk[k] = sc.ld3(sc.pd + 3 * k);
    }
    const V y7 = level == 2 ? y.yl[1] : y.ym, r7 = level == 2 ? sc.ld(SC_ST + 4) : sc.ld(SC_ST + 5);      // what column 7 multiplies: the knee's, or the motor's
    RowPairs<V> R;
    row_pairs<V, PAIR>(rv, dk, V(is_pair ? 0.0f : 1.0f), rv.jsh, rv.j7, rv.ah, R);
    V rho[3];
    row_residuals<V>(R, y.yr, Pk2<V>(y.yl[0], y7), rho);
    const V mr1 = mu * rho[1], mr2 = mu * rho[2], D = sel(on, rv.D, V(0));
    const V f0 = D * vmax(V(0), -(rho[0] + mr1)), f1 = D * vmax(V(0), -(rho[0] - mr1)), f2 = D * vmax(V(0), -(rho[0] + mr2)), f3 = D * vmax(V(0), -(rho[0] - mr2));
    const V fn = (f0 + f1) + (f2 + f3), ft1 = mu * (f0 - f1), ft2 = mu * (f2 - f3);
    // the distance, from the row - also where the candidate still has it (a slot beyond the cache): whether a slot is cached depends on
    // the env's wave-mates, and the row's bits must not
    V vel = rv.jsh[0] * sc.ld(SC_ST + 3) + rv.j7[0] * r7;
    if (!is_pair) vel = vel + (dot(cross(rv.x, dk[0]), sc.ld3(SC_ST)) + sc.ld(SC_DD + 21));
    const V tran = is_pair ? m.c.tran_of(1) + m.c.tran_of(3) : m.c.tran_of(level);
    const V Dc = rv.D * (tran * ((V(1) + m.c[LM_FR2]) * (V(2) * mu * mu)));
    const V imp = Dc * vrcp(V(1) + Dc);
    const V dist = -(rv.ah[0] + m.c[LM_BB] * vel) * vrcp(m.c[LM_KK] * imp);
    const Vec3<V> t = mul(P.R, rv.x);
    Vec3<V> force, normal;
    if (is_pair) {
        force = -mul(P.R, dk[0] * fn + dk[1] * ft1 + dk[2] * ft2);
        normal = -mul(P.R, dk[0]);
    } else {
        force = v3<V>(-ft2, ft1, fn);
        normal = v3<V>(V(0), V(0), V(1));
    }
    const V row[CT_W] = {P.px + t.x, P.py + t.y, (P.pz + t.z) + P.pz_lo, normal.x, normal.y, normal.z, force.x, force.y, force.z, dist, fn, V(1)};
#pragma unroll
    for (int i = 0; i < CT_W; i++) o.v[i] = sel(on, row[i], V(0));
    o.on = on;
}

}  // namespace jb

// jb_forward.hpp — the forward-dynamics pass: a state and an action -> the accelerations the next substep would integrate, the contact
// forces in joint space, the accelerations of the ten bodies and the motor's torque and power, without advancing time.
//
// The accelerations y are not computed here: they are what ONE substep of the step kernels (jb_sim.hpp substep, phase C) leaves in the
// warm-start fields wa / wl / wj / wm - the full contact solve, both pair contacts, the line-searched second solve, per-env models.  This
// file maps (state, y) to the outputs by inverse dynamics, lane by lane, with the readout's state loading, hi + lo rotation and kinematics
// (jb_readout.hpp) extended to accelerations.  The device pass around it is jb_forward_kernel (jb_api.hip: it needs the step kernels'
// scratch binding and table staging).
//
// Outputs per env-state (each may be absent).  Vectors are in MuJoCo's qvel order, as jb_get_state has it:
// [linear, world (3) | angular, root frame (3) | leg hinges, 6 + 2l shoulder, 7 + 2l knee of leg l | motor].  h: timestep, b: hinge damping.
//   qacc     [15]      y = (M + h diag(b))^-1 (tau + J^T f): the acceleration the next substep integrates
//   qfrc     [15]      J^T f = M y + h b o y - tau, by inverse dynamics from y (M is never formed).  0-2: the net floor force on the robot in
//                      world axes (the pair contacts act between two bodies of one robot and cancel there), 3-5: the net contact moment
//                      about the root origin in root axes, 6-14: the contact torque on each hinge.  A difference of inertial terms much
//                      larger than itself: in fp32 its error scales with what cancels, not with its own size.
//   body_acc [10][6]   per body (the readout's order): world linear acceleration of the centre of mass, world angular acceleration - the
//                      time derivative of the readout's body_vel along q' = v, v' = y.  Gravity is not subtracted.
//   motor    [3]       [ctrl clamped to ctrlrange | joint torque gear * force | mechanical power torque * phi'], force as in the substep:
//                      gain u + biasprm0 + biasprm1 gear (phi + 2 pi turns) + biasprm2 gear phi'
//
// Lane mapping: the readout's - lane l owns leg l (its two bodies, its two hinge rows), lane 0 the root body, lane 3 the motor body and
// the motor row.  The six root rows of qfrc are the quad sum of the lanes' partial sums.  Written once on the real type: the device runs
// it in fp32, tests/forward_harness.cpp runs the same source on the host in fp32 and fp64.
#pragma once
#include "jb_readout.hpp"

namespace jb {

constexpr int FW_NV = 15, FW_BACC = RO_NBODY * 6, FW_MOTOR = 3;
// state fields the readout does not read (jb_api.hip RootF / LegF; static_assert there): whole motor turns, the contact solve's warm start
constexpr int FW_RF_TURNS = 15, FW_RF_WA = 16, FW_RF_WL = 19, FW_RF_WM = 22, FW_LF_WJ0 = 4, FW_LF_WJ1 = 5;

// where one env-state's outputs go (a null pointer: that output is absent)
template <typename T> struct FwOut { T* qacc; T* qfrc; T* bacc; T* motor; };
// y as a lane holds it after the substep: world linear (wl), root-frame angular (wa), its own leg's two hinges (wj), the motor (wm)
template <typename T> struct FwAcc { T lin[3], ang[3], j1, j2, m; };
// what a lane reads of the state: the readout's fields and the motor's whole turns (the actuator's length bias sees the unwrapped angle)
template <typename T> struct FwState { RoState<T> r; T turns; };
template <typename T> JB_HD FwState<T> fw_load(const SnapView& v, long long env, int leg) {
    FwState<T> s;
    s.r = ro_load<T>(v, env, leg);
    s.turns = (T)ro_word(v.root[(long long)FW_RF_TURNS * v.n + env]);
    return s;
}

// One body in ROOT coordinates (rotation Rj from its orientation at qpos0, centre of mass c, its inertial acceleration a with the root
// origin's included, angular acceleration al, angular velocity w; gr: gravity): the body_acc row, and its inertial wrench - force
// F = m (a - g), moment N = I al + w x I w about the centre of mass - returned, with F and the moment about the root origin added to fs / ns.
template <typename T> JB_HD void fw_body(const FwOut<T>& o, const Mat3<T>& R0, const Vec3<T>& gr, int b, const Mat3<T>& Rj, const Vec3<T>& c, const Vec3<T>& a,
                                         const Vec3<T>& al, const Vec3<T>& w, const T& m, const Sym3<T>& I, Vec3<T>& F, Vec3<T>& N, Vec3<T>& fs, Vec3<T>& ns) {
    if (o.bacc) {
        const Vec3<T> aw = mul(R0, a), alw = mul(R0, al);
        T* q = o.bacc + 6 * b;
        q[0] = aw.x; q[1] = aw.y; q[2] = aw.z; q[3] = alw.x; q[4] = alw.y; q[5] = alw.z;
    }
    F = (a - gr) * m;
    N = mul(Rj, mul(I, mulT(Rj, al))) + cross(w, mul(Rj, mul(I, mulT(Rj, w))));
    fs = fs + F;
    ns = ns + N + cross(c, F);
}

// Everything lane `leg` of an env-state's quad contributes: its rows of qacc / qfrc / body_acc / motor (written through o) and its partial
// sums p of the six root rows of qfrc ([force, world | moment about the root origin, root axes], overwritten).  tab: the env's packed
// constant table (LM_TABLE entries); ctrl: the action as given (clamped here, as the substep clamps it).
template <typename T> JB_HD void fw_lane(const FwState<T>& fs_, const FwAcc<T>& y, const T& ctrl, const T* tab, int leg, const FwOut<T>& o, T (&p)[6]) {
    const RoState<T>& s = fs_.r;
    auto C = [&](int i) { return tab[lm_offset(i, leg)]; };
    auto C3 = [&](int i) { return v3<T>(C(i), C(i + 1), C(i + 2)); };
    auto CS = [&](int i) { Sym3<T> q; q.xx = C(i); q.yy = C(i + 1); q.zz = C(i + 2); q.xy = C(i + 3); q.xz = C(i + 4); q.yz = C(i + 5); return q; };
    const Mat3<T> R0 = ro_quat2mat(s.q, s.ql);
    const Vec3<T> w0 = v3<T>(s.wx, s.wy, s.wz), al0 = v3<T>(y.ang[0], y.ang[1], y.ang[2]);
    const Vec3<T> A0 = mulT(R0, v3<T>(y.lin[0], y.lin[1], y.lin[2])), gr = mulT(R0, C3(LM_GRAV));      // the root origin's acceleration and gravity, root coordinates
    const T h = C(LM_H), w0_2 = dot(w0, w0);
    auto accel_at = [&](const Vec3<T>& x) { return A0 + cross(al0, x) + wxwx(w0, w0_2, x); };           // a point fixed on the root body
    Vec3<T> fsum = v3<T>(T(0), T(0), T(0)), nsum = fsum, F, N;

    // ---- the lane's own leg: upper body 1 + 2 leg (shoulder hinge on the root), lower body 2 + 2 leg (knee hinge on the upper body)
    T s1, c1, s2, c2;
    vsincos_pi(s.th1, s1, c1); vsincos_pi(s.th2, s2, c2);
    const Vec3<T> a1 = C3(LM_A1), e1 = C3(LM_E1);
    const Mat3<T> R1 = rodrigues(e1, s1, c1), R12 = mul(R1, rodrigues(C3(LM_E2), s2, c2));
    const Vec3<T> a2 = a1 + mul(R1, C3(LM_DA2)), e2 = mul(R1, C3(LM_E2));
    const Vec3<T> cu = a1 + mul(R1, C3(LM_DC1)), cl = a2 + mul(R12, C3(LM_DC2));
    const Vec3<T> w1 = w0 + e1 * s.thd1, w2 = w1 + e2 * s.thd2;
    const Vec3<T> al1 = al0 + e1 * y.j1 + cross(w0, e1) * s.thd1, al2 = al1 + e2 * y.j2 + cross(w1, e2) * s.thd2;
    const T w1_2 = dot(w1, w1), w2_2 = dot(w2, w2);
    const Vec3<T> ru = cu - a1, r12 = a2 - a1, rl = cl - a2;
    const Vec3<T> Aa1 = accel_at(a1);
    const Vec3<T> Aa2 = Aa1 + cross(al1, r12) + wxwx(w1, w1_2, r12);
    const Vec3<T> Au = Aa1 + cross(al1, ru) + wxwx(w1, w1_2, ru), Al = Aa2 + cross(al2, rl) + wxwx(w2, w2_2, rl);
    Vec3<T> Fl, Nl;
    fw_body(o, R0, gr, 1 + 2 * leg, R1, cu, Au, al1, w1, C(LM_M1), CS(LM_I1), F, N, fsum, nsum);
    fw_body(o, R0, gr, 2 + 2 * leg, R12, cl, Al, al2, w2, C(LM_M2), CS(LM_I2), Fl, Nl, fsum, nsum);
    if (o.qfrc) {
        const T b1 = C(LM_B1), b2 = C(LM_B2);
        o.qfrc[6 + 2 * leg] = dot(e1, N + cross(ru, F) + Nl + cross(cl - a1, Fl)) + C(LM_K1) * s.th1 + b1 * s.thd1 + h * b1 * y.j1;
        o.qfrc[7 + 2 * leg] = dot(e2, Nl + cross(rl, Fl)) + C(LM_K2) * s.th2 + b2 * s.thd2 + h * b2 * y.j2;
    }
    if (o.qacc) { o.qacc[6 + 2 * leg] = y.j1; o.qacc[7 + 2 * leg] = y.j2; }

    // ---- the lane's share of the rest: lane 0 the root body and the linear rows of qacc, lane 1 its angular rows, lane 3 the motor
    if (leg == 0) {
        const Vec3<T> c0 = C3(LM_C0);
        fw_body(o, R0, gr, 0, ro_identity<T>(), c0, accel_at(c0), al0, w0, C(LM_M0), CS(LM_I0), F, N, fsum, nsum);
        if (o.qacc) { o.qacc[0] = y.lin[0]; o.qacc[1] = y.lin[1]; o.qacc[2] = y.lin[2]; }
    }
    if (leg == 1 && o.qacc) { o.qacc[3] = y.ang[0]; o.qacc[4] = y.ang[1]; o.qacc[5] = y.ang[2]; }
    if (leg == 3) {
        T sp, cp;
        vsincos_pi(s.phi, sp, cp);
        const Vec3<T> am = C3(LM_AM), em = C3(LM_EM);
        const Mat3<T> Rm = rodrigues(em, sp, cp);
        const Vec3<T> rm = mul(Rm, C3(LM_DCM)), cm = am + rm;
        const Vec3<T> wm = w0 + em * s.phid, alm = al0 + em * y.m + cross(w0, em) * s.phid;
        const Vec3<T> Am = accel_at(am) + cross(alm, rm) + wxwx(wm, dot(wm, wm), rm);
        fw_body(o, R0, gr, 9, Rm, cm, Am, alm, wm, C(LM_MM), CS(LM_IM), F, N, fsum, nsum);
        const T uc = vmin(vmax(ctrl, C(LM_CTRL_LO)), C(LM_CTRL_HI)), gear = C(LM_GEAR);
        const T len = gear * (s.phi + fs_.turns * T(6.283185307179586));
        const T force = C(LM_GAIN) * uc + C(LM_BIAS) + C(LM_BIAS + 1) * len + C(LM_BIAS + 2) * gear * s.phid;
        const T torque = gear * force;
        if (o.qfrc) o.qfrc[14] = dot(em, N + cross(rm, F)) - torque;
        if (o.qacc) o.qacc[14] = y.m;
        if (o.motor) { o.motor[0] = uc; o.motor[1] = torque; o.motor[2] = torque * s.phid; }
    }
    const Vec3<T> fw = mul(R0, fsum);
    p[0] = fw.x; p[1] = fw.y; p[2] = fw.z; p[3] = nsum.x; p[4] = nsum.y; p[5] = nsum.z;
}

}  // namespace jb

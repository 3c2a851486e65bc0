// jb_inertia.hpp — the inertia pass: a state and an action -> the terms of the equation of motion  M qacc + bias = passive + actuator
// (+ J^T f) and the Jacobians of the bodies and the feet: the library's counterparts of MuJoCo's mj_fullM, qfrc_bias, qfrc_passive,
// qfrc_actuator, qacc_smooth and mj_jacBodyCom / mj_jacGeom.  It reads the state through SnapView with the readout's loading, hi + lo
// rotation and kinematics (jb_readout.hpp, jb_forward.hpp fw_load for the motor's whole turns) and the constant tables the step kernels
// read (jb_sim.hpp LM_*); it writes nothing but its outputs and never runs a substep.
//
// Outputs per env-state (each may be absent).  Vectors are in MuJoCo's qvel order, as jb_get_state has it:
// [linear, world (3) | angular, root axes (3) | leg hinges, 6 + 2l shoulder, 7 + 2l knee of leg l | motor].
//   qM          [15][15]    the dense symmetric joint-space inertia, sum over the bodies of m Jv^T Jv + Jw^T I Jw.  An arrow: the 6 x 6 root
//                           block, per leg a 6 x 2 column pair and a 2 x 2 block, for the motor a 6 x 1 column and a 1 x 1 block; the
//                           leg-leg and leg-motor blocks are exact zeros.  Both triangles and the zeros are written.
//   qfrc        [3][15]     row 0 qfrc_bias: Coriolis, centrifugal and gravity terms (gravity folded in as an acceleration -g of the root,
//                           as oracle/jb_oracle.c dynamics() does); row 1 qfrc_passive: -k th - b th' on the eight leg hinges, 0 elsewhere;
//                           row 2 qfrc_actuator: entry 14 alone, gear * force with the action clamped to the ctrlrange and the force as
//                           the substep and jb_forward.hpp compute it (the length bias sees the unwrapped motor angle)
//   qacc_smooth [15]        M^-1 (passive + actuator - bias): the unconstrained acceleration.  This is PLAIN M: jb_forward's qacc solves
//                           (M + h diag(b)) y = tau + J^T f with the implicit damping term h b, this output does not carry it.  So
//                           jb_forward's qfrc_constraint = qM y + h b o y - (passive + actuator - bias) with y = jb_forward's qacc.
//   jac         [14][6][15] per row block [jacp (3) | jacr (3)] x 15 in world axes: d(world velocity of the point) / d(qvel) and d(world
//                           angular velocity of its body) / d(qvel).  Blocks 0-9: the ten bodies at their centres of mass, the readout's
//                           order (mj_jacBodyCom); block 10 + l: the centre of leg l's foot sphere (mj_jacGeom; model.FOOT_GEOMS order).
//                           The free joint's rotational columns are about the root's own axes through the root origin, as the oracle's
//                           jacobian() has them.  Every entry is written, zeros included.  The other geoms have no block: a point p on
//                           body b, r = p - centre of mass, has jacp(p) = jacp - [r]x jacr with body b's block.
//
// Lane mapping: the readout's - FOUR LANES PER ENV-STATE, lane l owns leg l (bodies 1 + 2l and 2 + 2l, hinge dofs 6 + 2l and 7 + 2l, foot
// block 10 + l), lane 0 the root body, lane 3 the motor body and dof 14.  A lane works in ROOT coordinates on its own dofs (IN_NL lane-local
// ones: 0-2 linear in root axes, 3-5 angular, 6 / 7 its hinges, 8 the motor); rows 0-2 turn to world axes (R0) where they are written.
//
// The solve goes through the arrow: every lane eliminates its own 2 x 2 hinge block (lane 3 the motor's 1 x 1 too), the Schur terms and
// the reduced right-hand sides are quad-summed onto the root block, every lane factors the same 6 x 6 (Cholesky) and substitutes, and then
// back-substitutes its own hinges.  Between the two halves stand the quad sums, so the element function comes in two parts (in_lane_a,
// in_lane_b) with the IN_NP partial sums between them, and in_jac for the Jacobian blocks.  Written once on the real type: the device runs
// it in fp32 (jb_inertia_kernel below), tests/inertia_harness.cpp runs the same source on the host in fp32 and fp64.
#pragma once
#include "jb_forward.hpp"

namespace jb {

constexpr int IN_NV = 15, IN_NJAC = 14, IN_QM = IN_NV * IN_NV, IN_QFRC = 3 * IN_NV, IN_QACC = IN_NV, IN_JBLOCK = 6 * IN_NV, IN_JAC = IN_NJAC * IN_JBLOCK;
constexpr int IN_NL = 9, IN_TRI = IN_NL * (IN_NL + 1) / 2;
// the partial sums a lane hands to the quad: the root block of M (lower triangle, tri()), the Schur terms B H^-1 B^T of its hinges (the
// same), the root rows of passive + actuator - bias (= -bias; the linear rows without gravity), and B H^-1 r of its hinges
constexpr int IN_P_ARR = 0, IN_P_SCHUR = 21, IN_P_RHS = 42, IN_P_BZ = 48, IN_NP = 54;

// where one env-state's outputs go (a null pointer: that output is absent)
template <typename T> struct InOut { T* qM; T* qfrc; T* qacc; T* jac; };
// a hinge in root coordinates: unit axis, a point on it
template <typename T> struct InHinge { Vec3<T> e, a; };
// what a lane keeps between its parts: the kinematics (root coordinates) for the Jacobian blocks, its lane-local M, forces and eliminations
template <typename T> struct InLane {
    Mat3<T> R0;
    InHinge<T> h1, h2, hx;       // shoulder, knee; lane 3: the motor hinge
    Vec3<T> cu, cl, foot, cx;    // centres of mass of the upper and the lower body, the foot sphere's centre; lane 0: the root body's centre of mass, lane 3: the motor body's
    Vec3<T> grav, gr;            // gravity in world and in root axes
    T A[IN_TRI];                 // lane-local M, lower triangle
    T bias[IN_NL], pas[2], act;
    T W[2][6], z[2], Wm[6], zm;  // H^-1 B^T and H^-1 r of the leg's 2 x 2 block, the same of the motor's 1 x 1
};
template <typename T> JB_HD Vec3<T> in_unit(int i) { return v3<T>(T(i == 0 ? 1 : 0), T(i == 1 ? 1 : 0), T(i == 2 ? 1 : 0)); }

// One body in ROOT coordinates (mass m, inertia I about its centre of mass c, root axes; NH hinges hg between it and the root, on the
// lane-local dofs FIRST ..; the velocity-product acceleration a of c, gravity gr, the inertial moment N about c): m Jv^T Jv + Jw^T I Jw
// added to A, Jv^T F + Jw^T N with F = m (a - gr) to bias.  The three linear rows of bias take m a alone: gravity joins them in world
// axes (in_lane_b), where its horizontal components are exact zeros - these rows are scaled by their velocity products, which a state
// at rest does not have.  The body's OWN hinge (its last one) takes a_own, the acceleration without the centripetal term -r |w|^2 about
// that hinge's anchor: r = c - anchor is at right angles to the column e x r, the term contributes an exact zero, and summing it in would
// leave its rounding - m r^2 w^2 eps, at a fast motor far more than the torque itself - on a dof that has this one body behind it.
template <typename T, int NH, int FIRST> JB_HD void in_body(T (&A)[IN_TRI], T (&bias)[IN_NL], const T& m, const Sym3<T>& I, const Vec3<T>& c, const InHinge<T>* hg, const Vec3<T>& a, const Vec3<T>& a_own, const Vec3<T>& gr, const Vec3<T>& N) {
    const Vec3<T> Fa = a * m, F = (a - gr) * m, Fo = (a_own - gr) * m;
    constexpr int NC = 6 + NH;
    Vec3<T> jv[NC], jw[NC];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        jv[i] = in_unit<T>(i); jw[i] = v3<T>(T(0), T(0), T(0));
        jv[3 + i] = cross(in_unit<T>(i), c); jw[3 + i] = in_unit<T>(i);
    }
#pragma unroll
    for (int k = 0; k < NH; k++) { jv[6 + k] = cross(hg[k].e, c - hg[k].a); jw[6 + k] = hg[k].e; }
#pragma unroll
    for (int i = 0; i < NC; i++) {
        const int li = i < 6 ? i : FIRST + i - 6;
        bias[li] += i == 0 ? Fa.x : i == 1 ? Fa.y : i == 2 ? Fa.z : dot(jv[i], (NH > 0 && i == NC - 1) ? Fo : F) + dot(jw[i], N);
        const Vec3<T> mj = jv[i] * m, ij = mul(I, jw[i]);
#pragma unroll
        for (int j = 0; j <= i; j++) A[tri(li, j < 6 ? j : FIRST + j - 6)] += dot(mj, jv[j]) + dot(ij, jw[j]);
    }
}

// The first part of lane `leg` of an env-state's quad: its kinematics, its lane-local M and forces, the elimination of its hinges (only
// when qacc is asked for), its own rows and columns of qM and its own entries of qfrc (written through o), and its partial sums p.
// tab: the env's packed constant table (LM_TABLE entries); ctrl: the action as given (clamped here, as the substep clamps it).
template <typename T> JB_HD void in_lane_a(const FwState<T>& fs_, const T& ctrl, const T* tab, int leg, const InOut<T>& o, InLane<T>& L, T (&p)[IN_NP]) {
    const RoState<T>& s = fs_.r;
    auto C = [&](int i) { return tab[lm_offset(i, leg)]; };
    auto C3 = [&](int i) { return v3<T>(C(i), C(i + 1), C(i + 2)); };
    auto CS = [&](int i) { Sym3<T> q; q.xx = C(i); q.yy = C(i + 1); q.zz = C(i + 2); q.xy = C(i + 3); q.xz = C(i + 4); q.yz = C(i + 5); return q; };
    L.R0 = ro_quat2mat(s.q, s.ql);
    // ---- kinematics of the lane's own leg, as the readout has them
    T s1, c1, s2, c2;
    vsincos_pi(s.th1, s1, c1); vsincos_pi(s.th2, s2, c2);
    const Vec3<T> a1 = C3(LM_A1), e1 = C3(LM_E1);
    const Mat3<T> R1 = rodrigues(e1, s1, c1), R12 = mul(R1, rodrigues(C3(LM_E2), s2, c2));
    const Vec3<T> a2 = a1 + mul(R1, C3(LM_DA2)), e2 = mul(R1, C3(LM_E2));
    L.h1.e = e1; L.h1.a = a1; L.h2.e = e2; L.h2.a = a2;
    L.cu = a1 + mul(R1, C3(LM_DC1)); L.cl = a2 + mul(R12, C3(LM_DC2)); L.foot = a2 + mul(R12, C3(LM_DFOOT));
    Mat3<T> Rm = ro_identity<T>();
    L.hx = L.h1; L.cx = C3(LM_C0);
    if (leg == 3) {
        T sp, cp;
        vsincos_pi(s.phi, sp, cp);
        L.hx.e = C3(LM_EM); L.hx.a = C3(LM_AM);
        Rm = rodrigues(L.hx.e, sp, cp);
        L.cx = L.hx.a + mul(Rm, C3(LM_DCM));
    }
#pragma unroll
    for (int i = 0; i < IN_NP; i++) p[i] = T(0);
    if (!(o.qM || o.qfrc || o.qacc)) return;

    // ---- velocity-product accelerations at qacc = 0 (jb_forward.hpp's recursion at y = 0); gravity is folded in as -g at the root by in_body
    L.grav = C3(LM_GRAV); L.gr = mulT(L.R0, L.grav);
    const Vec3<T> w0 = v3<T>(s.wx, s.wy, s.wz), gr = L.gr;
    const T w0_2 = dot(w0, w0);
    auto accel_at = [&](const Vec3<T>& x) { return wxwx(w0, w0_2, x); };      // a point fixed on the root body
    const Vec3<T> w1 = w0 + e1 * s.thd1, w2 = w1 + e2 * s.thd2;
    const Vec3<T> al1 = cross(w0, e1) * s.thd1, al2 = al1 + cross(w1, e2) * s.thd2;
    const T w1_2 = dot(w1, w1), w2_2 = dot(w2, w2);
    const Vec3<T> ru = L.cu - a1, r12 = a2 - a1, rl = L.cl - a2;
    const Vec3<T> Aa1 = accel_at(a1);
    const Vec3<T> Aa2 = Aa1 + cross(al1, r12) + wxwx(w1, w1_2, r12);
    // (w x (w x r) = w (w . r) - r |w|^2: the two halves apart for the bodies' own hinges, in_body)
    const Vec3<T> Auo = Aa1 + cross(al1, ru) + w1 * dot(w1, ru), Alo = Aa2 + cross(al2, rl) + w2 * dot(w2, rl);
    const Vec3<T> Au = Auo - ru * w1_2, Al = Alo - rl * w2_2;
    auto moment = [&](const Sym3<T>& I, const Vec3<T>& al, const Vec3<T>& w) { return mul(I, al) + cross(w, mul(I, w)); };
#pragma unroll
    for (int i = 0; i < IN_TRI; i++) L.A[i] = T(0);
#pragma unroll
    for (int i = 0; i < IN_NL; i++) L.bias[i] = T(0);
    {
        const Sym3<T> Iu = rotate(R1, CS(LM_I1)), Il = rotate(R12, CS(LM_I2));
        const T mu = C(LM_M1), ml = C(LM_M2);
        const InHinge<T> hg[2] = {L.h1, L.h2};
        in_body<T, 1, 6>(L.A, L.bias, mu, Iu, L.cu, hg, Au, Auo, gr, moment(Iu, al1, w1));
        in_body<T, 2, 6>(L.A, L.bias, ml, Il, L.cl, hg, Al, Alo, gr, moment(Il, al2, w2));
    }
    if (leg == 0) {
        const Sym3<T> I0 = CS(LM_I0);
        const T m0 = C(LM_M0);
        in_body<T, 0, 6>(L.A, L.bias, m0, I0, L.cx, &L.hx, accel_at(L.cx), accel_at(L.cx), gr, moment(I0, v3<T>(T(0), T(0), T(0)), w0));
    }
    L.act = T(0);
    if (leg == 3) {
        const Sym3<T> Im = rotate(Rm, CS(LM_IM));
        const T mm = C(LM_MM);
        const Vec3<T> rm = L.cx - L.hx.a, wm = w0 + L.hx.e * s.phid, alm = cross(w0, L.hx.e) * s.phid;
        const Vec3<T> Amo = accel_at(L.hx.a) + cross(alm, rm) + wm * dot(wm, rm), Am = Amo - rm * dot(wm, wm);
        in_body<T, 1, 8>(L.A, L.bias, mm, Im, L.cx, &L.hx, Am, Amo, gr, moment(Im, alm, wm));
        const T uc = vmin(vmax(ctrl, C(LM_CTRL_LO)), C(LM_CTRL_HI)), gear = C(LM_GEAR);
        const T len = gear * (s.phi + fs_.turns * T(6.283185307179586));
        const T force = C(LM_GAIN) * uc + C(LM_BIAS) + C(LM_BIAS + 1) * len + C(LM_BIAS + 2) * gear * s.phid;
        L.act = gear * force;
    }
    L.pas[0] = -(C(LM_K1) * s.th1) - C(LM_B1) * s.thd1;
    L.pas[1] = -(C(LM_K2) * s.th2) - C(LM_B2) * s.thd2;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        p[IN_P_RHS + i] = -L.bias[i];
#pragma unroll
        for (int j = 0; j <= i; j++) p[IN_P_ARR + tri(i, j)] = L.A[tri(i, j)];
    }

    // ---- the lane's own entries of qfrc, its own rows and columns of qM
    const int g1 = 6 + 2 * leg, g2 = g1 + 1;
    if (o.qfrc) {
        o.qfrc[g1] = L.bias[6]; o.qfrc[IN_NV + g1] = L.pas[0]; o.qfrc[2 * IN_NV + g1] = T(0);
        o.qfrc[g2] = L.bias[7]; o.qfrc[IN_NV + g2] = L.pas[1]; o.qfrc[2 * IN_NV + g2] = T(0);
        if (leg == 3) { o.qfrc[14] = L.bias[8]; o.qfrc[IN_NV + 14] = T(0); o.qfrc[2 * IN_NV + 14] = L.act; }
    }
    if (o.qM) {
#pragma unroll
        for (int hl = 6; hl < IN_NL; hl++) {
            if (hl == 8 && leg != 3) break;
            const int g = hl == 8 ? 14 : g1 + (hl - 6);
            const Vec3<T> lw = mul(L.R0, v3<T>(L.A[tri(hl, 0)], L.A[tri(hl, 1)], L.A[tri(hl, 2)]));      // the linear rows: root axes -> world axes
            const T col[6] = {lw.x, lw.y, lw.z, L.A[tri(hl, 3)], L.A[tri(hl, 4)], L.A[tri(hl, 5)]};
#pragma unroll
            for (int j = 0; j < 6; j++) { o.qM[g * IN_NV + j] = col[j]; o.qM[j * IN_NV + g] = col[j]; }
#pragma unroll
            for (int c = 6; c < IN_NV; c++) {
                T x = T(0);
                if (c == g1) x = L.A[tri(hl, 6)];
                if (c == g2) x = L.A[tri(hl, 7)];
                if (c == 14 && leg == 3) x = L.A[tri(hl, 8)];
                o.qM[g * IN_NV + c] = x;
            }
        }
    }
    if (!o.qacc) return;

    // ---- the lane's hinges out of the arrow: H = L D L^T of its 2 x 2 block, W = H^-1 B^T, z = H^-1 r; lane 3 the motor's 1 x 1 as well
    const T d1 = L.A[tri(6, 6)], l21 = L.A[tri(7, 6)] / d1, d2 = L.A[tri(7, 7)] - l21 * L.A[tri(7, 6)];
    const T id1 = T(1) / d1, id2 = T(1) / d2;
    auto hsolve = [&](const T& u1, const T& u2, T& x1, T& x2) { x2 = (u2 - l21 * u1) * id2; x1 = u1 * id1 - l21 * x2; };
    hsolve(L.pas[0] - L.bias[6], L.pas[1] - L.bias[7], L.z[0], L.z[1]);
#pragma unroll
    for (int i = 0; i < 6; i++) hsolve(L.A[tri(6, i)], L.A[tri(7, i)], L.W[0][i], L.W[1][i]);
    const T idm = leg == 3 ? T(1) / L.A[tri(8, 8)] : T(0);
    L.zm = (L.act - L.bias[8]) * idm;
#pragma unroll
    for (int i = 0; i < 6; i++) L.Wm[i] = L.A[tri(8, i)] * idm;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        p[IN_P_BZ + i] = L.A[tri(6, i)] * L.z[0] + L.A[tri(7, i)] * L.z[1] + L.A[tri(8, i)] * L.zm;
#pragma unroll
        for (int j = 0; j <= i; j++) p[IN_P_SCHUR + tri(i, j)] = L.A[tri(6, i)] * L.W[0][j] + L.A[tri(7, i)] * L.W[1][j] + L.A[tri(8, i)] * L.Wm[j];
    }
}

// The second part: t are the quad totals of the four lanes' p (ro_quad_total's association).  The root block of qM and the root entries
// of qfrc (entry i by lane i & 3), and qacc_smooth: the 6 x 6 Schur complement factored and solved by every lane alike, then the lane's
// own hinges.
template <typename T> JB_HD void in_lane_b(const InLane<T>& L, const T (&t)[IN_NP], int leg, const InOut<T>& o) {
    if (o.qM) {
        // linear x angular: R0 times the root-axes block; linear x linear is m_total 1 in any axes
        T la[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) la[i][j] = L.R0.m[3 * i] * t[IN_P_ARR + tri(3 + j, 0)] + L.R0.m[3 * i + 1] * t[IN_P_ARR + tri(3 + j, 1)] + L.R0.m[3 * i + 2] * t[IN_P_ARR + tri(3 + j, 2)];
#pragma unroll
        for (int i = 0; i < 6; i++)
            if (leg == (i & 3)) {
#pragma unroll
                for (int j = 0; j < 6; j++) o.qM[i * IN_NV + j] = (i < 3 && j >= 3) ? la[i][j - 3] : (i >= 3 && j < 3) ? la[j][i - 3] : t[IN_P_ARR + tri(i, j)];
            }
    }
    if (o.qfrc) {
        const Vec3<T> bw = mul(L.R0, v3<T>(-t[IN_P_RHS], -t[IN_P_RHS + 1], -t[IN_P_RHS + 2])) - L.grav * t[IN_P_ARR];      // t[IN_P_ARR]: the total mass
        const T b[6] = {bw.x, bw.y, bw.z, -t[IN_P_RHS + 3], -t[IN_P_RHS + 4], -t[IN_P_RHS + 5]};
#pragma unroll
        for (int i = 0; i < 6; i++)
            if (leg == (i & 3)) { o.qfrc[i] = b[i]; o.qfrc[IN_NV + i] = T(0); o.qfrc[2 * IN_NV + i] = T(0); }
    }
    if (!o.qacc) return;
    T S[21], x[6];
#pragma unroll
    for (int i = 0; i < 21; i++) S[i] = t[IN_P_ARR + i] - t[IN_P_SCHUR + i];
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = t[IN_P_RHS + i] - t[IN_P_BZ + i];
    x[0] += t[IN_P_ARR] * L.gr.x; x[1] += t[IN_P_ARR] * L.gr.y; x[2] += t[IN_P_ARR] * L.gr.z;      // gravity joins the linear rows here
    // Cholesky S = G G^T in place (the diagonal kept as its reciprocal), G u = r, G^T x = u
#pragma unroll
    for (int j = 0; j < 6; j++) {
        T d = S[tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) d -= S[tri(j, k)] * S[tri(j, k)];
        const T inv = T(1) / vsqrt(d);
        S[tri(j, j)] = inv;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            T v = S[tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; k++) v -= S[tri(i, k)] * S[tri(j, k)];
            S[tri(i, j)] = v * inv;
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        T v = x[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= S[tri(i, k)] * x[k];
        x[i] = v * S[tri(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        T v = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) v -= S[tri(k, i)] * x[k];
        x[i] = v * S[tri(i, i)];
    }
    T y1 = L.z[0], y2 = L.z[1], ym = L.zm;
#pragma unroll
    for (int i = 0; i < 6; i++) { y1 -= L.W[0][i] * x[i]; y2 -= L.W[1][i] * x[i]; ym -= L.Wm[i] * x[i]; }
    o.qacc[6 + 2 * leg] = y1; o.qacc[7 + 2 * leg] = y2;
    if (leg == 0) { const Vec3<T> lw = mul(L.R0, v3<T>(x[0], x[1], x[2])); o.qacc[0] = lw.x; o.qacc[1] = lw.y; o.qacc[2] = lw.z; }
    if (leg == 1) { o.qacc[3] = x[3]; o.qacc[4] = x[4]; o.qacc[5] = x[5]; }
    if (leg == 3) o.qacc[14] = ym;
}

// One Jacobian block [6][15]: the point x (root coordinates) on a body with up to two hinges below it, h1 on dof g1 and h2 on dof g2
// (g < 0: no such hinge).  Rows 0-2 jacp, 3-5 jacr, world axes.
template <typename T> JB_HD void in_jac_block(T* blk, const Mat3<T>& R0, const Vec3<T>& x, const InHinge<T>& h1, int g1, const InHinge<T>& h2, int g2) {
    Vec3<T> pv[5], rv[5];      // world columns: the three root rotations, the two hinges
#pragma unroll
    for (int j = 0; j < 3; j++) { pv[j] = mul(R0, cross(in_unit<T>(j), x)); rv[j] = v3<T>(R0.m[j], R0.m[3 + j], R0.m[6 + j]); }
    pv[3] = mul(R0, cross(h1.e, x - h1.a)); rv[3] = mul(R0, h1.e);
    pv[4] = mul(R0, cross(h2.e, x - h2.a)); rv[4] = mul(R0, h2.e);
    auto comp = [](const Vec3<T>& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : v.z; };
#pragma unroll
    for (int i = 0; i < 3; i++) {
        T* jp = blk + i * IN_NV;
        T* jr = blk + (3 + i) * IN_NV;
#pragma unroll
        for (int c = 0; c < 3; c++) { jp[c] = T(c == i ? 1 : 0); jr[c] = T(0); jp[3 + c] = comp(pv[c], i); jr[3 + c] = comp(rv[c], i); }
#pragma unroll
        for (int c = 6; c < IN_NV; c++) {
            T a = T(0), b = T(0);
            if (c == g1) { a = comp(pv[3], i); b = comp(rv[3], i); }
            if (c == g2) { a = comp(pv[4], i); b = comp(rv[4], i); }
            jp[c] = a; jr[c] = b;
        }
    }
}
// The Jacobian blocks of lane `leg`: its two bodies, its foot, and lane 0 the root body's, lane 3 the motor body's.  jac: the env-state's [14][6][15].
template <typename T> JB_HD void in_jac(const InLane<T>& L, int leg, T* jac) {
    const int g1 = 6 + 2 * leg, g2 = g1 + 1;
    in_jac_block(jac + (1 + 2 * leg) * IN_JBLOCK, L.R0, L.cu, L.h1, g1, L.h2, -1);
    in_jac_block(jac + (2 + 2 * leg) * IN_JBLOCK, L.R0, L.cl, L.h1, g1, L.h2, g2);
    in_jac_block(jac + (10 + leg) * IN_JBLOCK, L.R0, L.foot, L.h1, g1, L.h2, g2);
    if (leg == 0) in_jac_block(jac, L.R0, L.cx, L.hx, -1, L.hx, -1);
    if (leg == 3) in_jac_block(jac + 9 * IN_JBLOCK, L.R0, L.cx, L.hx, 14, L.hx, -1);
}

#if defined(__HIPCC__)
// ---- the device pass, on jb_readout_kernel's plan: one wave per block, RO_EPB env-states per block (a quad each), field-major state
// loads, a lane past the end repeats the last env-state, and every present output leaves the block as ONE contiguous segment copied from an
// LDS image in 16-byte words (ro_store_segment: scalar tail, `vec4` alignment flag).
//
// The images of all four outputs for 16 env-states would be 98 880 bytes, jac's alone 80 640: more than the 64 KB of a static __shared__
// array.  So the images TAKE TURNS in one buffer: first qM, qfrc and qacc_smooth of the 16 env-states together (18 240 bytes), then jac in
// IN_JTURNS turns of IN_JEPT env-states (20 160 bytes: the quads of the turn write their blocks from the kinematics they kept in
// registers, the wave copies the turn's segment out), with a barrier on either side of every copy.  A turn's segment is IN_JEPT whole
// env-states, so it starts on a 16-byte word whenever the array does and is whole 16-byte words.  The buffer is 20 160 bytes: eight
// blocks share a CU's LDS.  An env-state's numbers come from its own quad alone, whatever else is in the launch.
constexpr int IN_JEPT = 4, IN_JTURNS = RO_EPB / IN_JEPT;
constexpr int IN_LDS_QM = 0, IN_LDS_QFRC = IN_LDS_QM + RO_EPB * IN_QM, IN_LDS_QACC = IN_LDS_QFRC + RO_EPB * IN_QFRC, IN_LDS_SMALL = IN_LDS_QACC + RO_EPB * IN_QACC;
constexpr int IN_LDS_FLOATS = IN_LDS_SMALL > IN_JEPT * IN_JAC ? IN_LDS_SMALL : IN_JEPT * IN_JAC;
static_assert(IN_LDS_QFRC % 4 == 0 && IN_LDS_QACC % 4 == 0, "every LDS image starts on a 16-byte word");
static_assert((RO_EPB * IN_QM) % 4 == 0 && (RO_EPB * IN_QFRC) % 4 == 0 && (RO_EPB * IN_QACC) % 4 == 0 && IN_JAC % 4 == 0, "a full block's segment and any jac turn's are whole 16-byte words");
static_assert(IN_LDS_FLOATS * sizeof(float) <= 64 * 1024 && RO_EPB % IN_JEPT == 0, "the buffer is a static __shared__ array");
struct InArgs {
    SnapView first;              // snapshot 0 (or the handle's blocks); first.n = N envs
    long long stride_words;      // distance between consecutive snapshots, in 4-byte words
    long long total;             // n_snaps * N env-states
    const float* tab; int n_tab; // n_tab tables of LM_TABLE floats: one shared, or one per env (taken by env % n_tab)
    const float* ctrl;           // [total] actions, or null: 0
    float *qM, *qfrc, *qacc, *jac;
    int vec4;                    // every present output array is 16-byte aligned
};
__global__ __launch_bounds__(64) void jb_inertia_kernel(InArgs a) {
    __shared__ __attribute__((aligned(16))) float img[IN_LDS_FLOATS];
    const int tid = threadIdx.x, q = tid >> 2, leg = tid & 3;
    const long long first_es = (long long)blockIdx.x * RO_EPB;
    long long es = first_es + q;
    if (es >= a.total) es = a.total - 1;      // a lane past the end repeats the last env-state: its loads stay inside the blocks, its rows are never copied out
    const long long k = es / a.first.n, env = es - k * a.first.n;
    SnapView v = a.first;
    v.root += k * a.stride_words; v.leg += k * a.stride_words;
    const FwState<float> s = fw_load<float>(v, env, leg);
    const float ctrl = a.ctrl ? a.ctrl[es] : 0.f;
    InOut<float> o;
    o.qM = a.qM ? img + IN_LDS_QM + q * IN_QM : nullptr;
    o.qfrc = a.qfrc ? img + IN_LDS_QFRC + q * IN_QFRC : nullptr;
    o.qacc = a.qacc ? img + IN_LDS_QACC + q * IN_QACC : nullptr;
    o.jac = nullptr;
    InLane<float> L;
    float p[IN_NP];
    in_lane_a<float>(s, ctrl, a.tab + (size_t)(env % a.n_tab) * LM_TABLE, leg, o, L, p);
    const long long left = a.total - first_es;
    const int n_es = left < RO_EPB ? (int)left : RO_EPB;
    if (a.qM || a.qfrc || a.qacc) {
#pragma unroll
        for (int i = 0; i < IN_NP; i++)
            if (a.qacc || !((i >= IN_P_SCHUR && i < IN_P_RHS) || i >= IN_P_BZ)) p[i] = quad_sum(p[i]);      // (the Schur terms and B z are zeros unless qacc_smooth is asked for)
        in_lane_b<float>(L, p, leg, o);
        __syncthreads();
        if (a.qM) ro_store_segment(a.qM + (size_t)first_es * IN_QM, img + IN_LDS_QM, n_es * IN_QM, a.vec4, tid);
        if (a.qfrc) ro_store_segment(a.qfrc + (size_t)first_es * IN_QFRC, img + IN_LDS_QFRC, n_es * IN_QFRC, a.vec4, tid);
        if (a.qacc) ro_store_segment(a.qacc + (size_t)first_es * IN_QACC, img + IN_LDS_QACC, n_es * IN_QACC, a.vec4, tid);
    }
    if (!a.jac) return;
#pragma unroll 1
    for (int t = 0; t * IN_JEPT < n_es; t++) {
        __syncthreads();                      // the copy before this turn has read the buffer
        if (q / IN_JEPT == t) in_jac<float>(L, leg, img + (q % IN_JEPT) * IN_JAC);
        __syncthreads();
        const int n = n_es - t * IN_JEPT < IN_JEPT ? n_es - t * IN_JEPT : IN_JEPT;
        ro_store_segment(a.jac + (size_t)(first_es + t * IN_JEPT) * IN_JAC, img, n * IN_JAC, a.vec4, tid);
    }
}
#endif

}  // namespace jb

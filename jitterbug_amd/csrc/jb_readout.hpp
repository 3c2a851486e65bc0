// jb_readout.hpp — the readout pass: a state (the handle's blocks or a snapshot, jb_snapshot.hpp SnapView) -> world frames of every body
// and geom, signed floor clearance of every geom, body velocities, momentum and energy.  It reads the state and the constant tables
// the step kernels read (jb_sim.hpp LM_*) and writes nothing but its outputs.
//
// Outputs per env-state (each may be absent):
//   frames    [RO_NFRAME][12]  [pos(3) | R(9) row major], R takes frame-local vectors to world vectors (MuJoCo's xmat)
//                              0-9    the ten moving bodies (include/jitterbug_model.h order): pos = centre of mass (xipos), R = the body's
//                                     rotation from its orientation at qpos0
//                              10-31  the 22 geoms in the parameter table's order: pos = geom centre, R = geom frame (cylinder axis = column 2)
//                              32     the target: (tx, ty, target z), rotation about z by the target yaw
//   clearance [22]             smallest height of the geom's surface above the plane z = 0 (negative: it reaches below the floor)
//   body_vel  [10][6]          world linear velocity of the body's centre of mass, world angular velocity
//   energy    [8]              P(3), L(3) about the world origin, kinetic T, potential V (gravity + the hinge springs)
//
// Lane mapping: the step kernels' - FOUR LANES PER ENV-STATE, lane l owns leg l (its two bodies, its four geoms) and a share of the rest:
// lane 0 the root body and coreBody1, lane 1 coreBody2 and the target, lane 2 screw1 / screw2, lane 3 the motor body with threadMass / mass.
// `energy` is the quad sum of the lanes' partial sums.  The element function is written once on the real type: the device runs it in
// fp32 (jb_readout_kernel below), tests/readout_harness.cpp runs the same source on the host in fp32 and fp64.
//
// The height and the quaternion come as hi + lo words.  The height's low word is added LAST to every world z ((pz + z_rel) + pz_lo, as the
// step kernel's floor tests do): a clearance is a difference of nearly equal heights.  The quaternion's low words enter the rotation's
// quadratic forms at first order.  The motor angle is wrapped angle + whole turns; every output is periodic in it, so only the wrapped
// angle is read.
#pragma once
#include "jb_sim.hpp"
#include "jb_snapshot.hpp"

namespace jb {

constexpr int RO_NFRAME = 33, RO_NGEOM = 22, RO_NBODY = 10;
constexpr int RO_FRAME_W = 12, RO_FRAMES = RO_NFRAME * RO_FRAME_W, RO_CLEAR = RO_NGEOM, RO_BVEL = RO_NBODY * 6, RO_ENERGY = 8;
constexpr int RO_FRAME_GEOM0 = RO_NBODY, RO_FRAME_TARGET = RO_NBODY + RO_NGEOM;

// where one env-state's outputs go (a null pointer: that output is absent)
template <typename T> struct RoOut { T* frames; T* clear; T* bvel; T* energy; };

// what a lane reads of the state: the root's replicated fields and its own leg's
template <typename T> struct RoState {
    T px, py, pz, pz_lo, q[4], ql[4], vx, vy, vz, wx, wy, wz, phi, phid, tx, ty, tpsi;
    T th1, th2, thd1, thd2;
};
JB_HD float ro_word(uint32_t w) { return __builtin_bit_cast(float, w); }
// state field indices (jb_api.hip RootF / LegF; static_assert there)
constexpr int RO_RF_P = 0, RO_RF_Q = 3, RO_RF_V = 7, RO_RF_W = 10, RO_RF_PHI = 13, RO_RF_PHID = 14, RO_RF_TGT = 24, RO_RF_LO = 27;
constexpr int RO_LF_TH1 = 0, RO_LF_TH2 = 1, RO_LF_THD1 = 2, RO_LF_THD2 = 3;
// env in [0, v.n), leg in [0, 4): root words are read at [field][env] (the four lanes of a quad read one word), leg words at [field][4 env + leg]
template <typename T> JB_HD RoState<T> ro_load(const SnapView& v, long long env, int leg) {
    const long long N = v.n;
    auto R = [&](int f) { return (T)ro_word(v.root[(long long)f * N + env]); };
    auto L = [&](int f) { return (T)ro_word(v.leg[(long long)f * 4 * N + 4 * env + leg]); };
    RoState<T> s;
    s.px = R(RO_RF_P); s.py = R(RO_RF_P + 1); s.pz = R(RO_RF_P + 2); s.pz_lo = R(RO_RF_LO);
    for (int i = 0; i < 4; i++) { s.q[i] = R(RO_RF_Q + i); s.ql[i] = R(RO_RF_LO + 1 + i); }
    s.vx = R(RO_RF_V); s.vy = R(RO_RF_V + 1); s.vz = R(RO_RF_V + 2);
    s.wx = R(RO_RF_W); s.wy = R(RO_RF_W + 1); s.wz = R(RO_RF_W + 2);
    s.phi = R(RO_RF_PHI); s.phid = R(RO_RF_PHID);
    s.tx = R(RO_RF_TGT); s.ty = R(RO_RF_TGT + 1); s.tpsi = R(RO_RF_TGT + 2);
    s.th1 = L(RO_LF_TH1); s.th2 = L(RO_LF_TH2); s.thd1 = L(RO_LF_THD1); s.thd2 = L(RO_LF_THD2);
    return s;
}

// rotation of the quaternion (h + l) / |h + l|: every product h_i h_j of the quadratic forms carries its first-order correction
template <typename T> JB_HD Mat3<T> ro_quat2mat(const T (&h)[4], const T (&l)[4]) {
    auto pr = [&](int i, int j) { return h[i] * h[j] + (h[i] * l[j] + l[i] * h[j]); };
    const T ww = pr(0, 0), xx = pr(1, 1), yy = pr(2, 2), zz = pr(3, 3), wx = pr(0, 1), wy = pr(0, 2), wz = pr(0, 3), xy = pr(1, 2), xz = pr(1, 3), yz = pr(2, 3);
    const T inv = T(1) / ((ww + xx) + (yy + zz)), inv2 = inv + inv;
    Mat3<T> R;
    R.m[0] = ((ww + xx) - (yy + zz)) * inv; R.m[1] = (xy - wz) * inv2;              R.m[2] = (xz + wy) * inv2;
    R.m[3] = (xy + wz) * inv2;              R.m[4] = ((ww - xx) + (yy - zz)) * inv; R.m[5] = (yz - wx) * inv2;
    R.m[6] = (xz - wy) * inv2;              R.m[7] = (yz + wx) * inv2;              R.m[8] = ((ww - xx) - (yy - zz)) * inv;
    return R;
}
template <typename T> JB_HD Mat3<T> ro_identity() { Mat3<T> R; for (int i = 0; i < 9; i++) R.m[i] = T(i % 4 == 0 ? 1 : 0); return R; }
// geom frame of a cylinder from its axis (column 2) and its x axis (column 0): column 1 = axis x xaxis
template <typename T> JB_HD Mat3<T> ro_cyl_frame(const Vec3<T>& ax, const Vec3<T>& xa) {
    const Vec3<T> ya = cross(ax, xa);
    Mat3<T> R;
    R.m[0] = xa.x; R.m[1] = ya.x; R.m[2] = ax.x; R.m[3] = xa.y; R.m[4] = ya.y; R.m[5] = ax.y; R.m[6] = xa.z; R.m[7] = ya.z; R.m[8] = ax.z;
    return R;
}

// the root's world pose, with the floor normal in root coordinates (row 2 of R0) and the height as hi + lo
template <typename T> struct RoRoot { Mat3<T> R0; Vec3<T> nb; T px, py, pz, pz_lo; };
template <typename T> JB_HD Vec3<T> ro_world(const RoRoot<T>& r, const Vec3<T>& c) {
    const Vec3<T> t = mul(r.R0, c);
    return v3<T>(r.px + t.x, r.py + t.y, (r.pz + t.z) + r.pz_lo);
}
template <typename T> JB_HD void ro_put_frame(T* frames, int f, const Vec3<T>& pos, const Mat3<T>& R) {
    T* o = frames + f * RO_FRAME_W;
    o[0] = pos.x; o[1] = pos.y; o[2] = pos.z;
    for (int i = 0; i < 9; i++) o[3 + i] = R.m[i];
}
// One geom, given in ROOT coordinates (centre c, frame Rg): its frame row and its clearance.  type: include/jitterbug_model.h JB_GEOM_*
// (0 sphere: s.x = r; 1 cylinder: s.x = r, s.y = half length; 2 box, 3 ellipsoid: half sizes).  The support height below the centre is
// taken off the centre's height BEFORE the root height's words are added: (pz + (z_rel - support)) + pz_lo.
template <typename T> JB_HD void ro_geom(const RoOut<T>& o, const RoRoot<T>& r, int g, int type, const Vec3<T>& c, const Mat3<T>& Rg, const Vec3<T>& s) {
    if (o.frames) ro_put_frame(o.frames, RO_FRAME_GEOM0 + g, ro_world(r, c), mul(r.R0, Rg));
    if (o.clear) {
        const Vec3<T> z = mulT(Rg, r.nb);            // row 2 of the world frame: R_20, R_21, R_22
        T sup;
        if (type == 0) sup = s.x;
        else if (type == 1) sup = s.y * vabs(z.z) + s.x * vsqrt(vmax(T(0), T(1) - z.z * z.z));
        else if (type == 2) sup = s.x * vabs(z.x) + s.y * vabs(z.y) + s.z * vabs(z.z);
        else { const T a = s.x * z.x, b = s.y * z.y, d = s.z * z.z; sup = vsqrt(a * a + b * b + d * d); }
        o.clear[g] = (r.pz + (dot(r.nb, c) - sup)) + r.pz_lo;
    }
}
// One body, given in ROOT coordinates (rotation Rj from its orientation at qpos0, centre of mass c, velocity u of the centre of mass relative
// to the root origin's, angular velocity w): frame row, velocity row and its terms of [P, L, T, V] added to e.
template <typename T> JB_HD void ro_body(const RoOut<T>& o, const RoRoot<T>& r, const Vec3<T>& v0, const Vec3<T>& grav, int b, const Mat3<T>& Rj, const Vec3<T>& c,
                                         const Vec3<T>& u, const Vec3<T>& w, const T& m, const Sym3<T>& I, T (&e)[8]) {
    const Vec3<T> cw = ro_world(r, c), vc = v0 + mul(r.R0, u), ww = mul(r.R0, w);
    if (o.frames) ro_put_frame(o.frames, b, cw, mul(r.R0, Rj));
    if (o.bvel) { T* q = o.bvel + 6 * b; q[0] = vc.x; q[1] = vc.y; q[2] = vc.z; q[3] = ww.x; q[4] = ww.y; q[5] = ww.z; }
    const Vec3<T> hr = mul(Rj, mul(I, mulT(Rj, w)));      // angular momentum about the centre of mass, root coordinates
    const Vec3<T> hw = mul(r.R0, hr), l = cross(cw, vc);
    e[0] += m * vc.x; e[1] += m * vc.y; e[2] += m * vc.z;
    e[3] += hw.x + m * l.x; e[4] += hw.y + m * l.y; e[5] += hw.z + m * l.z;
    e[6] += T(0.5) * m * dot(vc, vc) + T(0.5) * dot(w, hr);
    e[7] -= m * dot(grav, cw);
}

// Everything lane `leg` of an env-state's quad contributes: its rows of frames / clearance / body_vel (written through o) and its partial
// sums of energy (e, overwritten).  tab: the env's packed constant table (LM_TABLE entries).
template <typename T> JB_HD void ro_lane(const RoState<T>& s, const T* tab, int leg, const RoOut<T>& o, T (&e)[8]) {
    auto C = [&](int i) { return tab[lm_offset(i, leg)]; };
    auto C3 = [&](int i) { return v3<T>(C(i), C(i + 1), C(i + 2)); };
    auto CS = [&](int i) { Sym3<T> q; q.xx = C(i); q.yy = C(i + 1); q.zz = C(i + 2); q.xy = C(i + 3); q.xz = C(i + 4); q.yz = C(i + 5); return q; };
    auto CM = [&](int i) { Mat3<T> q; for (int k = 0; k < 9; k++) q.m[k] = C(i + k); return q; };
    for (int i = 0; i < 8; i++) e[i] = T(0);
    RoRoot<T> r;
    r.R0 = ro_quat2mat(s.q, s.ql);
    r.nb = v3<T>(r.R0.m[6], r.R0.m[7], r.R0.m[8]);
    r.px = s.px; r.py = s.py; r.pz = s.pz; r.pz_lo = s.pz_lo;
    const Vec3<T> v0 = v3<T>(s.vx, s.vy, s.vz), w0 = v3<T>(s.wx, s.wy, s.wz), grav = C3(LM_GRAV);
    const Vec3<T> zero = v3<T>(T(0), T(0), T(0));

    // ---- the lane's own leg: upper body 1 + 2 leg (shoulder hinge), lower body 2 + 2 leg (knee hinge on the upper body)
    T s1, c1, s2, c2;
    vsincos_pi(s.th1, s1, c1); vsincos_pi(s.th2, s2, c2);
    const Vec3<T> a1 = C3(LM_A1), e1 = C3(LM_E1);
    const Mat3<T> R1 = rodrigues(e1, s1, c1), R12 = mul(R1, rodrigues(C3(LM_E2), s2, c2));
    const Vec3<T> a2 = a1 + mul(R1, C3(LM_DA2)), e2 = mul(R1, C3(LM_E2));
    const Vec3<T> cu = a1 + mul(R1, C3(LM_DC1)), cl = a2 + mul(R12, C3(LM_DC2));
    const Vec3<T> w1 = w0 + e1 * s.thd1, w2 = w1 + e2 * s.thd2;
    const Vec3<T> uu = cross(w0, cu) + cross(e1, cu - a1) * s.thd1;
    const Vec3<T> ul = cross(w0, cl) + cross(e1, cl - a1) * s.thd1 + cross(e2, cl - a2) * s.thd2;
    ro_body(o, r, v0, grav, 1 + 2 * leg, R1, cu, uu, w1, C(LM_M1), CS(LM_I1), e);
    ro_body(o, r, v0, grav, 2 + 2 * leg, R12, cl, ul, w2, C(LM_M2), CS(LM_I2), e);
    e[7] += T(0.5) * C(LM_K1) * s.th1 * s.th1 + T(0.5) * C(LM_K2) * s.th2 * s.th2;
    if (o.frames || o.clear) {
        const int g0 = 4 + 4 * leg;
        ro_geom(o, r, g0, 1, a1 + mul(R1, C3(LM_UC_D)), mul(R1, ro_cyl_frame(C3(LM_UC_AX), C3(LM_UC_XA))), v3<T>(C(LM_UC_R), C(LM_UC_H), T(0)));
        ro_geom(o, r, g0 + 1, 0, a1 + mul(R1, C3(LM_DTIP)), R1, v3<T>(C(LM_TIP_R), T(0), T(0)));
        ro_geom(o, r, g0 + 2, 1, a2 + mul(R12, C3(LM_LC_D)), mul(R12, ro_cyl_frame(C3(LM_LC_AX), C3(LM_LC_XA))), v3<T>(C(LM_LC_R), C(LM_LC_H), T(0)));
        ro_geom(o, r, g0 + 3, 0, a2 + mul(R12, C3(LM_DFOOT)), R12, v3<T>(C(LM_FOOT_R), T(0), T(0)));
    }

    // ---- the lane's share of the root body, the motor body and the target
    if (leg == 0) ro_body(o, r, v0, grav, 0, ro_identity<T>(), C3(LM_C0), cross(w0, C3(LM_C0)), w0, C(LM_M0), CS(LM_I0), e);
    if (leg < 2) {
        if (o.frames || o.clear) ro_geom(o, r, leg, 2, C3(LM_XB_C), CM(LM_XB_R), C3(LM_XB_S));
        if (leg == 1 && o.frames) {
            T st, ct;
            vsincos_pi(s.tpsi, st, ct);
            Mat3<T> Rt = ro_identity<T>();
            Rt.m[0] = ct; Rt.m[1] = -st; Rt.m[3] = st; Rt.m[4] = ct;
            ro_put_frame(o.frames, RO_FRAME_TARGET, v3<T>(s.tx, s.ty, C(LM_TARGET_Z)), Rt);
        }
    } else {
        // lane 2: screw1 / screw2 on the root body; lane 3: threadMass / mass on the motor body, turned about the motor hinge
        Mat3<T> Rx = ro_identity<T>();
        Vec3<T> ax = zero;
        if (leg == 3) {
            T sp, cp;
            vsincos_pi(s.phi, sp, cp);
            const Vec3<T> am = C3(LM_AM), em = C3(LM_EM);
            Rx = rodrigues(em, sp, cp); ax = am;
            const Vec3<T> cm = am + mul(Rx, C3(LM_DCM));
            ro_body(o, r, v0, grav, 9, Rx, cm, cross(w0, cm) + cross(em, cm - am) * s.phid, w0 + em * s.phid, C(LM_MM), CS(LM_IM), e);
        }
        if (o.frames || o.clear) {
            const int gc = leg == 3 ? 20 : 2, ge = leg == 3 ? 21 : 3;
            ro_geom(o, r, gc, 1, ax + mul(Rx, C3(LM_XC_C) - ax), mul(Rx, ro_cyl_frame(C3(LM_XC_AX), C3(LM_XC_XA))), v3<T>(C(LM_XC_R), C(LM_XC_H), T(0)));
            ro_geom(o, r, ge, 3, ax + mul(Rx, C3(LM_XE_C) - ax), mul(Rx, CM(LM_XE_R)), C3(LM_XE_S));
        }
    }
}
// energy of an env-state from its four lanes' partial sums, associated like the device's quad reduction: (e0 + e1) + (e2 + e3)
template <typename T> JB_HD T ro_quad_total(const T& e0, const T& e1, const T& e2, const T& e3) { return (e0 + e1) + (e2 + e3); }

#if defined(__HIPCC__)
// ---- the device pass.  One wave per block, RO_EPB env-states per block (a quad each).  Env-state es = snapshot es / N, env es % N.  The
// state loads are field-major: a root field is one 64-byte run of the block's 16 envs (each word read by the four lanes of its quad), a leg
// field one 256-byte run.  Every output leaves the block as ONE contiguous segment: the lanes write their rows into an LDS image of the
// block's part of each output array ([RO_EPB][len], the arrays' own layout), and the wave then copies each present image out in 16-byte
// words (the segments start at multiples of 16 env-states, so they are 16-byte aligned whenever the array is).  An absent output is
// neither computed into LDS nor stored.
constexpr int RO_EPB = 16;
constexpr int RO_LDS_FRAMES = 0, RO_LDS_CLEAR = RO_LDS_FRAMES + RO_EPB * RO_FRAMES, RO_LDS_BVEL = RO_LDS_CLEAR + RO_EPB * RO_CLEAR,
              RO_LDS_ENERGY = RO_LDS_BVEL + RO_EPB * RO_BVEL, RO_LDS_FLOATS = RO_LDS_ENERGY + RO_EPB * RO_ENERGY;
static_assert(RO_LDS_CLEAR % 4 == 0 && RO_LDS_BVEL % 4 == 0 && RO_LDS_ENERGY % 4 == 0, "every LDS image starts on a 16-byte word");
static_assert((RO_EPB * RO_FRAMES) % 4 == 0 && (RO_EPB * RO_CLEAR) % 4 == 0 && (RO_EPB * RO_BVEL) % 4 == 0 && (RO_EPB * RO_ENERGY) % 4 == 0, "a full block's segment is whole 16-byte words");
struct RoArgs {
    SnapView first;              // snapshot 0 (or the handle's blocks); first.n = N envs
    long long stride_words;      // distance between consecutive snapshots, in 4-byte words (every block pointer moves by it)
    long long total;             // n_snaps * N env-states
    const float* tab; int n_tab; // n_tab tables of LM_TABLE floats: one shared, or one per env (taken by env % n_tab)
    float *frames, *clear, *bvel, *energy;
    int vec4;                    // every present output array is 16-byte aligned
};
// n floats from an LDS image to its global segment, 16-byte words where `vec4`, the last n % 4 floats (a ragged last block) one by one
JB_D void ro_store_segment(float* __restrict__ dst, const float* src, int n, int vec4, int tid) {
    const int nv = vec4 ? n >> 2 : 0;
    for (int i = tid; i < nv; i += 64) ((float4*)dst)[i] = ((const float4*)src)[i];
    for (int i = 4 * nv + tid; i < n; i += 64) dst[i] = src[i];
}
__global__ __launch_bounds__(64) void jb_readout_kernel(RoArgs a) {
    __shared__ __attribute__((aligned(16))) float img[RO_LDS_FLOATS];
    const int tid = threadIdx.x, q = tid >> 2, leg = tid & 3;
    const long long first_es = (long long)blockIdx.x * RO_EPB;
    long long es = first_es + q;
    if (es >= a.total) es = a.total - 1;      // a lane past the end repeats the last env-state: its loads stay inside the blocks, its rows are never copied out
    const long long k = es / a.first.n, env = es - k * a.first.n;
    SnapView v = a.first;
    v.root += k * a.stride_words; v.leg += k * a.stride_words;
    const RoState<float> s = ro_load<float>(v, env, leg);
    RoOut<float> o;
    o.frames = a.frames ? img + RO_LDS_FRAMES + q * RO_FRAMES : nullptr;
    o.clear = a.clear ? img + RO_LDS_CLEAR + q * RO_CLEAR : nullptr;
    o.bvel = a.bvel ? img + RO_LDS_BVEL + q * RO_BVEL : nullptr;
    o.energy = a.energy ? img + RO_LDS_ENERGY + q * RO_ENERGY : nullptr;
    float e[8];
    ro_lane<float>(s, a.tab + (size_t)(env % a.n_tab) * LM_TABLE, leg, o, e);
    if (o.energy) {
#pragma unroll
        for (int i = 0; i < 8; i++) { const float t = quad_sum(e[i]); if (leg == (i & 3)) o.energy[i] = t; }
    }
    __syncthreads();
    const long long left = a.total - first_es;
    const int n_es = left < RO_EPB ? (int)left : RO_EPB;
    if (a.frames) ro_store_segment(a.frames + (size_t)first_es * RO_FRAMES, img + RO_LDS_FRAMES, n_es * RO_FRAMES, a.vec4, tid);
    if (a.clear) ro_store_segment(a.clear + (size_t)first_es * RO_CLEAR, img + RO_LDS_CLEAR, n_es * RO_CLEAR, a.vec4, tid);
    if (a.bvel) ro_store_segment(a.bvel + (size_t)first_es * RO_BVEL, img + RO_LDS_BVEL, n_es * RO_BVEL, a.vec4, tid);
    if (a.energy) ro_store_segment(a.energy + (size_t)first_es * RO_ENERGY, img + RO_LDS_ENERGY, n_es * RO_ENERGY, a.vec4, tid);
}
#endif

}  // namespace jb

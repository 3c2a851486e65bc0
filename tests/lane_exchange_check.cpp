// Stand-alone host check of jb_lane.hpp's DPP vocabulary (tests/test_lane_exchanges_cpu.py builds and runs it):
//   1. dpp_every_lane_has_a_source(ctrl) - the condition under which dpp_mov may set bound_ctrl - against a lane-by-lane model of the DPP
//      controls written from the instruction set manual: true for a control only if all 64 lanes have a source lane, true for every quad
//      permutation and row rotation, false for every shift and row broadcast;
//   2. the controls the device helpers pass (dpp_quad_rot_ctrl, dpp_quad_bcast_ctrl, DPP_QUAD_XOR1/2, DPP_ROW_ROR4/8) against the host
//      emulation of the same helpers (Quad<T>): the model moves values the way the control says, the emulation the way jb_sim.hpp is tested
//      on the host - same lanes, same bits, fp32 and fp64, random and special values (+-0, infinities, denormals, extremes) in all four
//      quad positions, every rotation and every broadcast, quad_sum's two butterfly stages, quad_pick's four broadcasts and selects.
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../jitterbug_amd/csrc/jb_lane.hpp"

using namespace jb;

// source lane of `lane` (0-63) under a 9-bit DPP control, -1 where the lane has none (or the control is reserved)
static int dpp_src(int ctrl, int lane) {
    const int row = lane & ~15, r = lane & 15;
    if (ctrl >= 0x000 && ctrl <= 0x0FF) return (lane & ~3) | ((ctrl >> (2 * (lane & 3))) & 3);      // quad_perm
    if (ctrl >= 0x101 && ctrl <= 0x10F) { const int n = ctrl & 15; return r + n <= 15 ? lane + n : -1; }      // row_shl
    if (ctrl >= 0x111 && ctrl <= 0x11F) { const int n = ctrl & 15; return r >= n ? lane - n : -1; }           // row_shr
    if (ctrl >= 0x121 && ctrl <= 0x12F) { const int n = ctrl & 15; return row | ((r - n) & 15); }             // row_ror
    if (ctrl == 0x130) return lane < 63 ? lane + 1 : -1;      // wave_shl:1
    if (ctrl == 0x134) return (lane + 1) & 63;                // wave_rol:1
    if (ctrl == 0x138) return lane > 0 ? lane - 1 : -1;       // wave_shr:1
    if (ctrl == 0x13C) return (lane - 1) & 63;                // wave_ror:1
    if (ctrl == 0x140) return row | (15 - r);                 // row_mirror
    if (ctrl == 0x141) return (lane & ~7) | (7 - (lane & 7)); // row_half_mirror
    if (ctrl == 0x142) return lane >= 16 ? row - 1 : -1;      // row_bcast:15 (lane 15 of a row to the next row)
    if (ctrl == 0x143) return lane >= 32 ? 31 : -1;           // row_bcast:31
    return -1;
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

template <typename T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

// a quad's four values moved the way the control says (the quad sits at lanes 4q .. 4q+3 of the wave: every quad of the wave is tried)
template <typename T> static Quad<T> model_move(int ctrl, const Quad<T>& x, int q) {
    Quad<T> r;
    for (int i = 0; i < 4; i++) {
        const int s = dpp_src(ctrl, 4 * q + i);
        r.v[i] = (s >= 4 * q && s < 4 * q + 4) ? x.v[s - 4 * q] : std::numeric_limits<T>::quiet_NaN();      // (a source outside the quad: not a quad exchange)
    }
    return r;
}

template <typename T> static std::vector<T> values() {
    using L = std::numeric_limits<T>;
    std::vector<T> v = {T(0), -T(0), L::infinity(), -L::infinity(), L::denorm_min(), -L::denorm_min(), L::min(), -L::min() / 2, L::max(), L::lowest(), T(1), T(-1), L::epsilon()};
    std::mt19937_64 g(12345);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (int i = 0; i < 51; i++) v.push_back((T)(u(g) * std::pow(10.0, (double)(i % 9 - 4))));
    return v;
}

template <typename T, int K> static void check_rot(const Quad<T>& x, int q) {
    const Quad<T> want = model_move(dpp_quad_rot_ctrl(K), x, q), got = quad_rot<K>(x);
    for (int i = 0; i < 4; i++) CHECK(same_bits(want.v[i], got.v[i]), "quad_rot<%d> lane %d of quad %d", K, i, q);
}
template <typename T, int J> static void check_bcast(const Quad<T>& x, int q) {
    const Quad<T> want = model_move(dpp_quad_bcast_ctrl(J), x, q), got = quad_bcast<J>(x);
    for (int i = 0; i < 4; i++) CHECK(same_bits(want.v[i], got.v[i]), "quad_bcast<%d> lane %d of quad %d", J, i, q);
}

template <typename T> static void check_values() {
    const std::vector<T> v = values<T>();
    const int n = (int)v.size();
    for (int a = 0; a < n; a++) {
        for (int pos = 0; pos < 4; pos++) {          // value a in position pos, three others drawn from the list
            Quad<T> x(v[(a + 7) % n], v[(a + 19) % n], v[(a + 31) % n], v[(a + 43) % n]);
            x.v[pos] = v[a];
            const int q = (a + pos) & 15;
            check_rot<T, 1>(x, q); check_rot<T, 2>(x, q); check_rot<T, 3>(x, q);
            check_bcast<T, 0>(x, q); check_bcast<T, 1>(x, q); check_bcast<T, 2>(x, q); check_bcast<T, 3>(x, q);
            // quad_sum on the device: x += x[lane ^ 1], then x += x[lane ^ 2], in every lane
            Quad<T> s = x;
            s = s + model_move(DPP_QUAD_XOR1, s, q);
            s = s + model_move(DPP_QUAD_XOR2, s, q);
            const Quad<T> hs = quad_sum(x);
            const bool nan = s.v[0] != s.v[0];       // (inf - inf: which NaN comes out is no property of the exchange)
            for (int i = 0; i < 4; i++) CHECK(nan ? hs.v[i] != hs.v[i] : same_bits(s.v[i], hs.v[i]), "quad_sum lane %d, value %d at %d", i, a, pos);
            // quad_pick on the device: four broadcasts, then selects on the two bits of src
            for (int rot = 0; rot < 4; rot++) {
                const UQuad src{{(uint32_t)rot, (uint32_t)((rot + 1) & 3), (uint32_t)((rot * 3 + 2) & 3), (uint32_t)(3 - rot)}};
                Quad<T> b[4];
                for (int j = 0; j < 4; j++) b[j] = model_move(dpp_quad_perm_ctrl(j, j, j, j), x, q);
                const Quad<T> hp = quad_pick(x, src);
                for (int i = 0; i < 4; i++) {
                    const T lo = (src.v[i] & 1u) ? b[1].v[i] : b[0].v[i], hi = (src.v[i] & 1u) ? b[3].v[i] : b[2].v[i];
                    CHECK(same_bits((src.v[i] & 2u) ? hi : lo, hp.v[i]), "quad_pick lane %d src %u", i, src.v[i]);
                }
            }
        }
    }
    // the unsigned forms take the same controls
    const UQuad u{{0x80000001u, 2u, 0xFFFFFFFFu, 0x12345678u}};
    const UQuad r1 = quad_rot_u<1>(u), r2 = quad_rot_u<2>(u), r3 = quad_rot_u<3>(u), b2 = quad_bcast_u<2>(u), su = quad_sum_u(u);
    for (int i = 0; i < 4; i++) {
        CHECK(r1.v[i] == u.v[dpp_src(dpp_quad_rot_ctrl(1), i)] && r2.v[i] == u.v[dpp_src(dpp_quad_rot_ctrl(2), i)] && r3.v[i] == u.v[dpp_src(dpp_quad_rot_ctrl(3), i)], "quad_rot_u lane %d", i);
        CHECK(b2.v[i] == u.v[dpp_src(dpp_quad_bcast_ctrl(2), i)], "quad_bcast_u lane %d", i);
        CHECK(su.v[i] == u.v[0] + u.v[1] + u.v[2] + u.v[3], "quad_sum_u lane %d", i);
    }
}

int main() {
    // 1. the predicate against the model
    for (int ctrl = 0; ctrl < 0x200; ctrl++) {
        bool all = true;
        for (int lane = 0; lane < 64; lane++) all = all && dpp_src(ctrl, lane) >= 0;
        if (dpp_every_lane_has_a_source(ctrl)) CHECK(all, "control 0x%03x may set bound_ctrl, but a lane has no source", ctrl);
        const bool quad_or_ror = ctrl <= 0xFF || (ctrl >= 0x121 && ctrl <= 0x12F);
        const bool shift_or_bcast = (ctrl >= 0x101 && ctrl <= 0x10F) || (ctrl >= 0x111 && ctrl <= 0x11F) || ctrl == 0x130 || ctrl == 0x138 || ctrl == 0x142 || ctrl == 0x143;
        if (quad_or_ror) CHECK(dpp_every_lane_has_a_source(ctrl) && all, "control 0x%03x is a quad permutation or a row rotation", ctrl);
        if (shift_or_bcast) CHECK(!dpp_every_lane_has_a_source(ctrl) && !all, "control 0x%03x leaves lanes without a source", ctrl);
    }
    // 2. the controls in use: named constants against their meaning
    CHECK(dpp_quad_rot_ctrl(1) == 0x39 && dpp_quad_rot_ctrl(2) == 0x4E && dpp_quad_rot_ctrl(3) == 0x93, "rotation controls");
    CHECK(dpp_quad_bcast_ctrl(0) == 0x00 && dpp_quad_bcast_ctrl(1) == 0x55 && dpp_quad_bcast_ctrl(2) == 0xAA && dpp_quad_bcast_ctrl(3) == 0xFF, "broadcast controls");
    for (int lane = 0; lane < 64; lane++) {
        CHECK(dpp_src(DPP_QUAD_XOR1, lane) == (lane ^ 1) && dpp_src(DPP_QUAD_XOR2, lane) == (lane ^ 2), "quad xor controls, lane %d", lane);
        CHECK(dpp_src(DPP_ROW_ROR8, lane) == (lane ^ 8), "row_ror:8 is the xor with 8, lane %d", lane);
        // row_ror:4 reads lane ^ 4 or that lane's partner eight lanes on: equal values once the xor-8 stage has run (xor_sum's sym2)
        const int s = dpp_src(DPP_ROW_ROR4, lane);
        CHECK(s == (lane ^ 4) || s == (lane ^ 4 ^ 8), "row_ror:4, lane %d", lane);
    }
    check_values<float>();
    check_values<double>();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}

// [k]B + [l]P on the device: the kernel that joins the comb's half and the ladder's half of a double-scalar multiplication
// (what a Schnorr-type verification R' = [s]B + [h]A needs) and lowers the sum to its canonical affine point, its 32-byte
// encoding, or one byte "the encoding equals the expected one".  Included by fourq_chain.hip only (FQ_CHAIN=1: the GF(p^2)
// products keep their carries inside the multiply-add chain, as normalize_kernel beside it).
//
// Both halves arrive as projective (X, Y, Z), each in the layout its producer writes: the comb's deferred flavour leaves planes of
// uint4 (store_proj, kernels.hip.h), the ladder rows of canonical words -- (X, Y, Z) at words 0, 4, 8 of a 12-word row behind the
// fused kernels (LADDER_IO_XYZ_OUT) or of a 20-word R1 row behind every other route.  No repacking pass in between.
//
// The addition is the projective twisted-Edwards addition for a = -1 (Bernstein, Birkner, Joye, Lange, Peters, "Twisted Edwards
// curves", section 6: 10M + 1S + 1D), complete on the whole curve because d is a non-square: doubling, inverse points, a neutral half
// and points outside the order-N subgroup take no branch.  It needs no Ta * Tb of either input, which (X, Y, Z) rows do not carry.
// Only 2d is a compiled-in constant (constants.inc), so the formulas run on doubled intermediates:
//     A = Z1 Z2     B' = 2 A^2     C = X1 X2     D = Y1 Y2     E' = 2d C D     F' = B' - E' = 2F     G' = B' + E' = 2G
//     X3 = (2A) F' ((X1 + Y1)(X2 + Y2) - C - D)     Y3 = (2A) G' (D + C)     Z3 = F' G'            = 4 x (X3, Y3, Z3) of the paper,
// the same projective point.  11 products + 1 square in GF(p^2); every operand's limb bound is in its type and every product's
// column bound is static_asserted by fe2_mul (fp127.hip.h), the widest being Z3 = F' G' with bounds 4 and 3.
//
// R1toAffine behind it as lower_kernel does it (fourq_amd.hip): lane t owns elements t, t + T, ..., t + (K-1) T with T = ceil(n / K)
// and inverts the product of their norms |Z3|^2 ONCE (Montgomery's trick; GFp2.inv = conj / norm, fields.py:193-199).  Z3 != 0 for any
// two points of the curve; pairs of field elements that are not on it (MUL_* checks nothing, and a key that fails to decode is lifted
// as the all-zero pair) can give Z3 = 0: such an element contributes a 1 to the lane's product, so it cannot touch the other K - 1
// elements of its lane, and gets conj(0) * (...) = (0, 0) itself.  The sums of the lane's K elements stay in registers between the two
// passes (30 limbs each): K = 2 takes 157 VGPRs and no scratch memory; K = 4 would fill all 256 of a two-wave kernel and spill.
#pragma once
#include "kernels.hip.h"

namespace fq {

namespace {

struct XYZ { Fe2<1> X, Y, Z; };

FQ_DEV XYZ add_projective(const Fe2<1>& X1, const Fe2<1>& Y1, const Fe2<1>& Z1, const Fe2<1>& X2, const Fe2<1>& Y2, const Fe2<1>& Z2) {
    const Fe2<1> A = fe2_mul(Z1, Z2);
    const Fe2<2> B2 = fe2_dbl(fe2_sqr(A));
    const Fe2<1> C = fe2_mul(X1, X2), D = fe2_mul(Y1, Y2);
    const Fe2<1> E2 = fe2_mul(fe2_mul(C, D), fe2_two_d());
    const Fe2<4> F2 = fe2_sub(B2, E2);
    const Fe2<3> G2 = fe2_add(B2, E2);
    const Fe2<5> H = fe2_sub(fe2_sub(fe2_mul(fe2_add(X1, Y1), fe2_add(X2, Y2)), C), D);
    const Fe2<2> A2 = fe2_dbl(A);
    XYZ r;
    r.X = fe2_mul(fe2_mul(A2, F2), H);
    r.Y = fe2_mul(fe2_mul(A2, G2), fe2_add(D, C));
    r.Z = fe2_mul(G2, F2);
    return r;
}

// proj / proj_stride: the comb's half (planes, kernels.hip.h store_proj); rows / row_stride: the ladder's half (12 or 20 words per
// element).  st_decode (COMBINE_ENCODE / COMBINE_VERIFY; may be NULL): decode status of the element's key -- non-zero zeroes the
// output, forces ok = 0 and is reported as FOURQ_BYTES_DECODE_BASE + itself.  COMBINE_VERIFY writes ok[i] and status[i] and nothing else.
template <int K, int OUT>
__global__ __launch_bounds__(BLOCK, 2) void combine_kernel(const uint4* proj, u32 proj_stride, const u64* rows, u32 row_stride, const uint8_t* st_decode,
                                                           const u64* expect, u64* out, uint8_t* status, uint8_t* ok, u32 n) {
    const u32 T = (n + K - 1) / K;
    const u32 t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= T) return;
    Fe<1> one;
    one.l[0] = 1; one.l[1] = one.l[2] = one.l[3] = one.l[4] = 0;
    XYZ s[K];
    Fe<1> nz[K], pre[K];
#pragma clang loop unroll(full)
    for (int j = 0; j < K; j++) {                     // a lane's slots past the end of the batch redo its first element and store nothing
        const u32 id = t + (u32)j * T, at = id < n ? id : t;
        Fe2<1> X1, Y1;
        load_proj_xy(proj, proj_stride, at, X1, Y1);
        const Fe2<1> Z1 = load_proj_z(proj, proj_stride, at);
        const u64* row = rows + row_stride * (size_t)at;
        s[j] = add_projective(X1, Y1, Z1, load_fe2(row), load_fe2(row + 4), load_fe2(row + 8));
        const Fe<1> norm = fe_carry(fe_add(fe_sqr(s[j].Z.re), fe_sqr(s[j].Z.im)));
        nz[j] = (K > 1) ? fe_select(fe_is_zero(norm) ? 0u : ~0u, norm, one) : norm;
        if (j == 0) pre[0] = nz[0]; else pre[j] = fe_mul(pre[j - 1], nz[j]);
        __builtin_amdgcn_sched_barrier(0);            // one addition after the other: interleaved, their temporaries would not fit the lane's registers
    }
    Fe<1> inv = fe_inv(pre[K - 1]);
#pragma clang loop unroll(full)
    for (int j = K - 1; j >= 0; j--) {
        const u32 id = t + (u32)j * T;
        Fe<1> ninv = inv;                                              // 1 / |Z_j|^2
        if (j > 0) { ninv = fe_mul(inv, pre[j - 1]); inv = fe_mul(inv, nz[j]); }
        Fe2<1> zi;
        zi.re = fe_mul(ninv, s[j].Z.re);                               // conj(Z) / |Z|^2     fields.py:193-199
        zi.im = fe_mul(ninv, fe_neg(s[j].Z.im));
        const Fe2<1> ax = fe2_mul(s[j].X, zi), ay = fe2_mul(s[j].Y, zi);
        if (id >= n) continue;
        if constexpr (OUT == COMBINE_AFFINE) {
            u64 o[8];
            store_fe2(o, ax); store_fe2(o + 4, ay);
            uint4* dst = reinterpret_cast<uint4*>(out + 8 * (size_t)id);
#pragma clang loop unroll(full)
            for (int k = 0; k < 4; k++) dst[k] = make_uint4((u32)o[2 * k], (u32)(o[2 * k] >> 32), (u32)o[2 * k + 1], (u32)(o[2 * k + 1] >> 32));
        } else {
            const uint8_t sd = st_decode ? st_decode[id] : (uint8_t)0;
            const uint8_t st = sd ? (uint8_t)(FOURQ_BYTES_DECODE_BASE + sd) : (uint8_t)0;
            u64 w[4];
            point_encode(ax, ay, w);
            if constexpr (OUT == COMBINE_ENCODE) {
                if (st) w[0] = w[1] = w[2] = w[3] = 0;
                uint4* dst = reinterpret_cast<uint4*>(out + 4 * (size_t)id);
                dst[0] = make_uint4((u32)w[0], (u32)(w[0] >> 32), (u32)w[1], (u32)(w[1] >> 32));
                dst[1] = make_uint4((u32)w[2], (u32)(w[2] >> 32), (u32)w[3], (u32)(w[3] >> 32));
            } else {
                const uint4* e = reinterpret_cast<const uint4*>(expect + 4 * (size_t)id);
                const uint4 e0 = e[0], e1 = e[1];
                const bool same = e0.x == (u32)w[0] && e0.y == (u32)(w[0] >> 32) && e0.z == (u32)w[1] && e0.w == (u32)(w[1] >> 32) &&
                                  e1.x == (u32)w[2] && e1.y == (u32)(w[2] >> 32) && e1.z == (u32)w[3] && e1.w == (u32)(w[3] >> 32);
                ok[id] = (same && !st) ? (uint8_t)1 : (uint8_t)0;
            }
            status[id] = st;
        }
    }
}

}  // namespace

}  // namespace fq

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
// R1toAffine behind it by the shared inversion of lower.hip.h.  Z3 != 0 for any two points of the curve; pairs of field elements that are not on it
// can give Z3 = 0 and are masked (K > 1).  The sums of the lane's K elements stay in registers between the two passes (30 limbs each): K = 2
// takes 157 VGPRs and no scratch memory; K = 4 would fill all 256 of a two-wave kernel and spill.
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
    LaneSlots<K> s(n);
    if (!s.lane(blockIdx.x * BLOCK + threadIdx.x)) return;
    XYZ sum[K];
    SharedInverse<K, FeOps<false>> si;
#pragma clang loop unroll(full)
    for (int j = 0; j < K; j++) {
        const u32 at = s.at(j);
        Fe2<1> X1, Y1;
        load_proj_xy(proj, proj_stride, at, X1, Y1);
        const Fe2<1> Z1 = load_proj_z(proj, proj_stride, at);
        const u64* row = rows + row_stride * (size_t)at;
        sum[j] = add_projective(X1, Y1, Z1, load_fe2(row), load_fe2(row + 4), load_fe2(row + 8));
        const Fe<1> norm = z_norm(sum[j].Z);
        if constexpr (K > 1) si.take(j, norm, !fe_is_zero(norm)); else si.take(j, norm);
        __builtin_amdgcn_sched_barrier(0);            // one addition after the other: interleaved, their temporaries would not fit the lane's registers
    }
    si.invert();
#pragma clang loop unroll(full)
    for (int j = K - 1; j >= 0; j--) {
        const Fe2<1> zi = z_inverse(sum[j].Z, si.peel(j));
        const Fe2<1> ax = fe2_mul(sum[j].X, zi), ay = fe2_mul(sum[j].Y, zi);
        if (!s.live(j)) continue;
        const u32 id = s.id(j);
        if constexpr (OUT == COMBINE_AFFINE) {
            put_affine(out, id, ax, ay);
        } else {
            const uint8_t st = bytes_decode_status(st_decode ? st_decode[id] : (uint8_t)0);
            if constexpr (OUT == COMBINE_ENCODE) put_encoded(out, status, id, ax, ay, st);
            else put_verdict(expect, ok, status, id, ax, ay, st);
        }
    }
}

}  // namespace

}  // namespace fq

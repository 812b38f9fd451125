// Signatures of registered keys: [k]B + [l]A_id where A_id is one of the public keys the context holds as one comb per key
// (fourq_keyset_set, fourq_amd.hip): the combs back to back, each of the single comb's object shape, as the generator set of the
// commitments (commit.hip.h, COMMIT_COMB_U32).  Included by fourq_chain.hip behind kernels.hip.h, whose comb it reuses.
//
//   keyset_order_kernel   one lane per key: [N]A by plain double-and-add over the bits of the constant N -- neither MUL_endo nor the
//                         comb is [k]P outside the subgroup of order N, and a comb is [k]A only for a key inside it.  N is public and the
//                         same for every lane: the control flow is uniform.
//   keyset_comb_kernel    256-lane blocks, one lane per row, no LDS.  The lane recodes both scalars and walks the generator's comb and
//                         comb `id` in ONE accumulator: per row of the comb one doubling, per column one mixed addition from each table,
//                         every entry read where it lies (as the gather route of commit_kernel).  The two scalars' even-scalar negations
//                         differ, so each is folded into its own table's per-column sign (keyset_digits) instead of being applied to
//                         the result.
//   keyset_lower_kernel   R1toAffine + encode of the 12-word rows; with VERIFY the comparison with R, ok and status instead of the bytes.
//   keyset_gather_kernel, keyset_fix_kernel   constant-time selection: a gathered address is a digit, so that mode runs the existing
//                         routes on the rows' key bytes, gathered by index, and this pair puts the key set's statuses on the result.
//
// A row's key index is clamped to the set wherever it becomes an address; an index outside the set is reported, never followed.
#pragma once
#include "kernels.hip.h"
#include "commit.hip.h"

namespace fq {

namespace {

FQ_DEV u32 keyset_clamp(u32 id, u32 count) { return id < count ? id : count - 1; }
// what a row inherits from its key: FOURQ_KEYSET_ID_RANGE, or the slot's own status (0 for an accepted key)
FQ_DEV uint8_t keyset_row_status(u32 id, u32 count, const uint8_t* key_status) {
    return id < count ? key_status[id] : (uint8_t)FOURQ_KEYSET_ID_RANGE;
}

// status[i]: in, decode's raw code; out, the slot's status: FOURQ_BYTES_DECODE_BASE + code, FOURQ_KEYSET_NOT_ORDER_N, or 0
__global__ __launch_bounds__(BLOCK) void keyset_order_kernel(const u64* affine, uint8_t* status, u32 m) {
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    const R1 P = affine_to_r1(load_fe2(affine + 8 * (size_t)i), load_fe2(affine + 8 * (size_t)i + 4));
    const R2s T = as_signed(r1_to_r2(P));
    R1 Q = P;
    int top = 255;
    while (!((ORDER_N[top >> 6] >> (top & 63)) & 1)) top--;
#pragma unroll 1
    for (int b = top - 1; b >= 0; b--) {
        Q = dbl(Q);
        if ((ORDER_N[b >> 6] >> (b & 63)) & 1) Q = add(Q, T);
    }
    u64 x[4], y[4], z[4];
    store_fe2(x, Q.X); store_fe2(y, Q.Y); store_fe2(z, Q.Z);
    const bool neutral = (x[0] | x[1] | x[2] | x[3]) == 0 && y[0] == z[0] && y[1] == z[1] && y[2] == z[2] && y[3] == z[3];
    const uint8_t raw = status[i];
    status[i] = raw ? (uint8_t)(FOURQ_BYTES_DECODE_BASE + raw) : neutral ? (uint8_t)0 : (uint8_t)FOURQ_KEYSET_NOT_ORDER_N;
}

// A scalar's recoding as the walk consumes it: the column visited t-th (t = (E - 1 - i) V + j) at bits [9 t, 9 t + 9) of 256 bits -- its
// table index and, in bit 8, "negate the entry", the even-scalar negation folded in ([k]B = -[N - k]B, and the negation of a sum of
// entries is the sum of the negated entries).  Eight registers per scalar instead of the ten of CombDigits: with the accumulator's 50
// limbs and an addition's temporaries, two recodings as planes do not fit the 128 registers of a lane at four waves per SIMD.
struct KeysetDigits { u32 w[8]; };
FQ_DEV KeysetDigits keyset_digits(const CombDigits<CombFast>& c) {
    using S = CombFast;
    static_assert(S::W == 9 && 9 * S::D <= 256, "nine bits per column, all columns in 256 bits");
    KeysetDigits d;
#pragma unroll
    for (int q = 0; q < 8; q++) d.w[q] = 0;
#pragma unroll
    for (int t = 0; t < S::D; t++) {
        const int col = S::E * (t % S::V) + (S::E - 1 - t / S::V), bit = 9 * t;
        const u32 v = comb_index(c, col) | ((comb_neg_mask(c, col) ^ c.negate) & 0x100u);
        d.w[bit >> 5] |= v << (bit & 31);
        if ((bit & 31) > 23) d.w[(bit >> 5) + 1] |= v >> (32 - (bit & 31));
    }
    return d;
}
FQ_DEV u32 keyset_next_digit(KeysetDigits& d) {            // the next column's nine bits; the rest moves down
    const u32 v = d.w[0] & 0x1ffu;
#pragma unroll
    for (int q = 0; q < 7; q++) d.w[q] = (d.w[q] >> 9) | (d.w[q + 1] << 23);
    d.w[7] >>= 9;
    return v;
}

// add_affine_table (curve.hip.h) -- the same products on the same operands, so the same bound annotations -- in the order that keeps the
// fewest values alive, and held to it: the entry's 2dxy first (with T, after which Ta and Tb are dead), then F and G (Z is dead), then the
// entry's x + y and y - x against X and Y.  Left to itself the scheduler starts all three loads of the entry at once, and beside two
// recodings that is more than a lane's 128 registers.
template <typename P> FQ_DEV R1 keyset_add(const R1& q, const P* entry, u32 neg_mask) {
    Fe2<4> Ta = q.Ta;
    Fe2<2> Tb = q.Tb;
    fe2_here(Ta); fe2_here(Tb);                                // as add_affine_table: keeps the 90 products single instructions
    const Fe2<1> T = fe2_mul_signed(Ta, Tb);
    const Fe2<1> C = fe2_mul_signed(fe2_cneg_signed(load_fe2_limbs(entry + 2 * COORD_U32), neg_mask), T);
    __builtin_amdgcn_sched_barrier(0);
    const Fe2<2> D = fe2_dbl(q.Z);
    const Fe2<3> G = fe2_add(D, C);
    const Fe2<3> F = fe2_sub_signed(D, C);                     // signed limbs: D - C has bound 3 and fits the 8*b operand
    __builtin_amdgcn_sched_barrier(0);
    Fe2<1> tN, tD;
    load_signed_nd<LimbSlots>(entry, neg_mask, tN, tD);
    const Fe2<1> B = fe2_mul_signed(fe2_add(q.X, q.Y), tN);
    const Fe2<1> A = fe2_mul_signed(fe2_sub_signed(q.Y, q.X), tD);
    __builtin_amdgcn_sched_barrier(0);
    const Fe2<2> E = fe2_sub_signed(B, A);
    const Fe2<2> H = fe2_add(B, A);
    R1 r;
    r.X = fe2_mul_signed(E, F);
    r.Z = fe2_mul_signed(G, F);
    r.Y = fe2_mul_signed(G, H);
    r.Ta = widen<4>(E);
    r.Tb = H;
    return r;
}

// rows[i] = [k_i]B + [l_i]A_id as a canonical 12-word (X, Y, Z) row.  pre (or NULL: the challenge kernel has written it): the row's
// inherited status.  Tail lanes redo row n - 1 and store nothing.
__global__ __launch_bounds__(BLOCK, 4) void keyset_comb_kernel(const u64* k, const u64* l, const u32* key_ids, const u32* comb_g, const u32* combs,
                                                               const uint8_t* key_status, u32 count, u64* rows, uint8_t* pre, u32 n) {
    using S = CombFast;
    // nothing but the digits, the key's slot and the accumulator lives across the walk: the row number is formed again behind it
    u32 key;
    KeysetDigits dg, da;
    {
        const u32 it = blockIdx.x * BLOCK + threadIdx.x, row = it < n ? it : n - 1;
        const u32 id = key_ids[row];
        key = keyset_clamp(id, count);
        if (pre && it < n) pre[row] = keyset_row_status(id, count, key_status);
        u64 m[4];
        load_scalar(k + 4 * (size_t)row, m);
        dg = keyset_digits(comb_recode<S>(m));
        load_scalar(l + 4 * (size_t)row, m);
        da = keyset_digits(comb_recode<S>(m));
    }
    R1 Q;
#pragma unroll 1
    for (int i = S::E - 1; i >= 0; i--) {
#pragma unroll 1
        for (int j = 0; j < S::V; j++) {
            {
                const u32 v = keyset_next_digit(dg);
                const u32* entry = comb_g + ((j << (S::W - 1)) + (v & 0xffu)) * COMB_ENTRY_U32;
                if (i == S::E - 1 && j == 0) {
                    Q = affine_table_start(entry, 0u - (v >> 8));
                } else {
                    if (j == 0) Q = dbl<Mul::Signed>(Q.X, Q.Y, Q.Z);
                    Q = keyset_add(Q, entry, 0u - (v >> 8));
                }
            }
            __builtin_amdgcn_sched_barrier(0);         // one addition after the other: with both entries' loads in flight the lane's registers do not suffice
            {
                const u32 v = keyset_next_digit(da);
                const u32* entry = combs + (size_t)key * COMMIT_COMB_U32 + ((j << (S::W - 1)) + (v & 0xffu)) * COMB_ENTRY_U32;
                Q = keyset_add(Q, entry, 0u - (v >> 8));
            }
        }
    }
    Q = r1_unsign(Q);
    const u32 row = blockIdx.x * BLOCK + threadIdx.x;
    if (row >= n) return;
    u64 w[12];
    store_fe2(w, Q.X); store_fe2(w + 4, Q.Y); store_fe2(w + 8, Q.Z);
    put_words<12>(rows + 12 * (size_t)row, w);
}

// One inversion per row (the lowering is a hundredth of the comb in front of it).  pre[i] != 0: ok = 0 or a zero row, and status = pre[i].
template <bool VERIFY>
__global__ __launch_bounds__(BLOCK) void keyset_lower_kernel(const u64* rows, const uint8_t* pre, const u64* expect, u64* out, uint8_t* ok, uint8_t* status, u32 n) {
    LaneSlots<1> s(n);
    if (!s.lane(blockIdx.x * BLOCK + threadIdx.x)) return;
    const u32 i = s.id(0);
    const u64* row = rows + 12 * (size_t)i;
    const Fe2<1> X = load_fe2(row), Y = load_fe2(row + 4), Z = load_fe2(row + 8);
    SharedInverse<1, FeOps<false>> si;
    si.take(0, z_norm(Z));                                         // nobody is masked
    si.invert();
    const Fe2<1> zi = z_inverse(Z, si.peel(0));
    if constexpr (VERIFY) put_verdict(expect, ok, status, i, fe2_mul(X, zi), fe2_mul(Y, zi), pre[i]);
    else put_encoded(out, status, i, fe2_mul(X, zi), fe2_mul(Y, zi), pre[i]);
}

// pk32[i] = the registered bytes of key id_i (of the last key for an index outside the set)
__global__ __launch_bounds__(BLOCK) void keyset_gather_kernel(const u32* key_ids, const uint8_t* key_bytes, u32 count, uint8_t* pk32, u32 n) {
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(key_bytes + 32 * (size_t)keyset_clamp(key_ids[i], count));
    uint4* dst = reinterpret_cast<uint4*>(pk32 + 32 * (size_t)i);
    dst[0] = src[0]; dst[1] = src[1];
}
// behind the existing routes: a row whose key is outside the set or refused gets that status, ok = 0 (ok != NULL) or a zero row (out != NULL)
__global__ __launch_bounds__(BLOCK) void keyset_fix_kernel(const u32* key_ids, const uint8_t* key_status, u32 count, u64* out, uint8_t* ok, uint8_t* status, u32 n) {
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t st = keyset_row_status(key_ids[i], count, key_status);
    if (!st) return;
    status[i] = st;
    if (ok) ok[i] = 0;
    if (out) {
        uint4* dst = reinterpret_cast<uint4*>(out + 4 * (size_t)i);
        dst[0] = make_uint4(0, 0, 0, 0); dst[1] = make_uint4(0, 0, 0, 0);
    }
}

}  // namespace

}  // namespace fq

// Bytes to a point (include/fourq_amd.h, "hash to curve"): RFC 9380's expand_message_xmd with SHA-512, hash_to_field into GF(p^2), the
// Montgomery-form Elligator 2, the rational map onto the twisted Edwards curve and the x392 chain -- kernels and launchers; included by
// fourq_amd.hip, whose C ABI strings them together.
//
// Hashing (h2f_kernel).  b_0 = H(Z_pad || msg || I2OSP(len_in_bytes, 2) || 0x00 || DST_prime), b_1 = H(b_0 || 0x01 || DST_prime),
// b_2 = H((b_0 xor b_1) || 0x02 || DST_prime).  Everything but msg and the digests is the same for every lane and travels BY VALUE in
// the kernel arguments (H2cDst), already laid out as big-endian words:
//   tail0   what follows a row in b_0's string: a ShaTail (sha512.hip.h), which sha512_fill reads behind the row with `before` = 128
//   tail1   whole padded blocks of b_1's string behind the 64 digest bytes, the bit length in place; b_2's differ in the counter byte alone
// The state behind the all-zero Z_pad block is a constant (SHA512_ZPAD_MID, constants.inc).  One lane runs its blocks of all three
// strings through ONE copy of the compression function (as sig_nonce_kernel does); only the number of blocks differs between lanes.
// The PREFIXED flavour hashes a 32-byte row (the VRF's pk32) in front of msg without a concatenated copy: the row is sha512_fill's
// register prefix, loaded in the step that uses it, and msg follows at string offset 32, so an aligned row keeps its vector loads.
//
// Field and map (ell2_kernel).  Every decision is a mask: no branch and no address depends on u or on a message byte (the message may
// be a password), so the same code serves both table-selection modes of the library.  Per map three GF(p) exponentiations --
// the inversion of 1 + Z u^2, the norm's root that decides "is g(x1) a square", the root of (g0 + |g|) / 2 -- and no fourth one for the
// second candidate: g(x2) = Z u^2 g(x1), so |g(x2)| = |Z| |u|^2 |g(x1)| follows from the root already taken (c_h2c_sqrt_m5).  The
// rational map stays projective; the two maps of the RO flavour meet in the complete addition of combine.hip.h, the sum goes through
// the x392 chain in R1 form, and one inversion per element lowers the result.
#pragma once
#include "combine.hip.h"    // XYZ, add_projective
#include "sig.hip.h"        // SigMsgs, lane_msg, SIG_BLOCK; sha512.hip.h

namespace fq {

constexpr int H2C_TAIL1_WORDS = 40;      // 3 blocks - 64 bytes: 0x01 || DST_prime (257 bytes at most) || padding || bit length
struct H2cDst {
    ShaTail tail0;                       // I2OSP(len_in_bytes, 2) || 0x00 || DST_prime
    u64 tail1[H2C_TAIL1_WORDS];
    u32 blocks1;                         // blocks of b_0 || 0x01 || DST_prime: 1..3
};
enum H2cOut { H2C_OUT_MAP = 0, H2C_OUT_AFFINE = 1, H2C_OUT_BYTES = 2 };     // map + rational map only | + x392, affine words | + x392, 32 bytes

// dst: 1..255 bytes (checked by the caller); count: field elements asked of expand_message_xmd / 2, i.e. 2 (RO) or 1 (NU)
inline H2cDst h2c_make_dst(const uint8_t* dst, size_t dst_len, int count) {
    H2cDst d;
    memset(&d, 0, sizeof d);
    const size_t len_in_bytes = 64 * (size_t)count;
    const uint8_t head0[3] = { (uint8_t)(len_in_bytes >> 8), (uint8_t)len_in_bytes, 0 }, head1[1] = { 0x01 };
    d.tail0 = sha_make_tail(head0, sizeof head0, dst, dst_len);
    const ShaTail t1 = sha_make_tail(head1, sizeof head1, dst, dst_len);
    static_assert(SHA_TAIL_WORDS <= H2C_TAIL1_WORDS, "tail1 starts as a ShaTail's words");
    for (int w = 0; w < SHA_TAIL_WORDS; w++) d.tail1[w] = t1.w[w];
    d.blocks1 = sha512_blocks(64 + t1.len);
    d.tail1[16 * d.blocks1 - 8 - 1] = 8 * (uint64_t)(64 + t1.len);      // the bit length ends the last block
    return d;
}

namespace {

// ---- hashing ----------------------------------------------------------------------------------------------------------------------
// OS2IP(32 bytes) mod p for the big-endian words (a, b, c, e), a first: 2^128 = 2 (mod 2^127 - 1), so the value is 2 (a : b) + (c : e)
FQ_DEV Fe<3> h2c_reduce256(u64 a, u64 b, u64 c, u64 e) { return fe_add(fe_dbl(fe_unpack(b, a)), fe_unpack(e, c)); }

// out_u: n x COUNT x 4 canonical words.  b_0 stays live across b_1 for COUNT = 2: eight more 64-bit values than the 40 of the signature
// layer's hashing kernels, which do not fit 128 VGPRs (4 spilled) -- that flavour is held to three waves per SIMD instead of four.
// PREFIXED: the string is pk32[i] || msg_i (pk32: n rows of 32 bytes, 16-byte aligned; not read otherwise)
template <int COUNT, bool PREFIXED>
__global__ __launch_bounds__(SIG_BLOCK, COUNT == 2 ? SIG_WAVES - 1 : SIG_WAVES) void h2f_kernel(const uint8_t* pk32, SigMsgs m, H2cDst d, u64* out_u, u32 n) {
    constexpr int PW = PREFIXED ? 4 : 0;
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const LaneMsg l = lane_msg(m, i);
    const int mode = sha_load_mode(m.rows, m.stride);
    const u32 blocks0 = sha512_blocks(8 * PW + l.len + d.tail0.len), blocks1 = d.blocks1, steps = blocks0 + COUNT * blocks1;
    u64 h[8], b0[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { h[k] = SHA512_ZPAD_MID[k]; b0[k] = 0; }
#pragma unroll 1
    for (u32 step = 0; step < steps; step++) {
        u64 w[16];
        const bool msg_phase = step < blocks0;
        const u32 s1 = step - blocks0;                                        // wraps in the message phase: not used then
        const u32 r = (COUNT == 2 && !msg_phase && s1 >= blocks1) ? 1u : 0u;    // which of b_1, b_2
        const u32 bb = s1 - r * blocks1;                                      // its block
        if (msg_phase) {
            u64 pre[4];
            if (PREFIXED && step == 0) dleq_row_words(pk32 + 32 * (size_t)i, pre);
            sha512_fill<PW>(w, pre, l.row, l.len, d.tail0, 128, step, blocks0, mode);      // behind Z_pad
        } else if (bb == 0) {
            // h is b_0 (r == 0) or b_1 (r == 1): the string starts with b_0, or with b_0 xor b_1
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (r == 0) b0[k] = h[k];
                w[k] = r ? b0[k] ^ h[k] : h[k];
                w[8 + k] = d.tail1[k];
            }
            w[8] ^= r ? (u64)0x03 << 56 : 0;                                  // the counter byte: 0x01 -> 0x02
            sha512_init(h);
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) w[j] = d.tail1[8 + 16 * (bb - 1) + j];
        }
        sha512_compress(h, w);
        if (!msg_phase && bb + 1 == blocks1) {                                // b_(r+1) is complete: u_r = (e_r0, e_r1)
            u64 o[4];
            fe_canon(h2c_reduce256(h[0], h[1], h[2], h[3]), o[0], o[1]);
            fe_canon(h2c_reduce256(h[4], h[5], h[6], h[7]), o[2], o[3]);
            store32(reinterpret_cast<uint8_t*>(out_u + 4 * ((size_t)i * COUNT + r)), o);
        }
    }
}

// ---- GF(p^2): squares, roots, sgn0 ------------------------------------------------------------------------------------------------
FQ_DEV Fe<1> fe2_norm(const Fe2<1>& a) { return fe_carry(fe_add(fe_sqr(a.re), fe_sqr(a.im))); }
FQ_DEV u32 fe2_is_zero_mask(const Fe2<1>& a) {
    const bool re0 = fe_is_zero(a.re), im0 = fe_is_zero(a.im);              // both evaluated: no branch
    return (re0 & im0) ? ~0u : 0u;
}
// a is a square of GF(p^2) iff its norm is a square of GF(p) or zero.  s = norm^((p + 1) / 4), so s^2 = +-norm: returns ~0 and the
// norm's root in s for a square, 0 and a root of MINUS the norm otherwise
FQ_DEV u32 fe2_is_square(const Fe2<1>& a, Fe<1>& s) {
    const Fe<1> nrm = fe2_norm(a);
    s = fe_mul(nrm, fe_invsqrt(nrm));
    return fe_equal(fe_sqr(s), nrm) ? ~0u : 0u;
}
// a square root of the square g, given s with s^2 = |g|^2: with t = (g0 + s) / 2 either t is a square -- then (sqrt t, g1 / (2 sqrt t)) --
// or -t is -- then (g1 / (2 sqrt -t), sqrt -t).  e = t^((p - 3) / 4) gives both the root t e and its inverse +-e.  t = 0 means g = g0 = -s,
// a non-square (or zero) of GF(p): t = g0 then takes the second route to (0, sqrt s).  WHICH root comes out is left to sgn0.
FQ_DEV Fe2<1> fe2_sqrt(const Fe2<1>& g, const Fe<1>& s) {
    Fe<1> t = fe_mul(fe_add(g.re, s), fe_half());
    t = fe_select(fe_is_zero(t) ? ~0u : 0u, g.re, t);
    const Fe<1> e = fe_invsqrt(t);
    const Fe<1> r = fe_mul(t, e);
    const u32 plus = fe_equal(fe_sqr(r), t) ? ~0u : 0u;
    const Fe<1> w = fe_mul(fe_mul(g.im, e), fe_half());
    Fe2<1> y;
    y.re = fe_select(plus, r, fe_carry(fe_neg(w)));
    y.im = fe_select(plus, w, r);
    return y;
}
// RFC 9380 section 4.1 for m = 2, on the canonical words
FQ_DEV u32 fe2_sgn0(const Fe2<1>& a) {
    u64 w[4];
    store_fe2_words(w, a);
    return ((u32)w[0] & 1u) | (((w[0] | w[1]) == 0 ? 1u : 0u) & ((u32)w[2] & 1u));
}

// ---- the map ------------------------------------------------------------------------------------------------------------------------
// Elligator 2 (RFC 9380 section 6.7.1) on K t^2 = s^3 + J s^2 + s and the rational map of appendix D.1, projective:
// (x_E, y_E) = (s / t, (s - 1) / (s + 1)) = (x (s + 1) : y (s - 1) : y (s + 1)) for (s, t) = (x K, y K); y (s + 1) = 0 gives (0, 1).
// 1 + Z u^2 is never zero (-1 / Z is a non-square), so inv0's zero and the x1 = -J/K rule behind it cannot be reached; g(x2) = Z u^2 g(x1)
// rests on that.
FQ_DEV XYZ ell2_map(const Fe2<1>& u) {
    const Fe2<1> zu2 = fe2_mul(fe2_sqr(u), c_h2c_z());
    const Fe2<1> x1 = fe2_mul(fe2_inv(fe2_carry(fe2_add(zu2, fe2_one()))), c_h2c_neg_jk());
    const Fe2<2> x1jk = fe2_add(x1, c_h2c_jk());
    const Fe2<1> gx1 = fe2_mul(x1, fe2_add(fe2_mul(x1, x1jk), c_h2c_ik2()));          // x (x (x + J/K) + 1/K^2)
    const Fe2<1> x2 = fe2_carry(fe2_neg(x1jk)), gx2 = fe2_mul(zu2, gx1);
    Fe<1> s1;
    const u32 sq = fe2_is_square(gx1, s1);
    // gx1 not a square: s1^2 = -|gx1|^2, and |gx2|^2 = 5 |u|^4 |gx1|^2 = (|u|^2 sqrt(-5) s1)^2
    const Fe<1> s2 = fe_mul(fe_mul(fe2_norm(u), c_h2c_sqrt_m5()), s1);
    const Fe2<1> x = fe2_select(sq, x1, x2);
    Fe2<1> y = fe2_sqrt(fe2_select(sq, gx1, gx2), fe_select(sq, s1, s2));
    y = fe2_carry(fe2_cneg(y, fe2_sgn0(y) != (sq & 1u) ? ~0u : 0u));                  // sgn0(y) = 1 with x1, 0 with x2
    const Fe2<1> sm = fe2_mul(x, c_h2c_k());
    const Fe2<2> sp1 = fe2_add(sm, fe2_one());
    XYZ r;
    r.X = fe2_mul(x, sp1);
    r.Y = fe2_mul(y, fe2_sub(sm, fe2_one()));
    r.Z = fe2_mul(y, sp1);
    const u32 z0 = fe2_is_zero_mask(r.Z);
    Fe2<1> zero;
#pragma unroll
    for (int k = 0; k < 5; k++) zero.re.l[k] = zero.im.l[k] = 0;
    r.X = fe2_select(z0, zero, r.X);
    r.Y = fe2_select(z0, fe2_one(), r.Y);
    r.Z = fe2_select(z0, fe2_one(), r.Z);
    return r;
}
// [392]P for a projective P: (X Z, Y Z, Z^2, X, Y) is P in R1 form (Ta Tb = X Y = T Z), then the chain of clear_cofactor_392
FQ_DEV R1 h2c_cofactor_392(const XYZ& p) {
    R1 p0;
    p0.X = fe2_mul(p.X, p.Z); p0.Y = fe2_mul(p.Y, p.Z); p0.Z = fe2_sqr(p.Z);
    p0.Ta = widen<4>(p.X); p0.Tb = widen<2>(p.Y);
    const R2s t0 = as_signed(r1_to_r2(p0));
    R1 q = add(dbl(p0), t0);                  // 3P
#pragma unroll 1
    for (int i = 0; i < 4; i++) q = dbl(q);   // 48P
    q = add(q, t0);                           // 49P
#pragma unroll 1
    for (int i = 0; i < 3; i++) q = dbl(q);   // 392P
    return q;
}

// u: n x COUNT x 4 words, each coordinate any value in [0, 2^128).  OUT (H2cOut): the mapped point itself as affine words (COUNT = 1), or
// [392](map(u_0) [+ map(u_1)]) as affine words or as its 32-byte encoding; one inversion per element either way
template <int COUNT, int OUT>
__global__ __launch_bounds__(BLOCK) void ell2_kernel(const u64* u, u64* out, u32 n) {
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 uw[4 * COUNT];
    load32(reinterpret_cast<const uint8_t*>(u + 4 * COUNT * (size_t)i), uw);
    if constexpr (COUNT == 2) load32(reinterpret_cast<const uint8_t*>(u + 4 * COUNT * (size_t)i + 4), uw + 4 * (COUNT - 1));
    XYZ q = ell2_map(load_fe2(uw));
    if constexpr (COUNT == 2) {
        __builtin_amdgcn_sched_barrier(0);      // one map after the other: interleaved, their temporaries would not fit the lane's registers
        const XYZ q1 = ell2_map(load_fe2(uw + 4));
        q = add_projective(q.X, q.Y, q.Z, q1.X, q1.Y, q1.Z);
    }
    Fe2<1> ax, ay;
    if constexpr (OUT == H2C_OUT_MAP) {
        const Fe2<1> zi = fe2_inv(q.Z);
        ax = fe2_mul(q.X, zi); ay = fe2_mul(q.Y, zi);
    } else {
        r1_to_affine(h2c_cofactor_392(q), ax, ay);
    }
    if constexpr (OUT == H2C_OUT_BYTES) {
        u64 w[4];
        point_encode(ax, ay, w);
        store32(reinterpret_cast<uint8_t*>(out + 4 * (size_t)i), w);
    } else {
        u64 o[8];
        store_fe2(o, ax); store_fe2(o + 4, ay);
        store32(reinterpret_cast<uint8_t*>(out + 8 * (size_t)i), o);
        store32(reinterpret_cast<uint8_t*>(out + 8 * (size_t)i + 4), o + 4);
    }
}

// ---- launchers: each returns the hipError_t of its launch ---------------------------------------------------------------------------
// pk32 != NULL: the 32-byte row hashed in front of every message (two elements only)
int h2c_launch_h2f(hipStream_t stream, int count, const uint8_t* pk32, SigMsgs m, const H2cDst& d, uint64_t* out_u, uint32_t n) {
    if (pk32) hipLaunchKernelGGL((h2f_kernel<2, true>), sig_grid(n), dim3(SIG_BLOCK), 0, stream, pk32, m, d, (u64*)out_u, n);
    else if (count == 2) hipLaunchKernelGGL((h2f_kernel<2, false>), sig_grid(n), dim3(SIG_BLOCK), 0, stream, pk32, m, d, (u64*)out_u, n);
    else hipLaunchKernelGGL((h2f_kernel<1, false>), sig_grid(n), dim3(SIG_BLOCK), 0, stream, pk32, m, d, (u64*)out_u, n);
    return (int)hipGetLastError();
}
int h2c_launch_ell2(hipStream_t stream, int count, int out_kind, const uint64_t* u, uint64_t* out, uint32_t n) {
    const dim3 grid((n + BLOCK - 1) / BLOCK), block(BLOCK);
    if (out_kind == H2C_OUT_MAP) hipLaunchKernelGGL((ell2_kernel<1, H2C_OUT_MAP>), grid, block, 0, stream, (const u64*)u, (u64*)out, n);
    else if (count == 2 && out_kind == H2C_OUT_AFFINE) hipLaunchKernelGGL((ell2_kernel<2, H2C_OUT_AFFINE>), grid, block, 0, stream, (const u64*)u, (u64*)out, n);
    else if (count == 2) hipLaunchKernelGGL((ell2_kernel<2, H2C_OUT_BYTES>), grid, block, 0, stream, (const u64*)u, (u64*)out, n);
    else if (out_kind == H2C_OUT_AFFINE) hipLaunchKernelGGL((ell2_kernel<1, H2C_OUT_AFFINE>), grid, block, 0, stream, (const u64*)u, (u64*)out, n);
    else hipLaunchKernelGGL((ell2_kernel<1, H2C_OUT_BYTES>), grid, block, 0, stream, (const u64*)u, (u64*)out, n);
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace fq

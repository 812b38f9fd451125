// The verifiable random function's own kernels (include/fourq_amd.h, "verifiable random function"): hash_to_field of pk32 || alpha, the
// prover's scalars and its final row, the verifier's cleared Gamma with the operand rows of the two inner calls, its check with the output
// hash, and proof_to_hash -- and their launchers; included by fourq_amd.hip, whose C ABI strings them together with the map, MUL_endo on
// encodings, the comb, [k]B + [l]P (or its keyed sibling) and the grouped sum over groups of two.
//
// Hashing.  hash_to_field's string is Z_pad || pk32 || alpha || tail0 (h2c.hip.h): the 32 bytes of pk32 go from their row straight into
// the first four words of the first block, and alpha follows at string offset 32 -- a multiple of 16, so an aligned row keeps its vector
// loads (as E || msg in oprf_final_kernel); nothing is concatenated in memory.  The challenge has dleq.hip.h's fixed layout, five rows of
// 32 bytes and a tail by value, under the label "VrfVerify"; the output hash is one row and the tail "VrfOutput".  The prover's two
// hashes, H(sk32) and H(k[32:64] || h32), are one block each.
//
// Secrets.  k = H(sk32), x = LE(k[0:32]) and r pass through vrf_scalar_kernel and vrf_prove_kernel: one reduction and the mul-sub of
// scalar_n.hip.h, straight-line code on whole words.  h32, Gamma, c, s and every status are public.
#pragma once
#include "dleq.hip.h"       // dleq_challenge, dleq_row_words, dleq_make_tail; oprf.hip.h: OprfTail; h2c.hip.h: H2cDst, h2c_word; sig.hip.h

namespace fq {

namespace {

// ---- hash_to_field of pk32 || alpha: h2f_kernel<2> with a 32-byte row in front of the message ----------------------------------------------
// block b of the padded string pk_row[0..32) ++ row[0..len) ++ tail0 that FOLLOWS the Z_pad block (sha512_fill_tail with oprf_fill's prefix)
FQ_DEV void vrf_fill_prefixed(u64 w[16], const uint8_t* pk_row, const uint8_t* row, u32 len, const H2cDst& d, u32 b, u32 blocks, int mode) {
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
        const u32 m = 128 * b + 8 * j - 32;         // offset into row ++ tail0 (wraps for a prefix word: not used then)
        if (j < 4 && b == 0) {
            w[j] = w[j + 1] = 0;                    // the prefix: filled below
        } else if (mode == SHA_LOAD_16 && m + 16 <= len) {
            const uint4 q = *reinterpret_cast<const uint4*>(row + m);
            w[j] = __builtin_bswap64(((u64)q.y << 32) | q.x);
            w[j + 1] = __builtin_bswap64(((u64)q.w << 32) | q.z);
        } else {
            w[j] = h2c_word(row, len, d, m, mode);
            w[j + 1] = h2c_word(row, len, d, m + 8, mode);
        }
    }
    if (b == 0) dleq_row_words(pk_row, w);
    if (b + 1 == blocks) w[15] = (u64)(128 + 32 + len + d.tail0_len) * 8;      // the bit length, Z_pad and pk32 included
}
// out_u: n x 2 x 4 canonical words.  As h2f_kernel<2>: b_0 stays live across b_1, three waves per SIMD
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES - 1) void vrf_h2f_kernel(const uint8_t* pk32, SigMsgs m, H2cDst d, u64* out_u, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const LaneMsg l = lane_msg(m, i);
    const int mode = sha_load_mode(m.rows, m.stride);
    const u32 blocks0 = sha512_blocks(32 + l.len + d.tail0_len), blocks1 = d.blocks1, steps = blocks0 + 2 * blocks1;
    u64 h[8], b0[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { h[k] = SHA512_ZPAD_MID[k]; b0[k] = 0; }
#pragma unroll 1
    for (u32 step = 0; step < steps; step++) {
        u64 w[16];
        const bool msg_phase = step < blocks0;
        const u32 s1 = step - blocks0;                                        // wraps in the message phase: not used then
        const u32 r = (!msg_phase && s1 >= blocks1) ? 1u : 0u;                // which of b_1, b_2
        const u32 bb = s1 - r * blocks1;                                      // its block
        if (msg_phase) {
            vrf_fill_prefixed(w, pk32 + 32 * (size_t)i, l.row, l.len, d, step, blocks0, mode);
        } else if (bb == 0) {
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
            store32(reinterpret_cast<uint8_t*>(out_u + 4 * ((size_t)i * 2 + r)), o);
        }
    }
}

// ---- prove: k = H(sk32); x = LE(k[0:32]) (unreduced, as the signatures' a); r = LE(H(k[32:64] || h32)) mod N ---------------------------------
// Two strings of one block each through ONE copy of the compression function (as sig_nonce_kernel)
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void vrf_scalar_kernel(const uint8_t* sk32, const uint8_t* h32, u64* x_out, u64* r_out, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 h[8];
    sha512_init(h);
#pragma unroll 1
    for (u32 step = 0; step < 2; step++) {
        u64 w[16];
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = 0;
        if (step == 0) {
            dleq_row_words(sk32 + 32 * (size_t)i, w);
            w[4] = (u64)0x80 << 56;
            w[15] = 32 * 8;
        } else {                                           // k is complete: x leaves, k[32:64] starts the next string
            u64 x[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { x[k] = __builtin_bswap64(h[k]); w[k] = h[4 + k]; }
            store32(reinterpret_cast<uint8_t*>(x_out + 4 * (size_t)i), x);
            dleq_row_words(h32 + 32 * (size_t)i, w + 4);
            w[8] = (u64)0x80 << 56;
            w[15] = 64 * 8;
            sha512_init(h);
        }
        sha512_compress(h, w);
    }
    u64 d[8], r[4];
    sha512_digest_le(h, d);
    sc_reduce512(d, r);
    store32(reinterpret_cast<uint8_t*>(r_out + 4 * (size_t)i), r);
}

// ---- prove: c = LE(H(pk32 || h32 || gamma32 || u32 || v32 || tail)) mod N, s = (r - c x) mod N, proof96 = gamma32 || c || s --------------------
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void vrf_prove_kernel(const uint8_t* pk32, const uint8_t* h32, const uint8_t* g32, const uint8_t* t_u, const uint8_t* t_v,
                                                                        OprfTail tail, const u64* x_rows, const u64* r_rows, uint8_t* proof96, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t at = 32 * (size_t)i;
    u64 c[4], x[4], r[4], s[4], g[4];
    dleq_challenge(pk32 + at, h32 + at, g32 + at, t_u + at, t_v + at, tail, c);
    load32(reinterpret_cast<const uint8_t*>(x_rows + 4 * (size_t)i), x);
    load32(reinterpret_cast<const uint8_t*>(r_rows + 4 * (size_t)i), r);
    sc_mulsub(r, x, c, s);
    load32(g32 + at, g);
    store32(proof96 + 96 * (size_t)i, g);
    store32(proof96 + 96 * (size_t)i + 32, c);
    store32(proof96 + 96 * (size_t)i + 64, s);
}

// ---- verify: W = [392]decode(gamma32) ------------------------------------------------------------------------------------------------------
// w: encode(W), all zero where gamma32 does not decode; returns FOURQ_BYTES_DECODE_BASE + the decode code, or 0.  neutral: W = (0, 1), the only
// point whose y is 1, i.e. the encoding 01 00 .. 00.  Gamma comes from the prover: it meets the doublings and the complete addition of the
// x392 chain only, never a ladder (MUL_endo is not [k]P outside the subgroup of order N).
FQ_DEV uint8_t vrf_clear_gamma(const u64 g[4], u64 w[4], bool& neutral) {
    Fe2<1> x, y, ax, ay;
    const int st = point_decode(g, x, y);
    r1_to_affine(clear_cofactor_392(x, y), ax, ay);
    point_encode(ax, ay, w);
    neutral = w[0] == 1 && (w[1] | w[2] | w[3]) == 0;
    if (st) w[0] = w[1] = w[2] = w[3] = 0;
    return st ? (uint8_t)(FOURQ_BYTES_DECODE_BASE + st) : (uint8_t)0;
}
// beta = H(w32 || tail): one row, then the tail; zero unless keep
FQ_DEV void vrf_beta(const u64 w32[4], const OprfTail& tail, bool keep, uint8_t* out64) {
    const u32 total = 32 + tail.tail_len, blocks = sha512_blocks(total);      // 1..3, the same for every lane
    u64 h[8], x[8];
    sha512_init(h);
#pragma unroll 1
    for (u32 b = 0; b < blocks; b++) {
        u64 w[16];
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = oprf_tail_word(tail, 128 * b + 8 * k - 32);      // wraps in front of the tail: overwritten below
        if (b == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = __builtin_bswap64(w32[k]);
        }
        if (b + 1 == blocks) w[15] = (u64)total * 8;
        sha512_compress(h, w);
    }
    sha512_digest_le(h, x);
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = keep ? x[k] : 0;
    store32(out64, x);
    store32(out64 + 32, x + 4);
}
// proof96 = gamma32 || c || s into the operand rows of the two inner calls; one lane per row.  s_rows / c_rows: the scalars of [s]G + [c]Y;
// pair_sc / pair_pt: (s, h32), (c / 392 mod N, w32) interleaved, the groups of two of [s]Hpt + [c / 392]W; st_gamma[i]: the decode code of
// gamma32; pre[i]: FOURQ_SIG_S_RANGE unless LE(c) < N and LE(s) < N, else FOURQ_VRF_GAMMA_NEUTRAL when W is the neutral point
__global__ __launch_bounds__(BLOCK) void vrf_gamma_kernel(const uint8_t* proof96, const uint8_t* h32, u64* w32, u64* s_rows, u64* c_rows, u64* pair_sc, u64* pair_pt,
                                                          uint8_t* st_gamma, uint8_t* pre, u32 n) {
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* row = proof96 + 96 * (size_t)i;
    u64 g[4], w[4], c[4], s[4], ci[4], inv[4], hp[4];
    bool neutral;
    load32(row, g);
    st_gamma[i] = vrf_clear_gamma(g, w, neutral);
    load32(row + 32, c);
    load32(row + 64, s);
    load32(h32 + 32 * (size_t)i, hp);
#pragma unroll
    for (int k = 0; k < 4; k++) inv[k] = SC_INV392[k];
    sc_mul(c, inv, ci);
    store32(reinterpret_cast<uint8_t*>(w32 + 4 * (size_t)i), w);
    store32(reinterpret_cast<uint8_t*>(s_rows + 4 * (size_t)i), s);
    store32(reinterpret_cast<uint8_t*>(c_rows + 4 * (size_t)i), c);
    store32(reinterpret_cast<uint8_t*>(pair_sc + 8 * (size_t)i), s);
    store32(reinterpret_cast<uint8_t*>(pair_sc + 8 * (size_t)i + 4), ci);
    store32(reinterpret_cast<uint8_t*>(pair_pt + 8 * (size_t)i), hp);
    store32(reinterpret_cast<uint8_t*>(pair_pt + 8 * (size_t)i + 4), w);
    pre[i] = !(sc_lt_n(c) && sc_lt_n(s)) ? (uint8_t)FOURQ_SIG_S_RANGE : neutral ? (uint8_t)FOURQ_VRF_GAMMA_NEUTRAL : (uint8_t)0;
}
// proof_to_hash: the front of vrf_gamma_kernel and the output hash; c and s are not looked at
__global__ __launch_bounds__(BLOCK) void vrf_proof_to_hash_kernel(const uint8_t* proof96, OprfTail tail, uint8_t* beta64, uint8_t* status, u32 n) {
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 g[4], w[4];
    bool neutral;
    load32(proof96 + 96 * (size_t)i, g);
    uint8_t st = vrf_clear_gamma(g, w, neutral);
    if (st == 0 && neutral) st = (uint8_t)FOURQ_VRF_GAMMA_NEUTRAL;
    vrf_beta(w, tail, st == 0, beta64 + 64 * (size_t)i);
    status[i] = st;
}

// ---- verify: the challenge hash, the compare, the status merge, the output hash; one lane per row ---------------------------------------------
// status[i], the first that is set: the key's (key_ids != NULL: FOURQ_KEYSET_ID_RANGE, else the slot's own status), st_u[i] (pk32 does not
// decode), st_gamma[i], FOURQ_SIG_MSG_CLAMPED, pre[i] (the range of c and s, then the neutral W), st_v[i] (an Hpt that is the neutral point
// does not decode); ok[i] = (c' == c) where it is 0; beta64[i] is all zero unless ok[i]
struct VrfKeys { const u32* ids; const uint8_t* status; u32 count; };
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void vrf_check_kernel(const uint8_t* pk32, const uint8_t* h32, const uint8_t* proof96, const uint8_t* w32, const uint8_t* t_u,
                                                                        const uint8_t* t_v, OprfTail challenge, OprfTail output, const u64* c_rows, VrfKeys keys, SigMsgs m,
                                                                        const uint8_t* st_u, const uint8_t* st_gamma, const uint8_t* pre, const uint8_t* st_v, uint8_t* beta64,
                                                                        uint8_t* ok, uint8_t* status, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t at = 32 * (size_t)i;
    u64 c[4], want[4], w[4];
    dleq_challenge(pk32 + at, h32 + at, proof96 + 96 * (size_t)i, t_u + at, t_v + at, challenge, c);
    load32(reinterpret_cast<const uint8_t*>(c_rows + 4 * (size_t)i), want);
    uint8_t st = 0;
    if (keys.ids) {
        const u32 id = keys.ids[i];
        st = id < keys.count ? keys.status[id] : (uint8_t)FOURQ_KEYSET_ID_RANGE;
    }
    if (st == 0) st = st_u[i];
    if (st == 0) st = st_gamma[i];
    if (st == 0 && lane_msg(m, i).clamped) st = (uint8_t)FOURQ_SIG_MSG_CLAMPED;
    if (st == 0) st = pre[i];
    if (st == 0) st = st_v[i];
    const bool same = ((c[0] ^ want[0]) | (c[1] ^ want[1]) | (c[2] ^ want[2]) | (c[3] ^ want[3])) == 0;
    const bool good = st == 0 && same;
    load32(w32 + at, w);
    vrf_beta(w, output, good, beta64 + 64 * (size_t)i);
    ok[i] = good ? (uint8_t)1 : (uint8_t)0;
    status[i] = st;
}

// ---- launchers: each returns the hipError_t of its launch ---------------------------------------------------------------------------
int vrf_launch_h2f(hipStream_t stream, const uint8_t* pk32, SigMsgs m, const H2cDst& d, uint64_t* out_u, uint32_t n) {
    hipLaunchKernelGGL(vrf_h2f_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, pk32, m, d, (u64*)out_u, n);
    return (int)hipGetLastError();
}
int vrf_launch_scalars(hipStream_t stream, const uint8_t* sk32, const uint8_t* h32, uint64_t* x_out, uint64_t* r_out, uint32_t n) {
    hipLaunchKernelGGL(vrf_scalar_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, sk32, h32, (u64*)x_out, (u64*)r_out, n);
    return (int)hipGetLastError();
}
int vrf_launch_prove(hipStream_t stream, const uint8_t* pk32, const uint8_t* h32, const uint8_t* g32, const uint8_t* t_u, const uint8_t* t_v, const OprfTail& tail,
                     const uint64_t* x_rows, const uint64_t* r_rows, uint8_t* proof96, uint32_t n) {
    hipLaunchKernelGGL(vrf_prove_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, pk32, h32, g32, t_u, t_v, tail, (const u64*)x_rows, (const u64*)r_rows, proof96, n);
    return (int)hipGetLastError();
}
int vrf_launch_gamma(hipStream_t stream, const uint8_t* proof96, const uint8_t* h32, uint64_t* w32, uint64_t* s_rows, uint64_t* c_rows, uint64_t* pair_sc, uint64_t* pair_pt,
                     uint8_t* st_gamma, uint8_t* pre, uint32_t n) {
    hipLaunchKernelGGL(vrf_gamma_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, proof96, h32, (u64*)w32, (u64*)s_rows, (u64*)c_rows, (u64*)pair_sc, (u64*)pair_pt,
                       st_gamma, pre, n);
    return (int)hipGetLastError();
}
int vrf_launch_proof_to_hash(hipStream_t stream, const uint8_t* proof96, const OprfTail& tail, uint8_t* beta64, uint8_t* status, uint32_t n) {
    hipLaunchKernelGGL(vrf_proof_to_hash_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, proof96, tail, beta64, status, n);
    return (int)hipGetLastError();
}
int vrf_launch_check(hipStream_t stream, const uint8_t* pk32, const uint8_t* h32, const uint8_t* proof96, const uint8_t* w32, const uint8_t* t_u, const uint8_t* t_v,
                     const OprfTail& challenge, const OprfTail& output, const uint64_t* c_rows, const VrfKeys& keys, SigMsgs m, const uint8_t* st_u, const uint8_t* st_gamma,
                     const uint8_t* pre, const uint8_t* st_v, uint8_t* beta64, uint8_t* ok, uint8_t* status, uint32_t n) {
    hipLaunchKernelGGL(vrf_check_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, pk32, h32, proof96, w32, t_u, t_v, challenge, output, (const u64*)c_rows, keys, m, st_u, st_gamma,
                       pre, st_v, beta64, ok, status, n);
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace fq

// The verifiable random function's own kernels (include/fourq_amd.h, "verifiable random function"): hash_to_field of pk32 || alpha, the
// prover's scalars and its final row, the verifier's cleared Gamma with the operand rows of the two inner calls, its check with the output
// hash, and proof_to_hash -- and their launchers; included by fourq_amd.hip, whose C ABI strings them together with the map, MUL_endo on
// encodings, the comb, [k]B + [l]P (or its keyed sibling) and the grouped sum over groups of two.
//
// Hashing.  hash_to_field's string is Z_pad || pk32 || alpha || tail0: h2f_kernel's PREFIXED flavour (h2c.hip.h), nothing is concatenated
// in memory.  The challenge has dleq.hip.h's fixed layout, five rows of 32 bytes and a tail by value, under the label "VrfVerify".  The
// output hash is W's 32 bytes, which proof_to_hash holds in registers, and the tail "VrfOutput": sha512_hash with a register prefix and an
// empty row.  The prover's two hashes, H(sk32) and H(k[32:64] || h32), are one block each.
//
// Secrets.  k = H(sk32), x = LE(k[0:32]) and r pass through vrf_scalar_kernel and vrf_prove_kernel: one reduction and the mul-sub of
// scalar_n.hip.h, straight-line code on whole words.  h32, Gamma, c, s and every status are public.
#pragma once
#include "dleq.hip.h"       // dleq_challenge, verifier_operand_rows, DLEQ_LABEL; h2c.hip.h: h2f_kernel; sig.hip.h: KeyRows, dleq_row_words; sha512.hip.h

namespace fq {

namespace {

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
                                                                        ShaTail tail, const u64* x_rows, const u64* r_rows, uint8_t* proof96, u32 n) {
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
// beta = H(w32 || tail); zero unless keep
FQ_DEV void vrf_beta(const u64 w32[4], const ShaTail& tail, bool keep, uint8_t* out64) {
    u64 pre[4], h[8], x[8];
#pragma unroll
    for (int k = 0; k < 4; k++) pre[k] = __builtin_bswap64(w32[k]);
    sha512_hash<4>(h, pre, nullptr, 0, tail, SHA_LOAD_BYTES);
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
    verifier_operand_rows(i, s, c, ci, hp, w, s_rows, c_rows, pair_sc, pair_pt);
    pre[i] = !(sc_lt_n(c) && sc_lt_n(s)) ? (uint8_t)FOURQ_SIG_S_RANGE : neutral ? (uint8_t)FOURQ_VRF_GAMMA_NEUTRAL : (uint8_t)0;
}
// proof_to_hash: the front of vrf_gamma_kernel and the output hash; c and s are not looked at
__global__ __launch_bounds__(BLOCK) void vrf_proof_to_hash_kernel(const uint8_t* proof96, ShaTail tail, uint8_t* beta64, uint8_t* status, u32 n) {
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
// status[i], the first that is set: the key's (key_row: FOURQ_KEYSET_ID_RANGE, else the slot's own status), st_u[i] (pk32 does not
// decode), st_gamma[i], FOURQ_SIG_MSG_CLAMPED, pre[i] (the range of c and s, then the neutral W), st_v[i] (an Hpt that is the neutral point
// does not decode); ok[i] = (c' == c) where it is 0; beta64[i] is all zero unless ok[i]
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void vrf_check_kernel(const uint8_t* pk32, const uint8_t* h32, const uint8_t* proof96, const uint8_t* w32, const uint8_t* t_u,
                                                                        const uint8_t* t_v, ShaTail challenge, ShaTail output, const u64* c_rows, KeyRows keys, SigMsgs m,
                                                                        const uint8_t* st_u, const uint8_t* st_gamma, const uint8_t* pre, const uint8_t* st_v, uint8_t* beta64,
                                                                        uint8_t* ok, uint8_t* status, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const size_t at = 32 * (size_t)i;
    u64 c[4], want[4], w[4];
    dleq_challenge(pk32 + at, h32 + at, proof96 + 96 * (size_t)i, t_u + at, t_v + at, challenge, c);
    load32(reinterpret_cast<const uint8_t*>(c_rows + 4 * (size_t)i), want);
    u32 slot;
    uint8_t st = key_row(keys, i, slot);
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
int vrf_launch_scalars(hipStream_t stream, const uint8_t* sk32, const uint8_t* h32, uint64_t* x_out, uint64_t* r_out, uint32_t n) {
    hipLaunchKernelGGL(vrf_scalar_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, sk32, h32, (u64*)x_out, (u64*)r_out, n);
    return (int)hipGetLastError();
}
int vrf_launch_prove(hipStream_t stream, const uint8_t* pk32, const uint8_t* h32, const uint8_t* g32, const uint8_t* t_u, const uint8_t* t_v, const ShaTail& tail,
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
int vrf_launch_proof_to_hash(hipStream_t stream, const uint8_t* proof96, const ShaTail& tail, uint8_t* beta64, uint8_t* status, uint32_t n) {
    hipLaunchKernelGGL(vrf_proof_to_hash_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, proof96, tail, beta64, status, n);
    return (int)hipGetLastError();
}
int vrf_launch_check(hipStream_t stream, const uint8_t* pk32, const uint8_t* h32, const uint8_t* proof96, const uint8_t* w32, const uint8_t* t_u, const uint8_t* t_v,
                     const ShaTail& challenge, const ShaTail& output, const uint64_t* c_rows, const KeyRows& keys, SigMsgs m, const uint8_t* st_u, const uint8_t* st_gamma,
                     const uint8_t* pre, const uint8_t* st_v, uint8_t* beta64, uint8_t* ok, uint8_t* status, uint32_t n) {
    hipLaunchKernelGGL(vrf_check_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, pk32, h32, proof96, w32, t_u, t_v, challenge, output, (const u64*)c_rows, keys, m, st_u, st_gamma,
                       pre, st_v, beta64, ok, status, n);
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace fq

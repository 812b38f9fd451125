// The batched DLEQ proofs' own kernels (include/fourq_amd.h, "oblivious PRF: proofs"): the composite scalar of every row, the prover's
// nonce rows, challenge and response, the verifier's split / gather and its final check -- and their launchers; included by fourq_amd.hip,
// whose C ABI strings them together with the grouped sum, [k]B + [l]P, DH_endo, MUL_endo on encodings and the comb.
//
// Hashing.  Both hashed strings have a FIXED layout: 32-byte rows -- pk32 || C || D and I2OSP(j, 4), or pk32 || M32 || Z32 || t2 || t3 --
// then a tail that is the same for every lane, label || DST || I2OSP(len(DST), 1), a ShaTail by value in the kernel arguments.  That is
// sha512_hash_rows (sha512.hip.h): every lane of a launch hashes the same number of blocks, and nothing but the state lives across a
// compression.
//
// Secrets.  The key k, K = 392 k mod N and the nonce r pass through dleq_nonce_kernel and dleq_prove_kernel: reductions, one product, the
// mul-sub and the zero tests are scalar_n.hip.h's straight-line code, and the status and the zeroing of a refused row are masks.  d, M, Z
// and c are public.
#pragma once
#include "oprf.hip.h"       // ScalarArg; sig.hip.h: load32 / store32, SIG_BLOCK; sha512.hip.h: ShaTail, sha512_hash_rows; scalar_n.hip.h

namespace fq {

constexpr int DLEQ_LABEL = 9;            // "Composite" and "Challenge"; the VRF's "VrfVerify" and "VrfOutput"
static_assert(DLEQ_LABEL <= SHA_TAIL_MAX_HEAD, "the labels are ShaTail heads");

namespace {

// the digest as a scalar: LE(h) mod N
FQ_DEV void dleq_digest_scalar(const u64 h[8], u64 out[4]) {
    u64 x[8];
    sha512_digest_le(h, x);
    sc_reduce512(x, out);
}

// ---- d_i = LE(H(pk32 || C_i || D_i || I2OSP(j, 4) || tail)) mod N, one lane per row, j = i mod group_size --------------------------------
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void dleq_composite_kernel(const uint8_t* pk32, const uint8_t* c32, const uint8_t* d32, ShaTail tail, u64* d_out,
                                                                             u32 group_size, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t* const rows[3] = { pk32, c32 + 32 * (size_t)i, d32 + 32 * (size_t)i };
    u64 h[8], d[4];
    sha512_hash_rows<3, true>(h, rows, i % group_size, tail);
    dleq_digest_scalar(h, d);
    store32(reinterpret_cast<uint8_t*>(d_out + 4 * (size_t)i), d);
}

// c = LE(H(pk32 || M32 || Z32 || t2 || t3 || tail)) mod N
FQ_DEV void dleq_challenge(const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3, const ShaTail& tail, u64 c[4]) {
    const uint8_t* const rows[5] = { pk32, m32, z32, t2, t3 };
    u64 h[8];
    sha512_hash_rows<5, false>(h, rows, 0, tail);
    dleq_digest_scalar(h, c);
}

// ---- prove: the scalars the comb and the ladder take: rows[g] = nonces[g] mod N for g < groups, rows[groups] = K = 392 (k mod N) mod N ----
__global__ __launch_bounds__(BLOCK) void dleq_nonce_kernel(ScalarArg key, const u64* nonces, u64* rows, u32 groups) {
    const u32 g = blockIdx.x * BLOCK + threadIdx.x;
    if (g > groups) return;
    u64 v[4];
    if (g < groups) {
        load32(reinterpret_cast<const uint8_t*>(nonces + 4 * (size_t)g), v);
        sc_reduce256(v, v);
    } else {
        const u64 cofactor[4] = { 392, 0, 0, 0 };
        sc_mul(key.w, cofactor, v);
    }
    store32(reinterpret_cast<uint8_t*>(rows + 4 * (size_t)g), v);
}

// ---- prove: challenge, response, status; one lane per group.  r: the reduced nonces (dleq_nonce_kernel's rows) -----------------------------
// status[g]: st_m (the decode codes of the group's C rows), else FOURQ_DH_NEUTRAL when k = 0 (mod N), else what DH_endo and MUL_endo said of
// M (a neutral composite does not decode), else FOURQ_DLEQ_NONCE_ZERO when r = 0 (mod N); the row is all zero unless 0
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void dleq_prove_kernel(const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3,
                                                                         ShaTail tail, ScalarArg key, const u64* r_rows, const uint8_t* st_m, const uint8_t* st_z,
                                                                         const uint8_t* st_t3, uint8_t* proof64, uint8_t* status, u32 groups) {
    const u32 g = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (g >= groups) return;
    const size_t at = 32 * (size_t)g;
    u64 c[4], k[4], K[4], r[4], s[4];
    dleq_challenge(pk32, m32 + at, z32 + at, t2 + at, t3 + at, tail, c);
    const u64 cofactor[4] = { 392, 0, 0, 0 };
    sc_reduce256(key.w, k);
    sc_mul(k, cofactor, K);
    load32(reinterpret_cast<const uint8_t*>(r_rows + 4 * (size_t)g), r);
    sc_mulsub(r, c, K, s);
    // the first stage that objects names the status: each later code counts only where everything in front of it is 0
    const u32 k_zero = (u32)sc_is_zero_mask(k) & FOURQ_DH_NEUTRAL, r_zero = (u32)sc_is_zero_mask(r) & FOURQ_DLEQ_NONCE_ZERO;
    u32 st = st_m[g];
    st |= k_zero & (0u - (u32)(st == 0));
    st |= (u32)st_z[g] & (0u - (u32)(st == 0));
    st |= (u32)st_t3[g] & (0u - (u32)(st == 0));
    st |= r_zero & (0u - (u32)(st == 0));
    const u64 keep = 0 - (u64)(st == 0);
#pragma unroll
    for (int i = 0; i < 4; i++) { c[i] &= keep; s[i] &= keep; }
    store32(proof64 + 64 * (size_t)g, c);
    store32(proof64 + 64 * (size_t)g + 32, s);
    status[g] = (uint8_t)st;
}

// the operand rows of a verifier's two inner calls, row g: s_rows / c_rows, the scalars of [s]G + [c]Y; pair_sc / pair_pt, (s, p0), (c2, p1)
// interleaved, the group of two of [s]P0 + [c2]P1 (p0, p1: the points' 32-byte encodings as words)
FQ_DEV void verifier_operand_rows(u32 g, const u64 s[4], const u64 c[4], const u64 c2[4], const u64 p0[4], const u64 p1[4], u64* s_rows, u64* c_rows, u64* pair_sc,
                                  u64* pair_pt) {
    store32(reinterpret_cast<uint8_t*>(s_rows + 4 * (size_t)g), s);
    store32(reinterpret_cast<uint8_t*>(c_rows + 4 * (size_t)g), c);
    store32(reinterpret_cast<uint8_t*>(pair_sc + 8 * (size_t)g), s);
    store32(reinterpret_cast<uint8_t*>(pair_sc + 8 * (size_t)g + 4), c2);
    store32(reinterpret_cast<uint8_t*>(pair_pt + 8 * (size_t)g), p0);
    store32(reinterpret_cast<uint8_t*>(pair_pt + 8 * (size_t)g + 4), p1);
}

// ---- verify: proof64 = c || s into the operand rows of the two inner calls; one lane per group -------------------------------------------------
// s_rows / c_rows: the scalars of [s]G + [c]pk; pair_sc / pair_pt: (s, M32), (c, Z32) interleaved, the groups of two of [s]M + [c]Z;
// pre[g]: FOURQ_SIG_S_RANGE unless LE(c) < N and LE(s) < N.  The public key's rows are filled before the composites (oprf_fill_key_kernel).
__global__ __launch_bounds__(SIG_BLOCK) void dleq_split_kernel(const uint8_t* proof64, const uint8_t* m32, const uint8_t* z32, u64* s_rows, u64* c_rows, u64* pair_sc, u64* pair_pt,
                                                               uint8_t* pre, u32 groups) {
    const u32 g = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (g >= groups) return;
    u64 c[4], s[4], m[4], z[4];
    load32(proof64 + 64 * (size_t)g, c);
    load32(proof64 + 64 * (size_t)g + 32, s);
    load32(m32 + 32 * (size_t)g, m);
    load32(z32 + 32 * (size_t)g, z);
    verifier_operand_rows(g, s, c, c, m, z, s_rows, c_rows, pair_sc, pair_pt);
    pre[g] = sc_lt_n(c) && sc_lt_n(s) ? (uint8_t)0 : (uint8_t)FOURQ_SIG_S_RANGE;
}

// ---- verify: hash, compare, status; one lane per group -----------------------------------------------------------------------------------------
// status[g]: the largest of the three decode codes (the group's C rows, its D rows, pk32), else pre[g], else what the sum of two said of M and
// Z (a neutral composite does not decode), else 0 with ok[g] = (c' == c)
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void dleq_check_kernel(const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3,
                                                                         ShaTail tail, const u64* c_rows, const uint8_t* st_m, const uint8_t* st_z, const uint8_t* st_t2,
                                                                         const uint8_t* pre, const uint8_t* st_t3, uint8_t* ok, uint8_t* status, u32 groups) {
    const u32 g = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (g >= groups) return;
    const size_t at = 32 * (size_t)g;
    u64 c[4], want[4];
    dleq_challenge(pk32, m32 + at, z32 + at, t2 + at, t3 + at, tail, c);
    load32(reinterpret_cast<const uint8_t*>(c_rows + 4 * (size_t)g), want);
    const uint8_t a = st_m[g], b = st_z[g], p = st_t2[g];
    uint8_t st = a > b ? a : b;
    st = st > p ? st : p;
    if (st == 0) st = pre[g];
    if (st == 0) st = st_t3[g];
    const bool same = ((c[0] ^ want[0]) | (c[1] ^ want[1]) | (c[2] ^ want[2]) | (c[3] ^ want[3])) == 0;
    ok[g] = st == 0 && same ? (uint8_t)1 : (uint8_t)0;
    status[g] = st;
}

// ---- composites as a call of its own: one status per group from the two sums', both rows zero unless it is 0 ------------------------------------
__global__ __launch_bounds__(SIG_BLOCK) void dleq_composites_merge_kernel(const uint8_t* st_m, const uint8_t* st_z, u64* m32, u64* z32, uint8_t* status, u32 groups) {
    const u32 g = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (g >= groups) return;
    const uint8_t a = st_m[g], b = st_z[g], st = a > b ? a : b;
    status[g] = st;
    if (st == 0) return;
    const u64 zero[4] = { 0, 0, 0, 0 };
    store32(reinterpret_cast<uint8_t*>(m32 + 4 * (size_t)g), zero);
    store32(reinterpret_cast<uint8_t*>(z32 + 4 * (size_t)g), zero);
}

// ---- launchers: each returns the hipError_t of its launch ---------------------------------------------------------------------------
inline ScalarArg dleq_scalar_arg(const void* words32) {
    ScalarArg a;
    memcpy(a.w, words32, 32);
    return a;
}
int dleq_launch_composite(hipStream_t stream, const uint8_t* pk32, const uint8_t* c32, const uint8_t* d32, const ShaTail& tail, uint64_t* d_out, uint32_t group_size, uint32_t n) {
    hipLaunchKernelGGL(dleq_composite_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, pk32, c32, d32, tail, (u64*)d_out, group_size, n);
    return (int)hipGetLastError();
}
int dleq_launch_nonces(hipStream_t stream, const uint64_t key[4], const uint64_t* nonces, uint64_t* rows, uint32_t groups) {
    hipLaunchKernelGGL(dleq_nonce_kernel, dim3(groups / BLOCK + 1), dim3(BLOCK), 0, stream, dleq_scalar_arg(key), (const u64*)nonces, (u64*)rows, groups);
    return (int)hipGetLastError();
}
int dleq_launch_prove(hipStream_t stream, const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3, const ShaTail& tail,
                      const uint64_t key[4], const uint64_t* r_rows, const uint8_t* st_m, const uint8_t* st_z, const uint8_t* st_t3, uint8_t* proof64, uint8_t* status, uint32_t groups) {
    hipLaunchKernelGGL(dleq_prove_kernel, sig_grid(groups), dim3(SIG_BLOCK), 0, stream, pk32, m32, z32, t2, t3, tail, dleq_scalar_arg(key), (const u64*)r_rows, st_m, st_z, st_t3,
                       proof64, status, groups);
    return (int)hipGetLastError();
}
int dleq_launch_split(hipStream_t stream, const uint8_t* proof64, const uint8_t* m32, const uint8_t* z32, uint64_t* s_rows, uint64_t* c_rows, uint64_t* pair_sc, uint64_t* pair_pt,
                      uint8_t* pre, uint32_t groups) {
    hipLaunchKernelGGL(dleq_split_kernel, sig_grid(groups), dim3(SIG_BLOCK), 0, stream, proof64, m32, z32, (u64*)s_rows, (u64*)c_rows, (u64*)pair_sc, (u64*)pair_pt, pre, groups);
    return (int)hipGetLastError();
}
int dleq_launch_check(hipStream_t stream, const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3, const ShaTail& tail,
                      const uint64_t* c_rows, const uint8_t* st_m, const uint8_t* st_z, const uint8_t* st_t2, const uint8_t* pre, const uint8_t* st_t3, uint8_t* ok, uint8_t* status,
                      uint32_t groups) {
    hipLaunchKernelGGL(dleq_check_kernel, sig_grid(groups), dim3(SIG_BLOCK), 0, stream, pk32, m32, z32, t2, t3, tail, (const u64*)c_rows, st_m, st_z, st_t2, pre, st_t3, ok, status,
                       groups);
    return (int)hipGetLastError();
}
int dleq_launch_composites_merge(hipStream_t stream, const uint8_t* st_m, const uint8_t* st_z, uint8_t* m32, uint8_t* z32, uint8_t* status, uint32_t groups) {
    hipLaunchKernelGGL(dleq_composites_merge_kernel, sig_grid(groups), dim3(SIG_BLOCK), 0, stream, st_m, st_z, (u64*)m32, (u64*)z32, status, groups);
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace fq

// The batched DLEQ proofs' own kernels (include/fourq_amd.h, "oblivious PRF: proofs"): the composite scalar of every row, the prover's
// nonce rows, challenge and response, the verifier's split / gather and its final check -- and their launchers; included by fourq_amd.hip,
// whose C ABI strings them together with the grouped sum, [k]B + [l]P, DH_endo, MUL_endo on encodings and the comb.
//
// Hashing.  Both hashed strings have a FIXED layout: 100 bytes (pk32 || C || D || I2OSP(j, 4)) or 160 bytes (pk32 || M32 || Z32 || t2 || t3)
// of 32-byte rows, then a tail that is the same for every lane -- label || DST || I2OSP(len(DST), 1) -- and travels BY VALUE in the kernel
// arguments as oprf_final_kernel's does (OprfTail: big-endian words with the 0x80 marker and the zero fill in place).  So every lane of a
// launch hashes the same number of blocks and reads the tail at the same, wave-uniform offsets; the rows go from memory straight into the
// message schedule of the block they belong to, and nothing but the state lives across a compression.
//
// Secrets.  The key k, K = 392 k mod N and the nonce r pass through dleq_nonce_kernel and dleq_prove_kernel: reductions, one product, the
// mul-sub and the zero tests are scalar_n.hip.h's straight-line code, and the status and the zeroing of a refused row are masks.  d, M, Z
// and c are public.
#pragma once
#include "oprf.hip.h"       // OprfTail, oprf_tail_word, ScalarArg; sig.hip.h: load32 / store32, SIG_BLOCK; scalar_n.hip.h

namespace fq {

constexpr int DLEQ_LABEL = 9;            // "Composite" and "Challenge"
static_assert(DLEQ_LABEL + FOURQ_H2C_MAX_DST + 1 + 1 <= 8 * (OPRF_TAIL_WORDS - 1), "the tail, its marker and one zero word fit OprfTail");
// label: DLEQ_LABEL bytes; dst: 1..255 bytes (checked by the caller)
inline OprfTail dleq_make_tail(const char* label, const uint8_t* dst, size_t dst_len) {
    OprfTail d;
    memset(&d, 0, sizeof d);
    uint8_t t[8 * OPRF_TAIL_WORDS] = { 0 };
    memcpy(t, label, DLEQ_LABEL);
    memcpy(t + DLEQ_LABEL, dst, dst_len);
    t[DLEQ_LABEL + dst_len] = (uint8_t)dst_len;
    d.tail_len = (u32)(DLEQ_LABEL + dst_len + 1);
    t[d.tail_len] = 0x80;
    for (int w = 0; w < OPRF_TAIL_WORDS; w++) for (int k = 0; k < 8; k++) d.tail[w] = (d.tail[w] << 8) | t[8 * w + k];
    return d;
}

namespace {

constexpr u32 DLEQ_COMPOSITE_PREFIX = 100, DLEQ_CHALLENGE_PREFIX = 160;

// a 32-byte row as the four big-endian words of the hashed string
FQ_DEV void dleq_row_words(const uint8_t* row, u64 w[4]) {
    u64 x[4];
    load32(row, x);
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = __builtin_bswap64(x[k]);
}

// ---- d_i = LE(H(pk32 || C_i || D_i || I2OSP(j, 4) || tail)) mod N, one lane per row, j = i mod group_size --------------------------------
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void dleq_composite_kernel(const uint8_t* pk32, const uint8_t* c32, const uint8_t* d32, OprfTail tail, u64* d_out,
                                                                             u32 group_size, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const u32 j = i % group_size;
    const u32 total = DLEQ_COMPOSITE_PREFIX + tail.tail_len, blocks = sha512_blocks(total);       // 1..3, the same for every lane
    u64 h[8], x[8], d[4];
    sha512_init(h);
#pragma unroll 1
    for (u32 b = 0; b < blocks; b++) {
        u64 w[16];
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = oprf_tail_word(tail, 128 * b + 8 * k - DLEQ_COMPOSITE_PREFIX);     // wraps in front of the tail: overwritten below
        if (b == 0) {
            dleq_row_words(pk32, w);
            dleq_row_words(c32 + 32 * (size_t)i, w + 4);
            dleq_row_words(d32 + 32 * (size_t)i, w + 8);
            w[12] = ((u64)j << 32) | (tail.tail[0] >> 32);          // the prefix ends in the middle of word 12
        }
        if (b + 1 == blocks) w[15] = (u64)total * 8;                // the bit length; w[14] is the zero fill already there
        sha512_compress(h, w);
    }
    sha512_digest_le(h, x);
    sc_reduce512(x, d);
    store32(reinterpret_cast<uint8_t*>(d_out + 4 * (size_t)i), d);
}

// block b of pk32 || M32 || Z32 || t2 || t3 || tail: 160 bytes of rows, then the tail
FQ_DEV void dleq_challenge_fill(u64 w[16], const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3, const OprfTail& tail,
                                u32 b, u32 blocks) {
    if (b == 0) {
        dleq_row_words(pk32, w); dleq_row_words(m32, w + 4); dleq_row_words(z32, w + 8); dleq_row_words(t2, w + 12);
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = oprf_tail_word(tail, 128 * b + 8 * k - DLEQ_CHALLENGE_PREFIX);     // wraps in front of the tail: overwritten below
        if (b == 1) dleq_row_words(t3, w);
    }
    if (b + 1 == blocks) w[15] = (u64)(DLEQ_CHALLENGE_PREFIX + tail.tail_len) * 8;
}
// c = LE(H(pk32 || M32 || Z32 || t2 || t3 || tail)) mod N
FQ_DEV void dleq_challenge(const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3, const OprfTail& tail, u64 c[4]) {
    const u32 blocks = sha512_blocks(DLEQ_CHALLENGE_PREFIX + tail.tail_len);       // 2..4, the same for every lane
    u64 h[8], x[8];
    sha512_init(h);
#pragma unroll 1
    for (u32 b = 0; b < blocks; b++) {
        u64 w[16];
        dleq_challenge_fill(w, pk32, m32, z32, t2, t3, tail, b, blocks);
        sha512_compress(h, w);
    }
    sha512_digest_le(h, x);
    sc_reduce512(x, c);
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
                                                                         OprfTail tail, ScalarArg key, const u64* r_rows, const uint8_t* st_m, const uint8_t* st_z,
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
    store32(reinterpret_cast<uint8_t*>(s_rows + 4 * (size_t)g), s);
    store32(reinterpret_cast<uint8_t*>(c_rows + 4 * (size_t)g), c);
    store32(reinterpret_cast<uint8_t*>(pair_sc + 8 * (size_t)g), s);
    store32(reinterpret_cast<uint8_t*>(pair_sc + 8 * (size_t)g + 4), c);
    store32(reinterpret_cast<uint8_t*>(pair_pt + 8 * (size_t)g), m);
    store32(reinterpret_cast<uint8_t*>(pair_pt + 8 * (size_t)g + 4), z);
    pre[g] = sc_lt_n(c) && sc_lt_n(s) ? (uint8_t)0 : (uint8_t)FOURQ_SIG_S_RANGE;
}

// ---- verify: hash, compare, status; one lane per group -----------------------------------------------------------------------------------------
// status[g]: the largest of the three decode codes (the group's C rows, its D rows, pk32), else pre[g], else what the sum of two said of M and
// Z (a neutral composite does not decode), else 0 with ok[g] = (c' == c)
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void dleq_check_kernel(const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3,
                                                                         OprfTail tail, const u64* c_rows, const uint8_t* st_m, const uint8_t* st_z, const uint8_t* st_t2,
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
int dleq_launch_composite(hipStream_t stream, const uint8_t* pk32, const uint8_t* c32, const uint8_t* d32, const OprfTail& tail, uint64_t* d_out, uint32_t group_size, uint32_t n) {
    hipLaunchKernelGGL(dleq_composite_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, pk32, c32, d32, tail, (u64*)d_out, group_size, n);
    return (int)hipGetLastError();
}
int dleq_launch_nonces(hipStream_t stream, const uint64_t key[4], const uint64_t* nonces, uint64_t* rows, uint32_t groups) {
    hipLaunchKernelGGL(dleq_nonce_kernel, dim3(groups / BLOCK + 1), dim3(BLOCK), 0, stream, dleq_scalar_arg(key), (const u64*)nonces, (u64*)rows, groups);
    return (int)hipGetLastError();
}
int dleq_launch_prove(hipStream_t stream, const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3, const OprfTail& tail,
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
int dleq_launch_check(hipStream_t stream, const uint8_t* pk32, const uint8_t* m32, const uint8_t* z32, const uint8_t* t2, const uint8_t* t3, const OprfTail& tail,
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

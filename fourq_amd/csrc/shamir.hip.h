// Threshold sharing's own kernels (include/fourq_amd.h, "threshold sharing"): Shamir's evaluation by Horner's rule, the powers of an id, the
// Lagrange coefficients at 0 with the merge of a set's status, the combination of scalar shares, the filler that lays the grouped sum's two
// operands out, and the status merges behind the grouped sum -- and their launchers; included by fourq_amd.hip, whose C ABI strings them
// together with the grouped sum on encodings, the comb and encode.
//
// Layout.  Party-major: item (i, r) of an array with one 32-byte item per (party, row) lies at index i * n + r.
//
// Secrets.  Coefficients, shares and combined scalars pass through shamir_shares_kernel and shamir_combine_kernel: sc_horner_step and
// scalar_n.hip.h's sc_mul, straight-line code on whole words, masked selects, no branch and no address that depends on a value.  Ids are
// public and steer control flow; so do the coefficients lambda, which are functions of the ids alone.
//
// A Horner step is v = acc x + a with acc < N, x < 2^32 and a < 2^256, so v < 2^278 + 2^256 < 2^279: five words.  sc_mul would spend 16 word
// products on acc x and 50 on Barrett's reduction of eight words.  Here: 4 for acc x, and the quotient from the TOP words alone,
//     q' = floor(floor(v / 2^192) floor(mu / 2^192) / 2^128),       mu = floor(2^512 / N) (SC_MU),
// which is 4 word products (v / 2^192 < 2^87, mu / 2^192 < 2^75), and 4 for the low words of q' N (q' < 2^35).  With V = v / 2^192 and
// M = mu / 2^192 as reals, floor(V) floor(M) > V M - V - M, and (V + M) / 2^128 < 1, so q' > v mu / 2^512 - 2 > v / N - 3 (scalar_n.hip.h:
// v mu / 2^512 > v / N - 1): q' is Q = floor(v / N), Q - 1 or Q - 2 and never above Q, v - q' N lies in [0, 3 N), below 2^248, and TWO masked
// subtractions finish.  tests/test_shamir_oracle.py restates the step on Python integers at its bounds.
#pragma once
#include "sig.hip.h"        // load32 / store32, SIG_BLOCK, SIG_WAVES, sig_grid; scalar_n.hip.h

namespace fq {

namespace {

// acc <- (acc x + a) mod N, canonical; acc < N on entry, a ANY value in [0, 2^256)
FQ_DEV void sc_horner_step(u64 acc[4], u32 x, const u64 a[4]) {
    u64 v[5], carry = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const sc_u128 p = (sc_u128)acc[k] * x + a[k] + carry;          // < 2^96 + 2^65
        v[k] = (u64)p;
        carry = (u64)(p >> 64);
    }
    v[4] = carry;                                                      // < 2^23
    const u64 m3 = SC_MU[3], m4 = SC_MU[4];                            // mu / 2^192: m4 < 2^11
    const sc_u128 mid = (((sc_u128)v[3] * m3) >> 64) + (sc_u128)v[3] * m4 + (sc_u128)v[4] * m3;      // < 2^64 + 2^75 + 2^87
    const u64 q = (u64)(mid >> 64) + v[4] * m4;                        // < 2^35
    u64 n[4], qn[4], r[4];
    sc_order(n);
    carry = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const sc_u128 p = (sc_u128)q * n[k] + carry;
        qn[k] = (u64)p;
        carry = (u64)(p >> 64);
    }
    (void)sc_sub4(v, qn, r);                                           // mod 2^256: the true difference is below 3 N < 2^248
    sc_cond_sub_n(r);
    sc_cond_sub_n(r);
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = r[k];
}
// (a + b) mod N for a, b in [0, N)
FQ_DEV void sc_add(const u64 a[4], const u64 b[4], u64 r[4]) {
    u64 carry = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const sc_u128 s = (sc_u128)a[k] + b[k] + carry;               // the sum is below 2^247: no carry leaves the top word
        r[k] = (u64)s;
        carry = (u64)(s >> 64);
    }
    sc_cond_sub_n(r);
}
FQ_DEV void sc_zero_row(u64* row) {
    const u64 z[4] = { 0, 0, 0, 0 };
    store32(reinterpret_cast<uint8_t*>(row), z);
}

// ---- shares[p][r] = sum_j a_rj ids[p]^j mod N: one (party, row) per lane, Horner from a_(t-1) down --------------------------------------------
// coeffs: n x t rows, row r's coefficients together; shares: party-major m x n rows; status[p]: FOURQ_SHAMIR_ID_ZERO where ids[p] == 0 (the
// block is zero then, and no coefficient is read), written by the lane of row 0
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void shamir_shares_kernel(const u64* coeffs, const u32* ids, u64* shares, uint8_t* status, u32 n, u32 t, u32 lanes) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= lanes) return;
    const u32 p = i / n, r = i - p * n, x = ids[p];
    u64 acc[4] = { 0, 0, 0, 0 };
    if (x != 0) {                                                      // the id is public
        const u64* row = coeffs + 4 * (size_t)r * t;
#pragma unroll 1
        for (u32 j = t; j-- > 0;) {
            u64 a[4];
            load32(reinterpret_cast<const uint8_t*>(row + 4 * (size_t)j), a);
            sc_horner_step(acc, x, a);
        }
    }
    store32(reinterpret_cast<uint8_t*>(shares + 4 * (size_t)i), acc);
    if (r == 0) status[p] = x == 0 ? (uint8_t)FOURQ_SHAMIR_ID_ZERO : (uint8_t)0;
}

// ---- sc[g][j] = ids[g]^j mod N, j = 0 .. t - 1: one lane per group, t sequential products; j = 0 gives 1 (also for the id 0) ---------------------
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void shamir_powers_kernel(const u32* ids, u64* sc, u32 groups, u32 t) {
    const u32 g = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (g >= groups) return;
    const u32 x = ids[g];
    const u64 zero[4] = { 0, 0, 0, 0 };
    u64 pw[4] = { 1, 0, 0, 0 };
    u64* row = sc + 4 * (size_t)g * t;
#pragma unroll 1
    for (u32 j = 0; j < t; j++) {
        store32(reinterpret_cast<uint8_t*>(row + 4 * (size_t)j), pw);
        sc_horner_step(pw, x, zero);
    }
}

// ---- lambda[set][i] = prod_(j != i) x_j / (x_j - x_i) mod N: one lane per (set, i) with its own inversion; nothing here is secret ----------------
// The products run over 32-bit factors: x_j, and |x_j - x_i| with the sign counted apart.  flags[set][i]: FOURQ_SHAMIR_ID_ZERO where x_i == 0,
// else FOURQ_SHAMIR_ID_REPEATED where some x_j == x_i, j != i (lambda is 0 there: the denominator is); shamir_set_status_kernel merges them.
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void shamir_lagrange_kernel(const u32* ids, u64* lambda, uint8_t* flags, u32 t, u32 lanes) {
    const u32 lane = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (lane >= lanes) return;
    const u32 set = lane / t, i = lane - set * t;
    const u32* x = ids + (size_t)set * t;
    const u32 xi = x[i];
    const u64 zero[4] = { 0, 0, 0, 0 };
    u64 num[4] = { 1, 0, 0, 0 }, den[4] = { 1, 0, 0, 0 };
    bool negative = false, repeated = false;
#pragma unroll 1
    for (u32 j = 0; j < t; j++) {
        if (j == i) continue;
        const u32 xj = x[j];
        negative ^= xj < xi;
        repeated |= xj == xi;
        sc_horner_step(num, xj, zero);
        sc_horner_step(den, xj < xi ? xi - xj : xj - xi, zero);
    }
    u64 inv[4], l[4], n[4], neg[4];
    sc_inv_reduced(den, inv);                                          // 0 for the denominator 0
    sc_mul(num, inv, l);
    sc_order(n);
    (void)sc_sub4(n, l, neg);                                          // N - l, for l != 0
    const bool flip = negative && (l[0] | l[1] | l[2] | l[3]) != 0;
#pragma unroll
    for (int k = 0; k < 4; k++) l[k] = flip ? neg[k] : l[k];
    store32(reinterpret_cast<uint8_t*>(lambda + 4 * (size_t)lane), l);
    flags[lane] = xi == 0 ? (uint8_t)FOURQ_SHAMIR_ID_ZERO : repeated ? (uint8_t)FOURQ_SHAMIR_ID_REPEATED : (uint8_t)0;
}
// status[set]: FOURQ_SHAMIR_ID_ZERO if any id of the set is 0, else FOURQ_SHAMIR_ID_REPEATED if two are equal, else 0; a set with a status has
// ALL its rows zeroed.  One lane per set
__global__ __launch_bounds__(SIG_BLOCK) void shamir_set_status_kernel(const uint8_t* flags, u64* lambda, uint8_t* status, u32 sets, u32 t) {
    const u32 set = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (set >= sets) return;
    const uint8_t* f = flags + (size_t)set * t;
    bool zero = false, repeated = false;
    for (u32 i = 0; i < t; i++) { zero |= f[i] == FOURQ_SHAMIR_ID_ZERO; repeated |= f[i] == FOURQ_SHAMIR_ID_REPEATED; }
    const uint8_t st = zero ? (uint8_t)FOURQ_SHAMIR_ID_ZERO : repeated ? (uint8_t)FOURQ_SHAMIR_ID_REPEATED : (uint8_t)0;
    status[set] = st;
    if (st) for (u32 i = 0; i < t; i++) sc_zero_row(lambda + 4 * ((size_t)set * t + i));
}

// ---- out[r] = sum_i lambda_i shares[i][r] mod N: one row per lane, t products; shares party-major, ANY value below 2^256 ------------------------
// A bad id set has every lambda zero (shamir_set_status_kernel), so every out row is zero; status: the set's byte, copied by lane 0
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void shamir_combine_kernel(const u64* lambda, const u64* shares, const uint8_t* st_set, u64* out, uint8_t* status, u32 n, u32 t) {
    const u32 r = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (r >= n) return;
    u64 acc[4] = { 0, 0, 0, 0 };
#pragma unroll 1
    for (u32 i = 0; i < t; i++) {
        u64 l[4], s[4], p[4];
        load32(reinterpret_cast<const uint8_t*>(lambda + 4 * (size_t)i), l);
        load32(reinterpret_cast<const uint8_t*>(shares + 4 * ((size_t)i * n + r)), s);
        sc_mul(l, s, p);
        sc_add(acc, p, acc);
    }
    store32(reinterpret_cast<uint8_t*>(out + 4 * (size_t)r), acc);
    if (r == 0) status[0] = st_set[0];
}

// ---- the grouped sum's operands for combine_points: sc[r][i] = lambda_i, pt[r][i] = points32[i][r] -------------------------------------------
// One lane per OUTPUT row (r, i): rows of 32 bytes as two 16-byte loads and stores; the stores of a wave are contiguous, its loads run along
// t party blocks
__global__ __launch_bounds__(SIG_BLOCK) void shamir_fill_kernel(const uint4* lambda, const uint4* points32, uint4* sc, uint4* pt, u32 n, u32 t, u32 lanes) {
    const u32 o = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (o >= lanes) return;
    const u32 r = o / t, i = o - r * t;
    const size_t from = 2 * ((size_t)i * n + r), to = 2 * (size_t)o;
    const uint4 l0 = lambda[2 * i], l1 = lambda[2 * i + 1], p0 = points32[from], p1 = points32[from + 1];
    sc[to] = l0; sc[to + 1] = l1;
    pt[to] = p0; pt[to + 1] = p1;
}
// behind the grouped sum of combine_points: a bad id set marks every row with its code and zeroes it, ahead of the sum's own codes
__global__ __launch_bounds__(SIG_BLOCK) void shamir_set_merge_kernel(const uint8_t* st_set, u64* out32, uint8_t* status, u32 n) {
    const u32 r = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (r >= n) return;
    const uint8_t st = st_set[0];
    if (st == 0) return;
    status[r] = st;
    sc_zero_row(out32 + 4 * (size_t)r);
}
// behind the grouped sum of public_shares: the id 0 marks its group FOURQ_SHAMIR_ID_ZERO and zeroes its row, ahead of the sum's own codes
__global__ __launch_bounds__(SIG_BLOCK) void shamir_id_merge_kernel(const u32* ids, u64* out32, uint8_t* status, u32 groups) {
    const u32 g = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (g >= groups) return;
    if (ids[g] != 0) return;
    status[g] = (uint8_t)FOURQ_SHAMIR_ID_ZERO;
    sc_zero_row(out32 + 4 * (size_t)g);
}
// verify: ok[g] = (pub32[g] == g32[g]) where the status is 0; the status, the first that is set: FOURQ_SHAMIR_ID_ZERO, the grouped sum's
// (st_pub), FOURQ_SIG_S_RANGE where LE(shares[g]) >= N.  The neutral point on both sides compares equal: the grouped sum encodes it as any
// point, the comb marks it FOURQ_DH_NEUTRAL in st_comb
__global__ __launch_bounds__(SIG_BLOCK) void shamir_compare_kernel(const u32* ids, const u64* pub32, const u64* g32, const u64* shares, const uint8_t* st_pub, const uint8_t* st_comb,
                                                                   uint8_t* ok, uint8_t* status, u32 groups) {
    const u32 g = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (g >= groups) return;
    u64 a[4], b[4], s[4];
    load32(reinterpret_cast<const uint8_t*>(pub32 + 4 * (size_t)g), a);
    load32(reinterpret_cast<const uint8_t*>(g32 + 4 * (size_t)g), b);
    load32(reinterpret_cast<const uint8_t*>(shares + 4 * (size_t)g), s);
    if (st_comb[g] == FOURQ_DH_NEUTRAL) { b[0] = 1; b[1] = b[2] = b[3] = 0; }          // the comb reports [0]G by its status and a zero row: 01 00 .. 00 is its encoding
    uint8_t st = ids[g] == 0 ? (uint8_t)FOURQ_SHAMIR_ID_ZERO : st_pub[g];
    if (st == 0 && !sc_lt_n(s)) st = (uint8_t)FOURQ_SIG_S_RANGE;
    const bool same = ((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3])) == 0;
    ok[g] = st == 0 && same ? (uint8_t)1 : (uint8_t)0;
    status[g] = st;
}

// ---- launchers: each returns the hipError_t of its launch ---------------------------------------------------------------------------
int shamir_launch_shares(hipStream_t stream, const uint64_t* coeffs, const uint32_t* ids, uint64_t* shares, uint8_t* status, uint32_t n, uint32_t t, uint32_t m) {
    hipLaunchKernelGGL(shamir_shares_kernel, sig_grid(n * m), dim3(SIG_BLOCK), 0, stream, (const u64*)coeffs, ids, (u64*)shares, status, n, t, n * m);
    return (int)hipGetLastError();
}
int shamir_launch_powers(hipStream_t stream, const uint32_t* ids, uint64_t* sc, uint32_t groups, uint32_t t) {
    hipLaunchKernelGGL(shamir_powers_kernel, sig_grid(groups), dim3(SIG_BLOCK), 0, stream, ids, (u64*)sc, groups, t);
    return (int)hipGetLastError();
}
// both kernels of the coefficients: lambda and the sets' statuses, the rows of a refused set zeroed
int shamir_launch_lagrange(hipStream_t stream, const uint32_t* ids, uint64_t* lambda, uint8_t* flags, uint8_t* status, uint32_t sets, uint32_t t) {
    hipLaunchKernelGGL(shamir_lagrange_kernel, sig_grid(sets * t), dim3(SIG_BLOCK), 0, stream, ids, (u64*)lambda, flags, t, sets * t);
    if (hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(shamir_set_status_kernel, sig_grid(sets), dim3(SIG_BLOCK), 0, stream, flags, (u64*)lambda, status, sets, t);
    return (int)hipGetLastError();
}
int shamir_launch_combine(hipStream_t stream, const uint64_t* lambda, const uint64_t* shares, const uint8_t* st_set, uint64_t* out, uint8_t* status, uint32_t n, uint32_t t) {
    hipLaunchKernelGGL(shamir_combine_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, (const u64*)lambda, (const u64*)shares, st_set, (u64*)out, status, n, t);
    return (int)hipGetLastError();
}
int shamir_launch_fill(hipStream_t stream, const uint64_t* lambda, const uint8_t* points32, uint64_t* sc, uint64_t* pt, uint32_t n, uint32_t t) {
    hipLaunchKernelGGL(shamir_fill_kernel, sig_grid(n * t), dim3(SIG_BLOCK), 0, stream, (const uint4*)lambda, (const uint4*)points32, (uint4*)sc, (uint4*)pt, n, t, n * t);
    return (int)hipGetLastError();
}
int shamir_launch_set_merge(hipStream_t stream, const uint8_t* st_set, uint8_t* out32, uint8_t* status, uint32_t n) {
    hipLaunchKernelGGL(shamir_set_merge_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, st_set, (u64*)out32, status, n);
    return (int)hipGetLastError();
}
int shamir_launch_id_merge(hipStream_t stream, const uint32_t* ids, uint8_t* out32, uint8_t* status, uint32_t groups) {
    hipLaunchKernelGGL(shamir_id_merge_kernel, sig_grid(groups), dim3(SIG_BLOCK), 0, stream, ids, (u64*)out32, status, groups);
    return (int)hipGetLastError();
}
int shamir_launch_compare(hipStream_t stream, const uint32_t* ids, const uint64_t* pub32, const uint64_t* g32, const uint64_t* shares, const uint8_t* st_pub, const uint8_t* st_comb,
                          uint8_t* ok, uint8_t* status, uint32_t groups) {
    hipLaunchKernelGGL(shamir_compare_kernel, sig_grid(groups), dim3(SIG_BLOCK), 0, stream, ids, (const u64*)pub32, (const u64*)g32, (const u64*)shares, st_pub, st_comb, ok, status, groups);
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace fq

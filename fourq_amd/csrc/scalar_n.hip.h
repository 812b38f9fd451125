// Arithmetic modulo the group order N (246 bits, constants.inc ORDER_N) on four 64-bit words, one value per lane.
//
//   sc_reduce512(x[8]) -> [0, N)       the little-endian integer of a SHA-512 digest
//   sc_mul(a, b), sc_mulsub(r, a, h)   a, b, r, h: ANY value in [0, 2^256); results canonical
//   sc_sub(a, b)                       a, b in [0, N)
//   sc_lt_n(s)                         s < N
//   sc_inv(a)                          a: ANY value in [0, 2^256); a^-1 mod N canonical, 0 when a = 0 (mod N) -- "inversion" below
//
// Reduction is Barrett's with mu = floor(2^512 / N) (SC_MU, 267 bits): for x < 2^512, q = floor(x * mu / 2^512) is Q = floor(x / N) or
// Q - 1 (x * mu / 2^512 > x / N - x / 2^512 > x / N - 1, so its floor is above Q - 2), hence x - q N lies in [0, 2N) and ONE masked
// subtraction of N finishes.  2N < 2^247, so the remainder needs only the low four words of x and of q N.
// The secret key's scalar and the nonce pass through here (sig_finish_kernel): everything is straight-line code on whole words --
// products, carries and masked selects; no branch and no address depends on a value.
#pragma once
#include "fp127.hip.h"      // u64, FQ_DEV; ORDER_N and SC_MU: constants.inc, which curve.hip.h includes (sig.hip.h)

namespace fq {

typedef unsigned __int128 sc_u128;

// out[0 .. NA + NB) = a * b, schoolbook by rows
template <int NA, int NB> FQ_DEV void sc_mp_mul(const u64* a, const u64* b, u64* out) {
#pragma unroll
    for (int i = 0; i < NA + NB; i++) out[i] = 0;
#pragma unroll
    for (int i = 0; i < NA; i++) {
        u64 carry = 0;
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const sc_u128 t = (sc_u128)a[i] * b[j] + out[i + j] + carry;      // < 2^128: (2^64 - 1)^2 + 2 (2^64 - 1)
            out[i + j] = (u64)t;
            carry = (u64)(t >> 64);
        }
        out[i + NB] = carry;
    }
}
// r = a - b on four words; returns the borrow (1 when a < b)
FQ_DEV u64 sc_sub4(const u64 a[4], const u64 b[4], u64 r[4]) {
    u64 borrow = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const sc_u128 t = (sc_u128)a[i] - b[i] - borrow;
        r[i] = (u64)t;
        borrow = (u64)(t >> 64) & 1;
    }
    return borrow;
}
FQ_DEV void sc_order(u64 n[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) n[i] = ORDER_N[i];
}
FQ_DEV bool sc_lt_n(const u64 s[4]) {
    u64 n[4], d[4];
    sc_order(n);
    return sc_sub4(s, n, d) != 0;
}
// r in [0, 2N) -> r mod N
FQ_DEV void sc_cond_sub_n(u64 r[4]) {
    u64 n[4], d[4];
    sc_order(n);
    const u64 keep = (u64)0 - sc_sub4(r, n, d);          // all ones when r < N
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = d[i] ^ (keep & (r[i] ^ d[i]));
}
FQ_DEV void sc_reduce512(const u64 x[8], u64 r[4]) {
    u64 mu[5], prod[13];
#pragma unroll
    for (int i = 0; i < 5; i++) mu[i] = SC_MU[i];
    sc_mp_mul<8, 5>(x, mu, prod);
    // low four words of q N, q = prod[8..12] (only its low four words can reach them)
    u64 n[4], qn[4] = { 0, 0, 0, 0 };
    sc_order(n);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u64 carry = 0;
#pragma unroll
        for (int j = 0; i + j < 4; j++) {
            const sc_u128 t = (sc_u128)prod[8 + i] * n[j] + qn[i + j] + carry;
            qn[i + j] = (u64)t;
            carry = (u64)(t >> 64);
        }
    }
    (void)sc_sub4(x, qn, r);                              // mod 2^256: the true difference is below 2^247
    sc_cond_sub_n(r);
}
FQ_DEV void sc_reduce256(const u64 a[4], u64 r[4]) {
    const u64 x[8] = { a[0], a[1], a[2], a[3], 0, 0, 0, 0 };
    sc_reduce512(x, r);
}
FQ_DEV void sc_mul(const u64 a[4], const u64 b[4], u64 r[4]) {
    u64 p[8];
    sc_mp_mul<4, 4>(a, b, p);
    sc_reduce512(p, r);
}
// a, b in [0, N)
FQ_DEV void sc_sub(const u64 a[4], const u64 b[4], u64 r[4]) {
    u64 n[4], d[4];
    sc_order(n);
    const u64 add = (u64)0 - sc_sub4(a, b, d);            // a < b: add N back
    u64 carry = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const sc_u128 t = (sc_u128)d[i] + (n[i] & add) + carry;
        r[i] = (u64)t;
        carry = (u64)(t >> 64);
    }
}
// (r - a h) mod N
FQ_DEV void sc_mulsub(const u64 r[4], const u64 a[4], const u64 h[4], u64 out[4]) {
    u64 rr[4], p[4];
    sc_reduce256(r, rr);
    sc_mul(a, h, p);
    sc_sub(rr, p, out);
}

// ---- inversion ------------------------------------------------------------------------------------------------------------------------
// a^-1 = a^(N - 2) (Fermat; N is prime), the exponent PUBLIC and fixed: 82 windows of three bits from the top, three squarings and -- where
// the window's digit is not zero -- one product with a^digit each.  The digits are read off ORDER_N by the wave-uniform window counter;
// the table entry a digit names is picked by seven masked selects, so neither a branch nor an address depends on a: the blind of an
// oblivious PRF passes through here.
//
// The 246 + 75 + 6 products of the chain are Montgomery products, a b 2^-256 mod N, 36 word products each where sc_mul's Barrett takes 66.
// For a, b < 2^247 the running sum stays below b + N + 1 < 2^248 (it is divided by 2^64 after each of the four rows), so five words
// hold it, and the result (a b + m N) / 2^256 with m < 2^256 is below 2^238 + N < 2N: no subtraction between the products.  No constant
// of the Montgomery domain is needed: a ITSELF is read as the Montgomery form of a 2^-256, the chain then ends in a^(N-2) 2^(-256 (N-3)) =
// a^-1 2^512 (2^(256 (N-1)) = 1), and two products with 1 take the 2^512 off.
FQ_DEV u64 sc_mont_n0() {                                 // -1 / N mod 2^64, by Newton from N's low word (N odd: N is its own inverse mod 8)
    const u64 n = ORDER_N[0];
    u64 x = n;
#pragma unroll
    for (int i = 0; i < 5; i++) x *= 2 - n * x;           // 3 -> 6 -> 12 -> 24 -> 48 -> 96 correct bits
    return (u64)0 - x;
}
// a b 2^-256 mod N, below 2N, for a, b < 2^247
FQ_DEV void sc_montmul(const u64 a[4], const u64 b[4], u64 n0, u64 r[4]) {
    u64 n[4], t[5] = { 0, 0, 0, 0, 0 };
    sc_order(n);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        u64 carry = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const sc_u128 x = (sc_u128)a[i] * b[j] + t[j] + carry;
            t[j] = (u64)x;
            carry = (u64)(x >> 64);
        }
        t[4] += carry;                                    // the sum is below 2^312
        const u64 m = t[0] * n0;
        carry = (u64)(((sc_u128)m * n[0] + t[0]) >> 64);  // the low word is zero by the choice of m
#pragma unroll
        for (int j = 1; j < 4; j++) {
            const sc_u128 x = (sc_u128)m * n[j] + t[j] + carry;
            t[j - 1] = (u64)x;
            carry = (u64)(x >> 64);
        }
        const sc_u128 top = (sc_u128)t[4] + carry;
        t[3] = (u64)top;
        t[4] = (u64)(top >> 64);                          // zero: the quotient is below 2^248
    }
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = t[i];
}
// digit w (0 = lowest) of N - 2 in base 8; w is wave-uniform.  N's low word ends in ...e7, so the subtraction borrows nothing
FQ_DEV u32 sc_inv_digit(u32 w) {
    const u32 bit = 3 * w, q = bit >> 6, r = bit & 63;
    const u64 lo = ORDER_N[q] - (q == 0 ? 2 : 0);
    u64 v = lo >> r;
    if (r > 61 && q < 3) v |= ORDER_N[q + 1] << (64 - r);
    return (u32)v & 7u;
}
constexpr int SC_INV_WINDOWS = 82;                        // 246 bits
// a in [0, N) -> a^-1 mod N, canonical; 0 -> 0 (every power of zero is zero)
FQ_DEV void sc_inv_reduced(const u64 a[4], u64 r[4]) {
    const u64 n0 = sc_mont_n0();
    u64 tab[8][4];                                        // tab[d] = a^d in the domain; tab[0] is never read
#pragma unroll
    for (int k = 0; k < 4; k++) { tab[0][k] = 0; tab[1][k] = a[k]; }
    sc_montmul(tab[1], tab[1], n0, tab[2]);
    sc_montmul(tab[2], tab[1], n0, tab[3]);
    sc_montmul(tab[2], tab[2], n0, tab[4]);
    sc_montmul(tab[4], tab[1], n0, tab[5]);
    sc_montmul(tab[3], tab[3], n0, tab[6]);
    sc_montmul(tab[6], tab[1], n0, tab[7]);
    u64 acc[4], sel[4];
    const u32 top = sc_inv_digit(SC_INV_WINDOWS - 1);     // 5: bit 245 is set
#pragma unroll
    for (int k = 0; k < 4; k++) {
        acc[k] = 0;
#pragma unroll
        for (int d = 1; d < 8; d++) acc[k] |= tab[d][k] & ((u64)0 - (u64)(top == (u32)d));
    }
#pragma unroll 1
    for (int w = SC_INV_WINDOWS - 2; w >= 0; w--) {
#pragma unroll 1
        for (int s = 0; s < 3; s++) sc_montmul(acc, acc, n0, acc);
        const u32 digit = sc_inv_digit((u32)w);
        if (digit == 0) continue;                         // wave-uniform: the exponent is public
#pragma unroll
        for (int k = 0; k < 4; k++) {
            sel[k] = 0;
#pragma unroll
            for (int d = 1; d < 8; d++) sel[k] |= tab[d][k] & ((u64)0 - (u64)(digit == (u32)d));
        }
        sc_montmul(acc, sel, n0, acc);
    }
    const u64 one[4] = { 1, 0, 0, 0 };
    sc_montmul(acc, one, n0, acc);
    sc_montmul(acc, one, n0, acc);                        // (x + m N) / 2^256 <= N for x < 2^247
    sc_cond_sub_n(acc);
#pragma unroll
    for (int k = 0; k < 4; k++) r[k] = acc[k];
}
// any a in [0, 2^256) -> a^-1 mod N, canonical; 0 when a = 0 (mod N)
FQ_DEV void sc_inv(const u64 a[4], u64 r[4]) {
    u64 x[4];
    sc_reduce256(a, x);
    sc_inv_reduced(x, r);
}
FQ_DEV u64 sc_is_zero_mask(const u64 a[4]) { return (a[0] | a[1] | a[2] | a[3]) == 0 ? ~(u64)0 : (u64)0; }

}  // namespace fq

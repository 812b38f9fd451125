// Arithmetic modulo the group order N (246 bits, constants.inc ORDER_N) on four 64-bit words, one value per lane.
//
//   sc_reduce512(x[8]) -> [0, N)       the little-endian integer of a SHA-512 digest
//   sc_mul(a, b), sc_mulsub(r, a, h)   a, b, r, h: ANY value in [0, 2^256); results canonical
//   sc_sub(a, b)                       a, b in [0, N)
//   sc_lt_n(s)                         s < N
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

}  // namespace fq

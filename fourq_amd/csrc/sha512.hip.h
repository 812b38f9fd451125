// SHA-512 (FIPS 180-4) on gfx950, one message per lane.
//
// The state (8), the rolling message schedule (16) and the working variables (8) are 64-bit values in VGPR pairs; rotations are written
// on the 32-bit halves as funnel shifts (v_alignbit_b32), Ch / Maj / the three-way XORs per half so that the compiler can fold them into
// v_bfi_b32 / v_bitop3_b32.  The 80 round constants are the same for every lane: they live in constant memory (constants.inc) and are
// indexed by wave-uniform values only, so they arrive through the scalar path.  Rounds 0-15 are straight-line code; rounds 16-79 are four
// trips through one 16-round body (the schedule's indices repeat with period 16 and the working variables return to their names every 8
// rounds), which keeps the whole compression at about a third of the instruction-cache footprint of 80 unrolled rounds.
//
// The hashed string of a lane is `PW` 64-bit words that are already in registers (a prefix of 0, 32 or 64 bytes: big-endian words, i.e.
// the byte string's own order) followed by `len` bytes at `row`.  Nothing is ever written behind the caller's bytes: the padding (0x80,
// zeros, the 128-bit big-endian bit length) is produced in registers.  No byte at or past row + len is read: whole 8- or 16-byte
// words are loaded only where they lie entirely inside the message, and the last, partial word is gathered byte by byte.  Lanes of one
// wave may hash strings of different lengths; the block loop then runs per lane under exec.
#pragma once
#include "fp127.hip.h"      // u32 / u64, FQ_DEV; SHA512_IV and SHA512_K: constants.inc, which curve.hip.h includes (sig.hip.h)

namespace fq {

// how a lane may load its row: by bytes (any address), or by whole 8- / 16-byte words (row start aligned that far)
enum ShaLoad { SHA_LOAD_BYTES = 0, SHA_LOAD_8 = 1, SHA_LOAD_16 = 2 };
FQ_DEV int sha_load_mode(const void* base, size_t stride) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(base) | (uintptr_t)stride;
    return (bits & 15) == 0 ? SHA_LOAD_16 : (bits & 7) == 0 ? SHA_LOAD_8 : SHA_LOAD_BYTES;
}

template <int N> FQ_DEV u64 sha_rotr(u64 x) {
    static_assert(N > 0 && N < 64, "rotation count");
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    if (N == 32) return ((u64)lo << 32) | hi;
    const u32 a = N < 32 ? lo : hi, b = N < 32 ? hi : lo;          // rotate the pair (b:a) right by N mod 32
    const u32 r_lo = __builtin_amdgcn_alignbit(b, a, N & 31), r_hi = __builtin_amdgcn_alignbit(a, b, N & 31);
    return ((u64)r_hi << 32) | r_lo;
}
FQ_DEV u64 sha_big_sigma0(u64 x) { return sha_rotr<28>(x) ^ sha_rotr<34>(x) ^ sha_rotr<39>(x); }
FQ_DEV u64 sha_big_sigma1(u64 x) { return sha_rotr<14>(x) ^ sha_rotr<18>(x) ^ sha_rotr<41>(x); }
FQ_DEV u64 sha_small_sigma0(u64 x) { return sha_rotr<1>(x) ^ sha_rotr<8>(x) ^ (x >> 7); }
FQ_DEV u64 sha_small_sigma1(u64 x) { return sha_rotr<19>(x) ^ sha_rotr<61>(x) ^ (x >> 6); }
FQ_DEV u64 sha_ch(u64 e, u64 f, u64 g) { return g ^ (e & (f ^ g)); }
FQ_DEV u64 sha_maj(u64 a, u64 b, u64 c) { return (a & b) | (c & (a | b)); }

FQ_DEV void sha512_init(u64 h[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = SHA512_IV[i];
}

// sixteen rounds from round `base` (wave-uniform, a multiple of 16) on the working variables v[0..7] = a..h
template <bool SCHEDULE> FQ_DEV void sha512_rounds16(u64 v[8], u64 w[16], u32 base) {
#pragma unroll
    for (int t = 0; t < 16; t++) {
        if (SCHEDULE) w[t] += sha_small_sigma1(w[(t + 14) & 15]) + w[(t + 9) & 15] + sha_small_sigma0(w[(t + 1) & 15]);
        // a..h rotate by one name per round: round t reads a at v[(8 - t) & 7]
        u64 &a = v[(0 - t) & 7], &b = v[(1 - t) & 7], &c = v[(2 - t) & 7], &d = v[(3 - t) & 7];
        u64 &e = v[(4 - t) & 7], &f = v[(5 - t) & 7], &g = v[(6 - t) & 7], &hh = v[(7 - t) & 7];
        const u64 t1 = hh + sha_big_sigma1(e) + sha_ch(e, f, g) + SHA512_K[base + t] + w[t];
        const u64 t2 = sha_big_sigma0(a) + sha_maj(a, b, c);
        d += t1;
        hh = t1 + t2;                 // the new a, under the name the next round expects it
    }
}
// one 128-byte block: w[0..15] big-endian words (destroyed)
FQ_DEV void sha512_compress(u64 h[8], u64 w[16]) {
    u64 v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = h[i];
    sha512_rounds16<false>(v, w, 0);
#pragma unroll 1
    for (u32 base = 16; base < 80; base += 16) sha512_rounds16<true>(v, w, base);
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] += v[i];
}

// big-endian word of the padded message at message offset m (a multiple of 8): data, the 0x80 marker behind the last byte, zeros
FQ_DEV u64 sha_word(const uint8_t* row, u32 len, u32 m, int mode) {
    if (m + 8 <= len) {
        if (mode != SHA_LOAD_BYTES) return __builtin_bswap64(*reinterpret_cast<const u64*>(row + m));
        u64 v = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) v |= (u64)row[m + k] << (56 - 8 * k);
        return v;
    }
    if (m > len) return 0;
    const u32 rem = len - m;                        // 0..7 bytes of data, then the marker
    u64 v = (u64)0x80 << (56 - 8 * rem);
#pragma unroll 1
    for (u32 k = 0; k < rem; k++) v |= (u64)row[m + k] << (56 - 8 * k);
    return v;
}

FQ_DEV u32 sha512_blocks(u32 total_bytes) { return (total_bytes + 17 + 127) / 128; }

// block b of the padded string `pre[0..PW)` ++ row[0..len) into w[0..15]
template <int PW> FQ_DEV void sha512_fill(u64 w[16], const u64* pre, const uint8_t* row, u32 len, u32 b, u32 blocks, int mode) {
    static_assert(PW >= 0 && PW <= 8 && PW % 2 == 0, "prefix: whole 16-byte units, within the first block");
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
        const u32 m = 128 * b + 8 * j - 8 * PW;     // message offset of word j (wraps for a prefix word: not used then)
        if (j < PW && b == 0) {
            w[j] = pre[j]; w[j + 1] = pre[j + 1];
        } else if (mode == SHA_LOAD_16 && m + 16 <= len) {
            const uint4 q = *reinterpret_cast<const uint4*>(row + m);
            w[j] = __builtin_bswap64(((u64)q.y << 32) | q.x);
            w[j + 1] = __builtin_bswap64(((u64)q.w << 32) | q.z);
        } else {
            w[j] = sha_word(row, len, m, mode);
            w[j + 1] = sha_word(row, len, m + 8, mode);
        }
    }
    if (b + 1 == blocks) w[15] = (u64)(8 * PW + len) * 8;      // the bit length; its upper 64 bits (w[14]) are the zeros already there
}

// SHA-512 of pre ++ row[0..len): h[0..7] big-endian words of the digest
template <int PW> FQ_DEV void sha512_hash(u64 h[8], const u64* pre, const uint8_t* row, u32 len, int mode) {
    sha512_init(h);
    const u32 blocks = sha512_blocks(8 * PW + len);
#pragma unroll 1
    for (u32 b = 0; b < blocks; b++) {
        u64 w[16];
        sha512_fill<PW>(w, pre, row, len, b, blocks, mode);
        sha512_compress(h, w);
    }
}

// the digest as the little-endian integer of its 64 bytes: word k of LE(digest) is the byte-swapped h[k]
FQ_DEV void sha512_digest_le(const u64 h[8], u64 x[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = __builtin_bswap64(h[k]);
}

}  // namespace fq

// SHA-512 (FIPS 180-4) on gfx950, one message per lane.
//
// The state (8), the rolling message schedule (16) and the working variables (8) are 64-bit values in VGPR pairs; rotations are written
// on the 32-bit halves as funnel shifts (v_alignbit_b32), Ch / Maj / the three-way XORs per half so that the compiler can fold them into
// v_bfi_b32 / v_bitop3_b32.  The 80 round constants are the same for every lane: they live in constant memory (constants.inc) and are
// indexed by wave-uniform values only, so they arrive through the scalar path.  Rounds 0-15 are straight-line code; rounds 16-79 are four
// trips through one 16-round body (the schedule's indices repeat with period 16 and the working variables return to their names every 8
// rounds), which keeps the whole compression at about a third of the instruction-cache footprint of 80 unrolled rounds.
//
// The hashed string of a lane -- EVERY string the library hashes that has a row of per-lane length in it -- is
//     `before` bytes already hashed || `PW` register words || row[0..len) || tail
// `before` is 0, or 128 behind expand_message_xmd's Z_pad block (the caller starts from SHA512_ZPAD_MID); it enters the bit length only.
// The PW words are a prefix of 0, 32 or 64 bytes: big-endian words, i.e. the byte string's own order.  The tail is the same for every
// lane: either nothing but the padding (ShaPad: the 0x80 marker, then zeros) or a ShaTail, which travels BY VALUE in the kernel arguments
// (nothing is staged, so the _dev calls stay capturable) as big-endian words with the marker and the zero fill in place; a lane reads it
// at the byte offset its row's length gives.  sha512_fill is the one place that lays such a string into message blocks, and its rules are:
//   - nothing is ever written behind the caller's bytes: marker, zeros and the 128-bit big-endian bit length are produced in registers;
//   - no byte at or past row + len is read, and a row of length 0 is never dereferenced: whole 8- or 16-byte words are loaded only where
//     they lie entirely inside the row and the load mode (the alignment of base and stride) allows them; the word that straddles the
//     row's end is gathered byte by byte;
//   - branches and addresses depend on lengths, offsets and the load mode only, never on a message byte or a prefix word (a prefix may
//     be a secret, a message a password).
// Lanes of one wave may hash strings of different lengths; the block loop then runs per lane under exec.  sha512_hash_rows is the
// fixed-layout sibling: whole 32-byte rows, an optional counter, a ShaTail -- every lane the same number of blocks.
//
// Everything here but the launch side is plain C++ behind one qualifier macro: a stand-alone program that includes this header with an
// ordinary C++ compiler gets the same filler, tail builder, compression function and rows hasher (tests/c/sha_string_check.cpp runs them
// on the CPU, under the sanitizers too, each row at the end of its own allocation).
#pragma once
#include "../../include/fourq_amd.h"      // FOURQ_H2C_MAX_DST
#if defined(__HIPCC__)
#include "fp127.hip.h"      // u32 / u64, FQ_DEV; SHA512_IV, SHA512_K, SHA512_ZPAD_MID: constants.inc, which curve.hip.h includes (sig.hip.h)
#define FQ_HD __host__ __device__ __forceinline__
#else
#include <stdint.h>
#include <string.h>
namespace fq {
typedef uint32_t u32;
typedef uint64_t u64;
#include "constants.inc"
}
#define FQ_DEV inline
#define FQ_HD inline
#endif

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
#if defined(__HIPCC__)
    const u32 r_lo = __builtin_amdgcn_alignbit(b, a, N & 31), r_hi = __builtin_amdgcn_alignbit(a, b, N & 31);
#else
    const u32 r_lo = (a >> (N & 31)) | (b << (32 - (N & 31))), r_hi = (b >> (N & 31)) | (a << (32 - (N & 31)));
#endif
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

FQ_HD u32 sha512_blocks(u32 total_bytes) { return (total_bytes + 17 + 127) / 128; }

// ---- the tail -------------------------------------------------------------------------------------------------------------------------
// head || DST || I2OSP(len(DST), 1) || 0x80 || zeros as big-endian words; len counts the bytes in front of the marker.  The heads are
// "Finalize" (oprf.hip.h), the 9-byte labels of dleq.hip.h and vrf.hip.h, I2OSP(len_in_bytes, 2) || 0x00 and the counter byte 0x01 of
// expand_message_xmd (h2c.hip.h)
constexpr int SHA_TAIL_WORDS = 35, SHA_TAIL_MAX_HEAD = 9;
static_assert(SHA_TAIL_MAX_HEAD + FOURQ_H2C_MAX_DST + 1 + 1 <= 8 * (SHA_TAIL_WORDS - 1),
              "the longest head, DST, its length byte and the marker, and one zero word behind what a shifted read can reach");
struct ShaTail {
    u64 w[SHA_TAIL_WORDS];
    u32 len;
};
struct ShaPad {};                        // no tail: the marker follows the row
// head_len <= SHA_TAIL_MAX_HEAD; dst: 1..FOURQ_H2C_MAX_DST bytes (both checked by the caller)
inline ShaTail sha_make_tail(const void* head, size_t head_len, const uint8_t* dst, size_t dst_len) {
    ShaTail t;
    memset(&t, 0, sizeof t);
    uint8_t b[8 * SHA_TAIL_WORDS] = { 0 };
    memcpy(b, head, head_len);
    memcpy(b + head_len, dst, dst_len);
    b[head_len + dst_len] = (uint8_t)dst_len;
    t.len = (u32)(head_len + dst_len + 1);
    b[t.len] = 0x80;
    for (int w = 0; w < SHA_TAIL_WORDS; w++) for (int k = 0; k < 8; k++) t.w[w] = (t.w[w] << 8) | b[8 * w + k];
    return t;
}
FQ_DEV u32 sha_tail_len(const ShaTail& t) { return t.len; }
FQ_DEV u32 sha_tail_len(const ShaPad&) { return 0; }
// big-endian word of the tail at byte offset `at` (marker and zeros included; zero behind the array, so an offset that wrapped is harmless)
FQ_DEV u64 sha_tail_word(const ShaTail& t, u32 at) {
    const u32 q = at >> 3, r = 8 * (at & 7);
    const u32 qa = q < (u32)SHA_TAIL_WORDS - 1 ? q : (u32)SHA_TAIL_WORDS - 1;          // the last word is zero
    const u32 qb = q + 1 < (u32)SHA_TAIL_WORDS - 1 ? q + 1 : (u32)SHA_TAIL_WORDS - 1;
    const u64 a = t.w[qa], b = t.w[qb];
    return r ? (a << r) | (b >> (64 - r)) : a;
}
FQ_DEV u64 sha_tail_word(const ShaPad&, u32 at) { return at == 0 ? (u64)0x80 << 56 : 0; }

// ---- the string -----------------------------------------------------------------------------------------------------------------------
// 16 bytes at a 16-byte aligned address as two big-endian words
FQ_DEV void sha_load16(const uint8_t* p, u64& hi, u64& lo) {
    typedef u64 pair_t __attribute__((vector_size(16)));
    const pair_t q = *reinterpret_cast<const pair_t*>(p);
    hi = __builtin_bswap64(q[0]);
    lo = __builtin_bswap64(q[1]);
}
// big-endian word at offset m (a multiple of 8) of row[0..len) ++ tail: data, the word that straddles the row's end, tail
template <class Tail> FQ_DEV u64 sha_string_word(const uint8_t* row, u32 len, const Tail& tail, u32 m, int mode) {
    if (m + 8 <= len) {
        if (mode != SHA_LOAD_BYTES) return __builtin_bswap64(*reinterpret_cast<const u64*>(row + m));
        u64 v = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) v |= (u64)row[m + k] << (56 - 8 * k);
        return v;
    }
    if (m >= len) return sha_tail_word(tail, m - len);
    const u32 rem = len - m;                        // 1..7 bytes of data, then the tail's first bytes
    u64 v = sha_tail_word(tail, 0) >> (8 * rem);
#pragma unroll 1
    for (u32 k = 0; k < rem; k++) v |= (u64)row[m + k] << (56 - 8 * k);
    return v;
}
// block b of the padded string into w[0..15]; `blocks` = sha512_blocks(8 PW + len + the tail's length) -- `before` is whole blocks
template <int PW, class Tail>
FQ_DEV void sha512_fill(u64 w[16], const u64* pre, const uint8_t* row, u32 len, const Tail& tail, u32 before, u32 b, u32 blocks, int mode) {
    static_assert(PW >= 0 && PW <= 8 && PW % 2 == 0, "prefix: whole 16-byte units, within the first block");
#pragma unroll
    for (int j = 0; j < 16; j += 2) {
        const u32 m = 128 * b + 8 * j - 8 * PW;     // offset of word j into row ++ tail (wraps for a prefix word: not used then)
        if (j < PW && b == 0) {
            w[j] = pre[j]; w[j + 1] = pre[j + 1];
        } else if (mode == SHA_LOAD_16 && m + 16 <= len) {
            sha_load16(row + m, w[j], w[j + 1]);
        } else {
            w[j] = sha_string_word(row, len, tail, m, mode);
            w[j + 1] = sha_string_word(row, len, tail, m + 8, mode);
        }
    }
    // the bit length; its upper 64 bits (w[14]) are the zeros already there
    if (b + 1 == blocks) w[15] = (u64)(before + 8 * PW + len + sha_tail_len(tail)) * 8;
}

// SHA-512 of pre ++ row[0..len) ++ tail: h[0..7] big-endian words of the digest
template <int PW, class Tail> FQ_DEV void sha512_hash(u64 h[8], const u64* pre, const uint8_t* row, u32 len, const Tail& tail, int mode) {
    sha512_init(h);
    const u32 blocks = sha512_blocks(8 * PW + len + sha_tail_len(tail));
#pragma unroll 1
    for (u32 b = 0; b < blocks; b++) {
        u64 w[16];
        sha512_fill<PW>(w, pre, row, len, tail, 0, b, blocks, mode);
        sha512_compress(h, w);
    }
}

// SHA-512 of R rows of 32 bytes (16-byte aligned) [++ I2OSP(counter, 4)] ++ tail.  The layout is fixed: every lane hashes the same number
// of blocks and reads the tail at the same, wave-uniform offsets; a row never straddles a block and goes from memory straight into the
// message schedule of the block it belongs to, so nothing but the state lives across a compression
template <int R, bool COUNTER> FQ_DEV void sha512_hash_rows(u64 h[8], const uint8_t* const (&rows)[R], u32 counter, const ShaTail& tail) {
    constexpr u32 PREFIX = 32 * R + (COUNTER ? 4 : 0);
    const u32 total = PREFIX + tail.len, blocks = sha512_blocks(total);
    sha512_init(h);
#pragma unroll 1
    for (u32 b = 0; b < blocks; b++) {
        u64 w[16];
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = sha_tail_word(tail, 128 * b + 8 * k - PREFIX);      // wraps in front of the tail: replaced below
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (b != (u32)r / 4) continue;
            sha_load16(rows[r], w[4 * (r % 4)], w[4 * (r % 4) + 1]);
            sha_load16(rows[r] + 16, w[4 * (r % 4) + 2], w[4 * (r % 4) + 3]);
        }
        if (COUNTER && b == (u32)R / 4) w[4 * (R % 4)] = ((u64)counter << 32) | (tail.w[0] >> 32);      // the rows end in the middle of this word
        if (b + 1 == blocks) w[15] = (u64)total * 8;
        sha512_compress(h, w);
    }
}

// the digest as the little-endian integer of its 64 bytes: word k of LE(digest) is the byte-swapped h[k]
FQ_DEV void sha512_digest_le(const u64 h[8], u64 x[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = __builtin_bswap64(h[k]);
}

}  // namespace fq

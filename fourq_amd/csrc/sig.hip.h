// The signature layer's own kernels -- SHA-512 with one message per lane (sha512.hip.h) and arithmetic modulo the group order
// (scalar_n.hip.h) -- and their launchers; included by fourq_amd.hip, whose C ABI strings them together with the comb, the ladder and
// the combiner.  The scheme (include/fourq_amd.h, "signatures from bytes"):
//   keygen   k = H(sk), pk = encode([LE(k[0:32])]G)
//   sign     r = LE(H(k[32:64] || msg)) mod N, R = encode([r]G), h = LE(H(R || pk || msg)) mod N, s = (r - LE(k[0:32]) h) mod N
//   verify   s < N, h as above, encode([s]G + [h]decode(pk)) == R
// Every hashed string is sha512.hip.h's: prefix words in registers (k[32:64], or R || pk), the message row, padding only (ShaPad).  ONE
// challenge kernel serves sig_verify and its keyed sibling: KeyRows says whether the key row is row i or a slot of the registered set.
// Throughput kernels: ~2 600 instructions of code, 40 live 64-bit values, no LDS, no scratch memory.  Every launcher returns the
// hipError_t of its launch.
#pragma once
#include "curve.hip.h"      // constants.inc: ORDER_N, SC_MU, SHA512_IV, SHA512_K
#include "lower.hip.h"      // put_words
#include "sha512.hip.h"
#include "scalar_n.hip.h"
#include "../../include/fourq_amd.h"

namespace fq {

// a batch of messages: row i is `stride` bytes apart from row i - 1 and holds lens[i] (lens == NULL: msg_len) bytes; a length above
// `stride` is clamped to it by the kernels (and reported where the call has a status)
struct SigMsgs {
    const uint8_t* rows;
    size_t stride;
    const uint32_t* lens;
    uint32_t msg_len;
};
// whose public key a row is checked against: row i of `bytes` (ids == NULL; no key status), or slot ids[i] of a registered key set of `count`
// keys (fourq_keyset_set) with the slots' 32-byte rows in `bytes` and their statuses in `status`
struct KeyRows {
    const uint32_t* ids;
    const uint8_t* bytes;
    const uint8_t* status;
    uint32_t count;
};

namespace {

constexpr int SIG_BLOCK = 256;
constexpr int SIG_WAVES = 4;      // waves per SIMD the hashing kernels are held to (128 VGPRs): 40 live 64-bit values fit with room to spare

struct LaneMsg { const uint8_t* row; u32 len; bool clamped; };
FQ_DEV LaneMsg lane_msg(const SigMsgs& m, u32 i) {
    LaneMsg l;
    u32 len = m.lens ? m.lens[i] : m.msg_len;
    l.clamped = len > m.stride;
    l.len = l.clamped ? (u32)m.stride : len;
    l.row = m.rows + (size_t)i * m.stride;
    return l;
}
// 32 bytes at a 16-byte aligned row as four little-endian words
FQ_DEV void load32(const uint8_t* p, u64 w[4]) {
    const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
    w[0] = ((u64)lo.y << 32) | lo.x; w[1] = ((u64)lo.w << 32) | lo.z;
    w[2] = ((u64)hi.y << 32) | hi.x; w[3] = ((u64)hi.w << 32) | hi.z;
}
FQ_DEV void store32(uint8_t* p, const u64 w[4]) {
    put_words<4>(reinterpret_cast<u64*>(p), w);
}
// a 32-byte row as the four big-endian words of a hashed string
FQ_DEV void dleq_row_words(const uint8_t* row, u64 w[4]) {
    sha_load16(row, w[0], w[1]);
    sha_load16(row + 16, w[2], w[3]);
}
// the key row of lane i (`at`) and the key's status: an index outside the set is clamped BEFORE it becomes an address
FQ_DEV uint8_t key_row(const KeyRows& keys, u32 i, u32& at) {
    at = i;
    if (!keys.ids) return 0;
    const u32 id = keys.ids[i];
    at = id < keys.count ? id : keys.count - 1;
    return id < keys.count ? keys.status[at] : (uint8_t)FOURQ_KEYSET_ID_RANGE;
}
// the challenge h = LE(SHA-512(R || pk || msg)) mod N; R, pk as little-endian words of their 32 bytes
FQ_DEV void challenge(const u64 R[4], const u64 pk[4], const LaneMsg& l, int mode, u64 h[4]) {
    u64 pre[8], d[8], x[8];
#pragma unroll
    for (int k = 0; k < 4; k++) { pre[k] = __builtin_bswap64(R[k]); pre[4 + k] = __builtin_bswap64(pk[k]); }
    sha512_hash<8>(d, pre, l.row, l.len, ShaPad{}, mode);
    sha512_digest_le(d, x);
    sc_reduce512(x, h);
}

__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void sha512_kernel(SigMsgs m, uint8_t* out64, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const LaneMsg l = lane_msg(m, i);
    u64 d[8], x[8];
    sha512_hash<0>(d, nullptr, l.row, l.len, ShaPad{}, sha_load_mode(m.rows, m.stride));
    sha512_digest_le(d, x);
    store32(out64 + 64 * (size_t)i, x);
    store32(out64 + 64 * (size_t)i + 32, x + 4);
}

// the pre-status carries the whole precedence: the key's (key_row), a clamped message, s >= N
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void sig_challenge_kernel(KeyRows keys, SigMsgs m, const uint8_t* sig64, u64* s_out, u64* h_out, u64* r_out,
                                                                            uint8_t* pre_status, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const LaneMsg l = lane_msg(m, i);
    u32 at;
    const uint8_t key = key_row(keys, i, at);
    u64 R[4], s[4], pk[4], h[4];
    load32(sig64 + 64 * (size_t)i, R);
    load32(sig64 + 64 * (size_t)i + 32, s);
    load32(keys.bytes + 32 * (size_t)at, pk);
    // s, R and the status byte leave before the hash: nothing of them stays live across it
    store32(reinterpret_cast<uint8_t*>(s_out + 4 * (size_t)i), s);
    store32(reinterpret_cast<uint8_t*>(r_out + 4 * (size_t)i), R);
    pre_status[i] = key ? key : l.clamped ? (uint8_t)FOURQ_SIG_MSG_CLAMPED : sc_lt_n(s) ? (uint8_t)0 : (uint8_t)FOURQ_SIG_S_RANGE;
    challenge(R, pk, l, sha_load_mode(m.rows, m.stride), h);
    store32(reinterpret_cast<uint8_t*>(h_out + 4 * (size_t)i), h);
}

// One pass through ONE copy of the compression function: step 0 hashes the 32-byte secret key (a single block), steps 1.. hash
// k[32:64] || msg.  The step counter is wave-uniform; only the number of steps differs between lanes (by the message's length).
template <bool NONCE>
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void sig_nonce_kernel(const uint8_t* sk32, SigMsgs m, u64* a_out, u64* r_out, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 sk[4], pre[4], h[8];
    load32(sk32 + 32 * (size_t)i, sk);
#pragma unroll
    for (int k = 0; k < 4; k++) pre[k] = __builtin_bswap64(sk[k]);
    LaneMsg l = { nullptr, 0, false };
    if (NONCE) l = lane_msg(m, i);
    const int mode = NONCE ? sha_load_mode(m.rows, m.stride) : SHA_LOAD_BYTES;
    const u32 blocks = sha512_blocks(32 + l.len), steps = NONCE ? 1 + blocks : 1;
    sha512_init(h);
#pragma unroll 1
    for (u32 step = 0; step < steps; step++) {
        u64 w[16];
        if (step == 1) {                                   // k = H(sk) is complete: a leaves, k[32:64] becomes the next string's prefix
            u64 a[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { a[k] = __builtin_bswap64(h[k]); pre[k] = h[4 + k]; }
            store32(reinterpret_cast<uint8_t*>(a_out + 4 * (size_t)i), a);
            sha512_init(h);
        }
        // step 0: the string is the prefix alone (sk, one block); afterwards block step - 1 of k[32:64] || msg
        const bool first = step == 0;
        sha512_fill<4>(w, pre, l.row, first ? 0 : l.len, ShaPad{}, 0, first ? 0 : step - 1, first ? 1 : blocks, mode);
        sha512_compress(h, w);
    }
    if (NONCE) {
        u64 x[8], r[4];
        sha512_digest_le(h, x);
        sc_reduce512(x, r);
        store32(reinterpret_cast<uint8_t*>(r_out + 4 * (size_t)i), r);
    } else {
        u64 a[4];
#pragma unroll
        for (int k = 0; k < 4; k++) a[k] = __builtin_bswap64(h[k]);
        store32(reinterpret_cast<uint8_t*>(a_out + 4 * (size_t)i), a);
    }
}

__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void sig_finish_kernel(const uint8_t* r32, const uint8_t* pk32, SigMsgs m, const u64* a_in, const u64* r_in, uint8_t* sig64, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const LaneMsg l = lane_msg(m, i);
    u64 R[4], pk[4], h[4], a[4], r[4], s[4];
    load32(r32 + 32 * (size_t)i, R);
    load32(pk32 + 32 * (size_t)i, pk);
    store32(sig64 + 64 * (size_t)i, R);
    challenge(R, pk, l, sha_load_mode(m.rows, m.stride), h);
    load32(reinterpret_cast<const uint8_t*>(a_in + 4 * (size_t)i), a);
    load32(reinterpret_cast<const uint8_t*>(r_in + 4 * (size_t)i), r);
    sc_mulsub(r, a, h, s);
    store32(sig64 + 64 * (size_t)i + 32, s);
}

__global__ __launch_bounds__(SIG_BLOCK) void sig_merge_kernel(const uint8_t* pre_status, uint8_t* ok, uint8_t* status, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t pre = pre_status[i];
    if (pre && status[i] == 0) { ok[i] = 0; status[i] = pre; }          // a key that does not decode takes precedence
}

__global__ __launch_bounds__(64) void scalar_prim_kernel(int op, const u64* in, u64* out, u32 n) {
    const u32 i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    u64* y = out + 4 * (size_t)i;
    u64 r[4];
    if (op == FOURQ_SC_REDUCE512) {
        const u64* x = in + 8 * (size_t)i;
        const u64 v[8] = { x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7] };
        sc_reduce512(v, r);
    } else if (op == FOURQ_SC_MUL) {
        const u64* x = in + 8 * (size_t)i;
        const u64 a[4] = { x[0], x[1], x[2], x[3] }, b[4] = { x[4], x[5], x[6], x[7] };
        sc_mul(a, b, r);
    } else if (op == FOURQ_SC_INV) {
        const u64* x = in + 4 * (size_t)i;
        const u64 a[4] = { x[0], x[1], x[2], x[3] };
        sc_inv(a, r);
    } else {
        const u64* x = in + 12 * (size_t)i;
        const u64 rr[4] = { x[0], x[1], x[2], x[3] }, a[4] = { x[4], x[5], x[6], x[7] }, h[4] = { x[8], x[9], x[10], x[11] };
        sc_mulsub(rr, a, h, r);
    }
    y[0] = r[0]; y[1] = r[1]; y[2] = r[2]; y[3] = r[3];
}

inline dim3 sig_grid(u32 n) { return dim3((n + SIG_BLOCK - 1) / SIG_BLOCK); }

int sig_launch_sha512(hipStream_t stream, SigMsgs m, uint8_t* out64, uint32_t n) {
    hipLaunchKernelGGL(sha512_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, m, out64, n);
    return (int)hipGetLastError();
}
// h = SHA-512(R || pk || msg) mod N from sig64 = R || s; writes s, h, R as 32-byte rows and the pre-status byte the merge reads
int sig_launch_challenge(hipStream_t stream, const KeyRows& keys, SigMsgs m, const uint8_t* sig64, uint64_t* s_out, uint64_t* h_out, uint64_t* r_out, uint8_t* pre_status,
                         uint32_t n) {
    hipLaunchKernelGGL(sig_challenge_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, keys, m, sig64, (u64*)s_out, (u64*)h_out, (u64*)r_out, pre_status, n);
    return (int)hipGetLastError();
}
// k = SHA-512(sk): a = LE(k[0:32]) (not reduced) into a_out; with `nonce`, r = SHA-512(k[32:64] || msg) mod N into r_out
int sig_launch_nonce(hipStream_t stream, bool nonce, const uint8_t* sk32, SigMsgs m, uint64_t* a_out, uint64_t* r_out, uint32_t n) {
    if (nonce) hipLaunchKernelGGL(sig_nonce_kernel<true>, sig_grid(n), dim3(SIG_BLOCK), 0, stream, sk32, m, (u64*)a_out, (u64*)r_out, n);
    else hipLaunchKernelGGL(sig_nonce_kernel<false>, sig_grid(n), dim3(SIG_BLOCK), 0, stream, sk32, m, (u64*)a_out, (u64*)r_out, n);
    return (int)hipGetLastError();
}
int sig_launch_finish(hipStream_t stream, const uint8_t* r32, const uint8_t* pk32, SigMsgs m, const uint64_t* a, const uint64_t* r, uint8_t* sig64, uint32_t n) {
    hipLaunchKernelGGL(sig_finish_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, r32, pk32, m, (const u64*)a, (const u64*)r, sig64, n);
    return (int)hipGetLastError();
}
// behind the combiner: where the key decoded (status == 0) and pre_status is set, ok = 0 and status = pre_status
int sig_launch_merge(hipStream_t stream, const uint8_t* pre_status, uint8_t* ok, uint8_t* status, uint32_t n) {
    hipLaunchKernelGGL(sig_merge_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, pre_status, ok, status, n);
    return (int)hipGetLastError();
}
int sig_launch_scalar_prim(hipStream_t stream, int op, const uint64_t* in, uint64_t* out, uint32_t n) {
    hipLaunchKernelGGL(scalar_prim_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, op, (const u64*)in, (u64*)out, n);
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace fq

// The oblivious PRF's own kernels (include/fourq_amd.h, "oblivious PRF"): the batched inversion modulo N, the key broadcast, the status
// merge behind a blinding and the finalisation hash -- and their launchers; included by fourq_amd.hip, whose C ABI strings them together
// with the hash-to-curve stages, the ladders, DH_endo and the lowering.
//
// Inversion (sc_inv_kernel<K>).  One Fermat chain (scalar_n.hip.h, sc_inv_reduced) costs about as much as a whole ladder, so a lane inverts
// the PRODUCT of its K elements t, t + T, ..., t + (K-1) T, T = ceil(n / K), and unfolds it (Montgomery's trick inside a lane, as
// lower_kernel does for the field inversion): 3 (K - 1) sc_mul beside the chain.  An element that is 0 mod N contributes a 1 to the
// product by mask and gets 0 back, so it cannot touch its neighbours.  Only the K - 1 prefix products stay in registers across the chain;
// the elements are loaded and reduced again on the way back.  A lane's slots past the end of the batch redo its first element and store
// nothing.  Everything is masks and straight-line code on whole words: no branch and no address depends on a value.
//
// Finalisation (oprf_final_kernel).  F(E, msg) = SHA-512(E || msg || tail), tail = "Finalize" || DST || I2OSP(len(DST), 1): sha512_hash
// (sha512.hip.h) with the 32 bytes of E as its register prefix (PW = 4) -- the row follows at string offset 32, a multiple of 16, so an
// aligned row keeps its vector loads -- and the tail as a ShaTail by value in the kernel arguments.
#pragma once
#include "h2c.hip.h"        // sig.hip.h: SigMsgs, lane_msg, load32 / store32, SIG_BLOCK; scalar_n.hip.h

namespace fq {

struct ScalarArg { u64 w[4]; };

namespace {

// ---- inversion modulo N ------------------------------------------------------------------------------------------------------------------
// zero (optional): FOURQ_OPRF_BLIND_ZERO where the element is 0 mod N, 0 elsewhere
template <int K>
__global__ __launch_bounds__(BLOCK) void sc_inv_kernel(const u64* in, u64* out, uint8_t* zero, u32 n) {
    const u32 T = (n + K - 1) / K;
    const u32 t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= T) return;
    u64 pre[K][4];
#pragma clang loop unroll(full)
    for (int j = 0; j < K; j++) {
        const u32 id = t + (u32)j * T, at = id < n ? id : t;
        u64 a[4];
        load32(reinterpret_cast<const uint8_t*>(in + 4 * (size_t)at), a);
        sc_reduce256(a, a);
        const u64 z = sc_is_zero_mask(a);
        a[0] |= z & 1;                                                    // 0 -> 1
        if (j == 0) { pre[0][0] = a[0]; pre[0][1] = a[1]; pre[0][2] = a[2]; pre[0][3] = a[3]; }
        else sc_mul(pre[j - 1], a, pre[j]);
    }
    u64 inv[4];
    sc_inv_reduced(pre[K - 1], inv);
#pragma clang loop unroll(full)
    for (int j = K - 1; j >= 0; j--) {
        const u32 id = t + (u32)j * T, at = id < n ? id : t;
        u64 a[4], r[4];
        load32(reinterpret_cast<const uint8_t*>(in + 4 * (size_t)at), a);
        sc_reduce256(a, a);
        const u64 z = sc_is_zero_mask(a);
        a[0] |= z & 1;
        if (j > 0) { sc_mul(inv, pre[j - 1], r); sc_mul(inv, a, inv); }
        else { r[0] = inv[0]; r[1] = inv[1]; r[2] = inv[2]; r[3] = inv[3]; }
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] &= ~z;
        if (id >= n) continue;
        store32(reinterpret_cast<uint8_t*>(out + 4 * (size_t)id), r);
        if (zero) zero[id] = z ? (uint8_t)FOURQ_OPRF_BLIND_ZERO : (uint8_t)0;
    }
}

// ---- one scalar on n rows (the key of a batch of evaluations); it travels as a kernel argument, as broadcast_point_kernel's point does
__global__ __launch_bounds__(BLOCK) void oprf_fill_key_kernel(ScalarArg key, u64* out, u32 n) {
    const u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    store32(reinterpret_cast<uint8_t*>(out + 4 * (size_t)i), key.w);
}

// ---- behind a blinding: the lowering has left 0 in status (its points come from the map); the call's own codes go on top, the row is zeroed
__global__ __launch_bounds__(SIG_BLOCK) void oprf_blind_merge_kernel(const u64* blinds, SigMsgs m, u64* out32, uint8_t* status, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 b[4];
    load32(reinterpret_cast<const uint8_t*>(blinds + 4 * (size_t)i), b);
    sc_reduce256(b, b);
    const bool zero = sc_is_zero_mask(b) != 0, clamped = lane_msg(m, i).clamped;
    const uint8_t st = zero ? (uint8_t)FOURQ_OPRF_BLIND_ZERO : clamped ? (uint8_t)FOURQ_SIG_MSG_CLAMPED : (uint8_t)0;
    if (status[i] != 0 || st == 0) return;
    const u64 z[4] = { 0, 0, 0, 0 };
    store32(reinterpret_cast<uint8_t*>(out32 + 4 * (size_t)i), z);
    status[i] = st;
}

// ---- the finalisation hash ---------------------------------------------------------------------------------------------------------------
// out64[i] = F(e32[i], msg_i); status[i] = st_in[i] (a decode or DH code of the stages in front), else st_zero[i] (optional: the blind was
// 0 mod N), else FOURQ_SIG_MSG_CLAMPED for a clamped row; the row is all zero unless 0
__global__ __launch_bounds__(SIG_BLOCK, SIG_WAVES) void oprf_final_kernel(const uint8_t* e32, SigMsgs m, ShaTail d, const uint8_t* st_in, const uint8_t* st_zero,
                                                                         uint8_t* out64, uint8_t* status, u32 n) {
    const u32 i = blockIdx.x * SIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const LaneMsg l = lane_msg(m, i);
    const int mode = sha_load_mode(m.rows, m.stride);
    u64 e[4], pre[4], h[8], x[8];
    load32(e32 + 32 * (size_t)i, e);
#pragma unroll
    for (int k = 0; k < 4; k++) pre[k] = __builtin_bswap64(e[k]);
    uint8_t st = st_in[i];
    if (st == 0 && st_zero) st = st_zero[i];
    if (st == 0 && l.clamped) st = (uint8_t)FOURQ_SIG_MSG_CLAMPED;
    sha512_hash<4>(h, pre, l.row, l.len, d, mode);
    sha512_digest_le(h, x);
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = st ? 0 : x[k];
    store32(out64 + 64 * (size_t)i, x);
    store32(out64 + 64 * (size_t)i + 32, x + 4);
    status[i] = st;
}

// ---- launchers: each returns the hipError_t of its launch ---------------------------------------------------------------------------
constexpr int OPRF_SCINV_K_MID = 8, OPRF_SCINV_K_BIG = 16;      // the K values shipped beside 1
int oprf_launch_sc_inv(hipStream_t stream, int k, const uint64_t* in, uint64_t* out, uint8_t* zero, uint32_t n) {
    const u32 lanes = (n + (u32)k - 1) / (u32)k;
    const dim3 grid((lanes + BLOCK - 1) / BLOCK), block(BLOCK);
    if (k == OPRF_SCINV_K_BIG) hipLaunchKernelGGL(sc_inv_kernel<OPRF_SCINV_K_BIG>, grid, block, 0, stream, (const u64*)in, (u64*)out, zero, n);
    else if (k == OPRF_SCINV_K_MID) hipLaunchKernelGGL(sc_inv_kernel<OPRF_SCINV_K_MID>, grid, block, 0, stream, (const u64*)in, (u64*)out, zero, n);
    else hipLaunchKernelGGL(sc_inv_kernel<1>, grid, block, 0, stream, (const u64*)in, (u64*)out, zero, n);
    return (int)hipGetLastError();
}
int oprf_launch_fill_key(hipStream_t stream, const uint64_t key[4], uint64_t* out, uint32_t n) {
    ScalarArg k;
    for (int i = 0; i < 4; i++) k.w[i] = key[i];
    hipLaunchKernelGGL(oprf_fill_key_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, k, (u64*)out, n);
    return (int)hipGetLastError();
}
int oprf_launch_blind_merge(hipStream_t stream, const uint64_t* blinds, SigMsgs m, uint8_t* out32, uint8_t* status, uint32_t n) {
    hipLaunchKernelGGL(oprf_blind_merge_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, (const u64*)blinds, m, (u64*)out32, status, n);
    return (int)hipGetLastError();
}
int oprf_launch_final(hipStream_t stream, const uint8_t* e32, SigMsgs m, const ShaTail& d, const uint8_t* st_in, const uint8_t* st_zero, uint8_t* out64,
                      uint8_t* status, uint32_t n) {
    hipLaunchKernelGGL(oprf_final_kernel, sig_grid(n), dim3(SIG_BLOCK), 0, stream, e32, m, d, st_in, st_zero, out64, status, n);
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace fq

// libfourq_amd.so -- first translation unit: the fused variable-base kernels, the small service kernels
// (tables, partition, wire format, primitives) and the C ABI declared in include/fourq_amd.h.  The
// fixed-base and comb kernels live in fourq_chain.hip; shared device code in kernels.hip.h.
//
// Kernel design (gfx950): one wavefront lane owns one (scalar, point) pair for the whole scalar
// multiplication.  Lanes never communicate; a workgroup is 256 lanes; the grid is sized to the
// number of resident lanes and strides over the batch.  (The exception: variable-base batches of at most
// half a generation, and remainders past whole generations, run TWO lanes per element -- real parts in even
// lanes, imaginary parts in odd lanes, halves exchanged by DPP -- at 0.66 of the latency: pair.hip.h.)
//
//   variable base : the lane builds its own 8-entry R2 table (table_endo / table_windowed): N, D of every entry into
//                   a 768-byte slot of HBM scratch (96 bytes per entry = two memory sectors), E, F into its rows of
//                   LDS; each ladder step then gathers the coordinates of the entry its digit selects (wavefront-
//                   level gather, one entry per lane) a whole doubling ahead of their use.
//   fixed base    : the 8-entry table is staged once per workgroup into LDS (padded to dodge bank
//                   conflicts) and gathered from there.
//   selection     : as the reference's selectpt (curve4q.py:193-206): the sign of a digit is applied by masked selects
//                   (N/D exchanged by one v_bitop3_b32 per limb, F negated by a two-op conditional negation) and never
//                   becomes an address; the table index is a per-lane address, as in the reference (curve4q.py:232,
//                   :440).  With FOURQ_CT_SELECT / fourq_ctx_set_ct_select every step reads the whole table instead
//                   and selects the entry by masks too (fourq_ct_*.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <mutex>
#include <new>
#include <optional>
#include <thread>
#include <utility>
#include <vector>

#ifndef FQ_CHAIN
#define FQ_CHAIN 0
#endif
#include "kernels.hip.h"
#include "pipeline_plan.h"
#include "work_layout.h"
#include "sig.hip.h"
#include "h2c.hip.h"
#include "oprf.hip.h"
#include "dleq_layout.h"
#include "keyset_layout.h"
#include "msm_shape.h"
#include "dleq.hip.h"
#include "vrf_layout.h"
#include "vrf.hip.h"
#include "shamir_layout.h"
#include "shamir.hip.h"

using namespace fq;

namespace {

// packed table (8 x 16 words) -> working limbs (8 x 48 u32)
__global__ void table_unpack_kernel(const u64* packed, u32* limbs) {
    int k = threadIdx.x;
    if (k < 8) store_r2_limbs(limbs + k * R2_LIMBS, load_r2_packed(packed + 16 * k));
}
// working limbs of one lane's scratch slot -> packed table
__global__ void table_build_kernel(int algo, const u64* p_r1, u32* scratch, u64* packed) {
    if (threadIdx.x != 0) return;
    R1 P = load_r1(p_r1);
    if (algo == ENDO) build_table_endo(P, scratch); else build_table_windowed(P, scratch);
    for (int k = 0; k < 8; k++) store_r2_packed(packed + 16 * k, load_r2_limbs(scratch + k * R2_LIMBS));
}
// Mixed batches: compacts the ids of the variable-base elements of one round (flags[i] != 0) into var_list (any
// order), counted in counter[0].  Sixteen flags per lane, a block scan in LDS and one atomic per 4 096 elements; one
// atomic per element (or per wave) serialises on the counter.
constexpr int PART_PER_LANE = 16;
// fix_list (optional): the ids of the fixed-base elements, counted in counter[1].
__global__ __launch_bounds__(BLOCK) void partition_kernel(const uint8_t* flags, u32 n, u32 first_id, u32* var_list, u32* counter, u32* fix_list) {
    __shared__ u32 scan[BLOCK], base, base_fix;
    const u32 t = threadIdx.x;
    const u32 first = (blockIdx.x * BLOCK + t) * PART_PER_LANE;
    const u32 valid = first < n ? (n - first < (u32)PART_PER_LANE ? n - first : (u32)PART_PER_LANE) : 0u;
    uint8_t f[PART_PER_LANE];
    if (valid == PART_PER_LANE && (reinterpret_cast<uintptr_t>(flags) & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(flags + first);
        const u32 w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (int k = 0; k < PART_PER_LANE; k++) f[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int k = 0; k < PART_PER_LANE; k++) f[k] = (u32)k < valid ? flags[first + k] : (uint8_t)0;
    }
    u32 mine = 0;
#pragma unroll
    for (int k = 0; k < PART_PER_LANE; k++) mine += ((u32)k < valid && f[k] != 0) ? 1u : 0u;
    scan[t] = mine;
    __syncthreads();
    for (u32 off = 1; off < BLOCK; off <<= 1) {           // inclusive scan
        const u32 below = t >= off ? scan[t - off] : 0u;
        __syncthreads();
        scan[t] += below;
        __syncthreads();
    }
    if (t == BLOCK - 1) {
        base = atomicAdd(counter, scan[t]);
        if (fix_list) {                                   // fixed-base elements of this block = its valid elements - variable ones
            const u32 block_first = blockIdx.x * BLOCK * PART_PER_LANE;
            const u32 block_valid = block_first < n ? (n - block_first < (u32)(BLOCK * PART_PER_LANE) ? n - block_first : (u32)(BLOCK * PART_PER_LANE)) : 0u;
            base_fix = atomicAdd(counter + 1, block_valid - scan[t]);
        }
    }
    __syncthreads();
    u32 rank = base + scan[t] - mine;
    // fixed-base elements before this lane inside the block: elements before it minus variable ones before it
    u32 rank_fix = fix_list ? base_fix + (t * PART_PER_LANE - (scan[t] - mine)) : 0u;
#pragma unroll
    for (int k = 0; k < PART_PER_LANE; k++) {
        if ((u32)k >= valid) break;
        if (f[k] != 0) var_list[rank++] = first_id + first + k;
        else if (fix_list) fix_list[rank_fix++] = first_id + first + k;
    }
}

// One lane per point of the table object (both shapes, recode.hip.h): [2^(e j) (1 + u0 2^d + u1 2^2d + ...)] B by the ordinary
// variable-base MUL_endo, normalised to affine and stored as (x+y, y-x, 2d x y), 12 packed words.
__global__ __launch_bounds__(BLOCK) void comb_table_kernel(const u64* p_r1, u32* scratch, u64* comb) {
    const u32 t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= (u32)COMB_POINTS) return;
    u64 m[4];
    if (t < (u32)CombFast::POINTS) comb_point_scalar<CombFast>(t, m); else comb_point_scalar<CombScan>(t - CombFast::POINTS, m);
    R1 P = load_r1(p_r1);
    u32* slot = scratch + (size_t)t * SLOT_U32;
    build_table_endo(P, slot);
    u64 v[4];
    decompose(m, v);
    R1 Q = ladder_endo_hipcc(recode(v), slot, R2_LIMBS);
    Fe2<1> x, y;
    r1_to_affine(Q, x, y);
    u64* dst = comb + 12 * (size_t)t;
    store_fe2(dst, fe2_add(x, y));
    store_fe2(dst + 4, fe2_sub(y, x));
    store_fe2(dst + 8, fe2_mul(fe2_mul(x, y), fe2_two_d()));
}
__global__ void comb_unpack_kernel(const u64* packed, u32* limbs) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= COMB_POINTS) return;
    for (int c = 0; c < 3; c++) store_fe2_limbs(limbs + k * COMB_ENTRY_U32 + c * COORD_U32, load_fe2(packed + 12 * k + 4 * c));
}
// ---- point compression ---------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void encode_kernel(const u64* affine, u64* out, u32 n) {
    u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 w[4];
    point_encode(load_fe2(affine + 8 * (size_t)i), load_fe2(affine + 8 * (size_t)i + 4), w);
    uint4* dst = reinterpret_cast<uint4*>(out + 4 * (size_t)i);
    dst[0] = make_uint4((u32)w[0], (u32)(w[0] >> 32), (u32)w[1], (u32)(w[1] >> 32));
    dst[1] = make_uint4((u32)w[2], (u32)(w[2] >> 32), (u32)w[3], (u32)(w[3] >> 32));
}
__global__ __launch_bounds__(BLOCK) void decode_kernel(const u64* in, u64* affine, uint8_t* status, u32 n) {
    u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 w[4];
    load_scalar(in + 4 * (size_t)i, w);
    Fe2<1> x, y;
    int st = point_decode(w, x, y);
    u64 o[8];
    store_fe2_words(o, x); store_fe2_words(o + 4, y);
    uint4* dst = reinterpret_cast<uint4*>(affine + 8 * (size_t)i);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        u64 lo = st ? 0 : o[2 * k], hi = st ? 0 : o[2 * k + 1];
        dst[k] = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    }
    status[i] = (uint8_t)st;
}

// Protocol step, last stage: encode the shared point and merge the per-stage verdicts into one status byte
//   0 ok | FOURQ_DH_* of the DH stage | 16 + FOURQ_DECODE_* of the decode stage (which wins); out32 is zero unless 0.
__global__ __launch_bounds__(BLOCK) void encode_status_kernel(const u64* affine, const uint8_t* st_decode, const uint8_t* st_dh,
                                                              u64* out, uint8_t* status, u32 n) {
    u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint8_t sd = st_decode[i], sh = st_dh ? st_dh[i] : 0;        // st_dh == NULL: a stage that cannot fail (MUL_*)
    const uint8_t st = sd ? (uint8_t)(16 + sd) : sh;
    u64 w[4];
    point_encode(load_fe2(affine + 8 * (size_t)i), load_fe2(affine + 8 * (size_t)i + 4), w);
    if (st) w[0] = w[1] = w[2] = w[3] = 0;
    put_words<4>(out + 4 * (size_t)i, w);
    status[i] = st;
}
// one affine point replicated n times (the public base of a batch of exchanges); the point travels as a kernel argument,
// so the call neither copies from pageable host memory nor keeps a host buffer alive behind the caller's back
struct AffineArg { u64 w[FOURQ_AFFINE_WORDS]; };
__global__ __launch_bounds__(BLOCK) void broadcast_point_kernel(AffineArg point, u64* out, u32 n) {
    u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    put_words<8>(out + 8 * (size_t)i, point.w);
}
// MUL_* with affine I/O ("affine-only I/O variant"): AffineToR1 in front (curve4q.py:100-101), R1toAffine behind
// (curve4q.py:103-106, one GFp2.inv per element: ~2 % of a MUL_endo's multiply-adds).  The R1 rows in between stay on the device.
__global__ __launch_bounds__(BLOCK) void lift_affine_kernel(const u64* affine, u64* r1, u32 n) {
    u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint4* src = reinterpret_cast<const uint4*>(affine + 8 * (size_t)i);
    uint4* dst = reinterpret_cast<uint4*>(r1 + 20 * (size_t)i);
    const uint4 x0 = src[0], x1 = src[1], y0 = src[2], y1 = src[3];
    dst[0] = x0; dst[1] = x1; dst[2] = y0; dst[3] = y1;                                  // X, Y
    dst[4] = make_uint4(1, 0, 0, 0); dst[5] = make_uint4(0, 0, 0, 0);                   // Z = 1
    dst[6] = x0; dst[7] = x1; dst[8] = y0; dst[9] = y1;                                  // Ta = X, Tb = Y
}
// R1toAffine behind a MUL_*, K elements per lane with one GFp.inv (lower.hip.h; ~2 % of a MUL_endo's multiply-adds at K = 1).  Source: rows of
// `stride` words, 20 (R1) or 12 ((X, Y, Z)).  Masked: a zero norm, when K > 1 -- MUL_* accepts any pair of field elements (curve4q.py never checks),
// and the all-zero point a failed decode is lifted to DOES come out with Z = 0.  K = 1 for chunks within two generations (one wave per SIMD: the
// chain's latency is the time either way), K = 4 beyond (throughput: 0.29 -> 0.12 ms per 2^20 elements).  ENC: the result leaves as a 32-byte
// encoding + status byte instead of 64 bytes of affine words.
template <int K, bool ENC>
__global__ __launch_bounds__(BLOCK) void lower_kernel(const u64* r1, u32 stride, const uint8_t* st_decode, u64* out, uint8_t* status, u32 n) {
    LaneSlots<K> s(n);
    if (!s.lane(blockIdx.x * BLOCK + threadIdx.x)) return;
    Fe2<1> z[K];
#pragma clang loop unroll(full)
    for (int j = 0; j < K; j++) z[j] = load_fe2(r1 + stride * (size_t)s.at(j) + 8);
    SharedInverse<K, FeOps<false>> si;
#pragma clang loop unroll(full)
    for (int j = 0; j < K; j++) {
        const Fe<1> norm = z_norm(z[j]);
        if constexpr (K > 1) si.take(j, norm, !fe_is_zero(norm)); else si.take(j, norm);
    }
    si.invert();
#pragma clang loop unroll(full)
    for (int j = K - 1; j >= 0; j--) {
        const u64* row = r1 + stride * (size_t)s.at(j);
        const Fe2<1> X = load_fe2(row), Y = load_fe2(row + 4);
        const Fe2<1> zi = z_inverse(z[j], si.peel(j));
        const Fe2<1> ax = fe2_mul(X, zi), ay = fe2_mul(Y, zi);
        if (!s.live(j)) continue;
        if constexpr (ENC) put_encoded(out, status, s.id(j), ax, ay, bytes_decode_status(st_decode[s.id(j)]));
        else put_affine(out, s.id(j), ax, ay);
    }
}
// The 32-byte I/O flavour of MUL_* as THREE kernels per chunk instead of five (round 5): decode + AffineToR1 in one (the decoded point
// never exists as an affine row), R1toAffine + encode + status in one.  Same values as decode_kernel -> lift_affine_kernel and
// lower_r1_kernel -> encode_status_kernel: a point that does not decode is lifted as all-zero coordinates with Z = 1, its product is
// computed like any other and its output zeroed by the status (lower_kernel<K, true>).
__global__ __launch_bounds__(BLOCK) void decode_lift_kernel(const u64* in, u64* r1, uint8_t* status, u32 n) {
    u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 w[4];
    load_scalar(in + 4 * (size_t)i, w);
    Fe2<1> x, y;
    const int st = point_decode(w, x, y);
    u64 o[8];
    store_fe2_words(o, x); store_fe2_words(o + 4, y);
    uint4 q[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u64 lo = st ? 0 : o[2 * k], hi = st ? 0 : o[2 * k + 1];
        q[k] = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    }
    uint4* dst = reinterpret_cast<uint4*>(r1 + 20 * (size_t)i);
    dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2]; dst[3] = q[3];                          // X, Y
    dst[4] = make_uint4(1, 0, 0, 0); dst[5] = make_uint4(0, 0, 0, 0);                   // Z = 1
    dst[6] = q[0]; dst[7] = q[1]; dst[8] = q[2]; dst[9] = q[3];                          // Ta = X, Tb = Y
    status[i] = (uint8_t)st;
}
// status of a two-stage exchange: the first failure of either half (the second half already zeroed its output)
// Diagnostic (fourq_diag_clock): one wave per block stamps the shader-cycle counter (s_memtime) and the constant 100 MHz counter
// (s_memrealtime), sleeps until the latter has advanced by `ticks`, and stamps again: shader cycles per 10 ns = the clock the chip holds
// while whatever ELSE is running runs.  No product kernel carries a stamp.  Every wave leaves: the wait is on a free-running counter and
// bounded by a spin limit besides.
__global__ __launch_bounds__(64) void clock_probe_kernel(u64* stamps, u64 ticks) {
    const u64 c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    u64 r1 = r0;
    for (u32 spin = 0; spin < (1u << 24) && r1 - r0 < ticks; spin++) {
        __builtin_amdgcn_s_sleep(64);
        r1 = __builtin_amdgcn_s_memrealtime();
    }
    const u64 c1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { stamps[2 * blockIdx.x] = c1 - c0; stamps[2 * blockIdx.x + 1] = r1 - r0; }
}

// The bracket form (fourq_diag_clock_begin / _stop / _end): NO probe stays resident beside the work -- a sleeping wave still holds eight
// registers of its SIMD, and a kernel that fills the register file (the LDS-table ladders: 2 x 256 VGPRs per SIMD) then loses a whole
// workgroup slot on that CU: config 3 ran 30 % slower under the round-6 first attempt (profiles/r06_clock_probe.txt).  Instead two launches
// of this kernel ON THE CONTEXT'S STREAM, one before and one after the bracketed work, each wave recording its CU's cycle counter and the
// global 100 MHz counter.  s_memtime is a PER-CU counter (tools/microbench/stamp_coherence.hip: 256 CUs, each coherent within 113 cycles,
// offsets between CUs up to 4 x 10^7), so the host pairs the two launches' stamps CU by CU (key = XCC_ID, and SE / SH / CU of HW_ID).
__global__ __launch_bounds__(64) void clock_stamp_kernel(u64* stamps) {
    u64 t, r;
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t), "=s"(r) :: "memory");
    const u32 xcc = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20) & 15;        // HW_REG_XCC_ID[3:0]
    const u32 hw = __builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4) & 0xFF00;      // HW_REG_HW_ID: cu 11:8, sh 12, se 15:13
    if (threadIdx.x == 0) { u64* o = stamps + 3 * (size_t)blockIdx.x; o[0] = (u64)xcc << 16 | hw; o[1] = t; o[2] = r; }
}

__global__ __launch_bounds__(BLOCK) void merge_status_kernel(const uint8_t* first, uint8_t* status, u32 n) {
    u32 i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n && first[i]) status[i] = first[i];
}

// ---- primitives ----------------------------------------------------------------------------------
FQ_DEV Fe<1> ld_fe(const u64* w) { return fe_unpack(w[0], w[1]); }
template <int B> FQ_DEV void st_fe(u64* w, const Fe<B>& a) { fe_canon(a, w[0], w[1]); }
template <int BX, int BY, int BZ> FQ_DEV void st_proj(u64* w, const Proj<BX, BY, BZ>& p) {
    store_fe2(w, p.X); store_fe2(w + 4, p.Y); store_fe2(w + 8, p.Z);
}
FQ_DEV R2s ld_r2s(const u64* w) { return as_signed(load_r2_packed(w)); }

__global__ __launch_bounds__(64) void prim_kernel(int op, const u64* in, u64* out, u32 n, u32 iw, u32 ow) {
    u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64* x = in + (size_t)i * iw;
    u64* y = out + (size_t)i * ow;
    switch (op) {
    case FOURQ_FP_ADD: st_fe(y, fe_add(ld_fe(x), ld_fe(x + 2))); break;
    case FOURQ_FP_SUB: st_fe(y, fe_sub(ld_fe(x), ld_fe(x + 2))); break;
    case FOURQ_FP_MUL: st_fe(y, fe_mul(ld_fe(x), ld_fe(x + 2))); break;
    case FOURQ_FP_SQR: st_fe(y, fe_sqr(ld_fe(x))); break;
    case FOURQ_FP_NEG: st_fe(y, fe_neg(ld_fe(x))); break;
    case FOURQ_FP_INV: st_fe(y, fe_inv(fe_carry(ld_fe(x)))); break;
    case FOURQ_FP_INVSQRT: st_fe(y, fe_invsqrt(fe_carry(ld_fe(x)))); break;
    case FOURQ_FP_SELECT:
    case FOURQ_FP2_SELECT: {
        // (mask * c) mod 2^128 = -c mod 2^128 for the reference's mask = 2^512 - 1; bit operations on the raw words,
        // no reduction (the reference's select does none either)
        const u64 m_lo = 0 - x[0], m_hi = ~x[1] + (x[0] == 0 ? 1 : 0);
        const int parts = op == FOURQ_FP_SELECT ? 1 : 2;
        const u64* a = x + 2;
        const u64* b = x + 2 + 2 * parts;
        for (int k = 0; k < parts; k++) {
            y[2 * k] = b[2 * k] ^ (m_lo & (a[2 * k] ^ b[2 * k]));
            y[2 * k + 1] = b[2 * k + 1] ^ (m_hi & (a[2 * k + 1] ^ b[2 * k + 1]));
        }
        break;
    }
    case FOURQ_FP2_ADD: store_fe2(y, fe2_add(load_fe2(x), load_fe2(x + 4))); break;
    case FOURQ_FP2_SUB: store_fe2(y, fe2_sub(load_fe2(x), load_fe2(x + 4))); break;
    case FOURQ_FP2_MUL: store_fe2(y, fe2_mul(load_fe2(x), load_fe2(x + 4))); break;
    case FOURQ_FP2_SQR: store_fe2(y, fe2_sqr(load_fe2(x))); break;
    case FOURQ_FP2_NEG: store_fe2(y, fe2_neg(load_fe2(x))); break;
    case FOURQ_FP2_CONJ: store_fe2(y, fe2_conj(load_fe2(x))); break;
    case FOURQ_FP2_INV: store_fe2(y, fe2_inv(load_fe2(x))); break;
    case FOURQ_PT_DBL: store_r1(y, dbl(load_r1(x))); break;
    case FOURQ_PT_ADD: store_r1(y, add(load_r1(x), ld_r2s(x + 20))); break;
    case FOURQ_PT_ADD_CORE: {
        R2 p = load_r2_packed(x);
        R3 p3; p3.N = widen<2>(p.N); p3.D = widen<3>(p.D); p3.E = p.E; p3.F = p.F;
        store_r1(y, add_core(p3, ld_r2s(x + 16)));
        break;
    }
    case FOURQ_PT_R1TOR2: store_r2_packed(y, r1_to_r2(load_r1(x))); break;
    case FOURQ_PT_R1TOR3: {
        R3 r = r1_to_r3(load_r1(x));
        store_fe2(y, r.N); store_fe2(y + 4, r.D); store_fe2(y + 8, r.E); store_fe2(y + 12, r.F);
        break;
    }
    case FOURQ_PT_R2TOR4: st_proj(y, r2_to_r4(ld_r2s(x))); break;
    case FOURQ_PT_TAU: st_proj(y, tau(load_fe2(x), load_fe2(x + 4), load_fe2(x + 8))); break;
    case FOURQ_PT_TAU_DUAL:
        store_r1(y, tau_dual(widen<2>(load_fe2(x)), widen<2>(load_fe2(x + 4)), widen<2>(load_fe2(x + 8))));
        break;
    case FOURQ_PT_UPSILON:
    case FOURQ_PT_CHI: {
        Proj<1, 2, 1> p; p.X = load_fe2(x); p.Y = widen<2>(load_fe2(x + 4)); p.Z = load_fe2(x + 8);
        if (op == FOURQ_PT_UPSILON) st_proj(y, upsilon(p)); else st_proj(y, chi(p));
        break;
    }
    case FOURQ_PT_PHI: store_r1(y, phi(load_r1(x))); break;
    case FOURQ_PT_PSI: store_r1(y, psi(load_r1(x))); break;
    case FOURQ_PT_ON_CURVE: y[0] = point_on_curve(load_fe2(x), load_fe2(x + 4)) ? 1 : 0; break;
    case FOURQ_PT_COFACTOR392: store_r1(y, clear_cofactor_392(load_fe2(x), load_fe2(x + 4))); break;
    case FOURQ_PT_R1TOAFFINE: {
        Fe2<1> ax, ay;
        r1_to_affine(load_r1(x), ax, ay);
        store_fe2(y, ax); store_fe2(y + 4, ay);
        break;
    }
    case FOURQ_SC_DECOMPOSE: {
        u64 m[4] = { x[0], x[1], x[2], x[3] }, v[4];
        decompose(m, v);
        y[0] = v[0]; y[1] = v[1]; y[2] = v[2]; y[3] = v[3];
        break;
    }
    case FOURQ_SC_RECODE: {
        u64 v[4] = { x[0], x[1], x[2], x[3] };
        EndoDigits e = recode(v);
        y[0] = e.sign; y[1] = e.d[0]; y[2] = e.d[1]; y[3] = e.d[2]; y[4] = e.top;
        break;
    }
    case FOURQ_SC_RECODE_NIBBLES: {
        u64 v[4] = { x[0], x[1], x[2], x[3] };
        EndoNibbles e = recode_nibbles(v);
        for (int k = 0; k < 8; k++) y[k] = e.w[k];
        y[8] = e.top;
        break;
    }
    case FOURQ_SC_WINDOWED: {
        u64 m[4] = { x[0], x[1], x[2], x[3] };
        WinScalar w = win_reduce(m);
        uint8_t* b = reinterpret_cast<uint8_t*>(y);
        for (int k = 0; k < 62; k++) b[k] = (uint8_t)win_code_from_window(win_window(w, k));
        b[62] = (uint8_t)win_top_code(w);
        b[63] = 0;
        break;
    }
    default: break;
    }
}

struct PrimShape { int op; size_t in_words, out_words; };
const PrimShape PRIMS[] = {
    { FOURQ_FP_ADD, 4, 2 }, { FOURQ_FP_SUB, 4, 2 }, { FOURQ_FP_MUL, 4, 2 }, { FOURQ_FP_SQR, 4, 2 }, { FOURQ_FP_NEG, 4, 2 }, { FOURQ_FP_INV, 4, 2 }, { FOURQ_FP_INVSQRT, 4, 2 },
    { FOURQ_FP_SELECT, 6, 2 }, { FOURQ_FP2_SELECT, 10, 4 },
    { FOURQ_FP2_ADD, 8, 4 }, { FOURQ_FP2_SUB, 8, 4 }, { FOURQ_FP2_MUL, 8, 4 }, { FOURQ_FP2_SQR, 8, 4 }, { FOURQ_FP2_NEG, 8, 4 },
    { FOURQ_FP2_CONJ, 8, 4 }, { FOURQ_FP2_INV, 8, 4 },
    { FOURQ_PT_DBL, 20, 20 }, { FOURQ_PT_ADD, 36, 20 }, { FOURQ_PT_ADD_CORE, 32, 20 }, { FOURQ_PT_R1TOR2, 20, 16 },
    { FOURQ_PT_R1TOR3, 20, 16 }, { FOURQ_PT_R2TOR4, 16, 12 }, { FOURQ_PT_TAU, 12, 12 }, { FOURQ_PT_TAU_DUAL, 12, 20 },
    { FOURQ_PT_UPSILON, 12, 12 }, { FOURQ_PT_CHI, 12, 12 }, { FOURQ_PT_PHI, 20, 20 }, { FOURQ_PT_PSI, 20, 20 },
    { FOURQ_PT_ON_CURVE, 8, 1 }, { FOURQ_PT_COFACTOR392, 8, 20 }, { FOURQ_PT_R1TOAFFINE, 20, 8 },
    { FOURQ_PT_MAP_ELL2, 4, 8 },                                                             // h2c.hip.h
    { FOURQ_SC_DECOMPOSE, 4, 4 }, { FOURQ_SC_RECODE, 4, 5 }, { FOURQ_SC_RECODE_NIBBLES, 4, 9 }, { FOURQ_SC_WINDOWED, 4, 8 },
    { FOURQ_SC_REDUCE512, 8, 4 }, { FOURQ_SC_MULSUB, 12, 4 }, { FOURQ_SC_MUL, 8, 4 }, { FOURQ_SC_INV, 4, 4 },        // sig.hip.h (scalar_n.hip.h)
};
const PrimShape* find_prim(int op) {
    for (const PrimShape& p : PRIMS) if (p.op == op) return &p;
    return nullptr;
}

}  // namespace

// ====================================================================================== C ABI
// Which host-array call this is, for the measured planner inputs (fourq_ctx::plan_kt).  A call with two flavours that are timed apart
// (ENDO / WINDOWED, RO / NU, without / with table392) names the flavour in PipeRoute::variant, 0 or 1.
enum PipeRouteId { PR_MUL_VAR, PR_MUL_FIX, PR_DH_VAR, PR_DH_FIX, PR_MIXED, PR_COMB, PR_ENCODE, PR_DECODE, PR_DHB_VAR, PR_DHB_FIX, PR_AFF, PR_BYTES, PR_EXCH, PR_EXCH_COMB,
                   PR_DOUBLE_AFF, PR_DOUBLE_BYTES, PR_DOUBLE_VERIFY, PR_SHA512, PR_SIG_KEYGEN, PR_SIG_SIGN, PR_SIG_VERIFY, PR_H2F, PR_H2C_MAP, PR_H2C, PR_H2C_AFFINE,
                   PR_OPRF_BLIND, PR_OPRF_EVALUATE, PR_OPRF_FINALIZE, PR_OPRF_EVAL, PR_SC_INV, PR_KEYSET_DOUBLE, PR_KEYSET_VERIFY, PR_VRF_PROVE, PR_VRF_VERIFY, PR_VRF_KEYED, PR_VRF_HASH,
                   PR_COUNT };
constexpr int PIPE_SLOTS_MAX = 6;
struct fourq_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int cus = 0;
    size_t lanes = 0;              // resident lanes of the fused variable-base kernels (1 wave per SIMD)
    size_t lanes_w4 = 0;           // resident lanes of the 128-VGPR kernels (4 waves per SIMD)
    size_t mixed_round = 0;        // elements per round of a mixed batch (<= lanes_w4; FOURQ_MIXED_ROUND)
    u32* scratch = nullptr;        // table slots: the largest of its users (fourq_ctx_create)
    u32* table_limbs = nullptr;    // 8 x 48: the staged fixed-base table as working limbs
    u64* table_packed = nullptr;   // 128 words
    u32* comb_limbs = nullptr;     // FOURQ_COMB_POINTS x 36 working limbs of the staged comb table
    u64* comb_packed = nullptr;    // FOURQ_COMB_POINTS x 12 words
    u32* commit_combs = nullptr;   // fourq_commit_bases_set: commit_count combs of COMB_POINTS x COMB_ENTRY_U32 working limbs, back to back
    size_t commit_count = 0;
    u32* keyset_combs = nullptr;   // fourq_keyset_set: keyset_count combs of the same shape, one per registered public key (a refused slot's is all zero)
    uint8_t* keyset_bytes = nullptr;   // ... the keys as registered, keyset_count x 32 bytes, and behind them one status byte per slot
    uint8_t* keyset_status = nullptr;
    size_t keyset_count = 0;
    fq_work::ShapePlan shape;      // fourq_raggedsum_shape_set: the installed shape's passes (groups == 0: none was ever set) ...
    uint2* shape_desc = nullptr;   // ... and every pass's descriptors on the device, back to back as in shape.desc (NULL where no pass is needed)
    uint64_t table_shadow[FOURQ_TABLE_WORDS];   // host copies of what table_limbs / comb_limbs currently hold
    uint64_t comb_shadow[FOURQ_COMB_WORDS];
    bool table_staged = false, comb_staged = false;
    bool comb_known = false;           // comb_shadow holds a caller's table (it survives a change of stream; the device copy is staged again from it)
    hipEvent_t shadow_read = nullptr;   // recorded behind every upload from a shadow: a shadow is rewritten only after its last upload has read it
    u32* part_counter = nullptr;   // mixed batches: number of variable-base elements of the current round (device side)
    u32* part_list = nullptr;      // their ids, lanes_w4 entries
    u32* part_fix = nullptr;       // ids of the round's fixed-base elements
    bool ct = false;               // constant-time table selection (FOURQ_CT_SELECT / fourq_ctx_set_ct_select)
    int mixed_queue = -1;          // FOURQ_MIXED_QUEUE (test hook): 0 or 1 keeps a mixed batch off the pair-lane kernels; in constant-time mode 1 forces the
                                   // work-queue kernel and 0 the fused kernel + mixed_ct_tail_kernel for every round; the default mode runs the queue kernel either way
    size_t quad_max = 0;           // ... and of at most this many, four lanes per element (a quarter generation fills the chip)
    size_t pair_max = 0;           // variable-base batches (and tails past whole generations) of at most this many elements run two lanes per element
    uint4* proj = nullptr;         // deferred normalisation of DH batches: PROJ_PLANES planes of proj_capacity uint4, grown on demand
    size_t proj_capacity = 0;
    int scinv_k = 0;               // fourq_ctx_set_scinv_group (test hook): 1 / 8 / 16 = that many elements per inversion modulo N whatever the batch size; 0 = by batch size
    int norm_k = -1;               // FOURQ_NORM_K: 0 = always invert per element, 2/4/8 = always batch; -1 = by batch size
    char* stage = nullptr;         // staging for the small host-pointer calls (tables, primitives) and the grouped calls' host arrays
    size_t stage_bytes = 0;
    char* work = nullptr;          // intermediates of the protocol-level calls (decoded points, first-half results): WorkScope
    size_t work_bytes = 0;
    fq_work::Hold work_hold, proj_hold, stage_hold;    // who is using work / proj / stage right now (work_layout.h): a held buffer does not grow
    // host-pointer batches: pipe_slots device slots (and pinned bounce slots for pageable callers) cycled through
    // H2D copy -> kernels -> D2H copy on three streams
    hipStream_t copy_in = nullptr, copy_out = nullptr;
    hipEvent_t in_done[PIPE_SLOTS_MAX] = {}, kernels_done[PIPE_SLOTS_MAX] = {}, out_done[PIPE_SLOTS_MAX] = {};
    std::vector<hipEvent_t> ticks;     // timing events around the copies, four per chunk of the call: recorded only under host_timing
    int pipe_slots = 0;            // FOURQ_PIPE_SLOTS (test hook): slots in flight, 2..PIPE_SLOTS_MAX; 0 = 4 when the GPU hands slots on, 3 when the host does
    int pipe_gens = 0;             // FOURQ_PIPE_GENS (test hook): > 0 = that many kernel generations per inner chunk instead of the planned sizes (pipeline_plan.h)
    bool pipe_host_poll = false;   // FOURQ_PIPE_HOST_POLL=1 (test hook): the host's wait for a slot spins on hipEventQuery instead of hipEventSynchronize
    bool pipe_host_wait = false;   // FOURQ_PIPE_HOST_WAIT=1 (test hook): the host waits for a slot's last use before refilling it, as rounds 2-4 did
    bool host_timing = false;      // fourq_ctx_set_host_timing: time the chunk copies with HIP events (h2d_ms / d2h_ms of fourq_host_stats)
    // Measured planner inputs (round 6): every multi-chunk host-array call times ONE middle chunk (six events, `probe_ticks`) and leaves the
    // kernel time per element of its route -- per variant and selection mode -- and the link's rate each way here; the next call of that route
    // is planned with them.  0 = not measured yet: the first call plans with the KT_* guesses (x KT_CT_GUESS in constant-time mode) and 48 GB/s.
    double plan_kt[PR_COUNT][2][2] = {};
    double plan_link_in = 0, plan_link_out = 0;     // bytes per nanosecond
    hipEvent_t probe_ticks[6] = {};
    bool fused_io = true;          // FOURQ_FUSED_IO=0 (test hook): the affine / encoded flavours of MUL_* always through lift + full R1 rows, as round 5
    int plan_measure = 1;          // FOURQ_PIPE_MEASURE=0 (test hook): plan with the compiled-in guesses only, as round 5 did
    std::vector<float> chunk_stamps;   // under host_timing: six stamps per chunk of the last call, ms since its first event (fourq_ctx_host_chunk_stamps)
    char* pipe_dev = nullptr;      size_t pipe_dev_bytes = 0;
    char* pipe_pin = nullptr;      size_t pipe_pin_bytes = 0;
    u64* diag_stamps = nullptr;    // fourq_diag_clock: 2 x 16 stamps, allocated at its first call
    hipEvent_t diag_mark = nullptr; // fourq_diag_clock: the end of the stream's backlog at the time of the call
    u64* diag_bracket = nullptr;   // fourq_diag_clock_begin / _stop: 2 x DIAG_STAMP_BLOCKS x {CU key, memtime, memrealtime}
    bool diag_open = false;        // the first stamp launch of a bracket has been enqueued
    bool diag_stopped = false;     // ... and the second
    char* zero_copy = nullptr;     // 64 KiB of pinned host memory the kernels of a TINY host call read and write directly (no copy engine)
    fourq_host_stats host_stats = {};
    bool host_bounce = true;       // FOURQ_HOST_BOUNCE=0: hand pageable arrays to hipMemcpyAsync directly (measurement knob)
    bool host_zero_copy = true;    // FOURQ_HOST_ZERO_COPY=0: tiny host calls through hipMemcpyAsync like the others (measurement knob)
    char err[256] = { 0 };
    mutable std::recursive_mutex mu;   // CtxGuard: calls on one context take turns
};

namespace {

int fail(fourq_ctx* c, hipError_t e, const char* what) {
    if (c) snprintf(c->err, sizeof c->err, "%s: %s", what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? FOURQ_ERR_NOMEM : FOURQ_ERR_HIP;
}
#define HIP_TRY(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail((c), e_, #call); } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; (void)hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// What every entry point holds for its duration: the context's lock, then the context's device.  The reference's functions are
// pure (curve4q.py), so a drop-in caller may well call them from several threads at once -- fourq_amd.curve4q does so on ONE
// process-wide context -- while a context is one stream, one set of scratch slots and one set of pipeline buffers.  Calls on the
// same context therefore take turns (host-array calls for their whole duration, _dev calls for their enqueue); contexts are
// independent of each other.  Recursive, because host-array entry points are built from the _dev ones.
struct CtxGuard {
    std::unique_lock<std::recursive_mutex> lock;
    DeviceGuard dev;
    explicit CtxGuard(const fourq_ctx* c) : lock(c->mu), dev(c->device) {}
};

// device arrays are accessed as 16-byte vectors: every array pointer of the _dev API must be 16-byte aligned
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- the buffers that grow on demand, and who may grow them (the rule: work_layout.h).  A user that fq_work::Hold does not admit would free the buffer
// under its caller's values and return FOURQ_OK with wrong bytes: refused like a staging under capture (staging_allowed).  Only a wrong layout header leads here.
int refuse_held(fourq_ctx* c, const char* what, const char* who, size_t need, const fq_work::Hold& hold) {
    snprintf(c->err, sizeof c->err, "%s: %s needs %zu, but %s is using it and admits %zu of the %zu it holds (a layout header is wrong)", what, who, need, hold.who,
             hold.extent, hold.held);
    return FOURQ_ERR_HIP;
}
// Grow by free + allocate once the stream has run dry; a buffer somebody holds stays where it is.  *have and want count units of `unit` bytes.
template <class T> int grow(fourq_ctx* c, T** buf, size_t* have, size_t want, const char* what = nullptr, const fq_work::Hold* hold = nullptr, size_t unit = 1, bool pinned = false) {
    if (want <= *have) return FOURQ_OK;
    if (hold && hold->depth) return refuse_held(c, what, "a call made meanwhile", want, *hold);
    if (*buf) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, pinned ? hipHostFree(*buf) : hipFree(*buf));
        *buf = nullptr; *have = 0;
    }
    void* p = nullptr;
    HIP_TRY(c, pinned ? hipHostMalloc(&p, want * unit, hipHostMallocDefault) : hipMalloc(&p, want * unit));
    *buf = (T*)p; *have = want;
    return FOURQ_OK;
}
// The staging buffer and the planes (in rows) grow when the request exceeds them, to a quarter more; the work buffer when a quarter more does, to that.
int ensure_stage(fourq_ctx* c, size_t bytes) { return bytes <= c->stage_bytes ? FOURQ_OK : grow(c, &c->stage, &c->stage_bytes, bytes + bytes / 4, "the staging buffer", &c->stage_hold); }
int ensure_proj(fourq_ctx* c, size_t n) {
    return n <= c->proj_capacity ? FOURQ_OK : grow(c, &c->proj, &c->proj_capacity, n + n / 4, "the projective planes", &c->proj_hold, PROJ_PLANES * sizeof(uint4));
}
int ensure_work(fourq_ctx* c, size_t bytes) { return grow(c, &c->work, &c->work_bytes, bytes + bytes / 4, "the work buffer", &c->work_hold); }
// What a layout's call sizes: the work buffer, and the planes as the layout says.  PLANES_BY_DH: the _dev call leaves them to dh_dev, while its
// host twin and the *_reserve calls, which must leave nothing to allocate in mid-pipeline or under a capture, size both (reserve_for: a PipeReserve).
template <class L, class... A> int size_for(fourq_ctx* c, bool dev_call, A... a) {
    if (L::planes == fq_work::PLANES_SIZED || (L::planes == fq_work::PLANES_BY_DH && !dev_call)) if (int rc = ensure_proj(c, L::plane_rows(a...))) return rc;
    return ensure_work(c, L::bytes(a...));
}
template <class L> int reserve_for(fourq_ctx* c, size_t big) { return size_for<L>(c, false, big); }
// The one place that sizes the work buffer for a _dev call and carves it: WORK_SCOPE(w, Vrf, n); then w->h32.  The outermost scope on a context may
// move the buffers; a scope opened inside it -- a call made by a call -- must fit what its parent admits, or the call is refused.  A scope that sized
// the planes holds them too.  bucket_dev hands over to msm_dev before it opens a scope; dh_dev, mul_dev and the comb have no layout and keep no book.
template <class L> struct WorkScope {
    fourq_ctx* c;
    const char* name;
    fq_work::Hold work_parent, proj_parent;
    std::optional<L> carving;
    ~WorkScope() { if (carving) { c->work_hold = work_parent; if (L::planes == fq_work::PLANES_SIZED) c->proj_hold = proj_parent; } }
    template <class... A> int open(A... a) {
        const fq_work::Hold& held = c->work_hold;
        const size_t need = L::bytes(a...) - L::lent(a...);
        if (!held.admits(need)) return refuse_held(c, "the work buffer", name, need, held);
        if (held.depth == 0) { if (int rc = size_for<L>(c, true, a...)) return rc; }
        else if (L::planes == fq_work::PLANES_SIZED) { if (int rc = ensure_proj(c, L::plane_rows(a...))) return rc; }
        work_parent = held; proj_parent = c->proj_hold;
        c->work_hold = work_parent.opened(name, c->work_bytes, L::inner_extent(a...));
        if (L::planes == fq_work::PLANES_SIZED) c->proj_hold = proj_parent.opened(name, c->proj_capacity, c->proj_capacity);
        carving.emplace(c->work, a...);
        return FOURQ_OK;
    }
    const L* operator->() const { return &*carving; }
    const L& operator*() const { return *carving; }
};
#define WORK_SCOPE(w, Layout, ...) WorkScope<fq_work::Layout> w{ c, #Layout }; if (int rc_ = w.open(__VA_ARGS__)) return rc_

#define HIPRC_TRY(c, expr) do { hipError_t e_ = (hipError_t)(expr); if (e_ != hipSuccess) return fail((c), e_, #expr); } while (0)

template <int ALGO, int SRC, bool DH> int launch_ladder(fourq_ctx* c, LadderArgs a) {
    if (a.n == 0) return FOURQ_OK;
    size_t blocks_needed = ((size_t)a.n + BLOCK - 1) / BLOCK;
    size_t blocks_max = (SRC == FUSED ? c->lanes : c->lanes_w4) / BLOCK;
    unsigned grid = (unsigned)(blocks_needed < blocks_max ? blocks_needed : blocks_max);
    a.scratch = c->scratch;
    a.table = c->table_limbs;
    if (c->ct) {                            // constant-time selection: fourq_ct_fused.hip / fourq_ct_chain.hip
        HIPRC_TRY(c, SRC == FUSED ? ct_launch_fused(ALGO, DH, grid, c->stream, a) : ct_launch_lds(ALGO, DH, grid, c->stream, a));
    } else if (SRC == FUSED) {              // this translation unit's code object (FQ_CHAIN=0)
        hipLaunchKernelGGL((ladder_kernel<ALGO, FUSED, DH>), dim3(grid), dim3(BLOCK), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
    } else {                                // fourq_chain.hip's (FQ_CHAIN=1)
        HIPRC_TRY(c, chain_launch_ladder(ALGO, DH, grid, c->stream, a));
    }
    return FOURQ_OK;
}
// The variable-base kernels with two lanes per element (pair.hip.h): 0.66 of the one-lane kernels' latency for at most half a
// generation of elements.  A batch that small runs on them alone; a batch of q generations + r elements, 0 < r <= pair_max, on the
// fused route runs q fused generations and then the r elements two lanes each, so the element past a generation costs half a
// generation instead of a whole one.  Both selection modes.
// At most quad_max (a QUARTER generation) elements: FOUR lanes per element -- the element's two pairs take every other product of a
// formula level in the ladder steps -- 0.73 of the two-lane latency again (profiles/r03_quadlane.txt).
// The grid of n elements on the two- / four-lane kernels.  *quad: at most a quarter generation, four lanes per element, the ladder steps' products
// shared between two pairs.  The ladders walk their elements with one block per CU at the most; the comb's kernels take every block.
unsigned pair_grid(const fourq_ctx* c, size_t n, bool one_block_per_cu, bool* quad) {
    *quad = n <= c->quad_max;
    const size_t per_block = BLOCK / (*quad ? 4 : 2);
    const size_t blocks = (n + per_block - 1) / per_block;
    return (unsigned)(one_block_per_cu && blocks > (size_t)c->cus ? (size_t)c->cus : blocks);
}
// FIXED: the staged fixed-base table (c->table_limbs) instead of a table built per element.
template <int ALGO, bool DH, bool FIXED = false> int launch_pair(fourq_ctx* c, LadderArgs a) {
    if (a.n == 0) return FOURQ_OK;
    bool quad;
    const unsigned grid = pair_grid(c, a.n, true, &quad);
    a.table = c->table_limbs;
    if (c->ct) {                            // fourq_ct_fused.hip: the same kernels with the lane's table scanned at every step
        HIPRC_TRY(c, ct_launch_pair(ALGO, DH, FIXED, quad, grid, c->stream, a));
        return FOURQ_OK;
    }
    if (quad) hipLaunchKernelGGL((pair_kernel<ALGO, DH, false, FIXED, 4>), dim3(grid), dim3(BLOCK), 0, c->stream, a);
    else hipLaunchKernelGGL((pair_kernel<ALGO, DH, false, FIXED>), dim3(grid), dim3(BLOCK), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
// A mixed batch of at most half a generation: the same kernels with the table chosen per element (kernels.hip.h, pair_kernel<..., MIXED>)
int launch_pair_mixed(fourq_ctx* c, LadderArgs a) {
    bool quad;
    const unsigned grid = pair_grid(c, a.n, true, &quad);
    a.table = c->table_limbs;
    if (c->ct) {
        HIPRC_TRY(c, ct_launch_pair_mixed(quad, grid, c->stream, a));
        return FOURQ_OK;
    }
    if (quad) hipLaunchKernelGGL((pair_kernel<ENDO, false, false, false, 4, true>), dim3(grid), dim3(BLOCK), 0, c->stream, a);
    else hipLaunchKernelGGL((pair_kernel<ENDO, false, false, false, 2, true>), dim3(grid), dim3(BLOCK), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
// fixed-base batches of at most half a generation: the same two-lanes-per-element kernels on the caller's table (the LDS ladders
// of fourq_chain.hip take over above that: one lane per element, up to four waves per SIMD)
bool fixed_takes_pair(const fourq_ctx* c, size_t n) { return c->pair_max && n <= c->pair_max; }
// The route of a variable-base batch.  PAIR_TAIL: whole fused generations, then the remainder two lanes per element (also a batch
// that is nothing but such a remainder).
enum Route { ROUTE_FUSED, ROUTE_PAIR_TAIL };
Route variable_route(const fourq_ctx* c, size_t n, bool indexed) {
    const size_t tail = n % c->lanes;
    return !indexed && c->pair_max && tail != 0 && tail <= c->pair_max ? ROUTE_PAIR_TAIL : ROUTE_FUSED;
}
template <int ALGO, bool DH> int launch_variable(fourq_ctx* c, LadderArgs a) {
    if (variable_route(c, a.n, a.index != nullptr) == ROUTE_FUSED) return launch_ladder<ALGO, FUSED, DH>(c, a);
    const u32 tail = (u32)(a.n % c->lanes);
    LadderArgs whole = a, rest = a;
    whole.n = a.n - tail;
    rest.base = a.base + whole.n; rest.n = tail;
    int rc = whole.n ? launch_ladder<ALGO, FUSED, DH>(c, whole) : FOURQ_OK;
    return rc ? rc : launch_pair<ALGO, DH>(c, rest);
}

// Mixed rounds run on the persistent work-queue kernel (BASELINE config 5's mechanism; profiles/r04_mixed_queue.txt), except that in
// constant-time mode a round larger than one generation takes the fused kernel + mixed_ct_tail_kernel, which is as fast there (0.800 ms both).
bool mixed_queue_default(const fourq_ctx* c, size_t round) { return !c->ct || round <= c->lanes; }

// DH outputs are affine: from two resident generations of lanes upwards each lane meets several elements, and
// the inversions of K of them are merged into one (normalize_kernel).  Returns K (0: invert per element).
int normalize_group(const fourq_ctx* c, size_t n) {
    if (c->norm_k >= 0) return n >= (size_t)c->norm_k ? c->norm_k : 0;
    for (int k = 8; k >= 2; k >>= 1) if (n >= (size_t)k * c->lanes) return k;
    return 0;
}

// The working-limb copy of the caller's fixed-base table stays staged between calls: a call with the same 1 KiB
// (compared on the host) skips the copy and the unpack launch.
// The uploads read the context's shadow copies asynchronously.  HIP stages a copy from pageable memory before hipMemcpyAsync
// returns, but the API does not promise it: the event makes "the previous upload has read its shadow" explicit before a shadow
// is overwritten (only when the caller's table changes, i.e. never in a steady-state or captured sequence).
int shadow_free(fourq_ctx* c) {
    HIP_TRY(c, hipEventSynchronize(c->shadow_read));
    return FOURQ_OK;
}
// A table must be staged OUTSIDE a stream capture: the upload would be captured reading the context's mutable shadow at
// replay time, and shadow_read would become a captured event that no later hipEventSynchronize accepts.  A call that finds
// its table staged captures fine (it enqueues kernels only); one that would have to stage is refused with a message.
int staging_allowed(fourq_ctx* c) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (c->stream && hipStreamIsCapturing(c->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone) {
        snprintf(c->err, sizeof c->err, "a table would have to be staged while the stream is being captured: stage it before "
                 "the capture (one call with the same table, or fourq_comb_stage), then capture");
        return FOURQ_ERR_HIP;                                 // what the runtime itself would answer (hipErrorStreamCaptureUnsupported), with the reason
    }
    return FOURQ_OK;
}
int stage_table(fourq_ctx* c, const uint64_t* table_host) {
    if (c->table_staged && memcmp(c->table_shadow, table_host, sizeof c->table_shadow) == 0) return FOURQ_OK;
    if (int rc = staging_allowed(c)) return rc;
    c->table_staged = false;
    if (int rc = shadow_free(c)) return rc;
    memcpy(c->table_shadow, table_host, sizeof c->table_shadow);
    HIP_TRY(c, hipMemcpyAsync(c->table_packed, c->table_shadow, FOURQ_TABLE_WORDS * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(c->shadow_read, c->stream));
    hipLaunchKernelGGL(table_unpack_kernel, dim3(1), dim3(64), 0, c->stream, c->table_packed, c->table_limbs);
    HIP_TRY(c, hipGetLastError());
    c->table_staged = true;
    return FOURQ_OK;
}

int mul_dev(fourq_ctx* c, int algo, const uint64_t* scalars, const uint64_t* points, const uint64_t* table, uint64_t* out,
            const u32* index, size_t n, u32 io = 0) {
    if (!c || !scalars || !out || (!points && !table) || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(scalars) || !aligned16(out) || !aligned16(points)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    LadderArgs a = {};
    a.scalars = scalars; a.points = points; a.out = out; a.index = index; a.n = (u32)n;
    if (io) {                                       // only the fused one-lane kernels read LadderArgs::io: the caller has checked the route (fused_io)
        if (!points || index || variable_route(c, n, false) != ROUTE_FUSED) return FOURQ_ERR_INVALID;
        a.io = io;
    }
    if (points) return algo == ENDO ? launch_variable<ENDO, false>(c, a) : launch_variable<WINDOWED, false>(c, a);
    int rc = stage_table(c, table);
    if (rc) return rc;
    if (!index && fixed_takes_pair(c, n)) return algo == ENDO ? launch_pair<ENDO, false, true>(c, a) : launch_pair<WINDOWED, false, true>(c, a);
    return algo == ENDO ? launch_ladder<ENDO, LDS, false>(c, a) : launch_ladder<WINDOWED, LDS, false>(c, a);
}

int dh_dev(fourq_ctx* c, int algo, const uint64_t* scalars, const uint64_t* points, const uint64_t* table, uint64_t* out,
           uint8_t* status, size_t n) {
    if (!c || !scalars || !points || !out || !status || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(scalars) || !aligned16(points) || !aligned16(out)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    LadderArgs a = {};
    a.scalars = scalars; a.points = points; a.out = out; a.status = status; a.n = (u32)n;
    if (table && fixed_takes_pair(c, n)) {         // small fixed-base DH batches: two lanes per element, inversion in the kernel
        int rc = stage_table(c, table);
        if (rc) return rc;
        return algo == ENDO ? launch_pair<ENDO, true, true>(c, a) : launch_pair<WINDOWED, true, true>(c, a);
    }
    int group = normalize_group(c, n);
    // variable base: the fused kernels defer from two generations on (K = 2, 4, 8), except with a two-lane tail, whose kernels invert in place
    if (!table && variable_route(c, n, false) != ROUTE_FUSED) group = 0;
    int rc = group ? ensure_proj(c, n) : FOURQ_OK;
    if (rc) return rc;
    a.proj = group ? c->proj : nullptr;
    a.proj_stride = (u32)c->proj_capacity;
    if (!table) {
        rc = algo == ENDO ? launch_variable<ENDO, true>(c, a) : launch_variable<WINDOWED, true>(c, a);
    } else {
        rc = stage_table(c, table);
        if (rc) return rc;
        rc = algo == ENDO ? launch_ladder<ENDO, LDS, true>(c, a) : launch_ladder<WINDOWED, LDS, true>(c, a);
    }
    if (rc || !group) return rc;
    HIPRC_TRY(c, chain_launch_normalize(group, c->stream, c->proj, (u32)c->proj_capacity, out, status, (u32)n));
    return FOURQ_OK;
}

// ---- host-pointer batches ---------------------------------------------------------------------------------
// The caller's arrays are cut into chunks of whole kernel generations; chunk k uses slot k mod pipe_slots and goes
// H2D copy (stream copy_in) -> kernels (the context's stream) -> D2H copy (stream copy_out), the three stages of
// consecutive chunks overlapping.  Arrays in pinned host memory (fourq_host_alloc, hipHostMalloc, torch pin_memory)
// are copied by DMA straight from / to the caller's buffer; pageable arrays go through pinned bounce slots filled
// and drained by a few host threads (a single memcpy stream would be slower than the link).
//
// Round 5.  What a call costs beyond its kernels is (a) the first chunk's copy in and the last chunk's copy out, which
// nothing can overlap, and (b) whatever keeps the kernel stream waiting between chunks.  So: the FIRST and the LAST chunk are one generation
// (the smallest unit that fills the chip), the chunks in between `pipe_gens` generations (fewer stream hops per element); a slot is handed
// on ON THE GPU -- the copy-in stream waits for the event behind the slot's previous copy-out -- so the host enqueues every chunk without
// ever blocking and the queues never run dry because the host was asleep in hipEventSynchronize; and the six timing events per chunk
// are recorded only when the caller asked for copy durations (fourq_ctx_set_host_timing).  Pageable callers keep the host-side hand-over:
// their bounce slots are filled and drained by the host anyway.
constexpr int PIPE_MAX_ARRAYS = 4;
struct PipeArray {
    const char* src;     // input array (host) or NULL
    char* dst;           // output array (host) or NULL
    size_t stride;       // bytes per element
};
using fq_work::align256;

bool is_pinned(const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeHost;
}
void host_copy(char* dst, const char* src, size_t bytes) {
    constexpr size_t SLICE = 2u << 20;
    unsigned hw = std::thread::hardware_concurrency();
    size_t threads = bytes / SLICE;
    if (threads > 6) threads = 6;
    if (hw && threads > hw) threads = hw;
    if (threads <= 1) { memcpy(dst, src, bytes); return; }
    std::vector<std::thread> pool;
    const size_t per = (bytes / threads + 63) & ~(size_t)63;
    size_t done_to = per;                      // [0, per) is this thread's slice; helpers take the rest
    try {
        pool.reserve(threads - 1);
        for (size_t t = 1; t < threads; t++) {
            const size_t lo = t * per, hi = (t + 1 == threads) ? bytes : (t + 1) * per;
            pool.emplace_back([=] { memcpy(dst + lo, src + lo, hi - lo); });
            done_to = hi;
        }
    } catch (...) {                            // no more threads to be had: nothing may cross the C ABI; copy the remainder here
        done_to = pool.empty() ? per : done_to;
    }
    memcpy(dst, src, per);
    for (auto& th : pool) th.join();
    if (done_to < bytes) memcpy(dst + done_to, src + done_to, bytes - done_to);
}

int ensure_ticks(fourq_ctx* c, size_t count) {
    while (c->ticks.size() < count) {
        hipEvent_t e;
        HIP_TRY(c, hipEventCreate(&e));
        try { c->ticks.push_back(e); } catch (...) { (void)hipEventDestroy(e); return FOURQ_ERR_NOMEM; }
    }
    return FOURQ_OK;
}

using ChunkLaunch = std::function<int(char* const* in_dev, char* const* out_dev, size_t m)>;

// Which call this is (PipeRouteId and its variant, 0 or 1), and the guess of its kernel time per element for the context's first call of it
struct PipeRoute { int id, variant; double kt_guess; };
// Kernel time per element of each route in nanoseconds, device-resident at 2^20 elements (profiles/r04_perf_probe.txt, tools/perf_probe.py).
// They only size the chunks of the host-array calls (pipeline_plan.h): a kernel slower than its figure (constant-time mode, a slower box)
// gets chunks smaller than it could have had, one faster by more than the plan's 15 % margin a short stall on the first chunks.
constexpr double KT_ENDO_VAR = 4.63, KT_WIN_VAR = 8.18, KT_DH_VAR = 4.90, KT_ENDO_FIXED = 3.58, KT_WIN_FIXED = 7.65, KT_DH_FIXED = 3.65, KT_COMB = 1.09,
                 KT_LIFT_LOWER = 0.10, KT_CODEC = 0.30, KT_DECODE = 0.25, KT_ENCODE = 0.05;
constexpr double KT_DOUBLE = KT_COMB + KT_ENDO_VAR + KT_LIFT_LOWER;
// ... and first-call guesses without a measurement behind them: one 128-byte block of SHA-512 per element (~5 000 VALU instructions); one
// Elligator map (four GF(p) exponentiations' worth); one inversion modulo N (a Fermat chain is about 1.2 ladders' worth of instructions,
// shared by 8 elements)
constexpr double KT_SHA_BLOCK = 0.05, KT_ELL2 = 0.20, KT_SCINV = 0.70;
constexpr double KT_CT_GUESS = 1.3;                 // constant-time selection: x 1.07 - 1.5 by route until the context has measured it
using PipeReserve = int (*)(fourq_ctx* c, size_t big);  // sizes the context's intermediates for the largest chunk BEFORE the first chunk is enqueued
int run_pipeline_inner(fourq_ctx* c, const PipeArray* in, int n_in, const PipeArray* out, int n_out, size_t n, size_t chunk, PipeRoute route, const ChunkLaunch& launch, size_t chunk_bounce, PipeReserve reserve);
// `chunk`: elements of one kernel generation of the route the call takes; `ns_per_elem`: that route's kernel time per element (the
// KT_* constants above: what sizes the chunks is the ratio of kernel time to copy time, pipeline_plan.h).  `chunk_bounce` (0 = `chunk`):
// the uniform chunk of a call from PAGEABLE arrays -- its pace is the host's bounce copies (and, where the call allocates its result, the
// page faults of 160 fresh bytes per element), not the link: such calls keep the chunk shape they were measured with in rounds 2-4
// (cfg3's call, result array reused: 10.3-10.4 ms at 2^20 then and now; profiles/r02_host_api.txt, profiles/r05_pipeline.txt).
int run_pipeline(fourq_ctx* c, const PipeArray* in, int n_in, const PipeArray* out, int n_out, size_t n, size_t chunk, PipeRoute route, const ChunkLaunch& launch,
                 size_t chunk_bounce = 0, PipeReserve reserve = nullptr) {
    const int rc = run_pipeline_inner(c, in, n_in, out, n_out, n, chunk, route, launch, chunk_bounce, reserve);
    if (rc != FOURQ_OK) {                      // a chunk failed half way: nothing of this call may still be in flight when the caller
        (void)hipStreamSynchronize(c->copy_in);    // gets its buffers (and the context its slots) back
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->copy_out);
    }
    return rc;
}
// One host-array call as its three paths below see it.  pin_in / pin_out: the array is copied "directly", hipMemcpyAsync on the caller's
// array -- pinned arrays always; pageable ones when the batch is a single chunk (nothing to overlap with, and the runtime's own staging of
// a pageable copy beats a bounce pass: 0.92 vs 1.29 ms at 2^16 variable-base elements), through the bounce slots otherwise (8.5 vs 13.9 ms at 2^20).
struct PipeCall {
    fourq_ctx* c;
    const PipeArray* in; int n_in;
    const PipeArray* out; int n_out;
    size_t n;
    const ChunkLaunch& launch;
    bool pin_in[PIPE_MAX_ARRAYS], pin_out[PIPE_MAX_ARRAYS], bounce;
};
// A slot holds the arrays of one chunk of m elements, inputs then outputs, each on a 256-byte boundary
struct SlotLayout { size_t off_in[PIPE_MAX_ARRAYS], off_out[PIPE_MAX_ARRAYS], bytes; };
SlotLayout slot_layout(const PipeCall& p, size_t m) {
    SlotLayout s = {};
    for (int i = 0; i < p.n_in; i++) { s.off_in[i] = s.bytes; s.bytes += align256(m * p.in[i].stride); }
    for (int i = 0; i < p.n_out; i++) { s.off_out[i] = s.bytes; s.bytes += align256(m * p.out[i].stride); }
    return s;
}
// Tiny calls (the batch of one above all): the arrays fit 64 KiB of pinned host memory that the kernels read and write in
// place -- two CPU memcpys of a few hundred bytes instead of three trips through the copy engine (profiles/r03_single_call.txt).
constexpr size_t ZERO_COPY_BYTES = 64u << 10;
int pipe_zero_copy(const PipeCall& p, const SlotLayout& s, const fourq_host_stats& st) {
    fourq_ctx* c = p.c;
    if (!c->zero_copy) HIP_TRY(c, hipHostMalloc((void**)&c->zero_copy, ZERO_COPY_BYTES, hipHostMallocDefault));
    char *din[PIPE_MAX_ARRAYS], *dout[PIPE_MAX_ARRAYS];
    for (int i = 0; i < p.n_in; i++) {
        din[i] = c->zero_copy + s.off_in[i];
        memcpy(din[i], p.in[i].src, p.n * p.in[i].stride);            // a CPU copy: no h2d / d2h bytes or times are reported for it
    }
    for (int i = 0; i < p.n_out; i++) dout[i] = c->zero_copy + s.off_out[i];
    if (int rc = p.launch(din, dout, p.n)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < p.n_out; i++) memcpy(p.out[i].dst, dout[i], p.n * p.out[i].stride);
    c->host_stats = st;
    return FOURQ_OK;
}
// A single chunk (down to the reference-shaped call, a batch of one): copies and kernels in order on the context's own stream.
// Nothing can overlap, so the three-stream choreography below would only add its cross-stream event hops (50 us) to the call.
// The four timing events around the copies are recorded only under fourq_ctx_set_host_timing; otherwise copy durations read 0.
int pipe_single_chunk(const PipeCall& p, const SlotLayout& s, fourq_host_stats st) {
    fourq_ctx* c = p.c;
    const size_t n = p.n;
    int rc = grow(c, &c->pipe_dev, &c->pipe_dev_bytes, s.bytes);
    if (rc) return rc;
    const bool timed = c->host_timing;
    if (timed && (rc = ensure_ticks(c, 4))) return rc;
    char *din[PIPE_MAX_ARRAYS], *dout[PIPE_MAX_ARRAYS];
    if (timed) HIP_TRY(c, hipEventRecord(c->ticks[0], c->stream));
    for (int i = 0; i < p.n_in; i++) {
        din[i] = c->pipe_dev + s.off_in[i];
        HIP_TRY(c, hipMemcpyAsync(din[i], p.in[i].src, n * p.in[i].stride, hipMemcpyHostToDevice, c->stream));
        st.h2d_bytes += n * p.in[i].stride;
    }
    if (timed) HIP_TRY(c, hipEventRecord(c->ticks[1], c->stream));
    for (int i = 0; i < p.n_out; i++) dout[i] = c->pipe_dev + s.off_out[i];
    if ((rc = p.launch(din, dout, n))) return rc;
    if (timed) HIP_TRY(c, hipEventRecord(c->ticks[2], c->stream));
    for (int i = 0; i < p.n_out; i++) {
        HIP_TRY(c, hipMemcpyAsync(p.out[i].dst, dout[i], n * p.out[i].stride, hipMemcpyDeviceToHost, c->stream));
        st.d2h_bytes += n * p.out[i].stride;
    }
    if (timed) HIP_TRY(c, hipEventRecord(c->ticks[3], c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (timed) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ticks[0], c->ticks[1]));
        st.h2d_ms = ms;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ticks[2], c->ticks[3]));
        st.d2h_ms = ms;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ticks[1], c->ticks[2]));
        st.kernels_ms = st.kernels_span_ms = ms;
    }
    c->host_stats = st;
    return FOURQ_OK;
}
// What a plan is priced with: this context's own measurements of this route in this selection mode, or the first call's guesses
fq_plan::Rates plan_rates(const fourq_ctx* c, PipeRoute route, fourq_host_stats* st) {
    const int mode = c->ct ? 1 : 0;
    fq_plan::Rates rates;
    const bool measured = c->plan_measure && c->plan_kt[route.id][route.variant][mode] > 0;
    rates.ns_per_elem = measured ? c->plan_kt[route.id][route.variant][mode] : route.kt_guess * (c->ct ? KT_CT_GUESS : 1.0);
    rates.link_in = c->plan_measure && c->plan_link_in > 0 ? c->plan_link_in : fq_plan::LINK_BYTES_PER_NS;
    rates.link_out = c->plan_measure && c->plan_link_out > 0 ? c->plan_link_out : fq_plan::LINK_BYTES_PER_NS;
    st->planned_kernel_ns_per_elem = rates.ns_per_elem; st->planned_link_in_gbs = rates.link_in; st->planned_link_out_gbs = rates.link_out;
    st->planned_from_measurement = measured ? 1 : 0;
    return rates;
}
// What the next call of this route will be planned with, from the probed chunk of m elements.  The link's rates only from a chunk that had
// neighbours on both sides (a call of one or two chunks copies with the link to itself), and only from a chunk copied directly (a bounce
// slot's copy is paced by the host threads that fill it): `link`.
int read_probe(fourq_ctx* c, PipeRoute route, double m, bool link, size_t bytes_in, size_t bytes_out, fourq_host_stats* st) {
    const int mode = c->ct ? 1 : 0;
    float t_in = 0, t_k = 0, t_out = 0;
    HIP_TRY(c, hipEventElapsedTime(&t_in, c->probe_ticks[0], c->probe_ticks[1]));
    HIP_TRY(c, hipEventElapsedTime(&t_k, c->probe_ticks[2], c->probe_ticks[3]));
    HIP_TRY(c, hipEventElapsedTime(&t_out, c->probe_ticks[4], c->probe_ticks[5]));
    if (t_k > 0) c->plan_kt[route.id][route.variant][mode] = (double)t_k * 1e6 / m;
    if (link) {
        if (t_in > 0 && bytes_in) c->plan_link_in = m * (double)bytes_in / ((double)t_in * 1e6);
        if (t_out > 0 && bytes_out) c->plan_link_out = m * (double)bytes_out / ((double)t_out * 1e6);
    }
    st->measured_kernel_ns_per_elem = c->plan_kt[route.id][route.variant][mode];
    return FOURQ_OK;
}
// Timing (on request): six events per chunk -- around its copy in, its kernels, its copy out -- for the first TIMED_MAX chunks; a call of
// more chunks reports their copy durations scaled to the call's bytes (a 2^28-element call has 4 096 chunks: it does not get 24 576 events)
constexpr size_t TIMED_MAX = 256, TK = 6;
int read_chunk_timing(fourq_ctx* c, size_t timed_pieces, uint64_t timed_h2d, uint64_t timed_d2h, fourq_host_stats* st) {
    try {
        c->chunk_stamps.resize(TK * timed_pieces);
        for (size_t i = 0; i < TK * timed_pieces; i++) HIP_TRY(c, hipEventElapsedTime(&c->chunk_stamps[i], c->ticks[0], c->ticks[i]));
    } catch (...) { c->chunk_stamps.clear(); }
    for (size_t k = 0; k < timed_pieces; k++) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ticks[TK * k], c->ticks[TK * k + 1]));
        st->h2d_ms += ms;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ticks[TK * k + 2], c->ticks[TK * k + 3]));
        st->d2h_ms += ms;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ticks[TK * k + 4], c->ticks[TK * k + 5]));
        st->kernels_ms += ms;
    }
    float span = 0;
    HIP_TRY(c, hipEventElapsedTime(&span, c->ticks[4], c->ticks[TK * (timed_pieces - 1) + 5]));
    st->kernels_span_ms = span;
    if (timed_h2d && timed_h2d < st->h2d_bytes) st->h2d_ms *= (double)st->h2d_bytes / (double)timed_h2d;
    if (timed_d2h && timed_d2h < st->d2h_bytes) st->d2h_ms *= (double)st->d2h_bytes / (double)timed_d2h;
    return FOURQ_OK;
}
// Several chunks: chunk k uses slot k mod slots and goes copy in -> kernels -> copy out on three streams
int pipe_chunked(const PipeCall& p, size_t chunk, PipeRoute route, PipeReserve reserve, fourq_host_stats st) {
    fourq_ctx* c = p.c;
    const PipeArray *in = p.in, *out = p.out;
    const int n_in = p.n_in, n_out = p.n_out;
    const bool bounce = p.bounce;
    // The chunks of this call (pipeline_plan.h): one generation first and last, growing in between as far as the copies' lead allows
    size_t bytes_in = 0, bytes_out = 0;
    for (int i = 0; i < n_in; i++) bytes_in += in[i].stride;
    for (int i = 0; i < n_out; i++) bytes_out += out[i].stride;
    using fq_plan::Piece;
    std::vector<Piece> plan;
    const fq_plan::Rates rates = plan_rates(c, route, &st);
    try { plan = fq_plan::plan_pieces(p.n, chunk, bytes_in, bytes_out, rates, (bounce && !c->pipe_gens) ? 1 : c->pipe_gens); } catch (...) { return FOURQ_ERR_NOMEM; }
    const size_t pieces = plan.size();
    size_t big = 0;
    for (const Piece& pc : plan) if (pc.m > big) big = pc.m;
    // planned chunks grow within a call; the context's intermediates (work, proj) are sized ONCE for the largest, so that no
    // launch() inside the loop reaches grow() -- which would drain the kernel stream and block the host in mid-pipeline
    if (reserve) { if (int rrc = reserve(c, big)) return rrc; }
    const SlotLayout s = slot_layout(p, big);
    const size_t slot = s.bytes;
    st.chunks = (uint32_t)pieces;
    // who hands a slot on: the GPU when every array is copied directly, the host when it has bounce slots to fill and drain
    const bool host_wait = bounce || c->pipe_host_wait;
    // Slots in flight: four -- with the GPU's hand-over, and with the host's when it fills and drains bounce slots anyway (pageable callers:
    // raw R1 7.28 against 7.78 ms at 2^20 with three, the other formats unchanged, profiles/r06_pipeline.txt).  The host's hand-over on PINNED arrays
    // (FOURQ_PIPE_HOST_WAIT, a test hook) keeps three: with four or more the copy out of chunk slots + 2 -- the one the host is waiting for
    // with nothing left to enqueue -- makes almost no progress while the three chunks queued behind it run their kernels and completes only
    // once they are done (1.66 ms instead of 0.42; per-chunk stamps in the same file; a spinning hipEventQuery instead of the blocking wait
    // changes nothing), so the slot it frees comes 0.6 ms late.  The device copy out is a blit kernel on this runtime; handing slots on
    // ON THE GPU never leaves that queue without a successor, and does not show it.
    const int want_slots = c->pipe_slots ? c->pipe_slots : ((host_wait && !bounce) ? 3 : 4);
    const int slots = pieces < (size_t)want_slots ? (int)pieces : want_slots;
    int rc = grow(c, &c->pipe_dev, &c->pipe_dev_bytes, slot * slots);
    if (rc) return rc;
    if (bounce && (rc = grow(c, &c->pipe_pin, &c->pipe_pin_bytes, slot * slots, nullptr, nullptr, 1, true))) return rc;
    const size_t timed_pieces = c->host_timing ? (pieces < TIMED_MAX ? pieces : TIMED_MAX) : 0;
    if (timed_pieces && (rc = ensure_ticks(c, TK * timed_pieces))) return rc;
    uint64_t timed_h2d = 0, timed_d2h = 0;
    // the measured planner inputs: ONE chunk of whole generations from the middle of the call, where both directions of the link are busy
    const size_t whole_pieces = pieces - ((p.n % chunk) ? 1 : 0);
    const size_t probe = (c->plan_measure && whole_pieces >= 1) ? (whole_pieces >= 3 ? whole_pieces / 2 : 0) : (size_t)-1;
    if (probe != (size_t)-1)
        for (hipEvent_t& e : c->probe_ticks) if (!e) HIP_TRY(c, hipEventCreate(&e));
    auto drain = [&](size_t k) -> int {          // chunk k has left the device: hand a pageable caller its bytes
        const int b = (int)(k % slots);
        if (c->pipe_host_poll) {                 // FOURQ_PIPE_HOST_POLL=1 (experiment, profiles/r06_pipeline.txt): spin on hipEventQuery instead of blocking
            hipError_t q;
            while ((q = hipEventQuery(c->out_done[b])) == hipErrorNotReady) {}
            HIP_TRY(c, q);
        } else {
            HIP_TRY(c, hipEventSynchronize(c->out_done[b]));
        }
        for (int i = 0; i < n_out; i++)
            if (!p.pin_out[i]) host_copy(out[i].dst + plan[k].off * out[i].stride, c->pipe_pin + (size_t)b * slot + s.off_out[i], plan[k].m * out[i].stride);
        return FOURQ_OK;
    };
    for (size_t k = 0; k < pieces; k++) {
        const int b = (int)(k % slots);
        const size_t off = plan[k].off, m = plan[k].m;
        if (k >= (size_t)slots) {                                       // slot b is free again once chunk k - slots has been copied out of it
            if (host_wait) { if ((rc = drain(k - slots))) return rc; }
            else HIP_TRY(c, hipStreamWaitEvent(c->copy_in, c->out_done[b], 0));    // ... which the kernels of chunk k inherit through in_done[b]
        }
        char* dev = c->pipe_dev + (size_t)b * slot;
        char* pin = bounce ? c->pipe_pin + (size_t)b * slot : nullptr;
        char *din[PIPE_MAX_ARRAYS], *dout[PIPE_MAX_ARRAYS];
        for (int i = 0; i < n_in; i++) {
            din[i] = dev + s.off_in[i];
            if (!p.pin_in[i]) host_copy(pin + s.off_in[i], in[i].src + off * in[i].stride, m * in[i].stride);
        }
        const bool timed = k < timed_pieces, probed = k == probe;
        if (probed) HIP_TRY(c, hipEventRecord(c->probe_ticks[0], c->copy_in));
        if (timed) HIP_TRY(c, hipEventRecord(c->ticks[TK * k], c->copy_in));
        for (int i = 0; i < n_in; i++) {
            const char* src = p.pin_in[i] ? in[i].src + off * in[i].stride : pin + s.off_in[i];
            HIP_TRY(c, hipMemcpyAsync(din[i], src, m * in[i].stride, hipMemcpyHostToDevice, c->copy_in));
            st.h2d_bytes += m * in[i].stride;
            if (timed) timed_h2d += m * in[i].stride;
        }
        if (timed) HIP_TRY(c, hipEventRecord(c->ticks[TK * k + 1], c->copy_in));
        if (probed) HIP_TRY(c, hipEventRecord(c->probe_ticks[1], c->copy_in));
        HIP_TRY(c, hipEventRecord(c->in_done[b], c->copy_in));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->in_done[b], 0));
        if (timed) HIP_TRY(c, hipEventRecord(c->ticks[TK * k + 4], c->stream));      // the kernel stream is past its wait: the chunk's bytes are there
        if (probed) HIP_TRY(c, hipEventRecord(c->probe_ticks[2], c->stream));
        for (int i = 0; i < n_out; i++) dout[i] = dev + s.off_out[i];
        if ((rc = p.launch(din, dout, m))) return rc;
        if (probed) HIP_TRY(c, hipEventRecord(c->probe_ticks[3], c->stream));
        if (timed) HIP_TRY(c, hipEventRecord(c->ticks[TK * k + 5], c->stream));
        HIP_TRY(c, hipEventRecord(c->kernels_done[b], c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->copy_out, c->kernels_done[b], 0));
        if (probed) HIP_TRY(c, hipEventRecord(c->probe_ticks[4], c->copy_out));
        if (timed) HIP_TRY(c, hipEventRecord(c->ticks[TK * k + 2], c->copy_out));
        for (int i = 0; i < n_out; i++) {
            char* dst = p.pin_out[i] ? out[i].dst + off * out[i].stride : pin + s.off_out[i];
            HIP_TRY(c, hipMemcpyAsync(dst, dout[i], m * out[i].stride, hipMemcpyDeviceToHost, c->copy_out));
            st.d2h_bytes += m * out[i].stride;
            if (timed) timed_d2h += m * out[i].stride;
        }
        if (timed) HIP_TRY(c, hipEventRecord(c->ticks[TK * k + 3], c->copy_out));
        if (probed) HIP_TRY(c, hipEventRecord(c->probe_ticks[5], c->copy_out));
        HIP_TRY(c, hipEventRecord(c->out_done[b], c->copy_out));
    }
    if (host_wait) {
        for (size_t k = pieces > (size_t)slots ? pieces - slots : 0; k < pieces; k++)
            if ((rc = drain(k))) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->copy_out));      // in order behind every chunk's copy out, which is behind its kernels and its copy in
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (probe != (size_t)-1 && (rc = read_probe(c, route, (double)plan[probe].m, whole_pieces >= 3 && !bounce, bytes_in, bytes_out, &st))) return rc;
    try { c->chunk_stamps.clear(); } catch (...) {}
    if (timed_pieces && (rc = read_chunk_timing(c, timed_pieces, timed_h2d, timed_d2h, &st))) return rc;
    c->host_stats = st;
    return FOURQ_OK;
}
int run_pipeline_inner(fourq_ctx* c, const PipeArray* in, int n_in, const PipeArray* out, int n_out, size_t n, size_t chunk, PipeRoute route, const ChunkLaunch& launch, size_t chunk_bounce, PipeReserve reserve) {
    if (n_in > PIPE_MAX_ARRAYS || n_out > PIPE_MAX_ARRAYS || chunk == 0 || route.id < 0 || route.id >= PR_COUNT || (route.variant & ~1)) return FOURQ_ERR_INVALID;
    bool is_pin_in[PIPE_MAX_ARRAYS], is_pin_out[PIPE_MAX_ARRAYS], any_pageable = false;
    for (int i = 0; i < n_in; i++) { is_pin_in[i] = is_pinned(in[i].src); any_pageable |= !is_pin_in[i]; }
    for (int i = 0; i < n_out; i++) { is_pin_out[i] = is_pinned(out[i].dst); any_pageable |= !is_pin_out[i]; }
    const bool uniform = any_pageable && c->host_bounce && chunk_bounce > chunk && n > chunk_bounce;
    if (uniform) chunk = chunk_bounce;
    if (chunk > n) chunk = n;
    const size_t chunks = (n + chunk - 1) / chunk;
    const bool direct_pageable = !c->host_bounce || chunks == 1;
    PipeCall p = { c, in, n_in, out, n_out, n, launch, {}, {}, false };
    fourq_host_stats st = {};
    st.chunks = (uint32_t)chunks;
    st.pinned_in = st.pinned_out = 1;
    for (int i = 0; i < n_in; i++) { p.pin_in[i] = is_pin_in[i] || direct_pageable; p.bounce |= !p.pin_in[i]; st.pinned_in &= is_pin_in[i] ? 1 : 0; }
    for (int i = 0; i < n_out; i++) { p.pin_out[i] = is_pin_out[i] || direct_pageable; p.bounce |= !p.pin_out[i]; st.pinned_out &= is_pin_out[i] ? 1 : 0; }
    if (chunks > 1) return pipe_chunked(p, chunk, route, reserve, st);
    const SlotLayout s = slot_layout(p, chunk);
    return s.bytes <= ZERO_COPY_BYTES && c->host_zero_copy ? pipe_zero_copy(p, s, st) : pipe_single_chunk(p, s, st);
}

// ---- one host-array call, described once ------------------------------------------------------------------------------------------
// A call states its arrays as (pointer, bytes per element), its route and first-call guess, its chunk unit, what it reserves, and what to
// launch on one chunk; host_call owns the argument contract (include/fourq_amd.h), the lock and the pipeline.
// An input that is absent from the chunks: one of stride 0 (the message matrix of empty messages), and a NULL one that MAY_BE_NULL (lens).
constexpr bool MAY_BE_NULL = true;
struct HostIn { const void* p; size_t stride; bool may_be_null = false; };
struct HostOut { void* p; size_t stride; };
// The chunk units are functions of the context: host_call evaluates them once it has refused a NULL one.
using ChunkUnit = size_t (*)(const fourq_ctx*);
size_t pipe_chunk(const fourq_ctx* c) { return c->lanes; }              // variable base: whole generations of the fused kernels that will run it
size_t unit_w4(const fourq_ctx* c) { return c->lanes_w4; }              // one generation of the 128-VGPR kernels
// fixed base: the LDS ladders hold two waves per SIMD, so HALF of lanes_w4 is one generation of theirs -- the unit that sizes the first
// chunk's copy in and the last chunk's copy out (cfg3's call: 160 B out per element, 21 MB instead of 42 behind the last kernel)
size_t unit_w4_half(const fourq_ctx* c) { return c->lanes_w4 / 2; }
size_t unit_w4_x4(const fourq_ctx* c) { return 4 * c->lanes_w4; }       // the kernels that only stream: encode, SHA-512, hash to field
// one pass of the work-queue kernel's 4 x CUs waves over 64-element items is `lanes` elements: the unit that lets the copies of a
// config-5-sized call (2 x lanes) overlap its kernels; raw R1 in and out keeps the chunks at that size (pipeline_plan.h)
size_t unit_mixed(const fourq_ctx* c) { return c->mixed_round < c->lanes ? c->mixed_round : c->lanes; }
size_t unit_mixed_round(const fourq_ctx* c) { return c->mixed_round; }
size_t unit_scinv(const fourq_ctx* c) { return 16 * (size_t)c->cus * BLOCK; }
// chunk of a call that carries a message matrix: the route's own chunk, cut down (to no less than one block's worth of rows) where rows of
// `stride` bytes would make a pipeline slot larger than 64 MiB
size_t sig_chunk(size_t chunk, size_t stride) {
    const size_t cap = stride ? (size_t)(64u << 20) / stride : chunk;
    if (cap < chunk) chunk = cap < (size_t)BLOCK ? (size_t)BLOCK : cap;
    return chunk;
}
struct HostCall {
    HostIn in[PIPE_MAX_ARRAYS];
    HostOut out[PIPE_MAX_ARRAYS];
    PipeRoute route;
    ChunkUnit unit, unit_pageable;      // unit_pageable (or nullptr): run_pipeline's chunk_bounce
    PipeReserve reserve;                // reserve_for<the work layout of the _dev call>, ensure_proj, or nullptr
    bool ok = true;                     // the call's own predicates: a required pointer that is no array, sig_msgs_host_ok, h2c_args_ok
    size_t msg_stride = 0;              // the row of a message matrix: caps the chunk (sig_chunk)
};
// One chunk as the launch sees it: the arrays by their position in HostCall::in / ::out, nullptr for an absent input
struct Chunk {
    char* const* din; char* const* dout; const int* slot; size_t m;
    template <class T> const T* in(int i) const { return slot[i] < 0 ? nullptr : (const T*)din[slot[i]]; }
    template <class T> T* out(int i) const { return (T*)dout[i]; }
};
struct HostArrays { PipeArray in[PIPE_MAX_ARRAYS] = {}, out[PIPE_MAX_ARRAYS] = {}; int n_in = 0, n_out = 0, slot[PIPE_MAX_ARRAYS]; };
// The argument contract: FOURQ_ERR_INVALID for a NULL context, a NULL array that may not be, a failed predicate or n > FOURQ_MAX_BATCH
int host_arrays(const fourq_ctx* c, size_t n, const HostCall& d, HostArrays* a) {
    if (!c || !d.ok || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    for (int i = 0; i < PIPE_MAX_ARRAYS; i++) {
        const HostIn& x = d.in[i];
        const bool present = x.stride && (x.p || !x.may_be_null);
        if (present && !x.p) return FOURQ_ERR_INVALID;
        a->slot[i] = present ? a->n_in : -1;
        if (present) { a->in[a->n_in].src = (const char*)x.p; a->in[a->n_in++].stride = x.stride; }
    }
    for (; a->n_out < PIPE_MAX_ARRAYS && d.out[a->n_out].stride; a->n_out++) {
        if (!d.out[a->n_out].p) return FOURQ_ERR_INVALID;
        a->out[a->n_out].dst = (char*)d.out[a->n_out].p; a->out[a->n_out].stride = d.out[a->n_out].stride;
    }
    return FOURQ_OK;
}
// In this order: argument errors; n == 0 is FOURQ_OK with nothing touched; the lock; `prepare` once per call (stage_comb: the chunks
// then pass comb == NULL, "the staged one", and the table is compared once, not once per chunk); the chunks.
template <class Prepare, class Launch> int host_call(fourq_ctx* c, size_t n, const HostCall& d, Prepare&& prepare, Launch&& launch) {
    HostArrays a;
    if (int rc = host_arrays(c, n, d, &a)) return rc;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    if (int rc = prepare()) return rc;
    return run_pipeline(c, a.in, a.n_in, a.out, a.n_out, n, sig_chunk(d.unit(c), d.msg_stride), d.route,
                        [&](char* const* din, char* const* dout, size_t m) { return launch(Chunk{ din, dout, a.slot, m }); },
                        d.unit_pageable ? d.unit_pageable(c) : 0, d.reserve);
}
template <class Launch> int host_call(fourq_ctx* c, size_t n, const HostCall& d, Launch&& launch) {
    return host_call(c, n, d, [] { return FOURQ_OK; }, launch);
}

// ---- one grouped call, described once: one output row per GROUP of group_size elements (the grouped sums, the commitments, the proofs) ----
// The grouped argument contract (include/fourq_amd.h), spelt here only and in the order every grouped call and *_reserve observes: the
// call's own predicates first (`args_ok`: the context, NULL pointers, aligned16 for _dev, the window, the route, h2c_args_ok, ...), a failed
// one is FOURQ_ERR_INVALID whatever the counts are; then groups == 0 is FOURQ_OK with *n == 0 and nothing touched; then group_size == 0 or
// groups x group_size overflowing or above FOURQ_MAX_BATCH is FOURQ_ERR_INVALID.  Otherwise FOURQ_OK with *n = groups x group_size > 0.
// Callers write `if (rc || !n) return rc;`.
int grouped_rows(bool args_ok, size_t groups, size_t group_size, size_t* n) {
    *n = 0;
    if (!args_ok) return FOURQ_ERR_INVALID;
    if (groups == 0) return FOURQ_OK;
    size_t rows;
    if (group_size == 0 || __builtin_mul_overflow(groups, group_size, &rows) || rows > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    *n = rows;
    return FOURQ_OK;
}
// Host arrays of a grouped call: copy in through the staging buffer, the _dev call, copy out, synchronise, in one piece.  No chunk overlap:
// run_pipeline's arrays are per element, and these outputs are per group.  c->host_stats describes the last PIPELINE call and is not written.
// One array of a call: copied in where `in` is set (n rows with `per_row`, `groups` rows otherwise), copied out (`groups` rows) where `out`
// is; an array the call does not have (the status of the affine flavours) is not listed.  `call` gets the device arrays in listed order.
struct GroupedArray { const void* in; void* out; size_t row_bytes; bool per_row; };
constexpr size_t GROUPED_MAX_ARRAYS = 8;
int grouped_host(fourq_ctx* c, size_t n, size_t groups, const GroupedArray* arrays, size_t count, const std::function<int(char* const*)>& call) {
    if (count > GROUPED_MAX_ARRAYS) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    size_t total = 0;
    for (size_t k = 0; k < count; k++) total += (arrays[k].per_row ? n : groups) * arrays[k].row_bytes;
    if (int rc = ensure_stage(c, total)) return rc;
    // c->stage is carved here and held until the copies out: an ensure_stage that would have to move it meanwhile is refused
    const fq_work::Hold stage_parent = c->stage_hold;
    c->stage_hold = stage_parent.opened("grouped_host's arrays", c->stage_bytes, c->stage_bytes);
    char* dev[GROUPED_MAX_ARRAYS] = {};
    auto staged = [&]() -> int {
        size_t used = 0;
        for (size_t k = 0; k < count; k++) {                      // the caller lists the 32- and 64-byte rows first: every one of them starts 16-byte aligned
            const size_t bytes = (arrays[k].per_row ? n : groups) * arrays[k].row_bytes;
            dev[k] = c->stage + used;
            if (arrays[k].in) HIP_TRY(c, hipMemcpyAsync(dev[k], arrays[k].in, bytes, hipMemcpyHostToDevice, c->stream));
            used += bytes;
        }
        if (int rc = call(dev)) return rc;
        for (size_t k = 0; k < count; k++)
            if (arrays[k].out) HIP_TRY(c, hipMemcpyAsync(arrays[k].out, dev[k], groups * arrays[k].row_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return FOURQ_OK;
    };
    const int rc = staged();
    c->stage_hold = stage_parent;
    if (rc != FOURQ_OK) (void)hipStreamSynchronize(c->stream);    // as run_pipeline: nothing of this call may still read or write the caller's arrays
    return rc;
}
// The value of the last row of an ascending threshold table that `x` has reached; the first row is { 0, the value below every threshold }
struct Threshold { size_t from; int value; };
template <size_t K> int threshold_value(const Threshold (&table)[K], size_t x) {
    int value = table[0].value;
    for (const Threshold& row : table) if (x >= row.from) value = row.value;
    return value;
}

int mul_host(fourq_ctx* c, int algo, const uint64_t* scalars, const uint64_t* points, const uint64_t* table, uint64_t* out, size_t n) {
    const int v = algo == ENDO ? 0 : 1;
    const HostCall variable = { { { scalars, 32 }, { points, 160 } }, { { out, 160 } }, { PR_MUL_VAR, v, v ? KT_WIN_VAR : KT_ENDO_VAR }, pipe_chunk, pipe_chunk };
    const HostCall fixed = { { { scalars, 32 } }, { { out, 160 } }, { PR_MUL_FIX, v, v ? KT_WIN_FIXED : KT_ENDO_FIXED }, unit_w4_half, unit_w4, nullptr, table != nullptr };
    return host_call(c, n, points ? variable : fixed, [&](const Chunk& k) {
        return mul_dev(c, algo, k.in<uint64_t>(0), k.in<uint64_t>(1), table, k.out<uint64_t>(0), nullptr, k.m);
    });
}
int dh_host(fourq_ctx* c, int algo, const uint64_t* scalars, const uint64_t* points, const uint64_t* table, uint64_t* out,
            uint8_t* status, size_t n) {
    const int v = algo == ENDO ? 0 : 1;
    HostCall d = { { { scalars, 32 }, { points, 64 } }, { { out, 64 }, { status, 1 } }, { PR_DH_VAR, v, v ? KT_WIN_VAR + 0.3 : KT_DH_VAR }, pipe_chunk, pipe_chunk, ensure_proj };
    if (table) { d.route = { PR_DH_FIX, v, KT_DH_FIXED }; d.unit = unit_w4_half; d.unit_pageable = unit_w4; }
    return host_call(c, n, d, [&](const Chunk& k) { return dh_dev(c, algo, k.in<uint64_t>(0), k.in<uint64_t>(1), table, k.out<uint64_t>(0), k.out<uint8_t>(1), k.m); });
}

int table_host(fourq_ctx* c, int algo, const uint64_t* p_r1, uint64_t* table) {
    if (!c || !p_r1 || !table) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    int rc = ensure_stage(c, 160);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->stage, p_r1, 160, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(table_build_kernel, dim3(1), dim3(64), 0, c->stream, algo, (const u64*)c->stage, c->scratch, c->table_packed);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(table, c->table_packed, FOURQ_TABLE_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FOURQ_OK;
}

}  // namespace

extern "C" {

#define FQ_API __attribute__((visibility("default")))

FQ_API int fourq_version(void) { return 600; }    // 0.6.0; fourq_amd/_lib.py checks it at load time
#ifndef FQ_BUILD_ID
#define FQ_BUILD_ID "unknown"
#endif
FQ_API const char* fourq_build_id(void) { return FQ_BUILD_ID; }   // fourq_amd/build.py: hash of the sources and flags of this build

FQ_API const char* fourq_strerror(int code) {
    switch (code) {
    case FOURQ_OK: return "ok";
    case FOURQ_ERR_INVALID: return "invalid argument";
    case FOURQ_ERR_NODEVICE: return "no usable gfx950 HIP device";
    case FOURQ_ERR_NOMEM: return "out of memory";
    case FOURQ_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}
FQ_API const char* fourq_last_error(const fourq_ctx* ctx) { return ctx ? ctx->err : "no context"; }

FQ_API int fourq_device_count(int* count) {
    if (!count) return FOURQ_ERR_INVALID;
    *count = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return FOURQ_OK; }
    for (int d = 0; d < n; d++) {                   // devices are numbered as HIP numbers them; a non-gfx950 device ends the usable prefix
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) break;
        *count = d + 1;
    }
    return FOURQ_OK;
}

// Environment.  ONE product option is read from the environment: FOURQ_CT_SELECT (include/fourq_amd.h).  Everything else that
// changes which kernels a call takes is a TEST HOOK -- it exists so that the tests, tools/fuzz.py and the A/B probes can reach every
// route at small sizes -- and is read only when FOURQ_DEBUG_ROUTES=1 is set as well (tools/README.md lists the hooks); a production
// process cannot be re-routed by a stray variable.
static const char* route_env(const char* name) {
    const char* gate = getenv("FOURQ_DEBUG_ROUTES");
    return (gate && atoi(gate) != 0) ? getenv(name) : nullptr;
}
FQ_API int fourq_ctx_create(int device, fourq_ctx** out) {
    if (!out) return FOURQ_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return FOURQ_ERR_NODEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return FOURQ_ERR_NODEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FOURQ_ERR_NODEVICE;   // the code object is gfx950 only
    fourq_ctx* c = new (std::nothrow) fourq_ctx();
    if (!c) return FOURQ_ERR_NOMEM;
    c->device = device;
    c->cus = prop.multiProcessorCount;
    DeviceGuard g(device);
    int rc = FOURQ_OK;
    do {
        if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { rc = FOURQ_ERR_HIP; break; }
        c->stream = c->own_stream;
        if (hipStreamCreateWithFlags(&c->copy_in, hipStreamNonBlocking) != hipSuccess) { rc = FOURQ_ERR_HIP; break; }
        if (hipStreamCreateWithFlags(&c->copy_out, hipStreamNonBlocking) != hipSuccess) { rc = FOURQ_ERR_HIP; break; }
        for (int i = 0; i < PIPE_SLOTS_MAX && rc == FOURQ_OK; i++) {
            if (hipEventCreateWithFlags(&c->in_done[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->kernels_done[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->out_done[i], hipEventDisableTiming) != hipSuccess) rc = FOURQ_ERR_HIP;
        }
        if (rc) break;
        if (hipEventCreateWithFlags(&c->shadow_read, hipEventDisableTiming) != hipSuccess) { rc = FOURQ_ERR_HIP; break; }
        if (chain_setup_device() != 0) { rc = FOURQ_ERR_HIP; break; }
        // resident blocks per CU of the fused variable-base kernels (they own the per-lane scratch slots)
        int occ = 8, o = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, ladder_kernel<ENDO, FUSED, false>, BLOCK, 0) == hipSuccess && o > 0 && o < occ) occ = o;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, ladder_kernel<WINDOWED, FUSED, true>, BLOCK, 0) == hipSuccess && o > 0 && o < occ) occ = o;
        if (const char* env = route_env("FOURQ_BLOCKS_PER_CU")) { int v = atoi(env); if (v > 0 && v <= 8) occ = v; }
        c->lanes = (size_t)c->cus * occ * BLOCK;
        c->lanes_w4 = (size_t)c->cus * 4 * BLOCK;
        if (const char* env = route_env("FOURQ_HOST_BOUNCE")) c->host_bounce = atoi(env) != 0;
        if (const char* env = route_env("FOURQ_HOST_ZERO_COPY")) c->host_zero_copy = atoi(env) != 0;
        if (const char* env = route_env("FOURQ_PIPE_SLOTS")) { int v = atoi(env); if (v >= 2 && v <= PIPE_SLOTS_MAX) c->pipe_slots = v; }
        if (const char* env = route_env("FOURQ_PIPE_GENS")) { int v = atoi(env); if (v >= 0 && v <= 64) c->pipe_gens = v; }
        if (const char* env = route_env("FOURQ_PIPE_HOST_WAIT")) c->pipe_host_wait = atoi(env) != 0;
        if (const char* env = route_env("FOURQ_PIPE_HOST_POLL")) c->pipe_host_poll = atoi(env) != 0;
        if (const char* env = route_env("FOURQ_PIPE_MEASURE")) c->plan_measure = atoi(env) != 0;
        if (const char* env = route_env("FOURQ_FUSED_IO")) c->fused_io = atoi(env) != 0;
        if (const char* env = getenv("FOURQ_CT_SELECT")) c->ct = atoi(env) != 0;
        if (const char* env = route_env("FOURQ_MIXED_QUEUE")) { int v = atoi(env); if (v == 0 || v == 1) c->mixed_queue = v; }
        c->pair_max = c->lanes / 2;                        // two lanes per element: half a generation fills the chip
        if (const char* env = route_env("FOURQ_PAIR_MAX")) { long v = atol(env); if (v >= 0 && (size_t)v <= c->lanes / 2) c->pair_max = (size_t)v; }
        c->quad_max = c->pair_max < c->lanes / 4 ? c->pair_max : c->lanes / 4;
        if (const char* env = route_env("FOURQ_QUAD_MAX")) { long v = atol(env); if (v >= 0 && (size_t)v <= c->quad_max) c->quad_max = (size_t)v; }
        if (const char* env = route_env("FOURQ_NORM_K")) { int v = atoi(env); if (v == 0 || v == 2 || v == 4 || v == 8) c->norm_k = v; }
        c->mixed_round = c->lanes_w4;
        if (const char* env = route_env("FOURQ_MIXED_ROUND")) { long v = atol(env); if (v >= BLOCK && (size_t)v <= c->lanes_w4) c->mixed_round = (size_t)v; }
        const size_t scratch_u32 = std::max({
            c->lanes * NDSlots::SLOT,                                              // fused ladders (both modes), mixed_queue_kernel: N, D per resident lane; grids of at most lanes / BLOCK blocks
            c->lanes * NDSlots::SLOT + (c->lanes / 8) * LimbSlots::SLOT,           // constant-time mixed rounds: behind the fused slots, whole entries of at most lanes / 8 overflow ids (over_scratch)
            (size_t)COMB_POINTS * SLOT_U32,                                        // comb_table_kernel: whole entries + two parked points per point of the comb
            (size_t)SLOT_U32 });                                                   // table_build_kernel: one such slot
        if (hipMalloc(&c->scratch, scratch_u32 * sizeof(u32)) != hipSuccess) { rc = FOURQ_ERR_NOMEM; break; }
        if (hipMalloc(&c->table_limbs, 8 * R2_LIMBS * sizeof(u32)) != hipSuccess) { rc = FOURQ_ERR_NOMEM; break; }
        if (hipMalloc(&c->table_packed, FOURQ_TABLE_WORDS * 8) != hipSuccess) { rc = FOURQ_ERR_NOMEM; break; }
        if (hipMalloc(&c->part_counter, 8 * sizeof(u32)) != hipSuccess) { rc = FOURQ_ERR_NOMEM; break; }   // n_var, n_fix, queue head, -, fused, overflow
        if (hipMalloc(&c->part_fix, c->lanes_w4 * sizeof(u32)) != hipSuccess) { rc = FOURQ_ERR_NOMEM; break; }
        if (hipMalloc(&c->part_list, c->lanes_w4 * sizeof(u32)) != hipSuccess) { rc = FOURQ_ERR_NOMEM; break; }
        if (hipMalloc(&c->comb_limbs, COMB_POINTS * COMB_ENTRY_U32 * sizeof(u32)) != hipSuccess) { rc = FOURQ_ERR_NOMEM; break; }
        if (hipMalloc(&c->comb_packed, FOURQ_COMB_WORDS * 8) != hipSuccess) { rc = FOURQ_ERR_NOMEM; break; }
    } while (0);
    if (rc) { fourq_ctx_destroy(c); return rc; }
    *out = c;
    return FOURQ_OK;
}

FQ_API int fourq_ctx_destroy(fourq_ctx* c) {
    if (!c) return FOURQ_ERR_INVALID;
    { CtxGuard last(c); }                      // a call still running on another thread finishes first; the caller must not start new ones
    DeviceGuard g(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    for (void* p : { (void*)c->scratch, (void*)c->proj, (void*)c->table_limbs, (void*)c->table_packed, (void*)c->part_counter, (void*)c->part_list,
                     (void*)c->part_fix, (void*)c->comb_limbs, (void*)c->comb_packed, (void*)c->commit_combs, (void*)c->keyset_combs, (void*)c->keyset_bytes, (void*)c->shape_desc, (void*)c->stage, (void*)c->work, (void*)c->pipe_dev })
        if (p) (void)hipFree(p);
    if (c->pipe_pin) (void)hipHostFree(c->pipe_pin);
    if (c->zero_copy) (void)hipHostFree(c->zero_copy);
    if (c->diag_stamps) (void)hipFree(c->diag_stamps);
    if (c->diag_bracket) (void)hipFree(c->diag_bracket);
    if (c->diag_mark) (void)hipEventDestroy(c->diag_mark);
    if (c->shadow_read) (void)hipEventDestroy(c->shadow_read);
    for (hipEvent_t e : c->ticks) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->probe_ticks) if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < PIPE_SLOTS_MAX; i++) {
        if (c->in_done[i]) (void)hipEventDestroy(c->in_done[i]);
        if (c->kernels_done[i]) (void)hipEventDestroy(c->kernels_done[i]);
        if (c->out_done[i]) (void)hipEventDestroy(c->out_done[i]);
    }
    if (c->copy_in) (void)hipStreamDestroy(c->copy_in);
    if (c->copy_out) (void)hipStreamDestroy(c->copy_out);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return FOURQ_OK;
}

FQ_API int fourq_ctx_set_stream(fourq_ctx* c, void* hip_stream) {
    if (!c) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    if (next != c->stream) {
        // the staged fixed-base / comb tables were unpacked by launches on the old stream: nothing orders the new
        // stream behind them, so they are staged again (1 KiB / 7.5 KiB) by the next call that needs them
        c->table_staged = false;
        c->comb_staged = false;
    }
    c->stream = next;
    return FOURQ_OK;
}
FQ_API int fourq_ctx_set_ct_select(fourq_ctx* c, int on) {
    if (!c) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    c->ct = on != 0;
    return FOURQ_OK;
}
FQ_API int fourq_ctx_get_ct_select(const fourq_ctx* c, int* on) {
    if (!c || !on) return FOURQ_ERR_INVALID;
    *on = c->ct ? 1 : 0;
    return FOURQ_OK;
}
FQ_API int fourq_ctx_sync(fourq_ctx* c) {
    if (!c) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FOURQ_OK;
}
// Pre-sizes every buffer a _dev call for up to n elements can need (the deferred-normalisation planes and the intermediates
// of the protocol-level calls), so that those calls only enqueue: without it the first batch larger than any seen before
// synchronises the stream and reallocates inside the call (not capturable into a graph).
FQ_API int fourq_ctx_reserve(fourq_ctx* c, size_t n) {
    if (!c || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (int rc = ensure_proj(c, n)) return rc;
    return ensure_work(c, fq_work::All::max_bytes(n));
}
FQ_API int fourq_ctx_lanes(const fourq_ctx* c, size_t* lanes) {
    if (!c || !lanes) return FOURQ_ERR_INVALID;
    *lanes = c->lanes;
    return FOURQ_OK;
}

FQ_API int fourq_dev_alloc(fourq_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    HIP_TRY(c, hipMalloc(out, bytes ? bytes : 16));
    return FOURQ_OK;
}
FQ_API int fourq_dev_free(fourq_ctx* c, void* ptr) {
    if (!c) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    HIP_TRY(c, hipFree(ptr));
    return FOURQ_OK;
}
FQ_API int fourq_dev_upload(fourq_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || (bytes && (!dst || !src))) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FOURQ_OK;
}
FQ_API int fourq_dev_download(fourq_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || (bytes && (!dst || !src))) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FOURQ_OK;
}

FQ_API int fourq_table_windowed(fourq_ctx* c, const uint64_t* p, uint64_t* t) { return table_host(c, WINDOWED, p, t); }
FQ_API int fourq_table_endo(fourq_ctx* c, const uint64_t* p, uint64_t* t) { return table_host(c, ENDO, p, t); }

FQ_API int fourq_mul_endo_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t n) { return p ? mul_host(c, ENDO, s, p, nullptr, o, n) : FOURQ_ERR_INVALID; }
FQ_API int fourq_mul_windowed_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t n) { return p ? mul_host(c, WINDOWED, s, p, nullptr, o, n) : FOURQ_ERR_INVALID; }
FQ_API int fourq_mul_endo_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t n) { return p ? mul_dev(c, ENDO, s, p, nullptr, o, nullptr, n) : FOURQ_ERR_INVALID; }
FQ_API int fourq_mul_windowed_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t n) { return p ? mul_dev(c, WINDOWED, s, p, nullptr, o, nullptr, n) : FOURQ_ERR_INVALID; }
FQ_API int fourq_mul_endo_fixed_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* t, uint64_t* o, size_t n) { return t ? mul_host(c, ENDO, s, nullptr, t, o, n) : FOURQ_ERR_INVALID; }
FQ_API int fourq_mul_windowed_fixed_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* t, uint64_t* o, size_t n) { return t ? mul_host(c, WINDOWED, s, nullptr, t, o, n) : FOURQ_ERR_INVALID; }
FQ_API int fourq_mul_endo_fixed_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* t, uint64_t* o, size_t n) { return t ? mul_dev(c, ENDO, s, nullptr, t, o, nullptr, n) : FOURQ_ERR_INVALID; }
FQ_API int fourq_mul_windowed_fixed_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* t, uint64_t* o, size_t n) { return t ? mul_dev(c, WINDOWED, s, nullptr, t, o, nullptr, n) : FOURQ_ERR_INVALID; }

FQ_API int fourq_mul_endo_mixed_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, const uint8_t* flags,
                                          const uint64_t* table, uint64_t* o, size_t n) {
    if (!c || !s || !p || !flags || !table || !o || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(s) || !aligned16(p) || !aligned16(o)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    int rc = stage_table(c, table);
    if (rc) return rc;
    // At most half a generation (and no route forced): one launch of the two- / four-lane kernels, each element on its own kind of
    // table -- 0.15-0.23 ms where the work-queue kernel takes a one-lane ladder's 0.35 (profiles/r03_quadlane.txt).
    if (c->mixed_queue < 0 && c->pair_max && n <= c->pair_max) {
        LadderArgs a = {};
        a.scalars = s; a.points = p; a.out = o; a.n = (u32)n; a.flags = flags;
        return launch_pair_mixed(c, a);
    }
    // Rounds of up to mixed_round elements.  Per round: compact the ids of both kinds (counts stay on the device), then ONE persistent
    // kernel whose waves pull 64-element work items off a device-side queue (mixed_queue_kernel) or, in constant-time mode past one
    // generation (or with FOURQ_MIXED_QUEUE=0), the fused kernel over the variable-base ids + mixed_ct_tail_kernel.
    const size_t per_block = (size_t)BLOCK * PART_PER_LANE;
    for (size_t off = 0; off < n; off += c->mixed_round) {
        const u32 m = (u32)(n - off < c->mixed_round ? n - off : c->mixed_round);
        const bool queue = c->ct && c->mixed_queue >= 0 ? c->mixed_queue != 0 : mixed_queue_default(c, m);
        HIP_TRY(c, hipMemsetAsync(c->part_counter, 0, 8 * sizeof(u32), c->stream));
        hipLaunchKernelGGL(partition_kernel, dim3((unsigned)((m + per_block - 1) / per_block)), dim3(BLOCK), 0, c->stream,
                           flags + off, m, (u32)off, c->part_list, c->part_counter, c->part_fix);
        HIP_TRY(c, hipGetLastError());
        LadderArgs a = {};
        a.scalars = s; a.points = p; a.out = o; a.n = m;
        a.scratch = c->scratch; a.table = c->table_limbs;
        if (queue) {
            // BASELINE config 5's mechanism: one persistent kernel, one block per CU, every wave pulling 64-element work items
            // (variable-base first) from a device-side queue until it is empty (kernels.hip.h, mixed_queue_kernel)
            const size_t items = ((size_t)m + 63) / 64, blocks = (items + 3) / 4;
            const unsigned grid = (unsigned)(blocks < (size_t)c->cus ? blocks : (size_t)c->cus);
            if (c->ct) {
                HIPRC_TRY(c, ct_launch_mixed_queue(grid, c->stream, a, c->part_list, c->part_fix, c->part_counter, c->part_counter + 2));
            } else {
                hipLaunchKernelGGL(mixed_queue_kernel<false>, dim3(grid), dim3(BLOCK), 0, c->stream, a, c->part_list, c->part_fix, c->part_counter, c->part_counter + 2);
                HIP_TRY(c, hipGetLastError());
            }
            continue;
        }
        // Constant-time mode only: which elements are fixed-base is public, the digits are not.  The variable-base
        // ids go through the fused kernel (table in registers), the fixed-base ids through the tail kernel; both
        // read their element counts on the device.
        // A remainder of at most lanes / 8 ids past whole generations of the fused kernel is cut off on the device and
        // runs with the fixed-base elements (kernels.hip.h, mixed_ct_tail_kernel): config 5's 65 550 variable-base ids
        // are one fused generation + 14 riders, not two generations.
        const u32 limit = (u32)(c->lanes / 8);
        u32* over_scratch = c->scratch + c->lanes * NDSlots::SLOT;           // behind the fused kernels' per-lane slots
        HIPRC_TRY(c, ct_launch_split_counts(c->stream, c->part_counter, (u32)c->lanes, limit));
        LadderArgs av = a;
        av.index = c->part_list; av.n_dev = c->part_counter + 4;
        if ((rc = launch_ladder<ENDO, FUSED, false>(c, av))) return rc;
        const size_t tail_blocks = ((size_t)m + BLOCK - 1) / BLOCK, tail_max = c->lanes_w4 / BLOCK;
        HIPRC_TRY(c, ct_launch_mixed_tail((limit + BLOCK - 1) / BLOCK, (unsigned)(tail_blocks < tail_max ? tail_blocks : tail_max), c->stream, a,
                                          c->part_fix, c->part_list, c->part_counter, over_scratch));
    }
    return FOURQ_OK;
}
FQ_API int fourq_mul_endo_mixed_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* p, const uint8_t* flags,
                                      const uint64_t* table, uint64_t* o, size_t n) {
    const HostCall d = { { { s, 32 }, { p, 160 }, { flags, 1 } }, { { o, 160 } }, { PR_MIXED, 0, KT_ENDO_VAR }, unit_mixed, unit_mixed_round, nullptr, table != nullptr };
    return host_call(c, n, d, [&](const Chunk& k) {
        return fourq_mul_endo_mixed_batch_dev(c, k.in<uint64_t>(0), k.in<uint64_t>(1), k.in<uint8_t>(2), table, k.out<uint64_t>(0), k.m);
    });
}

FQ_API int fourq_dh_endo_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* p, const uint64_t* t, uint64_t* o, uint8_t* st, size_t n) { return dh_host(c, ENDO, s, p, t, o, st, n); }
FQ_API int fourq_dh_windowed_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* p, const uint64_t* t, uint64_t* o, uint8_t* st, size_t n) { return dh_host(c, WINDOWED, s, p, t, o, st, n); }
FQ_API int fourq_dh_endo_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, const uint64_t* t, uint64_t* o, uint8_t* st, size_t n) { return dh_dev(c, ENDO, s, p, t, o, st, n); }
FQ_API int fourq_dh_windowed_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, const uint64_t* t, uint64_t* o, uint8_t* st, size_t n) { return dh_dev(c, WINDOWED, s, p, t, o, st, n); }

FQ_API int fourq_comb_table(fourq_ctx* c, const uint64_t* p_r1, uint64_t* comb) {
    if (!c || !p_r1 || !comb) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    int rc = ensure_stage(c, 160);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->stage, p_r1, 160, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(comb_table_kernel, dim3((COMB_POINTS + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, (const u64*)c->stage, c->scratch, c->comb_packed);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(comb, c->comb_packed, FOURQ_COMB_WORDS * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FOURQ_OK;
}
// The staged comb stays on the device between calls.  fourq_comb_stage does the 106 KB compare-and-upload once; batch calls
// that pass comb == NULL use what is staged and do no host-side work on the table at all (a non-NULL comb is compared with the
// staged copy on every call, which costs microseconds of host time per call on the key-generation path).
// comb == NULL: "the table fourq_comb_stage was given" -- staged again from the shadow if the stream has changed since
static int stage_comb(fourq_ctx* c, const uint64_t* comb) {
    if (!comb) {
        if (!c->comb_known) return FOURQ_ERR_INVALID;          // NULL = "the staged table": there must be one
        if (c->comb_staged) return FOURQ_OK;
        if (int rc = staging_allowed(c)) return rc;
    } else {
        if (c->comb_staged && memcmp(c->comb_shadow, comb, sizeof c->comb_shadow) == 0) return FOURQ_OK;      // as stage_table
        if (int rc = staging_allowed(c)) return rc;
        c->comb_staged = false;
        if (int rc = shadow_free(c)) return rc;
        memcpy(c->comb_shadow, comb, sizeof c->comb_shadow);
        c->comb_known = true;
    }
    HIP_TRY(c, hipMemcpyAsync(c->comb_packed, c->comb_shadow, FOURQ_COMB_WORDS * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(c->shadow_read, c->stream));
    hipLaunchKernelGGL(comb_unpack_kernel, dim3((COMB_POINTS + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, c->comb_packed, c->comb_limbs);
    HIP_TRY(c, hipGetLastError());
    c->comb_staged = true;
    return FOURQ_OK;
}
FQ_API int fourq_comb_stage(fourq_ctx* c, const uint64_t* comb) {
    if (!c || !comb) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    return stage_comb(c, comb);
}
// The one-lane comb.  Constant-time mode: 256-lane blocks, four per CU, over the small shape; otherwise one block per CU with the fast shape's
// table.  proj != NULL defers the normalisation: (X, Y, Z) go to the context's projective planes.
static int launch_comb(fourq_ctx* c, const uint64_t* scalars, uint64_t* out, uint8_t* status, uint4* proj, size_t n) {
    const size_t blocks = (n + BLOCK - 1) / BLOCK, blocks_max = c->lanes_w4 / BLOCK;
    const unsigned grid_or_cus = c->ct ? (unsigned)(blocks < blocks_max ? blocks : blocks_max) : (unsigned)c->cus;
    HIPRC_TRY(c, (c->ct ? ct_launch_comb : chain_launch_comb)(grid_or_cus, c->stream, scalars, c->comb_limbs, out, status, proj, (u32)c->proj_capacity, (u32)n));
    return FOURQ_OK;
}
// ... deferred for EVERY n, also the sizes fourq_comb_mul_batch_dev gives to comb_quad_kernel; the caller has sized the planes (ensure_proj)
static int launch_comb_deferred(fourq_ctx* c, const uint64_t* scalars, uint8_t* status, size_t n) { return launch_comb(c, scalars, nullptr, status, c->proj, n); }
// comb -> normalize -> encode: [k_i]B as 32-byte strings through `affine` (key generation's public keys, a signature's R)
static int comb_encode(fourq_ctx* c, const uint64_t* scalars, uint64_t* affine, uint8_t* st_comb, uint8_t* out32, size_t n) {
    if (int rc = launch_comb_deferred(c, scalars, st_comb, n)) return rc;
    const int group = normalize_group(c, n);
    HIPRC_TRY(c, chain_launch_normalize(group ? group : 1, c->stream, c->proj, (u32)c->proj_capacity, affine, st_comb, (u32)n));
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, affine, (u64*)out32, (u32)n);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
FQ_API int fourq_comb_mul_batch_dev(fourq_ctx* c, const uint64_t* scalars, const uint64_t* comb, uint64_t* out, uint8_t* status, size_t n) {
    if (!c || !scalars || !out || !status || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(scalars) || !aligned16(out)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    if (int rc = stage_comb(c, comb)) return rc;
    const int group = normalize_group(c, n);
    // At most a quarter generation, selection by address: four lanes per element, entries gathered where the table lies (kernels.hip.h,
    // comb_quad_kernel): a batch of one 0.107 -> 0.05x ms (profiles/r03_quadlane.txt)
    if (!group && n <= c->pair_max) {         // two lanes per element between a quarter and half a generation: 0.100 -> 0.06x ms
        bool quad;
        const unsigned grid = pair_grid(c, n, false, &quad);
        if (c->ct) {
            HIPRC_TRY(c, ct_launch_comb_quad(quad, grid, c->stream, scalars, c->comb_limbs, out, status, (u32)n));
            return FOURQ_OK;
        }
        if (quad) hipLaunchKernelGGL((comb_quad_kernel<false, 4>), dim3(grid), dim3(BLOCK), 0, c->stream, scalars, c->comb_limbs, out, status, (u32)n);
        else hipLaunchKernelGGL((comb_quad_kernel<false, 2>), dim3(grid), dim3(BLOCK), 0, c->stream, scalars, c->comb_limbs, out, status, (u32)n);
        HIP_TRY(c, hipGetLastError());
        return FOURQ_OK;
    }
    int rc = group ? ensure_proj(c, n) : FOURQ_OK;
    if (rc) return rc;
    if ((rc = launch_comb(c, scalars, out, status, group ? c->proj : nullptr, n))) return rc;
    if (group) HIPRC_TRY(c, chain_launch_normalize(group, c->stream, c->proj, (u32)c->proj_capacity, out, status, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_comb_mul_batch(fourq_ctx* c, const uint64_t* scalars, const uint64_t* comb, uint64_t* out, uint8_t* status, size_t n) {
    const HostCall d = { { { scalars, 32 } }, { { out, 64 }, { status, 1 } }, { PR_COMB, 0, KT_COMB }, unit_w4 };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& k) {
        return fourq_comb_mul_batch_dev(c, k.in<uint64_t>(0), nullptr, k.out<uint64_t>(0), k.out<uint8_t>(1), k.m);
    });
}

FQ_API int fourq_encode_batch_dev(fourq_ctx* c, const uint64_t* affine, uint8_t* out32, size_t n) {
    if (!c || !affine || !out32 || n > FOURQ_MAX_BATCH || !aligned16(affine) || !aligned16(out32)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    hipLaunchKernelGGL(encode_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, affine, (u64*)out32, (u32)n);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
FQ_API int fourq_decode_batch_dev(fourq_ctx* c, const uint8_t* in32, uint64_t* affine, uint8_t* status, size_t n) {
    if (!c || !in32 || !affine || !status || n > FOURQ_MAX_BATCH || !aligned16(in32) || !aligned16(affine)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    hipLaunchKernelGGL(decode_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, (const u64*)in32, affine, status, (u32)n);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
FQ_API int fourq_encode_batch(fourq_ctx* c, const uint64_t* affine, uint8_t* out32, size_t n) {
    const HostCall d = { { { affine, 64 } }, { { out32, 32 } }, { PR_ENCODE, 0, KT_ENCODE }, unit_w4_x4 };
    return host_call(c, n, d, [&](const Chunk& k) { return fourq_encode_batch_dev(c, k.in<uint64_t>(0), k.out<uint8_t>(0), k.m); });
}
FQ_API int fourq_decode_batch(fourq_ctx* c, const uint8_t* in32, uint64_t* affine, uint8_t* status, size_t n) {
    const HostCall d = { { { in32, 32 } }, { { affine, 64 }, { status, 1 } }, { PR_DECODE, 0, KT_DECODE }, unit_w4 };
    return host_call(c, n, d, [&](const Chunk& k) { return fourq_decode_batch_dev(c, k.in<uint8_t>(0), k.out<uint64_t>(0), k.out<uint8_t>(1), k.m); });
}

// ---- protocol-level calls: every intermediate stays on the device -------------------------------------------
// decode -> DH_<algo> -> encode (draft-ladd-cfrg-4q.md:707-723; curve4q.py:49-96, :446-462, :41-46)
static int dh_bytes_dev(fourq_ctx* c, int algo, const uint64_t* scalars, const uint8_t* keys32, const uint64_t* table, uint8_t* out32,
                        uint8_t* status, size_t n) {
    if (!c || !scalars || !keys32 || !out32 || !status || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(scalars) || !aligned16(keys32) || !aligned16(out32)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, DhBytes, n);
    if (int rc = fourq_decode_batch_dev(c, keys32, w->pts, w->st_decode, n)) return rc;
    if (int rc = dh_dev(c, algo, scalars, w->pts, table, w->shared, w->st_dh, n)) return rc;    // an undecodable key is (0, 0): rejected again here
    hipLaunchKernelGGL(encode_status_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, w->shared, w->st_decode, w->st_dh,
                       (u64*)out32, status, (u32)n);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
static int dh_bytes_host(fourq_ctx* c, int algo, const uint64_t* scalars, const uint8_t* keys32, const uint64_t* table, uint8_t* out32,
                         uint8_t* status, size_t n) {
    const int v = algo == ENDO ? 0 : 1;
    HostCall d = { { { scalars, 32 }, { keys32, 32 } }, { { out32, 32 }, { status, 1 } }, { PR_DHB_VAR, v, (v ? KT_WIN_VAR + 0.3 : KT_DH_VAR) + KT_CODEC }, pipe_chunk, pipe_chunk,
                   reserve_for<fq_work::DhBytes> };
    if (table) { d.route = { PR_DHB_FIX, v, KT_DH_FIXED + KT_CODEC }; d.unit = unit_w4_half; d.unit_pageable = unit_w4; }
    return host_call(c, n, d, [&](const Chunk& k) { return dh_bytes_dev(c, algo, k.in<uint64_t>(0), k.in<uint8_t>(1), table, k.out<uint8_t>(0), k.out<uint8_t>(1), k.m); });
}
// ---- MUL_* with affine / encoded I/O: R1toAffine(MUL_<algo>(m, AffineToR1(P))) and encode(.) of it --------------------------
// 160 (96) bytes per operation across the ABI instead of the raw-R1 form's 352: the host-array calls are bound by the link, not by the
// kernels ("PCIe-inclusive").  Parity level L1 (canonical affine); the raw-R1 entry points are untouched.
// R1toAffine (+ encode) behind a MUL_*: one inversion per element while the chunk is at most two generations, one per four beyond
static int launch_lower(fourq_ctx* c, bool enc, const uint64_t* r1, u32 stride, const uint8_t* st_decode, uint64_t* out, uint8_t* status, size_t n) {
    const bool batched = n > 2 * c->lanes;
    const size_t lanes = batched ? (n + 3) / 4 : n;
    const unsigned grid = (unsigned)((lanes + BLOCK - 1) / BLOCK);
    if (enc && batched) hipLaunchKernelGGL((lower_kernel<4, true>), dim3(grid), dim3(BLOCK), 0, c->stream, r1, stride, st_decode, out, status, (u32)n);
    else if (enc) hipLaunchKernelGGL((lower_kernel<1, true>), dim3(grid), dim3(BLOCK), 0, c->stream, r1, stride, st_decode, out, status, (u32)n);
    else if (batched) hipLaunchKernelGGL((lower_kernel<4, false>), dim3(grid), dim3(BLOCK), 0, c->stream, r1, stride, st_decode, out, status, (u32)n);
    else hipLaunchKernelGGL((lower_kernel<1, false>), dim3(grid), dim3(BLOCK), 0, c->stream, r1, stride, st_decode, out, status, (u32)n);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
// Does the whole batch run on the fused one-lane-per-element kernels?  Only those take the affine-in / (X, Y, Z)-out flags (LadderArgs::io):
// then the lane lifts its own point and leaves the three coordinates R1toAffine reads -- no lift kernel, no R1 rows.  Batches with a
// two-lane tail keep the separate lift and full R1 rows (FOURQ_FUSED_IO=0, a test hook, forces that everywhere).
static bool fused_io(const fourq_ctx* c, size_t n) { return c->fused_io && variable_route(c, n, false) == ROUTE_FUSED; }
// The ladder half that MUL_* with affine / encoded I/O and [k]B + [l]P share: prepares the ladder's input rows and runs MUL_<algo> into rows_out.
// Where the whole batch runs on the fused kernels the lanes lift their own points and leave (X, Y, Z): encoded points are decoded to affine rows,
// affine ones read where they lie, and *stride, the words per row of rows_out, is 12; otherwise decode + lift / lift to full R1 rows, and 20.
static int mul_rows_dev(fourq_ctx* c, int algo, const uint64_t* scalars, const void* points, bool encoded, uint64_t* rows_in, uint64_t* rows_out,
                        uint8_t* st_decode, size_t n, u32* stride) {
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    const bool fused = fused_io(c, n);
    const uint64_t* ladder_in = rows_in;
    if (encoded) {
        if (fused) hipLaunchKernelGGL(decode_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, (const u64*)points, rows_in, st_decode, (u32)n);
        else hipLaunchKernelGGL(decode_lift_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, (const u64*)points, rows_in, st_decode, (u32)n);
        HIP_TRY(c, hipGetLastError());
    } else if (fused) {
        ladder_in = (const uint64_t*)points;
    } else {
        hipLaunchKernelGGL(lift_affine_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, (const u64*)points, rows_in, (u32)n);
        HIP_TRY(c, hipGetLastError());
    }
    *stride = fused ? 12 : 20;
    return mul_dev(c, algo, scalars, ladder_in, nullptr, rows_out, nullptr, n, fused ? (LADDER_IO_AFFINE_IN | LADDER_IO_XYZ_OUT) : 0);
}
static int mul_affine_dev(fourq_ctx* c, int algo, const uint64_t* scalars, const uint64_t* points_affine, uint64_t* out_affine, size_t n) {
    if (!c || !scalars || !points_affine || !out_affine || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(scalars) || !aligned16(points_affine) || !aligned16(out_affine)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, MulRows, n);
    u32 stride;
    if (int rc = mul_rows_dev(c, algo, scalars, points_affine, false, w->rows_in, w->rows_out, nullptr, n, &stride)) return rc;
    return launch_lower(c, false, w->rows_out, stride, nullptr, out_affine, nullptr, n);
}
static int mul_affine_host(fourq_ctx* c, int algo, const uint64_t* scalars, const uint64_t* points_affine, uint64_t* out_affine, size_t n) {
    const int v = algo == ENDO ? 0 : 1;
    const HostCall d = { { { scalars, 32 }, { points_affine, 64 } }, { { out_affine, 64 } }, { PR_AFF, v, (v ? KT_WIN_VAR : KT_ENDO_VAR) + KT_LIFT_LOWER }, pipe_chunk, nullptr,
                         reserve_for<fq_work::MulRows> };
    return host_call(c, n, d, [&](const Chunk& k) { return mul_affine_dev(c, algo, k.in<uint64_t>(0), k.in<uint64_t>(1), k.out<uint64_t>(0), k.m); });
}
// decode -> MUL_<algo> -> encode.  status: 0 ok | 16 + FOURQ_DECODE_* (out32 is zero then); MUL_* itself cannot fail.
static int mul_bytes_dev(fourq_ctx* c, int algo, const uint64_t* scalars, const uint8_t* points32, uint8_t* out32, uint8_t* status, size_t n) {
    if (!c || !scalars || !points32 || !out32 || !status || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(scalars) || !aligned16(points32) || !aligned16(out32)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, MulRows, n);
    u32 stride;
    if (int rc = mul_rows_dev(c, algo, scalars, points32, true, w->rows_in, w->rows_out, w->st_decode, n, &stride)) return rc;
    return launch_lower(c, true, w->rows_out, stride, w->st_decode, (uint64_t*)out32, status, n);
}
static int mul_bytes_host(fourq_ctx* c, int algo, const uint64_t* scalars, const uint8_t* points32, uint8_t* out32, uint8_t* status, size_t n) {
    const int v = algo == ENDO ? 0 : 1;
    const HostCall d = { { { scalars, 32 }, { points32, 32 } }, { { out32, 32 }, { status, 1 } }, { PR_BYTES, v, (v ? KT_WIN_VAR : KT_ENDO_VAR) + KT_LIFT_LOWER + KT_CODEC }, pipe_chunk, nullptr,
                         reserve_for<fq_work::MulRows> };
    return host_call(c, n, d, [&](const Chunk& k) { return mul_bytes_dev(c, algo, k.in<uint64_t>(0), k.in<uint8_t>(1), k.out<uint8_t>(0), k.out<uint8_t>(1), k.m); });
}
FQ_API int fourq_mul_endo_affine_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t n) { return mul_affine_dev(c, ENDO, s, p, o, n); }
FQ_API int fourq_mul_windowed_affine_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t n) { return mul_affine_dev(c, WINDOWED, s, p, o, n); }
FQ_API int fourq_mul_endo_affine_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t n) { return mul_affine_host(c, ENDO, s, p, o, n); }
FQ_API int fourq_mul_windowed_affine_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t n) { return mul_affine_host(c, WINDOWED, s, p, o, n); }
FQ_API int fourq_mul_endo_bytes_batch_dev(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st, size_t n) { return mul_bytes_dev(c, ENDO, s, p, o, st, n); }
FQ_API int fourq_mul_windowed_bytes_batch_dev(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st, size_t n) { return mul_bytes_dev(c, WINDOWED, s, p, o, st, n); }
FQ_API int fourq_mul_endo_bytes_batch(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st, size_t n) { return mul_bytes_host(c, ENDO, s, p, o, st, n); }
FQ_API int fourq_mul_windowed_bytes_batch(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st, size_t n) { return mul_bytes_host(c, WINDOWED, s, p, o, st, n); }

FQ_API int fourq_dh_endo_bytes_batch_dev(fourq_ctx* c, const uint64_t* s, const uint8_t* k, const uint64_t* t, uint8_t* o, uint8_t* st, size_t n) { return dh_bytes_dev(c, ENDO, s, k, t, o, st, n); }
FQ_API int fourq_dh_windowed_bytes_batch_dev(fourq_ctx* c, const uint64_t* s, const uint8_t* k, const uint64_t* t, uint8_t* o, uint8_t* st, size_t n) { return dh_bytes_dev(c, WINDOWED, s, k, t, o, st, n); }
FQ_API int fourq_dh_endo_bytes_batch(fourq_ctx* c, const uint64_t* s, const uint8_t* k, const uint64_t* t, uint8_t* o, uint8_t* st, size_t n) { return dh_bytes_host(c, ENDO, s, k, t, o, st, n); }
FQ_API int fourq_dh_windowed_bytes_batch(fourq_ctx* c, const uint64_t* s, const uint8_t* k, const uint64_t* t, uint8_t* o, uint8_t* st, size_t n) { return dh_bytes_host(c, WINDOWED, s, k, t, o, st, n); }

// dh_exchange: DH_endo(a_i, DH_endo(b_i, base [, table392])) with the first half's public keys kept on the device
FQ_API int fourq_dh_exchange_batch_dev(fourq_ctx* c, const uint64_t* a, const uint64_t* b, const uint64_t* base_affine, const uint64_t* table392,
                                       uint64_t* out, uint8_t* status, size_t n) {
    if (!c || !a || !b || !base_affine || !out || !status || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(a) || !aligned16(b) || !aligned16(out)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, Exchange, n);      // mid = DH(b_i, base): the public keys
    AffineArg point;
    memcpy(point.w, base_affine, sizeof point.w);             // read once, here: the launch carries it
    const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(broadcast_point_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, point, w->base_pts, (u32)n);
    HIP_TRY(c, hipGetLastError());
    if (int rc = dh_dev(c, ENDO, b, w->base_pts, table392, w->mid, w->st_first, n)) return rc;
    if (int rc = dh_dev(c, ENDO, a, w->mid, nullptr, out, status, n)) return rc;
    hipLaunchKernelGGL(merge_status_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, w->st_first, status, (u32)n);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
FQ_API int fourq_dh_exchange_batch(fourq_ctx* c, const uint64_t* a, const uint64_t* b, const uint64_t* base_affine, const uint64_t* table392,
                                   uint64_t* out, uint8_t* status, size_t n) {
    uint64_t base_copy[8];
    // unit: one generation of the fixed-base half (two waves per SIMD) = two of the variable-base half (one wave per SIMD)
    const HostCall d = { { { a, 32 }, { b, 32 } }, { { out, 64 }, { status, 1 } }, { PR_EXCH, table392 ? 1 : 0, (table392 ? KT_DH_FIXED : KT_DH_VAR) + KT_DH_VAR }, unit_w4_half, unit_w4,
                         reserve_for<fq_work::Exchange>, base_affine != nullptr };
    return host_call(c, n, d, [&] { memcpy(base_copy, base_affine, sizeof base_copy); return FOURQ_OK; }, [&](const Chunk& k) {      // the caller's buffer is read once
        return fourq_dh_exchange_batch_dev(c, k.in<uint64_t>(0), k.in<uint64_t>(1), base_copy, table392, k.out<uint64_t>(0), k.out<uint8_t>(1), k.m);
    });
}

// dh_exchange with the key-generation half through the comb (bench.py's cfg4 step as one call)
FQ_API int fourq_dh_exchange_comb_batch_dev(fourq_ctx* c, const uint64_t* a, const uint64_t* b, const uint64_t* comb, uint64_t* out, uint8_t* status, size_t n) {
    if (!c || !a || !b || !out || !status || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(a) || !aligned16(b) || !aligned16(out)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, Exchange, n);      // mid = [b_i]B: the public keys
    if (int rc = fourq_comb_mul_batch_dev(c, b, comb, w->mid, w->st_first, n)) return rc;
    if (int rc = dh_dev(c, ENDO, a, w->mid, nullptr, out, status, n)) return rc;
    hipLaunchKernelGGL(merge_status_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, w->st_first, status, (u32)n);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
FQ_API int fourq_dh_exchange_comb_batch(fourq_ctx* c, const uint64_t* a, const uint64_t* b, const uint64_t* comb, uint64_t* out, uint8_t* status, size_t n) {
    const HostCall d = { { { a, 32 }, { b, 32 } }, { { out, 64 }, { status, 1 } }, { PR_EXCH_COMB, 0, KT_COMB + KT_DH_VAR }, unit_w4_half, unit_w4, reserve_for<fq_work::Exchange> };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& k) {
        return fourq_dh_exchange_comb_batch_dev(c, k.in<uint64_t>(0), k.in<uint64_t>(1), nullptr, k.out<uint64_t>(0), k.out<uint8_t>(1), k.m);
    });
}

// ---- [k]B + [l]P: the curve part of a Schnorr-type verification (R' = [s]B + [h]A) -------------------------------------------
// Three stages on the context's stream, nothing affine in between: (1) the comb with deferred normalisation leaves (X, Y, Z) of [k_i]B in
// the context's projective planes -- comb_kernel<true, CT> for EVERY n, also the sizes fourq_comb_mul_batch gives to comb_quad_kernel, which
// has only an affine + status output; its projective neutral for k = 0 (mod N) is an ordinary operand of the
// addition, not FOURQ_DH_NEUTRAL; (2) MUL_endo through mul_dev as mul_affine_dev / mul_bytes_dev call it, so every variable-base route is
// inherited: (X, Y, Z) rows of 12 words where the batch runs on the fused kernels, lift + R1 rows of 20 words otherwise; (3) combine_kernel
// (combine.hip.h) adds the halves and lowers the sum, one inversion per element while the batch is within two generations (one wave per SIMD: the chain's latency is the
// time either way, as launch_lower) and one per two beyond.  `points`: n x 8 affine words, or n x 32 bytes when `encoded`; out_kind: CombineOut.
static int double_mul_dev(fourq_ctx* c, const uint64_t* k, const uint64_t* comb, const uint64_t* l, const void* points, bool encoded, int out_kind,
                          const uint8_t* expect32, void* out, uint8_t* status, uint8_t* ok, size_t n) {
    if (!c || !k || !l || !points || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (out_kind == COMBINE_VERIFY ? (!expect32 || !ok || !status || !aligned16(expect32)) : (!out || !aligned16(out))) return FOURQ_ERR_INVALID;
    if (out_kind == COMBINE_ENCODE && !status) return FOURQ_ERR_INVALID;
    if (!aligned16(k) || !aligned16(l) || !aligned16(points)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    int rc = stage_comb(c, comb);
    if (rc) return rc;
    WORK_SCOPE(w, DoubleMul, n);
    // (1) [k_i]B, projective
    if ((rc = launch_comb_deferred(c, k, w->st_comb, n))) return rc;
    // (2) [l_i]P_i, projective
    u32 stride;
    if ((rc = mul_rows_dev(c, ENDO, l, points, encoded, w->rows_in, w->rows_out, w->st_decode, n, &stride))) return rc;
    // (3) the sum, lowered
    HIPRC_TRY(c, chain_launch_combine(n > 2 * c->lanes ? 2 : 1, out_kind, c->stream, c->proj, (u32)c->proj_capacity, w->rows_out, stride,
                                      encoded ? w->st_decode : nullptr, (const u64*)expect32, (u64*)out, status, ok, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_double_mul_affine_batch_dev(fourq_ctx* c, const uint64_t* k, const uint64_t* comb, const uint64_t* l, const uint64_t* p, uint64_t* o, size_t n) { return double_mul_dev(c, k, comb, l, p, false, COMBINE_AFFINE, nullptr, o, nullptr, nullptr, n); }
FQ_API int fourq_double_mul_bytes_batch_dev(fourq_ctx* c, const uint64_t* k, const uint64_t* comb, const uint64_t* l, const uint8_t* p, uint8_t* o, uint8_t* st, size_t n) { return double_mul_dev(c, k, comb, l, p, true, COMBINE_ENCODE, nullptr, o, st, nullptr, n); }
FQ_API int fourq_verify_bytes_batch_dev(fourq_ctx* c, const uint64_t* k, const uint64_t* comb, const uint64_t* l, const uint8_t* p, const uint8_t* expect32, uint8_t* ok, uint8_t* st, size_t n) { return double_mul_dev(c, k, comb, l, p, true, COMBINE_VERIFY, expect32, nullptr, st, ok, n); }
FQ_API int fourq_double_mul_affine_batch(fourq_ctx* c, const uint64_t* k, const uint64_t* comb, const uint64_t* l, const uint64_t* points_affine, uint64_t* out_affine, size_t n) {
    const HostCall d = { { { k, 32 }, { l, 32 }, { points_affine, 64 } }, { { out_affine, 64 } }, { PR_DOUBLE_AFF, 0, KT_DOUBLE }, pipe_chunk, nullptr, reserve_for<fq_work::DoubleMul> };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& x) {
        return fourq_double_mul_affine_batch_dev(c, x.in<uint64_t>(0), nullptr, x.in<uint64_t>(1), x.in<uint64_t>(2), x.out<uint64_t>(0), x.m);
    });
}
FQ_API int fourq_double_mul_bytes_batch(fourq_ctx* c, const uint64_t* k, const uint64_t* comb, const uint64_t* l, const uint8_t* points32, uint8_t* out32, uint8_t* status, size_t n) {
    const HostCall d = { { { k, 32 }, { l, 32 }, { points32, 32 } }, { { out32, 32 }, { status, 1 } }, { PR_DOUBLE_BYTES, 0, KT_DOUBLE + KT_DECODE }, pipe_chunk, nullptr,
                         reserve_for<fq_work::DoubleMul> };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& x) {
        return fourq_double_mul_bytes_batch_dev(c, x.in<uint64_t>(0), nullptr, x.in<uint64_t>(1), x.in<uint8_t>(2), x.out<uint8_t>(0), x.out<uint8_t>(1), x.m);
    });
}
FQ_API int fourq_verify_bytes_batch(fourq_ctx* c, const uint64_t* k, const uint64_t* comb, const uint64_t* l, const uint8_t* points32, const uint8_t* expect32,
                                    uint8_t* ok, uint8_t* status, size_t n) {
    const HostCall d = { { { k, 32 }, { l, 32 }, { points32, 32 }, { expect32, 32 } }, { { ok, 1 }, { status, 1 } }, { PR_DOUBLE_VERIFY, 0, KT_DOUBLE + KT_DECODE }, pipe_chunk, nullptr,
                         reserve_for<fq_work::DoubleMul> };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& x) {
        return fourq_verify_bytes_batch_dev(c, x.in<uint64_t>(0), nullptr, x.in<uint64_t>(1), x.in<uint8_t>(2), x.in<uint8_t>(3), x.out<uint8_t>(0), x.out<uint8_t>(1), x.m);
    });
}

// ---- grouped multi-scalar multiplication: out[g] = R1toAffine(sum_j MUL_endo(k_gj, AffineToR1(P_gj))) over groups of one length ----------
// (1) MUL_endo through mul_rows_dev over all groups x group_size elements, projective rows of 12 or 20 words; (2) fold passes (msm.hip.h),
// each turning m rows per group into ceil(m / MSM_FOLD), alternating between the layout's two regions until one row per group is left;
// (3) lower_kernel over the `groups` rows, which also turns a group's largest decode code into its status.  The geometry of every launch
// follows from (groups, group_size) on the host: nothing is staged and, once the work buffer is large enough, nothing allocated.
// The fold passes: the first writes part_a, the next part_b, and so on, until one row per group is left; *rows, *stride and *st then name
// it (they are unchanged where group_size == 1).  st_a / st_b: the status planes that ride along where *st is not NULL.
struct FoldParts { uint64_t *a, *b; uint8_t *st_a, *st_b; };
static int fold_to_one_row(fourq_ctx* c, const FoldParts& parts, size_t groups, size_t group_size, const uint64_t** rows, u32* stride, const uint8_t** st) {
    bool to_a = true;
    for (size_t m = group_size; m > 1; to_a = !to_a) {
        uint64_t* part = to_a ? parts.a : parts.b;
        uint8_t* part_st = to_a ? parts.st_a : parts.st_b;
        HIPRC_TRY(c, chain_launch_msm_fold(c->stream, *rows, *stride, *st, part, part_st, groups, m));
        m = (m + MSM_FOLD - 1) / MSM_FOLD;
        *rows = part; *stride = 12;
        if (*st) *st = part_st;
    }
    return FOURQ_OK;
}
static int msm_dev(fourq_ctx* c, const uint64_t* scalars, const void* points, bool encoded, void* out, uint8_t* status, size_t groups, size_t group_size) {
    size_t n;
    int rc = grouped_rows(c && scalars && points && out && (!encoded || status) && aligned16(scalars) && aligned16(points) && aligned16(out), groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    WORK_SCOPE(w, Msm, n);
    u32 stride;
    if ((rc = mul_rows_dev(c, ENDO, scalars, points, encoded, w->rows_in, w->rows_out, encoded ? w->st_decode : nullptr, n, &stride))) return rc;
    const uint64_t* rows = w->rows_out;
    const uint8_t* st = encoded ? w->st_decode : nullptr;
    if ((rc = fold_to_one_row(c, { w->part_a, w->part_b, w->st_a, w->st_b }, groups, group_size, &rows, &stride, &st))) return rc;
    return launch_lower(c, encoded, rows, stride, st, (uint64_t*)out, status, groups);
}
// Host arrays of the grouped sums on either route (grouped_host).  sum_dev: the _dev call to make -- it gets msm_dev's five arguments behind the
// context, over the staged arrays; args_ok: what that call asks beyond the arrays (the bucket route's window).
using SumDev = std::function<int(const uint64_t* scalars, const void* points, bool encoded, void* out, uint8_t* status)>;
static int sum_host(fourq_ctx* c, bool args_ok, const uint64_t* scalars, const void* points, bool encoded, void* out, uint8_t* status, size_t groups, size_t group_size,
                    const SumDev& sum_dev) {
    size_t n;
    const int rc = grouped_rows(c && scalars && points && out && (!encoded || status) && args_ok, groups, group_size, &n);
    if (rc || !n) return rc;
    const size_t point_bytes = encoded ? 32 : 64;
    const GroupedArray arrays[] = { { scalars, nullptr, 32, true }, { points, nullptr, point_bytes, true }, { nullptr, out, point_bytes, false }, { nullptr, status, 1, false } };
    return grouped_host(c, n, groups, arrays, encoded ? 4 : 3, [&](char* const* d) {
        return sum_dev((const uint64_t*)d[0], (const void*)d[1], encoded, (void*)d[2], encoded ? (uint8_t*)d[3] : nullptr);
    });
}
FQ_API int fourq_msm_affine_batch_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t groups, size_t group_size) { return msm_dev(c, s, p, false, o, nullptr, groups, group_size); }
FQ_API int fourq_msm_bytes_batch_dev(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st, size_t groups, size_t group_size) { return msm_dev(c, s, p, true, o, st, groups, group_size); }
FQ_API int fourq_msm_affine_batch(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t groups, size_t group_size) { return sum_host(c, true, s, p, false, o, nullptr, groups, group_size, [&](auto... staged) { return msm_dev(c, staged..., groups, group_size); }); }
FQ_API int fourq_msm_bytes_batch(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st, size_t groups, size_t group_size) { return sum_host(c, true, s, p, true, o, st, groups, group_size, [&](auto... staged) { return msm_dev(c, staged..., groups, group_size); }); }

// ---- ragged grouped sums (msm_shape.h): the same sums over groups of any length, 0 included, by a registered shape -----------------------
// The offsets are public metadata: the host validates them and turns them into the geometry of every fold pass (fq_work::ShapePlan), and the
// context holds that -- the passes here, their descriptors on the device -- the way it holds the commitment bases and the key set.  No
// kernel reads an offset.  Route: mul_rows_dev over the shape's n rows (skipped where n == 0), the planned passes, launch_lower over `groups`.
static_assert(fq_work::ShapePlan::FOLD == MSM_FOLD, "msm_shape.h plans the passes for msm_fold_desc_kernel's segment");
static_assert(sizeof(fq_work::ShapeDesc) == sizeof(uint2), "a descriptor is the 8 bytes a team's lanes load");
// Everything goes into a NEW plan and a NEW array, and the old shape is replaced once they are complete: a failure keeps it.
FQ_API int fourq_raggedsum_shape_set(fourq_ctx* c, const uint32_t* offsets, size_t groups) {
    if (!c || !offsets) return FOURQ_ERR_INVALID;
    fq_work::ShapePlan plan;
    const auto built = plan.build(offsets, groups, FOURQ_MAX_BATCH);
    if (built != fq_work::ShapePlan::OK) return built == fq_work::ShapePlan::NOMEM ? FOURQ_ERR_NOMEM : FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (int rc = staging_allowed(c)) return rc;
    uint2* desc = nullptr;
    if (!plan.desc.empty()) {
        const size_t bytes = plan.desc.size() * sizeof(fq_work::ShapeDesc);
        hipError_t e = hipMalloc(&desc, bytes);
        if (e != hipSuccess) return fail(c, e, "hipMalloc(the descriptors of the shape)");
        e = hipMemcpyAsync(desc, plan.desc.data(), bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); (void)hipFree(desc); return fail(c, e, "uploading the descriptors of the shape"); }
    } else {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (c->shape_desc) (void)hipFree(c->shape_desc);          // the stream is idle: nothing reads the old descriptors any more
    std::vector<fq_work::ShapeDesc>().swap(plan.desc);        // the device has them; the context keeps the passes only
    c->shape = std::move(plan);
    c->shape_desc = desc;
    return FOURQ_OK;
}
FQ_API int fourq_raggedsum_shape_count(const fourq_ctx* c, size_t* groups, size_t* rows) {
    if (!c || !groups || !rows) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    *groups = c->shape.groups;
    *rows = c->shape.rows;
    return FOURQ_OK;
}
FQ_API int fourq_raggedsum_shape_reserve(fourq_ctx* c) {
    if (!c) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (c->shape.groups == 0) return FOURQ_ERR_INVALID;
    return size_for<fq_work::MsmRagged>(c, false, c->shape.rows, c->shape.groups);
}
// fold_to_one_row over the planned passes: the first writes part_a, the next part_b, and so on; *rows, *stride and *st then name the one row
// per group (they are unchanged where the plan has no pass: every group has exactly one row).
static int fold_planned(fourq_ctx* c, const FoldParts& parts, const uint64_t** rows, u32* stride, const uint8_t** st) {
    bool to_a = true;
    for (const fq_work::ShapePass& pass : c->shape.passes) {
        uint64_t* part = to_a ? parts.a : parts.b;
        uint8_t* part_st = to_a ? parts.st_a : parts.st_b;
        HIPRC_TRY(c, chain_launch_msm_fold_desc(c->stream, *rows, *stride, *st, part, part_st, c->shape_desc + pass.desc_at, pass.rows_out, pass.team, pass.iters));
        *rows = part; *stride = 12;
        if (*st) *st = part_st;
        to_a = !to_a;
    }
    return FOURQ_OK;
}
static int ragged_dev(fourq_ctx* c, const uint64_t* scalars, const void* points, bool encoded, void* out, uint8_t* status) {
    if (!c || !scalars || !points || !out || (encoded && !status) || !aligned16(scalars) || !aligned16(points) || !aligned16(out)) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    const size_t groups = c->shape.groups, n = c->shape.rows;
    if (groups == 0) return FOURQ_ERR_INVALID;                // no shape
    WORK_SCOPE(w, MsmRagged, n, groups);
    int rc;
    u32 stride = 12;
    if (n && (rc = mul_rows_dev(c, ENDO, scalars, points, encoded, w->rows_in, w->rows_out, encoded ? w->st_decode : nullptr, n, &stride))) return rc;
    const uint64_t* rows = w->rows_out;
    const uint8_t* st = encoded ? w->st_decode : nullptr;
    if ((rc = fold_planned(c, { w->part_a, w->part_b, w->st_a, w->st_b }, &rows, &stride, &st))) return rc;
    return launch_lower(c, encoded, rows, stride, st, (uint64_t*)out, status, groups);
}
// Host arrays (grouped_host): n rows in, `groups` rows out.  The shape is read under the lock, which grouped_host takes again around the copies.
static int ragged_host(fourq_ctx* c, const uint64_t* scalars, const void* points, bool encoded, void* out, uint8_t* status) {
    if (!c || !scalars || !points || !out || (encoded && !status)) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (c->shape.groups == 0) return FOURQ_ERR_INVALID;
    const size_t point_bytes = encoded ? 32 : 64;
    const GroupedArray arrays[] = { { scalars, nullptr, 32, true }, { points, nullptr, point_bytes, true }, { nullptr, out, point_bytes, false }, { nullptr, status, 1, false } };
    return grouped_host(c, c->shape.rows, c->shape.groups, arrays, encoded ? 4 : 3, [&](char* const* d) {
        return ragged_dev(c, (const uint64_t*)d[0], (const void*)d[1], encoded, (void*)d[2], encoded ? (uint8_t*)d[3] : nullptr);
    });
}
FQ_API int fourq_raggedsum_affine_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o) { return ragged_dev(c, s, p, false, o, nullptr); }
FQ_API int fourq_raggedsum_bytes_dev(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st) { return ragged_dev(c, s, p, true, o, st); }
FQ_API int fourq_raggedsum_affine(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o) { return ragged_host(c, s, p, false, o, nullptr); }
FQ_API int fourq_raggedsum_bytes(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st) { return ragged_host(c, s, p, true, o, st); }

// ---- the same sums by the bucket method (bucket.hip.h, bucket_layout.h): same arrays, same bytes, another route -------------------------
// window 0: the window measured fastest for the group size, or the ladder route where no window beat it by more than msm_dev's own run-to-run
// spread (profiles/bucket_sum_timing.txt: the ladder route up to one group of 2^18, 1.10 of it there; window 11 at 2^19, 0.72, and at 2^20,
// 0.52).  The threshold is the smallest MEASURED group size at which a window won; the table is indexed by group_size alone.
static const Threshold BUCKET_WINDOWS[] = { { 0, 0 }, { (size_t)1 << 19, 11 } };      // { smallest group_size, window }, ascending
FQ_API int fourq_bucketsum_window(size_t group_size) { return threshold_value(BUCKET_WINDOWS, group_size); }
static bool bucket_window_ok(unsigned window) { return window == 0 || fq_work::BucketGeom::window_ok(window); }
FQ_API int fourq_bucketsum_reserve(fourq_ctx* c, size_t groups, size_t group_size, unsigned window) {
    size_t n;
    const int rc = grouped_rows(c && bucket_window_ok(window), groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if (!window) window = (unsigned)fourq_bucketsum_window(group_size);
    if (!window) return reserve_for<fq_work::Msm>(c, n);
    return size_for<fq_work::Bucket>(c, false, groups, group_size, window);
}
// In constant-time selection mode the ladder route runs whatever the window is: a bucket's address is a digit of a scalar.
static int bucket_dev(fourq_ctx* c, const uint64_t* scalars, const void* points, bool encoded, void* out, uint8_t* status, size_t groups, size_t group_size, unsigned window) {
    size_t n;
    int rc = grouped_rows(c && scalars && points && out && (!encoded || status) && bucket_window_ok(window) && aligned16(scalars) && aligned16(points) && aligned16(out),
                          groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if (!window) window = (unsigned)fourq_bucketsum_window(group_size);
    if (c->ct || !window) return msm_dev(c, scalars, points, encoded, out, status, groups, group_size);
    WORK_SCOPE(w, Bucket, groups, group_size, window);
    if (encoded) {
        hipLaunchKernelGGL(decode_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, (const u64*)points, w->affine, w->st_decode, (u32)n);
        HIP_TRY(c, hipGetLastError());
    }
    HIPRC_TRY(c, chain_launch_bucket_sum(c->stream, *w, scalars, encoded ? w->affine : (const u64*)points, encoded ? w->st_decode : nullptr));
    return launch_lower(c, encoded, w->sum, 12, w->st_sum, (uint64_t*)out, status, groups);
}
FQ_API int fourq_bucketsum_affine_dev(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t groups, size_t group_size, unsigned window) { return bucket_dev(c, s, p, false, o, nullptr, groups, group_size, window); }
FQ_API int fourq_bucketsum_bytes_dev(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st, size_t groups, size_t group_size, unsigned window) { return bucket_dev(c, s, p, true, o, st, groups, group_size, window); }
FQ_API int fourq_bucketsum_affine(fourq_ctx* c, const uint64_t* s, const uint64_t* p, uint64_t* o, size_t groups, size_t group_size, unsigned window) {
    return sum_host(c, bucket_window_ok(window), s, p, false, o, nullptr, groups, group_size, [&](auto... staged) { return bucket_dev(c, staged..., groups, group_size, window); });
}
FQ_API int fourq_bucketsum_bytes(fourq_ctx* c, const uint64_t* s, const uint8_t* p, uint8_t* o, uint8_t* st, size_t groups, size_t group_size, unsigned window) {
    return sum_host(c, bucket_window_ok(window), s, p, true, o, st, groups, group_size, [&](auto... staged) { return bucket_dev(c, staged..., groups, group_size, window); });
}

// ---- commitments over a fixed generator set (commit.hip.h, commit_layout.h): out[g] = sum_j [k_gj]B_j, one comb per generator ------------
static_assert(fq_work::Commit::FOLD == MSM_FOLD, "commit_layout.h sizes the fold regions for msm_fold_kernel's segment");
// One comb per base, built where the single comb is (comb_table_kernel over the context's scratch slots, comb_unpack_kernel) and written
// into a NEW array: the old set is replaced only once the new one is complete, so a failure keeps it.  The staged single comb
// (comb_limbs, its shadow) is not touched; comb_packed is only the bounce row between the two kernels, as in fourq_comb_table.
// comb j of `combs` from the R1 row j of `r1` (device), on the context's stream; refused (host, or NULL: none): a slot with a non-zero byte
// gets an all-zero comb instead -- limbs that any addition may read
static int build_combs(fourq_ctx* c, const u64* r1, const uint8_t* refused, u32* combs, size_t m) {
    for (size_t j = 0; j < m; j++) {
        u32* comb = combs + j * COMB_POINTS * COMB_ENTRY_U32;
        if (refused && refused[j]) { HIP_TRY(c, hipMemsetAsync(comb, 0, (size_t)COMB_POINTS * COMB_ENTRY_U32 * sizeof(u32), c->stream)); continue; }
        hipLaunchKernelGGL(comb_table_kernel, dim3((COMB_POINTS + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, (const u64*)(r1 + 20 * j), c->scratch, c->comb_packed);
        HIP_TRY(c, hipGetLastError());
        hipLaunchKernelGGL(comb_unpack_kernel, dim3((COMB_POINTS + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, c->comb_packed, comb);
        HIP_TRY(c, hipGetLastError());
    }
    return FOURQ_OK;
}
FQ_API int fourq_commit_bases_set(fourq_ctx* c, const uint64_t* points_affine, size_t m) {
    if (!c || !points_affine || m == 0 || m > FOURQ_COMMIT_MAX_BASES) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (int rc = staging_allowed(c)) return rc;
    if (int rc = ensure_stage(c, m * (64 + 160))) return rc;
    u64* affine = (u64*)c->stage;
    u64* r1 = affine + 8 * m;
    u32* combs = nullptr;
    hipError_t e = hipMalloc(&combs, m * COMB_POINTS * COMB_ENTRY_U32 * sizeof(u32));
    if (e != hipSuccess) return fail(c, e, "hipMalloc(the combs of the generator set)");
    auto build = [&]() -> int {
        HIP_TRY(c, hipMemcpyAsync(affine, points_affine, m * 64, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(lift_affine_kernel, dim3((unsigned)((m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, affine, r1, (u32)m);
        HIP_TRY(c, hipGetLastError());
        if (int rc = build_combs(c, r1, nullptr, combs, m)) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return FOURQ_OK;
    };
    if (int rc = build()) { (void)hipStreamSynchronize(c->stream); (void)hipFree(combs); return rc; }
    if (c->commit_combs) (void)hipFree(c->commit_combs);      // the stream is idle: nothing reads the old set any more
    c->commit_combs = combs;
    c->commit_count = m;
    return FOURQ_OK;
}
FQ_API int fourq_commit_bases_count(const fourq_ctx* c, size_t* m) {
    if (!c || !m) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    *m = c->commit_count;
    return FOURQ_OK;
}
// route 0: the staged route from the smallest MEASURED number of groups at which it beat the gather route by more than the spread of msm_dev's
// own timings (profiles/commit_timing.txt: 1024 x 64, 0.1460 against 0.1494 ms, 2.3 % with a spread of 2.0 %; at 32768 x 2 and 65536 x 1 the two
// are within the spread, at 64 x 1024 and 1 x 4096 the gather route is 2.8 and 44 times faster), the gather route below; the table is indexed
// by `groups` alone, as BUCKET_WINDOWS is by group_size.
static const Threshold COMMIT_ROUTES[] = { { 0, 2 }, { 1024, 1 } };      // { smallest groups, route }, ascending
FQ_API int fourq_commit_route(size_t groups) { return threshold_value(COMMIT_ROUTES, groups); }
FQ_API int fourq_commit_reserve(fourq_ctx* c, size_t groups, size_t group_size) {
    size_t n;
    const int rc = grouped_rows(c != nullptr, groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    return size_for<fq_work::Commit>(c, false, groups, group_size);
}
// The combs into w->rows, the fold passes of the grouped sums until one row per group is left, the lowering: affine words, or the encoding.
static int commit_dev(fourq_ctx* c, const uint64_t* scalars, void* out, bool encoded, size_t groups, size_t group_size, int route) {
    size_t n;
    int rc = grouped_rows(c && scalars && out && route >= 0 && route <= 2 && aligned16(scalars) && aligned16(out), groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if (group_size > c->commit_count) return FOURQ_ERR_INVALID;     // no set: count 0
    if (!route) route = fourq_commit_route(groups);
    WORK_SCOPE(w, Commit, groups, group_size);
    if (c->ct) HIPRC_TRY(c, ct_launch_commit((unsigned)(c->lanes_w4 / BLOCK), c->stream, scalars, c->commit_combs, w->rows, groups, group_size));
    else HIPRC_TRY(c, chain_launch_commit(route, (unsigned)c->cus, c->stream, scalars, c->commit_combs, w->rows, groups, group_size));
    const uint64_t* rows = w->rows;
    const uint8_t* st = nullptr;
    u32 stride = 12;
    if ((rc = fold_to_one_row(c, { w->part_a, w->part_b, nullptr, nullptr }, groups, group_size, &rows, &stride, &st))) return rc;
    if (!encoded) return launch_lower(c, false, rows, stride, nullptr, (uint64_t*)out, nullptr, groups);
    HIP_TRY(c, hipMemsetAsync(w->st_zero, 0, groups, c->stream));
    return launch_lower(c, true, rows, stride, w->st_zero, (uint64_t*)out, w->st_out, groups);
}
// Host arrays (grouped_host).  The set's size is read under the lock, as in commit_dev.
static int commit_arrays(fourq_ctx* c, const uint64_t* scalars, void* out, bool encoded, size_t groups, size_t group_size, int route) {
    size_t n;
    const int rc = grouped_rows(c && scalars && out && route >= 0 && route <= 2, groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if (group_size > c->commit_count) return FOURQ_ERR_INVALID;
    const GroupedArray arrays[] = { { scalars, nullptr, 32, true }, { nullptr, out, encoded ? (size_t)32 : 64, false } };
    return grouped_host(c, n, groups, arrays, 2, [&](char* const* d) { return commit_dev(c, (const uint64_t*)d[0], d[1], encoded, groups, group_size, route); });
}
FQ_API int fourq_commit_affine_dev(fourq_ctx* c, const uint64_t* s, uint64_t* o, size_t groups, size_t group_size, int route) { return commit_dev(c, s, o, false, groups, group_size, route); }
FQ_API int fourq_commit_bytes_dev(fourq_ctx* c, const uint64_t* s, uint8_t* o, size_t groups, size_t group_size, int route) { return commit_dev(c, s, o, true, groups, group_size, route); }
FQ_API int fourq_commit_affine(fourq_ctx* c, const uint64_t* s, uint64_t* o, size_t groups, size_t group_size, int route) { return commit_arrays(c, s, o, false, groups, group_size, route); }
FQ_API int fourq_commit_bytes(fourq_ctx* c, const uint64_t* s, uint8_t* o, size_t groups, size_t group_size, int route) { return commit_arrays(c, s, o, true, groups, group_size, route); }

// ---- signatures from bytes (include/fourq_amd.h): SHA-512 and the arithmetic modulo N on the device (sig.hip.h) around the comb, the
// ladder and the combiner.  Every intermediate -- H(sk), the nonce, the challenge, s / h / R as rows -- lives in the context's work buffer.
static bool sig_msgs_dev_ok(const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len) {
    if (msg_len > 0xffffffffu || (!msgs && stride != 0)) return false;
    return aligned16(msgs) && aligned16(lens);
}
// the host-pointer calls can look at the lengths: nothing above `stride` or FOURQ_SIG_MAX_MSG gets through.  A batch above the limit is
// refused here too: the call sites evaluate this before host_call has looked at n, and no caller has that many lengths.
static bool sig_msgs_host_ok(const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len, size_t n) {
    if ((!msgs && stride != 0) || n > FOURQ_MAX_BATCH) return false;
    if (!lens) return msg_len <= stride && msg_len <= FOURQ_SIG_MAX_MSG;
    for (size_t i = 0; i < n; i++) if (lens[i] > stride || lens[i] > FOURQ_SIG_MAX_MSG) return false;
    return true;
}
static double sig_kt_hash(size_t stride, int prefix_bytes) { return KT_SHA_BLOCK * (double)((stride + prefix_bytes + 17 + 127) / 128); }

FQ_API int fourq_sha512_batch_dev(fourq_ctx* c, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len, uint8_t* out64, size_t n) {
    if (!c || !out64 || n > FOURQ_MAX_BATCH || !aligned16(out64) || !sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    HIPRC_TRY(c, sig_launch_sha512(c->stream, SigMsgs{ msgs, stride, lens, (uint32_t)msg_len }, out64, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_sig_keygen_batch_dev(fourq_ctx* c, const uint8_t* sk32, const uint64_t* comb, uint8_t* pk32, size_t n) {
    if (!c || !sk32 || !pk32 || n > FOURQ_MAX_BATCH || !aligned16(sk32) || !aligned16(pk32)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    int rc = stage_comb(c, comb);
    if (rc) return rc;
    WORK_SCOPE(w, Sig, n);
    HIPRC_TRY(c, sig_launch_nonce(c->stream, false, sk32, SigMsgs{ nullptr, 0, nullptr, 0 }, w->a, nullptr, (u32)n));
    return comb_encode(c, w->a, w->affine, w->st_comb, pk32, n);      // [a]G; the projective neutral would need a = 0 mod N
}
FQ_API int fourq_sig_sign_batch_dev(fourq_ctx* c, const uint8_t* sk32, const uint8_t* pk32, const uint64_t* comb,
                                    const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len, uint8_t* sig64, size_t n) {
    if (!c || !sk32 || !pk32 || !sig64 || n > FOURQ_MAX_BATCH || !aligned16(sk32) || !aligned16(pk32) || !aligned16(sig64)) return FOURQ_ERR_INVALID;
    if (!sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    int rc = stage_comb(c, comb);
    if (rc) return rc;
    WORK_SCOPE(w, Sig, n);
    const SigMsgs m{ msgs, stride, lens, (uint32_t)msg_len };
    HIPRC_TRY(c, sig_launch_nonce(c->stream, true, sk32, m, w->a, w->r, (u32)n));
    if ((rc = comb_encode(c, w->r, w->affine, w->st_comb, w->r32, n))) return rc;
    HIPRC_TRY(c, sig_launch_finish(c->stream, w->r32, pk32, m, w->a, w->r, sig64, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_sig_verify_batch_dev(fourq_ctx* c, const uint8_t* pk32, const uint64_t* comb, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                                      const uint8_t* sig64, uint8_t* ok, uint8_t* status, size_t n) {
    if (!c || !pk32 || !sig64 || !ok || !status || n > FOURQ_MAX_BATCH || !aligned16(pk32) || !aligned16(sig64)) return FOURQ_ERR_INVALID;
    if (!sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    int rc = stage_comb(c, comb);
    if (rc) return rc;
    WORK_SCOPE(scope, SigVerify, n);
    const fq_work::SigTail& w = scope->sig;
    HIPRC_TRY(c, sig_launch_challenge(c->stream, KeyRows{ nullptr, pk32, nullptr, 0 }, SigMsgs{ msgs, stride, lens, (uint32_t)msg_len }, sig64, w.s, w.h, w.r32, w.pre, (u32)n));
    if ((rc = double_mul_dev(c, w.s, nullptr, w.h, pk32, true, COMBINE_VERIFY, (const uint8_t*)w.r32, nullptr, status, ok, n))) return rc;
    HIPRC_TRY(c, sig_launch_merge(c->stream, w.pre, ok, status, (u32)n));
    return FOURQ_OK;
}

// host-pointer twins: a message matrix is one more input array of `stride` bytes per element (absent when stride is 0), the lengths one of
// four (absent when NULL); the launch gets nullptr for an absent one, which is what the _dev call takes in its place.
FQ_API int fourq_sha512_batch(fourq_ctx* c, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len, uint8_t* out64, size_t n) {
    const HostCall d = { { { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { out64, 64 } }, { PR_SHA512, 0, sig_kt_hash(stride, 0) }, unit_w4_x4, nullptr, nullptr,
                         sig_msgs_host_ok(msgs, stride, lens, msg_len, n), stride };
    return host_call(c, n, d, [&](const Chunk& k) { return fourq_sha512_batch_dev(c, k.in<uint8_t>(0), stride, k.in<uint32_t>(1), msg_len, k.out<uint8_t>(0), k.m); });
}
FQ_API int fourq_sig_keygen_batch(fourq_ctx* c, const uint8_t* sk32, const uint64_t* comb, uint8_t* pk32, size_t n) {
    const HostCall d = { { { sk32, 32 } }, { { pk32, 32 } }, { PR_SIG_KEYGEN, 0, KT_COMB + KT_SHA_BLOCK + KT_ENCODE }, unit_w4, nullptr, reserve_for<fq_work::Sig> };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& k) { return fourq_sig_keygen_batch_dev(c, k.in<uint8_t>(0), nullptr, k.out<uint8_t>(0), k.m); });
}
FQ_API int fourq_sig_sign_batch(fourq_ctx* c, const uint8_t* sk32, const uint8_t* pk32, const uint64_t* comb,
                                const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len, uint8_t* sig64, size_t n) {
    const double kt = KT_COMB + KT_ENCODE + KT_SHA_BLOCK + sig_kt_hash(stride, 32) + sig_kt_hash(stride, 64);
    const HostCall d = { { { sk32, 32 }, { pk32, 32 }, { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { sig64, 64 } }, { PR_SIG_SIGN, 0, kt }, unit_w4, nullptr, reserve_for<fq_work::Sig>,
                         sig_msgs_host_ok(msgs, stride, lens, msg_len, n), stride };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& k) {
        return fourq_sig_sign_batch_dev(c, k.in<uint8_t>(0), k.in<uint8_t>(1), nullptr, k.in<uint8_t>(2), stride, k.in<uint32_t>(3), msg_len, k.out<uint8_t>(0), k.m);
    });
}
FQ_API int fourq_sig_verify_batch(fourq_ctx* c, const uint8_t* pk32, const uint64_t* comb, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                                  const uint8_t* sig64, uint8_t* ok, uint8_t* status, size_t n) {
    const HostCall d = { { { pk32, 32 }, { sig64, 64 }, { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { ok, 1 }, { status, 1 } },
                         { PR_SIG_VERIFY, 0, KT_DOUBLE + KT_DECODE + sig_kt_hash(stride, 64) }, pipe_chunk, nullptr, reserve_for<fq_work::SigVerify>,
                         sig_msgs_host_ok(msgs, stride, lens, msg_len, n), stride };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& k) {
        return fourq_sig_verify_batch_dev(c, k.in<uint8_t>(0), nullptr, k.in<uint8_t>(2), stride, k.in<uint32_t>(3), msg_len, k.in<uint8_t>(1), k.out<uint8_t>(0), k.out<uint8_t>(1), k.m);
    });
}

// ---- signatures of registered keys (include/fourq_amd.h; keyset.hip.h, keyset_layout.h): [s]G + [h]A_id with A_id as fixed as G ----------
// The set: decode (decode_kernel), the order check (keyset_order_kernel), AffineToR1, then one comb per accepted key where the commitment
// bases get theirs (build_combs).  Everything goes into NEW arrays, and the old set is replaced once they are complete.
FQ_API int fourq_keyset_set(fourq_ctx* c, const uint8_t* pk32, size_t m, uint8_t* key_status) {
    if (!c || !pk32 || m == 0 || m > FOURQ_KEYSET_MAX_KEYS) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (int rc = staging_allowed(c)) return rc;
    if (int rc = ensure_stage(c, m * (64 + 160))) return rc;
    u64* affine = (u64*)c->stage;
    u64* r1 = affine + 8 * m;
    u32* combs = nullptr;
    uint8_t* bytes = nullptr;
    hipError_t e = hipMalloc(&combs, m * COMB_POINTS * COMB_ENTRY_U32 * sizeof(u32));
    if (e == hipSuccess) e = hipMalloc(&bytes, m * 32 + fq_work::align256(m));
    if (e != hipSuccess) { if (combs) (void)hipFree(combs); return fail(c, e, "hipMalloc(the combs of the key set)"); }
    uint8_t* status = bytes + m * 32;
    std::vector<uint8_t> st(m);
    auto build = [&]() -> int {
        const unsigned grid = (unsigned)((m + BLOCK - 1) / BLOCK);
        HIP_TRY(c, hipMemcpyAsync(bytes, pk32, m * 32, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(decode_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, (const u64*)bytes, affine, status, (u32)m);
        HIP_TRY(c, hipGetLastError());
        HIPRC_TRY(c, chain_launch_keyset_order(c->stream, affine, status, (u32)m));
        hipLaunchKernelGGL(lift_affine_kernel, dim3(grid), dim3(BLOCK), 0, c->stream, affine, r1, (u32)m);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(st.data(), status, m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (int rc = build_combs(c, r1, st.data(), combs, m)) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return FOURQ_OK;
    };
    if (int rc = build()) { (void)hipStreamSynchronize(c->stream); (void)hipFree(combs); (void)hipFree(bytes); return rc; }
    if (c->keyset_combs) (void)hipFree(c->keyset_combs);      // the stream is idle: nothing reads the old set any more
    if (c->keyset_bytes) (void)hipFree(c->keyset_bytes);
    c->keyset_combs = combs;
    c->keyset_bytes = bytes;
    c->keyset_status = status;
    c->keyset_count = m;
    if (key_status) memcpy(key_status, st.data(), m);
    return FOURQ_OK;
}
FQ_API int fourq_keyset_count(const fourq_ctx* c, size_t* m) {
    if (!c || !m) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    *m = c->keyset_count;
    return FOURQ_OK;
}
FQ_API int fourq_keyset_reserve(fourq_ctx* c, size_t n) {
    if (!c || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    return reserve_for<fq_work::Keyset>(c, n);
}
// the host-pointer calls can look at the indices: one outside the set is an argument error there
static bool keyset_ids_host_ok(const fourq_ctx* c, const uint32_t* key_ids, size_t n) {
    if (!c || !key_ids || n > FOURQ_MAX_BATCH) return false;
    size_t count;
    { CtxGuard g(c); count = c->keyset_count; }
    for (size_t i = 0; i < n; i++) if (key_ids[i] >= count) return false;
    return true;
}
// Default mode: the two combs in one accumulator, then the lowering.  Constant-time selection: the rows' key bytes gathered by index, the
// existing route over them, and the set's statuses put on its result -- a gathered address would be a digit of l.
FQ_API int fourq_keyset_double_mul_bytes_dev(fourq_ctx* c, const uint64_t* k, const uint64_t* comb, const uint64_t* l, const uint32_t* key_ids, uint8_t* out32,
                                             uint8_t* status, size_t n) {
    if (!c) return FOURQ_ERR_INVALID;
    if (!k || !l || !key_ids || !out32 || !status || n > FOURQ_MAX_BATCH) return FOURQ_ERR_INVALID;
    if (!aligned16(k) || !aligned16(l) || !aligned16(key_ids) || !aligned16(out32)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    if (c->keyset_count == 0) return FOURQ_ERR_INVALID;
    int rc = stage_comb(c, comb);
    if (rc) return rc;
    WORK_SCOPE(w, Keyset, n);
    const u32 count = (u32)c->keyset_count;
    if (c->ct) {
        HIPRC_TRY(c, chain_launch_keyset_gather(c->stream, key_ids, c->keyset_bytes, count, w->pk32, (u32)n));
        if ((rc = double_mul_dev(c, k, nullptr, l, w->pk32, true, COMBINE_ENCODE, nullptr, out32, status, nullptr, n))) return rc;
        HIPRC_TRY(c, chain_launch_keyset_fix(c->stream, key_ids, c->keyset_status, count, (u64*)out32, nullptr, status, (u32)n));
        return FOURQ_OK;
    }
    HIPRC_TRY(c, chain_launch_keyset_comb(c->stream, k, l, key_ids, c->comb_limbs, c->keyset_combs, c->keyset_status, count, w->rows, w->pre, (u32)n));
    HIPRC_TRY(c, chain_launch_keyset_lower(c->stream, false, w->rows, w->pre, nullptr, (u64*)out32, nullptr, status, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_keyset_sig_verify_dev(fourq_ctx* c, const uint32_t* key_ids, const uint64_t* comb, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                                            const uint8_t* sig64, uint8_t* ok, uint8_t* status, size_t n) {
    if (!c) return FOURQ_ERR_INVALID;
    if (!key_ids || !sig64 || !ok || !status || n > FOURQ_MAX_BATCH || !aligned16(key_ids) || !aligned16(sig64)) return FOURQ_ERR_INVALID;
    if (!sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    if (c->keyset_count == 0) return FOURQ_ERR_INVALID;
    int rc = stage_comb(c, comb);
    if (rc) return rc;
    WORK_SCOPE(w, Keyset, n);
    const u32 count = (u32)c->keyset_count;
    if (c->ct) {
        HIPRC_TRY(c, chain_launch_keyset_gather(c->stream, key_ids, c->keyset_bytes, count, w->pk32, (u32)n));
        if ((rc = fourq_sig_verify_batch_dev(c, w->pk32, nullptr, msgs, stride, lens, msg_len, sig64, ok, status, n))) return rc;
        HIPRC_TRY(c, chain_launch_keyset_fix(c->stream, key_ids, c->keyset_status, count, nullptr, ok, status, (u32)n));
        return FOURQ_OK;
    }
    HIPRC_TRY(c, sig_launch_challenge(c->stream, KeyRows{ key_ids, c->keyset_bytes, c->keyset_status, count }, SigMsgs{ msgs, stride, lens, (uint32_t)msg_len }, sig64, w->s, w->h, w->r32,
                                      w->pre, (u32)n));
    HIPRC_TRY(c, chain_launch_keyset_comb(c->stream, w->s, w->h, key_ids, c->comb_limbs, c->keyset_combs, c->keyset_status, count, w->rows, nullptr, (u32)n));
    HIPRC_TRY(c, chain_launch_keyset_lower(c->stream, true, w->rows, w->pre, w->r32, nullptr, ok, status, (u32)n));
    return FOURQ_OK;
}
// host-pointer twins: key_ids is a 4-byte-per-row input in place of the key bytes
static int keyset_prepare(fourq_ctx* c, const uint64_t* comb) { return c->keyset_count == 0 ? FOURQ_ERR_INVALID : stage_comb(c, comb); }
FQ_API int fourq_keyset_double_mul_bytes(fourq_ctx* c, const uint64_t* k, const uint64_t* comb, const uint64_t* l, const uint32_t* key_ids, uint8_t* out32, uint8_t* status,
                                         size_t n) {
    const HostCall d = { { { k, 32 }, { l, 32 }, { key_ids, 4 } }, { { out32, 32 }, { status, 1 } }, { PR_KEYSET_DOUBLE, 0, 2 * KT_COMB + KT_ENCODE }, pipe_chunk, nullptr,
                         reserve_for<fq_work::Keyset>, keyset_ids_host_ok(c, key_ids, n) };
    return host_call(c, n, d, [&] { return keyset_prepare(c, comb); }, [&](const Chunk& x) {
        return fourq_keyset_double_mul_bytes_dev(c, x.in<uint64_t>(0), nullptr, x.in<uint64_t>(1), x.in<uint32_t>(2), x.out<uint8_t>(0), x.out<uint8_t>(1), x.m);
    });
}
FQ_API int fourq_keyset_sig_verify(fourq_ctx* c, const uint32_t* key_ids, const uint64_t* comb, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                                        const uint8_t* sig64, uint8_t* ok, uint8_t* status, size_t n) {
    const HostCall d = { { { key_ids, 4 }, { sig64, 64 }, { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { ok, 1 }, { status, 1 } },
                         { PR_KEYSET_VERIFY, 0, 2 * KT_COMB + KT_ENCODE + sig_kt_hash(stride, 64) }, pipe_chunk, nullptr, reserve_for<fq_work::Keyset>,
                         sig_msgs_host_ok(msgs, stride, lens, msg_len, n) && keyset_ids_host_ok(c, key_ids, n), stride };
    return host_call(c, n, d, [&] { return keyset_prepare(c, comb); }, [&](const Chunk& x) {
        return fourq_keyset_sig_verify_dev(c, x.in<uint32_t>(0), nullptr, x.in<uint8_t>(2), stride, x.in<uint32_t>(3), msg_len, x.in<uint8_t>(1), x.out<uint8_t>(0), x.out<uint8_t>(1), x.m);
    });
}

// ---- bytes to a point (include/fourq_amd.h, "hash to curve"): expand_message_xmd + hash_to_field in one kernel, the map, the addition, the
// x392 chain and the lowering in a second (h2c.hip.h).  The only intermediate is u: n x count rows of 32 bytes in the context's work buffer.
// DST_prime travels in the kernel arguments, so nothing is staged and every _dev call below only enqueues once the work buffer is sized.
static bool h2c_args_ok(const uint8_t* dst, size_t dst_len, int mode) {
    return dst && dst_len >= 1 && dst_len <= FOURQ_H2C_MAX_DST && (mode == FOURQ_H2C_RO || mode == FOURQ_H2C_NU);
}
static double h2c_kt_hash(size_t stride, size_t dst_len, int count) {
    return KT_SHA_BLOCK * (double)((stride + dst_len + 4 + 17 + 127) / 128 + count * ((64 + dst_len + 2 + 17 + 127) / 128));
}
FQ_API int fourq_hash_to_field_batch_dev(fourq_ctx* c, const uint8_t* dst, size_t dst_len, int mode, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                                         uint64_t* out_u, size_t n) {
    if (!c || !out_u || n > FOURQ_MAX_BATCH || !aligned16(out_u) || !h2c_args_ok(dst, dst_len, mode) || !sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    const int count = mode == FOURQ_H2C_RO ? 2 : 1;
    HIPRC_TRY(c, h2c_launch_h2f(c->stream, count, nullptr, SigMsgs{ msgs, stride, lens, (uint32_t)msg_len }, h2c_make_dst(dst, dst_len, count), out_u, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_map_to_curve_batch_dev(fourq_ctx* c, const uint64_t* u, uint64_t* out_affine, size_t n) {
    if (!c || !u || !out_affine || n > FOURQ_MAX_BATCH || !aligned16(u) || !aligned16(out_affine)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    HIPRC_TRY(c, h2c_launch_ell2(c->stream, 1, H2C_OUT_MAP, u, out_affine, (u32)n));
    return FOURQ_OK;
}
static int hash_to_curve_dev(fourq_ctx* c, const uint8_t* dst, size_t dst_len, int mode, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                             int out_kind, void* out, size_t n) {
    if (!c || !out || n > FOURQ_MAX_BATCH || !aligned16(out) || !h2c_args_ok(dst, dst_len, mode) || !sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, H2c, n);
    const int count = mode == FOURQ_H2C_RO ? 2 : 1;
    HIPRC_TRY(c, h2c_launch_h2f(c->stream, count, nullptr, SigMsgs{ msgs, stride, lens, (uint32_t)msg_len }, h2c_make_dst(dst, dst_len, count), w->u, (u32)n));
    HIPRC_TRY(c, h2c_launch_ell2(c->stream, count, out_kind, w->u, (uint64_t*)out, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_hash_to_curve_batch_dev(fourq_ctx* c, const uint8_t* dst, size_t dl, int mode, const uint8_t* m, size_t st, const uint32_t* ln, size_t ml, uint8_t* o, size_t n) { return hash_to_curve_dev(c, dst, dl, mode, m, st, ln, ml, H2C_OUT_BYTES, o, n); }
FQ_API int fourq_hash_to_curve_affine_batch_dev(fourq_ctx* c, const uint8_t* dst, size_t dl, int mode, const uint8_t* m, size_t st, const uint32_t* ln, size_t ml, uint64_t* o, size_t n) { return hash_to_curve_dev(c, dst, dl, mode, m, st, ln, ml, H2C_OUT_AFFINE, o, n); }
// host-pointer twins; what = 0: hash_to_field (out: count x 32 bytes per row), 1: 32-byte points, 2: affine words
static int h2c_host(fourq_ctx* c, int what, const uint8_t* dst, size_t dst_len, int mode, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len, void* out, size_t n) {
    const bool ok = h2c_args_ok(dst, dst_len, mode) && sig_msgs_host_ok(msgs, stride, lens, msg_len, n);
    const int count = mode == FOURQ_H2C_RO ? 2 : 1, nu = mode == FOURQ_H2C_NU ? 1 : 0;
    const double kt_hash = h2c_kt_hash(stride, dst_len, count), kt_map = count * KT_ELL2 + KT_LIFT_LOWER;
    const HostIn msg = { msgs, stride }, len = { lens, 4, MAY_BE_NULL };
    const HostCall field = { { msg, len }, { { out, (size_t)32 * count } }, { PR_H2F, 0, kt_hash }, unit_w4_x4, nullptr, nullptr, ok, stride };
    const HostCall curve = { { msg, len }, { { out, what == 1 ? (size_t)32 : (size_t)64 } }, { what == 1 ? PR_H2C : PR_H2C_AFFINE, nu, kt_hash + kt_map }, pipe_chunk, nullptr,
                             reserve_for<fq_work::H2c>, ok, stride };
    return host_call(c, n, what == 0 ? field : curve, [&](const Chunk& k) {
        if (what == 0) return fourq_hash_to_field_batch_dev(c, dst, dst_len, mode, k.in<uint8_t>(0), stride, k.in<uint32_t>(1), msg_len, k.out<uint64_t>(0), k.m);
        return hash_to_curve_dev(c, dst, dst_len, mode, k.in<uint8_t>(0), stride, k.in<uint32_t>(1), msg_len, what == 1 ? H2C_OUT_BYTES : H2C_OUT_AFFINE, k.out<void>(0), k.m);
    });
}
FQ_API int fourq_hash_to_field_batch(fourq_ctx* c, const uint8_t* dst, size_t dl, int mode, const uint8_t* m, size_t st, const uint32_t* ln, size_t ml, uint64_t* o, size_t n) { return h2c_host(c, 0, dst, dl, mode, m, st, ln, ml, o, n); }
FQ_API int fourq_hash_to_curve_batch(fourq_ctx* c, const uint8_t* dst, size_t dl, int mode, const uint8_t* m, size_t st, const uint32_t* ln, size_t ml, uint8_t* o, size_t n) { return h2c_host(c, 1, dst, dl, mode, m, st, ln, ml, o, n); }
FQ_API int fourq_hash_to_curve_affine_batch(fourq_ctx* c, const uint8_t* dst, size_t dl, int mode, const uint8_t* m, size_t st, const uint32_t* ln, size_t ml, uint64_t* o, size_t n) { return h2c_host(c, 2, dst, dl, mode, m, st, ln, ml, o, n); }
FQ_API int fourq_map_to_curve_batch(fourq_ctx* c, const uint64_t* u, uint64_t* out_affine, size_t n) {
    const HostCall d = { { { u, 32 } }, { { out_affine, 64 } }, { PR_H2C_MAP, 0, KT_ELL2 + KT_LIFT_LOWER }, pipe_chunk };
    return host_call(c, n, d, [&](const Chunk& k) { return fourq_map_to_curve_batch_dev(c, k.in<uint64_t>(0), k.out<uint64_t>(0), k.m); });
}

// ---- oblivious PRF (include/fourq_amd.h, "oblivious PRF"): the hash-to-curve stages, the ladders with affine / encoded I/O, DH_endo and the
// lowering above, strung together with the inversion modulo N, the key broadcast and the finalisation hash of oprf.hip.h.  Every
// intermediate -- G(msg), the inverted blind, the unblinded element -- lives in the context's work buffer (work_layout.h, Oprf*).
// Elements per inversion: one while the batch is at most one wave per SIMD (the chain's latency is the time either way), 8 up to eight
// times that, 16 beyond (the chain is shared by more elements once there are lanes enough to fill the chip).  fourq_ctx_set_scinv_group (a test hook) forces it.
static int scinv_group(const fourq_ctx* c, size_t n) {
    if (c->scinv_k) return c->scinv_k;
    const size_t wave_per_simd = (size_t)c->cus * BLOCK;
    return n <= wave_per_simd ? 1 : n <= 8 * wave_per_simd ? OPRF_SCINV_K_MID : OPRF_SCINV_K_BIG;
}

// Test hook, gated like the routing variables (route_env): refused unless FOURQ_DEBUG_ROUTES=1 is set.  It is a call and not one more variable:
// the set of variables the library reads is pinned (tests/test_host.py).  k: 1, 8 or 16 elements per inversion, 0 = by batch size again.
FQ_API int fourq_ctx_set_scinv_group(fourq_ctx* c, int k) {
    const char* gate = getenv("FOURQ_DEBUG_ROUTES");
    if (!c || !gate || atoi(gate) == 0 || (k != 0 && k != 1 && k != OPRF_SCINV_K_MID && k != OPRF_SCINV_K_BIG)) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    c->scinv_k = k;
    return FOURQ_OK;
}
FQ_API int fourq_scalar_inv_batch_dev(fourq_ctx* c, const uint64_t* scalars, uint64_t* out, size_t n) {
    if (!c || !scalars || !out || n > FOURQ_MAX_BATCH || !aligned16(scalars) || !aligned16(out)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    HIPRC_TRY(c, oprf_launch_sc_inv(c->stream, scinv_group(c, n), scalars, out, nullptr, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_scalar_inv_batch(fourq_ctx* c, const uint64_t* scalars, uint64_t* out, size_t n) {
    const HostCall d = { { { scalars, 32 } }, { { out, 32 } }, { PR_SC_INV, 0, KT_SCINV }, unit_scinv };
    return host_call(c, n, d, [&](const Chunk& k) { return fourq_scalar_inv_batch_dev(c, k.in<uint64_t>(0), k.out<uint64_t>(0), k.m); });
}

FQ_API int fourq_oprf_blind_batch_dev(fourq_ctx* c, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                                      const uint64_t* blinds, uint8_t* out32, uint8_t* status, size_t n) {
    if (!c || !blinds || !out32 || !status || n > FOURQ_MAX_BATCH || !aligned16(blinds) || !aligned16(out32)) return FOURQ_ERR_INVALID;
    if (!h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) || !sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, OprfBlind, n);
    const SigMsgs m{ msgs, stride, lens, (uint32_t)msg_len };
    HIPRC_TRY(c, h2c_launch_h2f(c->stream, 2, nullptr, m, h2c_make_dst(dst, dst_len, 2), w->u, (u32)n));
    HIPRC_TRY(c, h2c_launch_ell2(c->stream, 2, H2C_OUT_AFFINE, w->u, w->pts, (u32)n));
    HIP_TRY(c, hipMemsetAsync(w->st_decode, 0, n, c->stream));              // the lowering reads a decode code per row: these points were never decoded
    u32 row_words;
    if (int rc = mul_rows_dev(c, ENDO, blinds, w->pts, false, w->rows_in, w->rows_out, nullptr, n, &row_words)) return rc;
    if (int rc = launch_lower(c, true, w->rows_out, row_words, w->st_decode, (uint64_t*)out32, status, n)) return rc;
    HIPRC_TRY(c, oprf_launch_blind_merge(c->stream, blinds, m, out32, status, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_oprf_evaluate_batch_dev(fourq_ctx* c, const uint64_t* key, const uint8_t* blinded32, uint8_t* out32, uint8_t* status, size_t n) {
    if (!c || !key || !blinded32 || !out32 || !status || n > FOURQ_MAX_BATCH || !aligned16(blinded32) || !aligned16(out32)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, OprfEvaluate, n);
    HIPRC_TRY(c, oprf_launch_fill_key(c->stream, key, w->keys, (u32)n));
    return dh_bytes_dev(c, ENDO, w->keys, blinded32, nullptr, out32, status, n);     // carves DhBytes at the buffer's start: w->dh
}
FQ_API int fourq_oprf_finalize_batch_dev(fourq_ctx* c, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                                         const uint64_t* blinds, const uint8_t* evaluated32, uint8_t* out64, uint8_t* status, size_t n) {
    if (!c || !blinds || !evaluated32 || !out64 || !status || n > FOURQ_MAX_BATCH || !aligned16(blinds) || !aligned16(evaluated32) || !aligned16(out64)) return FOURQ_ERR_INVALID;
    if (!h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) || !sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, OprfFinalize, n);
    HIPRC_TRY(c, oprf_launch_sc_inv(c->stream, scinv_group(c, n), blinds, w->inv, w->st_zero, (u32)n));
    u32 row_words;
    if (int rc = mul_rows_dev(c, ENDO, w->inv, evaluated32, true, w->rows_in, w->rows_out, w->st_decode, n, &row_words)) return rc;
    if (int rc = launch_lower(c, true, w->rows_out, row_words, w->st_decode, w->e32, w->st_lower, n)) return rc;
    HIPRC_TRY(c, oprf_launch_final(c->stream, (const uint8_t*)w->e32, SigMsgs{ msgs, stride, lens, (uint32_t)msg_len }, sha_make_tail("Finalize", 8, dst, dst_len), w->st_lower, w->st_zero,
                                   out64, status, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_oprf_eval_batch_dev(fourq_ctx* c, const uint64_t* key, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride, const uint32_t* lens,
                                     size_t msg_len, uint8_t* out64, uint8_t* status, size_t n) {
    if (!c || !key || !out64 || !status || n > FOURQ_MAX_BATCH || !aligned16(out64)) return FOURQ_ERR_INVALID;
    if (!h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) || !sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    WORK_SCOPE(w, OprfEval, n);
    const SigMsgs m{ msgs, stride, lens, (uint32_t)msg_len };
    HIPRC_TRY(c, h2c_launch_h2f(c->stream, 2, nullptr, m, h2c_make_dst(dst, dst_len, 2), w->u, (u32)n));
    HIPRC_TRY(c, h2c_launch_ell2(c->stream, 2, H2C_OUT_AFFINE, w->u, w->pts, (u32)n));
    HIPRC_TRY(c, oprf_launch_fill_key(c->stream, key, w->keys, (u32)n));
    if (int rc = dh_dev(c, ENDO, w->keys, w->pts, nullptr, w->shared, w->st_dh, n)) return rc;
    if (int rc = fourq_encode_batch_dev(c, w->shared, (uint8_t*)w->e32, n)) return rc;
    HIPRC_TRY(c, oprf_launch_final(c->stream, (const uint8_t*)w->e32, m, sha_make_tail("Finalize", 8, dst, dst_len), w->st_dh, nullptr, out64, status, (u32)n));
    return FOURQ_OK;
}
// host-pointer twins
static double oprf_kt_final(size_t stride, size_t dst_len) { return KT_SHA_BLOCK * (double)((32 + stride + 9 + dst_len + 17 + 127) / 128); }
FQ_API int fourq_oprf_blind_batch(fourq_ctx* c, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                                  const uint64_t* blinds, uint8_t* out32, uint8_t* status, size_t n) {
    const double kt = h2c_kt_hash(stride, dst_len, 2) + 2 * KT_ELL2 + KT_ENDO_VAR + 2 * KT_LIFT_LOWER;
    const HostCall d = { { { blinds, 32 }, { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { out32, 32 }, { status, 1 } }, { PR_OPRF_BLIND, 0, kt }, pipe_chunk, nullptr,
                         reserve_for<fq_work::OprfBlind>, h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) && sig_msgs_host_ok(msgs, stride, lens, msg_len, n), stride };
    return host_call(c, n, d, [&](const Chunk& k) {
        return fourq_oprf_blind_batch_dev(c, dst, dst_len, k.in<uint8_t>(1), stride, k.in<uint32_t>(2), msg_len, k.in<uint64_t>(0), k.out<uint8_t>(0), k.out<uint8_t>(1), k.m);
    });
}
FQ_API int fourq_oprf_evaluate_batch(fourq_ctx* c, const uint64_t* key, const uint8_t* blinded32, uint8_t* out32, uint8_t* status, size_t n) {
    const HostCall d = { { { blinded32, 32 } }, { { out32, 32 }, { status, 1 } }, { PR_OPRF_EVALUATE, 0, KT_DH_VAR + KT_CODEC }, pipe_chunk, nullptr, reserve_for<fq_work::OprfEvaluate>,
                         key != nullptr };
    return host_call(c, n, d, [&](const Chunk& k) { return fourq_oprf_evaluate_batch_dev(c, key, k.in<uint8_t>(0), k.out<uint8_t>(0), k.out<uint8_t>(1), k.m); });
}
FQ_API int fourq_oprf_finalize_batch(fourq_ctx* c, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride, const uint32_t* lens, size_t msg_len,
                                     const uint64_t* blinds, const uint8_t* evaluated32, uint8_t* out64, uint8_t* status, size_t n) {
    const double kt = KT_SCINV + KT_ENDO_VAR + KT_LIFT_LOWER + KT_CODEC + oprf_kt_final(stride, dst_len);
    const HostCall d = { { { blinds, 32 }, { evaluated32, 32 }, { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { out64, 64 }, { status, 1 } }, { PR_OPRF_FINALIZE, 0, kt }, pipe_chunk, nullptr,
                         reserve_for<fq_work::OprfFinalize>, h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) && sig_msgs_host_ok(msgs, stride, lens, msg_len, n), stride };
    return host_call(c, n, d, [&](const Chunk& k) {
        return fourq_oprf_finalize_batch_dev(c, dst, dst_len, k.in<uint8_t>(2), stride, k.in<uint32_t>(3), msg_len, k.in<uint64_t>(0), k.in<uint8_t>(1), k.out<uint8_t>(0), k.out<uint8_t>(1), k.m);
    });
}
FQ_API int fourq_oprf_eval_batch(fourq_ctx* c, const uint64_t* key, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride, const uint32_t* lens,
                                 size_t msg_len, uint8_t* out64, uint8_t* status, size_t n) {
    const double kt = h2c_kt_hash(stride, dst_len, 2) + 2 * KT_ELL2 + KT_LIFT_LOWER + KT_DH_VAR + KT_ENCODE + oprf_kt_final(stride, dst_len);
    const HostCall d = { { { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { out64, 64 }, { status, 1 } }, { PR_OPRF_EVAL, 0, kt }, pipe_chunk, nullptr, reserve_for<fq_work::OprfEval>,
                         key && h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) && sig_msgs_host_ok(msgs, stride, lens, msg_len, n), stride };
    return host_call(c, n, d, [&](const Chunk& k) {
        return fourq_oprf_eval_batch_dev(c, key, dst, dst_len, k.in<uint8_t>(0), stride, k.in<uint32_t>(1), msg_len, k.out<uint8_t>(0), k.out<uint8_t>(1), k.m);
    });
}

// ---- batched DLEQ proofs (include/fourq_amd.h, "oblivious PRF: proofs"): that a batch was evaluated with the key behind pk32 ------------------
// Every curve operation is one of the calls above -- the grouped sum (M, Z and [s]M + [c]Z), [k]B + [l]P ([s]G + [c]pk), DH_endo and MUL_endo
// on encodings (Z = DH_endo(k, M), [r]M), the comb with its encoding ([r]G and the public key in one launch) -- and dleq.hip.h's kernels
// hash, reduce, split and compare in between: a composite layout (dleq_layout.h) by work_layout.h's rule.
// what every call asks of its context and DST; verify and reserve ask dleq_pair_ok too: verify's sum of two is a grouped sum over 2 x groups rows
static bool dleq_args_ok(const fourq_ctx* c, const uint8_t* dst, size_t dst_len) { return c && h2c_args_ok(dst, dst_len, FOURQ_H2C_RO); }
static bool dleq_pair_ok(size_t groups) { return groups <= FOURQ_MAX_BATCH / 2; }
FQ_API int fourq_dleq_reserve(fourq_ctx* c, size_t groups, size_t group_size) {
    size_t n;
    const int rc = grouped_rows(c && dleq_pair_ok(groups), groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    return size_for<fq_work::Dleq>(c, false, n, groups);
}
// d, then M32 = sum [d]C and (with_z) Z32 = sum [d]D with their statuses, from the public key's row at pk_dev
static int dleq_composites_stage(fourq_ctx* c, const fq_work::Dleq& w, const ShaTail& tail, const uint8_t* pk_dev, const uint8_t* blinded32, const uint8_t* evaluated32,
                                 uint8_t* m32, uint8_t* z32, bool with_z, size_t groups, size_t group_size) {
    const size_t n = groups * group_size;
    HIPRC_TRY(c, dleq_launch_composite(c->stream, pk_dev, blinded32, evaluated32, tail, w.d, (u32)group_size, (u32)n));
    if (int rc = msm_dev(c, w.d, blinded32, true, m32, w.st_m, groups, group_size)) return rc;
    return with_z ? msm_dev(c, w.d, evaluated32, true, z32, w.st_z, groups, group_size) : FOURQ_OK;
}
FQ_API int fourq_dleq_composites_dev(fourq_ctx* c, const uint8_t* dst, size_t dst_len, const uint8_t* pk32, const uint8_t* blinded32, const uint8_t* evaluated32,
                                     uint8_t* m32, uint8_t* z32, uint8_t* status, size_t groups, size_t group_size) {
    size_t n;
    int rc = grouped_rows(dleq_args_ok(c, dst, dst_len) && pk32 && blinded32 && evaluated32 && m32 && z32 && status && aligned16(blinded32) && aligned16(evaluated32) &&
                          aligned16(m32) && aligned16(z32), groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    WORK_SCOPE(w, Dleq, n, groups);
    HIPRC_TRY(c, oprf_launch_fill_key(c->stream, dleq_scalar_arg(pk32).w, w->pk, 1));
    if ((rc = dleq_composites_stage(c, *w, sha_make_tail("Composite", DLEQ_LABEL, dst, dst_len), (const uint8_t*)w->pk, blinded32, evaluated32, m32, z32, true, groups, group_size))) return rc;
    HIPRC_TRY(c, dleq_launch_composites_merge(c->stream, w->st_m, w->st_z, m32, z32, status, (u32)groups));
    return FOURQ_OK;
}
FQ_API int fourq_dleq_prove_dev(fourq_ctx* c, const uint64_t* key, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* blinded32, const uint8_t* evaluated32,
                                const uint64_t* nonces, uint8_t* proof64, uint8_t* status, size_t groups, size_t group_size) {
    size_t n;
    int rc = grouped_rows(dleq_args_ok(c, dst, dst_len) && key && blinded32 && evaluated32 && nonces && proof64 && status && aligned16(blinded32) && aligned16(evaluated32) &&
                          aligned16(nonces) && aligned16(proof64), groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if ((rc = stage_comb(c, comb))) return rc;
    WORK_SCOPE(w, Dleq, n, groups);
    uint8_t *m32 = (uint8_t*)w->m32, *z32 = (uint8_t*)w->z32, *t2 = (uint8_t*)w->t2, *t3 = (uint8_t*)w->t3;
    const uint8_t* pk_dev = t2 + 32 * groups;
    // r mod N on the groups' rows and K behind them: ONE comb launch gives every t2 and the public key
    HIPRC_TRY(c, dleq_launch_nonces(c->stream, key, nonces, w->sc_a, (u32)groups));
    HIPRC_TRY(c, oprf_launch_fill_key(c->stream, key, w->sc_b, (u32)groups));
    if ((rc = comb_encode(c, w->sc_a, w->affine, w->st_t2, t2, groups + 1))) return rc;
    if ((rc = dleq_composites_stage(c, *w, sha_make_tail("Composite", DLEQ_LABEL, dst, dst_len), pk_dev, blinded32, evaluated32, m32, nullptr, false, groups, group_size))) return rc;
    if ((rc = dh_bytes_dev(c, ENDO, w->sc_b, m32, nullptr, z32, w->st_z, groups))) return rc;                 // Z = DH_endo(k, M): D is hashed, never decoded
    if ((rc = mul_bytes_dev(c, ENDO, w->sc_a, m32, t3, w->st_t3, groups))) return rc;                        // t3 = encode([r]M)
    HIPRC_TRY(c, dleq_launch_prove(c->stream, pk_dev, m32, z32, t2, t3, sha_make_tail("Challenge", DLEQ_LABEL, dst, dst_len), key, w->sc_a, w->st_m, w->st_z, w->st_t3, proof64, status,
                                   (u32)groups));
    return FOURQ_OK;
}
FQ_API int fourq_dleq_verify_dev(fourq_ctx* c, const uint8_t* pk32, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* blinded32, const uint8_t* evaluated32,
                                 const uint8_t* proof64, uint8_t* ok, uint8_t* status, size_t groups, size_t group_size) {
    size_t n;
    int rc = grouped_rows(dleq_args_ok(c, dst, dst_len) && dleq_pair_ok(groups) && pk32 && blinded32 && evaluated32 && proof64 && ok && status && aligned16(blinded32) &&
                          aligned16(evaluated32) && aligned16(proof64), groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if ((rc = stage_comb(c, comb))) return rc;
    WORK_SCOPE(w, Dleq, n, groups);
    uint8_t *m32 = (uint8_t*)w->m32, *z32 = (uint8_t*)w->z32, *t2 = (uint8_t*)w->t2, *t3 = (uint8_t*)w->t3;
    const uint8_t* pk_dev = (const uint8_t*)w->pk;
    HIPRC_TRY(c, oprf_launch_fill_key(c->stream, dleq_scalar_arg(pk32).w, w->pk, (u32)groups));             // pk on every group's row: the point of [s]G + [c]pk
    if ((rc = dleq_composites_stage(c, *w, sha_make_tail("Composite", DLEQ_LABEL, dst, dst_len), pk_dev, blinded32, evaluated32, m32, z32, true, groups, group_size))) return rc;
    HIPRC_TRY(c, dleq_launch_split(c->stream, proof64, m32, z32, w->sc_a, w->sc_b, w->pair_sc, w->pair_pt, w->st_pre, (u32)groups));
    if ((rc = double_mul_dev(c, w->sc_a, nullptr, w->sc_b, pk_dev, true, COMBINE_ENCODE, nullptr, t2, w->st_t2, nullptr, groups))) return rc;       // t2' = [s]G + [c]pk
    if ((rc = msm_dev(c, w->pair_sc, w->pair_pt, true, t3, w->st_t3, groups, 2))) return rc;                                                     // t3' = [s]M + [c]Z
    HIPRC_TRY(c, dleq_launch_check(c->stream, pk_dev, m32, z32, t2, t3, sha_make_tail("Challenge", DLEQ_LABEL, dst, dst_len), w->sc_b, w->st_m, w->st_z, w->st_t2, w->st_pre, w->st_t3, ok, status,
                                   (u32)groups));
    return FOURQ_OK;
}
// Host arrays (grouped_host), the 32- and 64-byte rows listed first.  prove and verify stage the comb BEFORE the arrays and pass comb == NULL on.
FQ_API int fourq_dleq_composites(fourq_ctx* c, const uint8_t* dst, size_t dst_len, const uint8_t* pk32, const uint8_t* blinded32, const uint8_t* evaluated32, uint8_t* m32,
                                 uint8_t* z32, uint8_t* status, size_t groups, size_t group_size) {
    size_t n;
    const int rc = grouped_rows(dleq_args_ok(c, dst, dst_len) && pk32 && blinded32 && evaluated32 && m32 && z32 && status, groups, group_size, &n);
    if (rc || !n) return rc;
    const GroupedArray arrays[] = { { blinded32, nullptr, 32, true }, { evaluated32, nullptr, 32, true }, { nullptr, m32, 32, false }, { nullptr, z32, 32, false }, { nullptr, status, 1, false } };
    return grouped_host(c, n, groups, arrays, 5, [&](char* const* d) {
        return fourq_dleq_composites_dev(c, dst, dst_len, pk32, (uint8_t*)d[0], (uint8_t*)d[1], (uint8_t*)d[2], (uint8_t*)d[3], (uint8_t*)d[4], groups, group_size);
    });
}
FQ_API int fourq_dleq_prove(fourq_ctx* c, const uint64_t* key, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* blinded32, const uint8_t* evaluated32,
                            const uint64_t* nonces, uint8_t* proof64, uint8_t* status, size_t groups, size_t group_size) {
    size_t n;
    int rc = grouped_rows(dleq_args_ok(c, dst, dst_len) && key && blinded32 && evaluated32 && nonces && proof64 && status, groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if ((rc = stage_comb(c, comb))) return rc;
    const GroupedArray arrays[] = { { blinded32, nullptr, 32, true }, { evaluated32, nullptr, 32, true }, { nonces, nullptr, 32, false }, { nullptr, proof64, 64, false }, { nullptr, status, 1, false } };
    return grouped_host(c, n, groups, arrays, 5, [&](char* const* d) {
        return fourq_dleq_prove_dev(c, key, nullptr, dst, dst_len, (uint8_t*)d[0], (uint8_t*)d[1], (uint64_t*)d[2], (uint8_t*)d[3], (uint8_t*)d[4], groups, group_size);
    });
}
FQ_API int fourq_dleq_verify(fourq_ctx* c, const uint8_t* pk32, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* blinded32, const uint8_t* evaluated32,
                             const uint8_t* proof64, uint8_t* ok, uint8_t* status, size_t groups, size_t group_size) {
    size_t n;
    int rc = grouped_rows(dleq_args_ok(c, dst, dst_len) && dleq_pair_ok(groups) && pk32 && blinded32 && evaluated32 && proof64 && ok && status, groups, group_size, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if ((rc = stage_comb(c, comb))) return rc;
    const GroupedArray arrays[] = { { blinded32, nullptr, 32, true }, { evaluated32, nullptr, 32, true }, { proof64, nullptr, 64, false }, { nullptr, ok, 1, false }, { nullptr, status, 1, false } };
    return grouped_host(c, n, groups, arrays, 5, [&](char* const* d) {
        return fourq_dleq_verify_dev(c, pk32, nullptr, dst, dst_len, (uint8_t*)d[0], (uint8_t*)d[1], (uint8_t*)d[2], (uint8_t*)d[3], (uint8_t*)d[4], groups, group_size);
    });
}

// ---- verifiable random function (include/fourq_amd.h, "verifiable random function"): prove, verify, proof_to_hash under SchnorrQ keys ------
// Every curve operation is one of the calls above -- the Elligator map, MUL_endo on encodings (Gamma = [x]Hpt, [r]Hpt), the comb with its
// encoding ([r]G), [k]B + [l]P or its keyed sibling ([s]G + [c]Y), the grouped sum over groups of two ([s]Hpt + [c / 392]W) -- and
// vrf.hip.h's kernels hash, reduce, clear Gamma's cofactor, split and compare in between.  As the DLEQ proofs, a composite layout (vrf_layout.h).
static bool vrf_args_ok(const fourq_ctx* c, const uint8_t* dst, size_t dst_len) { return c && h2c_args_ok(dst, dst_len, FOURQ_H2C_RO); }
static bool vrf_pair_ok(size_t n) { return n <= FOURQ_MAX_BATCH / 2; }        // verify's sum of two is a grouped sum over 2 n rows
FQ_API int fourq_vrf_reserve(fourq_ctx* c, size_t n) {
    if (!c || !vrf_pair_ok(n)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    return reserve_for<fq_work::Vrf>(c, n);
}
// h32 = encode(hash to curve, RO, of pk32 || alpha): pk32 is a register prefix of the message loop, nothing is concatenated
static int vrf_hash_stage(fourq_ctx* c, const fq_work::Vrf& w, const uint8_t* pk32, const SigMsgs& m, const uint8_t* dst, size_t dst_len, size_t n) {
    HIPRC_TRY(c, h2c_launch_h2f(c->stream, 2, pk32, m, h2c_make_dst(dst, dst_len, 2), w.u, (u32)n));
    HIPRC_TRY(c, h2c_launch_ell2(c->stream, 2, H2C_OUT_BYTES, w.u, w.h32, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_vrf_prove_dev(fourq_ctx* c, const uint8_t* sk32, const uint8_t* pk32, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride,
                               const uint32_t* lens, size_t msg_len, uint8_t* proof96, size_t n) {
    if (!vrf_args_ok(c, dst, dst_len) || !sk32 || !pk32 || !proof96 || n > FOURQ_MAX_BATCH || !aligned16(sk32) || !aligned16(pk32) || !aligned16(proof96)) return FOURQ_ERR_INVALID;
    if (!sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    int rc = stage_comb(c, comb);
    if (rc) return rc;
    WORK_SCOPE(w, Vrf, n);
    uint8_t *h32 = (uint8_t*)w->h32, *g32 = (uint8_t*)w->g32, *t_u = (uint8_t*)w->u32, *t_v = (uint8_t*)w->v32;
    if ((rc = vrf_hash_stage(c, *w, pk32, SigMsgs{ msgs, stride, lens, (uint32_t)msg_len }, dst, dst_len, n))) return rc;
    HIPRC_TRY(c, vrf_launch_scalars(c->stream, sk32, h32, w->sc_a, w->sc_b, (u32)n));                          // x and r
    if ((rc = comb_encode(c, w->sc_b, w->affine, w->st_u, t_u, n))) return rc;                                // u32 = encode([r]G)
    if ((rc = mul_bytes_dev(c, ENDO, w->sc_a, h32, g32, w->st_a, n))) return rc;                             // gamma32 = encode([x]Hpt)
    if ((rc = mul_bytes_dev(c, ENDO, w->sc_b, h32, t_v, w->st_b, n))) return rc;                             // v32 = encode([r]Hpt)
    HIPRC_TRY(c, vrf_launch_prove(c->stream, pk32, h32, g32, t_u, t_v, sha_make_tail("VrfVerify", DLEQ_LABEL, dst, dst_len), w->sc_a, w->sc_b, proof96, (u32)n));
    return FOURQ_OK;
}
// Both verify calls.  key_ids == NULL: the keys are the rows of pk32.  Otherwise the rows' key bytes are gathered by index (the hashes read
// them exactly as registered), and [s]G + [c]Y goes through the two combs -- or, with constant-time selection, through the unkeyed route on
// the gathered bytes; the check kernel puts the key set's statuses in front of every other.
static int vrf_verify_dev(fourq_ctx* c, const uint8_t* pk32, const uint32_t* key_ids, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride,
                          const uint32_t* lens, size_t msg_len, const uint8_t* proof96, uint8_t* beta64, uint8_t* ok, uint8_t* status, size_t n) {
    const void* keys = key_ids ? (const void*)key_ids : (const void*)pk32;
    if (!vrf_args_ok(c, dst, dst_len) || !keys || !proof96 || !beta64 || !ok || !status || !vrf_pair_ok(n) || !aligned16(keys) || !aligned16(proof96) || !aligned16(beta64))
        return FOURQ_ERR_INVALID;
    if (!sig_msgs_dev_ok(msgs, stride, lens, msg_len)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    if (key_ids && c->keyset_count == 0) return FOURQ_ERR_INVALID;
    int rc = stage_comb(c, comb);
    if (rc) return rc;
    WORK_SCOPE(w, Vrf, n);
    uint8_t *h32 = (uint8_t*)w->h32, *w32 = (uint8_t*)w->g32, *t_u = (uint8_t*)w->u32, *t_v = (uint8_t*)w->v32;
    const SigMsgs m{ msgs, stride, lens, (uint32_t)msg_len };
    const u32 count = (u32)c->keyset_count;
    if (key_ids) {
        HIPRC_TRY(c, chain_launch_keyset_gather(c->stream, key_ids, c->keyset_bytes, count, (uint8_t*)w->pk32, (u32)n));
        pk32 = (const uint8_t*)w->pk32;
    }
    if ((rc = vrf_hash_stage(c, *w, pk32, m, dst, dst_len, n))) return rc;
    HIPRC_TRY(c, vrf_launch_gamma(c->stream, proof96, h32, w->g32, w->sc_a, w->sc_b, w->pair_sc, w->pair_pt, w->st_a, w->st_pre, (u32)n));
    if (key_ids && !c->ct) rc = fourq_keyset_double_mul_bytes_dev(c, w->sc_a, nullptr, w->sc_b, key_ids, t_u, w->st_u, n);                  // u32' = [s]G + [c]A_id
    else rc = double_mul_dev(c, w->sc_a, nullptr, w->sc_b, pk32, true, COMBINE_ENCODE, nullptr, t_u, w->st_u, nullptr, n);                 // u32' = [s]G + [c]Y
    if (rc) return rc;
    if ((rc = msm_dev(c, w->pair_sc, w->pair_pt, true, t_v, w->st_v, n, 2))) return rc;                                                   // v32' = [s]Hpt + [c / 392]W
    const KeyRows set = { key_ids, c->keyset_bytes, c->keyset_status, count };
    HIPRC_TRY(c, vrf_launch_check(c->stream, pk32, h32, proof96, w32, t_u, t_v, sha_make_tail("VrfVerify", DLEQ_LABEL, dst, dst_len), sha_make_tail("VrfOutput", DLEQ_LABEL, dst, dst_len), w->sc_b, set, m,
                                  w->st_u, w->st_a, w->st_pre, w->st_v, beta64, ok, status, (u32)n));
    return FOURQ_OK;
}
FQ_API int fourq_vrf_verify_dev(fourq_ctx* c, const uint8_t* pk32, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride, const uint32_t* lens,
                                size_t msg_len, const uint8_t* proof96, uint8_t* beta64, uint8_t* ok, uint8_t* status, size_t n) {
    return vrf_verify_dev(c, pk32, nullptr, comb, dst, dst_len, msgs, stride, lens, msg_len, proof96, beta64, ok, status, n);
}
FQ_API int fourq_vrf_verify_keyed_dev(fourq_ctx* c, const uint32_t* key_ids, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride,
                                       const uint32_t* lens, size_t msg_len, const uint8_t* proof96, uint8_t* beta64, uint8_t* ok, uint8_t* status, size_t n) {
    if (!key_ids) return FOURQ_ERR_INVALID;
    return vrf_verify_dev(c, nullptr, key_ids, comb, dst, dst_len, msgs, stride, lens, msg_len, proof96, beta64, ok, status, n);
}
FQ_API int fourq_vrf_proof_to_hash_dev(fourq_ctx* c, const uint8_t* dst, size_t dst_len, const uint8_t* proof96, uint8_t* beta64, uint8_t* status, size_t n) {
    if (!vrf_args_ok(c, dst, dst_len) || !proof96 || !beta64 || !status || n > FOURQ_MAX_BATCH || !aligned16(proof96) || !aligned16(beta64)) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    HIPRC_TRY(c, vrf_launch_proof_to_hash(c->stream, proof96, sha_make_tail("VrfOutput", DLEQ_LABEL, dst, dst_len), beta64, status, (u32)n));
    return FOURQ_OK;
}
// host-pointer twins: copy in, the _dev call, copy out, through the pipeline's chunks; the comb is staged once, before the arrays
static double vrf_kt_hash(size_t stride, size_t dst_len) { return h2c_kt_hash(stride + 32, dst_len, 2) + 2 * KT_ELL2 + KT_LIFT_LOWER + KT_SHA_BLOCK * (double)(2 + (160 + dst_len + 27 + 127) / 128); }
FQ_API int fourq_vrf_prove(fourq_ctx* c, const uint8_t* sk32, const uint8_t* pk32, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride,
                           const uint32_t* lens, size_t msg_len, uint8_t* proof96, size_t n) {
    const double kt = vrf_kt_hash(stride, dst_len) + KT_COMB + KT_ENCODE + 2 * (KT_ENDO_VAR + KT_LIFT_LOWER + KT_CODEC);
    const HostCall d = { { { sk32, 32 }, { pk32, 32 }, { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { proof96, 96 } }, { PR_VRF_PROVE, 0, kt }, pipe_chunk, nullptr,
                         reserve_for<fq_work::Vrf>, h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) && sig_msgs_host_ok(msgs, stride, lens, msg_len, n), stride };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& k) {
        return fourq_vrf_prove_dev(c, k.in<uint8_t>(0), k.in<uint8_t>(1), nullptr, dst, dst_len, k.in<uint8_t>(2), stride, k.in<uint32_t>(3), msg_len, k.out<uint8_t>(0), k.m);
    });
}
FQ_API int fourq_vrf_verify(fourq_ctx* c, const uint8_t* pk32, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride, const uint32_t* lens,
                            size_t msg_len, const uint8_t* proof96, uint8_t* beta64, uint8_t* ok, uint8_t* status, size_t n) {
    const double kt = vrf_kt_hash(stride, dst_len) + KT_DOUBLE + KT_DECODE + 2 * (KT_ENDO_VAR + KT_DECODE) + KT_LIFT_LOWER;
    const HostCall d = { { { pk32, 32 }, { proof96, 96 }, { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { beta64, 64 }, { ok, 1 }, { status, 1 } }, { PR_VRF_VERIFY, 0, kt },
                         pipe_chunk, nullptr, reserve_for<fq_work::Vrf>,
                         h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) && vrf_pair_ok(n) && sig_msgs_host_ok(msgs, stride, lens, msg_len, n), stride };
    return host_call(c, n, d, [&] { return stage_comb(c, comb); }, [&](const Chunk& k) {
        return fourq_vrf_verify_dev(c, k.in<uint8_t>(0), nullptr, dst, dst_len, k.in<uint8_t>(2), stride, k.in<uint32_t>(3), msg_len, k.in<uint8_t>(1), k.out<uint8_t>(0),
                                    k.out<uint8_t>(1), k.out<uint8_t>(2), k.m);
    });
}
FQ_API int fourq_vrf_verify_keyed(fourq_ctx* c, const uint32_t* key_ids, const uint64_t* comb, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, size_t stride,
                                   const uint32_t* lens, size_t msg_len, const uint8_t* proof96, uint8_t* beta64, uint8_t* ok, uint8_t* status, size_t n) {
    const double kt = vrf_kt_hash(stride, dst_len) + 2 * KT_COMB + KT_ENCODE + 2 * (KT_ENDO_VAR + KT_DECODE) + KT_LIFT_LOWER;
    const HostCall d = { { { key_ids, 4 }, { proof96, 96 }, { msgs, stride }, { lens, 4, MAY_BE_NULL } }, { { beta64, 64 }, { ok, 1 }, { status, 1 } }, { PR_VRF_KEYED, 0, kt },
                         pipe_chunk, nullptr, reserve_for<fq_work::Vrf>,
                         h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) && vrf_pair_ok(n) && sig_msgs_host_ok(msgs, stride, lens, msg_len, n) && keyset_ids_host_ok(c, key_ids, n), stride };
    return host_call(c, n, d, [&] { return keyset_prepare(c, comb); }, [&](const Chunk& k) {
        return fourq_vrf_verify_keyed_dev(c, k.in<uint32_t>(0), nullptr, dst, dst_len, k.in<uint8_t>(2), stride, k.in<uint32_t>(3), msg_len, k.in<uint8_t>(1), k.out<uint8_t>(0),
                                           k.out<uint8_t>(1), k.out<uint8_t>(2), k.m);
    });
}
FQ_API int fourq_vrf_proof_to_hash(fourq_ctx* c, const uint8_t* dst, size_t dst_len, const uint8_t* proof96, uint8_t* beta64, uint8_t* status, size_t n) {
    const HostCall d = { { { proof96, 96 } }, { { beta64, 64 }, { status, 1 } }, { PR_VRF_HASH, 0, KT_DECODE + KT_LIFT_LOWER + KT_SHA_BLOCK * (double)((32 + dst_len + 27 + 127) / 128) },
                         unit_w4, nullptr, nullptr, h2c_args_ok(dst, dst_len, FOURQ_H2C_RO) };
    return host_call(c, n, d, [&](const Chunk& k) { return fourq_vrf_proof_to_hash_dev(c, dst, dst_len, k.in<uint8_t>(0), k.out<uint8_t>(0), k.out<uint8_t>(1), k.m); });
}

// ---- threshold sharing (include/fourq_amd.h, "threshold sharing"): deal, verify, Lagrange, combine -------------------------------------------
// The curve work is the calls above -- the grouped sum on encodings over groups of t, the comb with its encoding -- and shamir.hip.h's
// kernels evaluate, multiply and lay the operands out in between.  As the VRF, a composite layout (shamir_layout.h).
// The argument contract of every call: grouped_rows over (rows, t) -- the call's predicates, then rows == 0 is FOURQ_OK, then t == 0 or a
// product above FOURQ_MAX_BATCH is FOURQ_ERR_INVALID -- and t above FOURQ_SHAMIR_MAX_T refused with them.
static int shamir_rows(bool args_ok, size_t rows, size_t t, size_t* n) {
    const int rc = grouped_rows(args_ok, rows, t, n);
    if (rc == FOURQ_OK && *n && t > FOURQ_SHAMIR_MAX_T) { *n = 0; return FOURQ_ERR_INVALID; }
    return rc;
}
FQ_API int fourq_shamir_reserve(fourq_ctx* c, size_t rows, size_t t) {
    size_t n;
    const int rc = shamir_rows(c != nullptr, rows, t, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    return size_for<fq_work::Shamir>(c, false, rows, t);
}
FQ_API int fourq_shamir_shares_dev(fourq_ctx* c, const uint64_t* coeffs, const uint32_t* ids, uint64_t* shares, uint8_t* status, size_t n, size_t t, size_t m) {
    if (!c || !coeffs || !ids || !shares || !status || !aligned16(coeffs) || !aligned16(ids) || !aligned16(shares)) return FOURQ_ERR_INVALID;
    if (n == 0 || m == 0) return FOURQ_OK;
    size_t items, lanes;
    if (int rc = shamir_rows(true, n, t, &items)) return rc;
    if (int rc = grouped_rows(true, m, n, &lanes)) return rc;
    CtxGuard g(c);
    HIPRC_TRY(c, shamir_launch_shares(c->stream, coeffs, ids, shares, status, (u32)n, (u32)t, (u32)m));
    return FOURQ_OK;
}
FQ_API int fourq_shamir_lagrange_dev(fourq_ctx* c, const uint32_t* ids, uint64_t* lambda, uint8_t* status, size_t sets, size_t t) {
    size_t n;
    const int rc = shamir_rows(c && ids && lambda && status && aligned16(ids) && aligned16(lambda), sets, t, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    WORK_SCOPE(w, Shamir, sets, t);
    HIPRC_TRY(c, shamir_launch_lagrange(c->stream, ids, lambda, w->flags, status, (u32)sets, (u32)t));
    return FOURQ_OK;
}
FQ_API int fourq_shamir_combine_dev(fourq_ctx* c, const uint32_t* ids, const uint64_t* shares, uint64_t* out, uint8_t* status, size_t n, size_t t) {
    size_t items;
    const int rc = shamir_rows(c && ids && shares && out && status && aligned16(ids) && aligned16(shares) && aligned16(out), n, t, &items);
    if (rc || !items) return rc;
    CtxGuard g(c);
    WORK_SCOPE(w, Shamir, n, t);
    HIPRC_TRY(c, shamir_launch_lagrange(c->stream, ids, w->lambda, w->flags, w->st_set, 1, (u32)t));
    HIPRC_TRY(c, shamir_launch_combine(c->stream, w->lambda, shares, w->st_set, out, status, (u32)n, (u32)t));
    return FOURQ_OK;
}
FQ_API int fourq_shamir_combine_points_dev(fourq_ctx* c, const uint32_t* ids, const uint8_t* points32, uint8_t* out32, uint8_t* status, size_t n, size_t t) {
    size_t items;
    int rc = shamir_rows(c && ids && points32 && out32 && status && aligned16(ids) && aligned16(points32) && aligned16(out32), n, t, &items);
    if (rc || !items) return rc;
    CtxGuard g(c);
    WORK_SCOPE(w, Shamir, n, t);
    HIPRC_TRY(c, shamir_launch_lagrange(c->stream, ids, w->lambda, w->flags, w->st_set, 1, (u32)t));
    HIPRC_TRY(c, shamir_launch_fill(c->stream, w->lambda, points32, w->sc, w->pt, (u32)n, (u32)t));
    if ((rc = msm_dev(c, w->sc, w->pt, true, out32, status, n, t))) return rc;
    HIPRC_TRY(c, shamir_launch_set_merge(c->stream, w->st_set, out32, status, (u32)n));
    return FOURQ_OK;
}
// the verification shares of `groups` polynomials into out32 / status, the id 0 not yet merged: the powers, then the grouped sum over commits32 in place
static int shamir_public_stage(fourq_ctx* c, const fq_work::Shamir& w, const uint8_t* commits32, const uint32_t* ids, uint8_t* out32, uint8_t* status, size_t groups, size_t t) {
    HIPRC_TRY(c, shamir_launch_powers(c->stream, ids, w.sc, (u32)groups, (u32)t));
    return msm_dev(c, w.sc, commits32, true, out32, status, groups, t);
}
FQ_API int fourq_shamir_public_shares_dev(fourq_ctx* c, const uint8_t* commits32, const uint32_t* ids, uint8_t* out32, uint8_t* status, size_t groups, size_t t) {
    size_t n;
    int rc = shamir_rows(c && commits32 && ids && out32 && status && aligned16(commits32) && aligned16(ids) && aligned16(out32), groups, t, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    WORK_SCOPE(w, Shamir, groups, t);
    if ((rc = shamir_public_stage(c, *w, commits32, ids, out32, status, groups, t))) return rc;
    HIPRC_TRY(c, shamir_launch_id_merge(c->stream, ids, out32, status, (u32)groups));
    return FOURQ_OK;
}
FQ_API int fourq_shamir_verify_dev(fourq_ctx* c, const uint64_t* comb, const uint8_t* commits32, const uint32_t* ids, const uint64_t* shares, uint8_t* ok, uint8_t* status,
                                   size_t groups, size_t t) {
    size_t n;
    int rc = shamir_rows(c && commits32 && ids && shares && ok && status && aligned16(commits32) && aligned16(ids) && aligned16(shares), groups, t, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if ((rc = stage_comb(c, comb))) return rc;
    WORK_SCOPE(w, Shamir, groups, t);
    if ((rc = shamir_public_stage(c, *w, commits32, ids, (uint8_t*)w->pub32, w->st_pub, groups, t))) return rc;
    if ((rc = comb_encode(c, shares, w->affine, w->st_comb, (uint8_t*)w->g32, groups))) return rc;          // encode([share]G)
    HIPRC_TRY(c, shamir_launch_compare(c->stream, ids, w->pub32, w->g32, shares, w->st_pub, w->st_comb, ok, status, (u32)groups));
    return FOURQ_OK;
}
// Host arrays: copy in through the staging buffer, the _dev call, copy out, synchronise, in one piece (as grouped_host, whose arrays have one
// row per element or per group; these have their own extents).  `call` gets the device arrays in listed order, each 16-byte aligned.
struct ShamirArray { const void* in; void* out; size_t bytes; };
static int shamir_host(fourq_ctx* c, const ShamirArray* arrays, size_t count, const std::function<int(char* const*)>& call) {
    if (count > GROUPED_MAX_ARRAYS) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    size_t total = 0;
    for (size_t k = 0; k < count; k++) total += fq_work::align256(arrays[k].bytes);
    if (int rc = ensure_stage(c, total)) return rc;
    const fq_work::Hold stage_parent = c->stage_hold;
    c->stage_hold = stage_parent.opened("shamir_host's arrays", c->stage_bytes, c->stage_bytes);
    char* dev[GROUPED_MAX_ARRAYS] = {};
    auto staged = [&]() -> int {
        size_t used = 0;
        for (size_t k = 0; k < count; k++) {
            dev[k] = c->stage + used;
            if (arrays[k].in) HIP_TRY(c, hipMemcpyAsync(dev[k], arrays[k].in, arrays[k].bytes, hipMemcpyHostToDevice, c->stream));
            used += fq_work::align256(arrays[k].bytes);
        }
        if (int rc = call(dev)) return rc;
        for (size_t k = 0; k < count; k++)
            if (arrays[k].out) HIP_TRY(c, hipMemcpyAsync(arrays[k].out, dev[k], arrays[k].bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return FOURQ_OK;
    };
    const int rc = staged();
    c->stage_hold = stage_parent;
    if (rc != FOURQ_OK) (void)hipStreamSynchronize(c->stream);    // as grouped_host: nothing of this call may still read or write the caller's arrays
    return rc;
}
FQ_API int fourq_shamir_shares(fourq_ctx* c, const uint64_t* coeffs, const uint32_t* ids, uint64_t* shares, uint8_t* status, size_t n, size_t t, size_t m) {
    if (!c || !coeffs || !ids || !shares || !status) return FOURQ_ERR_INVALID;
    if (n == 0 || m == 0) return FOURQ_OK;
    size_t items, lanes;
    if (int rc = shamir_rows(true, n, t, &items)) return rc;
    if (int rc = grouped_rows(true, m, n, &lanes)) return rc;
    const ShamirArray arrays[] = { { coeffs, nullptr, items * 32 }, { ids, nullptr, m * 4 }, { nullptr, shares, lanes * 32 }, { nullptr, status, m } };
    return shamir_host(c, arrays, 4, [&](char* const* d) { return fourq_shamir_shares_dev(c, (uint64_t*)d[0], (uint32_t*)d[1], (uint64_t*)d[2], (uint8_t*)d[3], n, t, m); });
}
FQ_API int fourq_shamir_lagrange(fourq_ctx* c, const uint32_t* ids, uint64_t* lambda, uint8_t* status, size_t sets, size_t t) {
    size_t n;
    const int rc = shamir_rows(c && ids && lambda && status, sets, t, &n);
    if (rc || !n) return rc;
    const ShamirArray arrays[] = { { ids, nullptr, n * 4 }, { nullptr, lambda, n * 32 }, { nullptr, status, sets } };
    return shamir_host(c, arrays, 3, [&](char* const* d) { return fourq_shamir_lagrange_dev(c, (uint32_t*)d[0], (uint64_t*)d[1], (uint8_t*)d[2], sets, t); });
}
FQ_API int fourq_shamir_combine(fourq_ctx* c, const uint32_t* ids, const uint64_t* shares, uint64_t* out, uint8_t* status, size_t n, size_t t) {
    size_t items;
    const int rc = shamir_rows(c && ids && shares && out && status, n, t, &items);
    if (rc || !items) return rc;
    const ShamirArray arrays[] = { { ids, nullptr, t * 4 }, { shares, nullptr, items * 32 }, { nullptr, out, n * 32 }, { nullptr, status, 1 } };
    return shamir_host(c, arrays, 4, [&](char* const* d) { return fourq_shamir_combine_dev(c, (uint32_t*)d[0], (uint64_t*)d[1], (uint64_t*)d[2], (uint8_t*)d[3], n, t); });
}
FQ_API int fourq_shamir_combine_points(fourq_ctx* c, const uint32_t* ids, const uint8_t* points32, uint8_t* out32, uint8_t* status, size_t n, size_t t) {
    size_t items;
    const int rc = shamir_rows(c && ids && points32 && out32 && status, n, t, &items);
    if (rc || !items) return rc;
    const ShamirArray arrays[] = { { ids, nullptr, t * 4 }, { points32, nullptr, items * 32 }, { nullptr, out32, n * 32 }, { nullptr, status, n } };
    return shamir_host(c, arrays, 4, [&](char* const* d) { return fourq_shamir_combine_points_dev(c, (uint32_t*)d[0], (uint8_t*)d[1], (uint8_t*)d[2], (uint8_t*)d[3], n, t); });
}
FQ_API int fourq_shamir_public_shares(fourq_ctx* c, const uint8_t* commits32, const uint32_t* ids, uint8_t* out32, uint8_t* status, size_t groups, size_t t) {
    size_t n;
    const int rc = shamir_rows(c && commits32 && ids && out32 && status, groups, t, &n);
    if (rc || !n) return rc;
    const ShamirArray arrays[] = { { commits32, nullptr, n * 32 }, { ids, nullptr, groups * 4 }, { nullptr, out32, groups * 32 }, { nullptr, status, groups } };
    return shamir_host(c, arrays, 4, [&](char* const* d) { return fourq_shamir_public_shares_dev(c, (uint8_t*)d[0], (uint32_t*)d[1], (uint8_t*)d[2], (uint8_t*)d[3], groups, t); });
}
// the comb is staged BEFORE the arrays, and the _dev call gets comb == NULL (as fourq_dleq_verify)
FQ_API int fourq_shamir_verify(fourq_ctx* c, const uint64_t* comb, const uint8_t* commits32, const uint32_t* ids, const uint64_t* shares, uint8_t* ok, uint8_t* status, size_t groups,
                               size_t t) {
    size_t n;
    int rc = shamir_rows(c && commits32 && ids && shares && ok && status, groups, t, &n);
    if (rc || !n) return rc;
    CtxGuard g(c);
    if ((rc = stage_comb(c, comb))) return rc;
    const ShamirArray arrays[] = { { commits32, nullptr, n * 32 }, { ids, nullptr, groups * 4 }, { shares, nullptr, groups * 32 }, { nullptr, ok, groups }, { nullptr, status, groups } };
    return shamir_host(c, arrays, 5, [&](char* const* d) {
        return fourq_shamir_verify_dev(c, nullptr, (uint8_t*)d[0], (uint32_t*)d[1], (uint64_t*)d[2], (uint8_t*)d[3], (uint8_t*)d[4], groups, t);
    });
}

// ---- pinned host memory and transfer statistics of the host-pointer calls ---------------------------------------
FQ_API int fourq_host_alloc(fourq_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    HIP_TRY(c, hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault));
    return FOURQ_OK;
}
FQ_API int fourq_host_free(fourq_ctx* c, void* ptr) {
    if (!c) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    HIP_TRY(c, hipHostFree(ptr));
    return FOURQ_OK;
}
FQ_API int fourq_ctx_set_host_timing(fourq_ctx* c, int on) {
    if (!c) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    c->host_timing = on != 0;
    return FOURQ_OK;
}
// The shader clock the chip holds right now, from inside a kernel (MI355X_MICROARCH "DVFS give-back" item 6): a probe of FOURQ_DIAG_BLOCKS
// single-wave blocks on a stream of the context's own (not the one its kernels are enqueued on), each timing `window_us` of the 100 MHz
// counter in shader cycles.  Call it while the context's stream has work queued for longer than the window (the _dev calls only enqueue)
// and the answer is the clock under THAT load: what turns a time measured on one box into cycles comparable with another's.
namespace {
constexpr int DIAG_BLOCKS = 16;                     // consecutive workgroups go to consecutive XCDs: two probes on each of the eight
int diag_alloc(fourq_ctx* c) {
    if (!c->diag_stamps) HIP_TRY(c, hipMalloc(&c->diag_stamps, 2 * DIAG_BLOCKS * sizeof(u64)));      // kept: hipFree would wait for the whole device
    return FOURQ_OK;
}
int diag_reduce(fourq_ctx* c, double* mhz_median, double* mhz_min, double* mhz_max, double* window_us) {
    u64 host[2 * DIAG_BLOCKS];
    HIP_TRY(c, hipMemcpyAsync(host, c->diag_stamps, sizeof host, hipMemcpyDeviceToHost, c->copy_out));
    HIP_TRY(c, hipStreamSynchronize(c->copy_out));
    double mhz[DIAG_BLOCKS], win = 0.0;
    for (int i = 0; i < DIAG_BLOCKS; i++) {
        mhz[i] = host[2 * i + 1] ? (double)host[2 * i] / ((double)host[2 * i + 1] / 100.0) : 0.0;
        win += (double)host[2 * i + 1] / 100.0 / DIAG_BLOCKS;
    }
    for (int i = 1; i < DIAG_BLOCKS; i++) for (int j = i; j > 0 && mhz[j] < mhz[j - 1]; j--) { const double t = mhz[j]; mhz[j] = mhz[j - 1]; mhz[j - 1] = t; }
    *mhz_median = 0.5 * (mhz[DIAG_BLOCKS / 2 - 1] + mhz[DIAG_BLOCKS / 2]);
    if (mhz_min) *mhz_min = mhz[0];
    if (mhz_max) *mhz_max = mhz[DIAG_BLOCKS - 1];
    if (window_us) *window_us = win;
    return FOURQ_OK;
}
}  // namespace
FQ_API int fourq_diag_clock(fourq_ctx* c, uint32_t window_us, double* mhz_median, double* mhz_min, double* mhz_max, int* under_load) {
    if (!c || !mhz_median || window_us == 0 || window_us > 1000000) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (int rc = diag_alloc(c)) return rc;
    // the end of the stream's backlog as it stands now: still pending when the window has closed = the window lay inside the load
    if (!c->diag_mark) HIP_TRY(c, hipEventCreateWithFlags(&c->diag_mark, hipEventDisableTiming));
    HIP_TRY(c, hipEventRecord(c->diag_mark, c->stream));
    hipLaunchKernelGGL(clock_probe_kernel, dim3(DIAG_BLOCKS), dim3(64), 0, c->copy_out, c->diag_stamps, (u64)window_us * 100u);
    HIP_TRY(c, hipGetLastError());
    int rc = diag_reduce(c, mhz_median, mhz_min, mhz_max, nullptr);
    // Was the context's stream still busy when the window closed?  If the backlog was shorter than the window -- or the probe shared a hardware
    // queue with the kernels and waited behind them -- it timed an idle chip: the caller must be able to tell.  (An event, not
    // hipStreamQuery: that one still answered hipErrorNotReady 19 ms after a 1 ms backlog had drained.)
    if (under_load) {
        const hipError_t q = hipEventQuery(c->diag_mark);
        if (q != hipSuccess && q != hipErrorNotReady) return fail(c, q, "hipEventQuery(diag_mark)");
        *under_load = q == hipErrorNotReady ? 1 : 0;
    }
    return rc;
}
// The bracket form: begin and stop each enqueue one launch of clock_stamp_kernel on the context's stream -- before and behind the work the
// caller enqueues in between, so the host never waits; end waits for the stream, pairs the stamps per CU and reduces.
namespace {
constexpr int DIAG_STAMP_BLOCKS = 1024;             // single-wave workgroups: about four per CU, so that (nearly) every CU is in both launches
int diag_stamp(fourq_ctx* c, int which) {
    if (!c->diag_bracket) HIP_TRY(c, hipMalloc(&c->diag_bracket, 2 * 3 * DIAG_STAMP_BLOCKS * sizeof(u64)));
    hipLaunchKernelGGL(clock_stamp_kernel, dim3(DIAG_STAMP_BLOCKS), dim3(64), 0, c->stream, c->diag_bracket + (size_t)which * 3 * DIAG_STAMP_BLOCKS);
    HIP_TRY(c, hipGetLastError());
    return FOURQ_OK;
}
}  // namespace
FQ_API int fourq_diag_clock_begin(fourq_ctx* c) {
    if (!c) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (c->diag_open) return FOURQ_ERR_INVALID;
    if (int rc = diag_stamp(c, 0)) return rc;
    c->diag_open = true;
    c->diag_stopped = false;
    return FOURQ_OK;
}
FQ_API int fourq_diag_clock_stop(fourq_ctx* c) {
    if (!c) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (!c->diag_open || c->diag_stopped) return FOURQ_ERR_INVALID;
    if (int rc = diag_stamp(c, 1)) return rc;
    c->diag_stopped = true;
    return FOURQ_OK;
}
FQ_API int fourq_diag_clock_end(fourq_ctx* c, double* mhz_median, double* mhz_min, double* mhz_max, double* window_us) {
    if (!c || !mhz_median) return FOURQ_ERR_INVALID;
    CtxGuard g(c);
    if (!c->diag_open) return FOURQ_ERR_INVALID;
    if (!c->diag_stopped) { if (int rc = diag_stamp(c, 1)) return rc; }
    c->diag_open = c->diag_stopped = false;
    std::vector<u64> h;
    try { h.resize(2 * 3 * DIAG_STAMP_BLOCKS); } catch (...) { return FOURQ_ERR_NOMEM; }
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->diag_bracket, h.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // one (memtime, memrealtime) pair per CU and launch -- the first block that landed on it; then per CU seen in both: cycles per 10 ns
    const u64 *a = h.data(), *b = h.data() + 3 * DIAG_STAMP_BLOCKS;
    std::vector<double> mhz;
    double win = 0.0;
    try {
        std::vector<std::pair<u64, int>> first;          // (CU key, block of the first launch)
        for (int i = 0; i < DIAG_STAMP_BLOCKS; i++) first.emplace_back(a[3 * i], i);
        std::sort(first.begin(), first.end());
        std::vector<bool> used(DIAG_STAMP_BLOCKS, false);
        for (int j = 0; j < DIAG_STAMP_BLOCKS; j++) {
            auto it = std::lower_bound(first.begin(), first.end(), std::make_pair(b[3 * j], 0));
            if (it == first.end() || it->first != b[3 * j]) continue;
            const int slot = (int)(it - first.begin());
            if (used[slot]) continue;                    // this CU is paired already
            used[slot] = true;
            const int i = it->second;
            const double ticks = (double)(b[3 * j + 2] - a[3 * i + 2]);
            if (ticks <= 0) continue;
            mhz.push_back((double)(b[3 * j + 1] - a[3 * i + 1]) / (ticks / 100.0));
            win += ticks / 100.0;
        }
    } catch (...) { return FOURQ_ERR_NOMEM; }
    if (mhz.size() < 8) { snprintf(c->err, sizeof c->err, "fourq_diag_clock_end: only %zu CUs were stamped by both launches", mhz.size()); return FOURQ_ERR_HIP; }
    std::sort(mhz.begin(), mhz.end());
    const size_t m = mhz.size();
    *mhz_median = 0.5 * (mhz[(m - 1) / 2] + mhz[m / 2]);
    if (mhz_min) *mhz_min = mhz[m / 20];                 // 5th and 95th percentile over the CUs: the spread of the chip's clock domains, not of stragglers
    if (mhz_max) *mhz_max = mhz[m - 1 - m / 20];
    if (window_us) *window_us = win / (double)m;
    return FOURQ_OK;
}
FQ_API int fourq_ctx_host_stats(const fourq_ctx* c, fourq_host_stats* out) {
    if (!c || !out) return FOURQ_ERR_INVALID;
    *out = c->host_stats;
    return FOURQ_OK;
}

FQ_API int fourq_ctx_host_chunk_stamps(const fourq_ctx* c, uint32_t chunk, double out_ms[6]) {
    if (!c || !out_ms) return FOURQ_ERR_INVALID;
    std::unique_lock<std::recursive_mutex> lock(c->mu);
    if ((size_t)chunk * 6 + 6 > c->chunk_stamps.size()) return FOURQ_ERR_INVALID;
    // event order in the pipeline: copy-in start, copy-in end, copy-out start, copy-out end, kernels start, kernels end
    for (int i = 0; i < 6; i++) out_ms[i] = c->chunk_stamps[(size_t)chunk * 6 + i];
    return FOURQ_OK;
}
FQ_API int fourq_ctx_host_stats_sized(const fourq_ctx* c, void* out, size_t size) {
    if (!c || !out) return FOURQ_ERR_INVALID;
    memcpy(out, &c->host_stats, size < sizeof c->host_stats ? size : sizeof c->host_stats);
    return FOURQ_OK;
}

FQ_API int fourq_prim_words(int op, size_t* in_words, size_t* out_words) {
    const PrimShape* p = find_prim(op);
    if (!p || !in_words || !out_words) return FOURQ_ERR_INVALID;
    *in_words = p->in_words; *out_words = p->out_words;
    return FOURQ_OK;
}
FQ_API int fourq_prim_batch(fourq_ctx* c, int op, const uint64_t* in, uint64_t* out, size_t n) {
    const PrimShape* p = find_prim(op);
    if (!c || !p || !in || !out || n > 0x7fffffffu) return FOURQ_ERR_INVALID;
    if (n == 0) return FOURQ_OK;
    CtxGuard g(c);
    size_t ib = n * p->in_words * 8, ob = n * p->out_words * 8;
    int rc = ensure_stage(c, ib + ob);
    if (rc) return rc;
    char* base = (char*)c->stage;
    HIP_TRY(c, hipMemcpyAsync(base, in, ib, hipMemcpyHostToDevice, c->stream));
    if (op == FOURQ_SC_REDUCE512 || op == FOURQ_SC_MULSUB || op == FOURQ_SC_MUL || op == FOURQ_SC_INV) {
        HIPRC_TRY(c, sig_launch_scalar_prim(c->stream, op, (const uint64_t*)base, (uint64_t*)(base + ib), (u32)n));
    } else if (op == FOURQ_PT_MAP_ELL2) {
        HIPRC_TRY(c, h2c_launch_ell2(c->stream, 1, H2C_OUT_MAP, (const uint64_t*)base, (uint64_t*)(base + ib), (u32)n));
    } else {
        hipLaunchKernelGGL(prim_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, op, (const u64*)base, (u64*)(base + ib),
                           (u32)n, (u32)p->in_words, (u32)p->out_words);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(out, base + ib, ob, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FOURQ_OK;
}

}  // extern "C"

// Second translation unit of libfourq_amd.so: the kernels that profit from chained carries (FQ_CHAIN=1, see
// kernels.hip.h): fixed-base ladders (table in LDS), the fixed-base comb and the batched normalisation.  Only launchers are exported to the other
// translation unit; the C ABI lives in fourq_amd.hip.  combine.hip.h adds the kernel that joins the comb's and the ladder's halves of [k]B + [l]P,
// msm.hip.h the ones that fold the ladder's rows of a group into one (equal lengths, and by descriptors), bucket.hip.h the bucket route of the same sums, commit.hip.h the combs of a
// fixed generator set, keyset.hip.h the two combs in one accumulator of a signature check over registered keys.
#ifndef FQ_CHAIN
#define FQ_CHAIN 1
#endif
#include "kernels.hip.h"
#include "combine.hip.h"
#include "msm.hip.h"
#include "bucket.hip.h"
#include "commit.hip.h"
#include "keyset.hip.h"

namespace fq {

namespace {
template <int ALGO, bool DH, bool DEFER> int launch(unsigned grid, hipStream_t stream, const LadderArgs& a) {
    hipLaunchKernelGGL((ladder_kernel<ALGO, LDS, DH, DEFER>), dim3(grid), dim3(BLOCK), 0, stream, a);
    return (int)hipGetLastError();
}
template <int ALGO> int launch_algo(bool dh, unsigned grid, hipStream_t stream, const LadderArgs& a) {
    if (!dh) return launch<ALGO, false, false>(grid, stream, a);
    return a.proj ? launch<ALGO, true, true>(grid, stream, a) : launch<ALGO, true, false>(grid, stream, a);
}
}  // namespace

int chain_launch_ladder(int algo, bool dh, unsigned grid, hipStream_t stream, const LadderArgs& a) {
    return algo == ENDO ? launch_algo<ENDO>(dh, grid, stream, a) : launch_algo<WINDOWED>(dh, grid, stream, a);
}
// The comb's table needs more dynamic LDS than the 64 KB a kernel gets by default: raised once per device, at context creation
// (a launch then only enqueues, so the _dev entry points stay capturable into a graph).
int chain_setup_device() {
    hipError_t e = hipFuncSetAttribute((const void*)comb_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)COMB_FAST_LDS_BYTES);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)comb_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)COMB_FAST_LDS_BYTES);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)commit_kernel<COMMIT_STAGED, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)COMB_FAST_LDS_BYTES);
    return (int)e;
}
// One block per CU holds the whole 144 KB table; its width follows the batch so that a small batch still reaches every CU.
int chain_launch_comb(unsigned cus, hipStream_t stream, const u64* scalars, const u32* comb_limbs, u64* out, uint8_t* status, uint4* proj, u32 proj_stride, u32 n) {
    unsigned width = 64;
    while (width < (unsigned)COMB_BLOCK_MAX && (size_t)width * cus < n) width *= 2;
    const unsigned blocks = (n + width - 1) / width, grid = blocks < cus ? blocks : cus;
    if (proj) hipLaunchKernelGGL(comb_kernel<true>, dim3(grid), dim3(width), COMB_FAST_LDS_BYTES, stream, scalars, comb_limbs, out, status, proj, proj_stride, n);
    else hipLaunchKernelGGL(comb_kernel<false>, dim3(grid), dim3(width), COMB_FAST_LDS_BYTES, stream, scalars, comb_limbs, out, status, proj, proj_stride, n);
    return (int)hipGetLastError();
}
int chain_launch_normalize(int k, hipStream_t stream, const uint4* proj, u32 proj_stride, u64* out, uint8_t* status, u32 n) {
    const unsigned grid = ((n + k - 1) / k + BLOCK - 1) / BLOCK;
    if (k == 8) hipLaunchKernelGGL(normalize_kernel<8>, dim3(grid), dim3(BLOCK), 0, stream, proj, proj_stride, out, status, n);
    else if (k == 4) hipLaunchKernelGGL(normalize_kernel<4>, dim3(grid), dim3(BLOCK), 0, stream, proj, proj_stride, out, status, n);
    else if (k == 2) hipLaunchKernelGGL(normalize_kernel<2>, dim3(grid), dim3(BLOCK), 0, stream, proj, proj_stride, out, status, n);
    else hipLaunchKernelGGL(normalize_kernel<1>, dim3(grid), dim3(BLOCK), 0, stream, proj, proj_stride, out, status, n);
    return (int)hipGetLastError();
}

namespace {
template <int OUT> int launch_combine(int k, hipStream_t stream, const uint4* proj, u32 proj_stride, const u64* rows, u32 row_stride, const uint8_t* st_decode,
                                      const u64* expect, u64* out, uint8_t* status, uint8_t* ok, u32 n) {
    const unsigned grid = ((n + k - 1) / k + BLOCK - 1) / BLOCK;
    if (k == 2) hipLaunchKernelGGL((combine_kernel<2, OUT>), dim3(grid), dim3(BLOCK), 0, stream, proj, proj_stride, rows, row_stride, st_decode, expect, out, status, ok, n);
    else hipLaunchKernelGGL((combine_kernel<1, OUT>), dim3(grid), dim3(BLOCK), 0, stream, proj, proj_stride, rows, row_stride, st_decode, expect, out, status, ok, n);
    return (int)hipGetLastError();
}
}  // namespace
// [k]B + [l]P from the two halves' projective results (combine.hip.h).  k: elements per inversion (1 or 2); out_kind: CombineOut
int chain_launch_combine(int k, int out_kind, hipStream_t stream, const uint4* proj, u32 proj_stride, const u64* rows, u32 row_stride, const uint8_t* st_decode,
                         const u64* expect, u64* out, uint8_t* status, uint8_t* ok, u32 n) {
    if (out_kind == COMBINE_AFFINE) return launch_combine<COMBINE_AFFINE>(k, stream, proj, proj_stride, rows, row_stride, st_decode, expect, out, status, ok, n);
    if (out_kind == COMBINE_ENCODE) return launch_combine<COMBINE_ENCODE>(k, stream, proj, proj_stride, rows, row_stride, st_decode, expect, out, status, ok, n);
    return launch_combine<COMBINE_VERIFY>(k, stream, proj, proj_stride, rows, row_stride, st_decode, expect, out, status, ok, n);
}
// One fold pass of a grouped sum (msm.hip.h).  A team is as wide as its segment is long, up to 16 lanes: a full segment of MSM_FOLD rows
// then costs a lane 3 + 4 dependent additions, and a group of two one.
int chain_launch_msm_fold(hipStream_t stream, const u64* rows, u32 stride, const uint8_t* st_in, u64* rows_out, uint8_t* st_out, size_t groups, size_t m_in) {
    const size_t m_out = (m_in + MSM_FOLD - 1) / MSM_FOLD, segment = m_in < MSM_FOLD ? m_in : MSM_FOLD;
    u32 team = 1;
    while (team < 16 && team < segment) team *= 2;
    const u64 teams = (u64)groups * m_out, blocks = (teams * team + BLOCK - 1) / BLOCK;
    if (blocks == 0 || blocks > 0x7fffffffu || m_in > 0xffffffffu) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(msm_fold_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, stream, rows, stride, st_in, rows_out, st_out, (u32)m_in, (u32)m_out, team,
                       (u32)((segment + team - 1) / team), teams);
    return (int)hipGetLastError();
}
// One planned pass of a ragged sum: the geometry is the plan's (fq_work::ShapePass), checked once more where it becomes a launch
int chain_launch_msm_fold_desc(hipStream_t stream, const u64* rows, u32 stride, const uint8_t* st_in, u64* rows_out, uint8_t* st_out, const uint2* desc, size_t teams,
                               u32 team, u32 iters) {
    const u64 blocks = ((u64)teams * team + BLOCK - 1) / BLOCK;
    if (!desc || blocks == 0 || blocks > 0x7fffffffu || teams > 0xffffffffu || team == 0 || team > 16 || (team & (team - 1)) || iters == 0 || (u64)team * iters > MSM_FOLD)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(msm_fold_desc_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, stream, rows, stride, st_in, rows_out, st_out, desc, team, iters, (u32)teams);
    return (int)hipGetLastError();
}
// The combs of a commitment (commit.hip.h): row g * group_size + j from comb j, canonical (X, Y, Z) rows.  route: COMMIT_STAGED or COMMIT_GATHER
int chain_launch_commit(int route, unsigned cus, hipStream_t stream, const u64* scalars, const u32* combs, u64* rows, size_t groups, size_t group_size) {
    if (route == COMMIT_GATHER) {
        const size_t blocks = (groups * group_size + BLOCK - 1) / BLOCK;
        if (blocks > 0x7fffffffu) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL((commit_kernel<COMMIT_GATHER, false>), dim3((unsigned)blocks), dim3(BLOCK), 0, stream, scalars, combs, rows, (u32)groups, (u32)group_size, 0u, 0u);
        return (int)hipGetLastError();
    }
    const fq_work::CommitGeom geom(groups, group_size, cus, COMB_BLOCK_MAX);
    hipLaunchKernelGGL((commit_kernel<COMMIT_STAGED, false>), dim3(geom.grid), dim3(geom.width), COMB_FAST_LDS_BYTES, stream, scalars, combs, rows, (u32)groups, (u32)group_size,
                       (u32)geom.slices, (u32)geom.items);
    return (int)hipGetLastError();
}

// Signatures of registered keys (keyset.hip.h).  Every grid follows from the row count.
int chain_launch_keyset_order(hipStream_t stream, const u64* affine, uint8_t* status, u32 m) {
    hipLaunchKernelGGL(keyset_order_kernel, dim3((m + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, affine, status, m);
    return (int)hipGetLastError();
}
int chain_launch_keyset_comb(hipStream_t stream, const u64* k, const u64* l, const u32* key_ids, const u32* comb_g, const u32* combs, const uint8_t* key_status, u32 count,
                             u64* rows, uint8_t* pre, u32 n) {
    hipLaunchKernelGGL(keyset_comb_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, k, l, key_ids, comb_g, combs, key_status, count, rows, pre, n);
    return (int)hipGetLastError();
}
int chain_launch_keyset_lower(hipStream_t stream, bool verify, const u64* rows, const uint8_t* pre, const u64* expect, u64* out, uint8_t* ok, uint8_t* status, u32 n) {
    if (verify) hipLaunchKernelGGL(keyset_lower_kernel<true>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, rows, pre, expect, out, ok, status, n);
    else hipLaunchKernelGGL(keyset_lower_kernel<false>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, rows, pre, expect, out, ok, status, n);
    return (int)hipGetLastError();
}
int chain_launch_keyset_gather(hipStream_t stream, const u32* key_ids, const uint8_t* key_bytes, u32 count, uint8_t* pk32, u32 n) {
    hipLaunchKernelGGL(keyset_gather_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, key_ids, key_bytes, count, pk32, n);
    return (int)hipGetLastError();
}
int chain_launch_keyset_fix(hipStream_t stream, const u32* key_ids, const uint8_t* key_status, u32 count, u64* out, uint8_t* ok, uint8_t* status, u32 n) {
    hipLaunchKernelGGL(keyset_fix_kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, key_ids, key_status, count, out, ok, status, n);
    return (int)hipGetLastError();
}

}  // namespace fq

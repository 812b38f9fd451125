// Commitments over a fixed generator set: row g * group_size + j of a call is [k_gj]B_j, computed from comb j of the context's set
// (fourq_commit_bases_set, fourq_amd.hip): m combs back to back, each of the single comb's object shape -- CombFast's 1 024 points, then
// CombScan's 80, COMB_ENTRY_U32 working limbs per point.  Included by fourq_chain.hip (selection by address) and fourq_ct_chain.hip
// (constant-time selection) behind kernels.hip.h, whose comb it reuses: the recoding, the index and sign of a column, the mixed
// additions on signed limbs.  What is new is WHICH table a lane reads.
//
//   staged (COMMIT_STAGED)   One block per CU, 64 to COMB_BLOCK_MAX lanes wide, comb j in the CU's LDS (144 KB).  The block works through
//                            its contiguous range of (base, slice of the groups) items (commit_layout.h, CommitGeom) and stages a comb
//                            again only when the base changes: for many groups per base.
//   gather (COMMIT_GATHER)   256-lane blocks, one lane per row, base-major (lane index = j * groups + g, so a wave's lanes share a
//                            comb where the groups allow it); every entry is read where it lies in the set's array, as
//                            comb_quad_kernel reads the single comb: for few groups per base -- one group of 4 096 bases is 4 096 combs
//                            with one row each.
//   constant time (CT)       The staged structure over the 80-point shape: 11.5 KB per block, up to 256 lanes, four blocks per CU; an
//                            addition reads ALL 16 entries of its block of the table and keeps one by masks, as comb_kernel<.., true>.
//                            No address depends on a scalar: which comb a lane reads follows from its row number.  The route argument
//                            makes no difference in this mode.
//
// Every lane writes a canonical 12-word (X, Y, Z) row, the even-scalar negation applied, which msm_fold_kernel and lower_kernel take from
// there.  Tail lanes redo an existing row and store nothing.
#pragma once
#include "kernels.hip.h"

namespace fq {

namespace {

constexpr size_t COMMIT_COMB_U32 = (size_t)COMB_POINTS * COMB_ENTRY_U32;      // one comb of the set, in dwords

// [k]B for the scalar of `row` from one comb: `table` is the comb's fast shape (LDS or memory) or, CT, its 80-point shape in LDS
template <bool CT> FQ_DEV void commit_row(const u64* scalars, const u32* table, u64* rows, u64 row, bool live) {
    using S = typename std::conditional<CT, CombScan, CombFast>::type;
    u64 m[4];
    load_scalar(scalars + 4 * row, m);
    CombDigits<S> c = comb_recode<S>(m);
    R1 Q;
#pragma unroll 1
    for (int i = S::E - 1; i >= 0; i--) {
#pragma unroll 1
        for (int j = 0; j < S::V; j++) {
            const int col = S::E * j + i;
            const u32 neg = comb_neg_mask(c, col);
            if constexpr (CT) {
                const ScanMem<S::BLOCK_POINTS, u32> block{ table + (j << (S::W - 1)) * COMB_LDS_U32, COMB_LDS_U32 };
                if (i == S::E - 1 && j == 0) { Q = affine_scan_start(block, comb_index(c, col), neg); continue; }
                if (j == 0) Q = dbl<Mul::Signed>(Q.X, Q.Y, Q.Z);
                Q = add_affine_scan(Q, block, comb_index(c, col), neg);
            } else {
                const u32* entry = table + ((j << (S::W - 1)) + comb_index(c, col)) * COMB_LDS_U32;
                if (i == S::E - 1 && j == 0) { Q = affine_table_start(entry, neg); continue; }
                if (j == 0) Q = dbl<Mul::Signed>(Q.X, Q.Y, Q.Z);
                Q = add_affine_table(Q, entry, neg);
            }
        }
    }
    Q = r1_unsign(Q);
    if (!live) return;
    u64 w[12];
    store_fe2(w, fe2_carry(fe2_cneg(Q.X, c.negate)));           // even scalar: [k]B = -[N - k]B, -(x, y) = (-x, y)
    store_fe2(w + 4, Q.Y); store_fe2(w + 8, Q.Z);
    put_words<12>(rows + 12 * row, w);
}

enum CommitRoute { COMMIT_STAGED = 1, COMMIT_GATHER = 2 };
constexpr bool commit_wide(int route, bool ct) { return route == COMMIT_STAGED && !ct; }     // the one shape with the 144 KB table in LDS

// staged / CT: blockDim.x = CommitGeom::width, gridDim.x = CommitGeom::grid, dynamic LDS = the staged shape; gather: BLOCK lanes, no LDS
template <int ROUTE, bool CT>
__global__ __launch_bounds__(commit_wide(ROUTE, CT) ? COMB_BLOCK_MAX : BLOCK, commit_wide(ROUTE, CT) ? 1 : 4)
void commit_kernel(const u64* scalars, const u32* combs, u64* rows, u32 groups, u32 group_size, u32 slices, u32 items) {
    if constexpr (ROUTE == COMMIT_GATHER && !CT) {
        const u64 n = (u64)groups * group_size, it = (u64)blockIdx.x * BLOCK + threadIdx.x;
        const bool live = it < n;
        const u64 at = live ? it : n - 1;
        const u32 j = (u32)(at / groups), g = (u32)(at % groups);
        commit_row<false>(scalars, combs + (size_t)j * COMMIT_COMB_U32, rows, (u64)g * group_size + j, live);
    } else {
        using S = typename std::conditional<CT, CombScan, CombFast>::type;
        extern __shared__ __attribute__((aligned(16))) u32 lds[];            // S::POINTS * COMB_LDS_U32 dwords, sized by the launcher
        static_assert(COMB_LDS_U32 == COMB_ENTRY_U32, "a comb is staged as it lies");
        const u32 width = blockDim.x;
        const u32 first = (u32)((u64)blockIdx.x * items / gridDim.x), last = (u32)((u64)(blockIdx.x + 1) * items / gridDim.x);
        u32 staged = ~0u;
#pragma unroll 1
        for (u32 item = first; item < last; item++) {           // the range is the block's: every lane takes every barrier
            const u32 j = item / slices, s = item % slices;
            if (j != staged) {
                __syncthreads();                                 // the last row on the old comb is done in every wave
                const u32* sub = combs + (size_t)j * COMMIT_COMB_U32 + (CT ? CombFast::POINTS * COMB_ENTRY_U32 : 0);
                for (u32 i = threadIdx.x; i < (u32)(S::POINTS * COMB_ENTRY_U32 / 4); i += width)
                    reinterpret_cast<uint4*>(lds)[i] = reinterpret_cast<const uint4*>(sub)[i];
                __syncthreads();
                staged = j;
            }
            const u32 g = s * width + threadIdx.x;
            const bool live = g < groups;
            commit_row<CT>(scalars, lds, rows, (u64)(live ? g : groups - 1) * group_size + j, live);
        }
    }
}

}  // namespace

}  // namespace fq

// out[g] = sum_j [k_gj] P_gj on the device: the kernel that folds the ladder's projective rows of a group into one row.  Included by
// fourq_chain.hip only, beside combine.hip.h, whose complete addition (add_projective, limb bounds in its types) it reuses.
//
// Every group has the same length, so the whole geometry of a pass is known on the host: m_in rows per group become
// m_out = ceil(m_in / MSM_FOLD) rows per group, and the host repeats passes until m_out == 1 (fourq_amd.hip, msm_dev).  A team of T lanes
// (a power of two, at most 64, the same for the whole launch: a wave holds 64 / T whole teams) owns one output row.  Lane j of a team sums
// the rows j, j + T, ... of its MSM_FOLD-row segment; log2 T butterfly steps then add the partner's sum across lanes (ds_bpermute through
// __shfl_xor, 30 limbs per step), after which every lane of the team holds the team's sum and lane 0 stores it.
//
// No lane leaves before the last cross-lane step: teams past the last group and lanes past the end of a short segment carry the neutral
// (0, 1, 1) -- an ordinary operand of a complete addition -- read a row that exists (row 0) and store nothing.  Which lanes those are follows
// from the launch geometry alone; no address and no branch depends on a scalar or a coordinate.
//
// Rows in: (X, Y, Z) at words 0, 4, 8 of `stride` words (12 or 20, as combine_kernel takes them from mul_rows_dev); rows out: canonical
// 12-word (X, Y, Z).  st_in (NULL for affine input): one raw decode code per input row; st_out gets the maximum of a team's codes, which
// lower_kernel behind the last pass reports as FOURQ_BYTES_DECODE_BASE + itself.  A point that did not decode was lifted as the all-zero
// pair and may drive a group's Z to 0: lower_kernel keeps such a row away from its neighbours' shared inversion, and the status zeroes it.
#pragma once
#include "combine.hip.h"

namespace fq {

namespace {

FQ_DEV Fe2<1> shfl_xor_fe2(const Fe2<1>& a, int mask) {
    Fe2<1> r;
#pragma unroll
    for (int i = 0; i < 5; i++) { r.re.l[i] = (u32)__shfl_xor((int)a.re.l[i], mask); r.im.l[i] = (u32)__shfl_xor((int)a.im.l[i], mask); }
    return r;
}

// teams = groups * m_out; iters = ceil(min(m_in, MSM_FOLD) / T): the rows a lane sums before the butterfly
__global__ __launch_bounds__(BLOCK, 2) void msm_fold_kernel(const u64* rows, u32 stride, const uint8_t* st_in, u64* rows_out, uint8_t* st_out,
                                                            u32 m_in, u32 m_out, u32 T, u32 iters, u64 teams) {
    const u64 lane = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const u64 team = lane / T;
    const u32 j = (u32)(lane % T);
    const bool live = team < teams;
    const u64 g = live ? team / m_out : 0;
    const u32 o = live ? (u32)(team % m_out) : 0;
    const u32 first = o * MSM_FOLD, left = m_in - first, count = left < MSM_FOLD ? left : MSM_FOLD;   // the team's segment of its group
    Fe2<1> zero;
#pragma unroll
    for (int i = 0; i < 5; i++) zero.re.l[i] = zero.im.l[i] = 0;
    const Fe2<1> one = fe2_one();
    XYZ acc;
    u32 st = 0;
    for (u32 k = 0; k < iters; k++) {
        const u32 r = j + k * T;
        const bool have = live && r < count;
        const u64 at = have ? g * m_in + first + r : 0;
        const u32 keep = have ? ~0u : 0u;
        const u64* row = rows + stride * at;
        const Fe2<1> X = fe2_select(keep, load_fe2(row), zero), Y = fe2_select(keep, load_fe2(row + 4), one), Z = fe2_select(keep, load_fe2(row + 8), one);
        if (st_in) { const u32 s = st_in[at]; st = (have && s > st) ? s : st; }
        if (k == 0) { acc.X = X; acc.Y = Y; acc.Z = Z; }
        else acc = add_projective(acc.X, acc.Y, acc.Z, X, Y, Z);
    }
    for (u32 step = T >> 1; step; step >>= 1) {                    // every lane of the wave takes every step
        const Fe2<1> X = shfl_xor_fe2(acc.X, (int)step), Y = shfl_xor_fe2(acc.Y, (int)step), Z = shfl_xor_fe2(acc.Z, (int)step);
        const u32 s = (u32)__shfl_xor((int)st, (int)step);
        st = s > st ? s : st;
        acc = add_projective(acc.X, acc.Y, acc.Z, X, Y, Z);
    }
    if (!live || j != 0) return;
    u64 w[12];
    store_fe2(w, acc.X); store_fe2(w + 4, acc.Y); store_fe2(w + 8, acc.Z);
    put_words<12>(rows_out + 12 * team, w);
    if (st_in) st_out[team] = (uint8_t)st;
}

// The same pass over groups of ANY length (the ragged grouped sums; msm_shape.h): team t owns output row t and reads desc[t] = { first, count },
// the rows first .. first + count - 1 of the level below, 0 <= count <= MSM_FOLD.  The host built the descriptors from validated offsets
// (fq_work::ShapePlan::build) so that those of a pass partition the level below exactly: every first + r with r < count lies inside it, and
// this kernel derives no address from anything else.  A wave holds 64 / T teams, so the descriptor is not wave-uniform: every lane of a
// team loads the same 8 bytes (one dwordx2 per lane, the wave's 64 / T descriptors in one or two cache lines).
//
// The invariants of msm_fold_kernel hold.  No lane leaves before the last cross-lane step.  Lanes past a short segment, teams past the last
// descriptor and EVERY lane of a team whose count is 0 carry the neutral (0, 1, 1), read a row that exists (row 0; the layout keeps one
// even where the call has no element at all); a live team stores what its descriptor says -- for count 0 the neutral, with code 0 -- and
// a team past the last descriptor stores nothing.  No branch and no address depends on a scalar or a coordinate.
// teams: the pass's output rows; iters = max(1, ceil(largest count of the pass / T))
__global__ __launch_bounds__(BLOCK, 2) void msm_fold_desc_kernel(const u64* rows, u32 stride, const uint8_t* st_in, u64* rows_out, uint8_t* st_out,
                                                                 const uint2* desc, u32 T, u32 iters, u32 teams) {
    const u64 lane = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const u64 team = lane / T;
    const u32 j = (u32)(lane % T);
    const bool live = team < teams;
    const uint2 d = desc[live ? team : 0];
    const u32 first = d.x, count = live ? d.y : 0;
    Fe2<1> zero;
#pragma unroll
    for (int i = 0; i < 5; i++) zero.re.l[i] = zero.im.l[i] = 0;
    const Fe2<1> one = fe2_one();
    XYZ acc;
    u32 st = 0;
    for (u32 k = 0; k < iters; k++) {
        const u32 r = j + k * T;
        const bool have = r < count;
        const u64 at = have ? (u64)first + r : 0;
        const u32 keep = have ? ~0u : 0u;
        const u64* row = rows + stride * at;
        const Fe2<1> X = fe2_select(keep, load_fe2(row), zero), Y = fe2_select(keep, load_fe2(row + 4), one), Z = fe2_select(keep, load_fe2(row + 8), one);
        if (st_in) { const u32 s = st_in[at]; st = (have && s > st) ? s : st; }
        if (k == 0) { acc.X = X; acc.Y = Y; acc.Z = Z; }
        else acc = add_projective(acc.X, acc.Y, acc.Z, X, Y, Z);
    }
    for (u32 step = T >> 1; step; step >>= 1) {                    // every lane of the wave takes every step
        const Fe2<1> X = shfl_xor_fe2(acc.X, (int)step), Y = shfl_xor_fe2(acc.Y, (int)step), Z = shfl_xor_fe2(acc.Z, (int)step);
        const u32 s = (u32)__shfl_xor((int)st, (int)step);
        st = s > st ? s : st;
        acc = add_projective(acc.X, acc.Y, acc.Z, X, Y, Z);
    }
    if (!live || j != 0) return;
    u64 w[12];
    store_fe2(w, acc.X); store_fe2(w + 4, acc.Y); store_fe2(w + 8, acc.Z);
    put_words<12>(rows_out + 12 * team, w);
    if (st_in) st_out[team] = (uint8_t)st;
}

}  // namespace

}  // namespace fq

// out[g] = sum_j MUL_endo(k_gj, P_gj) by the bucket method (Pippenger): the second route of the grouped sums, for large groups.  Included by
// fourq_chain.hip only, beside msm.hip.h, whose fold kernel and complete addition (add_projective, combine.hip.h) it reuses.
//
// decompose(k) yields v_0..v_3 < 2^64 with MUL_endo(k, P) = [v_0]P + [v_1]phi(P) + [v_2]psi(P) + [v_3]psi(phi(P)), and phi, psi are
// homomorphisms, so  sum_i MUL_endo(k_i, P_i) = S_0 + phi(S_1) + psi(S_2) + psi(phi(S_3))  with  S_j = sum_i [v_j(k_i)]P_i : four plain
// 64-bit sums over the SAME affine points, and three endomorphisms per group instead of per element.  The identity holds for every pair the
// ladder accepts, points outside the order-N subgroup included, so the canonical affine result is the ladder route's byte for byte.
//
// With c = window, W = ceil(64 / c), B = 2^c a group has 4 W columns (sub-scalar j, window w) of B - 1 buckets (unsigned digits, digit 0
// skipped).  bucket_layout.h fixes the geometry of every launch from (groups, group_size, window) on the host; the steps are
//   1  bucket_digits_kernel      one lane per element: v = decompose(k); the group's largest decode code (bytes flavour)
//   2  bucket_sort_kernel<0>     counting sort of the element indices of every column by digit: histogram (atomicAdd on u32, in LDS first),
//      bucket_scan_kernel        exclusive scan of the counts and of the part counts ceil(count / 64), one block per column,
//      bucket_sort_kernel<1>     scatter (the position inside a bucket is an atomic cursor: it may vary from run to run, the sum does not)
//   3  bucket_accumulate_kernel  every bucket's run of rows is cut into parts of at most 64 and ONE LANE SUMS ONE PART, so no lane's chain is
//                                longer than 64 additions whatever the scalars are (all scalars equal: one bucket per column holds the
//                                whole group); repeated `passes` times, after which no bucket holds more than one row
//   4  bucket_weighted_kernel    sum_d d B_d over 16 consecutive buckets per lane by running sums, then msm_fold_kernel down to one row per column
//   5  bucket_horner_kernel      one lane per (group, j): Horner over the W windows, top first, c doublings between them, then the
//                                endomorphism of j; msm_fold_kernel adds the four rows and carries the group's decode code to the lowering
// Bucket addresses are digits of the scalars: in constant-time selection mode the host never comes here (fourq_amd.hip, bucket_dev).
#pragma once
#include "msm.hip.h"
#include "bucket_layout.h"

namespace fq {

namespace {

constexpr u32 BUCKET_PART = fq_work::BucketGeom::PART, BUCKET_CHUNK = fq_work::BucketGeom::CHUNK;

FQ_DEV Fe2<1> fe2_zero() {
    Fe2<1> z;
#pragma unroll
    for (int i = 0; i < 5; i++) z.re.l[i] = z.im.l[i] = 0;
    return z;
}
FQ_DEV void store_xyz(u64* dst_row, const Fe2<1>& X, const Fe2<1>& Y, const Fe2<1>& Z) {
    u64 w[12];
    store_fe2(w, X); store_fe2(w + 4, Y); store_fe2(w + 8, Z);
    put_words<12>(dst_row, w);
}

// ---- 1. digits: v[i] = decompose(k_i); group_code[g] = the largest raw decode code among the group's elements (st_decode NULL: affine flavour)
__global__ __launch_bounds__(BLOCK) void bucket_digits_kernel(const u64* scalars, u64* v_out, const uint8_t* st_decode, u32* group_code, u32 n, u32 group_size) {
    const u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 m[4], v[4];
    load_scalar(scalars + 4 * i, m);
    decompose(m, v);
    put_words<4>(v_out + 4 * i, v);
    if (st_decode) {
        const u32 s = st_decode[i];
        if (s) atomicMax(group_code + i / group_size, s);
    }
}

// ---- 2. the counting sort.  Block (tile, column-in-group): BUCKET_TILE consecutive elements and one (sub-scalar j, window w).  Where the
// tile lies inside ONE group -- every tile of a large group, which is where thousands of elements meet in a few hundred counters -- the block
// counts in LDS first and goes to the column's global counters once per digit: SCATTER = false adds its counts; SCATTER = true takes its
// range of every bucket by counting the same counters back down (they end at zero) and places each element at off[digit] + the range's
// start + the element's rank inside the block.  A tile that spans groups (small groups: little contention) goes to the counters directly.
// The position inside a bucket depends on the order of the atomics: it may vary from run to run.
constexpr u32 BUCKET_TILE = 2048;
template <bool SCATTER>
__global__ __launch_bounds__(BLOCK) void bucket_sort_kernel(const u64* v, u32* counts, const u32* off, u32* idx, u32 n, u32 group_size, u32 c, u32 W) {
    __shared__ u32 hist[1u << fq_work::BucketGeom::WINDOW_MAX];
    constexpr u32 PER = BUCKET_TILE / BLOCK;
    const u32 B = 1u << c, mask = B - 1, t = threadIdx.x;
    const u32 j = blockIdx.y / W, w = blockIdx.y % W, shift = w * c;
    const u64 first = (u64)blockIdx.x * BUCKET_TILE, end = first + BUCKET_TILE < n ? first + BUCKET_TILE : n;
    const u64 g0 = first / group_size;
    if ((end - 1) / group_size != g0) {                            // the same for the whole block
        for (u32 e = 0; e < PER; e++) {
            const u64 i = first + e * BLOCK + t;
            if (i >= end) break;
            const u32 d = (u32)(v[4 * i + j] >> shift) & mask;
            if (d == 0) continue;
            const u64 col = ((i / group_size) * 4 + j) * W + w;
            if constexpr (SCATTER) {
                const u32 cursor = atomicSub(counts + (col << c) + d, 1u) - 1;
                idx[col * group_size + off[col * (B + 1) + d] + cursor] = (u32)i;
            } else {
                atomicAdd(counts + (col << c) + d, 1u);
            }
        }
        return;
    }
    const u64 col = (g0 * 4 + j) * W + w;
    for (u32 d = t; d < B; d += BLOCK) hist[d] = 0;
    __syncthreads();
    u32 digit[PER], rank[PER];
#pragma unroll
    for (u32 e = 0; e < PER; e++) {
        const u64 i = first + e * BLOCK + t;
        digit[e] = i < end ? (u32)(v[4 * i + j] >> shift) & mask : 0;
        rank[e] = digit[e] ? atomicAdd(&hist[digit[e]], 1u) : 0;
    }
    __syncthreads();
    u32* column_counts = counts + (col << c);
    for (u32 d = t; d < B; d += BLOCK) {
        const u32 local = hist[d];
        if (local == 0) continue;
        if constexpr (SCATTER) hist[d] = atomicSub(column_counts + d, local) - local;      // where the block's range of bucket d starts
        else atomicAdd(column_counts + d, local);
    }
    if constexpr (SCATTER) {
        __syncthreads();
        const u32* o = off + col * (B + 1);
        u32* dst = idx + col * group_size;
#pragma unroll
        for (u32 e = 0; e < PER; e++)
            if (digit[e]) dst[o[digit[e]] + hist[digit[e]] + rank[e]] = (u32)(first + e * BLOCK + t);
    }
}

// One block per column.  The count of digit d is counts[col][d] (FROM_COUNTS) or the difference of the previous pass's part starts
// prev[col][d + 1] - prev[col][d].  off_out (FROM_COUNTS only): exclusive scan of the counts; part_out: exclusive scan of ceil(count / 64);
// B + 1 entries per column each, the last one the total.
template <bool FROM_COUNTS>
__global__ __launch_bounds__(BLOCK) void bucket_scan_kernel(const u32* in, u32* off_out, u32* part_out, u32 c) {
    __shared__ u32 s_count[BLOCK], s_part[BLOCK];
    const u32 B = 1u << c, per = (B + BLOCK - 1) / BLOCK, t = threadIdx.x, lo = t * per;
    const u64 col = blockIdx.x;
    const u32* src = in + col * (FROM_COUNTS ? B : B + 1);
    u32 counts = 0, parts = 0;
    for (u32 d = lo; d < lo + per && d < B; d++) {
        const u32 n = FROM_COUNTS ? src[d] : src[d + 1] - src[d];
        counts += n; parts += (n + BUCKET_PART - 1) / BUCKET_PART;
    }
    s_count[t] = counts; s_part[t] = parts;
    __syncthreads();
    for (u32 step = 1; step < BLOCK; step <<= 1) {                 // inclusive scan over the block's threads
        const u32 a = t >= step ? s_count[t - step] : 0, b = t >= step ? s_part[t - step] : 0;
        __syncthreads();
        s_count[t] += a; s_part[t] += b;
        __syncthreads();
    }
    u32 run_count = s_count[t] - counts, run_part = s_part[t] - parts;
    u32* off = FROM_COUNTS ? off_out + col * (B + 1) : nullptr;
    u32* part = part_out + col * (B + 1);
    for (u32 d = lo; d < lo + per && d < B; d++) {
        const u32 n = FROM_COUNTS ? src[d] : src[d + 1] - src[d];
        if (FROM_COUNTS) off[d] = run_count;
        part[d] = run_part;
        run_count += n; run_part += (n + BUCKET_PART - 1) / BUCKET_PART;
    }
    if (t == BLOCK - 1) {                                          // the last thread's inclusive sums are the totals
        if (FROM_COUNTS) off[B] = s_count[t];
        part[B] = s_part[t];
    }
}

// ---- 3. accumulate.  Lane (column, p), p < out_rows (the host's bound), sums part p of its column: the parts are numbered bucket after bucket,
// `part` holding every bucket's first part number, so the lane finds its bucket by binary search and its rows behind off[bucket].  A lane past
// the column's actual part count finds nothing and stores nothing.  FIRST: the rows are the affine points (8 words, Z = 1) gathered through
// idx; later passes read the 12-word rows the pass before left, in_rows per column.  Output row p of the column: the buckets' partial sums,
// contiguous and in digit order -- the next pass's input, whose bucket starts are this pass's part starts.
template <bool FIRST>
__global__ __launch_bounds__(BLOCK, 2) void bucket_accumulate_kernel(const u64* rows_in, const u32* idx, const u32* off, const u32* part, u64* rows_out,
                                                                     u64 cols, u32 in_rows, u32 out_rows, u32 c) {
    const u64 lane = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const u64 col = lane / out_rows;
    const u32 p = (u32)(lane % out_rows);
    if (col >= cols) return;
    const u32 B = 1u << c;
    const u32* po = part + col * (B + 1);
    if (p >= po[B]) return;
    u32 d = 0;
    for (u32 half = B >> 1; half; half >>= 1) d += po[d + half] <= p ? half : 0;     // the largest d with po[d] <= p: po[0] = 0 and B is a power of two
    const u32* o = off + col * (B + 1);
    const u32 start = o[d] + (p - po[d]) * BUCKET_PART, left = o[d + 1] - start, count = left < BUCKET_PART ? left : BUCKET_PART;
    const u64 first = col * in_rows + start;
    const Fe2<1> one = fe2_one();
    XYZ acc;
    for (u32 r = 0; r < count; r++) {
        const u64* row = FIRST ? rows_in + 8 * (u64)idx[first + r] : rows_in + 12 * (first + r);
        const Fe2<1> X = load_fe2(row), Y = load_fe2(row + 4), Z = FIRST ? one : load_fe2(row + 8);
        if (r == 0) { acc.X = X; acc.Y = Y; acc.Z = Z; }
        else acc = add_projective(acc.X, acc.Y, acc.Z, X, Y, Z);
    }
    store_xyz(rows_out + 12 * (col * out_rows + p), acc.X, acc.Y, acc.Z);
}

// ---- 4. sum_d d B_d.  Lane (column, t) takes the buckets d0 + 1 .. d0 + 16, d0 = 16 t, highest first: run += B_d, tot += run leaves
// tot = sum_i i B_(d0 + i) and run = sum_i B_(d0 + i); the lane's share is tot + [d0]run.  d0 is geometry, not data: double-and-add over its c bits,
// every lane the same steps, the addend chosen by a select.  A bucket is present when its part count is 1 (part: the last pass's part starts,
// which are the rows' positions); an absent one -- and digit B, past the column's last bucket -- is the neutral (0, 1, 1).
__global__ __launch_bounds__(BLOCK, 2) void bucket_weighted_kernel(const u64* rows, const u32* part, u64* out, u64 cols, u32 in_rows, u32 c) {
    const u32 B = 1u << c, chunks = B / BUCKET_CHUNK;
    const u64 lane = (u64)blockIdx.x * BLOCK + threadIdx.x;
    const u64 col = lane / chunks;
    if (col >= cols) return;
    const u32 d0 = (u32)(lane % chunks) * BUCKET_CHUNK;
    const u32* po = part + col * (B + 1);
    const Fe2<1> zero = fe2_zero(), one = fe2_one();
    XYZ run, tot;
    run.X = tot.X = zero; run.Y = tot.Y = one; run.Z = tot.Z = one;
#pragma unroll 1
    for (u32 i = BUCKET_CHUNK; i >= 1; i--) {                      // one addition after the other: interleaved, two running sums and their temporaries spill
        const u32 d = d0 + i;
        const bool have = d < B && po[d + 1] != po[d];
        const u64* row = rows + 12 * (have ? col * in_rows + po[d] : 0);
        const u32 keep = have ? ~0u : 0u;
        const Fe2<1> X = fe2_select(keep, load_fe2(row), zero), Y = fe2_select(keep, load_fe2(row + 4), one), Z = fe2_select(keep, load_fe2(row + 8), one);
        run = add_projective(run.X, run.Y, run.Z, X, Y, Z);
        __builtin_amdgcn_sched_barrier(0);
        tot = add_projective(tot.X, tot.Y, tot.Z, run.X, run.Y, run.Z);
    }
    u64* dst = out + 12 * lane;
    store_xyz(dst, tot.X, tot.Y, tot.Z);
    if (chunks == 1) return;
    // tot waits in the lane's output row while [d0]run is formed: four sums alive at once (tot, run, acc, acc + run) do not fit the registers
    XYZ acc;
    acc.X = zero; acc.Y = one; acc.Z = one;
#pragma unroll 1
    for (int b = (int)c - 1; b >= 0; b--) {
        acc = add_projective(acc.X, acc.Y, acc.Z, acc.X, acc.Y, acc.Z);
        __builtin_amdgcn_sched_barrier(0);
        const XYZ with = add_projective(acc.X, acc.Y, acc.Z, run.X, run.Y, run.Z);
        const u32 keep = 0u - ((d0 >> b) & 1u);
        acc.X = fe2_select(keep, with.X, acc.X); acc.Y = fe2_select(keep, with.Y, acc.Y); acc.Z = fe2_select(keep, with.Z, acc.Z);
    }
    __builtin_amdgcn_sched_barrier(0);
    tot = add_projective(load_fe2(dst), load_fe2(dst + 4), load_fe2(dst + 8), acc.X, acc.Y, acc.Z);
    store_xyz(dst, tot.X, tot.Y, tot.Z);
}

// ---- 5. lane (group, j): S_j = sum_w 2^(c w) column(g, j, w) by Horner, top window first, then the endomorphism of j -- none, phi, psi,
// psi(phi) -- so that the four rows of a group add up to its result.  group_code (NULL: affine flavour) goes on all four rows.
__global__ __launch_bounds__(BLOCK) void bucket_horner_kernel(const u64* columns, const u32* group_code, u64* out, uint8_t* st_out, u64 lanes, u32 c, u32 W) {
    const u64 t = (u64)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= lanes) return;
    const u64* top = columns + 12 * (t * W + (W - 1));
    R1 s;
    s.X = load_fe2(top); s.Y = load_fe2(top + 4); s.Z = load_fe2(top + 8);
    for (u32 w = W - 1; w-- > 0;) {
#pragma unroll 1
        for (u32 k = 0; k < c; k++) s = dbl(s.X, s.Y, s.Z);
        const u64* row = columns + 12 * (t * W + w);
        const XYZ sum = add_projective(s.X, s.Y, s.Z, load_fe2(row), load_fe2(row + 4), load_fe2(row + 8));
        s.X = sum.X; s.Y = sum.Y; s.Z = sum.Z;
    }
    if (t & 1) s = phi(s);
    if (t & 2) s = psi(s);
    store_xyz(out + 12 * t, s.X, s.Y, s.Z);
    if (group_code) st_out[t] = (uint8_t)group_code[t >> 2];
}

hipError_t bucket_grid(u64 lanes, unsigned* grid) {
    const u64 blocks = (lanes + BLOCK - 1) / BLOCK;
    if (blocks == 0 || blocks > 0x7fffffffu) return hipErrorInvalidValue;
    *grid = (unsigned)blocks;
    return hipSuccess;
}

}  // namespace

// Everything between the decode (fourq_amd.hip) and the lowering: enqueues steps 1-5 on `stream` and leaves one row per group in w.sum (and,
// with st_decode, the group's raw decode code in w.st_sum).  points: n x 8 affine words; st_decode: one raw code per element, or NULL.
int chain_launch_bucket_sum(hipStream_t stream, const fq_work::Bucket& w, const u64* scalars, const u64* points, const uint8_t* st_decode) {
#define BUCKET_TRY(expr) do { const hipError_t e_ = (hipError_t)(expr); if (e_ != hipSuccess) return (int)e_; } while (0)
    const fq_work::BucketGeom& g = w.g;
    const u32 c = g.window, W = g.windows;
    if (g.cols > 0x7fffffffu || g.group_size > 0xffffffffu || g.n > 0xffffffffu) return (int)hipErrorInvalidValue;
    unsigned grid;
    BUCKET_TRY(hipMemsetAsync(w.group_code, 0, w.zeroed_bytes(), stream));
    BUCKET_TRY(bucket_grid(g.n, &grid));
    hipLaunchKernelGGL(bucket_digits_kernel, dim3(grid), dim3(BLOCK), 0, stream, scalars, w.v, st_decode, w.group_code, (u32)g.n, (u32)g.group_size);
    const dim3 tiles((unsigned)((g.n + BUCKET_TILE - 1) / BUCKET_TILE), 4 * W);
    hipLaunchKernelGGL(bucket_sort_kernel<false>, tiles, dim3(BLOCK), 0, stream, w.v, w.counts, nullptr, nullptr, (u32)g.n, (u32)g.group_size, c, W);
    hipLaunchKernelGGL(bucket_scan_kernel<true>, dim3((unsigned)g.cols), dim3(BLOCK), 0, stream, w.counts, w.off_a, w.off_b, c);
    hipLaunchKernelGGL(bucket_sort_kernel<true>, tiles, dim3(BLOCK), 0, stream, w.v, w.counts, w.off_a, w.idx, (u32)g.n, (u32)g.group_size, c, W);
    BUCKET_TRY(hipGetLastError());
    const u32* off = w.off_a;
    u32* part = w.off_b;
    const u64* rows = points;
    for (unsigned k = 0; k < g.passes; k++) {
        u64* rows_out = (k & 1) ? w.rows_b : w.rows_a;
        if (k) {                                                   // this pass's bucket starts are the last pass's part starts
            u32* next = const_cast<u32*>(off);
            off = part; part = next;
            hipLaunchKernelGGL(bucket_scan_kernel<false>, dim3((unsigned)g.cols), dim3(BLOCK), 0, stream, off, nullptr, part, c);
        }
        BUCKET_TRY(bucket_grid((u64)g.cols * g.rows[k + 1], &grid));
        if (k == 0) hipLaunchKernelGGL(bucket_accumulate_kernel<true>, dim3(grid), dim3(BLOCK), 0, stream, rows, w.idx, off, part, rows_out, (u64)g.cols, (u32)g.rows[0], (u32)g.rows[1], c);
        else hipLaunchKernelGGL(bucket_accumulate_kernel<false>, dim3(grid), dim3(BLOCK), 0, stream, rows, nullptr, off, part, rows_out, (u64)g.cols, (u32)g.rows[k], (u32)g.rows[k + 1], c);
        BUCKET_TRY(hipGetLastError());
        rows = rows_out;
    }
    BUCKET_TRY(bucket_grid((u64)g.cols * g.chunks, &grid));
    hipLaunchKernelGGL(bucket_weighted_kernel, dim3(grid), dim3(BLOCK), 0, stream, rows, part, w.weighted, (u64)g.cols, (u32)g.rows[g.passes], c);
    BUCKET_TRY(hipGetLastError());
    const u64* columns = w.weighted;
    if (g.chunks > 1) { BUCKET_TRY(chain_launch_msm_fold(stream, columns, 12, nullptr, w.fold_a, nullptr, g.cols, g.chunks)); columns = w.fold_a; }
    if (g.fold1 > 1) { BUCKET_TRY(chain_launch_msm_fold(stream, columns, 12, nullptr, w.fold_b, nullptr, g.cols, g.fold1)); columns = w.fold_b; }
    BUCKET_TRY(bucket_grid(4 * (u64)g.groups, &grid));
    hipLaunchKernelGGL(bucket_horner_kernel, dim3(grid), dim3(BLOCK), 0, stream, columns, st_decode ? w.group_code : nullptr, w.endo, w.st_endo, 4 * (u64)g.groups, c, W);
    BUCKET_TRY(hipGetLastError());
    return chain_launch_msm_fold(stream, w.endo, 12, st_decode ? w.st_endo : nullptr, w.sum, w.st_sum, g.groups, 4);
#undef BUCKET_TRY
}

}  // namespace fq

// Launch geometry and work-buffer layout of the fixed-generator commitments (include/fourq_amd.h, "commitments over a fixed generator set";
// commit.hip.h).  Plain C++, no HIP, built on work_layout.h's Carver: tests/test_commit_oracle.py compiles it with g++
// (tests/c/commit_layout_dump.cpp).
//
// A call has n = groups x group_size rows; row g * group_size + j is [k_gj]B_j and comes from comb j.  The comb kernel leaves one canonical
// 12-word (X, Y, Z) row per row of scalars in `rows`; the fold passes of the grouped sums (msm.hip.h) then turn m rows per group into
// ceil(m / 64), alternating between part_a and part_b, and the lowering reads the one row per group that is left (`rows` itself when
// group_size == 1).  The bytes flavour lowers through lower_kernel<K, true>, which reads one decode code per group and writes one status
// byte per group: nothing is decoded here, so the codes are a zeroed region and the status bytes go to a region nobody reads.
#pragma once
#include "work_layout.h"

namespace fq_work {

// The staged kernel (and the constant-time one): a work item is (base j, slice s): lanes s * width .. of the groups, all on comb j.  Items are
// ordered base-major, item = j * slices + s, and block b owns the ONE contiguous range [b * items / grid, (b + 1) * items / grid): it stages a
// comb only when the base changes inside its range.  The width is the narrowest that lets one pass of `blocks_max` resident blocks hold all n
// rows -- as the single comb's launcher chooses it -- but no wider than the groups of one base need; the grid is no larger than the blocks
// that hold n rows at that width, so that a call of few rows stages few combs.
struct CommitGeom {
    unsigned width, grid;
    size_t slices, items;
    CommitGeom(size_t groups, size_t group_size, unsigned blocks_max, unsigned width_max) {
        const size_t n = groups * group_size;
        width = 64;
        while (width < width_max && width < groups && (size_t)width * blocks_max < n) width *= 2;
        slices = (groups + width - 1) / width;
        items = slices * group_size;
        const size_t cover = (n + width - 1) / width;          // <= items, because slices * width >= groups
        grid = (unsigned)(cover < blocks_max ? cover : blocks_max);
    }
    size_t first_item(unsigned block) const { return (size_t)((unsigned long long)block * items / grid); }
};

struct Commit : Leaf {
    static constexpr size_t FOLD = 64;                          // msm.hip.h, MSM_FOLD (fourq_amd.hip asserts that they agree)
    uint64_t* rows;                 // the combs' results: n rows of 12 words
    uint64_t *part_a, *part_b;      // partial sums, rows of 12 words: groups x ceil(group_size / 64), and groups x ceil of that / 64 again
    uint8_t *st_zero, *st_out;      // bytes flavour: the all-zero decode codes the lowering reads, and the status bytes it writes: groups each
    size_t end;
    static size_t folded(size_t m) { return (m + FOLD - 1) / FOLD; }
    Commit(char* base, size_t groups, size_t group_size) {
        Carver w(base);
        const size_t first = folded(group_size), second = folded(first);
        rows = w.take<uint64_t>(groups * group_size * 12);
        part_a = w.take<uint64_t>(group_size > 1 ? groups * first * 12 : 0);
        part_b = w.take<uint64_t>(first > 1 ? groups * second * 12 : 0);
        st_zero = w.take_status(groups); st_out = w.take_status(groups);
        end = w.used;
    }
    static size_t bytes(size_t groups, size_t group_size) { return Commit(nullptr, groups, group_size).end; }
};

}  // namespace fq_work

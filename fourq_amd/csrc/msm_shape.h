// The registered shape of the ragged grouped sums (include/fourq_amd.h, "ragged grouped sums"): from groups + 1 row offsets, validated HERE,
// the geometry of every fold pass and the work-buffer layout of the call.  Plain C++, no HIP, built on work_layout.h's Carver:
// tests/test_msm_ragged_oracle.py compiles it with g++ (tests/c/msm_shape_dump.cpp), once more under the address and undefined-behaviour
// sanitizers, and checks every descriptor and offset on the CPU.
//
// Levels.  Level 0 is the caller's rows, L_0[g] = offsets[g + 1] - offsets[g] per group, 0 allowed.  Level p holds
// L_p[g] = max(1, ceil(L_{p-1}[g] / FOLD)) rows per group, compact and in group order; the max gives an empty group its neutral row.
// Passes repeat until every group has one row: none where every length is exactly 1, at least one as soon as a group is empty or longer.
//
// Descriptors.  Output row t of a pass is team t of msm_fold_desc_kernel (msm.hip.h) and owns desc[t] = { first, count }: the rows
// first .. first + count - 1 of the previous level, 0 <= count <= FOLD.  The descriptors of a pass partition the previous level exactly and
// in order -- desc[t + 1].first == desc[t].first + desc[t].count, the first one starts at 0, the last one ends at the level's size -- so
// every first + r with r < count that the kernel turns into an address lies inside the previous level by construction.  A descriptor with
// count 0 (an empty group in the first pass; there is none in later ones) names no row: its `first` is where the group would begin and
// is never made an address.
//
// A pass's team width is uniform, as in the equal-length fold: min(16, 2^ceil(log2(largest count of the pass))), and a lane sums
// `iters` = max(1, ceil(largest count / width)) rows before the butterfly.
#pragma once
#include <new>
#include <vector>
#include "work_layout.h"

namespace fq_work {

struct ShapeDesc { uint32_t first, count; };            // 8 bytes: what a team's lanes load
struct ShapePass {
    size_t rows_in, rows_out;                           // the sizes of the level read and of the level written: rows_out teams
    size_t desc_at;                                     // the pass's descriptors are desc[desc_at .. desc_at + rows_out)
    uint32_t largest, team, iters;                      // the largest count, the team width, rows per lane
};

struct ShapePlan {
    static constexpr size_t FOLD = 64;                  // msm.hip.h, MSM_FOLD (fourq_amd.hip asserts that they agree)
    static constexpr size_t TEAM_MAX = 16;
    size_t groups = 0, rows = 0;
    std::vector<ShapePass> passes;
    std::vector<ShapeDesc> desc;                        // every pass's descriptors, back to back

    enum Result { OK = 0, INVALID = 1, NOMEM = 2 };
    // offsets: groups + 1 ascending values from 0; `cap`: the most groups and the most rows a call takes (FOURQ_MAX_BATCH).  *this is
    // written only on OK.  A level of more than 2^32 - 1 rows (short groups by the billion) is INVALID: a descriptor could not name its rows.
    Result build(const uint32_t* offsets, size_t n_groups, size_t cap) {
        if (!offsets || n_groups == 0 || n_groups > cap || offsets[0] != 0) return INVALID;
        for (size_t g = 0; g < n_groups; g++) if (offsets[g + 1] < offsets[g]) return INVALID;
        if (offsets[n_groups] > cap) return INVALID;
        try {
            ShapePlan next;
            next.groups = n_groups;
            next.rows = offsets[n_groups];
            std::vector<uint32_t> len(n_groups);
            bool more = false;                          // is there a group that does not have exactly one row?
            for (size_t g = 0; g < n_groups; g++) { len[g] = offsets[g + 1] - offsets[g]; more = more || len[g] != 1; }
            size_t level = next.rows;
            while (more) {
                ShapePass pass = { level, 0, next.desc.size(), 0, 1, 1 };
                uint64_t at = 0;
                more = false;
                for (size_t g = 0; g < n_groups; g++) {
                    const uint32_t m = len[g], out = m == 0 ? 1 : (uint32_t)((m + FOLD - 1) / FOLD);
                    for (uint32_t o = 0; o < out; o++) {
                        const uint32_t left = m - o * (uint32_t)FOLD, count = left < FOLD ? left : (uint32_t)FOLD;
                        next.desc.push_back({ (uint32_t)at, count });
                        at += count;
                        if (count > pass.largest) pass.largest = count;
                    }
                    pass.rows_out += out;
                    len[g] = out;
                    more = more || out != 1;
                }
                if (pass.rows_out > 0xffffffffu) return INVALID;
                while (pass.team < TEAM_MAX && pass.team < pass.largest) pass.team *= 2;
                pass.iters = pass.largest ? (pass.largest + pass.team - 1) / pass.team : 1;
                next.passes.push_back(pass);
                level = pass.rows_out;
            }
            *this = std::move(next);
        } catch (const std::bad_alloc&) {
            return NOMEM;
        }
        return OK;
    }
};

// Work buffer of a ragged call over n rows in `groups` groups.  Level 1 holds sum_g max(1, ceil(L_g / 64)) <= groups + n / 64 rows -- more
// than Msm's n / 2 where many groups are short or empty -- and level 2 at most groups + (groups + n / 64) / 64; from level 1 on a pass never
// makes a level longer, so the later passes alternate between the same two regions.  The ladder's regions hold at least ONE row and one
// status byte even where n == 0: the lanes of a team whose count is 0 read row 0 of the level below (and discard it), as every idle lane does.
struct MsmRagged : Leaf {
    uint64_t *rows_in, *rows_out;   // as MulRows
    uint8_t* st_decode;
    uint64_t *part_a, *part_b;      // levels 1, 3, ... and 2, 4, ...: rows of 12 words
    uint8_t *st_a, *st_b;           // the largest decode code among a partial sum's elements
    size_t end;
    static size_t level1(size_t n, size_t groups) { return groups + n / ShapePlan::FOLD; }
    static size_t level2(size_t n, size_t groups) { return groups + level1(n, groups) / ShapePlan::FOLD; }
    MsmRagged(char* base, size_t n, size_t groups) {
        Carver w(base);
        const size_t ladder = n ? n : 1;
        rows_in = w.take<uint64_t>(ladder * 20); rows_out = w.take<uint64_t>(ladder * 20); st_decode = w.take_status(ladder);
        part_a = w.take<uint64_t>(level1(n, groups) * 12); st_a = w.take_status(level1(n, groups));
        part_b = w.take<uint64_t>(level2(n, groups) * 12); st_b = w.take_status(level2(n, groups));
        end = w.used;
    }
    static size_t bytes(size_t n, size_t groups) { return MsmRagged(nullptr, n, groups).end; }
};

}  // namespace fq_work

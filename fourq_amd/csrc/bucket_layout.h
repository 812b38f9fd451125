// Geometry and work-buffer layout of the bucket route of the grouped sums (include/fourq_amd.h, "sums across elements: the bucket route";
// bucket.hip.h).  Plain C++, no HIP, built on work_layout.h's Carver: tests/test_bucket_oracle.py compiles it with g++
// (tests/c/bucket_layout_dump.cpp).
//
// With c = window and W = ceil(64 / c) a group has 4 W columns -- one per 64-bit sub-scalar v_j of decompose() and window -- of B = 2^c
// digits each; digit 0 is skipped, so a column has B - 1 buckets.  ALL columns of a call are alive at once (one histogram, one scatter and
// one launch per accumulation pass for the whole call; DESIGN.md section 5 has the sizes this comes to).
//
// Everything a launch needs follows from (groups, group_size, window) here, on the host:
//   passes      the smallest p >= 1 with 64^p >= group_size: a bucket of `count` rows leaves ceil(count / 64) per pass, so after p passes
//               no bucket holds more than one row, whatever the scalars are
//   rows[k]     rows per column that pass k + 1 may read: rows[0] = group_size, and a pass over R rows in B - 1 buckets leaves at most
//               floor(R / 64) full parts plus one part per non-empty bucket, never more than R: rows[k + 1] = min(R, min(B - 1, R) + R / 64)
//   chunks      B / 16: one weighted sum over 16 consecutive buckets each, folded 64 to 1 (fold_a, fold_b) down to one row per column
//
// The call falls back to the ladder route (msm_dev) in constant-time mode and below the window table's threshold, and msm_dev carves ITS
// layout at the start of the buffer: this call's own regions lie BEHIND that inner layout, as dleq_layout.h's do.
#pragma once
#include "work_layout.h"

namespace fq_work {

struct BucketGeom {
    static constexpr unsigned MAX_PASSES = 6, PART = 64, CHUNK = 16, WINDOW_MIN = 4, WINDOW_MAX = 12;
    size_t groups, group_size, n;
    unsigned window, windows;       // c and W = ceil(64 / c)
    size_t digits, cols;            // B = 2^c; groups x 4 x W
    unsigned passes;
    size_t rows[MAX_PASSES + 1];
    size_t chunks, fold1;           // B / 16 weighted sums per column; ceil(chunks / 64) rows behind the first fold pass
    BucketGeom(size_t groups_, size_t group_size_, unsigned window_) : groups(groups_), group_size(group_size_), n(groups_ * group_size_), window(window_) {
        windows = (64 + window - 1) / window;
        digits = (size_t)1 << window;
        cols = groups * 4 * windows;
        passes = 1;
        for (size_t reach = PART; reach < group_size; reach *= PART) passes++;
        rows[0] = group_size;
        for (unsigned k = 0; k < MAX_PASSES; k++) {
            const size_t r = rows[k], filled = r < digits - 1 ? r : digits - 1, bound = filled + r / PART;
            rows[k + 1] = bound < r ? bound : r;
        }
        chunks = digits / CHUNK;
        fold1 = (chunks + 63) / 64;
    }
    static bool window_ok(unsigned window) { return window >= WINDOW_MIN && window <= WINDOW_MAX; }
};

inline size_t round4(size_t x) { return (x + 3) & ~(size_t)3; }

struct Bucket : Leaf {
    BucketGeom g;
    char* inner;                    // Msm, carved by msm_dev itself when the call takes the ladder route
    uint64_t* v;                    // step 1: the four sub-scalars of decompose(k): n x 4 words
    uint64_t* affine;               // bytes flavour: the decoded points, n x 8 words (the affine flavour reads the caller's array)
    uint8_t* st_decode;             // bytes flavour: one raw decode code per element
    uint32_t* group_code;           // the largest decode code of each group: round4(groups) words; zeroed together with `counts` behind it
    uint32_t* counts;               // step 2: cols x B histogram, also the scatter's cursors (counted back down to zero)
    uint32_t *off_a, *off_b;        // cols x (B + 1) exclusive scans each: a pass reads bucket starts from one and its part starts from the other;
                                    // the next pass reads the part starts as its bucket starts and writes the first again
    uint32_t* idx;                  // step 2: element indices sorted by digit: cols x group_size
    uint64_t *rows_a, *rows_b;      // step 3: projective rows of 12 words, cols x rows[1] and cols x rows[2]; the passes alternate a, b, a, ...
    uint64_t* weighted;             // step 4: cols x chunks rows of 12 words
    uint64_t *fold_a, *fold_b;      // ... folded to cols x fold1 and cols x 1 rows (nothing where the pass before already leaves one row)
    uint64_t* endo;                 // step 5: S_0, phi(S_1), psi(S_2), psi(phi(S_3)): groups x 4 rows of 12 words
    uint8_t* st_endo;               // the group's code on each of its four rows
    uint64_t* sum;                  // their sum: groups rows of 12 words, what the lowering reads
    uint8_t* st_sum;
    size_t end;
    Bucket(char* base, size_t groups, size_t group_size, unsigned window) : g(groups, group_size, window) {
        Carver w(base);
        inner = w.take<char>(Msm::bytes(g.n));
        v = w.take<uint64_t>(g.n * 4); affine = w.take<uint64_t>(g.n * 8); st_decode = w.take_status(g.n);
        group_code = w.take<uint32_t>(round4(groups)); counts = w.take<uint32_t>(g.cols * g.digits);
        off_a = w.take<uint32_t>(round4(g.cols * (g.digits + 1))); off_b = w.take<uint32_t>(round4(g.cols * (g.digits + 1)));
        idx = w.take<uint32_t>(g.cols * group_size);
        rows_a = w.take<uint64_t>(g.cols * g.rows[1] * 12); rows_b = w.take<uint64_t>(g.passes > 1 ? g.cols * g.rows[2] * 12 : 0);
        weighted = w.take<uint64_t>(g.cols * g.chunks * 12);
        fold_a = w.take<uint64_t>(g.chunks > 1 ? g.cols * g.fold1 * 12 : 0); fold_b = w.take<uint64_t>(g.fold1 > 1 ? g.cols * 12 : 0);
        endo = w.take<uint64_t>(groups * 4 * 12); st_endo = w.take_status(groups * 4); sum = w.take<uint64_t>(groups * 12); st_sum = w.take_status(groups);
        end = w.used;
    }
    size_t zeroed_bytes() const { return (round4(g.groups) + g.cols * g.digits) * sizeof(uint32_t); }      // group_code and counts, one memset
    static size_t bytes(size_t groups, size_t group_size, unsigned window) { return Bucket(nullptr, groups, group_size, window).end; }
};

}  // namespace fq_work

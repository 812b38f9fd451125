// Where threshold sharing (include/fourq_amd.h, "threshold sharing"; shamir.hip.h) keeps its intermediates in the context's work buffer.
// Plain C++, no HIP, built on work_layout.h's Carver: tests/test_shamir_oracle.py compiles it with g++ (tests/c/shamir_layout_dump.cpp).
//
// As the VRF (vrf_layout.h): the curve work of a call is the library's own protocol calls -- the grouped sum on encodings over rows x t
// elements (combine_points, public_shares, verify) and the comb with its encoding over `rows` scalars (verify) -- so this is a composite
// layout by work_layout.h's rule, its own regions behind `inner`.  rows: output rows (batch rows, groups or sets); t: the threshold;
// n = rows x t items.  The scalar-side calls (shares, combine) use `lambda`, `flags` and `st_set` only.
#pragma once
#include "work_layout.h"

namespace fq_work {

struct ShamirInner {
    // the extent of every layout an inner call carves, at the size it is called with
    static size_t msm_rows(size_t n) { return Msm::bytes(n); }                  // combine_points, public_shares, verify: sum over groups of t
    static size_t comb_encode(size_t rows) { return Sig::bytes(rows); }         // verify: encode([share]G); what the comb with its encoding takes where it has a layout
    static size_t bytes(size_t rows, size_t t) { return most({ msm_rows(rows * t), comb_encode(rows) }); }
};

struct Shamir : Leaf {
    char* inner;                    // what the inner calls carve for themselves
    uint64_t* sc;                   // the grouped sum's scalar rows: lambda tiled over the batch, or the powers of the ids: n x 4 words
    uint64_t* pt;                   // combine_points: the servers' rows transposed into group order: n x 4 words
    uint64_t* lambda;               // combine, combine_points: the coefficients of the call's one id set: t x 4 words
    uint64_t* pub32;                // verify: the verification shares: rows x 4 words
    uint64_t* g32;                  // verify: encode([share]G): rows x 4 words
    uint64_t* affine;               // verify: the comb's affine rows: rows x 8 words
    uint8_t* flags;                 // lagrange: one byte per (set, i), merged into the set's status: n
    uint8_t* st_set;                // combine, combine_points: the status of the call's one id set
    uint8_t *st_pub, *st_comb;      // verify: the grouped sum's status per group; the comb's (FOURQ_DH_NEUTRAL marks [0]G)
    size_t own, end;
    Shamir(char* base, size_t rows, size_t t) {
        Carver w(base);
        const size_t n = rows * t;
        inner = w.take<char>(ShamirInner::bytes(rows, t)); own = w.used;
        sc = w.take<uint64_t>(n * 4); pt = w.take<uint64_t>(n * 4); lambda = w.take<uint64_t>(t * 4);
        pub32 = w.take<uint64_t>(rows * 4); g32 = w.take<uint64_t>(rows * 4); affine = w.take<uint64_t>(rows * 8);
        flags = w.take_status(n); st_set = w.take_status(1); st_pub = w.take_status(rows); st_comb = w.take_status(rows);
        end = w.used;
    }
    static constexpr Planes planes = PLANES_SIZED;        // the comb defers its normalisation into the context's planes: `rows` rows
    static size_t bytes(size_t rows, size_t t) { return Shamir(nullptr, rows, t).end; }
    static size_t inner_extent(size_t rows, size_t t) { return Shamir(nullptr, rows, t).own; }
};

}  // namespace fq_work

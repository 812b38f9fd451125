// Where the batched DLEQ proofs (include/fourq_amd.h, "oblivious PRF: proofs"; dleq.hip.h) keep their intermediates in the context's work
// buffer.  Plain C++, no HIP, built on work_layout.h's Carver: tests/test_dleq_oracle.py compiles it with g++ (tests/c/dleq_layout_dump.cpp).
//
// A proof call is a string of the library's own protocol calls -- the grouped sum, [k]B + [l]P, DH_endo and MUL_endo on encodings, the comb:
// a composite layout by work_layout.h's rule, its own regions behind `inner`, the largest of the inner calls' layouts.
// n = groups x group_size rows; every own region but `d` has one row per group (the comb's have one more: the public key's).
#pragma once
#include "work_layout.h"

namespace fq_work {

struct DleqInner {
    // the extent of every layout an inner call carves, at the size it is called with
    static size_t msm_rows(size_t n) { return Msm::bytes(n); }                          // M = sum [d]C, Z = sum [d]D
    static size_t msm_pair(size_t groups) { return Msm::bytes(2 * groups); }            // [s]M + [c]Z: groups of two
    static size_t double_mul(size_t groups) { return DoubleMul::bytes(groups); }        // [s]G + [c]pk
    static size_t evaluate(size_t groups) { return OprfEvaluate::bytes(groups); }       // Z = DH_endo(k, M); DhBytes lies inside it
    static size_t mul_rows(size_t groups) { return MulRows::bytes(groups); }            // [r]M
    static size_t sig(size_t groups) { return Sig::bytes(groups + 1); }                 // the comb with its encoding: [r]G and the public key
    static size_t bytes(size_t n, size_t groups) { return most({ msm_rows(n), msm_pair(groups), double_mul(groups), evaluate(groups), mul_rows(groups), sig(groups) }); }
};

struct Dleq : Leaf {
    char* inner;                    // what the inner calls carve for themselves
    uint64_t* d;                    // the composite scalars: n x 4 words
    uint64_t* pk;                   // verify: the public key on every group's row (the variable point of [s]G + [c]pk): groups x 4 words
    uint64_t *m32, *z32;            // the composites as 32-byte rows: groups x 4 words each
    uint64_t* t2;                   // prove: encode([r]G) and, on row `groups`, the public key; verify: encode([s]G + [c]pk): (groups + 1) x 4 words
    uint64_t* t3;                   // encode([r]M) / encode([s]M + [c]Z): groups x 4 words
    uint64_t* sc_a;                 // prove: r mod N and, on row `groups`, K = 392 k mod N; verify: s: (groups + 1) x 4 words
    uint64_t* sc_b;                 // prove: the key on every row; verify: c: groups x 4 words
    uint64_t *pair_sc, *pair_pt;    // verify: (s, c) and (M32, Z32) interleaved, the operands of the sum of two: 2 groups x 4 words each
    uint64_t* affine;               // prove: the comb's affine rows: (groups + 1) x 8 words
    uint8_t *st_m, *st_z, *st_t2, *st_t3, *st_pre;      // one status byte per group and stage; st_t2 has groups + 1
    size_t own, end;
    Dleq(char* base, size_t n, size_t groups) {
        Carver w(base);
        const size_t g1 = groups + 1;
        inner = w.take<char>(DleqInner::bytes(n, groups)); own = w.used;
        d = w.take<uint64_t>(n * 4); pk = w.take<uint64_t>(groups * 4); m32 = w.take<uint64_t>(groups * 4); z32 = w.take<uint64_t>(groups * 4);
        t2 = w.take<uint64_t>(g1 * 4); t3 = w.take<uint64_t>(groups * 4); sc_a = w.take<uint64_t>(g1 * 4); sc_b = w.take<uint64_t>(groups * 4);
        pair_sc = w.take<uint64_t>(2 * groups * 4); pair_pt = w.take<uint64_t>(2 * groups * 4); affine = w.take<uint64_t>(g1 * 8);
        st_m = w.take_status(groups); st_z = w.take_status(groups); st_t2 = w.take_status(g1); st_t3 = w.take_status(groups); st_pre = w.take_status(groups);
        end = w.used;
    }
    static constexpr Planes planes = PLANES_SIZED;
    static size_t plane_rows(size_t groups) { return groups + 1; }      // the projective planes: the comb's rows are the most any stage defers
    static size_t plane_rows(size_t, size_t groups) { return plane_rows(groups); }      // as a call sizes them: by the layout's own arguments
    static size_t bytes(size_t n, size_t groups) { return Dleq(nullptr, n, groups).end; }
    static size_t inner_extent(size_t n, size_t groups) { return Dleq(nullptr, n, groups).own; }
};

}  // namespace fq_work

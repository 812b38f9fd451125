// Where the verifiable random function (include/fourq_amd.h, "verifiable random function"; vrf.hip.h) keeps its intermediates in the context's
// work buffer.  Plain C++, no HIP, built on work_layout.h's Carver: tests/test_vrf_oracle.py compiles it with g++ (tests/c/vrf_layout_dump.cpp).
//
// As the DLEQ proofs (dleq_layout.h): a call is a string of the library's own protocol calls -- MUL_endo on encodings, the comb with its
// encoding, [k]B + [l]P, its keyed sibling, the grouped sum over groups of two: a composite layout by work_layout.h's rule, its own regions
// behind `inner`.  n rows; the sum of two has 2 n.
#pragma once
#include "keyset_layout.h"

namespace fq_work {

struct VrfInner {
    // the extent of every layout an inner call carves, at the size it is called with
    static size_t mul_rows(size_t n) { return MulRows::bytes(n); }              // prove: Gamma = [x]Hpt, [r]Hpt
    static size_t double_mul(size_t n) { return DoubleMul::bytes(n); }          // verify: [s]G + [c]Y
    static size_t keyset(size_t n) { return Keyset::bytes(n); }                 // keyed verify: the same through the two combs
    static size_t msm_pair(size_t n) { return Msm::bytes(2 * n); }              // verify: [s]Hpt + [c / 392]W, groups of two
    static size_t bytes(size_t n) { return most({ mul_rows(n), double_mul(n), keyset(n), msm_pair(n) }); }
};

struct Vrf : Leaf {
    char* inner;                    // what the inner calls carve for themselves
    uint64_t* u;                    // hash_to_field's u_0, u_1: n x 8 words; dead once the map has run
    uint64_t* affine;               // prove: the comb's affine rows: n x 8 words ON u -- the comb runs after the map
    uint64_t* pk32;                 // keyed verify: the rows' key bytes, gathered by index: n x 4 words
    uint64_t* h32;                  // encode(Hpt): n x 4 words
    uint64_t* g32;                  // prove: gamma32; verify: w32 = encode([392]Gamma): n x 4 words
    uint64_t *u32, *v32;            // prove: encode([r]G), encode([r]Hpt); verify: encode([s]G + [c]Y), encode([s]Hpt + [c / 392]W): n x 4 words each
    uint64_t* sc_a;                 // prove: x = LE(k[0:32]); verify: s: n x 4 words
    uint64_t* sc_b;                 // prove: r; verify: c: n x 4 words
    uint64_t *pair_sc, *pair_pt;    // verify: (s, c / 392) and (h32, w32) interleaved, the operands of the sum of two: 2 n x 4 words each
    uint8_t *st_a, *st_b, *st_u, *st_v, *st_pre;    // one status byte per row and stage
    size_t own, end;
    Vrf(char* base, size_t n) {
        Carver w(base);
        inner = w.take<char>(VrfInner::bytes(n)); own = w.used;
        u = w.take<uint64_t>(n * 8); affine = u;
        pk32 = w.take<uint64_t>(n * 4); h32 = w.take<uint64_t>(n * 4); g32 = w.take<uint64_t>(n * 4); u32 = w.take<uint64_t>(n * 4); v32 = w.take<uint64_t>(n * 4);
        sc_a = w.take<uint64_t>(n * 4); sc_b = w.take<uint64_t>(n * 4);
        pair_sc = w.take<uint64_t>(2 * n * 4); pair_pt = w.take<uint64_t>(2 * n * 4);
        st_a = w.take_status(n); st_b = w.take_status(n); st_u = w.take_status(n); st_v = w.take_status(n); st_pre = w.take_status(n);
        end = w.used;
    }
    static constexpr Planes planes = PLANES_SIZED;        // the comb and [s]G + [c]Y defer their normalisation into the context's planes: n rows
    static size_t bytes(size_t n) { return Vrf(nullptr, n).end; }
    static size_t inner_extent(size_t n) { return Vrf(nullptr, n).own; }
};

}  // namespace fq_work

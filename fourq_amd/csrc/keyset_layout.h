// Work-buffer layout of the calls over registered keys (include/fourq_amd.h, "signatures of registered keys"; keyset.hip.h).  Plain C++,
// no HIP, built on work_layout.h's Carver: tests/test_keyset_oracle.py compiles it with g++ (tests/c/keyset_layout_dump.cpp).
//
// Default mode: the challenge kernel (or the caller) leaves s, h and R as rows of 32 bytes and one inherited status byte per row, the comb
// kernel one canonical 12-word (X, Y, Z) row, and the lowering reads both.  Constant-time selection runs the existing routes instead:
// `inner` is the region THEY carve (work_layout.h's rule), and pk32 holds the rows' key bytes, gathered by index.
#pragma once
#include "work_layout.h"

namespace fq_work {

struct Keyset : Leaf {
    char* inner;                    // DoubleMul (SigVerify), carved by double_mul_dev / fourq_sig_verify_batch_dev themselves
    uint64_t *s, *h, *r32;          // the verify call: s, h and R as rows of 32 bytes
    uint64_t* rows;                 // [k]B + [l]A_id: n rows of 12 words
    uint8_t* pk32;                  // constant-time selection: n x 32 gathered key bytes
    uint8_t* pre;                   // one inherited status byte per row
    size_t own, end;
    Keyset(char* base, size_t n) {
        Carver w(base);
        inner = w.take<char>(DoubleMul::bytes(n)); own = w.used;
        s = w.take<uint64_t>(n * 4); h = w.take<uint64_t>(n * 4); r32 = w.take<uint64_t>(n * 4);
        rows = w.take<uint64_t>(n * 12);
        pk32 = w.take<uint8_t>(n * 32);
        pre = w.take_status(n);
        end = w.used;
    }
    static constexpr Planes planes = PLANES_SIZED;        // the constant-time route defers the comb's normalisation into the context's planes
    static size_t bytes(size_t n) { return Keyset(nullptr, n).end; }
    static size_t inner_extent(size_t n) { return Keyset(nullptr, n).own; }
};

}  // namespace fq_work

// Where each protocol-level call keeps its intermediates in the context's work buffer (fourq_ctx::work in fourq_amd.hip).  Plain C++, no HIP:
// tests/test_work_layout.py compiles it with g++ (tests/c/work_layout_dump.cpp) and checks every offset and total on the CPU.
//
// One struct per layout: built from (base, n) it hands out its regions as typed pointers, and bytes(n) is where the same carving of n
// elements ends -- size and offsets come from ONE sequence of take() calls, so they cannot drift apart.  Nothing at run time would notice
// if they did: the buffer is grown by free + allocate, and a region carved past a too-small total is somebody else's memory.  Rows are
// multiples of 32 bytes and a status region is align256(n) bytes (one byte per element), so every region starts 16-byte aligned.
//
// A layout that sizes the buffer for a call also says, in `planes`, whether the _dev call behind it may defer a normalisation into the
// context's projective planes (fourq_ctx::proj): what a host-array call sizes for its largest chunk before the first one is enqueued
// (reserve_for<Layout> in fourq_amd.hip).  Every such layout is named once more, in `All` at the end of this file.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace fq_work {

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Bump allocator over [base, ...).  Addresses are computed as integers, so a carving over base == nullptr (bytes(n) below) only counts.
struct Carver {
    uintptr_t base;
    size_t used = 0;
    explicit Carver(char* b) : base(reinterpret_cast<uintptr_t>(b)) {}
    template <class T> T* take(size_t count) { T* p = reinterpret_cast<T*>(base + used); used += count * sizeof(T); return p; }
    uint8_t* take_status(size_t n) { return take<uint8_t>(align256(n)); }
};

struct DhBytes {                    // decode -> DH_* -> encode
    uint64_t *pts, *shared;         // decoded public keys, affine shared points: n x 8 words each
    uint8_t *st_decode, *st_dh;
    size_t end;
    DhBytes(char* base, size_t n) { Carver w(base); pts = w.take<uint64_t>(n * 8); shared = w.take<uint64_t>(n * 8); st_decode = w.take_status(n); st_dh = w.take_status(n); end = w.used; }
    static constexpr bool planes = true;
    static size_t bytes(size_t n) { return DhBytes(nullptr, n).end; }
};
struct Exchange {                   // both exchange calls; the one whose first half goes through the comb leaves base_pts unused
    uint64_t *base_pts, *mid;       // the base point once per exchange, the first half's public keys: n x 8 words each
    uint8_t* st_first;
    size_t end;
    Exchange(char* base, size_t n) { Carver w(base); base_pts = w.take<uint64_t>(n * 8); mid = w.take<uint64_t>(n * 8); st_first = w.take_status(n); end = w.used; }
    static constexpr bool planes = true;
    static size_t bytes(size_t n) { return Exchange(nullptr, n).end; }
};
struct MulRows {                    // MUL_* with affine or encoded I/O
    uint64_t *rows_in, *rows_out;   // affine (fused I/O) or R1 rows of the decoded / lifted points, the ladder's result rows: n x 20 words each
    uint64_t* unused;               // n x 8 words nothing uses: kept, because the total decides at which batch sizes the buffer is reallocated
    uint8_t* st_decode;
    size_t end;
    MulRows(char* base, size_t n) { Carver w(base); rows_in = w.take<uint64_t>(n * 20); rows_out = w.take<uint64_t>(n * 20); unused = w.take<uint64_t>(n * 8); st_decode = w.take_status(n); end = w.used; }
    static constexpr bool planes = false;
    static size_t bytes(size_t n) { return MulRows(nullptr, n).end; }
};
struct SigTail {                    // what the signature check hands the double multiplication
    uint64_t *s, *h, *r32;          // s, h and R as rows of 32 bytes
    uint8_t* pre;                   // one pre-status byte per row
    size_t end;
    SigTail(char* base, size_t n) { Carver w(base); s = w.take<uint64_t>(n * 4); h = w.take<uint64_t>(n * 4); r32 = w.take<uint64_t>(n * 4); pre = w.take_status(n); end = w.used; }
    static size_t bytes(size_t n) { return SigTail(nullptr, n).end; }
};
// [k]B + [l]P.  Its total includes the tail that only the signature check carves: either call asks for the same size, so the double
// multiplication inside a signature check finds the buffer large enough and does not move it.
struct DoubleMul {
    uint64_t *rows_in, *rows_out;   // as MulRows
    uint8_t *st_decode, *st_comb;   // the comb writes FOURQ_DH_OK per element; nobody reads it
    char* tail;
    size_t end;
    DoubleMul(char* base, size_t n) { Carver w(base); rows_in = w.take<uint64_t>(n * 20); rows_out = w.take<uint64_t>(n * 20); st_decode = w.take_status(n); st_comb = w.take_status(n); tail = w.take<char>(SigTail::bytes(n)); end = w.used; }
    static constexpr bool planes = true;
    static size_t bytes(size_t n) { return DoubleMul(nullptr, n).end; }
};
struct SigVerify : DoubleMul {      // the signature check: the double multiplication's layout with its tail carved
    SigTail sig;
    SigVerify(char* base, size_t n) : DoubleMul(base, n), sig(tail, n) {}
};
struct Sig {                        // keygen / sign
    uint64_t *a, *r;                // a = LE(k[0:32]) and the nonce: n x 4 words each
    uint8_t* r32;                   // encode([r]G): n x 32 bytes
    uint64_t* affine;               // the comb's affine rows: n x 8 words
    uint8_t* st_comb;
    size_t end;
    Sig(char* base, size_t n) { Carver w(base); a = w.take<uint64_t>(n * 4); r = w.take<uint64_t>(n * 4); r32 = w.take<uint8_t>(n * 32); affine = w.take<uint64_t>(n * 8); st_comb = w.take_status(n); end = w.used; }
    static constexpr bool planes = true;
    static size_t bytes(size_t n) { return Sig(nullptr, n).end; }
};
struct H2c {                        // hash to curve
    uint64_t* u;                    // u_0, u_1 as rows of 32 bytes: n x 8 words
    size_t end;
    H2c(char* base, size_t n) { Carver w(base); u = w.take<uint64_t>(n * 8); end = w.used; }
    static constexpr bool planes = false;
    static size_t bytes(size_t n) { return H2c(nullptr, n).end; }
};
// Grouped sums out[g] = sum [k]P over groups of one length; n = groups x group_size elements.  A fold pass turns m rows per group into
// ceil(m / 64), which is at most floor(m / 2) for m >= 2: the first pass leaves at most n / 2 rows, the second at most n / 4, and later
// passes alternate between the same two regions with fewer rows still.  392 n bytes + 1.75 n of status, below SigVerify's 416 n + 3 n:
// fourq_ctx_reserve does not grow.
struct Msm {
    uint64_t *rows_in, *rows_out;   // as MulRows
    uint8_t* st_decode;
    uint64_t *part_a, *part_b;      // partial sums, rows of 12 words: n / 2 and n / 4 of them
    uint8_t *st_a, *st_b;           // the largest decode code among a partial sum's elements
    size_t end;
    Msm(char* base, size_t n) { Carver w(base); rows_in = w.take<uint64_t>(n * 20); rows_out = w.take<uint64_t>(n * 20); st_decode = w.take_status(n); part_a = w.take<uint64_t>(n / 2 * 12); st_a = w.take_status(n / 2); part_b = w.take<uint64_t>(n / 4 * 12); st_b = w.take_status(n / 4); end = w.used; }
    static constexpr bool planes = false;
    static size_t bytes(size_t n) { return Msm(nullptr, n).end; }
};
// ---- the oblivious PRF (oprf.hip.h).  Each of the four totals is below SigVerify's 416 n + 3 n (blind and finalize: 384 n + n and
// 384 n + 3 n of status; evaluate: DhBytes + 32 n; eval: 192 n + n): fourq_ctx_reserve does not grow.
struct OprfBlind {                  // hash to curve -> MUL_endo by the blind -> encode
    uint64_t* pts;                  // G(msg) as affine words: n x 8
    uint64_t *rows_in, *rows_out;   // as MulRows
    uint64_t* u;                    // u_0, u_1: n x 8 words ON rows_in -- u is dead once the map has run, and the lift that fills rows_in comes after it
    uint8_t* st_decode;             // all zero (the points come from the map, not from a decode): what lower_kernel<K, true> reads
    size_t end;
    OprfBlind(char* base, size_t n) { Carver w(base); pts = w.take<uint64_t>(n * 8); rows_in = w.take<uint64_t>(n * 20); u = rows_in; rows_out = w.take<uint64_t>(n * 20); st_decode = w.take_status(n); end = w.used; }
    static constexpr bool planes = false;
    static size_t bytes(size_t n) { return OprfBlind(nullptr, n).end; }
};
struct OprfEvaluate {               // the key on n scalar rows -> decode -> DH_endo -> encode
    char* dh;                       // DhBytes, carved by the DH call itself: it asks for less than this layout's total and moves nothing
    uint64_t* keys;                 // n x 4 words
    size_t end;
    OprfEvaluate(char* base, size_t n) { Carver w(base); dh = w.take<char>(DhBytes::bytes(n)); keys = w.take<uint64_t>(n * 4); end = w.used; }
    static constexpr bool planes = true;
    static size_t bytes(size_t n) { return OprfEvaluate(nullptr, n).end; }
};
struct OprfFinalize {               // 1 / blind -> decode -> MUL_endo -> encode -> hash
    uint64_t* inv;                  // the inverted blinds: n x 4 words
    uint64_t *rows_in, *rows_out;   // as MulRows
    uint64_t* e32;                  // the unblinded element as 32 bytes: n x 4 words
    uint8_t *st_decode, *st_lower;  // decode's codes, and 16 + code as the lowering reports them
    uint8_t* st_zero;               // FOURQ_OPRF_BLIND_ZERO where the blind is 0 mod N
    size_t end;
    OprfFinalize(char* base, size_t n) { Carver w(base); inv = w.take<uint64_t>(n * 4); rows_in = w.take<uint64_t>(n * 20); rows_out = w.take<uint64_t>(n * 20); e32 = w.take<uint64_t>(n * 4); st_decode = w.take_status(n); st_lower = w.take_status(n); st_zero = w.take_status(n); end = w.used; }
    static constexpr bool planes = false;
    static size_t bytes(size_t n) { return OprfFinalize(nullptr, n).end; }
};
struct OprfEval {                   // hash to curve -> DH_endo by the key -> encode -> hash
    uint64_t* pts;                  // G(msg) as affine words: n x 8
    uint64_t* shared;               // DH_endo's affine result: n x 8
    uint64_t* u;                    // n x 8 words ON shared: dead once the map has run, before DH_endo writes there
    uint64_t *keys, *e32;           // the key on n scalar rows, the evaluated element as 32 bytes: n x 4 words each
    uint8_t* st_dh;
    size_t end;
    OprfEval(char* base, size_t n) { Carver w(base); pts = w.take<uint64_t>(n * 8); shared = w.take<uint64_t>(n * 8); u = shared; keys = w.take<uint64_t>(n * 4); e32 = w.take<uint64_t>(n * 4); st_dh = w.take_status(n); end = w.used; }
    static constexpr bool planes = true;
    static size_t bytes(size_t n) { return OprfEval(nullptr, n).end; }
};

// Every layout a call sizes the work buffer by: fourq_ctx_reserve allocates max_bytes(n), so that no _dev call of at most n elements
// reallocates.  SigTail is not one of them (it is carved inside DoubleMul's tail, whose total includes it), and SigVerify is DoubleMul's
// carving with that tail opened: the same total.  tests/test_work_layout.py compares this list with the structs of this file.
template <class... L> struct Layouts {
    static size_t max_bytes(size_t n) { size_t most = 0; for (size_t b : { L::bytes(n)... }) if (b > most) most = b; return most; }
};
using All = Layouts<DhBytes, Exchange, MulRows, DoubleMul, Sig, H2c, Msm, OprfBlind, OprfEvaluate, OprfFinalize, OprfEval>;

}  // namespace fq_work

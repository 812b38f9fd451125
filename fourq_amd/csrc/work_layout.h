// Where each protocol-level call keeps its intermediates in the context's work buffer (fourq_ctx::work in fourq_amd.hip).  Plain C++, no HIP:
// tests/test_work_layout.py compiles it with g++ (tests/c/work_layout_dump.cpp) and checks every offset and total on the CPU.
//
// One struct per layout: built from (base, n) it hands out its regions as typed pointers, and bytes(n) is where the same carving of n
// elements ends -- size and offsets come from ONE sequence of take() calls, so they cannot drift apart.  Rows are multiples of 32 bytes
// and a status region is align256(n) bytes (one byte per element), so every region starts 16-byte aligned.
// THE RULE by which calls share the buffer.  Every call carves its layout from the buffer's first byte, also a call made by another call.  A
// composite layout therefore begins with the room its inner calls carve and keeps the regions that carry values across them behind it:
// inner_extent(...) is where that room ends, the offset of the first own region (0: no inner call).  The outermost call sizes the buffer and may
// move it; while its layout is open, an inner call's layout must end within the inner extent of the layout open above it and within what the
// buffer holds: `Hold` keeps that book, and WorkScope in fourq_amd.hip refuses a nested call that does not fit.  DoubleMul alone lends room, the
// tail that only the signature check carves (lent(n)): nested there it must fit without it.  `planes`: who sizes the context's projective planes
// for the call, plane_rows(...) rows of them.  `All` at the end names every layout of this file that sizes the buffer.
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
enum Planes { PLANES_NONE, PLANES_SIZED, PLANES_BY_DH };     // not used; sized with the work buffer; left to dh_dev, which sizes them if it defers
struct Leaf {                       // what a layout says unless it says otherwise: no inner call, no room lent, one plane row per element, if any
    template <class... A> static size_t inner_extent(A...) { return 0; }
    template <class... A> static size_t lent(A...) { return 0; }
    template <class... A> static size_t plane_rows(size_t n, A...) { return n; }
    static constexpr Planes planes = PLANES_NONE;
};
// The book of one buffer while calls are using it: how deep the open layouts nest, what the buffer held when the outermost had sized it, and how
// much of that a layout opened now may carve.  A scope keeps its parent's Hold and puts it back when it closes.  Stage and planes: extent == held.
struct Hold {
    const char* who = nullptr;      // the innermost open layout, for the refusal's message
    size_t held = 0, extent = 0;
    int depth = 0;
    bool admits(size_t need) const { return depth == 0 || (need <= extent && need <= held); }      // depth 0: nobody holds it, it may grow
    Hold opened(const char* name, size_t held_now, size_t inner_extent) const { return { name, depth ? held : held_now, inner_extent, depth + 1 }; }
};

struct DhBytes : Leaf {             // decode -> DH_* -> encode
    uint64_t *pts, *shared;         // decoded public keys, affine shared points: n x 8 words each
    uint8_t *st_decode, *st_dh;
    size_t end;
    DhBytes(char* base, size_t n) { Carver w(base); pts = w.take<uint64_t>(n * 8); shared = w.take<uint64_t>(n * 8); st_decode = w.take_status(n); st_dh = w.take_status(n); end = w.used; }
    static constexpr Planes planes = PLANES_BY_DH;
    static size_t bytes(size_t n) { return DhBytes(nullptr, n).end; }
};
struct Exchange : Leaf {            // both exchange calls; the one whose first half goes through the comb leaves base_pts unused
    uint64_t *base_pts, *mid;       // the base point once per exchange, the first half's public keys: n x 8 words each
    uint8_t* st_first;
    size_t end;
    Exchange(char* base, size_t n) { Carver w(base); base_pts = w.take<uint64_t>(n * 8); mid = w.take<uint64_t>(n * 8); st_first = w.take_status(n); end = w.used; }
    static constexpr Planes planes = PLANES_BY_DH;
    static size_t bytes(size_t n) { return Exchange(nullptr, n).end; }
};
struct MulRows : Leaf {             // MUL_* with affine or encoded I/O
    uint64_t *rows_in, *rows_out;   // affine (fused I/O) or R1 rows of the decoded / lifted points, the ladder's result rows: n x 20 words each
    uint64_t* unused;               // n x 8 words nothing uses: kept, because the total decides at which batch sizes the buffer is reallocated
    uint8_t* st_decode;
    size_t end;
    MulRows(char* base, size_t n) { Carver w(base); rows_in = w.take<uint64_t>(n * 20); rows_out = w.take<uint64_t>(n * 20); unused = w.take<uint64_t>(n * 8); st_decode = w.take_status(n); end = w.used; }
    static size_t bytes(size_t n) { return MulRows(nullptr, n).end; }
};
struct SigTail {                    // what the signature check hands the double multiplication
    uint64_t *s, *h, *r32;          // s, h and R as rows of 32 bytes
    uint8_t* pre;                   // one pre-status byte per row
    size_t end;
    SigTail(char* base, size_t n) { Carver w(base); s = w.take<uint64_t>(n * 4); h = w.take<uint64_t>(n * 4); r32 = w.take<uint64_t>(n * 4); pre = w.take_status(n); end = w.used; }
    static size_t bytes(size_t n) { return SigTail(nullptr, n).end; }
};
struct DoubleMul : Leaf {           // [k]B + [l]P.  Its total includes the tail that only the signature check carves: both size the buffer alike
    uint64_t *rows_in, *rows_out;   // as MulRows
    uint8_t *st_decode, *st_comb;   // the comb writes FOURQ_DH_OK per element; nobody reads it
    char* tail;
    size_t own, end;                // own: where the call's own regions end and the tail begins
    DoubleMul(char* base, size_t n) { Carver w(base); rows_in = w.take<uint64_t>(n * 20); rows_out = w.take<uint64_t>(n * 20); st_decode = w.take_status(n); st_comb = w.take_status(n); own = w.used; tail = w.take<char>(SigTail::bytes(n)); end = w.used; }
    static constexpr Planes planes = PLANES_SIZED;
    static size_t bytes(size_t n) { return DoubleMul(nullptr, n).end; }
    static size_t lent(size_t n) { const DoubleMul w(nullptr, n); return w.end - w.own; }
};
struct SigVerify : DoubleMul {      // the signature check: the double multiplication's layout with its tail carved
    SigTail sig;
    SigVerify(char* base, size_t n) : DoubleMul(base, n), sig(tail, n) {}
    static size_t inner_extent(size_t n) { return DoubleMul(nullptr, n).own; }      // the double multiplication, without the tail it lends
    static size_t lent(size_t) { return 0; }
};
struct Sig : Leaf {                 // keygen / sign
    uint64_t *a, *r;                // a = LE(k[0:32]) and the nonce: n x 4 words each
    uint8_t* r32;                   // encode([r]G): n x 32 bytes
    uint64_t* affine;               // the comb's affine rows: n x 8 words
    uint8_t* st_comb;
    size_t end;
    Sig(char* base, size_t n) { Carver w(base); a = w.take<uint64_t>(n * 4); r = w.take<uint64_t>(n * 4); r32 = w.take<uint8_t>(n * 32); affine = w.take<uint64_t>(n * 8); st_comb = w.take_status(n); end = w.used; }
    static constexpr Planes planes = PLANES_SIZED;
    static size_t bytes(size_t n) { return Sig(nullptr, n).end; }
};
struct H2c : Leaf {                 // hash to curve
    uint64_t* u;                    // u_0, u_1 as rows of 32 bytes: n x 8 words
    size_t end;
    H2c(char* base, size_t n) { Carver w(base); u = w.take<uint64_t>(n * 8); end = w.used; }
    static size_t bytes(size_t n) { return H2c(nullptr, n).end; }
};
// Grouped sums out[g] = sum [k]P over groups of one length; n = groups x group_size elements.  A fold pass turns m rows per group into
// ceil(m / 64), which is at most floor(m / 2) for m >= 2: the first pass leaves at most n / 2 rows, the second at most n / 4, and later
// passes alternate between the same two regions with fewer rows still.  392 n bytes + 1.75 n of status, below SigVerify's 416 n + 3 n:
// fourq_ctx_reserve does not grow.
struct Msm : Leaf {
    uint64_t *rows_in, *rows_out;   // as MulRows
    uint8_t* st_decode;
    uint64_t *part_a, *part_b;      // partial sums, rows of 12 words: n / 2 and n / 4 of them
    uint8_t *st_a, *st_b;           // the largest decode code among a partial sum's elements
    size_t end;
    Msm(char* base, size_t n) { Carver w(base); rows_in = w.take<uint64_t>(n * 20); rows_out = w.take<uint64_t>(n * 20); st_decode = w.take_status(n); part_a = w.take<uint64_t>(n / 2 * 12); st_a = w.take_status(n / 2); part_b = w.take<uint64_t>(n / 4 * 12); st_b = w.take_status(n / 4); end = w.used; }
    static size_t bytes(size_t n) { return Msm(nullptr, n).end; }
};
// ---- the oblivious PRF (oprf.hip.h).  Each of the four totals is below SigVerify's 416 n + 3 n (blind and finalize: 384 n + n and
// 384 n + 3 n of status; evaluate: DhBytes + 32 n; eval: 192 n + n): fourq_ctx_reserve does not grow.
struct OprfBlind : Leaf {           // hash to curve -> MUL_endo by the blind -> encode
    uint64_t* pts;                  // G(msg) as affine words: n x 8
    uint64_t *rows_in, *rows_out;   // as MulRows
    uint64_t* u;                    // u_0, u_1: n x 8 words ON rows_in -- u is dead once the map has run, and the lift that fills rows_in comes after it
    uint8_t* st_decode;             // all zero (the points come from the map, not from a decode): what lower_kernel<K, true> reads
    size_t end;
    OprfBlind(char* base, size_t n) { Carver w(base); pts = w.take<uint64_t>(n * 8); rows_in = w.take<uint64_t>(n * 20); u = rows_in; rows_out = w.take<uint64_t>(n * 20); st_decode = w.take_status(n); end = w.used; }
    static size_t bytes(size_t n) { return OprfBlind(nullptr, n).end; }
};
struct OprfEvaluate : Leaf {        // the key on n scalar rows -> decode -> DH_endo -> encode
    char* dh;                       // DhBytes, carved by the DH call itself
    uint64_t* keys;                 // n x 4 words
    size_t own, end;
    OprfEvaluate(char* base, size_t n) { Carver w(base); dh = w.take<char>(DhBytes::bytes(n)); own = w.used; keys = w.take<uint64_t>(n * 4); end = w.used; }
    static constexpr Planes planes = PLANES_BY_DH;
    static size_t bytes(size_t n) { return OprfEvaluate(nullptr, n).end; }
    static size_t inner_extent(size_t n) { return OprfEvaluate(nullptr, n).own; }
};
struct OprfFinalize : Leaf {        // 1 / blind -> decode -> MUL_endo -> encode -> hash
    uint64_t* inv;                  // the inverted blinds: n x 4 words
    uint64_t *rows_in, *rows_out;   // as MulRows
    uint64_t* e32;                  // the unblinded element as 32 bytes: n x 4 words
    uint8_t *st_decode, *st_lower;  // decode's codes, and 16 + code as the lowering reports them
    uint8_t* st_zero;               // FOURQ_OPRF_BLIND_ZERO where the blind is 0 mod N
    size_t end;
    OprfFinalize(char* base, size_t n) { Carver w(base); inv = w.take<uint64_t>(n * 4); rows_in = w.take<uint64_t>(n * 20); rows_out = w.take<uint64_t>(n * 20); e32 = w.take<uint64_t>(n * 4); st_decode = w.take_status(n); st_lower = w.take_status(n); st_zero = w.take_status(n); end = w.used; }
    static size_t bytes(size_t n) { return OprfFinalize(nullptr, n).end; }
};
struct OprfEval : Leaf {            // hash to curve -> DH_endo by the key -> encode -> hash
    uint64_t* pts;                  // G(msg) as affine words: n x 8
    uint64_t* shared;               // DH_endo's affine result: n x 8
    uint64_t* u;                    // n x 8 words ON shared: dead once the map has run, before DH_endo writes there
    uint64_t *keys, *e32;           // the key on n scalar rows, the evaluated element as 32 bytes: n x 4 words each
    uint8_t* st_dh;
    size_t end;
    OprfEval(char* base, size_t n) { Carver w(base); pts = w.take<uint64_t>(n * 8); shared = w.take<uint64_t>(n * 8); u = shared; keys = w.take<uint64_t>(n * 4); e32 = w.take<uint64_t>(n * 4); st_dh = w.take_status(n); end = w.used; }
    static constexpr Planes planes = PLANES_BY_DH;
    static size_t bytes(size_t n) { return OprfEval(nullptr, n).end; }
};

// Every layout a call sizes the work buffer by: fourq_ctx_reserve allocates max_bytes(n), so that no _dev call of at most n elements
// reallocates.  SigTail is not one of them (it is carved inside DoubleMul's tail, whose total includes it), and SigVerify is DoubleMul's
// carving with that tail opened: the same total.  tests/test_work_layout.py compares this list with the structs of this file.
inline size_t most(std::initializer_list<size_t> totals) { size_t m = 0; for (size_t b : totals) if (b > m) m = b; return m; }
template <class... L> struct Layouts {
    static size_t max_bytes(size_t n) { return most({ L::bytes(n)... }); }
};
using All = Layouts<DhBytes, Exchange, MulRows, DoubleMul, Sig, H2c, Msm, OprfBlind, OprfEvaluate, OprfFinalize, OprfEval>;

}  // namespace fq_work

// The step every protocol ends with: a projective (X, Y, Z) becomes what the caller gets.  One spelling of
//
//   the slots of a lane    lane t of a kernel that gives K elements to a lane owns elements t, t + T, ..., t + (K-1) T with T = ceil(n / K);
//                          a slot past the end of the batch redoes the lane's first element and stores nothing (LaneSlots)
//   the shared inversion   Montgomery's trick inside a lane: the lane multiplies its K elements up, inverts the product ONCE and peels the
//                          individual inverses off on the way back (SharedInverse).  A masked element enters the product as a 1, so it
//                          cannot touch the other K - 1 elements of its lane; what its own result means is the caller's business
//   R1toAffine             curve4q.py:103-106 with GFp2.inv = conj / norm (fields.py:193-199): the elements that are multiplied up are the
//                          norms |Z|^2 in GF(p), and 1 / Z = conj(Z) / |Z|^2.  Z != 0 for every point of the curve (the addition law is
//                          complete); Z = 0 comes from pairs of field elements that are no point (MUL_* checks nothing, and a key that fails to
//                          decode is lifted as the all-zero pair).  Masked, such an element gets conj(0) * (...) = (0, 0), which is also what
//                          0^(p-2) = 0 gives the reference and an unmasked lane of one element
//   the tails              canonical words by 16-byte stores (put_words), and three ways a result leaves: affine words, a 32-byte encoding with a
//                          status byte, the verdict "the encoding equals the expected one".  (The DH tail -- a neutral result is refused, a
//                          zero row on any status -- stays spelled out in ladder_kernel, comb_kernel and normalize_kernel, kernels.hip.h:
//                          behind any helper hipcc schedules those three kernels differently, and their code is held to what was measured.)
//
// The first two are plain C++ behind FQ_HD and compile for the host as well (as the recoders of recode.hip.h do): tests/c/shared_inverse_check.cpp
// runs them over a toy field on the CPU, under the sanitizers too.  The rest is device code and exists under hipcc only.
#pragma once
#if defined(__HIPCC__)
#include "../../include/fourq_amd.h"
#include "curve.hip.h"
#define FQ_HD __host__ __device__ __forceinline__
#else
#include <stdint.h>
namespace fq {
typedef uint32_t u32;
typedef uint64_t u64;
}
#define FQ_HD inline
#endif

namespace fq {

// Two steps on purpose, T from n before the caller's lane index is formed: a constructor (n, t) evaluates t first, and every kernel's listing moves.
template <int K> struct LaneSlots {
    u32 n, T, t;
    FQ_HD explicit LaneSlots(u32 n_) : n(n_), T((n_ + K - 1) / K), t(0) {}
    FQ_HD bool lane(u32 t_) { t = t_; return t < T; }               // false: a lane past the last first slot owns nothing
    FQ_HD u32 id(int j) const { return t + (u32)j * T; }
    FQ_HD bool live(int j) const { return id(j) < n; }
    FQ_HD u32 at(int j) const { return live(j) ? id(j) : t; }       // the row slot j loads: always < n
};

// Ops: struct { typedef ... E; static E one(); static E mul(E, E); static E inv(E); static E select(bool keep, E x, E y); }, select branch-free.
// take(0), ..., take(K - 1) in this order, then invert(), then peel(K - 1), ..., peel(0) in THIS order: peel(j) turns 1 / (e_0 ... e_j) into
// 1 / e_j by the prefix product in front of it and strips e_j from the running inverse -- the other way round is right for K = 1 only.
// The callers' loops over j are unrolled in full (#pragma clang loop unroll(full)): left to its size heuristics the compiler walks nz[] and
// pre[] in scratch memory by a run-time index.  When take(j) happens is the caller's choice: in a pass of its own, or inside its loading loop.
template <int K, typename Ops> struct SharedInverse {
    typedef typename Ops::E E;
    E nz[K], pre[K], inv;
    FQ_HD void take(int j, const E& e) {
        nz[j] = e;
        if (j == 0) pre[0] = nz[0]; else pre[j] = Ops::mul(pre[j - 1], nz[j]);
    }
    FQ_HD void take(int j, const E& e, bool keep) { take(j, Ops::select(keep, e, Ops::one())); }      // !keep: masked
    FQ_HD void invert() { inv = Ops::inv(pre[K - 1]); }
    FQ_HD E peel(int j) {
        E r = inv;
        if (j > 0) { r = Ops::mul(inv, pre[j - 1]); inv = Ops::mul(inv, nz[j]); }
        return r;
    }
};

#if defined(__HIPCC__)
namespace {
// GF(p) for the template; INLINE: the chain in the caller's body instead of a call (fp127.hip.h, fe_inv_inline: normalize_kernel)
template <bool INLINE> struct FeOps {
    typedef Fe<1> E;
    static FQ_DEV Fe<1> one() { Fe<1> r; r.l[0] = 1; r.l[1] = r.l[2] = r.l[3] = r.l[4] = 0; return r; }
    static FQ_DEV Fe<1> mul(const Fe<1>& a, const Fe<1>& b) { return fe_mul(a, b); }
    static FQ_DEV Fe<1> inv(const Fe<1>& a) { if constexpr (INLINE) return fe_inv_inline(a); else return fe_inv(a); }
    static FQ_DEV Fe<1> select(bool keep, const Fe<1>& x, const Fe<1>& y) { return fe_select(keep ? ~0u : 0u, x, y); }
};
FQ_DEV Fe<1> z_norm(const Fe2<1>& z) { return fe_carry(fe_add(fe_sqr(z.re), fe_sqr(z.im))); }
FQ_DEV Fe2<1> z_inverse(const Fe2<1>& z, const Fe<1>& ninv) {        // ninv = 1 / |Z|^2
    Fe2<1> zi;
    zi.re = fe_mul(ninv, z.re);
    zi.im = fe_mul(ninv, fe_neg(z.im));
    return zi;
}

// N canonical words, one 16-byte store per two; dst is 16-byte aligned
template <int N> FQ_DEV void put_words(u64* dst, const u64* w) {
    static_assert(N % 2 == 0, "whole 16-byte stores");
    uint4* q = reinterpret_cast<uint4*>(dst);
#pragma clang loop unroll(full)
    for (int k = 0; k < N / 2; k++) q[k] = make_uint4((u32)w[2 * k], (u32)(w[2 * k] >> 32), (u32)w[2 * k + 1], (u32)(w[2 * k + 1] >> 32));
}
FQ_DEV bool encoding_equals(const u64* expect_row, const u64 w[4]) {
    const uint4* e = reinterpret_cast<const uint4*>(expect_row);
    const uint4 e0 = e[0], e1 = e[1];
    return e0.x == (u32)w[0] && e0.y == (u32)(w[0] >> 32) && e0.z == (u32)w[1] && e0.w == (u32)(w[1] >> 32) &&
           e1.x == (u32)w[2] && e1.y == (u32)(w[2] >> 32) && e1.z == (u32)w[3] && e1.w == (u32)(w[3] >> 32);
}
// a raw decode code as the *_bytes_* calls report it
FQ_DEV uint8_t bytes_decode_status(uint8_t code) { return code ? (uint8_t)(FOURQ_BYTES_DECODE_BASE + code) : (uint8_t)0; }

// ---- the tails: element `id` of the batch leaves as ...
// ... 8 canonical affine words
FQ_DEV void put_affine(u64* out, u32 id, const Fe2<1>& x, const Fe2<1>& y) {
    u64 o[8];
    store_fe2(o, x); store_fe2(o + 4, y);
    put_words<8>(out + 8 * (size_t)id, o);
}
// ... its encoding (curve4q.py:41-47), all zero unless st == 0, and st
FQ_DEV void put_encoded(u64* out, uint8_t* status, u32 id, const Fe2<1>& x, const Fe2<1>& y, uint8_t st) {
    u64 w[4];
    point_encode(x, y, w);
    if (st) w[0] = w[1] = w[2] = w[3] = 0;
    put_words<4>(out + 4 * (size_t)id, w);
    status[id] = st;
}
// ... one byte "its encoding is expect[id], and st == 0", and st
FQ_DEV void put_verdict(const u64* expect, uint8_t* ok, uint8_t* status, u32 id, const Fe2<1>& x, const Fe2<1>& y, uint8_t st) {
    u64 w[4];
    point_encode(x, y, w);
    const bool same = encoding_equals(expect + 4 * (size_t)id, w);
    ok[id] = (same && !st) ? (uint8_t)1 : (uint8_t)0;
    status[id] = st;
}
}  // namespace
#endif      // __HIPCC__

}  // namespace fq

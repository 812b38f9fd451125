// The field arithmetic hipcc compiles from C++ (fp127.hip.h, pair.hip.h, curve.hip.h), one template instantiation per launch on raw limbs
// (tests/test_gpu_field_corners.py).  Each lane loads its record of 128 words, runs ONE entry of FQ_PROBE_TABLE on it and stores raw limbs,
// canonical words or a verdict.  Record layout, mirrored by tests/field_model.py: operand k of an entry at words 10k.. (a GF(p^2) element
// re|im, a GF(p) element or a lane's half in the first five), a table entry's coordinates at words 64 + 12c (16-byte aligned, as the
// library's limb slots), the mask of a conditional negation at word 120; output m at words 10m...  Two- and four-lane entries: element k
// lives in lanes 2k, 2k+1 (4k..4k+3) and each lane's record holds that lane's halves, as pair.hip.h holds them in registers.
// The id of an entry is its position in FQ_PROBE_TABLE; the Python side reads the table from this file's text.
#include "pair.hip.h"

namespace {
using namespace fq;

constexpr int WORDS = 128, ENTRY_AT = 64, MASK_AT = 120;

template <int B> FQ_DEV Fe<B> ldf(const u32* r, int base) {
    Fe<B> x;
#pragma unroll
    for (int i = 0; i < 5; i++) x.l[i] = r[base + i];
    return x;
}
template <int B> FQ_DEV Fe2<B> ld2(const u32* r, int base) {
    Fe2<B> x; x.re = ldf<B>(r, base); x.im = ldf<B>(r, base + 5); return x;
}
template <int B> FQ_DEV PF<B> ldp(const u32* r, int base) {
    PF<B> x;
#pragma unroll
    for (int i = 0; i < 5; i++) x.l[i] = r[base + i];
    return x;
}
template <int B> FQ_DEV void st(u32* w, int base, const Fe<B>& x) {
#pragma unroll
    for (int i = 0; i < 5; i++) w[base + i] = x.l[i];
}
template <int B> FQ_DEV void st(u32* w, int base, const Fe2<B>& x) { st(w, base, x.re); st(w, base + 5, x.im); }
template <int B> FQ_DEV void st(u32* w, int base, const PF<B>& x) {
#pragma unroll
    for (int i = 0; i < 5; i++) w[base + i] = x.l[i];
}
FQ_DEV void st_words(u32* w, u64 lo, u64 hi) { w[0] = (u32)lo; w[1] = (u32)(lo >> 32); w[2] = (u32)hi; w[3] = (u32)(hi >> 32); }
FQ_DEV R1 ld_r1(const u32* r) {
    R1 q; q.X = ld2<1>(r, 0); q.Y = ld2<1>(r, 10); q.Z = ld2<1>(r, 20); q.Ta = ld2<4>(r, 30); q.Tb = ld2<2>(r, 40); return q;
}
FQ_DEV void st_r1(u32* w, const R1& q) { st(w, 0, q.X); st(w, 10, q.Y); st(w, 20, q.Z); st(w, 30, q.Ta); st(w, 40, q.Tb); }
FQ_DEV PR1 ld_pr1(const u32* r) {
    PR1 q; q.X = ldp<1>(r, 0); q.Y = ldp<1>(r, 10); q.Z = ldp<1>(r, 20); q.Ta = ldp<3>(r, 30); q.Tb = ldp<2>(r, 40); return q;
}
FQ_DEV void st_pr1(u32* w, const PR1& q) { st(w, 0, q.X); st(w, 10, q.Y); st(w, 20, q.Z); st(w, 30, q.Ta); st(w, 40, q.Tb); }

// an entry: NAME<A, B>::run(record in, record out, the lane's pair and quad roles); B is 0 where the function has one bound
#define FQ_OP(NAME, ...)                                                                                              \
    template <int A, int B> struct NAME {                                                                             \
        static FQ_DEV void run(const u32* r, u32* w, const PairLane& pl, const QuadLane& ql) { (void)pl; (void)ql; __VA_ARGS__ } \
    };
// ---- products and squares
FQ_OP(FeMul, st(w, 0, fe_mul(ldf<A>(r, 0), ldf<B>(r, 10)));)
FQ_OP(FeSqr, st(w, 0, fe_sqr(ldf<A>(r, 0)));)
FQ_OP(Fe2MulPlain, st(w, 0, fe2_mulx<Mul::Plain>(ld2<A>(r, 0), ld2<B>(r, 10)));)
FQ_OP(Fe2MulChain, st(w, 0, fe2_mulx<Mul::Chain>(ld2<A>(r, 0), ld2<B>(r, 10)));)
FQ_OP(Fe2MulSigned, st(w, 0, fe2_mulx<Mul::Signed>(ld2<A>(r, 0), ld2<B>(r, 10)));)
FQ_OP(Fe2MulGen, st(w, 0, fe2_mulx<Mul::Gen>(ld2<A>(r, 0), ld2<B>(r, 10)));)
FQ_OP(Fe2SqrPlain, st(w, 0, fe2_sqrx<Mul::Plain>(ld2<A>(r, 0)));)
FQ_OP(Fe2SqrChain, st(w, 0, fe2_sqrx<Mul::Chain>(ld2<A>(r, 0)));)
FQ_OP(Fe2SqrSigned, st(w, 0, fe2_sqrx<Mul::Signed>(ld2<A>(r, 0)));)
FQ_OP(Fe2SqrGen, st(w, 0, fe2_sqrx<Mul::Gen>(ld2<A>(r, 0)));)
FQ_OP(PMul, st(w, 0, pmul(ldp<A>(r, 0), ldp<B>(r, 10), pl));)
FQ_OP(PMulConst, st(w, 0, pmul_const(ldp<A>(r, 0), ld2<1>(r, 10), pl));)      // the constant: both halves in every lane's record
FQ_OP(PSqr, st(w, 0, psqr(ldp<A>(r, 0), pl));)
// ---- lazy operations and exits
FQ_OP(FeAdd, st(w, 0, fe_add(ldf<A>(r, 0), ldf<B>(r, 10)));)
FQ_OP(FeSub, st(w, 0, fe_sub(ldf<A>(r, 0), ldf<B>(r, 10)));)
FQ_OP(FeNeg, st(w, 0, fe_neg(ldf<A>(r, 0)));)
FQ_OP(FeCneg, st(w, 0, fe_cneg(ldf<A>(r, 0), r[MASK_AT]));)
FQ_OP(Fe2Conj, st(w, 0, fe2_conj(ld2<A>(r, 0)));)
FQ_OP(FeCarry, st(w, 0, fe_carry(ldf<A>(r, 0)));)
FQ_OP(FeSubSigned, st(w, 0, fe_sub_signed(ldf<A>(r, 0), ldf<B>(r, 10)));)
FQ_OP(FeNegSigned, st(w, 0, fe_neg_signed(ldf<A>(r, 0)));)
FQ_OP(FeCnegSigned, st(w, 0, fe_cneg_signed(ldf<A>(r, 0), r[MASK_AT]));)
FQ_OP(FeUnsign, st(w, 0, fe_unsign(ldf<A>(r, 0)));)
FQ_OP(FeUnsignWide, st(w, 0, fe_unsign_wide(ldf<A>(r, 0)));)
FQ_OP(PAdd, st(w, 0, padd(ldp<A>(r, 0), ldp<B>(r, 10)));)
FQ_OP(PSub, st(w, 0, psub(ldp<A>(r, 0), ldp<B>(r, 10)));)
FQ_OP(PCneg, st(w, 0, pcneg(ldp<A>(r, 0), r[MASK_AT]));)
FQ_OP(PConj, st(w, 0, pconj(ldp<A>(r, 0), pl));)
FQ_OP(PTighten, st(w, 0, ptighten(ldp<A>(r, 0)));)
// ---- canonical form and verdicts
FQ_OP(FeCanon, u64 lo; u64 hi; fe_canon(ldf<A>(r, 0), lo, hi); st_words(w, lo, hi);)
FQ_OP(FeIsZero, w[0] = fe_is_zero(ldf<A>(r, 0)) ? 1u : 0u;)
FQ_OP(FeEqual, w[0] = fe_equal(ldf<A>(r, 0), ldf<B>(r, 10)) ? 1u : 0u;)
FQ_OP(Fe2Equal, w[0] = fe2_equal(ld2<A>(r, 0), ld2<B>(r, 10)) ? 1u : 0u;)
FQ_OP(PairCanon, u64 lo; u64 hi; pair_canon(ldp<A>(r, 0), lo, hi); st_words(w, lo, hi);)
// ---- the group law on the same limbs
FQ_OP(DblPlain, st_r1(w, dbl<Mul::Plain>(ld2<1>(r, 0), ld2<1>(r, 10), ld2<1>(r, 20)));)
FQ_OP(DblChain, st_r1(w, dbl<Mul::Chain>(ld2<1>(r, 0), ld2<1>(r, 10), ld2<1>(r, 20)));)
FQ_OP(DblSigned, st_r1(w, dbl<Mul::Signed>(ld2<1>(r, 0), ld2<1>(r, 10), ld2<1>(r, 20)));)
FQ_OP(AddAffineTable, st_r1(w, add_affine_table(ld_r1(r), r + ENTRY_AT, r[MASK_AT]));)     // entry: x+y, y-x, 2dxy
FQ_OP(AddTable, st_r1(w, add_table(ld_r1(r), r + ENTRY_AT, r[MASK_AT]));)                  // entry: N, D, E, F; the unit's MUL_GROUP products
FQ_OP(PDblPoint, st_pr1(w, pdbl_point(ldp<1>(r, 0), ldp<1>(r, 10), ldp<1>(r, 20), pl));)
FQ_OP(PAddCore,
      PR3 p; p.N = ldp<2>(r, 0); p.D = ldp<2>(r, 10); p.E = ldp<1>(r, 20); p.F = ldp<1>(r, 30);
      PR2 q; q.N = ldp<2>(r, 40); q.D = ldp<2>(r, 50); q.E = ldp<2>(r, 60); q.F = ldp<1>(r, 70);
      st_pr1(w, padd_core(p, q, pl));)
FQ_OP(QDblPoint, PF<1> T; st_pr1(w, qdbl_point<(A != 0)>(ldp<1>(r, 0), ldp<1>(r, 10), ldp<1>(r, 20), pl, ql, T)); st(w, 50, T);)   // A: WITH_T
FQ_OP(PAddAffineEntry, st_pr1(w, padd_affine_entry(ld_pr1(r), ldp<1>(r, 50), ldp<1>(r, 60), ldp<1>(r, 70), r[MASK_AT], pl));)
FQ_OP(QAddAffineEntry, PF<1> T = ldp<1>(r, 80);
      st_pr1(w, qadd_affine_entry(ld_pr1(r), T, ldp<1>(r, 50), ldp<1>(r, 60), ldp<1>(r, 70), r[MASK_AT], pl, ql)); st(w, 50, T);)
#undef FQ_OP

// 64 threads per block: a budget of 512 VGPRs per lane, so the Gen entries own the registers their bodies clobber (up to v255).  Every lane
// of the grid is active (the host pads to whole waves), so the quad_perm exchanges of the pair entries always read a live partner.
template <class OP> __global__ void __launch_bounds__(64) fq_field_probe(const u32* in, u32* out) {
    const u32 lane = blockIdx.x * 64 + threadIdx.x;
    const u32 odd = threadIdx.x & 1u;
    const PairLane pl{ odd - 1u, 0u - odd };
    const QuadLane ql{ (threadIdx.x & 2) != 0 };
    OP::run(in + (size_t)lane * WORDS, out + (size_t)lane * WORDS, pl, ql);
}
}  // namespace

// The table: E(entry, A, B), the id its position.  The instantiations the library makes (tests/test_field_probe.py lists them from the
// units' IR) and the frontier of every product's static_asserts.
#define FQ_PROBE_TABLE(E) \
    E(FeMul, 1, 1) E(FeMul, 1, 2) E(FeMul, 2, 1) E(FeMul, 3, 2) E(FeMul, 4, 2) E(FeMul, 5, 4) \
    E(FeMul, 1, 7) E(FeMul, 2, 7) E(FeMul, 3, 7) E(FeMul, 4, 7) E(FeMul, 5, 7) E(FeMul, 6, 7) E(FeMul, 7, 7) E(FeMul, 8, 7) \
    E(FeSqr, 1, 0) E(FeSqr, 7, 0) \
    E(Fe2MulPlain, 1, 1) E(Fe2MulPlain, 2, 1) E(Fe2MulPlain, 2, 2) E(Fe2MulPlain, 2, 3) E(Fe2MulPlain, 3, 1) E(Fe2MulPlain, 3, 2) \
    E(Fe2MulPlain, 3, 3) E(Fe2MulPlain, 3, 6) E(Fe2MulPlain, 4, 2) E(Fe2MulPlain, 4, 6) \
    E(Fe2MulPlain, 1, 7) E(Fe2MulPlain, 2, 7) E(Fe2MulPlain, 3, 7) E(Fe2MulPlain, 4, 7) E(Fe2MulPlain, 5, 7) E(Fe2MulPlain, 6, 7) \
    E(Fe2MulPlain, 7, 6) E(Fe2MulPlain, 8, 6) \
    E(Fe2MulChain, 1, 1) E(Fe2MulChain, 1, 2) E(Fe2MulChain, 1, 5) E(Fe2MulChain, 2, 1) E(Fe2MulChain, 2, 2) E(Fe2MulChain, 2, 3) \
    E(Fe2MulChain, 2, 4) E(Fe2MulChain, 3, 1) E(Fe2MulChain, 3, 2) E(Fe2MulChain, 3, 3) E(Fe2MulChain, 3, 4) E(Fe2MulChain, 3, 6) \
    E(Fe2MulChain, 4, 2) E(Fe2MulChain, 4, 3) E(Fe2MulChain, 4, 6) E(Fe2MulChain, 5, 2) E(Fe2MulChain, 6, 2) E(Fe2MulChain, 6, 3) \
    E(Fe2MulChain, 1, 7) E(Fe2MulChain, 2, 7) E(Fe2MulChain, 3, 7) E(Fe2MulChain, 4, 7) E(Fe2MulChain, 5, 7) E(Fe2MulChain, 6, 7) \
    E(Fe2MulChain, 7, 6) E(Fe2MulChain, 8, 6) \
    E(Fe2MulSigned, 1, 1) E(Fe2MulSigned, 2, 1) E(Fe2MulSigned, 2, 2) E(Fe2MulSigned, 2, 3) E(Fe2MulSigned, 3, 2) E(Fe2MulSigned, 3, 3) \
    E(Fe2MulSigned, 4, 2) E(Fe2MulSigned, 4, 3) \
    E(Fe2MulSigned, 1, 3) E(Fe2MulSigned, 5, 3) E(Fe2MulSigned, 6, 3) E(Fe2MulSigned, 7, 3) E(Fe2MulSigned, 8, 3) \
    E(Fe2MulGen, 1, 1) E(Fe2MulGen, 1, 2) E(Fe2MulGen, 1, 3) E(Fe2MulGen, 1, 5) E(Fe2MulGen, 2, 1) E(Fe2MulGen, 2, 2) E(Fe2MulGen, 2, 3) \
    E(Fe2MulGen, 2, 4) E(Fe2MulGen, 3, 1) E(Fe2MulGen, 3, 2) E(Fe2MulGen, 3, 3) E(Fe2MulGen, 3, 4) E(Fe2MulGen, 4, 2) E(Fe2MulGen, 4, 3) \
    E(Fe2MulGen, 5, 2) E(Fe2MulGen, 6, 2) E(Fe2MulGen, 6, 3) \
    E(Fe2MulGen, 1, 7) E(Fe2MulGen, 2, 7) E(Fe2MulGen, 3, 7) E(Fe2MulGen, 4, 7) E(Fe2MulGen, 5, 7) E(Fe2MulGen, 6, 7) E(Fe2MulGen, 7, 6) \
    E(Fe2MulGen, 8, 6) \
    E(Fe2SqrPlain, 1, 0) E(Fe2SqrPlain, 2, 0) E(Fe2SqrPlain, 3, 0) E(Fe2SqrChain, 1, 0) E(Fe2SqrChain, 2, 0) E(Fe2SqrChain, 3, 0) \
    E(Fe2SqrSigned, 1, 0) E(Fe2SqrSigned, 2, 0) E(Fe2SqrSigned, 3, 0) E(Fe2SqrGen, 1, 0) E(Fe2SqrGen, 2, 0) E(Fe2SqrGen, 3, 0) \
    E(PMul, 1, 1) E(PMul, 1, 2) E(PMul, 2, 1) E(PMul, 2, 2) E(PMul, 2, 3) E(PMul, 3, 1) E(PMul, 3, 2) E(PMul, 3, 3) E(PMul, 4, 2) E(PMul, 4, 3) \
    E(PMul, 5, 3) E(PMul, 6, 3) E(PMul, 7, 3) E(PMul, 8, 3) E(PMul, 3, 4) E(PMul, 3, 5) E(PMul, 3, 6) E(PMul, 3, 7) E(PMul, 3, 8) \
    E(PMulConst, 1, 0) E(PSqr, 1, 0) E(PSqr, 2, 0) E(PSqr, 3, 0) \
    E(FeAdd, 1, 1) E(FeAdd, 1, 2) E(FeAdd, 2, 1) E(FeAdd, 2, 2) E(FeAdd, 2, 3) \
    E(FeSub, 1, 1) E(FeSub, 1, 2) E(FeSub, 2, 1) E(FeSub, 2, 2) E(FeSub, 2, 3) E(FeSub, 3, 1) \
    E(FeNeg, 1, 0) E(FeNeg, 2, 0) E(FeNeg, 3, 0) E(FeNeg, 4, 0) E(FeNeg, 5, 0) E(FeNeg, 6, 0) E(FeNeg, 7, 0) E(FeNeg, 8, 0) \
    E(FeCneg, 1, 0) E(Fe2Conj, 1, 0) E(Fe2Conj, 2, 0) \
    E(FeCarry, 1, 0) E(FeCarry, 2, 0) E(FeCarry, 3, 0) E(FeCarry, 4, 0) E(FeCarry, 5, 0) E(FeCarry, 7, 0) E(FeCarry, 9, 0) E(FeCarry, 63, 0) \
    E(FeSubSigned, 1, 1) E(FeSubSigned, 1, 2) E(FeSubSigned, 2, 1) E(FeSubSigned, 2, 2) \
    E(FeNegSigned, 1, 0) E(FeNegSigned, 2, 0) E(FeNegSigned, 3, 0) E(FeNegSigned, 4, 0) E(FeCnegSigned, 1, 0) \
    E(FeUnsign, 1, 0) E(FeUnsign, 2, 0) E(FeUnsign, 3, 0) E(FeUnsign, 4, 0) E(FeUnsignWide, 1, 0) E(FeUnsignWide, 2, 0) E(FeUnsignWide, 4, 0) \
    E(PAdd, 1, 1) E(PAdd, 1, 2) E(PAdd, 2, 1) E(PAdd, 2, 2) E(PSub, 1, 1) E(PSub, 1, 2) E(PSub, 2, 1) E(PSub, 2, 2) \
    E(PCneg, 1, 0) E(PCneg, 2, 0) E(PCneg, 3, 0) E(PCneg, 4, 0) E(PConj, 1, 0) E(PTighten, 2, 0) E(PTighten, 4, 0) \
    E(FeCanon, 1, 0) E(FeCanon, 2, 0) E(FeCanon, 3, 0) E(FeCanon, 4, 0) E(FeCanon, 5, 0) E(FeCanon, 9, 0) E(FeCanon, 63, 0) \
    E(FeIsZero, 1, 0) E(FeEqual, 1, 1) E(FeEqual, 3, 2) E(Fe2Equal, 3, 2) E(PairCanon, 1, 0) E(PairCanon, 2, 0) E(PairCanon, 3, 0) \
    E(DblPlain, 0, 0) E(DblChain, 0, 0) E(DblSigned, 0, 0) E(AddAffineTable, 0, 0) E(AddTable, 0, 0) \
    E(PDblPoint, 0, 0) E(PAddCore, 0, 0) E(QDblPoint, 0, 0) E(QDblPoint, 1, 0) E(PAddAffineEntry, 0, 0) E(QAddAffineEntry, 0, 0)

namespace {
typedef void (*ProbeKernel)(const u32*, u32*);
#define FQ_PROBE_KERNEL(F, A, B) fq_field_probe<F<A, B>>,
const ProbeKernel PROBE_KERNELS[] = { FQ_PROBE_TABLE(FQ_PROBE_KERNEL) };
#undef FQ_PROBE_KERNEL
constexpr int PROBE_COUNT = (int)(sizeof(PROBE_KERNELS) / sizeof(PROBE_KERNELS[0]));
}  // namespace

extern "C" __attribute__((visibility("default"))) int fq_field_probe_count() { return PROBE_COUNT; }

// host side: copy n lane records in, run entry `id` on them, copy n records out.  The grid is padded to whole waves of zeroed records (a
// valid input of every entry).  0 on success, otherwise the first failing hipError_t.
extern "C" __attribute__((visibility("default"))) int fq_field_probe_run(int id, const uint32_t* host_in, uint32_t* host_out, uint32_t n) {
    if (n == 0) return 0;
    if (id < 0 || id >= PROBE_COUNT || !host_in || !host_out) return (int)hipErrorInvalidValue;
    const uint32_t padded = (n + 63u) / 64u * 64u;
    const size_t bytes = (size_t)n * WORDS * sizeof(uint32_t), padded_bytes = (size_t)padded * WORDS * sizeof(uint32_t);
    u32 *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&din, padded_bytes);
    if (e == hipSuccess) e = hipMalloc(&dout, padded_bytes);
    if (e == hipSuccess) e = hipMemset(din, 0, padded_bytes);
    if (e == hipSuccess) e = hipMemset(dout, 0, padded_bytes);
    if (e == hipSuccess) e = hipMemcpy(din, host_in, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(PROBE_KERNELS[id], dim3(padded / 64u), dim3(64), 0, 0, din, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host_out, dout, bytes, hipMemcpyDeviceToHost);
    const hipError_t f1 = din ? hipFree(din) : hipSuccess;
    const hipError_t f2 = dout ? hipFree(dout) : hipSuccess;
    if (e == hipSuccess) e = f1 != hipSuccess ? f1 : f2;
    return (int)e;
}

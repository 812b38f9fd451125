// Shared device code of libfourq_amd.so: ladder arguments, table construction, the ladders and the kernels
// built from them.  Included by four translation units; the first two differ only in FQ_CHAIN (fp127.hip.h), the last
// two are their builds with constant-time table selection (ladder_kernel<..., CT = true>):
//   fourq_amd.hip       FQ_CHAIN=0  fused variable-base kernels (table + ladder in one launch), primitives, C ABI
//   fourq_chain.hip     FQ_CHAIN=1  fixed-base (LDS) ladders, comb, batched normalisation
//   fourq_ct_fused.hip  FQ_CHAIN=0  fused kernels, the lane's table scanned in registers
//   fourq_ct_chain.hip  FQ_CHAIN=1  fixed-base (LDS) ladders and comb, the whole table read at every step; the mixed-batch tail
// Measured on MI355X (2^20 elements): chaining each column's carry into the next column's first multiply-add
// gains 4-10 % for every kernel of the second group and costs the fused kernels 12-15 % when applied wholesale;
// the fused kernels therefore use it only in their ladders, with preloaded table entries (see "the ladders").
// Designs that were measured and rejected are kept as patches under tools/experiments/, not as switches in this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/fourq_amd.h"
#include "curve.hip.h"
#include "lower.hip.h"
#include "ladder_asm.hip.h"
#include "recode.hip.h"
#include "pair.hip.h"
#include "bucket_layout.h"
#include "commit_layout.h"

namespace fq {

constexpr int BLOCK = 256;
constexpr int SLOT_U32 = LimbSlots::SLOT;   // a whole-entry scratch slot (table_build_kernel, comb_table_kernel): 8 x 48 dwords + two parked points
// (The fused kernels keep N, D in dense NDSlots -- 2^16 slots = 42 MB, inside the Infinity Cache -- and E, F in LDS, below.)
constexpr int PROJ_PLANES = 8;            // deferred normalisation: the 30 working limbs of (X, Y, Z) in eight uint4 planes
constexpr int LDS_ENTRY_U32 = 52;      // 48 + 4 pad: entry k starts at bank 52k mod 64 -> eight entries never share a b128 bank group

// A second copy of the E and F coordinates of the lane's eight entries in LDS (fused kernels, one wave per SIMD: 8 entries x
// 2 coordinates x 40 bytes x 256 lanes = exactly the CU's 160 KiB).  A ladder step then gathers only N and D from the lane's
// HBM slot -- bytes 0..95 of a 192-byte entry: two 64-byte sectors instead of three -- and reads E and F from LDS, with no
// extra arithmetic.  Layout [entry][coordinate][limb pair][lane] x 8 bytes: a wave's 64 lanes hit 64 distinct bank pairs
// whatever their digits are.  The constant-time fused kernels use the same layout (ScanSplit, curve.hip.h).
constexpr int EF_LDS_U32 = 8 * 2 * 5 * 2 * 256;               // dwords: 163 840 bytes
struct LdsEF {
    static constexpr bool ON = true;
    uint2* lane;                                               // the block's array + threadIdx.x
    FQ_DEV void put1(int k, int c, const Fe2<1>& v) const {
        uint2* q = lane + (size_t)((k * 2 + c) * 5) * 256;
        q[0] = make_uint2(v.re.l[0], v.re.l[1]); q[256] = make_uint2(v.re.l[2], v.re.l[3]); q[512] = make_uint2(v.re.l[4], v.im.l[0]);
        q[768] = make_uint2(v.im.l[1], v.im.l[2]); q[1024] = make_uint2(v.im.l[3], v.im.l[4]);
    }
    FQ_DEV void put(int k, const R2& t) const { put1(k, 0, t.E); put1(k, 1, t.F); }
    // The ten rows of an entry whose E, F are not there yet are free storage: table_endo parks its working values in them
    // (build_table_endo_lds_asm) instead of making round trips through the HBM slot.
    FQ_DEV void park_nd(int k, const Fe2<1>& n, const Fe2<1>& d) const { put1(k, 0, n); put1(k, 1, d); }
    FQ_DEV void unpark_nd(int k, Fe2<1>& n, Fe2<1>& d) const { n = get((u32)k, 0); d = get((u32)k, 1); }
    FQ_DEV void park_xyz(int k, const Fe2<1>& x, const Fe2<1>& y, const Fe2<1>& z) const { put1(k, 0, x); put1(k, 1, y); put1(k + 1, 0, z); }
    FQ_DEV void unpark_xyz(int k, Fe2<1>& x, Fe2<1>& y, Fe2<1>& z) const { x = get((u32)k, 0); y = get((u32)k, 1); z = get((u32)k + 1, 0); }
    FQ_DEV Fe2<1> get(u32 k, int c) const {
        const uint2* q = lane + (size_t)((k * 2 + c) * 5) * 256;
        const uint2 a = q[0], b = q[256], d = q[512], e = q[768], f = q[1024];
        Fe2<1> r;
        r.re.l[0] = a.x; r.re.l[1] = a.y; r.re.l[2] = b.x; r.re.l[3] = b.y; r.re.l[4] = d.x;
        r.im.l[0] = d.y; r.im.l[1] = e.x; r.im.l[2] = e.y; r.im.l[3] = f.x; r.im.l[4] = f.y;
        return r;
    }
};
struct NoEF {
    static constexpr bool ON = false;
    FQ_DEV void put(int, const R2&) const {}
    FQ_DEV Fe2<1> get(u32, int) const { return Fe2<1>{}; }
};

// entry k of a lane's table: with an LdsEF only N and D go to (come from) the HBM slot, E and F live in LDS alone
template <typename L, typename EF> FQ_DEV void store_entry(u32* slot, int k, const R2& t, const EF& ef) {
    if constexpr (EF::ON) {
        store_nd<L>(slot + k * L::ENTRY, t.N, t.D);
        ef.put(k, t);
    } else {
        store_r2<L>(slot + k * L::ENTRY, t);
    }
}

enum Algo { ENDO = 0, WINDOWED = 1 };
// where the ladder finds its table:
//   FUSED     built by the same lane into its scratch slot just before the ladder (variable base: one launch)
//   LDS       one shared table staged into LDS (fixed base)
enum Src { FUSED = 0, LDS = 1 };

struct LadderArgs {
    const u64* scalars;    // n x 4
    const u64* points;     // variable base: n x 20 (R1) ; DH: n x 8 (affine) ; else unused
    u64* out;              // n x 20 (R1) or n x 8 (affine, DH)
    uint8_t* status;       // DH only
    const uint8_t* flags;  // mixed batches on the two- and four-lane kernels: flags[i] != 0 = variable base (points[i]), 0 = the fixed-base table
    const u32* index;      // optional: element ids to process (the variable-base ids of a mixed batch); NULL = identity
    u32 base;              // first position of this launch (chunked large batches)
    const u32* base_dev;   // optional: added to `base`, read on the device (the overflow part of a list whose split is decided on the device)
    const u32* n_dev;      // optional: element count read on the device (mixed batches: no host round trip)
    const void* pad_n_dev; // unused padding, as pad_table below: the kernels' code was scheduled, and measured, with the fields behind these two at
                           // their present kernel-argument offsets; without the slots hipcc schedules mixed_queue_kernel and the LDS ladders differently
    const u32* table;      // fixed base: 8 x 48 working limbs (global), staged to LDS
    const void* pad_table; // unused padding
    u32* scratch;          // variable base: NDSlots::SLOT dwords per resident lane (prep_kernel: LimbSlots::SLOT per overflow id)
    uint4* proj;           // DH, optional: PROJ_PLANES x proj_stride; non-NULL selects the kernels that leave (X, Y, Z)
                           // there for normalize_kernel
    u32 proj_stride;       // elements per plane
    u32 n;
    u32 io;                // fused MUL_* kernels (one lane per element) only -- LADDER_IO_AFFINE_IN: `points` is n x 8 affine words and the lane lifts
                           // it itself (curve4q.py:100-101); LADDER_IO_XYZ_OUT: `out` is n x 12 words, (X, Y, Z) of the result only (what
                           // R1toAffine reads, curve4q.py:103-106).  Wave-uniform branches in front of and behind the ladder: the affine / encoded
                           // I/O flavours of MUL_* need no lift kernel and no 160-byte R1 rows on either side (round 6)
};
constexpr u32 LADDER_IO_AFFINE_IN = 1, LADDER_IO_XYZ_OUT = 2;

// ---- small helpers -----------------------------------------------------------------------------
FQ_DEV void store_xyz(u32* dst, const Fe2<1>& X, const Fe2<1>& Y, const Fe2<1>& Z) {
    const Fe2<1>* f[3] = { &X, &Y, &Z };
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int i = 0; i < 5; i++) { dst[10 * k + i] = f[k]->re.l[i]; dst[10 * k + 5 + i] = f[k]->im.l[i]; }
    }
}
FQ_DEV void load_xyz(const u32* src, Fe2<1>& X, Fe2<1>& Y, Fe2<1>& Z) {
    Fe2<1>* f[3] = { &X, &Y, &Z };
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int i = 0; i < 5; i++) { f[k]->re.l[i] = src[10 * k + i]; f[k]->im.l[i] = src[10 * k + 5 + i]; }
    }
}

// (X, Y, Z) of element `id` for normalize_kernel: plane p holds limbs 4p .. 4p+3 of the 30-limb record
// X.re X.im Y.re Y.im Z.re Z.im, so that consecutive elements are consecutive uint4s in every plane (coalesced
// for the ladder's stores and for the normaliser's loads alike); Z occupies planes 5..7.
FQ_DEV void store_proj(uint4* proj, u32 stride, u32 id, const Fe2<1>& X, const Fe2<1>& Y, const Fe2<1>& Z) {
    u32 w[32];
    store_xyz(w, X, Y, Z);
    w[30] = w[31] = 0;
#pragma unroll
    for (int p = 0; p < PROJ_PLANES; p++) proj[(size_t)p * stride + id] = make_uint4(w[4 * p], w[4 * p + 1], w[4 * p + 2], w[4 * p + 3]);
}
FQ_DEV Fe2<1> load_proj_z(const uint4* proj, u32 stride, u32 id) {
    uint4 a = proj[(size_t)5 * stride + id], b = proj[(size_t)6 * stride + id], c = proj[(size_t)7 * stride + id];
    Fe2<1> z;
    z.re.l[0] = a.x; z.re.l[1] = a.y; z.re.l[2] = a.z; z.re.l[3] = a.w; z.re.l[4] = b.x;
    z.im.l[0] = b.y; z.im.l[1] = b.z; z.im.l[2] = b.w; z.im.l[3] = c.x; z.im.l[4] = c.y;
    return z;
}
FQ_DEV void load_proj_xy(const uint4* proj, u32 stride, u32 id, Fe2<1>& X, Fe2<1>& Y) {
    u32 w[20];
#pragma unroll
    for (int p = 0; p < 5; p++) {
        uint4 v = proj[(size_t)p * stride + id];
        w[4 * p] = v.x; w[4 * p + 1] = v.y; w[4 * p + 2] = v.z; w[4 * p + 3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 5; i++) { X.re.l[i] = w[i]; X.im.l[i] = w[5 + i]; Y.re.l[i] = w[10 + i]; Y.im.l[i] = w[15 + i]; }
}

// T[0] = R1toR2(P); T[i] = R1toR2(ADD(DBL(P), T[i-1]))                       curve4q.py:179-185
template <typename L = LimbSlots, typename EF = NoEF> FQ_DEV void build_table_windowed(const R1& P, u32* tbl, const EF& ef = EF()) {
    R3 twoP = r1_to_r3(dbl(P));
    R2 t = r1_to_r2(P);
    store_entry<L>(tbl, 0, t, ef);
#pragma unroll 1
    for (int i = 1; i < 8; i++) {
        t = r1_to_r2(add_core(twoP, as_signed(t)));
        store_entry<L>(tbl, i, t, ef);
    }
}

// T[k] = P + k0*phi(P) + k1*psi(P) + k2*psi(phi(P)), built in the reference's order      curve4q.py:385-403
//   step 0: Q = phi(P) -> T[1] = Q + T[0]
//   step 1: R = psi(P) -> T[2] = R + T[0], T[3] = R + T[1]
//   step 2: S = psi(Q) -> T[4..7] = S + T[0..3]
// tau and tau_dual are shared by the three steps (one code instance each): the working points P and
// Q are parked in the lane's scratch slot so that they do not pin 60 VGPRs across the endomorphisms.
template <typename L = LimbSlots> FQ_DEV void build_table_endo(const R1& P, u32* slot) {
    constexpr int SLOT_P = L::PARK_P, SLOT_Q = L::PARK_Q;
    static_assert(SLOT_Q > SLOT_P && SLOT_Q + 30 <= L::SLOT, "this builder parks two points in the slot");
    store_r2<L>(slot, r1_to_r2(P));
    store_xyz(slot + SLOT_P, P.X, P.Y, P.Z);
#pragma unroll 1
    for (int step = 0; step < 3; step++) {
        Fe2<1> X, Y, Z;
        load_xyz(slot + (step == 2 ? SLOT_Q : SLOT_P), X, Y, Z);
        Proj<1, 2, 1> t;
        if (step == 1) {                 // tau(P), parked by step 0 in P's place (phi and psi share it, curve4q.py:318-322)
            t.X = X; t.Y = widen<2>(Y); t.Z = Z;
        } else {
            t = tau(X, Y, Z);
            if (step == 0) store_xyz(slot + SLOT_P, t.X, fe2_carry(t.Y), t.Z);
        }
        Proj<2, 2, 2> u;
        if (step == 0) {
            u = upsilon(t);
        } else {
            Proj<1, 1, 1> c = chi(t);
            u.X = widen<2>(c.X); u.Y = widen<2>(c.Y); u.Z = widen<2>(c.Z);
        }
        R1 V = tau_dual(u.X, u.Y, u.Z);
        if (step == 0) store_xyz(slot + SLOT_Q, V.X, V.Y, V.Z);
        R3 V3 = r1_to_r3(V);
        int half = 1 << step;
#pragma unroll 1
        for (int m = 0; m < half; m++) {
            R2 base = load_r2<L>(slot + m * L::ENTRY);
            store_r2<L>(slot + (half + m) * L::ENTRY, r1_to_r2(add_core(V3, as_signed(base))));
        }
    }
}

// The same table with its slot traffic reordered (prep_kernel): on gfx950 loads and stores retire through one in-order counter,
// so a load issued after a store waits for that store to drain to L2 as well (microseconds when 64 lanes scatter 16 bytes each to
// their own lines).  build_table_endo above reads back ten times right behind its own stores.  Here every read-back is issued
// BEFORE the stores of the stretch it belongs to: the base T[0] and the next step's working point ahead of this step's parking /
// result stores, the base T[m+1] ahead of the store of T[half+m]; step 0 takes P from registers.  Same values, same table.
template <typename L = LimbSlots> FQ_DEV void build_table_endo_pipelined(const R1& P, u32* slot) {
    constexpr int SLOT_P = L::PARK_P, SLOT_Q = L::PARK_Q;
    static_assert(SLOT_Q > SLOT_P && SLOT_Q + 30 <= L::SLOT, "this builder parks two points in the slot");
    store_r2<L>(slot, r1_to_r2(P));
    Fe2<1> X = P.X, Y = P.Y, Z = P.Z;
#pragma unroll 1
    for (int step = 0; step < 3; step++) {
        Proj<1, 2, 1> t;
        if (step == 1) {                 // tau(P), parked by step 0 (phi and psi share it, curve4q.py:318-322)
            t.X = X; t.Y = widen<2>(Y); t.Z = Z;
        } else {
            t = tau(X, Y, Z);
            if (step == 0) store_xyz(slot + SLOT_P, t.X, fe2_carry(t.Y), t.Z);
        }
        Proj<2, 2, 2> u;
        if (step == 0) {
            u = upsilon(t);
        } else {
            Proj<1, 1, 1> c = chi(t);
            u.X = widen<2>(c.X); u.Y = widen<2>(c.Y); u.Z = widen<2>(c.Z);
        }
        R1 V = tau_dual(u.X, u.Y, u.Z);
        R2 base = load_r2<L>(slot);                                              // T[0]: behind stores that drained an endomorphism ago
        if (step < 2) load_xyz(slot + (step == 0 ? SLOT_P : SLOT_Q), X, Y, Z);   // next step's input; step 1 reads the Q parked by step 0
        if (step == 0) store_xyz(slot + SLOT_Q, V.X, V.Y, V.Z);
        R3 V3 = r1_to_r3(V);
        const int half = 1 << step;
#pragma unroll 1
        for (int m = 0; m < half; m++) {
            R2 next = base;
            if (m + 1 < half) next = load_r2<L>(slot + (m + 1) * L::ENTRY);      // ahead of this iteration's store
            store_r2<L>(slot + (half + m) * L::ENTRY, r1_to_r2(add_core(V3, as_signed(base))));
            base = next;
        }
    }
}

// ---- the ladders -------------------------------------------------------------------------------
// Two forms exist:
//   the bodies   Every product ladder: the step as hand-scheduled asm bodies on SIGNED limbs (ladder_asm.hip.h,
//                tools/asmgen/gen_ladder_step.py; fp127.hip.h "signed flavour": 5 % fewer instructions per step, per-kernel A/Bs in DESIGN.md
//                section 9), the entry in registers, requested a doubling ahead.  The fused kernels, whose lone wave per SIMD pays for
//                every issue slot (profiles/r04_ladder_step.txt); the fixed-base ladders with the table in LDS (256 VGPRs, two waves per
//                SIMD); the constant-time ladders, where the whole-table scan (select trees, compiler code) produces the entry and the
//                bodies consume it.  Such a ladder leaves the signed flavour through r1_unsign or store_r1_signed.
//   hipcc's      ladder_endo_hipcc: dbl() + add_table() on unsigned limbs with the unit's MUL_GROUP products, the entry read inside the
//                addition.  Not a product ladder: comb_table_kernel runs it once per point of the comb when a context is created.
// (The combs are no ladders: hipcc's dbl<Mul::Signed> + add_affine_table / add_affine_scan on signed limbs, left through r1_unsign too.)
// signed limbs, every coordinate within its bound -> the same point on non-negative limbs
FQ_DEV R1 r1_unsign(const R1& Q) {
    R1 r;
    r.X = fe2_unsign(Q.X); r.Y = fe2_unsign(Q.Y); r.Z = fe2_unsign(Q.Z);
    r.Ta = widen<4>(fe2_unsign(Q.Ta)); r.Tb = widen<2>(fe2_unsign(Q.Tb));
    return r;
}
// the ladder's first value: the starting entry (start_table / start_scan) as an R1 tuple, T = X * Y
FQ_DEV R1 ladder_start(const Proj<1, 1, 1>& q4) {
    R1 Q; Q.X = q4.X; Q.Y = q4.Y; Q.Z = q4.Z; Q.Ta = widen<4>(q4.X); Q.Tb = widen<2>(q4.Y);
    return Q;
}
template <typename TP> FQ_DEV R1 ladder_endo_hipcc(const EndoDigits& e, const TP* tbl, int stride) {   // curve4q.py:436-442
    R1 Q = ladder_start(start_table(tbl + (e.top & 7) * stride, 0u));      // s[64] = 1: the entry itself
#pragma unroll 1
    for (int i = 63; i >= 0; i--) {
        const TP* entry = tbl + endo_digit(e, i) * stride;
        Q = dbl(Q.X, Q.Y, Q.Z);
        Q = add_table(Q, entry, endo_neg_mask(e, i));
    }
    return R1(Q);   // a copy: with Q itself built in the caller's result, hipcc allocates comb_table_kernel's registers another way
}
// The MUL_endo ladder on the nibble stream (recode_nibbles): the bodies, one DBLT + ADD per digit.  The glue between them is per step one
// bit-field extract, one arithmetic shift (the negation mask) and one shift of the stream (a walk over EndoDigits' digit words takes four
// 64-bit shifts and five bit operations: VERDICT r5 item 4).  `at(digit)` is the address of an entry.
// SIGNED_OUT: hand the ladder's point back on signed limbs (bound 1 each) -- for store_r1_signed, which folds the bias into the canonical
// reduction of the final store
template <typename L, typename EF, bool SIGNED_OUT, typename AT> FQ_DEV R1 ladder_endo_nibbles_by(const EndoNibbles& e, const AT& at, const EF& ef) {   // curve4q.py:436-442
    Proj<1, 1, 1> q4 = start_table<L>(at(e.top & 7), 0u);                         // s[64] = 1: the entry itself
    if constexpr (EF::ON) q4.Z = ef.get(e.top & 7, 0);
    R1 Q = ladder_start(q4);
    u32 w[8];
#pragma unroll
    for (int t = 0; t < 8; t++) w[t] = e.w[t];
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        u32 cur = w[7];
#pragma unroll
        for (int t = 7; t > 0; t--) w[t] = w[t - 1];
#pragma unroll 1
        for (int j = 0; j < 8; j++) {
            const u32 digit = (cur >> 28) & 7;                                    // top nibble, bits 0..2
            const u32 neg = (u32)((int32_t)cur >> 31);                            // its bit 3, spread: ~0 when the step subtracts
            cur <<= 4;
            EntryRegs t = load_entry<L>(at(digit), digit, ef);
            Fe2<1> T;
            dblt_asm(Q.X, Q.Y, Q.Z, T);
            add_asm(Q, T, t, neg);
        }
    }
    if constexpr (SIGNED_OUT) return Q;
    else return r1_unsign(Q);
}
// The fused kernels: the lane's entries addressed as a 32-bit dword offset on the kernel's scratch pointer (`base` is wave-uniform: the
// loads take it as their scalar base) -- two multiply-adds for the two addresses of a step instead of two multiplications and a 64-bit
// address addition.
template <typename L, typename EF, bool SIGNED_OUT = false> FQ_DEV R1 ladder_endo_nibbles(const EndoNibbles& e, const u32* base, u32 lane_off, const EF& ef) {
    static_assert(EF::ON, "the fused kernels' ladder: E, F in the lane's LDS rows");
    return ladder_endo_nibbles_by<L, EF, SIGNED_OUT>(e, [=](u32 d) { return base + (size_t)(lane_off + d * (u32)L::ENTRY); }, ef);
}
// Any table a pointer and an entry stride describe -- the shared fixed-base table in LDS (ladder_kernel<ENDO, LDS>) or in global memory
// (the fixed-base items of mixed_queue_kernel).
template <typename L, typename EF, typename TP> FQ_DEV R1 ladder_endo_nibbles_at(const EndoNibbles& e, const TP* tbl, int stride, const EF& ef = EF()) {
    return ladder_endo_nibbles_by<L, EF, false>(e, [=](u32 d) { return tbl + d * stride; }, ef);
}
// canonical words of a point the asm bodies left on SIGNED limbs (every limb of every coordinate within bound 1): bias, then fe_canon's
// own carry -- what r1_unsign + store_r1 compute, with one carry chain per field element less
template <int B> FQ_DEV void store_fe2_signed(u64* w, const Fe2<B>& a) {
    fe_canon(fe_unsign_wide(a.re), w[0], w[1]); fe_canon(fe_unsign_wide(a.im), w[2], w[3]);
}
FQ_DEV void store_r1_signed(u64* w, const R1& q) {
    store_fe2_signed(w, q.X); store_fe2_signed(w + 4, q.Y); store_fe2_signed(w + 8, q.Z); store_fe2_signed(w + 12, q.Ta); store_fe2_signed(w + 16, q.Tb);
}
// the windowed ladder on the bodies: three DBL, one DBLT + ADD per window
template <typename L = LimbSlots, typename EF = NoEF, typename TP> FQ_DEV R1 ladder_windowed(const WinScalar& w, const TP* tbl, int stride, const EF& ef = EF()) {   // curve4q.py:228-235
    u32 code = win_top_code(w);
    Proj<1, 1, 1> q4 = start_table<L>(tbl + (code & 7) * stride, (code >> 3) - 1u);
    if constexpr (EF::ON) q4.Z = ef.get(code & 7, 0);
    R1 Q = ladder_start(q4);
#pragma unroll 1
    for (int i = 61; i >= 0; i--) {
        code = win_code_from_window(win_window(w, i));
        const TP* entry = tbl + (code & 7) * stride;
        const u32 neg = (code >> 3) - 1u;
        EntryRegs t = load_entry<L>(entry, code & 7, ef);          // requested ahead of the doublings
#pragma unroll 1
        for (int k = 0; k < 3; k++) dbl_asm(Q.X, Q.Y, Q.Z);
        Fe2<1> T;
        dblt_asm(Q.X, Q.Y, Q.Z, T);
        add_asm(Q, T, t, neg);
    }
    return r1_unsign(Q);
}

// The ladders with constant-time selection (curve.hip.h, "constant-time selection"): `src` reads the whole table at
// every step.  Same digits, same DAG, same R1 tuple as the ladders above.
// the four coordinates of entry `digit` out of a scanned table, as they are stored (add_asm applies the sign: masked selects, no address)
template <typename SRC> FQ_DEV EntryRegs scan_entry(const SRC& src, u32 digit_value) {
    const typename SRC::Bits digit(digit_value);
    EntryRegs t;
    t.N = src.coord(digit, 0); t.D = src.coord(digit, 1); t.E = src.coord(digit, 2); t.F = src.coord(digit, 3);
    return t;
}
// the asm bodies: the scan's select trees hand them the entry as operands
template <typename SRC> FQ_DEV R1 ladder_endo_scan(const EndoDigits& e, const SRC& src) {
    R1 Q = ladder_start(start_scan(src, e.top & 7, 0u));
#pragma unroll 1
    for (int i = 63; i >= 0; i--) {
        Fe2<1> T;
        dblt_asm(Q.X, Q.Y, Q.Z, T);
        add_asm(Q, T, scan_entry(src, endo_digit(e, i)), endo_neg_mask(e, i));
    }
    return r1_unsign(Q);
}
template <typename SRC> FQ_DEV R1 ladder_windowed_scan(const WinScalar& w, const SRC& src) {
    u32 code = win_top_code(w);
    R1 Q = ladder_start(start_scan(src, code & 7, (code >> 3) - 1u));
#pragma unroll 1
    for (int i = 61; i >= 0; i--) {
        code = win_code_from_window(win_window(w, i));
#pragma unroll 1
        for (int k = 0; k < 3; k++) dbl_asm(Q.X, Q.Y, Q.Z);
        Fe2<1> T;
        dblt_asm(Q.X, Q.Y, Q.Z, T);
        add_asm(Q, T, scan_entry(src, code & 7), (code >> 3) - 1u);
    }
    return r1_unsign(Q);
}

// table_endo for the fused kernels that keep E, F in LDS (LdsEF): the same DAG and the same order as above, but nothing is
// ever read back from the HBM slot.  The working points and the N, D of the entries that later additions need are parked in
// the LDS rows of entries that do not exist yet (each entry owns 80 bytes per lane):
//     tau(P)      entries 6, 7   step 0 -> read at the end of step 0
//     Q = phi(P)  entries 4, 5   step 0 -> read at the end of step 1
//     N, D of T[k], k = 1, 2, 3: entry 8 - k, written when T[k] is stored, read as the base of T[2 + k] / T[4 + k] before
//                 that entry's own E, F arrive (an iteration loads its next base BEFORE it stores the previous result)
// T[0]'s N, D stay in registers.  The HBM slot receives N, D of every entry, write-only; loads and stores share vmcnt on
// gfx950, so a table phase without loads has nothing to wait for until the ladder's first gather.
// Every formula is a generated body (ladder_asm.hip.h: tau / upsilon / chi / tau_dual + R1toR3 / R1toR2 / table addition, 22 500
// instructions per table against 24 400 for hipcc's own, no register shuffles between products; cycles per body: profiles/r04_table_phases.txt);
// the entries are tight and non-negative.
template <typename L, typename EF> FQ_DEV void build_table_endo_lds_asm(const R1& P, u32* slot, const EF& ef) {
    static_assert(EF::ON, "needs the LDS copy of E and F");
    R2 result = r1_to_r2_asm(P);               // T[0]
    int result_at = 0;
    const Fe2<1> n0 = result.N, d0 = result.D;
    Fe2<1> X = P.X, Y = P.Y, Z = P.Z;          // step 0: P; step 1: tau(P); step 2: phi(P)
    auto store_result = [&]() {
        store_entry<L>(slot, result_at, result, ef);
        if (result_at >= 1 && result_at <= 3) ef.park_nd(8 - result_at, result.N, result.D);
    };
#pragma unroll 1
    for (int step = 0; step < 3; step++) {
        store_result();
        if (step != 1) {                       // phi and psi share tau(P), curve4q.py:318-322
            tau_asm(X, Y, Z);
            if (step == 0) ef.park_xyz(6, X, Y, Z);
        }
        if (step == 0) upsilon_asm(X, Y, Z); else chi_asm(X, Y, Z);
        Fe2<2> N3, D3;
        Fe2<1> F3;
        taudual_asm(X, Y, Z, N3, D3, F3);      // (X, Y, Z) = phi(P) / psi(P) / psi(phi(P)); (N3, D3, Z, F3) its R3 form
        const Fe2<1> E3 = Z;
        R2 base;
        base.N = n0; base.D = d0; base.E = ef.get(0, 0); base.F = ef.get(0, 1);
        const int half = 1 << step;
#pragma unroll 1
        for (int m = 0; m < half; m++) {
            R2 next = base;
            if (m + 1 < half) { ef.unpark_nd(8 - (m + 1), next.N, next.D); next.E = ef.get((u32)(m + 1), 0); next.F = ef.get((u32)(m + 1), 1); }
            if (m > 0) store_result();
            if (m == 0 && step == 0) ef.park_xyz(4, X, Y, Z);
            if (m == half - 1 && step < 2) ef.unpark_xyz(step == 0 ? 6 : 4, X, Y, Z);   // for the next step
            result = base;
            table_add_asm(result, N3, D3, E3, F3);
            result_at = half + m;
            base = next;
        }
    }
    store_result();                            // T[7]
}

FQ_DEV void load_scalar(const u64* p, u64 m[4]) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 a = q[0], b = q[1];
    m[0] = (u64)a.x | ((u64)a.y << 32); m[1] = (u64)a.z | ((u64)a.w << 32);
    m[2] = (u64)b.x | ((u64)b.y << 32); m[3] = (u64)b.z | ((u64)b.w << 32);
}

// the fused constant-time ladders' source: N, D of the lane's eight entries from its slot into registers, E, F where they are
template <typename L, typename EF> FQ_DEV ScanSplit<EF> scan_split(const u32* slot, const EF& ef) {
    ScanSplit<EF> regs;
    regs.ef = ef;
    regs.template load<L>(slot);
    return regs;
}

namespace {   // kernels: one private copy per translation unit (their code objects differ by FQ_CHAIN)

// ALGO: ENDO / WINDOWED.  SRC: where the table is.  DH: affine in, cofactor clearing, affine out + status.
// DEFER (DH only): leave (X, Y, Z) in a.proj for normalize_kernel instead of inverting Z here.
// CT: constant-time table selection (every entry read at every step); FUSED keeps N, D of the lane's table in registers and
// scans E, F in the lane's LDS rows, LDS scans the shared table where it lies.
constexpr int ladder_waves(int src) {                          // wave slots per SIMD a ladder kernel is built for
    if (src == FUSED) return 1;                                // the endomorphisms' 256 VGPRs and the CU's whole LDS
    return 2;                                                  // the asm bodies: 256 VGPRs
}
template <int ALGO, int SRC, bool DH, bool DEFER = false, bool CT = false>
__global__ __launch_bounds__(BLOCK, ladder_waves(SRC)) void ladder_kernel(LadderArgs a) {
    static_assert(!DEFER || DH, "only DH outputs are normalised");
    constexpr bool USE_EF = SRC == FUSED;                      // LdsEF: the CU's whole LDS for one block of a fused kernel
    __shared__ __attribute__((aligned(16))) u32 lds_table[SRC == LDS ? 8 * LDS_ENTRY_U32 : EF_LDS_U32];
    using EF = typename std::conditional<USE_EF, LdsEF, NoEF>::type;
    using L = NDSlots;                                         // the lane's slot (unused with SRC == LDS)
    EF ef;
    if constexpr (USE_EF) ef.lane = reinterpret_cast<uint2*>(lds_table) + threadIdx.x;
    if (SRC == LDS) {
        for (int i = threadIdx.x; i < 8 * R2_LIMBS; i += BLOCK)
            lds_table[(i / R2_LIMBS) * LDS_ENTRY_U32 + (i % R2_LIMBS)] = a.table[i];
        __syncthreads();
    }
    const u32 n = a.n_dev ? *a.n_dev : a.n;
    const u32 lane_slot = blockIdx.x * BLOCK + threadIdx.x;
    const u32 lanes = gridDim.x * BLOCK;
    const u32 n_round = (n + BLOCK - 1) / BLOCK * BLOCK;
#pragma unroll 1
    for (u32 it = lane_slot; it < n_round; it += lanes) {
        const bool live = it < n;
        const u32 pos = live ? it : n - 1;                // idle tail lanes redo the last element, store nothing
        const u32 id = a.index ? a.index[a.base + pos] : a.base + pos;
        u64 m[4];
        load_scalar(a.scalars + 4 * (size_t)id, m);
        u32* slot = SRC == LDS ? nullptr : a.scratch + (size_t)lane_slot * L::SLOT;

        uint8_t st = FOURQ_DH_OK;
        R1 P;
        if (DH) {
            Fe2<1> x = load_fe2(a.points + 8 * (size_t)id), y = load_fe2(a.points + 8 * (size_t)id + 4);
            if (!point_on_curve(x, y)) st = FOURQ_DH_NOT_ON_CURVE;      // keep going branch-free; masked at the end
            if (SRC == FUSED) P = clear_cofactor_392(x, y);             // with a table the reference discards [392]P (curve4q.py:209)
        } else if (SRC == FUSED) {
            if (a.io & LADDER_IO_AFFINE_IN) P = affine_to_r1(load_fe2(a.points + 8 * (size_t)id), load_fe2(a.points + 8 * (size_t)id + 4));
            else P = load_r1(a.points + 20 * (size_t)id);
        }
        if constexpr (SRC == FUSED) {
            if constexpr (ALGO == ENDO) build_table_endo_lds_asm<L>(P, slot, ef);
            else build_table_windowed<L>(P, slot, ef);
        }
        R1 Q;                                                           // every ladder below runs the asm bodies (see "the ladders")
        if constexpr (ALGO == ENDO) {
            u64 v[4];
            decompose(m, v);
            if constexpr (CT && SRC == FUSED) {
                const EndoDigits e = recode(v);
                Q = ladder_endo_scan(e, scan_split<L>(slot, ef));
            } else if constexpr (CT) {
                Q = ladder_endo_scan(recode(v), ScanMem<8, u32>{ lds_table, LDS_ENTRY_U32 });
            } else if constexpr (SRC == FUSED) {
                Q = ladder_endo_nibbles<L, EF, !DH>(recode_nibbles(v), a.scratch, lane_slot * (u32)L::SLOT, ef);      // MUL_*: signed limbs, see the store
            } else {
                Q = ladder_endo_nibbles_at<LimbSlots, NoEF>(recode_nibbles(v), lds_table, LDS_ENTRY_U32);
            }
        } else {
            const WinScalar w = win_reduce(m);
            if constexpr (CT && SRC == FUSED) {
                Q = ladder_windowed_scan(w, scan_split<L>(slot, ef));
            } else if constexpr (CT) {
                Q = ladder_windowed_scan(w, ScanMem<8, u32>{ lds_table, LDS_ENTRY_U32 });
            } else if constexpr (SRC == LDS) {
                Q = ladder_windowed(w, lds_table, LDS_ENTRY_U32);
            } else {
                Q = ladder_windowed<L, EF>(w, slot, L::ENTRY, ef);
            }
        }
        // One inversion per K elements, later (normalize_kernel).  FUSED: by a wave-uniform flag, no second instance -- DH batches of at least
        // two generations defer like the fixed-base ladders (round 6) instead of inverting per element at one wave per SIMD.
        if (DH && (DEFER || (SRC == FUSED && a.proj != nullptr))) {
            if (live) {
                store_proj(a.proj, a.proj_stride, id, Q.X, Q.Y, Q.Z);
                a.status[id] = st;
            }
        } else if (DH) {
            Fe2<1> ax, ay;
            r1_to_affine(Q, ax, ay);
            u64 o[8];
            store_fe2(o, ax); store_fe2(o + 4, ay);
            bool neutral = (o[0] | o[1] | o[2] | o[3] | o[5] | o[6] | o[7]) == 0 && o[4] == 1;   // (Ox, Oy) = ((0,0),(1,0))
            if (st == FOURQ_DH_OK && neutral) st = FOURQ_DH_NEUTRAL;
            if (live) {
                uint4* dst = reinterpret_cast<uint4*>(a.out + 8 * (size_t)id);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    u64 lo = st ? 0 : o[2 * k], hi = st ? 0 : o[2 * k + 1];
                    dst[k] = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
                }
                a.status[id] = st;
            }
        } else if (live) {
            u64 o[20];
            if constexpr (ALGO == ENDO && SRC == FUSED && !CT) store_r1_signed(o, Q);
            else store_r1(o, Q);
            const bool xyz = SRC == FUSED && (a.io & LADDER_IO_XYZ_OUT);
            u64* dst = a.out + (xyz ? 12 : 20) * (size_t)id;
#pragma unroll
            for (int k = 0; k < 10; k++)
                if (k < 6 || !xyz) put_words<2>(dst + 2 * k, o + 2 * k);
        }
    }
}

// ---- two lanes per element (pair.hip.h): the variable-base kernels for small batches and for the tail past whole generations --
// 128 elements per 256-lane block (the pair's table fills the CU's LDS), one block per CU, grid-stride over the batch.  Each lane
// loads, computes and stores ITS half (real or imaginary parts) of every coordinate; the scalar is recoded in both lanes.
// CT: constant-time table selection -- the lane scans its eight entries in LDS at every step (PairTable::scan_entry).
// FIXED: the caller's table (a.table, working limbs) instead of one built from a point: every lane copies its halves of the
// eight entries into its LDS rows once, then the same ladders run (with a table the reference ignores the point: curve4q.py:209,
// :426; DH still tests it, curve4q.py:447-448).
// LPE = 4: four lanes per element (pair.hip.h, "four lanes per element"): 64 elements per block, both pairs of an element keep the
// whole table and every value; the ladder steps share their products between the pairs; the first pair stores.
// MIXED (BASELINE config 5's batch shape, small): element i takes its table from its own point (flags[i] != 0) or from the caller's
// fixed-base table -- every lane builds a table (from zeros where the element is fixed-base: no divergence in the long part), then the
// fixed-base elements overwrite their LDS rows with the caller's entries.  Which kind an element is, is public.
template <int ALGO, bool DH, bool CT = false, bool FIXED = false, int LPE = 2, bool MIXED = false>
__global__ __launch_bounds__(BLOCK, 1) void pair_kernel(LadderArgs a) {
    static_assert(LPE == 2 || LPE == 4, "two or four lanes per element");
    static_assert(!MIXED || (ALGO == ENDO && !DH && !FIXED), "mixed batches are MUL_endo batches");
    constexpr bool QUAD = LPE == 4;
    const QuadLane ql{ QUAD && (threadIdx.x & 2) != 0 };
    const bool writer = !ql.second;
    __shared__ __attribute__((aligned(16))) u32 lds_pair[PAIR_LDS_U32];
    PairTable tbl;
    tbl.two = reinterpret_cast<uint2*>(lds_pair) + threadIdx.x;
    tbl.one = lds_pair + PAIR_VALUES * 2 * 256 * 2 + threadIdx.x;             // behind the region of limb pairs
    const u32 odd = threadIdx.x & 1;
    const PairLane pl{ odd - 1u, 0u - odd };
    constexpr u32 PER_BLOCK = BLOCK / LPE;
    constexpr int IN_WORDS = DH ? 8 : 20, OUT_WORDS = DH ? 8 : 20;
    const u32 n = a.n, n_round = (n + PER_BLOCK - 1) / PER_BLOCK * PER_BLOCK;
    if constexpr (FIXED) {                       // entry k, coordinate c: 12 dwords = re limbs 0..4 | im limbs 0..4 | 2 pad (load_fe2_limbs)
#pragma unroll 1
        for (int v = 0; v < PAIR_VALUES; v++) {
            const u32* src = a.table + (v >> 2) * R2_LIMBS + (v & 3) * COORD_U32 + 5 * odd;
            PF<1> h;
#pragma unroll
            for (int i = 0; i < 5; i++) { h.l[i] = src[i]; FQ_SIGN_UNKNOWN(h.l[i]); }
            tbl.put(v, h);
        }
    }
#pragma unroll 1
    for (u32 it = blockIdx.x * PER_BLOCK + threadIdx.x / LPE; it < n_round; it += gridDim.x * PER_BLOCK) {
        const bool live = it < n && writer;
        const u32 id = a.base + (it < n ? it : n - 1);           // idle tail pairs redo the last element, store nothing
        u64 m[4];
        load_scalar(a.scalars + 4 * (size_t)id, m);
        bool variable = true;
        if constexpr (MIXED) variable = a.flags[id] != 0;
        auto half = [&](int c) {                                  // this lane's half of coordinate c of the input point: words 4c + 2 odd, + 1
            const uint4 w = *reinterpret_cast<const uint4*>(a.points + IN_WORDS * (size_t)id + 4 * c + 2 * odd);
            const Fe<1> f = fe_unpack((u64)w.x | ((u64)w.y << 32), (u64)w.z | ((u64)w.w << 32));
            PF<1> r;
#pragma unroll
            for (int i = 0; i < 5; i++) { r.l[i] = (!MIXED || variable) ? f.l[i] : 0u; FQ_SIGN_UNKNOWN(r.l[i]); }
            return r;
        };
        auto store_half = [&](int c, u64 lo, u64 hi) {
            *reinterpret_cast<uint4*>(a.out + OUT_WORDS * (size_t)id + 4 * c + 2 * odd) = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
        };
        uint8_t st = FOURQ_DH_OK;
        PR1 P;
        if constexpr (DH) {
            const PF<1> x = half(0), y = half(1);
            if (!pair_point_on_curve(x, y, pl)) st = FOURQ_DH_NOT_ON_CURVE;      // keep going branch-free; masked at the end
            if constexpr (!FIXED) P = pair_clear_cofactor_392<QUAD>(x, y, pl, ql);
        } else if constexpr (!FIXED) {
            P.X = half(0); P.Y = half(1); P.Z = half(2); P.Ta = pwiden<3>(half(3)); P.Tb = pwiden<2>(half(4));
        }
        PR1 Q;
        if constexpr (ALGO == ENDO) {
            if constexpr (!FIXED) pair_build_table_endo<QUAD>(P, tbl, pl, ql);
            if constexpr (MIXED) {
                if (!variable) {
#pragma unroll 1
                    for (int v = 0; v < PAIR_VALUES; v++) {
                        const u32* src = a.table + (v >> 2) * R2_LIMBS + (v & 3) * COORD_U32 + 5 * odd;
                        PF<1> h;
#pragma unroll
                        for (int i = 0; i < 5; i++) { h.l[i] = src[i]; FQ_SIGN_UNKNOWN(h.l[i]); }
                        tbl.put(v, h);
                    }
                }
            }
            u64 v[4];
            decompose(m, v);
            Q = pair_ladder_endo<CT, QUAD>(recode(v), tbl, pl, ql);
        } else {
            if constexpr (!FIXED) pair_build_table_windowed<QUAD>(P, tbl, pl, ql);
            Q = pair_ladder_windowed<CT, QUAD>(win_reduce(m), tbl, pl, ql);
        }
        if constexpr (DH) {
            PF<1> ax, ay;
            pair_to_affine(Q, pl, ax, ay);
            u64 x0, x1, y0, y1;
            pair_canon(ax, x0, x1); pair_canon(ay, y0, y1);
            // (Ox, Oy) = ((0, 0), (1, 0)): this lane's half of it is (0, 1) on even lanes and (0, 0) on odd ones
            const u32 neutral = pair_both(((x0 | x1 | y1) == 0 && y0 == (u64)(pl.even & 1u)) ? 1u : 0u);
            if (st == FOURQ_DH_OK && neutral) st = FOURQ_DH_NEUTRAL;
            if (live) {
                store_half(0, st ? 0 : x0, st ? 0 : x1);
                store_half(1, st ? 0 : y0, st ? 0 : y1);
                if (!odd) a.status[id] = st;
            }
        } else if (live) {
            u64 lo, hi;
            pair_canon(Q.X, lo, hi); store_half(0, lo, hi);
            pair_canon(Q.Y, lo, hi); store_half(1, lo, hi);
            pair_canon(Q.Z, lo, hi); store_half(2, lo, hi);
            pair_canon(Q.Ta, lo, hi); store_half(3, lo, hi);
            pair_canon(Q.Tb, lo, hi); store_half(4, lo, hi);
        }
    }
}

// ---- mixed batches: ONE persistent kernel pulling work from a device-side queue (BASELINE config 5) ----------------
// partition_kernel has compacted the ids of the round's variable-base and fixed-base elements (counts[0], counts[1]).  A work
// item is 64 consecutive positions of the two lists laid end to end, variable-base first: items wholly inside the first list are
// variable-base (fused table_endo + ladder, as ladder_kernel<ENDO, FUSED>), items wholly inside the second fixed-base (the shared
// table, gathered through L1 a doubling ahead), and the ONE item that straddles the boundary runs as a variable-base item whose
// fixed-base lanes copy the shared table into their own slot and LDS rows instead of building one -- so 65 550 + 65 522 elements
// are 2 048 items, two per resident wave, not 1 025 + 1 024 with a third item (a whole ladder) for one wave (round 3's version:
// profiles/r03_mixed_queue.txt).  One block per CU owns the CU's LDS (E, F of the lanes' tables) and a scratch slot per lane; each
// of its four waves loops on its own: take the next item with one atomic, run it, until the queue is empty.  Except in the
// boundary item no wave diverges, and the long items are handed out first.  CT: constant-time table selection for both kinds
// (the kind of an element is public, its digits are not).  Every wave leaves the loop: the queue head only grows and `total` is
// fixed before the launch.
template <bool CT>
__global__ __launch_bounds__(BLOCK, 1) void mixed_queue_kernel(LadderArgs a, const u32* var_list, const u32* fix_list, const u32* counts, u32* queue_head) {
    __shared__ __attribute__((aligned(16))) u32 lds_ef[EF_LDS_U32];
    LdsEF ef;
    ef.lane = reinterpret_cast<uint2*>(lds_ef) + threadIdx.x;
    const u32 n_var = counts[0], n_all = n_var + counts[1];
    const u32 total = (n_all + 63) / 64;
    u32* slot = a.scratch + (size_t)(blockIdx.x * BLOCK + threadIdx.x) * NDSlots::SLOT;
    const u32 lane = threadIdx.x & 63;
#pragma unroll 1
    for (;;) {
        u32 item = 0;
        if (lane == 0) item = atomicAdd(queue_head, 1u);
        item = __builtin_amdgcn_readfirstlane(item);
        if (item >= total) break;
        const u32 first = item * 64;
        const bool all_fixed = first >= n_var;                      // wave-uniform
        const bool live = first + lane < n_all;
        const u32 pos = live ? first + lane : n_all - 1;            // idle tail lanes redo the last element, store nothing
        const bool variable = pos < n_var;                          // per lane: differs inside the wave in the boundary item only
        const u32 id = variable ? var_list[pos] : fix_list[pos - n_var];
        u64 m[4];
        load_scalar(a.scalars + 4 * (size_t)id, m);
        R1 Q;
        if (!all_fixed) {
            if (variable) {
                const R1 P = load_r1(a.points + 20 * (size_t)id);
                build_table_endo_lds_asm<NDSlots>(P, slot, ef);
            } else {                                                // a fixed-base lane of the boundary item: the shared table as its own
#pragma unroll 1
                for (int k = 0; k < 8; k++) store_entry<NDSlots>(slot, k, load_r2_limbs(a.table + k * R2_LIMBS), ef);
            }
            u64 v[4];
            decompose(m, v);
            if constexpr (CT) {
                const EndoDigits e = recode(v);
                Q = ladder_endo_scan(e, scan_split<NDSlots>(slot, ef));
            } else {                                                // the headline kernel's ladder (nibble stream, 32-bit entry offsets)
                Q = ladder_endo_nibbles<NDSlots, LdsEF>(recode_nibbles(v), a.scratch, (blockIdx.x * BLOCK + threadIdx.x) * (u32)NDSlots::SLOT, ef);
            }
        } else {
            u64 v[4];
            decompose(m, v);
            if constexpr (CT) Q = ladder_endo_scan(recode(v), ScanMem<8, u32>{ a.table, R2_LIMBS });      // wave-uniform addresses
            else Q = ladder_endo_nibbles_at<LimbSlots, NoEF>(recode_nibbles(v), a.table, R2_LIMBS);
        }
        if (live) {
            u64 o[20];
            store_r1(o, Q);
            put_words<20>(a.out + 20 * (size_t)id, o);
        }
    }
}

// Mixed batches in CONSTANT-TIME mode, rounds larger than one generation.  The variable-base ids run through the fused constant-
// time kernel (table in registers + LDS, one wave per SIMD), whose generations hold exactly `lanes` elements: config 5's 65 550
// ids would cost a second generation of the whole chip for 14 elements.  split_counts_kernel therefore cuts a small remainder
// (at most `limit` ids) off the list on the device; prep_kernel builds those ids' tables into scratch, and
// this kernel -- 128 registers, 1.6 KB of LDS, up to four waves per SIMD -- runs them TOGETHER with the round's fixed-base
// elements: a wave whose 64 elements are all fixed-base scans the shared table in LDS (as ladder_kernel<ENDO, LDS, CT>), any other
// wave scans each lane's own table through a per-lane pointer in global memory (every entry read at every step: no address depends
// on a digit).  Which kind an element is, is public.
template <int UNIT_ONLY = 0>        // a template so that only the translation unit that launches it carries a copy
__global__ void split_counts_kernel(u32* counts, u32 lanes, u32 limit) {         // counts: [n_var, n_fix, -, -, fused, over]
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const u32 n_var = counts[0], rem = n_var % lanes, whole = n_var - rem;
    const bool cut = whole > 0 && rem > 0 && rem <= limit;
    counts[4] = cut ? whole : n_var;
    counts[5] = cut ? rem : 0u;
}
// The overflow ids' tables for mixed_ct_tail_kernel: per id, table_endo into scratch slot `pos` as whole entries of working limbs
// (what ScanMem reads).  A kernel of its own so that the endomorphisms' register appetite does not set the tail's occupancy.
template <int UNIT_ONLY = 0>
__global__ __launch_bounds__(BLOCK) void prep_kernel(LadderArgs a) {
    const u32 pos = blockIdx.x * BLOCK + threadIdx.x;
    if (pos >= (a.n_dev ? *a.n_dev : a.n)) return;
    const u32 first = a.base + (a.base_dev ? *a.base_dev : 0u);
    const u32 id = a.index ? a.index[first + pos] : first + pos;
    const R1 P = load_r1(a.points + 20 * (size_t)id);
    build_table_endo_pipelined<LimbSlots>(P, a.scratch + (size_t)pos * LimbSlots::SLOT);
}
template <int UNIT_ONLY = 0>
__global__ __launch_bounds__(BLOCK, 2) void mixed_ct_tail_kernel(LadderArgs a, const u32* fix_list, const u32* var_list, const u32* counts, const u32* over_scratch) {
    __shared__ __attribute__((aligned(16))) u32 lds_table[8 * LDS_ENTRY_U32];
    for (int i = threadIdx.x; i < 8 * R2_LIMBS; i += BLOCK)
        lds_table[(i / R2_LIMBS) * LDS_ENTRY_U32 + (i % R2_LIMBS)] = a.table[i];
    __syncthreads();
    const u32 n_fix = counts[1], fused = counts[4], total = n_fix + counts[5];
    const u32 lanes = gridDim.x * BLOCK, n_round = (total + BLOCK - 1) / BLOCK * BLOCK;
#pragma unroll 1
    for (u32 it = blockIdx.x * BLOCK + threadIdx.x; it < n_round; it += lanes) {
        const bool live = it < total;
        const u32 pos = live ? it : total - 1;                // idle tail lanes redo the last element, store nothing
        const bool fixed = pos < n_fix;
        const u32 id = fixed ? fix_list[pos] : var_list[fused + (pos - n_fix)];
        u64 m[4], v[4];
        load_scalar(a.scalars + 4 * (size_t)id, m);
        decompose(m, v);
        const EndoDigits e = recode(v);
        R1 Q;
        if (__all(fixed)) {                                   // wave-uniform, and public
            Q = ladder_endo_scan(e, ScanMem<8, u32>{ lds_table, LDS_ENTRY_U32 });
        } else {
            const u32* tbl = fixed ? a.table : over_scratch + (size_t)(pos - n_fix) * LimbSlots::SLOT;
            Q = ladder_endo_scan(e, ScanMem<8, u32>{ tbl, LimbSlots::ENTRY });
        }
        if (live) {
            u64 o[20];
            store_r1(o, Q);
            put_words<20>(a.out + 20 * (size_t)id, o);
        }
    }
}

// ---- fixed-base comb -------------------------------------------------------------
constexpr int COMB_POINTS = COMB_POINTS_ALL;                  // 1 024 (by address) + 80 (constant-time mode)
static_assert(COMB_POINTS == FOURQ_COMB_POINTS, "include/fourq_amd.h and recode.hip.h disagree on the comb's shape");
constexpr int COMB_ENTRY_U32 = 3 * COORD_U32;                 // (x+y, y-x, 2dxy)
constexpr int COMB_LDS_U32 = COMB_ENTRY_U32;                  // stride in LDS (pads of 0, 4, 8, 12 dwords measured alike)
constexpr int COMB_BLOCK_MAX = 1024;                          // the fast shape's table is 144 KB of LDS: ONE block per CU, up to 16 waves wide
constexpr size_t COMB_FAST_LDS_BYTES = (size_t)CombFast::POINTS * COMB_LDS_U32 * sizeof(u32);
static_assert(COMB_FAST_LDS_BYTES <= 160 * 1024, "the fast comb table must fit the CU's LDS");

// ---- key generation for small batches: the comb (recode.hip.h, CombFast: 6 doublings + 27 mixed additions) four lanes per element ----
// comb_kernel stages the 144 KB table into LDS once per block -- nothing when a block works through thousands of elements, a third of
// the 0.11 ms of a batch of one.  Here every lane gathers ITS HALF of an entry (15 dwords) from the table where it lies (L2), one
// column ahead of its use, and the element's two pairs share the products of the doubling and of the mixed addition (pair.hip.h):
// 64 elements per block, no LDS in the default mode.
// CT: the constant-time shape (80 points, 16-entry blocks; recode.hip.h, CombScan), its 11.5 KB staged into LDS; an addition reads its WHOLE
// block -- every lane the same addresses but for its half -- and keeps one entry by the select tree (curve.hip.h): no address depends on the scalar.
template <bool CT, int P, typename TREE, typename BITS> FQ_DEV void comb_scan_pairs(const u32* blk, u32 odd, const BITS& bits, TREE& tree, u32 out[15]) {
    u32 v0[15], v1[15];
#pragma unroll
    for (int cidx = 0; cidx < 3; cidx++) {
#pragma unroll
        for (int i = 0; i < 5; i++) {
            v0[5 * cidx + i] = blk[(2 * P) * COMB_ENTRY_U32 + cidx * COORD_U32 + 5 * odd + i];
            v1[5 * cidx + i] = blk[(2 * P + 1) * COMB_ENTRY_U32 + cidx * COORD_U32 + 5 * odd + i];
        }
    }
    tree.template feed<P>(bits, v0, v1, out);
    __builtin_amdgcn_sched_barrier(0);                         // two entries per round, as ScanMem
    if constexpr (2 * P + 2 < CombScan::BLOCK_POINTS) comb_scan_pairs<CT, P + 1>(blk, odd, bits, tree, out);
}
// LPE = 2: two lanes per element (batches between a quarter and half a generation): the same walk on the pair code, T = Ta*Tb inside the addition.
template <bool CT = false, int LPE = 4>
__global__ __launch_bounds__(BLOCK) void comb_quad_kernel(const u64* scalars, const u32* comb_limbs, u64* out, uint8_t* status, u32 n) {
    static_assert(LPE == 2 || LPE == 4, "two or four lanes per element");
    using S = typename std::conditional<CT, CombScan, CombFast>::type;
    __shared__ __attribute__((aligned(16))) u32 lds_scan[CT ? CombScan::POINTS * COMB_ENTRY_U32 : 4];
    if constexpr (CT) {
        const u32* sub = comb_limbs + CombFast::POINTS * COMB_ENTRY_U32;
        for (u32 i = threadIdx.x; i < (u32)(CombScan::POINTS * COMB_ENTRY_U32 / 4); i += BLOCK)
            reinterpret_cast<uint4*>(lds_scan)[i] = reinterpret_cast<const uint4*>(sub)[i];
        __syncthreads();
    }
    const u32 odd = threadIdx.x & 1;
    const PairLane pl{ odd - 1u, 0u - odd };
    const QuadLane ql{ LPE == 4 && (threadIdx.x & 2) != 0 };
    const u32 it = blockIdx.x * (BLOCK / LPE) + threadIdx.x / LPE;
    const bool live = it < n && !ql.second;
    const u32 id = it < n ? it : n - 1;                       // idle tail quads redo the last element, store nothing
    u64 m[4];
    load_scalar(scalars + 4 * (size_t)id, m);
    const CombDigits<S> c = comb_recode<S>(m);
    auto column = [&](int t) { return S::E * (t % S::V) + (S::E - 1 - t / S::V); };          // the t-th column in processing order
    auto entry = [&](int t, PF<1>& hN, PF<1>& hD, PF<1>& hF) {  // this lane's halves of the three coordinates of the entry of the t-th column
        const int col = column(t);
        u32 w[15];
        if constexpr (CT) {
            const DigitBits<S::W - 1> bits(comb_index(c, col));
            SelectTree<15, S::W - 1> tree;
            comb_scan_pairs<CT, 0>(lds_scan + (((u32)(t % S::V)) << (S::W - 1)) * COMB_ENTRY_U32, odd, bits, tree, w);
        } else {
            const u32* e = comb_limbs + (size_t)((((u32)(t % S::V)) << (S::W - 1)) + comb_index(c, col)) * COMB_ENTRY_U32 + 5 * odd;
#pragma unroll
            for (int cidx = 0; cidx < 3; cidx++) {
#pragma unroll
                for (int i = 0; i < 5; i++) w[5 * cidx + i] = e[cidx * COORD_U32 + i];
            }
        }
#pragma unroll
        for (int i = 0; i < 5; i++) {
            hN.l[i] = w[i]; hD.l[i] = w[5 + i]; hF.l[i] = w[10 + i];
            FQ_SIGN_UNKNOWN(hN.l[i]); FQ_SIGN_UNKNOWN(hD.l[i]); FQ_SIGN_UNKNOWN(hF.l[i]);
        }
    };
    PF<1> aN, aD, aF;
    entry(0, aN, aD, aF);
    PR1 Q;
    PF<1> T;
    {                                                           // +-A as a point with Z = 2: (N - D, N + D, 2), T = X*Y/Z
        const u32 neg = comb_neg_mask(c, column(0));
        PF<1> N, D;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            N.l[k] = __builtin_amdgcn_bitop3_b32(neg, aD.l[k], aN.l[k], 0xCA);
            D.l[k] = __builtin_amdgcn_bitop3_b32(neg, aN.l[k], aD.l[k], 0xCA);
        }
        Q.X = ptighten(psub(N, D)); Q.Y = ptighten(padd(N, D));
        Q.Z.l[0] = pl.even & 2u; Q.Z.l[1] = Q.Z.l[2] = Q.Z.l[3] = Q.Z.l[4] = 0;
        const PF<1> y_half = pmul_const(Q.Y, fe2_half_const(), pl);
        Q.Ta = pwiden<3>(Q.X); Q.Tb = pwiden<2>(y_half);        // Ta*Tb = X*Y/Z
        T = pmul(Q.X, y_half, pl);
    }
#pragma unroll 1
    for (int t = 1; t < S::V * S::E; t++) {
        entry(t, aN, aD, aF);
        if constexpr (LPE == 4) {
            if (t % S::V == 0) Q = qdbl_point<true>(Q.X, Q.Y, Q.Z, pl, ql, T);
            Q = qadd_affine_entry(Q, T, aN, aD, aF, comb_neg_mask(c, column(t)), pl, ql);
        } else {
            if (t % S::V == 0) Q = pdbl_point(Q.X, Q.Y, Q.Z, pl);
            Q = padd_affine_entry(Q, aN, aD, aF, comb_neg_mask(c, column(t)), pl);
        }
    }
    PF<1> ax, ay;
    pair_to_affine(Q, pl, ax, ay);
    ax = pcneg(ax, c.negate);                                   // even scalar: [k]B = -[N - k]B, -(x, y) = (-x, y)
    u64 x0, x1, y0, y1;
    pair_canon(ax, x0, x1); pair_canon(ay, y0, y1);
    const u32 neutral = pair_both(((x0 | x1 | y1) == 0 && y0 == (u64)(pl.even & 1u)) ? 1u : 0u);
    if (live) {
        auto store_half = [&](int k, u64 lo, u64 hi) {
            *reinterpret_cast<uint4*>(out + 8 * (size_t)id + 4 * k + 2 * odd) = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
        };
        store_half(0, neutral ? 0 : x0, neutral ? 0 : x1);
        store_half(1, neutral ? 0 : y0, neutral ? 0 : y1);
        if (!odd) status[id] = neutral ? FOURQ_DH_NEUTRAL : FOURQ_DH_OK;
    }
}

#if FQ_CHAIN   // only fourq_chain.hip launches it
// [m]B, affine, from the comb: 6 doublings + 27 mixed additions per element (constant-time mode: 9 + 49 on the small shape).
// The block width is the launcher's choice (blockDim.x, a multiple of 64): the table is staged once per block.
// The doublings and mixed additions are hipcc's, on signed limbs (dbl<Mul::Signed>, add_affine_table / add_affine_scan).
template <bool DEFER, bool CT = false>
__global__ __launch_bounds__(CT ? BLOCK : COMB_BLOCK_MAX, CT ? 4 : 1) void comb_kernel(const u64* scalars, const u32* comb_limbs, u64* out, uint8_t* status, uint4* proj, u32 proj_stride, u32 n) {
    using S = typename std::conditional<CT, CombScan, CombFast>::type;       // the constant-time mode scans the small sub-table
    extern __shared__ __attribute__((aligned(16))) u32 lds[];                // S::POINTS * COMB_LDS_U32 dwords, sized by the launcher
    const u32* sub = comb_limbs + (CT ? CombFast::POINTS * COMB_ENTRY_U32 : 0);
    const u32 width = blockDim.x;
    static_assert(COMB_LDS_U32 == COMB_ENTRY_U32, "a comb is staged as it lies");
    for (u32 i = threadIdx.x; i < (u32)(S::POINTS * COMB_ENTRY_U32 / 4); i += width)
        reinterpret_cast<uint4*>(lds)[i] = reinterpret_cast<const uint4*>(sub)[i];
    __syncthreads();
    const u32 lanes = gridDim.x * width;
    const u32 n_round = (n + width - 1) / width * width;
#pragma unroll 1
    for (u32 it = blockIdx.x * width + threadIdx.x; it < n_round; it += lanes) {
        const bool live = it < n;
        const u32 id = live ? it : n - 1;
        u64 m[4];
        load_scalar(scalars + 4 * (size_t)id, m);
        CombDigits<S> c = comb_recode<S>(m);
        R1 Q;
#pragma unroll 1
        for (int i = S::E - 1; i >= 0; i--) {
#pragma unroll 1
            for (int j = 0; j < S::V; j++) {
                const int col = S::E * j + i;
                const u32 neg = comb_neg_mask(c, col);
                if constexpr (CT) {                      // all entries of block j are read; the index only forms masks
                    const ScanMem<S::BLOCK_POINTS, u32> block{ lds + (j << (S::W - 1)) * COMB_LDS_U32, COMB_LDS_U32 };
                    if (i == S::E - 1 && j == 0) { Q = affine_scan_start(block, comb_index(c, col), neg); continue; }
                    if (j == 0) Q = dbl<Mul::Signed>(Q.X, Q.Y, Q.Z);
                    Q = add_affine_scan(Q, block, comb_index(c, col), neg);
                } else {
                    const u32* entry = lds + ((j << (S::W - 1)) + comb_index(c, col)) * COMB_LDS_U32;
                    if (i == S::E - 1 && j == 0) { Q = affine_table_start(entry, neg); continue; }
                    if (j == 0) Q = dbl<Mul::Signed>(Q.X, Q.Y, Q.Z);
                    Q = add_affine_table(Q, entry, neg);
                }
            }
        }
        Q = r1_unsign(Q);
        if (DEFER) {                                          // deferred normalisation, see normalize_kernel
            if (live) {
                store_proj(proj, proj_stride, id, fe2_carry(fe2_cneg(Q.X, c.negate)), Q.Y, Q.Z);   // even scalar: -(x, y) = (-x, y)
                status[id] = FOURQ_DH_OK;
            }
            continue;
        }
        Fe2<1> ax, ay;
        r1_to_affine(Q, ax, ay);
        ax = fe2_carry(fe2_cneg(ax, c.negate));               // even scalar: [k]B = -[N - k]B, -(x, y) = (-x, y)
        u64 o[8];
        store_fe2(o, ax); store_fe2(o + 4, ay);
        const bool neutral = (o[0] | o[1] | o[2] | o[3] | o[5] | o[6] | o[7]) == 0 && o[4] == 1;
        if (live) {
            uint4* dst = reinterpret_cast<uint4*>(out + 8 * (size_t)id);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                u64 lo = neutral ? 0 : o[2 * k], hi = neutral ? 0 : o[2 * k + 1];
                dst[k] = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
            }
            status[id] = neutral ? FOURQ_DH_NEUTRAL : FOURQ_DH_OK;
        }
    }
}

// R1toAffine for a whole DH batch with one GF(p) inversion per K elements (lower.hip.h).  Source: the planes of store_proj.
// Masked: elements already rejected (status != 0), at every K -- a point of the curve has Z != 0, so a product is zero only for those.
// The chain is inlined (fe_inv_inline): around a call the lane's live values spill.  The affine result is canonical, hence identical to
// the per-element inversion.
template <int K>
__global__ __launch_bounds__(BLOCK) void normalize_kernel(const uint4* proj, u32 stride, u64* out, uint8_t* status, u32 n) {
    LaneSlots<K> s(n);
    if (!s.lane(blockIdx.x * BLOCK + threadIdx.x)) return;
    Fe2<1> z[K];
    uint8_t st[K];
#pragma clang loop unroll(full)
    for (int j = 0; j < K; j++) {                     // all loads first: the lane's K elements are K separate cache lines
        const u32 at = s.at(j);
        z[j] = load_proj_z(proj, stride, at);
        st[j] = s.live(j) ? status[at] : (uint8_t)FOURQ_DH_NOT_ON_CURVE;
    }
    SharedInverse<K, FeOps<true>> si;
#pragma clang loop unroll(full)
    for (int j = 0; j < K; j++) si.take(j, z_norm(z[j]), st[j] == FOURQ_DH_OK);
    si.invert();
#pragma clang loop unroll(full)
    for (int j = K - 1; j >= 0; j--) {
        Fe2<1> X, Y;
        load_proj_xy(proj, stride, s.at(j), X, Y);
        const Fe2<1> zi = z_inverse(z[j], si.peel(j));
        u64 o[8];
        store_fe2(o, fe2_mul(X, zi));
        store_fe2(o + 4, fe2_mul(Y, zi));
        uint8_t st_j = st[j];
        if (st_j == FOURQ_DH_OK && (o[0] | o[1] | o[2] | o[3] | o[5] | o[6] | o[7]) == 0 && o[4] == 1) st_j = FOURQ_DH_NEUTRAL;   // curve4q.py:459-460
        if (s.live(j)) {
            uint4* dst = reinterpret_cast<uint4*>(out + 8 * (size_t)s.id(j));
#pragma clang loop unroll(full)
            for (int k = 0; k < 4; k++) {
                u64 lo = st_j ? 0 : o[2 * k], hi = st_j ? 0 : o[2 * k + 1];
                dst[k] = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
            }
            status[s.id(j)] = st_j;
        }
    }
}

#endif

}  // namespace

// launchers implemented in fourq_chain.hip (FQ_CHAIN=1 code objects)
int chain_launch_ladder(int algo, bool dh, unsigned grid, hipStream_t stream, const LadderArgs& a);   // the fixed-base (LDS) ladders; defers when a.proj != NULL
int chain_setup_device();       // per-device function attributes (the comb's dynamic LDS); called by fourq_ctx_create
int chain_launch_comb(unsigned grid, hipStream_t stream, const u64* scalars, const u32* comb_limbs, u64* out, uint8_t* status, uint4* proj, u32 proj_stride, u32 n);
int chain_launch_normalize(int k, hipStream_t stream, const uint4* proj, u32 proj_stride, u64* out, uint8_t* status, u32 n);   // k in {1, 2, 4, 8}
// combine.hip.h: [k]B + [l]P from the comb's planes and the ladder's rows; k in {1, 2}; out_kind: canonical affine words, 32-byte encoding + status,
// or one byte "the encoding equals expect" + status
enum CombineOut { COMBINE_AFFINE = 0, COMBINE_ENCODE = 1, COMBINE_VERIFY = 2 };
int chain_launch_combine(int k, int out_kind, hipStream_t stream, const uint4* proj, u32 proj_stride, const u64* rows, u32 row_stride, const uint8_t* st_decode,
                         const u64* expect, u64* out, uint8_t* status, uint8_t* ok, u32 n);
// msm.hip.h: one fold pass of a grouped sum.  Rows of `stride` words, m_in per group, become canonical 12-word rows, ceil(m_in / MSM_FOLD) per group;
// st_in (NULL: none) / st_out: one raw decode code per row, folded as a maximum
constexpr u32 MSM_FOLD = 64;
int chain_launch_msm_fold(hipStream_t stream, const u64* rows, u32 stride, const uint8_t* st_in, u64* rows_out, uint8_t* st_out, size_t groups, size_t m_in);
// ... and one planned pass of a RAGGED sum (msm_shape.h): output row t sums the rows desc[t] = { first, count } names; `teams` output rows, teams
// of `team` lanes (a power of two, at most 16) that each sum `iters` rows before the butterfly
int chain_launch_msm_fold_desc(hipStream_t stream, const u64* rows, u32 stride, const uint8_t* st_in, u64* rows_out, uint8_t* st_out, const uint2* desc, size_t teams,
                               u32 team, u32 iters);
// bucket.hip.h: the grouped sums by the bucket method, from the sub-scalars to one projective row (and decode code) per group in w.sum / w.st_sum
int chain_launch_bucket_sum(hipStream_t stream, const fq_work::Bucket& w, const u64* scalars, const u64* points_affine, const uint8_t* st_decode);
// commit.hip.h: the combs of a commitment, row g * group_size + j from comb j of `combs` as a canonical 12-word (X, Y, Z) row; route 1 = staged, 2 = gather
// (commit_layout.h has the geometry); ct_launch_commit: the constant-time build, blocks_max = resident 256-lane blocks
int chain_launch_commit(int route, unsigned cus, hipStream_t stream, const u64* scalars, const u32* combs, u64* rows, size_t groups, size_t group_size);
int ct_launch_commit(unsigned blocks_max, hipStream_t stream, const u64* scalars, const u32* combs, u64* rows, size_t groups, size_t group_size);
// keyset.hip.h: signatures of registered keys.  order: status[i] from decode's raw code to the slot's status; comb: [k]B + [l]A_id as canonical 12-word rows
// from the generator's comb and comb id of `combs` (pre, or NULL: the row's inherited status); lower: the rows' encodings, or with `verify` ok = (encoding ==
// expect); gather + fix: the constant-time route's key bytes by index, and the set's statuses on the existing routes' results
int chain_launch_keyset_order(hipStream_t stream, const u64* affine, uint8_t* status, u32 m);
int chain_launch_keyset_comb(hipStream_t stream, const u64* k, const u64* l, const u32* key_ids, const u32* comb_g, const u32* combs, const uint8_t* key_status, u32 count,
                             u64* rows, uint8_t* pre, u32 n);
int chain_launch_keyset_lower(hipStream_t stream, bool verify, const u64* rows, const uint8_t* pre, const u64* expect, u64* out, uint8_t* ok, uint8_t* status, u32 n);
int chain_launch_keyset_gather(hipStream_t stream, const u32* key_ids, const uint8_t* key_bytes, u32 count, uint8_t* pk32, u32 n);
int chain_launch_keyset_fix(hipStream_t stream, const u32* key_ids, const uint8_t* key_status, u32 count, u64* out, uint8_t* ok, uint8_t* status, u32 n);
// constant-time selection builds of the same kernels: fourq_ct_fused.hip (FQ_CHAIN=0) and fourq_ct_chain.hip (FQ_CHAIN=1)
int ct_launch_fused(int algo, bool dh, unsigned grid, hipStream_t stream, const LadderArgs& a);
int ct_launch_pair(int algo, bool dh, bool fixed, bool quad, unsigned grid, hipStream_t stream, const LadderArgs& a);
int ct_launch_pair_mixed(bool quad, unsigned grid, hipStream_t stream, const LadderArgs& a);
int ct_launch_comb_quad(bool quad, unsigned grid, hipStream_t stream, const u64* scalars, const u32* comb_limbs, u64* out, uint8_t* status, u32 n);
int ct_launch_mixed_tail(unsigned prep_grid, unsigned tail_grid, hipStream_t stream, const LadderArgs& a, const u32* fix_list, const u32* var_list, u32* counts,
                         u32* over_scratch);     // split_counts_kernel must already have run: see fourq_ct_chain.hip
int ct_launch_split_counts(hipStream_t stream, u32* counts, u32 lanes, u32 limit);
int ct_launch_mixed_queue(unsigned grid, hipStream_t stream, const LadderArgs& a, const u32* var_list, const u32* fix_list, const u32* counts, u32* queue_head);
int ct_launch_lds(int algo, bool dh, unsigned grid, hipStream_t stream, const LadderArgs& a);        // defers when a.proj != NULL
int ct_launch_comb(unsigned grid, hipStream_t stream, const u64* scalars, const u32* comb_limbs, u64* out, uint8_t* status, uint4* proj, u32 proj_stride, u32 n);

}  // namespace fq

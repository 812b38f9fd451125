// hipcc's own ladder addition with the entry's coordinates in registers: the step the product ran before the generated bodies
// (add_asm, ladder_asm.hip.h) replaced it.  Kept here as variant A of ladder_step.hip and pairlane.hip; include after curve.hip.h.
#pragma once
namespace fq {
template <int CH> FQ_DEV R1 add_entry(const R1& q, const EntryRegs& t, u32 neg_mask) {
    // The masked exchange of N and D must not be scheduled next to the gathers (hipcc does that when it may, and the lone
    // wave then sits out the gather latency at the top of every step: measured -7 % on the headline kernel).  The mask is
    // made to depend on the doubled point, so the twenty selects can only issue once the doubling has been computed.
    asm("" : "+v"(neg_mask) : "v"(q.X.re.l[0]), "v"(q.Y.re.l[0]), "v"(q.Z.re.l[0]));
    const Fe2<1> tN = fe2_bitselect(neg_mask, t.D, t.N), tD = fe2_bitselect(neg_mask, t.N, t.D);
    Fe2<1> T = fe2_mulx<CH>(q.Ta, q.Tb);
    Fe2<2> N1 = fe2_add(q.X, q.Y);
    Fe2<3> D1 = fe2_subx<CH>(q.Y, q.X);
    Fe2<1> A = fe2_mulx<CH>(D1, tD);
    Fe2<1> B = fe2_mulx<CH>(N1, tN);
    Fe2<1> C = fe2_mulx<CH>(fe2_cnegx<CH>(t.F, neg_mask), T);
    Fe2<1> D = fe2_mulx<CH>(t.E, q.Z);
    Fe2<3> E = fe2_subx<CH>(B, A);
    Fe2<3> F = fe2_subx<CH>(D, C);
    Fe2<2> G = fe2_add(D, C);
    Fe2<2> H = fe2_add(B, A);
    R1 r;
    r.X = fe2_mulx<CH>(E, F);
    r.Z = fe2_mulx<CH>(G, F);
    r.Y = fe2_mulx<CH>(G, H);
    r.Ta = widen<4>(E);
    r.Tb = H;
    return r;
}
}  // namespace fq

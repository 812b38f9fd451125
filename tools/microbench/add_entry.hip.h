// hipcc's own ladder addition on signed limbs with the entry's coordinates in registers: the step the product ran before the
// generated bodies (add_asm, ladder_asm.hip.h) replaced it.  Kept here as variant A of ladder_step.hip and pairlane.hip, beside
// dbl<Mul::Signed>; include after curve.hip.h.
#pragma once
namespace fq {
FQ_DEV R1 add_entry(const R1& q, const EntryRegs& t, u32 neg_mask) {
    // The masked exchange of N and D must not be scheduled next to the gathers (hipcc does that when it may, and the lone
    // wave then sits out the gather latency at the top of every step: measured -7 % on the headline kernel).  The mask is
    // made to depend on the doubled point, so the twenty selects can only issue once the doubling has been computed.
    asm("" : "+v"(neg_mask) : "v"(q.X.re.l[0]), "v"(q.Y.re.l[0]), "v"(q.Z.re.l[0]));
    const Fe2<1> tN = fe2_bitselect(neg_mask, t.D, t.N), tD = fe2_bitselect(neg_mask, t.N, t.D);
    Fe2<1> T = fe2_mul_signed(q.Ta, q.Tb);
    Fe2<2> N1 = fe2_add(q.X, q.Y);
    Fe2<2> D1 = fe2_sub_signed(q.Y, q.X);
    Fe2<1> A = fe2_mul_signed(D1, tD);
    Fe2<1> B = fe2_mul_signed(N1, tN);
    Fe2<1> C = fe2_mul_signed(fe2_cneg_signed(t.F, neg_mask), T);
    Fe2<1> D = fe2_mul_signed(t.E, q.Z);
    Fe2<2> E = fe2_sub_signed(B, A);
    Fe2<2> F = fe2_sub_signed(D, C);
    Fe2<2> G = fe2_add(D, C);
    Fe2<2> H = fe2_add(B, A);
    R1 r;
    r.X = fe2_mul_signed(E, F);
    r.Z = fe2_mul_signed(G, F);
    r.Y = fe2_mul_signed(G, H);
    r.Ta = widen<4>(E);
    r.Tb = H;
    return r;
}
}  // namespace fq

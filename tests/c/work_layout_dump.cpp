// prints every work-buffer layout for n elements: ./work_layout_dump n  ->  lines "layout region offset" and "layout bytes total", then the
// list of all layouts as the header has it: "list Struct total" per member and "list max_bytes value"; then "extent layout value", the bytes
// from the buffer's start that the layout admits for its inner calls, and "lent layout value", the tail of its total that its caller carves
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "work_layout.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layouts only compute addresses
static void region(const char* layout, const char* name, const void* p) { printf("%s %s %zu\n", layout, name, (size_t)(static_cast<const char*>(p) - BASE)); }
#define REGION(layout, w, member) region(layout, #member, w.member)
template <class L> static void listed(size_t n) {          // g++ spells the type out: "... [with L = fq_work::DhBytes; ...]"
    const char* at = strstr(__PRETTY_FUNCTION__, "fq_work::") + 9;
    printf("list %.*s %zu\n", (int)strcspn(at, ";]"), at, L::bytes(n));
}
template <class... L> static void list_all(fq_work::Layouts<L...>, size_t n) { (listed<L>(n), ...); printf("list max_bytes %zu\n", fq_work::Layouts<L...>::max_bytes(n)); }
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const size_t n = strtoull(argv[1], 0, 10);
    using namespace fq_work;
    { const DhBytes w(BASE, n); REGION("dh_bytes", w, pts); REGION("dh_bytes", w, shared); REGION("dh_bytes", w, st_decode); REGION("dh_bytes", w, st_dh); }
    { const Exchange w(BASE, n); REGION("exchange", w, base_pts); REGION("exchange", w, mid); REGION("exchange", w, st_first); }
    { const MulRows w(BASE, n); REGION("mul_rows", w, rows_in); REGION("mul_rows", w, rows_out); REGION("mul_rows", w, unused); REGION("mul_rows", w, st_decode); }
    { const DoubleMul w(BASE, n); REGION("double_mul", w, rows_in); REGION("double_mul", w, rows_out); REGION("double_mul", w, st_decode); REGION("double_mul", w, st_comb); REGION("double_mul", w, tail); }
    { const SigVerify w(BASE, n); REGION("sig_verify", w, rows_in); REGION("sig_verify", w, rows_out); REGION("sig_verify", w, st_decode); REGION("sig_verify", w, st_comb);
      REGION("sig_verify", w, sig.s); REGION("sig_verify", w, sig.h); REGION("sig_verify", w, sig.r32); REGION("sig_verify", w, sig.pre); }
    { const Sig w(BASE, n); REGION("sig", w, a); REGION("sig", w, r); REGION("sig", w, r32); REGION("sig", w, affine); REGION("sig", w, st_comb); }
    { const H2c w(BASE, n); REGION("h2c", w, u); }
    printf("dh_bytes bytes %zu\nexchange bytes %zu\nmul_rows bytes %zu\ndouble_mul bytes %zu\nsig_verify bytes %zu\nsig bytes %zu\nh2c bytes %zu\n",
           DhBytes::bytes(n), Exchange::bytes(n), MulRows::bytes(n), DoubleMul::bytes(n), SigVerify::bytes(n), Sig::bytes(n), H2c::bytes(n));
    list_all(All(), n);
    printf("extent dh_bytes %zu\nextent exchange %zu\nextent mul_rows %zu\nextent double_mul %zu\nextent sig_verify %zu\nextent sig %zu\nextent h2c %zu\n",
           DhBytes::inner_extent(n), Exchange::inner_extent(n), MulRows::inner_extent(n), DoubleMul::inner_extent(n), SigVerify::inner_extent(n), Sig::inner_extent(n), H2c::inner_extent(n));
    printf("lent dh_bytes %zu\nlent exchange %zu\nlent mul_rows %zu\nlent double_mul %zu\nlent sig_verify %zu\nlent sig %zu\nlent h2c %zu\n",
           DhBytes::lent(n), Exchange::lent(n), MulRows::lent(n), DoubleMul::lent(n), SigVerify::lent(n), Sig::lent(n), H2c::lent(n));
    return 0;
}

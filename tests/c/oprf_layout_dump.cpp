// prints the work-buffer layouts of the four oblivious-PRF calls for n elements: ./oprf_layout_dump n  ->  lines "layout.region offset",
// "layout.bytes total", "sig_verify_bytes total" (the layout that has sized fourq_ctx_reserve so far) and "layout_inner_extent value" (the
// bytes from the buffer's start that the layout admits for its inner calls)
#include <cstdio>
#include <cstdlib>
#include "work_layout.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layouts only compute addresses
static void region(const char* layout, const char* name, const void* p) { printf("%s.%s %zu\n", layout, name, (size_t)(static_cast<const char*>(p) - BASE)); }
#define REGION(layout, w, member) region(layout, #member, w.member)
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const size_t n = strtoull(argv[1], 0, 10);
    using namespace fq_work;
    const OprfBlind b(BASE, n);
    REGION("blind", b, pts); REGION("blind", b, rows_in); REGION("blind", b, u); REGION("blind", b, rows_out); REGION("blind", b, st_decode);
    const OprfEvaluate e(BASE, n);
    REGION("evaluate", e, dh); REGION("evaluate", e, keys);
    const OprfFinalize f(BASE, n);
    REGION("finalize", f, inv); REGION("finalize", f, rows_in); REGION("finalize", f, rows_out); REGION("finalize", f, e32);
    REGION("finalize", f, st_decode); REGION("finalize", f, st_lower); REGION("finalize", f, st_zero);
    const OprfEval d(BASE, n);
    REGION("eval", d, pts); REGION("eval", d, shared); REGION("eval", d, u); REGION("eval", d, keys); REGION("eval", d, e32); REGION("eval", d, st_dh);
    printf("blind.bytes %zu\nevaluate.bytes %zu\nfinalize.bytes %zu\neval.bytes %zu\n", OprfBlind::bytes(n), OprfEvaluate::bytes(n), OprfFinalize::bytes(n), OprfEval::bytes(n));
    printf("dh_bytes_bytes %zu\nsig_verify_bytes %zu\n", DhBytes::bytes(n), SigVerify::bytes(n));
    printf("blind_inner_extent %zu\nevaluate_inner_extent %zu\nfinalize_inner_extent %zu\neval_inner_extent %zu\n", OprfBlind::inner_extent(n), OprfEvaluate::inner_extent(n),
           OprfFinalize::inner_extent(n), OprfEval::inner_extent(n));
    return 0;
}

// prints the work-buffer layout of the grouped sums for n elements: ./msm_layout_dump n  ->  lines "region offset", "bytes total" and
// "sig_verify_bytes total" (the layout that has sized fourq_ctx_reserve so far)
#include <cstdio>
#include <cstdlib>
#include "work_layout.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layout only computes addresses
static void region(const char* name, const void* p) { printf("%s %zu\n", name, (size_t)(static_cast<const char*>(p) - BASE)); }
#define REGION(w, member) region(#member, w.member)
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const size_t n = strtoull(argv[1], 0, 10);
    using namespace fq_work;
    const Msm w(BASE, n);
    REGION(w, rows_in); REGION(w, rows_out); REGION(w, st_decode); REGION(w, part_a); REGION(w, st_a); REGION(w, part_b); REGION(w, st_b);
    printf("bytes %zu\nsig_verify_bytes %zu\n", Msm::bytes(n), SigVerify::bytes(n));
    return 0;
}

// prints the work-buffer layout of the DLEQ proof calls for n rows in `groups` groups: ./dleq_layout_dump n groups  ->  lines
// "own.region offset", "inner.layout total" (what each inner call's own layout takes at the size it is called with), "inner_bytes total",
// "inner_extent value" (the bytes from the buffer's start that the layout admits for its inner calls) and "bytes total"
#include <cstdio>
#include <cstdlib>
#include "dleq_layout.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layout only computes addresses
static void region(const char* name, const void* p) { printf("own.%s %zu\n", name, (size_t)(static_cast<const char*>(p) - BASE)); }
#define REGION(w, member) region(#member, w.member)
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const size_t n = strtoull(argv[1], 0, 10), groups = strtoull(argv[2], 0, 10);
    using namespace fq_work;
    const Dleq w(BASE, n, groups);
    REGION(w, inner); REGION(w, d); REGION(w, pk); REGION(w, m32); REGION(w, z32); REGION(w, t2); REGION(w, t3); REGION(w, sc_a); REGION(w, sc_b);
    REGION(w, pair_sc); REGION(w, pair_pt); REGION(w, affine); REGION(w, st_m); REGION(w, st_z); REGION(w, st_t2); REGION(w, st_t3); REGION(w, st_pre);
    printf("inner.msm_rows %zu\ninner.msm_pair %zu\ninner.double_mul %zu\ninner.evaluate %zu\ninner.mul_rows %zu\ninner.sig %zu\n", Msm::bytes(n), Msm::bytes(2 * groups),
           DoubleMul::bytes(groups), OprfEvaluate::bytes(groups), MulRows::bytes(groups), Sig::bytes(groups + 1));
    printf("inner_bytes %zu\nbytes %zu\nplane_rows %zu\n", DleqInner::bytes(n, groups), Dleq::bytes(n, groups), Dleq::plane_rows(groups));
    printf("inner_extent %zu\n", Dleq::inner_extent(n, groups));
    return 0;
}

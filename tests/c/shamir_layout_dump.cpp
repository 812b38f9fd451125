// prints the work-buffer layout of the threshold-sharing calls for `rows` output rows and threshold t: ./shamir_layout_dump rows t  ->  lines
// "own.region offset", "inner.layout total" (what each inner call's own layout takes at the size it is called with), "inner_bytes total",
// "inner_extent value" (the bytes from the buffer's start that the layout admits for its inner calls), "plane_rows value" and "bytes total"
#include <cstdio>
#include <cstdlib>
#include "shamir_layout.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layout only computes addresses
static void region(const char* name, const void* p) { printf("own.%s %zu\n", name, (size_t)(static_cast<const char*>(p) - BASE)); }
#define REGION(w, member) region(#member, w.member)
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const size_t rows = strtoull(argv[1], 0, 10), t = strtoull(argv[2], 0, 10);
    using namespace fq_work;
    const Shamir w(BASE, rows, t);
    REGION(w, inner); REGION(w, sc); REGION(w, pt); REGION(w, lambda); REGION(w, pub32); REGION(w, g32); REGION(w, affine);
    REGION(w, flags); REGION(w, st_set); REGION(w, st_pub); REGION(w, st_comb);
    printf("inner.msm_rows %zu\ninner.comb_encode %zu\n", Msm::bytes(rows * t), Sig::bytes(rows));
    printf("inner_bytes %zu\nbytes %zu\nplanes %d\nplane_rows %zu\n", ShamirInner::bytes(rows, t), Shamir::bytes(rows, t), Shamir::planes ? 1 : 0, Shamir::plane_rows(rows, t));
    printf("inner_extent %zu\n", Shamir::inner_extent(rows, t));
    return 0;
}

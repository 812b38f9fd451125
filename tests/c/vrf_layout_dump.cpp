// prints the work-buffer layout of the VRF calls for n rows: ./vrf_layout_dump n  ->  lines "own.region offset", "inner.layout total" (what
// each inner call's own layout takes at the size it is called with), "inner_bytes total", "inner_extent value" (the bytes from the buffer's start that the layout admits for its inner calls) and "bytes total"
#include <cstdio>
#include <cstdlib>
#include "vrf_layout.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layout only computes addresses
static void region(const char* name, const void* p) { printf("own.%s %zu\n", name, (size_t)(static_cast<const char*>(p) - BASE)); }
#define REGION(w, member) region(#member, w.member)
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const size_t n = strtoull(argv[1], 0, 10);
    using namespace fq_work;
    const Vrf w(BASE, n);
    REGION(w, inner); REGION(w, u); REGION(w, affine); REGION(w, pk32); REGION(w, h32); REGION(w, g32); REGION(w, u32); REGION(w, v32); REGION(w, sc_a); REGION(w, sc_b);
    REGION(w, pair_sc); REGION(w, pair_pt); REGION(w, st_a); REGION(w, st_b); REGION(w, st_u); REGION(w, st_v); REGION(w, st_pre);
    printf("inner.mul_rows %zu\ninner.double_mul %zu\ninner.keyset %zu\ninner.msm_pair %zu\n", MulRows::bytes(n), DoubleMul::bytes(n), Keyset::bytes(n), Msm::bytes(2 * n));
    printf("inner_bytes %zu\nbytes %zu\nplanes %d\n", VrfInner::bytes(n), Vrf::bytes(n), Vrf::planes ? 1 : 0);
    printf("inner_extent %zu\n", Vrf::inner_extent(n));
    return 0;
}

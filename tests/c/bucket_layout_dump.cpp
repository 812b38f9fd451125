// prints the geometry and the work-buffer layout of the bucket route of the grouped sums: ./bucket_layout_dump groups group_size window  ->
// lines "geom.name value", "rows.k value" (rows per column before pass k + 1), "own.region offset", "inner_bytes total", "zeroed_bytes total"
// and "bytes total"
#include <cstdio>
#include <cstdlib>
#include "bucket_layout.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layout only computes addresses
static void region(const char* name, const void* p) { printf("own.%s %zu\n", name, (size_t)(static_cast<const char*>(p) - BASE)); }
#define REGION(w, member) region(#member, w.member)
int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const size_t groups = strtoull(argv[1], 0, 10), group_size = strtoull(argv[2], 0, 10);
    const unsigned window = (unsigned)strtoul(argv[3], 0, 10);
    using namespace fq_work;
    if (!BucketGeom::window_ok(window)) return 3;
    const Bucket w(BASE, groups, group_size, window);
    printf("geom.n %zu\ngeom.windows %u\ngeom.digits %zu\ngeom.cols %zu\ngeom.passes %u\ngeom.chunks %zu\ngeom.fold1 %zu\n", w.g.n, w.g.windows, w.g.digits, w.g.cols, w.g.passes,
           w.g.chunks, w.g.fold1);
    for (unsigned k = 0; k <= BucketGeom::MAX_PASSES; k++) printf("rows.%u %zu\n", k, w.g.rows[k]);
    REGION(w, inner); REGION(w, v); REGION(w, affine); REGION(w, st_decode); REGION(w, group_code); REGION(w, counts); REGION(w, off_a); REGION(w, off_b);
    REGION(w, idx); REGION(w, rows_a); REGION(w, rows_b); REGION(w, weighted); REGION(w, fold_a); REGION(w, fold_b); REGION(w, endo); REGION(w, st_endo);
    REGION(w, sum); REGION(w, st_sum);
    printf("inner_bytes %zu\nzeroed_bytes %zu\nbytes %zu\n", Msm::bytes(w.g.n), w.zeroed_bytes(), Bucket::bytes(groups, group_size, window));
    return 0;
}

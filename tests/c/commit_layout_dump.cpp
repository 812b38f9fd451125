// prints the launch geometry and the work-buffer layout of the fixed-generator commitments: ./commit_layout_dump groups group_size blocks_max
// width_max  ->  lines "geom.name value", "geom.changes value" (blocks whose item range holds more than one base), "own.region offset" and
// "bytes total"
#include <cstdio>
#include <cstdlib>
#include "commit_layout.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layout only computes addresses
static void region(const char* name, const void* p) { printf("own.%s %zu\n", name, (size_t)(static_cast<const char*>(p) - BASE)); }
#define REGION(w, member) region(#member, w.member)
int main(int argc, char** argv) {
    if (argc != 5) return 2;
    const size_t groups = strtoull(argv[1], 0, 10), group_size = strtoull(argv[2], 0, 10);
    const unsigned blocks_max = (unsigned)strtoul(argv[3], 0, 10), width_max = (unsigned)strtoul(argv[4], 0, 10);
    using namespace fq_work;
    const CommitGeom g(groups, group_size, blocks_max, width_max);
    size_t changes = 0, covered = 0;
    for (unsigned b = 0; b < g.grid; b++) {
        const size_t first = g.first_item(b), last = g.first_item(b + 1);
        if (first != covered) return 3;                                      // the ranges tile the items in order
        covered = last;
        if (last > first && (last - 1) / g.slices != first / g.slices) changes++;
    }
    if (covered != g.items) return 3;
    printf("geom.width %u\ngeom.grid %u\ngeom.slices %zu\ngeom.items %zu\ngeom.changes %zu\n", g.width, g.grid, g.slices, g.items, changes);
    const Commit w(BASE, groups, group_size);
    REGION(w, rows); REGION(w, part_a); REGION(w, part_b); REGION(w, st_zero); REGION(w, st_out);
    printf("bytes %zu\n", Commit::bytes(groups, group_size));
    return 0;
}

// prints what msm_shape.h plans for shapes given as row offsets: ./msm_shape_dump cap o_0 o_1 .. o_G [/ o_0 .. o_G' ...]  (cap: the most groups
// and rows a call takes; shapes are separated by "/").  Per shape either "shape i invalid" or
//   shape i groups G rows N passes P
//   pass p rows_in A rows_out B largest C team T iters I
//   desc first:count first:count ...                      (one line per pass, behind its "pass" line)
//   layout rows_in OFF rows_out OFF st_decode OFF part_a OFF st_a OFF part_b OFF st_b OFF bytes TOTAL
// A plan that was valid is built over an invalid shape once more, to show that a refused shape leaves the old plan as it was.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "msm_shape.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layout only computes addresses
static size_t off(const void* p) { return (size_t)(static_cast<const char*>(p) - BASE); }
static int dump(size_t index, const std::vector<uint32_t>& offsets, size_t cap) {
    using namespace fq_work;
    ShapePlan plan;
    const size_t groups = offsets.empty() ? 0 : offsets.size() - 1;
    if (plan.build(offsets.empty() ? nullptr : offsets.data(), groups, cap) != ShapePlan::OK) {
        if (plan.groups || plan.rows || !plan.passes.empty() || !plan.desc.empty()) return 3;        // a refused shape writes nothing
        printf("shape %zu invalid\n", index);
        return 0;
    }
    printf("shape %zu groups %zu rows %zu passes %zu\n", index, plan.groups, plan.rows, plan.passes.size());
    for (size_t p = 0; p < plan.passes.size(); p++) {
        const ShapePass& s = plan.passes[p];
        printf("pass %zu rows_in %zu rows_out %zu largest %u team %u iters %u\ndesc", p, s.rows_in, s.rows_out, s.largest, s.team, s.iters);
        for (size_t t = 0; t < s.rows_out; t++) printf(" %u:%u", plan.desc[s.desc_at + t].first, plan.desc[s.desc_at + t].count);
        printf("\n");
    }
    const MsmRagged w(BASE, plan.rows, plan.groups);
    printf("layout rows_in %zu rows_out %zu st_decode %zu part_a %zu st_a %zu part_b %zu st_b %zu bytes %zu\n", off(w.rows_in), off(w.rows_out), off(w.st_decode),
           off(w.part_a), off(w.st_a), off(w.part_b), off(w.st_b), MsmRagged::bytes(plan.rows, plan.groups));
    const uint32_t descending[] = { 0, 2, 1 };
    const ShapePlan before = plan;
    if (plan.build(descending, 2, cap) != ShapePlan::INVALID || plan.groups != before.groups || plan.rows != before.rows || plan.passes.size() != before.passes.size() ||
        plan.desc.size() != before.desc.size())
        return 4;
    return 0;
}
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const size_t cap = strtoull(argv[1], 0, 10);
    std::vector<uint32_t> offsets;
    size_t index = 0;
    for (int i = 2; i <= argc; i++) {
        if (i == argc || strcmp(argv[i], "/") == 0) {
            if (int rc = dump(index++, offsets, cap)) return rc;
            offsets.clear();
            continue;
        }
        offsets.push_back((uint32_t)strtoull(argv[i], 0, 10));
    }
    return 0;
}

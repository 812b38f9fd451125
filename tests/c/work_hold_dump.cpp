// drives fq_work::Hold (work_layout.h), the book of a buffer while calls are using it, the way WorkScope in fourq_amd.hip does: every scope
// keeps its parent's Hold and puts it back when it closes.  ./work_hold_dump buffer_bytes op...  with op = "open:NEED:EXTENT" or "close"
//   open   ->  "admit depth held extent grew" (at depth 0 the buffer grows to NEED where it is smaller: grew = 1), or "refuse depth held extent"
//              with the book unchanged -- a refused call opens nothing
//   close  ->  "close depth held extent", the parent's book again
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "work_layout.h"
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    size_t buffer = strtoull(argv[1], 0, 10);
    fq_work::Hold now;
    std::vector<fq_work::Hold> parents;
    for (int k = 2; k < argc; k++) {
        size_t need, extent;
        if (sscanf(argv[k], "open:%zu:%zu", &need, &extent) == 2) {
            if (!now.admits(need)) { printf("refuse %d %zu %zu\n", now.depth, now.held, now.extent); continue; }
            const bool grew = now.depth == 0 && need > buffer;
            if (grew) buffer = need;
            parents.push_back(now);
            now = now.opened(argv[k], buffer, extent);
            printf("admit %d %zu %zu %d\n", now.depth, now.held, now.extent, grew ? 1 : 0);
        } else {
            if (parents.empty()) return 3;
            now = parents.back();
            parents.pop_back();
            printf("close %d %zu %zu\n", now.depth, now.held, now.extent);
        }
    }
    return 0;
}

// prints what the work-buffer layouts of the later families take at given shapes: ./seq_layout_dump Layout a [b [c]] ...  ->  one line
// "Layout a b c bytes" per request (requests are separated by the layout names).  Keyset n | Commit groups group_size | Bucket groups
// group_size window | MsmRagged rows groups | Dleq rows groups | Vrf n | Shamir rows t | MulRows n
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "bucket_layout.h"
#include "commit_layout.h"
#include "dleq_layout.h"
#include "keyset_layout.h"
#include "msm_shape.h"
#include "shamir_layout.h"
#include "vrf_layout.h"
int main(int argc, char** argv) {
    using namespace fq_work;
    for (int i = 1; i < argc;) {
        const char* name = argv[i++];
        size_t a[3] = { 0, 0, 0 };
        int k = 0;
        while (i < argc && argv[i][0] >= '0' && argv[i][0] <= '9' && k < 3) a[k++] = strtoull(argv[i++], 0, 10);
        size_t bytes;
        if (!strcmp(name, "Keyset") && k == 1) bytes = Keyset::bytes(a[0]);
        else if (!strcmp(name, "Commit") && k == 2) bytes = Commit::bytes(a[0], a[1]);
        else if (!strcmp(name, "Bucket") && k == 3) bytes = Bucket::bytes(a[0], a[1], (unsigned)a[2]);
        else if (!strcmp(name, "MsmRagged") && k == 2) bytes = MsmRagged::bytes(a[0], a[1]);
        else if (!strcmp(name, "Dleq") && k == 2) bytes = Dleq::bytes(a[0], a[1]);
        else if (!strcmp(name, "Vrf") && k == 1) bytes = Vrf::bytes(a[0]);
        else if (!strcmp(name, "Shamir") && k == 2) bytes = Shamir::bytes(a[0], a[1]);
        else if (!strcmp(name, "MulRows") && k == 1) bytes = MulRows::bytes(a[0]);
        else return 2;
        printf("%s %zu %zu %zu %zu\n", name, a[0], a[1], a[2], bytes);
    }
    return 0;
}

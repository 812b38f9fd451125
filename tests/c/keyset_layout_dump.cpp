// prints the work-buffer layout of the calls over registered keys: ./keyset_layout_dump n  ->  lines "own.region offset", "inner bytes" (what
// the existing routes carve at the buffer's first byte in constant-time mode), "bytes total", "inner_extent value" (what the layout admits for
// its inner calls) and, of the two layouts those calls carve, "sig_verify.bytes", "sig_verify.inner_extent" and "double_mul.lent"
#include <cstdio>
#include <cstdlib>
#include "keyset_layout.h"
static char* const BASE = reinterpret_cast<char*>(uintptr_t(1) << 44);      // never dereferenced: the layout only computes addresses
static void region(const char* name, const void* p) { printf("own.%s %zu\n", name, (size_t)(static_cast<const char*>(p) - BASE)); }
#define REGION(w, member) region(#member, w.member)
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const size_t n = strtoull(argv[1], 0, 10);
    using namespace fq_work;
    const Keyset w(BASE, n);
    REGION(w, inner); REGION(w, s); REGION(w, h); REGION(w, r32); REGION(w, rows); REGION(w, pk32); REGION(w, pre);
    printf("inner %zu\n", DoubleMul::bytes(n));
    printf("bytes %zu\n", Keyset::bytes(n));
    printf("inner_extent %zu\nsig_verify.bytes %zu\nsig_verify.inner_extent %zu\ndouble_mul.lent %zu\n", Keyset::inner_extent(n), SigVerify::bytes(n), SigVerify::inner_extent(n), DoubleMul::lent(n));
    return 0;
}

// Runs the SHIPPED recoders of fourq_amd/csrc/recode.hip.h (recode, recode_nibbles: plain C++, compiled here for the host) against the
// bit-serial loop they replaced, which is kept below as the reference's loop reads (curve4q.py:358-380).
//   ./recode_check rows.bin out.bin n_random
// rows.bin: rows of four 64-bit words v[4].  out.bin receives, per row of rows.bin, 14 words from the SHIPPED code: sign, the three
// planes, top, the eight nibble words, top again (of recode_nibbles), for the caller to hold against its own oracle.  Then n_random more
// rows from a seeded generator.  Prints "rows", "differ", and for the file rows and the random rows separately how often every top digit
// and every carry out occurred (counted with the LOOP, i.e. on the inputs themselves).  Exit status 1 when anything differs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "recode.hip.h"

using fq::u32;
using fq::u64;

struct Ref {
    u64 sign, d[3];
    u32 w[8];
    u32 carry[3];
};
static Ref loop(const u64 vin[4]) {
    Ref r;
    memset(&r, 0, sizeof r);
    r.sign = vin[0] >> 1;
    u64 v[3] = { vin[1], vin[2], vin[3] };
    for (int i = 0; i < 64; i++) {
        const u64 nb1 = ~(r.sign >> i) & 1;
        u32 digit = 0;
        for (int j = 0; j < 3; j++) {
            const u64 b = v[j] & 1;
            r.d[j] |= b << i;
            v[j] = (v[j] >> 1) + (nb1 & b);
            digit |= (u32)b << j;
        }
        r.w[i / 8] |= (digit | ((u32)nb1 << 3)) << (4 * (i % 8));
    }
    for (int j = 0; j < 3; j++) {
        if (v[j] > 1) { fprintf(stderr, "the loop left %llu\n", (unsigned long long)v[j]); exit(3); }
        r.carry[j] = (u32)v[j];
    }
    return r;
}

struct Seen { unsigned long long top[8], carry[3][2]; };
static unsigned long long differ = 0;

static void check(const u64 v[4], Seen& seen, u64* out) {
    const Ref want = loop(v);
    const u32 top = want.carry[0] + 2 * want.carry[1] + 4 * want.carry[2];
    seen.top[top]++;
    for (int j = 0; j < 3; j++) seen.carry[j][want.carry[j]]++;
    const fq::EndoDigits e = fq::recode(v);
    const fq::EndoNibbles n = fq::recode_nibbles(v);
    bool ok = e.sign == want.sign && e.top == top && n.top == top;
    for (int j = 0; j < 3; j++) ok = ok && e.d[j] == want.d[j];
    for (int k = 0; k < 8; k++) ok = ok && n.w[k] == want.w[k];
    for (int i = 0; i < 64 && ok; i++)          // the two accessors the ladders read the planes with
        ok = fq::endo_digit(e, i) == ((want.w[i / 8] >> (4 * (i % 8))) & 7) && fq::endo_neg_mask(e, i) == 0u - ((want.w[i / 8] >> (4 * (i % 8) + 3)) & 1);
    if (!ok && differ++ < 5)
        fprintf(stderr, "differs: v = %016llx %016llx %016llx %016llx\n", (unsigned long long)v[0], (unsigned long long)v[1], (unsigned long long)v[2], (unsigned long long)v[3]);
    if (out) {
        out[0] = e.sign; out[1] = e.d[0]; out[2] = e.d[1]; out[3] = e.d[2]; out[4] = e.top;
        for (int k = 0; k < 8; k++) out[5 + k] = n.w[k];
        out[13] = n.top;
    }
}

static void report(const char* what, const Seen& s) {
    for (int t = 0; t < 8; t++) printf("%s top %d %llu\n", what, t, s.top[t]);
    for (int j = 0; j < 3; j++) for (int c = 0; c < 2; c++) printf("%s carry %d %d %llu\n", what, j + 1, c, s.carry[j][c]);
}

static u64 state = 0x243f6a8885a308d3ull;
static u64 next() {                             // splitmix64
    u64 z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<u64> rows;
    u64 v[4];
    while (fread(v, sizeof v, 1, fh) == 1) rows.insert(rows.end(), v, v + 4);
    fclose(fh);
    const size_t n = rows.size() / 4;
    std::vector<u64> out(n * 14);
    Seen file_seen, random_seen;
    memset(&file_seen, 0, sizeof file_seen);
    memset(&random_seen, 0, sizeof random_seen);
    for (size_t i = 0; i < n; i++) check(&rows[4 * i], file_seen, &out[14 * i]);
    fh = fopen(argv[2], "wb");
    if (!fh || fwrite(out.data(), 8, out.size(), fh) != out.size()) return 2;
    fclose(fh);
    const unsigned long long n_random = strtoull(argv[3], 0, 10);
    for (unsigned long long i = 0; i < n_random; i++) {
        // uniform words, and words thinned or thickened by a second draw: long runs where the carry of x + N dies at once or never
        const int kind = (int)(i % 4);
        for (int k = 0; k < 4; k++) {
            const u64 a = next(), b = next();
            v[k] = kind == 0 ? a : kind == 1 ? (a & b) : kind == 2 ? (a | b) : (k == 0 ? (a | b) : (a & b));
        }
        v[0] |= 1;                              // decompose() hands over an odd first word
        check(v, random_seen, 0);
    }
    printf("rows %zu %llu\n", n, n_random);
    report("file", file_seen);
    report("random", random_seen);
    printf("differ %llu\n", differ);
    return differ ? 1 : 0;
}

/* A C (not C++, not Python) host of libfourq_amd.so for the double-scalar calls: reads the fixture rows tests/test_gpu_double_mul.py
 * wrote (the reference's [k]G + [l]P: scalars, affine points and results, their encodings), builds the comb of G through the C ABI and
 * runs fourq_double_mul_affine_batch, fourq_double_mul_bytes_batch and fourq_verify_bytes_batch on host pointers; compares bit for bit.
 *   cc -std=c99 -I include -o double_mul_check tests/c/double_mul_check.c -L fourq_amd -lfourq_amd        exit status 0 = all equal */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fourq_amd.h"

static int fail(const char *what, int rc, fourq_ctx *ctx) {
    fprintf(stderr, "%s: %s (%d) %s\n", what, fourq_strerror(rc), rc, ctx ? fourq_last_error(ctx) : "");
    return 2;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: double_mul_check <vector file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    uint64_t n = 0, ct = 0, g_r1[FOURQ_R1_WORDS];
    if (fread(&n, 8, 1, f) != 1 || fread(&ct, 8, 1, f) != 1 || fread(g_r1, 8, FOURQ_R1_WORDS, f) != FOURQ_R1_WORDS || n == 0 || n > 4096) {
        fprintf(stderr, "bad header\n"); return 2; }
    uint64_t *k = malloc(n * 32), *l = malloc(n * 32), *points = malloc(n * 64), *want = malloc(n * 64), *got = malloc(n * 64);
    uint8_t *points32 = malloc(n * 32), *want32 = malloc(n * 32), *got32 = malloc(n * 32), *status = malloc(n), *ok = malloc(n);
    uint64_t *comb = malloc(FOURQ_COMB_WORDS * 8);
    if (fread(k, 32, n, f) != n || fread(l, 32, n, f) != n || fread(points, 64, n, f) != n || fread(want, 64, n, f) != n ||
        fread(points32, 32, n, f) != n || fread(want32, 32, n, f) != n) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);

    fourq_ctx *ctx = NULL;
    int rc = fourq_ctx_create(0, &ctx);
    if (rc != FOURQ_OK) return fail("fourq_ctx_create", rc, NULL);
    if (fourq_version() != FOURQ_ABI_VERSION) { fprintf(stderr, "library %d, header %d\n", fourq_version(), FOURQ_ABI_VERSION); return 1; }
    if ((rc = fourq_ctx_set_ct_select(ctx, (int)ct)) != FOURQ_OK) return fail("fourq_ctx_set_ct_select", rc, ctx);
    if ((rc = fourq_comb_table(ctx, g_r1, comb)) != FOURQ_OK) return fail("fourq_comb_table", rc, ctx);
    /* a NULL comb before any table was given is an error, not a guess */
    if (fourq_double_mul_affine_batch(ctx, k, NULL, l, points, got, (size_t)n) != FOURQ_ERR_INVALID) { fprintf(stderr, "NULL comb accepted with nothing staged\n"); return 1; }

    if ((rc = fourq_double_mul_affine_batch(ctx, k, comb, l, points, got, (size_t)n)) != FOURQ_OK) return fail("fourq_double_mul_affine_batch", rc, ctx);
    if (memcmp(got, want, n * 64) != 0) { fprintf(stderr, "affine results differ from the reference's\n"); return 1; }

    if ((rc = fourq_double_mul_bytes_batch(ctx, k, NULL, l, points32, got32, status, (size_t)n)) != FOURQ_OK) return fail("fourq_double_mul_bytes_batch", rc, ctx);
    for (uint64_t i = 0; i < n; i++) if (status[i] != 0) { fprintf(stderr, "row %llu: status %d\n", (unsigned long long)i, status[i]); return 1; }
    if (memcmp(got32, want32, n * 32) != 0) { fprintf(stderr, "encoded results differ from the reference's\n"); return 1; }

    if ((rc = fourq_verify_bytes_batch(ctx, k, comb, l, points32, want32, ok, status, (size_t)n)) != FOURQ_OK) return fail("fourq_verify_bytes_batch", rc, ctx);
    for (uint64_t i = 0; i < n; i++) if (ok[i] != 1 || status[i] != 0) { fprintf(stderr, "row %llu: a valid row was refused (ok %d, status %d)\n", (unsigned long long)i, ok[i], status[i]); return 1; }
    /* one flipped bit in what is expected, one key with its reserved bit set: exactly those two rows are refused */
    want32[5] ^= 0x10;
    if (n > 1) points32[32 + 15] |= 0x80;
    if ((rc = fourq_verify_bytes_batch(ctx, k, NULL, l, points32, want32, ok, status, (size_t)n)) != FOURQ_OK) return fail("fourq_verify_bytes_batch (spoiled)", rc, ctx);
    for (uint64_t i = 0; i < n; i++) {
        const int want_ok = !(i == 0 || i == 1), want_st = (i == 1) ? FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_RESERVED_BIT : 0;
        if (ok[i] != want_ok || status[i] != want_st) { fprintf(stderr, "row %llu: ok %d status %d, expected %d %d\n", (unsigned long long)i, ok[i], status[i], want_ok, want_st); return 1; }
    }
    fourq_ctx_destroy(ctx);
    printf("double_mul_check: %llu double-scalar rows bit-exact through the C ABI (affine, encoded, verify)\n", (unsigned long long)n);
    return 0;
}

/* A C (not C++, not Python) host of libfourq_amd.so for the grouped sums: reads the fixture groups tests/test_gpu_msm.py wrote (the
 * reference's sums: scalars, affine points and results, their encodings) and runs fourq_msm_affine_batch and fourq_msm_bytes_batch on host
 * pointers; compares bit for bit, then checks the argument rules and that a string which does not decode marks its own group only.
 *   cc -std=c99 -I include -o msm_check tests/c/msm_check.c -L fourq_amd -lfourq_amd        exit status 0 = all equal */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fourq_amd.h"

static int fail(const char *what, int rc, fourq_ctx *ctx) {
    fprintf(stderr, "%s: %s (%d) %s\n", what, fourq_strerror(rc), rc, ctx ? fourq_last_error(ctx) : "");
    return 2;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: msm_check <vector file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    uint64_t groups = 0, size = 0, ct = 0;
    if (fread(&groups, 8, 1, f) != 1 || fread(&size, 8, 1, f) != 1 || fread(&ct, 8, 1, f) != 1 || groups == 0 || size == 0 || groups * size > 4096) {
        fprintf(stderr, "bad header\n"); return 2; }
    const size_t n = (size_t)(groups * size), g = (size_t)groups;
    uint64_t *k = malloc(n * 32), *points = malloc(n * 64), *want = malloc(g * 64), *got = malloc(g * 64);
    uint8_t *points32 = malloc(n * 32), *want32 = malloc(g * 32), *got32 = malloc(g * 32), *status = malloc(g);
    if (fread(k, 32, n, f) != n || fread(points, 64, n, f) != n || fread(want, 64, g, f) != g || fread(points32, 32, n, f) != n ||
        fread(want32, 32, g, f) != g) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);

    fourq_ctx *ctx = NULL;
    int rc = fourq_ctx_create(0, &ctx);
    if (rc != FOURQ_OK) return fail("fourq_ctx_create", rc, NULL);
    if (fourq_version() != FOURQ_ABI_VERSION) { fprintf(stderr, "library %d, header %d\n", fourq_version(), FOURQ_ABI_VERSION); return 1; }
    if ((rc = fourq_ctx_set_ct_select(ctx, (int)ct)) != FOURQ_OK) return fail("fourq_ctx_set_ct_select", rc, ctx);

    if ((rc = fourq_msm_affine_batch(ctx, k, points, got, g, (size_t)size)) != FOURQ_OK) return fail("fourq_msm_affine_batch", rc, ctx);
    if (memcmp(got, want, g * 64) != 0) { fprintf(stderr, "affine sums differ from the reference's\n"); return 1; }

    if ((rc = fourq_msm_bytes_batch(ctx, k, points32, got32, status, g, (size_t)size)) != FOURQ_OK) return fail("fourq_msm_bytes_batch", rc, ctx);
    for (size_t i = 0; i < g; i++) if (status[i] != 0) { fprintf(stderr, "group %zu: status %d\n", i, status[i]); return 1; }
    if (memcmp(got32, want32, g * 32) != 0) { fprintf(stderr, "encoded sums differ from the reference's\n"); return 1; }

    /* no groups: nothing is touched; a group size of 0, or a count above the limit, is refused */
    memset(got, 0x5a, g * 64);
    if ((rc = fourq_msm_affine_batch(ctx, k, points, got, 0, (size_t)size)) != FOURQ_OK) return fail("fourq_msm_affine_batch (no groups)", rc, ctx);
    for (size_t i = 0; i < g * 64; i++) if (((uint8_t *)got)[i] != 0x5a) { fprintf(stderr, "a call without groups wrote\n"); return 1; }
    if (fourq_msm_affine_batch(ctx, k, points, got, g, 0) != FOURQ_ERR_INVALID) { fprintf(stderr, "group_size 0 accepted\n"); return 1; }
    if (fourq_msm_affine_batch(ctx, k, points, got, (size_t)FOURQ_MAX_BATCH, 2) != FOURQ_ERR_INVALID) { fprintf(stderr, "a count above FOURQ_MAX_BATCH accepted\n"); return 1; }
    if (fourq_msm_bytes_batch(ctx, k, points32, got32, status, (size_t)-1 / 2 + 2, 2) != FOURQ_ERR_INVALID) { fprintf(stderr, "an overflowing count accepted\n"); return 1; }

    /* the last element of the first group with its reserved bit set: that group reports it and is zeroed, the others are exact */
    points32[(size - 1) * 32 + 15] |= 0x80;
    if ((rc = fourq_msm_bytes_batch(ctx, k, points32, got32, status, g, (size_t)size)) != FOURQ_OK) return fail("fourq_msm_bytes_batch (spoiled)", rc, ctx);
    for (size_t i = 0; i < g; i++) {
        const int want_st = (i == 0) ? FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_RESERVED_BIT : 0;
        if (status[i] != want_st) { fprintf(stderr, "group %zu: status %d, expected %d\n", i, status[i], want_st); return 1; }
        for (size_t b = 0; b < 32; b++)
            if (got32[i * 32 + b] != (i == 0 ? 0 : want32[i * 32 + b])) { fprintf(stderr, "group %zu: byte %zu differs\n", i, b); return 1; }
    }
    fourq_ctx_destroy(ctx);
    printf("msm_check: %zu grouped sums bit-exact through the C ABI (affine, encoded, argument rules, status)\n", g);
    return 0;
}

/* A C (not C++, not Python) host of libfourq_amd.so for the hash-to-curve calls: reads the rows tests/test_gpu_h2c.py wrote (a DST,
 * messages, and the field elements, mapped points and results expected for them in both modes), runs every host-pointer call and the
 * primitive; compares bit for bit.
 *   cc -std=c99 -I include -o h2c_check tests/c/h2c_check.c -L fourq_amd -lfourq_amd        exit status 0 = all equal */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fourq_amd.h"

static int fail(const char *what, int rc, fourq_ctx *ctx) {
    fprintf(stderr, "%s: %s (%d) %s\n", what, fourq_strerror(rc), rc, ctx ? fourq_last_error(ctx) : "");
    return 2;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: h2c_check <vector file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    uint64_t n = 0, ct = 0, stride = 0, dst_len = 0;
    uint8_t dst[FOURQ_H2C_MAX_DST + 1];
    if (fread(&n, 8, 1, f) != 1 || fread(&ct, 8, 1, f) != 1 || fread(&stride, 8, 1, f) != 1 || fread(&dst_len, 8, 1, f) != 1 ||
        n < 2 || n > 4096 || stride == 0 || stride > FOURQ_SIG_MAX_MSG || dst_len < 1 || dst_len > FOURQ_H2C_MAX_DST ||
        fread(dst, 1, sizeof dst, f) != sizeof dst) { fprintf(stderr, "bad header\n"); return 2; }
    uint8_t *msgs = malloc(n * stride), *want32[2], *got32 = malloc(n * 32);
    uint32_t *lens = malloc(n * 4);
    uint64_t *want_u[2], *want_aff[2], *want_map = malloc(n * 64), *got_u = malloc(n * 64), *got_aff = malloc(n * 64);
    if (fread(msgs, stride, n, f) != n || fread(lens, 4, n, f) != n) { fprintf(stderr, "short file\n"); return 2; }
    for (int mode = 0; mode < 2; mode++) {           /* FOURQ_H2C_RO, then FOURQ_H2C_NU */
        const size_t count = mode == FOURQ_H2C_RO ? 2 : 1;
        want_u[mode] = malloc(n * count * 32); want_aff[mode] = malloc(n * 64); want32[mode] = malloc(n * 32);
        if (fread(want_u[mode], count * 32, n, f) != n || fread(want_aff[mode], 64, n, f) != n || fread(want32[mode], 32, n, f) != n) { fprintf(stderr, "short file\n"); return 2; }
    }
    if (fread(want_map, 64, n, f) != n) { fprintf(stderr, "short file\n"); return 2; }      /* map_to_curve of the NU mode's u */
    fclose(f);

    fourq_ctx *ctx = NULL;
    int rc = fourq_ctx_create(0, &ctx);
    if (rc != FOURQ_OK) return fail("fourq_ctx_create", rc, NULL);
    if (fourq_version() != FOURQ_ABI_VERSION) { fprintf(stderr, "library %d, header %d\n", fourq_version(), FOURQ_ABI_VERSION); return 1; }
    if ((rc = fourq_ctx_set_ct_select(ctx, (int)ct)) != FOURQ_OK) return fail("fourq_ctx_set_ct_select", rc, ctx);

    for (int mode = 0; mode < 2; mode++) {
        const size_t count = mode == FOURQ_H2C_RO ? 2 : 1;
        if ((rc = fourq_hash_to_field_batch(ctx, dst, (size_t)dst_len, mode, msgs, (size_t)stride, lens, 0, got_u, (size_t)n)) != FOURQ_OK) return fail("fourq_hash_to_field_batch", rc, ctx);
        if (memcmp(got_u, want_u[mode], n * count * 32) != 0) { fprintf(stderr, "mode %d: field elements differ\n", mode); return 1; }
        if ((rc = fourq_hash_to_curve_batch(ctx, dst, (size_t)dst_len, mode, msgs, (size_t)stride, lens, 0, got32, (size_t)n)) != FOURQ_OK) return fail("fourq_hash_to_curve_batch", rc, ctx);
        if (memcmp(got32, want32[mode], n * 32) != 0) { fprintf(stderr, "mode %d: encoded points differ\n", mode); return 1; }
        if ((rc = fourq_hash_to_curve_affine_batch(ctx, dst, (size_t)dst_len, mode, msgs, (size_t)stride, lens, 0, got_aff, (size_t)n)) != FOURQ_OK) return fail("fourq_hash_to_curve_affine_batch", rc, ctx);
        if (memcmp(got_aff, want_aff[mode], n * 64) != 0) { fprintf(stderr, "mode %d: affine points differ\n", mode); return 1; }
    }
    if ((rc = fourq_map_to_curve_batch(ctx, want_u[FOURQ_H2C_NU], got_aff, (size_t)n)) != FOURQ_OK) return fail("fourq_map_to_curve_batch", rc, ctx);
    if (memcmp(got_aff, want_map, n * 64) != 0) { fprintf(stderr, "mapped points differ\n"); return 1; }
    size_t iw = 0, ow = 0;
    if ((rc = fourq_prim_words(FOURQ_PT_MAP_ELL2, &iw, &ow)) != FOURQ_OK || iw != 4 || ow != 8) { fprintf(stderr, "FOURQ_PT_MAP_ELL2: %d, %zu -> %zu words\n", rc, iw, ow); return 1; }
    memset(got_aff, 0, n * 64);
    if ((rc = fourq_prim_batch(ctx, FOURQ_PT_MAP_ELL2, want_u[FOURQ_H2C_NU], got_aff, (size_t)n)) != FOURQ_OK) return fail("fourq_prim_batch", rc, ctx);
    if (memcmp(got_aff, want_map, n * 64) != 0) { fprintf(stderr, "mapped points of the primitive differ\n"); return 1; }

    /* what the calls refuse: an empty or oversize DST, an unknown mode, a length beyond the stride */
    if (fourq_hash_to_curve_batch(ctx, dst, 0, FOURQ_H2C_RO, msgs, (size_t)stride, lens, 0, got32, (size_t)n) != FOURQ_ERR_INVALID ||
        fourq_hash_to_curve_batch(ctx, dst, FOURQ_H2C_MAX_DST + 1, FOURQ_H2C_RO, msgs, (size_t)stride, lens, 0, got32, (size_t)n) != FOURQ_ERR_INVALID ||
        fourq_hash_to_curve_batch(ctx, NULL, (size_t)dst_len, FOURQ_H2C_RO, msgs, (size_t)stride, lens, 0, got32, (size_t)n) != FOURQ_ERR_INVALID ||
        fourq_hash_to_field_batch(ctx, dst, (size_t)dst_len, 2, msgs, (size_t)stride, lens, 0, got_u, (size_t)n) != FOURQ_ERR_INVALID) {
        fprintf(stderr, "a bad DST or mode was accepted\n"); return 1;
    }
    lens[0] = (uint32_t)stride + 1;
    if (fourq_hash_to_curve_batch(ctx, dst, (size_t)dst_len, FOURQ_H2C_RO, msgs, (size_t)stride, lens, 0, got32, (size_t)n) != FOURQ_ERR_INVALID) { fprintf(stderr, "a length beyond the stride was accepted\n"); return 1; }
    fourq_ctx_destroy(ctx);
    printf("h2c_check: %llu rows bit-exact through the C ABI (hash_to_field, map_to_curve, hash_to_curve, both modes)\n", (unsigned long long)n);
    return 0;
}

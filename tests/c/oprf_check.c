/* A C (not C++, not Python) host of libfourq_amd.so for the oblivious-PRF calls: reads the rows tests/test_gpu_oprf.py wrote (a DST,
 * messages, blinds, one key, and the inverses, blinded and evaluated elements and outputs expected for them), runs every host-pointer call
 * and the primitive; compares bit for bit.
 *   cc -std=c99 -I include -o oprf_check tests/c/oprf_check.c -L fourq_amd -lfourq_amd        exit status 0 = all equal */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fourq_amd.h"

static int fail(const char *what, int rc, fourq_ctx *ctx) {
    fprintf(stderr, "%s: %s (%d) %s\n", what, fourq_strerror(rc), rc, ctx ? fourq_last_error(ctx) : "");
    return 2;
}
static int all_zero(const uint8_t *p, size_t bytes) {
    for (size_t i = 0; i < bytes; i++) if (p[i]) return 0;
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: oprf_check <vector file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    uint64_t n = 0, ct = 0, stride = 0, dst_len = 0, key[4];
    uint8_t dst[FOURQ_H2C_MAX_DST + 1];
    if (fread(&n, 8, 1, f) != 1 || fread(&ct, 8, 1, f) != 1 || fread(&stride, 8, 1, f) != 1 || fread(&dst_len, 8, 1, f) != 1 ||
        n < 2 || n > 4096 || stride == 0 || stride > FOURQ_SIG_MAX_MSG || dst_len < 1 || dst_len > FOURQ_H2C_MAX_DST ||
        fread(dst, 1, sizeof dst, f) != sizeof dst) { fprintf(stderr, "bad header\n"); return 2; }
    uint8_t *msgs = malloc(n * stride), *want_blinded = malloc(n * 32), *want_evaluated = malloc(n * 32), *want_out = malloc(n * 64);
    uint8_t *got32 = malloc(n * 32), *got64 = malloc(n * 64), *status = malloc(n);
    uint32_t *lens = malloc(n * 4);
    uint64_t *blinds = malloc(n * 32), *want_inv = malloc(n * 32), *got_inv = malloc(n * 32);
    if (fread(msgs, stride, n, f) != n || fread(lens, 4, n, f) != n || fread(blinds, 32, n, f) != n || fread(key, 8, 4, f) != 4 || fread(want_inv, 32, n, f) != n ||
        fread(want_blinded, 32, n, f) != n || fread(want_evaluated, 32, n, f) != n || fread(want_out, 64, n, f) != n) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);

    fourq_ctx *ctx = NULL;
    int rc = fourq_ctx_create(0, &ctx);
    if (rc != FOURQ_OK) return fail("fourq_ctx_create", rc, NULL);
    if (fourq_version() != FOURQ_ABI_VERSION) { fprintf(stderr, "library %d, header %d\n", fourq_version(), FOURQ_ABI_VERSION); return 1; }
    if ((rc = fourq_ctx_set_ct_select(ctx, (int)ct)) != FOURQ_OK) return fail("fourq_ctx_set_ct_select", rc, ctx);

    if ((rc = fourq_scalar_inv_batch(ctx, blinds, got_inv, (size_t)n)) != FOURQ_OK) return fail("fourq_scalar_inv_batch", rc, ctx);
    if (memcmp(got_inv, want_inv, n * 32) != 0) { fprintf(stderr, "inverses differ\n"); return 1; }
    size_t iw = 0, ow = 0;
    if ((rc = fourq_prim_words(FOURQ_SC_INV, &iw, &ow)) != FOURQ_OK || iw != 4 || ow != 4) { fprintf(stderr, "FOURQ_SC_INV: %d, %zu -> %zu words\n", rc, iw, ow); return 1; }
    memset(got_inv, 0xff, n * 32);
    if ((rc = fourq_prim_batch(ctx, FOURQ_SC_INV, blinds, got_inv, (size_t)n)) != FOURQ_OK) return fail("fourq_prim_batch", rc, ctx);
    if (memcmp(got_inv, want_inv, n * 32) != 0) { fprintf(stderr, "inverses of the primitive differ\n"); return 1; }

    if ((rc = fourq_oprf_blind_batch(ctx, dst, (size_t)dst_len, msgs, (size_t)stride, lens, 0, blinds, got32, status, (size_t)n)) != FOURQ_OK) return fail("fourq_oprf_blind_batch", rc, ctx);
    if (!all_zero(status, n) || memcmp(got32, want_blinded, n * 32) != 0) { fprintf(stderr, "blinded elements differ\n"); return 1; }
    if ((rc = fourq_oprf_evaluate_batch(ctx, key, want_blinded, got32, status, (size_t)n)) != FOURQ_OK) return fail("fourq_oprf_evaluate_batch", rc, ctx);
    if (!all_zero(status, n) || memcmp(got32, want_evaluated, n * 32) != 0) { fprintf(stderr, "evaluated elements differ\n"); return 1; }
    if ((rc = fourq_oprf_finalize_batch(ctx, dst, (size_t)dst_len, msgs, (size_t)stride, lens, 0, blinds, want_evaluated, got64, status, (size_t)n)) != FOURQ_OK) return fail("fourq_oprf_finalize_batch", rc, ctx);
    if (!all_zero(status, n) || memcmp(got64, want_out, n * 64) != 0) { fprintf(stderr, "finalized outputs differ\n"); return 1; }
    memset(got64, 0xff, n * 64);
    if ((rc = fourq_oprf_eval_batch(ctx, key, dst, (size_t)dst_len, msgs, (size_t)stride, lens, 0, got64, status, (size_t)n)) != FOURQ_OK) return fail("fourq_oprf_eval_batch", rc, ctx);
    if (!all_zero(status, n) || memcmp(got64, want_out, n * 64) != 0) { fprintf(stderr, "direct evaluations differ\n"); return 1; }

    /* a zero blind: FOURQ_OPRF_BLIND_ZERO and a zero row, the neighbour untouched */
    memset(blinds, 0, 32);
    if ((rc = fourq_oprf_blind_batch(ctx, dst, (size_t)dst_len, msgs, (size_t)stride, lens, 0, blinds, got32, status, (size_t)n)) != FOURQ_OK) return fail("fourq_oprf_blind_batch", rc, ctx);
    if (status[0] != FOURQ_OPRF_BLIND_ZERO || !all_zero(got32, 32) || status[1] != 0 || memcmp(got32 + 32, want_blinded + 32, 32) != 0) { fprintf(stderr, "a zero blind was not reported\n"); return 1; }
    if ((rc = fourq_oprf_finalize_batch(ctx, dst, (size_t)dst_len, msgs, (size_t)stride, lens, 0, blinds, want_evaluated, got64, status, (size_t)n)) != FOURQ_OK) return fail("fourq_oprf_finalize_batch", rc, ctx);
    if (status[0] != FOURQ_OPRF_BLIND_ZERO || !all_zero(got64, 64) || status[1] != 0 || memcmp(got64 + 64, want_out + 64, 64) != 0) { fprintf(stderr, "a zero blind was not reported by finalize\n"); return 1; }

    /* what the calls refuse: an empty or oversize DST, a missing key, a length beyond the stride */
    if (fourq_oprf_blind_batch(ctx, dst, 0, msgs, (size_t)stride, lens, 0, blinds, got32, status, (size_t)n) != FOURQ_ERR_INVALID ||
        fourq_oprf_eval_batch(ctx, key, dst, FOURQ_H2C_MAX_DST + 1, msgs, (size_t)stride, lens, 0, got64, status, (size_t)n) != FOURQ_ERR_INVALID ||
        fourq_oprf_finalize_batch(ctx, NULL, (size_t)dst_len, msgs, (size_t)stride, lens, 0, blinds, want_evaluated, got64, status, (size_t)n) != FOURQ_ERR_INVALID ||
        fourq_oprf_evaluate_batch(ctx, NULL, want_blinded, got32, status, (size_t)n) != FOURQ_ERR_INVALID) {
        fprintf(stderr, "a bad DST or key was accepted\n"); return 1;
    }
    lens[0] = (uint32_t)stride + 1;
    if (fourq_oprf_eval_batch(ctx, key, dst, (size_t)dst_len, msgs, (size_t)stride, lens, 0, got64, status, (size_t)n) != FOURQ_ERR_INVALID) { fprintf(stderr, "a length beyond the stride was accepted\n"); return 1; }
    fourq_ctx_destroy(ctx);
    printf("oprf_check: %llu rows bit-exact through the C ABI (scalar_inv, blind, evaluate, finalize, eval)\n", (unsigned long long)n);
    return 0;
}

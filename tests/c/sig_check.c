/* A C (not C++, not Python) host of libfourq_amd.so for the signature calls: reads the rows tests/test_gpu_sig.py wrote (secret keys,
 * messages, and the public keys, signatures and SHA-512 digests expected for them), builds the comb of G through the C ABI, generates
 * the keys, signs and verifies on host pointers; compares bit for bit.
 *   cc -std=c99 -I include -o sig_check tests/c/sig_check.c -L fourq_amd -lfourq_amd        exit status 0 = all equal */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fourq_amd.h"

static int fail(const char *what, int rc, fourq_ctx *ctx) {
    fprintf(stderr, "%s: %s (%d) %s\n", what, fourq_strerror(rc), rc, ctx ? fourq_last_error(ctx) : "");
    return 2;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: sig_check <vector file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    uint64_t n = 0, ct = 0, stride = 0, g_r1[FOURQ_R1_WORDS];
    if (fread(&n, 8, 1, f) != 1 || fread(&ct, 8, 1, f) != 1 || fread(&stride, 8, 1, f) != 1 || fread(g_r1, 8, FOURQ_R1_WORDS, f) != FOURQ_R1_WORDS ||
        n < 3 || n > 4096 || stride == 0 || stride > FOURQ_SIG_MAX_MSG) { fprintf(stderr, "bad header\n"); return 2; }
    uint8_t *sk = malloc(n * 32), *msgs = malloc(n * stride), *want_pk = malloc(n * 32), *want_sig = malloc(n * 64), *want_hash = malloc(n * 64);
    uint8_t *pk = malloc(n * 32), *sig = malloc(n * 64), *hash = malloc(n * 64), *ok = malloc(n), *status = malloc(n);
    uint32_t *lens = malloc(n * 4);
    uint64_t *comb = malloc(FOURQ_COMB_WORDS * 8);
    if (fread(sk, 32, n, f) != n || fread(msgs, stride, n, f) != n || fread(lens, 4, n, f) != n || fread(want_pk, 32, n, f) != n ||
        fread(want_sig, 64, n, f) != n || fread(want_hash, 64, n, f) != n) { fprintf(stderr, "short file\n"); return 2; }
    fclose(f);

    fourq_ctx *ctx = NULL;
    int rc = fourq_ctx_create(0, &ctx);
    if (rc != FOURQ_OK) return fail("fourq_ctx_create", rc, NULL);
    if (fourq_version() != FOURQ_ABI_VERSION) { fprintf(stderr, "library %d, header %d\n", fourq_version(), FOURQ_ABI_VERSION); return 1; }
    if ((rc = fourq_ctx_set_ct_select(ctx, (int)ct)) != FOURQ_OK) return fail("fourq_ctx_set_ct_select", rc, ctx);
    if ((rc = fourq_comb_table(ctx, g_r1, comb)) != FOURQ_OK) return fail("fourq_comb_table", rc, ctx);

    if ((rc = fourq_sha512_batch(ctx, msgs, (size_t)stride, lens, 0, hash, (size_t)n)) != FOURQ_OK) return fail("fourq_sha512_batch", rc, ctx);
    if (memcmp(hash, want_hash, n * 64) != 0) { fprintf(stderr, "SHA-512 digests differ\n"); return 1; }

    /* a NULL comb before any table was given is an error, not a guess */
    if (fourq_sig_keygen_batch(ctx, sk, NULL, pk, (size_t)n) != FOURQ_ERR_INVALID) { fprintf(stderr, "NULL comb accepted with nothing staged\n"); return 1; }
    if ((rc = fourq_sig_keygen_batch(ctx, sk, comb, pk, (size_t)n)) != FOURQ_OK) return fail("fourq_sig_keygen_batch", rc, ctx);
    if (memcmp(pk, want_pk, n * 32) != 0) { fprintf(stderr, "public keys differ\n"); return 1; }

    if ((rc = fourq_sig_sign_batch(ctx, sk, pk, NULL, msgs, (size_t)stride, lens, 0, sig, (size_t)n)) != FOURQ_OK) return fail("fourq_sig_sign_batch", rc, ctx);
    if (memcmp(sig, want_sig, n * 64) != 0) { fprintf(stderr, "signatures differ\n"); return 1; }

    if ((rc = fourq_sig_verify_batch(ctx, pk, comb, msgs, (size_t)stride, lens, 0, sig, ok, status, (size_t)n)) != FOURQ_OK) return fail("fourq_sig_verify_batch", rc, ctx);
    for (uint64_t i = 0; i < n; i++) if (ok[i] != 1 || status[i] != 0) { fprintf(stderr, "row %llu: a valid signature was refused (ok %d, status %d)\n", (unsigned long long)i, ok[i], status[i]); return 1; }

    /* a flipped bit in R, a key with its reserved bit set, an s of all ones: exactly those three rows are refused, each with its reason */
    sig[5] ^= 0x10;
    pk[32 + 15] |= 0x80;
    memset(sig + 2 * 64 + 32, 0xff, 32);
    if ((rc = fourq_sig_verify_batch(ctx, pk, NULL, msgs, (size_t)stride, lens, 0, sig, ok, status, (size_t)n)) != FOURQ_OK) return fail("fourq_sig_verify_batch (spoiled)", rc, ctx);
    for (uint64_t i = 0; i < n; i++) {
        const int want_ok = i > 2, want_st = i == 1 ? FOURQ_BYTES_DECODE_BASE + FOURQ_DECODE_RESERVED_BIT : i == 2 ? FOURQ_SIG_S_RANGE : 0;
        if (ok[i] != want_ok || status[i] != want_st) { fprintf(stderr, "row %llu: ok %d status %d, expected %d %d\n", (unsigned long long)i, ok[i], status[i], want_ok, want_st); return 1; }
    }
    /* a length beyond the stride is refused by the host-pointer calls */
    lens[0] = (uint32_t)stride + 1;
    if (fourq_sig_verify_batch(ctx, pk, NULL, msgs, (size_t)stride, lens, 0, sig, ok, status, (size_t)n) != FOURQ_ERR_INVALID) { fprintf(stderr, "a length beyond the stride was accepted\n"); return 1; }
    fourq_ctx_destroy(ctx);
    printf("sig_check: %llu signature rows bit-exact through the C ABI (hash, keygen, sign, verify)\n", (unsigned long long)n);
    return 0;
}

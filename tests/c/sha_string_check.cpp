// Runs the SHIPPED string filler, tail builder and rows hasher of fourq_amd/csrc/sha512.hip.h (plain C++, compiled here for the host) on
// cases a file describes, and writes what they produce for the caller to hold against its own SHA-512 of the string it assembled itself.
//   ./sha_string_check cases.bin out.bin
// cases.bin: u32 pool_len, the pool, then cases of twelve u32 (struct Case); every byte string of a case is a slice of the pool.
// out.bin: per case 64 digest bytes -- for SHAPE_TAIL the tail's words as big-endian bytes and its length instead.
// Every row is copied to the END of a heap allocation of its own that is exactly as long as the row needs, at the alignment the case asks
// for, so under AddressSanitizer a read at or past row + len stops the program; UndefinedBehaviorSanitizer stops a whole-word load from an
// address its load mode does not allow.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sha512.hip.h"

using namespace fq;

enum Shape {
    SHAPE_PAD_0 = 0, SHAPE_PAD_4 = 1, SHAPE_PAD_8 = 2,      // PW words || row, padding only
    SHAPE_TAIL_BEFORE = 3,                                   // 128 bytes hashed in front; row || tail
    SHAPE_PRE_TAIL = 4,                                      // 4 words || row || tail
    SHAPE_PRE_TAIL_BEFORE = 5,                               // 128 bytes hashed in front; 4 words || row || tail
    SHAPE_ROWS_1 = 6, SHAPE_ROWS_3_COUNTER = 7, SHAPE_ROWS_5 = 8,
    SHAPE_TAIL = 9                                           // the builder's words
};
struct Case { u32 shape, align, mode, len, row_off, head_len, head_off, dst_len, dst_off, counter, pre_off, unused; };

static std::vector<uint8_t> pool;

// `len` pool bytes from `off` at the end of their own allocation, the first of them at `align` modulo 16
struct Row {
    uint8_t* block;
    uint8_t* at;
    Row(u32 off, u32 len, u32 align) {
        block = (uint8_t*)malloc(16 + align + len);          // never empty, so that a row of length 0 is the end of something
        if (!block || ((uintptr_t)block & 15)) { fprintf(stderr, "malloc: no 16-byte aligned block\n"); exit(2); }
        at = block + 16 + align;
        if (len) memcpy(at, &pool[off], len);
    }
    ~Row() { free(block); }
    Row(const Row&) = delete;
};

template <int PW, class Tail> static void hash_string(u64 h[8], const u64* pre, const Row& row, const Case& c, const Tail& tail, u32 before) {
    if (before == 0) {
        sha512_hash<PW>(h, pre, row.at, c.len, tail, (int)c.mode);
        return;
    }
    for (int k = 0; k < 8; k++) h[k] = SHA512_ZPAD_MID[k];
    const u32 blocks = sha512_blocks(8 * PW + c.len + sha_tail_len(tail));
    for (u32 b = 0; b < blocks; b++) {
        u64 w[16];
        sha512_fill<PW>(w, pre, row.at, c.len, tail, before, b, blocks, (int)c.mode);
        sha512_compress(h, w);
    }
}

template <int R, bool COUNTER> static void hash_rows(u64 h[8], const Case& c, const ShaTail& tail) {
    std::vector<Row*> own;
    const uint8_t* rows[R];
    for (int r = 0; r < R; r++) {
        own.push_back(new Row(c.pre_off + 32 * r, 32, 0));
        rows[r] = own.back()->at;
    }
    sha512_hash_rows<R, COUNTER>(h, rows, c.counter, tail);
    for (Row* r : own) delete r;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = fopen(argv[1], "rb");
    u32 pool_len;
    if (!fh || fread(&pool_len, 4, 1, fh) != 1) return 2;
    pool.resize(pool_len);
    if (fread(pool.data(), 1, pool_len, fh) != pool_len) return 2;
    std::vector<Case> cases;
    Case c;
    while (fread(&c, sizeof c, 1, fh) == 1) cases.push_back(c);
    fclose(fh);
    fh = fopen(argv[2], "wb");
    if (!fh) return 2;
    unsigned long long hashes = 0;
    for (const Case& k : cases) {
        if (k.align > 15 || k.mode > SHA_LOAD_16 || (k.mode == SHA_LOAD_16 && k.align % 16) || (k.mode == SHA_LOAD_8 && k.align % 8)) return 2;
        const ShaTail tail = k.dst_len ? sha_make_tail(&pool[k.head_off], k.head_len, &pool[k.dst_off], k.dst_len) : ShaTail();
        if (k.shape == SHAPE_TAIL) {
            uint8_t out[8 * SHA_TAIL_WORDS + 4];
            for (int w = 0; w < SHA_TAIL_WORDS; w++) for (int b = 0; b < 8; b++) out[8 * w + b] = (uint8_t)(tail.w[w] >> (56 - 8 * b));
            memcpy(out + 8 * SHA_TAIL_WORDS, &tail.len, 4);
            if (fwrite(out, 1, sizeof out, fh) != sizeof out) return 2;
            continue;
        }
        u64 pre[8], h[8];
        for (int w = 0; w < 8; w++) {
            pre[w] = 0;
            for (int b = 0; b < 8; b++) pre[w] = (pre[w] << 8) | pool[k.pre_off + 8 * w + b];
        }
        if (k.shape <= SHAPE_PRE_TAIL_BEFORE) {
            const Row row(k.row_off, k.len, k.align);
            switch (k.shape) {
            case SHAPE_PAD_0: hash_string<0>(h, nullptr, row, k, ShaPad{}, 0); break;
            case SHAPE_PAD_4: hash_string<4>(h, pre, row, k, ShaPad{}, 0); break;
            case SHAPE_PAD_8: hash_string<8>(h, pre, row, k, ShaPad{}, 0); break;
            case SHAPE_TAIL_BEFORE: hash_string<0>(h, nullptr, row, k, tail, 128); break;
            case SHAPE_PRE_TAIL: hash_string<4>(h, pre, row, k, tail, 0); break;
            default: hash_string<4>(h, pre, row, k, tail, 128); break;
            }
        } else if (k.shape == SHAPE_ROWS_1) hash_rows<1, false>(h, k, tail);
        else if (k.shape == SHAPE_ROWS_3_COUNTER) hash_rows<3, true>(h, k, tail);
        else if (k.shape == SHAPE_ROWS_5) hash_rows<5, false>(h, k, tail);
        else return 2;
        uint8_t out[64];
        for (int w = 0; w < 8; w++) for (int b = 0; b < 8; b++) out[8 * w + b] = (uint8_t)(h[w] >> (56 - 8 * b));
        if (fwrite(out, 1, 64, fh) != 64) return 2;
        hashes++;
    }
    if (fclose(fh)) return 2;
    printf("cases %zu hashes %llu\n", cases.size(), hashes);
    return 0;
}

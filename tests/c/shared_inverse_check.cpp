// The slot geometry of a lane and the shared inversion (fourq_amd/csrc/lower.hip.h: LaneSlots, SharedInverse) on the CPU: this program
// includes the shipped header with an ordinary C++ compiler and instantiates both over the integers modulo 251 -- a field small enough that
// zeros are frequent and every inverse can be checked by one multiplication.  tests/test_shared_inverse_host.py builds and runs it, a second
// time under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// K in {1, 2, 4, 8}, every n from 1 to 4 K + 3, every lane t < T and three lanes past it; masks: none, all, each single element, 200 seeded
// random ones.  An element that is zero is masked besides (as lower_kernel masks a zero norm); on every second mask the slots past the end
// are masked too (as normalize_kernel masks them), on the others they enter with the value of the lane's first element (as lower_kernel lets them).
// The elements sit in a heap block of exactly n bytes, so a slot that loads a row >= n is a heap overflow for the sanitizer as well.
//
//   usage: shared_inverse_check        prints "cases <masks run> lanes <lanes run>"; exit status 1 and one line on the first failure
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "lower.hip.h"

using fq::u32;

static const u32 P = 251;
static unsigned long inv_calls = 0;

struct ToyOps {
    typedef u32 E;
    static E one() { return 1; }
    static E mul(E a, E b) { return a * b % P; }
    static E inv(E a) {                                    // a^(P - 2); 0 -> 0, as the field's chain
        inv_calls++;
        E r = 1;
        for (u32 e = P - 2; e; e >>= 1, a = a * a % P) if (e & 1) r = r * a % P;
        return r;
    }
    static E select(bool keep, E x, E y) { return keep ? x : y; }
};

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static u32 rnd() {                                         // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (u32)((rng_state * 0x2545F4914F6CDD1Dull) >> 33);
}

#define FAIL(...) do { printf("FAIL K=%d n=%u mask=%d: ", K, n, mask_no); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

static unsigned long cases = 0, lanes = 0;

// one pass over all lanes: res[id] = what slot `id` got; the checks that need no second run are made here
template <int K> static void run(const uint8_t* elem, u32 n, const std::vector<uint8_t>& masked, bool mask_dead, int mask_no, std::vector<u32>& res) {
    std::vector<int> produced(n, 0);
    const u32 T = (n + K - 1) / K;
    for (u32 t = 0; t < T + 3; t++) {
        fq::LaneSlots<K> s(n);
        const bool owns = s.lane(t);
        if (s.T != T) FAIL("T = %u, want %u", s.T, T);
        if (owns != (t < T)) FAIL("lane %u: owns = %d", t, (int)owns);
        if (!owns) {
            for (int j = 0; j < K; j++) if (s.live(j) && s.id(j) < T) FAIL("lane %u past the end claims id %u of a lane in front", t, s.id(j));
            continue;
        }
        lanes++;
        const unsigned long before = inv_calls;
        fq::SharedInverse<K, ToyOps> si;
        u32 e[K];
        bool keep[K];
        for (int j = 0; j < K; j++) {
            const u32 at = s.at(j);
            if (at >= n) FAIL("lane %u slot %d loads row %u", t, j, at);
            if (s.live(j) != (s.id(j) < n)) FAIL("lane %u slot %d: live", t, j);
            if (s.live(j) && at != s.id(j)) FAIL("lane %u slot %d: a live slot loads row %u, not its own %u", t, j, at, s.id(j));
            if (!s.live(j) && at != t) FAIL("lane %u slot %d: a slot past the end loads row %u, not the lane's first", t, j, at);
            e[j] = elem[at];
            keep[j] = e[j] != 0 && !masked[at] && !(mask_dead && !s.live(j));
            si.take(j, e[j], keep[j]);
        }
        si.invert();
        for (int j = K - 1; j >= 0; j--) {
            const u32 r = si.peel(j);
            if (keep[j] && ToyOps::mul(r, e[j]) != 1) FAIL("lane %u slot %d: %u * %u != 1", t, j, e[j], r);
            if (!s.live(j)) continue;
            produced[s.id(j)]++;
            res[s.id(j)] = r;
        }
        if (inv_calls != before + 1) FAIL("lane %u called inv %lu times", t, inv_calls - before);
    }
    for (u32 i = 0; i < n; i++) if (produced[i] != 1) FAIL("id %u produced %d times", i, produced[i]);
    cases++;
}

template <int K> static void all_sizes() {
    for (u32 n = 1; n <= 4 * K + 3; n++) {
        uint8_t* elem = (uint8_t*)malloc(n);               // exactly n bytes: row n is past the block
        for (u32 i = 0; i < n; i++) elem[i] = (rnd() % 4 == 0) ? 0 : (uint8_t)(rnd() % P);
        std::vector<uint8_t> masked(n, 0);
        std::vector<u32> base(n, 0), res(n, 0);
        int mask_no = 0;
        run<K>(elem, n, masked, false, mask_no, base);     // nobody masked (but the zeros)
        for (u32 i = 0; i < n; i++) if (elem[i] != 0 && ToyOps::mul(base[i], elem[i]) != 1) FAIL("id %u: %u * %u != 1", i, (u32)elem[i], base[i]);
        // a masked element leaves every other result as the run without the mask gave it
        const int total = 2 + (int)n + 200;
        for (mask_no = 1; mask_no < total; mask_no++) {
            for (u32 i = 0; i < n; i++) masked[i] = mask_no == 1 ? 1 : mask_no < 2 + (int)n ? (i == (u32)(mask_no - 2)) : (uint8_t)(rnd() & 1);
            run<K>(elem, n, masked, (mask_no & 1) != 0, mask_no, res);
            for (u32 i = 0; i < n; i++)
                if (!masked[i] && elem[i] != 0 && res[i] != base[i]) FAIL("id %u: %u with the mask, %u without", i, res[i], base[i]);
        }
        free(elem);
    }
}

int main() {
    all_sizes<1>();
    all_sizes<2>();
    all_sizes<4>();
    all_sizes<8>();
    printf("cases %lu lanes %lu\n", cases, lanes);
    return 0;
}

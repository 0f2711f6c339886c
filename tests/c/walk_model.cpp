/*
 * walk_model.cpp -- the fused segment walk of K1's greedy path (csrc/dmx_walk.h:
 * dmx_walk_segment, one literal run plus one match per trip) against a position-by-position
 * sequential walk, under AddressSanitizer + UBSan.  Built by tests/c/Makefile.walk from this
 * file alone; runs without a GPU.
 * The length table is a heap block of exactly bn bytes, so ASan sees a read at or past bn.
 * Compared in every case: the path word, the exit, the merged flag; the trip count stays
 * <= DMX_WALK_TRIPS.  Case classes: every literal word with <= 4 runs; random literal words;
 * random lengths 3..258 (and short ones, so that a segment holds many matches); every entry
 * offset 0..31; bn cutting the segment at every offset; literal bits set past bn; a current
 * path word met first inside a literal run, first at a match, and never.
 * Exit status 0 = "0 failed checks" (the sanitizers abort on their own findings).
 */
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "dmx_walk.h"

static int fails;
static long checks;
#define CHECK(c, ...) do { checks++; if (!(c)) { if (fails < 50) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } fails++; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t rnd(uint32_t n) { return (uint32_t)(rnd64() % n); }

enum Met { MET_NEVER, MET_LITERAL, MET_MATCH };

// the sequential walk: one position per step
static uint32_t seq_walk(uint32_t lo, uint32_t e, uint32_t bn, uint32_t lw, bool merge, uint32_t m, uint32_t x,
                         const uint8_t* len8, uint32_t& word, bool& merged, Met& met) {
    uint32_t nm = 0, p = e;
    merged = false;
    met = MET_NEVER;
    while (p < lo + 32 && p < bn) {
        const uint32_t sh = p - lo, bit = 1u << sh;
        const bool lit = (lw >> sh) & 1u;
        if (merge && (m & bit)) {
            word = nm | (m & ~(bit - 1u));
            merged = true;
            met = lit ? MET_LITERAL : MET_MATCH;
            return x;
        }
        nm |= bit;
        p += lit ? 1u : (uint32_t)len8[p] + 3u;
    }
    word = nm;
    return p;
}

static long met_count[3];

static void check(uint32_t lo, uint32_t e, uint32_t bn, uint32_t lw, bool merge, uint32_t m, uint32_t x,
                  const std::vector<uint8_t>& len8, const char* what) {
    uint32_t w0, w1, trips = 0;
    bool g0, g1;
    Met met;
    const uint8_t* T = len8.data();
    const uint32_t x0 = seq_walk(lo, e, bn, lw, merge, m, x, T, w0, g0, met);
    auto len_at = [T](uint32_t p) { return (uint32_t)T[p]; };
    const uint32_t x1 = merge ? dmx_walk_segment<true>(lo, e, bn, lw, m, x, len_at, w1, g1, &trips)
                              : dmx_walk_segment<false>(lo, e, bn, lw, 0u, 0u, len_at, w1, g1, &trips);
    if (merge) met_count[met]++;
    CHECK(x0 == x1 && w0 == w1 && g0 == g1 && trips <= DMX_WALK_TRIPS,
          "%s: lo=%u e=%u bn=%u lw=%08x merge=%d m=%08x x=%u: exit %u/%u word %08x/%08x merged %d/%d trips %u", what, lo, e,
          bn, lw, (int)merge, m, x, x1, x0, w1, w0, (int)g1, (int)g0, trips);
}

static void fill(std::vector<uint8_t>& t, int mode) {   // 0: lengths 3..258; 1: 3..6 (many matches per segment); 2: all 258
    for (auto& b : t) b = mode == 0 ? (uint8_t)rnd(256) : mode == 1 ? (uint8_t)rnd(4) : (uint8_t)255;
}

// the current path of a segment: the sequential walk from some entry (what W1 or a round left)
static uint32_t path_from(uint32_t lo, uint32_t e, uint32_t bn, uint32_t lw, const std::vector<uint8_t>& len8, uint32_t& x) {
    uint32_t w;
    bool g;
    Met met;
    x = seq_walk(lo, e, bn, lw, false, 0, 0, len8.data(), w, g, met);
    return w;
}

int main() {
    // every literal word with <= 4 runs of literals (<= 8 boundaries among 33), from the segment start
    {
        const uint32_t lo = 32, bn = 96;
        std::vector<uint8_t> t0(bn), t1(bn);
        fill(t0, 0);
        fill(t1, 1);
        long words = 0;
        uint32_t b[8];
        for (int nb = 0; nb <= 8; nb += 2) {
            // boundaries b[0] < b[1] < ... in 0..32: bits [b[0], b[1]), [b[2], b[3]), ... are literals
            for (int i = 0; i < nb; i++) b[i] = (uint32_t)i;
            for (;;) {
                uint64_t lw = 0;
                for (int i = 0; i < nb; i += 2) lw |= ((1ull << b[i + 1]) - 1ull) & ~((1ull << b[i]) - 1ull);
                words++;
                check(lo, lo, bn, (uint32_t)lw, false, 0, 0, (words & 1) ? t0 : t1, "runs<=4");
                int i = nb - 1;
                while (i >= 0 && b[i] == 32u - (uint32_t)(nb - 1 - i)) i--;
                if (i < 0) break;
                b[i]++;
                for (int j = i + 1; j < nb; j++) b[j] = b[j - 1] + 1;
            }
        }
        CHECK(words == 1 + 528 + 40920 + 1107568 + 13884156, "enumerated %ld words", words);
    }
    // random words and lengths: every entry offset, bn cutting the segment at every offset (and
    // not at all), literal bits past bn as they come (random words) and all set
    for (int mode = 0; mode < 3; mode++)
        for (uint32_t seg = 0; seg < 3; seg++) {
            const uint32_t lo = seg * 32;
            for (uint32_t cut = 1; cut <= 33; cut++) {   // bn = lo + cut; 33: the segment is whole
                const uint32_t bn = lo + cut + (cut == 33 ? 40 : 0);
                std::vector<uint8_t> t(bn);
                for (int rep = 0; rep < 40; rep++) {
                    fill(t, mode);
                    uint32_t lw = (uint32_t)rnd64();
                    if (rep % 4 == 1) lw &= (uint32_t)rnd64();   // fewer literals
                    if (rep % 4 == 2) lw |= (uint32_t)rnd64();   // more literals
                    if (rep % 8 == 3 && cut < 32) lw |= ~0u << cut;   // every bit past bn set
                    if (rep % 8 == 7) lw = rep & 8 ? 0u : ~0u;
                    for (uint32_t off = 0; off < 32; off++) {
                        check(lo, lo + off, bn, lw, false, 0, 0, t, "random");
                        // against the segment's current path from another entry: met in a run, at a match, never
                        for (uint32_t o2 = 0; o2 < 32; o2 += 1 + rnd(5)) {
                            uint32_t x;
                            const uint32_t m = path_from(lo, lo + o2, bn, lw, t, x);
                            check(lo, lo + off, bn, lw, true, m, x, t, "merge");
                        }
                        check(lo, lo + off, bn, lw, true, (uint32_t)rnd64(), lo + 32 + rnd(258), t, "merge-random-word");
                        check(lo, lo + off, bn, lw, true, 0u, lo + 32, t, "merge-empty-word");
                    }
                    // an entry at or past the segment end (a long match over the segment) or past bn
                    check(lo, lo + 32 + rnd(227), bn, lw, true, (uint32_t)rnd64(), lo + 40, t, "entry-past");
                    check(lo, bn + rnd(3), bn, lw, false, 0, 0, t, "entry-at-bn");
                }
            }
        }
    CHECK(met_count[MET_NEVER] > 1000 && met_count[MET_LITERAL] > 1000 && met_count[MET_MATCH] > 1000,
          "merge classes: never %ld, in a literal run %ld, at a match %ld", met_count[0], met_count[1], met_count[2]);
    printf("merge classes: never %ld, in a literal run %ld, at a match %ld\n", met_count[0], met_count[1], met_count[2]);
    printf("%ld checks, %d failed checks\n", checks, fails);
    return fails ? 1 : 0;
}

/*
 * ext_rounds_model.cpp -- the first-mismatch arithmetic of the match extension's rounds
 * (csrc/dmx_extbits.h: dmx_first_diff_bit, the text ext_len2 runs per round with v_ffbl_b32 in
 * place of the host's ctz) against a byte loop, under AddressSanitizer + UBSan.  Built by
 * tests/c/Makefile.ext_rounds from this file alone; runs without a GPU.
 * One round as the kernel runs it: W + 1 aligned words per side, realigned by the byte offset
 * of each side (v_alignbyte), xored, and the first differing bit taken as the min over the
 * words of ffbl(x_t) + 32 t, saturating.  Checked for W = 6 and 8 (EXT_W1, EXT_W2), all 16
 * alignments of the two sides, every position of the first differing byte (and none), the
 * differing byte's xor in {0x01, 0x80, 0xFF, random}, and the bytes behind it equal or random.
 * Both sides are heap blocks of exactly the words a round reads, so ASan sees a read behind them.
 * Exit status 0 = "0 failed checks" (the sanitizers abort on their own findings).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dmx_extbits.h"

static int fails;
static long checks;
#define CHECK(c, ...) do { checks++; if (!(c)) { if (fails < 50) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } fails++; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

// v_alignbyte_b32: bytes sh .. sh + 3 of the 8-byte value hi:lo
static uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (sh & 3)));
}
static uint32_t word_at(const uint8_t* p) {   // little-endian aligned word
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// one round at byte offsets sa, sc of two blocks of W + 1 words: equal leading bytes, 4 W = all
template <int W>
static uint32_t round_model(const uint8_t* a, uint32_t sa, const uint8_t* c, uint32_t sc) {
    uint32_t wa[W + 1], wc[W + 1], x[W];
    for (int t = 0; t < W + 1; t++) { wa[t] = word_at(a + 4 * t); wc[t] = word_at(c + 4 * t); }
    for (int t = 0; t < W; t++) x[t] = alignbyte(wa[t + 1], wa[t], sa) ^ alignbyte(wc[t + 1], wc[t], sc);
    const uint32_t m = dmx_first_diff_bit<W>(x);
    return m != 0xFFFFFFFFu ? m >> 3 : 4u * W;
}

template <int W>
static void run() {
    const uint32_t NB = 4 * (W + 1);
    static const uint8_t XORS[4] = {0x01, 0x80, 0xFF, 0};
    for (uint32_t sa = 0; sa < 4; sa++)
        for (uint32_t sc = 0; sc < 4; sc++)
            for (uint32_t p = 0; p <= 4u * W; p++)   // first differing byte; 4 W = none
                for (int xi = 0; xi < 4; xi++)
                    for (int tail = 0; tail < 2; tail++) {
                        std::vector<uint8_t> a(NB), c(NB);   // exact size: W + 1 words per side
                        for (uint32_t k = 0; k < NB; k++) { a[k] = (uint8_t)rnd(256); c[k] = (uint8_t)rnd(256); }
                        for (uint32_t k = 0; k < 4u * W; k++) {
                            if (k < p || (k > p && !tail)) c[sc + k] = a[sa + k];
                            else if (k == p) c[sc + k] = a[sa + k] ^ (XORS[xi] ? XORS[xi] : (uint8_t)(1 + rnd(255)));
                        }
                        uint32_t want = 0;   // the byte loop
                        while (want < 4u * W && a[sa + want] == c[sc + want]) want++;
                        const uint32_t got = round_model<W>(a.data(), sa, c.data(), sc);
                        CHECK(got == want && (p == 4u * W || want == p), "W=%d sa=%u sc=%u p=%u xor=%d tail=%d: %u, byte loop %u",
                              W, sa, sc, p, xi, tail, got, want);
                    }
    // the words alone: one non-zero word at t with its lowest set bit at b, noise above and behind
    for (int t = 0; t < W; t++)
        for (uint32_t b = 0; b < 32; b++) {
            uint32_t x[W];
            for (int u = 0; u < W; u++) x[u] = u < t ? 0u : u == t ? ((rnd(0xFFFFFFFFu) | 1u) << b) : rnd(0xFFFFFFFFu);
            CHECK(dmx_first_diff_bit<W>(x) == 32u * (uint32_t)t + b, "W=%d word %d bit %u", W, t, b);
        }
    uint32_t z[W];
    memset(z, 0, sizeof z);
    CHECK(dmx_first_diff_bit<W>(z) == 0xFFFFFFFFu, "W=%d all equal", W);
}

int main() {
    CHECK(dmx_ffbl(0) == 0xFFFFFFFFu && dmx_ffbl(1) == 0 && dmx_ffbl(0x80000000u) == 31, "ffbl");
    CHECK(dmx_add_sat(0xFFFFFFFFu, 32) == 0xFFFFFFFFu && dmx_add_sat(31, 224) == 255 &&
          dmx_add_sat(0xFFFFFFF0u, 224) == 0xFFFFFFFFu, "add_sat");
    run<6>();
    run<8>();
    printf("%ld checks, %d failed checks\n", checks, fails);
    return fails ? 1 : 0;
}

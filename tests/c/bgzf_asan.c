/*
 * bgzf_asan.c -- dmx_bgzf_index (csrc/dmx_inflate.c, host C) under AddressSanitizer + UBSan.
 * Built by tests/c/Makefile.bgzf from dmx_inflate.c alone (the index walk needs nothing of the
 * HIP layer); runs without a GPU.  For every BGZF file on the command line:
 *   - the whole file indexes (0), twice with the same entries, and with cap one short gives
 *     -E_SZ and the same count;
 *   - every truncation, in a heap copy of exactly that size so that ASan sees any read past
 *     the end, returns 0 (a member boundary) or a negative -E_*;
 *   - single-bit flips of every byte of the first two members' headers and of the last 40
 *     bytes return 0 or -E_*.
 * Also a member whose ISIZE is 40 000 (-E_RANGE), members with other FEXTRA subfields, a
 * subfield whose SLEN runs past XLEN, and BSIZE values that leave no room for the trailer.
 * Exit status 0 = no failed check (the sanitizers abort on their own findings).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dmx.h"

static int fails;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fails++; } } while (0)

/* the call on an exact-size heap copy; entries and CRCs into exact-size arrays too */
static int index_copy(const uint8_t* z, size_t n, uint32_t cap, uint32_t* nblk, uint64_t* total) {
    uint8_t* c = (uint8_t*)malloc(n ? n : 1);
    dmx_iblock* ix = (dmx_iblock*)malloc(cap ? cap * sizeof(dmx_iblock) : 1);
    uint32_t* crc = (uint32_t*)malloc(cap ? cap * sizeof(uint32_t) : 1);
    memcpy(c, z, n);
    const int r = dmx_bgzf_index(c, n, cap ? ix : NULL, cap ? crc : NULL, cap, nblk, total);
    free(c);
    free(ix);
    free(crc);
    return r;
}

/* a member with a stored block of n bytes, XLEN = 6 + nx (extra subfield bytes in front of BC) */
static size_t stored_member(uint8_t* o, const uint8_t* d, uint32_t n, const uint8_t* extra, uint32_t nx, uint32_t isize) {
    static const uint8_t h[10] = {0x1F, 0x8B, 8, 4, 0, 0, 0, 0, 0, 0xFF};
    size_t p = 0;
    memcpy(o, h, 10); p = 10;
    o[p++] = (uint8_t)(6 + nx); o[p++] = (uint8_t)((6 + nx) >> 8);
    if (nx) { memcpy(o + p, extra, nx); p += nx; }
    const size_t size = 12 + 6 + nx + 5 + n + 8;
    o[p++] = 'B'; o[p++] = 'C'; o[p++] = 2; o[p++] = 0;
    o[p++] = (uint8_t)(size - 1); o[p++] = (uint8_t)((size - 1) >> 8);
    o[p++] = 1; o[p++] = (uint8_t)n; o[p++] = (uint8_t)(n >> 8); o[p++] = (uint8_t)~n; o[p++] = (uint8_t)(~n >> 8);
    memcpy(o + p, d, n); p += n;
    for (int k = 0; k < 4; k++) o[p++] = 0;   /* (the CRC is not checked by the index) */
    for (int k = 0; k < 4; k++) o[p++] = (uint8_t)(isize >> (8 * k));
    return p;
}

int main(int argc, char** argv) {
    long calls = 0;
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* z = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);
        if (fread(z, 1, (size_t)n, f) != (size_t)n) return 2;
        fclose(f);
        uint32_t nb = 0, nb2 = 0;
        uint64_t tot = 0, tot2 = 0;
        int r = index_copy(z, (size_t)n, 0, &nb, &tot);
        CHECK(r == (nb ? -E_SZ : 0), "%s: count pass %d", argv[a], r);
        r = index_copy(z, (size_t)n, nb, &nb2, &tot2);
        CHECK(r == 0 && nb2 == nb && tot2 == tot, "%s: index %d", argv[a], r);
        if (nb) {
            r = index_copy(z, (size_t)n, nb - 1, &nb2, &tot2);
            CHECK(r == -E_SZ && nb2 == nb, "%s: cap - 1: %d", argv[a], r);
        }
        /* every truncation up to 70 000 bytes (two members of 32 KiB), then 500 spread over the rest */
        const long tstep = n > 70000 ? (n - 70000) / 500 + 1 : 1;
        for (long t = 0; t < n; t = t < 70000 ? t + 1 : t + tstep) {
            r = index_copy(z, (size_t)t, nb, &nb2, &tot2);
            CHECK(r <= 0, "%s: truncation %ld: %d", argv[a], t, r);
            calls++;
        }
        for (long p = 0; p < n; p++) {
            if (p >= 40 && p < n - 40) continue;
            for (int bit = 0; bit < 8; bit++) {
                z[p] ^= (uint8_t)(1u << bit);
                r = index_copy(z, (size_t)n, nb, &nb2, &tot2);
                CHECK(r <= 0, "%s: flip %ld.%d: %d", argv[a], p, bit, r);
                z[p] ^= (uint8_t)(1u << bit);
                calls++;
            }
        }
        free(z);
    }
    {   /* hand-made members */
        uint8_t d[300], m[1024];
        for (int k = 0; k < 300; k++) d[k] = (uint8_t)(k * 7);
        uint32_t nb = 0;
        uint64_t tot = 0;
        size_t n = stored_member(m, d, 300, NULL, 0, 300);
        CHECK(index_copy(m, n, 4, &nb, &tot) == 0 && nb == 1 && tot == 300, "stored member");
        static const uint8_t ex[7] = {'X', 'Y', 3, 0, 1, 2, 3};
        n = stored_member(m, d, 300, ex, 7, 300);
        dmx_iblock e;
        uint32_t crc = 1;
        CHECK(dmx_bgzf_index(m, n, &e, &crc, 1, &nb, &tot) == 0 && nb == 1 && e.bit == 8 * (18 + 7) && e.out_len == 300 &&
              e.out_off == 0 && crc == 0, "subfield before BC");
        static const uint8_t over[4] = {'X', 'Y', 200, 0};   /* SLEN runs past XLEN: BC is never reached */
        n = stored_member(m, d, 300, over, 4, 300);
        CHECK(index_copy(m, n, 4, &nb, &tot) == -(int)E_ZHEAD, "subfield past XLEN");
        n = stored_member(m, d, 300, NULL, 0, 40000);
        CHECK(index_copy(m, n, 4, &nb, &tot) == -E_RANGE, "ISIZE 40000");
        n = stored_member(m, d, 300, NULL, 0, 0);
        CHECK(index_copy(m, n, 4, &nb, &tot) == 0 && nb == 0 && tot == 0, "empty member");
        n = stored_member(m, d, 300, NULL, 0, 300);
        for (uint32_t bs = 0; bs < 40; bs++) {   /* BSIZE too small for header + trailer, or inside them */
            m[16] = (uint8_t)bs;
            m[17] = 0;
            const int r = index_copy(m, n, 4, &nb, &tot);
            CHECK(r < 0, "BSIZE %u: %d", bs, r);
        }
        CHECK(dmx_bgzf_index(NULL, 0, NULL, NULL, 0, &nb, &tot) == 0 && nb == 0, "empty file");
    }
    printf("bgzf_asan: %ld truncations and flips, %d failed checks\n", calls, fails);
    return fails ? 1 : 0;
}

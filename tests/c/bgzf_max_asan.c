/*
 * bgzf_max_asan.c -- dmx_bgzf_index_max (csrc/dmx_inflate.c, host C) under AddressSanitizer +
 * UBSan, on files whose members hold up to 65 536 bytes.  Built by tests/c/Makefile.bgzf_max from
 * dmx_inflate.c alone; runs without a GPU.  For every BGZF file on the command line, with the
 * bound DMX_BGZF_MAX_ISIZE:
 *   - the whole file indexes (0), twice with the same entries; cap one short gives -E_SZ and the
 *     same count; the bound one below the file's largest ISIZE gives -E_RANGE, the largest ISIZE
 *     itself 0; the bounds 0 and 65 537 give -E_RANGE whatever the file;
 *   - dmx_bgzf_index gives what dmx_bgzf_index_max gives with 32 768;
 *   - truncations, in a heap copy of exactly that size so that ASan sees any read past the end,
 *     return 0 (a member boundary) or a negative -E_*: every one for a file of up to 20 000
 *     bytes, otherwise every one in the 4 096 bytes around each member boundary and 500 spread
 *     over the rest;
 *   - single-bit flips of every byte of every member's 18-byte header and 8-byte trailer return
 *     0 or -E_*, and entries of a call that returns 0 stay inside the bound.
 * Exit status 0 = no failed check (the sanitizers abort on their own findings).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dmx.h"

static int fails;
#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fails++; } } while (0)
#define MAXM 64

/* the call on an exact-size heap copy; entries and CRCs into exact-size arrays too.  Entries of
 * a sound answer lie inside the bound and follow each other in the output. */
static int index_copy(const uint8_t* z, size_t n, uint32_t bound, uint32_t cap, uint32_t* nblk, uint64_t* total) {
    uint8_t* c = (uint8_t*)malloc(n ? n : 1);
    dmx_iblock* ix = (dmx_iblock*)malloc(cap ? cap * sizeof(dmx_iblock) : 1);
    uint32_t* crc = (uint32_t*)malloc(cap ? cap * sizeof(uint32_t) : 1);
    memcpy(c, z, n);
    const int r = dmx_bgzf_index_max(c, n, bound, cap ? ix : NULL, cap ? crc : NULL, cap, nblk, total);
    if (r == 0) {
        uint64_t off = 0;
        for (uint32_t k = 0; k < *nblk && k < cap; k++) {
            CHECK(ix[k].out_len >= 1 && ix[k].out_len <= bound && ix[k].out_off == off && ix[k].bit / 8 < n,
                  "entry %u outside the bound or the file", k);
            off += ix[k].out_len;
        }
        CHECK(off == *total, "total %llu, entries %llu", (unsigned long long)*total, (unsigned long long)off);
    }
    free(c);
    free(ix);
    free(crc);
    return r;
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
        /* the members of the (valid) file by their BSIZE at offset 16, and the largest ISIZE */
        long mo[MAXM + 1];
        int nm = 0;
        uint32_t top = 0;
        for (long p = 0; p + 26 <= n && nm < MAXM;) {
            const long bs = (long)(z[p + 16] | (z[p + 17] << 8)) + 1;
            mo[nm++] = p;
            const uint8_t* t = z + p + bs - 4;
            const uint32_t isz = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
            if (isz > top) top = isz;
            p += bs;
        }
        mo[nm] = n;
        const uint32_t B = DMX_BGZF_MAX_ISIZE;
        uint32_t nb = 0, nb2 = 0;
        uint64_t tot = 0, tot2 = 0;
        int r = index_copy(z, (size_t)n, B, 0, &nb, &tot);
        CHECK(r == (nb ? -E_SZ : 0), "%s: count pass %d", argv[a], r);
        r = index_copy(z, (size_t)n, B, nb, &nb2, &tot2);
        CHECK(r == 0 && nb2 == nb && tot2 == tot, "%s: index %d", argv[a], r);
        if (nb) {
            r = index_copy(z, (size_t)n, B, nb - 1, &nb2, &tot2);
            CHECK(r == -E_SZ && nb2 == nb, "%s: cap - 1: %d", argv[a], r);
        }
        if (top > 1) CHECK(index_copy(z, (size_t)n, top - 1, nb, &nb2, &tot2) == -E_RANGE, "%s: bound %u", argv[a], top - 1);
        if (top) CHECK(index_copy(z, (size_t)n, top, nb, &nb2, &tot2) == 0 && nb2 == nb, "%s: bound %u", argv[a], top);
        CHECK(index_copy(z, (size_t)n, 0, nb, &nb2, &tot2) == -E_RANGE && nb2 == 0, "%s: bound 0", argv[a]);
        CHECK(index_copy(z, (size_t)n, B + 1, nb, &nb2, &tot2) == -E_RANGE && nb2 == 0, "%s: bound 65537", argv[a]);
        {   /* the 32 KiB call is the general one with 32 768 */
            dmx_iblock* x0 = (dmx_iblock*)calloc(nb ? nb : 1, sizeof(dmx_iblock));
            dmx_iblock* x1 = (dmx_iblock*)calloc(nb ? nb : 1, sizeof(dmx_iblock));
            uint32_t n0 = 0, n1 = 0;
            uint64_t t0 = 0, t1 = 0;
            const int r0 = dmx_bgzf_index(z, (uint64_t)n, x0, NULL, nb, &n0, &t0);
            const int r1 = dmx_bgzf_index_max(z, (uint64_t)n, 32768, x1, NULL, nb, &n1, &t1);
            CHECK(r0 == r1 && n0 == n1 && t0 == t1 && memcmp(x0, x1, (nb ? nb : 1) * sizeof(dmx_iblock)) == 0,
                  "%s: dmx_bgzf_index %d, with 32768 %d", argv[a], r0, r1);
            CHECK(r0 == (top > 32768 ? -E_RANGE : 0), "%s: dmx_bgzf_index %d, largest ISIZE %u", argv[a], r0, top);
            free(x0);
            free(x1);
        }
        const long tstep = (n > 20000 ? n / 500 : 0) + 1;
        for (long t = 0; t < n;) {
            r = index_copy(z, (size_t)t, B, nb, &nb2, &tot2);
            CHECK(r <= 0, "%s: truncation %ld: %d", argv[a], t, r);
            calls++;
            long next = t + tstep;
            for (int k = 0; k <= nm; k++)   /* every byte within 2 048 of a member boundary */
                if (t + 1 >= mo[k] - 2048 && t + 1 <= mo[k] + 2048) next = t + 1;
            for (int k = 0; k <= nm; k++)
                if (t < mo[k] - 2048 && next > mo[k] - 2048) next = mo[k] - 2048;
            t = next;
        }
        for (int k = 0; k < nm; k++) {
            for (long p = mo[k]; p < mo[k + 1]; p++) {
                if (p >= mo[k] + 18 && p < mo[k + 1] - 8) continue;
                for (int bit = 0; bit < 8; bit++) {
                    z[p] ^= (uint8_t)(1u << bit);
                    r = index_copy(z, (size_t)n, B, nb, &nb2, &tot2);
                    CHECK(r <= 0, "%s: flip %ld.%d: %d", argv[a], p, bit, r);
                    z[p] ^= (uint8_t)(1u << bit);
                    calls++;
                }
            }
        }
        free(z);
    }
    uint32_t nb = 1;
    uint64_t tot = 1;
    CHECK(dmx_bgzf_index_max(NULL, 0, DMX_BGZF_MAX_ISIZE, NULL, NULL, 0, &nb, &tot) == 0 && nb == 0 && tot == 0, "empty file");
    printf("bgzf_max_asan: %ld truncations and flips, %d failed checks\n", calls, fails);
    return fails ? 1 : 0;
}

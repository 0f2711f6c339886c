/*
 * bgzf_dindex_model.cpp -- the host twin of the device BGZF index (csrc/dmx_bgzf_index.hip) under
 * AddressSanitizer + UBSan.  Built by tests/c/Makefile.bgzf_dindex from this file and dmx_inflate.c;
 * runs without a GPU.  It includes csrc/dmx_bgzf_step.h -- the text every kernel thread runs -- and
 * runs the stages as plain loops over the kernels' own data layout (tiles of aligned 16-byte groups
 * counted, scanned and written; candidates, links, rounds of marked-prefix doubling with two node
 * buffers, finish), then compares the record, the entries and the CRC words with
 * dmx_bgzf_index_max's, byte for byte over the whole output arrays (so also what an erring walk
 * wrote before it stopped).  For every sound BGZF file on the command line:
 *   - the whole file under the bounds 65 536, 32 768 and one below its largest ISIZE, with cap
 *     ample, 0 and 2, at the alignments 0, 1 and 15 of its first byte, and with a work buffer of
 *     4 candidates (the overflow answer);
 *   - every truncation, the bytes behind the cut poisoned so that ASan sees any read of them;
 *   - every single-bit flip of every byte of every member's header and trailer (the bounds 65 536
 *     and 32 768 by turns, member by member).
 * Exit status 0 = "0 failed checks" (the sanitizers abort on their own findings).
 */
#include <sanitizer/asan_interface.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dmx.h"
#include "dmx_bgzf_step.h"

static int fails;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 50) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } fails++; } } while (0)

static const uint32_t TILE_GROUPS = 1024;   // as BIX_TILE_GROUPS

// the five words the scan kernel holds for group g: bytes outside the file read as 0 here (the
// kernel loads them and never looks at them)
static void group_words(const uint8_t* z, uint64_t zlen, uint32_t head, uint64_t g, uint32_t w[5]) {
    if (g * 16 >= head && g * 16 - head + 20 <= zlen) {   // all 20 bytes in the file
        for (int k = 0; k < 5; k++) __builtin_memcpy(&w[k], z + (g * 16 - head) + 4 * k, 4);   // (checked inline)
        return;
    }
    for (int k = 0; k < 5; k++) w[k] = 0;
    for (uint32_t b = 0; b < 20; b++) {
        const uint64_t a = g * 16 + b;
        if (a < head || a - head >= zlen) continue;
        w[b / 4] |= (uint32_t)z[a - head] << (8 * (b & 3));
    }
}

struct Work {
    std::vector<uint32_t> tile;
    std::vector<dmx_bgzf_cand> cand;
    std::vector<dmx_bgzf_node> na, nb;
    std::vector<dmx_bgzf_mark> mark;
};

// dmx_bgzf_index_async as loops: the same launches in the same order
static void model(const uint8_t* z, uint64_t zlen, uint32_t head, uint32_t max_isize, dmx_iblock* idx, uint32_t* crc,
                  uint32_t cap, uint32_t max_cand, Work& W, dmx_bgzf_istat* st) {
    const uint64_t ngroups = zlen ? (head + zlen + 15) / 16 : 0;
    const uint64_t ntiles = ngroups ? (ngroups + TILE_GROUPS - 1) / TILE_GROUPS : 1;
    W.tile.assign(ntiles + 1, 0);
    uint32_t w[5];
    // count
    for (uint64_t g = 0; g < ngroups; g++) {
        group_words(z, zlen, head, g, w);
        W.tile[g / TILE_GROUPS] += dmx_bgzf_group(z, zlen, max_isize, head, g, w, nullptr, 0);
    }
    // plan
    uint32_t run = 0;
    for (uint64_t t = 0; t < ntiles; t++) {
        const uint32_t c = W.tile[t];
        W.tile[t] = run;
        run += c;
    }
    W.tile[ntiles] = run;
    const uint32_t total = run;
    dmx_bgzf_istat r = {0, 0, 0, total, 0};
    uint32_t n = total;
    dmx_bgzf_member m;
    const int e0 = zlen ? dmx_bgzf_step(z, zlen, 0, max_isize, &m) : 0;
    if (e0) {
        r.status = e0;
        n = 0;
    } else if (total > max_cand) {
        r.status = -(int)E_SZ;
        n = 0;
    }
    *st = r;
    if (!n) return;
    // write
    W.cand.assign(n + 1, dmx_bgzf_cand());
    for (uint64_t t = 0; t < ntiles; t++) {
        uint32_t at = W.tile[t];
        const uint32_t end = W.tile[t + 1];
        if (at == end) continue;
        for (uint64_t g = t * TILE_GROUPS; g < (t + 1) * TILE_GROUPS && g < ngroups; g++) {
            group_words(z, zlen, head, g, w);
            if (at < end) at += dmx_bgzf_group(z, zlen, max_isize, head, g, w, &W.cand[at], end - at);
        }
        CHECK(at == end, "tile %llu: wrote %u of %u", (unsigned long long)t, at, end);
    }
    for (uint32_t i = 1; i < n; i++) CHECK(W.cand[i - 1].off < W.cand[i].off, "candidates out of order at %u", i);
    // link
    W.na.assign(n + 1, dmx_bgzf_node());
    W.nb.assign(n + 1, dmx_bgzf_node());
    W.mark.assign(n + 1, dmx_bgzf_mark());
    for (uint32_t i = 0; i <= n; i++) dmx_bgzf_link(z, zlen, max_isize, W.cand.data(), n, i, W.na.data(), W.mark.data());
    // rounds: as many as the launches, from the bound and never from n
    const uint64_t bound = max_cand < zlen / 26 + 1 ? max_cand : zlen / 26 + 1;
    uint32_t rounds = 0;
    while ((1ull << rounds) < bound + 1) rounds++;
    dmx_bgzf_node *a = W.na.data(), *b = W.nb.data();
    for (uint32_t k = 0; k < rounds; k++) {
        // the threads of a launch run in any order: forwards in even rounds, backwards in odd ones
        for (uint32_t i = 0; i <= n; i++) dmx_bgzf_round(a, b, W.mark.data(), n, (k & 1) ? n - i : i, k);
        dmx_bgzf_node* t = a;
        a = b;
        b = t;
    }
    // finish
    for (uint32_t i = 0; i < n; i++) dmx_bgzf_finish(W.cand.data(), W.mark.data(), n, i, zlen, idx, crc, cap, st);
}

static Work g_work;
static long g_runs;

// one comparison: z[0..zlen) must be readable and nothing behind it
static void compare(const char* what, long arg, const uint8_t* z, uint64_t zlen, uint32_t head, uint32_t max_isize,
                    uint32_t cap, uint32_t max_cand) {
    std::vector<dmx_iblock> ih(cap + 1), im(cap + 1);
    std::vector<uint32_t> ch(cap + 1), cm(cap + 1);
    memset(ih.data(), 0xEE, ih.size() * sizeof(dmx_iblock));
    memset(im.data(), 0xEE, im.size() * sizeof(dmx_iblock));
    memset(ch.data(), 0xEE, ch.size() * 4);
    memset(cm.data(), 0xEE, cm.size() * 4);
    uint32_t nb = 0;
    uint64_t tot = 0;
    const int r = dmx_bgzf_index_max(z, zlen, max_isize, ih.data(), ch.data(), cap, &nb, &tot);
    dmx_bgzf_istat st = {1, 1, 1, 1, 1};
    model(z, zlen, head, max_isize, im.data(), cm.data(), cap, max_cand, g_work, &st);
    g_runs++;
    if (st.status == -(int)E_SZ && st.nblk == 0 && st.ncand > max_cand) {   // the documented difference
        CHECK(st.out_len == 0, "%s %ld: overflow record", what, arg);
        return;
    }
    CHECK(st.status == r && st.nblk == nb && st.out_len == tot && st.reserved == 0,
          "%s %ld (head %u, bound %u, cap %u): model %d %u %llu, walk %d %u %llu", what, arg, head, max_isize, cap, st.status,
          st.nblk, (unsigned long long)st.out_len, r, nb, (unsigned long long)tot);
    CHECK(memcmp(ih.data(), im.data(), ih.size() * sizeof(dmx_iblock)) == 0, "%s %ld (head %u, bound %u, cap %u): entries differ",
          what, arg, head, max_isize, cap);
    CHECK(memcmp(ch.data(), cm.data(), ch.size() * 4) == 0, "%s %ld (head %u, bound %u, cap %u): CRC words differ", what, arg,
          head, max_isize, cap);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* z = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);
        if (fread(z, 1, (size_t)n, f) != (size_t)n) return 2;
        fclose(f);
        // the members of the (sound) file, and its largest ISIZE
        std::vector<long> mo;
        uint32_t top = 0, full = 0;
        for (uint64_t p = 0; p < (uint64_t)n;) {
            dmx_bgzf_member m;
            if (dmx_bgzf_step(z, (uint64_t)n, p, DMX_BGZF_MAX_ISIZE, &m)) { fprintf(stderr, "%s is not a sound BGZF file\n", argv[a]); return 2; }
            mo.push_back((long)p);
            if (m.isize > top) top = m.isize;
            full += m.isize ? 1 : 0;
            p += m.bsize;
        }
        mo.push_back(n);
        const uint32_t many = (uint32_t)n / 3 + 2;
        const uint32_t bounds[3] = {DMX_BGZF_MAX_ISIZE, 32768, top > 1 ? top - 1 : 1};
        const uint32_t caps[3] = {full + 3, 0, 2};
        const uint32_t heads[3] = {0, 1, 15};
        for (uint32_t bound : bounds)
            for (uint32_t cap : caps)
                for (uint32_t head : heads) compare(argv[a], -1, z, (uint64_t)n, head, bound, cap, many);
        compare(argv[a], -2, z, (uint64_t)n, 0, DMX_BGZF_MAX_ISIZE, full + 3, 4);
        {   // with room for 4 a file of more candidates overflows, and reports how many
            dmx_bgzf_istat st;
            model(z, (uint64_t)n, 0, DMX_BGZF_MAX_ISIZE, nullptr, nullptr, 0, 4, g_work, &st);
            if (mo.size() - 1 > 4)
                CHECK(st.status == -(int)E_SZ && st.nblk == 0 && st.out_len == 0 && st.ncand >= mo.size() - 1, "%s: overflow %d %u",
                      argv[a], st.status, st.ncand);
        }
        // every truncation, longest first: the bytes behind the cut are poisoned
        for (long t = n - 1; t >= 0; t--) {
            ASAN_POISON_MEMORY_REGION(z + t, (size_t)(n - t));
            compare("truncation", t, z, (uint64_t)t, (uint32_t)(t % 3 == 0 ? 0 : t % 16), DMX_BGZF_MAX_ISIZE, full + 3, many);
        }
        ASAN_UNPOISON_MEMORY_REGION(z, (size_t)n);
        // every single-bit flip of the members' headers and trailers
        for (size_t k = 0; k + 1 < mo.size(); k++) {
            for (long p = mo[k]; p < mo[k + 1]; p++) {
                if (p >= mo[k] + 18 && p < mo[k + 1] - 8) continue;
                for (int bit = 0; bit < 8; bit++) {
                    z[p] ^= (uint8_t)(1u << bit);
                    compare("flip", p * 8 + bit, z, (uint64_t)n, 0, (k & 1) ? 32768 : DMX_BGZF_MAX_ISIZE, full + 3, many);
                    z[p] ^= (uint8_t)(1u << bit);
                }
            }
        }
        free(z);
    }
    compare("empty", 0, (const uint8_t*)"", 0, 0, DMX_BGZF_MAX_ISIZE, 1, 4);
    printf("bgzf_dindex_model: %ld comparisons, %d failed checks\n", g_runs, fails);
    return fails ? 1 : 0;
}

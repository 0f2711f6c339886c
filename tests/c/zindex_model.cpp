/*
 * zindex_model.cpp -- the seek-point builder dmx_zindex_build_host (csrc/dmx_inflate.c) under
 * AddressSanitizer + UBSan.  Built by tests/c/Makefile.zindex from this file and dmx_inflate.c
 * alone; runs without a GPU.  The arguments are files that each hold one stream (zlib, gzip or raw:
 * a name with "raw" in it is raw).  For every stream and the spans 1, 4 096, 65 536 and the default:
 *   - the builder's status is deflate_decompress's (dmx_inflate_dict_host's for a raw stream), and a
 *     refused stream leaves no index;
 *   - the points follow one another in the stream and tile the output, every point but the last
 *     holds span bytes, the record names the stream's length, input and check value;
 *   - every point is decoded again here from its window slot alone, by a plain restatement of
 *     RFC 1951 (a reader that takes one bit at a time, the canonical walk by counts): it must end
 *     exactly at end_bit on a block boundary and give the bytes the whole decode gave, whose
 *     Adler-32 is the point's; the slot is the output in front of the point, right-aligned, zeros
 *     before it.
 * The first two streams are also indexed at every cut point (every prefix, an exact-size heap block,
 * so ASan sees a read behind it) and under 10 000 seeded mutations of one to three bytes.
 * Exit status 0 = "0 failed checks" (the sanitizers abort on their own findings).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dmx.h"

static int fails;
static long checks, nindexes, npoints_again;
#define CHECK(c, ...) do { checks++; if (!(c)) { if (fails < 50) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } fails++; } } while (0)

typedef std::vector<uint8_t> bytes;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

static uint32_t adler_plain(const uint8_t* d, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; i++) {
        a = (a + d[i]) % 65521u;
        b = (b + a) % 65521u;
    }
    return (b << 16) | a;
}

// ---- the plain restatement: bits [pos, end) of z, one at a time; out begins with the window ----
struct RB {
    const uint8_t* z;
    uint64_t pos, end;
    bool bad;
};
static uint32_t rbits(RB& r, int k) {
    uint32_t v = 0;
    for (int i = 0; i < k; i++, r.pos++) {
        if (r.pos >= r.end) { r.bad = true; return 0; }
        v |= (uint32_t)((r.z[r.pos >> 3] >> (r.pos & 7)) & 1) << i;
    }
    return v;
}
struct Code {
    int count[16];
    int sym[320];
};
static void code_build(Code& c, const uint8_t* len, int n) {
    memset(c.count, 0, sizeof(c.count));
    for (int s = 0; s < n; s++) c.count[len[s]]++;
    c.count[0] = 0;
    int offs[16] = {0};
    for (int l = 1; l < 15; l++) offs[l + 1] = offs[l] + c.count[l];
    for (int s = 0; s < n; s++)
        if (len[s]) c.sym[offs[len[s]]++] = s;
}
static int code_read(RB& r, const Code& c) {   // puff's loop
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; l++) {
        code |= (int)rbits(r, 1);
        if (r.bad) return -1;
        if (code - c.count[l] < first) return c.sym[index + (code - first)];
        index += c.count[l];
        first += c.count[l];
        first <<= 1;
        code <<= 1;
    }
    r.bad = true;
    return -1;
}
// the blocks of bits [bit, end) appended to out (which holds the window); true iff they end at `end`
static bool plain_point(const uint8_t* z, uint64_t bit, uint64_t end, bytes& out, bool want_final) {
    static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    RB r = {z, bit, end, false};
    bool final = false;
    while (r.pos < end) {
        if (final) return false;   // blocks behind BFINAL
        final = rbits(r, 1) != 0;
        const uint32_t type = rbits(r, 2);
        if (r.bad || type == 3) return false;
        if (type == 0) {
            r.pos = (r.pos + 7) & ~7ull;   // the padding is counted in the stream's own bytes
            const uint32_t len = rbits(r, 16), nlen = rbits(r, 16);
            if (r.bad || len != (~nlen & 0xFFFFu)) return false;
            for (uint32_t i = 0; i < len; i++) {
                const uint32_t c = rbits(r, 8);
                if (r.bad) return false;
                out.push_back((uint8_t)c);
            }
            continue;
        }
        uint8_t len[320];
        int nl = 288, nd = 30;
        if (type == 1) {
            for (int k = 0; k < 288; k++) len[k] = (uint8_t)(k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : 8);
            for (int k = 0; k < 30; k++) len[288 + k] = 5;
        } else {
            nl = (int)rbits(r, 5) + 257;
            nd = (int)rbits(r, 5) + 1;
            const int nc = (int)rbits(r, 4) + 4;
            if (r.bad || nl > 286 || nd > 30) return false;
            uint8_t cl[19] = {0};
            for (int k = 0; k < nc; k++) cl[order[k]] = (uint8_t)rbits(r, 3);
            if (r.bad) return false;
            Code cc;
            code_build(cc, cl, 19);
            int idx = 0;
            while (idx < nl + nd) {
                const int s = code_read(r, cc);
                if (s < 0) return false;
                if (s < 16) { len[idx++] = (uint8_t)s; continue; }
                int v = 0, rep;
                if (s == 16) {
                    if (!idx) return false;
                    v = len[idx - 1];
                    rep = 3 + (int)rbits(r, 2);
                } else if (s == 17) {
                    rep = 3 + (int)rbits(r, 3);
                } else {
                    rep = 11 + (int)rbits(r, 7);
                }
                if (r.bad || idx + rep > nl + nd) return false;
                while (rep--) len[idx++] = (uint8_t)v;
            }
        }
        Code lc, dc;
        code_build(lc, len, nl);
        code_build(dc, len + nl, nd);
        for (;;) {
            int s = code_read(r, lc);
            if (s < 0) return false;
            if (s < 256) { out.push_back((uint8_t)s); continue; }
            if (s == 256) break;
            s -= 257;
            if (s >= 29) return false;
            const uint32_t l = lbase[s] + rbits(r, lext[s]);
            const int ds = code_read(r, dc);
            if (ds < 0 || ds >= 30) return false;
            const uint32_t dist = dbase[ds] + rbits(r, dext[ds]);
            if (r.bad || dist > out.size()) return false;
            for (uint32_t i = 0; i < l; i++) out.push_back(out[out.size() - dist]);
        }
    }
    return !r.bad && r.pos == end && final == want_final;
}

// the host's whole decode of z under fmt: status, and the bytes and in_used where it is 0
static int whole(const bytes& z, uint32_t fmt, bytes& data, uint64_t* used) {
    void* o = NULL;
    uint64_t on = 0;
    *used = 0;
    // (an exact-size copy: a read behind the stream is a heap overflow)
    uint8_t* zz = (uint8_t*)malloc(z.size() ? z.size() : 1);
    if (z.size()) memcpy(zz, z.data(), z.size());
    int r;
    if (fmt != DMX_BATCH_AUTO) {   // an explicit framing: the host's one-stream decode without a dictionary
        r = dmx_inflate_dict_host(zz, z.size(), fmt, NULL, 0, &o, &on, used);
    } else {
        struct string_len in = {zz, z.size()}, out = {NULL, 0};
        r = deflate_decompress(&out, &in, 0);
        o = out.str;
        on = out.len;
    }
    data.assign((uint8_t*)o, (uint8_t*)o + (r ? 0 : on));
    if (!r) free(o);
    free(zz);
    return r;
}

static void one(const char* name, const bytes& z, uint32_t fmt, uint32_t span, bool again) {
    bytes data;
    uint64_t used = 0;
    const int want = whole(z, fmt, data, &used);
    uint8_t* zz = (uint8_t*)malloc(z.size() ? z.size() : 1);
    if (z.size()) memcpy(zz, z.data(), z.size());
    dmx_zpoint* pts = (dmx_zpoint*)1;
    uint32_t* adl = (uint32_t*)1;
    uint8_t* win = (uint8_t*)1;
    dmx_zindex_status st;
    const int r = dmx_zindex_build_host(zz, z.size(), fmt, span, &pts, &adl, &win, &st);
    CHECK(r == 0, "%s span %u: the call returned %d", name, span, r);
    if (r) { free(zz); return; }
    CHECK(st.status == want, "%s span %u: status %d, the whole decode's %d", name, span, st.status, want);
    CHECK(st.span == (span ? span : DMX_ZINDEX_DEF_SPAN), "%s: span %u recorded as %u", name, span, st.span);
    if (st.status) {
        CHECK(!pts && !adl && !win && !st.npoints && !st.out_len && !st.in_used && !st.check, "%s span %u: an index beside status %d",
              name, span, st.status);
        free(zz);
        return;
    }
    nindexes++;
    CHECK(st.out_len == data.size(), "%s: out_len %llu of %zu", name, (unsigned long long)st.out_len, data.size());
    if (fmt != DMX_BATCH_AUTO) CHECK(st.in_used == used, "%s: in_used %llu", name, (unsigned long long)st.in_used);
    CHECK(st.in_used <= z.size(), "%s: in_used %llu of %zu", name, (unsigned long long)st.in_used, z.size());
    CHECK(st.npoints >= 1 && pts && adl && win, "%s: no points", name);
    uint64_t off = 0;
    for (uint32_t k = 0; k < st.npoints && st.out_len == data.size(); k++) {
        const dmx_zpoint p = pts[k];
        CHECK(p.out_off == off && p.end_bit > p.bit && p.end_bit <= 8 * st.in_used, "%s: point %u is {%llu, %llu, %llu, %llu}", name, k,
              (unsigned long long)p.bit, (unsigned long long)p.end_bit, (unsigned long long)p.out_off, (unsigned long long)p.out_len);
        if (k + 1 < st.npoints) {
            CHECK(pts[k + 1].bit == p.end_bit, "%s: point %u does not end where %u begins", name, k, k + 1);
            CHECK(p.out_len >= st.span, "%s: point %u holds %llu of span %u", name, k, (unsigned long long)p.out_len, st.span);
        }
        if (p.out_off + p.out_len > data.size() || p.out_off != off) break;
        CHECK(adl[k] == adler_plain(data.data() + p.out_off, p.out_len), "%s: Adler-32 of point %u", name, k);
        const size_t wlen = p.out_off < DMX_ZINDEX_WINDOW ? (size_t)p.out_off : DMX_ZINDEX_WINDOW;
        const uint8_t* slot = win + (size_t)k * DMX_ZINDEX_WINDOW;
        bool zeros = true;
        for (size_t i = 0; i < DMX_ZINDEX_WINDOW - wlen; i++) zeros = zeros && slot[i] == 0;
        CHECK(zeros && (!wlen || !memcmp(slot + (DMX_ZINDEX_WINDOW - wlen), data.data() + (p.out_off - wlen), wlen)),
              "%s: window of point %u", name, k);
        if (again) {
            bytes out(slot + (DMX_ZINDEX_WINDOW - wlen), slot + DMX_ZINDEX_WINDOW);
            const bool ok = plain_point(zz, p.bit, p.end_bit, out, k + 1 == st.npoints);
            CHECK(ok && out.size() == wlen + p.out_len && (!p.out_len || !memcmp(out.data() + wlen, data.data() + p.out_off, p.out_len)),
                  "%s span %u: point %u decoded again from its window: %d, %zu bytes of %llu", name, span, k, (int)ok, out.size() - wlen,
                  (unsigned long long)p.out_len);
            npoints_again++;
        }
        off += p.out_len;
    }
    CHECK(off == st.out_len, "%s: the points hold %llu of %llu bytes", name, (unsigned long long)off, (unsigned long long)st.out_len);
    free(pts);
    free(adl);
    free(win);
    free(zz);
}

int main(int argc, char** argv) {
    std::vector<bytes> files;
    std::vector<uint32_t> fmts;
    static const uint32_t spans[4] = {1, 4096, 65536, 0};
    for (int a = 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        bytes z;
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) z.insert(z.end(), buf, buf + n);
        fclose(f);
        const uint32_t fmt = strstr(argv[a], "raw") ? DMX_BATCH_RAW : DMX_BATCH_AUTO;
        files.push_back(z);
        fmts.push_back(fmt);
        for (uint32_t span : spans) one(argv[a], z, fmt, span, true);
        // bytes behind the trailer are ignored
        bytes junk = z;
        junk.insert(junk.end(), 9, 0xA5);
        one(argv[a], junk, fmt, 4096, false);
    }
    for (size_t a = 0; a < files.size() && a < 2; a++) {
        const bytes& z = files[a];
        for (size_t cut = 0; cut <= z.size(); cut++) {
            bytes c(z.begin(), z.begin() + cut);
            one("cut", c, fmts[a], 1, true);
            if (fmts[a] == DMX_BATCH_AUTO) one("cut-as-gzip", c, DMX_BATCH_GZIP, 1, false);
        }
        for (int m = 0; m < 5000; m++) {
            bytes c = z;
            const int nmut = 1 + (int)rnd(3);
            for (int q = 0; q < nmut; q++) c[rnd((uint32_t)c.size())] ^= (uint8_t)(1u << rnd(8));
            one("mutation", c, fmts[a], m & 1 ? 1 : 300, true);
        }
    }
    printf("%ld indexes, %ld points decoded again\n", nindexes, npoints_again);
    printf("%ld checks, %d failed checks\n", checks, fails);
    return fails ? 1 : 0;
}

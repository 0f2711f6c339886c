/*
 * frame_dict_model.cpp -- the host twin of the framing that dmx_inflate_batch_dict_async runs per
 * stream (dmx_frame_head_dict, csrc/dmx_gz_head.h) under AddressSanitizer + UBSan.  Built by
 * tests/c/Makefile.frame_dict from this file and dmx_inflate.c; runs without a GPU.  The verdict of
 * dmx_frame_head_dict is compared with dmx_inflate_dict_host on the same bytes and dictionary:
 *   - a verdict other than 0 is the host's status;
 *   - a verdict of 0 names a format, the offset of the DEFLATE data and whether the window is
 *     primed: the bytes from that offset on, decoded raw with the dictionary exactly when primed,
 *     must give the bytes the host gives the whole input, or the host's status (a trailer's status
 *     aside, which a raw decode does not have).
 * Inputs: a zlib stream with FDICT whose first token is a match that reaches the dictionary's first
 * byte, the same data raw, a zlib stream without FDICT and a gzip member; each with no dictionary,
 * the right one, a wrong one and an empty one, under all four formats; whole, at every cut point, and
 * 6 000 seeded mutations of the first eight bytes, a third of them cut as well.  Every input and
 * every dictionary is a heap block of its exact size, so ASan sees a read behind it.
 * Exit status 0 = "0 failed checks" (the sanitizers abort on their own findings).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dmx.h"
#include "dmx_crc.h"
#include "dmx_gz_head.h"

static int fails;
static long checks;
#define CHECK(c, ...) do { checks++; if (!(c)) { if (fails < 50) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } fails++; } } while (0)

typedef std::vector<uint8_t> bytes;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) % n);
}

static uint32_t adler(const bytes& d) {
    uint32_t a = 1, b = 0;
    for (uint8_t c : d) { a = (a + c) % 65521u; b = (b + a) % 65521u; }
    return (b << 16) | a;
}
static void be32(bytes& b, uint32_t v) { for (int k = 3; k >= 0; k--) b.push_back((uint8_t)(v >> (8 * k))); }
static void le32(bytes& b, uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k))); }

// a fixed-code block (final): a match of 10 bytes at distance `dist`, the literals "abc", end of block
struct Bits {
    bytes b;
    uint32_t acc = 0, n = 0;
    void put(uint32_t v, uint32_t k) {   // k bits of v, least significant first
        for (uint32_t i = 0; i < k; i++) {
            acc |= ((v >> i) & 1u) << n;
            if (++n == 8) { b.push_back((uint8_t)acc); acc = 0; n = 0; }
        }
    }
    void code(uint32_t c, uint32_t k) {   // a Huffman code, most significant bit first
        for (uint32_t i = 0; i < k; i++) put((c >> (k - 1 - i)) & 1u, 1);
    }
    bytes done() { if (n) b.push_back((uint8_t)acc); return b; }
};
static bytes match_block(uint32_t dist) {
    Bits w;
    w.put(1, 1);
    w.put(1, 2);
    w.code(264 - 256, 7);   // length 10
    uint32_t ds = 0, base = 1, extra = 0;
    for (uint32_t s = 0; s < 30; s++) {   // the distance symbol of dist
        const uint32_t x = s < 4 ? 0 : (s - 2) >> 1, bs = s < 4 ? s + 1 : ((2 + (s & 1)) << x) + 1;
        if (bs <= dist) { ds = s; base = bs; extra = x; }
    }
    w.code(ds, 5);
    w.put(dist - base, extra);
    for (const char* c = "abc"; *c; c++) w.code(0x30 + (uint8_t)*c, 8);
    w.code(0, 7);
    return w.done();
}
static bytes stored(const bytes& d) {
    bytes b = {1, (uint8_t)d.size(), (uint8_t)(d.size() >> 8), (uint8_t)~d.size(), (uint8_t)(~d.size() >> 8)};
    b.insert(b.end(), d.begin(), d.end());
    return b;
}

struct Dict { bool have; bytes d; };

// dmx_inflate_dict_host on exact-size heap copies
static int host(const uint8_t* p, size_t n, uint32_t fmt, const Dict& dc, bytes* out, uint64_t* used) {
    uint8_t* c = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(c, p, n);
    uint8_t* dd = dc.have ? (uint8_t*)malloc(dc.d.size() ? dc.d.size() : 1) : NULL;
    if (dd && dc.d.size()) memcpy(dd, dc.d.data(), dc.d.size());
    void* o = NULL;
    uint64_t on = 0, u = 0;
    const int r = dmx_inflate_dict_host(c, n, fmt, dd, dc.have ? dc.d.size() : 0, &o, &on, &u);
    if (out) out->assign((uint8_t*)o, (uint8_t*)o + (r == 0 ? on : 0));
    if (used) *used = u;
    CHECK(r == 0 || (o == NULL && on == 0 && u == 0), "a failed host decode left %p %llu %llu", o, (unsigned long long)on,
          (unsigned long long)u);
    free(o);
    free(dd);
    free(c);
    return r;
}

static void check_one(const uint8_t* src, size_t n, uint32_t fmt, const Dict& dc, const char* what, long id) {
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);   // exact size: a read at or behind p + n is ASan's
    if (n) memcpy(p, src, n);
    uint32_t format = 99;
    uint64_t body = ~0ull;
    bool primed = false;
    const int v = dmx_frame_head_dict(p, n, fmt, dc.have, adler(dc.d), &format, &body, &primed);
    bytes want;
    uint64_t used = 0;
    const int h = host(p, n, fmt, dc, &want, &used);
    const bool magic = n >= 2 && p[0] == 0x1F && p[1] == 0x8B;
    const uint32_t f = fmt != DMX_BATCH_AUTO ? fmt : magic ? DMX_BATCH_GZIP : DMX_BATCH_ZLIB;
    CHECK(format == f, "%s %ld fmt %u: format %u", what, id, fmt, format);
    if (v != 0) {
        CHECK(v == h, "%s %ld fmt %u: verdict %d, host %d", what, id, fmt, v, h);
        CHECK(!primed, "%s %ld fmt %u: primed with verdict %d", what, id, fmt, v);
    } else {
        CHECK(body <= n, "%s %ld fmt %u: body %llu of %zu", what, id, fmt, (unsigned long long)body, n);
        if (f == DMX_BATCH_RAW) CHECK(body == 0 && primed == dc.have, "%s %ld: raw body %llu primed %d", what, id, (unsigned long long)body, primed);
        if (f == DMX_BATCH_ZLIB) CHECK(body == (primed ? 6u : 2u) && (primed == ((p[1] & 0x20) != 0)), "%s %ld: zlib body %llu primed %d", what, id, (unsigned long long)body, primed);
        if (f == DMX_BATCH_GZIP) CHECK(!primed && body >= 10, "%s %ld: gzip body %llu primed %d", what, id, (unsigned long long)body, primed);
        if (body <= n) {
            const Dict none = {false, {}};
            bytes got;
            uint64_t u2 = 0;
            const int h2 = host(p + body, n - body, DMX_BATCH_RAW, primed ? dc : none, &got, &u2);
            const bool trailer = f != DMX_BATCH_RAW && h2 == 0 && (h == -(int)E_ZADL32 || h == -(int)E_CRC || h == -(int)E_LEN);
            CHECK(trailer || (h2 == h && got == want), "%s %ld fmt %u: from body %llu the host says %d, on the whole %d", what,
                  id, fmt, (unsigned long long)body, h2, h);
            if (h == 0)
                CHECK(used == body + u2 + (f == DMX_BATCH_ZLIB ? 4u : f == DMX_BATCH_GZIP ? 8u : 0u), "%s %ld fmt %u: in_used %llu",
                      what, id, fmt, (unsigned long long)used);
        }
    }
    free(p);
}

int main(void) {
    bytes dict;
    for (int k = 0; k < 300; k++) dict.push_back((uint8_t)(k * 31 + (k >> 3)));
    bytes wrong = dict;
    wrong[7] ^= 1;
    const Dict dicts[4] = {{false, {}}, {true, dict}, {true, wrong}, {true, {}}};
    bytes data(dict.begin(), dict.begin() + 10);   // what the match block decodes to with `dict`
    data.push_back('a'); data.push_back('b'); data.push_back('c');
    const bytes raw = match_block((uint32_t)dict.size());

    bytes zf = {0x78, 0xBB};   // FDICT
    be32(zf, adler(dict));
    zf.insert(zf.end(), raw.begin(), raw.end());
    be32(zf, adler(data));
    bytes zp = {0x78, 0x9C};   // no FDICT
    { const bytes s = stored(data); zp.insert(zp.end(), s.begin(), s.end()); }
    be32(zp, adler(data));
    bytes gz = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3};
    { const bytes s = stored(data); gz.insert(gz.end(), s.begin(), s.end()); }
    le32(gz, dmx_crc32_host(0, data.data(), data.size()));
    le32(gz, (uint32_t)data.size());
    const std::vector<bytes> pool = {zf, raw, zp, gz};

    // the sound cases, by hand
    {
        bytes out;
        uint64_t used = 0;
        CHECK(host(zf.data(), zf.size(), DMX_BATCH_AUTO, dicts[1], &out, &used) == 0 && out == data && used == zf.size(), "FDICT with its dictionary");
        CHECK(host(zf.data(), zf.size(), DMX_BATCH_ZLIB, dicts[0], &out, &used) == -(int)E_ZPDICT, "FDICT without a dictionary");
        CHECK(host(zf.data(), zf.size(), DMX_BATCH_ZLIB, dicts[2], &out, &used) == -(int)E_ZPDICT, "FDICT with a wrong dictionary");
        CHECK(host(zf.data(), zf.size(), DMX_BATCH_ZLIB, dicts[3], &out, &used) == -(int)E_ZPDICT, "FDICT with an empty dictionary");
        for (size_t k = 2; k < 6; k++)
            for (int d = 0; d < 4; d++)
                CHECK(host(zf.data(), k, DMX_BATCH_ZLIB, dicts[d], &out, &used) == -(int)E_ZHEAD, "FDICT cut at %zu", k);
        CHECK(host(raw.data(), raw.size(), DMX_BATCH_RAW, dicts[1], &out, &used) == 0 && out == data && used == raw.size(), "raw with the dictionary");
        CHECK(host(raw.data(), raw.size(), DMX_BATCH_RAW, dicts[0], &out, &used) == -(int)E_HUFDIS, "raw without");
        CHECK(host(raw.data(), raw.size(), DMX_BATCH_RAW, dicts[3], &out, &used) == -(int)E_HUFDIS, "raw with an empty one");
        CHECK(host(zp.data(), zp.size(), DMX_BATCH_AUTO, dicts[1], &out, &used) == 0 && out == data && used == zp.size(), "no FDICT: the dictionary is ignored");
        CHECK(host(gz.data(), gz.size(), DMX_BATCH_AUTO, dicts[1], &out, &used) == 0 && out == data && used == gz.size(), "gzip: no dictionary");
        // one byte farther than the dictionary reaches
        const bytes far = match_block((uint32_t)dict.size() + 1);
        CHECK(host(far.data(), far.size(), DMX_BATCH_RAW, dicts[1], &out, &used) == -(int)E_HUFDIS, "dlen + 1");
    }
    long id = 0;
    for (const bytes& m : pool)
        for (int d = 0; d < 4; d++)
            for (uint32_t fmt = DMX_BATCH_AUTO; fmt <= DMX_BATCH_RAW; fmt++)
                for (size_t k = 0; k <= m.size(); k++) check_one(m.data(), k, fmt, dicts[d], k == m.size() ? "whole" : "cut", id++);
    // every FLG of CMF 78 (FDICT in half of them), and a spread of CMF
    for (uint32_t b = 0; b < 256; b++)
        for (int d = 0; d < 4; d++) {
            bytes m = zf;
            m[1] = (uint8_t)b;
            check_one(m.data(), m.size(), DMX_BATCH_AUTO, dicts[d], "flg", id++);
            m[0] = (uint8_t)(b * 7 + 8);
            check_one(m.data(), m.size(), DMX_BATCH_ZLIB, dicts[d], "cmf", id++);
        }
    for (int it = 0; it < 6000; it++) {
        bytes m = pool[rnd((uint32_t)pool.size())];
        const uint32_t nm = 1 + rnd(3);
        for (uint32_t q = 0; q < nm; q++) {
            const uint32_t at = rnd(m.size() < 8 ? (uint32_t)m.size() : 8u);
            m[at] = rnd(3) ? (uint8_t)(m[at] ^ (1u << rnd(8))) : (uint8_t)rnd(256);
        }
        const size_t n = rnd(3) == 0 ? rnd((uint32_t)m.size() + 1) : m.size();
        check_one(m.data(), n, rnd(4), dicts[rnd(4)], "mutation", it);
    }
    printf("%ld checks, %d failed checks\n", checks, fails);
    return fails ? 1 : 0;
}

/*
 * gz_head_model.cpp -- the host twin of the batch decoder's framing (csrc/dmx_gz_head.h, the text
 * dmx_inflate_batch_kernel runs per stream) under AddressSanitizer + UBSan.  Built by
 * tests/c/Makefile.gz_head from this file and dmx_inflate.c; runs without a GPU.  The verdict of
 * dmx_frame_head is compared with deflate_decompress on the same bytes:
 *   - a verdict other than 0 is deflate_decompress's status;
 *   - a verdict of 0 names a format and the offset of the DEFLATE data: the bytes from there on,
 *     behind a plain header of that format, must get the status and the bytes that
 *     deflate_decompress gives the whole input (so the offset is the one the host decodes from).
 * Inputs: gzip members with all 16 combinations of FEXTRA / FNAME / FCOMMENT / FHCRC in three
 * field sizes, each whole (status 0) and at every cut point; zlib streams the same way; and 10 000
 * seeded mutations of one to three bytes, a third of them cut as well.  Every input is a heap block
 * of its exact size, so ASan sees a read behind it.  The explicit formats are checked against the
 * automatic one.  Exit status 0 = "0 failed checks" (the sanitizers abort on their own findings).
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

// deflate_decompress on an exact-size heap copy: the status, and the bytes when it is 0
static int host(const uint8_t* p, size_t n, bytes* out) {
    uint8_t* c = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(c, p, n);
    struct string_len in = {c, n}, o = {NULL, 0};
    const int r = deflate_decompress(&o, &in, 0);
    if (out) out->assign(o.str, o.str + (r == 0 ? o.len : 0));
    free(o.str);
    free(c);
    return r;
}

// a stored block holding d (final)
static bytes stored(const bytes& d) {
    bytes b = {1, (uint8_t)d.size(), (uint8_t)(d.size() >> 8), (uint8_t)~d.size(), (uint8_t)(~d.size() >> 8)};
    b.insert(b.end(), d.begin(), d.end());
    return b;
}
static void le32(bytes& b, uint32_t v) { for (int k = 0; k < 4; k++) b.push_back((uint8_t)(v >> (8 * k))); }

static bytes gz_member(uint32_t flg, uint32_t xlen, uint32_t namelen, const bytes& d) {
    bytes b = {0x1F, 0x8B, 8, (uint8_t)flg, 1, 2, 3, 4, 0, 3};
    if (flg & 4) {
        b.push_back((uint8_t)xlen);
        b.push_back((uint8_t)(xlen >> 8));
        for (uint32_t k = 0; k < xlen; k++) b.push_back((uint8_t)(k * 7));   // (zeros among them)
    }
    for (uint32_t f = 8; f <= 16; f <<= 1)
        if (flg & f) {
            for (uint32_t k = 0; k < namelen; k++) b.push_back((uint8_t)('a' + k % 26));
            b.push_back(0);
        }
    if (flg & 2) { b.push_back(0x12); b.push_back(0x34); }
    const bytes s = stored(d);
    b.insert(b.end(), s.begin(), s.end());
    le32(b, dmx_crc32_host(0, d.data(), d.size()));
    le32(b, (uint32_t)d.size());
    return b;
}

static uint32_t adler(const bytes& d) {
    uint32_t a = 1, b = 0;
    for (uint8_t c : d) { a = (a + c) % 65521u; b = (b + a) % 65521u; }
    return (b << 16) | a;
}
static bytes z_stream(const bytes& d) {
    bytes b = {0x78, 0x9C};
    const bytes s = stored(d);
    b.insert(b.end(), s.begin(), s.end());
    const uint32_t a = adler(d);
    for (int k = 3; k >= 0; k--) b.push_back((uint8_t)(a >> (8 * k)));
    return b;
}

static void check_one(const uint8_t* src, size_t n, const char* what, long id) {
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);   // exact size: a read at or behind p + n is ASan's
    if (n) memcpy(p, src, n);
    uint32_t format = 99;
    uint64_t body = ~0ull;
    const int v = dmx_frame_head(p, n, DMX_BATCH_AUTO, &format, &body);
    bytes want;
    const int h = host(p, n, &want);
    const bool magic = n >= 2 && p[0] == 0x1F && p[1] == 0x8B;
    CHECK(format == (magic ? DMX_BATCH_GZIP : DMX_BATCH_ZLIB), "%s %ld: format %u", what, id, format);
    if (v != 0) {
        CHECK(v == h, "%s %ld: verdict %d, host %d", what, id, v, h);
    } else {
        CHECK(body <= n && body >= 2, "%s %ld: body %llu of %zu", what, id, (unsigned long long)body, n);
        if (body <= n) {
            bytes plain;
            if (format == DMX_BATCH_GZIP) plain = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 3};
            else plain = {0x78, 0x9C};
            plain.insert(plain.end(), p + body, p + n);
            bytes got;
            const int h2 = host(plain.data(), plain.size(), &got);
            CHECK(h2 == h && got == want, "%s %ld: from body %llu the host says %d, on the whole %d", what, id,
                  (unsigned long long)body, h2, h);
        }
    }
    // the explicit formats: the automatic verdict where the bytes name that format
    uint32_t f2 = 99;
    uint64_t b2 = ~0ull;
    const int vg = dmx_frame_head(p, n, DMX_BATCH_GZIP, &f2, &b2);
    CHECK(f2 == DMX_BATCH_GZIP, "%s %ld: explicit gzip format %u", what, id, f2);
    if (magic) CHECK(vg == v && (v || b2 == body), "%s %ld: explicit gzip %d / %d", what, id, vg, v);
    else CHECK(vg == -(int)E_ZHEAD, "%s %ld: explicit gzip without magic %d", what, id, vg);
    const int vz = dmx_frame_head(p, n, DMX_BATCH_ZLIB, &f2, &b2);
    CHECK(f2 == DMX_BATCH_ZLIB, "%s %ld: explicit zlib format %u", what, id, f2);
    if (!magic) CHECK(vz == v && (v || b2 == body), "%s %ld: explicit zlib %d / %d", what, id, vz, v);
    else CHECK(vz == -(int)E_ZCMPMT, "%s %ld: explicit zlib on a gzip magic %d", what, id, vz);
    const int vr = dmx_frame_head(p, n, DMX_BATCH_RAW, &f2, &b2);
    CHECK(vr == 0 && f2 == DMX_BATCH_RAW && b2 == 0, "%s %ld: raw %d", what, id, vr);
    free(p);
}

int main(void) {
    bytes data;
    for (int k = 0; k < 300; k++) data.push_back((uint8_t)(k * 31 + (k >> 3)));
    std::vector<bytes> pool;
    const uint32_t xl[3] = {0, 5, 300}, nl[3] = {0, 3, 40};
    long id = 0;
    for (uint32_t flg = 0; flg < 32; flg += 2)   // FHCRC 2, FEXTRA 4, FNAME 8, FCOMMENT 16
        for (int sz = 0; sz < 3; sz++) {
            const bytes m = gz_member(flg, xl[sz], nl[sz], data);
            bytes out;
            CHECK(host(m.data(), m.size(), &out) == 0 && out == data, "member flg %u size %d is not sound", flg, sz);
            uint32_t format = 0;
            uint64_t body = 0;
            CHECK(dmx_frame_head(m.data(), m.size(), DMX_BATCH_AUTO, &format, &body) == 0 && format == DMX_BATCH_GZIP &&
                      body == m.size() - 8 - (5 + data.size()),
                  "member flg %u size %d: body %llu", flg, sz, (unsigned long long)body);
            check_one(m.data(), m.size(), "whole", id++);
            bytes junk = m;
            junk.push_back(0xAA);
            check_one(junk.data(), junk.size(), "junk", id++);
            // every cut inside the header and the first bytes of the data, and inside the trailer
            for (size_t k = 0; k < m.size(); k++)
                if (k < body + 8 || k + 10 > m.size()) check_one(m.data(), k, "cut", id++);
            pool.push_back(m);
        }
    // the reserved FLG bits, CM != 8, the magic
    for (uint32_t bit = 0x20; bit <= 0x80; bit <<= 1) {
        bytes m = gz_member(bit | 8, 0, 3, data);
        check_one(m.data(), m.size(), "reserved", id++);
    }
    for (uint32_t cm = 0; cm < 16; cm++) {
        bytes m = pool[5];
        m[2] = (uint8_t)cm;
        check_one(m.data(), m.size(), "cm", id++);
    }
    {
        const bytes zs = z_stream(data);
        bytes out;
        CHECK(host(zs.data(), zs.size(), &out) == 0 && out == data, "the zlib stream is not sound");
        for (size_t k = 0; k <= zs.size(); k++)
            if (k < 12 || k + 6 > zs.size()) check_one(zs.data(), k, "zcut", id++);
        for (uint32_t a = 0; a < 256; a++)
            for (uint32_t b = 0; b < 256; b += 5) {   // every CMF with a spread of FLG, 1F 8B among them
                bytes m = zs;
                m[0] = (uint8_t)a;
                m[1] = (uint8_t)(a == 0x1F && b == 0x8C ? 0x8B : b);
                check_one(m.data(), m.size(), "zhead", id++);
            }
        pool.push_back(zs);
    }
    // 10 000 seeded mutations
    for (int it = 0; it < 10000; it++) {
        bytes m = pool[rnd((uint32_t)pool.size())];
        const uint32_t nm = 1 + rnd(3);
        const uint32_t span = rnd(4) ? (m.size() < 64 ? (uint32_t)m.size() : 64u) : (uint32_t)m.size();   // mostly the header
        for (uint32_t q = 0; q < nm; q++) {
            const uint32_t at = rnd(span);
            m[at] = rnd(3) ? (uint8_t)(m[at] ^ (1u << rnd(8))) : (uint8_t)rnd(256);
        }
        const size_t n = rnd(3) == 0 ? rnd((uint32_t)m.size() + 1) : m.size();
        check_one(m.data(), n, "mutation", it);
    }
    printf("%ld checks, %d failed checks\n", checks, fails);
    return fails ? 1 : 0;
}

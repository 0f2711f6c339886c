// zsel_model.cpp -- the rule that turns a plan's live chunks into seek points (csrc/dmx_zsel.h, the
// text dmx_zindex_from_chunks_host and the select kernel run) on the CPU, under ASan + UBSan: random
// chunk tables -- chunks of no output, one chunk, spans of 1 and above the total -- go through
// dmx_zs_select, and the points are compared with a plain restatement of dmx_zindex_build_host's
// loop taken chunk by chunk (a point ends behind the first chunk at which it holds span bytes, unless
// that chunk is the last), with the consequences the callers rely on: the points tile the chunks and
// the output, all but the last hold min(span, total) bytes, npoints <= dmx_zs_bound, the piece bases
// are the running sum of ceil(out_len / 65536), and a capacity below npoints writes nothing beyond it.
// Stand-alone: its own main, no HIP, nothing preloaded.  Ends with "N checks, 0 failed checks".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dmx_zsel.h"

namespace {

uint64_t g_checks = 0, g_failed = 0;
#define CHECK(c, ...) do { g_checks++; if (!(c)) { g_failed++; printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {   // 0 .. n - 1
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 11) % n);
}

// the host builder's loop with a chunk for a block: the output of the chunk goes to the current
// point; behind a chunk that is not the last, a point that holds span bytes ends
std::vector<dmx_zpoint> plain(const std::vector<dmx_pchunk>& ch, uint32_t span) {
    std::vector<dmx_zpoint> pts;
    pts.push_back({ch[0].bit, 0, 0, 0});
    for (size_t c = 0; c < ch.size(); c++) {
        dmx_zpoint& p = pts.back();
        p.out_len += ch[c].out_len;
        p.end_bit = ch[c].end_bit;
        const bool last = c + 1 == ch.size();
        if (!last && p.out_len >= span) pts.push_back({ch[c].end_bit, 0, ch[c].out_off + ch[c].out_len, 0});
    }
    return pts;
}

std::vector<dmx_pchunk> table(uint32_t n, uint32_t kind) {
    std::vector<dmx_pchunk> ch(n);
    uint64_t bit = 16 + rnd(8), off = 0;
    for (uint32_t c = 0; c < n; c++) {
        uint64_t len;
        switch (kind) {
            case 0: len = rnd(200000); break;                       // text-like chunks
            case 1: len = rnd(3) ? rnd(5000) : 0; break;            // many chunks of no output
            case 2: len = rnd(8) ? rnd(70000) : 65536 * (1 + rnd(3)); break;   // whole pieces among them
            default: len = rnd(4) ? 0 : rnd(300); break;            // nearly nothing
        }
        if (c + 1 == n && rnd(3) == 0) len = 0;                     // an empty last chunk
        ch[c].bit = bit;
        bit += 3 + rnd(100000);
        ch[c].end_bit = bit;
        ch[c].out_off = off;
        ch[c].out_len = len;
        off += len;
    }
    return ch;
}

void one(const std::vector<dmx_pchunk>& ch, uint32_t span) {
    const uint32_t nlive = (uint32_t)ch.size();
    const uint64_t total = ch.back().out_off + ch.back().out_len;
    const std::vector<dmx_zpoint> want = plain(ch, span);
    const uint32_t n = dmx_zs_select(ch.data(), nlive, span, NULL, NULL, 0);
    CHECK(n == want.size(), "npoints %u, plain %zu (nlive %u span %u)", n, want.size(), nlive, span);
    CHECK(n >= 1 && n <= dmx_zs_bound(total, nlive, span), "npoints %u above the bound %u", n, dmx_zs_bound(total, nlive, span));
    std::vector<dmx_zpoint> pts(n);
    std::vector<uint32_t> base(n + 1);
    CHECK(dmx_zs_select(ch.data(), nlive, span, pts.data(), base.data(), n) == n, "the second walk counts otherwise");
    if (n != want.size()) return;
    CHECK(!memcmp(pts.data(), want.data(), n * sizeof(dmx_zpoint)), "points differ (nlive %u span %u)", nlive, span);
    uint64_t off = 0, pieces = 0;
    for (uint32_t k = 0; k < n; k++) {
        CHECK(pts[k].out_off == off && base[k] == pieces, "point %u: out_off %llu base %u", k, (unsigned long long)pts[k].out_off, base[k]);
        CHECK(k + 1 == n ? pts[k].end_bit == ch.back().end_bit : pts[k].end_bit == pts[k + 1].bit, "point %u: end_bit", k);
        if (k + 1 < n) CHECK(pts[k].out_len >= (span < total ? span : total), "point %u holds %llu", k, (unsigned long long)pts[k].out_len);
        off += pts[k].out_len;
        pieces += (pts[k].out_len + 65535) / 65536;
    }
    CHECK(off == total && base[n] == pieces && pieces <= dmx_zs_max_pieces(total, n), "the points' sum %llu of %llu", (unsigned long long)off,
          (unsigned long long)total);
    CHECK(pts[0].bit == ch[0].bit, "point 0 begins at chunk 0");
    if (span == 1) {   // every chunk that follows output begins a point
        // (output was produced since the current point began: the chunk's out_off is not that point's)
        uint32_t m = 1;
        uint64_t cur = 0;
        for (uint32_t c = 1; c < nlive; c++)
            if (ch[c].out_off != cur) { m++; cur = ch[c].out_off; }
        CHECK(n == m, "span 1: %u points, %u chunks follow output", n, m);
    }
    if (span > total) CHECK(n == 1, "span above the total: %u points", n);
    // a capacity below npoints: entries [0, cap) as before, nothing behind them
    if (n >= 2) {
        const uint32_t cap = 1 + rnd(n - 1);
        std::vector<dmx_zpoint> p2(cap);
        std::vector<uint32_t> b2(cap + 1, 0xA5A5A5A5u);
        CHECK(dmx_zs_select(ch.data(), nlive, span, p2.data(), b2.data(), cap) == n, "a small capacity changes the count");
        CHECK(!memcmp(p2.data(), pts.data(), cap * sizeof(dmx_zpoint)) && !memcmp(b2.data(), base.data(), cap * 4) &&
              b2[cap] == 0xA5A5A5A5u, "a small capacity: entries differ or one more is written");
    }
}

}   // namespace

int main() {
    uint64_t tables = 0;
    for (uint32_t round = 0; round < 4000; round++) {
        const uint32_t kind = round & 3;
        const uint32_t n = round < 40 ? 1 + round / 8 : 1 + rnd(round & 4 ? 12 : 400);
        const std::vector<dmx_pchunk> ch = table(n, kind);
        const uint64_t total = ch.back().out_off + ch.back().out_len;
        const uint32_t spans[] = {1, 2, 1 + rnd(70000), 65536, DMX_ZINDEX_DEF_SPAN, 1 + rnd(1u << 22),
                                  (uint32_t)(total < DMX_ZINDEX_MAX_SPAN ? total + 1 : DMX_ZINDEX_MAX_SPAN), DMX_ZINDEX_MAX_SPAN,
                                  (uint32_t)(total && total <= DMX_ZINDEX_MAX_SPAN ? total : 1)};
        for (uint32_t s : spans) one(ch, s);
        tables++;
    }
    CHECK(dmx_zs_span(0) == DMX_ZINDEX_DEF_SPAN && dmx_zs_span(7) == 7, "span 0 is the default");
    CHECK(dmx_zs_bound(0, 0, 0) == 1 && dmx_zs_bound(0, 9, 1) == 1 && dmx_zs_bound(100, 0, 1) == 1 && dmx_zs_bound(100, 9, 1) == 9 &&
          dmx_zs_bound(100, 900, 1) == 101 && dmx_zs_bound(1 << 20, 900, 0) == 5, "dmx_zs_bound");
    CHECK(dmx_zs_work(0, 0) % 256 == 0 && dmx_zs_work(1 << 30, 1000) % 256 == 0 && dmx_zs_work(0, 1) == 768, "dmx_zs_work");
    printf("%llu chunk tables\n", (unsigned long long)tables);
    printf("%llu checks, %llu failed checks\n", (unsigned long long)g_checks, (unsigned long long)g_failed);
    return g_failed ? 1 : 0;
}

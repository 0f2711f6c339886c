// ptail_model.cpp -- the tail and pack rules of the parallel decode of one foreign stream
// (csrc/dmx_ptail.h, the text the kernels dmx_par_tails_kernel / dmx_par_pack_kernel run) on the
// CPU, under ASan + UBSan: random token streams are cut at random chunk starts, every chunk's
// cells are made as the CELL decoder makes them (a reference is relative to the chunk's start; a
// copy inside the chunk copies cells), the rules run over them as the kernels do -- two windows,
// the tail resolved in place, then the pack -- and the bytes are compared with a plain decode.
// Stand-alone: its own main, no HIP, nothing preloaded.  Ends with "N checks, 0 failed checks".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dmx_ptail.h"

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

struct Tok { uint32_t len, dist; uint8_t lit; };   // len 0: a literal
struct Chunk { uint64_t off, len; std::vector<Tok> toks; };

// tokens that produce exactly `len` bytes from output position `off` on; far: the share (in 1/8) of
// matches at the distances in `fars`; a distance never reaches before `floor_pos` (0: the output's start)
std::vector<Tok> make_tokens(uint64_t off, uint64_t len, uint32_t far8, const std::vector<uint32_t>& fars, uint64_t floor_pos = 0) {
    std::vector<Tok> t;
    uint64_t made = 0;
    while (made < len) {
        const uint64_t pos = off + made, left = len - made, reach = pos - floor_pos;
        Tok k = {0, 0, (uint8_t)rnd(256)};
        if (left >= 3 && reach >= 1 && rnd(4) != 0) {
            k.len = 3 + rnd(left - 3 < 256 ? (uint32_t)(left - 3) + 1 : 256);
            uint32_t d;
            if (!fars.empty() && rnd(8) < far8) d = fars[rnd((uint32_t)fars.size())];
            else d = 1 + rnd(rnd(2) ? 64 : DMX_PT_WIN);
            if (d > reach) d = (uint32_t)(reach < DMX_PT_WIN ? reach : DMX_PT_WIN);
            k.dist = d;
        }
        t.push_back(k);
        made += k.len ? k.len : 1;
    }
    return t;
}

void plain(const std::vector<Chunk>& cs, std::vector<uint8_t>& out) {
    for (const Chunk& c : cs)
        for (const Tok& k : c.toks) {
            if (!k.len) { out.push_back(k.lit); continue; }
            for (uint32_t j = 0; j < k.len; j++) out.push_back(out[out.size() - k.dist]);
        }
}

// the cells of one chunk, as iblock's CELL instantiation leaves them
void make_cells(const Chunk& c, std::vector<uint16_t>& cells) {
    uint64_t op = 0;
    for (const Tok& k : c.toks) {
        if (!k.len) { cells[c.off + op++] = k.lit; continue; }
        for (uint32_t j = 0; j < k.len; j++, op++) {
            const int64_t sp = (int64_t)op - (int64_t)k.dist;
            cells[c.off + op] = sp < 0 ? (uint16_t)dmx_pt_ref((uint32_t)-sp) : cells[c.off + (uint64_t)sp];
        }
    }
}

// the tail pass and the pack pass as the kernels run them; returns the number of cells the rules refused
uint64_t resolve(const std::vector<Chunk>& cs, std::vector<uint16_t>& cells, std::vector<uint8_t>& out) {
    std::vector<uint8_t> win[2] = {std::vector<uint8_t>(DMX_PT_WIN, 0xEE), std::vector<uint8_t>(DMX_PT_WIN, 0xEE)};
    uint32_t cur = 0;
    uint64_t bad = 0;
    for (const Chunk& c : cs) {
        uint16_t* tc = cells.data() + c.off + c.len - dmx_pt_tail(c.len);
        const uint8_t* W = win[cur].data();
        uint8_t* N = win[cur ^ 1].data();
        for (uint32_t k = 0; k < DMX_PT_WIN; k++) {
            uint32_t idx;
            int v;
            if (dmx_pt_next(k, c.len, &idx)) {
                CHECK(idx < dmx_pt_tail(c.len), "tail index %u of %u", idx, dmx_pt_tail(c.len));
                v = dmx_pt_cell(tc[idx], W, c.off);
                if (v < 0) { bad++; v = 0; }
                tc[idx] = (uint16_t)v;
            } else {
                CHECK(idx < DMX_PT_WIN, "window index %u", idx);
                v = W[idx];
            }
            N[k] = (uint8_t)v;
        }
        cur ^= 1;
    }
    uint64_t total = 0;
    for (const Chunk& c : cs) total += c.len;
    out.assign(total, 0);
    for (const Chunk& c : cs)
        for (uint64_t p = c.off; p < c.off + c.len; p++) {
            int v = dmx_pt_pack(cells.data(), p, c.off);
            if (v < 0) { bad++; v = 0; }
            out[p] = (uint8_t)v;
        }
    return bad;
}

std::vector<Chunk> build(const std::vector<uint64_t>& lens, uint32_t far8, const std::vector<uint32_t>& fars) {
    std::vector<Chunk> cs;
    uint64_t off = 0;
    for (uint64_t n : lens) {
        Chunk c = {off, n, make_tokens(off, n, far8, fars)};
        cs.push_back(c);
        off += n;
    }
    return cs;
}

void run(const char* what, const std::vector<uint64_t>& lens, uint32_t far8, const std::vector<uint32_t>& fars) {
    const std::vector<Chunk> cs = build(lens, far8, fars);
    std::vector<uint8_t> want, got;
    plain(cs, want);
    std::vector<uint16_t> cells(want.size() + 1, 0xFFFF);
    for (const Chunk& c : cs) make_cells(c, cells);
    uint64_t refs = 0;
    for (size_t p = 0; p < want.size(); p++) refs += cells[p] >= DMX_PT_REF;
    const uint64_t bad = resolve(cs, cells, got);
    CHECK(bad == 0, "%s: %llu cells refused", what, (unsigned long long)bad);
    CHECK(got.size() == want.size() && (want.empty() || !memcmp(got.data(), want.data(), want.size())), "%s: bytes differ", what);
    if (lens.size() > 1 && want.size() - lens[0] >= 1000 && lens[0] >= 1000)   // (enough tokens behind a start that some reach across it)
        CHECK(refs > 0, "%s: no reference cell at all", what);
}

// references before output offset 0: the rules refuse them and read nothing outside their arrays
void before_zero() {
    for (uint32_t first : {1u, 100u, 5000u, 32767u}) {
        for (uint32_t extra : {1u, 7u, 32768u}) {
            std::vector<Chunk> cs = build({first, 300, 40000}, 2, {});
            std::vector<uint16_t> cells(first + 300 + 40000, 0);
            for (const Chunk& c : cs) make_cells(c, cells);
            // chunk 1 begins at `first` < 32 768: a reference first + extra back reaches before the output
            const uint32_t b = first + extra;
            if (b > 65280) continue;
            cells[first + 5] = (uint16_t)dmx_pt_ref(b);
            cells[first + 300 + 10] = (uint16_t)dmx_pt_ref(first + 300 + extra <= 65280 ? first + 300 + extra : 65280);   // outside chunk 2's tail: the pack meets it
            std::vector<uint8_t> got;
            const uint64_t bad = resolve(cs, cells, got);
            CHECK(bad == 2, "before zero (%u, %u): %llu refused, 2 wanted", first, extra, (unsigned long long)bad);
        }
    }
    // every 16-bit cell value against every window position the rule may touch
    std::vector<uint8_t> W(DMX_PT_WIN, 7);
    for (uint32_t c = 0; c < 65536; c++)
        for (uint64_t off : {0ull, 1ull, 32767ull, 32768ull, 1ull << 31}) {
            const int v = dmx_pt_cell(c, W.data(), off);
            const bool ok = c < DMX_PT_REF || (dmx_pt_back(c) <= DMX_PT_WIN && dmx_pt_back(c) <= off);
            CHECK((v >= 0) == ok, "cell %u at %llu", c, (unsigned long long)off);
        }
}

}   // namespace

int main() {
    const std::vector<uint32_t> edge = {32768, 32767};
    // the chunk lengths around the window, alone and in every order of two
    const uint64_t L[] = {1, 100, 32767, 32768, 32769, 70000};
    for (uint64_t a : L)
        for (uint64_t b : L) {
            run("pair", {40000, a, b}, 4, edge);
            run("pair-first", {a, b, 40000}, 4, edge);
        }
    // distances 32 768 and 32 767 across one and across several chunk starts
    run("one start", {40000, 70000}, 7, edge);
    run("several starts", {40000, 5, 5, 5, 70000}, 7, edge);
    run("several short", {33000, 900, 1, 2000, 100, 32769, 100, 32768}, 7, edge);
    // a window assembled from up to 40 short chunks
    for (uint32_t n : {2u, 17u, 40u}) {
        std::vector<uint64_t> lens = {50000};
        for (uint32_t k = 0; k < n; k++) lens.push_back(1 + rnd(32768 / n + 64));
        lens.push_back(70000);
        lens.push_back(100);
        run("assembled", lens, 6, edge);
    }
    // random cuts
    for (int rep = 0; rep < 60; rep++) {
        std::vector<uint64_t> lens;
        const uint32_t n = 1 + rnd(12);
        for (uint32_t k = 0; k < n; k++) lens.push_back(rnd(3) ? 1 + rnd(4000) : 1 + rnd(90000));
        run("random", lens, rnd(8), edge);
    }
    // a chunk whose last 32 768 cells are all references to before its own start: a run copied from
    // 32 768 back, then copied on at distance 8
    {
        Chunk a = {0, 40000, make_tokens(0, 40000, 0, {})};
        Chunk b = {40000, 8 + 300 * 258, {}};
        b.toks.push_back({8, 32768, 0});
        for (int k = 0; k < 300; k++) b.toks.push_back({258, 8, 0});
        Chunk c = {b.off + b.len, 5000, make_tokens(b.off + b.len, 5000, 6, edge)};
        const std::vector<Chunk> cs = {a, b, c};
        std::vector<uint8_t> want, got;
        plain(cs, want);
        std::vector<uint16_t> cells(want.size(), 0xFFFF);
        for (const Chunk& x : cs) make_cells(x, cells);
        uint64_t refs = 0;
        for (uint64_t p = b.off + b.len - DMX_PT_WIN; p < b.off + b.len; p++) refs += cells[p] >= DMX_PT_REF;
        CHECK(refs == DMX_PT_WIN, "run chunk: %llu of its last 32768 cells are references", (unsigned long long)refs);
        CHECK(resolve(cs, cells, got) == 0 && got == want, "run chunk: bytes differ");
    }
    before_zero();
    printf("%llu checks, %llu failed checks\n", (unsigned long long)g_checks, (unsigned long long)g_failed);
    return g_failed ? 1 : 0;
}

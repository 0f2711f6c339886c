// The host twin of the batch encode's plan (csrc/dmx_encode_batch.hip): the four planning stages run
// as loops over the per-thread text of csrc/dmx_encode_batch.h, with the scan tile shrunk
// (DMX_EB_STILE / DMX_EB_STHREADS from the Makefile) so that small batches cross many tile edges,
// against a brute-force loop: the block table, the starts, the streams' records and the -E_RANGE /
// -E_SZ decisions, for seeded random stream lists that hold the lengths 0, 1, sw - 1, sw, sw + 1,
// offsets at the end of the input and in_off + in_len wrapping 2^64, with max_blocks below, at and
// above the need.  Built with ASan + UBSan; prints `<n> failed checks`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dmx_encode_batch.h"

static long g_failed = 0, g_checks = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        g_checks++;                                    \
        if (!(c)) {                                    \
            if (g_failed++ < 20) {                     \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);                   \
                printf("\n");                          \
            }                                          \
        }                                              \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Plan {
    dmx_eb_head head;
    std::vector<uint64_t> starts;
    std::vector<dmx_eresult> res;
    std::vector<dmx_bblk> tab;
};

// the four kernels as loops: a "workgroup" is a tile of DMX_EB_STILE streams, its collectives are loops
static Plan run_plan(const std::vector<dmx_estream>& st, uint64_t in_bytes, uint32_t sw, uint32_t max_blocks) {
    Plan P;
    const uint32_t n = (uint32_t)st.size();
    const uint32_t ntiles = (n + DMX_EB_STILE - 1) / DMX_EB_STILE;
    std::vector<dmx_eb_tile> tiles(ntiles + 1, dmx_eb_tile_zero());
    // 1. dmx_eb_count_kernel
    for (uint32_t t = 0; t < ntiles; t++) {
        dmx_eb_tile sum = dmx_eb_tile_zero();
        for (uint32_t i = 0; i < DMX_EB_STILE; i++) {
            const uint64_t k = (uint64_t)t * DMX_EB_STILE + i;
            if (k < n) sum = dmx_eb_tile_add(sum, dmx_eb_stream_sums(st.data(), (uint32_t)k, in_bytes, sw));
        }
        tiles[t] = sum;
    }
    // 2. dmx_eb_plan_scan_kernel: every thread's share, the scan over the threads, the decision
    {
        std::vector<dmx_eb_tile> mine(DMX_EB_STHREADS);
        for (uint32_t t = 0; t < DMX_EB_STHREADS; t++) mine[t] = dmx_eb_chunk_sum(tiles.data(), ntiles, DMX_EB_STHREADS, t);
        dmx_eb_tile total = dmx_eb_tile_zero();
        std::vector<uint64_t> before(DMX_EB_STHREADS);
        for (uint32_t t = 0; t < DMX_EB_STHREADS; t++) {
            before[t] = total.blocks;
            total = dmx_eb_tile_add(total, mine[t]);
        }
        for (uint32_t t = 0; t < DMX_EB_STHREADS; t++) dmx_eb_chunk_apply(tiles.data(), ntiles, DMX_EB_STHREADS, t, before[t]);
        dmx_eb_decide(&P.head, total, max_blocks);
    }
    // 3. dmx_eb_starts_kernel
    P.starts.assign((size_t)n + 1, 0xDEADull);
    P.res.resize(n);
    for (uint32_t t = 0; t < ntiles; t++) {
        uint64_t run = 0;
        for (uint32_t i = 0; i < DMX_EB_STILE; i++) {
            const uint64_t k = (uint64_t)t * DMX_EB_STILE + i;
            if (k >= n) break;
            dmx_eb_start(st.data(), (uint32_t)k, n, in_bytes, sw, dmx_eb_sat(tiles[t].blocks, run), P.starts.data(),
                         P.res.data());
            run = dmx_eb_sat(run, dmx_eb_count(st[k], in_bytes, sw));
        }
    }
    // 4. dmx_eb_table_kernel
    P.tab.resize(max_blocks);
    for (uint32_t b = 0; b < max_blocks; b++)
        P.tab[b] = dmx_eb_entry(st.data(), P.starts.data(), n, &P.head, sw, b);
    return P;
}

static void check_batch(const std::vector<dmx_estream>& st, uint64_t in_bytes, uint32_t sw, uint32_t max_blocks,
                        const char* what) {
    const Plan P = run_plan(st, in_bytes, sw, max_blocks);
    const uint32_t n = (uint32_t)st.size();
    // brute force, with 128-bit sums where a 64-bit one could wrap
    std::vector<dmx_bblk> want;
    unsigned __int128 nblocks = 0, bytes = 0;
    uint32_t nfailed = 0, first_bad = DMX_EB_NOBAD;
    std::vector<uint64_t> starts(n + 1, 0);
    for (uint32_t k = 0; k < n; k++) {
        starts[k] = nblocks > ~0ull ? ~0ull : (uint64_t)nblocks;
        const unsigned __int128 end = (unsigned __int128)st[k].in_off + st[k].in_len;
        const bool ok = end <= in_bytes;
        CHECK(P.res[k].status == (ok ? 0 : -(int32_t)E_RANGE), "%s: stream %u status %d", what, k, P.res[k].status);
        CHECK(P.res[k].out_off == 0 && P.res[k].out_len == 0 && P.res[k].check == 0 && P.res[k].reserved == 0,
              "%s: stream %u record not clean", what, k);
        if (!ok) {
            nfailed++;
            if (first_bad == DMX_EB_NOBAD) first_bad = k;
            CHECK(P.res[k].nblocks == 0, "%s: bad stream %u has blocks", what, k);
            continue;
        }
        bytes += st[k].in_len;
        uint64_t cnt = 0;
        for (uint64_t o = 0; o < st[k].in_len; o += sw) {
            const uint64_t left = st[k].in_len - o;
            dmx_bblk e;
            e.off = st[k].in_off + o;
            e.len = (uint32_t)(left < sw ? left : sw) | (o == 0 ? DMX_BB_FIRST : 0u) | (left <= sw ? DMX_BB_LAST : 0u);
            e.stream = k;
            if (want.size() <= (size_t)max_blocks) want.push_back(e);
            cnt++;
        }
        if (!st[k].in_len) {   // the empty stream's one block
            const dmx_bblk e = {st[k].in_off, DMX_BB_FIRST | DMX_BB_LAST, k};
            if (want.size() <= (size_t)max_blocks) want.push_back(e);
            cnt = 1;
        }
        CHECK(P.res[k].nblocks == cnt, "%s: stream %u nblocks %u want %llu", what, k, P.res[k].nblocks, (unsigned long long)cnt);
        nblocks += cnt;
    }
    starts[n] = nblocks > ~0ull ? ~0ull : (uint64_t)nblocks;
    CHECK(P.head.nblocks == starts[n], "%s: nblocks %llu want %llu", what, (unsigned long long)P.head.nblocks,
          (unsigned long long)starts[n]);
    CHECK(P.head.in_len == (bytes > ~0ull ? ~0ull : (uint64_t)bytes), "%s: in_len", what);
    CHECK(P.head.nfailed == nfailed && P.head.first_bad == first_bad, "%s: nfailed %u first_bad %u", what, P.head.nfailed,
          P.head.first_bad);
    const bool sz = nblocks > max_blocks;
    CHECK(P.head.status == (sz ? -(int32_t)E_SZ : 0), "%s: status %d", what, P.head.status);
    if (n)
        for (uint32_t k = 0; k <= n; k++)
            CHECK(P.starts[k] == starts[k], "%s: starts[%u] %llu want %llu", what, k, (unsigned long long)P.starts[k],
                  (unsigned long long)starts[k]);
    for (uint32_t b = 0; b < max_blocks; b++) {
        const dmx_bblk& e = P.tab[b];
        if (sz || b >= nblocks) {
            CHECK(e.len == DMX_BB_VOID, "%s: entry %u not void", what, b);
        } else {
            const dmx_bblk& w = want[b];
            CHECK(e.off == w.off && e.len == w.len && e.stream == w.stream, "%s: entry %u {%llu, %x, %u} want {%llu, %x, %u}",
                  what, b, (unsigned long long)e.off, e.len, e.stream, (unsigned long long)w.off, w.len, w.stream);
        }
    }
    // every stream is found from each of its blocks (the binary search, from the brute-force starts)
    if (n && !sz)
        for (uint64_t b = 0; b < nblocks && b < 4096; b++) {
            const uint32_t k = dmx_eb_find(starts.data(), n, b);
            CHECK(starts[k] <= b && b < starts[k + 1], "%s: find(%llu) = %u", what, (unsigned long long)b, k);
        }
}

int main() {
    // the bounds: monotone, and at least the real block count
    for (int it = 0; it < 2000; it++) {
        const uint32_t sw = 1 + (uint32_t)(rnd() % 300), n = (uint32_t)(rnd() % 40);
        const uint64_t total = rnd() % 5000;
        uint64_t left = total, blocks = 0;
        for (uint32_t k = 0; k < n; k++) {
            const uint64_t len = k + 1 == n ? left : (rnd() % 3 == 0 ? 0 : rnd() % (left + 1));
            left -= len;
            const uint64_t c = (len + sw - 1) / sw;
            blocks += c ? c : 1;
        }
        CHECK(dmx_eb_blocks_bound(total, n, sw) >= (n ? blocks : 0), "blocks bound %u < %llu", dmx_eb_blocks_bound(total, n, sw),
              (unsigned long long)blocks);
        CHECK(dmx_eb_blocks_bound(total + 1, n, sw) >= dmx_eb_blocks_bound(total, n, sw) &&
              dmx_eb_blocks_bound(total, n + 1, sw) >= dmx_eb_blocks_bound(total, n, sw), "blocks bound not monotone");
    }
    CHECK(dmx_eb_blocks_bound(~0ull, 0xFFFFFFFFu, 1) == 0xFFFFFFFFu, "blocks bound saturates");

    // fixed lists: no stream, one empty stream, the edge lengths, offsets at the end, wrapping sums
    const uint32_t sws[] = {1, 2, 7, 64, 1024, 32768};
    for (uint32_t sw : sws) {
        const uint64_t in_bytes = 4ull * sw + 37;
        std::vector<dmx_estream> st;
        check_batch(st, in_bytes, sw, 0, "no stream");
        check_batch(st, in_bytes, sw, 5, "no stream, capacity");
        st.push_back({0, 0});
        check_batch(st, in_bytes, sw, 1, "one empty stream");
        check_batch(st, in_bytes, sw, 0, "one empty stream, no capacity");
        st.clear();
        const uint64_t lens[] = {0, 1, (uint64_t)sw - 1, sw, (uint64_t)sw + 1, 2ull * sw, 2ull * sw + 1, 3ull * sw - 1};
        for (uint64_t len : lens)
            for (uint64_t off : {(uint64_t)0, (uint64_t)5, in_bytes - len, in_bytes - len + 1, in_bytes, in_bytes + 1})
                st.push_back({off, len});
        st.push_back({in_bytes, 0});                          // an empty stream at the very end: inside
        st.push_back({~0ull, 1});                             // in_off + in_len wraps to 0
        st.push_back({~0ull - 3, 8});                         // ... to 4
        st.push_back({8, ~0ull - 3});                         // ... to 4, a huge length
        st.push_back({0, ~0ull});
        st.push_back({1ull << 63, 1ull << 63});               // ... to exactly 0
        st.push_back({3, 2});
        uint32_t need = 0;
        {
            const Plan P = run_plan(st, in_bytes, sw, 0);
            need = (uint32_t)P.head.nblocks;
        }
        for (uint32_t mb : {0u, need - 1, need, need + 1, 2 * need + 7}) check_batch(st, in_bytes, sw, mb, "edge lengths");
    }

    // seeded random lists
    for (int it = 0; it < 1500; it++) {
        const uint32_t sw = (rnd() & 1) ? 1 + (uint32_t)(rnd() % 9) : 1 + (uint32_t)(rnd() % 600);
        const uint64_t in_bytes = rnd() % (20ull * sw + 3);
        const uint32_t n = (uint32_t)(rnd() % 70);
        std::vector<dmx_estream> st(n);
        for (uint32_t k = 0; k < n; k++) {
            const uint64_t pick = rnd() % 16;
            const uint64_t edge[] = {0, 1, (uint64_t)sw - 1, sw, (uint64_t)sw + 1};
            uint64_t len = pick < 5 ? edge[pick] : rnd() % (in_bytes + 2);
            uint64_t off = rnd() % 4 == 0 ? in_bytes - (len < in_bytes ? len : in_bytes) : rnd() % (in_bytes + 2);
            if (pick == 15) { off = ~0ull - rnd() % 8; len = 1 + rnd() % 16; }        // wraps
            if (pick == 14) { off = rnd() % (in_bytes + 1); len = ~0ull - rnd() % 8; }   // wraps or far too long
            st[k].in_off = off;
            st[k].in_len = len;
        }
        const Plan P0 = run_plan(st, in_bytes, sw, 0);
        const uint64_t need = P0.head.nblocks;
        const uint32_t caps[] = {0u, (uint32_t)(need ? need - 1 : 0), (uint32_t)need, (uint32_t)need + 1, (uint32_t)(2 * need + 7),
                                 (uint32_t)(rnd() % (need + 2))};
        for (uint32_t mb : caps) check_batch(st, in_bytes, sw, mb, "random");
    }
    printf("%ld checks, %ld failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}

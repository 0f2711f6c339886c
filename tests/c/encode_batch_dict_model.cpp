// The host twin of the dictionary batch's plan (csrc/dmx_encode_batch_dict.hip): the planning stages
// run as loops over the dmx_ebd_* per-thread text of csrc/dmx_encode_batch.h, with the scan tile
// shrunk (DMX_EB_STILE / DMX_EB_STHREADS from the Makefile), against a brute-force loop: every
// stream's status (-E_RANGE for a bad buffer, a bad dictionary index or a record outside d_dict,
// off + len wrapping 2^64 included; -E_INVAL under DMX_F_FDICT for a dictionary of length 0 or
// sw + 1), the block table with its DMX_BB_DICT marks, the starts, the first blocks' histories and
// the -E_SZ decision, for fixed and seeded random lists with DMX_BATCH_NODICT, a NULL d_dict_of and
// ndicts 0, with max_blocks below, at and above the need.  Built with ASan + UBSan; prints
// `<n> failed checks`.
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

// dmx_ebd_count_kernel, dmx_eb_plan_scan_kernel, dmx_ebd_starts_kernel and dmx_ebd_table_kernel as loops
static Plan run_plan(const std::vector<dmx_estream>& st, uint64_t in_bytes, uint32_t sw, const dmx_ebd& d, uint32_t max_blocks) {
    Plan P;
    const uint32_t n = (uint32_t)st.size();
    const uint32_t ntiles = (n + DMX_EB_STILE - 1) / DMX_EB_STILE;
    std::vector<dmx_eb_tile> tiles(ntiles + 1, dmx_eb_tile_zero());
    for (uint32_t t = 0; t < ntiles; t++) {
        dmx_eb_tile sum = dmx_eb_tile_zero();
        for (uint32_t i = 0; i < DMX_EB_STILE; i++) {
            const uint64_t k = (uint64_t)t * DMX_EB_STILE + i;
            if (k < n) sum = dmx_eb_tile_add(sum, dmx_ebd_stream_sums(st.data(), (uint32_t)k, in_bytes, sw, d));
        }
        tiles[t] = sum;
    }
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
    P.starts.assign((size_t)n + 1, 0xDEADull);
    P.res.resize(n);
    for (uint32_t t = 0; t < ntiles; t++) {
        uint64_t run = 0;
        for (uint32_t i = 0; i < DMX_EB_STILE; i++) {
            const uint64_t k = (uint64_t)t * DMX_EB_STILE + i;
            if (k >= n) break;
            dmx_ebd_start(st.data(), (uint32_t)k, n, in_bytes, sw, d, dmx_eb_sat(tiles[t].blocks, run), P.starts.data(),
                          P.res.data());
            run = dmx_eb_sat(run, dmx_ebd_count(st.data(), (uint32_t)k, in_bytes, sw, d));
        }
    }
    P.tab.resize(max_blocks);
    for (uint32_t b = 0; b < max_blocks; b++)
        P.tab[b] = dmx_ebd_entry(st.data(), P.starts.data(), n, &P.head, sw, d, b);
    return P;
}

static void check_batch(const std::vector<dmx_estream>& st, uint64_t in_bytes, uint32_t sw, const dmx_ebd& d,
                        uint32_t max_blocks, const char* what) {
    const Plan P = run_plan(st, in_bytes, sw, d, max_blocks);
    const uint32_t n = (uint32_t)st.size();
    std::vector<dmx_bblk> want;
    unsigned __int128 nblocks = 0, bytes = 0;
    uint32_t nfailed = 0, first_bad = DMX_EB_NOBAD;
    std::vector<uint64_t> starts(n + 1, 0);
    for (uint32_t k = 0; k < n; k++) {
        starts[k] = nblocks > ~0ull ? ~0ull : (uint64_t)nblocks;
        // brute force, with 128-bit sums where a 64-bit one could wrap
        int32_t status = 0;
        uint32_t di = d.dict_of ? d.dict_of[k] : d.ndicts ? 0u : DMX_BATCH_NODICT;
        uint64_t hn = 0, hoff = 0;
        if ((unsigned __int128)st[k].in_off + st[k].in_len > in_bytes) status = -(int32_t)E_RANGE;
        else if (di != DMX_BATCH_NODICT) {
            if (di >= d.ndicts) status = -(int32_t)E_RANGE;
            else if ((unsigned __int128)d.dicts[di].off + d.dicts[di].len > d.dict_bytes) status = -(int32_t)E_RANGE;
            else if (d.fdict && (d.dicts[di].len == 0 || d.dicts[di].len > sw)) status = -(int32_t)E_INVAL;
            else {
                hn = d.dicts[di].len < sw ? d.dicts[di].len : sw;
                hoff = d.dicts[di].off + d.dicts[di].len - hn;
            }
        }
        CHECK(P.res[k].status == status, "%s: stream %u status %d want %d", what, k, P.res[k].status, status);
        CHECK(P.res[k].out_off == 0 && P.res[k].out_len == 0 && P.res[k].check == 0 && P.res[k].reserved == 0,
              "%s: stream %u record not clean", what, k);
        if (status) {
            nfailed++;
            if (first_bad == DMX_EB_NOBAD) first_bad = k;
            CHECK(P.res[k].nblocks == 0, "%s: bad stream %u has blocks", what, k);
            continue;
        }
        {   // the first block's history: inside the dictionary, its last min(len, sw) bytes
            uint64_t off = 1;
            uint32_t slot = 77;
            const uint32_t h = dmx_ebd_history(d, k, sw, &off, &slot);
            CHECK(h == hn && (di == DMX_BATCH_NODICT || (off == hoff && slot == di)), "%s: stream %u history %u at %llu slot %u",
                  what, k, h, (unsigned long long)off, slot);
            CHECK(h <= sw && (!h || off + h <= d.dict_bytes), "%s: stream %u history outside d_dict", what, k);
        }
        const uint32_t mark = di != DMX_BATCH_NODICT ? DMX_BB_DICT : 0u;
        bytes += st[k].in_len;
        uint64_t cnt = 0;
        for (uint64_t o = 0; o < st[k].in_len; o += sw) {
            const uint64_t left = st[k].in_len - o;
            dmx_bblk e;
            e.off = st[k].in_off + o;
            e.len = (uint32_t)(left < sw ? left : sw) | (o == 0 ? DMX_BB_FIRST : 0u) | (left <= sw ? DMX_BB_LAST : 0u) | mark;
            e.stream = k;
            if (want.size() <= (size_t)max_blocks) want.push_back(e);
            cnt++;
        }
        if (!st[k].in_len) {
            const dmx_bblk e = {st[k].in_off, DMX_BB_FIRST | DMX_BB_LAST | mark, k};
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
    CHECK(P.head.nfailed == nfailed && P.head.first_bad == first_bad, "%s: nfailed %u first_bad %u want %u %u", what,
          P.head.nfailed, P.head.first_bad, nfailed, first_bad);
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
}

// every capacity around the need, under both settings of DMX_F_FDICT and with d_dict_of NULL as well
static void check_all(const std::vector<dmx_estream>& st, uint64_t in_bytes, uint32_t sw, const std::vector<dmx_bdict>& dicts,
                      uint64_t dict_bytes, const std::vector<uint32_t>& of, const char* what) {
    for (uint32_t fdict = 0; fdict < 2; fdict++)
        for (int with_of = 0; with_of < 2; with_of++) {
            const dmx_ebd d = {dicts.data(), with_of ? of.data() : nullptr, dict_bytes, (uint32_t)dicts.size(), fdict};
            const uint64_t need = run_plan(st, in_bytes, sw, d, 0).head.nblocks;
            const uint32_t caps[] = {0u, (uint32_t)(need ? need - 1 : 0), (uint32_t)need, (uint32_t)need + 1,
                                     (uint32_t)(2 * need + 7), (uint32_t)(rnd() % (need + 2))};
            for (uint32_t mb : caps) check_batch(st, in_bytes, sw, d, mb, what);
        }
}

int main() {
    const uint32_t sws[] = {1, 2, 7, 64, 1024, 32768};
    for (uint32_t sw : sws) {
        const uint64_t in_bytes = 4ull * sw + 37, dict_bytes = 3ull * sw + 11;
        // the dictionaries: the lengths 0, 1, sw - 1, sw, sw + 1, records at the end, past it and wrapping
        std::vector<dmx_bdict> dicts = {{0, 0}, {0, 1}, {3, (uint64_t)sw - 1}, {5, sw}, {7, (uint64_t)sw + 1},
                                        {dict_bytes, 0}, {dict_bytes - sw, sw}, {dict_bytes - sw + 1, sw}, {dict_bytes + 1, 0},
                                        {~0ull, 1}, {~0ull - 3, 8}, {8, ~0ull - 3}, {1ull << 63, 1ull << 63}, {0, dict_bytes}};
        std::vector<dmx_estream> st;
        std::vector<uint32_t> of;
        const uint64_t lens[] = {0, 1, sw, (uint64_t)sw + 1, 2ull * sw + 1};
        for (uint32_t j = 0; j < dicts.size() + 2; j++)
            for (uint64_t len : lens) {
                st.push_back({5, len});
                of.push_back(j < dicts.size() ? j : j == dicts.size() ? DMX_BATCH_NODICT : 1000u + j);
            }
        st.push_back({in_bytes, 1});   // bad buffers beat every dictionary verdict
        of.push_back(0);
        st.push_back({~0ull, 2});
        of.push_back(DMX_BATCH_NODICT);
        st.push_back({0, in_bytes});
        of.push_back(0xFFFFFFFEu);
        check_all(st, in_bytes, sw, dicts, dict_bytes, of, "edge dictionaries");
        // no dictionaries at all: with d_dict_of NULL every stream is written without one
        check_all(st, in_bytes, sw, std::vector<dmx_bdict>(), 0, of, "ndicts 0");
        check_all(std::vector<dmx_estream>(), in_bytes, sw, dicts, dict_bytes, std::vector<uint32_t>(), "no stream");
    }
    for (int it = 0; it < 1200; it++) {
        const uint32_t sw = (rnd() & 1) ? 1 + (uint32_t)(rnd() % 9) : 1 + (uint32_t)(rnd() % 600);
        const uint64_t in_bytes = rnd() % (20ull * sw + 3), dict_bytes = rnd() % (6ull * sw + 3);
        const uint32_t n = (uint32_t)(rnd() % 70), nd = (uint32_t)(rnd() % 6);
        std::vector<dmx_bdict> dicts(nd);
        for (uint32_t j = 0; j < nd; j++) {
            const uint64_t pick = rnd() % 12;
            const uint64_t edge[] = {0, 1, (uint64_t)sw - 1, sw, (uint64_t)sw + 1};
            uint64_t len = pick < 5 ? edge[pick] : rnd() % (dict_bytes + 2);
            uint64_t off = rnd() % 3 == 0 ? dict_bytes - (len < dict_bytes ? len : dict_bytes) : rnd() % (dict_bytes + 2);
            if (pick == 11) { off = ~0ull - rnd() % 8; len = 1 + rnd() % 16; }            // wraps
            if (pick == 10) { off = rnd() % (dict_bytes + 1); len = ~0ull - rnd() % 8; }   // wraps or far too long
            dicts[j] = {off, len};
        }
        std::vector<dmx_estream> st(n);
        std::vector<uint32_t> of(n);
        for (uint32_t k = 0; k < n; k++) {
            const uint64_t pick = rnd() % 16;
            const uint64_t edge[] = {0, 1, (uint64_t)sw - 1, sw, (uint64_t)sw + 1};
            uint64_t len = pick < 5 ? edge[pick] : rnd() % (in_bytes + 2);
            uint64_t off = rnd() % 4 == 0 ? in_bytes - (len < in_bytes ? len : in_bytes) : rnd() % (in_bytes + 2);
            if (pick == 15) { off = ~0ull - rnd() % 8; len = 1 + rnd() % 16; }
            if (pick == 14) { off = rnd() % (in_bytes + 1); len = ~0ull - rnd() % 8; }
            st[k] = {off, len};
            const uint64_t dp = rnd() % 10;
            of[k] = dp == 0 ? DMX_BATCH_NODICT : dp == 1 ? nd + (uint32_t)(rnd() % 3) : dp == 2 ? 0xFFFFFFFEu
                    : nd ? (uint32_t)(rnd() % nd) : DMX_BATCH_NODICT;
        }
        check_all(st, in_bytes, sw, dicts, dict_bytes, of, "random");
    }
    printf("%ld checks, %ld failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}

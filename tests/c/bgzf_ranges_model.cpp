// The host twin of the batched range reads (csrc/dmx_bgzf_ranges.hip): the planning stages and the
// gather run as loops over the per-thread text of csrc/dmx_bgzf_ranges.h, with the scan tiles
// shrunk (DMX_BRR_MTILE / DMX_BRR_RTILE / DMX_BRR_STHREADS from the Makefile) so that small inputs
// cross many tile edges, against brute force: every (off, len) of small layouts with empty
// members, every virtual offset of them, broken indexes, and seeded random batches with random
// capacities and alignments of d_out.  The decode is a copy of the member's bytes.  Built with
// ASan + UBSan; prints `<n> failed checks`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dmx_bgzf_ranges.h"

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

// A file of members that dmx_bgzf_step parses (the DEFLATE data is filler: nothing here inflates),
// its decoded bytes, its index (members with data only) and every member's file offset and ISIZE.
struct File {
    std::vector<uint8_t> z, data;
    std::vector<dmx_iblock> idx;
    std::vector<uint32_t> crc;
    std::vector<uint64_t> moff;    // file offset of every member, empty ones included
    std::vector<uint32_t> isize;
};
static File make_file(const std::vector<uint32_t>& sizes, bool names) {
    File f;
    uint64_t o = 0;
    for (size_t k = 0; k < sizes.size(); k++) {
        const uint32_t n = sizes[k];
        const uint32_t xlen = names ? 14 : 6, fill = 2 + (uint32_t)(rnd() % 5);
        std::vector<uint8_t> h = {0x1F, 0x8B, 8, (uint8_t)(names ? 0x0C : 0x04), 0, 0, 0, 0, 0, 0xFF, (uint8_t)xlen, 0};
        if (names) { const uint8_t x[8] = {'X', 'Y', 4, 0, 1, 2, 3, 4}; h.insert(h.end(), x, x + 8); }
        const uint32_t name = names ? 4 : 0;   // "abc\0"
        const uint32_t bsize = 12 + xlen + name + fill + 8;
        const uint8_t bc[6] = {'B', 'C', 2, 0, (uint8_t)((bsize - 1) & 255), (uint8_t)((bsize - 1) >> 8)};
        h.insert(h.end(), bc, bc + 6);
        if (names) { const uint8_t nm[4] = {'a', 'b', 'c', 0}; h.insert(h.end(), nm, nm + 4); }
        const uint32_t body = (uint32_t)h.size();
        for (uint32_t i = 0; i < fill; i++) h.push_back((uint8_t)rnd());
        const uint32_t crc = (uint32_t)rnd();
        for (int i = 0; i < 4; i++) h.push_back((uint8_t)(crc >> (8 * i)));
        for (int i = 0; i < 4; i++) h.push_back((uint8_t)(n >> (8 * i)));
        f.moff.push_back(f.z.size());
        f.isize.push_back(n);
        if (n) {
            dmx_iblock e = {8 * (f.z.size() + body), o, n, 0};
            f.idx.push_back(e);
            f.crc.push_back(crc);
        }
        f.z.insert(f.z.end(), h.begin(), h.end());
        for (uint32_t i = 0; i < n; i++) f.data.push_back((uint8_t)(rnd() | 1));
        o += n;
    }
    return f;
}

struct Run {
    dmx_bgzf_ranges_status rec;
    std::vector<uint64_t> out_off;
    std::vector<uint8_t> outbuf;   // canary 0xA5 | d_out at hd mod 16 | canary
    uint8_t* out;
    uint64_t out_cap;
    dmx_brr_head head;
    std::vector<dmx_iblock> sub;
    std::vector<uint32_t> subcrc;
};

// exclusive scan of mine[0..nth) in place (the workgroup's scan)
template <typename T, typename Op>
static void excl(std::vector<T>& v, Op op) {
    T run = 0;
    for (auto& x : v) { const T c = x; x = run; run = op(run, c); }
}

// dmx_bgzf_read_ranges_async, kernel by kernel
static Run model(const File& f, const std::vector<dmx_iblock>& idx, const std::vector<dmx_brange>& rg, uint32_t flags,
                 uint64_t out_cap, uint32_t max_members, uint64_t scratch_bytes, uint32_t hd, bool with_crc) {
    const uint32_t nblk = (uint32_t)idx.size(), nranges = (uint32_t)rg.size();
    const uint32_t MT = DMX_BRR_MTILE, RT = DMX_BRR_RTILE, ST = DMX_BRR_STHREADS;
    Run R;
    R.out_off.assign(nranges + 1, 0xEEEEEEEEEEEEEEEEull);
    R.outbuf.assign(out_cap + 64, 0xA5);
    R.out = R.outbuf.data() + 16;
    R.out += (16 - ((uintptr_t)R.out & 15)) % 16 + hd;
    R.out_cap = out_cap;
    memset(&R.rec, 0xEE, sizeof(R.rec));
    if (!nranges || !nblk) {   // dmx_brr_empty_kernel
        for (auto& x : R.out_off) x = 0;
        const dmx_bgzf_ranges_status r = {0, 0, 0, 0, DMX_BRR_NOBAD, 0};
        R.rec = r;
        return R;
    }
    const uint32_t mtiles = (nblk + MT - 1) / MT, rtiles = (nranges + RT - 1) / RT;
    std::vector<int32_t> diff(nblk + 1, 0x55555555), dsum(mtiles);
    std::vector<uint32_t> ncnt(mtiles), rm0(nranges), rdelta(nranges);
    std::vector<uint64_t> nlen(mtiles), rsum(rtiles), clen(nranges), moff(nblk, 1ull << 40);
    R.sub.assign(max_members, dmx_iblock{7, 7, 7, 7});
    R.subcrc.assign(max_members, 7);
    std::vector<uint8_t> scratch(scratch_bytes, 0x5A);
    dmx_brr_head& head = R.head;
    // reset
    for (uint32_t i = 0; i <= nblk; i++) diff[i] = 0;
    memset(&head, 0, sizeof(head));
    head.bad = DMX_BRR_NOBAD;
    // plan: a workgroup per range tile
    for (uint32_t t = 0; t < rtiles; t++) {
        uint64_t sum = 0;
        for (uint32_t l = 0; l < RT; l++) {
            const uint64_t q = (uint64_t)t * RT + l;
            if (q < nranges)
                sum = dmx_brr_sat(sum, dmx_brr_plan(f.z.data(), f.z.size(), idx.data(), nblk, rg.data(), (uint32_t)q, flags,
                                                    diff.data(), clen.data(), rm0.data(), rdelta.data(), &head));
        }
        rsum[t] = sum;
    }
    // msum
    for (uint32_t t = 0; t < mtiles; t++) {
        int32_t sum = 0;
        for (uint32_t l = 0; l < MT; l++) {
            const uint64_t m = (uint64_t)t * MT + l;
            if (m < nblk) {
                sum += diff[m];
                if (!dmx_brr_entry_ok(idx.data(), (uint32_t)m)) DMX_BRR_OR(&head.invalid, 1u);
            }
        }
        dsum[t] = sum;
    }
    // scan1
    {
        std::vector<int32_t> dm(ST);
        std::vector<uint64_t> rm(ST);
        for (uint32_t t = 0; t < ST; t++) dm[t] = dmx_brr_chunk_sum(dsum.data(), mtiles, ST, t, dmx_brr_op_add());
        excl(dm, dmx_brr_op_add());
        for (uint32_t t = 0; t < ST; t++) dmx_brr_chunk_apply(dsum.data(), mtiles, ST, t, dm[t], dmx_brr_op_add());
        for (uint32_t t = 0; t < ST; t++) rm[t] = dmx_brr_chunk_sum(rsum.data(), rtiles, ST, t, dmx_brr_op_sat());
        uint64_t tot = 0;
        for (uint32_t t = 0; t < ST; t++) tot = dmx_brr_sat(tot, rm[t]);
        excl(rm, dmx_brr_op_sat());
        for (uint32_t t = 0; t < ST; t++) dmx_brr_chunk_apply(rsum.data(), rtiles, ST, t, rm[t], dmx_brr_op_sat());
        head.out_len = tot;
    }
    // need
    for (uint32_t t = 0; t < mtiles; t++) {
        int32_t before = dsum[t];
        uint32_t cnt = 0;
        uint64_t len = 0;
        for (uint32_t l = 0; l < MT; l++) {
            const uint64_t m = (uint64_t)t * MT + l;
            if (m >= nblk) break;
            const int32_t v = diff[m];
            const uint32_t need = dmx_brr_need(before, v);
            before += v;
            diff[m] = (int32_t)need;
            cnt += need;
            if (need) len += idx[m].out_len;
        }
        ncnt[t] = cnt;
        nlen[t] = len;
    }
    // scan2
    {
        std::vector<uint32_t> cm(ST);
        std::vector<uint64_t> lm(ST);
        uint32_t ctot = 0;
        uint64_t ltot = 0;
        for (uint32_t t = 0; t < ST; t++) ctot += cm[t] = dmx_brr_chunk_sum(ncnt.data(), mtiles, ST, t, dmx_brr_op_add());
        for (uint32_t t = 0; t < ST; t++) ltot += lm[t] = dmx_brr_chunk_sum(nlen.data(), mtiles, ST, t, dmx_brr_op_add());
        excl(cm, dmx_brr_op_add());
        excl(lm, dmx_brr_op_add());
        for (uint32_t t = 0; t < ST; t++) dmx_brr_chunk_apply(ncnt.data(), mtiles, ST, t, cm[t], dmx_brr_op_add());
        for (uint32_t t = 0; t < ST; t++) dmx_brr_chunk_apply(nlen.data(), mtiles, ST, t, lm[t], dmx_brr_op_add());
        dmx_brr_decide(&head, ctot, ltot, max_members, scratch_bytes, out_cap, &R.rec);
    }
    // emit
    const uint32_t count = head.count;
    if (count)
        for (uint32_t t = 0; t < mtiles; t++) {
            uint32_t rank = ncnt[t];
            uint64_t soff = nlen[t];
            for (uint32_t l = 0; l < MT; l++) {
                const uint64_t m = (uint64_t)t * MT + l;
                if (m >= nblk || !diff[m]) continue;
                if (rank < max_members)
                    dmx_brr_emit_member(idx.data(), with_crc ? f.crc.data() : nullptr, (uint32_t)m, rank, soff, R.sub.data(),
                                        R.subcrc.data(), moff.data());
                rank++;
                soff += idx[m].out_len;
            }
        }
    for (uint32_t j = count; j < max_members; j++) dmx_brr_emit_slot(j, R.sub.data(), R.subcrc.data());
    if (R.rec.status == 0 || R.rec.status == -(int32_t)E_SZ) {
        for (uint32_t t = 0; t < rtiles; t++) {
            uint64_t at = rsum[t];
            for (uint32_t l = 0; l < RT; l++) {
                const uint64_t q = (uint64_t)t * RT + l;
                if (q >= nranges) break;
                R.out_off[q] = at;
                at = dmx_brr_sat(at, clen[q]);
            }
        }
        R.out_off[nranges] = head.out_len;
    }
    // decode: the counted kernel, as a copy of the member's bytes (the entry's bit names the member)
    for (uint32_t j = 0; j < count; j++) {
        const uint32_t m = dmx_brr_find_bit(idx.data(), nblk, R.sub[j].bit);
        CHECK(idx[m].bit == R.sub[j].bit && R.sub[j].out_len == idx[m].out_len, "sub-index entry %u", j);
        CHECK(R.sub[j].out_off + R.sub[j].out_len <= scratch_bytes, "sub-index entry %u outside the scratch", j);
        if (with_crc) CHECK(R.subcrc[j] == f.crc[m], "CRC word of entry %u", j);
        memcpy(scratch.data() + R.sub[j].out_off, f.data.data() + idx[m].out_off, idx[m].out_len);
    }
    // gather
    if (!R.rec.status && head.out_len) {
        const uint32_t h16 = (uint32_t)((uintptr_t)R.out & 15);
        const uint64_t ngroups = (h16 + head.out_len + DMX_BRR_GROUP - 1) / DMX_BRR_GROUP;
        for (uint64_t g = 0; g < ngroups; g++)
            dmx_brr_gather_group(g, h16, head.out_len, R.out_off.data(), nranges, rm0.data(), rdelta.data(), moff.data(),
                                 scratch.data(), R.out);
    }
    return R;
}

// brute force: the clipped ranges in bytes, the members they touch
struct Want {
    int32_t status;
    uint32_t bad, nmembers;
    uint64_t out_len, scratch_len;
    std::vector<uint64_t> off, lin, len;
};
static Want brute(const File& f, const std::vector<dmx_brange>& rg, uint32_t flags) {
    Want w;
    const uint64_t total = f.data.size();
    w.status = 0;
    w.bad = DMX_BRR_NOBAD;
    std::vector<uint8_t> touched(total + 1, 0);
    uint64_t at = 0;
    for (size_t q = 0; q < rg.size(); q++) {
        uint64_t off = rg[q].off;
        const uint64_t len = rg[q].len;
        bool bad = false;
        if (flags & DMX_RANGES_VIRTUAL) {
            const uint64_t p = off >> 16, within = off & 0xFFFF;
            bad = true;
            uint64_t o = 0;
            for (size_t k = 0; k < f.moff.size(); k++) {
                if (f.moff[k] == p && f.isize[k] && (within < f.isize[k] || !len)) {
                    bad = false;
                    off = o + within;
                }
                o += f.isize[k];
            }
        }
        if (bad && w.bad == DMX_BRR_NOBAD) w.bad = (uint32_t)q;
        uint64_t c = 0;
        if (!bad && off < total) c = len < total - off ? len : total - off;
        w.off.push_back(at);
        w.lin.push_back(off);
        w.len.push_back(c);
        at = dmx_brr_sat(at, c);
        for (uint64_t b = 0; b < c; b++) touched[off + b] = 1;
    }
    w.off.push_back(at);
    w.out_len = at;
    w.nmembers = 0;
    w.scratch_len = 0;
    for (const auto& e : f.idx) {
        bool any = false;
        for (uint32_t b = 0; b < e.out_len; b++) any |= touched[e.out_off + b] != 0;
        if (any) {
            w.nmembers++;
            w.scratch_len += e.out_len;
        }
    }
    if (w.bad != DMX_BRR_NOBAD) w.status = -(int32_t)E_RANGE;
    return w;
}

static bool canaries(const Run& R, bool untouched) {
    const uint8_t* lo = R.outbuf.data();
    const uint8_t* hi = lo + R.outbuf.size();
    const uint64_t written = untouched ? 0 : R.rec.out_len;
    for (const uint8_t* p = lo; p < hi; p++)
        if ((p < R.out || p >= R.out + written) && *p != 0xA5) return false;
    return true;
}

// one call with room for everything, checked in full; then (squeeze) each capacity one below need
static void check(const File& f, const std::vector<dmx_brange>& rg, uint32_t flags, uint32_t hd, bool squeeze, const char* what) {
    if (f.idx.empty()) {   // nblk == 0: nothing to read, whatever the ranges say
        const Run R = model(f, f.idx, rg, flags, 8, 2, 8, hd, true);
        CHECK(R.rec.status == 0 && R.rec.out_len == 0 && R.rec.nmembers == 0 && R.rec.bad == DMX_BRR_NOBAD, "%s: an empty index", what);
        for (size_t q = 0; q <= rg.size(); q++) CHECK(R.out_off[q] == 0, "%s: an empty index: out_off[%zu]", what, q);
        CHECK(canaries(R, true), "%s: an empty index: d_out written", what);
        return;
    }
    const Want w = brute(f, rg, flags);
    const uint64_t cap = w.status ? 8 : w.out_len, sb = w.status ? 8 : w.scratch_len;
    const uint32_t mm = w.status ? 2 : w.nmembers + (uint32_t)(rnd() % 3);
    const Run R = model(f, f.idx, rg, flags, cap, mm, sb, hd, true);
    CHECK(R.rec.status == w.status, "%s: status %d, want %d", what, R.rec.status, w.status);
    CHECK(R.rec.bad == w.bad, "%s: bad %u, want %u", what, R.rec.bad, w.bad);
    if (w.status) {
        CHECK(canaries(R, true), "%s: d_out written with a status", what);
        return;
    }
    CHECK(R.rec.nmembers == w.nmembers, "%s: nmembers %u, want %u", what, R.rec.nmembers, w.nmembers);
    CHECK(R.rec.out_len == w.out_len, "%s: out_len", what);
    CHECK(R.rec.scratch_len == w.scratch_len, "%s: scratch_len", what);
    CHECK(rg.empty() || R.head.count == w.nmembers, "%s: count", what);
    for (size_t q = 0; q <= rg.size(); q++) CHECK(R.out_off[q] == w.off[q], "%s: out_off[%zu]", what, q);
    for (size_t q = 0; q < rg.size(); q++)
        CHECK(!w.len[q] || !memcmp(R.out + w.off[q], f.data.data() + w.lin[q], w.len[q]), "%s: bytes of range %zu", what, q);
    CHECK(canaries(R, false), "%s: canaries", what);
    for (uint32_t j = R.rec.nmembers; j < mm && !rg.empty(); j++)
        CHECK(R.sub[j].out_len == 0 && R.sub[j].out_off == 0 && R.subcrc[j] == 0, "%s: slot %u", what, j);
    if (!squeeze) return;
    for (int k = 0; k < 3; k++) {
        if ((k == 0 && !w.nmembers) || (k == 1 && !w.scratch_len) || (k == 2 && !w.out_len)) continue;
        const Run S = model(f, f.idx, rg, flags, w.out_len - (k == 2), w.nmembers - (k == 0), w.scratch_len - (k == 1), hd, false);
        CHECK(S.rec.status == -(int32_t)E_SZ, "%s: capacity %d one below need: status %d", what, k, S.rec.status);
        CHECK(S.rec.nmembers == w.nmembers && S.rec.out_len == w.out_len && S.rec.scratch_len == w.scratch_len,
              "%s: capacity %d: the needs", what, k);
        CHECK(S.head.count == 0 && canaries(S, true), "%s: capacity %d: d_out written", what, k);
        for (size_t q = 0; q <= rg.size(); q++) CHECK(S.out_off[q] == w.off[q], "%s: capacity %d: out_off[%zu]", what, k, q);
    }
}

int main(void) {
    const std::vector<std::vector<uint32_t>> layouts = {
        {3, 1, 0, 5, 2, 4, 0}, {0, 0, 2, 0}, {1, 1, 1, 1, 1, 1, 1, 1, 1, 0}, {7}, {0}, {2, 0, 0, 0, 3, 1, 1, 2, 1, 1, 1, 1, 1, 2, 0}};
    for (size_t li = 0; li < layouts.size(); li++)
        for (int names = 0; names < 2; names++) {
            const File f = make_file(layouts[li], names != 0);
            const uint64_t total = f.data.size();
            // every (off, len), one batch and one by one
            std::vector<dmx_brange> all;
            for (uint64_t off = 0; off <= total + 2; off++)
                for (uint64_t len = 0; len <= total + 2; len++) {
                    all.push_back(dmx_brange{off, len});
                    check(f, {dmx_brange{off, len}}, 0, (uint32_t)((off + len) & 15), false, "one range");
                }
            all.push_back(dmx_brange{total, 1ull << 63});
            all.push_back(dmx_brange{1ull << 40, 5});
            all.push_back(dmx_brange{0, ~0ull});
            check(f, all, 0, 3, true, "every range");
            // every virtual offset, good and bad, one by one; then batches with the bad ones in them
            std::vector<dmx_brange> vall;
            for (size_t k = 0; k < f.moff.size(); k++)
                for (uint64_t within = 0; within <= f.isize[k] + 1u; within++)
                    for (uint64_t len = 0; len <= total + 1; len += 1 + len / 3) {
                        for (uint64_t d = 0; d < 2; d++) {
                            const dmx_brange r = {((f.moff[k] + d) << 16) | within, len};
                            check(f, {r}, DMX_RANGES_VIRTUAL, (uint32_t)(within & 15), false, "one virtual offset");
                            vall.push_back(r);
                        }
                    }
            vall.push_back(dmx_brange{(uint64_t)f.z.size() << 16, 1});
            vall.push_back(dmx_brange{~0ull, 1});
            check(f, vall, DMX_RANGES_VIRTUAL, 0, false, "every virtual offset");
            std::vector<dmx_brange> good;
            for (const auto& r : vall)
                if (!brute(f, {r}, DMX_RANGES_VIRTUAL).status) good.push_back(r);
            check(f, good, DMX_RANGES_VIRTUAL, 9, true, "the good virtual offsets");
            // a broken index: -E_INVAL, nothing written
            for (size_t m = 0; m < f.idx.size(); m++)
                for (int how = 0; how < 3; how++) {
                    std::vector<dmx_iblock> ix = f.idx;
                    if (how == 0) ix[m].out_off += 1;
                    if (how == 1) ix[m].out_len = 0;
                    if (how == 2) ix[m].out_len = DMX_BGZF_MAX_ISIZE + 1;
                    const Run R = model(f, ix, all, 0, 1 << 16, (uint32_t)ix.size(), 1 << 12, 0, false);
                    CHECK(R.rec.status == -(int32_t)E_INVAL && R.head.count == 0 && canaries(R, true), "broken index %zu/%d", m, how);
                }
        }
    // seeded random batches
    for (int it = 0; it < 400; it++) {
        std::vector<uint32_t> sizes(1 + rnd() % 40);
        for (auto& s : sizes) s = (uint32_t)(rnd() % 10) * (uint32_t)(rnd() % 4 != 0);
        const File f = make_file(sizes, (it & 1) != 0);
        const uint64_t total = f.data.size();
        std::vector<dmx_brange> rg(rnd() % 40);
        const bool virt = it % 3 == 0 && !f.idx.empty();
        for (auto& r : rg) {
            if (virt) {
                size_t k = rnd() % f.moff.size();
                while (!f.isize[k]) k = (k + 1) % f.moff.size();
                r.off = (f.moff[k] << 16) | (rnd() % f.isize[k]);
            } else {
                r.off = rnd() % (total + 3);
                if (rnd() % 16 == 0) r.off = rnd();
            }
            r.len = rnd() % 8 ? rnd() % 12 : (rnd() % 2 ? rnd() : total);
        }
        check(f, rg, virt ? DMX_RANGES_VIRTUAL : 0, (uint32_t)(rnd() % 16), true, "random batch");
    }
    printf("%ld checks, %ld failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}

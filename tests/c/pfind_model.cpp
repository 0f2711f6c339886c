/*
 * pfind_model.cpp -- the block-start predicate of dmx_inflate_parallel_plan_host (csrc/dmx_pfind.h,
 * written to run one lane per bit offset) under AddressSanitizer + UBSan.  Built by
 * tests/c/Makefile.pfind from this file and dmx_inflate_par_host.cpp; runs without a GPU.  The
 * arguments are files that each hold one stream (zlib, gzip or raw: told by name, a name with
 * "raw" in it is raw).  For every bit offset of every stream:
 *   - dmx_pf_valid agrees with the decoder's accept / reject of a non-final dynamic block header at
 *     that offset, restated here the plain way (arrays and a table build, as dynamic() of
 *     dmx_inflate.c does it: counts per length, Kraft sums, the repeat codes' rules);
 *   - every true start of a non-final dynamic block (the serial walk from the framing) is accepted;
 *   - the offsets that are accepted without being one are counted: the false starts per megabit.
 * The first two streams are also scanned at every cut point (every prefix, an exact-size heap block,
 * so ASan sees a read behind it) and under 10 000 seeded mutations of one to three bytes.  The
 * plan of every stream (dmx_inflate_parallel_plan_host, chunk_bytes 1 024) must start only at true
 * block starts.  Exit status 0 = "0 failed checks" (the sanitizers abort on their own findings).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <vector>

#include "dmx.h"
#include "dmx_gz_head.h"
#include "dmx_pfind.h"

extern "C" int dmx_pf_host_blocks(const uint8_t* z, uint64_t n, uint64_t bit, uint64_t* starts, uint8_t* kinds, uint64_t cap,
                                  uint64_t* nblocks, uint64_t* out_len);

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

// ---- the plain restatement: a bit reader that fails at the end, arrays, a count-based build ----
struct RB {
    const uint8_t* z;
    uint64_t n, pos;
    bool short_;
};
static uint32_t rbits(RB& r, int k) {
    uint32_t v = 0;
    for (int i = 0; i < k; i++, r.pos++) {
        if ((r.pos >> 3) >= r.n) { r.short_ = true; return 0; }
        v |= (uint32_t)((r.z[r.pos >> 3] >> (r.pos & 7)) & 1) << i;
    }
    return v;
}
// 0 complete, > 0 incomplete, < 0 over-subscribed; ncodes = the symbols with a code
static int kraft(const uint8_t* len, int n, int* ncodes, int* ones) {
    int count[16] = {0};
    for (int s = 0; s < n; s++) count[len[s]]++;
    *ncodes = n - count[0];
    *ones = count[1];
    int left = 1;
    for (int l = 1; l <= 15; l++) {
        left = 2 * left - count[l];
        if (left < 0) return left;
    }
    return left;
}
static int cl_decode(RB& r, const uint8_t* cl) {   // canonical, one bit a step (puff's loop)
    int count[8] = {0};
    uint8_t sym[19];
    for (int s = 0; s < 19; s++) count[cl[s]]++;
    count[0] = 0;
    int offs[8] = {0};
    for (int l = 1; l < 7; l++) offs[l + 1] = offs[l] + count[l];
    for (int s = 0; s < 19; s++)
        if (cl[s]) sym[offs[cl[s]]++] = (uint8_t)s;
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 7; l++) {
        code |= (int)rbits(r, 1);
        if (r.short_) return -1;
        if (code - count[l] < first) return sym[index + (code - first)];
        index += count[l];
        first += count[l];
        first <<= 1;
        code <<= 1;
    }
    return -1;
}
static bool ref_valid(const uint8_t* z, uint64_t n, uint64_t bit) {
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    RB r = {z, n, bit, false};
    if (rbits(r, 1) != 0 || rbits(r, 2) != 2 || r.short_) return false;
    const int nlen = (int)rbits(r, 5) + 257, ndist = (int)rbits(r, 5) + 1, ncode = (int)rbits(r, 4) + 4;
    if (r.short_ || nlen > 286 || ndist > 30) return false;
    uint8_t len[320];
    memset(len, 0, sizeof(len));
    for (int k = 0; k < ncode; k++) len[order[k]] = (uint8_t)rbits(r, 3);
    if (r.short_) return false;
    int nc, ones;
    if (kraft(len, 19, &nc, &ones) != 0 || nc == 0) return false;
    uint8_t cl[19];
    memcpy(cl, len, 19);
    int idx = 0;
    while (idx < nlen + ndist) {
        const int sym = cl_decode(r, cl);
        if (sym < 0) return false;
        if (sym < 16) {
            len[idx++] = (uint8_t)sym;
        } else {
            int v = 0, rep;
            if (sym == 16) {
                if (idx == 0) return false;
                v = len[idx - 1];
                rep = 3 + (int)rbits(r, 2);
            } else if (sym == 17) {
                rep = 3 + (int)rbits(r, 3);
            } else {
                rep = 11 + (int)rbits(r, 7);
            }
            if (r.short_ || idx + rep > nlen + ndist) return false;
            while (rep--) len[idx++] = (uint8_t)v;
        }
    }
    if (len[256] == 0) return false;
    int e = kraft(len, nlen, &nc, &ones);
    if (e < 0 || (e > 0 && !(nc == 1 && ones == 1))) return false;
    e = kraft(len + nlen, ndist, &nc, &ones);
    if (e < 0 || (e > 0 && nc != 0 && !(nc == 1 && ones == 1))) return false;
    return true;
}

// every bit offset of an exact-size heap copy of z[0, n): both predicates agree; returns the accepted ones
static long scan(const uint8_t* src, uint64_t n, const char* what, const std::vector<bool>* truth, long* falses) {
    uint8_t* z = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(z, src, n);
    long accepted = 0;
    for (uint64_t bit = 0; bit < 8 * n; bit++) {
        const bool a = dmx_pf_valid(z, n, bit), b = ref_valid(z, n, bit);
        CHECK(a == b, "%s: bit %llu: dmx_pf_valid %d, the restated header %d", what, (unsigned long long)bit, a, b);
        accepted += a;
        if (truth) {
            const bool t = (*truth)[bit];
            CHECK(a || !t, "%s: bit %llu starts a non-final dynamic block and was rejected", what, (unsigned long long)bit);
            if (a && !t) (*falses)++;
        }
    }
    free(z);
    return accepted;
}

int main(int argc, char** argv) {
    std::vector<bytes> streams;
    double mbits = 0;
    long falses = 0, trues = 0;
    for (int i = 1; i < argc; i++) {
        FILE* f = fopen(argv[i], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        bytes b;
        uint8_t buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + k);
        fclose(f);
        const uint32_t fmt = strstr(argv[i], "raw") ? DMX_BATCH_RAW : DMX_BATCH_AUTO;
        uint32_t format = 0;
        uint64_t body = 0;
        CHECK(dmx_frame_head(b.data(), b.size(), fmt, &format, &body) == 0, "%s: framing", argv[i]);
        // the truth: the serial walk's blocks
        std::vector<uint64_t> starts(1 << 20);
        std::vector<uint8_t> kinds(1 << 20);
        uint64_t nb = 0, olen = 0;
        const int r = dmx_pf_host_blocks(b.data(), b.size(), 8 * body, starts.data(), kinds.data(), starts.size(), &nb, &olen);
        CHECK(r == 0 && nb <= starts.size(), "%s: the serial walk: %d", argv[i], r);
        std::vector<bool> truth(8 * b.size() + 1, false);
        std::set<uint64_t> all;
        long nt = 0;
        for (uint64_t j = 0; j < nb && j < starts.size(); j++) {
            all.insert(starts[j]);
            if (kinds[j] == 2) { truth[starts[j]] = true; nt++; }   // BTYPE 2, BFINAL 0
        }
        trues += nt;
        long fs = 0;
        scan(b.data(), b.size(), argv[i], &truth, &fs);
        falses += fs;
        mbits += 8.0 * (double)b.size() / 1e6;
        // the plan starts only at block starts, and tiles the output
        std::vector<dmx_pchunk> ch(b.size() / 1024 + 2);
        dmx_par_status st;
        const int pr = dmx_inflate_parallel_plan_host(b.data(), b.size(), fmt, 1024, ch.data(), (uint32_t)ch.size(), &st);
        CHECK(pr == 0 && st.status == 0 && st.out_len == olen, "%s: plan %d status %d", argv[i], pr, st.status);
        for (uint32_t j = 0; pr == 0 && j < st.nlive; j++)
            CHECK(all.count(ch[j].bit) != 0, "%s: chunk %u starts at bit %llu, no block start", argv[i], j, (unsigned long long)ch[j].bit);
        printf("%s: %zu bytes, %llu blocks (%zu non-final dynamic), %ld false starts, plan: %u chunks, %u candidates, %u live\n", argv[i],
               b.size(), (unsigned long long)nb, (size_t)nt, fs, st.nchunks, st.ncand, st.nlive);
        if (streams.size() < 2) {   // two small ones for the cuts and the mutations
            const size_t n = b.size() < 700 ? b.size() : 700;
            streams.push_back(bytes(b.begin(), b.begin() + (long)n));
        }
    }
    for (const bytes& s : streams)
        for (size_t k = 0; k <= s.size(); k++) scan(s.data(), k, "cut", NULL, NULL);
    for (int m = 0; m < 10000 && !streams.empty(); m++) {
        bytes s = streams[rnd((uint32_t)streams.size())];
        const uint32_t nm = 1 + rnd(3);
        for (uint32_t j = 0; j < nm && !s.empty(); j++) s[rnd((uint32_t)s.size())] = (uint8_t)rnd(256);
        if (rnd(3) == 0 && !s.empty()) s.resize(rnd((uint32_t)s.size()) + 1);
        scan(s.data(), s.size(), "mutation", NULL, NULL);
    }
    printf("%.2f megabits scanned, %ld true starts, %ld fully valid false starts: %.3f per megabit\n", mbits, trues, falses,
           mbits > 0 ? (double)falses / mbits : 0.0);
    printf("%ld checks, %d failed checks\n", checks, fails);
    return fails ? 1 : 0;
}

// pmulti_model.cpp -- the host plan of one file of many gzip members under ASan + UBSan
// (dmx_inflate_parallel_multi_plan_host: csrc/dmx_pfind.h, csrc/dmx_gz_head.h,
// csrc/dmx_inflate_par_host.cpp) and the member-bounded pack and tail rules of csrc/dmx_ptail.h, in
// a stand-alone program.  Usage: pmulti_model file... [-t file...]: every file is planned at
// chunk_bytes 1024 and 4096 and the plan checked: the two-call idiom, the chunks and the members
// tile the output, every member on its own (its header, a serial walk over its blocks:
// dmx_pf_host_blocks) gives the table's numbers; the files behind -t also at every truncation.
// Ends with "<n> checks, <m> failed checks"; exit status 1 where m > 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dmx.h"
#include "dmx_gz_head.h"
#include "dmx_pfind.h"
#include "dmx_ptail.h"

extern "C" int dmx_pf_host_blocks(const uint8_t* z, uint64_t n, uint64_t bit, uint64_t* starts, uint8_t* kinds, uint64_t cap,
                                  uint64_t* nblocks, uint64_t* out_len);

static uint64_t g_checks, g_failed;
#define CHECK(c, ...)                                  \
    do {                                               \
        g_checks++;                                    \
        if (!(c)) {                                    \
            g_failed++;                                \
            if (g_failed < 20) {                       \
                printf("FAILED %s: ", #c);             \
                printf(__VA_ARGS__);                   \
                printf("\n");                          \
            }                                          \
        }                                              \
    } while (0)

static void check_plan(const char* name, const uint8_t* z, uint64_t n, uint32_t chunk) {
    dmx_par_multi_status ms;
    int r = dmx_inflate_parallel_multi_plan_host(z, n, DMX_BATCH_GZIP, chunk, NULL, 0, NULL, 0, &ms);
    CHECK(r == 0 || r == -(int)E_SZ, "%s: first call %d", name, r);
    if (r != -(int)E_SZ) {
        CHECK(ms.st.status != 0 || (ms.st.nlive == 0 && ms.nmembers == 0), "%s: a clean plan without chunks", name);
        return;
    }
    std::vector<dmx_pchunk> ch(ms.st.nlive);
    std::vector<dmx_pmember> mem(ms.nmembers ? ms.nmembers : 1);
    // one record short on either side: -E_SZ, nothing written behind the capacity
    if (ms.st.nlive > 1) {
        dmx_par_multi_status m2;
        std::vector<dmx_pchunk> c2(ms.st.nlive - 1);
        CHECK(dmx_inflate_parallel_multi_plan_host(z, n, DMX_BATCH_GZIP, chunk, c2.data(), ms.st.nlive - 1, mem.data(),
                                                   ms.nmembers, &m2) == -(int)E_SZ,
              "%s: a chunk short", name);
    }
    if (ms.nmembers > 1) {
        dmx_par_multi_status m2;
        std::vector<dmx_pmember> e2(ms.nmembers - 1);
        CHECK(dmx_inflate_parallel_multi_plan_host(z, n, DMX_BATCH_GZIP, chunk, ch.data(), ms.st.nlive, e2.data(),
                                                   ms.nmembers - 1, &m2) == -(int)E_SZ,
              "%s: a member short", name);
    }
    dmx_par_multi_status st;
    r = dmx_inflate_parallel_multi_plan_host(z, n, DMX_BATCH_GZIP, chunk, ch.data(), ms.st.nlive, mem.data(), ms.nmembers, &st);
    CHECK(r == 0, "%s: second call %d", name, r);
    CHECK(memcmp(&st, &ms, sizeof(st)) == 0, "%s: the record differs between the calls", name);
    if (st.st.status) {
        CHECK(st.st.out_len == 0 && st.st.in_used == 0 && st.nmembers == 0, "%s: numbers behind a status", name);
        return;
    }
    CHECK(st.st.in_used <= n && st.st.in_used >= 18 && st.nmembers >= 1 && st.bad_member == 0xFFFFFFFFu, "%s: record", name);
    CHECK(st.st.work_len == dmx_pf_mwork(st.st.out_len, st.st.nlive, st.nmembers), "%s: work_len", name);
    uint64_t off = 0;
    for (uint32_t k = 0; k < st.st.nlive; k++) {
        CHECK(ch[k].out_off == off && ch[k].bit < ch[k].end_bit && ch[k].end_bit <= 8 * n, "%s: chunk %u", name, k);
        if (k + 1 < st.st.nlive) CHECK(ch[k + 1].bit == ch[k].end_bit, "%s: chunk %u does not end where %u begins", name, k, k + 1);
        off += ch[k].out_len;
    }
    CHECK(ch[0].bit == 0 && off == st.st.out_len, "%s: the chunks tile the output", name);
    off = 0;
    for (uint32_t m = 0; m < st.nmembers; m++) {
        CHECK(mem[m].out_off == off && mem[m].in_off + 18 <= n && z[mem[m].in_off] == 0x1F && z[mem[m].in_off + 1] == 0x8B,
              "%s: member %u", name, m);
        if (m) CHECK(mem[m].in_off >= mem[m - 1].in_off + 18, "%s: member %u's in_off", name, m);
        // the member on its own: its header, and its blocks give out_len
        uint64_t body = 0, start = 0, nb = 0, out = 0;
        uint8_t kind = 0;
        CHECK(dmx_gz_head(z + mem[m].in_off, n - mem[m].in_off, &body) == 0, "%s: member %u's header", name, m);
        CHECK(dmx_pf_host_blocks(z, n, 8 * (mem[m].in_off + body), &start, &kind, 1, &nb, &out) == 0 && out == mem[m].out_len,
              "%s: member %u's blocks", name, m);
        off += mem[m].out_len;
    }
    CHECK(off == st.st.out_len && mem[st.nmembers - 1].crc == st.st.check, "%s: the members tile the output", name);
}

// the member-bounded rules: a chunk at chunk_off whose member began `limit` bytes in front of it
static void check_rules() {
    std::vector<uint16_t> cells(70000);
    for (size_t k = 0; k < cells.size(); k++) cells[k] = (uint16_t)(k * 7 & 0xFF);
    std::vector<uint8_t> window(DMX_PT_WIN);
    const uint64_t chunk_off = 40000;
    for (uint32_t k = 0; k < DMX_PT_WIN; k++) window[k] = (uint8_t)cells[chunk_off - DMX_PT_WIN + k];
    const uint64_t limits[] = {0, 1, 2, 100, 32767, 32768, 40000};
    for (uint64_t limit : limits) {
        for (uint32_t b = 1; b <= 33000; b += (b < 200 || (b > 32700 && b < 32800)) ? 1 : 97) {
            const uint16_t ref = (uint16_t)dmx_pt_ref(b);
            if (dmx_pt_ref(b) > 0xFFFF) break;
            cells[chunk_off + 5] = ref;
            const int v = dmx_pt_pack_lim(cells.data(), chunk_off + 5, chunk_off, limit);
            const int w = dmx_pt_cell(ref, window.data(), limit);
            if (b <= limit && b <= DMX_PT_WIN) {
                CHECK(v == cells[chunk_off - b] && w == cells[chunk_off - b], "rule: limit %llu back %u: %d %d",
                      (unsigned long long)limit, b, v, w);
            } else if (b > limit) {
                CHECK(v == -1 && w == -1, "rule: limit %llu back %u passes: %d %d", (unsigned long long)limit, b, v, w);
            } else {
                CHECK(w == -1, "rule: beyond the window %u: %d", b, w);
            }
            CHECK(dmx_pt_pack_lim(cells.data(), chunk_off + 4, chunk_off, limit) == cells[chunk_off + 4], "rule: a byte cell");
        }
    }
    // limit = chunk_off: the single stream's rule
    for (uint32_t b = 1; b <= 300; b++) {
        cells[chunk_off + 5] = (uint16_t)dmx_pt_ref(b);
        CHECK(dmx_pt_pack_lim(cells.data(), chunk_off + 5, chunk_off, chunk_off) == dmx_pt_pack(cells.data(), chunk_off + 5, chunk_off),
              "rule: limit = chunk_off");
    }
}

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        printf("cannot read %s\n", path);
        exit(2);
    }
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    bool trunc = false;
    check_rules();
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "-t")) {
            trunc = true;
            continue;
        }
        const std::vector<uint8_t> z = slurp(argv[a]);
        check_plan(argv[a], z.data(), z.size(), 1024);
        check_plan(argv[a], z.data(), z.size(), 4096);
        if (!trunc) continue;
        for (uint64_t n = 0; n < z.size(); n++) {
            // a copy of exactly n bytes: a read past the cut is a read past the allocation
            std::vector<uint8_t> c(z.begin(), z.begin() + n);
            check_plan(argv[a], c.data(), n, 1024);
        }
    }
    // argument errors
    dmx_par_multi_status st;
    dmx_pchunk c1;
    dmx_pmember m1;
    const uint8_t two[2] = {0x1F, 0x8B};
    CHECK(dmx_inflate_parallel_multi_plan_host(two, 2, DMX_BATCH_ZLIB, 0, &c1, 1, &m1, 1, &st) == -(int)E_INVAL, "fmt zlib");
    CHECK(dmx_inflate_parallel_multi_plan_host(two, 2, DMX_BATCH_RAW, 0, &c1, 1, &m1, 1, &st) == -(int)E_INVAL, "fmt raw");
    CHECK(dmx_inflate_parallel_multi_plan_host(two, 2, DMX_BATCH_AUTO, 0, &c1, 1, NULL, 1, &st) == -(int)E_INVAL, "members NULL");
    CHECK(dmx_inflate_parallel_multi_plan_host(two, 2, DMX_BATCH_AUTO, 0, &c1, 1, &m1, 1, NULL) == -(int)E_INVAL, "st NULL");
    CHECK(dmx_inflate_parallel_multi_plan_host(two, 2, DMX_BATCH_AUTO, 0, &c1, 1, &m1, 1, &st) == 0 && st.st.status == -(int)E_ZHEAD,
          "a header cut short");
    const uint8_t zl[2] = {0x78, 0x9C};
    CHECK(dmx_inflate_parallel_multi_plan_host(zl, 2, DMX_BATCH_AUTO, 0, &c1, 1, &m1, 1, &st) == 0 && st.st.status == -(int)E_ZHEAD,
          "no gzip under AUTO");
    CHECK(dmx_inflate_parallel_multi_plan_host(zl, 2, DMX_BATCH_GZIP, 0, &c1, 1, &m1, 1, &st) == 0 && st.st.status == -(int)E_ZHEAD,
          "no gzip under GZIP");
    printf("%llu checks, %llu failed checks\n", (unsigned long long)g_checks, (unsigned long long)g_failed);
    return g_failed ? 1 : 0;
}

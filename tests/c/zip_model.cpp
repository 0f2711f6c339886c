// zip_model.cpp -- the host twin of the device ZIP index: the stages of csrc/dmx_zip_dev.hip run as
// loops over csrc/dmx_zip.h (the text the kernel threads run) against dmx_zip_index_host, in a
// stand-alone program under ASan + UBSan.  Host code only.
//   zip_model FILE...          every file: the model and the host walk agree on record and entries,
//                              at every alignment of the buffer 0..15 and with a candidate buffer
//                              that is too small
//   zip_model --mutate FILE... also every truncation length, and every single byte of the central
//                              directory and the end records set to 00 and FF
// Every buffer is an exact-size heap copy, so a read outside z[0, zbytes) is an ASan report.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dmx.h"
#include "dmx_zip.h"

static long g_fail = 0, g_checks = 0;

#define TILE_GROUPS 1024u

// The device index as loops.  `head`: the alignment the buffer pretends to have (the group loads
// are built from the file's own bytes, zeros where the file has none).
static void model(const uint8_t* z, uint64_t zbytes, uint32_t head, uint32_t max_cand, uint32_t cap, dmx_zip_entry* entries,
                  dmx_zip_status* st) {
    // 1. tail: every position of the window is tested; the last match wins
    uint64_t eocd = ~0ull;
    if (zbytes <= DMX_ZIP_MAXZ) {
        uint32_t best = 0;
        if (zbytes >= 4)
            for (uint64_t p = dmx_zip_tail_lo(zbytes); p + 4 <= zbytes; p++)
                if (dmx_zip_end_sig(z, p)) best = std::max(best, (uint32_t)p + 1);
        if (dmx_zip_end_fast(z, zbytes)) eocd = zbytes - DMX_ZIP_EOCD;
        else if (best) eocd = best - 1;
    }
    dmx_zip_tail t;
    dmx_zip_end_parse(z, zbytes, eocd, &t);
    dmx_zip_status r = {t.status, 0, 0, t.cd_begin, t.cd_end - t.cd_begin, 0, 0};
    int32_t status = t.status;
    // 2. count + write: the groups of the directory
    std::vector<dmx_zip_cand> cand;
    if (!status && t.cd_end - t.cd_begin >= DMX_ZIP_CDH) {
        const uint64_t ngroups = (head + zbytes + DMX_ZIP_GROUP - 1) / DMX_ZIP_GROUP;
        const uint64_t g0 = (head + t.cd_begin) / DMX_ZIP_GROUP, g1 = (head + t.cd_end - 1) / DMX_ZIP_GROUP + 1;
        for (uint64_t g = g0; g < g1 && g < ngroups; g++) {
            uint32_t w[5] = {0, 0, 0, 0, 0};
            for (uint32_t b = 0; b < 20; b++) {
                const uint64_t a = g * DMX_ZIP_GROUP + b;
                if (b >= 16 && g + 1 >= ngroups) break;
                if (a >= head && a - head < zbytes) w[b / 4] |= (uint32_t)z[a - head] << (8 * (b & 3));
            }
            dmx_zip_cand tmp[DMX_ZIP_GROUP];
            const uint32_t c = dmx_zip_group(z, t.cd_begin, t.cd_end, head, g, w, nullptr, 0);
            const uint32_t c2 = dmx_zip_group(z, t.cd_begin, t.cd_end, head, g, w, tmp, DMX_ZIP_GROUP);
            g_checks++;
            if (c != c2) g_fail++;
            for (uint32_t k = 0; k < c; k++) cand.push_back(tmp[k]);
        }
    }
    // 3. plan
    const uint32_t total = (uint32_t)cand.size();
    uint32_t n = total;
    if (status) n = 0;
    else if (!t.nentries) {
        if (t.cd_begin != t.cd_end) status = -(int)E_LEN;
        n = 0;
    } else if (t.cd_begin == t.cd_end || !dmx_zip_cd_step(z, t.cd_end, t.cd_begin)) {
        status = -(int)E_LEN;
        n = 0;
    } else if (total > max_cand) {
        status = -(int)E_SZ;
        n = 0;
    }
    uint32_t ok = 0;
    unsigned long long out_len = 0;
    if (n) {
        // 4. link, 5. rounds
        cand.resize(n + 1);
        std::vector<dmx_zip_node> a(n + 1), b(n + 1);
        std::vector<dmx_zip_mark> mark(n + 1);
        for (uint32_t i = n + 1; i-- > 0;) dmx_zip_link(t.cd_begin, t.cd_end, cand.data(), n, i, a.data(), mark.data());
        const uint64_t bound = std::min<uint64_t>(n, zbytes / DMX_ZIP_CDH + 1);
        uint32_t rounds = 0;
        while ((1ull << rounds) < bound + 1) rounds++;
        for (uint32_t k = 0; k < rounds; k++) {
            for (uint32_t i = n + 1; i-- > 0;) dmx_zip_round(a.data(), b.data(), mark.data(), n, i, k);   // (any order)
            a.swap(b);
        }
        // 6. decide
        uint32_t answers = 0;
        for (uint32_t i = 0; i < n; i++) {
            const int v = dmx_zip_decide(cand.data(), mark.data(), i, t.nentries);
            if (v) answers++;
            if (v > 0) ok = 1;
            else if (v < 0) status = -(int)E_LEN;
        }
        g_checks++;
        if (answers != 1) g_fail++;
        // 7. finish
        if (ok)
            for (uint32_t i = 0; i < n; i++) {
                if (!mark[i].round) continue;
                dmx_zip_entry e;
                dmx_zip_finish(z, zbytes, t.concat, cand[i].off, &e);
                out_len += dmx_zip_len(&e);
                if (mark[i].c < cap) entries[mark[i].c] = e;
            }
    }
    // 8. scan and record
    r.status = status;
    if (ok) {
        const uint32_t count = std::min(t.nentries, cap);
        uint64_t run = 0;
        for (uint32_t i = 0; i < count; i++) {
            entries[i].out_off = run;
            run += dmx_zip_len(&entries[i]);
        }
        r.nentries = t.nentries;
        r.out_len = out_len;
        if (t.nentries > cap) r.status = -(int)E_SZ;
    } else if (!status && t.nentries) {
        r.status = -(int)E_LEN;
    } else if (status == -(int)E_SZ) {
        r.ncand = total;
    }
    *st = r;
}

static bool compare(const uint8_t* src, uint64_t zbytes, uint32_t head, const char* what, long tag) {
    uint8_t* z = zbytes ? (uint8_t*)malloc(zbytes) : nullptr;   // exact size: ASan sees every byte outside
    if (zbytes) memcpy(z, src, zbytes);
    dmx_zip_status hs, ms;
    memset(&hs, 0xEE, sizeof hs);
    memset(&ms, 0xEE, sizeof ms);
    int r = dmx_zip_index_host(z, zbytes, nullptr, 0, &hs);
    const uint32_t cap = hs.nentries;
    std::vector<dmx_zip_entry> he(cap + 1), me(cap + 1);
    memset(he.data(), 0, (cap + 1) * sizeof(dmx_zip_entry));
    memset(me.data(), 0, (cap + 1) * sizeof(dmx_zip_entry));
    r |= dmx_zip_index_host(z, zbytes, he.data(), cap, &hs);
    model(z, zbytes, head, (uint32_t)(zbytes / 4 + 1), cap, me.data(), &ms);
    bool good = r == 0 && !memcmp(&hs, &ms, sizeof hs) && !memcmp(he.data(), me.data(), (cap + 1) * sizeof(dmx_zip_entry));
    g_checks++;
    if (!good) {
        g_fail++;
        if (g_fail < 20)
            printf("MISMATCH %s %ld head %u: host status %d n %u out %llu, model status %d n %u out %llu\n", what, tag, head,
                   hs.status, hs.nentries, (unsigned long long)hs.out_len, ms.status, ms.nentries, (unsigned long long)ms.out_len);
    }
    free(z);
    return good;
}

int main(int argc, char** argv) {
    bool mutate = false;
    for (int a = 1; a < argc; a++) {
        if (!strcmp(argv[a], "--mutate")) {
            mutate = true;
            continue;
        }
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            printf("cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> buf;
        uint8_t tmp[65536];
        size_t got;
        while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
        fclose(f);
        const uint64_t n = buf.size();
        for (uint32_t head = 0; head < 16; head++) compare(buf.data(), n, head, "file", 0);
        // a candidate buffer that is too small, and too few entries: the model alone, against the contract
        {
            dmx_zip_status hs, ms;
            dmx_zip_index_host(buf.data(), n, nullptr, 0, &hs);
            if (!hs.status || hs.status == -(int)E_SZ) {
                std::vector<dmx_zip_entry> he(hs.nentries + 1), me(hs.nentries + 1);
                if (hs.nentries > 1) {
                    const uint32_t cap = hs.nentries / 2;
                    memset(he.data(), 0, he.size() * sizeof(dmx_zip_entry));
                    memset(me.data(), 0, me.size() * sizeof(dmx_zip_entry));
                    dmx_zip_index_host(buf.data(), n, he.data(), cap, &hs);
                    model(buf.data(), n, 3, (uint32_t)(n / 4 + 1), cap, me.data(), &ms);
                    g_checks++;
                    if (hs.status != -(int)E_SZ || memcmp(&hs, &ms, sizeof hs) || memcmp(he.data(), me.data(), he.size() * sizeof(dmx_zip_entry)))
                        g_fail++, printf("MISMATCH small cap %s\n", argv[a]);
                    model(buf.data(), n, 5, hs.nentries - 1, hs.nentries, me.data(), &ms);
                    g_checks++;
                    if (ms.status != -(int)E_SZ || ms.nentries != 0 || ms.ncand < hs.nentries) g_fail++, printf("MISMATCH small work %s\n", argv[a]);
                }
            }
        }
        if (mutate) {
            for (uint64_t len = 0; len < n; len++) compare(buf.data(), len, (uint32_t)(len & 15), "truncation", (long)len);
            dmx_zip_status hs;
            dmx_zip_index_host(buf.data(), n, nullptr, 0, &hs);
            const uint64_t from = hs.status && hs.status != -(int)E_SZ ? (n > 200 ? n - 200 : 0) : hs.cd_off;
            for (uint64_t p = from; p < n; p++)
                for (int v = 0; v < 2; v++) {
                    const uint8_t keep = buf[p];
                    buf[p] = v ? 0xFF : 0x00;
                    if (buf[p] != keep) compare(buf.data(), n, (uint32_t)(p & 15), v ? "byte=FF" : "byte=00", (long)p);
                    buf[p] = keep;
                }
        }
    }
    printf("%ld checks, %ld failed checks\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}

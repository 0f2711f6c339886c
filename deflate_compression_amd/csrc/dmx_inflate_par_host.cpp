// dmx_inflate_par_host.cpp -- one foreign stream cut at true block starts, on the host
// (include/dmx.h: dmx_inflate_parallel_plan_host; DESIGN.md 3.1 "One foreign stream").  No GPU, no
// HIP call.  The search for candidates, the landing rule and the walk over the live chunks are
// dmx_pfind.h's, the framing dmx_gz_head.h's; the measure pass's block decode is here: lengths
// only, from any bit, with the statuses of dmx_inflate.c as the device's reader reports them
// (zeros past the end, and the end of the input folded in afterwards: ib_status).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dmx.h"
#include "dmx_gz_head.h"
#include "dmx_pfind.h"
#include "dmx_zsel.h"

namespace {

struct HB {   // a reader at a bit position; bits past the input read as zeros
    const uint8_t* z;
    uint64_t n, pos;
};
inline uint32_t hb_peek(const HB& s) { return (uint32_t)dmx_pf_peek(s.z, s.n, s.pos); }
inline uint32_t hb_bits(HB& s, uint32_t k) {   // k <= 16
    const uint32_t v = hb_peek(s) & ((1u << k) - 1);
    s.pos += k;
    return v;
}

#define HT_FAST 10
struct HT {
    uint16_t count[16];
    uint16_t symbol[320];
    uint16_t fast[1 << HT_FAST];   // len << 12 | symbol; 0: the slow path
};

// a canonical decoder from code lengths: 0 complete, > 0 incomplete, < 0 over-subscribed
int ht_build(HT& h, const uint8_t* len, int n) {
    memset(h.count, 0, sizeof(h.count));
    memset(h.fast, 0, sizeof(h.fast));
    for (int s = 0; s < n; s++) h.count[len[s]]++;
    if (h.count[0] == n) {
        h.count[0] = 0;
        return 0;   // no codes: every lookup fails
    }
    h.count[0] = 0;
    int left = 1;
    for (int l = 1; l <= 15; l++) {
        left = 2 * left - h.count[l];
        if (left < 0) return left;
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (int s = 0; s < n; s++)
        if (len[s]) h.symbol[offs[len[s]]++] = (uint16_t)s;
    int code = 0, idx = 0;
    for (int l = 1; l <= HT_FAST; l++) {
        for (int k = 0; k < h.count[l]; k++, code++, idx++) {
            int r = 0;
            for (int b = 0; b < l; b++) r |= ((code >> b) & 1) << (l - 1 - b);
            for (int fill = r; fill < (1 << HT_FAST); fill += 1 << l) h.fast[fill] = (uint16_t)((l << 12) | h.symbol[idx]);
        }
        code <<= 1;
    }
    return left;
}
// the symbol at the reader, or -1 where the bits are no code (nothing is consumed then)
int ht_decode(HB& s, const HT& h) {
    const uint32_t v = hb_peek(s);
    const uint16_t e = h.fast[v & ((1u << HT_FAST) - 1)];
    if (e) {
        s.pos += e >> 12;
        return e & 0xFFF;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; l++) {
        code |= (int)((v >> (l - 1)) & 1);
        const int count = h.count[l];
        if (code - count < first) {
            s.pos += (uint64_t)l;
            return h.symbol[index + (code - first)];
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

const uint16_t k_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t k_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint8_t k_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
const uint8_t k_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// One block at the reader: *out grows by the bytes it produces, *last = BFINAL.  0 or -E_*, before
// the end of the input is folded in (hb_status).
int hb_block(HB& s, uint64_t* out, bool* last, uint64_t cap) {   // cap: -E_SZ once *out would pass it (as iblock's capacity)
    *last = hb_bits(s, 1) != 0;
    const uint32_t type = hb_bits(s, 2);
    if (type == 0) {
        s.pos = (s.pos + 7) & ~7ull;
        const uint32_t len = hb_bits(s, 16), nlen = hb_bits(s, 16);
        if (len != (~nlen & 0xFFFFu)) return -(int)E_ZNLEN;
        if (len > cap - *out) return -(int)E_SZ;
        if (s.pos / 8 + len > s.n) return -(int)E_LEN;
        s.pos += 8ull * len;
        *out += len;
        return 0;
    }
    if (type == 3) return -(int)E_ZBTYPE;
    uint8_t len[320];
    int nlen = 288, ndist = 30;
    HT lh, dh;
    if (type == 1) {
        for (int k = 0; k < 288; k++) len[k] = (uint8_t)(k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : 8);
        for (int k = 0; k < 30; k++) len[288 + k] = 5;
    } else {
        nlen = (int)hb_bits(s, 5) + 257;
        ndist = (int)hb_bits(s, 5) + 1;
        const int ncode = (int)hb_bits(s, 4) + 4;
        if (nlen > 286 || ndist > 30) return -(int)E_ZINV;
        memset(len, 0, sizeof(len));
        for (int k = 0; k < ncode; k++) len[k_order[k]] = (uint8_t)hb_bits(s, 3);
        int nz = 0;
        for (int k = 0; k < 19; k++) nz += len[k] != 0;
        if (ht_build(lh, len, 19) != 0 || nz == 0) return -(int)E_HUFAMB;
        int idx = 0;
        while (idx < nlen + ndist) {
            const int sym = ht_decode(s, lh);
            if (sym < 0) return -(int)E_HUFINV;
            if (sym < 16) {
                len[idx++] = (uint8_t)sym;
            } else {
                int v = 0, rep;
                if (sym == 16) {
                    if (idx == 0) return -(int)E_ZINV;
                    v = len[idx - 1];
                    rep = 3 + (int)hb_bits(s, 2);
                } else if (sym == 17) {
                    rep = 3 + (int)hb_bits(s, 3);
                } else {
                    rep = 11 + (int)hb_bits(s, 7);
                }
                if (idx + rep > nlen + ndist) return -(int)E_ZINV;
                while (rep--) len[idx++] = (uint8_t)v;
            }
        }
        if (len[256] == 0) return -(int)E_ZINV;
    }
    int nl = 0, nd = 0;
    for (int k = 0; k < nlen; k++) nl += len[k] != 0;
    for (int k = 0; k < ndist; k++) nd += len[nlen + k] != 0;
    int e = ht_build(lh, len, nlen);
    if (e < 0 || (e > 0 && type == 2 && !(nl == 1 && lh.count[1] == 1))) return -(int)E_HUFAMB;
    e = ht_build(dh, len + nlen, ndist);
    if (e < 0 || (e > 0 && type == 2 && !(nd == 1 && dh.count[1] == 1))) return -(int)E_HUFAMB;
    for (;;) {
        int sym = ht_decode(s, lh);
        if (sym < 0) return -(int)E_HUFINV;
        if (sym < 256) {
            if (*out >= cap) return -(int)E_SZ;
            *out += 1;
        } else if (sym == 256) {
            return 0;
        } else {
            sym -= 257;
            if (sym >= 29) return -(int)E_HUFVAL;
            const uint32_t l = k_lbase[sym] + hb_bits(s, k_lext[sym]);
            const int ds = ht_decode(s, dh);
            if (ds < 0) return -(int)E_HUFINV;
            if (ds >= 30) return -(int)E_HUFVAL;
            s.pos += k_dext[ds];
            if (l > cap - *out) return -(int)E_SZ;
            *out += l;
        }
        if (s.pos > 8 * s.n + 64) return -(int)E_LEN;   // far behind the input: zeros decode for ever otherwise
    }
}
// as ib_status: input that ended before the block did is -E_LEN whatever the zeros decoded to
int hb_status(const HB& s, int err) {
    if (s.pos > 8 * s.n) return -(int)E_LEN;
    if (err == -(int)E_HUFINV && s.pos + 15 > 8 * s.n) return -(int)E_LEN;
    return err;
}

// the measure pass of chunk k
dmx_pf_meas measure(const uint8_t* z, uint64_t n, const uint64_t* cand, uint32_t nc, uint32_t k) {
    const uint64_t max_out = DMX_PF_MAX_CHUNK_OUT;
    HB s = {z, n, cand[k]};
    dmx_pf_meas m;
    memset(&m, 0, sizeof(m));
    m.next = 0xFFFFFFFFu;
    uint32_t t = k + 1, skipped = 0;
    for (;;) {
        bool last = false;
        m.status = hb_status(s, hb_block(s, &m.out_len, &last, max_out + 1));
        if (m.status == -(int)E_SZ || (!m.status && m.out_len > max_out)) {   // too much for one chunk
            m.status = 0;
            m.flags = DMX_PF_LOST;
            break;
        }
        if (m.status) break;
        if (last) {
            m.flags = DMX_PF_LAST;
            break;
        }
        const int ld = dmx_pf_land(cand, nc, &t, s.pos, &skipped);
        if (ld == 1) {
            m.next = t;
            break;
        }
        if (ld == 2) {
            m.flags = DMX_PF_LOST;
            break;
        }
    }
    m.end_bit = s.pos;
    return m;
}

// What a multi-member walk tells the host plan about the members it meets (the device's cell pass
// writes the same table): begin and end events in file order, offsets inside the walk.
struct MemberSink {
    dmx_pmember* m;
    uint32_t cap, n;    // n: members begun so far
    uint64_t off;       // the output offset of the walk's chunk
    void begin(uint64_t in_off, uint64_t local) {
        if (n < cap) {
            m[n].in_off = in_off;
            m[n].out_off = off + local;
            m[n].out_len = 0;
            m[n].crc = m[n].isize = 0;
        }
        n++;
    }
    void end(uint64_t local, uint32_t crc, uint32_t isize) {   // of the member begun last
        if (n == 0 || n > cap) return;
        m[n - 1].out_len = off + local - m[n - 1].out_off;
        m[n - 1].crc = crc;
        m[n - 1].isize = isize;
    }
};

// the measure pass of chunk k of a file of members: over BFINAL, the trailer and the next header,
// standing at the member's first byte and at its first block (dmx_pfind.h)
dmx_pf_meas measure_multi(const uint8_t* z, uint64_t n, const uint64_t* cand, uint32_t nc, uint32_t k, uint64_t* mloc,
                          MemberSink& sink) {
    const uint64_t max_out = DMX_PF_MAX_CHUNK_OUT;
    HB s = {z, n, cand[k]};
    dmx_pf_meas m;
    memset(&m, 0, sizeof(m));
    m.next = 0xFFFFFFFFu;
    uint32_t t = k + 1, skipped = 0, first = DMX_PF_NOMEM, lastm = DMX_PF_NOMEM;
    bool open = false;   // a landing is due before the next block
    if (dmx_pf_at_member(z, s.pos)) {
        uint64_t body = 0;
        m.status = dmx_gz_head(z + (s.pos >> 3), n - (s.pos >> 3), &body);
        if (!m.status) {
            sink.begin(s.pos >> 3, 0);
            m.reserved = 1;
            first = lastm = 0;
            s.pos += 8 * body;
            open = true;
        }
    }
    while (!m.status) {
        if (open) {
            const int ld = dmx_pf_land(cand, nc, &t, s.pos, &skipped);
            if (ld == 1) { m.next = t; break; }
            if (ld == 2) { m.flags = DMX_PF_LOST; break; }
            open = false;
        }
        bool last = false;
        m.status = hb_status(s, hb_block(s, &m.out_len, &last, max_out + 1));
        if (m.status == -(int)E_SZ || (!m.status && m.out_len > max_out)) {   // too much for one chunk
            m.status = 0;
            m.flags = DMX_PF_LOST;
            break;
        }
        if (m.status) break;
        open = true;
        if (!last) continue;
        uint64_t q, body;
        uint32_t crc, isize;
        const int r = dmx_pf_member_end(z, n, s.pos, &q, &body, &crc, &isize);
        if (r < 0) { m.status = r; break; }
        sink.end(m.out_len, crc, isize);
        if (r == 0) { m.flags = DMX_PF_LAST; break; }
        const uint64_t e = s.pos;
        s.pos = 8 * q;   // at the member's first byte
        const int ld = dmx_pf_land(cand, nc, &t, s.pos, &skipped);
        if (ld == 1) { m.next = t; break; }
        if (ld == 2) { s.pos = e; m.flags = DMX_PF_LOST; break; }
        sink.begin(q, m.out_len);
        m.reserved++;
        lastm = (uint32_t)m.out_len;
        if (first == DMX_PF_NOMEM) first = lastm;
        s.pos = 8 * (q + body);   // at its first block
    }
    m.end_bit = s.pos;
    mloc[k] = (uint64_t)first | ((uint64_t)lastm << 32);
    return m;
}

}   // namespace

// The serial walk over the blocks of z[0, n) from `bit` (internal; tests/c/pfind_model.cpp counts
// the candidates that are no block starts with it): starts[k] is the first bit of block k, kinds[k]
// its BTYPE | BFINAL << 2, for at most cap blocks; *nblocks counts them all.  Returns 0 at BFINAL or
// the status of the block that failed.
extern "C" __attribute__((visibility("hidden"))) int dmx_pf_host_blocks(const uint8_t* z, uint64_t n, uint64_t bit,
                                                                        uint64_t* starts, uint8_t* kinds, uint64_t cap,
                                                                        uint64_t* nblocks, uint64_t* out_len) {
    HB s = {z, n, bit};
    uint64_t k = 0, out = 0;
    int r = 0;
    for (;;) {
        if (k < cap) {
            starts[k] = s.pos;
            kinds[k] = (uint8_t)(((hb_peek(s) >> 1) & 3) | ((hb_peek(s) & 1) << 2));
        }
        k++;
        bool last = false;
        r = hb_status(s, hb_block(s, &out, &last, ~0ull));
        if (r || last) break;
    }
    *nblocks = k;
    *out_len = out;
    return r;
}

extern "C" int dmx_inflate_parallel_plan_host(const void* zv, uint64_t zbytes, uint32_t fmt, uint32_t chunk_bytes,
                                              dmx_pchunk* chunks, uint32_t cap, dmx_par_status* st) {
    if (!st || (!zv && zbytes) || (!chunks && cap) || fmt > DMX_BATCH_RAW) return -(int)E_INVAL;
    const uint32_t chunk = chunk_bytes ? chunk_bytes : DMX_PF_DEF_CHUNK;
    if (chunk < DMX_PF_MIN_CHUNK || chunk > DMX_PF_MAX_CHUNK) return -(int)E_INVAL;
    if (zbytes > DMX_PF_MAX_POS) return -(int)E_RANGE;
    const uint8_t* z = (const uint8_t*)zv;
    const uint32_t nc = dmx_pf_nchunks(zbytes, chunk);
    memset(st, 0, sizeof(*st));
    st->nchunks = nc;
    uint64_t body = 0;
    st->status = dmx_frame_head(z, zbytes, fmt, &st->format, &body);
    if (st->status) return 0;
    uint64_t* cand = (uint64_t*)malloc(8ull * nc);
    dmx_pf_meas* meas = (dmx_pf_meas*)calloc(nc, sizeof(dmx_pf_meas));
    if (!cand || !meas) {
        free(cand);
        free(meas);
        return -(int)E_MALLOC;
    }
    cand[0] = 8 * body;
    st->ncand = 1;
    for (uint32_t c = 1; c < nc; c++) {
        uint64_t lo, hi;
        dmx_pf_range(c, chunk, zbytes, 8 * body, &lo, &hi);
        cand[c] = DMX_PF_NONE;
        for (uint64_t bit = lo; bit < hi; bit++)
            if (dmx_pf_valid(z, zbytes, bit)) {
                cand[c] = bit;
                st->ncand++;
                break;
            }
    }
    // only the chunks the walk reaches are measured: the others' records are never read
    for (uint32_t i = 0;;) {
        meas[i] = measure(z, zbytes, cand, nc, i);
        if (meas[i].status || meas[i].flags) break;
        i = meas[i].next;
    }
    uint32_t isize = 0;
    dmx_pf_link(z, zbytes, cand, meas, chunks, cap, st, &isize);
    free(cand);
    free(meas);
    return st->nlive > cap ? -(int)E_SZ : 0;
}

// ---- one file of many gzip members (include/dmx.h: dmx_inflate_parallel_multi_plan_host) ----------
extern "C" int dmx_inflate_parallel_multi_plan_host(const void* zv, uint64_t zbytes, uint32_t fmt, uint32_t chunk_bytes,
                                                    dmx_pchunk* chunks, uint32_t cap, dmx_pmember* members, uint32_t mcap,
                                                    dmx_par_multi_status* ms) {
    if (!ms || (!zv && zbytes) || (!chunks && cap) || (!members && mcap)) return -(int)E_INVAL;
    if (fmt != DMX_BATCH_AUTO && fmt != DMX_BATCH_GZIP) return -(int)E_INVAL;
    const uint32_t chunk = chunk_bytes ? chunk_bytes : DMX_PF_DEF_CHUNK;
    if (chunk < DMX_PF_MIN_CHUNK || chunk > DMX_PF_MAX_CHUNK) return -(int)E_INVAL;
    if (zbytes > DMX_PF_MAX_POS) return -(int)E_RANGE;
    const uint8_t* z = (const uint8_t*)zv;
    const uint32_t nc = dmx_pf_nchunks(zbytes, chunk);
    memset(ms, 0, sizeof(*ms));
    ms->bad_member = 0xFFFFFFFFu;
    dmx_par_status* st = &ms->st;
    st->nchunks = nc;
    uint64_t body = 0;
    st->status = dmx_frame_head(z, zbytes, DMX_BATCH_GZIP, &st->format, &body);
    if (st->status) return 0;
    uint64_t* cand = (uint64_t*)malloc(8ull * nc);
    uint64_t* mloc = (uint64_t*)malloc(8ull * nc);
    dmx_pf_meas* meas = (dmx_pf_meas*)calloc(nc, sizeof(dmx_pf_meas));
    dmx_pf_mside* sides = (dmx_pf_mside*)malloc(sizeof(dmx_pf_mside) * (cap ? cap : 1ull));
    if (!cand || !mloc || !meas || !sides) {
        free(cand);
        free(mloc);
        free(meas);
        free(sides);
        return -(int)E_MALLOC;
    }
    cand[0] = 0;   // the first header
    st->ncand = 1;
    for (uint32_t c = 1; c < nc; c++) {
        uint64_t lo, hi;
        dmx_pf_range(c, chunk, zbytes, 0, &lo, &hi);
        cand[c] = DMX_PF_NONE;
        for (uint64_t bit = lo; bit < hi; bit++)
            if (((bit & 7) == 0 && dmx_pf_member(z, zbytes, bit >> 3)) || dmx_pf_valid(z, zbytes, bit)) {
                cand[c] = bit;
                st->ncand++;
                break;
            }
    }
    MemberSink sink = {members, mcap, 0, 0};
    for (uint32_t i = 0;;) {
        meas[i] = measure_multi(z, zbytes, cand, nc, i, mloc, sink);
        sink.off += meas[i].out_len;
        if (meas[i].status || meas[i].flags) break;
        i = meas[i].next;
    }
    uint32_t isize = 0;
    dmx_pf_link_multi(z, zbytes, cand, meas, mloc, chunks, sides, cap, ms, &isize);
    free(cand);
    free(mloc);
    free(meas);
    free(sides);
    return st->nlive > cap || ms->nmembers > mcap ? -(int)E_SZ : 0;
}

// ---- seek points from a plan's live chunks (include/dmx.h: dmx_zindex_from_chunks_host) ----------
extern "C" uint32_t dmx_zindex_points_bound(uint64_t out_cap, uint32_t max_live, uint32_t span) {
    return dmx_zs_bound(out_cap, max_live, span);
}

extern "C" uint64_t dmx_zindex_device_work(uint64_t out_cap, uint32_t max_points) { return dmx_zs_work(out_cap, max_points); }

static uint32_t zs_adler32(const uint8_t* d, uint64_t n) {
    uint32_t a = 1, b = 0;
    while (n) {
        uint64_t k = n < 5552 ? n : 5552;
        n -= k;
        while (k--) { a += *d++; b += a; }
        a %= 65521u;
        b %= 65521u;
    }
    return (b << 16) | a;
}

// The host twin of dmx_zindex_from_parallel_async: dmx_zs_select over the chunks, then every point's
// window and Adler-32 from the decoded bytes.  The chunks must tile out[0, out_len) in order.
extern "C" int dmx_zindex_from_chunks_host(const dmx_pchunk* chunks, uint32_t nlive, const void* outv, uint64_t out_len,
                                           uint32_t span, dmx_zpoint** points, uint32_t** adlers, uint8_t** windows,
                                           uint32_t* npoints) {
    if (!chunks || !nlive || (!outv && out_len) || !points || !adlers || !windows || !npoints) return -(int)E_INVAL;
    if (span > DMX_ZINDEX_MAX_SPAN) return -(int)E_RANGE;
    *points = NULL;
    *adlers = NULL;
    *windows = NULL;
    *npoints = 0;
    uint64_t off = 0;
    for (uint32_t c = 0; c < nlive; c++) {
        if (chunks[c].out_off != off || chunks[c].out_len > out_len - off) return -(int)E_INVAL;
        off += chunks[c].out_len;
    }
    if (off != out_len) return -(int)E_INVAL;
    const uint32_t sp = dmx_zs_span(span);
    const uint32_t n = dmx_zs_select(chunks, nlive, sp, NULL, NULL, 0);
    dmx_zpoint* p = (dmx_zpoint*)malloc(n * sizeof(dmx_zpoint));
    uint32_t* a = (uint32_t*)malloc(n * sizeof(uint32_t));
    uint32_t* base = (uint32_t*)malloc((n + 1ull) * sizeof(uint32_t));
    uint8_t* w = (uint8_t*)malloc(n * (uint64_t)DMX_ZINDEX_WINDOW);
    if (!p || !a || !base || !w) {
        free(p);
        free(a);
        free(base);
        free(w);
        return -(int)E_MALLOC;
    }
    dmx_zs_select(chunks, nlive, sp, p, base, n);
    free(base);
    const uint8_t* out = (const uint8_t*)outv;
    for (uint32_t k = 0; k < n; k++) {
        const uint64_t o = p[k].out_off;
        const size_t wlen = o < DMX_ZINDEX_WINDOW ? (size_t)o : DMX_ZINDEX_WINDOW;
        uint8_t* slot = w + k * (uint64_t)DMX_ZINDEX_WINDOW;
        memset(slot, 0, DMX_ZINDEX_WINDOW - wlen);
        if (wlen) memcpy(slot + (DMX_ZINDEX_WINDOW - wlen), out + (o - wlen), wlen);
        a[k] = zs_adler32(out ? out + o : NULL, p[k].out_len);
    }
    *points = p;
    *adlers = a;
    *windows = w;
    *npoints = n;
    return 0;
}

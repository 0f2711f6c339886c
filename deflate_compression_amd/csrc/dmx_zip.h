// dmx_zip.h -- the parse steps of a ZIP archive (PKWARE APPNOTE 4.3; the end-record rule of
// CPython's zipfile._EndRecData), as functions of a position alone, for the host index
// (dmx_zip_host.cpp: the serial walk), the device index (dmx_zip_dev.hip: a thread per position)
// and its host twin (tests/c/zip_model.cpp): all three compile this text.  Everything is
// little-endian and byte-wise, and reads nothing outside z[0, zbytes).  Host and device, C++ only,
// internal.
#ifndef DMX_ZIP_H
#define DMX_ZIP_H

#include <stdint.h>

#include "../../include/dmx.h"

#ifndef DMX_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMX_HD __host__ __device__
#else
#define DMX_HD
#endif
#endif

#define DMX_ZIP_EOCD 22u          // the end record without its comment
#define DMX_ZIP_LOC64 20u         // the ZIP64 locator
#define DMX_ZIP_EOCD64 56u        // the ZIP64 end record without extensible data
#define DMX_ZIP_TAIL 65557u       // the end record begins within this many bytes of the end (22 + 65 535)
#define DMX_ZIP_CDH 46u           // a central directory header without name / extra / comment
#define DMX_ZIP_LFH 30u           // a local header without name / extra
#define DMX_ZIP_MAXZ 0xFFFFFFF0ull

DMX_HD static inline uint32_t dmx_zip_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
DMX_HD static inline uint32_t dmx_zip_u32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
DMX_HD static inline uint64_t dmx_zip_u64(const uint8_t* p) { return (uint64_t)dmx_zip_u32(p) | ((uint64_t)dmx_zip_u32(p + 4) << 32); }
#define DMX_ZIP_SIG_EOCD 0x06054B50u     // PK\5\6
#define DMX_ZIP_SIG_LOC64 0x07064B50u    // PK\6\7
#define DMX_ZIP_SIG_EOCD64 0x06064B50u   // PK\6\6
#define DMX_ZIP_SIG_CDH 0x02014B50u      // PK\1\2
#define DMX_ZIP_SIG_LFH 0x04034B50u      // PK\3\4

// ---- the end record ----

// What the tail of the file says: the central directory's range in the file, the entries it
// announces and the shift of every stored offset; or the file's status.
struct dmx_zip_tail {
    int32_t status;
    uint32_t nentries;
    uint64_t cd_begin, cd_end, concat;
};

// The first lower bound of the search and the fast rule: the last 22 bytes are an end record with
// an empty comment.
DMX_HD static inline uint64_t dmx_zip_tail_lo(uint64_t zbytes) { return zbytes > DMX_ZIP_TAIL ? zbytes - DMX_ZIP_TAIL : 0; }
DMX_HD static inline bool dmx_zip_end_fast(const uint8_t* z, uint64_t zbytes) {
    if (zbytes < DMX_ZIP_EOCD) return false;
    const uint8_t* e = z + zbytes - DMX_ZIP_EOCD;
    return dmx_zip_u32(e) == DMX_ZIP_SIG_EOCD && e[20] == 0 && e[21] == 0;
}
// Is p (p + 4 <= zbytes) a position of the signature PK\5\6?  The slow rule takes the last such p
// at or behind dmx_zip_tail_lo.
DMX_HD static inline bool dmx_zip_end_sig(const uint8_t* z, uint64_t p) { return dmx_zip_u32(z + p) == DMX_ZIP_SIG_EOCD; }

// The serial search (the host walk; the device does it with a lane per position and a maximum):
// the position of the end record, or UINT64_MAX.
DMX_HD static inline uint64_t dmx_zip_end_find(const uint8_t* z, uint64_t zbytes) {
    if (dmx_zip_end_fast(z, zbytes)) return zbytes - DMX_ZIP_EOCD;
    if (zbytes < 4) return ~0ull;
    const uint64_t lo = dmx_zip_tail_lo(zbytes);
    for (uint64_t p = zbytes - 4;; p--) {
        if (dmx_zip_end_sig(z, p)) return p;
        if (p == lo) break;
    }
    return ~0ull;
}

// The end record at `eocd` (UINT64_MAX: none was found), the ZIP64 locator 20 bytes in front of it
// and the ZIP64 end record 56 bytes in front of that, as zipfile reads them; then the checks of
// the file: one disk, the directory inside the file.
DMX_HD static inline void dmx_zip_end_parse(const uint8_t* z, uint64_t zbytes, uint64_t eocd, dmx_zip_tail* t) {
    t->status = 0;
    t->nentries = 0;
    t->cd_begin = t->cd_end = t->concat = 0;
    if (zbytes > DMX_ZIP_MAXZ) {
        t->status = -(int)E_RANGE;
        return;
    }
    if (eocd == ~0ull || eocd > zbytes || zbytes - eocd < DMX_ZIP_EOCD) {   // none, or cut
        t->status = -(int)E_ZHEAD;
        return;
    }
    const uint8_t* e = z + eocd;
    uint64_t disk = dmx_zip_u16(e + 4), cd_disk = dmx_zip_u16(e + 6), n_here = dmx_zip_u16(e + 8), n_all = dmx_zip_u16(e + 10);
    uint64_t cd_size = dmx_zip_u32(e + 12), cd_off = dmx_zip_u32(e + 16);
    uint64_t behind = eocd;   // where the directory ends
    if (eocd >= DMX_ZIP_LOC64 && dmx_zip_u32(e - DMX_ZIP_LOC64) == DMX_ZIP_SIG_LOC64) {
        const uint8_t* l = e - DMX_ZIP_LOC64;
        const bool rec = eocd >= DMX_ZIP_LOC64 + DMX_ZIP_EOCD64 && dmx_zip_u32(l - DMX_ZIP_EOCD64) == DMX_ZIP_SIG_EOCD64;
        if (rec) {
            if (dmx_zip_u32(l + 4) != 0 || dmx_zip_u32(l + 16) > 1) {   // the locator's disk numbers
                t->status = -(int)E_RANGE;
                return;
            }
            const uint8_t* r = l - DMX_ZIP_EOCD64;
            disk = dmx_zip_u32(r + 16);
            cd_disk = dmx_zip_u32(r + 20);
            n_here = dmx_zip_u64(r + 24);
            n_all = dmx_zip_u64(r + 32);
            cd_size = dmx_zip_u64(r + 40);
            cd_off = dmx_zip_u64(r + 48);
            behind = eocd - DMX_ZIP_LOC64 - DMX_ZIP_EOCD64;
        } else if (n_here == 0xFFFF || n_all == 0xFFFF || cd_size == 0xFFFFFFFFu || cd_off == 0xFFFFFFFFu) {
            // a locator, markers that need its record, and no record
            t->status = -(int)E_ZHEAD;
            return;
        }
        // (a locator's signature without a record and without markers: bytes of the last header, as zipfile reads it)
    }
    if (disk != 0 || cd_disk != 0 || n_here != n_all || n_all > 0xFFFFFFFFull) {
        t->status = -(int)E_RANGE;
        return;
    }
    if (cd_size > behind || cd_off > behind - cd_size) {   // the directory, or concat, in front of the file
        t->status = -(int)E_RANGE;
        return;
    }
    t->nentries = (uint32_t)n_all;
    t->cd_begin = behind - cd_size;
    t->cd_end = behind;
    t->concat = t->cd_begin - cd_off;
}

// ---- a central directory header ----

// The step at p: cd_begin <= p < cd_end <= zbytes.  The header's whole length (46 + n + m + k),
// or 0 where p is no header of the region: the signature, the 46 bytes, the three lengths.
DMX_HD static inline uint32_t dmx_zip_cd_step(const uint8_t* z, uint64_t cd_end, uint64_t p) {
    if (cd_end - p < DMX_ZIP_CDH) return 0;
    const uint8_t* h = z + p;
    if (dmx_zip_u32(h) != DMX_ZIP_SIG_CDH) return 0;
    const uint64_t len = (uint64_t)DMX_ZIP_CDH + dmx_zip_u16(h + 28) + dmx_zip_u16(h + 30) + dmx_zip_u16(h + 32);
    if (len > cd_end - p) return 0;
    return (uint32_t)len;
}

// The entry of the header at p (a position where dmx_zip_cd_step succeeded): the ZIP64 extra, then
// the local header at hdr_off + concat, whose own name and extra lengths place the data.  Sizes and
// CRC are the central directory's.  out_off is left 0: the scan's.
DMX_HD static inline void dmx_zip_finish(const uint8_t* z, uint64_t zbytes, uint64_t concat, uint64_t p, dmx_zip_entry* out) {
    const uint8_t* h = z + p;
    dmx_zip_entry e;
    e.flags = (uint16_t)dmx_zip_u16(h + 8);
    e.method = (uint16_t)dmx_zip_u16(h + 10);
    e.crc = dmx_zip_u32(h + 16);
    uint64_t csize = dmx_zip_u32(h + 20), usize = dmx_zip_u32(h + 24), hoff = dmx_zip_u32(h + 42);
    const uint32_t n = dmx_zip_u16(h + 28), m = dmx_zip_u16(h + 30);
    e.name_len = (uint16_t)n;
    e.name_off = p + DMX_ZIP_CDH;
    e.reserved = 0;
    const uint8_t* x = h + DMX_ZIP_CDH + n;   // the extra field: (id, size, data) records
    for (uint32_t q = 0; q + 4 <= m;) {
        const uint32_t id = dmx_zip_u16(x + q), ln = dmx_zip_u16(x + q + 2);
        if (q + 4 + ln > m) break;
        if (id == 0x0001) {   // ZIP64: a field for every value that holds the marker, in this order
            uint32_t at = 0;
            if (usize == 0xFFFFFFFFu && at + 8 <= ln) {
                usize = dmx_zip_u64(x + q + 4 + at);
                at += 8;
            }
            if (csize == 0xFFFFFFFFu && at + 8 <= ln) {
                csize = dmx_zip_u64(x + q + 4 + at);
                at += 8;
            }
            if (hoff == 0xFFFFFFFFu && at + 8 <= ln) {
                hoff = dmx_zip_u64(x + q + 4 + at);
                at += 8;
            }
        }
        q += 4 + ln;
    }
    e.csize = csize;
    e.usize = usize;
    e.out_off = 0;
    e.data_off = 0;
    e.hdr_off = hoff <= DMX_ZIP_MAXZ ? hoff + concat : ~0ull;
    int32_t st = 0;
    if (e.method != 0 && e.method != 8) st = -(int)E_ZCMPMT;
    else if (e.flags & 0x41) st = -(int)E_RESERV;   // encrypted, or bit 6 (strong encryption)
    if (e.hdr_off > zbytes || zbytes - e.hdr_off < DMX_ZIP_LFH || dmx_zip_u32(z + e.hdr_off) != DMX_ZIP_SIG_LFH) {
        if (!st) st = -(int)E_ZHEAD;
    } else {
        const uint8_t* l = z + e.hdr_off;
        e.data_off = e.hdr_off + DMX_ZIP_LFH + dmx_zip_u16(l + 26) + dmx_zip_u16(l + 28);
        if (!st && (e.data_off > zbytes || csize > zbytes - e.data_off)) st = -(int)E_RANGE;
        if (!st && e.method == 0 && csize != usize) st = -(int)E_LEN;
    }
    e.status = st;
    *out = e;
}

// ---- the device index, stage by stage: what one thread does, so that the kernels
// of dmx_zip_dev.hip and the loops of the host twin run the same text ----

// A candidate: a position of the directory where dmx_zip_cd_step succeeds.  term: what lies behind
// it -- 0 another candidate, 1 the directory's end, 2 neither (the chain breaks there).
struct dmx_zip_cand {
    uint32_t off, len, term, reserved;
};
// Pointer doubling: after k rounds j = the 2^k-th successor (n = behind the end), c = the nodes over
// the 2^k from here.
struct dmx_zip_node {
    uint32_t j, c;
};
// A node of the true chain once reached: round = 1 + the round that marked it (0 = not marked; the
// node at cd_begin starts with 1), c = the nodes before it: its rank.
struct dmx_zip_mark {
    uint32_t round, c;
};
#define DMX_ZIP_GROUP 16u   // bytes per aligned load of the scan

// Stage 2.  The candidates among the 16 positions of aligned group g of a file that starts `head`
// bytes into group 0 (position k is offset 16 g + k - head): w = the group's four words and the
// first word of the group behind it (anything where the file has no bytes).  Only positions in
// [cd_begin, cd_end - 46] are looked at.  Returns their number; the first `room` of them go to
// out[] in offset order.
DMX_HD static inline uint32_t dmx_zip_group(const uint8_t* z, uint64_t cd_begin, uint64_t cd_end, uint32_t head, uint64_t g,
                                            const uint32_t w[5], dmx_zip_cand* out, uint32_t room) {
    uint32_t n = 0, any = 0;
    for (uint32_t k = 0; k < 4; k++) {   // a byte 'P' among the 16?  (the zero-byte test on w ^ 50505050)
        const uint32_t x = w[k] ^ 0x50505050u;
        any |= (x - 0x01010101u) & ~x & 0x80808080u;
    }
    if (!any) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < DMX_ZIP_GROUP; k++) {
        const uint64_t a = g * DMX_ZIP_GROUP + k;
        if (a < head + cd_begin || a - head + DMX_ZIP_CDH > cd_end) continue;
        const uint32_t v = (uint32_t)((((uint64_t)w[k / 4 + 1] << 32) | w[k / 4]) >> (8 * (k & 3)));
        if (v != DMX_ZIP_SIG_CDH) continue;
        const uint32_t len = dmx_zip_cd_step(z, cd_end, a - head);
        if (!len) continue;
        if (n < room) {
            dmx_zip_cand c = {(uint32_t)(a - head), len, 0, 0};
            out[n] = c;
        }
        n++;
    }
    return n;
}

// Stage 3 for node i of n candidates (sorted by offset) + the end node n: the link and the first
// mark (on the candidate at cd_begin, which is candidate 0 or none).
DMX_HD static inline void dmx_zip_link(uint64_t cd_begin, uint64_t cd_end, dmx_zip_cand* cand, uint32_t n, uint32_t i,
                                       dmx_zip_node* node, dmx_zip_mark* mark) {
    dmx_zip_mark mk = {i == 0 && n && cand[0].off == cd_begin ? 1u : 0u, 0};
    mark[i] = mk;
    dmx_zip_node x = {n, 0};
    if (i < n) {
        const uint64_t q = (uint64_t)cand[i].off + cand[i].len;
        uint32_t term = 1;
        if (q < cd_end) {
            uint32_t lo = i + 1, hi = n;   // the first candidate at or behind q
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (cand[mid].off < q) lo = mid + 1;
                else hi = mid;
            }
            if (lo < n && cand[lo].off == q) {
                x.j = lo;
                term = 0;
            } else {
                term = 2;
            }
        }
        cand[i].term = term;
        x.c = 1;
    }
    node[i] = x;
}

// Stage 4, round k = 0, 1, ... for node i <= n: a node marked before this round marks its 2^k-th
// successor, then the node doubles from a[] into b[].
DMX_HD static inline void dmx_zip_round(const dmx_zip_node* a, dmx_zip_node* b, dmx_zip_mark* mark, uint32_t n, uint32_t i,
                                        uint32_t k) {
    const dmx_zip_node x = a[i];
    const uint32_t r = mark[i].round;
    if (r && r <= k + 1 && x.j != n) {   // (a mark of this round has round k + 2: its c may not be there yet)
        dmx_zip_mark mk = {k + 2, mark[i].c + x.c};
        mark[x.j] = mk;
    }
    const dmx_zip_node y = a[x.j];
    dmx_zip_node d = {y.j, x.c + y.c};
    b[i] = d;
}

// Stage 5 for candidate i < n: is it the chain's last node, and does the chain then consist of
// exactly nentries headers that end at cd_end?  1 yes, -1 no, 0 not the last node (one candidate
// answers with a non-zero value, none where the chain is empty).
DMX_HD static inline int dmx_zip_decide(const dmx_zip_cand* cand, const dmx_zip_mark* mark, uint32_t i, uint32_t nentries) {
    if (!mark[i].round || !cand[i].term) return 0;
    return cand[i].term == 1 && mark[i].c + 1 == nentries ? 1 : -1;
}

// Stage 7 for entry i of `count` written entries, serially: out_off.  (The device scans.)
DMX_HD static inline uint64_t dmx_zip_len(const dmx_zip_entry* e) { return e->status ? 0 : e->usize; }

#endif

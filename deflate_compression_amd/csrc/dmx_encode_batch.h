// dmx_encode_batch.h -- the plan of a batch encode (dmx_encode_batch_async and
// dmx_encode_batch_dict_async), stage by stage: what one thread of every planning
// kernel does, so that the kernels of dmx_encode_batch.hip and the loops of the host twins
// (tests/c/encode_batch_model.cpp, tests/c/encode_batch_dict_model.cpp) run the same text.  The collectives
// between the per-thread parts -- the sums and the exclusive scan over a workgroup -- are the
// caller's: LDS on the device, a loop in the twin.  Host and device, C++ only, internal.
#ifndef DMX_ENCODE_BATCH_H
#define DMX_ENCODE_BATCH_H

#include <stdint.h>

#include "../../include/dmx.h"
#include "dmx_internal.h"

#if defined(__HIPCC__)
#define DMX_EB_HD __host__ __device__
#else
#define DMX_EB_HD
#endif

// Scan tile: a workgroup's share of the streams, one per thread.  The twin shrinks it (4 and 8) so
// that small batches cross many tile edges.
#ifndef DMX_EB_STILE
#define DMX_EB_STILE 256u
#endif
// threads of the one workgroup that scans the tile sums (a contiguous share of the tiles each)
#ifndef DMX_EB_STHREADS
#define DMX_EB_STHREADS 1024u
#endif
#define DMX_EB_NOBAD 0xFFFFFFFFu

// What the plan hands to the encode's kernels (the head of the plan scratch, 64 bytes).
struct dmx_eb_head {
    uint64_t nblocks;    // blocks the batch needs (saturating): the sum of dmx_eb_count over the streams
    uint64_t in_len;     // the sum of in_len over the streams with status 0 (saturating)
    int32_t status;      // 0, or -E_SZ: nblocks > max_blocks -- every table entry is then void
    uint32_t nfailed;    // streams with -E_RANGE
    uint32_t first_bad;  // the lowest such index, else DMX_EB_NOBAD
    uint32_t reserved[9];
};

// What a tile of streams sums to.
struct dmx_eb_tile {
    uint64_t blocks;     // dmx_eb_scan: replaced by the blocks of the tiles before this one
    uint64_t bytes;
    uint32_t nfailed;
    uint32_t first_bad;
};

DMX_EB_HD static inline uint64_t dmx_eb_sat(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
}

// ---- A stream's verdict.  dmx_encode_batch_dict_async's also depends on the stream's preset dictionary,
// so the plan is written once, with a dmx_ebd; dmx_encode_batch_async passes the empty one
// (dmx_ebd_none), under which every stream is DMX_BATCH_NODICT and the verdict is dmx_eb_valid alone.
// The dmx_eb_* forms without a dmx_ebd are that call (the host twin of the plain batch runs them).
struct dmx_ebd {
    const dmx_bdict* dicts;    // ndicts records into d_dict[0, dict_bytes)
    const uint32_t* dict_of;   // per stream: an index or DMX_BATCH_NODICT; NULL: every stream uses 0
    uint64_t dict_bytes;
    uint32_t ndicts;
    uint32_t fdict;            // DMX_F_FDICT: the header names the dictionary, which is then whole
};
DMX_EB_HD static inline dmx_ebd dmx_ebd_none() {
    dmx_ebd d = {NULL, NULL, 0, 0, 0};
    return d;
}
// stream k lies inside d_in[0, in_bytes): the test that cannot wrap
DMX_EB_HD static inline bool dmx_eb_valid(const dmx_estream& s, uint64_t in_bytes) {
    return s.in_off <= in_bytes && s.in_len <= in_bytes - s.in_off;
}
// the dictionary stream k names: an index, or DMX_BATCH_NODICT (also every stream of a call without
// dictionaries and without d_dict_of) -- dmx_inflate_batch_dict_async's rule
DMX_EB_HD static inline uint32_t dmx_ebd_index(const dmx_ebd& d, uint32_t k) {
    return d.dict_of ? d.dict_of[k] : d.ndicts ? 0u : DMX_BATCH_NODICT;
}
// record j lies inside d_dict[0, dict_bytes): the test that cannot wrap
DMX_EB_HD static inline bool dmx_ebd_inside(const dmx_bdict& r, uint64_t dict_bytes) {
    return r.off <= dict_bytes && r.len <= dict_bytes - r.off;
}
// stream k's status: -E_RANGE for a buffer outside d_in, a dictionary index at or above ndicts or a
// record outside d_dict; under DMX_F_FDICT -E_INVAL for a dictionary of length 0 or above sw, the
// single encode's verdict (its DICTID must cover what the parse may reference); else 0
DMX_EB_HD static inline int32_t dmx_ebd_status(const dmx_estream* st, uint32_t k, uint64_t in_bytes, uint32_t sw,
                                               const dmx_ebd& d) {
    if (!dmx_eb_valid(st[k], in_bytes)) return -(int32_t)E_RANGE;
    const uint32_t di = dmx_ebd_index(d, k);
    if (di == DMX_BATCH_NODICT) return 0;
    if (di >= d.ndicts || !dmx_ebd_inside(d.dicts[di], d.dict_bytes)) return -(int32_t)E_RANGE;
    if (d.fdict && (d.dicts[di].len < 1 || d.dicts[di].len > sw)) return -(int32_t)E_INVAL;
    return 0;
}
// the history of a first block: the last min(len, sw) bytes of the stream's dictionary (hn 0: none),
// at d_dict + *off, its chain slot *slot = the dictionary's index.  For a stream with status 0.
DMX_EB_HD static inline uint32_t dmx_ebd_history(const dmx_ebd& d, uint32_t k, uint32_t sw, uint64_t* off, uint32_t* slot) {
    const uint32_t di = dmx_ebd_index(d, k);
    *off = 0;
    *slot = 0;
    if (di == DMX_BATCH_NODICT) return 0;
    const dmx_bdict r = d.dicts[di];
    const uint32_t hn = r.len < sw ? (uint32_t)r.len : sw;
    *off = r.off + (r.len - hn);
    *slot = di;
    return hn;
}
// blocks of a stream: an empty one has one (empty) block, which carries its whole framing; a stream
// that is refused has none
DMX_EB_HD static inline uint64_t dmx_eb_nblocks(bool ok, uint64_t len, uint32_t sw) {
    const uint64_t c = len / sw + (len % sw ? 1u : 0u);
    return !ok ? 0u : c ? c : 1u;
}
DMX_EB_HD static inline uint64_t dmx_ebd_count(const dmx_estream* st, uint32_t k, uint64_t in_bytes, uint32_t sw,
                                               const dmx_ebd& d) {
    return dmx_eb_nblocks(dmx_ebd_status(st, k, in_bytes, sw, d) == 0, st[k].in_len, sw);
}
DMX_EB_HD static inline uint64_t dmx_eb_count(const dmx_estream& s, uint64_t in_bytes, uint32_t sw) {
    return dmx_ebd_count(&s, 0, in_bytes, sw, dmx_ebd_none());
}

// ---- dmx_eb_count_kernel: a thread per stream; the caller sums the four over the tile
DMX_EB_HD static inline dmx_eb_tile dmx_ebd_stream_sums(const dmx_estream* st, uint32_t k, uint64_t in_bytes, uint32_t sw,
                                                        const dmx_ebd& d) {
    dmx_eb_tile t;
    const bool ok = dmx_ebd_status(st, k, in_bytes, sw, d) == 0;
    t.blocks = dmx_eb_nblocks(ok, st[k].in_len, sw);
    t.bytes = ok ? st[k].in_len : 0u;
    t.nfailed = ok ? 0u : 1u;
    t.first_bad = ok ? DMX_EB_NOBAD : k;
    return t;
}
DMX_EB_HD static inline dmx_eb_tile dmx_eb_stream_sums(const dmx_estream* st, uint32_t k, uint64_t in_bytes, uint32_t sw) {
    return dmx_ebd_stream_sums(st, k, in_bytes, sw, dmx_ebd_none());
}
DMX_EB_HD static inline dmx_eb_tile dmx_eb_tile_add(const dmx_eb_tile& a, const dmx_eb_tile& b) {
    dmx_eb_tile t;
    t.blocks = dmx_eb_sat(a.blocks, b.blocks);
    t.bytes = dmx_eb_sat(a.bytes, b.bytes);
    t.nfailed = a.nfailed + b.nfailed;
    t.first_bad = a.first_bad < b.first_bad ? a.first_bad : b.first_bad;
    return t;
}
DMX_EB_HD static inline dmx_eb_tile dmx_eb_tile_zero() {
    dmx_eb_tile t = {0, 0, 0, DMX_EB_NOBAD};
    return t;
}

// ---- dmx_eb_plan_scan_kernel, by the one workgroup of DMX_EB_STHREADS threads: thread t owns the tiles
// [a, b) of n, sums them (dmx_eb_chunk_sum) and -- given the sum over the threads before it --
// replaces every tile's block count by the blocks of the tiles before it (dmx_eb_chunk_apply).
DMX_EB_HD static inline void dmx_eb_chunk(uint32_t n, uint32_t nth, uint32_t t, uint32_t* a, uint32_t* b) {
    const uint64_t per = ((uint64_t)n + nth - 1) / nth;
    const uint64_t lo = (uint64_t)t * per < n ? (uint64_t)t * per : n;
    *a = (uint32_t)lo;
    *b = (uint32_t)(lo + per < n ? lo + per : n);
}
DMX_EB_HD static inline dmx_eb_tile dmx_eb_chunk_sum(const dmx_eb_tile* v, uint32_t n, uint32_t nth, uint32_t t) {
    uint32_t a, b;
    dmx_eb_chunk(n, nth, t, &a, &b);
    dmx_eb_tile s = dmx_eb_tile_zero();
    for (uint32_t k = a; k < b; k++) s = dmx_eb_tile_add(s, v[k]);
    return s;
}
DMX_EB_HD static inline void dmx_eb_chunk_apply(dmx_eb_tile* v, uint32_t n, uint32_t nth, uint32_t t, uint64_t run) {
    uint32_t a, b;
    dmx_eb_chunk(n, nth, t, &a, &b);
    for (uint32_t k = a; k < b; k++) {
        const uint64_t c = v[k].blocks;
        v[k].blocks = run;
        run = dmx_eb_sat(run, c);
    }
}
// the decision, by one thread once the scan is done: the head from the batch's totals
DMX_EB_HD static inline void dmx_eb_decide(dmx_eb_head* head, const dmx_eb_tile& total, uint32_t max_blocks) {
    dmx_eb_head h;
    h.nblocks = total.blocks;
    h.in_len = total.bytes;
    h.status = total.blocks > max_blocks ? -(int32_t)E_SZ : 0;
    h.nfailed = total.nfailed;
    h.first_bad = total.first_bad;
    for (int i = 0; i < 9; i++) h.reserved[i] = 0;
    *head = h;
}

// ---- dmx_eb_starts_kernel: a thread per stream: starts[k] = the blocks before stream k (`before`:
// the tile's prefix plus the streams before k in its tile, saturating); the thread of the last
// stream also writes starts[nstreams].  Then the stream's record before any kernel encodes: its
// status and block count (out_off, out_len and check come from the finish).
DMX_EB_HD static inline void dmx_ebd_start(const dmx_estream* st, uint32_t k, uint32_t nstreams, uint64_t in_bytes,
                                           uint32_t sw, const dmx_ebd& d, uint64_t before, uint64_t* starts,
                                           dmx_eresult* res) {
    const int32_t status = dmx_ebd_status(st, k, in_bytes, sw, d);
    const uint64_t c = dmx_eb_nblocks(status == 0, st[k].in_len, sw);
    starts[k] = before;
    if (k + 1 == nstreams) starts[nstreams] = dmx_eb_sat(before, c);
    dmx_eresult r;
    r.status = status;
    r.nblocks = c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c;
    r.out_off = 0;
    r.out_len = 0;
    r.check = 0;
    r.reserved = 0;
    res[k] = r;
}
DMX_EB_HD static inline void dmx_eb_start(const dmx_estream* st, uint32_t k, uint32_t nstreams, uint64_t in_bytes,
                                          uint32_t sw, uint64_t before, uint64_t* starts, dmx_eresult* res) {
    dmx_ebd_start(st, k, nstreams, in_bytes, sw, dmx_ebd_none(), before, starts, res);
}

// the stream that block b belongs to: the last k of 0..nstreams-1 with starts[k] <= b (nstreams >= 1,
// starts[0] == 0).  A stream without blocks shares its start with the next one, so the last such k
// is the one that has block b whenever b < starts[nstreams].  Ends inside 0..nstreams-1 whatever
// the entries hold.
DMX_EB_HD static inline uint32_t dmx_eb_find(const uint64_t* starts, uint32_t nstreams, uint64_t b) {
    uint32_t lo = 0, hi = nstreams;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (starts[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- dmx_eb_table_kernel: a thread per table entry b < max_blocks.  Entries at or beyond the real
// block count, and every entry of a batch that does not fit max_blocks, are void.  starts[] already
// holds the verdict: a refused stream has no blocks, so no entry finds it.  DMX_BB_DICT: the
// entry's stream names a dictionary.
DMX_EB_HD static inline dmx_bblk dmx_ebd_entry(const dmx_estream* st, const uint64_t* starts, uint32_t nstreams,
                                               const dmx_eb_head* head, uint32_t sw, const dmx_ebd& d, uint32_t b) {
    dmx_bblk e;
    e.off = 0;
    e.len = DMX_BB_VOID;
    e.stream = 0xFFFFFFFFu;
    if (head->status || b >= head->nblocks || !nstreams) return e;
    const uint32_t k = dmx_eb_find(starts, nstreams, b);
    const uint64_t j = b - starts[k], len = st[k].in_len;
    const uint64_t cnt = len / sw + (len % sw ? 1u : 0u);   // (0 for the empty stream's one block)
    const uint64_t left = len - j * sw;
    e.off = st[k].in_off + j * sw;
    e.len = (uint32_t)(left < sw ? left : sw) | (j == 0 ? DMX_BB_FIRST : 0u) | (j + 1 >= cnt ? DMX_BB_LAST : 0u) |
            (dmx_ebd_index(d, k) != DMX_BATCH_NODICT ? DMX_BB_DICT : 0u);
    e.stream = k;
    return e;
}
DMX_EB_HD static inline dmx_bblk dmx_eb_entry(const dmx_estream* st, const uint64_t* starts, uint32_t nstreams,
                                              const dmx_eb_head* head, uint32_t sw, uint32_t b) {
    return dmx_ebd_entry(st, starts, nstreams, head, sw, dmx_ebd_none(), b);
}

// The bytes the batch's streams may need at most, packed: stream k at most
// align4(dmx_max_compressed_flags(len_k, sw, flags)).  With B = the bound on blocks every stream pays
// 5 bytes per block, and per stream the fixed part of dmx_max_compressed (27), the gzip framing's 12
// more and 3 of rounding.
DMX_EB_HD static inline uint32_t dmx_eb_blocks_bound(uint64_t total_in, uint32_t nstreams, uint32_t sw) {
    // sum of max(1, ceil(len / sw)) <= total / sw + nstreams (a partial or empty block per stream)
    const uint64_t b = dmx_eb_sat(total_in / sw, nstreams);
    return b > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)b;
}

#endif

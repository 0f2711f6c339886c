// dmx_zsel.h -- which live chunks of a plan become seek points (dmx_zindex_from_parallel_async,
// dmx_zindex_from_chunks_host, include/dmx.h; DESIGN.md 3.1 "Seek points from the one-pass decode"):
// dmx_zindex_build_host's rule restricted to chunk boundaries.  Point 0 is live chunk 0; a further
// point begins at the first live chunk at which the output since the current point's start is
// >= span.  A chunk's out_off is the exclusive scan of out_len, so that output is a difference of
// two out_off and the rule is one comparison per chunk (dmx_zs_starts).  A point has the bit and
// out_off of its first chunk, the next point's bit as its end_bit (the last: the last chunk's
// end_bit) and the sum of its chunks' out_len; a last chunk of no output behind such a boundary is
// a last point of length 0, as on the host.  Every point is a run of whole chunks, so of whole
// blocks.  One text for the host twin (dmx_inflate_par_host.cpp), the model under the sanitizers
// (tests/c/zsel_model.cpp) and the select kernel (dmx_zindex_dev.hip), where a lane tests a chunk.
// Host and device, C++ only, internal.
#ifndef DMX_ZSEL_H
#define DMX_ZSEL_H

#include <stdint.h>

#include "../../include/dmx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMX_ZS_HD __host__ __device__
#else
#define DMX_ZS_HD
#endif

#define DMX_ZS_PIECE 65536u   // the fold's pieces: 64 KiB of one point, counted from the point's start

static inline DMX_ZS_HD uint64_t dmx_zs_a256(uint64_t x) { return (x + 255) & ~255ull; }
static inline DMX_ZS_HD uint32_t dmx_zs_span(uint32_t span) { return span ? span : DMX_ZINDEX_DEF_SPAN; }

// the rule: a live chunk (not chunk 0) at output offset chunk_off begins a point iff the current
// point, which began at point_off, holds at least span bytes in front of it
static inline DMX_ZS_HD bool dmx_zs_starts(uint64_t chunk_off, uint64_t point_off, uint32_t span) {
    return chunk_off - point_off >= span;
}

// the pieces of a point of out_len bytes (an empty point has none)
static inline DMX_ZS_HD uint64_t dmx_zs_pieces(uint64_t out_len) { return (out_len + DMX_ZS_PIECE - 1) / DMX_ZS_PIECE; }

// min(out_cap / span + 1, max_live), at least 1: every point but the last holds span bytes or more
static inline DMX_ZS_HD uint32_t dmx_zs_bound(uint64_t out_cap, uint32_t max_live, uint32_t span) {
    const uint64_t n = out_cap / dmx_zs_span(span) + 1;
    const uint64_t m = n < max_live ? n : max_live;
    return m ? (uint32_t)m : 1u;
}

// d_work of the index call: [control 256][piece bases 4 x (npoints + 1)][piece sums 8 x pieces], every
// part 256-byte aligned; npoints points over out_len bytes have at most out_len / 65536 + npoints pieces
static inline DMX_ZS_HD uint64_t dmx_zs_max_pieces(uint64_t out_len, uint32_t npoints) { return out_len / DMX_ZS_PIECE + npoints; }
static inline DMX_ZS_HD uint64_t dmx_zs_work(uint64_t out_len, uint32_t npoints) {
    return 256 + dmx_zs_a256(4ull * npoints + 4) + dmx_zs_a256(8 * dmx_zs_max_pieces(out_len, npoints));
}

// The walk, chunk after chunk: the points of chunks[0, nlive) (nlive >= 1) under span (not 0).
// Returns their number, npoints.  points[k] and base[k] (the pieces of the points before k) are
// written for k < cap only, and base[npoints], the total, where npoints <= cap: base holds cap + 1
// entries.  cap 0 writes nothing: it counts.
static inline DMX_ZS_HD uint32_t dmx_zs_select(const dmx_pchunk* chunks, uint32_t nlive, uint32_t span, dmx_zpoint* points,
                                               uint32_t* base, uint32_t cap) {
    uint32_t k = 0;        // the current point
    uint32_t first = 0;    // its first chunk
    uint64_t pieces = 0;   // of the points before it
    for (uint32_t c = 1; c <= nlive; c++) {
        if (c < nlive && !dmx_zs_starts(chunks[c].out_off, chunks[first].out_off, span)) continue;
        const uint64_t end = chunks[c - 1].out_off + chunks[c - 1].out_len;
        if (k < cap) {
            points[k].bit = chunks[first].bit;
            points[k].end_bit = chunks[c - 1].end_bit;
            points[k].out_off = chunks[first].out_off;
            points[k].out_len = end - chunks[first].out_off;
            base[k] = (uint32_t)pieces;
        }
        pieces += dmx_zs_pieces(end - chunks[first].out_off);
        k++;
        first = c;
    }
    if (k <= cap && cap) base[k] = (uint32_t)pieces;
    return k;
}

#endif

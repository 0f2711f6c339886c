// dmx_ptail.h -- the rules that turn the cells of a parallel decode of one foreign stream into
// bytes (dmx_inflate_parallel_decode_async, include/dmx.h; DESIGN.md 3.1 "One foreign stream: the
// decode").  Every live chunk decodes on its own into 16-bit cells: a byte value, or a reference
// 0x100 + b - 1 to the byte b positions before the CHUNK's first output byte (b in 1..32768; a copy
// inside the chunk copies cells, so a reference never names the chunk's own output).  The tail pass
// walks the chunks in order with the 32 768 resolved bytes in front of the current chunk as its
// window, resolves the chunk's last min(out_len, 32768) cells from it and builds the next window;
// the pack pass resolves what is left from the cells the tail pass resolved.  One text for the
// kernels (dmx_inflate_dev.hip) and the model under the sanitizers (tests/c/ptail_model.cpp).
// Host and device, C++ only, internal.
#ifndef DMX_PTAIL_H
#define DMX_PTAIL_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMX_PT_HD __host__ __device__
#else
#define DMX_PT_HD
#endif

#define DMX_PT_WIN 32768u   // the window: no DEFLATE distance is longer
#define DMX_PT_REF 0x100u   // the first reference cell: the byte one position before the chunk

// a reference cell for the byte b >= 1 positions before the chunk's start (the cell decoder's rule)
static inline DMX_PT_HD uint32_t dmx_pt_ref(uint32_t b) { return DMX_PT_REF + b - 1; }
// how far before the chunk's start a reference cell points (1..65 280 for any 16-bit cell)
static inline DMX_PT_HD uint32_t dmx_pt_back(uint32_t c) { return c - (DMX_PT_REF - 1); }
// the cells of a chunk the tail pass resolves: its last dmx_pt_tail(out_len)
static inline DMX_PT_HD uint32_t dmx_pt_tail(uint64_t out_len) { return out_len < DMX_PT_WIN ? (uint32_t)out_len : DMX_PT_WIN; }

// The per-cell rule of the tail pass.  window[0, 32768) holds the output bytes
// [out_off - 32768, out_off) in front of the chunk (what lies before output offset 0 is never read).
// Returns the byte, or -1 for a reference before the first output byte or beyond the window.
static inline DMX_PT_HD int dmx_pt_cell(uint32_t c, const uint8_t* window, uint64_t out_off) {
    if (c < DMX_PT_REF) return (int)c;
    const uint32_t b = dmx_pt_back(c);
    if (b > DMX_PT_WIN || b > out_off) return -1;
    return window[DMX_PT_WIN - b];
}

// The window-advance rule: byte k (0..32767) of the window behind a chunk of out_len bytes is
// entry *idx of the chunk's resolved tail (returns true), or byte *idx of the old window (false).
// A chunk of 32 768 bytes or more replaces the window with its tail; a shorter one shifts the old
// window by out_len and appends itself.
static inline DMX_PT_HD bool dmx_pt_next(uint32_t k, uint64_t out_len, uint32_t* idx) {
    if (out_len >= DMX_PT_WIN) {
        *idx = k;
        return true;
    }
    const uint32_t keep = DMX_PT_WIN - (uint32_t)out_len;
    if (k < keep) {
        *idx = k + (uint32_t)out_len;
        return false;
    }
    *idx = k - keep;
    return true;
}

// The pack rule for output position p of a chunk that begins at chunk_off: a byte cell is the byte;
// a reference reads cells[chunk_off - b], which the tail pass has resolved (it lies in the last
// 32 768 cells of an earlier chunk, because that chunk ends at or before chunk_off).  -1: the
// reference reaches before the first output byte, or its source is not a byte.
static inline DMX_PT_HD int dmx_pt_pack(const uint16_t* cells, uint64_t p, uint64_t chunk_off) {
    const uint32_t c = cells[p];
    if (c < DMX_PT_REF) return (int)c;
    const uint32_t b = dmx_pt_back(c);
    if (b > chunk_off) return -1;
    const uint32_t s = cells[chunk_off - b];
    return s < DMX_PT_REF ? (int)s : -1;
}

// dmx_pt_pack for a file of members (dmx_inflate_parallel_multi_decode_async): a reference may reach
// `limit` bytes in front of the chunk at most -- to its member's first byte; 0 behind a member start
// inside the chunk.  (dmx_pt_cell takes the same limit in place of out_off.)
static inline DMX_PT_HD int dmx_pt_pack_lim(const uint16_t* cells, uint64_t p, uint64_t chunk_off, uint64_t limit) {
    const uint32_t c = cells[p];
    if (c < DMX_PT_REF) return (int)c;
    const uint32_t b = dmx_pt_back(c);
    if (b > limit || b > chunk_off) return -1;
    const uint32_t s = cells[chunk_off - b];
    return s < DMX_PT_REF ? (int)s : -1;
}

#endif

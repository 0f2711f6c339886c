// dmx_gz_head.h -- the framing in front of a DEFLATE stream as deflate_decompress (dmx_inflate.c)
// reads it: which container the first bytes name, the zlib header checks and the gzip member header
// walk of gzip_header.  One text for the batch decoder (dmx_inflate_batch_kernel, dmx_inflate_dev.hip)
// and its host twin (tests/c/gz_head_model.cpp): both compile this file.  Host and device, C++ only,
// internal.
#ifndef DMX_GZ_HEAD_H
#define DMX_GZ_HEAD_H

#include <stdint.h>

#include "../../include/dmx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMX_GZ_HD __host__ __device__
#else
#define DMX_GZ_HD
#endif

// The gzip member header (RFC 1952 2.3) at in[0..n): ID1 ID2 CM FLG MTIME(4) XFL OS, then FEXTRA
// (XLEN + bytes), FNAME and FCOMMENT (zero-terminated), FHCRC (2 bytes, not checked).  ID1 / ID2 are
// the caller's (they chose this walk).  0 and *body = the offset of the DEFLATE data, or gzip_header's
// status: -E_ZCMPMT, -E_RESERV, and -E_ZHEAD for a header cut short.  Reads in[2..n) only.
DMX_GZ_HD static inline int dmx_gz_head(const uint8_t* in, uint64_t n, uint64_t* body) {
    if (n < 3) return -(int)E_ZHEAD;
    if (in[2] != 8) return -(int)E_ZCMPMT;
    if (n < 4) return -(int)E_ZHEAD;
    const uint32_t flg = in[3];
    if (flg & 0xE0) return -(int)E_RESERV;
    if (n < 10) return -(int)E_ZHEAD;
    uint64_t p = 10;
    if (flg & 4) {   // FEXTRA
        if (n - p < 2) return -(int)E_ZHEAD;
        const uint64_t xlen = (uint64_t)in[p] | ((uint64_t)in[p + 1] << 8);
        p += 2;
        if (n - p < xlen) return -(int)E_ZHEAD;
        p += xlen;
    }
    for (uint32_t f = 8; f <= 16; f <<= 1) {   // FNAME, FCOMMENT
        if (!(flg & f)) continue;
        while (p < n && in[p]) p++;
        if (p >= n) return -(int)E_ZHEAD;
        p++;
    }
    if (flg & 2) {   // FHCRC
        if (n - p < 2) return -(int)E_ZHEAD;
        p += 2;
    }
    *body = p;
    return 0;
}

// The framing of in[0..n) under fmt (DMX_BATCH_AUTO / ZLIB / GZIP / RAW): *format receives the
// container that is decoded (1, 2 or 3; under AUTO 1F 8B names gzip and anything else zlib,
// deflate_decompress's rule) and *body the offset of the DEFLATE data.  Returns 0 or the status
// deflate_decompress gives the same bytes before it reads a block.  A raw stream has no header: any
// n passes.  An explicit gzip whose first two bytes are not 1F 8B is -E_ZHEAD.
DMX_GZ_HD static inline int dmx_frame_head(const uint8_t* in, uint64_t n, uint32_t fmt, uint32_t* format,
                                           uint64_t* body) {
    *body = 0;
    *format = fmt == DMX_BATCH_AUTO ? DMX_BATCH_ZLIB : fmt;
    if (fmt == DMX_BATCH_RAW) return 0;
    if (n < 2) return -(int)E_ZHEAD;
    const uint32_t cmf = in[0], flg = in[1];
    const bool magic = cmf == 0x1F && flg == 0x8B;
    if (fmt == DMX_BATCH_AUTO && magic) *format = DMX_BATCH_GZIP;
    if (*format == DMX_BATCH_GZIP) {
        if (!magic) return -(int)E_ZHEAD;
        return dmx_gz_head(in, n, body);
    }
    if ((cmf & 0x0F) != 8) return -(int)E_ZCMPMT;
    if ((cmf >> 4) > 7) return -(int)E_ZSLWIN;
    if (((cmf << 8) | flg) % 31) return -(int)E_ZFCHCK;
    if (flg & 0x20) return -(int)E_ZPDICT;
    *body = 2;
    return 0;
}

// dmx_frame_head for a stream that may come with a preset dictionary (dmx_inflate_batch_dict_async;
// host twin: tests/c/frame_dict_model.cpp against dmx_inflate_dict_host).  have_dict / dict_adler: whether
// the caller gave this stream a dictionary, and the Adler-32 of all its bytes.  *primed: the window
// starts with the dictionary's tail -- a raw stream with a dictionary always (inflateSetDictionary on
// a raw stream), a zlib stream only where its header has FDICT and its DICTID (RFC 1950 2.2: four
// bytes behind FLG, most significant first) is dict_adler; then *body is 6.  A zlib stream without
// FDICT ignores the dictionary, a gzip member has none.  FDICT with the header cut inside the DICTID
// is -E_ZHEAD (before the dictionary is looked at); FDICT without a dictionary, or with another
// DICTID, -E_ZPDICT.  Everything else is dmx_frame_head's.  Reads in[0..6) at most, in[0..n) only.
DMX_GZ_HD static inline int dmx_frame_head_dict(const uint8_t* in, uint64_t n, uint32_t fmt, bool have_dict,
                                                uint32_t dict_adler, uint32_t* format, uint64_t* body, bool* primed) {
    *primed = false;
    *body = 0;
    *format = fmt == DMX_BATCH_AUTO ? DMX_BATCH_ZLIB : fmt;
    if (fmt == DMX_BATCH_RAW) {
        *primed = have_dict;
        return 0;
    }
    if (n < 2) return -(int)E_ZHEAD;
    const uint32_t cmf = in[0], flg = in[1];
    const bool magic = cmf == 0x1F && flg == 0x8B;
    if (fmt == DMX_BATCH_AUTO && magic) *format = DMX_BATCH_GZIP;
    if (*format == DMX_BATCH_GZIP) {
        if (!magic) return -(int)E_ZHEAD;
        return dmx_gz_head(in, n, body);
    }
    if ((cmf & 0x0F) != 8) return -(int)E_ZCMPMT;
    if ((cmf >> 4) > 7) return -(int)E_ZSLWIN;
    if (((cmf << 8) | flg) % 31) return -(int)E_ZFCHCK;
    if (!(flg & 0x20)) {
        *body = 2;
        return 0;
    }
    if (n < 6) return -(int)E_ZHEAD;
    const uint32_t dictid = ((uint32_t)in[2] << 24) | ((uint32_t)in[3] << 16) | ((uint32_t)in[4] << 8) | (uint32_t)in[5];
    if (!have_dict || dictid != dict_adler) return -(int)E_ZPDICT;
    *body = 6;
    *primed = true;
    return 0;
}

#endif

/*
 * dmx_inflate.c -- RFC 1950/1951 inflate behind the reference's
 * deflate_decompress() signature (src/include/deflate_ext.h:16).
 *
 * The reference implementation (src/deflate_decompress.c:371-409) does not compile
 * and decodes incorrectly (dangling else at :247-250, reverse_bits
 * off by 2x, Adler-32 read little-endian at :402, 256 garbage prefix bytes at
 * :382-384).  This is a fresh decoder with the same contract:
 *   - zlib header checks as deflate_decompress_header (:347-368): CM = 8, CINFO <= 7,
 *     FCHECK, no preset dictionary;
 *   - blocks until BFINAL (:391-397): stored (:303-314), fixed (:325-334), dynamic
 *     (form_d1/form_d2 :164-235);
 *   - Adler-32 trailer verified MSB-first (RFC 1950 §2.2);
 *   - output malloc'd into decompr_dat (caller frees), '\0' appended with
 *     DEFLATE_NULLTERM (:399).
 * Returns 0 or -E_*.  Decoding is canonical-Huffman by code-length counts (one bit
 * per step), with a 9-bit first-level lookup table for the common short codes.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dmx.h"
#include "dmx_crc.h"
#include "dmx_internal.h"

#define MAXBITS 15
#define FAST 9

typedef struct {
    const uint8_t* in;
    size_t n, pos;   /* byte position */
    uint64_t bitbuf;
    int bitcnt;
    uint8_t* out;
    size_t olen, ocap;
    int err;
} ist;

typedef struct {
    uint16_t count[MAXBITS + 1];
    uint16_t symbol[320];
    uint16_t fast[1 << FAST]; /* (len << 12) | sym, 0 = slow path */
} huff;

static inline int need(ist* s, int k) {
    while (s->bitcnt < k) {
        if (s->pos >= s->n) return 0;
        s->bitbuf |= (uint64_t)s->in[s->pos++] << s->bitcnt;
        s->bitcnt += 8;
    }
    return 1;
}

static inline int bits(ist* s, int k) {
    if (k == 0) return 0;
    if (!need(s, k)) { s->err = -E_LEN; return 0; }
    int v = (int)(s->bitbuf & ((1ull << k) - 1));
    s->bitbuf >>= k;
    s->bitcnt -= k;
    return v;
}

static int put(ist* s, uint8_t c) {
    if (s->olen == s->ocap) {
        size_t nc = s->ocap ? s->ocap * 2 : 1 << 16;
        uint8_t* no = (uint8_t*)realloc(s->out, nc + 1);
        if (!no) return -E_MALLOC;
        s->out = no;
        s->ocap = nc;
    }
    s->out[s->olen++] = c;
    return 0;
}

/* build a canonical decoder; returns 0 complete, >0 incomplete, <0 over-subscribed */
static int build(huff* h, const uint8_t* len, int n) {
    memset(h->count, 0, sizeof(h->count));
    for (int s = 0; s < n; s++) h->count[len[s]]++;
    if (h->count[0] == n) { memset(h->fast, 0, sizeof(h->fast)); return 0; }
    int left = 1;
    for (int l = 1; l <= MAXBITS; l++) {
        left <<= 1;
        left -= h->count[l];
        if (left < 0) return left;
    }
    uint16_t offs[MAXBITS + 1];
    offs[1] = 0;
    for (int l = 1; l < MAXBITS; l++) offs[l + 1] = offs[l] + h->count[l];
    for (int s = 0; s < n; s++)
        if (len[s]) h->symbol[offs[len[s]]++] = (uint16_t)s;
    /* first-level table: reversed canonical codes of length <= FAST */
    memset(h->fast, 0, sizeof(h->fast));
    int code = 0, idx = 0;
    for (int l = 1; l <= FAST; l++) {
        for (int k = 0; k < h->count[l]; k++, code++, idx++) {
            int r = 0;
            for (int b = 0; b < l; b++) r |= ((code >> b) & 1) << (l - 1 - b);
            for (int fill = r; fill < (1 << FAST); fill += 1 << l)
                h->fast[fill] = (uint16_t)((l << 12) | h->symbol[idx]);
        }
        code <<= 1;
    }
    return left;
}

/* Slow path: the canonical-code walk by per-length counts (first code / count / index per
 * length, one bit at a time) is the well-known loop of Mark Adler's puff.c (zlib
 * contrib/puff, zlib licence); restated here, it is not from the reference. */
static int decode(ist* s, const huff* h) {
    need(s, FAST);  /* may be short at the very end; the slow path copes */
    if (s->bitcnt >= FAST) {
        uint16_t e = h->fast[s->bitbuf & ((1u << FAST) - 1)];
        if (e) {
            int l = e >> 12;
            s->bitbuf >>= l;
            s->bitcnt -= l;
            return e & 0xFFF;
        }
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= MAXBITS; l++) {
        code |= bits(s, 1);
        if (s->err) return -1;
        int count = h->count[l];
        if (code - count < first) return h->symbol[index + (code - first)];
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    s->err = -(int)E_HUFINV;
    return -1;
}

static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31,
                                   35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385,
                                   513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

static int codes(ist* s, const huff* lh, const huff* dh) {
    for (;;) {
        int sym = decode(s, lh);
        if (s->err) return s->err;
        if (sym < 256) {
            int r = put(s, (uint8_t)sym);
            if (r) return r;
        } else if (sym == 256) {
            return 0;
        } else {
            sym -= 257;
            if (sym >= 29) return -(int)E_HUFVAL;
            int len = lbase[sym] + bits(s, lext[sym]);
            int ds = decode(s, dh);
            if (s->err) return s->err;
            if (ds < 0 || ds >= 30) return -(int)E_HUFVAL;
            size_t dist = (size_t)dbase[ds] + (size_t)bits(s, dext[ds]);
            if (s->err) return s->err;
            if (dist > s->olen) return -(int)E_HUFDIS;
            for (int k = 0; k < len; k++) {
                int r = put(s, s->out[s->olen - dist]);
                if (r) return r;
            }
        }
    }
}

static int stored(ist* s) {
    s->bitbuf >>= s->bitcnt & 7;  /* to a byte boundary */
    s->bitcnt -= s->bitcnt & 7;
    int len = bits(s, 16), nlen = bits(s, 16);
    if (s->err) return s->err;
    if (len != (~nlen & 0xFFFF)) return -(int)E_ZNLEN;
    for (int k = 0; k < len; k++) {
        int c = bits(s, 8);
        if (s->err) return s->err;
        int r = put(s, (uint8_t)c);
        if (r) return r;
    }
    return 0;
}

/* The fixed-code tables (RFC 1951 §3.2.6), built once: pthread_once makes concurrent
 * callers of deflate_decompress wait for the complete tables instead of reading a table
 * another thread is still writing. */
static huff fixed_lh, fixed_dh;
static pthread_once_t fixed_once = PTHREAD_ONCE_INIT;
static void fixed_build(void) {
    uint8_t l[288];
    for (int k = 0; k < 288; k++) l[k] = k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : 8;
    build(&fixed_lh, l, 288);
    for (int k = 0; k < 30; k++) l[k] = 5;
    build(&fixed_dh, l, 30);
}

static int fixed(ist* s) {
    pthread_once(&fixed_once, fixed_build);
    return codes(s, &fixed_lh, &fixed_dh);
}

static int dynamic(ist* s) {
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t len[320];
    huff lh, dh;
    int nlen = bits(s, 5) + 257, ndist = bits(s, 5) + 1, ncode = bits(s, 4) + 4;
    if (s->err) return s->err;
    if (nlen > 286 || ndist > 30) return -(int)E_ZINV;
    memset(len, 0, sizeof(len));
    for (int k = 0; k < ncode; k++) len[order[k]] = (uint8_t)bits(s, 3);
    if (s->err) return s->err;
    /* the code length code must be complete (an empty one is not a code either) */
    if (build(&lh, len, 19) != 0 || lh.count[0] == 19) return -(int)E_HUFAMB;
    int idx = 0;
    while (idx < nlen + ndist) {
        int sym = decode(s, &lh);
        if (s->err) return s->err;
        if (sym < 16) {
            len[idx++] = (uint8_t)sym;
        } else {
            int v = 0, rep;
            if (sym == 16) {
                if (idx == 0) return -(int)E_ZINV;
                v = len[idx - 1];
                rep = 3 + bits(s, 2);
            } else if (sym == 17) {
                rep = 3 + bits(s, 3);
            } else {
                rep = 11 + bits(s, 7);
            }
            if (s->err) return s->err;
            if (idx + rep > nlen + ndist) return -(int)E_ZINV;
            while (rep--) len[idx++] = (uint8_t)v;
        }
    }
    if (len[256] == 0) return -(int)E_ZINV;
    /* an incomplete code is allowed only as a single code of length 1 (zlib's rule and puff's);
     * a distance table without any code is legal until a length symbol needs it (-E_HUFINV) */
    int e = build(&lh, len, nlen);
    if (e < 0 || (e > 0 && !(nlen - lh.count[0] == 1 && lh.count[1] == 1))) return -(int)E_HUFAMB;
    e = build(&dh, len + nlen, ndist);
    if (e < 0 || (e > 0 && !(ndist - dh.count[0] == 1 && dh.count[1] == 1))) return -(int)E_HUFAMB;
    return codes(s, &lh, &dh);
}

static uint32_t adler32(const uint8_t* d, size_t n) {
    uint32_t a = 1, b = 0;
    while (n) {
        size_t k = n < 5552 ? n : 5552;
        n -= k;
        while (k--) { a += *d++; b += a; }
        a %= 65521u;
        b %= 65521u;
    }
    return (b << 16) | a;
}

/* CRC-32 (RFC 1952 §8), slice-by-4 tables built on first use (idempotent: every thread that
 * races writes the same values; the ready flag is published last). */
static uint32_t g_crc_tab[4][256];
static int g_crc_ready;
uint32_t dmx_crc32_host(uint32_t crc, const uint8_t* d, uint64_t n) {
    if (!__atomic_load_n(&g_crc_ready, __ATOMIC_ACQUIRE)) {
        for (uint32_t b = 0; b < 256; b++) {
            uint32_t c = b;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((0u - (c & 1u)) & DMX_CRC_POLY);
            g_crc_tab[0][b] = c;
        }
        for (int k = 1; k < 4; k++)
            for (uint32_t b = 0; b < 256; b++)
                g_crc_tab[k][b] = (g_crc_tab[k - 1][b] >> 8) ^ g_crc_tab[0][g_crc_tab[k - 1][b] & 0xFFu];
        __atomic_store_n(&g_crc_ready, 1, __ATOMIC_RELEASE);
    }
    uint32_t c = ~crc;
    while (n >= 4) {
        c ^= (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24);
        c = g_crc_tab[3][c & 0xFFu] ^ g_crc_tab[2][(c >> 8) & 0xFFu] ^ g_crc_tab[1][(c >> 16) & 0xFFu] ^ g_crc_tab[0][c >> 24];
        d += 4;
        n -= 4;
    }
    while (n--) c = g_crc_tab[0][(c ^ *d++) & 0xFFu] ^ (c >> 8);
    return ~c;
}

/* The gzip member header (RFC 1952 §2.3) at in[0..n): ID1 ID2 CM FLG MTIME(4) XFL OS, then
 * FEXTRA (XLEN + bytes), FNAME and FCOMMENT (zero-terminated), FHCRC (2 bytes, not checked).
 * Returns the offset of the DEFLATE data, or -E_* (a header cut short: -E_ZHEAD). */
static long gzip_header(const uint8_t* in, size_t n, size_t* body) {
    if (n < 3) return -(long)E_ZHEAD;
    if (in[2] != 8) return -(long)E_ZCMPMT;
    if (n < 4) return -(long)E_ZHEAD;
    const int flg = in[3];
    if (flg & 0xE0) return -(long)E_RESERV;
    if (n < 10) return -(long)E_ZHEAD;
    size_t p = 10;
    if (flg & 4) {   /* FEXTRA */
        if (n - p < 2) return -(long)E_ZHEAD;
        const size_t xlen = (size_t)in[p] | ((size_t)in[p + 1] << 8);
        p += 2;
        if (n - p < xlen) return -(long)E_ZHEAD;
        p += xlen;
    }
    for (int f = 8; f <= 16; f <<= 1) {   /* FNAME, FCOMMENT */
        if (!(flg & f)) continue;
        while (p < n && in[p]) p++;
        if (p >= n) return -(long)E_ZHEAD;
        p++;
    }
    if (flg & 2) {   /* FHCRC */
        if (n - p < 2) return -(long)E_ZHEAD;
        p += 2;
    }
    *body = p;
    return 0;
}

/* The blocks of a stream from the reader's position until BFINAL; shared by deflate_decompress and
 * dmx_inflate_dict_host.  Returns 0 or the status of the first block that fails. */
static int inflate_blocks(ist* s) {
    int last, r = 0;
    do {
        last = bits(s, 1);
        int type = bits(s, 2);
        if (s->err) { r = s->err; break; }
        if (type == 0) r = stored(s);
        else if (type == 1) r = fixed(s);
        else if (type == 2) r = dynamic(s);
        else r = -(int)E_ZBTYPE;
        if (r) break;
    } while (!last);
    return r;
}

/* The trailer behind the last block, for the output o[0, on): the partial byte is dropped; then gzip's
 * CRC-32 and ISIZE, little-endian (a trailer cut short is -E_CRC, the CRC is checked first), or
 * zlib's big-endian Adler-32 (-E_ZADL32, cut short too).  Bytes after the trailer are ignored. */
static int inflate_trailer(ist* s, int gz, const uint8_t* o, size_t on) {
    s->bitbuf >>= s->bitcnt & 7;
    s->bitcnt -= s->bitcnt & 7;
    if (gz) {
        uint32_t want = 0, isize = 0;
        for (int k = 0; k < 4; k++) want |= (uint32_t)bits(s, 8) << (8 * k);
        for (int k = 0; k < 4; k++) isize |= (uint32_t)bits(s, 8) << (8 * k);
        if (s->err) return -(int)E_CRC;
        if (want != dmx_crc32_host(0, o, on)) return -(int)E_CRC;
        if (isize != (uint32_t)on) return -(int)E_LEN;
        return 0;
    }
    uint32_t want = 0;
    for (int k = 0; k < 4; k++) want = (want << 8) | (uint32_t)bits(s, 8);
    if (s->err) return -(int)E_ZADL32;
    if (want != adler32(o, on)) return -(int)E_ZADL32;
    return 0;
}

int deflate_decompress(struct string_len* decompr_dat, struct string_len* compr_dat, int ops) {
    if (!decompr_dat || !compr_dat || (!compr_dat->str && compr_dat->len)) return -E_INVAL;
    ist s;
    memset(&s, 0, sizeof(s));
    s.in = compr_dat->str;
    s.n = compr_dat->len;
    decompr_dat->str = NULL;
    decompr_dat->len = 0;
    if (s.n < 2) return -(int)E_ZHEAD;
    const int cmf = s.in[0], flg = s.in[1];
    const int gz = cmf == 0x1F && flg == 0x8B;   /* a gzip member (as zlib it would be CM 15) */
    if (gz) {
        size_t body = 0;
        const long e = gzip_header(s.in, s.n, &body);
        if (e) return (int)e;
        s.pos = body;
    } else {
        if ((cmf & 0x0F) != 8) return -(int)E_ZCMPMT;
        if ((cmf >> 4) > 7) return -(int)E_ZSLWIN;
        if (((cmf << 8) | flg) % 31) return -(int)E_ZFCHCK;
        if (flg & 0x20) return -(int)E_ZPDICT;
        s.pos = 2;
    }
    int r = inflate_blocks(&s);
    if (!r) r = inflate_trailer(&s, gz, s.out, s.olen);
    if (r) {
        free(s.out);
        return r;
    }
    if (!s.out) {
        s.out = (uint8_t*)malloc(1);
        if (!s.out) return -E_MALLOC;
    }
    if (ops & DEFLATE_NULLTERM) s.out[s.olen] = 0;  /* buffer always has one spare byte */
    decompr_dat->str = s.out;
    decompr_dat->len = s.olen;
    return 0;
}

/* One stream of dmx_inflate_batch_dict_async on the host (include/dmx.h): the framing under fmt
 * (DMX_BATCH_*), a preset dictionary where the stream takes one -- a raw stream always, a zlib
 * stream whose header has FDICT and whose DICTID is the Adler-32 of all dict_len bytes -- and the
 * trailer.  The dictionary's last min(dict_len, 32768) bytes are put in front of the output, so a
 * distance reaches them as it reaches earlier output, and are taken off at the end; the trailer's
 * check covers the output alone.  deflate_decompress's statuses, and -E_ZPDICT for FDICT without a
 * dictionary or with another DICTID, -E_ZHEAD for a header cut inside the DICTID. */
int dmx_inflate_dict_host(const void* z, uint64_t n, uint32_t fmt, const void* dict, uint64_t dict_len, void** out,
                          uint64_t* out_len, uint64_t* in_used) {
    if (!out || !out_len || (!z && n) || (!dict && dict_len) || fmt > DMX_BATCH_RAW) return -(int)E_INVAL;
    *out = NULL;
    *out_len = 0;
    if (in_used) *in_used = 0;
    ist s;
    memset(&s, 0, sizeof(s));
    s.in = (const uint8_t*)z;
    s.n = (size_t)n;
    uint32_t format = fmt == DMX_BATCH_AUTO ? DMX_BATCH_ZLIB : fmt;
    int primed = 0;
    if (fmt == DMX_BATCH_RAW) {
        primed = dict != NULL;
    } else {
        if (s.n < 2) return -(int)E_ZHEAD;
        const int cmf = s.in[0], flg = s.in[1];
        const int magic = cmf == 0x1F && flg == 0x8B;
        if (fmt == DMX_BATCH_AUTO && magic) format = DMX_BATCH_GZIP;
        if (format == DMX_BATCH_GZIP) {
            if (!magic) return -(int)E_ZHEAD;
            size_t body = 0;
            const long e = gzip_header(s.in, s.n, &body);
            if (e) return (int)e;
            s.pos = body;
        } else {
            if ((cmf & 0x0F) != 8) return -(int)E_ZCMPMT;
            if ((cmf >> 4) > 7) return -(int)E_ZSLWIN;
            if (((cmf << 8) | flg) % 31) return -(int)E_ZFCHCK;
            s.pos = 2;
            if (flg & 0x20) {
                if (s.n < 6) return -(int)E_ZHEAD;
                const uint32_t id = ((uint32_t)s.in[2] << 24) | ((uint32_t)s.in[3] << 16) | ((uint32_t)s.in[4] << 8) | s.in[5];
                if (!dict || id != adler32((const uint8_t*)dict, (size_t)dict_len)) return -(int)E_ZPDICT;
                s.pos = 6;
                primed = 1;
            }
        }
    }
    const size_t dl = primed ? (size_t)(dict_len < DMX_BLK ? dict_len : DMX_BLK) : 0;
    int r = 0;
    if (dl) {
        s.ocap = dl + (1 << 16);
        s.out = (uint8_t*)malloc(s.ocap + 1);
        if (!s.out) return -E_MALLOC;
        memcpy(s.out, (const uint8_t*)dict + (dict_len - dl), dl);
        s.olen = dl;
    }
    r = inflate_blocks(&s);
    if (!r && format == DMX_BATCH_RAW) {   /* a raw stream ends at the next byte: no trailer */
        s.bitbuf >>= s.bitcnt & 7;
        s.bitcnt -= s.bitcnt & 7;
    } else if (!r) {                       /* the check covers the output alone */
        r = inflate_trailer(&s, format == DMX_BATCH_GZIP, s.out ? s.out + dl : NULL, s.olen - dl);
    }
    if (r) {
        free(s.out);
        return r;
    }
    if (!s.out) {
        s.out = (uint8_t*)malloc(1);
        if (!s.out) return -E_MALLOC;
    }
    if (dl) memmove(s.out, s.out + dl, s.olen - dl);
    *out = s.out;
    *out_len = s.olen - dl;
    if (in_used) *in_used = (uint64_t)s.pos - (uint64_t)(s.bitcnt / 8);
    return 0;
}

/* The seek-point index of one foreign stream (include/dmx.h: dmx_zindex_build_host; DESIGN.md §3.1
 * "Seek points"): one serial, exact decode with the block routines above, a point at the first block
 * boundary at which the output since the point before is >= span.  The output is not kept: at a block
 * boundary, once it has passed ZX_KEEP bytes, the buffer is cut back to its last 32 KiB (all a
 * distance reaches, and all a point's window needs), so the builder holds the largest block plus
 * ZX_KEEP + 32 KiB at most; the checks (Adler-32 per point, Adler-32 or CRC-32 + ISIZE of the stream)
 * are folded block by block in front of the cut. */
#define ZX_KEEP (1u << 20)

static uint32_t adler32_more(uint32_t adl, const uint8_t* d, size_t n) {
    uint32_t a = adl & 0xFFFFu, b = adl >> 16;
    while (n) {
        size_t k = n < 5552 ? n : 5552;
        n -= k;
        while (k--) { a += *d++; b += a; }
        a %= 65521u;
        b %= 65521u;
    }
    return (b << 16) | a;
}

typedef struct {
    dmx_zpoint* pts;
    uint32_t* adl;
    uint8_t* win;
    uint64_t n, cap;
} zx_arrays;

/* point n = {bit, 0, out_off, 0} with the window in front of out_off: the last wlen bytes of
 * buf[0, blen), right-aligned in the slot */
static int zx_push(zx_arrays* a, uint64_t bit, uint64_t out_off, const uint8_t* buf, size_t blen) {
    if (a->n == 0xFFFFFFFFull) return -(int)E_RANGE;
    if (a->n == a->cap) {
        const uint64_t nc = a->cap ? a->cap * 2 : 16;
        dmx_zpoint* p = (dmx_zpoint*)realloc(a->pts, nc * sizeof(dmx_zpoint));
        if (p) a->pts = p;
        uint32_t* q = (uint32_t*)realloc(a->adl, nc * sizeof(uint32_t));
        if (q) a->adl = q;
        uint8_t* w = (uint8_t*)realloc(a->win, nc * (uint64_t)DMX_ZINDEX_WINDOW);
        if (w) a->win = w;
        if (!p || !q || !w) return -(int)E_MALLOC;
        a->cap = nc;
    }
    const size_t wlen = out_off < DMX_ZINDEX_WINDOW ? (size_t)out_off : DMX_ZINDEX_WINDOW;
    uint8_t* slot = a->win + a->n * (uint64_t)DMX_ZINDEX_WINDOW;
    memset(slot, 0, DMX_ZINDEX_WINDOW - wlen);
    if (wlen) memcpy(slot + (DMX_ZINDEX_WINDOW - wlen), buf + (blen - wlen), wlen);
    a->pts[a->n].bit = bit;
    a->pts[a->n].end_bit = 0;
    a->pts[a->n].out_off = out_off;
    a->pts[a->n].out_len = 0;
    a->adl[a->n] = 1;
    a->n++;
    return 0;
}

int dmx_zindex_build_host(const void* z, uint64_t zbytes, uint32_t fmt, uint32_t span, dmx_zpoint** points,
                          uint32_t** adlers, uint8_t** windows, dmx_zindex_status* st) {
    if (!st || !points || !adlers || !windows || (!z && zbytes) || fmt > DMX_BATCH_RAW) return -(int)E_INVAL;
    if (span > DMX_ZINDEX_MAX_SPAN) return -(int)E_RANGE;
    *points = NULL;
    *adlers = NULL;
    *windows = NULL;
    memset(st, 0, sizeof(*st));
    st->span = span ? span : DMX_ZINDEX_DEF_SPAN;
    st->format = fmt == DMX_BATCH_AUTO ? DMX_BATCH_ZLIB : fmt;
    ist s;
    memset(&s, 0, sizeof(s));
    s.in = (const uint8_t*)z;
    s.n = (size_t)zbytes;
    /* the framing, as dmx_frame_head (dmx_gz_head.h) and deflate_decompress read it */
    if (fmt != DMX_BATCH_RAW) {
        if (s.n < 2) { st->status = -(int)E_ZHEAD; return 0; }
        const int cmf = s.in[0], flg = s.in[1];
        const int magic = cmf == 0x1F && flg == 0x8B;
        if (fmt == DMX_BATCH_AUTO && magic) st->format = DMX_BATCH_GZIP;
        if (st->format == DMX_BATCH_GZIP) {
            size_t body = 0;
            const long e = magic ? gzip_header(s.in, s.n, &body) : -(long)E_ZHEAD;
            if (e) { st->status = (int)e; return 0; }
            s.pos = body;
        } else {
            int e = 0;
            if ((cmf & 0x0F) != 8) e = -(int)E_ZCMPMT;
            else if ((cmf >> 4) > 7) e = -(int)E_ZSLWIN;
            else if (((cmf << 8) | flg) % 31) e = -(int)E_ZFCHCK;
            else if (flg & 0x20) e = -(int)E_ZPDICT;
            if (e) { st->status = e; return 0; }
            s.pos = 2;
        }
    }
    const int gz = st->format == DMX_BATCH_GZIP;
    zx_arrays a;
    memset(&a, 0, sizeof(a));
    uint64_t total = 0;        /* output bytes in front of s.out[0] plus s.olen: see done */
    uint64_t cut = 0;          /* output bytes no longer in the buffer */
    size_t done = 0;           /* s.out[0, done) is folded into the checks */
    uint32_t whole = gz ? 0u : 1u;   /* the stream's CRC-32 / Adler-32 so far */
    int r = zx_push(&a, 8ull * s.pos, 0, NULL, 0), last = 0;
    while (!r && !last) {
        last = bits(&s, 1);
        const int type = bits(&s, 2);
        if (s.err) { r = s.err; break; }
        if (type == 0) r = stored(&s);
        else if (type == 1) r = fixed(&s);
        else if (type == 2) r = dynamic(&s);
        else r = -(int)E_ZBTYPE;
        if (r) break;
        /* the block's bytes: into the point's Adler-32 and the stream's check */
        dmx_zpoint* p = &a.pts[a.n - 1];
        const size_t nb = s.olen - done;
        if (nb) {
            a.adl[a.n - 1] = adler32_more(a.adl[a.n - 1], s.out + done, nb);
            whole = gz ? dmx_crc32_host(whole, s.out + done, nb) : adler32_more(whole, s.out + done, nb);
            p->out_len += nb;
            done = s.olen;
        }
        total = cut + s.olen;
        const uint64_t bit = 8ull * s.pos - (uint64_t)s.bitcnt;
        if (!last && p->out_len >= st->span) {   /* the next block's BFINAL bit starts a point */
            p->end_bit = bit;
            r = zx_push(&a, bit, total, s.out, s.olen);
        } else if (last) {
            p->end_bit = bit;
        }
        if (s.olen >= ZX_KEEP + DMX_ZINDEX_WINDOW) {   /* keep what a distance can still reach */
            memmove(s.out, s.out + (s.olen - DMX_ZINDEX_WINDOW), DMX_ZINDEX_WINDOW);
            cut += s.olen - DMX_ZINDEX_WINDOW;
            s.olen = done = DMX_ZINDEX_WINDOW;
        }
    }
    if (!r) {   /* the trailer, as inflate_trailer checks it */
        s.bitbuf >>= s.bitcnt & 7;
        s.bitcnt -= s.bitcnt & 7;
        uint32_t want = 0, isize = 0;
        if (gz) {
            for (int k = 0; k < 4; k++) want |= (uint32_t)bits(&s, 8) << (8 * k);
            for (int k = 0; k < 4; k++) isize |= (uint32_t)bits(&s, 8) << (8 * k);
            if (s.err || want != whole) r = -(int)E_CRC;
            else if (isize != (uint32_t)total) r = -(int)E_LEN;
        } else if (st->format == DMX_BATCH_ZLIB) {
            for (int k = 0; k < 4; k++) want = (want << 8) | (uint32_t)bits(&s, 8);
            if (s.err || want != whole) r = -(int)E_ZADL32;
        }
        st->check = want;
    }
    free(s.out);
    if (r) {
        free(a.pts);
        free(a.adl);
        free(a.win);
        if (r == -(int)E_MALLOC || r == -(int)E_RANGE) return r;   /* the builder's own, not the stream's */
        st->status = r;
        st->check = 0;
        return 0;
    }
    st->out_len = total;
    st->in_used = (uint64_t)s.pos - (uint64_t)(s.bitcnt / 8);
    st->npoints = (uint32_t)a.n;
    /* the arrays grew by doubling: give back what is not used (a realloc that fails leaves them as they are) */
    void* t;
    if ((t = realloc(a.pts, a.n * sizeof(dmx_zpoint)))) a.pts = (dmx_zpoint*)t;
    if ((t = realloc(a.adl, a.n * sizeof(uint32_t)))) a.adl = (uint32_t*)t;
    if ((t = realloc(a.win, a.n * (uint64_t)DMX_ZINDEX_WINDOW))) a.win = (uint8_t*)t;
    *points = a.pts;
    *adlers = a.adl;
    *windows = a.win;
    return 0;
}

/* The block index of a BGZF file (SAM/BAM specification §4.1; include/dmx.h): a series of gzip
 * members with FEXTRA set, each carrying its own size - 1 as BSIZE in the "BC" subfield
 * (SI1 'B', SI2 'C', SLEN 2), so the walk reads headers and trailers only.  The DEFLATE data
 * of a member starts behind its header (gzip_header: FNAME / FCOMMENT / FHCRC are skipped if a
 * writer set them) and its trailer is the member's last 8 bytes. */
int dmx_bgzf_index_max(const uint8_t* z, uint64_t zlen, uint32_t max_isize, dmx_iblock* idx, uint32_t* crc,
                       uint32_t cap, uint32_t* nblk, uint64_t* out_len) {
    if ((!z && zlen) || !nblk || (!idx && cap)) return -(int)E_INVAL;
    uint64_t p = 0, total = 0, cnt = 0;
    *nblk = 0;
    if (out_len) *out_len = 0;
    if (max_isize < 1 || max_isize > DMX_BGZF_MAX_ISIZE) return -(int)E_RANGE;
    while (p < zlen) {
        const uint8_t* m = z + p;
        const uint64_t left = zlen - p;
        if (left < 12) {   /* the fixed header and XLEN: is what is there a gzip / deflate / FEXTRA member at all? */
            if (m[0] != 0x1F || (left > 1 && m[1] != 0x8B) || (left > 2 && m[2] != 8) || (left > 3 && !(m[3] & 4)))
                return -(int)E_ZHEAD;
            return -(int)E_LEN;
        }
        if (m[0] != 0x1F || m[1] != 0x8B || m[2] != 8 || !(m[3] & 4) || (m[3] & 0xE0)) return -(int)E_ZHEAD;
        const uint64_t xlen = (uint64_t)m[10] | ((uint64_t)m[11] << 8);
        if (left < 12 + xlen) return -(int)E_LEN;
        uint64_t bsize = 0;
        int found = 0;
        for (uint64_t q = 12; q + 4 <= 12 + xlen;) {   /* the subfields: SI1 SI2 SLEN(2) data */
            const uint64_t slen = (uint64_t)m[q + 2] | ((uint64_t)m[q + 3] << 8);
            if (q + 4 + slen > 12 + xlen) break;   /* a subfield past XLEN: no BC found in a sound one */
            if (m[q] == 'B' && m[q + 1] == 'C' && slen == 2) {
                bsize = ((uint64_t)m[q + 4] | ((uint64_t)m[q + 5] << 8)) + 1;
                found = 1;
                break;
            }
            q += 4 + slen;
        }
        if (!found) return -(int)E_ZHEAD;
        if (left < bsize) return -(int)E_LEN;
        size_t body = 0;
        const long e = gzip_header(m, (size_t)bsize, &body);   /* (the member alone: nothing behind it is read) */
        if (e) return -(int)E_ZHEAD;
        if ((uint64_t)body + 8 > bsize) return -(int)E_ZHEAD;   /* BSIZE leaves no room for the trailer */
        const uint8_t* t = m + bsize - 8;
        const uint32_t mcrc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        if (isize > max_isize) return -(int)E_RANGE;
        if (isize) {
            if (cnt < cap) {
                idx[cnt].bit = 8 * (p + (uint64_t)body);
                idx[cnt].out_off = total;
                idx[cnt].out_len = isize;
                idx[cnt].reserved = 0;
                if (crc) crc[cnt] = mcrc;
            }
            cnt++;
            if (cnt > 0xFFFFFFFFull) return -(int)E_RANGE;
            total += isize;
        }
        p += bsize;
    }
    *nblk = (uint32_t)cnt;
    if (out_len) *out_len = total;
    return cnt > cap ? -(int)E_SZ : 0;
}

/* the members the one-wave-per-block decoder of dmx_inflate_async takes: ISIZE <= 32768 */
int dmx_bgzf_index(const uint8_t* z, uint64_t zlen, dmx_iblock* idx, uint32_t* crc, uint32_t cap, uint32_t* nblk,
                   uint64_t* out_len) {
    return dmx_bgzf_index_max(z, zlen, DMX_BLK, idx, crc, cap, nblk, out_len);
}

/*
 * dmx.h -- C-ABI of libdmx, the MI355X-native DEFLATE encoder.
 *
 * Part 1 is the drop-in boundary: the exact entry points of the reference's public
 * codec API, src/include/deflate_ext.h of mparker97/deflate_compression, so a C
 * caller of the reference links against libdmx.so unchanged.
 * Part 2 is the device layer those entry points call: device-resident buffers,
 * explicit HIP streams, no allocation inside an encode (graph-capturable).
 *
 * All signatures are plain C types; no torch types cross this boundary.
 */
#ifndef DMX_H
#define DMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ======================= Part 1: reference API (deflate_ext.h) ======================= */

/* deflate_ext.h:6 -- deflate_decompress option: append a '\0' after the output */
#define DEFLATE_NULLTERM 1

/* deflate_ext.h:8 -- sliding-window index / window size type */
typedef unsigned short swi;

/* globals.h:42-46 -- byte string with explicit length */
struct string_len {
    unsigned char* str;
    size_t len;
};

/* deflate_ext.h:10-14 -- opaque compressor state + spawn/init/deinit.
 * Replaces struct deflate_compr (deflate_compress.c:69-81) and SPAWNABLE
 * (globals.h:20-29).  init never longjmps; errors surface from deflate_compress. */
typedef struct deflate_compr deflate_compr_t;
deflate_compr_t* spawn_deflate_compr_t(void);
void deflate_compr_init(deflate_compr_t* com, int fd_in, int fd_out, int fd_stats, swi sw);
void deflate_compr_deinit(deflate_compr_t* com);

/* deflate_ext.h:17, impl deflate_compress.c:362-376.
 * Reads fd_in to EOF, writes a zlib stream (RFC 1950/1951) to fd_out -- or, with
 * DMX_FORMAT=gzip in the environment, one gzip member (RFC 1952) around the same DEFLATE
 * data, or with DMX_FORMAT=bgzf a BGZF file (DMX_F_BGZF: a gzip member per sw block and the
 * end-of-file member; with DMX_DICT or DMX_SPLIT that is -E_INVAL); unset or "zlib" is the zlib
 * stream, any other value returns -E_INVAL before anything is read or written -- and if
 * fd_stats >= 0 one 24-byte struct compress_stats per token.  sw = block size /
 * window (1..32768; 0 means 32768).  ops is unused (as in the reference).
 * The parse is the reference's: exhaustive hash-chain search, greedy, longest
 * match >= 3, ties to the nearest (DMX_MAX_CHAIN=K in the environment selects the
 * bounded fast mode).  Returns 0, or -E_* on error (the reference returned
 * nothing).  The encode runs on the MI355X (device DMX_DEVICE, default 0); there is
 * no CPU fallback: without a usable GPU it fails with -E_NEXIST. */
int deflate_compress(int fd_in, int fd_out, int fd_stats, swi sw, int ops);

/* deflate_ext.h:16, impl deflate_decompress.c:371-409 (that implementation does not
 * compile; this one is a fresh RFC 1950/1951 inflate).
 * Inflates compr_dat (zlib stream, or a gzip member when it begins 1F 8B: optional
 * FEXTRA / FNAME / FCOMMENT / FHCRC fields skipped, CRC-32 (-E_CRC) and ISIZE (-E_LEN)
 * checked, bytes after the first member ignored) into a malloc'd decompr_dat->str that the
 * caller frees.  ops & DEFLATE_NULLTERM appends a '\0' (not counted in len).
 * Returns 0 or -E_*.  zlib decides what is a stream; a rejected one has this status, the same
 * from dmx_inflate_async's stream mode (tests/test_inflate_conformance.py):
 *   -E_ZHEAD    fewer than 2 bytes (or a gzip header cut short)
 *   -E_ZCMPMT / -E_ZSLWIN / -E_ZFCHCK / -E_ZPDICT   the zlib header: CM, CINFO, FCHECK, FDICT (here
 *               always: this call has no dictionary to give; dmx_inflate_batch_dict_async and
 *               dmx_inflate_dict_host take one, and there it means "none given, or another DICTID")
 *   -E_LEN      the input ends inside the DEFLATE data, whatever would have followed
 *   -E_ZBTYPE   BTYPE 3;   -E_ZNLEN  stored LEN != ~NLEN
 *   -E_ZINV     HLIT > 286, HDIST > 30, a 16 with no length before it, a repeat past
 *               HLIT + HDIST, no code for the end of block
 *   -E_HUFAMB   an over-subscribed code, or an incomplete one: the code length code must be
 *               complete; a literal/length or distance code may be incomplete only as a single
 *               code of length 1; a distance table without codes is legal until a length needs it
 *   -E_HUFINV   a bit pattern that is no code (the unused code of a single-code table, a length
 *               with an empty distance table, the fixed distance symbols 30 / 31), where the 15
 *               bits that show it are there (else -E_LEN)
 *   -E_HUFVAL   a decoded symbol out of range: the fixed code's 286 / 287
 *   -E_HUFDIS   a distance before the first output byte
 *   -E_ZADL32   a wrong Adler-32 or a stream cut inside it; bytes after the trailer are ignored */
int deflate_decompress(struct string_len* decompr_dat, struct string_len* compr_dat, int ops);

/* deflate_ext.h:19-31 -- per-token record written to fd_stats.
 * bytes = 1 + input offset of the token; ll/d = literal byte (d == 0) or length/
 * distance.  The *_bits fields depend on DMX_STATS in the environment:
 *   unset / "ref"  the reference's own estimates (deflate_compress.c:290-298): tree_bits =
 *                  the code-length description cost of its adaptive Huffman trees
 *                  (h_tree.c:75-148) + the code-length code's weighted depth (:242-302),
 *                  ll_bits / d_bits = the adaptive trees' scores after this token
 *                  (aht.c:239-277), running over the whole stream as in the reference.
 *                  Same records as the reference for the same tokens (dmx_refest_*).
 *                  Parity unpinned past one window: the reference itself is only correct
 *                  for its first 32 KiB window, so records of later blocks
 *                  are checked against this host restatement fed the oracle's tokens, not
 *                  against the reference's own output.
 *   "exact"        exact costs of this stream, running over the whole stream: tree_bits =
 *                  header bits of every DEFLATE block begun so far (its own included;
 *                  the empty stored blocks that end each DMX_CHUNK_MB chunk but the last
 *                  are framing, not coding, and are not counted),
 *                  ll_bits = lit/len code + length extra bits of every token so far (8 per
 *                  byte in stored blocks), d_bits = distance code + extra bits so far.
 * The fields are int, as in the reference: deflate_compress returns -E_RANGE, after the
 * complete stream to fd_out and every record before it, at the first record whose bytes
 * or *_bits would exceed INT_MAX (inputs past 2 GiB, or about 2^31 bits of running sum). */
struct compress_stats {
    int bytes;
    int tree_bits;
    int ll_bits;
    int d_bits;
    int ll;
    int d;
};

/* Error codes: src/include/global_errors.h:24-35 and src/include/deflate_errors.h:9-22 (returned negated). */
#define E_LEN 1
#define E_MALLOC 2
#define E_FORK 3
#define E_PIPE 4
#define E_CRC 5
#define E_SZ 6
#define E_EXIST 7
#define E_NEXIST 8
#define E_NONULL 9
#define E_RANGE 10
#define E_INVAL 11
#define E_RESERV 12
#define DEFLATE_ERROR_MASK (1U << 24)
#define E_HUFAMB (DEFLATE_ERROR_MASK + 1)
#define E_HUFINV (DEFLATE_ERROR_MASK + 2)
#define E_HUFVAL (DEFLATE_ERROR_MASK + 3)
#define E_HUFDIS (DEFLATE_ERROR_MASK + 4)
#define E_ZADL32 (DEFLATE_ERROR_MASK + 5)
#define E_ZHEAD (DEFLATE_ERROR_MASK + 6)
#define E_ZFCHCK (DEFLATE_ERROR_MASK + 7)
#define E_ZCMPMT (DEFLATE_ERROR_MASK + 8)
#define E_ZSLWIN (DEFLATE_ERROR_MASK + 9)
#define E_ZPDICT (DEFLATE_ERROR_MASK + 10)
#define E_ZBSZ (DEFLATE_ERROR_MASK + 11)
#define E_ZNLEN (DEFLATE_ERROR_MASK + 12)
#define E_ZINV (DEFLATE_ERROR_MASK + 13)
#define E_ZBTYPE (DEFLATE_ERROR_MASK + 14)
/* dmx additions (outside both reference ranges) */
#define E_DEVICE (DEFLATE_ERROR_MASK + 64) /* HIP runtime / launch failure */

/* ============================ Part 2: device layer ============================ */

/* Stream framing flags (dmx_opts.flags). DMX_ZLIB = a complete zlib stream, DMX_GZIP = a
 * complete gzip member (RFC 1952). */
#define DMX_F_HEADER 1u  /* write the container header: zlib 78 9C (2 bytes); with DMX_F_GZIP
                            1F 8B 08 00 00 00 00 00 00 FF (10 bytes: no name, mtime 0, XFL 0,
                            OS 255, so the output is deterministic) */
#define DMX_F_TRAILER 2u /* write the trailer: Adler-32 big-endian (4 bytes); with DMX_F_GZIP
                            CRC-32 then the input length mod 2^32, both little-endian (8 bytes) */
#define DMX_F_FINAL 4u   /* last block carries BFINAL; otherwise the stream ends with
                            an empty stored block (sync flush) so it is byte-aligned
                            and another shard can be appended */
#define DMX_ZLIB (DMX_F_HEADER | DMX_F_TRAILER | DMX_F_FINAL)
#define DMX_F_GZIP 512u  /* container option: DMX_F_HEADER and DMX_F_TRAILER mean the gzip ones
                            and the stream's check value is the CRC-32 of the input (computed on
                            the device on the encode's stream, csrc/dmx_crc.hip), also when no
                            trailer is written (shards: dmx_result.adler, dmx_crc32_combine).
                            The DEFLATE data is bit for bit that of the zlib stream. */
#define DMX_GZIP (DMX_ZLIB | DMX_F_GZIP)
#define DMX_F_BGZF 1024u /* container option: BGZF (SAM/BAM specification §4.1), blocked gzip -- every
                            sw block becomes a complete gzip member of its own: an 18-byte header
                            (1F 8B 08 04, mtime 0, XFL 0, OS 255, XLEN 6, the "BC" subfield with
                            BSIZE = member size - 1), the block's DEFLATE data from a byte boundary
                            with BFINAL set and zero bits up to the next one, then the CRC-32
                            (per block, csrc/dmx_crc.hip) and byte count of the block.  The DEFLATE
                            data is that of the zlib stream of the block alone (same parse, block
                            type and codes).  DMX_F_HEADER, DMX_F_TRAILER and DMX_F_GZIP are
                            ignored: every member frames itself.  DMX_F_FINAL appends the 28-byte
                            end-of-file member; without it nothing follows the last member (no
                            sync flush: members concatenate as they are).  An empty input gives the
                            end-of-file member alone, or nothing.  Any gzip reader decompresses
                            the output; dmx_bgzf_index finds the members for the GPU inflate.
                            DMX_F_DICT (members would depend on each other) and DMX_F_SPLIT (left
                            out so far) return -E_INVAL with it.  dmx_result: adler is 0 (no
                            stream-wide check value), end_bits = 8 x the offset just past the last
                            data member, out_len includes the end-of-file member.  dmx_block_index:
                            bit = first bit of the member's DEFLATE data, 8 x (member offset + 18). */
#define DMX_BGZF (DMX_F_BGZF | DMX_F_FINAL)
#define DMX_F_FDICT 2048u /* container option: the zlib header names the dictionary of a DMX_F_DICT
                            encode (RFC 1950 2.2) -- 78 BB and the DICTID, the Adler-32 of
                            opts->dict[0, dict_len) most significant byte first, 6 bytes instead of 2,
                            so that zlib.decompressobj(zdict=dict), inflateSetDictionary and
                            dmx_inflate_batch_dict_async decode the stream.  The DICTID is computed
                            on the device on the encode's stream.  Valid only with DMX_F_DICT and
                            DMX_F_HEADER, without DMX_F_GZIP and DMX_F_BGZF, with opts->dict not NULL
                            and 1 <= dict_len <= sw (the staged dictionary is then the whole
                            dictionary, and the DICTID covers exactly the bytes the parse may
                            reference); anything else is -E_INVAL.  The DEFLATE data is bit for bit
                            that of the same encode without the flag; dmx_max_compressed_flags adds
                            4.  dmx_encode_fd*, deflate_compress and dmx_encode_batch_async return
                            -E_INVAL for it. */
#define DMX_F_EXACT_SORT 16u  /* test hook: sort positions with the match-any grouping instead
                                of lane-ordered LDS atomics (same result; used by the tests) */
#define DMX_F_LAZY 8u    /* parse option: lazy evaluation, one position of
                            lookahead -- a match at i becomes a literal when the match at
                            i+1 is strictly longer.  Off = the reference's greedy parse. */
#define DMX_F_SPLIT 32u  /* block option: an sw block may be emitted as up to
                            four DEFLATE blocks cut at the token boundaries of its quarters,
                            each with its own codes, when that is smaller */

#define DMX_F_DICT 64u   /* parse option: cross-block dictionary -- every block
                            also searches the previous sw block (the K newest entries of its
                            hash chain, distance <= 32768); a history match is taken only when
                            strictly longer than the block's own.  Block 0
                            uses dmx_opts.dict when given.  Blocks then depend on their
                            predecessor: inflate with the stream mode, not the block index. */
#define DMX_F_STORE_CHECK 128u  /* block option: a block whose bytes pass an
                                 * integer noise check (flat byte histogram, few 4-byte
                                 * repeats) is emitted stored without a parse -- the stored
                                 * path runs at HBM speed instead of the match kernel's.  An
                                 * encoder policy of our own (the reference always parses);
                                 * the oracle applies the same rule.  Such blocks have no
                                 * tokens (no compress_stats records). */
#define DMX_F_DEEP 256u  /* parse option: adaptive chain depth for bounded
                            K < 64 -- a block whose trigrams are few (D distinct 13-bit
                            buckets among its positions p mod 2048 < 256, 4 D < samples:
                            small alphabets such as binary digits, hex, DNA) searches its
                            own chains 32 deep instead of K (dmx_opts.deep_chain sets
                            another depth; 32 is the cheapest depth that keeps every
                            reference-held text file within 2 % of the reference parse).  Text never qualifies. */
#define DMX_DEEP_CHAIN 32

typedef struct {
    int32_t sw;        /* block size 1..32768 (0 = 32768) */
    int32_t max_chain; /* 0 = exhaustive (reference semantics); K > 0 = the K newest chain entries */
    uint32_t flags;    /* DMX_F_* */
    int32_t deep_chain; /* DMX_F_DEEP: the chain depth of a small-alphabet block, 0..255
                           (0 = DMX_DEEP_CHAIN); values outside 0..255 return -E_RANGE, and a
                           depth <= max_chain has no effect (the block keeps K).  (This
                           field was `reserved`, always 0, before round 5.) */
    const void* dict;  /* DMX_F_DICT: the bytes just before the input (device memory for
                          dmx_encode_async, host memory for dmx_encode_host), history of
                          block 0; the last min(dict_len, sw) bytes are used.  NULL: none */
    uint64_t dict_len;
} dmx_opts;

/* Result of one encode, filled on the device, fetched by dmx_encode_result(). */
typedef struct {
    uint64_t out_len;   /* bytes written to d_out */
    uint64_t end_bits;  /* bit position after the last block (before flush/trailer) */
    uint64_t n;         /* input bytes */
    uint64_t ntokens;   /* tokens over all blocks */
    uint32_t adler;     /* the stream's check value: Adler-32 of this input (RFC 1950 §8.2), or
                           with DMX_F_GZIP its CRC-32 (RFC 1952 §8) */
    int32_t status;     /* 0 or -E_* */
    uint32_t nblocks;
    uint32_t nstored, nfixed, ndynamic;
    uint32_t nsortfallback; /* blocks of this encode whose lane-ordered radix sort failed its
                               order check and were re-sorted with the match-any grouping
                               (DESIGN.md §3); the DMX_F_EXACT_SORT test hook forces one per
                               searched block */
    uint32_t nsortfallback_total; /* the same, summed over every encode of the context */
} dmx_result;

typedef struct dmx_ctx dmx_ctx;

/* Allocate a device context (own HIP stream + workspace) for inputs up to max_input. */
int dmx_ctx_create(int device, uint64_t max_input, dmx_ctx** out);
void dmx_ctx_destroy(dmx_ctx* ctx);
/* Grow the workspace (synchronising) so that n bytes with block size sw fit. */
int dmx_ctx_reserve(dmx_ctx* ctx, uint64_t n, int32_t sw);
/* The same, plus the scratch the block options need from then on: DMX_F_SPLIT (split plans)
 * and DMX_F_DICT (every block's exported chains).  dmx_encode_async never allocates: with
 * those flags on a context not reserved for them it returns -E_SZ.  Synchronises only when
 * it allocates. */
int dmx_ctx_reserve_flags(dmx_ctx* ctx, uint64_t n, int32_t sw, uint32_t flags);
/* Worst-case output bytes for n input bytes with block size sw. */
uint64_t dmx_max_compressed(uint64_t n, int32_t sw);
/* The same for the container `flags` select: 12 bytes more under DMX_F_GZIP; under DMX_F_BGZF
 * 26 bytes more per block (18 + 8 of each member) and 28 for the end-of-file member. */
uint64_t dmx_max_compressed_flags(uint64_t n, int32_t sw, uint32_t flags);

/* Enqueue the whole encode of device buffer d_in[0..n) into d_out (capacity
 * out_cap) on `stream` (hipStream_t; NULL = the context's stream).  No host
 * synchronisation, no allocation (graph-capturable).  Returns 0 or -E_* for argument
 * errors: -E_SZ when n needs more blocks than the context holds, or DMX_F_SPLIT /
 * DMX_F_DICT on a context not reserved for them (dmx_ctx_reserve_flags).  With
 * DMX_F_STORE_CHECK, bytes of d_out past the final out_len (inside out_cap) may be
 * overwritten: a noise block is copied speculatively to the offset it would have if every
 * block before it were stored. */
int dmx_encode_async(dmx_ctx* ctx, const void* d_in, uint64_t n, void* d_out, uint64_t out_cap,
                     const dmx_opts* opts, void* stream);
/* Wait for the last encode on `stream` and copy its dmx_result to the host. */
int dmx_encode_result(dmx_ctx* ctx, dmx_result* r, void* stream);
/* Enqueue the copy of the last encode's dmx_result into r (pinned host memory for a truly
 * asynchronous copy) on `stream`, without waiting: the caller waits on the stream or on an
 * event recorded after this call.  Lets a pipeline (bench.py, N > 1) learn chunk i's length
 * while encode i + 1 runs. */
int dmx_encode_result_async(dmx_ctx* ctx, dmx_result* r, void* stream);

/* Host-buffer convenience (H2D, encode, D2H) on a cached per-device context.
 * *out_len receives the stream length; out must hold dmx_max_compressed_flags(n, sw, flags). */
int dmx_encode_host(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t out_cap,
                    uint64_t* out_len, const dmx_opts* opts);

/* Streaming file-in/file-out encode (deflate_compress without fd_stats): reads fd_in in
 * chunks of `chunk` bytes (rounded down to a multiple of sw; 0 = sw) into pinned memory,
 * encodes chunk i on the device while reading chunk i+1, writes one zlib stream to fd_out
 * (chunks joined by sync flushes, Adler-32 combined on the host; DMX_F_DICT carries the
 * history across chunks).  opts->flags: the parse/block options (DMX_F_LAZY, _SPLIT, _DICT)
 * and DMX_F_GZIP (one gzip member: chunk 0 carries the gzip header, the chunks' CRC-32s are
 * combined on the host, which writes CRC-32 and the byte count mod 2^32 at the end) or
 * DMX_F_BGZF (the chunks' members concatenated as they are -- the chunk size is a multiple of
 * sw, so the block cuts do not depend on it -- and the end-of-file member once, behind the last
 * chunk; nothing is combined on the host); the rest of the framing is its own.  Returns 0 or -E_*. */
int dmx_encode_fd(int fd_in, int fd_out, const dmx_opts* opts, uint64_t chunk);

/* Where the last single-device dmx_encode_fd call (or deflate_compress without fd_stats)
 * spent its time, per stage of its pipeline: wall time of the call; the
 * reader thread's time in read()/pread(); the H2D copies, encodes and D2H copies on the
 * device (HIP event times, summed over chunks); the writer thread's time in write().  The
 * stages overlap, so the largest of them bounds the call.  Returns 0, or -E_INVAL when no
 * such call has finished in this process. */
typedef struct {
    uint64_t chunks, bytes_in, bytes_out;
    double wall_ms, read_ms, h2d_ms, encode_ms, d2h_ms, write_ms;
} dmx_fd_stats;
int dmx_fd_last_stats(dmx_fd_stats* out);

/* The same stream as dmx_encode_fd with the chunks spread over several GPUs: chunk i is
 * read (pread), encoded and copied back by the host thread of devices[i % ndev], and the
 * chunks are written to fd_out in order (one host thread per GPU).  Needs a
 * regular file as fd_in (a pipe falls back to dmx_encode_fd on devices[0]).  A device may
 * be listed more than once (one context per entry).  deflate_compress uses it when
 * DMX_DEVICES lists more than one device ("0,1,2,3" or "all").  Returns 0 or -E_*. */
int dmx_encode_fd_multi(int fd_in, int fd_out, const dmx_opts* opts, uint64_t chunk, const int* devices, int ndev);

/* Test hook (fault injection): "malloc:N" makes the N-th device or pinned
 * allocation of the library from now fail, "launch:N" the N-th encode's launch check;
 * NULL or "" turns it off.  Also read from DMX_FAULT when the library loads.  The failing
 * call returns -E_DEVICE (or -E_MALLOC for pinned memory) and leaves no allocation behind
 * that its context does not own.  Returns 0, or -E_INVAL / -E_RANGE for a bad spec. */
int dmx_fault_set(const char* spec);

/* Test hooks of one context: launch shapes that every encode must turn into the same stream
 * (DESIGN.md §3.3).  Their defaults come from the environment, read once when the context is
 * created (DMX_WORKLIST = 0 | list | plain, DMX_DEDUPE = 0 | 1, DMX_SCAN3 = 1); an encode
 * never reads the environment.  Values: DMX_HOOK_WORKLIST -1 adaptive (default), 0 no work
 * lists, 1 the list shapes, 2 a workgroup per block; DMX_HOOK_DEDUPE -1 adaptive, 0 off,
 * 1 on; DMX_HOOK_SCAN3 0 / 1 (K3 in three launches at any size); DMX_HOOK_BDICT_SIMPLE 0 / 1
 * (dmx_encode_batch_dict_async's history search with a workgroup per table entry; no
 * environment variable).  Set them between encodes
 * on the context's own thread.  Returns 0, -E_INVAL (unknown hook) or -E_RANGE. */
#define DMX_HOOK_WORKLIST 1
#define DMX_HOOK_DEDUPE 2
#define DMX_HOOK_SCAN3 3
#define DMX_HOOK_BDICT_SIMPLE 4
int dmx_ctx_set_hook(dmx_ctx* ctx, int hook, int value);

/* ---- GPU inflate, csrc/dmx_inflate_dev.hip ---- */
/* One entry per independently decodable DEFLATE block: start bit in the stream, output
 * offset and length.  Blocks of a dmx stream never reference earlier blocks. */
typedef struct {
    uint64_t bit;
    uint64_t out_off;
    uint32_t out_len;
    uint32_t reserved;
} dmx_iblock;
typedef struct {
    int32_t status;     /* 0 or -E_* (first error) */
    uint32_t reserved;
    uint64_t out_len;   /* bytes produced */
} dmx_inflate_status;
/* Device block index of the last encode of ctx (nblk entries into d_index, on stream). */
int dmx_block_index(dmx_ctx* ctx, dmx_iblock* d_index, uint32_t cap, void* stream);
/* Inflate on the GPU.  d_index != NULL: decode the nblk listed blocks in parallel (one
 * wave each) into d_out + out_off.  d_index == NULL: decode the whole zlib stream d_z
 * (header, blocks until BFINAL, Adler-32 check) in one workgroup.  Status in the device
 * record d_status.  The first-level tables live in device scratch taken from a per-device
 * stream-ordered pool on every call (hipMallocFromPoolAsync before the launch, hipFreeAsync
 * after it on the same stream).  Returns 0 or -E_*: -E_MALLOC when that scratch cannot be
 * allocated, -E_DEVICE for launch errors.
 * d_status->status of the stream mode is deflate_decompress's status for the same bytes (the
 * table above), and -E_SZ when out_cap is too small.  The indexed mode has no header or
 * trailer: it reports the same status for an error that precedes a block's output (tables,
 * block headers, a first symbol), the status of whichever limit comes first otherwise, -E_SZ
 * for a block that ends short of or beyond its out_len and -E_RANGE for an entry outside the
 * stream or the output (out_len above 32768 included). */
int dmx_inflate_async(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, uint32_t nblk, void* d_out,
                      uint64_t out_cap, dmx_inflate_status* d_status, void* stream);

/* Chained GPU inflate: the blocks listed in d_index decoded in parallel although a block's
 * matches may reach into the blocks before it (DMX_F_DICT streams; any stream cut at block
 * starts).  Each block decodes into 16-bit cells -- a byte, or a reference to a position
 * before the block -- and pointer jumping over the references, about log2(nblk) + 2 short
 * launches, resolves them; then the cells become bytes in d_out.  d_work: device scratch of
 * dmx_inflate_chained_work(out_cap, nblk) bytes (about 10 per output byte), 256-byte aligned.  Status in d_status (out_len =
 * bytes decoded; a reference before the output start is -E_HUFDIS).  out_cap is a capacity:
 * only the ranges the index lists are written.  Returns 0 or -E_*. */
uint64_t dmx_inflate_chained_work(uint64_t out_cap, uint32_t nblk);
int dmx_inflate_chained_async(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, uint32_t nblk, void* d_out,
                              uint64_t out_cap, void* d_work, uint64_t work_bytes, dmx_inflate_status* d_status,
                              void* stream);
/* Diagnostic: the total length of the reference lists of the last chained decode that used
 * d_work -- host[0] after the prep kernel, host[r + 1] after jump launch r (n <= 41 entries;
 * synchronizes the stream).  Returns 0 or -E_*. */
int dmx_inflate_chained_lists(const void* d_work, uint32_t* host, uint32_t n, void* stream);

/* The block index of a BGZF file in host memory (DMX_F_BGZF output, or any BGZF file whose
 * members hold at most 32768 bytes of input each, the bound of dmx_inflate_async's indexed mode
 * -- for htslib's default 65280-byte blocks, and any member the format allows, use
 * dmx_bgzf_index_max and dmx_inflate_members_async): walks the members by the BSIZE of their "BC"
 * FEXTRA subfield (other subfields may precede or follow it) and emits one entry per member with
 * ISIZE > 0 -- bit = first bit of its DEFLATE data, out_off = the sum of the ISIZEs before it,
 * out_len = ISIZE -- and the member's stored CRC-32 into crc[] (may be NULL); empty members, the
 * end-of-file one included, give no entry.  *nblk receives the number of entries (also when cap
 * is too small), *out_len the total of the ISIZEs.  The entries are input for dmx_inflate_async
 * once copied to the device (a member may hold several DEFLATE blocks: the decoder runs to
 * BFINAL).  Returns 0, -E_ZHEAD (a member is not gzip / deflate or has no BC subfield), -E_LEN
 * (truncated), -E_SZ (cap too small), -E_RANGE (a member with ISIZE > 32768).  Host only (a file
 * in device memory: dmx_bgzf_index_async). */
int dmx_bgzf_index(const uint8_t* z, uint64_t zlen, dmx_iblock* idx, uint32_t* crc, uint32_t cap, uint32_t* nblk,
                   uint64_t* out_len);
/* The same walk with the caller's bound on a member's ISIZE: max_isize is 1..DMX_BGZF_MAX_ISIZE
 * (else -E_RANGE), and a member with ISIZE > max_isize is -E_RANGE.  BSIZE is 16 bits, so the
 * format itself allows no member of more than 65536 bytes, compressed or not: with
 * DMX_BGZF_MAX_ISIZE every sound BGZF file indexes, and the entries are input for
 * dmx_inflate_members_async.  dmx_bgzf_index is this call with 32768.  Host only; it is the
 * specification of dmx_bgzf_index_async, which does the same on a file in device memory. */
#define DMX_BGZF_MAX_ISIZE 65536
int dmx_bgzf_index_max(const uint8_t* z, uint64_t zlen, uint32_t max_isize, dmx_iblock* idx, uint32_t* crc,
                       uint32_t cap, uint32_t* nblk, uint64_t* out_len);
/* Inflate the nblk members (or any independently decodable entries) listed in d_index in
 * parallel, one wave each, into d_out + out_off: dmx_inflate_async's indexed mode with out_len up
 * to DMX_BGZF_MAX_ISIZE, same statuses, -E_RANGE for an entry outside the stream or the output or
 * with out_len > 65536.  d_crc_want != NULL (nblk words, 4-byte aligned: the members' stored
 * CRC-32s as dmx_bgzf_index_max gives them): the CRC-32 of every decoded range is then computed on
 * the same stream (dmx_crc32_ranges_async's kernel) and compared on the device; a member that
 * differs sets d_status->status = -E_CRC unless a status is already there (a decode error stays,
 * and after one the CRC pass does nothing).  Takes no context; the table scratch comes from the
 * pool dmx_inflate_async uses.  No host synchronisation (graph-capturable where the runtime
 * captures the pool's allocation).  Returns 0 or -E_* as dmx_inflate_async. */
int dmx_inflate_members_async(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, uint32_t nblk,
                              void* d_out, uint64_t out_cap, const uint32_t* d_crc_want,
                              dmx_inflate_status* d_status, void* stream);
/* The same index for a BGZF file that lies in device memory, built on the device
 * (csrc/dmx_bgzf_index.hip): every position of the file that parses as a member is
 * a candidate, and pointer doubling over the candidates' BSIZE links finds the chain that starts
 * at offset 0 -- the members of the host walk.  For the same bytes and max_isize the record and
 * the output equal dmx_bgzf_index_max's: status (0, -E_ZHEAD, -E_LEN, -E_RANGE, -E_SZ when cap is
 * too small, then with the first cap entries written and the full nblk and out_len), the entries
 * (bit, out_off, out_len, reserved = 0) into d_index (8-byte aligned; NULL only with cap 0) and
 * the members' stored CRC-32s into d_crc (4-byte aligned, or NULL), also on truncated and corrupt
 * files and on files whose data holds bytes that look like members.  The one difference: d_work
 * (256-byte aligned, work_bytes >= dmx_bgzf_index_work(zbytes, 1)) holds a candidate per parsing
 * position, and a file with more of them than work_bytes has room for gives status -E_SZ with
 * nblk = 0, out_len = 0 and ncand = the number needed: call again with
 * dmx_bgzf_index_work(zbytes, ncand) bytes.  A sound file has at most zbytes / 26 + 1 members,
 * and about as many candidates.  d_z may have any alignment; whole 16-byte aligned groups are
 * loaded as in dmx_crc32_async: up to 15 bytes before d_z and after d_z + zbytes, inside the
 * groups that hold the first and the last byte, are read and never looked at.  Takes no context
 * (the current device).  The number of launches (5 + ceil(log2(bound + 1)), bound = the smaller of
 * the candidates d_work holds and zbytes / 26 + 1) follows from the arguments alone: no
 * allocation, no host synchronisation, a linear chain under graph capture; the record is reset by
 * a kernel.  Returns before any device call: -E_INVAL (d_z NULL with zbytes > 0, d_status or d_work
 * NULL, d_index NULL with cap > 0, d_index or d_status not 8-byte, d_crc not 4-byte, d_work not
 * 256-byte aligned, work_bytes too small), -E_RANGE (max_isize outside 1..DMX_BGZF_MAX_ISIZE,
 * zbytes > 0xFFFFFFF0: the decoder's own bound); else 0 or -E_DEVICE. */
typedef struct {
    int32_t status;    /* 0 or -E_*: dmx_bgzf_index_max's status for the same bytes */
    uint32_t nblk;     /* members with ISIZE > 0 (also when cap is too small); 0 after any other error */
    uint64_t out_len;  /* sum of the ISIZEs; 0 after an error other than -E_SZ for cap */
    uint32_t ncand;    /* positions that parsed as a member (the capacity the work buffer needed) */
    uint32_t reserved;
} dmx_bgzf_index_status;
/* Bytes of d_work for a file of zbytes with room for max_cand candidates (a multiple of 256). */
uint64_t dmx_bgzf_index_work(uint64_t zbytes, uint32_t max_cand);
/* The scan's geometry (tests): bytes of aligned 16-byte groups per scan tile (a workgroup). */
void dmx_bgzf_index_geometry(uint32_t* tile);
int dmx_bgzf_index_async(const void* d_z, uint64_t zbytes, uint32_t max_isize, dmx_iblock* d_index, uint32_t* d_crc,
                         uint32_t cap, void* d_work, uint64_t work_bytes, dmx_bgzf_index_status* d_status, void* stream);
/* Any BGZF file in device memory into d_out, device to device: dmx_bgzf_index_async with
 * DMX_BGZF_MAX_ISIZE into scratch from the pool dmx_inflate_async uses (room for zbytes / 256 + 1024
 * candidates; once more with the number needed where the file has more), one 24-byte copy of its
 * record to the host -- the call's one synchronisation before the decode: the member count sizes
 * the decode's grid and table scratch -- then dmx_inflate_members_async (verify != 0: with the
 * members' CRC-32s, -E_CRC) and its status.  *out_len receives the decoded length whenever the
 * file indexes, also when out_cap is too small (-E_SZ, nothing decoded, d_out untouched).  An
 * empty file, or one of empty members only, gives 0 bytes and 0.  Returns 0, -E_INVAL / -E_RANGE
 * for the arguments (before any device call), the index's status, or the decode's. */
int dmx_bgzf_decode_device(const void* d_z, uint64_t zbytes, void* d_out, uint64_t out_cap, uint64_t* out_len,
                           int verify, void* stream);
/* Batched range reads from a BGZF file in device memory (csrc/dmx_bgzf_ranges.hip, DESIGN.md §3.5
 * "Reading ranges"): many (offset, length) requests against the decoded bytes of the file become
 * the set of members they touch, a decode of just those members into scratch, and the requested
 * bytes packed back to back into d_out -- all on the device, with no host round trip.
 * d_index / d_crc / nblk are what dmx_bgzf_index_async wrote for d_z: entries in file order, the
 * first at out_off 0, out_off[m + 1] == out_off[m] + out_len[m], out_len in 1..65536, bit rising; a
 * thread per entry checks this, a violation is status -E_INVAL and nothing is decoded.  d_crc == NULL:
 * no verification.  A range is clipped as pread clips: with total = the decoded length of the file,
 * range q yields min(len, total - off) bytes, or 0 when off >= total; len is any 64-bit value (the
 * sums saturate, and a saturated sum is above every capacity).  Ranges may overlap, repeat and come
 * in any order.  The bytes of range q land at d_out + d_out_off[q]; d_out_off (nranges + 1 words,
 * 8-byte aligned) is the exclusive scan of the clipped lengths, d_out_off[nranges] == out_len, and is
 * written whenever the status is 0 or -E_SZ.
 * flags & DMX_RANGES_VIRTUAL: off is a BGZF virtual offset, member file offset << 16 | offset in
 * the member's data.  off >> 16 must be the file offset of a member that has an index entry: the
 * member's header is parsed there (bounds-checked, as dmx_bgzf_index_max parses it) and the entry
 * whose bit is the first bit of its DEFLATE data -- 8 x (offset + 12 + XLEN) for a member without
 * FNAME / FCOMMENT / FHCRC -- is found by binary search; off & 0xFFFF must be below that member's
 * out_len unless len == 0.  Any other value makes the call -E_RANGE with bad = the lowest such range
 * index (an integer minimum: deterministic).  The range then reads on across the following members
 * like any other.
 * A member is decoded once, however many ranges touch it, and only if a non-empty clipped range
 * touches it; untouched members are never read, so a corrupt member or a wrong CRC in one is not an
 * error of the call.  nmembers > max_members, scratch_len > scratch_bytes or out_len > out_cap is
 * status -E_SZ: the record then holds all three needed numbers, nothing is decoded and d_out is
 * untouched.  Status precedence: -E_INVAL (index check), -E_RANGE, -E_SZ, then the decode's first
 * error (the statuses of dmx_inflate_members_async), then -E_CRC; after any of them d_out is
 * untouched.
 * No allocation, no host synchronisation; the number of launches and every grid follow from the
 * host arguments alone (nblk, nranges, max_members, out_cap) and the device's size, a linear chain
 * that can be captured into a graph; records and counters are reset by kernels.  Everything the
 * call needs lives in d_work (256-byte aligned, work_bytes >= dmx_bgzf_ranges_work(nblk, nranges,
 * max_members, scratch_bytes)): the members' need counts, the scans, the compact sub-index and its
 * CRC words, the decode's first-level tables and scratch_bytes of decoded members.  With all three
 * capacities 0 (d_out may be NULL) the call only plans: the record tells what the real call needs.
 * Returns before any device call: -E_INVAL (d_status, d_work or d_out_off NULL, d_z NULL with
 * zbytes > 0, d_index NULL with nblk > 0, d_ranges NULL with nranges > 0, d_out NULL with
 * out_cap > 0; d_index, d_ranges, d_out_off or d_status not 8-byte, d_crc not 4-byte, d_work not
 * 256-byte aligned; work_bytes too small), -E_RANGE (zbytes > 0xFFFFFFF0, nranges > 0x7FFFFFFF,
 * unknown flags); else 0 or -E_DEVICE.  nranges == 0 or nblk == 0 is status 0, out_len 0 and
 * d_out_off[..] = 0. */
typedef struct { uint64_t off; uint64_t len; } dmx_brange;      /* 16 bytes */
#define DMX_RANGES_VIRTUAL 1u   /* off is a BGZF virtual offset: member file offset << 16 | offset in the member's data */
typedef struct {
    int32_t  status;       /* 0 or -E_* (precedence above) */
    uint32_t nmembers;     /* distinct members the ranges touch (the capacity needed) */
    uint64_t out_len;      /* sum of the clipped lengths (bytes of d_out needed) */
    uint64_t scratch_len;  /* sum of the ISIZEs of the touched members (scratch needed) */
    uint32_t bad;          /* lowest index of a range that is -E_RANGE, else 0xFFFFFFFF */
    uint32_t reserved;
} dmx_bgzf_ranges_status;                                       /* 32 bytes */
/* Bytes of d_work for an index of nblk entries, nranges ranges, max_members members to decode and
 * scratch_bytes of decoded members (a multiple of 256, monotone in every argument). */
uint64_t dmx_bgzf_ranges_work(uint32_t nblk, uint32_t nranges, uint32_t max_members, uint64_t scratch_bytes);
/* The scans' geometry (tests): members and ranges per scan tile (a workgroup). */
void dmx_bgzf_ranges_geometry(uint32_t* member_tile, uint32_t* range_tile);
int dmx_bgzf_read_ranges_async(const void* d_z, uint64_t zbytes,
                               const dmx_iblock* d_index, const uint32_t* d_crc, uint32_t nblk,
                               const dmx_brange* d_ranges, uint32_t nranges, uint32_t flags,
                               void* d_out, uint64_t out_cap, uint64_t* d_out_off,
                               uint32_t max_members, uint64_t scratch_bytes,
                               void* d_work, uint64_t work_bytes,
                               dmx_bgzf_ranges_status* d_status, void* stream);
/* The convenience over it, with its work buffer from the pool dmx_inflate_async uses: the call above
 * with all three capacities 0 (plan only), one 32-byte copy of its record to the host -- the call's
 * one synchronisation before the decode -- then the real call sized by the record, its record and
 * its status.  *out_len receives the packed length whenever planning succeeded, also when out_cap is
 * too small (-E_SZ, d_out untouched: the two-call idiom of dmx_bgzf_decode_device); d_out_off is then
 * written too.  verify != 0 checks the touched members' CRC-32s (d_crc must then be given).  Returns
 * 0, -E_INVAL / -E_RANGE for the arguments (before any device call), -E_MALLOC, or the record's
 * status. */
int dmx_bgzf_read_device(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, const uint32_t* d_crc,
                         uint32_t nblk, const dmx_brange* d_ranges, uint32_t nranges, uint32_t flags,
                         void* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* out_len,
                         int verify, void* stream);
/* Batches of independent streams (csrc/dmx_inflate_dev.hip, DESIGN.md §3.1 "Batches"): nstreams zlib
 * streams, gzip members or raw DEFLATE streams (RFC 1950 / 1952 / 1951) of any size and unknown
 * decoded length, decoded side by side, one wave each, every one with a result of its own.
 * Stream k is d_z[in_off, in_off + in_len) and decodes into d_out[out_off, out_off + out_cap).  Both
 * offsets may have any alignment.  A stream whose input lies outside d_z[0, zbytes), whose window lies
 * outside d_out[0, out_bytes), or whose in_len is above 0xFFFFFFF0 (the reader's 32-bit positions)
 * gets -E_RANGE, and nothing of it is read or written.  Windows that overlap are the caller's error.
 * The reader loads whole aligned 4-byte words: up to 3 bytes before a stream's first byte, inside the
 * word that holds it, are read and never looked at (d_z must be readable there, which a stream
 * inside an allocation always is); the word that holds its last byte is assembled from the stream's
 * own bytes, and the reader hands out zeros past them.  So a stream that ends early is -E_LEN (or its
 * trailer's status), never a decode of the bytes behind it; bytes behind a stream's trailer are
 * ignored, as deflate_decompress ignores them.  The CRC pass loads whole 16-byte aligned groups as
 * dmx_crc32_async does: up to 15 bytes before and after a decoded range, inside the groups that hold
 * its first and last byte, are read and never looked at -- d_out must be readable there, which a
 * window inside an allocation always is.
 * flags: the framing in bits 0..3 -- DMX_BATCH_AUTO (a stream that begins 1F 8B is gzip, any other
 * zlib: deflate_decompress's rule), DMX_BATCH_ZLIB, DMX_BATCH_GZIP, DMX_BATCH_RAW -- and
 * DMX_BATCH_MEASURE.
 * d_results[k]: status 0 or -E_* for that stream alone (a failing stream never changes a neighbour's
 * result or bytes); format the framing that was decoded (1, 2 or 3; 0 where -E_RANGE came first
 * under AUTO); out_len the bytes produced; in_used the input bytes from in_off through the end of the
 * trailer (zlib: through the Adler-32; gzip: through ISIZE; raw: through the byte that holds the last
 * bit of the final block), which is what a caller needs to walk concatenated members; check the stored
 * Adler-32 or CRC-32 (0 for raw).  After an error out_len, in_used and check are 0, and the bytes
 * inside that stream's own window are unspecified.  No byte outside the windows is ever written.
 * Statuses: for zlib and gzip what deflate_decompress returns for the same bytes (the table above),
 * gzip_header's -E_ZHEAD / -E_ZCMPMT / -E_RESERV, -E_CRC for a wrong or cut gzip trailer and -E_LEN for
 * a wrong ISIZE included (the CRC is checked first, as on the host); an explicit DMX_BATCH_GZIP on
 * bytes that do not begin 1F 8B is -E_ZHEAD.  A raw stream has the status of the same data behind a
 * zlib header, minus the trailer's; an empty raw input is -E_LEN.  out_len > out_cap is -E_SZ.
 * DMX_BATCH_MEASURE: the same decode with every store to d_out left out -- lengths and statuses only.
 * d_out may be NULL and out_bytes is not looked at; out_cap is only a limit (UINT64_MAX: none) and
 * out_off is ignored.  Results as above with one difference: a gzip CRC-32 cannot be checked without
 * the bytes, so a member with a wrong CRC-32 passes (its check field holds the stored value).
 * Adler-32 and ISIZE are still checked.
 * d_status: nfailed the number of streams with a status (an integer sum), first_bad the lowest such
 * index (an integer minimum; 0xFFFFFFFF when none), total_out the sum of out_len over the streams
 * with status 0 -- nothing depends on the order in which workgroups run.  The record and the claim
 * counter are reset by a kernel of the call.
 * Two or three launches (reset, decode; the CRC-32 pass over the gzip members under DMX_BATCH_AUTO
 * and DMX_BATCH_GZIP unless measuring; the reset alone when nstreams == 0, status 0): no allocation, no host synchronisation, the number of
 * launches and every grid follow from nstreams, flags and the device's size, a linear chain that can
 * be captured into a graph.  The decode's grid is the smaller of nstreams, what the device holds at
 * once (four 34 KB workgroups per CU) and a fixed bound; workgroups claim streams from a counter in
 * index order.  Everything the call needs lives in d_work (256-byte aligned, work_bytes >=
 * dmx_inflate_batch_work(nstreams): a multiple of 256, monotone, bounded -- the counter and the
 * workgroups' first-level tables).
 * Returns before any device call: -E_INVAL (d_results, d_status or d_work NULL, d_streams NULL with
 * nstreams > 0, d_z NULL with zbytes > 0, d_out NULL without DMX_BATCH_MEASURE; d_streams, d_results
 * or d_status not 8-byte aligned; d_work not 256-byte aligned or work_bytes too small), -E_RANGE
 * (unknown flag bits, a format above 3); else 0 or -E_DEVICE. */
typedef struct { uint64_t in_off, in_len, out_off, out_cap; } dmx_bstream;      /* 32 bytes */
typedef struct { int32_t status; uint32_t format; uint64_t out_len; uint64_t in_used;
                 uint32_t check; uint32_t reserved; } dmx_bresult;               /* 32 bytes */
typedef struct { uint32_t nfailed; uint32_t first_bad; uint64_t total_out; } dmx_batch_status; /* 16 bytes */
#define DMX_BATCH_AUTO 0u      /* 1F 8B: gzip, else zlib -- deflate_decompress's rule */
#define DMX_BATCH_ZLIB 1u
#define DMX_BATCH_GZIP 2u
#define DMX_BATCH_RAW  3u      /* RFC 1951 data only, no header, no trailer */
#define DMX_BATCH_MEASURE 16u  /* decode without writing: lengths and statuses only */
uint64_t dmx_inflate_batch_work(uint32_t nstreams);
int dmx_inflate_batch_async(const void* d_z, uint64_t zbytes, const dmx_bstream* d_streams, uint32_t nstreams,
                            uint32_t flags, void* d_out, uint64_t out_bytes, dmx_bresult* d_results,
                            void* d_work, uint64_t work_bytes, dmx_batch_status* d_status, void* stream);
/* The same batches with preset dictionaries (RFC 1950 2.2: FDICT and DICTID; zlib's
 * inflateSetDictionary, Python's zdict=; DESIGN.md §3.1 "Dictionaries").  Everything
 * dmx_inflate_batch_async promises holds: a status per stream, neighbours untouched, no byte read
 * behind a stream, no allocation, no host synchronisation, a linear chain of launches that can be
 * captured into a graph, DMX_BATCH_MEASURE.
 * Dictionary j is d_dict[off, off + len) of d_dicts[j], of any length >= 0 at any alignment; stream k
 * uses dictionary d_dict_of[k], or none where that is DMX_BATCH_NODICT.  d_dict_of == NULL: every
 * stream uses dictionary 0 (none when ndicts == 0).  The last min(len, 32768) bytes prime the window;
 * the DICTID is the Adler-32 of all len bytes, computed on the device by a kernel of the call, so the
 * dictionaries may change between two replays of a captured call.  Only whole 16-byte aligned groups
 * inside a dictionary and single bytes at its edges are loaded: no byte outside [off, off + len).
 * Cost: every dictionary is folded by one workgroup of 256 threads, all len bytes of it (the DICTID
 * covers them all), before the decode starts: 32 KiB is a few microseconds, but a dictionary of many
 * megabytes is read by one CU and delays the whole batch -- pass only the bytes a writer passed to
 * deflateSetDictionary, which keeps 32 KiB at most.
 * zlib decides, as everywhere:
 *   a zlib stream with FDICT: a 6-byte header.  With a dictionary whose Adler-32 is the stored DICTID
 *     it decodes with the window primed; the Adler-32 trailer covers the output alone; in_used counts
 *     the 6 bytes.  Without a dictionary, or with another DICTID: -E_ZPDICT.  A header that ends
 *     inside the DICTID (2 to 5 bytes) is -E_ZHEAD, whether or not there is a dictionary.
 *   a zlib stream without FDICT ignores its dictionary (zlib.decompressobj(zdict=d) on such a
 *     stream): a distance before the first output byte stays -E_HUFDIS.
 *   a raw stream with a dictionary: the window is always primed (inflateSetDictionary on a raw stream).
 *   a gzip member has no dictionary and decodes as without one.
 *   a distance greater than (output so far + primed bytes): -E_HUFDIS.
 *   d_dict_of[k] >= ndicts and not DMX_BATCH_NODICT, or a d_dicts entry outside d_dict[0, dict_bytes):
 *     that stream alone gets -E_RANGE (format 0 under AUTO), whatever its framing.
 * Launches: reset, the dictionaries' Adler-32s (ndicts blocks of 256 threads; only when ndicts > 0),
 * decode, and the CRC-32 pass as above.  d_work: 256-byte aligned, work_bytes >=
 * dmx_inflate_batch_dict_work(nstreams, ndicts) -- a multiple of 256, monotone in both, equal to
 * dmx_inflate_batch_work(nstreams) at ndicts == 0.
 * Returns before any device call: what dmx_inflate_batch_async returns, and -E_INVAL for d_dicts NULL
 * with ndicts > 0, d_dict NULL with dict_bytes > 0, d_dicts not 8-byte or d_dict_of not 4-byte aligned.
 * dmx_inflate_batch_async itself is unchanged: its launches, its kernels, its statuses (an FDICT
 * stream there is -E_ZPDICT). */
typedef struct { uint64_t off, len; } dmx_bdict;   /* 16 bytes: dictionary j = d_dict[off, off + len) */
#define DMX_BATCH_NODICT 0xFFFFFFFFu
uint64_t dmx_inflate_batch_dict_work(uint32_t nstreams, uint32_t ndicts);
int dmx_inflate_batch_dict_async(const void* d_z, uint64_t zbytes, const dmx_bstream* d_streams, uint32_t nstreams,
                                 uint32_t flags,
                                 const void* d_dict, uint64_t dict_bytes, const dmx_bdict* d_dicts, uint32_t ndicts,
                                 const uint32_t* d_dict_of,      /* per stream: index or DMX_BATCH_NODICT; NULL = all use 0 */
                                 void* d_out, uint64_t out_bytes, dmx_bresult* d_results,
                                 void* d_work, uint64_t work_bytes, dmx_batch_status* d_status, void* stream);
/* One stream of such a batch on the host (csrc/dmx_inflate.c), the host side of "host == GPU" for the
 * statuses above: z[0, n) under fmt (DMX_BATCH_AUTO / ZLIB / GZIP / RAW) with the dictionary
 * dict[0, dict_len) (dict == NULL: none; a non-NULL dict with dict_len 0 is an empty dictionary,
 * DICTID 1).  *out is malloc'd (the caller frees it), *out_len the decoded bytes, *in_used (may be
 * NULL) as in dmx_bresult.  Returns 0, -E_INVAL (out or out_len NULL, z NULL with n > 0, dict NULL
 * with dict_len > 0, fmt above 3), -E_MALLOC, or the stream's status. */
int dmx_inflate_dict_host(const void* z, uint64_t n, uint32_t fmt, const void* dict, uint64_t dict_len,
                          void** out, uint64_t* out_len, uint64_t* in_used);
/* One foreign stream, cut for many decoders: the plan (csrc/dmx_inflate_par_host.cpp, csrc/dmx_pfind.h;
 * DESIGN.md §3.1 "One foreign stream").  A single zlib stream, gzip member or raw DEFLATE stream
 * that carries no block index -- what gzip, pigz, zlib, a Parquet or an HTTP writer leave -- is cut
 * into chunks that start at true block boundaries and whose output lengths are known, which is what
 * a parallel decode needs; the scheme is the one pugz and rapidgzip use on CPUs, with every
 * speculative step checked.  Host only, no GPU; the text of the search, the landing rule and the
 * walk (dmx_pfind.h) compiles for the device too.
 *   the framing gives chunk 0 its start (the first block); the compressed bytes are cut every
 *   chunk_bytes (0: 16 384; 1024..2^30) and every chunk is searched for the first bit offset at
 *   which a non-final dynamic block can start: a cheap filter (BFINAL 0, BTYPE 2, HLIT and HDIST at
 *   most 29, the code length code exactly complete), then the decoder's own header rules in full;
 *   a chunk with such a candidate is decoded from it for lengths only (the window taken as primed:
 *   no distance is too far), block after block, until a block boundary is exactly a later
 *   candidate; candidates it oversteps are false and are passed -- more than 8 of them, or more
 *   than 4 MiB produced, and the walk is lost; a walk from chunk 0 along the landings keeps the
 *   chunks it reaches.  A chunk is live iff that walk reaches it, so every live chunk began at a
 *   true block boundary; the others are dead, whatever they decoded.  Stored and fixed blocks are
 *   not searched for: a stream without dynamic blocks is one live chunk.
 * chunks receives at most cap live chunks in stream order (out_off is the exclusive scan of
 * out_len; end_bit of one is bit of the next); -E_SZ where there are more (st->nlive says how many).
 * The record (56 bytes): status 0 or -E_* (the framing's, or a live chunk's first error; distances
 * before the first output byte and the trailer's check value are a decode's to find); format the
 * framing (1, 2, 3); out_len; in_used through the trailer; check the stored Adler-32 / CRC-32;
 * nchunks, ncand (chunks with a candidate, chunk 0 included), nlive, ndead = ncand - nlive;
 * gave_up = 1 with -E_RANGE where a live walk was lost; work_len the scratch a decode into 16-bit
 * cells would need.  After an error out_len, in_used, check and work_len are 0.  zbytes and the
 * output are at most 0xFFFFFFF0, else -E_RANGE.  Returns 0 with the record in *st, -E_INVAL
 * (st NULL, z NULL with zbytes > 0, chunks NULL with cap > 0, fmt above 3, chunk_bytes out of
 * range), -E_RANGE, -E_MALLOC or -E_SZ. */
typedef struct { uint64_t bit, end_bit, out_off, out_len; } dmx_pchunk;          /* 32 bytes: a live chunk */
typedef struct { int32_t status; uint32_t format; uint64_t out_len; uint64_t in_used;
                 uint32_t check; uint32_t nchunks, ncand, nlive, ndead; uint32_t gave_up;
                 uint64_t work_len; } dmx_par_status;                             /* 56 bytes */
int dmx_inflate_parallel_plan_host(const void* z, uint64_t zbytes, uint32_t fmt, uint32_t chunk_bytes,
                                   dmx_pchunk* chunks, uint32_t cap, dmx_par_status* st);
/* The same stream decoded in one pass on the device (csrc/dmx_inflate_dev.hip, csrc/dmx_pfind.h,
 * csrc/dmx_ptail.h; DESIGN.md §3.1 "One foreign stream: the decode"): the plan above built on the
 * device, then every live chunk decoded by a wave of its own.  Two calls, so that a caller sizes the
 * output between them (the two-call idiom of dmx_bgzf_read_ranges_async) or captures both with
 * capacities.  Both follow dmx_inflate_batch_async's rules: no allocation, no host synchronisation;
 * the number of launches and every grid follow from the host arguments alone (zbytes, chunk_bytes,
 * max_live, out_cap, verify) and the device's size, a linear chain that can be captured into a
 * graph; every record and counter is reset by a kernel of the call; workgroups beyond the
 * device-side counts leave at once.  d_z may have any alignment; the reader loads whole aligned
 * 4-byte words (up to 3 bytes before d_z, inside the word that holds its first byte, are read and
 * never looked at) and hands out zeros past d_z + zbytes.
 * dmx_inflate_parallel_plan_async: four launches (head, find, measure, link) leave in d_plan
 * (256-byte aligned, plan_bytes >= dmx_inflate_parallel_plan_work(zbytes, chunk_bytes)):
 *   offset 0     a dmx_par_status: for the same bytes, fmt and chunk_bytes it equals
 *                dmx_inflate_parallel_plan_host's record field for field, gave_up = 1 with -E_RANGE
 *                included; behind it in the 256-byte head the chunk_bytes used (uint32 at 56), gzip's
 *                ISIZE (uint32 at 60), the bit of the first block (uint64 at 64) and zbytes (uint64 at
 *                72), so the decode needs no repeat of chunk_bytes and fmt
 *   offset 256   the live chunks, dmx_pchunk[nlive], equal to the host plan's (after a status the
 *                failing chunk's end_bit and out_len are where its decode stopped: unspecified)
 *   then         with nc = nchunks and every part rounded up to 256 bytes: room for nc chunks
 *                (32 nc), the candidates (uint64[nc], the first bit offset of chunk c at which a
 *                non-final dynamic block can start, or ~0), the measures (32 nc: end_bit, out_len,
 *                next, flags, status of every candidate's decode for lengths) and 8 KiB of
 *                first-level tables per workgroup of the measure pass (at most 1 024)
 * The device measures every candidate in parallel where the host measures only the chunks its walk
 * reaches; a dead candidate costs time and changes nothing.  chunk_bytes: 0 is the default, else
 * 1024..2^30.  Returns before any device call: -E_INVAL (d_plan NULL or not 256-byte aligned, d_z
 * NULL with zbytes > 0, fmt above 3, chunk_bytes out of range, plan_bytes too small), -E_RANGE
 * (zbytes > 0xFFFFFFF0); else 0 or -E_DEVICE.  dmx_inflate_parallel_plan_work is 0 for arguments
 * the call refuses, else a multiple of 256, monotone in zbytes.
 * dmx_inflate_parallel_decode_async: d_plan as the plan call left it for the same d_z and zbytes.
 * Launches: begin (the plan's record into d_status, the capacity checks, the reset), cells (a wave
 * per live chunk into 16-bit cells, a match source before the chunk's first byte as a reference
 * cell), tails (one workgroup walks the chunks in order with the 32 KiB in front of the current one
 * in LDS and resolves every chunk's last 32 768 cells), pack (cells to bytes; a reference left reads a
 * cell the tail pass resolved), check (only with verify != 0: Adler-32 sums or CRC-32 remainders per
 * 64 KiB of output) and status.  *d_status (8-byte aligned):
 *   the plan's record where the plan has a status (gave_up = 1 with -E_RANGE included): nothing is
 *     decoded, d_out is untouched;
 *   -E_SZ when nlive > max_live, out_len > out_cap or work_bytes < dmx_inflate_parallel_work(out_len,
 *     nlive): the record holds the needed nlive, out_len and work_len, d_out is untouched;
 *   -E_INVAL for a d_plan that is not a plan of zbytes bytes or needs more than plan_bytes;
 *   a live chunk's decode error (that of the first such chunk in stream order) where the cell pass
 *     meets one the measure pass did not: -E_HUFDIS for a distance before the first output byte, -E_SZ
 *     for a chunk that does not end at its end_bit with its out_len;
 *   with verify != 0, the trailer: -E_ZADL32 (zlib), -E_CRC, then -E_LEN for ISIZE (gzip); a raw
 *     stream has none;
 *   else 0 with format, out_len, in_used, check and the counts as the plan gave them.
 * After a status other than -E_SZ out_len, in_used, check and work_len are 0 and the bytes of
 * d_out[0, out_cap) are unspecified; no byte at or beyond out_cap is ever written, and none at or
 * beyond out_len.  d_work: 256-byte aligned; dmx_inflate_parallel_work(out_cap, max_live) bytes always
 * suffice (a multiple of 256, monotone in both).  Returns before any device call: -E_INVAL (d_plan,
 * d_work or d_status NULL, d_z NULL with zbytes > 0, d_out NULL with out_cap > 0; d_plan or d_work
 * not 256-byte, d_status not 8-byte aligned; plan_bytes below dmx_inflate_parallel_plan_work(1, 0) or work_bytes below 256), -E_RANGE
 * (zbytes > 0xFFFFFFF0); else 0 or -E_DEVICE. */
uint64_t dmx_inflate_parallel_plan_work(uint64_t zbytes, uint32_t chunk_bytes);
int dmx_inflate_parallel_plan_async(const void* d_z, uint64_t zbytes, uint32_t fmt, uint32_t chunk_bytes,
                                    void* d_plan, uint64_t plan_bytes, void* stream);
uint64_t dmx_inflate_parallel_work(uint64_t out_cap, uint32_t max_live);
int dmx_inflate_parallel_decode_async(const void* d_z, uint64_t zbytes, const void* d_plan, uint64_t plan_bytes,
                                      uint32_t max_live, void* d_out, uint64_t out_cap,
                                      void* d_work, uint64_t work_bytes, int verify,
                                      dmx_par_status* d_status, void* stream);
/* One foreign file of many gzip members, in one pass (csrc/dmx_pfind.h, csrc/dmx_inflate_par_host.cpp,
 * csrc/dmx_inflate_dev.hip; DESIGN.md §3.1 "One foreign file of many members"): what `cat a.gz b.gz`,
 * `gzip -c >> log.gz`, pgzip, Hadoop and WARC writers leave.  The calls above stop at the first
 * trailer; these go on.  gzip only: fmt is DMX_BATCH_AUTO or DMX_BATCH_GZIP (ZLIB and RAW: -E_INVAL),
 * and a file that does not begin 1F 8B has status -E_ZHEAD under both.
 *   The rule behind a member's 8-byte trailer, at byte q: the file ends there; or z[q], z[q + 1] are
 *   1F 8B and a member follows, whose header is read as the first one's (its error is the file's
 *   status: -E_ZCMPMT, -E_RESERV, -E_ZHEAD for a header cut short); anything else -- zero padding,
 *   junk, a lone 1F as the last byte -- is trailing data and ignored, in_used = q.  A trailer cut
 *   short is -E_CRC.  The output is the members' data back to back; a match distance that reaches
 *   before its own member's first byte is -E_HUFDIS.
 *   The plan is the single stream's with a second kind of candidate, a member start: a byte p inside
 *   the chunk with 1F 8B 08, no reserved flag bit, a header that dmx_gz_head accepts and a first
 *   block that is not of type 3.  A chunk's candidate is the lowest bit offset either rule accepts.
 *   A measure walk does not stop at BFINAL: it takes the trailer, applies the rule above, and stands
 *   at the member's first byte (bit 8 q) and at its first block (behind the header), so a candidate
 *   of either kind ends it.  Chunk 0 begins at bit 0, the first header.  end_bit of a live chunk is
 *   bit of the next (a chunk that ends with a member ends at bit 8 q of the next; the last one at the
 *   end of the last block), out_off the exclusive scan of out_len; a chunk may be a header alone, with
 *   out_len 0.
 * dmx_pmember (32 bytes) names a member: in_off the byte of its 1F, out_off / out_len its data in the
 * output, crc and isize as its trailer stores them.  dmx_par_multi_status (64 bytes) is a
 * dmx_par_status (check: the last member's stored CRC-32; ncand counts both kinds; work_len for
 * dmx_inflate_parallel_multi_work(out_len, nlive, nmembers)) with nmembers and bad_member: the first
 * member in file order whose CRC-32 or ISIZE is wrong where the status is -E_CRC / -E_LEN from the
 * check, else 0xFFFFFFFF.
 * dmx_inflate_parallel_multi_plan_host: the plan on the host.  chunks receives at most cap live
 * chunks, members at most mcap member records (the model for the device's table); -E_SZ where
 * nlive > cap or nmembers > mcap, with both counts in the record.  Otherwise as
 * dmx_inflate_parallel_plan_host (-E_INVAL also for members NULL with mcap > 0 and fmt ZLIB / RAW).
 * dmx_inflate_parallel_multi_plan_async: four launches as dmx_inflate_parallel_plan_async; d_plan
 * (256-byte aligned, plan_bytes >= dmx_inflate_parallel_multi_plan_work(zbytes, chunk_bytes)) holds
 * the dmx_par_multi_status at offset 0, the live chunks at 256, and behind the single plan's parts
 * (before the tables) the walks' member offsets (8 nc) and 16 bytes per live chunk: the output
 * offset at which the member it begins in began, the index of the first member that begins in it,
 * and the output offset inside it of its first member start.  Record and chunks equal the host
 * plan's field for field.
 * dmx_inflate_parallel_multi_decode_async: begin, cells, tails, pack, with verify != 0 the segmented
 * check (segment scan, CRC-32 remainders per segment of at most 64 KiB that never crosses a member,
 * a combine per member), status.  A wave per live chunk crosses the member boundaries inside its
 * chunk (trailer, header, on at the next body) and writes d_members: the begin side (in_off,
 * out_off) of the members whose header it reads, the end side (out_len, crc, isize) of those whose
 * last block it decodes.  *d_status (8-byte aligned, 64 bytes) as dmx_inflate_parallel_decode_async's,
 * with -E_SZ also for nmembers > max_members (the record holds the needed nlive, nmembers, out_len
 * and work_len) and, with verify != 0, per member the CRC-32 and then ISIZE mod 2^32: -E_CRC, -E_LEN,
 * bad_member the first such member.  With verify == 0 neither is looked at.  No byte at or beyond
 * out_cap and no record at or beyond max_members is ever written.  The rules of the single calls hold:
 * no allocation, no host synchronisation, grids from the host arguments alone (zbytes, chunk_bytes,
 * max_live, max_members, out_cap, verify), every record and counter reset by a kernel of the call,
 * surplus workgroups leave at once, after a status no later stage runs.  d_members: 8-byte aligned,
 * max_members records.  dmx_inflate_parallel_multi_work(out_cap, max_live, max_members) bytes of
 * d_work always suffice (a multiple of 256, monotone in all three).  Argument errors return before
 * any device call, as for the single calls (also d_members NULL with max_members > 0 or not 8-byte
 * aligned, fmt ZLIB / RAW).  An index of seek points across members is not built. */
typedef struct { uint64_t in_off, out_off, out_len; uint32_t crc, isize; } dmx_pmember;      /* 32 bytes */
typedef struct { dmx_par_status st; uint32_t nmembers, bad_member; } dmx_par_multi_status;   /* 64 bytes */
int dmx_inflate_parallel_multi_plan_host(const void* z, uint64_t zbytes, uint32_t fmt, uint32_t chunk_bytes,
                                         dmx_pchunk* chunks, uint32_t cap, dmx_pmember* members, uint32_t mcap,
                                         dmx_par_multi_status* st);
uint64_t dmx_inflate_parallel_multi_plan_work(uint64_t zbytes, uint32_t chunk_bytes);
int dmx_inflate_parallel_multi_plan_async(const void* d_z, uint64_t zbytes, uint32_t fmt, uint32_t chunk_bytes,
                                          void* d_plan, uint64_t plan_bytes, void* stream);
uint64_t dmx_inflate_parallel_multi_work(uint64_t out_cap, uint32_t max_live, uint32_t max_members);
int dmx_inflate_parallel_multi_decode_async(const void* d_z, uint64_t zbytes, const void* d_plan, uint64_t plan_bytes,
                                            uint32_t max_live, uint32_t max_members, void* d_out, uint64_t out_cap,
                                            dmx_pmember* d_members, void* d_work, uint64_t work_bytes, int verify,
                                            dmx_par_multi_status* d_status, void* stream);
/* One foreign stream, indexed once and read many times: seek points (csrc/dmx_inflate.c,
 * csrc/dmx_inflate_dev.hip; DESIGN.md §3.1 "Seek points").  The index of zran, indexed_gzip and
 * rapidgzip's --export-index: the stream is decoded once, serially and exactly, on the host, and at
 * block boundaries about every `span` bytes of output a point records the bit offset, the output
 * offset and the 32 KiB of output in front of it.  From then on every point decodes on its own: a
 * whole decode is one wave per point, a range read decodes only the points it touches.  No search,
 * no speculation: nothing of the plan above is used.
 * dmx_zindex_build_host: host only, no GPU.  z[0, zbytes) under fmt (DMX_BATCH_AUTO / ZLIB / GZIP /
 * RAW, dmx_frame_head's rules) is decoded with deflate_decompress's block routines and its trailer
 * (Adler-32, or CRC-32 and ISIZE) is checked here, once; a stream deflate_decompress refuses gets
 * the same status in st->status and no index (the three arrays stay NULL).  Bytes behind the trailer
 * are ignored; in_used says where they start (the next member of a multi-member .gz: the caller's).
 *   point 0 is the first block of the body: out_off 0, no window.  A further point is placed at the
 *   first block boundary at which the output since the point before is >= span; the boundary is the
 *   bit of the next block's BFINAL bit, before any stored block's alignment.  span: 0 is
 *   DMX_ZINDEX_DEF_SPAN (256 KiB: 12.5 % of the output in windows, about 400 points per 100 MB), else
 *   1 .. DMX_ZINDEX_MAX_SPAN (2^30); 1 makes every block that produced output end a point.  Points fall on
 *   block boundaries only, so a stream that is one giant block is one point, and a point is as long as
 *   the blocks that make up its span (zlib's blocks of text hold some 60 KB; of zeros 4.2 MB).  An
 *   empty final block behind a boundary is a last point with out_len 0.
 *   points[k] (dmx_zpoint = dmx_pchunk): bit, end_bit (the bit of the next point; the last point's is
 *   the bit behind the final block's last bit), out_off (the exclusive scan of out_len), out_len.
 *   adlers[k]: the Adler-32 of that point's out_len bytes.  windows + k * DMX_ZINDEX_WINDOW: a slot of
 *   32 768 bytes with the wlen = min(out_off, 32768) bytes in front of out_off right-aligned in it,
 *   zeros before them.
 * The three arrays are malloc'd (the caller frees each with free(), as dmx_inflate_dict_host's
 * output).  The record (40 bytes): status, format (1, 2, 3), out_len, in_used through the trailer,
 * check (the stored Adler-32 / CRC-32; 0 for raw), npoints, span (the value used).  After a stream
 * error everything but status, format and span is 0.  Memory: the output is not kept -- the builder
 * holds the largest block plus 1 MiB + 32 KiB of it, and the index; the index's arrays grow by doubling
 * while it is built, so at their peak they take up to twice their final size (32 804 bytes a point),
 * and are cut back to it before they are returned.  Returns 0 with the record in
 * *st, -E_INVAL (st or an array pointer NULL, z NULL with zbytes > 0, fmt above 3), -E_RANGE (span
 * above 2^30, more than 2^32 - 1 points) or -E_MALLOC.
 * dmx_inflate_points_async: nsel entries of such an index decoded on the device, side by side, one
 * wave each, with dmx_inflate_batch_async's geometry and promises: a dmx_bresult per entry, a failing
 * entry never changes a neighbour's bytes or result, no byte outside an entry's own
 * [dst, dst + out_len) is written, two launches (reset, decode), no allocation, no host
 * synchronisation, a linear chain that can be captured into a graph.  Entry e decodes point
 * k = d_sel[e] (d_sel NULL: k = e) to d_out + d_dst_off[e] (d_dst_off NULL: the point's own out_off):
 * the ring is primed with the point's window, the reader is set up on the point's own bytes
 * z[bit >> 3, ceil(end_bit / 8)) only -- zeros past them, so an overrun is -E_LEN, and streams above
 * 4 GiB work: only one point's compressed extent is bounded by 0xFFFFFFF0 -- and blocks are decoded
 * until exactly end_bit bits are consumed.  Statuses: the stream table's for what the blocks hold;
 * -E_SZ for a block boundary beyond end_bit, BFINAL short of end_bit, more than out_len bytes, or
 * fewer at the end; -E_HUFDIS for a distance before the window; -E_ZADL32 where d_adler is given and
 * d_adler[k] is not the Adler-32 of the bytes produced (per point, so any subset verifies; there is
 * no whole-stream check on the device); -E_RANGE, with nothing of the entry read or written, for
 * k >= npoints, bit >= end_bit, end_bit > 8 * zbytes, an extent above 0xFFFFFFF0, or
 * [dst, dst + out_len) outside d_out[0, out_bytes).  Destinations that overlap are the caller's error.
 * d_results[e]: status, format 3, out_len, in_used = the bytes of the point's extent, check = the
 * computed Adler-32; after an error the last three are 0.  d_status: dmx_batch_status over the
 * entries.  The capacity of an entry is always the finite out_len, so every loop ends by capacity or
 * by input.  Long zero-run streams (zlib's multi-megabyte blocks whose literal/length code is two
 * 1-bit codes) decode like any other: up to 16 MiB of zeros at level 6, whole and by ranges, is in
 * the GPU suite (tests/test_gpu_refill.py).  The runs that did not return on such streams had every
 * refill of the bit reader between a length and its distance, where the reader's stream segments
 * did not advance, so it re-read words it had consumed; that refill now advances them (DESIGN.md
 * §3.1 "Equal-size tokens").
 * d_work: 256-byte aligned, work_bytes >= dmx_inflate_points_work(nsel) (= dmx_inflate_batch_work).
 * Returns before any device call: -E_INVAL (d_results, d_status, d_work NULL; d_points or d_windows
 * NULL with nsel > 0; d_z NULL with zbytes > 0; d_out NULL with nsel > 0; d_points, d_dst_off,
 * d_results or d_status not 8-byte, d_adler or d_sel not 4-byte aligned; d_work not 256-byte aligned
 * or work_bytes too small); else 0 or -E_DEVICE. */
#define DMX_ZINDEX_WINDOW 32768u
#define DMX_ZINDEX_DEF_SPAN (256u << 10)
#define DMX_ZINDEX_MAX_SPAN (1u << 30)
typedef dmx_pchunk dmx_zpoint;                                                    /* 32 bytes: a seek point */
typedef struct { int32_t status; uint32_t format; uint64_t out_len; uint64_t in_used;
                 uint32_t check; uint32_t npoints; uint32_t span; uint32_t reserved; } dmx_zindex_status; /* 40 bytes */
int dmx_zindex_build_host(const void* z, uint64_t zbytes, uint32_t fmt, uint32_t span, dmx_zpoint** points,
                          uint32_t** adlers, uint8_t** windows, dmx_zindex_status* st);
uint64_t dmx_inflate_points_work(uint32_t nsel);
int dmx_inflate_points_async(const void* d_z, uint64_t zbytes, const dmx_zpoint* d_points,
                             const uint32_t* d_adler,     /* NULL: no verification */
                             const void* d_windows, uint32_t npoints,
                             const uint32_t* d_sel,       /* NULL: entry e is point e */
                             const uint64_t* d_dst_off,   /* NULL: the points' own out_off */
                             uint32_t nsel, void* d_out, uint64_t out_bytes, dmx_bresult* d_results,
                             void* d_work, uint64_t work_bytes, dmx_batch_status* d_status, void* stream);
/* Seek points from the one-pass decode (csrc/dmx_zindex_dev.hip, csrc/dmx_zsel.h; DESIGN.md §3.1 "Seek
 * points from the one-pass decode").  When dmx_inflate_parallel_decode_async ends, everything an index
 * holds is on the device: the live chunks in the plan buffer are true block boundaries with exact bit,
 * end_bit, out_off and out_len, and d_out supplies every window and every point's Adler-32.  So the
 * first read of a foreign stream costs about one one-pass decode and leaves the index of the calls
 * above in device memory: no host decode, and the stream never leaves the device.
 * The selection is dmx_zindex_build_host's rule restricted to chunk boundaries (dmx_zsel.h, one text
 * for host and device): point 0 is live chunk 0 (out_off 0, no window); a further point begins at the
 * first live chunk at which the output since the point before began is >= span (0: DMX_ZINDEX_DEF_SPAN,
 * else 1 .. DMX_ZINDEX_MAX_SPAN; 1: every live chunk that follows output).  A point has the bit and
 * out_off of its first chunk, the next point's bit as end_bit (the last: the last live chunk's
 * end_bit) and the sum of its chunks' out_len; a last chunk of no output behind such a boundary is a
 * last point of length 0, as on the host.  Every point but the last holds at least min(span, out_len)
 * bytes, so npoints <= min(out_len / span + 1, nlive): dmx_zindex_points_bound(out_cap, max_live, span)
 * is that bound for capacities, at least 1.  Every point is a run of whole blocks.
 * dmx_zindex_from_parallel_async runs behind dmx_inflate_parallel_decode_async on the same stream:
 * d_plan and d_out as those two calls left them, *d_dec_status the decode call's record (8-byte
 * aligned, device memory), out_cap and max_live the decode's capacities.  It follows their rules: no
 * allocation, no host synchronisation; four launches (select, windows, fold, finish) whose grids
 * follow from out_cap, max_live, max_points and span alone and the device's size, a linear chain that
 * can be captured into one graph with plan and decode; every record and counter is reset by a kernel
 * of the call; workgroups beyond the device-side counts leave at once.  d_plan and d_out are read,
 * never written.  *d_status (dmx_zindex_status, 40 bytes, 8-byte aligned):
 *   a decode record with a status: that status, -E_SZ included, with format and span; everything else
 *     is 0 and nothing of the three arrays is written;
 *   -E_INVAL for a record that does not fit d_plan, out_cap and max_live (nlive 0 or above max_live,
 *     out_len above out_cap, chunks beyond plan_bytes or that do not end at out_len);
 *   -E_SZ when npoints > max_points or work_bytes < dmx_zindex_device_work(out_len, npoints): the
 *     record holds the needed npoints, and format, out_len and span; nothing of the three arrays is
 *     written (the two-call idiom);
 *   else 0 with format, out_len, in_used and check from the decode's record, npoints, and span the
 *     value used.  d_points[0, npoints) follow the rule above; d_adlers[k] is the Adler-32 of
 *     d_out[out_off, out_off + out_len) -- always Adler-32, whatever the stream's own check is: it is
 *     what dmx_inflate_points_async compares; slot k of d_windows (DMX_ZINDEX_WINDOW bytes each) holds
 *     the wlen = min(out_off, 32768) bytes in front of out_off right-aligned, zeros before them.  No
 *     byte at or beyond d_points[npoints], d_adlers[npoints] or slot npoints is written.
 * The source of a window lies at any byte alignment: whole aligned 16-byte groups inside
 * d_out[0, out_len) are loaded, single bytes at its ends, nothing outside it.  d_work: 256-byte
 * aligned; dmx_zindex_device_work(out_cap, max_points) bytes always suffice (a multiple of 256,
 * monotone in both).  Returns before any device call: -E_INVAL (a NULL pointer; d_plan or d_work not
 * 256-byte, d_points, d_dec_status or d_status not 8-byte, d_adlers not 4-byte aligned; plan_bytes
 * below dmx_inflate_parallel_plan_work(1, 0) or work_bytes below dmx_zindex_device_work(0, 1)),
 * -E_RANGE (span above 2^30); else 0 or -E_DEVICE.
 * dmx_zindex_from_chunks_host is the host twin, no GPU: the same three arrays, malloc'd (the caller
 * frees each with free()), from the plan's live chunks (dmx_inflate_parallel_plan_host) and the
 * decoded bytes out[0, out_len), which the chunks must tile in order (else -E_INVAL, as for a NULL
 * pointer or nlive 0).  For the same chunks, bytes and span the device's arrays equal them byte for
 * byte.  Returns 0, -E_INVAL, -E_RANGE (span) or -E_MALLOC. */
uint32_t dmx_zindex_points_bound(uint64_t out_cap, uint32_t max_live, uint32_t span);
uint64_t dmx_zindex_device_work(uint64_t out_cap, uint32_t max_points);
int dmx_zindex_from_parallel_async(const void* d_plan, uint64_t plan_bytes,
                                   const dmx_par_status* d_dec_status,   /* the decode call's record */
                                   const void* d_out, uint64_t out_cap, uint32_t max_live, uint32_t span,
                                   dmx_zpoint* d_points, uint32_t* d_adlers, void* d_windows, uint32_t max_points,
                                   void* d_work, uint64_t work_bytes, dmx_zindex_status* d_status, void* stream);
int dmx_zindex_from_chunks_host(const dmx_pchunk* chunks, uint32_t nlive, const void* out, uint64_t out_len,
                                uint32_t span, dmx_zpoint** points, uint32_t** adlers, uint8_t** windows,
                                uint32_t* npoints);
/* Batches of independent buffers into independent streams (csrc/dmx_encode_batch.hip):
 * the encode's counterpart of dmx_inflate_batch_async.  nstreams buffers become nstreams complete
 * zlib streams, gzip members or raw DEFLATE streams, every one decodable on its own, in one chain of
 * launches: blocks are independent, so a thousand 100 KB buffers are the same workgroups as one
 * 100 MB buffer.
 * Stream k is d_in[in_off, in_off + in_len): any alignment, gaps and overlaps between streams
 * allowed.  Its output is written at d_out + d_results[k].out_off; the streams are packed back to
 * back in index order, each from a byte boundary: d_results[k + 1].out_off == d_results[k].out_off +
 * d_results[k].out_len, and d_status->out_len is the total.  The bytes of stream k are exactly what
 * dmx_encode_async writes for that buffer alone with the same opts (an empty buffer: the empty
 * input's stream, zlib 78 9C 03 00 00 00 00 01, raw 03 00, gzip 20 bytes); check is the stream's
 * Adler-32, its CRC-32 under DMX_F_GZIP, 0 for a raw stream.  The CRC pass loads whole 16-byte aligned
 * groups as dmx_crc32_async does: up to 15 bytes before and after a buffer, inside the groups that
 * hold its first and last byte, are read and never looked at -- d_in must be readable there, which
 * a buffer inside an allocation always is.
 * opts->flags must frame a complete stream: DMX_ZLIB, DMX_GZIP, or DMX_F_FINAL alone (raw RFC 1951).
 * Without DMX_F_FINAL, with only one of DMX_F_HEADER / DMX_F_TRAILER, with DMX_F_GZIP but no
 * header, or with DMX_F_DICT, DMX_F_SPLIT or DMX_F_BGZF the call returns -E_INVAL.  The parse and
 * block options work as in a single encode: max_chain (0 = exhaustive), DMX_F_LAZY, DMX_F_DEEP with
 * deep_chain, DMX_F_STORE_CHECK, DMX_F_EXACT_SORT, any sw.
 * The descriptors are device memory, so the grids follow from max_blocks, the caller's capacity:
 * dmx_encode_batch_blocks gives a safe one, and a caller who knows the lengths passes the exact sum
 * of max(1, ceil(in_len / sw)) over the streams (an empty stream has one empty block, which carries
 * its framing).  Workgroups beyond the real block count return at once.  No allocation, no host
 * synchronisation, a linear chain of launches whose number and grids follow from nstreams,
 * max_blocks, opts and the device's size, capturable into a graph; every record and counter is
 * reset by a kernel of the call.
 * Per stream: one that lies outside d_in[0, in_bytes) (a test that cannot wrap) gets -E_RANGE,
 * out_len 0 and nblocks 0 (its out_off is where the next stream begins); its neighbours keep the
 * bytes they would have had.  d_status->nfailed is an integer sum and first_bad an integer minimum
 * (0xFFFFFFFF when none): nothing depends on the order in which workgroups run.
 * The whole call: d_status->status = -E_SZ when the batch needs more than max_blocks blocks (the
 * record then holds the needed nblocks; nothing was encoded, so out_len and every stream's out_off
 * and out_len are 0), or when (out_len + 3) & ~3 exceeds out_cap, dmx_encode_async's own rule (the
 * record then holds the needed out_len, and d_results[*].out_off / out_len are written).  After
 * -E_SZ no byte of d_out is written: the two-call idiom of dmx_bgzf_read_ranges_async.  On success no
 * byte at or beyond (out_len + 3) & ~3 is written.  d_status->in_len is the sum of in_len over the
 * streams with status 0.
 * dmx_encode_result after a batch gives the totals: n, ntokens, the block counts (an empty stream's
 * block counts as a fixed one), out_len, status, and adler 0.  dmx_block_index after a batch is
 * -E_INVAL: its out_off = b * sw has no meaning there.
 * The context must be reserved with dmx_ctx_reserve_batch(ctx, max_blocks, max_streams, sw, flags),
 * the only place that allocates (synchronising when it does): the workspace for max_blocks blocks,
 * the block table, and the plan's scratch for max_streams streams.  A batch runs without the work
 * lists, the uniform-block dedupe and the noise check's speculative copy, and it leaves no
 * launch-shape hint: single encodes on the same context before and after it are unaffected.
 * dmx_encode_batch_blocks: a bound on the blocks of any nstreams buffers of total_in bytes together,
 * total_in / sw + nstreams.  dmx_encode_batch_bound: a bound on d_status->out_len rounded up to 4 for
 * them, at least the sum of dmx_max_compressed_flags(in_len_k, sw, flags) rounded up to 4.  Both are
 * monotone in total_in and nstreams (sw 0 = 32768; values that do not fit saturate).
 * Returns before any device call: -E_INVAL (ctx, d_results, d_status or d_out NULL, d_in NULL with
 * in_bytes > 0, d_streams NULL with nstreams > 0; d_streams, d_results or d_status not 8-byte
 * aligned, d_out not 4-byte aligned; the flags above), -E_RANGE (sw, max_chain, deep_chain, as
 * dmx_encode_async checks them; nstreams or max_blocks above 0x7FFFFFFF), -E_SZ (the context is not
 * reserved for max_blocks blocks or nstreams streams); else 0 or -E_DEVICE. */
typedef struct { uint64_t in_off, in_len; } dmx_estream;                 /* 16 bytes */
typedef struct { int32_t status; uint32_t nblocks; uint64_t out_off; uint64_t out_len;
                 uint32_t check; uint32_t reserved; } dmx_eresult;       /* 32 bytes */
typedef struct { int32_t status; uint32_t nfailed; uint32_t first_bad; uint32_t nblocks;
                 uint64_t out_len; uint64_t in_len; } dmx_ebatch_status; /* 32 bytes */
uint32_t dmx_encode_batch_blocks(uint64_t total_in, uint32_t nstreams, int32_t sw);
uint64_t dmx_encode_batch_bound(uint64_t total_in, uint32_t nstreams, int32_t sw, uint32_t flags);
int dmx_ctx_reserve_batch(dmx_ctx* ctx, uint32_t max_blocks, uint32_t max_streams, int32_t sw, uint32_t flags);
int dmx_encode_batch_async(dmx_ctx* ctx, const void* d_in, uint64_t in_bytes,
                           const dmx_estream* d_streams, uint32_t nstreams, uint32_t max_blocks,
                           const dmx_opts* opts, void* d_out, uint64_t out_cap,
                           dmx_eresult* d_results, dmx_ebatch_status* d_status, void* stream);
/* Batches against preset dictionaries (csrc/dmx_encode_batch.hip): the encode's
 * counterpart of dmx_inflate_batch_dict_async, beside dmx_encode_batch_async as that call is beside
 * dmx_inflate_batch_async.  The dictionaries are described as there: dictionary j is
 * d_dict[d_dicts[j].off, + d_dicts[j].len), any length and alignment, device memory; stream k uses
 * dictionary d_dict_of[k], or none where that is DMX_BATCH_NODICT; d_dict_of == NULL: every stream
 * uses dictionary 0 (none when ndicts == 0).
 * The bytes of stream k are exactly what dmx_encode_async writes for buffer k alone with the same opts
 * and opts->dict / dict_len set to stream k's dictionary (opts->dict itself is ignored here); a stream
 * without a dictionary is written as with DMX_F_FDICT cleared, a 78 9C header and no history for its
 * first block.  So block 0 of a stream searches the last min(len, sw) bytes of its dictionary, block
 * j >= 1 searches block j - 1 of its own stream, and no block searches another stream's bytes.
 * Every dictionary is sorted once per call, however many streams share it.  Under DMX_F_FDICT a
 * stream that names a dictionary begins 78 BB and the DICTID, the dictionary's Adler-32, which a
 * kernel of the call computes: the dictionaries' bytes may change between two replays of a captured
 * call.
 * opts->flags must hold DMX_F_DICT, and frame DMX_ZLIB or DMX_F_FINAL alone (raw); DMX_F_FDICT only
 * with DMX_ZLIB.  DMX_F_GZIP, DMX_F_BGZF, DMX_F_SPLIT, half a container or a missing DMX_F_DICT
 * return -E_INVAL.  The parse and block options work as in a single encode.
 * Everything dmx_encode_batch_async promises holds: streams packed in index order, a status per
 * stream, neighbours untouched, the -E_SZ two-call idiom for max_blocks and out_cap, no allocation,
 * no host synchronisation, a linear chain of launches whose number and grids follow from nstreams,
 * max_blocks, ndicts, opts and the device's size, capturable into a graph; every record is reset by
 * a kernel; dmx_encode_result gives the totals; dmx_block_index is -E_INVAL.
 * Per stream (no blocks, out_len 0, neighbours keep their bytes): -E_RANGE for a buffer outside
 * d_in, for d_dict_of[k] >= ndicts that is not DMX_BATCH_NODICT, and for a d_dicts record outside
 * d_dict[0, dict_bytes) (a test that cannot wrap); under DMX_F_FDICT -E_INVAL for a dictionary of
 * length 0 or above sw, the single encode's verdict.  Without DMX_F_FDICT a dictionary of length 0
 * is no history and a longer one gives its last sw bytes.  nfailed counts both, first_bad is the
 * lowest such index.
 * The context must be reserved with dmx_ctx_reserve_batch_dict(ctx, max_blocks, max_streams,
 * max_dicts, sw, flags), the only place that allocates: what dmx_ctx_reserve_batch allocates, chain
 * slots for max_blocks + max_dicts (a slot is 64 KiB of sorted positions and 16 KiB of bucket ends
 * whatever sw is: 80 KiB per block beside the workspace's own 260 KiB per block, about 5 GB of
 * slots for 65 536 one-block streams), and max_dicts DICTID words.  On a context not reserved for it
 * the call returns -E_SZ.  dmx_encode_batch_dict_bound: dmx_encode_batch_bound with 4 more bytes per
 * stream under DMX_F_FDICT.  dmx_encode_batch_dict_geometry (tests): the workgroups of the history
 * search's loop, one per compute unit of the current device; a call launches at most that many and
 * at most max_blocks, each over a contiguous range of table entries.  DMX_HOOK_BDICT_SIMPLE 1 (tests,
 * measurements) runs that search with a workgroup per table entry instead, as the single encode
 * does; the output is the same.
 * Returns before any device call: -E_INVAL (as dmx_encode_batch_async; d_dicts NULL with ndicts > 0,
 * d_dict NULL with dict_bytes > 0, d_dicts not 8-byte or d_dict_of not 4-byte aligned; the flags
 * above), -E_RANGE (as there; ndicts above 0x7FFFFFFF), -E_SZ (the reservation); else 0 or -E_DEVICE. */
uint64_t dmx_encode_batch_dict_bound(uint64_t total_in, uint32_t nstreams, int32_t sw, uint32_t flags);
void dmx_encode_batch_dict_geometry(uint32_t* hist_grid);
int dmx_ctx_reserve_batch_dict(dmx_ctx* ctx, uint32_t max_blocks, uint32_t max_streams, uint32_t max_dicts,
                               int32_t sw, uint32_t flags);
int dmx_encode_batch_dict_async(dmx_ctx* ctx, const void* d_in, uint64_t in_bytes,
                                const dmx_estream* d_streams, uint32_t nstreams, uint32_t max_blocks,
                                const void* d_dict, uint64_t dict_bytes, const dmx_bdict* d_dicts, uint32_t ndicts,
                                const uint32_t* d_dict_of,   /* per stream: index or DMX_BATCH_NODICT; NULL = all use 0 */
                                const dmx_opts* opts, void* d_out, uint64_t out_cap,
                                dmx_eresult* d_results, dmx_ebatch_status* d_status, void* stream);
/* Host-buffer convenience (H2D, index, decode, D2H) on the cached per-device context
 * dmx_encode_host uses: any BGZF file z[0..zlen) into out. *out_len receives the decoded length
 * (the sum of the ISIZEs) whenever the file indexes, also when out_cap is too small (-E_SZ,
 * nothing decoded).  verify != 0 checks every member's CRC-32 on the device (-E_CRC).  An empty
 * file, or one of empty members only, gives 0 bytes and 0.  Returns 0, the index walk's status,
 * or the decode's device status. */
int dmx_bgzf_decode_host(const uint8_t* z, uint64_t zlen, uint8_t* out, uint64_t out_cap, uint64_t* out_len,
                         int verify);

/* Introspection of the last encode of ctx (tests / fd_stats): per-block token
 * counts and the token stream (t = byte | dist << 9 | len),
 * per-block BTYPE, and the lit/len + distance code lengths (286 + 30 per block). */
int dmx_last_blocks(dmx_ctx* ctx, uint32_t* ntok, uint8_t* btype, uint32_t* hdr_bits,
                    uint32_t nblk_cap);
int dmx_last_tokens(dmx_ctx* ctx, uint32_t blk, uint32_t* tok, uint32_t cap);
int dmx_last_code_lengths(dmx_ctx* ctx, uint32_t blk, uint8_t* lens316);
/* DEFLATE block `sub` of sw block `blk` (DMX_F_SPLIT emits up to 4 per sw block):
 * token range [tok_range[0], tok_range[1]), BTYPE, header bits, and its 286 + 30 code
 * lengths.  Returns the number of DEFLATE blocks of `blk`, or -E_RANGE. */
int dmx_last_subblock(dmx_ctx* ctx, uint32_t blk, uint32_t sub, uint32_t* tok_range, uint32_t* btype,
                      uint32_t* hdr_bits, uint8_t* lens316);

/* Per-kernel HIP-event timing of subsequent encodes on the context's launches
 * (bench): enable, then read the mean milliseconds per launch of each stage
 * {chain, match, huff, scan, pack} and of the whole encode, and the number of timed encodes.
 * enable: 0 off, 1 every stage boundary, 0x100 | s only stage s's two events (s = 0..4; the
 * other stages and the whole encode read 0), and with | every << 12 (every = 2..255) on
 * every `every`-th encode only.  Each event record costs a few microseconds of idle
 * between kernels. */
int dmx_ctx_set_timing(dmx_ctx* ctx, int enable);
int dmx_ctx_stage_times(dmx_ctx* ctx, double* ms6, uint32_t* count);

/* Diagnostic: per-block match-kernel phase stamps (cycles) of the last encode, when the
 * process runs with DMX_STAMPS=1: 16 x u64 per block (see dmx_kernels.hip). */
int dmx_debug_stamps(dmx_ctx* ctx, uint64_t* out16, uint32_t nblk);

/* The reference's estimate fields of struct compress_stats (DMX_STATS=ref, the default of
 * deflate_compress's fd_stats channel): a host restatement of its two adaptive Huffman trees
 * and code-length pricing (csrc/dmx_refstats.c).  create() starts a stream (the end-of-block
 * code counted once, deflate_compress.c:234); feed() takes tokens in stream order (t = byte,
 * or dist << 9 | len) and fills rec[k].tree_bits / ll_bits / d_bits after token k (the other
 * fields untouched).  Returns 0, -E_INVAL, or -E_RANGE at the first token whose fields would
 * exceed INT_MAX or that is not a valid token; *nfilled = records filled.  Host only. */
typedef struct dmx_refest dmx_refest;
dmx_refest* dmx_refest_create(void);
void dmx_refest_destroy(dmx_refest* e);
int dmx_refest_feed(dmx_refest* e, const uint32_t* tok, uint32_t ntok, struct compress_stats* rec,
                    uint32_t* nfilled);

/* Adler-32 combine (RFC 1950 math): adler of A||B from adler(A), adler(B), len(B). */
uint32_t dmx_adler32_combine(uint32_t a, uint32_t b, uint64_t len_b);

/* ---- CRC-32 (IEEE 802.3 / RFC 1952 §8; also PNG's chunk CRC), csrc/dmx_crc.hip ---- */
/* Enqueue the CRC-32 of the device buffer d_in[0..n), any alignment, on `stream` (NULL = the
 * context's); the value lands in the device word d_crc (4-byte aligned).  n == 0 gives 0.  Two
 * launches, no allocation, no host synchronisation (graph-capturable).  The kernel loads whole
 * 16-byte aligned groups: up to 15 bytes before d_in and after d_in + n, in the aligned
 * groups that hold the first and the last byte, are read (and masked), never written -- a
 * sub-buffer's neighbours must be readable memory, which bytes of the same 16-byte group
 * are.  The scratch (4 bytes
 * per 32 KiB) is the context's: -E_SZ when n is more than the context is reserved for
 * (dmx_ctx_reserve), and calls that share a context -- DMX_F_GZIP encodes included -- must be
 * ordered on one stream.  Returns 0 or -E_*. */
int dmx_crc32_async(dmx_ctx* ctx, const void* d_in, uint64_t n, uint32_t* d_crc, void* stream);
/* Enqueue the CRC-32 of every sw-byte block of d_in[0..n) (the last one may be short) on
 * `stream`: d_crc[b] (4-byte aligned, ceil(n / sw) words) receives block b's finished value.
 * d_in may have any alignment, sw is 1..32768 (0 = 32768; else -E_RANGE).  One launch, no
 * allocation, no host synchronisation (graph-capturable), and no scratch of the context: calls
 * need no ordering against other work of the context.  Reads whole 16-byte groups as
 * dmx_crc32_async does.  -E_SZ when there are 2^31 blocks or more.  Returns 0 or -E_*. */
int dmx_crc32_blocks_async(dmx_ctx* ctx, const void* d_in, uint64_t n, int32_t sw, uint32_t* d_crc, void* stream);
/* Enqueue the CRC-32 of the nblk ranges of d_in[0..n) that the device index lists (bit is not
 * read): d_crc[k] (4-byte aligned, nblk words) receives the finished value of
 * d_in[out_off_k, out_off_k + out_len_k).  out_off is any byte offset, out_len 0..65536
 * (DMX_BGZF_MAX_ISIZE; 0 gives 0); the ranges may come in any order and may overlap.  An entry
 * with out_len > 65536 or out_off + out_len > n writes nothing to its word and, when d_status is
 * not NULL, sets d_status->status = -E_RANGE unless a status is already there; the other words are
 * written all the same.  d_status is the caller's to clear.  Takes no context (the current
 * device); one launch, no scratch, no allocation, no host synchronisation (graph-capturable).
 * Reads whole 16-byte groups around the ends of every range as dmx_crc32_async does: up to 15
 * bytes before and after it, inside the aligned groups that hold its first and last byte.
 * Returns 0 or -E_*. */
int dmx_crc32_ranges_async(const void* d_in, uint64_t n, const dmx_iblock* d_index, uint32_t nblk, uint32_t* d_crc,
                           dmx_inflate_status* d_status, void* stream);
/* CRC-32 combine: crc of A||B from crc(A), crc(B), len(B).  Host only. */
uint32_t dmx_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* The CRC kernel's geometry (tests): bytes per workgroup span and per lane slice. */
void dmx_crc32_geometry(uint32_t* span, uint32_t* lane_slice);

/* ZIP archives (csrc/dmx_zip.h, dmx_zip_host.cpp, dmx_zip_dev.hip, dmx_zip_read.inc):
 * the container around raw DEFLATE streams and stored bytes that .npz, .jar, .whl, .docx and most
 * "dataset in one file" bundles use.  An index of the archive's entries, made on the host or -- for
 * an archive that lies in device memory -- on the device, and a batched decode of any selection of
 * entries with every entry's length and CRC-32 checked on the device.
 * The end record is found by the rule of CPython's zipfile: the last 22 bytes where they begin
 * PK\5\6 and end in a zero comment length, else the last PK\5\6 whose first byte lies within the final
 * 65 557 bytes; a ZIP64 locator (PK\6\7) 20 bytes in front of it and the ZIP64 end record (PK\6\6) 56
 * bytes in front of that replace its fields.  concat = end record - cd_size - cd_off (less 76 with
 * the ZIP64 records) is added to every stored offset, so prefixed and self-extracting archives work.
 * Entry fields come from the central directory (sizes and CRC-32 always, so data descriptors need no
 * handling), the ZIP64 extra (id 0x0001: usize, csize, header offset, each only where the 32-bit
 * value is 0xFFFFFFFF) and the local header, whose own name and extra lengths place the data.
 * The record: status 0 or
 *   -E_ZHEAD  no end record (or one cut short), or ZIP64 markers with a locator but no ZIP64 record
 *   -E_RANGE  zbytes > 0xFFFFFFF0 (the decoder's bound), disk numbers other than 0 / 0 / equal
 *             counts (or the locator's), more than 2^32 - 1 entries, the directory outside the file
 *   -E_LEN    the chain of headers from cd_off is not exactly nentries headers ending at cd_off + cd_len
 *   -E_SZ     cap < nentries: the first cap entries are written, nentries and out_len are the full values
 * (device only: -E_SZ with nentries 0 and ncand set where the work buffer holds too few candidates).
 * After -E_ZHEAD, -E_RANGE, -E_LEN no entry is written and nentries / out_len are 0; cd_off / cd_len
 * are set once the end record parsed.  ncand is 0 but in that one device status, where it is the
 * number of positions of the directory that parse as headers: the candidates a work buffer must hold.
 * An entry: where its data lies (data_off, csize), its decoded length, out_off = the exclusive sum of
 * usize over the entries with status 0 before it (archive order), hdr_off = the local header (concat
 * added), name_off / name_len = the name's bytes inside the central directory, crc, method, flags and
 * a status of its own, which never fails the file: -E_ZCMPMT (method other than 0 and 8), -E_RESERV
 * (flag bit 0 or 6: encrypted), -E_ZHEAD (local header's signature wrong, or the header cut),
 * -E_RANGE (data_off + csize outside the file), -E_LEN (stored with csize != usize) -- the first of
 * these in this order.  Entries with a status count 0 bytes in out_off and out_len. */
typedef struct { int32_t status; uint32_t nentries; uint64_t out_len; uint64_t cd_off; uint64_t cd_len;
                 uint32_t ncand; uint32_t reserved; } dmx_zip_status;            /* 40 bytes */
typedef struct { uint64_t data_off, csize, usize, out_off; uint64_t hdr_off, name_off; uint32_t crc; int32_t status;
                 uint16_t method, flags, name_len, reserved; } dmx_zip_entry;    /* 64 bytes */
/* Host only, no GPU: the serial walk.  Returns 0 (the outcome is in *status) or -E_INVAL (status
 * NULL, z NULL with zbytes > 0, entries NULL with cap > 0). */
int dmx_zip_index_host(const void* z, uint64_t zbytes, dmx_zip_entry* entries, uint32_t cap, dmx_zip_status* status);
/* The same record and entries for the same bytes in device memory, with dmx_bgzf_index_async's
 * contract: no context, no allocation, no host synchronisation; the number of launches and every
 * grid follow from zbytes, cap and work_bytes alone, a linear chain that can be captured into a graph;
 * the record is reset by a kernel of the call.  d_z may have any alignment; whole aligned 16-byte
 * groups are loaded: up to 15 bytes before the first and after the last byte of the directory, inside
 * the groups that hold them, are read and never looked at.  Everything lives in d_work (256-byte
 * aligned, work_bytes >= dmx_zip_index_work(zbytes, max_cand), a multiple of 256, monotone in both);
 * the candidates it holds follow from work_bytes.
 * Returns before any device call: -E_INVAL (d_status or d_work NULL, d_z NULL with zbytes > 0,
 * d_entries NULL with cap > 0; d_entries or d_status not 8-byte, d_work not 256-byte aligned;
 * work_bytes < dmx_zip_index_work(zbytes, 1)), -E_RANGE (zbytes > 0xFFFFFFF0); else 0 or -E_DEVICE. */
uint64_t dmx_zip_index_work(uint64_t zbytes, uint32_t max_cand);
int dmx_zip_index_async(const void* d_z, uint64_t zbytes, dmx_zip_entry* d_entries, uint32_t cap,
                        void* d_work, uint64_t work_bytes, dmx_zip_status* d_status, void* stream);
/* The decode of a selection of entries.  d_entries / nentries are what an index call wrote for d_z.
 * d_sel == NULL: all entries in archive order (nsel must equal nentries); else nsel selectors in any
 * order, repeats allowed.  The selected entries land packed back to back in selection order:
 * d_offsets (nsel + 1 words, 8-byte aligned) is the exclusive sum of len_k = the entry's usize, or 0
 * where the index gave it a status or the selector is >= nentries; a prepare kernel computes it.
 * Deflated entries go through dmx_inflate_batch_async's decode on its raw path (a wave per entry: one
 * very large deflated entry runs at the one-stream rate), stored entries through a copy kernel, a
 * workgroup per 64 KiB span of output.  flags: DMX_ZIP_VERIFY checks every entry's CRC-32.
 * d_results[k] as dmx_inflate_batch_async writes it, with format = the method and check = the stored
 * CRC-32; status: the entry's index status; the decoder's own; -E_SZ when more than usize bytes
 * come out, -E_LEN when fewer do or the stream needs bytes past csize; -E_CRC; -E_RANGE for a selector
 * >= nentries, or an entry whose data lies outside d_z[0, zbytes) or whose usize is above 2^43 (more
 * than DEFLATE makes of 0xFFFFFFF0 bytes; len_k is then 0 too).  d_status as there.  A failing
 * entry never changes a neighbour's bytes or result; no byte outside [0, d_offsets[nsel]) is written.
 * out_bytes smaller than d_offsets[nsel]: the call cannot know without a synchronisation and returns
 * 0; the prepare kernel sees it, nothing is decoded or written, every d_results[k].status is -E_SZ,
 * nfailed == nsel, first_bad == 0 and total_out holds the bytes needed (d_offsets is complete), so a
 * captured graph reports it on every replay.
 * Six or seven launches (reset, prepare, decode, copy, fix-up, the CRC-32 pass under DMX_ZIP_VERIFY,
 * finalise), reset and prepare alone when nsel == 0: no allocation, no host synchronisation, a linear chain
 * whose grids follow from nsel, out_bytes and the device's size.  d_work: 256-byte aligned,
 * work_bytes >= dmx_zip_read_work(nsel) (a multiple of 256, monotone).
 * Returns before any device call: -E_INVAL (d_results, d_status, d_work or d_offsets NULL, d_entries
 * NULL with nentries > 0, d_z NULL with zbytes > 0, d_out NULL with out_bytes > 0, d_sel NULL with
 * nsel != nentries; d_entries, d_offsets, d_results or d_status not 8-byte, d_sel not 4-byte, d_work
 * not 256-byte aligned; work_bytes too small), -E_RANGE (unknown flags, zbytes > 0xFFFFFFF0); else 0
 * or -E_DEVICE. */
#define DMX_ZIP_VERIFY 1u
uint64_t dmx_zip_read_work(uint32_t nsel);
int dmx_zip_read_async(const void* d_z, uint64_t zbytes, const dmx_zip_entry* d_entries, uint32_t nentries,
                       const uint32_t* d_sel, uint32_t nsel, uint32_t flags, void* d_out, uint64_t out_bytes,
                       uint64_t* d_offsets, dmx_bresult* d_results, void* d_work, uint64_t work_bytes,
                       dmx_batch_status* d_status, void* stream);
/* The geometry (tests): bytes per scan tile of the index, bytes per span of the copy kernel. */
void dmx_zip_index_geometry(uint32_t* tile);
void dmx_zip_read_geometry(uint32_t* span);

/* Seeded synthetic inputs for the bench/tests (host, deterministic). */
void dmx_gen_text(uint8_t* buf, uint64_t n, uint64_t seed);    /* enwik-style wiki text */
void dmx_gen_random(uint8_t* buf, uint64_t n, uint64_t seed);  /* splitmix64 bytes */

#ifdef __cplusplus
}
#endif
#endif /* DMX_H */

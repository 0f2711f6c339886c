// dmx_ctx.h -- the encoder context (dmx_ctx) and the host helpers shared by the HIP layer
// (dmx_kernels.hip: kernels, launches, context management) and its host-only pipeline code
// (dmx_fd.cpp: the cached per-device contexts, dmx_encode_host, the fd streaming paths).
// C++ only, internal.
#ifndef DMX_CTX_H
#define DMX_CTX_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "dmx_internal.h"
#include "../../include/dmx.h"

#ifndef DMX_STAMPS
#define DMX_STAMPS 16   // diagnostic u64 stamps per block (DMX_STAMPS=1 in the environment)
#endif

struct ScanTile;   // (dmx_kernels.hip)
struct FdPipe;     // (dmx_fd.cpp)

#define DMX_EV_RING 32

struct dmx_ctx {
    int device;
    hipStream_t stream;
    uint64_t cap_blocks;
    uint16_t* dist;   // cap_blocks * DMX_BLK: best distances in bucket order (match kernel staging)
    uint32_t* tok;    // cap_blocks * DMX_BLK
    uint32_t* hist;   // cap_blocks * DMX_HIST
    uint32_t* codes;  // cap_blocks * DMX_HIST
    uint32_t* hdr;    // cap_blocks * DMX_NSUB * DMX_HDR_WORDS
    dmx_subinfo* sub; // cap_blocks * DMX_NSUB
    dmx_blkinfo* info;
    ScanTile* tiles;  // cap_blocks / SCAN_TILE + 1: per-tile aggregates and prefixes (scan)
    uint32_t* wl;     // WL_HDR + 3 cap_blocks: the work lists of DMX_F_STORE_CHECK (WL_* comment)
    volatile uint32_t* whint;   // host-mapped pinned {nblk, |L1|, |L2|, |L4|, uniform full blocks} of the latest encode (WL_HINT)
    uint32_t* whint_dev;        // its device address (the scan kernel writes it when an encode runs without the lists)
    uint32_t ncu;     // compute units (the persistent K1 grid of the work-list mode)
    dmx_result* res;
    uint32_t* nfb;        // [0] sort fallbacks of the encode in flight (kernels add, K3's scan reads and zeroes), [1] total,
                          // [2] the CRC-32 of a DMX_F_GZIP encode's input (dmx_crc.hip writes, K3's scan reads),
                          // [3] the DICTID of a DMX_F_FDICT encode (dmx_dict_adler_launch writes, put_header reads)
    uint32_t* crc_rem;    // CRC-32 scratch (dmx_crc.hip): crc_cap span remainders; under DMX_F_BGZF (which
                          // ignores DMX_F_GZIP) the encode's finished CRC-32 per block instead, read by K4
    uint64_t crc_cap;     // spans of DMX_BLK bytes it holds: cap_blocks + 2 (0: no workspace yet)
    uint64_t* dbg;        // optional per-block phase stamps (DMX_STAMPS=1)
    uint64_t dbg_cap;
    // last encode (introspection)
    uint32_t last_nblk;
    uint32_t last_sw;
    // host staging for dmx_encode_host
    void* d_in;
    uint64_t d_in_cap;
    void* d_out;
    uint64_t d_out_cap;
    void* d_dict;         // DMX_F_DICT history of block 0 (DMX_BLK bytes)
    // dmx_encode_fd streaming buffers, kept across calls (pinning ~100 MB costs ms)
    uint8_t* fd_hin[2];   // pinned input chunks
    uint8_t* fd_hout[2];  // pinned output chunks
    void* fd_din[2];      // device input chunks (the previous one is the next chunk's history);
                          // DMX_BLK bytes in front of the chunk hold a multi-GPU worker's history
    void* fd_dout[2];     // device output chunks (a multi-GPU worker copies one while encoding into the other)
    dmx_result* fd_hres[2];  // pinned
    hipStream_t fd_cs;    // multi-GPU worker: D2H copies beside the next encode
    hipEvent_t fd_ev[2];  // multi-GPU worker: encode i done
    uint64_t fd_chunk, fd_ocap;
    struct FdPipe* fdp;   // dmx_encode_fd's pipeline buffers (single device)
    uint16_t* chs;        // DMX_F_DICT: (cap_chain) x DMX_BLK bucket-sorted positions per block (+ the dict)
    uint16_t* che;        // DMX_F_DICT: (cap_chain) x DMX_NBUCKET bucket ends
    uint64_t cap_chain;
    void* split;          // DMX_F_SPLIT: cap_split x SplitScratch (per-block plans of the 10 groups)
    uint64_t cap_split;
    uint32_t want;        // DMX_F_SPLIT / DMX_F_DICT: scratch kept reserved with the workspace
    // batch encodes (dmx_encode_batch.hip; allocated by dmx_ctx_reserve_batch only)
    dmx_bblk* btab;       // cap_btab block table entries
    uint64_t cap_btab;
    void* bplan;          // the plan's scratch for cap_bstreams streams: head, tile sums, block starts
    uint64_t cap_bstreams;
    int last_batch;       // the last encode was a batch (dmx_block_index: -E_INVAL)
    // batch encodes against dictionaries (dmx_encode_batch_dict_async; dmx_ctx_reserve_batch_dict only)
    uint32_t* bdictid;    // cap_bdicts DICTIDs: the dictionaries' Adler-32s of the call in flight
    uint64_t cap_bdicts;
    uint64_t chain_dicts; // chain slots kept beyond a slot per block and the single encode's one
    // timing: a ring of event sets so timed encodes never block the host
    int timing;       // bit k: record event k (set_timing: 1 = all six, 0x100 | s = stage s's two)
    hipEvent_t ev[DMX_EV_RING][6];
    int ev_used[DMX_EV_RING];
    uint32_t ev_next;
    uint32_t ev_every, ev_count;   // with a one-stage mask: events on every ev_every-th encode only
    double stage_ms[6];
    uint32_t stage_n;
    // test hooks (dmx_ctx_set_hook; defaults from the environment, read once at creation):
    int hk_wl;       // -1 adaptive launch shapes, 0 no work lists, 1 list shapes, 2 per-block shapes (DMX_WORKLIST)
    int hk_dedupe;   // -1 adaptive, 0 / 1 the uniform-block dedupe forced off / on (DMX_DEDUPE)
    int hk_scan3;    // 1: K3 in three launches at any size (DMX_SCAN3)
    int hk_bdict_simple;   // 1: the dictionary batch's history search with a workgroup per table entry
};

#define DMX_HIDDEN __attribute__((visibility("hidden")))
// device / pinned allocations through the fault injection of dmx_fault_set (dmx_kernels.hip)
DMX_HIDDEN bool fault_hit(int kind);
DMX_HIDDEN hipError_t dmx_malloc(void** p, size_t n);
DMX_HIDDEN hipError_t dmx_host_malloc(void** p, size_t n);
template <typename T>
static inline hipError_t dmx_malloc(T** p, size_t n) { return dmx_malloc(reinterpret_cast<void**>(p), n); }
// prints the failing call and returns 1 on an error
DMX_HIDDEN int hip_fail(hipError_t e, const char* what);
#define HIPCHK(x) do { if (hip_fail((x), #x)) return -(int)E_DEVICE; } while (0)
// the launch of the CRC-32 over index ranges (dmx_crc.hip): into d_crc, or with d_want compared
// on the device (-E_CRC into d_status: dmx_inflate_members_async, dmx_inflate_dev.hip)
DMX_HIDDEN int dmx_crc32_ranges_launch(const void* d_in, uint64_t n, const dmx_iblock* d_index, uint32_t nblk,
                                       uint32_t* d_crc, const uint32_t* d_want, dmx_inflate_status* d_status,
                                       hipStream_t s);
// the Adler-32 of d_dict[0, n) into *d_adl, one launch (dmx_inflate_dev.hip: dmx_dict_adler_kernel's
// arithmetic on one dictionary given by value): the DICTID of a DMX_F_FDICT encode
DMX_HIDDEN int dmx_dict_adler_launch(const void* d_dict, uint64_t n, uint32_t* d_adl, hipStream_t s);
// dmx_dict_adler_kernel over ndicts records: d_adl[j] = the Adler-32 of dictionary j, 0 for a record
// outside d_dict[0, dict_bytes) (dmx_encode_batch_dict_async's DICTIDs)
DMX_HIDDEN int dmx_dict_adler_batch_launch(const void* d_dict, uint64_t dict_bytes, const dmx_bdict* d_dicts,
                                           uint32_t ndicts, uint32_t* d_adl, hipStream_t s);
// the CRC-32 pass of dmx_inflate_batch_async (dmx_crc.hip): every stream with status 0 and format
// gzip is finished -- -E_CRC, else the decode's note of a wrong ISIZE as -E_LEN -- and counted in
// the summary
DMX_HIDDEN int dmx_crc32_batch_launch(const void* d_out, uint64_t out_bytes, const dmx_bstream* d_streams,
                                      uint32_t nstreams, dmx_bresult* d_results, dmx_batch_status* d_status,
                                      hipStream_t s);
// `bytes` of device scratch from the inflate's per-device stream-ordered pool (dmx_inflate_dev.hip),
// allocated on s; NULL when that fails.  The caller frees it with hipFreeAsync on the same stream.
DMX_HIDDEN void* dmx_itab_scratch(hipStream_t s, uint64_t bytes);
// The counted form of the indexed decode (dmx_inflate_dev.hip) for dmx_bgzf_read_ranges_async: a
// grid of `slots` workgroups over d_index, of which those at or past *d_count leave at once; d_gtab
// holds dmx_itab_bytes(slots) bytes of first-level tables.  d_status is the caller's to reset.
DMX_HIDDEN uint64_t dmx_itab_bytes(uint32_t slots);
DMX_HIDDEN int dmx_inflate_counted_launch(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, uint32_t slots,
                                          const uint32_t* d_count, void* d_out, uint64_t out_cap, void* d_gtab,
                                          dmx_inflate_status* d_status, hipStream_t s);
// the fd pipeline's buffers of a context (dmx_fd.cpp), freed with the context
DMX_HIDDEN void fdp_free(FdPipe* P);

#endif

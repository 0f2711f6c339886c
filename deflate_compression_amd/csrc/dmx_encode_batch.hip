// dmx_encode_batch.hip -- batches of independent buffers into independent zlib / gzip / raw DEFLATE
// streams (include/dmx.h: dmx_encode_batch_async).  Compiled into dmx_kernels.hip's
// translation unit (included at its end): the batch runs the encoder's own block code.
//
// Blocks are independent, so a batch is one encode whose blocks belong to different streams.  What
// a single encode derives from the block index -- the block's input at b * sw, its length, "first"
// and "last" -- a batch reads from a block table that the plan builds on the device:
//   1. dmx_eb_count_kernel   a thread per stream: valid?, its blocks; the tile's sums
//   2. dmx_eb_plan_scan_kernel one workgroup: the tile sums into exclusive prefixes; the head (the
//                            batch's block count, -E_SZ against max_blocks, nfailed, first_bad)
//   3. dmx_eb_starts_kernel  a thread per stream: starts[k] = the blocks before it; its record
//   4. dmx_eb_table_kernel   a thread per table entry: its stream by binary search in starts[],
//                            input offset, length, first / last marks; void beyond the real count;
//                            the block record of void entries and of an empty stream's block
// The per-thread text of 1-4 is dmx_encode_batch.h, which tests/c/encode_batch_model.cpp runs as loops.
//   5. K0 (DMX_F_STORE_CHECK), K1: the batch instantiations of store_check_block / match_block
//   6. K2: dmx_huff_kernel as it is, without DMX_F_FINAL (BFINAL is K4's, from the table)
//   7. K3: dmx_eb_scan_tile_kernel, then dmx_eb_scan_apply1_kernel, or dmx_eb_scan_kernel +
//      dmx_eb_apply_kernel (more than SA1_MAXT tiles, or the scan3 hook): the single encode's
//      layout scan with one more container rule -- a stream's first block is "align to a byte,
//      header bits" before its own element, its last block adds "pad to a byte, trailer bits"
//   8. K4: dmx_eb_pack_kernel, pack_one's batch instantiation
//   9. dmx_eb_crc_kernel (DMX_F_GZIP): every stream's CRC-32, a sibling of dmx_crc_batch_kernel
//  10. dmx_eb_finish_kernel  a wave per stream: Adler-32 from its blocks' sums, out_off / out_len,
//                            and the stream's header and trailer ORed into the words K3 zeroed
// No atomics but the ORs into the output: sums and minima are reductions, so nothing depends on the
// order in which workgroups run.
//
// Against preset dictionaries (dmx_encode_batch_dict_async) it is the same encode (eb_run): the plan
// with the dictionary's verdict (a dmx_ebd; the plain batch passes the empty one), K3 and the finish
// with the stream's own header width (DB), and a history.  The bytes of stream k are the single
// encode's for buffer k with opts->dict = its dictionary, so block 0 of a stream searches its
// dictionary's last min(len, sw) bytes, block j >= 1 searches block j - 1 of its own stream, and no
// block ever searches the table entry before it when that belongs to another stream.  Chain slots:
// [0, ndicts) the dictionaries, each sorted once per call however many streams share it; ndicts + b
// table entry b.
//   dmx_dict_adler_kernel        the DICTIDs (DMX_F_FDICT), a kernel of the call: the dictionaries
//                                may change between two replays of a graph
//   dmx_ebd_chain_kernel         chain_block, the source from the table or d_dicts
//   dmx_ebd_hist_kernel<6|7|8>   hist_search as a loop: a workgroup walks a contiguous range of
//                                table entries and keeps a dictionary's staged history, S and
//                                bucket ends in LDS while the next entry's history is the same slot
//   K0 with uni_ok 0, K1 = match_block<true, 3, false, true>
#include "dmx_encode_batch.h"

#define EB_WG 256   // threads per workgroup of the plan: one stream or table entry each
static_assert(DMX_EB_STILE == EB_WG, "a scan tile is a workgroup");
static_assert(DMX_EB_STHREADS <= 1024, "one workgroup scans the tile sums");
static_assert(sizeof(dmx_estream) == 16 && sizeof(dmx_eresult) == 32 && sizeof(dmx_ebatch_status) == 32, "ABI");
static_assert(sizeof(dmx_bblk) == 16 && sizeof(dmx_eb_head) == 64 && sizeof(dmx_eb_tile) == 24, "plan records");

// The plan's scratch: [head (256 B) | tile sums | starts (streams + 1)], every part 256-byte aligned
static inline uint64_t eb_a256(uint64_t x) { return (x + 255) & ~255ull; }
static inline uint64_t eb_tiles_of(uint64_t nstreams) { return (nstreams + DMX_EB_STILE - 1) / DMX_EB_STILE; }
static inline uint64_t eb_off_starts(uint64_t cap_streams) { return 256 + eb_a256((eb_tiles_of(cap_streams) + 1) * sizeof(dmx_eb_tile)); }
static inline uint64_t eb_plan_bytes(uint64_t cap_streams) { return eb_off_starts(cap_streams) + eb_a256((cap_streams + 1) * 8); }

// Inclusive-to-exclusive scan of v over the workgroup with op (associative, ident its neutral
// element), in LDS: returns op over the threads before this one, *total = over all.
template <typename T, typename Op>
__device__ static inline T eb_scan(T v, T ident, T* sh, Op op, T* total) {
    const uint32_t t = threadIdx.x, n = blockDim.x;
    __syncthreads();   // (sh may still be read from the call before)
    sh[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < n; d <<= 1) {
        const T x = t >= d ? sh[t - d] : ident;
        __syncthreads();
        sh[t] = op(x, sh[t]);
        __syncthreads();
    }
    *total = sh[n - 1];
    return t ? sh[t - 1] : ident;
}
struct EbSat { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return dmx_eb_sat(a, b); } };
struct EbAdd { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct EbMin { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };
// the workgroup's sums of a tile record; *before = the blocks of the threads before this one
__device__ static inline dmx_eb_tile eb_wg_sums(const dmx_eb_tile& v, uint64_t* sh, uint64_t* before) {
    dmx_eb_tile t;
    *before = eb_scan<uint64_t>(v.blocks, 0, sh, EbSat(), &t.blocks);
    eb_scan<uint64_t>(v.bytes, 0, sh, EbSat(), &t.bytes);
    eb_scan<uint32_t>(v.nfailed, 0, reinterpret_cast<uint32_t*>(sh), EbAdd(), &t.nfailed);
    eb_scan<uint32_t>(v.first_bad, DMX_EB_NOBAD, reinterpret_cast<uint32_t*>(sh), EbMin(), &t.first_bad);
    return t;
}

__global__ __launch_bounds__(EB_WG) void dmx_eb_count_kernel(const dmx_estream* __restrict__ st, uint32_t nstreams,
                                                             uint64_t in_bytes, uint32_t sw, const dmx_ebd d,
                                                             dmx_eb_tile* __restrict__ tiles) {
    __shared__ uint64_t sh[EB_WG];
    const uint64_t k = (uint64_t)blockIdx.x * DMX_EB_STILE + threadIdx.x;
    const dmx_eb_tile v = k < nstreams ? dmx_ebd_stream_sums(st, (uint32_t)k, in_bytes, sw, d) : dmx_eb_tile_zero();
    uint64_t before;
    const dmx_eb_tile t = eb_wg_sums(v, sh, &before);
    if (threadIdx.x == 0) tiles[blockIdx.x] = t;
}

__global__ __launch_bounds__(DMX_EB_STHREADS) void dmx_eb_plan_scan_kernel(dmx_eb_tile* __restrict__ tiles, uint32_t ntiles,
                                                                      uint32_t max_blocks, dmx_eb_head* __restrict__ head) {
    __shared__ uint64_t sh[DMX_EB_STHREADS];
    const uint32_t t = threadIdx.x;
    const dmx_eb_tile mine = dmx_eb_chunk_sum(tiles, ntiles, DMX_EB_STHREADS, t);
    uint64_t before;
    const dmx_eb_tile total = eb_wg_sums(mine, sh, &before);
    dmx_eb_chunk_apply(tiles, ntiles, DMX_EB_STHREADS, t, before);
    if (t == 0) dmx_eb_decide(head, total, max_blocks);
}

__global__ __launch_bounds__(EB_WG) void dmx_eb_starts_kernel(const dmx_estream* __restrict__ st, uint32_t nstreams,
                                                              uint64_t in_bytes, uint32_t sw, const dmx_ebd d,
                                                              const dmx_eb_tile* __restrict__ tiles,
                                                              uint64_t* __restrict__ starts, dmx_eresult* __restrict__ res) {
    __shared__ uint64_t sh[EB_WG];
    const uint64_t k = (uint64_t)blockIdx.x * DMX_EB_STILE + threadIdx.x;
    const uint64_t c = k < nstreams ? dmx_ebd_count(st, (uint32_t)k, in_bytes, sw, d) : 0u;
    uint64_t tot;
    const uint64_t before = dmx_eb_sat(tiles[blockIdx.x].blocks, eb_scan<uint64_t>(c, 0, sh, EbSat(), &tot));
    if (k < nstreams) dmx_ebd_start(st, (uint32_t)k, nstreams, in_bytes, sw, d, before, starts, res);
}

__global__ __launch_bounds__(EB_WG) void dmx_eb_table_kernel(const dmx_estream* __restrict__ st,
                                                             const uint64_t* __restrict__ starts, uint32_t nstreams,
                                                             const dmx_eb_head* __restrict__ head, uint32_t sw,
                                                             const dmx_ebd d, uint32_t max_blocks,
                                                             dmx_bblk* __restrict__ tab, dmx_blkinfo* __restrict__ info) {
    const uint64_t b = (uint64_t)blockIdx.x * EB_WG + threadIdx.x;
    if (b >= max_blocks) return;
    const dmx_bblk e = dmx_ebd_entry(st, starts, nstreams, head, sw, d, (uint32_t)b);
    tab[b] = e;
    // the block record before K0 / K1: a void entry and an empty stream's block are complete here
    // (prestored 1: K1 and K2 leave them alone) -- the empty block is the empty input's fixed
    // block, BFINAL / BTYPE 01 and the end-of-block code, 10 bits
    dmx_blkinfo bi;
    memset(&bi, 0, sizeof(bi));
    bi.nsub = 1;
    if (e.len & DMX_BB_VOID) bi.prestored = 1;
    else if (!(e.len & DMX_BB_LEN)) { bi.prestored = 1; bi.btype = 1; bi.hdr_bits = 3; bi.body_bits = 7; }
    info[b] = bi;
}

// ---- K0 / K1 / K4: the batch instantiations (the table instead of b * sw) ----
__global__ __launch_bounds__(SCT) void dmx_eb_store_check_kernel(const uint8_t* __restrict__ in, uint32_t sw,
                                                                 dmx_blkinfo* __restrict__ info, uint32_t* __restrict__ tok_g,
                                                                 uint32_t* __restrict__ hist_g, uint32_t flags,
                                                                 const dmx_bblk* __restrict__ tab) {
    // out_cap 0: no speculative copy (its offsets are b * (sw + 5)); a noise block is prestored 1
    (void)store_check_block<false, true>(in, 0, sw, info, tok_g, hist_g, 1u, flags, nullptr, 0, tab);
}

struct EbMatchArgs {
    const uint8_t* in;
    uint32_t sw;
    int32_t max_chain;
    uint32_t mflags;
    uint16_t* dist_g;
    uint32_t* tok_g;
    uint32_t* hist_g;
    dmx_blkinfo* info;
    uint32_t* nfallback;
    const dmx_bblk* tab;
};
template <int NBX>
__global__ __launch_bounds__(MT) void dmx_eb_match_kernel(const EbMatchArgs a) {
    match_block<false, NBX, false, true>(blockIdx.x, a.in, 0, a.sw, a.max_chain, a.mflags, a.dist_g, nullptr, a.tok_g,
                                         a.hist_g, a.info, nullptr, a.nfallback, a.tab);
}

__global__ __launch_bounds__(PT) void dmx_eb_pack_kernel(const uint8_t* __restrict__ in, uint32_t sw,
                                                         const uint32_t* __restrict__ tok_g, const uint32_t* __restrict__ codes_g,
                                                         const uint32_t* __restrict__ hdr_g, const dmx_blkinfo* __restrict__ info,
                                                         const dmx_subinfo* __restrict__ sub_g, uint32_t max_blocks,
                                                         uint32_t flags, uint32_t* __restrict__ out32,
                                                         dmx_result* __restrict__ res, const dmx_bblk* __restrict__ tab) {
    const uint32_t b = blockIdx.x;
    const uint32_t el = tab[b].len;
    if (el & DMX_BB_VOID) return;
    if (!(el & DMX_BB_LEN)) {   // an empty stream's block: BFINAL = 1, BTYPE = 01, end of block 0000000
        if (threadIdx.x == 0 && !res->status) gor_bits(out32, info[b].off_bits, 3u, 3);
        return;
    }
    pack_one<true>(b, in, sw, tok_g, codes_g, hdr_g, info, sub_g, max_blocks, flags, out32, res, nullptr, tab);
}

// ---- K0 and K1 with a history (dmx_encode_batch_dict_async) ----
__global__ __launch_bounds__(SCT) void dmx_ebd_store_check_kernel(const uint8_t* __restrict__ in, uint32_t sw,
                                                                  dmx_blkinfo* __restrict__ info, uint32_t* __restrict__ tok_g,
                                                                  uint32_t* __restrict__ hist_g, uint32_t flags,
                                                                  const dmx_bblk* __restrict__ tab) {
    // uni_ok 0, as the single dictionary encode passes it: a block of one repeated byte is parsed by K1,
    // whose history may hold a longer match than the closed form knows
    (void)store_check_block<false, true>(in, 0, sw, info, tok_g, hist_g, 0u, flags, nullptr, 0, tab);
}

struct EbdMatchArgs {
    EbMatchArgs m;
    const uint16_t* chs;   // offset so that entry b's own slot, ndicts + b, is the b + 1 match_block adds
};
__global__ __launch_bounds__(MT) void dmx_ebd_match_kernel(const EbdMatchArgs a) {
    match_block<true, 3, false, true>(blockIdx.x, a.m.in, 0, a.m.sw, a.m.max_chain, a.m.mflags, a.m.dist_g, a.chs, a.m.tok_g,
                                      a.m.hist_g, a.m.info, nullptr, a.m.nfallback, a.m.tab);
}

// ---- the chains: slot < ndicts sorts that dictionary's last min(len, sw) bytes, slot ndicts + b table
// entry b.  Void entries, empty blocks and records outside d_dict (no stream that names one has
// blocks) return at once.
__global__ __launch_bounds__(MT) void dmx_ebd_chain_kernel(const uint8_t* __restrict__ in, uint32_t sw,
                                                           const uint8_t* __restrict__ dict, const dmx_ebd d,
                                                           const dmx_bblk* __restrict__ tab,
                                                           uint16_t* __restrict__ chs, uint16_t* __restrict__ che,
                                                           uint32_t* __restrict__ nfallback) {
    __shared__ MatchLDS L;
    __shared__ uint64_t tp0[3];
    const uint32_t slot = blockIdx.x;
    const uint8_t* src;
    uint32_t len;
    if (slot < d.ndicts) {
        const dmx_bdict r = d.dicts[slot];
        if (!dmx_ebd_inside(r, d.dict_bytes)) return;
        len = r.len < sw ? (uint32_t)r.len : sw;
        src = dict + r.off + (r.len - len);
    } else {
        const dmx_bblk e = tab[slot - d.ndicts];
        if (e.len & DMX_BB_VOID) return;
        len = e.len & DMX_BB_LEN;
        src = in + e.off;
    }
    chain_block(L, tp0, src, len, slot, chs, che, nfallback, threadIdx.x);
}

// ---- the history search ----
struct EbdHistArgs {
    const uint8_t* in;
    uint32_t sw;
    int32_t max_chain;
    const uint8_t* dict;
    dmx_ebd d;
    const uint16_t* chs;
    const uint16_t* che;
    uint32_t* hb_g;
    const dmx_bblk* tab;
    uint32_t max_blocks;
    uint32_t resident;   // 1: keep a dictionary's staged history, S and ends while the next entry uses the same slot
};

// A workgroup walks table entries [w per, (w + 1) per), per = ceil(max_blocks / grid): the ranges
// follow from the launch alone, so no claim counter.  A first block's history is its dictionary's
// staged tail and slot, any other block's the sw bytes before it in d_in (block j - 1 of its own
// stream, which is full) and slot ndicts + b - 1.  Resident: an entry whose history is the
// dictionary slot staged by the entry before it stages only the block and the crossing bytes behind
// the history (a dictionary's bytes, S and ends do not change within a call).  With a grid of
// max_blocks workgroups (the simple form) every workgroup has one entry and stages everything.
template <int HG>
__global__ __launch_bounds__(MT) void dmx_ebd_hist_kernel(const EbdHistArgs a) {
    __shared__ HistLDS L;
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (a.max_blocks + gridDim.x - 1) / gridDim.x;
    const uint64_t b0 = (uint64_t)blockIdx.x * per;
    const uint32_t b1 = (uint32_t)(b0 + per < a.max_blocks ? b0 + per : a.max_blocks);
    uint32_t held = 0xFFFFFFFFu, held_hn = 0;   // the dictionary slot whose history L holds (uniform)
    for (uint32_t b = (uint32_t)(b0 < b1 ? b0 : b1); b < b1; b++) {
        const dmx_bblk e = a.tab[b];
        if ((e.len & DMX_BB_VOID) || !(e.len & DMX_BB_LEN)) continue;
        const uint32_t bn = e.len & DMX_BB_LEN;
        const uint8_t* cur = a.in + e.off;
        uint32_t* hb = a.hb_g + (uint64_t)b * DMX_BLK;
        const uint32_t nvalid = bn > 2 ? bn - 2 : 0;
        uint32_t hn, slot;
        const uint8_t* hs;
        if (e.len & DMX_BB_FIRST) {
            uint64_t doff = 0;
            hn = (e.len & DMX_BB_DICT) ? dmx_ebd_history(a.d, e.stream, a.sw, &doff, &slot) : 0u;
            hs = a.dict + doff;
        } else {
            hn = a.sw;
            hs = cur - a.sw;
            slot = a.d.ndicts + b - 1;
        }
        if (hn < 3) {   // no history entries
            for (uint32_t k = tid; k < nvalid; k += MT) hb[k] = 0;
            continue;
        }
        __syncthreads();   // (the entry before this one has finished reading L)
        const bool same = a.resident && (e.len & DMX_BB_FIRST) && slot == held && hn == held_hn;
        if (same) {   // the chunks from the one that holds the history's last byte to the search's reach
            const uint32_t c1 = (hn + MAXLEN + 64) / 16 + 1;
            stage_range(L.data, hn / 16, c1 < DATA_WORDS / 4 ? c1 : DATA_WORDS / 4, hs, hn, cur, bn, tid);
        } else {
            stage_bytes(L.data, DATA_WORDS, hs, hn, cur, bn, tid);
            const uint4* Sg = reinterpret_cast<const uint4*>(a.chs + (uint64_t)slot * DMX_BLK);
            const uint4* Eg = reinterpret_cast<const uint4*>(a.che + (uint64_t)slot * DMX_NBUCKET);
            for (uint32_t k = tid; k < (hn - 2 + 7) / 8; k += MT) reinterpret_cast<uint4*>(L.sp)[k] = Sg[k];
            for (uint32_t k = tid; k < DMX_NBUCKET / 8; k += MT) reinterpret_cast<uint4*>(L.ep)[k] = Eg[k];
        }
        if (a.resident) {   // the block and the slack behind it the search may read (bytes past bn never decide)
            const uint32_t c1 = (bn + 15) / 16 + 6;
            stage_range(L.cur, 0, c1 < (DMX_BLK / 4 + 80) / 4 ? c1 : (DMX_BLK / 4 + 80) / 4, cur, bn, nullptr, 0, tid);
        } else {
            stage_bytes(L.cur, DMX_BLK / 4 + 80, cur, bn, nullptr, 0, tid);
        }
        held = (e.len & DMX_BB_FIRST) ? slot : 0xFFFFFFFFu;
        held_hn = hn;
        __syncthreads();
        hist_search<HG>(L, a.chs + (uint64_t)(a.d.ndicts + b) * DMX_BLK, hn, bn, a.max_chain, hb, tid);
    }
}

// ---- K3 for a batch: the layout scan of dmx_scan_tile_kernel / dmx_scan_kernel / dmx_scan_apply_kernel /
// dmx_scan_apply1_kernel with the batch's container rule (their Mono, ScanTile and ScanSums) ----

// a block's own bits: blk_elem without a container
__device__ __forceinline__ Mono eb_own(const dmx_blkinfo& bi) {
    Mono e = {0, 0, 0};
    if (bi.btype == 0) { e.s = 1; e.a = 3; e.c = 32 + 8 * (uint64_t)bi.n; }
    else { e.c = bi.hdr_bits + bi.body_bits; }
    return e;
}
// and with the framing of its stream: x -> align8(x) + header bits in front of a first block,
// x -> align8(x) + trailer bits behind a last one
// DB (dmx_encode_batch_dict_async): the header's width is the stream's own -- under DMX_F_FDICT 48
// bits where it names a dictionary (DMX_BB_DICT), 16 where it has none; 48 = 16 mod 32
template <bool DB>
__device__ __forceinline__ uint32_t eb_hdr(uint32_t marks, uint32_t flags) {
    if constexpr (DB) return (marks & DMX_BB_DICT) ? hdr_bits(flags) : hdr_bits(flags & ~DMX_F_FDICT);
    else return hdr_bits(flags);
}
template <bool DB = false>
__device__ __forceinline__ Mono eb_elem(const dmx_blkinfo& bi, uint32_t marks, uint32_t flags) {
    Mono e = eb_own(bi);
    if (marks & DMX_BB_FIRST) { const Mono h = {1, 0, eb_hdr<DB>(marks, flags)}; e = mcompose(h, e); }
    if (marks & DMX_BB_LAST) { const Mono t = {1, 0, trl_bits(flags)}; e = mcompose(e, t); }
    return e;
}

template <bool DB>
__global__ __launch_bounds__(SCAN_TILE) void dmx_eb_scan_tile_kernel(dmx_blkinfo* __restrict__ info,
                                                                    const dmx_bblk* __restrict__ tab, uint32_t max_blocks,
                                                                    uint32_t flags, ScanTile* __restrict__ tiles) {
    __shared__ Mono wtot[SCAN_TILE / 64];
    __shared__ uint64_t red[SCAN_TILE / 64][4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t b = blockIdx.x * SCAN_TILE + tid;
    Mono e = {0, 0, 0};
    uint64_t nt = 0, ns = 0, nf = 0, nr = 0;
    const uint32_t marks = b < max_blocks ? tab[b].len : DMX_BB_VOID;
    const bool real = !(marks & DMX_BB_VOID);
    if (real) {
        const dmx_blkinfo bi = info[b];
        e = eb_elem<DB>(bi, marks, flags);
        nt = bi.ntok;
        ns = bi.btype == 0;
        nf = bi.btype == 1;
        nr = 1;
    }
    const Mono x = mono_wave_scan(e, lane);
    const Mono before = mshfl_up(x, 1);
    if (lane == 63) wtot[wave] = x;
    nt = wave_sum_u64(nt);
    ns = wave_sum_u64(ns);
    nf = wave_sum_u64(nf);
    nr = wave_sum_u64(nr);
    if (lane == 0) { red[wave][0] = nt; red[wave][1] = ns; red[wave][2] = nf; red[wave][3] = nr; }
    __syncthreads();
    Mono pre = {0, 0, 0};
    for (uint32_t w = 0; w < wave; w++) pre = mcompose(pre, wtot[w]);
    if (lane) pre = mcompose(pre, before);
    if (real) {   // tile-local exclusive prefix, finished by eb_apply_block
        info[b].off_bits = pre.c;
        info[b].len_bits = ((uint64_t)pre.s << 32) | pre.a;
    }
    if (tid == 0) {
        Mono agg = {0, 0, 0};
        uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
        for (int w = 0; w < SCAN_TILE / 64; w++) {
            agg = mcompose(agg, wtot[w]);
            t0 += red[w][0]; t1 += red[w][1]; t2 += red[w][2]; t3 += red[w][3];
        }
        ScanTile& T = tiles[blockIdx.x];
        T.a = agg.a; T.c = agg.c; T.s = agg.s;
        T.adl_s1 = 0; T.adl_s2 = 0; T.ntok = t0; T.nsto = t1; T.nfix = t2;
        T.kinds = t3;   // (ScanSums::k0: the tile's real blocks, at most SCAN_TILE)
    }
}

// Where the batch ends: every stream ends on a byte boundary, so the composed layout applied to
// bit 0 is 8 x out_len.  The status: the plan's -E_SZ (more blocks than max_blocks; nothing was
// encoded), else stream_extent's rule for out_cap.
struct EbExtent {
    uint64_t T, out_len;
    int32_t status;
};
__device__ __forceinline__ EbExtent eb_extent(const Mono& total, const dmx_eb_head* __restrict__ head, uint64_t out_cap) {
    EbExtent x;
    x.T = mapply(total, 0);
    x.out_len = x.T / 8;
    x.status = head->status ? head->status : (((x.out_len + 3) & ~3ull) > out_cap) ? -(int32_t)E_SZ : 0;
    return x;
}
// One thread, once per batch: dmx_result (the totals), the fallback counters as scan_publish
// leaves them, and the call's record.
__device__ __forceinline__ void eb_publish(dmx_result* __restrict__ res, uint32_t* __restrict__ nfallback,
                                           dmx_ebatch_status* __restrict__ rec, const dmx_eb_head* __restrict__ head,
                                           const EbExtent& x, const ScanSums& sums) {
    res->out_len = x.out_len;
    res->end_bits = x.T;
    res->n = head->in_len;
    res->ntokens = sums.ntok;
    res->adler = 0;
    res->status = x.status;
    res->nblocks = sums.k0;
    res->nstored = sums.nsto;
    res->nfixed = sums.nfix;
    res->ndynamic = sums.k0 - sums.nsto - sums.nfix;
    res->nsortfallback = nfallback[0];
    nfallback[1] += nfallback[0];
    res->nsortfallback_total = nfallback[1];
    nfallback[0] = 0;
    dmx_ebatch_status r;
    r.status = x.status;
    r.nfailed = head->nfailed;
    r.first_bad = head->first_bad;
    r.nblocks = head->nblocks > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)head->nblocks;
    r.out_len = x.out_len;
    r.in_len = head->in_len;
    *rec = r;
}

// Block b's place from its tile's prefix `tp` and the tile-local prefix parked in its record; then
// every word it shares -- with a neighbour, or with its stream's header and trailer, which the
// finish kernel ORs in -- is zeroed for K4's ORs.  `write` false (-E_SZ for out_cap): the places
// only, which the finish kernel reports; no byte of the output is touched.
template <bool DB>
__device__ __forceinline__ void eb_apply_block(dmx_blkinfo* __restrict__ info, const dmx_bblk* __restrict__ tab, uint32_t b,
                                               uint32_t flags, const Mono& tp, uint32_t* __restrict__ out32, bool write) {
    const uint32_t marks = tab[b].len;
    if (marks & DMX_BB_VOID) return;
    const dmx_blkinfo bi = info[b];
    Mono lp;
    lp.c = bi.off_bits; lp.s = (uint32_t)(bi.len_bits >> 32); lp.a = bi.len_bits & 0xFFFFFFFFu;
    const uint64_t x = mapply(mcompose(tp, lp), 0);   // the end of the block before
    const uint64_t hs = align8(x);                    // a first block: its stream begins here
    const uint64_t o = (marks & DMX_BB_FIRST) ? hs + eb_hdr<DB>(marks, flags) : x;
    const uint64_t l = mapply(eb_own(bi), o) - o;
    info[b].off_bits = o;
    info[b].len_bits = l;
    if (!write) return;
    for (uint64_t w = ((marks & DMX_BB_FIRST) ? hs : o) >> 5; w <= (o >> 5); w++) out32[w] = 0;
    const uint64_t te = (marks & DMX_BB_LAST) ? align8(o + l) + trl_bits(flags) : o + l;
    for (uint64_t w = (o + l - 1) >> 5; w <= ((te - 1) >> 5); w++) out32[w] = 0;
}

__global__ __launch_bounds__(ST) void dmx_eb_scan_kernel(ScanTile* __restrict__ tiles, uint32_t max_blocks,
                                                         uint64_t out_cap, dmx_result* __restrict__ res,
                                                         uint32_t* __restrict__ nfallback,
                                                         const dmx_eb_head* __restrict__ head,
                                                         dmx_ebatch_status* __restrict__ rec) {
    __shared__ Mono wtot[ST / 64];
    __shared__ Mono carry_s;
    __shared__ ScanSums red[ST / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ntile = (max_blocks + SCAN_TILE - 1) / SCAN_TILE;
    const uint32_t C = (ntile + ST - 1) / ST;
    const uint32_t t0 = tid * C < ntile ? tid * C : ntile, t1 = t0 + C < ntile ? t0 + C : ntile;
    Mono agg = {0, 0, 0};
    ScanSums sums = {};
    for (uint32_t t = t0; t < t1; t++) {
        const ScanTile T = tiles[t];
        agg = mcompose(agg, tile_mono(T));
        sums.add(T);
    }
    const Mono x = mono_wave_scan(agg, lane);
    if (lane == 63) wtot[wave] = x;
    sums.wave_reduce();
    if (lane == 0) red[wave] = sums;
    __syncthreads();
    if (tid == 0) {   // exclusive prefix over waves
        Mono acc = {0, 0, 0};
        for (int w = 0; w < ST / 64; w++) {
            const Mono t = wtot[w];
            wtot[w] = acc;
            acc = mcompose(acc, t);
        }
        carry_s = acc;
    }
    __syncthreads();
    {
        const Mono before = mshfl_up(x, 1);
        Mono pre = (lane == 0) ? wtot[wave] : mcompose(wtot[wave], before);
        for (uint32_t t = t0; t < t1; t++) {
            tiles[t].ps = pre.s; tiles[t].pa = pre.a; tiles[t].pc = pre.c;
            pre = mcompose(pre, tile_mono(tiles[t]));
        }
    }
    if (tid == 0) eb_publish(res, nfallback, rec, head, eb_extent(carry_s, head, out_cap), ScanSums::total(red, ST / 64));
}

template <bool DB>
__global__ __launch_bounds__(SCAN_TILE) void dmx_eb_apply_kernel(dmx_blkinfo* __restrict__ info,
                                                                const dmx_bblk* __restrict__ tab, uint32_t max_blocks,
                                                                uint32_t flags, const ScanTile* __restrict__ tiles,
                                                                uint32_t* __restrict__ out32,
                                                                const dmx_result* __restrict__ res) {
    const uint32_t b = blockIdx.x * SCAN_TILE + threadIdx.x;
    if (b >= max_blocks) return;
    const ScanTile& T = tiles[blockIdx.x];
    Mono tp;   // the prefix dmx_eb_scan_kernel left
    tp.s = (uint32_t)T.ps; tp.a = T.pa; tp.c = T.pc;
    eb_apply_block<DB>(info, tab, b, flags, tp, out32, res->status == 0);
}

// up to SA1_MAXT tiles: a workgroup per tile composes the tile aggregates itself (dmx_scan_apply1_kernel)
template <bool DB>
__global__ __launch_bounds__(SCAN_TILE) void dmx_eb_scan_apply1_kernel(dmx_blkinfo* __restrict__ info,
                                                                      const dmx_bblk* __restrict__ tab, uint32_t max_blocks,
                                                                      uint32_t flags, uint64_t out_cap,
                                                                      const ScanTile* __restrict__ tiles,
                                                                      uint32_t* __restrict__ out32, dmx_result* __restrict__ res,
                                                                      uint32_t* __restrict__ nfallback,
                                                                      const dmx_eb_head* __restrict__ head,
                                                                      dmx_ebatch_status* __restrict__ rec) {
    __shared__ Mono wt[SCAN_TILE / 64];
    __shared__ Mono s_pre;
    __shared__ ScanSums red[SCAN_TILE / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t ntile = (max_blocks + SCAN_TILE - 1) / SCAN_TILE, tt = blockIdx.x;
    const bool lastwg = tt + 1 == ntile;
    const uint32_t C = (ntile + SCAN_TILE - 1) / SCAN_TILE;
    const uint32_t t0 = tid * C < ntile ? tid * C : ntile, t1 = t0 + C < ntile ? t0 + C : ntile;
    Mono agg = {0, 0, 0}, part = {0, 0, 0};
    bool mine = false;
    ScanSums sums = {};
    for (uint32_t u = t0; u < t1; u++) {
        const ScanTile T = tiles[u];
        if (u == tt) { part = agg; mine = true; }
        agg = mcompose(agg, tile_mono(T));
        if (lastwg) sums.add(T);
    }
    const Mono x = mono_wave_scan(agg, lane);
    const Mono before = mshfl_up(x, 1);
    if (lane == 63) wt[wave] = x;
    if (lastwg) {
        sums.wave_reduce();
        if (lane == 0) red[wave] = sums;
    }
    __syncthreads();
    Mono tot = {0, 0, 0}, wpre = {0, 0, 0};
#pragma unroll
    for (int w = 0; w < SCAN_TILE / 64; w++) {
        if (w == (int)wave) wpre = tot;
        tot = mcompose(tot, wt[w]);
    }
    if (mine) s_pre = mcompose(lane ? mcompose(wpre, before) : wpre, part);
    const EbExtent ext = eb_extent(tot, head, out_cap);   // (every workgroup: nothing is written past out_cap)
    if (lastwg && tid == 0) eb_publish(res, nfallback, rec, head, ext, ScanSums::total(red, SCAN_TILE / 64));
    __syncthreads();   // (s_pre)
    const uint32_t b = tt * SCAN_TILE + tid;
    if (b < max_blocks) eb_apply_block<DB>(info, tab, b, flags, s_pre, out32, ext.status == 0);
}

// ---- the streams' CRC-32s (DMX_F_GZIP): dmx_crc_batch_kernel with an entry's geometry read from the
// stream's descriptor; the value goes to the stream's record (check), which the finish kernel
// frames.  A stream that is -E_RANGE is one piece without data and keeps check 0.
__global__ __launch_bounds__(CRC_T) void dmx_eb_crc_kernel(const uint8_t* __restrict__ in, uint64_t n,
                                                           const dmx_estream* __restrict__ streams, uint32_t nstreams,
                                                           dmx_eresult* __restrict__ res) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[CRC_NS * 256];
    __shared__ __attribute__((aligned(16))) uint32_t stage[CRC_T * CRC_ROW];
    __shared__ uint32_t wred[CRC_T / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < CRC_NS * 256; i += CRC_T) tab[i] = (&g_crc.t[0][0])[i];
    const uint32_t klane = g_crc.lane[tid];
    constexpr uint32_t XS = crc_xspan();
    auto geom = [&](uint32_t k, uint64_t j, const uint8_t*& base, uint32_t& lo, uint32_t& hi, uint64_t& np, uint64_t& len) {
        const dmx_estream s = streams[k];
        const bool ok = dmx_eb_valid(s, n);
        len = s.in_len;
        uint64_t elo = 0, ehi = 0;   // the whole entry from its aligned base
        base = in;
        if (ok && len) {
            const uint8_t* p = in + s.in_off;
            elo = reinterpret_cast<uintptr_t>(p) & 15;
            base = p - elo;
            ehi = elo + len;
        }
        np = ehi > CRC_S ? (ehi + CRC_S - 1) / CRC_S : 1u;
        base += j * CRC_S;
        lo = j ? 0u : (uint32_t)elo;
        const uint64_t left = ehi - j * CRC_S;   // (j < np: ehi > j CRC_S, or both are 0)
        hi = left < CRC_S ? (uint32_t)left : (uint32_t)CRC_S;
        return ok;
    };
    uint4 v[CRC_Q];
    auto load = [&](uint32_t k, uint64_t j) {
        const uint8_t* base;
        uint32_t lo, hi;
        uint64_t np, len;
        geom(k, j, base, lo, hi, np, len);
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++) v[i] = crc_load16_blk(base, 16u * (tid + CRC_T * i), lo, hi);
    };
    uint32_t k = blockIdx.x, acc = 0;   // acc (thread 0): the raw remainder of the entry's pieces so far
    uint64_t j = 0;
    if (k < nstreams) load(k, 0);
    while (k < nstreams) {
        const uint8_t* base;
        uint32_t lo, hi;
        uint64_t np, len;
        const bool ok = geom(k, j, base, lo, hi, np, len);
        const bool last = j + 1 == np;
        uint32_t unshift = 0, affine = 0;   // x^-(8 Z) and the affine term, by wave 0 while the loads fly
        if (last && tid < 64) {
            const uint32_t Z = (CRC_S - hi) & (CRC_S - 1u);
            const uint64_t l = ok ? len : 0u;
            unshift = dmx_gf2_mulmod(g_crc_unshift.lo[Z & 255u], g_crc_unshift.hi[Z >> 8]);
            affine = dmx_gf2_mulmod(g_crc_shift.lo[l & 255u], g_crc_shift.hi[(l >> 8) & 255u]);
            if (l >> 16) affine = dmx_gf2_mulmod(affine, dmx_gf2_xpow(l >> 16, 19));   // x^(8 65 536 (l >> 16))
            affine ^= 0xFFFFFFFFu;
        }
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++) {
            const uint32_t q = tid + CRC_T * i, sl = q / (CRC_L / 16);
            if (sl * CRC_L < hi)   // (a slice behind the data is never read)
                *reinterpret_cast<uint4*>(&stage[sl * CRC_ROW + 4 * (q % (CRC_L / 16))]) = v[i];
        }
        __syncthreads();   // (and the tables, the first time)
        const uint32_t kn = last ? k + gridDim.x : k;
        const uint64_t jn = last ? 0u : j + 1;
        if (kn < nstreams) load(kn, jn);   // the next piece's loads fly during this one's lookups
        uint32_t c = 0;
        if (tid * CRC_L < hi) {
            const uint4* p = reinterpret_cast<const uint4*>(&stage[tid * CRC_ROW]);
#pragma unroll
            for (uint32_t s = 0; s < CRC_L / 16; s++) {
                const uint4 d = p[s];
                CRC_STEP16(c, d, tab);
            }
        }
        uint32_t r = dmx_gf2_mulmod(c, klane);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) r ^= __shfl_xor(r, o);
        if ((tid & 63) == 0) wred[tid >> 6] = r;
        __syncthreads();   // (also: every lane has read its slice before the next staging)
        if (tid == 0) {
            uint32_t t = 0;
#pragma unroll
            for (uint32_t w = 0; w < CRC_T / 64; w++) t ^= wred[w];
            acc = j ? dmx_gf2_mulmod(acc, XS) ^ t : t;
            if (last && ok) res[k].check = len ? dmx_gf2_mulmod(acc, unshift) ^ affine : 0u;
        }
        k = kn;
        j = jn;
    }
}

// ---- the per-stream finish: a wave per stream, lanes over its blocks ----
// Adler-32 from the blocks' sums: block j of a stream of len bytes ends at e_j = j sw + n_j of its
// own stream, so its bytes weigh adl_w + (len - e_j) adl_s in the second sum -- the weight is the
// bytes behind the block in its stream, not in the batch.  Then the stream's place (out_off,
// out_len, from its first and last block's places), its check value, and -- unless the call is
// -E_SZ -- its header and trailer ORed into the words eb_apply_block zeroed.
// DB (dmx_encode_batch_dict_async): a stream's verdict and header come from its dictionary (d) -- under
// DMX_F_FDICT 78 BB and the DICTID dictid[index] where it names one, 78 9C where it has none.
#define EB_FIN_WAVES 4
template <bool DB>
__device__ __forceinline__ void eb_finish(const dmx_estream* __restrict__ st, const uint64_t* __restrict__ starts,
                                          uint32_t nstreams, uint64_t in_bytes, uint32_t sw, const uint32_t flags0,
                                          const dmx_blkinfo* __restrict__ info, const dmx_eb_head* __restrict__ head,
                                          const dmx_result* __restrict__ res, uint32_t* __restrict__ out32,
                                          dmx_eresult* __restrict__ results, const dmx_ebd* d = nullptr,
                                          const uint32_t* __restrict__ dictid = nullptr,
                                          const dmx_bblk* __restrict__ tab = nullptr) {
    uint32_t flags = flags0;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t k = (uint64_t)blockIdx.x * EB_FIN_WAVES + (threadIdx.x >> 6);
    if (k >= nstreams) return;
    if (head->status) return;   // more blocks than max_blocks: nothing was laid out (the records hold zeros)
    const dmx_estream s = st[k];
    bool ok;
    uint32_t di = DMX_BATCH_NODICT;   // DB: the dictionary the stream's header names
    if constexpr (DB) {
        ok = dmx_ebd_status(st, (uint32_t)k, in_bytes, sw, *d) == 0;
        if (ok && (flags & DMX_F_FDICT)) di = dmx_ebd_index(*d, (uint32_t)k);
        if (di == DMX_BATCH_NODICT) flags &= ~DMX_F_FDICT;
    } else {
        ok = dmx_eb_valid(s, in_bytes);
    }
    const uint64_t b0 = starts[k], nb = ok ? starts[k + 1] - b0 : 0u;
    const uint64_t H = hdr_bits(flags), Tr = trl_bits(flags);
    uint64_t s1 = 0, s2 = 0;
    for (uint64_t j = lane; j < nb; j += 64) {
        const dmx_blkinfo bi = info[b0 + j];
        const uint64_t a = bi.adl_s % ADL_MOD;
        s1 += a;
        s2 += (bi.adl_w % ADL_MOD + ((s.in_len - (j * sw + bi.n)) % ADL_MOD) * a) % ADL_MOD;
    }
    s1 = wave_sum_u64(s1) % ADL_MOD;
    s2 = wave_sum_u64(s2) % ADL_MOD;
    if (lane) return;
    uint64_t o0, e0, end;   // the stream's first bit, the byte boundary behind its last block, its end
    if (nb) {
        const dmx_blkinfo last = info[b0 + nb - 1];
        o0 = info[b0].off_bits - H;
        e0 = align8(last.off_bits + last.len_bits);
        end = e0 + Tr;
    } else {   // -E_RANGE: no bytes, where the next stream begins
        if constexpr (DB) {   // (block b0 is the next stream's first: that header has its own width)
            o0 = b0 < head->nblocks ? info[b0].off_bits - eb_hdr<true>(tab[b0].len, flags0) : res->end_bits;
        } else {
            o0 = b0 < head->nblocks ? info[b0].off_bits - H : res->end_bits;
        }
        e0 = end = o0;
    }
    const uint32_t adler = (uint32_t)((((s.in_len % ADL_MOD + s2) % ADL_MOD) << 16) | ((1 + s1) % ADL_MOD));
    const uint32_t check = !nb || !(flags & DMX_F_TRAILER) ? 0u : (flags & DMX_F_GZIP) ? results[k].check : adler;
    results[k].out_off = o0 / 8;
    results[k].out_len = (end - o0) / 8;
    results[k].check = check;
    if (res->status || !nb) return;
    if (flags & DMX_F_HEADER) {
        if (flags & DMX_F_GZIP) {   // 1F 8B 08 00, mtime 0, XFL 0, OS 255 (put_header's bytes, at any byte offset)
            gor_bits(out32, o0, 0x00088B1Fu, 32);
            gor_bits(out32, o0 + 64, 0xFF00u, 16);
        } else if (DB && (flags & DMX_F_FDICT)) {   // 78 BB, the DICTID most significant byte first (put_header's bytes)
            const uint32_t id = dictid[di];
            gor_bits(out32, o0, 0xBB78u | ((id >> 24) << 16) | (((id >> 16) & 0xFFu) << 24), 32);
            gor_bits(out32, o0 + 32, ((id >> 8) & 0xFFu) | ((id & 0xFFu) << 8), 16);
        } else {
            gor_bits(out32, o0, 0x9C78u, 16);
        }
    }
    if ((flags & DMX_F_TRAILER) && (flags & DMX_F_GZIP)) {
        gor_bits(out32, e0, check, 32);
        gor_bits(out32, e0 + 32, (uint32_t)s.in_len, 32);
    } else if (flags & DMX_F_TRAILER) {
        const uint32_t be = (check >> 24) | ((check >> 8) & 0xFF00u) | ((check << 8) & 0xFF0000u) | (check << 24);
        gor_bits(out32, e0, be, 32);
    }
}
__global__ __launch_bounds__(64 * EB_FIN_WAVES) void dmx_eb_finish_kernel(const dmx_estream* __restrict__ st,
                                                                          const uint64_t* __restrict__ starts,
                                                                          uint32_t nstreams, uint64_t in_bytes, uint32_t sw,
                                                                          uint32_t flags, const dmx_blkinfo* __restrict__ info,
                                                                          const dmx_eb_head* __restrict__ head,
                                                                          const dmx_result* __restrict__ res,
                                                                          uint32_t* __restrict__ out32,
                                                                          dmx_eresult* __restrict__ results) {
    eb_finish<false>(st, starts, nstreams, in_bytes, sw, flags, info, head, res, out32, results);
}
__global__ __launch_bounds__(64 * EB_FIN_WAVES) void dmx_ebd_finish_kernel(const dmx_estream* __restrict__ st,
                                                                           const uint64_t* __restrict__ starts,
                                                                           uint32_t nstreams, uint64_t in_bytes, uint32_t sw,
                                                                           uint32_t flags, const dmx_blkinfo* __restrict__ info,
                                                                           const dmx_eb_head* __restrict__ head,
                                                                           const dmx_result* __restrict__ res,
                                                                           uint32_t* __restrict__ out32,
                                                                           dmx_eresult* __restrict__ results, const dmx_ebd d,
                                                                           const uint32_t* __restrict__ dictid,
                                                                           const dmx_bblk* __restrict__ tab) {
    eb_finish<true>(st, starts, nstreams, in_bytes, sw, flags, info, head, res, out32, results, &d, dictid, tab);
}

// ---- host ----
static uint32_t eb_sw(int32_t sw) { return (sw <= 0 || sw > DMX_BLK) ? (uint32_t)DMX_BLK : (uint32_t)sw; }

extern "C" uint32_t dmx_encode_batch_blocks(uint64_t total_in, uint32_t nstreams, int32_t sw) {
    return dmx_eb_blocks_bound(total_in, nstreams, eb_sw(sw));
}

// Stream k needs at most align4(dmx_max_compressed_flags(len_k, sw, flags)) <= len_k + 5 ceil(len_k / sw)
// + 27 + 3 (+ 12 under DMX_F_GZIP); the sum over the streams is below this, which saturates.
extern "C" uint64_t dmx_encode_batch_bound(uint64_t total_in, uint32_t nstreams, int32_t sw, uint32_t flags) {
    const uint64_t blocks = dmx_eb_sat(total_in / eb_sw(sw), nstreams);
    const uint64_t per = 30u + ((flags & DMX_F_GZIP) ? 12u : 0u);
    uint64_t r = dmx_eb_sat(total_in, blocks > ~0ull / 5 ? ~0ull : 5 * blocks);
    r = dmx_eb_sat(r, per * nstreams);
    r = dmx_eb_sat(r, 16);
    return r > ~0ull - 3 ? ~0ull & ~3ull : (r + 3) & ~3ull;
}
// ... with the DICTID's 4 bytes per stream under DMX_F_FDICT
extern "C" uint64_t dmx_encode_batch_dict_bound(uint64_t total_in, uint32_t nstreams, int32_t sw, uint32_t flags) {
    const uint64_t r = dmx_encode_batch_bound(total_in, nstreams, sw, flags & ~DMX_F_GZIP);
    if (!(flags & DMX_F_FDICT)) return r;
    const uint64_t x = dmx_eb_sat(r, 4ull * nstreams);
    return x > ~0ull - 3 ? ~0ull & ~3ull : x;
}

// the history loop's workgroups: one per compute unit (146 KB of LDS each), at most one per table entry
extern "C" void dmx_encode_batch_dict_geometry(uint32_t* hist_grid) {
    if (hist_grid) *hist_grid = crc_device_ncu();
}

static int eb_flags_ok(uint32_t f) {
    if (f & (DMX_F_DICT | DMX_F_SPLIT | DMX_F_BGZF | DMX_F_FDICT)) return 0;
    if (!(f & DMX_F_FINAL)) return 0;
    if (!(f & DMX_F_HEADER) != !(f & DMX_F_TRAILER)) return 0;
    if ((f & DMX_F_GZIP) && !(f & DMX_F_HEADER)) return 0;
    return 1;
}
static int ebd_flags_ok(uint32_t f) {
    if (!(f & DMX_F_DICT)) return 0;
    if (f & (DMX_F_SPLIT | DMX_F_BGZF | DMX_F_GZIP)) return 0;
    if (!(f & DMX_F_FINAL)) return 0;
    if (!(f & DMX_F_HEADER) != !(f & DMX_F_TRAILER)) return 0;
    if ((f & DMX_F_FDICT) && !(f & DMX_F_HEADER)) return 0;
    return 1;
}

extern "C" int dmx_ctx_reserve_batch(dmx_ctx* c, uint32_t max_blocks, uint32_t max_streams, int32_t sw, uint32_t flags) {
    if (!c) return -(int)E_INVAL;
    if (sw == 0) sw = DMX_BLK;
    if (sw < 1 || sw > DMX_BLK) return -(int)E_RANGE;
    if (max_blocks > 0x7FFFFFFFu || max_streams > 0x7FFFFFFFu) return -(int)E_RANGE;
    if (flags & (DMX_F_DICT | DMX_F_SPLIT | DMX_F_BGZF | DMX_F_FDICT)) return -(int)E_INVAL;
    if (max_blocks <= c->cap_blocks && max_blocks <= c->cap_btab && c->bplan && max_streams <= c->cap_bstreams)
        return 0;   // nothing to do: no synchronisation
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipDeviceSynchronize());
    if (max_blocks > c->cap_blocks) {
        const int r = ctx_reserve(c, max_blocks);
        if (r) return r;
    }
    if (max_blocks > c->cap_btab || !c->btab) {
        if (c->btab) (void)hipFree(c->btab);
        c->btab = NULL;
        c->cap_btab = 0;
        const uint64_t cb = max_blocks < 1 ? 1 : max_blocks;
        HIPCHK(dmx_malloc(&c->btab, cb * sizeof(dmx_bblk)));
        c->cap_btab = cb;
    }
    if (max_streams > c->cap_bstreams || !c->bplan) {
        if (c->bplan) (void)hipFree(c->bplan);
        c->bplan = NULL;
        c->cap_bstreams = 0;
        HIPCHK(dmx_malloc(&c->bplan, eb_plan_bytes(max_streams)));
        c->cap_bstreams = max_streams;
    }
    return 0;
}

extern "C" int dmx_ctx_reserve_batch_dict(dmx_ctx* c, uint32_t max_blocks, uint32_t max_streams, uint32_t max_dicts,
                                          int32_t sw, uint32_t flags) {
    if (!c) return -(int)E_INVAL;
    if (sw == 0) sw = DMX_BLK;
    if (sw < 1 || sw > DMX_BLK) return -(int)E_RANGE;
    if (max_blocks > 0x7FFFFFFFu || max_streams > 0x7FFFFFFFu || max_dicts > 0x7FFFFFFFu) return -(int)E_RANGE;
    if (flags & (DMX_F_SPLIT | DMX_F_BGZF | DMX_F_GZIP)) return -(int)E_INVAL;
    const uint64_t slots = (uint64_t)max_blocks + max_dicts;
    if (max_blocks <= c->cap_blocks && max_blocks <= c->cap_btab && c->bplan && max_streams <= c->cap_bstreams &&
        c->bdictid && max_dicts <= c->cap_bdicts && slots <= c->cap_chain)
        return 0;   // nothing to do: no synchronisation
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipDeviceSynchronize());
    // the chain slots grow with the workspace (ctx_reserve_scratch): a slot per block, one for a single
    // encode's dictionary, and one per dictionary of a batch
    c->want |= DMX_F_DICT;
    if (max_dicts > c->chain_dicts) c->chain_dicts = max_dicts;
    {
        const int r = ctx_reserve(c, max_blocks > c->cap_blocks ? max_blocks : c->cap_blocks);
        if (r) return r;
    }
    {
        const int r = dmx_ctx_reserve_batch(c, max_blocks, max_streams, sw, 0);
        if (r) return r;
    }
    if (max_dicts > c->cap_bdicts || !c->bdictid) {
        if (c->bdictid) (void)hipFree(c->bdictid);
        c->bdictid = NULL;
        c->cap_bdicts = 0;
        HIPCHK(dmx_malloc(&c->bdictid, ((uint64_t)max_dicts + 1) * sizeof(uint32_t)));
        c->cap_bdicts = max_dicts;
    }
    return 0;
}

// What only dmx_encode_batch_dict_async has: the dictionaries' bytes and the verdict's records.
struct EbDicts {
    const uint8_t* bytes;
    dmx_ebd d;
};

// The batch encode, once its caller has looked at the arguments only it has.  dict NULL:
// dmx_encode_batch_async, whose plan runs with the empty dmx_ebd.
static int eb_run(dmx_ctx* c, const void* d_in, uint64_t in_bytes, const dmx_estream* d_streams, uint32_t nstreams,
                  uint32_t max_blocks, const EbDicts* dict, const dmx_opts* opts, void* d_out, uint64_t out_cap,
                  dmx_eresult* d_results, dmx_ebatch_status* d_status, void* stream) {
    if (!c || !d_out || !d_results || !d_status || (!d_in && in_bytes) || (!d_streams && nstreams)) return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_streams) & 7) || (reinterpret_cast<uintptr_t>(d_results) & 7) ||
        (reinterpret_cast<uintptr_t>(d_status) & 7) || (reinterpret_cast<uintptr_t>(d_out) & 3))
        return -(int)E_INVAL;
    dmx_opts o = {0, 0, DMX_ZLIB, 0, NULL, 0};
    if (opts) o = *opts;
    if (!(dict ? ebd_flags_ok(o.flags) : eb_flags_ok(o.flags))) return -(int)E_INVAL;
    if (o.sw == 0) o.sw = DMX_BLK;
    if (o.sw < 1 || o.sw > DMX_BLK) return -(int)E_RANGE;
    if (o.max_chain < 0) return -(int)E_RANGE;
    if (o.deep_chain < 0 || o.deep_chain > 255) return -(int)E_RANGE;
    const uint32_t ndicts = dict ? dict->d.ndicts : 0u;
    if (nstreams > 0x7FFFFFFFu || max_blocks > 0x7FFFFFFFu || ndicts > 0x7FFFFFFFu) return -(int)E_RANGE;
    if (!c->bplan || !c->btab || max_blocks > c->cap_blocks || max_blocks > c->cap_btab || nstreams > c->cap_bstreams)
        return -(int)E_SZ;
    if (dict && (!c->bdictid || ndicts > c->cap_bdicts || (uint64_t)max_blocks + ndicts > c->cap_chain)) return -(int)E_SZ;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const uint32_t sw = (uint32_t)o.sw, maxb = max_blocks;
    uint8_t* const pl = (uint8_t*)c->bplan;
    dmx_eb_head* head = (dmx_eb_head*)pl;
    dmx_eb_tile* ptiles = (dmx_eb_tile*)(pl + 256);
    uint64_t* starts = (uint64_t*)(pl + eb_off_starts(c->cap_bstreams));
    const uint32_t stiles = (uint32_t)eb_tiles_of(nstreams);
    const dmx_ebd d = dict ? dict->d : dmx_ebd_none();
    const dmx_bblk* tab = (const dmx_bblk*)c->btab;
    // stage times (dmx_ctx_set_timing) of a dictionary batch, with the single encode's boundaries: [0] the
    // plan, the DICTIDs, the chains, the history search and K0, [1] K1, [2] K2, [3] K3, [4] K4 and the finish
    hipEvent_t* ev = NULL;
    if (dict && c->timing && (c->ev_every <= 1 || c->ev_count++ % c->ev_every == 0)) {
        const int j = (int)(c->ev_next++ % DMX_EV_RING);
        ctx_collect_set(c, j);
        ev = c->ev[j];
        c->ev_used[j] = 1;
    }
    auto stamp = [&](int k) { if (ev && ((c->timing >> k) & 1)) (void)hipEventRecord(ev[k], s); };
    stamp(0);
    // the plan
    if (nstreams)
        hipLaunchKernelGGL(dmx_eb_count_kernel, dim3(stiles), dim3(EB_WG), 0, s, d_streams, nstreams, in_bytes, sw, d, ptiles);
    hipLaunchKernelGGL(dmx_eb_plan_scan_kernel, dim3(1), dim3(DMX_EB_STHREADS), 0, s, ptiles, stiles, maxb, head);
    if (nstreams)
        hipLaunchKernelGGL(dmx_eb_starts_kernel, dim3(stiles), dim3(EB_WG), 0, s, d_streams, nstreams, in_bytes, sw, d,
                           (const dmx_eb_tile*)ptiles, starts, d_results);
    // the DICTIDs: the Adler-32 of every dictionary (0 for a record outside d_dict, which no header names)
    if ((o.flags & DMX_F_FDICT) && ndicts && dmx_dict_adler_batch_launch(dict->bytes, d.dict_bytes, d.dicts, ndicts, c->bdictid, s))
        return -(int)E_DEVICE;
    if (maxb) {
        hipLaunchKernelGGL(dmx_eb_table_kernel, dim3((maxb + EB_WG - 1) / EB_WG), dim3(EB_WG), 0, s, d_streams,
                           (const uint64_t*)starts, nstreams, (const dmx_eb_head*)head, sw, d, maxb, c->btab, c->info);
        // K0, K1, K2: a workgroup per table entry; void entries return at once
        const uint32_t mfl = ((o.flags & DMX_F_LAZY) ? 1u : 0u) | ((o.flags & DMX_F_EXACT_SORT) ? 2u : 0u) |
                             ((o.flags & DMX_F_STORE_CHECK) ? 4u : 0u) | ((o.flags & DMX_F_DEEP) ? 8u : 0u) |
                             ((uint32_t)o.deep_chain << 16);
        const EbMatchArgs ma = {(const uint8_t*)d_in, sw, o.max_chain, mfl, c->dist, c->tok, c->hist, c->info, c->nfb, tab};
        if (dict) {   // the chains of the dictionaries and of every table entry, then the history search
            hipLaunchKernelGGL(dmx_ebd_chain_kernel, dim3(ndicts + maxb), dim3(MT), 0, s, (const uint8_t*)d_in, sw,
                               dict->bytes, d, tab, c->chs, c->che, c->nfb);
            const uint32_t resident = c->hk_bdict_simple ? 0u : 1u;
            const EbdHistArgs ha = {(const uint8_t*)d_in, sw, o.max_chain, dict->bytes, d, c->chs, c->che, c->tok, tab, maxb,
                                    resident};
            hipLaunchKernelGGL((o.max_chain >= 1 && o.max_chain <= 6) ? dmx_ebd_hist_kernel<6>
                               : o.max_chain == 7 ? dmx_ebd_hist_kernel<7> : dmx_ebd_hist_kernel<8>,
                               dim3(resident ? (maxb < c->ncu ? maxb : c->ncu) : maxb), dim3(MT), 0, s, ha);
        }
        if (o.flags & DMX_F_STORE_CHECK)
            hipLaunchKernelGGL(dict ? dmx_ebd_store_check_kernel : dmx_eb_store_check_kernel, dim3(maxb), dim3(SCT), 0, s,
                               (const uint8_t*)d_in, sw, c->info, c->tok, c->hist, o.flags, tab);
        stamp(1);
        if (dict) {
            // (match_block reads its own chains at slot b + 1: ndicts - 1 slots further, that is ndicts + b)
            const uint16_t* chs1 = reinterpret_cast<const uint16_t*>(reinterpret_cast<uintptr_t>(c->chs) +
                                                                      ((uintptr_t)ndicts - 1) * DMX_BLK * sizeof(uint16_t));
            const EbdMatchArgs dma = {ma, chs1};
            hipLaunchKernelGGL(dmx_ebd_match_kernel, dim3(maxb), dim3(MT), 0, s, dma);
        } else if (o.max_chain == 0) {
            hipLaunchKernelGGL(dmx_eb_match_kernel<DMX_NBX>, dim3(maxb), dim3(MT), 0, s, ma);
        } else {
            hipLaunchKernelGGL(dmx_eb_match_kernel<3>, dim3(maxb), dim3(MT), 0, s, ma);
        }
        stamp(2);
        // (without DMX_F_FINAL: every header's BFINAL bit is 0, K4 sets it from the table; K2 and K4 frame
        // nothing in a batch, so the dictionary flags, which only a dictionary batch has, stop here too)
        hipLaunchKernelGGL(dmx_huff_kernel, dim3(maxb), dim3(64), 0, s, c->hist, c->info, c->codes, c->hdr, c->sub, maxb,
                           o.flags & ~(DMX_F_FINAL | DMX_F_FDICT), (const uint32_t*)NULL, (const uint32_t*)NULL,
                           (const uint16_t*)NULL);
        stamp(3);
    } else {
        for (int k = 1; k <= 3; k++) stamp(k);
    }
    // K3
    const uint32_t ntile = (maxb + SCAN_TILE - 1) / SCAN_TILE;
    if (maxb)
        hipLaunchKernelGGL(dict ? dmx_eb_scan_tile_kernel<true> : dmx_eb_scan_tile_kernel<false>, dim3(ntile), dim3(SCAN_TILE),
                           0, s, c->info, tab, maxb, o.flags, c->tiles);
    if (maxb && ntile <= SA1_MAXT && !c->hk_scan3) {
        hipLaunchKernelGGL(dict ? dmx_eb_scan_apply1_kernel<true> : dmx_eb_scan_apply1_kernel<false>, dim3(ntile),
                           dim3(SCAN_TILE), 0, s, c->info, tab, maxb, o.flags, out_cap, (const ScanTile*)c->tiles,
                           (uint32_t*)d_out, c->res, c->nfb, (const dmx_eb_head*)head, d_status);
    } else {
        hipLaunchKernelGGL(dmx_eb_scan_kernel, dim3(1), dim3(ST), 0, s, c->tiles, maxb, out_cap, c->res, c->nfb,
                           (const dmx_eb_head*)head, d_status);
        if (maxb)
            hipLaunchKernelGGL(dict ? dmx_eb_apply_kernel<true> : dmx_eb_apply_kernel<false>, dim3(ntile), dim3(SCAN_TILE), 0,
                               s, c->info, tab, maxb, o.flags, (const ScanTile*)c->tiles, (uint32_t*)d_out,
                               (const dmx_result*)c->res);
    }
    stamp(4);
    if (maxb)
        hipLaunchKernelGGL(dmx_eb_pack_kernel, dim3(maxb), dim3(PT), 0, s, (const uint8_t*)d_in, sw, c->tok, c->codes,
                           c->hdr, c->info, c->sub, maxb, o.flags & ~(DMX_F_FDICT | DMX_F_DICT), (uint32_t*)d_out, c->res, tab);
    if (nstreams) {
        const dim3 fgrid((nstreams + EB_FIN_WAVES - 1) / EB_FIN_WAVES), fwg(64 * EB_FIN_WAVES);
        if (o.flags & DMX_F_GZIP) {   // (the plain batch only: ebd_flags_ok refuses gzip)
            const uint32_t gmax = 3 * crc_device_ncu();   // 3 workgroups of 52 KiB LDS per CU
            hipLaunchKernelGGL(dmx_eb_crc_kernel, dim3(nstreams < gmax ? nstreams : gmax), dim3(CRC_T), 0, s,
                               (const uint8_t*)d_in, in_bytes, d_streams, nstreams, d_results);
        }
        if (dict)
            hipLaunchKernelGGL(dmx_ebd_finish_kernel, fgrid, fwg, 0, s, d_streams, (const uint64_t*)starts, nstreams, in_bytes,
                               sw, o.flags, (const dmx_blkinfo*)c->info, (const dmx_eb_head*)head, (const dmx_result*)c->res,
                               (uint32_t*)d_out, d_results, d, (const uint32_t*)c->bdictid, tab);
        else
            hipLaunchKernelGGL(dmx_eb_finish_kernel, fgrid, fwg, 0, s, d_streams, (const uint64_t*)starts, nstreams, in_bytes,
                               sw, o.flags, (const dmx_blkinfo*)c->info, (const dmx_eb_head*)head, (const dmx_result*)c->res,
                               (uint32_t*)d_out, d_results);
    }
    stamp(5);
    HIPCHK(fault_hit(2) ? hipErrorLaunchFailure : hipGetLastError());
    c->last_nblk = 0;   // (the per-block introspection addresses blocks by b * sw)
    c->last_sw = sw;
    c->last_batch = 1;
    return 0;
}

extern "C" int dmx_encode_batch_async(dmx_ctx* c, const void* d_in, uint64_t in_bytes, const dmx_estream* d_streams,
                                      uint32_t nstreams, uint32_t max_blocks, const dmx_opts* opts, void* d_out,
                                      uint64_t out_cap, dmx_eresult* d_results, dmx_ebatch_status* d_status, void* stream) {
    return eb_run(c, d_in, in_bytes, d_streams, nstreams, max_blocks, NULL, opts, d_out, out_cap, d_results, d_status, stream);
}

extern "C" int dmx_encode_batch_dict_async(dmx_ctx* c, const void* d_in, uint64_t in_bytes, const dmx_estream* d_streams,
                                           uint32_t nstreams, uint32_t max_blocks, const void* d_dict, uint64_t dict_bytes,
                                           const dmx_bdict* d_dicts, uint32_t ndicts, const uint32_t* d_dict_of,
                                           const dmx_opts* opts, void* d_out, uint64_t out_cap, dmx_eresult* d_results,
                                           dmx_ebatch_status* d_status, void* stream) {
    if ((!d_dicts && ndicts) || (!d_dict && dict_bytes)) return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_dicts) & 7) || (reinterpret_cast<uintptr_t>(d_dict_of) & 3)) return -(int)E_INVAL;
    const uint32_t fdict = (opts && (opts->flags & DMX_F_FDICT)) ? 1u : 0u;
    const EbDicts dict = {(const uint8_t*)d_dict, {d_dicts, d_dict_of, dict_bytes, ndicts, fdict}};
    return eb_run(c, d_in, in_bytes, d_streams, nstreams, max_blocks, &dict, opts, d_out, out_cap, d_results, d_status, stream);
}

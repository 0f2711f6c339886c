// dmx_encode_batch_dict.hip -- batches of independent buffers against preset dictionaries
// (include/dmx.h: dmx_encode_batch_dict_async).  Compiled into dmx_kernels.hip's
// translation unit behind dmx_encode_batch.hip, whose plan scratch, layout scan, pack and finish it
// runs with the dictionary's verdict (the DB forms there).
//
// The bytes of stream k are the single encode's for buffer k with opts->dict = its dictionary, so
// block 0 of a stream searches its dictionary's last min(len, sw) bytes, block j >= 1 searches
// block j - 1 of its own stream, and no block ever searches the table entry before it when that
// belongs to another stream.  Chain slots: [0, ndicts) the dictionaries, each sorted once per call
// however many streams share it; ndicts + b table entry b.
//   dmx_ebd_count / starts / table kernels   the plan of dmx_encode_batch.hip with dmx_ebd_status
//   dmx_dict_adler_kernel                    the DICTIDs (DMX_F_FDICT), a kernel of the call: the
//                                            dictionaries may change between two replays of a graph
//   dmx_ebd_chain_kernel                     dmx_chain_kernel's body, the source from the table or d_dicts
//   dmx_ebd_hist_kernel<6|7|8>               dmx_hist_kernel_t's search as a loop: a workgroup walks a
//                                            contiguous range of table entries and keeps a dictionary's
//                                            staged history, S and bucket ends in LDS while the next
//                                            entry's history is the same slot
//   K0 with uni_ok 0, K1 = match_block<true, 3, false, true>, K2, K3 (DB), K4, the finish (DB)

// ---- the plan with dictionaries: dmx_eb_count_kernel, dmx_eb_starts_kernel and dmx_eb_table_kernel
// with the dmx_ebd_* per-thread text (dmx_eb_plan_scan_kernel is shared) ----
__global__ __launch_bounds__(EB_WG) void dmx_ebd_count_kernel(const dmx_estream* __restrict__ st, uint32_t nstreams,
                                                              uint64_t in_bytes, uint32_t sw, const dmx_ebd d,
                                                              dmx_eb_tile* __restrict__ tiles) {
    __shared__ uint64_t sh[EB_WG];
    const uint64_t k = (uint64_t)blockIdx.x * DMX_EB_STILE + threadIdx.x;
    const dmx_eb_tile v = k < nstreams ? dmx_ebd_stream_sums(st, (uint32_t)k, in_bytes, sw, d) : dmx_eb_tile_zero();
    uint64_t before;
    const dmx_eb_tile t = eb_wg_sums(v, sh, &before);
    if (threadIdx.x == 0) tiles[blockIdx.x] = t;
}

__global__ __launch_bounds__(EB_WG) void dmx_ebd_starts_kernel(const dmx_estream* __restrict__ st, uint32_t nstreams,
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

__global__ __launch_bounds__(EB_WG) void dmx_ebd_table_kernel(const dmx_estream* __restrict__ st,
                                                              const uint64_t* __restrict__ starts, uint32_t nstreams,
                                                              const dmx_eb_head* __restrict__ head, uint32_t sw,
                                                              const dmx_ebd d, uint32_t max_blocks,
                                                              dmx_bblk* __restrict__ tab, dmx_blkinfo* __restrict__ info) {
    const uint64_t b = (uint64_t)blockIdx.x * EB_WG + threadIdx.x;
    if (b >= max_blocks) return;
    const dmx_bblk e = dmx_ebd_entry(st, starts, nstreams, head, sw, d, (uint32_t)b);
    tab[b] = e;
    dmx_blkinfo bi;   // (the block record before K0 / K1, as dmx_eb_table_kernel leaves it)
    memset(&bi, 0, sizeof(bi));
    bi.nsub = 1;
    if (e.len & DMX_BB_VOID) bi.prestored = 1;
    else if (!(e.len & DMX_BB_LEN)) { bi.prestored = 1; bi.btype = 1; bi.hdr_bits = 3; bi.body_bits = 7; }
    info[b] = bi;
}

// ---- the chains: slot < ndicts sorts that dictionary's last min(len, sw) bytes, slot ndicts + b table
// entry b.  dmx_chain_kernel's body; void entries, empty blocks and records outside d_dict (no stream
// that names one has blocks) return at once.
__global__ __launch_bounds__(MT) void dmx_ebd_chain_kernel(const uint8_t* __restrict__ in, uint32_t sw,
                                                           const uint8_t* __restrict__ dict, const dmx_ebd d,
                                                           const dmx_bblk* __restrict__ tab,
                                                           uint16_t* __restrict__ chs, uint16_t* __restrict__ che,
                                                           uint32_t* __restrict__ nfallback) {
    __shared__ MatchLDS L;
    __shared__ uint64_t tp0[3];
    __shared__ uint32_t nruns;
    const uint32_t tid = threadIdx.x;
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
    if (len < 3) return;   // no entries
    stage_bytes(L.data, DATA_WORDS, src, len, nullptr, 0, tid);
    const uint32_t nv = len - 2;
    uint16_t* S = chs + (uint64_t)slot * DMX_BLK;
    uint16_t* E = che + (uint64_t)slot * DMX_NBUCKET;
    if (tid == 0) nruns = 0;
    __syncthreads();
    uint32_t runny = 0;
    for (uint32_t k = tid; k < (len + 15) / 16; k += MT) {
        const uint4 v = reinterpret_cast<const uint4*>(L.data)[k];
        runny += (k * 16 + 16 <= len && v.x == v.y && v.y == v.z && v.z == v.w && v.x == (v.x & 0xFFu) * 0x01010101u) ? 1u : 0u;
    }
    if (runny) atomicAdd(&nruns, runny);
    __syncthreads();
    const bool runs = nruns * 4u >= (len + 15) / 16;
    for (uint32_t attempt = 0;; attempt++) {
        if (attempt == 0 && runs) sort_positions<false, true>(L, len, 1, tid, false, tp0);
        else if (attempt == 0) sort_positions<false, false>(L, len, 1, tid, false, tp0);
        else sort_positions<true>(L, len, 1, tid, false, tp0);
        for (uint32_t k = tid; k < DMX_NBUCKET; k += MT) L.bstart[k] = 0;
        __syncthreads();
        bool bad = false;   // (every adjacent pair ascends by (bucket, position), as dmx_chain_kernel verifies)
        for (uint32_t k = tid; k < nv; k += MT) {
            const uint32_t q = L.sorted[k];
            const uint32_t h = dmx_hash(ld4(L.data, q) & 0xFFFFFFu);
            if (k + 1 < nv) {
                const uint32_t q1 = L.sorted[k + 1];
                const uint32_t h1 = dmx_hash(ld4(L.data, q1) & 0xFFFFFFu);
                if (h1 != h) L.bstart[h] = (uint16_t)(k + 1);
                if (((h1 << 15) | q1) < ((h << 15) | q)) bad = true;
            } else {
                L.bstart[h] = (uint16_t)(k + 1);
            }
        }
        if (!__syncthreads_or(bad) || attempt) break;
        if (tid == 0) atomicAdd(nfallback, 1u);
    }
    for (uint32_t k = tid; k < (nv + 7) / 8; k += MT)   // 8 entries per 16-byte store
        reinterpret_cast<uint4*>(S)[k] = reinterpret_cast<const uint4*>(L.sorted)[k];
    for (uint32_t k = tid; k < DMX_NBUCKET / 8; k += MT)
        reinterpret_cast<uint4*>(E)[k] = reinterpret_cast<const uint4*>(L.bstart)[k];
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

// 16-byte chunks [c0, c1) of W: bytes src[0, len), then src2[0, len2), then zeros (stage_bytes on a range)
__device__ __forceinline__ void ebd_stage_range(uint32_t* W, uint32_t c0, uint32_t c1, const uint8_t* src, uint32_t len,
                                                const uint8_t* src2, uint32_t len2, uint32_t tid) {
    const bool al = ((reinterpret_cast<uintptr_t>(src) & 15) == 0);
    for (uint32_t k = c0 + tid; k < c1; k += MT) {
        const uint32_t p = k << 4;
        uint4 v;
        if (al && p + 16 <= len) {
            v = *reinterpret_cast<const uint4*>(src + p);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t j = 0; j < 16; j++) {
                const uint32_t x = p + j;
                const uint32_t c = x < len ? src[x] : (x - len < len2 ? src2[x - len] : 0u);
                w[j >> 2] |= c << (8 * (j & 3));
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(&W[k << 2]) = v;
    }
}

// The search of one staged block (dmx_hist_kernel_t's loop): for every entry k of the block's S, the
// longest match against the history in L, into hb[k].
template <int HG>
__device__ __forceinline__ void ebd_hist_search(HistLDS& L, const uint16_t* __restrict__ Sc, uint32_t hn, uint32_t bn,
                                                int32_t max_chain, uint32_t* __restrict__ hb, uint32_t tid) {
    const uint32_t nvalid = bn > 2 ? bn - 2 : 0;
    const uint16_t* Ep = L.ep;
    const uint32_t K = max_chain > 0 ? (uint32_t)max_chain : 0xFFFFFFFFu;
    const uint32_t lane = tid & 63, wave = wave_of(tid);
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t qn = 0;   // queued entries of this wave (K <= HG)
    uint32_t inext = tid < nvalid ? (uint32_t)Sc[tid] : 0u;
    for (uint32_t k0 = tid - lane; k0 < nvalid; k0 += MT) {   // (wave-uniform trip count)
        const uint32_t k = k0 + lane;
        const bool act = k < nvalid;
        const uint32_t i = inext;
        if (k + MT < nvalid) inext = Sc[k + MT];
        uint32_t best = 0, bq = 0, full = 0;
        int32_t x0 = -1;
        if (act) {
            uint32_t t0, t1, t2;
            ld12(L.cur, i, t0, t1, t2);
            const uint32_t h = dmx_hash(t0 & 0xFFFFFFu);
            const uint32_t lim = min(bn - i, (uint32_t)MAXLEN);
            const int32_t minq = (int32_t)(hn + i) - 32768;   // distance <= 32768
            x0 = (int32_t)Ep[h] - 1;
            if (K <= (uint32_t)HG) {
                hist_group<HG, true, true>(L, x0, 0, K, h, t0, t1, t2, i, lim, minq, best, bq, &full);
            } else {
                uint32_t cnt = 0;
                for (int32_t x = x0; x >= 0 && cnt < K && best < lim; x -= HG, cnt += HG)
                    if (hist_group<HG, false>(L, x, cnt, K, h, t0, t1, t2, i, lim, minq, best, bq)) break;
            }
        }
        const bool push = full != 0;
        const uint64_t pm = __ballot(push);
        const uint32_t np = (uint32_t)__popcll(pm);
        if (qn + np > 64) {
            hist_flush(L, wave, qn, lane, hn, bn, hb);
            qn = 0;
        }
        if (push) {
            const uint32_t slot = qn + (uint32_t)__popcll(pm & lt);
            lds_st(&L.qd[wave][slot][0], k | (full << 16));
            lds_st(&L.qd[wave][slot][1], (uint32_t)x0 | (i << 16));
        } else if (act) {
            hb[k] = best >= 3 ? (best << 16) | (hn - bq + i) : 0u;
        }
        qn += np;
    }
    if (qn) hist_flush(L, wave, qn, lane, hn, bn, hb);
}

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
            ebd_stage_range(L.data, hn / 16, c1 < DATA_WORDS / 4 ? c1 : DATA_WORDS / 4, hs, hn, cur, bn, tid);
        } else {
            stage_bytes(L.data, DATA_WORDS, hs, hn, cur, bn, tid);
            const uint4* Sg = reinterpret_cast<const uint4*>(a.chs + (uint64_t)slot * DMX_BLK);
            const uint4* Eg = reinterpret_cast<const uint4*>(a.che + (uint64_t)slot * DMX_NBUCKET);
            for (uint32_t k = tid; k < (hn - 2 + 7) / 8; k += MT) reinterpret_cast<uint4*>(L.sp)[k] = Sg[k];
            for (uint32_t k = tid; k < DMX_NBUCKET / 8; k += MT) reinterpret_cast<uint4*>(L.ep)[k] = Eg[k];
        }
        if (a.resident) {   // the block and the slack behind it the search may read (bytes past bn never decide)
            const uint32_t c1 = (bn + 15) / 16 + 6;
            ebd_stage_range(L.cur, 0, c1 < (DMX_BLK / 4 + 80) / 4 ? c1 : (DMX_BLK / 4 + 80) / 4, cur, bn, nullptr, 0, tid);
        } else {
            stage_bytes(L.cur, DMX_BLK / 4 + 80, cur, bn, nullptr, 0, tid);
        }
        held = (e.len & DMX_BB_FIRST) ? slot : 0xFFFFFFFFu;
        held_hn = hn;
        __syncthreads();
        ebd_hist_search<HG>(L, a.chs + (uint64_t)(a.d.ndicts + b) * DMX_BLK, hn, bn, a.max_chain, hb, tid);
    }
}

// ---- K0 and K1: the batch instantiations with a history ----
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

// ---- K3 and the finish with the per-stream header width ----
__global__ __launch_bounds__(SCAN_TILE) void dmx_ebd_scan_tile_kernel(dmx_blkinfo* __restrict__ info,
                                                                     const dmx_bblk* __restrict__ tab, uint32_t max_blocks,
                                                                     uint32_t flags, ScanTile* __restrict__ tiles) {
    eb_scan_tile<true>(info, tab, max_blocks, flags, tiles);
}
__global__ __launch_bounds__(SCAN_TILE) void dmx_ebd_apply_kernel(dmx_blkinfo* __restrict__ info,
                                                                 const dmx_bblk* __restrict__ tab, uint32_t max_blocks,
                                                                 uint32_t flags, const ScanTile* __restrict__ tiles,
                                                                 uint32_t* __restrict__ out32,
                                                                 const dmx_result* __restrict__ res) {
    const uint32_t b = blockIdx.x * SCAN_TILE + threadIdx.x;
    if (b >= max_blocks) return;
    const ScanTile& T = tiles[blockIdx.x];
    Mono tp;   // the prefix dmx_eb_scan_kernel left
    tp.s = (uint32_t)T.ps; tp.a = T.pa; tp.c = T.pc;
    eb_apply_block<true>(info, tab, b, flags, tp, out32, res->status == 0);
}
// (dmx_eb_scan_apply1_kernel's text with the DB forms of the block's place)
__global__ __launch_bounds__(SCAN_TILE) void dmx_ebd_scan_apply1_kernel(dmx_blkinfo* __restrict__ info,
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
    if (b < max_blocks) eb_apply_block<true>(info, tab, b, flags, s_pre, out32, ext.status == 0);
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
// Stream k needs at most align4(dmx_max_compressed_flags(len_k, sw, flags)): dmx_encode_batch_bound's sum
// with the DICTID's 4 bytes per stream under DMX_F_FDICT.
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

static int ebd_flags_ok(uint32_t f) {
    if (!(f & DMX_F_DICT)) return 0;
    if (f & (DMX_F_SPLIT | DMX_F_BGZF | DMX_F_GZIP)) return 0;
    if (!(f & DMX_F_FINAL)) return 0;
    if (!(f & DMX_F_HEADER) != !(f & DMX_F_TRAILER)) return 0;
    if ((f & DMX_F_FDICT) && !(f & DMX_F_HEADER)) return 0;
    return 1;
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

extern "C" int dmx_encode_batch_dict_async(dmx_ctx* c, const void* d_in, uint64_t in_bytes, const dmx_estream* d_streams,
                                           uint32_t nstreams, uint32_t max_blocks, const void* d_dict, uint64_t dict_bytes,
                                           const dmx_bdict* d_dicts, uint32_t ndicts, const uint32_t* d_dict_of,
                                           const dmx_opts* opts, void* d_out, uint64_t out_cap, dmx_eresult* d_results,
                                           dmx_ebatch_status* d_status, void* stream) {
    if (!c || !d_out || !d_results || !d_status || (!d_in && in_bytes) || (!d_streams && nstreams) ||
        (!d_dicts && ndicts) || (!d_dict && dict_bytes))
        return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_streams) & 7) || (reinterpret_cast<uintptr_t>(d_results) & 7) ||
        (reinterpret_cast<uintptr_t>(d_status) & 7) || (reinterpret_cast<uintptr_t>(d_out) & 3) ||
        (reinterpret_cast<uintptr_t>(d_dicts) & 7) || (reinterpret_cast<uintptr_t>(d_dict_of) & 3))
        return -(int)E_INVAL;
    dmx_opts o = {0, 0, DMX_ZLIB, 0, NULL, 0};
    if (opts) o = *opts;
    if (!ebd_flags_ok(o.flags)) return -(int)E_INVAL;
    if (o.sw == 0) o.sw = DMX_BLK;
    if (o.sw < 1 || o.sw > DMX_BLK) return -(int)E_RANGE;
    if (o.max_chain < 0) return -(int)E_RANGE;
    if (o.deep_chain < 0 || o.deep_chain > 255) return -(int)E_RANGE;
    if (nstreams > 0x7FFFFFFFu || max_blocks > 0x7FFFFFFFu || ndicts > 0x7FFFFFFFu) return -(int)E_RANGE;
    if (!c->bplan || !c->btab || !c->bdictid || max_blocks > c->cap_blocks || max_blocks > c->cap_btab ||
        nstreams > c->cap_bstreams || ndicts > c->cap_bdicts || (uint64_t)max_blocks + ndicts > c->cap_chain)
        return -(int)E_SZ;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const uint32_t sw = (uint32_t)o.sw, maxb = max_blocks;
    uint8_t* const pl = (uint8_t*)c->bplan;
    dmx_eb_head* head = (dmx_eb_head*)pl;
    dmx_eb_tile* ptiles = (dmx_eb_tile*)(pl + 256);
    uint64_t* starts = (uint64_t*)(pl + eb_off_starts(c->cap_bstreams));
    const uint32_t stiles = (uint32_t)eb_tiles_of(nstreams);
    const dmx_ebd d = {d_dicts, d_dict_of, dict_bytes, ndicts, (o.flags & DMX_F_FDICT) ? 1u : 0u};
    const dmx_bblk* tab = (const dmx_bblk*)c->btab;
    // stage times (dmx_ctx_set_timing), with the single encode's boundaries: [0] the plan, the DICTIDs,
    // the chains, the history search and K0, [1] K1, [2] K2, [3] K3, [4] K4 and the finish
    hipEvent_t* ev = NULL;
    if (c->timing && (c->ev_every <= 1 || c->ev_count++ % c->ev_every == 0)) {
        const int j = (int)(c->ev_next++ % DMX_EV_RING);
        ctx_collect_set(c, j);
        ev = c->ev[j];
        c->ev_used[j] = 1;
    }
    auto stamp = [&](int k) { if (ev && ((c->timing >> k) & 1)) (void)hipEventRecord(ev[k], s); };
    stamp(0);
    // the plan
    if (nstreams)
        hipLaunchKernelGGL(dmx_ebd_count_kernel, dim3(stiles), dim3(EB_WG), 0, s, d_streams, nstreams, in_bytes, sw, d, ptiles);
    hipLaunchKernelGGL(dmx_eb_plan_scan_kernel, dim3(1), dim3(DMX_EB_STHREADS), 0, s, ptiles, stiles, maxb, head);
    if (nstreams)
        hipLaunchKernelGGL(dmx_ebd_starts_kernel, dim3(stiles), dim3(EB_WG), 0, s, d_streams, nstreams, in_bytes, sw, d,
                           (const dmx_eb_tile*)ptiles, starts, d_results);
    // the DICTIDs: the Adler-32 of every dictionary (0 for a record outside d_dict, which no header names)
    if ((o.flags & DMX_F_FDICT) && ndicts && dmx_dict_adler_batch_launch(d_dict, dict_bytes, d_dicts, ndicts, c->bdictid, s))
        return -(int)E_DEVICE;
    if (maxb) {
        hipLaunchKernelGGL(dmx_ebd_table_kernel, dim3((maxb + EB_WG - 1) / EB_WG), dim3(EB_WG), 0, s, d_streams,
                           (const uint64_t*)starts, nstreams, (const dmx_eb_head*)head, sw, d, maxb, c->btab, c->info);
        // the chains of the dictionaries and of every table entry, then the history search
        hipLaunchKernelGGL(dmx_ebd_chain_kernel, dim3(ndicts + maxb), dim3(MT), 0, s, (const uint8_t*)d_in, sw,
                           (const uint8_t*)d_dict, d, tab, c->chs, c->che, c->nfb);
        const uint32_t resident = c->hk_bdict_simple ? 0u : 1u;
        const EbdHistArgs ha = {(const uint8_t*)d_in, sw, o.max_chain, (const uint8_t*)d_dict, d, c->chs, c->che, c->tok,
                                tab, maxb, resident};
        hipLaunchKernelGGL((o.max_chain >= 1 && o.max_chain <= 6) ? dmx_ebd_hist_kernel<6>
                           : o.max_chain == 7 ? dmx_ebd_hist_kernel<7> : dmx_ebd_hist_kernel<8>,
                           dim3(resident ? (maxb < c->ncu ? maxb : c->ncu) : maxb), dim3(MT), 0, s, ha);
        if (o.flags & DMX_F_STORE_CHECK)
            hipLaunchKernelGGL(dmx_ebd_store_check_kernel, dim3(maxb), dim3(SCT), 0, s, (const uint8_t*)d_in, sw, c->info,
                               c->tok, c->hist, o.flags, tab);
        stamp(1);
        const uint32_t mfl = ((o.flags & DMX_F_LAZY) ? 1u : 0u) | ((o.flags & DMX_F_EXACT_SORT) ? 2u : 0u) |
                             ((o.flags & DMX_F_STORE_CHECK) ? 4u : 0u) | ((o.flags & DMX_F_DEEP) ? 8u : 0u) |
                             ((uint32_t)o.deep_chain << 16);
        // (match_block reads its own chains at slot b + 1: ndicts - 1 slots further, that is ndicts + b)
        const uint16_t* chs1 = reinterpret_cast<const uint16_t*>(reinterpret_cast<uintptr_t>(c->chs) +
                                                                  ((uintptr_t)ndicts - 1) * DMX_BLK * sizeof(uint16_t));
        const EbdMatchArgs ma = {{(const uint8_t*)d_in, sw, o.max_chain, mfl, c->dist, c->tok, c->hist, c->info, c->nfb, tab},
                                 chs1};
        hipLaunchKernelGGL(dmx_ebd_match_kernel, dim3(maxb), dim3(MT), 0, s, ma);
        stamp(2);
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
        hipLaunchKernelGGL(dmx_ebd_scan_tile_kernel, dim3(ntile), dim3(SCAN_TILE), 0, s, c->info, tab, maxb, o.flags, c->tiles);
    if (maxb && ntile <= SA1_MAXT && !c->hk_scan3) {
        hipLaunchKernelGGL(dmx_ebd_scan_apply1_kernel, dim3(ntile), dim3(SCAN_TILE), 0, s, c->info, tab, maxb, o.flags, out_cap,
                           (const ScanTile*)c->tiles, (uint32_t*)d_out, c->res, c->nfb, (const dmx_eb_head*)head, d_status);
    } else {
        hipLaunchKernelGGL(dmx_eb_scan_kernel, dim3(1), dim3(ST), 0, s, c->tiles, maxb, out_cap, c->res, c->nfb,
                           (const dmx_eb_head*)head, d_status);
        if (maxb)
            hipLaunchKernelGGL(dmx_ebd_apply_kernel, dim3(ntile), dim3(SCAN_TILE), 0, s, c->info, tab, maxb, o.flags,
                               (const ScanTile*)c->tiles, (uint32_t*)d_out, (const dmx_result*)c->res);
    }
    stamp(4);
    if (maxb)   // (K4 frames nothing in a batch: without DMX_F_FDICT, as dmx_encode_batch_async passes its flags)
        hipLaunchKernelGGL(dmx_eb_pack_kernel, dim3(maxb), dim3(PT), 0, s, (const uint8_t*)d_in, sw, c->tok, c->codes,
                           c->hdr, c->info, c->sub, maxb, o.flags & ~(DMX_F_FDICT | DMX_F_DICT), (uint32_t*)d_out, c->res, tab);
    if (nstreams)
        hipLaunchKernelGGL(dmx_ebd_finish_kernel, dim3((nstreams + EB_FIN_WAVES - 1) / EB_FIN_WAVES), dim3(64 * EB_FIN_WAVES),
                           0, s, d_streams, (const uint64_t*)starts, nstreams, in_bytes, sw, o.flags,
                           (const dmx_blkinfo*)c->info, (const dmx_eb_head*)head, (const dmx_result*)c->res,
                           (uint32_t*)d_out, d_results, d, (const uint32_t*)c->bdictid, tab);
    stamp(5);
    HIPCHK(fault_hit(2) ? hipErrorLaunchFailure : hipGetLastError());
    c->last_nblk = 0;
    c->last_sw = sw;
    c->last_batch = 1;
    return 0;
}

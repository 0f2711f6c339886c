// dmx_bgzf_ranges.hip -- batched range reads from a BGZF file in device memory (include/dmx.h:
// dmx_bgzf_read_ranges_async, dmx_bgzf_read_device; DESIGN.md §3.5 "Reading ranges").
//
// Many (offset, length) requests against the decoded bytes become the members they touch, a decode
// of just those members into scratch, and the packed bytes, with no host round trip:
//   1. dmx_brr_reset_kernel   the members' difference array and the head of the work buffer, zeroed
//   2. dmx_brr_plan_kernel    a thread per range: clip, first and last member by binary search,
//                             +1 / -1 into the difference array; the tile's sum of clipped lengths
//   3. dmx_brr_msum_kernel    a thread per member: the index check; the tile's sum of differences
//   4. dmx_brr_scan1_kernel   one workgroup: both lists of tile sums into exclusive prefixes
//   5. dmx_brr_need_kernel    a thread per member: need = prefix of the differences above 0; the
//                             tile's count of needed members and of their bytes
//   6. dmx_brr_scan2_kernel   one workgroup: those tile sums into prefixes; the status, the record,
//                             the device count
//   7. dmx_brr_emit_kernel    the needed members' sub-index entries, CRC words and scratch offsets;
//                             empty entries behind them; d_out_off
//   8. dmx_inflate_index_kernel<false, true> (dmx_inflate_dev.hip: the counted form), grid = max_members
//   9. dmx_crc_ranges_kernel (dmx_crc.hip) over the sub-index, when CRC words are given
//  10. dmx_brr_gather_kernel  the ranges' bytes from the scratch into d_out, 16 bytes a thread
// The per-thread work of the planning stages and of the gather is in dmx_bgzf_ranges.h, which the
// host twin (tests/c/bgzf_ranges_model.cpp) runs as loops under the sanitizers.  Nothing depends on
// the order in which threads or atomics run: the atomics are integer sums, one minimum and one OR.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dmx.h"
#include "dmx_bgzf_ranges.h"
#include "dmx_ctx.h"

#define BRR_WG 256   // threads per workgroup: one member or range each
static_assert(DMX_BRR_MTILE == BRR_WG && DMX_BRR_RTILE == BRR_WG, "a scan tile is a workgroup");
static_assert(DMX_BRR_STHREADS <= 1024, "one workgroup scans the tile sums");
static_assert(sizeof(dmx_brange) == 16 && sizeof(dmx_bgzf_ranges_status) == 32, "ABI");
static_assert(sizeof(dmx_brr_head) <= 256 && offsetof(dmx_brr_head, ist) % 8 == 0, "work head");

// The work buffer, every part 256-byte aligned:
// [head | diff (nblk + 1) | dsum, ncnt, nlen (member tiles) | rsum (range tiles) | clen, rm0, rdelta (nranges) |
//  moff (nblk) | sub-index, CRC words (max_members) | tables (max_members) | scratch]
struct BrrLayout {
    uint64_t o_diff, o_dsum, o_ncnt, o_nlen, o_rsum, o_clen, o_rm0, o_rdelta, o_moff, o_sub, o_subcrc, o_tab, o_scratch, bytes;
    uint32_t mtiles, rtiles;
};
static inline uint64_t brr_a256(uint64_t x) { return (x + 255) & ~255ull; }
static BrrLayout brr_layout(uint32_t nblk, uint32_t nranges, uint32_t max_members, uint64_t scratch_bytes) {
    BrrLayout L;
    L.mtiles = (uint32_t)(((uint64_t)nblk + DMX_BRR_MTILE - 1) / DMX_BRR_MTILE);
    L.rtiles = (uint32_t)(((uint64_t)nranges + DMX_BRR_RTILE - 1) / DMX_BRR_RTILE);
    L.o_diff = 256;
    L.o_dsum = L.o_diff + brr_a256(((uint64_t)nblk + 1) * 4);
    L.o_ncnt = L.o_dsum + brr_a256((uint64_t)L.mtiles * 4);
    L.o_nlen = L.o_ncnt + brr_a256((uint64_t)L.mtiles * 4);
    L.o_rsum = L.o_nlen + brr_a256((uint64_t)L.mtiles * 8);
    L.o_clen = L.o_rsum + brr_a256((uint64_t)L.rtiles * 8);
    L.o_rm0 = L.o_clen + brr_a256((uint64_t)nranges * 8);
    L.o_rdelta = L.o_rm0 + brr_a256((uint64_t)nranges * 4);
    L.o_moff = L.o_rdelta + brr_a256((uint64_t)nranges * 4);
    L.o_sub = L.o_moff + brr_a256((uint64_t)nblk * 8);
    L.o_subcrc = L.o_sub + brr_a256((uint64_t)max_members * sizeof(dmx_iblock));
    L.o_tab = L.o_subcrc + brr_a256((uint64_t)max_members * 4);
    L.o_scratch = L.o_tab + brr_a256(dmx_itab_bytes(max_members));
    // (the CRC pass loads whole aligned 16-byte groups: the scratch begins and ends on one)
    const uint64_t sb = scratch_bytes > (1ull << 62) ? (1ull << 62) : scratch_bytes;
    L.bytes = L.o_scratch + brr_a256(sb);   // (clamped: no sum wraps, and no buffer is that large)
    return L;
}

// Exclusive scan of v over the workgroup with op (commutative, ident its neutral element), in LDS:
// returns op over the threads before this one, *total = over all.  sh: blockDim.x elements.
template <typename T, typename Op>
__device__ static inline T brr_scan(T v, T ident, T* sh, Op op, T* total) {
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

__global__ __launch_bounds__(BRR_WG) void dmx_brr_reset_kernel(int32_t* __restrict__ diff, uint32_t nblk,
                                                              dmx_brr_head* __restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * BRR_WG + threadIdx.x;
    if (i <= nblk) diff[i] = 0;
    if (i == 0) {
        dmx_brr_head h;
        memset(&h, 0, sizeof(h));
        h.bad = DMX_BRR_NOBAD;
        *head = h;
    }
}

// nranges == 0 or nblk == 0: nothing to read
__global__ __launch_bounds__(BRR_WG) void dmx_brr_empty_kernel(uint64_t* __restrict__ out_off, uint32_t nranges,
                                                              dmx_bgzf_ranges_status* __restrict__ rec) {
    const uint64_t i = (uint64_t)blockIdx.x * BRR_WG + threadIdx.x;
    if (i <= nranges) out_off[i] = 0;
    if (i == 0) {
        const dmx_bgzf_ranges_status r = {0, 0, 0, 0, DMX_BRR_NOBAD, 0};
        *rec = r;
    }
}

__global__ __launch_bounds__(BRR_WG) void dmx_brr_plan_kernel(const uint8_t* __restrict__ z, uint64_t zlen,
                                                             const dmx_iblock* __restrict__ idx, uint32_t nblk,
                                                             const dmx_brange* __restrict__ rg, uint32_t nranges,
                                                             uint32_t flags, int32_t* diff, uint64_t* __restrict__ clen,
                                                             uint32_t* __restrict__ rm0, uint32_t* __restrict__ rdelta,
                                                             uint64_t* __restrict__ rsum, dmx_brr_head* head) {
    __shared__ uint64_t sh[BRR_WG];
    const uint64_t q = (uint64_t)blockIdx.x * DMX_BRR_RTILE + threadIdx.x;
    uint64_t c = 0;
    if (q < nranges) c = dmx_brr_plan(z, zlen, idx, nblk, rg, (uint32_t)q, flags, diff, clen, rm0, rdelta, head);
    uint64_t sum;
    brr_scan<uint64_t>(c, 0, sh, dmx_brr_op_sat(), &sum);
    if (threadIdx.x == 0) rsum[blockIdx.x] = sum;
}

__global__ __launch_bounds__(BRR_WG) void dmx_brr_msum_kernel(const dmx_iblock* __restrict__ idx, uint32_t nblk,
                                                             const int32_t* __restrict__ diff,
                                                             int32_t* __restrict__ dsum, dmx_brr_head* head) {
    __shared__ int32_t sh[BRR_WG];
    const uint64_t m = (uint64_t)blockIdx.x * DMX_BRR_MTILE + threadIdx.x;
    int32_t v = 0;
    if (m < nblk) {
        v = diff[m];
        if (!dmx_brr_entry_ok(idx, (uint32_t)m)) DMX_BRR_OR(&head->invalid, 1u);
    }
    int32_t sum;
    brr_scan<int32_t>(v, 0, sh, dmx_brr_op_add(), &sum);
    if (threadIdx.x == 0) dsum[blockIdx.x] = sum;
}

__global__ __launch_bounds__(DMX_BRR_STHREADS) void dmx_brr_scan1_kernel(int32_t* __restrict__ dsum, uint32_t mtiles,
                                                                        uint64_t* __restrict__ rsum, uint32_t rtiles,
                                                                        dmx_brr_head* __restrict__ head) {
    __shared__ uint64_t sh[DMX_BRR_STHREADS];
    const uint32_t t = threadIdx.x;
    int32_t dtot;
    const int32_t dmine = dmx_brr_chunk_sum(dsum, mtiles, DMX_BRR_STHREADS, t, dmx_brr_op_add());
    const int32_t dbefore = brr_scan<int32_t>(dmine, 0, reinterpret_cast<int32_t*>(sh), dmx_brr_op_add(), &dtot);
    dmx_brr_chunk_apply(dsum, mtiles, DMX_BRR_STHREADS, t, dbefore, dmx_brr_op_add());
    uint64_t rtot;
    const uint64_t rmine = dmx_brr_chunk_sum(rsum, rtiles, DMX_BRR_STHREADS, t, dmx_brr_op_sat());
    const uint64_t rbefore = brr_scan<uint64_t>(rmine, 0, sh, dmx_brr_op_sat(), &rtot);
    dmx_brr_chunk_apply(rsum, rtiles, DMX_BRR_STHREADS, t, rbefore, dmx_brr_op_sat());
    if (t == 0) head->out_len = rtot;
}

// (diff[m] becomes need[m]: every word is read and written by its own thread only)
__global__ __launch_bounds__(BRR_WG) void dmx_brr_need_kernel(const dmx_iblock* __restrict__ idx, uint32_t nblk,
                                                             int32_t* __restrict__ diff,
                                                             const int32_t* __restrict__ dpre,
                                                             uint32_t* __restrict__ ncnt, uint64_t* __restrict__ nlen) {
    __shared__ uint64_t sh[BRR_WG];
    const uint64_t m = (uint64_t)blockIdx.x * DMX_BRR_MTILE + threadIdx.x;
    const int32_t v = m < nblk ? diff[m] : 0;
    int32_t dtot;
    const int32_t before = dpre[blockIdx.x] + brr_scan<int32_t>(v, 0, reinterpret_cast<int32_t*>(sh), dmx_brr_op_add(), &dtot);
    uint32_t need = 0;
    if (m < nblk) {
        need = dmx_brr_need(before, v);
        diff[m] = (int32_t)need;
    }
    uint32_t cnt;
    uint64_t len;
    brr_scan<uint32_t>(need, 0, reinterpret_cast<uint32_t*>(sh), dmx_brr_op_add(), &cnt);
    brr_scan<uint64_t>(need ? idx[m].out_len : 0u, 0, sh, dmx_brr_op_add(), &len);
    if (threadIdx.x == 0) {
        ncnt[blockIdx.x] = cnt;
        nlen[blockIdx.x] = len;
    }
}

__global__ __launch_bounds__(DMX_BRR_STHREADS) void dmx_brr_scan2_kernel(uint32_t* __restrict__ ncnt,
                                                                        uint64_t* __restrict__ nlen, uint32_t mtiles,
                                                                        uint32_t max_members, uint64_t scratch_bytes,
                                                                        uint64_t out_cap, dmx_brr_head* __restrict__ head,
                                                                        dmx_bgzf_ranges_status* __restrict__ rec) {
    __shared__ uint64_t sh[DMX_BRR_STHREADS];
    const uint32_t t = threadIdx.x;
    uint32_t ctot;
    const uint32_t cmine = dmx_brr_chunk_sum(ncnt, mtiles, DMX_BRR_STHREADS, t, dmx_brr_op_add());
    const uint32_t cbefore = brr_scan<uint32_t>(cmine, 0, reinterpret_cast<uint32_t*>(sh), dmx_brr_op_add(), &ctot);
    dmx_brr_chunk_apply(ncnt, mtiles, DMX_BRR_STHREADS, t, cbefore, dmx_brr_op_add());
    uint64_t ltot;
    const uint64_t lmine = dmx_brr_chunk_sum(nlen, mtiles, DMX_BRR_STHREADS, t, dmx_brr_op_add());
    const uint64_t lbefore = brr_scan<uint64_t>(lmine, 0, sh, dmx_brr_op_add(), &ltot);
    dmx_brr_chunk_apply(nlen, mtiles, DMX_BRR_STHREADS, t, lbefore, dmx_brr_op_add());
    if (t == 0) dmx_brr_decide(head, ctot, ltot, max_members, scratch_bytes, out_cap, rec);
}

// grid: tiles over the largest of nblk, max_members and nranges; every workgroup does its share of all three
__global__ __launch_bounds__(BRR_WG) void dmx_brr_emit_kernel(const dmx_iblock* __restrict__ idx,
                                                             const uint32_t* __restrict__ crc, uint32_t nblk,
                                                             const int32_t* __restrict__ need,
                                                             const uint32_t* __restrict__ npre,
                                                             const uint64_t* __restrict__ lpre, uint32_t mtiles,
                                                             const uint64_t* __restrict__ clen,
                                                             const uint64_t* __restrict__ rpre, uint32_t nranges,
                                                             uint32_t rtiles, uint32_t max_members,
                                                             const dmx_brr_head* __restrict__ head,
                                                             const dmx_bgzf_ranges_status* __restrict__ rec,
                                                             dmx_iblock* __restrict__ sub, uint32_t* __restrict__ subcrc,
                                                             uint64_t* __restrict__ moff, uint64_t* __restrict__ out_off) {
    __shared__ uint64_t sh[BRR_WG];
    const uint32_t count = head->count;
    const int32_t status = rec->status;
    const uint64_t i = (uint64_t)blockIdx.x * BRR_WG + threadIdx.x;
    if (blockIdx.x < mtiles && count) {   // (uniform over the workgroup)
        const uint32_t n = i < nblk ? (uint32_t)need[i] : 0u;
        uint32_t ctot;
        uint64_t ltot;
        const uint32_t rank = npre[blockIdx.x] + brr_scan<uint32_t>(n, 0, reinterpret_cast<uint32_t*>(sh), dmx_brr_op_add(), &ctot);
        const uint64_t soff = lpre[blockIdx.x] + brr_scan<uint64_t>(n ? idx[i].out_len : 0u, 0, sh, dmx_brr_op_add(), &ltot);
        if (n && rank < max_members) dmx_brr_emit_member(idx, crc, (uint32_t)i, rank, soff, sub, subcrc, moff);
    }
    if (i < max_members && i >= count) dmx_brr_emit_slot((uint32_t)i, sub, subcrc);
    if (blockIdx.x < rtiles && (status == 0 || status == -(int32_t)E_SZ)) {
        uint64_t tot;
        const uint64_t at = dmx_brr_sat(rpre[blockIdx.x],
                                        brr_scan<uint64_t>(i < nranges ? clen[i] : 0u, 0, sh, dmx_brr_op_sat(), &tot));
        if (i < nranges) out_off[i] = at;
        if (i == 0) out_off[nranges] = head->out_len;
    }
}

// A grid-stride loop over the aligned 16-byte groups of d_out.  One thread folds the decode's and the
// CRC pass's status into the record; every workgroup looks at both words, so none depends on that store.
__global__ __launch_bounds__(BRR_WG) void dmx_brr_gather_kernel(const dmx_brr_head* __restrict__ head,
                                                               dmx_bgzf_ranges_status* rec,
                                                               const uint64_t* __restrict__ out_off, uint32_t nranges,
                                                               const uint32_t* __restrict__ rm0,
                                                               const uint32_t* __restrict__ rdelta,
                                                               const uint64_t* __restrict__ moff,
                                                               const uint8_t* __restrict__ scratch,
                                                               uint8_t* __restrict__ out) {
    const int32_t s0 = rec->status, s1 = head->ist.status;
    if (s0 || s1) {
        if (!s0 && blockIdx.x == 0 && threadIdx.x == 0) rec->status = s1;
        return;
    }
    const uint64_t out_len = head->out_len;
    if (!out_len) return;
    const uint32_t hd = (uint32_t)(reinterpret_cast<uintptr_t>(out) & (DMX_BRR_GROUP - 1));
    const uint64_t ngroups = (hd + out_len + DMX_BRR_GROUP - 1) / DMX_BRR_GROUP;
    for (uint64_t g = (uint64_t)blockIdx.x * BRR_WG + threadIdx.x; g < ngroups; g += (uint64_t)gridDim.x * BRR_WG)
        dmx_brr_gather_group(g, hd, out_len, out_off, nranges, rm0, rdelta, moff, scratch, out);
}

extern "C" void dmx_bgzf_ranges_geometry(uint32_t* member_tile, uint32_t* range_tile) {
    if (member_tile) *member_tile = DMX_BRR_MTILE;
    if (range_tile) *range_tile = DMX_BRR_RTILE;
}

extern "C" uint64_t dmx_bgzf_ranges_work(uint32_t nblk, uint32_t nranges, uint32_t max_members, uint64_t scratch_bytes) {
    return brr_layout(nblk, nranges, max_members, scratch_bytes).bytes;
}

// compute units of the current device (the gather's grid)
static uint32_t brr_device_ncu(void) {
    static uint32_t ncu[64];
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256u;
    if (!ncu[dev])
        ncu[dev] = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0
                       ? (uint32_t)v : 256u;
    return ncu[dev];
}

extern "C" int dmx_bgzf_read_ranges_async(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, const uint32_t* d_crc,
                                          uint32_t nblk, const dmx_brange* d_ranges, uint32_t nranges, uint32_t flags,
                                          void* d_out, uint64_t out_cap, uint64_t* d_out_off, uint32_t max_members,
                                          uint64_t scratch_bytes, void* d_work, uint64_t work_bytes,
                                          dmx_bgzf_ranges_status* d_status, void* stream) {
    if (!d_status || !d_work || !d_out_off || (!d_z && zbytes) || (!d_index && nblk) || (!d_ranges && nranges) ||
        (!d_out && out_cap))
        return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_index) & 7) || (reinterpret_cast<uintptr_t>(d_ranges) & 7) ||
        (reinterpret_cast<uintptr_t>(d_out_off) & 7) || (reinterpret_cast<uintptr_t>(d_status) & 7) ||
        (reinterpret_cast<uintptr_t>(d_crc) & 3) || (reinterpret_cast<uintptr_t>(d_work) & 255))
        return -(int)E_INVAL;
    if (zbytes > 0xFFFFFFF0ull || nranges > 0x7FFFFFFFu || (flags & ~DMX_RANGES_VIRTUAL)) return -(int)E_RANGE;
    const BrrLayout L = brr_layout(nblk, nranges, max_members, scratch_bytes);
    if (work_bytes < L.bytes) return -(int)E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    if (!nranges || !nblk) {
        hipLaunchKernelGGL(dmx_brr_empty_kernel, dim3(nranges / BRR_WG + 1), dim3(BRR_WG), 0, s, d_out_off, nranges, d_status);
        return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
    }
    uint8_t* wk = static_cast<uint8_t*>(d_work);
    dmx_brr_head* head = reinterpret_cast<dmx_brr_head*>(wk);
    int32_t* diff = reinterpret_cast<int32_t*>(wk + L.o_diff);
    int32_t* dsum = reinterpret_cast<int32_t*>(wk + L.o_dsum);
    uint32_t* ncnt = reinterpret_cast<uint32_t*>(wk + L.o_ncnt);
    uint64_t* nlen = reinterpret_cast<uint64_t*>(wk + L.o_nlen);
    uint64_t* rsum = reinterpret_cast<uint64_t*>(wk + L.o_rsum);
    uint64_t* clen = reinterpret_cast<uint64_t*>(wk + L.o_clen);
    uint32_t* rm0 = reinterpret_cast<uint32_t*>(wk + L.o_rm0);
    uint32_t* rdelta = reinterpret_cast<uint32_t*>(wk + L.o_rdelta);
    uint64_t* moff = reinterpret_cast<uint64_t*>(wk + L.o_moff);
    dmx_iblock* sub = reinterpret_cast<dmx_iblock*>(wk + L.o_sub);
    uint32_t* subcrc = reinterpret_cast<uint32_t*>(wk + L.o_subcrc);
    uint8_t* scratch = wk + L.o_scratch;
    const uint8_t* z = static_cast<const uint8_t*>(d_z);

    hipLaunchKernelGGL(dmx_brr_reset_kernel, dim3(nblk / BRR_WG + 1), dim3(BRR_WG), 0, s, diff, nblk, head);
    hipLaunchKernelGGL(dmx_brr_plan_kernel, dim3(L.rtiles), dim3(BRR_WG), 0, s, z, zbytes, d_index, nblk, d_ranges, nranges,
                       flags, diff, clen, rm0, rdelta, rsum, head);
    hipLaunchKernelGGL(dmx_brr_msum_kernel, dim3(L.mtiles), dim3(BRR_WG), 0, s, d_index, nblk, (const int32_t*)diff, dsum, head);
    hipLaunchKernelGGL(dmx_brr_scan1_kernel, dim3(1), dim3(DMX_BRR_STHREADS), 0, s, dsum, L.mtiles, rsum, L.rtiles, head);
    hipLaunchKernelGGL(dmx_brr_need_kernel, dim3(L.mtiles), dim3(BRR_WG), 0, s, d_index, nblk, diff, (const int32_t*)dsum, ncnt,
                       nlen);
    hipLaunchKernelGGL(dmx_brr_scan2_kernel, dim3(1), dim3(DMX_BRR_STHREADS), 0, s, ncnt, nlen, L.mtiles, max_members,
                       scratch_bytes, out_cap, head, d_status);
    uint32_t etiles = L.mtiles > L.rtiles ? L.mtiles : L.rtiles;
    const uint32_t stiles = (uint32_t)(((uint64_t)max_members + BRR_WG - 1) / BRR_WG);
    if (stiles > etiles) etiles = stiles;
    hipLaunchKernelGGL(dmx_brr_emit_kernel, dim3(etiles), dim3(BRR_WG), 0, s, d_index, d_crc, nblk, (const int32_t*)diff,
                       (const uint32_t*)ncnt, (const uint64_t*)nlen, L.mtiles, (const uint64_t*)clen, (const uint64_t*)rsum,
                       nranges, L.rtiles, max_members, (const dmx_brr_head*)head, (const dmx_bgzf_ranges_status*)d_status, sub,
                       subcrc, moff, d_out_off);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    int r = dmx_inflate_counted_launch(d_z, zbytes, sub, max_members, &head->count, scratch, scratch_bytes, wk + L.o_tab,
                                       &head->ist, s);
    if (r) return r;
    if (d_crc && max_members) {
        r = dmx_crc32_ranges_launch(scratch, scratch_bytes, sub, max_members, NULL, subcrc, &head->ist, s);
        if (r) return r;
    }
    // enough workgroups to fill the device, no more than out_cap has groups
    const uint64_t cap_wg = (out_cap / DMX_BRR_GROUP + 2 + BRR_WG - 1) / BRR_WG;
    const uint64_t fill = 8ull * brr_device_ncu();
    hipLaunchKernelGGL(dmx_brr_gather_kernel, dim3((uint32_t)(cap_wg < fill ? cap_wg : fill)), dim3(BRR_WG), 0, s,
                       (const dmx_brr_head*)head, d_status, (const uint64_t*)d_out_off, nranges, (const uint32_t*)rm0,
                       (const uint32_t*)rdelta, (const uint64_t*)moff, (const uint8_t*)scratch, static_cast<uint8_t*>(d_out));
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    return 0;
}

// The convenience: plan with no capacities, the 32-byte record to the host, the real call sized by it.
extern "C" int dmx_bgzf_read_device(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, const uint32_t* d_crc,
                                    uint32_t nblk, const dmx_brange* d_ranges, uint32_t nranges, uint32_t flags, void* d_out,
                                    uint64_t out_cap, uint64_t* d_out_off, uint64_t* out_len, int verify, void* stream) {
    if (!out_len || !d_out_off || (!d_z && zbytes) || (!d_index && nblk) || (!d_ranges && nranges) || (!d_out && out_cap) ||
        (verify && nblk && !d_crc))
        return -(int)E_INVAL;
    *out_len = 0;
    if ((reinterpret_cast<uintptr_t>(d_index) & 7) || (reinterpret_cast<uintptr_t>(d_ranges) & 7) ||
        (reinterpret_cast<uintptr_t>(d_out_off) & 7) || (reinterpret_cast<uintptr_t>(d_crc) & 3))
        return -(int)E_INVAL;
    if (zbytes > 0xFFFFFFF0ull || nranges > 0x7FFFFFFFu || (flags & ~DMX_RANGES_VIRTUAL)) return -(int)E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t* crc = verify ? d_crc : NULL;
    dmx_bgzf_ranges_status st;
    uint32_t max_members = 0;
    uint64_t scratch_bytes = 0, cap = 0;
    int r = 0;
    for (int pass = 0; pass < 2 && !r; pass++) {   // [record | work]
        const uint64_t wb = dmx_bgzf_ranges_work(nblk, nranges, max_members, scratch_bytes);
        uint8_t* buf = static_cast<uint8_t*>(dmx_itab_scratch(s, 256 + wb));
        if (!buf) return -(int)E_MALLOC;
        r = dmx_bgzf_read_ranges_async(d_z, zbytes, d_index, crc, nblk, d_ranges, nranges, flags, pass ? d_out : NULL, cap,
                                       d_out_off, max_members, scratch_bytes, buf + 256, wb,
                                       reinterpret_cast<dmx_bgzf_ranges_status*>(buf), s);
        if (!r && (hip_fail(hipMemcpyAsync(&st, buf, sizeof(st), hipMemcpyDeviceToHost, s), "D2H(ranges status)") ||
                   hip_fail(hipStreamSynchronize(s), "hipStreamSynchronize")))
            r = -(int)E_DEVICE;
        (void)hipFreeAsync(buf, s);
        if (r) break;
        if (pass == 0 && st.status == -(int)E_SZ) {   // planned: the needs are known
            *out_len = st.out_len;
            if (st.out_len > out_cap) return -(int)E_SZ;
            max_members = st.nmembers;
            scratch_bytes = st.scratch_len;
            cap = out_cap;
            continue;
        }
        r = st.status;   // pass 0: nothing to decode (0), or the plan's status; pass 1: the call's
        if (!r) *out_len = st.out_len;
        break;
    }
    return r;
}

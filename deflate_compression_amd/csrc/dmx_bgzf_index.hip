// dmx_bgzf_index.hip -- the block index of a BGZF file that lies in device memory, built on the
// device (include/dmx.h: dmx_bgzf_index_async, dmx_bgzf_decode_device).
//
// The host walk (dmx_bgzf_index_max) follows the members by their BSIZE: a chain of dependent
// loads.  Here every byte of the file is looked at instead:
//   1. dmx_bgzf_count_kernel   a workgroup per 16 KiB tile of aligned 16-byte groups: the positions
//                              that parse as a member (dmx_bgzf_step: the walk's own step), counted
//   2. dmx_bgzf_plan_kernel    one workgroup: the exclusive scan of the tile counts, the walk's step
//                              at offset 0, the decision whether the work buffer holds the
//                              candidates, and the reset of the status record
//   3. dmx_bgzf_write_kernel   the tiles that hold candidates, again: the candidates in offset order
//   4. dmx_bgzf_link_kernel    a thread per candidate: its successor by binary search (or the end,
//                              or the status of the walk there), and the first mark on node 0
//   5. dmx_bgzf_round_kernel   ceil(log2(bound + 1)) launches of marked-prefix pointer doubling: the
//                              nodes of the chain from offset 0 receive their rank and output offset
//   6. dmx_bgzf_finish_kernel  the marked nodes write their entries; the last one the record
// The per-thread work of every stage is in dmx_bgzf_step.h, which the host twin
// (tests/c/bgzf_dindex_model.cpp) runs as loops under the sanitizers.  Nothing here depends on
// the order in which threads or atomics run: the one atomic is an integer sum in LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dmx.h"
#include "dmx_bgzf_step.h"
#include "dmx_ctx.h"

#define BIX_WG 256                              // threads per workgroup of every kernel but the plan
#define BIX_TILE_GROUPS 1024u                   // aligned groups per tile: 4 per thread
#define BIX_TILE (BIX_TILE_GROUPS * DMX_BGZF_GROUP)   // 16 KiB
#define BIX_PLAN_WG 1024

static_assert(sizeof(dmx_bgzf_istat) == sizeof(dmx_bgzf_index_status) && sizeof(dmx_bgzf_istat) == 24, "status record");
static_assert(sizeof(dmx_bgzf_cand) == 24 && sizeof(dmx_bgzf_node) == 16 && sizeof(dmx_bgzf_mark) == 16, "work layout");

// the head of the work buffer (256 bytes): what the plan kernel decided
struct BixPlan {
    uint32_t n;       // nodes of the doubling: the candidates, or 0 where the record is final already
    uint32_t total;   // positions that parsed
};

// The work buffer: [plan | tile offsets (ntiles + 1) | cand (m + 1) | node a (m + 1) | node b (m + 1) | mark (m + 1)],
// every part 256-byte aligned, m = the candidates it holds.
struct BixLayout {
    uint64_t o_tile, o_cand, o_na, o_nb, o_mark, bytes;
    uint64_t ngroups, ntiles;
    uint32_t head;
};
static inline uint64_t bix_a256(uint64_t x) { return (x + 255) & ~255ull; }
static BixLayout bix_layout(uintptr_t z, uint64_t zbytes, uint64_t m) {
    BixLayout L;
    L.head = (uint32_t)(z & (DMX_BGZF_GROUP - 1));
    // (for the size of the buffer the worst alignment counts: one group more)
    L.ngroups = zbytes ? (L.head + zbytes + DMX_BGZF_GROUP - 1) / DMX_BGZF_GROUP : 0;
    L.ntiles = L.ngroups ? (L.ngroups + BIX_TILE_GROUPS - 1) / BIX_TILE_GROUPS : 1;
    const uint64_t tiles_cap = (zbytes / DMX_BGZF_GROUP + 2 + BIX_TILE_GROUPS - 1) / BIX_TILE_GROUPS + 1;
    L.o_tile = 256;
    L.o_cand = L.o_tile + bix_a256((tiles_cap + 1) * 4);
    L.o_na = L.o_cand + bix_a256((m + 1) * sizeof(dmx_bgzf_cand));
    L.o_nb = L.o_na + bix_a256((m + 1) * sizeof(dmx_bgzf_node));
    L.o_mark = L.o_nb + bix_a256((m + 1) * sizeof(dmx_bgzf_node));
    L.bytes = L.o_mark + bix_a256((m + 1) * sizeof(dmx_bgzf_mark));
    return L;
}

// the five words of aligned group g of the file's groups: its own four and the first of the next
__device__ static inline void bix_load(const uint4* __restrict__ base, uint64_t g, uint64_t ngroups, uint32_t w[5]) {
    const uint4 v = base[g];
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
    w[4] = g + 1 < ngroups ? reinterpret_cast<const uint32_t*>(base + g + 1)[0] : 0u;
}

__global__ __launch_bounds__(BIX_WG) void dmx_bgzf_count_kernel(const uint8_t* __restrict__ z, uint64_t zlen,
                                                               uint32_t max_isize, uint32_t head, uint64_t ngroups,
                                                               uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const uint4* base = reinterpret_cast<const uint4*>(z - head);
    uint32_t n = 0;
    for (uint32_t it = 0; it < BIX_TILE_GROUPS / BIX_WG; it++) {
        const uint64_t g = (uint64_t)blockIdx.x * BIX_TILE_GROUPS + it * BIX_WG + threadIdx.x;
        if (g >= ngroups) break;
        uint32_t w[5];
        bix_load(base, g, ngroups, w);
        n += dmx_bgzf_group(z, zlen, max_isize, head, g, w, nullptr, 0);
    }
    if (n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// exclusive scan over the workgroup (blockDim.x a multiple of 64, at most 1024): returns the sum
// of v over the threads before this one, *sum = over all
__device__ static inline uint32_t bix_block_scan(uint32_t v, uint32_t* sh /* 17 words */, uint32_t* sum) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();   // (sh may still be read from the call before)
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < nw; k++) {
            const uint32_t t = sh[k];
            sh[k] = run;
            run += t;
        }
        sh[16] = run;
    }
    __syncthreads();
    *sum = sh[16];
    return sh[wv] + inc - v;
}

__global__ __launch_bounds__(BIX_PLAN_WG) void dmx_bgzf_plan_kernel(const uint8_t* __restrict__ z, uint64_t zlen,
                                                                   uint32_t max_isize, uint32_t ntiles, uint32_t max_cand,
                                                                   uint32_t* __restrict__ tile, BixPlan* __restrict__ plan,
                                                                   dmx_bgzf_istat* __restrict__ st) {
    __shared__ uint32_t sh[17];
    // tile[t] = count of tile t -> the candidates before tile t; tile[ntiles] = all
    const uint32_t per = (ntiles + BIX_PLAN_WG - 1) / BIX_PLAN_WG;
    const uint64_t t0 = (uint64_t)threadIdx.x * per;
    const uint64_t t1 = t0 + per < ntiles ? t0 + per : ntiles;
    uint32_t mine = 0;
    for (uint64_t t = t0; t < t1; t++) mine += tile[t];
    uint32_t total;
    uint32_t run = bix_block_scan(mine, sh, &total);
    for (uint64_t t = t0; t < t1; t++) {
        const uint32_t c = tile[t];
        tile[t] = run;
        run += c;
    }
    if (threadIdx.x == 0) {
        tile[ntiles] = total;
        dmx_bgzf_istat r = {0, 0, 0, total, 0};
        uint32_t n = total;
        dmx_bgzf_member m;
        const int e0 = zlen ? dmx_bgzf_step(z, zlen, 0, max_isize, &m) : 0;
        if (e0) {   // the walk ends at its first step
            r.status = e0;
            n = 0;
        } else if (total > max_cand) {   // more candidates than the work buffer holds
            r.status = -(int)E_SZ;
            n = 0;
        }
        plan->n = n;
        plan->total = total;
        *st = r;   // (final where n == 0: an empty file indexes to nothing)
    }
}

__global__ __launch_bounds__(BIX_WG) void dmx_bgzf_write_kernel(const uint8_t* __restrict__ z, uint64_t zlen,
                                                               uint32_t max_isize, uint32_t head, uint64_t ngroups,
                                                               const uint32_t* __restrict__ tile,
                                                               const BixPlan* __restrict__ plan,
                                                               dmx_bgzf_cand* __restrict__ cand) {
    __shared__ uint32_t sh[17];
    const uint32_t n = plan->n;
    uint32_t at = tile[blockIdx.x];
    const uint32_t end = tile[blockIdx.x + 1];
    if (!n || at == end) return;   // (uniform over the workgroup)
    const uint4* base = reinterpret_cast<const uint4*>(z - head);
    for (uint32_t it = 0; it < BIX_TILE_GROUPS / BIX_WG; it++) {
        const uint64_t g = (uint64_t)blockIdx.x * BIX_TILE_GROUPS + it * BIX_WG + threadIdx.x;
        uint32_t w[5] = {0, 0, 0, 0, 0};
        uint32_t c = 0;
        if (g < ngroups) {
            bix_load(base, g, ngroups, w);
            c = dmx_bgzf_group(z, zlen, max_isize, head, g, w, nullptr, 0);
        }
        uint32_t sum;
        const uint32_t before = bix_block_scan(c, sh, &sum);
        // (end <= n: were the file to change between the launches, nothing is written past the tile's share)
        const uint32_t to = at + before;
        if (c && to < end) dmx_bgzf_group(z, zlen, max_isize, head, g, w, cand + to, end - to);
        at += sum;
    }
}

__global__ __launch_bounds__(BIX_WG) void dmx_bgzf_link_kernel(const uint8_t* __restrict__ z, uint64_t zlen,
                                                              uint32_t max_isize, const BixPlan* __restrict__ plan,
                                                              dmx_bgzf_cand* __restrict__ cand,
                                                              dmx_bgzf_node* __restrict__ node,
                                                              dmx_bgzf_mark* __restrict__ mark) {
    const uint32_t n = plan->n;
    const uint64_t i = (uint64_t)blockIdx.x * BIX_WG + threadIdx.x;
    if (!n || i > n) return;
    dmx_bgzf_link(z, zlen, max_isize, cand, n, (uint32_t)i, node, mark);
}

__global__ __launch_bounds__(BIX_WG) void dmx_bgzf_round_kernel(const BixPlan* __restrict__ plan,
                                                               const dmx_bgzf_node* a, dmx_bgzf_node* b,
                                                               dmx_bgzf_mark* mark, uint32_t k) {
    const uint32_t n = plan->n;
    const uint64_t i = (uint64_t)blockIdx.x * BIX_WG + threadIdx.x;
    if (!n || i > n) return;
    dmx_bgzf_round(a, b, mark, n, (uint32_t)i, k);
}

__global__ __launch_bounds__(BIX_WG) void dmx_bgzf_finish_kernel(const BixPlan* __restrict__ plan,
                                                                const dmx_bgzf_cand* __restrict__ cand,
                                                                const dmx_bgzf_mark* __restrict__ mark, uint64_t zlen,
                                                                dmx_iblock* __restrict__ idx, uint32_t* __restrict__ crc,
                                                                uint32_t cap, dmx_bgzf_istat* __restrict__ st) {
    const uint32_t n = plan->n;
    const uint64_t i = (uint64_t)blockIdx.x * BIX_WG + threadIdx.x;
    if (i >= n) return;
    dmx_bgzf_finish(cand, mark, n, (uint32_t)i, zlen, idx, crc, cap, st);
}

extern "C" void dmx_bgzf_index_geometry(uint32_t* tile) {
    if (tile) *tile = BIX_TILE;
}

extern "C" uint64_t dmx_bgzf_index_work(uint64_t zbytes, uint32_t max_cand) {
    return bix_layout(0, zbytes, max_cand).bytes;
}

// the candidates a work buffer of work_bytes holds (work_bytes >= dmx_bgzf_index_work(zbytes, 1))
static uint32_t bix_max_cand(uint64_t zbytes, uint64_t work_bytes) {
    uint64_t lo = 1, hi = 0xFFFFFFFFull;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (bix_layout(0, zbytes, mid).bytes <= work_bytes) lo = mid;
        else hi = mid - 1;
    }
    return (uint32_t)lo;
}

extern "C" int dmx_bgzf_index_async(const void* d_z, uint64_t zbytes, uint32_t max_isize, dmx_iblock* d_index,
                                    uint32_t* d_crc, uint32_t cap, void* d_work, uint64_t work_bytes,
                                    dmx_bgzf_index_status* d_status, void* stream) {
    if ((!d_z && zbytes) || !d_status || (!d_index && cap) || !d_work) return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_index) & 7) || (reinterpret_cast<uintptr_t>(d_crc) & 3) ||
        (reinterpret_cast<uintptr_t>(d_work) & 255) || (reinterpret_cast<uintptr_t>(d_status) & 7))
        return -(int)E_INVAL;
    if (max_isize < 1 || max_isize > DMX_BGZF_MAX_ISIZE || zbytes > 0xFFFFFFF0ull) return -(int)E_RANGE;
    if (work_bytes < dmx_bgzf_index_work(zbytes, 1)) return -(int)E_INVAL;
    uint32_t max_cand = bix_max_cand(zbytes, work_bytes);
    // no two candidates lie less than three bytes apart (1F 8B 08 does not overlap itself)
    if (max_cand > zbytes / 3 + 1) max_cand = (uint32_t)(zbytes / 3 + 1);
    const BixLayout L = bix_layout(reinterpret_cast<uintptr_t>(d_z), zbytes, max_cand);
    uint8_t* wk = static_cast<uint8_t*>(d_work);
    BixPlan* plan = reinterpret_cast<BixPlan*>(wk);
    uint32_t* tile = reinterpret_cast<uint32_t*>(wk + L.o_tile);
    dmx_bgzf_cand* cand = reinterpret_cast<dmx_bgzf_cand*>(wk + L.o_cand);
    dmx_bgzf_node* na = reinterpret_cast<dmx_bgzf_node*>(wk + L.o_na);
    dmx_bgzf_node* nb = reinterpret_cast<dmx_bgzf_node*>(wk + L.o_nb);
    dmx_bgzf_mark* mark = reinterpret_cast<dmx_bgzf_mark*>(wk + L.o_mark);
    dmx_bgzf_istat* st = reinterpret_cast<dmx_bgzf_istat*>(d_status);
    const uint8_t* z = static_cast<const uint8_t*>(d_z);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t ntiles = (uint32_t)L.ntiles;
    const uint32_t nodes_wg = (uint32_t)(((uint64_t)max_cand + 1 + BIX_WG - 1) / BIX_WG);
    // the chain from offset 0 has at most `bound` nodes: a member is 26 bytes or more
    const uint64_t bound = max_cand < zbytes / 26 + 1 ? max_cand : zbytes / 26 + 1;
    uint32_t rounds = 0;
    while ((1ull << rounds) < bound + 1) rounds++;

    hipLaunchKernelGGL(dmx_bgzf_count_kernel, dim3(ntiles), dim3(BIX_WG), 0, s, z, zbytes, max_isize, L.head, L.ngroups, tile);
    hipLaunchKernelGGL(dmx_bgzf_plan_kernel, dim3(1), dim3(BIX_PLAN_WG), 0, s, z, zbytes, max_isize, ntiles, max_cand, tile,
                       plan, st);
    hipLaunchKernelGGL(dmx_bgzf_write_kernel, dim3(ntiles), dim3(BIX_WG), 0, s, z, zbytes, max_isize, L.head, L.ngroups,
                       (const uint32_t*)tile, (const BixPlan*)plan, cand);
    hipLaunchKernelGGL(dmx_bgzf_link_kernel, dim3(nodes_wg), dim3(BIX_WG), 0, s, z, zbytes, max_isize, (const BixPlan*)plan,
                       cand, na, mark);
    for (uint32_t k = 0; k < rounds; k++) {
        hipLaunchKernelGGL(dmx_bgzf_round_kernel, dim3(nodes_wg), dim3(BIX_WG), 0, s, (const BixPlan*)plan,
                           (const dmx_bgzf_node*)na, nb, mark, k);
        dmx_bgzf_node* t = na;
        na = nb;
        nb = t;
    }
    hipLaunchKernelGGL(dmx_bgzf_finish_kernel, dim3(nodes_wg), dim3(BIX_WG), 0, s, (const BixPlan*)plan,
                       (const dmx_bgzf_cand*)cand, (const dmx_bgzf_mark*)mark, zbytes, d_index, d_crc, cap, st);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    return 0;
}

// The device-to-device decode: the index above with the format's own bound on a member into pool
// scratch, its 24-byte record to the host (the member count sizes the inflate's grid and table
// scratch), then dmx_inflate_members_async.
extern "C" int dmx_bgzf_decode_device(const void* d_z, uint64_t zbytes, void* d_out, uint64_t out_cap, uint64_t* out_len,
                                      int verify, void* stream) {
    if ((!d_z && zbytes) || !out_len || (!d_out && out_cap)) return -(int)E_INVAL;
    *out_len = 0;
    if (zbytes > 0xFFFFFFF0ull) return -(int)E_RANGE;
    if (!zbytes) return 0;
    hipStream_t s = (hipStream_t)stream;
    uint64_t max_cand = zbytes / 256 + 1024;
    dmx_bgzf_index_status st;
    uint8_t* buf = nullptr;
    uint64_t o_idx = 0, o_crc = 0, o_ist = 0;
    int r = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (max_cand > zbytes / 3 + 1) max_cand = zbytes / 3 + 1;
        const uint64_t wb = dmx_bgzf_index_work(zbytes, (uint32_t)max_cand);
        o_idx = 256 + wb;   // [index record | work | index | CRCs | inflate record]
        o_crc = o_idx + bix_a256(max_cand * sizeof(dmx_iblock));
        o_ist = o_crc + bix_a256(max_cand * 4);
        buf = static_cast<uint8_t*>(dmx_itab_scratch(s, o_ist + 256));
        if (!buf) return -(int)E_MALLOC;
        r = dmx_bgzf_index_async(d_z, zbytes, DMX_BGZF_MAX_ISIZE, reinterpret_cast<dmx_iblock*>(buf + o_idx),
                                 reinterpret_cast<uint32_t*>(buf + o_crc), (uint32_t)max_cand, buf + 256, wb,
                                 reinterpret_cast<dmx_bgzf_index_status*>(buf), s);
        if (!r && (hip_fail(hipMemcpyAsync(&st, buf, sizeof(st), hipMemcpyDeviceToHost, s), "D2H(index status)") ||
                   hip_fail(hipStreamSynchronize(s), "hipStreamSynchronize")))
            r = -(int)E_DEVICE;
        if (!r && st.status == -(int)E_SZ && st.ncand > max_cand && attempt == 0) {   // look-alikes: once more, with room
            (void)hipFreeAsync(buf, s);
            max_cand = st.ncand;
            continue;
        }
        if (!r) r = st.status;
        break;
    }
    if (!r) {
        *out_len = st.out_len;
        if (st.out_len > out_cap) r = -(int)E_SZ;
    }
    if (!r && st.nblk) {
        dmx_inflate_status ist = {0, 0, 0};
        dmx_inflate_status* d_ist = reinterpret_cast<dmx_inflate_status*>(buf + o_ist);
        r = dmx_inflate_members_async(d_z, zbytes, reinterpret_cast<const dmx_iblock*>(buf + o_idx), st.nblk, d_out,
                                      st.out_len, verify ? reinterpret_cast<const uint32_t*>(buf + o_crc) : NULL, d_ist, s);
        if (!r && (hip_fail(hipMemcpyAsync(&ist, d_ist, sizeof(ist), hipMemcpyDeviceToHost, s), "D2H(status)") ||
                   hip_fail(hipStreamSynchronize(s), "hipStreamSynchronize")))
            r = -(int)E_DEVICE;
        if (!r && ist.status) r = ist.status;
        if (!r && ist.out_len != st.out_len) r = -(int)E_LEN;
    }
    (void)hipFreeAsync(buf, s);
    return r;
}

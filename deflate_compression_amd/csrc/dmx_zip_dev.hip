// dmx_zip_dev.hip -- the index of a ZIP archive that lies in device memory, built on the device
// (include/dmx.h: dmx_zip_index_async).
//
// The host walk (dmx_zip_index_host) finds the end record, follows the central directory header by
// header -- a chain of dependent loads -- and for every header loads the local header it names: a
// second dependent load somewhere else in the file.  Here, as in dmx_bgzf_index.hip:
//   1. dmx_zip_tail_kernel    one workgroup over the last 65 557 bytes: every lane tests positions
//                             for PK\5\6, the last match wins through an integer maximum in LDS (the
//                             fast rule -- the last 22 bytes -- is tested first by one lane); the
//                             locator and the ZIP64 record are parsed and cd_begin, cd_end, nentries,
//                             concat or the file's status published in the plan; the record is reset
//   2. dmx_zip_count_kernel   a workgroup per 16 KiB tile of aligned 16-byte groups of the central
//                             directory (not of the file: tiles behind cd_end leave at once; the
//                             grid is sized for a directory as large as the file, since its size is
//                             only known on the device): the positions that pass dmx_zip_cd_step
//   3. dmx_zip_plan_kernel    one workgroup: the exclusive scan of the tile counts, the step at
//                             cd_begin, the decision whether the work buffer holds the candidates
//   4. dmx_zip_write_kernel   the tiles that hold candidates, again: the candidates in offset order.
//                             Names, extras and comments may hold bytes that parse as headers; such
//                             look-alikes are candidates too, and the chain tells them apart
//   5. dmx_zip_link_kernel    a thread per candidate: its successor by binary search, or the end
//   6. dmx_zip_round_kernel   ceil(log2(bound + 1)) launches of marked-prefix pointer doubling: the
//                             nodes of the chain from cd_begin receive their rank
//   7. dmx_zip_decide_kernel  the chain's last node: exactly nentries headers, ending at cd_end?
//   8. dmx_zip_finish_kernel  a thread per chain node: the ZIP64 extra and the local header -- the
//                             load that makes the host walk slow is nentries independent loads
//                             here -- and the entry at its rank; the decoded lengths are summed
//   9. dmx_zip_scan_kernel    one workgroup: out_off, the exclusive scan of usize over the entries
//                             with status 0, and the final record
// The per-thread work of every stage is in dmx_zip.h, which the host twin (tests/c/zip_model.cpp)
// runs as loops under the sanitizers.  The grid of every launch follows from zbytes, cap and the
// work buffer's size, never from a value read back.  Nothing depends on the order in which threads
// or atomics run: the atomics are an integer maximum and an integer sum in LDS and one 64-bit
// integer sum in global memory.  All stores to global memory are ordinary vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dmx.h"
#include "dmx_zip.h"
#include "dmx_ctx.h"

#define ZIX_WG 256                              // threads per workgroup of the per-tile and per-node kernels
#define ZIX_TILE_GROUPS 1024u                   // aligned groups per tile: 4 per thread
#define ZIX_TILE (ZIX_TILE_GROUPS * DMX_ZIP_GROUP)   // 16 KiB
#define ZIX_ONE_WG 1024                         // threads of the one-workgroup kernels

static_assert(sizeof(dmx_zip_entry) == 64 && sizeof(dmx_zip_status) == 40, "record layout");
static_assert(sizeof(dmx_zip_cand) == 16 && sizeof(dmx_zip_node) == 8 && sizeof(dmx_zip_mark) == 8, "work layout");

// the head of the work buffer (256 bytes): what the tail and plan kernels decided
struct ZixPlan {
    dmx_zip_tail tail;
    uint32_t n;       // nodes of the doubling: the candidates, or 0 where the record is final already
    uint32_t total;   // positions that parsed
    int32_t status;   // the file's status so far
    uint32_t ok;      // 1: the chain is the directory (dmx_zip_decide_kernel)
    unsigned long long out_len;   // sum of usize over the chain's entries with status 0
};

// The work buffer: [plan | tile offsets (ntiles + 1) | cand (m + 1) | node a (m + 1) | node b (m + 1) | mark (m + 1)],
// every part 256-byte aligned, m = the candidates it holds.
struct ZixLayout {
    uint64_t o_tile, o_cand, o_na, o_nb, o_mark, bytes;
    uint64_t ngroups, ntiles;
    uint32_t head;
};
static inline uint64_t zix_a256(uint64_t x) { return (x + 255) & ~255ull; }
static ZixLayout zix_layout(uintptr_t z, uint64_t zbytes, uint64_t m) {
    ZixLayout L;
    L.head = (uint32_t)(z & (DMX_ZIP_GROUP - 1));
    L.ngroups = zbytes ? (L.head + zbytes + DMX_ZIP_GROUP - 1) / DMX_ZIP_GROUP : 0;
    L.ntiles = L.ngroups ? (L.ngroups + ZIX_TILE_GROUPS - 1) / ZIX_TILE_GROUPS : 1;
    // (for the size of the buffer the worst alignment counts: one group more)
    const uint64_t tiles_cap = (zbytes / DMX_ZIP_GROUP + 2 + ZIX_TILE_GROUPS - 1) / ZIX_TILE_GROUPS + 1;
    L.o_tile = 256;
    L.o_cand = L.o_tile + zix_a256((tiles_cap + 1) * 4);
    L.o_na = L.o_cand + zix_a256((m + 1) * sizeof(dmx_zip_cand));
    L.o_nb = L.o_na + zix_a256((m + 1) * sizeof(dmx_zip_node));
    L.o_mark = L.o_nb + zix_a256((m + 1) * sizeof(dmx_zip_node));
    L.bytes = L.o_mark + zix_a256((m + 1) * sizeof(dmx_zip_mark));
    return L;
}

__global__ __launch_bounds__(ZIX_ONE_WG) void dmx_zip_tail_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                                 ZixPlan* __restrict__ plan, dmx_zip_status* __restrict__ st) {
    __shared__ uint32_t best;   // 1 + the last position of PK\5\6 in the window, 0: none
    if (threadIdx.x == 0) best = 0;
    __syncthreads();
    if (zbytes >= 4 && zbytes <= DMX_ZIP_MAXZ) {
        const uint64_t lo = dmx_zip_tail_lo(zbytes);
        uint32_t mine = 0;
        for (uint64_t p = lo + threadIdx.x; p + 4 <= zbytes; p += ZIX_ONE_WG)
            if (dmx_zip_end_sig(z, p)) mine = (uint32_t)p + 1;
        if (mine) atomicMax(&best, mine);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t eocd = ~0ull;
        if (zbytes <= DMX_ZIP_MAXZ) {
            if (dmx_zip_end_fast(z, zbytes)) eocd = zbytes - DMX_ZIP_EOCD;
            else if (best) eocd = best - 1;
        }
        dmx_zip_tail t;
        dmx_zip_end_parse(z, zbytes, eocd, &t);
        plan->tail = t;
        plan->n = 0;
        plan->total = 0;
        plan->status = t.status;
        plan->ok = 0;
        plan->out_len = 0;
        dmx_zip_status r = {t.status, 0, 0, t.cd_begin, t.cd_end - t.cd_begin, 0, 0};
        *st = r;
    }
}

// the five words of aligned group g of the file's groups: its own four and the first of the next
__device__ static inline void zix_load(const uint4* __restrict__ base, uint64_t g, uint64_t ngroups, uint32_t w[5]) {
    const uint4 v = base[g];
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
    w[4] = g + 1 < ngroups ? reinterpret_cast<const uint32_t*>(base + g + 1)[0] : 0u;
}

// the groups of the directory: the first, and one behind the last (equal: none)
__device__ static inline void zix_span(const ZixPlan* plan, uint32_t head, uint64_t* g0, uint64_t* g1) {
    const uint64_t b = plan->tail.cd_begin, e = plan->tail.cd_end;
    *g0 = (head + b) / DMX_ZIP_GROUP;
    *g1 = plan->status || e - b < DMX_ZIP_CDH ? *g0 : (head + e - 1) / DMX_ZIP_GROUP + 1;
}

__global__ __launch_bounds__(ZIX_WG) void dmx_zip_count_kernel(const uint8_t* __restrict__ z, uint32_t head, uint64_t ngroups,
                                                              const ZixPlan* __restrict__ plan,
                                                              uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    uint64_t g0, g1;
    zix_span(plan, head, &g0, &g1);
    const uint4* base = reinterpret_cast<const uint4*>(z - head);
    uint32_t n = 0;
    for (uint32_t it = 0; it < ZIX_TILE_GROUPS / ZIX_WG; it++) {
        const uint64_t g = g0 + (uint64_t)blockIdx.x * ZIX_TILE_GROUPS + it * ZIX_WG + threadIdx.x;
        if (g >= g1 || g >= ngroups) break;
        uint32_t w[5];
        zix_load(base, g, ngroups, w);
        n += dmx_zip_group(z, plan->tail.cd_begin, plan->tail.cd_end, head, g, w, nullptr, 0);
    }
    if (n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// exclusive scan over the workgroup (blockDim.x a multiple of 64, at most 1024): returns the sum
// of v over the threads before this one, *sum = over all
template <typename T>
__device__ static inline T zix_block_scan(T v, T* sh /* 17 words */, T* sum) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    T inc = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();   // (sh may still be read from the call before)
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = 0;
        for (uint32_t k = 0; k < nw; k++) {
            const T t = sh[k];
            sh[k] = run;
            run += t;
        }
        sh[16] = run;
    }
    __syncthreads();
    *sum = sh[16];
    return sh[wv] + inc - v;
}

__global__ __launch_bounds__(ZIX_ONE_WG) void dmx_zip_plan_kernel(const uint8_t* __restrict__ z, uint32_t ntiles,
                                                                 uint32_t max_cand, uint32_t* __restrict__ tile,
                                                                 ZixPlan* __restrict__ plan) {
    __shared__ uint32_t sh[17];
    // tile[t] = count of tile t -> the candidates before tile t; tile[ntiles] = all
    const uint32_t per = (ntiles + ZIX_ONE_WG - 1) / ZIX_ONE_WG;
    const uint64_t t0 = (uint64_t)threadIdx.x * per;
    const uint64_t t1 = t0 + per < ntiles ? t0 + per : ntiles;
    uint32_t mine = 0;
    for (uint64_t t = t0; t < t1; t++) mine += tile[t];
    uint32_t total;
    uint32_t run = zix_block_scan<uint32_t>(mine, sh, &total);
    for (uint64_t t = t0; t < t1; t++) {
        const uint32_t c = tile[t];
        tile[t] = run;
        run += c;
    }
    if (threadIdx.x == 0) {
        tile[ntiles] = total;
        const dmx_zip_tail t = plan->tail;
        uint32_t n = total;
        int32_t status = t.status;
        if (status) {
            n = 0;
        } else if (!t.nentries) {   // no entry: then no directory
            if (t.cd_begin != t.cd_end) status = -(int)E_LEN;
            n = 0;
        } else if (t.cd_begin == t.cd_end || !dmx_zip_cd_step(z, t.cd_end, t.cd_begin)) {   // the walk ends at its first step
            status = -(int)E_LEN;
            n = 0;
        } else if (total > max_cand) {   // more candidates than the work buffer holds
            status = -(int)E_SZ;
            n = 0;
        }
        plan->n = n;
        plan->total = total;
        plan->status = status;
    }
}

__global__ __launch_bounds__(ZIX_WG) void dmx_zip_write_kernel(const uint8_t* __restrict__ z, uint32_t head, uint64_t ngroups,
                                                              const uint32_t* __restrict__ tile,
                                                              const ZixPlan* __restrict__ plan,
                                                              dmx_zip_cand* __restrict__ cand) {
    __shared__ uint32_t sh[17];
    const uint32_t n = plan->n;
    uint32_t at = tile[blockIdx.x];
    const uint32_t end = tile[blockIdx.x + 1];
    if (!n || at == end) return;   // (uniform over the workgroup)
    uint64_t g0, g1;
    zix_span(plan, head, &g0, &g1);
    const uint4* base = reinterpret_cast<const uint4*>(z - head);
    for (uint32_t it = 0; it < ZIX_TILE_GROUPS / ZIX_WG; it++) {
        const uint64_t g = g0 + (uint64_t)blockIdx.x * ZIX_TILE_GROUPS + it * ZIX_WG + threadIdx.x;
        uint32_t w[5] = {0, 0, 0, 0, 0};
        uint32_t c = 0;
        if (g < g1 && g < ngroups) {
            zix_load(base, g, ngroups, w);
            c = dmx_zip_group(z, plan->tail.cd_begin, plan->tail.cd_end, head, g, w, nullptr, 0);
        }
        uint32_t sum;
        const uint32_t before = zix_block_scan<uint32_t>(c, sh, &sum);
        // (end <= n: were the file to change between the launches, nothing is written past the tile's share)
        const uint32_t to = at + before;
        if (c && to < end) dmx_zip_group(z, plan->tail.cd_begin, plan->tail.cd_end, head, g, w, cand + to, end - to);
        at += sum;
    }
}

__global__ __launch_bounds__(ZIX_WG) void dmx_zip_link_kernel(const ZixPlan* __restrict__ plan, dmx_zip_cand* __restrict__ cand,
                                                             dmx_zip_node* __restrict__ node,
                                                             dmx_zip_mark* __restrict__ mark) {
    const uint32_t n = plan->n;
    const uint64_t i = (uint64_t)blockIdx.x * ZIX_WG + threadIdx.x;
    if (!n || i > n) return;
    dmx_zip_link(plan->tail.cd_begin, plan->tail.cd_end, cand, n, (uint32_t)i, node, mark);
}

__global__ __launch_bounds__(ZIX_WG) void dmx_zip_round_kernel(const ZixPlan* __restrict__ plan, const dmx_zip_node* a,
                                                              dmx_zip_node* b, dmx_zip_mark* mark, uint32_t k) {
    const uint32_t n = plan->n;
    const uint64_t i = (uint64_t)blockIdx.x * ZIX_WG + threadIdx.x;
    if (!n || i > n) return;
    dmx_zip_round(a, b, mark, n, (uint32_t)i, k);
}

__global__ __launch_bounds__(ZIX_WG) void dmx_zip_decide_kernel(ZixPlan* plan, const dmx_zip_cand* __restrict__ cand,
                                                               const dmx_zip_mark* __restrict__ mark) {
    const uint32_t n = plan->n;
    const uint64_t i = (uint64_t)blockIdx.x * ZIX_WG + threadIdx.x;
    if (i >= n) return;
    const int v = dmx_zip_decide(cand, mark, (uint32_t)i, plan->tail.nentries);   // (non-zero in one thread)
    if (v > 0) plan->ok = 1;
    else if (v < 0) plan->status = -(int)E_LEN;
}

__global__ __launch_bounds__(ZIX_WG) void dmx_zip_finish_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                               ZixPlan* plan, const dmx_zip_cand* __restrict__ cand,
                                                               const dmx_zip_mark* __restrict__ mark,
                                                               dmx_zip_entry* __restrict__ entries, uint32_t cap) {
    const uint32_t n = plan->ok ? plan->n : 0;
    const uint64_t i = (uint64_t)blockIdx.x * ZIX_WG + threadIdx.x;
    unsigned long long len = 0;
    if (i < n && mark[i].round) {
        dmx_zip_entry e;
        dmx_zip_finish(z, zbytes, plan->tail.concat, cand[i].off, &e);
        len = dmx_zip_len(&e);
        const uint32_t r = mark[i].c;
        if (r < cap) entries[r] = e;
    }
    for (int o = 32; o >= 1; o >>= 1) len += __shfl_xor(len, o, 64);   // (every lane of the wave is here)
    if ((threadIdx.x & 63) == 0 && len) atomicAdd(&plan->out_len, len);
}

__global__ __launch_bounds__(ZIX_ONE_WG) void dmx_zip_scan_kernel(const ZixPlan* __restrict__ plan,
                                                                 dmx_zip_entry* __restrict__ entries, uint32_t cap,
                                                                 dmx_zip_status* __restrict__ st) {
    __shared__ unsigned long long sh[17];
    const dmx_zip_tail t = plan->tail;
    const uint32_t count = !plan->ok ? 0 : t.nentries < cap ? t.nentries : cap;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < count; base += ZIX_ONE_WG) {
        const uint64_t i = base + threadIdx.x;
        const unsigned long long v = i < count ? dmx_zip_len(&entries[i]) : 0;
        unsigned long long sum;
        const unsigned long long before = zix_block_scan<unsigned long long>(v, sh, &sum);
        if (i < count) entries[i].out_off = carry + before;
        carry += sum;
    }
    if (threadIdx.x == 0) {
        dmx_zip_status r = {plan->status, 0, 0, t.cd_begin, t.cd_end - t.cd_begin, 0, 0};
        if (plan->ok) {
            r.nentries = t.nentries;
            r.out_len = plan->out_len;
            if (t.nentries > cap) r.status = -(int)E_SZ;
        } else if (!plan->status && t.nentries) {   // (not reached: a chain with a first node has a last one)
            r.status = -(int)E_LEN;
        } else if (plan->status == -(int)E_SZ) {
            r.ncand = plan->total;
        }
        *st = r;
    }
}

extern "C" void dmx_zip_index_geometry(uint32_t* tile) {
    if (tile) *tile = ZIX_TILE;
}

extern "C" uint64_t dmx_zip_index_work(uint64_t zbytes, uint32_t max_cand) {
    return zix_layout(0, zbytes, max_cand).bytes;
}

// the candidates a work buffer of work_bytes holds (work_bytes >= dmx_zip_index_work(zbytes, 1))
static uint32_t zix_max_cand(uint64_t zbytes, uint64_t work_bytes) {
    uint64_t lo = 1, hi = 0xFFFFFFFFull;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (zix_layout(0, zbytes, mid).bytes <= work_bytes) lo = mid;
        else hi = mid - 1;
    }
    return (uint32_t)lo;
}

extern "C" int dmx_zip_index_async(const void* d_z, uint64_t zbytes, dmx_zip_entry* d_entries, uint32_t cap, void* d_work,
                                   uint64_t work_bytes, dmx_zip_status* d_status, void* stream) {
    if ((!d_z && zbytes) || !d_status || (!d_entries && cap) || !d_work) return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_entries) & 7) || (reinterpret_cast<uintptr_t>(d_work) & 255) ||
        (reinterpret_cast<uintptr_t>(d_status) & 7))
        return -(int)E_INVAL;
    if (zbytes > DMX_ZIP_MAXZ) return -(int)E_RANGE;
    if (work_bytes < dmx_zip_index_work(zbytes, 1)) return -(int)E_INVAL;
    uint32_t max_cand = zix_max_cand(zbytes, work_bytes);
    // no two candidates lie less than four bytes apart (PK\1\2 does not overlap itself)
    if (max_cand > zbytes / 4 + 1) max_cand = (uint32_t)(zbytes / 4 + 1);
    const ZixLayout L = zix_layout(reinterpret_cast<uintptr_t>(d_z), zbytes, max_cand);
    uint8_t* wk = static_cast<uint8_t*>(d_work);
    ZixPlan* plan = reinterpret_cast<ZixPlan*>(wk);
    uint32_t* tile = reinterpret_cast<uint32_t*>(wk + L.o_tile);
    dmx_zip_cand* cand = reinterpret_cast<dmx_zip_cand*>(wk + L.o_cand);
    dmx_zip_node* na = reinterpret_cast<dmx_zip_node*>(wk + L.o_na);
    dmx_zip_node* nb = reinterpret_cast<dmx_zip_node*>(wk + L.o_nb);
    dmx_zip_mark* mark = reinterpret_cast<dmx_zip_mark*>(wk + L.o_mark);
    const uint8_t* z = static_cast<const uint8_t*>(d_z);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t ntiles = (uint32_t)L.ntiles;
    const uint32_t nodes_wg = (uint32_t)(((uint64_t)max_cand + 1 + ZIX_WG - 1) / ZIX_WG);
    // the chain from cd_begin has at most `bound` nodes: a header is 46 bytes or more
    const uint64_t bound = max_cand < zbytes / DMX_ZIP_CDH + 1 ? max_cand : zbytes / DMX_ZIP_CDH + 1;
    uint32_t rounds = 0;
    while ((1ull << rounds) < bound + 1) rounds++;

    hipLaunchKernelGGL(dmx_zip_tail_kernel, dim3(1), dim3(ZIX_ONE_WG), 0, s, z, zbytes, plan, d_status);
    hipLaunchKernelGGL(dmx_zip_count_kernel, dim3(ntiles), dim3(ZIX_WG), 0, s, z, L.head, L.ngroups, (const ZixPlan*)plan, tile);
    hipLaunchKernelGGL(dmx_zip_plan_kernel, dim3(1), dim3(ZIX_ONE_WG), 0, s, z, ntiles, max_cand, tile, plan);
    hipLaunchKernelGGL(dmx_zip_write_kernel, dim3(ntiles), dim3(ZIX_WG), 0, s, z, L.head, L.ngroups, (const uint32_t*)tile,
                       (const ZixPlan*)plan, cand);
    hipLaunchKernelGGL(dmx_zip_link_kernel, dim3(nodes_wg), dim3(ZIX_WG), 0, s, (const ZixPlan*)plan, cand, na, mark);
    for (uint32_t k = 0; k < rounds; k++) {
        hipLaunchKernelGGL(dmx_zip_round_kernel, dim3(nodes_wg), dim3(ZIX_WG), 0, s, (const ZixPlan*)plan,
                           (const dmx_zip_node*)na, nb, mark, k);
        dmx_zip_node* t = na;
        na = nb;
        nb = t;
    }
    hipLaunchKernelGGL(dmx_zip_decide_kernel, dim3(nodes_wg), dim3(ZIX_WG), 0, s, plan, (const dmx_zip_cand*)cand,
                       (const dmx_zip_mark*)mark);
    hipLaunchKernelGGL(dmx_zip_finish_kernel, dim3(nodes_wg), dim3(ZIX_WG), 0, s, z, zbytes, plan, (const dmx_zip_cand*)cand,
                       (const dmx_zip_mark*)mark, d_entries, cap);
    hipLaunchKernelGGL(dmx_zip_scan_kernel, dim3(1), dim3(ZIX_ONE_WG), 0, s, (const ZixPlan*)plan, d_entries, cap, d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    return 0;
}

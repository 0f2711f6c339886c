// dmx_zip_read.inc -- the decode of a selection of a ZIP archive's entries (include/dmx.h:
// dmx_zip_read_async; DESIGN.md §3.7).  Included by dmx_inflate_dev.hip behind the batch decode,
// whose kernel, claim counter, tables and grid it uses as they are: a deflated entry is one raw
// stream of a batch.
//   1. dmx_inflate_batch_clear_kernel   the claim counter and the summary
//   2. dmx_zip_prepare_kernel   one workgroup: the selected entries' lengths, their exclusive sum
//                               (d_offsets) and the dmx_bstream table.  A deflated entry is
//                               (data_off, csize) into a window of usize bytes.  Any other gets
//                               in_off = ZRD_STORED or ZRD_BAD, which lies behind every file, so the
//                               batch kernel gives it -E_RANGE before it reads or writes a byte;
//                               in_len then carries the source offset of a stored entry, or the
//                               status of one that is not decoded.  A total above out_bytes makes
//                               every entry ZRD_BAD with -E_SZ
//   3. dmx_inflate_batch_kernel<false>  the raw streams, a wave each
//   4. dmx_zip_copy_kernel      the stored entries: a workgroup per 64 KiB span of the output finds
//                               the entries that overlap it by binary search in d_offsets and
//                               copies its share of each, so one large stored entry is spread over
//                               many workgroups
//   5. dmx_zip_fix_kernel       a thread per entry: the result so far (the decoder's status, -E_LEN
//                               where fewer than usize bytes came out, the stored entries, the
//                               statuses prepare decided); under DMX_ZIP_VERIFY an entry that
//                               stands is dressed as a gzip member with the stored CRC-32 for the
//                               next launch.  Thread 0 resets the summary: the batch kernel counted
//                               what is no stream as failed
//   6. dmx_crc32_batch_launch   (DMX_ZIP_VERIFY) -E_CRC, and the summary of the entries it checks
//   7. dmx_zip_final_kernel     format = the method, check = the stored CRC-32, and the summary of
//                               the entries the CRC pass did not count (integer sums and a minimum)
#define ZRD_STORED 0xFFFFFFFFFFFFFFFFull
#define ZRD_BAD 0xFFFFFFFFFFFFFFFEull
#define ZRD_WG 256
#define ZRD_PREP_WG 1024
#define ZRD_SPAN 65536u        // bytes of output per workgroup of the copy kernel
#define ZRD_MAX_GRID 1048576u
#define ZRD_MAX_LEN (1ull << 43)   // above what DEFLATE makes of 0xFFFFFFF0 bytes (1032 : 1): such an entry is -E_RANGE

struct ZrdCtl {   // in the first 256 bytes of d_work, behind IBatchCtl
    unsigned long long total;   // d_offsets[nsel]
    uint32_t over;              // total > out_bytes: nothing is decoded
};
#define ZRD_CTL_OFF 64

// the selected entry of slot k, and what is decoded of it: 0 a raw stream, 1 stored bytes, else a status
__device__ static inline int zrd_pick(const dmx_zip_entry* __restrict__ entries, uint32_t nentries,
                                      const uint32_t* __restrict__ sel, uint32_t k, uint64_t zbytes, dmx_zip_entry* e) {
    const uint32_t j = sel ? sel[k] : k;
    if (j >= nentries) {
        memset(e, 0, sizeof(*e));
        return -(int)E_RANGE;
    }
    *e = entries[j];
    if (e->status) return e->status;
    if (e->method != 0 && e->method != 8) return -(int)E_ZCMPMT;   // (an index gives these a status)
    if (e->data_off > zbytes || e->csize > zbytes - e->data_off || e->usize > ZRD_MAX_LEN) return -(int)E_RANGE;
    if (e->method == 0) return e->csize == e->usize ? 1 : -(int)E_LEN;
    return 0;
}

template <typename T>
__device__ static inline T zrd_block_scan(T v, T* sh /* 17 words */, T* sum) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    T inc = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();
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

__device__ static inline unsigned long long zrd_sat_add(unsigned long long a, unsigned long long b) {
    return a > ~0ull - b ? ~0ull : a + b;
}

__global__ __launch_bounds__(ZRD_PREP_WG) void dmx_zip_prepare_kernel(const dmx_zip_entry* __restrict__ entries, uint32_t nentries,
                                                                     const uint32_t* __restrict__ sel, uint32_t nsel,
                                                                     uint64_t zbytes, uint64_t out_bytes,
                                                                     uint64_t* __restrict__ offsets,
                                                                     dmx_bstream* __restrict__ streams,
                                                                     ZrdCtl* __restrict__ zc) {
    __shared__ unsigned long long sh[17];
    unsigned long long carry = 0;   // (saturating: a sum that passes 2^64 is above every out_bytes)
    for (uint64_t base = 0; base < nsel; base += ZRD_PREP_WG) {
        const uint64_t k = base + threadIdx.x;
        unsigned long long len = 0;
        dmx_bstream b = {ZRD_BAD, 0, 0, 0};
        if (k < nsel) {
            dmx_zip_entry e;
            const int kind = zrd_pick(entries, nentries, sel, (uint32_t)k, zbytes, &e);
            if (kind == 0) {
                b.in_off = e.data_off;
                b.in_len = e.csize;
                len = e.usize;
            } else if (kind == 1) {
                b.in_off = ZRD_STORED;
                b.in_len = e.data_off;
                len = e.usize;
            } else {
                b.in_len = (uint64_t)(int64_t)kind;
            }
            b.out_cap = len;
        }
        // (len <= ZRD_MAX_LEN: the sum over a workgroup's 1024 entries cannot wrap; the carry saturates)
        unsigned long long sum;
        const unsigned long long before = zrd_block_scan<unsigned long long>(len, sh, &sum);
        const unsigned long long off = zrd_sat_add(carry, before);
        if (k < nsel) {
            b.out_off = off;
            offsets[k] = off;
            streams[k] = b;
        }
        carry = zrd_sat_add(carry, sum);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        offsets[nsel] = carry;
        zc->total = carry;
        zc->over = carry > out_bytes ? 1u : 0u;
    }
    // too small an output: no entry is decoded (the same thread wrote streams[k] above)
    if (carry > out_bytes)
        for (uint64_t k = threadIdx.x; k < nsel; k += ZRD_PREP_WG) {
            dmx_bstream b = {ZRD_BAD, (uint64_t)(int64_t)(-(int)E_SZ), offsets[k], 0};
            streams[k] = b;
        }
}

// n bytes from s to d by the threads of the workgroup: 16-byte stores to the aligned part of d, fed
// by 16-byte loads -- one where s and d agree modulo 16, else the two aligned groups that hold the
// 16 source bytes, shifted together; single bytes at both ends.  Only aligned groups that hold
// source bytes are loaded.
__device__ static inline void zrd_copy(uint8_t* __restrict__ d, const uint8_t* __restrict__ s, uint64_t n) {
    const uint32_t tid = threadIdx.x;
    uint64_t hb = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;
    if (hb > n) hb = n;
    if (tid < hb) d[tid] = s[tid];
    const uint64_t nv = (n - hb) / 16;
    uint4* dv = reinterpret_cast<uint4*>(d + hb);
    const uint8_t* sb = s + hb;
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(sb) & 15);
    if (!shift) {
        const uint4* sv = reinterpret_cast<const uint4*>(sb);
        for (uint64_t i = tid; i < nv; i += ZRD_WG) dv[i] = sv[i];
    } else {
        const uint4* sv = reinterpret_cast<const uint4*>(sb - shift);
        const uint32_t sw = shift >> 2, bits = 8 * (shift & 3);
        for (uint64_t i = tid; i < nv; i += ZRD_WG) {
            const uint4 a = sv[i], b = sv[i + 1];   // (b holds source bytes 16 - shift .. 15 of this vector)
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t o[4];
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) {
                const uint32_t lo = sw == 0 ? w[q] : sw == 1 ? w[q + 1] : sw == 2 ? w[q + 2] : w[q + 3];
                const uint32_t hi = sw == 0 ? w[q + 1] : sw == 1 ? w[q + 2] : sw == 2 ? w[q + 3] : w[q + 4];
                o[q] = (uint32_t)((((uint64_t)hi << 32) | lo) >> bits);
            }
            dv[i] = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
    const uint64_t done = hb + 16 * nv;
    if (tid < n - done) d[done + tid] = s[done + tid];
}

__global__ __launch_bounds__(ZRD_WG) void dmx_zip_copy_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                             const dmx_bstream* __restrict__ streams, uint32_t nsel,
                                                             const uint64_t* __restrict__ offsets, uint8_t* __restrict__ out,
                                                             uint64_t out_bytes, const ZrdCtl* __restrict__ zc) {
    if (zc->over) return;
    const uint64_t total = zc->total;   // (<= out_bytes)
    for (uint64_t t0 = (uint64_t)blockIdx.x * ZRD_SPAN; t0 < total; t0 += (uint64_t)gridDim.x * ZRD_SPAN) {
        const uint64_t t1 = total - t0 < ZRD_SPAN ? total : t0 + ZRD_SPAN;
        uint32_t lo = 0, hi = nsel;   // the first entry that ends behind t0
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (offsets[mid + 1] <= t0) lo = mid + 1;
            else hi = mid;
        }
        for (uint32_t k = lo; k < nsel; k++) {
            const uint64_t o0 = offsets[k], o1 = offsets[k + 1];
            if (o0 >= t1) break;
            const dmx_bstream b = streams[k];
            if (b.in_off != ZRD_STORED || o1 <= o0) continue;
            const uint64_t a = o0 > t0 ? o0 : t0, e = o1 < t1 ? o1 : t1;
            // (prepare checked [in_len, in_len + usize) against the file, and usize == o1 - o0)
            if (b.in_len > zbytes || o1 - o0 > zbytes - b.in_len || e > out_bytes) continue;
            zrd_copy(out + a, z + b.in_len + (a - o0), e - a);
        }
    }
}

__global__ __launch_bounds__(ZRD_WG) void dmx_zip_fix_kernel(const dmx_zip_entry* __restrict__ entries, uint32_t nentries,
                                                            const uint32_t* __restrict__ sel, uint32_t nsel,
                                                            const dmx_bstream* __restrict__ streams, int verify,
                                                            dmx_bresult* __restrict__ res, dmx_batch_status* __restrict__ st) {
    const uint64_t k = (uint64_t)blockIdx.x * ZRD_WG + threadIdx.x;
    if (k == 0) {   // (no thread of this launch counts)
        st->nfailed = 0;
        st->first_bad = 0xFFFFFFFFu;
        st->total_out = 0;
    }
    if (k >= nsel) return;
    const dmx_bstream b = streams[k];
    dmx_bresult r = res[k];
    if (b.in_off == ZRD_BAD) {
        r.status = (int32_t)(int64_t)b.in_len;
    } else if (b.in_off == ZRD_STORED) {
        r.status = 0;
        r.out_len = b.out_cap;
        r.in_used = b.out_cap;
    } else if (!r.status && r.out_len != b.out_cap) {
        r.status = -(int)E_LEN;
    }
    r.reserved = 0;
    if (r.status) {
        r.out_len = 0;
        r.in_used = 0;
        r.check = 0;
        r.format = 0;
    } else {
        const uint32_t j = sel ? sel[k] : (uint32_t)k;   // (< nentries: the entry was picked)
        r.check = entries[j].crc;
        r.format = verify ? DMX_BATCH_GZIP : 0u;
    }
    res[k] = r;
}

__global__ __launch_bounds__(ZRD_WG) void dmx_zip_final_kernel(const dmx_zip_entry* __restrict__ entries, uint32_t nentries,
                                                              const uint32_t* __restrict__ sel, uint32_t nsel, int verify,
                                                              dmx_bresult* __restrict__ res, dmx_batch_status* __restrict__ st,
                                                              const ZrdCtl* __restrict__ zc) {
    const uint64_t k = (uint64_t)blockIdx.x * ZRD_WG + threadIdx.x;
    if (k == 0 && zc->over) atomicAdd((unsigned long long*)&st->total_out, zc->total);   // the bytes needed
    if (k >= nsel) return;
    const uint32_t j = sel ? sel[k] : (uint32_t)k;
    const int32_t status = res[k].status;
    res[k].format = j < nentries ? entries[j].method : 0u;
    // the CRC pass counted the entries it checked: those that stand, and those it failed
    const bool counted = verify && (status == 0 || status == -(int)E_CRC);
    if (counted) return;
    if (status) {
        atomicAdd(&st->nfailed, 1u);
        atomicMin(&st->first_bad, (uint32_t)k);
    } else {
        atomicAdd((unsigned long long*)&st->total_out, (unsigned long long)res[k].out_len);
    }
}

extern "C" void dmx_zip_read_geometry(uint32_t* span) {
    if (span) *span = ZRD_SPAN;
}

// d_work: [IBatchCtl + ZrdCtl, 256 B][the batch decode's tables][the dmx_bstream table]
extern "C" uint64_t dmx_zip_read_work(uint32_t nsel) {
    return dmx_inflate_batch_work(nsel) + ((32ull * nsel + 255) & ~255ull);
}

extern "C" int dmx_zip_read_async(const void* d_z, uint64_t zbytes, const dmx_zip_entry* d_entries, uint32_t nentries,
                                  const uint32_t* d_sel, uint32_t nsel, uint32_t flags, void* d_out, uint64_t out_bytes,
                                  uint64_t* d_offsets, dmx_bresult* d_results, void* d_work, uint64_t work_bytes,
                                  dmx_batch_status* d_status, void* stream) {
    if (!d_results || !d_status || !d_work || !d_offsets || (!d_entries && nentries) || (!d_z && zbytes) ||
        (!d_out && out_bytes) || (!d_sel && nsel != nentries))
        return -(int)E_INVAL;
    if (((uintptr_t)d_entries & 7) || ((uintptr_t)d_offsets & 7) || ((uintptr_t)d_results & 7) || ((uintptr_t)d_status & 7) ||
        ((uintptr_t)d_sel & 3))
        return -(int)E_INVAL;
    if (((uintptr_t)d_work & 255) || work_bytes < dmx_zip_read_work(nsel)) return -(int)E_INVAL;
    if ((flags & ~DMX_ZIP_VERIFY) || zbytes > 0xFFFFFFF0ull) return -(int)E_RANGE;
    const int verify = (flags & DMX_ZIP_VERIFY) != 0;
    hipStream_t s = (hipStream_t)stream;
    IBatchCtl* ctl = (IBatchCtl*)d_work;
    ZrdCtl* zc = (ZrdCtl*)((uint8_t*)d_work + ZRD_CTL_OFF);
    uint32_t* gtab = (uint32_t*)((uint8_t*)d_work + 256);
    dmx_bstream* streams = (dmx_bstream*)((uint8_t*)d_work + dmx_inflate_batch_work(nsel));
    hipLaunchKernelGGL(dmx_inflate_batch_clear_kernel, dim3(1), dim3(1), 0, s, ctl, d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    if (!nsel) {
        hipLaunchKernelGGL(dmx_zip_prepare_kernel, dim3(1), dim3(ZRD_PREP_WG), 0, s, d_entries, nentries, d_sel, 0u, zbytes,
                           out_bytes, d_offsets, streams, zc);   // d_offsets[0] = 0
        return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
    }
    const uint32_t resident = ibatch_resident();
    if (!resident) return -(int)E_DEVICE;
    const uint32_t grid = nsel < resident ? nsel : resident;
    const uint32_t per_wg = (nsel + ZRD_WG - 1) / ZRD_WG;
    uint64_t spans = (out_bytes + ZRD_SPAN - 1) / ZRD_SPAN;
    if (spans > ZRD_MAX_GRID) spans = ZRD_MAX_GRID;
    const IBatchDict none = {nullptr, 0, nullptr, nullptr, nullptr, 0};
    hipLaunchKernelGGL(dmx_zip_prepare_kernel, dim3(1), dim3(ZRD_PREP_WG), 0, s, d_entries, nentries, d_sel, nsel, zbytes,
                       out_bytes, d_offsets, streams, zc);
    hipLaunchKernelGGL(dmx_inflate_batch_kernel<false>, dim3(grid), dim3(64), 0, s, (const uint8_t*)d_z, zbytes,
                       (const dmx_bstream*)streams, nsel, (uint32_t)DMX_BATCH_RAW, (uint8_t*)d_out, out_bytes, d_results, gtab,
                       ctl, d_status, none);
    if (spans)
        hipLaunchKernelGGL(dmx_zip_copy_kernel, dim3((uint32_t)spans), dim3(ZRD_WG), 0, s, (const uint8_t*)d_z, zbytes,
                           (const dmx_bstream*)streams, nsel, (const uint64_t*)d_offsets, (uint8_t*)d_out, out_bytes,
                           (const ZrdCtl*)zc);
    hipLaunchKernelGGL(dmx_zip_fix_kernel, dim3(per_wg), dim3(ZRD_WG), 0, s, d_entries, nentries, d_sel, nsel,
                       (const dmx_bstream*)streams, verify, d_results, d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    if (verify) {
        const int r = dmx_crc32_batch_launch(d_out, out_bytes, streams, nsel, d_results, d_status, s);
        if (r) return r;
    }
    hipLaunchKernelGGL(dmx_zip_final_kernel, dim3(per_wg), dim3(ZRD_WG), 0, s, d_entries, nentries, d_sel, nsel, verify,
                       d_results, d_status, (const ZrdCtl*)zc);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

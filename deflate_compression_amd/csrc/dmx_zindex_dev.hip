// dmx_zindex_dev.hip -- the seek-point index of one foreign stream from its one-pass decode
// (dmx_zindex_from_parallel_async, include/dmx.h; DESIGN.md 3.1 "Seek points from the one-pass
// decode").  When dmx_inflate_parallel_decode_async ends, the live chunks in the plan buffer are
// true block boundaries with exact bits and output ranges, and d_out holds every window and every
// point's bytes: the index is a selection of chunks, a copy of 32 KiB per point and one read of
// the output.  Four launches over d_work = [control 256][piece bases 4 x (npoints + 1)][piece sums
// 8 x pieces] (dmx_zs_work; every offset follows from the device-side npoints):
//   select   one wave: the decode's record, the capacity checks, then the rule of dmx_zsel.h over
//            the live chunks, 64 at a time -- a lane tests a chunk, the lowest lane that begins a
//            point is taken, the test runs again from it -- once to count, once to write the points
//            and the piece bases (base[k]: the 64 KiB pieces of the points before k)
//   windows  a workgroup per quarter slot: 16 bytes a thread, the source at any alignment
//   fold     a workgroup per piece of a point: the sums (a, b) of the piece from a = b = 0 with
//            position weights, as dmx_par_check_kernel's, from 16-byte loads; the point of a piece
//            by a search over the bases
//   finish   a thread per point combines its pieces into the Adler-32; thread 0 writes the record
// Neither d_plan nor d_out is written.  A workgroup beyond the device-side counts leaves at once;
// after a status only select writes (the record).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dmx.h"
#include "dmx_pfind.h"   // the plan buffer's sizes
#include "dmx_zsel.h"    // the selection rule, the work buffer's sizes

#define ZX_W DMX_ZINDEX_WINDOW
#define ZX_T 256u             // threads of windows, fold and finish
#define ZX_WIN_MAX_WG 4096u
#define ZX_FOLD_MAX_WG 4096u
static_assert(ZX_W == 4 * 2 * ZX_T * 16, "a quarter slot is two 16-byte groups a thread");
static_assert(DMX_ZS_PIECE == ZX_T * 256u, "a piece is 16 groups a thread, one more where it begins off a group");

struct ZCtl {   // the first 256 bytes of d_work
    uint32_t go, npoints, span, format;
    uint64_t out_len, in_used;
    uint32_t check, pieces;
};
static_assert(sizeof(ZCtl) <= 256 && sizeof(dmx_zindex_status) == 40 && sizeof(dmx_zpoint) == 32, "d_work's head, the record");

__device__ __forceinline__ uint32_t* zx_base(uint8_t* work) { return (uint32_t*)(work + 256); }
__device__ __forceinline__ uint2* zx_sums(uint8_t* work, uint32_t npoints) {
    return (uint2*)(work + 256 + dmx_zs_a256(4ull * npoints + 4));
}

// dmx_zs_select's walk by one wave.  A tile of 64 chunks: every lane holds its chunk's out_off and
// bit; the ballot of dmx_zs_starts names the chunks that would begin a point behind the current
// one, the lowest does, and the lanes above it are asked again against the new start.  The loop
// runs once per point and once per tile.  Returns npoints; WRITE: lane 0 stores points[0, npoints)
// and base[0, npoints].
template <bool WRITE>
__device__ uint32_t zx_walk(const dmx_pchunk* __restrict__ chunks, uint32_t nlive, uint32_t span, dmx_zpoint* __restrict__ points,
                            uint32_t* __restrict__ base) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t k = 0;
    uint64_t cur_off = chunks[0].out_off, cur_bit = chunks[0].bit, pieces = 0;
    for (uint32_t t = 0; t < nlive; t += 64) {
        const uint32_t c = t + lane;
        const bool in = c > 0 && c < nlive;
        const uint64_t off = in ? chunks[c].out_off : 0, bit = in ? chunks[c].bit : 0;
        unsigned long long m = __ballot(in && dmx_zs_starts(off, cur_off, span));
        while (m) {
            const int j = __ffsll(m) - 1;
            const uint64_t noff = __shfl(off, j), nbit = __shfl(bit, j);
            if (WRITE && lane == 0) {
                points[k].bit = cur_bit;
                points[k].end_bit = nbit;
                points[k].out_off = cur_off;
                points[k].out_len = noff - cur_off;
                base[k] = (uint32_t)pieces;
            }
            pieces += dmx_zs_pieces(noff - cur_off);
            k++;
            cur_off = noff;
            cur_bit = nbit;
            // (a lane at or below j holds an offset at or below the new start: the difference would wrap)
            m = __ballot(in && lane > (uint32_t)j && dmx_zs_starts(off, cur_off, span));
        }
    }
    const uint64_t end = chunks[nlive - 1].out_off + chunks[nlive - 1].out_len;
    if (WRITE && lane == 0) {
        points[k].bit = cur_bit;
        points[k].end_bit = chunks[nlive - 1].end_bit;
        points[k].out_off = cur_off;
        points[k].out_len = end - cur_off;
        base[k] = (uint32_t)pieces;
        base[k + 1] = (uint32_t)(pieces + dmx_zs_pieces(end - cur_off));
    }
    return k + 1;
}

__global__ __launch_bounds__(64) void dmx_zx_select_kernel(const dmx_pchunk* __restrict__ chunks, uint64_t plan_bytes,
                                                           const dmx_par_status* __restrict__ dec, uint64_t out_cap,
                                                           uint32_t max_live, uint32_t span, uint32_t max_points,
                                                           uint64_t work_bytes, dmx_zpoint* __restrict__ points,
                                                           uint8_t* __restrict__ work, dmx_zindex_status* __restrict__ st_out) {
    ZCtl* ctl = (ZCtl*)work;
    const dmx_par_status d = *dec;
    dmx_zindex_status st;
    st.status = d.status;
    st.format = d.format;
    st.out_len = st.in_used = 0;
    st.check = st.npoints = st.reserved = 0;
    st.span = span;
    bool go = false;
    if (!d.status) {
        // a record that is not this plan's and this output's: nothing below may trust its numbers
        if (!d.nlive || d.nlive > max_live || d.out_len > out_cap || plan_bytes < 256 + 32ull * d.nlive ||
            chunks[d.nlive - 1].out_off + chunks[d.nlive - 1].out_len != d.out_len) {
            st.status = -(int32_t)E_INVAL;
        } else {
            st.npoints = zx_walk<false>(chunks, d.nlive, span, nullptr, nullptr);
            st.out_len = d.out_len;
            if (st.npoints > max_points || work_bytes < dmx_zs_work(d.out_len, st.npoints)) {
                st.status = -(int32_t)E_SZ;   // the record holds the needed npoints
            } else {
                go = true;
                zx_walk<true>(chunks, d.nlive, span, points, zx_base(work));
            }
        }
    }
    if (threadIdx.x == 0) {
        ctl->go = go ? 1u : 0u;
        ctl->npoints = st.npoints;
        ctl->span = span;
        ctl->format = d.format;
        ctl->out_len = d.out_len;
        ctl->in_used = d.in_used;
        ctl->check = d.check;
        ctl->pieces = go ? zx_base(work)[st.npoints] : 0u;
        if (!go) *st_out = st;
    }
}

// 16 bytes of the slot of a point at out_off, from byte p of the slot (a multiple of 16): zeros
// before byte `zeros` = 32768 - wlen, out[out_off - 32768 + p ...] from there on.  Where the 16 bytes
// are all output and the one or two aligned 16-byte groups that hold them lie inside out[0, n),
// those are loaded whole and shifted together; at the edges single bytes are.
__device__ __forceinline__ void zx_window_group(const uint8_t* __restrict__ out, uint64_t n, uint64_t out_off,
                                                uint8_t* __restrict__ slot, uint32_t p, uint32_t zeros) {
    uint64_t o0 = 0, o1 = 0;
    if (p + 16 > zeros) {
        const uint64_t s = out_off + p - ZX_W;   // (wraps while p < zeros: used only for the bytes behind them)
        const uint8_t* a = out + s;
        const uint32_t r = (uint32_t)((uintptr_t)a & 15u);
        if (p >= zeros && s >= r && s - r + (r ? 32u : 16u) <= n) {
            const uint4 lo = *reinterpret_cast<const uint4*>(a - r);
            const uint4 hi = r ? *reinterpret_cast<const uint4*>(a - r + 16) : make_uint4(0, 0, 0, 0);
            const uint64_t w0 = lo.x | ((uint64_t)lo.y << 32), w1 = lo.z | ((uint64_t)lo.w << 32);
            const uint64_t w2 = hi.x | ((uint64_t)hi.y << 32), w3 = hi.z | ((uint64_t)hi.w << 32);
            const bool up = r & 8u;
            const uint32_t sh = (r & 7u) * 8;
            const uint64_t x0 = up ? w1 : w0, x1 = up ? w2 : w1, x2 = up ? w3 : w2;
            o0 = sh ? (x0 >> sh) | (x1 << (64 - sh)) : x0;
            o1 = sh ? (x1 >> sh) | (x2 << (64 - sh)) : x1;
        } else {
            for (uint32_t j = 0; j < 16; j++) {
                const uint64_t v = p + j >= zeros ? out[s + j] : 0u;
                if (j < 8) o0 |= v << (8 * j);
                else o1 |= v << (8 * (j - 8));
            }
        }
    }
    if (((uintptr_t)slot & 15u) == 0) {
        *reinterpret_cast<uint4*>(slot + p) = make_uint4((uint32_t)o0, (uint32_t)(o0 >> 32), (uint32_t)o1, (uint32_t)(o1 >> 32));
    } else {   // a d_windows off the 16-byte grid
        for (uint32_t j = 0; j < 8; j++) {
            slot[p + j] = (uint8_t)(o0 >> (8 * j));
            slot[p + 8 + j] = (uint8_t)(o1 >> (8 * j));
        }
    }
}

__global__ __launch_bounds__(ZX_T) void dmx_zx_windows_kernel(const uint8_t* __restrict__ out,
                                                              const dmx_zpoint* __restrict__ points,
                                                              uint8_t* __restrict__ windows, const uint8_t* __restrict__ work) {
    const ZCtl* ctl = (const ZCtl*)work;
    if (!ctl->go) return;
    const uint64_t n = ctl->out_len, units = 4ull * ctl->npoints;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint64_t k = u >> 2, off = points[k].out_off;
        const uint32_t zeros = off < ZX_W ? ZX_W - (uint32_t)off : 0u;
        uint8_t* slot = windows + k * ZX_W;
        const uint32_t p = (uint32_t)(u & 3) * (ZX_W / 4) + threadIdx.x * 16;
        zx_window_group(out, n, off, slot, p, zeros);
        zx_window_group(out, n, off, slot, p + ZX_T * 16, zeros);
    }
}

// the sum of the four bytes of w, and the sum of byte i times i
__device__ __forceinline__ void zx_word(uint32_t w, uint32_t& s, uint32_t& t) {
    const uint32_t b0 = w & 255u, b1 = (w >> 8) & 255u, b2 = (w >> 16) & 255u, b3 = w >> 24;
    s = b0 + b1 + b2 + b3;
    t = b1 + 2 * b2 + 3 * b3;
}

// Per piece of DMX_ZS_PIECE bytes of a point, counted from the point's start: the sums (a, b) of the
// piece from a = b = 0, b with position weights (a byte counts once for every byte from it to the
// piece's end), each mod 65521.  The piece is covered by the aligned 16-byte groups that hold it,
// at most 4 097, thread t taking groups t, t + 256, ...: a group inside the piece is one load, of
// byte sum S and index-weighted sum T, and adds (hi - p0) S - T to b; the two groups at the edges
// add their bytes inside the piece one by one, so nothing outside the piece is loaded.
// Bounds: a thread takes at most 17 groups of S <= 4 080 at weights <= 65 536, so its b stays below
// 17 x 4 080 x 65 536 < 2^33; a workgroup's b is at most 255 x 65 536 x 65 537 / 2 < 2^40 and its a at
// most 255 x 65 536 < 2^24: no sum needs a reduction before the last.
__global__ __launch_bounds__(ZX_T) void dmx_zx_fold_kernel(const uint8_t* __restrict__ out, const dmx_zpoint* __restrict__ points,
                                                           uint8_t* __restrict__ work) {
    __shared__ uint32_t wa[ZX_T / 64];
    __shared__ uint64_t wb[ZX_T / 64];
    const ZCtl* ctl = (const ZCtl*)work;
    if (!ctl->go) return;
    constexpr uint32_t M = 65521u;
    const uint32_t np = ctl->npoints, total = ctl->pieces, tid = threadIdx.x;
    const uint32_t* base = zx_base(work);
    uint2* sums = zx_sums(work, np);
    for (uint32_t q = blockIdx.x; q < total; q += gridDim.x) {
        uint32_t k = 0, above = np;   // base[k] <= q < base[above]: the last such k holds piece q
        while (above - k > 1) {
            const uint32_t mid = k + (above - k) / 2;
            if (base[mid] <= q) k = mid;
            else above = mid;
        }
        const uint64_t start = points[k].out_off, stop = start + points[k].out_len;
        const uint64_t lo = start + (uint64_t)(q - base[k]) * DMX_ZS_PIECE, hi = stop - lo < DMX_ZS_PIECE ? stop : lo + DMX_ZS_PIECE;
        const uint32_t head = (uint32_t)((uintptr_t)(out + lo) & 15u);
        const uint32_t groups = (uint32_t)((head + (hi - lo) + 15) / 16);
        uint32_t sa = 0;
        uint64_t sb = 0;
        for (uint32_t g = tid; g < groups; g += ZX_T) {
            // the position behind the group, and its first inside the piece (group 0 may begin before the piece, or before out)
            const uint64_t p1 = lo + 16ull * g + 16 - head, p0 = g || !head ? p1 - 16 : lo;
            if (p1 - p0 == 16 && p1 <= hi) {
                const uint4 v = *reinterpret_cast<const uint4*>(out + p0);
                uint32_t s0, s1, s2, s3, t0, t1, t2, t3;
                zx_word(v.x, s0, t0);
                zx_word(v.y, s1, t1);
                zx_word(v.z, s2, t2);
                zx_word(v.w, s3, t3);
                const uint32_t S = s0 + s1 + s2 + s3, T = t0 + t1 + t2 + t3 + 4 * s1 + 8 * s2 + 12 * s3;
                sa += S;
                sb += (hi - p0) * S - T;   // hi - p0 >= 16 and T <= 15 S
            } else {
                const uint64_t b1 = p1 < hi ? p1 : hi;
                for (uint64_t p = p0; p < b1; p++) {
                    const uint32_t x = out[p];
                    sa += x;
                    sb += (hi - p) * x;
                }
            }
        }
        for (int d = 32; d; d >>= 1) {
            sa += __shfl_down(sa, d);
            sb += __shfl_down(sb, d);
        }
        if ((tid & 63u) == 0) {
            wa[tid >> 6] = sa;
            wb[tid >> 6] = sb;
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t A = 0;
            uint64_t B = 0;
            for (uint32_t w = 0; w < ZX_T / 64; w++) {
                A += wa[w];
                B += wb[w];
            }
            sums[q] = make_uint2(A % M, (uint32_t)(B % M));
        }
        __syncthreads();
    }
}

// A thread per point: a' = a + S, b' = b + len a + T over its pieces from a = 1, b = 0.  len mod M,
// a, b, S and T are below 65 521, so len a + b + T stays below 2^33.  Thread 0 writes the record.
__global__ __launch_bounds__(ZX_T) void dmx_zx_finish_kernel(const dmx_zpoint* __restrict__ points, uint32_t* __restrict__ adlers,
                                                             uint8_t* __restrict__ work, dmx_zindex_status* __restrict__ st) {
    const ZCtl* ctl = (const ZCtl*)work;
    if (!ctl->go) return;
    constexpr uint64_t M = 65521u;
    const uint32_t np = ctl->npoints, k = blockIdx.x * ZX_T + threadIdx.x;
    if (k < np) {
        const uint32_t* base = zx_base(work);
        const uint2* sums = zx_sums(work, np);
        const uint64_t n = points[k].out_len;
        uint64_t a = 1, b = 0;
        for (uint32_t q = base[k]; q < base[k + 1]; q++) {
            const uint64_t len = q + 1 < base[k + 1] ? DMX_ZS_PIECE : n - (uint64_t)(q - base[k]) * DMX_ZS_PIECE;
            b = (b + (len % M) * a + sums[q].y) % M;
            a = (a + sums[q].x) % M;
        }
        adlers[k] = (uint32_t)((b << 16) | a);
    }
    if (k == 0) {
        st->status = 0;
        st->format = ctl->format;
        st->out_len = ctl->out_len;
        st->in_used = ctl->in_used;
        st->check = ctl->check;
        st->npoints = np;
        st->span = ctl->span;
        st->reserved = 0;
    }
}

extern "C" int dmx_zindex_from_parallel_async(const void* d_plan, uint64_t plan_bytes, const dmx_par_status* d_dec_status,
                                              const void* d_out, uint64_t out_cap, uint32_t max_live, uint32_t span,
                                              dmx_zpoint* d_points, uint32_t* d_adlers, void* d_windows, uint32_t max_points,
                                              void* d_work, uint64_t work_bytes, dmx_zindex_status* d_status, void* stream) {
    if (!d_plan || !d_dec_status || !d_out || !d_points || !d_adlers || !d_windows || !d_work || !d_status) return -(int)E_INVAL;
    if (((uintptr_t)d_plan & 255) || ((uintptr_t)d_work & 255) || ((uintptr_t)d_points & 7) || ((uintptr_t)d_status & 7) ||
        ((uintptr_t)d_dec_status & 7) || ((uintptr_t)d_adlers & 3))
        return -(int)E_INVAL;
    if (plan_bytes < dmx_pf_plan_bytes(1) || work_bytes < dmx_zs_work(0, 1)) return -(int)E_INVAL;
    if (span > DMX_ZINDEX_MAX_SPAN) return -(int)E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    const dmx_pchunk* chunks = (const dmx_pchunk*)((const uint8_t*)d_plan + 256);
    const uint8_t* out = (const uint8_t*)d_out;
    uint8_t* work = (uint8_t*)d_work;
    hipLaunchKernelGGL(dmx_zx_select_kernel, dim3(1), dim3(64), 0, s, chunks, plan_bytes, d_dec_status, out_cap, max_live,
                       dmx_zs_span(span), max_points, work_bytes, d_points, work, d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    const uint64_t units = 4ull * max_points;
    hipLaunchKernelGGL(dmx_zx_windows_kernel, dim3(units < ZX_WIN_MAX_WG ? (units ? (uint32_t)units : 1u) : ZX_WIN_MAX_WG),
                       dim3(ZX_T), 0, s, out, d_points, (uint8_t*)d_windows, work);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    const uint64_t pieces = dmx_zs_max_pieces(out_cap, max_points);
    hipLaunchKernelGGL(dmx_zx_fold_kernel, dim3(pieces < ZX_FOLD_MAX_WG ? (pieces ? (uint32_t)pieces : 1u) : ZX_FOLD_MAX_WG),
                       dim3(ZX_T), 0, s, out, d_points, work);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_zx_finish_kernel, dim3(max_points ? (max_points + ZX_T - 1) / ZX_T : 1u), dim3(ZX_T), 0, s, d_points,
                       d_adlers, work, d_status);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

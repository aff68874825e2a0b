// sz3_amd/csrc/sz3hip_reduce.hip — per-box min, max, moments and histogram of a request's boxes, no output array:
// a reduction in the strided gather's place.
//
//   k_region_reduce<T>        blockIdx.y: the box, blockIdx.x: its chunk of SZK_REDUCE_CHUNK consecutive row-major indices; one
//                             szk_reduce_part per chunk, the histogram through LDS counters
//   k_region_reduce_final     one workgroup per box folds the box's partials into its sz3hip_box_stats (a launch of its own, like
//                             k_verify_final and k_minmax_final: no hand-off between workgroups inside a launch)
//   ..._view                  the same two over ONE record passed by value (sz3hip_reduce_device: no table in device memory)
//
// The record is the strided gather's (szk_region_gather_strided_box: total, src, ext, str), built by the gather's builders; its `dst` word is
// SZK_REDUCE_DST(first partial record, the box's index in the request — its d_stats entry and histogram row), `dstr` is not read.
//
// A point v enters as x = (double)v. NaN and +-Inf are counted in n_nonfinite and left out of everything else (sz3hip_verify.hip's rule).
// Extremes travel as (value, index) pairs, "smaller index wins ties", so -0.0 and +0.0 tie and the earlier element is reported. The sums
// are of x - K and (x - K)^2 — each difference and each square rounded once, no fused multiply-add (-ffp-contract=off) — K the box's
// point of index 0 if finite, else 0.0: every workgroup reads it itself.
//
// The partition rule: lane l of chunk c meets the indices c * 4096 + i * 256 + l, i = 0 .. 15, in that order (lanes run along x); the
// wave's 64 states fold by __shfl_down 32, 16, .., 1; the four waves fold in wave order through LDS; the final's thread t folds the
// partials t, t + 256, .. in that order, then the same two folds. Nothing of this depends on the grid, on the number of boxes, on the
// handle's kind or on the device: every field is reproducible bit for bit. No flags, no float atomics; the histogram's counters are integers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sz3hip.h"
#include "sz3hip_kernels.h"

#include "sz3hip_devutil.h"

namespace {
static_assert(sizeof(szk_reduce_part) == 8 * 8 && sizeof(sz3hip_box_stats) == 11 * 8, "records are rows of words");
static_assert(SZK_REDUCE_CHUNK == 16 * 256, "a lane takes 16 points of its chunk");

// A lane's running state: it meets its points in increasing index order, so inside a lane "the first of equal minima" is a strict comparison
// (the partial record's own fields; index ~0: none yet)
using RAcc = szk_reduce_part;
__device__ __forceinline__ RAcc r_empty() {
    RAcc s;
    s.n_fin = s.n_nonfinite = 0;
    s.argmin = s.argmax = ~0ull;
    s.mn = INFINITY;
    s.mx = -INFINITY;
    s.sum = s.sum_sq = 0.0;
    return s;
}

__device__ __forceinline__ void r_elem(RAcc &s, double x, uint64_t idx, double K) {
    if (!(fabs(x) < INFINITY)) {  // (false for NaN)
        s.n_nonfinite++;
        return;
    }
    s.n_fin++;
    const bool below = x < s.mn, above = x > s.mx;
    s.mn = below ? x : s.mn;
    s.argmin = below ? idx : s.argmin;
    s.mx = above ? x : s.mx;
    s.argmax = above ? idx : s.argmax;
    const double u = x - K, q = u * u;
    s.sum += u;
    s.sum_sq += q;
}

__device__ __forceinline__ void r_merge(RAcc &x, const RAcc &y) {
    if (y.mn < x.mn || (y.mn == x.mn && y.argmin < x.argmin)) {
        x.mn = y.mn;
        x.argmin = y.argmin;
    }
    if (y.mx > x.mx || (y.mx == x.mx && y.argmax < x.argmax)) {
        x.mx = y.mx;
        x.argmax = y.argmax;
    }
    x.n_fin += y.n_fin;
    x.n_nonfinite += y.n_nonfinite;
    x.sum += y.sum;
    x.sum_sq += y.sum_sq;
}

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)v, d, WAVE), hi = (uint32_t)__shfl_down((int)(uint32_t)(v >> 32), d, WAVE);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ RAcc r_shfl_down(const RAcc &r, int d) {
    RAcc o;
    o.n_fin = shfl_down_u64(r.n_fin, d);
    o.n_nonfinite = shfl_down_u64(r.n_nonfinite, d);
    o.argmin = shfl_down_u64(r.argmin, d);
    o.argmax = shfl_down_u64(r.argmax, d);
    o.mn = __shfl_down(r.mn, d, WAVE);
    o.mx = __shfl_down(r.mx, d, WAVE);
    o.sum = __shfl_down(r.sum, d, WAVE);
    o.sum_sq = __shfl_down(r.sum_sq, d, WAVE);
    return o;
}
// the workgroup's (256 threads, all of them here) state: valid in thread 0. Lane l takes lane l + d's state for d = 32 .. 1 (what the lanes
// beyond 64 - d take is never read by lane 0's tree), then the waves 1 .. 3 in their order
__device__ __forceinline__ RAcc r_block_fold(RAcc r) {
#pragma unroll 1
    for (int d = WAVE / 2; d >= 1; d >>= 1) {
        const RAcc o = r_shfl_down(r, d);
        r_merge(r, o);
    }
    __shared__ RAcc sh[4];
    if (lane_id() == 0) sh[threadIdx.x / WAVE] = r;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) r_merge(r, sh[w]);
    return r;
}

// the slot of a finite x: 0 under, nbins + 1 over, else 1 + its bin
__device__ __forceinline__ uint32_t r_slot(double x, const szk_reduce_hist &h) {
    if (x < h.lo) return 0;
    if (x >= h.hi) return h.nbins + 1;
    const uint64_t k = (uint64_t)((x - h.lo) * h.scale);
    return 1 + (uint32_t)(k < (uint64_t)(h.nbins - 1) ? k : (uint64_t)(h.nbins - 1));
}

template <typename T>
__device__ __forceinline__ void reduce_chunk(const T *__restrict__ src, const szk_region_gather_strided_box &b, szk_reduce_part *__restrict__ partials,
                                             uint64_t *__restrict__ hist, const szk_reduce_hist &h) {
    __shared__ uint32_t bins[SZ3HIP_MAX_BINS + 2];
    const uint64_t c = blockIdx.x, total = b.total;
    if (c * SZK_REDUCE_CHUNK >= total) return;  // (workgroups beyond the box's chunks leave: the whole workgroup, before any barrier)
    const uint32_t slots = h.nbins ? h.nbins + 2 : 0;
    for (uint32_t k = threadIdx.x; k < slots; k += 256) bins[k] = 0;
    if (slots) __syncthreads();
    const double k0 = (double)src[b.src];
    const double K = fabs(k0) < INFINITY ? k0 : 0.0;
    RAcc s = r_empty();
#pragma unroll 4
    for (int i = 0; i < SZK_REDUCE_CHUNK / 256; i++) {
        const uint64_t t = c * SZK_REDUCE_CHUNK + (uint64_t)i * 256 + threadIdx.x;
        if (t >= total) break;
        uint64_t r = t, so = 0;
#pragma unroll
        for (int j = 3; j >= 0; j--) {
            so += (r % b.ext[j]) * b.str[j];
            r /= b.ext[j];
        }
        const double x = (double)src[b.src + so];
        r_elem(s, x, t, K);
        if (slots && fabs(x) < INFINITY) atomicAdd(&bins[r_slot(x, h)], 1u);
    }
    const RAcc f = r_block_fold(s);  // (holds a barrier: the LDS counters are complete behind it)
    if (threadIdx.x == 0) partials[SZK_REDUCE_DST_PART((uint64_t)(uintptr_t)b.dst) + c] = f;
    uint64_t *row = hist + SZK_REDUCE_DST_BOX((uint64_t)(uintptr_t)b.dst) * slots;
    for (uint32_t k = threadIdx.x; k < slots; k += 256) {
        const uint32_t v = bins[k];
        if (v) atomicAdd((unsigned long long *)&row[k], (unsigned long long)v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_region_reduce(const T *__restrict__ src, const szk_region_gather_strided_box *__restrict__ recs,
                                                       szk_reduce_part *__restrict__ partials, uint64_t *__restrict__ hist, szk_reduce_hist opts) {
    reduce_chunk<T>(src, recs[blockIdx.y], partials, hist, opts);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_reduce_view(const T *__restrict__ src, szk_region_gather_strided_box rec, szk_reduce_part *__restrict__ partials,
                                                            uint64_t *__restrict__ hist, szk_reduce_hist opts) {
    reduce_chunk<T>(src, rec, partials, hist, opts);
}

// the box's shift is read where the reduce kernel read it: the point of index 0
template <typename T>
__device__ __forceinline__ void reduce_final(const T *__restrict__ src, const szk_region_gather_strided_box &b, const szk_reduce_part *__restrict__ partials,
                                             sz3hip_box_stats *__restrict__ out) {
    const uint64_t nrec = szk_reduce_chunks(b.total);
    const szk_reduce_part *p = partials + SZK_REDUCE_DST_PART((uint64_t)(uintptr_t)b.dst);
    RAcc r = r_empty();
    for (uint64_t i = threadIdx.x; i < nrec; i += 256) r_merge(r, p[i]);
    r = r_block_fold(r);
    if (threadIdx.x == 0) {
        const double k0 = (double)src[b.src];
        sz3hip_box_stats st;
        st.n = b.total;
        st.n_nonfinite = r.n_nonfinite;
        st.argmin = r.n_fin ? r.argmin : b.total;
        st.argmax = r.n_fin ? r.argmax : b.total;
        st.min = r.n_fin ? r.mn : (double)NAN;
        st.max = r.n_fin ? r.mx : (double)NAN;
        st.shift = fabs(k0) < INFINITY ? k0 : 0.0;
        st.sum = r.sum;
        st.sum_sq = r.sum_sq;
        const double m = (double)(b.total - r.n_nonfinite);
        st.mean = st.shift + st.sum / m;
        st.variance = (st.sum_sq - st.sum * st.sum / m) / m;
        out[SZK_REDUCE_DST_BOX((uint64_t)(uintptr_t)b.dst)] = st;
    }
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_reduce_final(const T *__restrict__ src, const szk_region_gather_strided_box *__restrict__ recs,
                                                             const szk_reduce_part *__restrict__ partials, sz3hip_box_stats *__restrict__ stats) {
    reduce_final<T>(src, recs[blockIdx.x], partials, stats);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_reduce_final_view(const T *__restrict__ src, szk_region_gather_strided_box rec,
                                                                  const szk_reduce_part *__restrict__ partials, sz3hip_box_stats *__restrict__ stats) {
    reduce_final<T>(src, rec, partials, stats);
}
}  // namespace

int szk_launch_region_reduce(int dtype, const void *d_src, const szk_region_gather_strided_box *d_recs, const szk_region_gather_strided_box *rec_by_value, uint32_t n,
                             uint64_t most_total, const szk_region_sink *sink, hipStream_t s) {
    const uint64_t gx = szk_reduce_chunks(most_total);
    if (!sink || !sink->partials || !d_src || n < 1 || n > 65535 || gx < 1 || gx > 0x7FFFFFFFull || sink->hist.nbins > SZ3HIP_MAX_BINS) return -1;
    if ((d_recs == nullptr) == (rec_by_value == nullptr) || (rec_by_value && n != 1) || (sink->hist.nbins && !sink->d_hist)) return -1;
    const dim3 grid((uint32_t)gx, n);
    if (d_recs) {
        if (dtype == 0) hipLaunchKernelGGL(k_region_reduce<float>, grid, dim3(256), 0, s, (const float *)d_src, d_recs, sink->partials, sink->d_hist, sink->hist);
        else hipLaunchKernelGGL(k_region_reduce<double>, grid, dim3(256), 0, s, (const double *)d_src, d_recs, sink->partials, sink->d_hist, sink->hist);
    } else {
        if (dtype == 0) hipLaunchKernelGGL(k_region_reduce_view<float>, grid, dim3(256), 0, s, (const float *)d_src, *rec_by_value, sink->partials, sink->d_hist, sink->hist);
        else hipLaunchKernelGGL(k_region_reduce_view<double>, grid, dim3(256), 0, s, (const double *)d_src, *rec_by_value, sink->partials, sink->d_hist, sink->hist);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int szk_launch_region_reduce_final(int dtype, const void *d_src, const szk_region_gather_strided_box *d_recs, const szk_region_gather_strided_box *rec_by_value,
                                   uint32_t n, const szk_region_sink *sink, hipStream_t s) {
    if (!sink || !sink->partials || !sink->d_stats || !d_src || n < 1 || n > 65535) return -1;
    if ((d_recs == nullptr) == (rec_by_value == nullptr) || (rec_by_value && n != 1)) return -1;
    sz3hip_box_stats *st = static_cast<sz3hip_box_stats *>(sink->d_stats);
    if (d_recs) {
        if (dtype == 0) hipLaunchKernelGGL(k_region_reduce_final<float>, dim3(n), dim3(256), 0, s, (const float *)d_src, d_recs, sink->partials, st);
        else hipLaunchKernelGGL(k_region_reduce_final<double>, dim3(n), dim3(256), 0, s, (const double *)d_src, d_recs, sink->partials, st);
    } else {
        if (dtype == 0) hipLaunchKernelGGL(k_region_reduce_final_view<float>, dim3(1), dim3(256), 0, s, (const float *)d_src, *rec_by_value, sink->partials, st);
        else hipLaunchKernelGGL(k_region_reduce_final_view<double>, dim3(1), dim3(256), 0, s, (const double *)d_src, *rec_by_value, sink->partials, st);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

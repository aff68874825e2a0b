// sz3_amd/csrc/sz3hip_select.hip — the points of a request's boxes whose values lie in a range: three launches in the
// strided gather's place, over the gather's own records and sz3hip_reduce.hip's partition rule.
//
//   k_region_select_count<T>  blockIdx.y: the box, blockIdx.x: its chunk of SZK_REDUCE_CHUNK consecutive row-major indices; the chunk's hit
//                             count as one 64-bit word
//   k_region_select_scan      one workgroup per box turns the box's counts into exclusive offsets in place, 256 at a time with a running
//                             carry, and writes the box's sz3hip_select_head
//   k_region_select_write<T>  the count's grid: the predicate once more; a hit's rank is its chunk's offset + the hits of the earlier
//                             (i, wave) pairs of the chunk (a 16 x 4 table of wave counts in LDS, behind one barrier) + the hits of the lower
//                             lanes of its wave (__ballot, popcount under the lane mask); index and raw value go to place `rank` where
//                             rank < capacity
//   ..._view                  the same three over ONE record and one output passed by value (sz3hip_select_device)
//
// The record is the strided gather's (total, src, ext, str); its `dst` word is SZK_REDUCE_DST(the box's first chunk record, the box's index in
// the request), `dstr` is not read. Box i's outputs — d_index, d_value, capacity — are the words 3 i .. 3 i + 2 behind the request's records.
//
// Lane l of chunk c meets the indices c * 4096 + i * 256 + l, i = 0 .. 15, as reduce_chunk does: consecutive ranks come from consecutive
// lanes, so the stores coalesce. The write holds a lane's 16 values in registers (raw bits) between the two halves; the lane's coordinates are
// divided out once, for i = 0, and stepped by 256 points with carries from there. Nothing waits across workgroups; no flags, no atomics; a
// workgroup whose chunk starts at or past the capacity leaves before the barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sz3hip.h"
#include "sz3hip_kernels.h"

#include "sz3hip_devutil.h"

namespace {
static_assert(sizeof(sz3hip_select_head) == 4 * 8 && sizeof(sz3hip_select_req) == 96 && sizeof(sz3hip_select_opts) == 24 && sizeof(sz3hip_select_plan) == 40,
              "the header's sizes");
static_assert(SZK_REDUCE_CHUNK == 16 * 256, "a lane takes 16 points of its chunk");
constexpr int ROWS = SZK_REDUCE_CHUNK / 256;
using Box = szk_region_gather_strided_box;

__device__ __forceinline__ bool sel_hit(double x, const szk_select_opts &o) {
    if (x != x) return (o.flags & SZ3HIP_SELECT_NAN) != 0;
    const bool in = o.lo <= x && x <= o.hi;
    return in != ((o.flags & SZ3HIP_SELECT_INVERT) != 0);
}

// a lane's walk over its points: the coordinates of its first index divided out once, then steps of 256 points — 256's own digits added with
// carries (a digit sum stays below twice the extent: one subtraction). The slowest place takes what is left; an index at or past the box's
// total is never loaded
struct Walk {
    uint64_t c[4], d[4];
    __device__ __forceinline__ Walk(const Box &b, uint64_t t0) {
        uint64_t r = t0, q = 256;
#pragma unroll
        for (int j = 3; j >= 1; j--) {
            c[j] = r % b.ext[j];
            r /= b.ext[j];
            d[j] = q % b.ext[j];
            q /= b.ext[j];
        }
        c[0] = r;
        d[0] = q;
    }
    __device__ __forceinline__ uint64_t at(const Box &b) const { return b.src + c[0] * b.str[0] + c[1] * b.str[1] + c[2] * b.str[2] + c[3] * b.str[3]; }
    __device__ __forceinline__ void step(const Box &b) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 3; j >= 1; j--) {
            const uint64_t v = c[j] + d[j] + carry;
            carry = v >= b.ext[j] ? 1 : 0;
            c[j] = carry ? v - b.ext[j] : v;
        }
        c[0] += d[0] + carry;
    }
};

template <typename T>
__device__ __forceinline__ T from_bits(typename QTraits<T>::UQ u) {
    T v;
    __builtin_memcpy(&v, &u, sizeof(T));
    return v;
}

template <typename T>
__device__ __forceinline__ void select_count(const T *__restrict__ src, const Box &b, uint64_t *__restrict__ counts, const szk_select_opts &o) {
    const uint64_t c = blockIdx.x, total = b.total;
    if (c * SZK_REDUCE_CHUNK >= total) return;  // (workgroups beyond the box's chunks leave: the whole workgroup, before any barrier)
    const uint64_t t0 = c * SZK_REDUCE_CHUNK + threadIdx.x;
    Walk w(b, t0);
    uint32_t hits = 0;
#pragma unroll 4
    for (int i = 0; i < ROWS; i++) {
        if (t0 + (uint64_t)i * 256 < total) hits += sel_hit((double)src[w.at(b)], o) ? 1u : 0u;
        w.step(b);
    }
    __shared__ uint32_t sh[4];
    const uint32_t in_wave = wave_sum(hits);
    if (lane_id() == 0) sh[threadIdx.x / WAVE] = in_wave;
    __syncthreads();
    if (threadIdx.x == 0) counts[SZK_REDUCE_DST_PART((uint64_t)(uintptr_t)b.dst) + c] = (uint64_t)sh[0] + sh[1] + sh[2] + sh[3];
}

__device__ __forceinline__ void select_scan(const Box &b, uint64_t *__restrict__ counts, uint64_t capacity, sz3hip_select_head *__restrict__ head) {
    const uint64_t nrec = szk_reduce_chunks(b.total);
    uint64_t *p = counts + SZK_REDUCE_DST_PART((uint64_t)(uintptr_t)b.dst);
    __shared__ uint64_t sh[4];
    const uint32_t wave = threadIdx.x / WAVE;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nrec; base += 256) {  // (the trip count is the workgroup's)
        const uint64_t i = base + threadIdx.x;
        const uint64_t v = i < nrec ? p[i] : 0;
        const uint64_t incl = wave_incl_scan(v);
        if (lane_id() == WAVE - 1) sh[wave] = incl;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint64_t s = sh[k];
            before += k < wave ? s : 0;
            all += s;
        }
        if (i < nrec) p[i] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sz3hip_select_head h;
        h.n = b.total;
        h.count = carry;
        h.written = carry < capacity ? carry : capacity;
        h.capacity = capacity;
        *head = h;
    }
}

template <typename T>
__device__ __forceinline__ void select_write(const T *__restrict__ src, const Box &b, const uint64_t *__restrict__ counts, uint64_t *__restrict__ d_index,
                                             T *__restrict__ d_value, uint64_t capacity, const szk_select_opts &o) {
    using U = typename QTraits<T>::UQ;
    const uint64_t c = blockIdx.x, total = b.total;
    if (c * SZK_REDUCE_CHUNK >= total) return;
    const uint64_t first = counts[SZK_REDUCE_DST_PART((uint64_t)(uintptr_t)b.dst) + c];  // (the scan left the chunk's exclusive offset)
    if (first >= capacity) return;  // (nothing of this chunk has a place: the whole workgroup, before the barrier)
    __shared__ uint4 tbl[ROWS];  // the hits of (i, wave)
    const U *bits = reinterpret_cast<const U *>(src);
    U *vout = reinterpret_cast<U *>(d_value);
    const uint32_t wave = threadIdx.x / WAVE;
    const uint64_t t0 = c * SZK_REDUCE_CHUNK + threadIdx.x;
    Walk w(b, t0);
    U v[ROWS];
    uint32_t mask = 0;
#pragma unroll
    for (int i = 0; i < ROWS; i++) {
        bool hit = false;
        v[i] = 0;
        if (t0 + (uint64_t)i * 256 < total) {
            v[i] = bits[w.at(b)];
            hit = sel_hit((double)from_bits<T>(v[i]), o);
        }
        w.step(b);
        const uint32_t in_wave = (uint32_t)__popcll(__ballot(hit));
        if (lane_id() == 0) reinterpret_cast<uint32_t *>(&tbl[i])[wave] = in_wave;
        mask |= hit ? 1u << i : 0u;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane_id()) - 1ull;
    uint64_t run = first;
#pragma unroll
    for (int i = 0; i < ROWS; i++) {
        const uint4 q = tbl[i];
        const uint32_t before = (wave > 0 ? q.x : 0u) + (wave > 1 ? q.y : 0u) + (wave > 2 ? q.z : 0u);
        const bool hit = (mask >> i) & 1u;
        const uint64_t rank = run + before + (uint32_t)__popcll(__ballot(hit) & below);
        if (hit && rank < capacity) {
            d_index[rank] = t0 + (uint64_t)i * 256;
            if (vout) vout[rank] = v[i];
        }
        run += (uint64_t)q.x + q.y + q.z + q.w;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_region_select_count(const T *__restrict__ src, const Box *__restrict__ recs, uint64_t *__restrict__ counts, szk_select_opts opts) {
    select_count<T>(src, recs[blockIdx.y], counts, opts);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_select_count_view(const T *__restrict__ src, Box rec, uint64_t *__restrict__ counts, szk_select_opts opts) {
    select_count<T>(src, rec, counts, opts);
}
__global__ __launch_bounds__(256) void k_region_select_scan(const Box *__restrict__ recs, const uint64_t *__restrict__ outs, uint64_t *__restrict__ counts,
                                                            sz3hip_select_head *__restrict__ heads) {
    const Box &b = recs[blockIdx.x];
    const uint64_t box = SZK_REDUCE_DST_BOX((uint64_t)(uintptr_t)b.dst);
    select_scan(b, counts, outs[box * SZK_SELECT_OUT_WORDS + 2], heads + box);
}
__global__ __launch_bounds__(256) void k_region_select_scan_view(Box rec, uint64_t capacity, uint64_t *__restrict__ counts, sz3hip_select_head *__restrict__ head) {
    select_scan(rec, counts, capacity, head);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_select_write(const T *__restrict__ src, const Box *__restrict__ recs, const uint64_t *__restrict__ outs,
                                                             const uint64_t *__restrict__ counts, szk_select_opts opts) {
    const Box &b = recs[blockIdx.y];
    const uint64_t *o = outs + SZK_REDUCE_DST_BOX((uint64_t)(uintptr_t)b.dst) * SZK_SELECT_OUT_WORDS;
    select_write<T>(src, b, counts, reinterpret_cast<uint64_t *>((uintptr_t)o[0]), reinterpret_cast<T *>((uintptr_t)o[1]), o[2], opts);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_select_write_view(const T *__restrict__ src, Box rec, uint64_t *__restrict__ d_index, T *__restrict__ d_value,
                                                                  uint64_t capacity, const uint64_t *__restrict__ counts, szk_select_opts opts) {
    select_write<T>(src, rec, counts, d_index, d_value, capacity, opts);
}

bool select_args(const void *d_src, const Box *d_recs, const Box *rec_by_value, uint32_t n, uint64_t gx, const szk_region_sink *sink) {
    if (!sink || sink->kind != SZK_SINK_SELECT || !sink->sel_counts || !sink->sel_heads || !sink->sel_outs || !d_src) return false;
    if (n < 1 || n > 65535 || gx < 1 || gx > 0x7FFFFFFFull) return false;
    return (d_recs == nullptr) != (rec_by_value == nullptr) && (!rec_by_value || n == 1);
}
}  // namespace

int szk_launch_region_select_count(int dtype, const void *d_src, const Box *d_recs, const Box *rec_by_value, uint32_t n, uint64_t most_total,
                                   const szk_region_sink *sink, hipStream_t s) {
    const uint64_t gx = szk_reduce_chunks(most_total);
    if (!select_args(d_src, d_recs, rec_by_value, n, gx, sink)) return -1;
    const dim3 grid((uint32_t)gx, n);
    if (d_recs) {
        if (dtype == 0) hipLaunchKernelGGL(k_region_select_count<float>, grid, dim3(256), 0, s, (const float *)d_src, d_recs, sink->sel_counts, sink->sel);
        else hipLaunchKernelGGL(k_region_select_count<double>, grid, dim3(256), 0, s, (const double *)d_src, d_recs, sink->sel_counts, sink->sel);
    } else {
        if (dtype == 0) hipLaunchKernelGGL(k_region_select_count_view<float>, grid, dim3(256), 0, s, (const float *)d_src, *rec_by_value, sink->sel_counts, sink->sel);
        else hipLaunchKernelGGL(k_region_select_count_view<double>, grid, dim3(256), 0, s, (const double *)d_src, *rec_by_value, sink->sel_counts, sink->sel);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int szk_launch_region_select_place(int dtype, const void *d_src, const Box *d_recs, const Box *rec_by_value, uint32_t n, uint64_t most_total,
                                   const szk_region_sink *sink, hipStream_t s) {
    const uint64_t gx = szk_reduce_chunks(most_total);
    if (!select_args(d_src, d_recs, rec_by_value, n, gx, sink)) return -1;
    const dim3 grid((uint32_t)gx, n);
    sz3hip_select_head *heads = static_cast<sz3hip_select_head *>(sink->sel_heads);
    if (d_recs) {
        const uint64_t *outs = reinterpret_cast<const uint64_t *>(d_recs + n);  // (behind the boxes' records, in the same copy)
        hipLaunchKernelGGL(k_region_select_scan, dim3(n), dim3(256), 0, s, d_recs, outs, sink->sel_counts, heads);
        if (dtype == 0) hipLaunchKernelGGL(k_region_select_write<float>, grid, dim3(256), 0, s, (const float *)d_src, d_recs, outs, (const uint64_t *)sink->sel_counts, sink->sel);
        else hipLaunchKernelGGL(k_region_select_write<double>, grid, dim3(256), 0, s, (const double *)d_src, d_recs, outs, (const uint64_t *)sink->sel_counts, sink->sel);
    } else {
        uint64_t *d_index = reinterpret_cast<uint64_t *>((uintptr_t)sink->sel_outs[0]);
        void *d_value = reinterpret_cast<void *>((uintptr_t)sink->sel_outs[1]);
        const uint64_t capacity = sink->sel_outs[2];
        hipLaunchKernelGGL(k_region_select_scan_view, dim3(1), dim3(256), 0, s, *rec_by_value, capacity, sink->sel_counts, heads);
        if (dtype == 0)
            hipLaunchKernelGGL(k_region_select_write_view<float>, grid, dim3(256), 0, s, (const float *)d_src, *rec_by_value, d_index, (float *)d_value, capacity,
                               (const uint64_t *)sink->sel_counts, sink->sel);
        else
            hipLaunchKernelGGL(k_region_select_write_view<double>, grid, dim3(256), 0, s, (const double *)d_src, *rec_by_value, d_index, (double *)d_value, capacity,
                               (const uint64_t *)sink->sel_counts, sink->sel);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

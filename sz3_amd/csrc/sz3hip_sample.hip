// sz3_amd/csrc/sz3hip_sample.hip — boxes sampled at fractional positions: ONE launch in the strided gather's place, over
// the gather's own records (`src`, `ext`, `str`; the `dst` word names the box, `dstr` is not read), the boxes' queries behind them.
//
//   k_region_sample<T, C, N, FILTER>  blockIdx.y: the box, a thread per query: the query's N coordinates (read as C, or worked out from the
//                                     lattice), the inside test or the clamp, the addresses of all 2^N corners of the cell (i + 1 clamped to
//                                     ext - 1: every load is in bounds), all corner loads, then the fold — fastest dimension first, a
//                                     dimension with f == 0 taking the value at i alone — and one store. NEAREST: one load, the raw bytes.
//   ..._view                          the same over ONE record and ONE query passed by value (sz3hip_sample_device)
//
// A query's result depends on the box's values, the query and the options alone: every route and grid gives the same bytes. All arithmetic
// is IEEE double without a fused multiply-add (the build's -ffp-contract=off, and the pragma below). No LDS, no atomics, nothing waits
// across workgroups, plain vector loads and stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sz3hip.h"
#include "sz3hip_kernels.h"

#pragma clang fp contract(off)

namespace {
static_assert(sizeof(sz3hip_sample_req) == 248 && sizeof(sz3hip_sample_opts) == 24 && sizeof(sz3hip_sample_plan) == 40, "the header's sizes");
static_assert(sizeof(szk_sample_query) == SZK_SAMPLE_WORDS * 8, "a query's words in the table");
using Box = szk_region_gather_strided_box;

template <typename T>
struct raw_of {
    using type = uint32_t;
};
template <>
struct raw_of<double> {
    using type = uint64_t;
};

template <typename T, typename C, int N, int FILTER>
__device__ __forceinline__ void sample_query(const T *__restrict__ src, const Box &b, const szk_sample_query &q, const szk_sample_opts &o, uint64_t t) {
    if (t >= q.n_points) return;
    double c[N];
    if (q.coords) {
        const C *p = static_cast<const C *>(q.coords) + t * N;
#pragma unroll
        for (int j = 0; j < N; j++) c[j] = (double)p[j];
    } else {  // (t < 2^31 and every count <= n_points <= 2^31: 32-bit divisions)
        const uint32_t n1 = (uint32_t)q.counts[1], n2 = (uint32_t)q.counts[2], r = (uint32_t)t / n2;
        const double i0 = (double)(r / n1), i1 = (double)(r % n1), i2 = (double)((uint32_t)t % n2);
#pragma unroll
        for (int j = 0; j < N; j++) {
            const int p = 4 - N + j;
            c[j] = ((q.origin[p] + i0 * q.steps[0][p]) + i1 * q.steps[1][p]) + i2 * q.steps[2][p];
        }
    }
    bool inside = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        const double hi = (double)(b.ext[4 - N + j] - 1), x = c[j];
        if (x != x) inside = false;
        else if (o.flags & SZ3HIP_SAMPLE_CLAMP) c[j] = x < 0.0 ? 0.0 : x > hi ? hi : x;
        else if (!(0.0 <= x && x <= hi)) inside = false;
    }
    T *out = static_cast<T *>(q.out);
    if (!inside) {
        out[t] = (T)o.fill;
        return;
    }
    if constexpr (FILTER == (int)SZ3HIP_SAMPLE_NEAREST) {
        uint64_t at = b.src;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const uint64_t last = b.ext[4 - N + j] - 1;
            uint64_t i = (uint64_t)floor(c[j] + 0.5);
            i = i < last ? i : last;
            at += i * b.str[4 - N + j];
        }
        using R = typename raw_of<T>::type;  // (the point's bytes: a NaN keeps its payload)
        reinterpret_cast<R *>(out)[t] = reinterpret_cast<const R *>(src)[at];
    } else {
        double f[N];
        uint64_t a0[N], a1[N];  // the two corners' offsets along dimension j
#pragma unroll
        for (int j = 0; j < N; j++) {
            const uint64_t last = b.ext[4 - N + j] - 1, st = b.str[4 - N + j];
            const double fl = floor(c[j]);
            const uint64_t i = (uint64_t)fl;
            f[j] = c[j] - fl;
            a0[j] = i * st;
            a1[j] = (i < last ? i + 1 : last) * st;
        }
        T v[1 << N];  // corner k: bit d of k picks i + 1 along dimension N - 1 - d (bit 0: the fastest)
#pragma unroll
        for (int k = 0; k < (1 << N); k++) {
            uint64_t at = b.src;
#pragma unroll
            for (int j = 0; j < N; j++) at += (k >> (N - 1 - j)) & 1 ? a1[j] : a0[j];
            v[k] = src[at];
        }
        double w[1 << N];
#pragma unroll
        for (int k = 0; k < (1 << N); k++) w[k] = (double)v[k];
#pragma unroll
        for (int d = 0; d < N; d++) {
            const double fd = f[N - 1 - d], gd = 1.0 - fd;
#pragma unroll
            for (int m = 0; m < (1 << (N - 1 - d)); m++) {
                const double lo = w[2 * m], up = w[2 * m + 1];
                w[m] = fd == 0.0 ? lo : gd * lo + fd * up;
            }
        }
        out[t] = (T)w[0];
    }
}

template <typename T, typename C, int N, int FILTER>
__global__ __launch_bounds__(256) void k_region_sample(const T *__restrict__ src, const Box *__restrict__ recs, szk_sample_opts opts) {
    const szk_sample_query *qs = reinterpret_cast<const szk_sample_query *>(recs + gridDim.y);  // (the queries lie behind the launch's records)
    sample_query<T, C, N, FILTER>(src, recs[blockIdx.y], qs[blockIdx.y], opts, (uint64_t)blockIdx.x * 256 + threadIdx.x);
}
template <typename T, typename C, int N, int FILTER>
__global__ __launch_bounds__(256) void k_region_sample_view(const T *__restrict__ src, Box rec, szk_sample_query q, szk_sample_opts opts) {
    sample_query<T, C, N, FILTER>(src, rec, q, opts, (uint64_t)blockIdx.x * 256 + threadIdx.x);
}

template <typename T, typename C, int N, int FILTER>
void sample_launch(const T *src, const Box *d_recs, const Box *rec, const szk_sample_query *q, dim3 grid, const szk_sample_opts &o, hipStream_t s) {
    if (d_recs) hipLaunchKernelGGL((k_region_sample<T, C, N, FILTER>), grid, dim3(256), 0, s, src, d_recs, o);
    else hipLaunchKernelGGL((k_region_sample_view<T, C, N, FILTER>), grid, dim3(256), 0, s, src, *rec, *q, o);
}
template <typename T, typename C, int N>
void sample_launch_filter(const T *src, const Box *d_recs, const Box *rec, const szk_sample_query *q, dim3 grid, const szk_sample_opts &o, hipStream_t s) {
    if (o.filter == SZ3HIP_SAMPLE_NEAREST) sample_launch<T, C, N, (int)SZ3HIP_SAMPLE_NEAREST>(src, d_recs, rec, q, grid, o, s);
    else sample_launch<T, C, N, (int)SZ3HIP_SAMPLE_LINEAR>(src, d_recs, rec, q, grid, o, s);
}
template <typename T, typename C>
void sample_launch_dims(const T *src, const Box *d_recs, const Box *rec, const szk_sample_query *q, dim3 grid, const szk_sample_opts &o, hipStream_t s) {
    switch (o.N) {
    case 1: sample_launch_filter<T, C, 1>(src, d_recs, rec, q, grid, o, s); break;
    case 2: sample_launch_filter<T, C, 2>(src, d_recs, rec, q, grid, o, s); break;
    case 3: sample_launch_filter<T, C, 3>(src, d_recs, rec, q, grid, o, s); break;
    default: sample_launch_filter<T, C, 4>(src, d_recs, rec, q, grid, o, s);
    }
}
template <typename T>
void sample_launch_type(const T *src, const Box *d_recs, const Box *rec, const szk_sample_query *q, dim3 grid, const szk_sample_opts &o, hipStream_t s) {
    if (o.coord_type == 0) sample_launch_dims<T, float>(src, d_recs, rec, q, grid, o, s);
    else sample_launch_dims<T, double>(src, d_recs, rec, q, grid, o, s);
}
}  // namespace

int szk_launch_region_sample(int dtype, const void *d_src, const Box *d_recs, const Box *rec_by_value, uint32_t n, const szk_region_sink *sink, hipStream_t s) {
    if (!sink || sink->kind != SZK_SINK_SAMPLE || !sink->smp_queries || !d_src || n < 1 || n > 65535) return -1;
    if ((d_recs == nullptr) == (rec_by_value == nullptr) || (rec_by_value && n != 1)) return -1;
    const szk_sample_opts &o = sink->smp;
    if (o.filter > SZ3HIP_SAMPLE_LINEAR || o.coord_type > 1 || o.N < 1 || o.N > 4) return -1;
    const uint64_t gx = (sink->smp_threads + 255) / 256;
    if (gx < 1 || gx > 0x7FFFFFFFull) return -1;
    const dim3 grid((uint32_t)gx, n);
    if (dtype == 0) sample_launch_type<float>((const float *)d_src, d_recs, rec_by_value, sink->smp_queries, grid, o, s);
    else sample_launch_type<double>((const double *)d_src, d_recs, rec_by_value, sink->smp_queries, grid, o, s);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

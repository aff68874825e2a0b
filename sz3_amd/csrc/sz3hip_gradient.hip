// sz3_amd/csrc/sz3hip_gradient.hip — gradients of boxes: ONE launch in the strided gather's place, over the gather's
// own records (`src`, `ext`, `str`; the `dst` word names the box, `dstr` is not read), a szk_gradient_box per record behind them: the real
// destination, its strides in OUTPUT elements and the box's grid steps spacing[a] * 2^level.
//
//   k_region_gradient<T, N>  blockIdx.y: the box, a thread per OUTPUT point, lanes along x: a wave's load at one stencil offset is one row
//                            segment. The output index gives the point's coordinates (+1 along the axes INTERIOR trims); along a
//                            differentiated axis the neighbours are ip = min(i + 1, E - 1) and im = max(i, 1) - 1, so every load lies in the
//                            box and none sits behind a branch. DERIV: two loads; MAG2, MAG, VECTOR: 2 N loads, all issued ahead of the
//                            arithmetic they feed. The centre is not read.
//   ..._view                 the same over ONE record and ONE szk_gradient_box passed by value (sz3hip_gradient_device)
//
// An output point depends on the box's values, the box's grid steps and the options alone (grd_deriv, grd_store below): every form, route and
// grid gives the same bytes. All arithmetic is IEEE double — one subtraction, one multiplication and one division per derivative — without
// a fused multiply-add (the build's -ffp-contract=off, and the pragma below). No LDS, no atomics, nothing waits across workgroups, plain
// vector loads and stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sz3hip.h"
#include "sz3hip_kernels.h"

#pragma clang fp contract(off)

namespace {
static_assert(sizeof(sz3hip_gradient_opts) == 48 && sizeof(sz3hip_gradient_plan) == 48, "the header's sizes");
static_assert(sizeof(szk_gradient_box) == SZK_GRADIENT_WORDS * 8, "a box's words in the table");
using Box = szk_region_gather_strided_box;

// the derivative along one axis: xp and xm the values at ip and im, span = ip - im (0 where the extent is 1, else 1 or 2), s the grid step
__device__ __forceinline__ double grd_deriv(double xp, double xm, uint32_t span, double s) {
    const double d = (xp - xm) / ((double)span * s);
    return span == 0 ? 0.0 : d;
}
// the output element(s) of a point at element `at` of the box's view: d holds N derivatives (DERIV: d[0] alone)
template <int N>
__device__ __forceinline__ void grd_store(void *dst, int64_t at, const double *d, const szk_gradient_opts &o) {
    if (o.op == SZ3HIP_GRADIENT_VECTOR) {
        if (o.out_type == 0) {
            float *p = static_cast<float *>(dst) + at * N;
#pragma unroll
            for (int j = 0; j < N; j++) p[j] = (float)d[j];
        } else {
            double *p = static_cast<double *>(dst) + at * N;
#pragma unroll
            for (int j = 0; j < N; j++) p[j] = d[j];
        }
        return;
    }
    double r = d[0];
    if (o.op != SZ3HIP_GRADIENT_DERIV) {
        double m = 0.0;
#pragma unroll
        for (int j = 0; j < N; j++) m = m + d[j] * d[j];
        r = o.op == SZ3HIP_GRADIENT_MAG ? sqrt(m) : m;
    }
    if (o.out_type == 0) static_cast<float *>(dst)[at] = (float)r;
    else static_cast<double *>(dst)[at] = r;
}

// I: the index type of the output point's decomposition (32-bit where the box's output points fit: uniform over the workgroup)
template <typename T, int N, typename I>
__device__ __forceinline__ void grd_point(const T *__restrict__ src, const Box &b, const szk_gradient_box &g, const szk_gradient_opts &o, const uint64_t *oe, I t) {
    const bool all = o.op != SZ3HIP_GRADIENT_DERIV;
    const bool interior = (o.flags & SZ3HIP_GRADIENT_INTERIOR) != 0;
    // the point: its coordinates in the box, its source offset and its element in the view
    uint64_t at = b.src, ci[N];
    int64_t to = 0;
    I rem = t;
#pragma unroll
    for (int j = N - 1; j >= 0; j--) {
        const int p = 4 - N + j;
        I c;
        if (j > 0) {
            const I e = (I)oe[j], q = rem / e;
            c = rem - q * e;
            rem = q;
        } else c = rem;
        to += (int64_t)c * g.dstr[p];
        ci[j] = (uint64_t)c + (interior && (all || (uint32_t)p == o.axis) ? 1u : 0u);
        at += ci[j] * b.str[p];
    }
    double d[N];
    if (!all) {  // (uniform) one axis: its extent, index, stride and grid step picked without indexing the record by a register
        uint64_t E = 1, i = 0, st = 0;
        double s = 1.0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const int p = 4 - N + j;
            if ((uint32_t)p == o.axis) {
                E = b.ext[p];
                i = ci[j];
                st = b.str[p];
                s = g.scale[p];
            }
        }
        const uint32_t up = i + 1 < E ? 1u : 0u, dn = i > 0 ? 1u : 0u;
        const T vp = src[at + (up ? st : 0)], vm = src[at - (dn ? st : 0)];
        d[0] = grd_deriv((double)vp, (double)vm, up + dn, s);
    } else {
        T vp[N], vm[N];
        uint32_t span[N];
#pragma unroll
        for (int j = 0; j < N; j++) {
            const int p = 4 - N + j;
            const uint64_t E = b.ext[p], i = ci[j], st = b.str[p];
            const uint32_t up = i + 1 < E ? 1u : 0u, dn = i > 0 ? 1u : 0u;
            vp[j] = src[at + (up ? st : 0)];
            vm[j] = src[at - (dn ? st : 0)];
            span[j] = up + dn;
        }
#pragma unroll
        for (int j = 0; j < N; j++) d[j] = grd_deriv((double)vp[j], (double)vm[j], span[j], g.scale[4 - N + j]);
    }
    grd_store<N>(g.dst, to, d, o);
}

template <typename T, int N>
__device__ __forceinline__ void grd_box(const T *__restrict__ src, const Box &b, const szk_gradient_box &g, const szk_gradient_opts &o) {
    const bool all = o.op != SZ3HIP_GRADIENT_DERIV;
    const bool interior = (o.flags & SZ3HIP_GRADIENT_INTERIOR) != 0;
    uint64_t oe[N], total = 1;  // the output box (the host has checked: a trimmed extent is at least 3)
#pragma unroll
    for (int j = 0; j < N; j++) {
        const int p = 4 - N + j;
        oe[j] = b.ext[p] - (interior && (all || (uint32_t)p == o.axis) ? 2u : 0u);
        total *= oe[j];
    }
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    if (total <= 0xFFFFFFFFull) grd_point<T, N, uint32_t>(src, b, g, o, oe, (uint32_t)t);
    else grd_point<T, N, uint64_t>(src, b, g, o, oe, t);
}

template <typename T, int N>
__global__ __launch_bounds__(256) void k_region_gradient(const T *__restrict__ src, const Box *__restrict__ recs, szk_gradient_opts opts) {
    const szk_gradient_box *gs = reinterpret_cast<const szk_gradient_box *>(recs + gridDim.y);  // (the boxes' entries lie behind the launch's records)
    grd_box<T, N>(src, recs[blockIdx.y], gs[blockIdx.y], opts);
}
template <typename T, int N>
__global__ __launch_bounds__(256) void k_region_gradient_view(const T *__restrict__ src, Box rec, szk_gradient_box g, szk_gradient_opts opts) {
    grd_box<T, N>(src, rec, g, opts);
}

template <typename T, int N>
void gradient_launch(const T *src, const Box *d_recs, const Box *rec, const szk_gradient_box *g, dim3 grid, const szk_gradient_opts &o, hipStream_t s) {
    if (d_recs) hipLaunchKernelGGL((k_region_gradient<T, N>), grid, dim3(256), 0, s, src, d_recs, o);
    else hipLaunchKernelGGL((k_region_gradient_view<T, N>), grid, dim3(256), 0, s, src, *rec, *g, o);
}
template <typename T>
void gradient_launch_dims(const T *src, const Box *d_recs, const Box *rec, const szk_gradient_box *g, dim3 grid, const szk_gradient_opts &o, hipStream_t s) {
    switch (o.N) {
    case 1: gradient_launch<T, 1>(src, d_recs, rec, g, grid, o, s); break;
    case 2: gradient_launch<T, 2>(src, d_recs, rec, g, grid, o, s); break;
    case 3: gradient_launch<T, 3>(src, d_recs, rec, g, grid, o, s); break;
    default: gradient_launch<T, 4>(src, d_recs, rec, g, grid, o, s);
    }
}
}  // namespace

int szk_launch_region_gradient(int dtype, const void *d_src, const Box *d_recs, const Box *rec_by_value, uint32_t n, const szk_region_sink *sink, hipStream_t s) {
    if (!sink || sink->kind != SZK_SINK_GRADIENT || !sink->grd_boxes || !d_src || n < 1 || n > 65535) return -1;
    if ((d_recs == nullptr) == (rec_by_value == nullptr) || (rec_by_value && n != 1)) return -1;
    const szk_gradient_opts &o = sink->grd;
    if (o.op > SZ3HIP_GRADIENT_VECTOR || o.out_type > 1 || o.N < 1 || o.N > 4 || o.axis > 3 || o.axis < 4 - o.N) return -1;
    const uint64_t gx = (sink->grd_threads + 255) / 256;
    if (gx < 1 || gx > 0x7FFFFFFFull) return -1;
    const dim3 grid((uint32_t)gx, n);
    if (dtype == 0) gradient_launch_dims<float>((const float *)d_src, d_recs, rec_by_value, sink->grd_boxes, grid, o, s);
    else gradient_launch_dims<double>((const double *)d_src, d_recs, rec_by_value, sink->grd_boxes, grid, o, s);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// sz3_amd/csrc/sz3hip_composite.hip — boxes composited front to back along one axis through an RGBA table: ONE launch
// in the strided gather's place, over the gather's own records (`src`, `ext`, `str`; the `dst` word names the box, `dstr` is not read), a
// szk_composite_box per record behind them: the real destination, its strides in OUTPUT elements and the squarings s of the box's opacities.
//
//   k_region_composite<T>       blockIdx.y: the box, a thread per OUTPUT point, lanes along x: at step i a wave's loads are one row segment.
//                               The fold is serial per thread; CMP_BATCH loads are issued ahead of the CMP_BATCH folds they feed. A lane whose
//                               column has stopped keeps its state; the loop leaves once the whole wave has stopped (a ballot: uniform).
//   k_region_composite_rows<T>  the axis is the fastest dimension that counts (every dimension behind it has extent 1): a wave owns 64
//                               columns of the box ("rows" of the source). Per step it loads 64 rows x CMP COLS = 128 / sizeof(T) points —
//                               one load instruction is RPI = 64 / COLS row segments — into a wave-private LDS tile of row pitch COLS + 1
//                               elements, then lane = row folds its COLS points in the visiting order. Half the projection's tile width:
//                               4 x 64 x 33 x 4 = 33.8 KB (f64: 4 x 64 x 17 x 8 = 34.8 KB) and the table's 20 KB leave room for two
//                               workgroups in a CU's 160 KB. Banks: f32 row writes are ds_write_b32, a group of 32 lanes is one row
//                               segment of 32 consecutive dwords; the transposed reads are dword l * 33 + c, bank (l + c) % 32 within a
//                               group of 32 lanes. f64 row writes are ds_write_b64, a group of 16 lanes is one row segment of 16
//                               consecutive doubles; the transposed reads are dwords l * 34 + 2 c, banks (34 l + 2 c) % 64, 34 l % 64 =
//                               2 (17 l % 32) distinct over a group of 32 lanes. No conflicts either way.
//   ..._view                    the same over ONE record and ONE szk_composite_box passed by value (sz3hip_composite_device)
//
// The table is staged in LDS once per workgroup: three floats of colour and the opacity AS A DOUBLE per entry (20 bytes, 20 KB at most) —
// the opacity after s squarings, 1.0 - t, is a double by the rule and is worked out here once per entry, not per point. One barrier that
// every thread of a workgroup with work reaches; a workgroup wholly beyond its box leaves before it. An output point depends on its column,
// the box's s and the options alone (cmp_fold, cmp_store below): both bodies, every route and every grid give the same bytes. All
// arithmetic is IEEE double without a fused multiply-add (the build's -ffp-contract=off, and the pragma below). No atomics, nothing waits
// across workgroups, plain vector loads and stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sz3hip.h"
#include "sz3hip_kernels.h"

#pragma clang fp contract(off)

namespace {
static_assert(sizeof(sz3hip_composite_opts) == 56 && sizeof(sz3hip_composite_plan) == 48, "the header's sizes");
static_assert(sizeof(szk_composite_box) == SZK_COMPOSITE_WORDS * 8, "a box's words in the table");
using Box = szk_region_gather_strided_box;
constexpr int CMP_BATCH = 8;  // loads in flight per thread ahead of the fold

struct CmpTable {
    float rgb[SZ3HIP_MAX_LUT * 3];
    double a[SZ3HIP_MAX_LUT];  // the opacity after the box's squarings
};
// a column's state; done: the column has stopped (or the lane has none)
struct CmpAcc {
    double R, G, B, A;
    bool done;
};

// the table into LDS, the opacities corrected for s squarings; every thread of the workgroup comes here
__device__ __forceinline__ void cmp_stage(CmpTable &tab, const szk_composite_opts &o, uint64_t s) {
    const float4 *lut = reinterpret_cast<const float4 *>(o.d_lut);
    for (uint32_t k = threadIdx.x; k < o.win.lut_n; k += 256) {
        const float4 e = lut[k];
        tab.rgb[3 * k] = e.x;
        tab.rgb[3 * k + 1] = e.y;
        tab.rgb[3 * k + 2] = e.z;
        double a = (double)e.w;
        if (s) {
            double t = 1.0 - a;
            for (uint64_t q = 0; q < s; q++) t = t * t;
            a = 1.0 - t;
        }
        tab.a[k] = a;
    }
    __syncthreads();
}
__device__ __forceinline__ void cmp_init(CmpAcc &acc, const void *dst, int64_t at, const szk_composite_opts &o) {
    acc.R = acc.G = acc.B = acc.A = 0.0;
    acc.done = false;
    if (o.flags & SZ3HIP_COMPOSITE_ACCUMULATE) {  // (RGBA32F: the host has checked)
        const float4 f = static_cast<const float4 *>(dst)[at];
        acc.R = (double)f.x;
        acc.G = (double)f.y;
        acc.B = (double)f.z;
        acc.A = (double)f.w;
    }
}
// one visited point
template <typename T>
__device__ __forceinline__ void cmp_fold(CmpAcc &acc, T v, const CmpTable &tab, const szk_composite_opts &o) {
    const double x = (double)v;
    if (acc.done || x != x) return;
    const uint32_t c = szk_map_code(x, o.win);
    const double a = tab.a[c], r = (double)tab.rgb[3 * c], g = (double)tab.rgb[3 * c + 1], b = (double)tab.rgb[3 * c + 2];
    const double w = (1.0 - acc.A) * a;
    acc.R = acc.R + w * r;
    acc.G = acc.G + w * g;
    acc.B = acc.B + w * b;
    acc.A = acc.A + w;
    if (acc.A >= o.cutoff) acc.done = true;
}
__device__ __forceinline__ uint32_t cmp_byte(double c) {
    const double q = c * 255.0 + 0.5;
    return q > 0 ? (q >= 255 ? 255u : (uint32_t)(uint8_t)q) : 0u;  // (a NaN: 0)
}
// the output element of a finished column, stored at element `at` of the box's view
__device__ __forceinline__ void cmp_store(void *dst, int64_t at, const CmpAcc &acc, const szk_composite_opts &o) {
    if (o.out_type == SZ3HIP_COMPOSITE_RGBA32F) {
        static_cast<float4 *>(dst)[at] = make_float4((float)acc.R, (float)acc.G, (float)acc.B, (float)acc.A);
    } else {
        static_cast<uint32_t *>(dst)[at] = cmp_byte(acc.R) | cmp_byte(acc.G) << 8 | cmp_byte(acc.B) << 16 | cmp_byte(acc.A) << 24;
    }
}
__device__ __forceinline__ bool cmp_wave_done(bool done) { return __builtin_amdgcn_ballot_w64(!done) == 0; }

// output point t of the box: its column's first element in the source, its element in the view (the gather's index arithmetic, the axis left out)
__device__ __forceinline__ void cmp_point(const Box &b, const szk_composite_box &g, uint32_t a, uint64_t t, uint64_t *so, int64_t *dx) {
    uint64_t r = t, s = b.src;
    int64_t d = 0;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        if ((uint32_t)j == a) continue;
        const uint64_t q = r % b.ext[j];
        s += q * b.str[j];
        d += (int64_t)q * g.dstr[j];
        r /= b.ext[j];
    }
    *so = s;
    *dx = d;
}

// a thread per output point
template <typename T>
__device__ __forceinline__ void composite_point(const T *__restrict__ src, const Box &b, const szk_composite_box &g, const szk_composite_opts &o) {
    __shared__ CmpTable tab;
    const uint32_t a = o.axis;
    const uint64_t E = b.ext[a], sa = b.str[a], outs = b.total / E;
    if ((uint64_t)blockIdx.x * 256 >= outs) return;  // (the whole workgroup, before the barrier)
    cmp_stage(tab, o, g.s);
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= outs) return;
    uint64_t so;
    int64_t dx;
    cmp_point(b, g, a, t, &so, &dx);
    CmpAcc acc;
    cmp_init(acc, g.dst, dx, o);
    // REVERSE: the start and the step's sign, nothing else
    const bool rev = (o.flags & SZ3HIP_COMPOSITE_REVERSE) != 0;
    const int64_t step = rev ? -(int64_t)sa : (int64_t)sa;
    const T *p = src + so + (rev ? (E - 1) * sa : 0);
    uint64_t i = 0;
    for (; i + CMP_BATCH <= E; i += CMP_BATCH) {
        if (cmp_wave_done(acc.done)) break;  // (uniform: no load is issued for a wave that is done)
        T v[CMP_BATCH];
#pragma unroll
        for (int k = 0; k < CMP_BATCH; k++) v[k] = p[(int64_t)(i + k) * step];
#pragma unroll
        for (int k = 0; k < CMP_BATCH; k++) cmp_fold(acc, v[k], tab, o);
    }
    for (; i < E; i++) {
        if (cmp_wave_done(acc.done)) break;
        cmp_fold(acc, p[(int64_t)i * step], tab, o);
    }
    cmp_store(g.dst, dx, acc, o);
}

// the axis is the fastest dimension that counts: 64 rows of the source per wave through a wave-private LDS tile
template <typename T>
struct CmpTile {
    static constexpr uint32_t COLS = 128 / sizeof(T), PITCH = COLS + 1, RPI = 64 / COLS;  // RPI: rows one load instruction covers
};
__device__ __forceinline__ uint64_t cmp_shfl(uint64_t v, uint32_t lane) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)lane, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)lane, 64);
    return (uint64_t)hi << 32 | lo;
}
template <typename T>
__device__ __forceinline__ void composite_rows(const T *__restrict__ src, const Box &b, const szk_composite_box &g, const szk_composite_opts &o) {
    using L = CmpTile<T>;
    __shared__ T tiles[4][64 * L::PITCH];
    __shared__ CmpTable tab;
    const uint32_t a = o.axis, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t E = b.ext[a], sa = b.str[a], rows = b.total / E;
    if ((uint64_t)blockIdx.x * 256 >= rows) return;  // (the whole workgroup, before the barrier)
    cmp_stage(tab, o, g.s);
    const uint64_t first = (uint64_t)blockIdx.x * 256 + 64 * wave;  // the wave's first row
    if (first >= rows) return;                                     // (the whole wave: nothing below waits for another wave)
    const uint32_t nrows = rows - first < 64 ? (uint32_t)(rows - first) : 64u;
    T *tile = tiles[wave];
    uint64_t so = 0;
    int64_t dx = 0;
    CmpAcc acc;
    acc.R = acc.G = acc.B = acc.A = 0.0;
    acc.done = true;  // (a lane without a row has stopped)
    if (lane < nrows) {
        cmp_point(b, g, a, first + lane, &so, &dx);
        cmp_init(acc, g.dst, dx, o);
    }
    const bool rev = (o.flags & SZ3HIP_COMPOSITE_REVERSE) != 0;
    const uint32_t col = lane % L::COLS, sub = lane / L::COLS;
    for (uint64_t j0 = 0; j0 < E; j0 += L::COLS) {  // j: the place in the visiting order
        if (cmp_wave_done(acc.done)) break;          // (uniform: every lane of the wave is here)
        const uint32_t ncols = E - j0 < L::COLS ? (uint32_t)(E - j0) : L::COLS;
        // rows and columns beyond the box are clamped onto its last ones: every load has a valid address and none sits behind a branch
        const uint64_t jj = j0 + col < E ? j0 + col : E - 1;
        const uint64_t cc = (rev ? E - 1 - jj : jj) * sa;
        for (uint32_t r0 = 0; r0 < nrows; r0 += CMP_BATCH * L::RPI) {
            T v[CMP_BATCH];
#pragma unroll
            for (int k = 0; k < CMP_BATCH; k++) {
                const uint32_t r = r0 + L::RPI * k + sub;
                v[k] = src[cmp_shfl(so, r < nrows ? r : nrows - 1) + cc];
            }
#pragma unroll
            for (int k = 0; k < CMP_BATCH; k++) tile[(r0 + L::RPI * k + sub) * L::PITCH + col] = v[k];  // (at most row 63: 64 is a multiple of the batch's rows)
        }
        // the tile's writes before its transposed reads: the lanes of a wave issue in step and a wave's LDS operations complete in order;
        // the fences keep the compiler from moving either across. Every lane of the wave is here, rows beyond the box included.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < nrows) {
            const T *row = tile + lane * L::PITCH;
            for (uint32_t c = 0; c < ncols; c++) cmp_fold(acc, row[c], tab, o);
        }
        // ... and the reads before the next step's writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane < nrows) cmp_store(g.dst, dx, acc, o);
}

template <typename T>
__global__ __launch_bounds__(256) void k_region_composite(const T *__restrict__ src, const Box *__restrict__ recs, szk_composite_opts opts) {
    const szk_composite_box *gs = reinterpret_cast<const szk_composite_box *>(recs + gridDim.y);  // (the boxes' entries lie behind the launch's records)
    composite_point<T>(src, recs[blockIdx.y], gs[blockIdx.y], opts);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_composite_view(const T *__restrict__ src, Box rec, szk_composite_box g, szk_composite_opts opts) {
    composite_point<T>(src, rec, g, opts);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_composite_rows(const T *__restrict__ src, const Box *__restrict__ recs, szk_composite_opts opts) {
    const szk_composite_box *gs = reinterpret_cast<const szk_composite_box *>(recs + gridDim.y);
    composite_rows<T>(src, recs[blockIdx.y], gs[blockIdx.y], opts);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_composite_rows_view(const T *__restrict__ src, Box rec, szk_composite_box g, szk_composite_opts opts) {
    composite_rows<T>(src, rec, g, opts);
}

template <typename T>
void composite_launch(bool rows, const T *src, const Box *d_recs, const Box *rec, const szk_composite_box *g, dim3 grid, const szk_composite_opts &o, hipStream_t s) {
    if (rows) {
        if (d_recs) hipLaunchKernelGGL((k_region_composite_rows<T>), grid, dim3(256), 0, s, src, d_recs, o);
        else hipLaunchKernelGGL((k_region_composite_rows_view<T>), grid, dim3(256), 0, s, src, *rec, *g, o);
        return;
    }
    if (d_recs) hipLaunchKernelGGL((k_region_composite<T>), grid, dim3(256), 0, s, src, d_recs, o);
    else hipLaunchKernelGGL((k_region_composite_view<T>), grid, dim3(256), 0, s, src, *rec, *g, o);
}
}  // namespace

int szk_launch_region_composite(int dtype, const void *d_src, const Box *d_recs, const Box *rec_by_value, uint32_t n, const szk_region_sink *sink, hipStream_t s) {
    if (!sink || sink->kind != SZK_SINK_COMPOSITE || !sink->cmp_boxes || !d_src || n < 1 || n > 65535) return -1;
    if ((d_recs == nullptr) == (rec_by_value == nullptr) || (rec_by_value && n != 1)) return -1;
    const szk_composite_opts &o = sink->cmp;
    if (o.out_type > SZ3HIP_COMPOSITE_RGBA8 || o.N < 1 || o.N > 4 || o.axis > 3 || o.axis < 4 - o.N) return -1;
    if (!o.d_lut || o.win.lut_n < 2 || o.win.lut_n > SZ3HIP_MAX_LUT || o.win.M != o.win.lut_n - 1) return -1;
    if (rec_by_value && sink->cmp_boxes[0].s > 30) return -1;
    const uint64_t gx = (sink->cmp_threads + 255) / 256;
    if (gx < 1 || gx > 0x7FFFFFFFull) return -1;
    const dim3 grid((uint32_t)gx, n);
    if (dtype == 0) composite_launch<float>(sink->cmp_rows, (const float *)d_src, d_recs, rec_by_value, sink->cmp_boxes, grid, o, s);
    else composite_launch<double>(sink->cmp_rows, (const double *)d_src, d_recs, rec_by_value, sink->cmp_boxes, grid, o, s);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

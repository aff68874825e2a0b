// sz3_amd/csrc/sz3hip_project.hip — boxes collapsed along one axis: ONE launch in the strided gather's place, over the
// gather's own records, real `dst` and `dstr` included (in OUTPUT elements; the entry at the axis is not read).
//
//   k_region_project<T, CLS>       blockIdx.y: the box, a thread per OUTPUT point, lanes along x: at step i a wave's loads are one row segment.
//                                  The fold is serial per thread; PRJ_BATCH loads are issued ahead of the PRJ_BATCH folds they feed.
//   k_region_project_rows<T, CLS>  the axis is the fastest dimension that counts (every dimension behind it has extent 1): a wave owns 64
//                                  columns of the box ("rows" of the source). Per step it loads 64 rows x PRJ_COLS = 256 / sizeof(T) points
//                                  — one load instruction is one row segment (f64: two), the lane is the position along the axis — into a
//                                  wave-private LDS tile of row pitch PRJ_COLS + 1 elements, then lane = row folds its PRJ_COLS points in
//                                  ascending order. Row writes and transposed reads are free of bank conflicts (f32: dword l * 65 + c is
//                                  bank (l + c) % 32 per 32-lane half; f64: dwords l * 66 + 2 c, banks (2 l + 2 c) % 64).
//   ..._view                       the same over ONE record passed by value (sz3hip_project_device)
//
// CLS: PRJ_EXT (MIN, MAX, ARGMIN, ARGMAX) or PRJ_ADD (SUM, MEAN, COUNT); the op within the class is a uniform branch outside the loops. The
// result of an output point depends on its column, the op and the options alone (prj_fold, prj_store below): both bodies, every route and
// every grid give the same bytes. No atomics, nothing waits across workgroups — or across waves: the tile is a wave's own, and wavefront
// fences stand between its writes and its transposed reads.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sz3hip.h"
#include "sz3hip_kernels.h"

namespace {
static_assert(sizeof(sz3hip_project_opts) == 24 && sizeof(sz3hip_project_plan) == 48, "the header's sizes");
using Box = szk_region_gather_strided_box;
constexpr int PRJ_EXT = 0, PRJ_ADD = 1;
constexpr int PRJ_BATCH = 8;  // loads in flight per thread ahead of the fold

// a column's state. PRJ_EXT: d the best key so far (x for a maximum, -x for a minimum: the negation is exact and keeps the order's ties;
// -Inf: no finite point yet — every finite key lies above it), u its index (E: none). PRJ_ADD: d the sum, u the finite count.
struct PrjAcc {
    double d;
    uint32_t u;
};
template <int CLS>
__device__ __forceinline__ PrjAcc prj_init(uint64_t E) {
    PrjAcc a;
    a.d = CLS == PRJ_EXT ? -INFINITY : 0.0;
    a.u = CLS == PRJ_EXT ? (uint32_t)E : 0u;
    return a;
}
template <int CLS, typename T>
__device__ __forceinline__ void prj_fold(PrjAcc &a, T v, uint32_t i, bool neg) {
    const double x = (double)v;
    const bool fin = fabs(x) < INFINITY;
    if constexpr (CLS == PRJ_EXT) {
        const double key = neg ? -x : x;
        if (fin && key > a.d) {  // (strictly above: of equal keys, -0.0 and +0.0 among them, the first stays)
            a.d = key;
            a.u = i;
        }
    } else {
        if (fin) {
            a.d = a.d + x;
            a.u++;
        }
    }
}
// the output element of a finished column, stored at element `at` of the box's view
template <int CLS>
__device__ __forceinline__ void prj_store(void *dst, int64_t at, const PrjAcc &a, const szk_project_opts &o) {
    double r;
    if constexpr (CLS == PRJ_EXT) {
        if (o.op == SZ3HIP_PROJECT_ARGMIN || o.op == SZ3HIP_PROJECT_ARGMAX) {
            static_cast<uint32_t *>(dst)[at] = a.u;
            return;
        }
        r = a.d > -INFINITY ? (o.op == SZ3HIP_PROJECT_MIN ? -a.d : a.d) : o.fill;
    } else {
        if (o.op == SZ3HIP_PROJECT_COUNT) {
            static_cast<uint32_t *>(dst)[at] = a.u;
            return;
        }
        r = o.op == SZ3HIP_PROJECT_SUM ? a.d : a.u ? a.d / (double)a.u : o.fill;
    }
    if (o.out_type == 0) static_cast<float *>(dst)[at] = (float)r;
    else static_cast<double *>(dst)[at] = r;
}
__device__ __forceinline__ bool prj_neg(const szk_project_opts &o) { return o.op == SZ3HIP_PROJECT_MIN || o.op == SZ3HIP_PROJECT_ARGMIN; }

// output point t of the box: its column's first element in the source, its element in the view (the gather's index arithmetic, the axis left out)
__device__ __forceinline__ void prj_point(const Box &b, uint32_t a, uint64_t t, uint64_t *so, int64_t *dx) {
    uint64_t r = t, s = b.src;
    int64_t d = 0;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        if ((uint32_t)j == a) continue;
        const uint64_t q = r % b.ext[j];
        s += q * b.str[j];
        d += (int64_t)q * b.dstr[j];
        r /= b.ext[j];
    }
    *so = s;
    *dx = d;
}

// a thread per output point
template <typename T, int CLS>
__device__ __forceinline__ void project_point(const T *__restrict__ src, const Box &b, const szk_project_opts &o) {
    const uint32_t a = o.axis;
    const uint64_t E = b.ext[a], sa = b.str[a], t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= b.total / E) return;
    uint64_t so;
    int64_t dx;
    prj_point(b, a, t, &so, &dx);
    const bool neg = prj_neg(o);
    PrjAcc acc = prj_init<CLS>(E);
    const T *p = src + so;
    uint64_t i = 0;
    for (; i + PRJ_BATCH <= E; i += PRJ_BATCH) {
        T v[PRJ_BATCH];
#pragma unroll
        for (int k = 0; k < PRJ_BATCH; k++) v[k] = p[(i + k) * sa];
#pragma unroll
        for (int k = 0; k < PRJ_BATCH; k++) prj_fold<CLS>(acc, v[k], (uint32_t)(i + k), neg);
    }
    for (; i < E; i++) prj_fold<CLS>(acc, p[i * sa], (uint32_t)i, neg);
    prj_store<CLS>(b.dst, dx, acc, o);
}

// the axis is the fastest dimension that counts: 64 rows of the source per wave through a wave-private LDS tile
template <typename T>
struct PrjTile {
    static constexpr uint32_t COLS = 256 / sizeof(T), PITCH = COLS + 1, RPI = 64 / COLS;  // RPI: rows one load instruction covers
};
__device__ __forceinline__ uint64_t prj_readlane(uint64_t v, uint32_t lane) {  // (lane is uniform)
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane);
    return (uint64_t)hi << 32 | lo;
}
template <typename T, int CLS>
__device__ __forceinline__ void project_rows(const T *__restrict__ src, const Box &b, const szk_project_opts &o) {
    using L = PrjTile<T>;
    __shared__ T tiles[4][64 * L::PITCH];
    const uint32_t a = o.axis, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t E = b.ext[a], sa = b.str[a], rows = b.total / E;
    const uint64_t first = (uint64_t)blockIdx.x * 256 + 64 * wave;  // the wave's first row
    if (first >= rows) return;                                     // (the whole wave: nothing below waits for another wave)
    const uint32_t nrows = rows - first < 64 ? (uint32_t)(rows - first) : 64u;
    T *tile = tiles[wave];
    uint64_t so = 0;
    int64_t dx = 0;
    if (lane < nrows) prj_point(b, a, first + lane, &so, &dx);
    const bool neg = prj_neg(o);
    PrjAcc acc = prj_init<CLS>(E);
    const uint32_t col = lane % L::COLS, sub = lane / L::COLS;
    for (uint64_t c0 = 0; c0 < E; c0 += L::COLS) {
        const uint32_t ncols = E - c0 < L::COLS ? (uint32_t)(E - c0) : L::COLS;
        // rows and columns beyond the box are clamped onto its last ones: every load has a valid address and none sits behind a branch
        const uint64_t cc = (c0 + col < E ? c0 + col : E - 1) * sa;
        for (uint32_t r0 = 0; r0 < nrows; r0 += PRJ_BATCH * L::RPI) {
            T v[PRJ_BATCH];
#pragma unroll
            for (int k = 0; k < PRJ_BATCH; k++) {
                uint64_t off;
                if constexpr (L::RPI == 1) {
                    const uint32_t r = r0 + k;
                    off = prj_readlane(so, r < nrows ? r : nrows - 1);
                } else {
                    const uint32_t r = r0 + 2 * k;
                    const uint64_t o0 = prj_readlane(so, r < nrows ? r : nrows - 1), o1 = prj_readlane(so, r + 1 < nrows ? r + 1 : nrows - 1);
                    off = sub ? o1 : o0;
                }
                v[k] = src[off + cc];
            }
#pragma unroll
            for (int k = 0; k < PRJ_BATCH; k++) tile[(r0 + L::RPI * k + sub) * L::PITCH + col] = v[k];  // (r0 + ... <= 63: 64 is a multiple of the batch's rows)
        }
        // the tile's writes before its transposed reads: the lanes of a wave issue in step and a wave's LDS operations complete in order;
        // the fences keep the compiler from moving either across. Every lane of the wave is here, rows beyond the box included.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < nrows) {
            const T *row = tile + lane * L::PITCH;
            if (ncols == L::COLS) {
#pragma unroll 8
                for (uint32_t c = 0; c < L::COLS; c++) prj_fold<CLS>(acc, row[c], (uint32_t)(c0 + c), neg);
            } else {
                for (uint32_t c = 0; c < ncols; c++) prj_fold<CLS>(acc, row[c], (uint32_t)(c0 + c), neg);
            }
        }
        // ... and the reads before the next step's writes
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (lane < nrows) prj_store<CLS>(b.dst, dx, acc, o);
}

template <typename T, int CLS>
__global__ __launch_bounds__(256) void k_region_project(const T *__restrict__ src, const Box *__restrict__ recs, szk_project_opts opts) {
    project_point<T, CLS>(src, recs[blockIdx.y], opts);
}
template <typename T, int CLS>
__global__ __launch_bounds__(256) void k_region_project_view(const T *__restrict__ src, Box rec, szk_project_opts opts) {
    project_point<T, CLS>(src, rec, opts);
}
template <typename T, int CLS>
__global__ __launch_bounds__(256) void k_region_project_rows(const T *__restrict__ src, const Box *__restrict__ recs, szk_project_opts opts) {
    project_rows<T, CLS>(src, recs[blockIdx.y], opts);
}
template <typename T, int CLS>
__global__ __launch_bounds__(256) void k_region_project_rows_view(const T *__restrict__ src, Box rec, szk_project_opts opts) {
    project_rows<T, CLS>(src, rec, opts);
}

template <typename T, int CLS>
void project_launch(bool rows, const T *src, const Box *d_recs, const Box *rec, dim3 grid, const szk_project_opts &o, hipStream_t s) {
    if (rows) {
        if (d_recs) hipLaunchKernelGGL((k_region_project_rows<T, CLS>), grid, dim3(256), 0, s, src, d_recs, o);
        else hipLaunchKernelGGL((k_region_project_rows_view<T, CLS>), grid, dim3(256), 0, s, src, *rec, o);
        return;
    }
    if (d_recs) hipLaunchKernelGGL((k_region_project<T, CLS>), grid, dim3(256), 0, s, src, d_recs, o);
    else hipLaunchKernelGGL((k_region_project_view<T, CLS>), grid, dim3(256), 0, s, src, *rec, o);
}
template <typename T>
void project_launch_class(bool rows, const T *src, const Box *d_recs, const Box *rec, dim3 grid, const szk_project_opts &o, hipStream_t s) {
    const bool ext = o.op == SZ3HIP_PROJECT_MIN || o.op == SZ3HIP_PROJECT_MAX || o.op == SZ3HIP_PROJECT_ARGMIN || o.op == SZ3HIP_PROJECT_ARGMAX;
    if (ext) project_launch<T, PRJ_EXT>(rows, src, d_recs, rec, grid, o, s);
    else project_launch<T, PRJ_ADD>(rows, src, d_recs, rec, grid, o, s);
}
}  // namespace

int szk_launch_region_project(int dtype, const void *d_src, const Box *d_recs, const Box *rec_by_value, uint32_t n, const szk_region_sink *sink, hipStream_t s) {
    if (!sink || sink->kind != SZK_SINK_PROJECT || !d_src || n < 1 || n > 65535) return -1;
    if ((d_recs == nullptr) == (rec_by_value == nullptr) || (rec_by_value && n != 1)) return -1;
    const szk_project_opts &o = sink->prj;
    if (o.op > SZ3HIP_PROJECT_COUNT || o.axis > 3 || o.out_type > 1 || o.N < 1 || o.N > 4 || o.axis < 4 - o.N) return -1;
    const uint64_t gx = (sink->prj_threads + 255) / 256;
    if (gx < 1 || gx > 0x7FFFFFFFull) return -1;
    const dim3 grid((uint32_t)gx, n);
    if (dtype == 0) project_launch_class<float>(sink->prj_rows, (const float *)d_src, d_recs, rec_by_value, grid, o, s);
    else project_launch_class<double>(sink->prj_rows, (const double *)d_src, d_recs, rec_by_value, grid, o, s);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

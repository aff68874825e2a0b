// sz3_amd/csrc/sz3hip_verify.hip — error statistics of two arrays in device memory (sz3hip_verify_device): what the reference's
// verify<T> prints (utils/Statistic.hpp:79-137: Min, Max, range, max absolute error, max point-wise relative error, PSNR, NRMSE,
// normError, normErr_norm, acEff), reduced where the arrays lie, each array read ONCE.
//
//   k_verify<T, CONTIG, VEC>   the reduction: one szk_verify_rec per workgroup            (reference loops: Statistic.hpp:84-118)
//   k_verify_final             one workgroup folds those records into d_result (a launch of its own, like k_minmax_final: no
//                              hand-off between workgroups inside a launch)
//
// Per element a = ori, b = dec. Float types: e = |(double)b - (double)a|. Integer types: the difference is taken exactly, as the
// unsigned magnitude at the type's width, then converted to double (an int64 / uint64 pair beyond 2^53 that differs by 1 reports 1.0);
// a and b themselves enter the sums as (double). Every accumulator is f64 whatever T is.
//
// Non-finite positions: a position where a or b is NaN or +-Inf is counted in n_nonfinite and left out of every other statistic; it
// is also counted in n_nonfinite_mismatch when the two are not of the same kind (one NaN and the other not, an infinity against
// anything but the same infinity). With n_nonfinite == 0 every number means what the reference's verify means. The reference's own
// NaN behaviour depends on the element order (Max = ori_data[0], then "<": Statistic.hpp:84-96) and is NOT reproduced.
//
// Indices (argmax, first_over) are row-major indices over the view's logical extents; they travel through the lane, wave, LDS and final
// folds as (value, index) pairs, "smaller index wins ties": no atomics anywhere.
//
// acEff in one pass: every lane accumulates the moments of a - K and b - K, K = (double) the first finite ori element THAT LANE sees
// (a value inside the data's range, so the shift removes the offset of the data as the first element of the view would), turns them into a
// (count, mean_a, mean_b, M2_a, M2_b, C_ab) record when its loop ends, and records are merged pairwise from there on (Chan et al.:
// M2 += M2' + d^2 n n' / (n + n')): the merges do not cancel, and a lane's own sums hold n / lanes terms instead of n.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "sz3hip_kernels.h"

#include "sz3hip_devutil.h"

namespace {
#define SZK_VERIFY_CAP 2048  // workgroups of k_verify at most (= records k_verify_final folds): 8 per CU

// A lane's running state. A lane meets its elements in increasing index order (head, then its units or rows in order, then the tail), so
// inside a lane "the first of equal maxima" is a strict comparison; the folds compare (value, index) pairs. Lane counters are 32 bits wide:
// a lane of the capped grid sees n / 2^19 elements.
struct VAcc {
    uint32_t n_fin = 0, n_nonfinite = 0, n_mismatch = 0, n_over = 0;
    uint64_t first_over = ~0ull, argmax = ~0ull;
    double mn = INFINITY, mx = -INFINITY, max_diff = -1.0, max_pw_rel = 0.0;
    double sa = 0, sb = 0, see = 0, sbb = 0;
    double K = 0, da = 0, db = 0, daa = 0, dbb = 0, dab = 0;  // moments of a - K, b - K
};

template <typename T>
__device__ __forceinline__ void v_elem(VAcc &s, T A, T B, uint64_t idx, double bound) {
    const double a = (double)A, b = (double)B;
    double e;
    if constexpr (std::is_floating_point<T>::value) {
        const bool fa = fabs(a) < INFINITY, fb = fabs(b) < INFINITY;  // (false for NaN)
        if (!(fa && fb)) {
            s.n_nonfinite++;
            const bool same = (a != a && b != b) || (a == b);  // NaN with NaN, or the same infinity
            s.n_mismatch += same ? 0 : 1;
            return;
        }
        e = fabs(b - a);
    } else {
        using U = typename std::make_unsigned<T>::type;
        const U m = A > B ? (U)((U)A - (U)B) : (U)((U)B - (U)A);
        e = (double)m;
    }
    s.K = s.n_fin ? s.K : a;
    s.n_fin++;
    s.mn = fmin(s.mn, a);  // (both finite)
    s.mx = fmax(s.mx, a);
    const bool top = e > s.max_diff;
    s.max_diff = top ? e : s.max_diff;
    s.argmax = top ? idx : s.argmax;
    if (a != 0.0) s.max_pw_rel = fmax(s.max_pw_rel, e / fabs(a));  // (the one division per element)
    const bool over = e > bound;  // (bound = +Inf: none given)
    s.n_over += over ? 1 : 0;
    s.first_over = over && idx < s.first_over ? idx : s.first_over;
    s.sa += a;
    s.sb += b;
    s.see += e * e;
    s.sbb += b * b;
    const double ua = a - s.K, ub = b - s.K;
    s.da += ua;
    s.db += ub;
    s.daa = fma(ua, ua, s.daa);
    s.dbb = fma(ub, ub, s.dbb);
    s.dab = fma(ua, ub, s.dab);
}

__device__ __forceinline__ szk_verify_rec v_record(const VAcc &s) {
    szk_verify_rec r;
    r.n_fin = s.n_fin;
    r.n_nonfinite = s.n_nonfinite;
    r.n_mismatch = s.n_mismatch;
    r.n_over = s.n_over;
    r.first_over = s.first_over;
    r.argmax = s.argmax;
    r.mn = s.mn;
    r.mx = s.mx;
    r.max_diff = s.max_diff;
    r.max_pw_rel = s.max_pw_rel;
    r.sa = s.sa;
    r.sb = s.sb;
    r.see = s.see;
    r.sbb = s.sbb;
    if (s.n_fin) {
        const double m = (double)s.n_fin;
        r.mean_a = s.K + s.da / m;
        r.mean_b = s.K + s.db / m;
        r.m2a = s.daa - s.da * s.da / m;
        r.m2b = s.dbb - s.db * s.db / m;
        r.cab = s.dab - s.da * s.db / m;
    } else {
        r.mean_a = r.mean_b = r.m2a = r.m2b = r.cab = 0.0;
    }
    return r;
}

__device__ __forceinline__ void v_merge(szk_verify_rec &x, const szk_verify_rec &y) {
    if (y.max_diff > x.max_diff || (y.max_diff == x.max_diff && y.argmax < x.argmax)) {
        x.max_diff = y.max_diff;
        x.argmax = y.argmax;
    }
    x.first_over = y.first_over < x.first_over ? y.first_over : x.first_over;
    x.n_nonfinite += y.n_nonfinite;
    x.n_mismatch += y.n_mismatch;
    x.n_over += y.n_over;
    x.mn = y.mn < x.mn ? y.mn : x.mn;
    x.mx = y.mx > x.mx ? y.mx : x.mx;
    x.max_pw_rel = y.max_pw_rel > x.max_pw_rel ? y.max_pw_rel : x.max_pw_rel;
    x.sa += y.sa;
    x.sb += y.sb;
    x.see += y.see;
    x.sbb += y.sbb;
    if (y.n_fin) {
        if (!x.n_fin) {
            x.mean_a = y.mean_a;
            x.mean_b = y.mean_b;
            x.m2a = y.m2a;
            x.m2b = y.m2b;
            x.cab = y.cab;
        } else {
            const double nx = (double)x.n_fin, ny = (double)y.n_fin, nt = nx + ny;
            const double da = y.mean_a - x.mean_a, db = y.mean_b - x.mean_b, f = nx * ny / nt, w = ny / nt;
            x.m2a += y.m2a + da * da * f;
            x.m2b += y.m2b + db * db * f;
            x.cab += y.cab + da * db * f;
            x.mean_a += da * w;
            x.mean_b += db * w;
        }
        x.n_fin += y.n_fin;
    }
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, WAVE), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, WAVE);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ szk_verify_rec v_shfl_xor(const szk_verify_rec &r, int d) {
    szk_verify_rec o;
    o.n_fin = shfl_xor_u64(r.n_fin, d);
    o.n_nonfinite = shfl_xor_u64(r.n_nonfinite, d);
    o.n_mismatch = shfl_xor_u64(r.n_mismatch, d);
    o.n_over = shfl_xor_u64(r.n_over, d);
    o.first_over = shfl_xor_u64(r.first_over, d);
    o.argmax = shfl_xor_u64(r.argmax, d);
    o.mn = __shfl_xor(r.mn, d, WAVE);
    o.mx = __shfl_xor(r.mx, d, WAVE);
    o.max_diff = __shfl_xor(r.max_diff, d, WAVE);
    o.max_pw_rel = __shfl_xor(r.max_pw_rel, d, WAVE);
    o.sa = __shfl_xor(r.sa, d, WAVE);
    o.sb = __shfl_xor(r.sb, d, WAVE);
    o.see = __shfl_xor(r.see, d, WAVE);
    o.sbb = __shfl_xor(r.sbb, d, WAVE);
    o.mean_a = __shfl_xor(r.mean_a, d, WAVE);
    o.mean_b = __shfl_xor(r.mean_b, d, WAVE);
    o.m2a = __shfl_xor(r.m2a, d, WAVE);
    o.m2b = __shfl_xor(r.m2b, d, WAVE);
    o.cab = __shfl_xor(r.cab, d, WAVE);
    return o;
}
// the workgroup's (256 threads, all of them here) record: valid in thread 0
__device__ __forceinline__ szk_verify_rec v_block_fold(szk_verify_rec r) {
#pragma unroll 1
    for (int d = 1; d < WAVE; d <<= 1) {  // (a butterfly: every lane ends with the wave's record)
        const szk_verify_rec o = v_shfl_xor(r, d);
        v_merge(r, o);
    }
    __shared__ szk_verify_rec sh[4];
    if (lane_id() == 0) sh[threadIdx.x / WAVE] = r;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; w++) v_merge(r, sh[w]);
    return r;
}

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) VPack {
    T v[VEC];
};

// CONTIG: both views are contiguous: a flat grid-stride loop over units of VEC elements (VEC * sizeof(T) = 16 bytes where both bases
// have the same misalignment, after a scalar head of `head` elements that brings them to a 16-byte boundary, and with a scalar tail;
// VEC = 1 otherwise), four units (two of the 8- and 16-bit types) per array and lane in flight. Else: rows as k_strided walks them
// (sz3hip_kernels.hip): lanes along the innermost index, one wave per row (rows of fewer than 32 elements: 64 / inner rows per wave),
// four elements per array and lane in flight, both row offsets computed once per row in 64 bits. The two views share their extents
// (vo.dims), not their strides.
template <typename T, bool CONTIG, int VEC>
__global__ __launch_bounds__(256) void k_verify(const T *__restrict__ ori, const T *__restrict__ dec, szk_view vo, szk_view vd, uint64_t n, uint32_t head,
                                                double bound, szk_verify_rec *__restrict__ partial) {
    VAcc s;
    if constexpr (CONTIG) {
        const uint64_t G = (uint64_t)gridDim.x * 256, g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
        const uint64_t nv = (n - head) / VEC;  // (head <= n: the launcher's)
        if constexpr (VEC > 1)
            if (g < head) v_elem<T>(s, ori[g], dec[g], g, bound);
        using P = VPack<T, VEC>;
        const P *po = reinterpret_cast<const P *>(ori + head), *pd = reinterpret_cast<const P *>(dec + head);
        // (units of 8 or 16 elements — the 8- and 16-bit types — go two per array at a time: four 16-byte loads in flight, half the registers)
        constexpr int UNR = VEC > 4 ? 2 : 4;
        for (uint64_t v = g; v < nv; v += UNR * G) {
            P a[UNR], b[UNR];
#pragma unroll
            for (int k = 0; k < UNR; k++) {
                const uint64_t vk = v + (uint64_t)k * G;
                if (vk < nv) {
                    a[k] = po[vk];
                    b[k] = pd[vk];
                }
            }
#pragma unroll
            for (int k = 0; k < UNR; k++) {
                const uint64_t vk = v + (uint64_t)k * G;
                if (vk < nv) {
#pragma unroll
                    for (int j = 0; j < VEC; j++) v_elem<T>(s, a[k].v[j], b[k].v[j], head + vk * VEC + j, bound);
                }
            }
        }
        if constexpr (VEC > 1) {  // the tail: head + ntail < 2 * VEC <= 32 elements, all in workgroup 0
            const uint64_t tail0 = head + nv * VEC, ntail = n - tail0;
            if (g >= head && g - head < ntail) v_elem<T>(s, ori[tail0 + (g - head)], dec[tail0 + (g - head)], tail0 + (g - head), bound);
        }
    } else {
        const uint64_t inner = vo.dims[3], rows = n / inner;
        const int64_t so3 = vo.str[3], sd3 = vd.str[3];
        const uint32_t lane = threadIdx.x & 63;
        const uint32_t rpw = inner < 32 ? (uint32_t)(64 / inner) : 1;  // rows per wave
        const uint32_t sub = rpw > 1 ? lane / (uint32_t)inner : 0, x0 = rpw > 1 ? lane % (uint32_t)inner : lane;
        const uint64_t xstep = rpw > 1 ? inner : 64;  // (rpw > 1: one element per lane and row)
        const uint64_t nwaves = (uint64_t)gridDim.x * 4;
        for (uint64_t r = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * rpw + sub; sub < rpw && r < rows; r += nwaves * rpw) {
            const uint64_t q = r / vo.dims[2];
            const uint64_t i2 = r - q * vo.dims[2];
            const uint64_t i0 = q / vo.dims[1], i1 = q - i0 * vo.dims[1];
            const int64_t ob = (int64_t)i0 * vo.str[0] + (int64_t)i1 * vo.str[1] + (int64_t)i2 * vo.str[2];
            const int64_t db = (int64_t)i0 * vd.str[0] + (int64_t)i1 * vd.str[1] + (int64_t)i2 * vd.str[2];
            const uint64_t cb = r * inner;
            for (uint64_t x = x0; x < inner; x += 4 * xstep) {
                T a[4], b[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint64_t xk = x + (uint64_t)k * xstep;
                    if (xk < inner) {
                        a[k] = ori[ob + (int64_t)xk * so3];
                        b[k] = dec[db + (int64_t)xk * sd3];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint64_t xk = x + (uint64_t)k * xstep;
                    if (xk < inner) v_elem<T>(s, a[k], b[k], cb + xk, bound);
                }
            }
        }
    }
    const szk_verify_rec r = v_block_fold(v_record(s));
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ __launch_bounds__(256) void k_verify_final(const szk_verify_rec *__restrict__ partial, uint32_t nrec, uint64_t n, szk_verify_rec *__restrict__ out) {
    szk_verify_rec r = v_record(VAcc{});
    for (uint32_t i = threadIdx.x; i < nrec; i += 256) v_merge(r, partial[i]);
    r = v_block_fold(r);
    if (threadIdx.x == 0) {
        if (r.n_fin == 0) {  // nothing finite: no extremes, no error
            r.mn = r.mx = NAN;
            r.max_diff = 0.0;
        }
        if (r.argmax == ~0ull) r.argmax = n;
        if (r.first_over == ~0ull) r.first_over = n;
        *out = r;
    }
}

inline uint32_t grid_for(uint64_t n, uint32_t block, uint32_t cap) {
    uint64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (uint32_t)g;
}

template <typename T>
int launch_verify(const void *d_ori, const szk_view &vo, const void *d_dec, const szk_view &vd, uint64_t n, double bound, szk_verify_rec *d_partials,
                  szk_verify_rec *d_result, hipStream_t s) {
    const T *o = (const T *)d_ori, *d = (const T *)d_dec;
    uint32_t nb;
    if (vo.contig && vd.contig) {
        constexpr int VEC = 16 / sizeof(T);
        const uintptr_t ao = (uintptr_t)d_ori, ad = (uintptr_t)d_dec;
        // 16-byte loads: both bases reach a 16-byte boundary after the same number of elements (two units per lane and trip at least)
        uint64_t head = ((16 - ao % 16) % 16) / sizeof(T);
        const bool vec = VEC > 1 && ao % sizeof(T) == 0 && ao % 16 == ad % 16 && n >= head + VEC;
        if (vec) {
            nb = grid_for(((n - head) / VEC + 7) / 8, 256, SZK_VERIFY_CAP);
            hipLaunchKernelGGL((k_verify<T, true, VEC>), dim3(nb), dim3(256), 0, s, o, d, vo, vd, n, (uint32_t)head, bound, d_partials);
        } else {
            nb = grid_for((n + 7) / 8, 256, SZK_VERIFY_CAP);
            hipLaunchKernelGGL((k_verify<T, true, 1>), dim3(nb), dim3(256), 0, s, o, d, vo, vd, n, 0u, bound, d_partials);
        }
    } else {
        const uint64_t inner = vo.dims[3], rows = n / inner, rpw = inner < 32 ? 64 / inner : 1;
        nb = grid_for((rows + rpw - 1) / rpw * 64, 256, SZK_VERIFY_CAP);
        hipLaunchKernelGGL((k_verify<T, false, 1>), dim3(nb), dim3(256), 0, s, o, d, vo, vd, n, 0u, bound, d_partials);
    }
    hipLaunchKernelGGL(k_verify_final, dim3(1), dim3(256), 0, s, d_partials, nb, n, d_result);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
}  // namespace

// d_partials: SZK_VERIFY_RECORDS records; d_result: one. The two views have the same extents (all >= 1); bound < 0 or NaN: none given.
int szk_launch_verify(int sz_type, const void *d_ori, const szk_view *view_ori, const void *d_dec, const szk_view *view_dec, double bound,
                      szk_verify_rec *d_partials, szk_verify_rec *d_result, hipStream_t s) {
    static_assert(SZK_VERIFY_RECORDS >= SZK_VERIFY_CAP, "the partial records of every workgroup fit the workspace");
    uint64_t n = 1;
    for (int d = 0; d < 4; d++) {
        if (view_ori->dims[d] != view_dec->dims[d] || view_ori->dims[d] == 0) return -1;
        n *= view_ori->dims[d];
    }
    const double b = bound >= 0 ? bound : (double)INFINITY;  // (NaN fails the comparison too)
    switch (sz_type) {
        case 0: return launch_verify<float>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        case 1: return launch_verify<double>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        case 2: return launch_verify<uint8_t>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        case 3: return launch_verify<int8_t>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        case 4: return launch_verify<uint16_t>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        case 5: return launch_verify<int16_t>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        case 6: return launch_verify<uint32_t>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        case 7: return launch_verify<int32_t>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        case 8: return launch_verify<uint64_t>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        case 9: return launch_verify<int64_t>(d_ori, *view_ori, d_dec, *view_dec, n, b, d_partials, d_result, s);
        default: return -1;
    }
}

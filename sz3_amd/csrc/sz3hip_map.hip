// sz3_amd/csrc/sz3hip_map.hip — texels out of a request's boxes: ONE launch in the strided gather's place, over the
// gather's own records, real `dst` and `dstr` included (in OUTPUT elements).
//
//   k_region_map<T, OUT>         blockIdx.y: the box, lanes along x, a thread per point: the gather's index arithmetic, the point's texel,
//                                one store of the texel's size
//   k_region_map_packed<T, OUT>  one- and two-byte texels (U8, U16, F16): a row of the box is cut at the destination's 4-byte boundaries and a
//                                lane takes one piece — a whole piece is four / two consecutive x points and ONE 32-bit store, the pieces at a
//                                row's head and tail go texel by texel, so that no byte outside the box is written or read. A box whose view
//                                has an x stride other than 1 takes the thread-per-point body inside the same launch.
//   ..._view                     the same over ONE record passed by value (sz3hip_map_device)
//
// The texel of a point depends on the point's value and the options alone (map_code, to_half below): every route, grid and form gives the same
// bytes. LUT32 stages the table in LDS once per workgroup, behind one barrier that every thread of a workgroup with work reaches; nothing else
// uses LDS. No atomics, nothing waits across workgroups, plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/sz3hip.h"
#include "sz3hip_kernels.h"

#include "sz3hip_devutil.h"

namespace {
static_assert(sizeof(sz3hip_map_opts) == 48 && sizeof(sz3hip_map_plan) == 40, "the header's sizes");
using Box = szk_region_gather_strided_box;

// the code of a value in the window (szk_map_code, sz3hip_kernels.h: the compositing's too)
__device__ __forceinline__ uint32_t map_code(double x, const szk_map_opts &o) { return szk_map_code(x, o); }
__device__ __forceinline__ float to_float(float v) { return v; }
__device__ __forceinline__ float to_float(double v) { return (float)v; }
__device__ __forceinline__ uint32_t float_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
// (half)(float)x: two roundings to nearest even, on purpose
__device__ __forceinline__ uint32_t to_half(float f) {
    const _Float16 h = (_Float16)f;
    uint16_t u;
    __builtin_memcpy(&u, &h, 2);
    return u;
}
// the texel of one value, in the low bytes of a word (lut: the table in LDS, LUT32 only)
template <typename T, int OUT>
__device__ __forceinline__ uint32_t map_texel(T v, const szk_map_opts &o, const uint32_t *lut) {
    if constexpr (OUT == SZ3HIP_MAP_F32) return float_bits(to_float(v));  // (a float's bits pass unchanged)
    else if constexpr (OUT == SZ3HIP_MAP_F16) return to_half(to_float(v));
    else if constexpr (OUT == SZ3HIP_MAP_LUT32) return v != v ? o.nan_code : lut[map_code((double)v, o)];
    else return map_code((double)v, o);
}
template <int OUT>
__device__ __forceinline__ void map_store(void *dst, int64_t at, uint32_t texel) {
    if constexpr (OUT == SZ3HIP_MAP_U8) static_cast<uint8_t *>(dst)[at] = (uint8_t)texel;
    else if constexpr (OUT == SZ3HIP_MAP_U16 || OUT == SZ3HIP_MAP_F16) static_cast<uint16_t *>(dst)[at] = (uint16_t)texel;
    else static_cast<uint32_t *>(dst)[at] = texel;
}

// a thread per point: k_region_gather_strided's body with the texel in the copy's place
template <typename T, int OUT>
__device__ __forceinline__ void map_point(const T *__restrict__ src, const Box &b, const szk_map_opts &o, const uint32_t *lut, uint64_t t) {
    if (t >= b.total) return;
    uint64_t r = t, so = 0;
    int64_t dx = 0;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        const uint64_t q = r % b.ext[j];
        so += q * b.str[j];
        dx += (int64_t)q * b.dstr[j];
        r /= b.ext[j];
    }
    map_store<OUT>(b.dst, dx, map_texel<T, OUT>(src[b.src + so], o, lut));
}

template <typename T, int OUT>
__device__ __forceinline__ void map_plain(const T *__restrict__ src, const Box &b, const szk_map_opts &o) {
    if ((uint64_t)blockIdx.x * 256 >= b.total) return;  // (the whole workgroup, before the barrier)
    const uint32_t *lut = nullptr;
    if constexpr (OUT == SZ3HIP_MAP_LUT32) {
        __shared__ uint32_t table[SZ3HIP_MAX_LUT];
        for (uint32_t k = threadIdx.x; k < o.lut_n; k += 256) table[k] = o.d_lut[k];
        __syncthreads();
        lut = table;
    }
    map_point<T, OUT>(src, b, o, lut, (uint64_t)blockIdx.x * 256 + threadIdx.x);
}

// a lane per 4-byte piece of a destination row (the view's x stride is 1); a box whose view steps along x goes point by point
template <typename T, int OUT>
__device__ __forceinline__ void map_packed(const T *__restrict__ src, const Box &b, const szk_map_opts &o) {
    static_assert(OUT == SZ3HIP_MAP_U8 || OUT == SZ3HIP_MAP_U16 || OUT == SZ3HIP_MAP_F16, "texels narrower than a word");
    constexpr uint32_t OB = OUT == SZ3HIP_MAP_U8 ? 1 : 2, P = 4 / OB;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t ex = b.ext[3];
    if (!(ex == 1 || b.dstr[3] == 1)) {
        map_point<T, OUT>(src, b, o, nullptr, t);
        return;
    }
    const uint64_t units = szk_map_row_units(ex, OB);
    if (t >= b.total / ex * units) return;
    uint64_t r = t / units, so = b.src;
    const uint64_t u = t % units;
    int64_t dx = 0;
#pragma unroll
    for (int j = 2; j >= 0; j--) {
        const uint64_t q = r % b.ext[j];
        so += q * b.str[j];
        dx += (int64_t)q * b.dstr[j];
        r /= b.ext[j];
    }
    const uintptr_t head = (uintptr_t)b.dst + (uintptr_t)(dx * (int64_t)OB);  // the row's first texel
    const int64_t mis = (int64_t)(head & 3);                                // (a multiple of OB: dst is aligned to the texel)
    const int64_t e0 = ((int64_t)(4 * u) - mis) / (int64_t)OB;              // the piece's first x, below 0 for a head piece
    const int64_t first = e0 > 0 ? e0 : 0, last = e0 + (int64_t)P < (int64_t)ex ? e0 + (int64_t)P : (int64_t)ex;
    if (first >= last) return;
    const uint64_t sx = b.str[3];
    if (last - first == (int64_t)P) {
        uint32_t word = 0;
#pragma unroll
        for (uint32_t i = 0; i < P; i++) word |= map_texel<T, OUT>(src[so + (uint64_t)(e0 + i) * sx], o, nullptr) << (8 * OB * i);
        *reinterpret_cast<uint32_t *>(head + (uintptr_t)(e0 * (int64_t)OB)) = word;
    } else {
        for (int64_t e = first; e < last; e++) map_store<OUT>(reinterpret_cast<void *>(head), e, map_texel<T, OUT>(src[so + (uint64_t)e * sx], o, nullptr));
    }
}

template <typename T, int OUT>
__global__ __launch_bounds__(256) void k_region_map(const T *__restrict__ src, const Box *__restrict__ recs, szk_map_opts opts) {
    map_plain<T, OUT>(src, recs[blockIdx.y], opts);
}
template <typename T, int OUT>
__global__ __launch_bounds__(256) void k_region_map_view(const T *__restrict__ src, Box rec, szk_map_opts opts) {
    map_plain<T, OUT>(src, rec, opts);
}
template <typename T, int OUT>
__global__ __launch_bounds__(256) void k_region_map_packed(const T *__restrict__ src, const Box *__restrict__ recs, szk_map_opts opts) {
    map_packed<T, OUT>(src, recs[blockIdx.y], opts);
}
template <typename T, int OUT>
__global__ __launch_bounds__(256) void k_region_map_packed_view(const T *__restrict__ src, Box rec, szk_map_opts opts) {
    map_packed<T, OUT>(src, rec, opts);
}

template <typename T, int OUT>
void map_launch(bool packed, const T *src, const Box *d_recs, const Box *rec, dim3 grid, const szk_map_opts &o, hipStream_t s) {
    if constexpr (OUT == SZ3HIP_MAP_U8 || OUT == SZ3HIP_MAP_U16 || OUT == SZ3HIP_MAP_F16) {
        if (packed) {
            if (d_recs) hipLaunchKernelGGL((k_region_map_packed<T, OUT>), grid, dim3(256), 0, s, src, d_recs, o);
            else hipLaunchKernelGGL((k_region_map_packed_view<T, OUT>), grid, dim3(256), 0, s, src, *rec, o);
            return;
        }
    }
    if (d_recs) hipLaunchKernelGGL((k_region_map<T, OUT>), grid, dim3(256), 0, s, src, d_recs, o);
    else hipLaunchKernelGGL((k_region_map_view<T, OUT>), grid, dim3(256), 0, s, src, *rec, o);
}
template <typename T>
bool map_launch_type(bool packed, const T *src, const Box *d_recs, const Box *rec, dim3 grid, const szk_map_opts &o, hipStream_t s) {
    switch (o.out_type) {
    case SZ3HIP_MAP_U8: map_launch<T, SZ3HIP_MAP_U8>(packed, src, d_recs, rec, grid, o, s); return true;
    case SZ3HIP_MAP_U16: map_launch<T, SZ3HIP_MAP_U16>(packed, src, d_recs, rec, grid, o, s); return true;
    case SZ3HIP_MAP_F16: map_launch<T, SZ3HIP_MAP_F16>(packed, src, d_recs, rec, grid, o, s); return true;
    case SZ3HIP_MAP_F32: map_launch<T, SZ3HIP_MAP_F32>(packed, src, d_recs, rec, grid, o, s); return true;
    case SZ3HIP_MAP_LUT32: map_launch<T, SZ3HIP_MAP_LUT32>(packed, src, d_recs, rec, grid, o, s); return true;
    }
    return false;
}
}  // namespace

int szk_launch_region_map(int dtype, const void *d_src, const Box *d_recs, const Box *rec_by_value, uint32_t n, const szk_region_sink *sink, hipStream_t s) {
    if (!sink || sink->kind != SZK_SINK_MAP || !d_src || n < 1 || n > 65535) return -1;
    if ((d_recs == nullptr) == (rec_by_value == nullptr) || (rec_by_value && n != 1)) return -1;
    const szk_map_opts &o = sink->map;
    if (o.out_type == SZ3HIP_MAP_LUT32 && (!o.d_lut || o.lut_n < 2 || o.lut_n > SZ3HIP_MAX_LUT || o.M != o.lut_n - 1)) return -1;
    const uint64_t gx = (sink->map_threads + 255) / 256;
    if (gx < 1 || gx > 0x7FFFFFFFull) return -1;
    const dim3 grid((uint32_t)gx, n);
    const bool ok = dtype == 0 ? map_launch_type<float>(sink->map_packed, (const float *)d_src, d_recs, rec_by_value, grid, o, s)
                               : map_launch_type<double>(sink->map_packed, (const double *)d_src, d_recs, rec_by_value, grid, o, s);
    if (!ok) return -1;
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

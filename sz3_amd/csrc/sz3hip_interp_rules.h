// sz3_amd/csrc/sz3hip_interp_rules.h — the stencils and the case selection of the interpolation predictor, shared by the pass kernels of
// the full decode (sz3hip_interp.hip, interp_point) and of the region decode (sz3hip_region.hip, k_region_pass). Bit identity of the two
// rests on both running these very functions: same formulas, same operand order, same case for the same (i, n).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- Interpolators.hpp:12-39 ---------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T ip_linear(T a, T b) { return (a + b) / 2; }
template <typename T> __device__ __forceinline__ T ip_linear1(T a, T b) { return (T)(-0.5 * (double)a + 1.5 * (double)b); }
template <typename T> __device__ __forceinline__ T ip_quad_1(T a, T b, T c) { return (3 * a + 6 * b - c) / 8; }
template <typename T> __device__ __forceinline__ T ip_quad_2(T a, T b, T c) { return (-a + 6 * b + 3 * c) / 8; }
template <typename T> __device__ __forceinline__ T ip_quad_3(T a, T b, T c) { return (3 * a - 10 * b + 15 * c) / 8; }
template <typename T> __device__ __forceinline__ T ip_cubic(T a, T b, T c, T d) { return (-a + 9 * b + 9 * c - d) / 16; }

// The prediction of the point d points at: point i (odd, 1 <= i <= n - 1) of a line of n points whose neighbours lie st elements apart.
// deferred: linear mode's extrapolated last point of an even-length line (N >= 3) reads d[-2 st], a point of the same pass: it is
// predicted by the pass's second launch (subpass != 0) and by nobody else.
template <typename T>
__device__ __forceinline__ T interp_predict(const T *d, int64_t st, uint64_t i, uint64_t n, int old_api, int interp_id, int subpass, bool &deferred) {
    T pred;
    if (old_api) {  // interpolation_1d, InterpolationDecomposition.hpp:248-293 (N <= 2)
        if (interp_id == 0 || n < 5) {
            if (i + 1 < n) pred = ip_linear<T>(d[-st], d[st]);
            else pred = n < 4 ? d[-st] : ip_linear1<T>(d[-3 * st], d[-st]);
        } else {
            if (i == 1) pred = ip_quad_1<T>(d[-st], d[st], d[3 * st]);
            else if (i + 3 < n) pred = ip_cubic<T>(d[-3 * st], d[-st], d[st], d[3 * st]);
            else if (i + 1 < n) pred = ip_quad_2<T>(d[-3 * st], d[-st], d[st]);
            else pred = ip_quad_3<T>(d[-5 * st], d[-3 * st], d[-st]);
        }
    } else if (interp_id == 0) {  // interpolation_1d_fastest_dim_first, linear branch :334-351
        if (i + 1 < n) {
            pred = ip_linear<T>(d[-st], d[st]);
        } else if (n < 3) {
            pred = d[-st];
        } else {
            deferred = true;  // reads d[-2*st]: a point of this same pass -> second launch
            pred = subpass ? ip_linear1<T>(d[-2 * st], d[-st]) : (T)0;
        }
    } else {  // cubic branch :352-399
        if (i >= 3) {
            if (i + 3 < n) pred = ip_cubic<T>(d[-3 * st], d[-st], d[st], d[3 * st]);
            else if (i + 1 < n) pred = ip_quad_2<T>(d[-3 * st], d[-st], d[st]);
            else pred = ip_linear1<T>(d[-3 * st], d[-st]);
        } else {
            if (i + 3 < n) pred = ip_quad_1<T>(d[-st], d[st], d[3 * st]);
            else if (i + 1 < n) pred = ip_linear<T>(d[-st], d[st]);
            else pred = d[-st];
        }
    }
    return pred;
}

// sz3_amd/csrc/sz3hip_region.hip — region decode of an interpolation stream: the values of one box of the array, bit for bit what the full
// decode puts there, in work sized to the box.
//
// A point of level s (stride s) is predicted from a stencil of at most -L s .. +3 s along the pass's axis (L = 5 for the 1-D / 2-D rules,
// else 3), so the points a box depends on form a pyramid of windows, one per level, each a little wider than the one below it in units of
// its own stride. szk_region_geometry computes the windows (a pure host function: the plan the C ABI hands out is made of it); the decoder
// keeps one compact buffer per level — the grid of stride s restricted to the level's input window — and runs
//   k_region_scatter_raw  the raw records (anchors, unpredictable points) into the buffer of the level that owns the point,
//   k_region_regrid       the points of level 2 s's buffer that level s reads, into the even positions of level s's buffer,
//   k_region_pass         one directional pass over the pass's window: one thread per predicted point,
// and gathers the box from the finest level's buffer. The line geometry of a point (its block of 32 s, the line's length n, its place i)
// comes from the point's coordinate in the FULL array and the full extent, exactly as in interp_point; the prediction is interp_predict
// (sz3hip_interp_rules.h), the very function interp_point runs; the code is read from the FULL per-element code array.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sz3hip_format.h"
#include "sz3hip_kernels.h"
#include "sz3hip_devutil.h"
#include "sz3hip_interp_rules.h"

#include <algorithm>
#include <atomic>
#include <vector>

// ---- host: the windows ----------------------------------------------------------------------------------------------------------------
static inline uint64_t sub_sat(uint64_t a, uint64_t b) { return a > b ? a - b : 0; }

// all_anchor: every point of the grid is an anchor (a tile of a level at or beyond the anchor stride): no level runs, no first point
static int region_geometry(int N, const uint64_t *dims, int interp_id, int direction, uint64_t anchor_stride, bool all_anchor, const uint64_t *lo,
                           const uint64_t *ext, szk_region_geom *g) {
    memset(g, 0, sizeof(*g));
    if (N < 1 || N > 4) return -1;
    if (anchor_stride & (anchor_stride - 1)) return -3;  // (the levels' strides and the anchor grid only nest for a power of two)
    for (int j = 0; j < N; j++)
        if (dims[j] == 0 || ext[j] == 0 || lo[j] >= dims[j] || ext[j] > dims[j] - lo[j]) return -1;
    g->N = N;
    g->interp_id = interp_id;
    g->n_levels = szk_interp_level_count(N, dims, anchor_stride, &g->anchor);
    if (g->n_levels < 0) g->n_levels = 0;
    if (all_anchor) {
        g->n_levels = 0;
        g->anchor = 1;
    }
    if (g->n_levels > SZK_REGION_MAX_LEVELS) return -1;
    szk_interp_perm(N, direction, g->perm);
    for (int j = 0; j < N; j++) {
        g->dims[j] = g->full[j] = dims[j];
        g->lo[j] = lo[j];
        g->ext[j] = ext[j];
    }
    g->nbuf = g->n_levels > 0 ? g->n_levels : 1;
    const uint64_t L = N <= 2 ? 5 : 3, U = 3;
    uint64_t ml = 0, mu = 0;  // margins of the output window of the level at hand (finest first)
    for (int b = g->nbuf - 1; b >= 0; b--) {
        szk_region_level &lv = g->lv[b];
        lv.s = 1ull << (g->nbuf - 1 - b);
        const bool runs = g->n_levels > 0;  // (no level runs: the one buffer is the box itself, filled by the raw records / the first point)
        for (int j = 0; j < N; j++) {
            const uint64_t hi = lo[j] + ext[j] - 1;
            lv.out_lo[j] = sub_sat(lo[j], ml);
            lv.out_hi[j] = hi + mu < dims[j] - 1 ? hi + mu : dims[j] - 1;
            const uint64_t il = runs ? ml + L * lv.s : 0, iu = runs ? mu + U * lv.s : 0;
            lv.in_lo[j] = sub_sat(lo[j], il);
            lv.in_hi[j] = hi + iu < dims[j] - 1 ? hi + iu : dims[j] - 1;
            // the buffer: the grid of stride s from the input window's low corner, rounded down to a multiple of 2 s (lattice parity is the
            // full array's), to the last grid point inside the window
            lv.wlo[j] = runs ? lv.in_lo[j] & ~(2 * lv.s - 1) : lv.in_lo[j];
            lv.cnt[j] = (lv.in_hi[j] - lv.wlo[j]) / lv.s + 1;
        }
        ml += L * lv.s;
        mu += U * lv.s;
    }
    uint64_t base = 0;
    for (int b = 0; b < g->nbuf; b++) {
        szk_region_level &lv = g->lv[b];
        uint64_t run = 1;
        for (int j = N - 1; j >= 0; j--) {
            lv.boff[j] = run;
            if (lv.cnt[j] > (1ull << 40) / run) return -1;  // (no box of that size fits a device)
            run *= lv.cnt[j];
        }
        lv.elems = run;
        lv.base = base;
        base += (run + 3) & ~3ull;  // (buffers start at multiples of 16 bytes)
    }
    g->scratch_elems = base;
    g->points = 0;
    for (int b = 0; b < g->n_levels; b++)
        for (int k = 0; k < N; k++) {
            uint64_t first[4], step[4], cnt[4];
            g->points += szk_region_pass_window(g, b, k, first, step, cnt);
        }
    return 0;
}
int szk_region_geometry(int N, const uint64_t *dims, int interp_id, int direction, uint64_t anchor_stride, const uint64_t *lo, const uint64_t *ext,
                        szk_region_geom *g) {
    return region_geometry(N, dims, interp_id, direction, anchor_stride, false, lo, ext, g);
}
// The tile of level k: the grid of every 2^k-th point is itself an interpolation problem — extents ((D - 1) >> k) + 1,
// anchor stride A >> k, its level l the array's level l + k — so the windows, buffers and pass lattices are the region decode's on that grid, in
// coarse coordinates; g->shift and g->full say where a coarse point's code and raw record lie in the full array. With anchors in use and
// 2^k >= A every coarse point is an anchor. Level 0 is szk_region_geometry.
int szk_tile_geometry(int N, const uint64_t *dims, int interp_id, int direction, uint64_t anchor_stride, int level, const uint64_t *lo, const uint64_t *ext,
                      szk_region_geom *g) {
    memset(g, 0, sizeof(*g));
    if (N < 1 || N > 4 || level < 0 || level > 30) return -1;
    if (anchor_stride & (anchor_stride - 1)) return -3;
    uint64_t cd[4];
    bool use_anchor = false;
    for (int j = 0; j < N; j++) {
        if (dims[j] == 0) return -1;
        cd[j] = ((dims[j] - 1) >> level) + 1;
        if (dims[j] > anchor_stride) use_anchor = true;
    }
    const bool all_anchor = level > 0 && anchor_stride > 0 && use_anchor && (1ull << level) >= anchor_stride;
    // (A >> k is 0 only where the full array takes the first-point path too — no extent above A — or where every coarse point is an anchor)
    int rc = region_geometry(N, cd, interp_id, direction, all_anchor ? 0 : anchor_stride >> level, all_anchor, lo, ext, g);
    if (rc) return rc;
    g->shift = level;
    for (int j = 0; j < N; j++) g->full[j] = dims[j];
    return 0;
}

// ---- host: the decoder units a tile's passes read a code from ----------------------------------------------------
// A row-run is one line of a pass window along x; it marks every unit from the one that holds the code of its first lattice point to the
// one that holds its last. Where the lines of a slower dimension follow each other at most a unit apart their runs join into one interval
// (the next line's first unit is at most one past the previous line's first, which the previous run covers): that dimension is not walked.
// bits: one bit per unit, ceil(units_total / 64) words, zeroed by the caller. limit: stop once more than that many units are marked
// (the caller then decodes densely); returns the number marked (exact when <= limit).
uint64_t szk_tile_mark_units(const szk_region_geom *g, uint64_t *bits, uint64_t limit) {
    const int N = g->N;
    uint64_t off[4] = {0, 0, 0, 0}, run = 1;
    for (int j = N - 1; j >= 0; j--) {
        off[j] = run << g->shift;  // a coarse step in the full code array
        run *= g->full[j];
    }
    uint64_t marked = 0;
    auto mark = [&](uint64_t i0, uint64_t i1) {
        const uint64_t u0 = i0 / SZH_UNIT_SYMS, u1 = i1 / SZH_UNIT_SYMS;
        for (uint64_t w = u0 >> 6; w <= (u1 >> 6); w++) {
            uint64_t m = ~0ull;
            if (w == (u0 >> 6)) m &= ~0ull << (u0 & 63);
            if (w == (u1 >> 6)) m &= ~0ull >> (63 - (u1 & 63));
            marked += (uint64_t)__builtin_popcountll(m & ~bits[w]);
            bits[w] |= m;
        }
    };
    if (g->anchor == 0) {  // the first point reads codes[0] when the coarsest window holds it
        bool at0 = true;
        for (int j = 0; j < N; j++) at0 = at0 && g->lv[0].wlo[j] == 0;
        if (at0) mark(0, 0);
    }
    if (g->n_levels > 0 && N >= 2 && limit != ~0ull) {
        // a bound from below before any marking (a large box must not pay for a list it will not use): the lines of the finest level's last
        // pass start in units of their own where a step of the dimension above x is at least a unit
        uint64_t first[4], step[4], cnt[4], lines = 1;
        if (szk_region_pass_window(g, g->n_levels - 1, N - 1, first, step, cnt) && off[N - 2] >= SZH_UNIT_SYMS) {
            for (int j = 0; j < N - 1; j++) lines *= cnt[j];
            if (lines > limit) return lines;
        }
    }
    for (int b = g->n_levels - 1; b >= 0 && marked <= limit; b--)  // (finest first: the most units)
        for (int k = 0; k < N && marked <= limit; k++) {
            uint64_t first[4], step[4], cnt[4];
            if (szk_region_pass_window(g, b, k, first, step, cnt) == 0) continue;
            uint64_t i0 = 0, i1 = 0;  // the first line's run
            for (int j = 0; j < N; j++) i0 += first[j] * off[j];
            i1 = i0 + (cnt[N - 1] - 1) * step[N - 1] * off[N - 1];
            int walk = N - 1;  // dimensions [0, walk) are walked, [walk, N - 1) joined into the run
            while (walk > 0 && (cnt[walk - 1] == 1 || step[walk - 1] * off[walk - 1] <= SZH_UNIT_SYMS)) {
                i1 += (cnt[walk - 1] - 1) * step[walk - 1] * off[walk - 1];
                walk--;
            }
            if (walk == 0) {
                mark(i0, i1);
                continue;
            }
            // the innermost walked dimension runs in the loop below, the ones above it in the odometer q
            const int in = walk - 1;
            const uint64_t dstep = step[in] * off[in], n = cnt[in], span = i1 - i0;
            uint64_t q[4] = {0, 0, 0, 0};
            for (;;) {
                uint64_t a = i0;
                for (int j = 0; j < in; j++) a += q[j] * step[j] * off[j];
                for (uint64_t t = 0; t < n; t++, a += dstep) {
                    const uint64_t u0 = a / SZH_UNIT_SYMS, u1 = (a + span) / SZH_UNIT_SYMS;
                    if (u0 == u1) {  // (the usual line: inside one unit)
                        const uint64_t o = bits[u0 >> 6];
                        marked += ((o >> (u0 & 63)) & 1) ^ 1;
                        bits[u0 >> 6] = o | (1ull << (u0 & 63));
                    } else {
                        mark(a, a + span);
                    }
                }
                if (marked > limit) break;
                int j = in - 1;
                for (; j >= 0; j--) {
                    if (++q[j] < cnt[j]) break;
                    q[j] = 0;
                }
                if (j < 0) break;
            }
        }
    return marked;
}

// pass k of level b (buffer b): the lattice points it predicts inside its window — per dimension the first coordinate, the step and the count.
// The lattice is build_schedule's (the pass's own axis: odd multiples of s; axes of earlier passes: every multiple; later ones: even
// multiples). The window: the level's INPUT window along the axes of later passes (this level's later passes read those points), its
// OUTPUT window along the others; along its own axis 2 s more below where the rule defers a line's last point, which reads d[-2 s], a
// point of this pass. Returns the number of points.
uint64_t szk_region_pass_window(const szk_region_geom *g, int b, int k, uint64_t *first, uint64_t *step, uint64_t *cnt) {
    const szk_region_level &lv = g->lv[b];
    const int N = g->N, dir = g->perm[k];
    int pos[4];
    for (int q = 0; q < N; q++) pos[g->perm[q]] = q;
    const bool defers = g->interp_id == 0 && N >= 3;
    uint64_t total = 1;
    for (int j = 0; j < N; j++) {
        const uint64_t start = j == dir ? lv.s : 0;
        step[j] = j == dir || pos[j] > k ? 2 * lv.s : lv.s;
        uint64_t wl = pos[j] > k ? lv.in_lo[j] : lv.out_lo[j];
        const uint64_t wh = pos[j] > k ? lv.in_hi[j] : lv.out_hi[j];
        if (j == dir && defers) wl = sub_sat(wl, 2 * lv.s);
        const uint64_t q0 = wl > start ? (wl - start + step[j] - 1) / step[j] : 0;
        first[j] = start + q0 * step[j];
        cnt[j] = first[j] <= wh ? (wh - first[j]) / step[j] + 1 : 0;
        total *= cnt[j];
    }
    return total;
}

// ---- kernels --------------------------------------------------------------------------------------------------------------------------
// Every step of a box's reconstruction — raw records, first point, regrid, pass — has ONE device body; the kernels of the three forms are
// wrappers that say where the step's record comes from: kernel arguments (the single-box call), a table row chosen by blockIdx.y (the
// multi-box call), a step of the chain's table (section 15).
//
// The raw records. One level buffer of a box as the scatter sees it, extents in the last N of four places (1 in front), as the coarse
// decode's geometry has them: a row of words. The single call passes its box's rows as a kernel argument, the multi call keeps every box's
// in its table.
struct szk_region_scatter_row {
    uint64_t wlo[4], cnt[4], base;
};
struct szk_region_scatter_shared {
    uint64_t full[4];
    uint32_t nbuf;
    uint32_t shift;  // a tile of level k: wlo / cnt are coarse coordinates, a record's are the full array's — off the coarse grid it is dropped
};
struct szk_region_bufs {
    szk_region_scatter_shared sh;
    szk_region_scatter_row row[SZK_REGION_MAX_LEVELS];
};
// k_scatter_raw for the region: a record goes into the buffer of the level that predicts its point — the largest stride that divides all
// its coordinates, capped at the coarsest level (whose buffer also holds the anchors / the first point) — and is dropped outside that
// buffer's window. rows: the box's nbuf rows
template <typename T>
__device__ __forceinline__ void region_scatter_records(const uint8_t *__restrict__ payload, uint64_t idx_off, uint64_t val_off, uint64_t cnt, uint64_t n,
                                                       const szk_region_scatter_shared &g, const szk_region_scatter_row *__restrict__ rows, T *__restrict__ scratch) {
    const uint64_t *idx = reinterpret_cast<const uint64_t *>(payload + idx_off);
    const T *val = reinterpret_cast<const T *>(payload + val_off);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += (uint64_t)gridDim.x * 256) {
        uint64_t r = idx[i];
        if (r >= n) continue;
        uint64_t c[4];
        c[3] = r % g.full[3];
        r /= g.full[3];
        c[2] = r % g.full[2];
        r /= g.full[2];
        c[1] = r % g.full[1];
        c[0] = r / g.full[1];
        if ((c[0] | c[1] | c[2] | c[3]) & ((1ull << g.shift) - 1)) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) c[j] >>= g.shift;
        const uint64_t any = c[0] | c[1] | c[2] | c[3];
        const uint32_t top = g.nbuf - 1;  // log2 of the coarsest buffer's stride
        const uint32_t tz = any ? (uint32_t)(__ffsll((long long)any) - 1) : 64u;
        const uint32_t b = tz >= top ? 0u : top - tz;
        const uint32_t ls = top - b;
        const szk_region_scatter_row &lv = rows[b];
        uint64_t o = 0;
        bool in = true;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint64_t wlo = lv.wlo[j], bc = lv.cnt[j];
            const uint64_t q = (c[j] - wlo) >> ls;
            in = in && c[j] >= wlo && q < bc;
            o = o * bc + q;
        }
        if (in) scratch[lv.base + o] = val[i];
    }
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_scatter_raw(const uint8_t *__restrict__ payload, uint64_t idx_off, uint64_t val_off, uint64_t cnt, uint64_t n,
                                                            szk_region_bufs g, T *__restrict__ scratch) {
    region_scatter_records<T>(payload, idx_off, val_off, cnt, n, g.sh, g.row, scratch);
}

// the points of level 2 s's buffer (src) that lie on level s's buffer (dst): its even positions (dst's low corner is a multiple of 2 s).
// Lanes run along x.
struct szk_region_regrid {
    uint64_t ev[4];                  // even positions of dst per dimension: (cnt + 1) / 2
    uint64_t dcnt[4], scnt[4];       // points per dimension
    uint64_t shift[4];               // (dst.wlo - src.wlo) / (2 s): where dst's first point lies in src
    uint64_t total;
};
template <typename T>
__device__ __forceinline__ void region_regrid_point(const T *src, T *dst, const szk_region_regrid &p, uint64_t t) {
    uint64_t r = t, so = 0, dx = 0;
    uint64_t m[4];
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        m[j] = r % p.ev[j];
        r /= p.ev[j];
    }
    bool in = true;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t sq = m[j] + p.shift[j];
        in = in && sq < p.scnt[j];
        so = so * p.scnt[j] + sq;
        dx = dx * p.dcnt[j] + 2 * m[j];
    }
    if (in) dst[dx] = src[so];
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_regrid(const T *__restrict__ src, T *__restrict__ dst, szk_region_regrid p) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < p.total) region_regrid_point<T>(src, dst, p, t);
}

// one directional pass over its window. first / step / cnt: the window's lattice (full coordinates); wlo / boff: the level's buffer.
struct szk_region_pass {
    int N, dir, interp_id, old_api, subpass, radius;
    uint32_t ls;  // log2 s
    uint64_t s, bsz, total, belems;
    uint64_t dims[4], off[4], first[4], step[4], cnt[4], wlo[4], boff[4];
    double eb;
};
// (P: szk_region_pass, or the same fields put together from a shared and a per-box part — szk_region_pass_parts, the multi-box form below)
template <typename T, typename IT, typename P>
__device__ __forceinline__ void region_point(T *__restrict__ buf, const uint16_t *__restrict__ codes, const P &p, uint64_t t) {
    IT r = (IT)t;
    uint64_t idx = 0, a = 0, cd = 0;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        if (j >= p.N) continue;
        const IT cj = (IT)p.cnt[j];
        const IT q = r % cj;
        r /= cj;
        const uint64_t c = p.first[j] + (uint64_t)q * p.step[j];
        idx += c * p.off[j];                         // the point in the full array: where its code lies
        a += ((c - p.wlo[j]) >> p.ls) * p.boff[j];   // ... and in the level's buffer
        if (j == p.dir) cd = c;
    }
    if (a >= p.belems) return;  // (never: the host checked the window against the buffer)
    // the line the point lies on, from its FULL coordinate (interp_point's arithmetic)
    const uint64_t D = p.dims[p.dir];
    const uint64_t begin = cd & ~(p.bsz - 1);
    uint64_t end = begin + p.bsz;
    if (end > D - 1) end = D - 1;
    const uint64_t n = ((end - begin) >> p.ls) + 1, i = (cd - begin) >> p.ls;  // i is odd, 1 <= i <= n-1
    const int64_t st = (int64_t)p.boff[p.dir];  // one grid step of the level in the buffer
    T *d = buf + a;
    bool deferred = false;
    const T pred = interp_predict<T>(d, st, i, n, p.old_api, p.interp_id, p.subpass, deferred);
    if ((p.subpass != 0) != deferred) return;
    const int code = codes[idx];
    if (code) *d = ref_recover<T>(pred, code, p.eb, p.radius);  // code 0: raw value already scattered in place
}
// point t of a pass of p.total points, t < p.total: the index type by the total (a uniform branch; up to 2^32 points every count fits 32 bits too)
template <typename T, typename P>
__device__ __forceinline__ void region_pass_point(T *__restrict__ buf, const uint16_t *__restrict__ codes, const P &p, uint64_t t) {
    if (p.total <= 0xFFFFFFFFull) region_point<T, uint32_t>(buf, codes, p, t);
    else region_point<T, uint64_t>(buf, codes, p, t);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_pass(T *__restrict__ buf, const uint16_t *__restrict__ codes, szk_region_pass p) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < p.total) region_pass_point<T>(buf, codes, p, t);
}
// without anchors the first element is predicted by 0 (k_interp_first_dec); first: the coarsest buffer's first element
template <typename T>
__device__ __forceinline__ void region_first_point(T *first, const uint16_t *__restrict__ codes, double eb, int radius) {
    if (codes[0]) *first = ref_recover<T>((T)0, codes[0], eb, radius);
}
template <typename T>
__global__ __launch_bounds__(64) void k_region_first(T *__restrict__ buf, const uint16_t *__restrict__ codes, double eb, int radius) {
    if (threadIdx.x == 0 && blockIdx.x == 0) region_first_point<T>(buf, codes, eb, radius);
}

// ---- n boxes of one level of one stream in one launch sequence -------------------------------------------------------
// The boxes' reconstructions are independent and their launch sequences identical — the level count and the pass order are the grid's, not
// the box's —, so one sequence serves them all: blockIdx.y is the box, grid.x covers the largest box of the launch, and a workgroup reads its
// box's record from a table in device memory (a load that is uniform per workgroup) and leaves when it lies beyond its own box's total.
// What all boxes of a pass share stays a kernel argument; a record holds what differs. Every record is a row of 64-bit words.
struct szk_region_pass_shared {  // szk_region_pass without ...
    int N, dir, interp_id, old_api, subpass, radius;
    uint32_t ls;
    uint64_t s, bsz;
    uint64_t dims[4], off[4], step[4];
    double eb;
};
struct szk_region_pass_box {  // ... the box's part: the pass window's lattice, the level's buffer and where that lies in the scratch
    uint64_t total, belems, base;
    uint64_t first[4], cnt[4], wlo[4], boff[4];
};
// The two parts as region_point reads them. It indexes dims and boff by the pass's axis, a run-time value: an array in registers cannot be
// indexed so (the whole struct would go to scratch memory), a chain of selects can — and folds away where the index is a constant.
struct szk_sel4 {
    uint64_t v[4];
    __device__ __forceinline__ uint64_t operator[](int i) const { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }
};
struct szk_region_pass_parts {
    int N, dir, interp_id, old_api, subpass, radius;
    uint32_t ls;
    uint64_t s, bsz, total, belems;
    szk_sel4 dims, boff;
    uint64_t off[4], first[4], step[4], cnt[4], wlo[4];
    double eb;
};
__host__ __device__ __forceinline__ uint64_t *szk_words(uint64_t (&a)[4]) { return a; }
__host__ __device__ __forceinline__ uint64_t *szk_words(szk_sel4 &a) { return a.v; }
// the two parts put together, sub-pass `subpass`. P: szk_region_pass_parts — a workgroup of the multi kernels and of the chain, from its
// box's record — or szk_region_pass — the host, for the single call's kernel argument
template <typename P>
__host__ __device__ __forceinline__ P region_pass_join(const szk_region_pass_shared &sh, const szk_region_pass_box &b, int subpass) {
    P p;
    p.N = sh.N;
    p.dir = sh.dir;
    p.interp_id = sh.interp_id;
    p.old_api = sh.old_api;
    p.subpass = subpass;
    p.radius = sh.radius;
    p.ls = sh.ls;
    p.s = sh.s;
    p.bsz = sh.bsz;
    p.total = b.total;
    p.belems = b.belems;
    p.eb = sh.eb;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        szk_words(p.dims)[j] = sh.dims[j];
        p.off[j] = sh.off[j];
        p.step[j] = sh.step[j];
        p.first[j] = b.first[j];
        p.cnt[j] = b.cnt[j];
        p.wlo[j] = b.wlo[j];
        szk_words(p.boff)[j] = b.boff[j];
    }
    return p;
}
struct szk_region_regrid_box {
    szk_region_regrid g;
    uint64_t src, dst;  // the two buffers' bases in the scratch
};
struct szk_region_first_box {
    uint64_t total, base;  // total 1: the box's coarsest window holds the origin
};
struct szk_region_gather_box {
    uint64_t total, src;  // points of the box; its corner in the scratch
    void *dst;
    uint64_t ext[4], str[4];  // extents in the last N of four places; the finest buffer's element strides
};
#define SZK_WORDS(R) ((uint64_t)(sizeof(R) / 8))  // a record in the table
static_assert(sizeof(szk_region_scatter_row) == 9 * 8 && sizeof(szk_region_pass_box) == 19 * 8 && sizeof(szk_region_regrid_box) == 19 * 8 &&
                  sizeof(szk_region_gather_box) == 11 * 8,
              "table records are rows of words");

// k_region_scatter_raw per box: every box scans the whole list (as its own call would) and keeps what falls into its windows
template <typename T>
__global__ __launch_bounds__(256) void k_region_scatter_raw_multi(const uint8_t *__restrict__ payload, uint64_t idx_off, uint64_t val_off, uint64_t cnt, uint64_t n,
                                                                  szk_region_scatter_shared g, const uint64_t *__restrict__ tab, T *__restrict__ scratch) {
    region_scatter_records<T>(payload, idx_off, val_off, cnt, n, g, reinterpret_cast<const szk_region_scatter_row *>(tab) + (uint64_t)blockIdx.y * g.nbuf, scratch);
}
template <typename T>
__global__ __launch_bounds__(64) void k_region_first_multi(T *__restrict__ scratch, const uint16_t *__restrict__ codes, double eb, int radius,
                                                           const szk_region_first_box *__restrict__ recs) {
    const szk_region_first_box &r = recs[blockIdx.y];
    if (threadIdx.x == 0 && blockIdx.x == 0 && r.total) region_first_point<T>(scratch + r.base, codes, eb, radius);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_regrid_multi(T *__restrict__ scratch, const szk_region_regrid_box *__restrict__ recs) {
    const szk_region_regrid_box &b = recs[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < b.g.total) region_regrid_point<T>(scratch + b.src, scratch + b.dst, b.g, t);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_pass_multi(T *__restrict__ scratch, const uint16_t *__restrict__ codes, szk_region_pass_shared sh,
                                                           const szk_region_pass_box *__restrict__ recs) {
    const szk_region_pass_box &b = recs[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= b.total) return;
    const szk_region_pass_parts p = region_pass_join<szk_region_pass_parts>(sh, b, sh.subpass);
    region_pass_point<T>(scratch + b.base, codes, p, t);
}
// box i out of its finest buffer into d_outs[i], contiguous; lanes run along x
template <typename T>
__global__ __launch_bounds__(256) void k_region_gather_multi(const T *__restrict__ scratch, const szk_region_gather_box *__restrict__ recs) {
    const szk_region_gather_box &b = recs[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= b.total) return;
    uint64_t r = t, so = 0;
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        so += (r % b.ext[j]) * b.str[j];
        r /= b.ext[j];
    }
    static_cast<T *>(b.dst)[t] = scratch[b.src + so];
}

// ---- boxes of SEVERAL levels in one launch sequence --------------------------------------------------------------------
// A tile of level k is the region problem on the grid of every 2^k-th point, and its grid level l is the array's level l + k; for every box
// that runs levels at all n_levels + shift is the array's level count. So the boxes of a mixed request are aligned by ARRAY level: in the
// launch of array level A - b every box works on ITS buffer b (lv[b], stride 2^(nbuf - 1 - b) on its own grid), and a box of fewer than b + 1
// levels has finished — its record carries total 0. What the multi form passes as a kernel argument common to all boxes and the box's level
// decides — s, ls, bsz, off, dims, step; nbuf, shift — moves into the box's record; what an array level decides stays an argument. The
// bodies are the ones above.
struct szk_region_scatter_box {
    uint64_t rows;         // the box's nbuf rows (szk_region_scatter_row), in words from the table's start
    uint32_t nbuf, shift;
};
struct szk_region_pass_level {  // what all boxes share at an array level: szk_region_pass_shared without what the box's level decides
    int N, dir, interp_id, old_api, subpass, radius;
    double eb;
};
struct szk_region_pass_mixed_box {
    uint64_t s, ls, bsz;
    uint64_t dims[4], off[4], step[4];
    szk_region_pass_box box;
};
static_assert(sizeof(szk_region_scatter_box) == 2 * 8 && sizeof(szk_region_pass_mixed_box) == 34 * 8 && sizeof(szk_region_gather_strided_box) == 15 * 8 &&
                  sizeof(szk_region_pass_level) == 4 * 8,
              "table records are rows of words");
template <typename T>
__global__ __launch_bounds__(256) void k_region_scatter_raw_mixed(const uint8_t *__restrict__ payload, uint64_t idx_off, uint64_t val_off, uint64_t cnt, uint64_t n,
                                                                  szk_sel4 full, const uint64_t *__restrict__ tab, const szk_region_scatter_box *__restrict__ recs,
                                                                  T *__restrict__ scratch) {
    const szk_region_scatter_box &r = recs[blockIdx.y];
    szk_region_scatter_shared g;
#pragma unroll
    for (int j = 0; j < 4; j++) g.full[j] = full.v[j];
    g.nbuf = r.nbuf;
    g.shift = r.shift;
    region_scatter_records<T>(payload, idx_off, val_off, cnt, n, g, reinterpret_cast<const szk_region_scatter_row *>(tab + r.rows), scratch);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_pass_mixed(T *__restrict__ scratch, const uint16_t *__restrict__ codes, szk_region_pass_level lvl,
                                                           const szk_region_pass_mixed_box *__restrict__ recs) {
    const szk_region_pass_mixed_box &r = recs[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= r.box.total) return;  // (also every workgroup of a box that has finished: total 0)
    szk_region_pass_shared sh;
    sh.N = lvl.N;
    sh.dir = lvl.dir;
    sh.interp_id = lvl.interp_id;
    sh.old_api = lvl.old_api;
    sh.subpass = lvl.subpass;
    sh.radius = lvl.radius;
    sh.ls = (uint32_t)r.ls;
    sh.s = r.s;
    sh.bsz = r.bsz;
    sh.eb = lvl.eb;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        sh.dims[j] = r.dims[j];
        sh.off[j] = r.off[j];
        sh.step[j] = r.step[j];
    }
    const szk_region_pass_parts p = region_pass_join<szk_region_pass_parts>(sh, r.box, lvl.subpass);
    region_pass_point<T>(scratch + r.box.base, codes, p, t);
}
// k_region_gather_multi with the destination's element strides in the record: box i out of `src` (the scratch: its finest buffer; a handle
// that keeps the full array: that array, str the strides of its every 2^level-th point) into the view at b.dst; lanes run along x
template <typename T>
__global__ __launch_bounds__(256) void k_region_gather_strided(const T *__restrict__ src, const szk_region_gather_strided_box *__restrict__ recs) {
    const szk_region_gather_strided_box &b = recs[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
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
    static_cast<T *>(b.dst)[dx] = src[b.src + so];
}

// ---- the coarsest levels of a request in ONE launch ---------------------------------------------------------------------
// All but the finest one or two levels of a box are a few thousand points each, and every one of them costs a launch or two per pass. Here one
// workgroup per box (blockIdx.x) walks a step table — first point, regrid, pass, deferred sub-pass — over the request's coarsest levels: each
// step is a loop t = threadIdx.x, += 1024 over the body the multi kernel it replaces calls (the pass: region_point<T, uint32_t> over
// region_pass_join's szk_region_pass_parts). A __syncthreads() follows every step and every thread reaches it (no return around it): the only
// ordering there is. The box's level buffers are written and read by this one workgroup, in place, with plain loads and stores; `scratch`
// is neither read-only nor __restrict__ here. No waiting between workgroups, no flags, no atomics, no LDS. A step's records are the multi
// kernels' own, in the request's table: `rec` is box 0's record (box i's follows i records on), `shared` a pass's szk_region_pass_shared
// (subpass as the step says), both in words from the table's start.
struct szk_chain_step {
    uint64_t kind;  // 1 first point, 2 regrid, 3 pass
    uint64_t subpass;
    uint64_t rec, shared;
};
static_assert(sizeof(szk_chain_step) == 4 * 8 && sizeof(szk_region_pass_shared) == 19 * 8 && sizeof(szk_region_first_box) == 2 * 8, "table records are rows of words");
template <typename T>
__global__ __launch_bounds__(1024) void k_region_chain_multi(T *scratch, const uint16_t *__restrict__ codes, double eb0, int radius, const uint64_t *__restrict__ tab,
                                                             uint64_t steps_off, uint32_t n_steps) {
    const uint32_t box = blockIdx.x;
    const szk_chain_step *steps = reinterpret_cast<const szk_chain_step *>(tab + steps_off);
    for (uint32_t q = 0; q < n_steps; q++) {
        const szk_chain_step st = steps[q];
        if (st.kind == 1) {  // k_region_first_multi
            const szk_region_first_box &r = reinterpret_cast<const szk_region_first_box *>(tab + st.rec)[box];
            if (threadIdx.x == 0 && r.total) region_first_point<T>(scratch + r.base, codes, eb0, radius);
        } else if (st.kind == 2) {  // k_region_regrid_multi
            const szk_region_regrid_box &b = reinterpret_cast<const szk_region_regrid_box *>(tab + st.rec)[box];
            for (uint64_t t = threadIdx.x; t < b.g.total; t += 1024) region_regrid_point<T>(scratch + b.src, scratch + b.dst, b.g, t);
        } else {  // k_region_pass_multi; a pass's total is at most chain_points, a 32-bit number: the host chose the levels so
            const szk_region_pass_box &b = reinterpret_cast<const szk_region_pass_box *>(tab + st.rec)[box];
            const szk_region_pass_parts p = region_pass_join<szk_region_pass_parts>(*reinterpret_cast<const szk_region_pass_shared *>(tab + st.shared), b, (int)st.subpass);
            T *buf = scratch + b.base;
            for (uint64_t t = threadIdx.x; t < p.total; t += 1024) region_point<T, uint32_t>(buf, codes, p, t);
        }
        __syncthreads();
    }
}

// ---- host: a step's records from a box's geometry -------------------------------------------------------------------------------------------
// One builder per record, used by the single-box and the multi-box driver alike; a builder that can refuse returns -1 and holds that
// refusal's only copy. Four-place arrays hold the N extents in their last places, as the kernels read them.
//
// a step of the (coarse) grid along each dimension in the FULL code array; returns the full array's element count
static uint64_t region_code_steps(const szk_region_geom &g, uint64_t *off) {
    uint64_t num = 1;
    for (int j = 3; j >= 0; j--) {
        off[j] = j < g.N ? num << g.shift : 0;
        if (j < g.N) num *= g.full[j];
    }
    return num;
}
// workgroups of 256 threads over `total` points; false: more than a grid's 31 bits
static bool region_grid(uint64_t total, uint32_t *gx) {
    const uint64_t nb = (total + 255) / 256;
    if (nb > 0x7FFFFFFFull) return false;
    *gx = (uint32_t)nb;
    return true;
}
static uint32_t region_scatter_grid(uint64_t n_vout) { return (uint32_t)((n_vout + 255) / 256 < 4096 ? (n_vout + 255) / 256 : 4096); }
// the raw records: what the boxes of a request share, and a box's nbuf rows
static void region_scatter_shared(const szk_region_geom &g, szk_region_scatter_shared *sh) {
    memset(sh, 0, sizeof(*sh));
    sh->nbuf = (uint32_t)g.nbuf;
    sh->shift = (uint32_t)g.shift;
    for (int q = 0; q < 4; q++) sh->full[q] = q - (4 - g.N) >= 0 ? g.full[q - (4 - g.N)] : 1;
}
static void region_scatter_rows(const szk_region_geom &g, szk_region_scatter_row *rows) {
    for (int b = 0; b < g.nbuf; b++) {
        for (int q = 0; q < 4; q++) {
            const int j = q - (4 - g.N);
            rows[b].wlo[q] = j >= 0 ? g.lv[b].wlo[j] : 0;
            rows[b].cnt[q] = j >= 0 ? g.lv[b].cnt[j] : 1;
        }
        rows[b].base = g.lv[b].base;
    }
}
// the first point runs for a box whose coarsest window holds the origin (then it is that buffer's first element)
static szk_region_first_box region_first_record(const szk_region_geom &g) {
    bool at0 = true;
    for (int j = 0; j < g.N; j++) at0 = at0 && g.lv[0].wlo[j] == 0;
    return {at0 ? 1ull : 0ull, g.lv[0].base};
}
// level b >= 1 from level b - 1. -1: level b's buffer starts below the one it is filled from
static int region_regrid_record(const szk_region_geom &g, int b, szk_region_regrid_box *r) {
    const szk_region_level &lv = g.lv[b], &up = g.lv[b - 1];
    memset(r, 0, sizeof(*r));
    r->g.total = 1;
    for (int q = 0; q < 4; q++) {
        const int j = q - (4 - g.N);
        r->g.dcnt[q] = j >= 0 ? lv.cnt[j] : 1;
        r->g.scnt[q] = j >= 0 ? up.cnt[j] : 1;
        r->g.ev[q] = (r->g.dcnt[q] + 1) / 2;
        if (j >= 0 && lv.wlo[j] < up.wlo[j]) return -1;
        r->g.shift[q] = j >= 0 ? (lv.wlo[j] - up.wlo[j]) / up.s : 0;
        r->g.total *= r->g.ev[q];
    }
    r->src = up.base;
    r->dst = lv.base;
    return 0;
}
// what the passes of level b share (the boxes of a request too: these are the grid's); a pass adds its axis and its lattice's steps
static void region_pass_level(const szk_interp_params &ip, const szk_region_geom &g, int b, szk_region_pass_shared *sh) {
    const int level = g.n_levels - b;  // the level's number on the grid: stride 2^(level - 1); in the full array it is level + shift
    memset(sh, 0, sizeof(*sh));
    sh->N = g.N;
    sh->interp_id = ip.interp_id;
    sh->old_api = g.N <= 2;
    sh->radius = ip.radius;
    sh->s = g.lv[b].s;
    sh->ls = (uint32_t)(level - 1);
    sh->bsz = 32ull * sh->s;
    sh->eb = szk_interp_level_eb(ip.eb, ip.alpha, ip.beta, level + g.shift);
    region_code_steps(g, sh->off);
    for (int j = 0; j < g.N; j++) sh->dims[j] = g.dims[j];
}
// linear mode for N >= 3 defers the last point of even-length lines, as run_interp does: the pass is launched a second time with subpass 1
static bool region_pass_twice(const szk_region_pass_shared &sh) { return !sh.old_api && sh.interp_id == 0; }
// pass k of level b of one box: the axis and the steps into sh, the box's part into r. -1: the window does not lie on the level's buffer
static int region_pass_records(const szk_region_geom &g, int b, int k, szk_region_pass_shared *sh, szk_region_pass_box *r) {
    const szk_region_level &lv = g.lv[b];
    memset(r, 0, sizeof(*r));
    sh->dir = g.perm[k];
    r->total = szk_region_pass_window(&g, b, k, r->first, sh->step, r->cnt);
    for (int j = 0; j < g.N; j++) {
        if (r->total && (r->first[j] < lv.wlo[j] || (r->first[j] + (r->cnt[j] - 1) * sh->step[j] - lv.wlo[j]) / lv.s >= lv.cnt[j])) return -1;
        r->wlo[j] = lv.wlo[j];
        r->boff[j] = lv.boff[j];
    }
    r->belems = lv.elems;
    r->base = lv.base;
    return 0;
}
// the box, out of the finest buffer (stride 1). -1: the box does not lie on that buffer
static int region_gather_record(const szk_region_geom &g, void *dst, szk_region_gather_box *r) {
    const szk_region_level &fin = g.lv[g.nbuf - 1];
    memset(r, 0, sizeof(*r));
    r->total = 1;
    r->src = fin.base;
    r->dst = dst;
    for (int q = 0; q < 4; q++) {
        const int j = q - (4 - g.N);
        r->ext[q] = j >= 0 ? g.ext[j] : 1;
        r->str[q] = j >= 0 ? fin.boff[j] : 0;
        if (j < 0) continue;
        if (g.lo[j] < fin.wlo[j] || g.lo[j] - fin.wlo[j] + g.ext[j] > fin.cnt[j]) return -1;
        r->src += (g.lo[j] - fin.wlo[j]) * fin.boff[j];
        r->total *= g.ext[j];
    }
    return 0;
}
// the same into a strided view: the gather record and the destination's element strides (none for a dimension of extent 1)
static int region_gather_strided_record(const szk_region_geom &g, const szk_region_out &out, szk_region_gather_strided_box *r) {
    szk_region_gather_box c;
    if (region_gather_record(g, out.dst, &c)) return -1;
    memset(r, 0, sizeof(*r));
    r->total = c.total;
    r->src = c.src;
    r->dst = c.dst;
    for (int q = 0; q < 4; q++) {
        const int j = q - (4 - g.N);
        r->ext[q] = c.ext[q];
        r->str[q] = c.str[q];
        r->dstr[q] = j >= 0 && g.ext[j] > 1 ? out.str[j] : 0;
    }
    return 0;
}
// a box's gather record as its launch reads it — into the view *out, or (out null) into the contiguous array dst — as words; *total: the box's points
static int region_gather_words(const szk_region_geom &g, void *dst, const szk_region_out *out, uint64_t *rec, uint64_t *total) {
    szk_region_gather_box c;
    szk_region_gather_strided_box v;
    if (out ? region_gather_strided_record(g, *out, &v) : region_gather_record(g, dst, &c)) return -1;
    if (out) memcpy(rec, &v, sizeof(v));
    else memcpy(rec, &c, sizeof(c));
    *total = out ? v.total : c.total;
    return 0;
}
// a box's part of a pass at array level A - b as the mixed form keeps it: what the box's level decides, and the multi form's record. A box of
// fewer than b + 1 levels has finished: a record of zeros (total 0). sh: the level's shared part as the box sees it (eb, dir: the array level's)
static int region_pass_mixed_record(const szk_interp_params &ip, const szk_region_geom &g, int b, int k, szk_region_pass_shared *sh, szk_region_pass_mixed_box *r) {
    memset(r, 0, sizeof(*r));
    memset(sh, 0, sizeof(*sh));
    if (b >= g.n_levels) return 0;
    region_pass_level(ip, g, b, sh);
    if (region_pass_records(g, b, k, sh, &r->box)) return -1;
    r->s = sh->s;
    r->ls = sh->ls;
    r->bsz = sh->bsz;
    for (int j = 0; j < 4; j++) {
        r->dims[j] = sh->dims[j];
        r->off[j] = sh->off[j];
        r->step[j] = sh->step[j];
    }
    return 0;
}

// ---- host: the launches ---------------------------------------------------------------------------------------------------------------
// test hook (sz3hip_debug_region_launches): kernel launches the box reconstructions of this process issued, single and multi. Every launch
// is counted here, and for the request where the driver keeps a count (*issued)
static std::atomic<uint64_t> g_region_launches{0};
uint64_t szk_region_launches(void) { return g_region_launches.load(); }
static void region_count(uint32_t *issued) {
    g_region_launches++;
    if (issued) ++*issued;
}
template <typename... KA, typename... A>
static void region_launch(uint32_t *issued, void (*kernel)(KA...), dim3 grid, uint32_t block, hipStream_t s, const A &...args) {
    hipLaunchKernelGGL(kernel, grid, dim3(block), 0, s, args...);
    region_count(issued);
}

// the sink table (sz3hip_kernels.h), in the order of SZK_SINK_*; the launch functions of the sinks' files behind the one signature
#define SINK_FN(call)                                                                                                                          \
    [](int dtype, const void *src, const szk_region_gather_strided_box *d_recs, uint32_t n, uint64_t most, const szk_region_sink *sink, hipStream_t s) -> int { \
        (void)most;                                                                                                                            \
        return call;                                                                                                                           \
    }
#define SINK_ARRAY(field) [](const szk_region_sink *k) -> const void * { return k->field; }
// (complete per level group: one launch, no final — DESIGN.md sections 19, 20, 21, 23, 26)
#define SINK_PER_GROUP(words, array, dst, launch) {words, 0, array, dst, 0, SINK_FN(launch(dtype, src, d_recs, nullptr, n, sink, s)), nullptr, nullptr}
static const szk_sink_desc g_sinks[] = {
    // REDUCE: the reduction, then — once per request — the final fold
    {0, 0, nullptr, SZK_DST_PART, 1, SINK_FN(szk_launch_region_reduce(dtype, src, d_recs, nullptr, n, most, sink, s)),
     SINK_FN(szk_launch_region_reduce_final(dtype, src, d_recs, nullptr, n, sink, s)),
     [](const szk_region_sink *k) { return k->partials && k->d_stats && (!k->hist.nbins || k->d_hist); }},
    // SELECT: the count, then — once per request — scan and write, with every box's d_index, d_value and capacity
    {0, SZK_SELECT_OUT_WORDS, SINK_ARRAY(sel_outs), SZK_DST_PART, 2, SINK_FN(szk_launch_region_select_count(dtype, src, d_recs, nullptr, n, most, sink, s)),
     SINK_FN(szk_launch_region_select_place(dtype, src, d_recs, nullptr, n, most, sink, s)), [](const szk_region_sink *k) { return k->sel_counts && k->sel_heads; }},
    /* MAP */ SINK_PER_GROUP(0, nullptr, SZK_DST_VIEW, szk_launch_region_map),
    /* SAMPLE */ SINK_PER_GROUP(SZK_SAMPLE_WORDS, SINK_ARRAY(smp_queries), SZK_DST_INDEX, szk_launch_region_sample),
    /* PROJECT */ SINK_PER_GROUP(0, nullptr, SZK_DST_VIEW, szk_launch_region_project),
    /* GRADIENT */ SINK_PER_GROUP(SZK_GRADIENT_WORDS, SINK_ARRAY(grd_boxes), SZK_DST_INDEX, szk_launch_region_gradient),
    /* COMPOSITE */ SINK_PER_GROUP(SZK_COMPOSITE_WORDS, SINK_ARRAY(cmp_boxes), SZK_DST_INDEX, szk_launch_region_composite),
};
static const szk_sink_desc g_gather = {0, 0, nullptr, SZK_DST_VIEW, 0, nullptr, nullptr, nullptr};
const szk_sink_desc &szk_sink(const szk_region_sink *sink) {
    return !sink ? g_gather : g_sinks[(size_t)sink->kind < sizeof(g_sinks) / sizeof(g_sinks[0]) ? sink->kind : SZK_SINK_REDUCE];
}

// what rides in the table's one copy directly behind the n boxes' records at the cursor *w: the sink's per-box entries in the RECORDS' order
// (a record's `dst` word names its box in the request), or — with the final only — its flat words in the request's order
static bool region_sink_tail(const szk_region_sink *sink, uint32_t n, uint64_t *h_table, uint64_t *w, uint64_t table_words, bool with_final = true) {
    constexpr uint64_t RW = SZK_WORDS(szk_region_gather_strided_box);
    const szk_sink_desc &d = szk_sink(sink);
    const uint64_t per = d.box_words ? d.box_words : with_final ? d.flat_words : 0, words = (uint64_t)n * per;
    if (!words) return true;
    const char *from = static_cast<const char *>(d.entries(sink));
    if (!from || words > table_words || *w > table_words - words || (d.box_words && *w < (uint64_t)n * RW)) return false;
    if (!d.box_words) memcpy(h_table + *w, from, words * 8);
    for (uint32_t r = 0; d.box_words && r < n; r++) {
        szk_region_gather_strided_box b;
        memcpy(&b, h_table + *w - (uint64_t)n * RW + r * RW, sizeof(b));
        memcpy(h_table + *w + r * per, from + (uintptr_t)b.dst * per * 8, per * 8);
    }
    *w += words;
    return true;
}

// a sink's launches in the gather's place: its launch over the boxes' records, then — unless the caller issues it once for several groups —
// its final
template <typename T>
static int region_sink_launch(uint32_t *issued, const T *src, const szk_region_gather_strided_box *d_recs, uint32_t n, uint64_t most, const szk_region_sink *sink,
                              bool with_final, hipStream_t s) {
    const szk_sink_desc &d = szk_sink(sink);
    if (d.launch(sizeof(T) == 4 ? 0 : 1, src, d_recs, n, most, sink, s)) return -2;
    region_count(issued);
    if (!d.final_launches || !with_final) return 0;
    if (d.final(sizeof(T) == 4 ? 0 : 1, src, d_recs, n, most, sink, s)) return -2;
    for (uint32_t k = 0; k < d.final_launches; k++) region_count(issued);
    return 0;
}

template <typename T>
static int run_region(const szk_interp_params &ip, const szk_region_geom &g, const uint8_t *payload, uint64_t vout_idx_off, uint64_t vout_val_off,
                      uint64_t n_vout, const uint16_t *codes, T *scratch, T *d_out, hipStream_t s) {
    uint32_t gx;
    if (n_vout) {
        uint64_t off[4];
        szk_region_bufs rb;
        memset(&rb, 0, sizeof(rb));
        region_scatter_shared(g, &rb.sh);
        region_scatter_rows(g, rb.row);
        region_launch(nullptr, k_region_scatter_raw<T>, dim3(region_scatter_grid(n_vout)), 256, s, payload, vout_idx_off, vout_val_off, n_vout, region_code_steps(g, off), rb,
                      scratch);
    }
    if (g.anchor == 0 && region_first_record(g).total) region_launch(nullptr, k_region_first<T>, dim3(1), 64, s, scratch + g.lv[0].base, codes, ip.eb, ip.radius);
    for (int b = 0; b < g.n_levels; b++) {
        if (b > 0) {
            szk_region_regrid_box r;
            if (region_regrid_record(g, b, &r) || !region_grid(r.g.total, &gx)) return -1;
            region_launch(nullptr, k_region_regrid<T>, dim3(gx), 256, s, (const T *)(scratch + r.src), scratch + r.dst, r.g);
        }
        szk_region_pass_shared sh;
        region_pass_level(ip, g, b, &sh);
        for (int k = 0; k < g.N; k++) {
            szk_region_pass_box pb;
            if (region_pass_records(g, b, k, &sh, &pb)) return -1;
            if (pb.total == 0) continue;
            if (!region_grid(pb.total, &gx)) return -1;
            for (int sub = 0; sub < (region_pass_twice(sh) ? 2 : 1); sub++)
                region_launch(nullptr, k_region_pass<T>, dim3(gx), 256, s, scratch + pb.base, codes, region_pass_join<szk_region_pass>(sh, pb, sub));
        }
    }
    szk_region_gather_box gb;
    if (region_gather_record(g, d_out, &gb)) return -1;
    szk_view v;
    memset(&v, 0, sizeof(v));
    for (int q = 0; q < 4; q++) {
        v.dims[q] = gb.ext[q];
        v.str[q] = (int64_t)gb.str[q];
    }
    v.contig = 0;
    if (szk_launch_gather(sizeof(T) == 4 ? 0 : 1, 0, scratch + gb.src, &v, d_out, nullptr, s)) return -2;
    region_count(nullptr);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int szk_launch_interp_decompress_region(int dtype, const szk_interp_params *ip, const szk_region_geom *g, const uint8_t *payload, uint64_t vout_idx_off,
                                        uint64_t vout_val_off, uint64_t n_vout, const uint16_t *codes, void *scratch, void *d_out, hipStream_t s) {
    if (g->N != ip->N || g->nbuf < 1 || g->shift < 0 || g->shift > 30) return -1;
    for (int j = 0; j < ip->N; j++)
        if (g->full[j] != ip->dims[j] || g->dims[j] != ((ip->dims[j] - 1) >> g->shift) + 1) return -1;
    return dtype == 0 ? run_region<float>(*ip, *g, payload, vout_idx_off, vout_val_off, n_vout, codes, (float *)scratch, (float *)d_out, s)
                      : run_region<double>(*ip, *g, payload, vout_idx_off, vout_val_off, n_vout, codes, (double *)scratch, (double *)d_out, s);
}

// words the table of a request of n boxes takes (an upper bound: every box with every record; behind them the chain's pass parameters and steps)
uint64_t szk_region_multi_table_words(const szk_region_geom *gs, uint32_t n) {
    const uint64_t nb = (uint64_t)gs[0].nbuf, nl = (uint64_t)gs[0].n_levels, N = (uint64_t)gs[0].N;
    return (uint64_t)n * (nb * SZK_WORDS(szk_region_scatter_row) + SZK_WORDS(szk_region_first_box) + nl * SZK_WORDS(szk_region_regrid_box) +
                          nl * N * SZK_WORDS(szk_region_pass_box) + SZK_WORDS(szk_region_gather_box)) +
           nl * N * SZK_WORDS(szk_region_pass_shared) + (1 + nl * (1 + 2 * N)) * SZK_WORDS(szk_chain_step);
}

namespace {
struct MultiLaunch {
    int kind;  // 0 scatter, 1 first, 2 regrid, 3 pass, 4 gather
    uint64_t off;  // the launch's records in the table, in words
    uint32_t gx;
    bool twice;    // pass: the deferred points' launch follows
    szk_region_pass_shared sh;
    bool chained;  // the launch is a step of the chain's one launch instead
    uint64_t most;  // gather: the largest box's points
};
}  // namespace
template <typename T>
static int run_region_multi(const szk_interp_params &ip, const szk_region_geom *gs, uint32_t n, uint64_t scratch_elems, const uint8_t *payload,
                            uint64_t vout_idx_off, uint64_t vout_val_off, uint64_t n_vout, const uint16_t *codes, T *scratch, void *const *d_outs,
                            uint64_t *h_table, uint64_t *d_table, uint64_t table_words, hipEvent_t copied, hipStream_t s, uint32_t chain_points,
                            uint32_t *chain_levels, uint32_t *launches, const szk_region_out *outs = nullptr,  // (outs: strided views instead of d_outs)
                            const szk_region_sink *sink = nullptr, bool sink_final = true) {  // (sink: the boxes are reduced, not delivered)
    const szk_region_geom &g0 = gs[0];
    const int N = g0.N, nbuf = g0.nbuf, n_levels = g0.n_levels;
    // the chain takes the coarsest c levels: the largest count such that every pass of those levels has at most chain_points points for EVERY box
    // (the launch sequence is common to all boxes: the largest one decides)
    int c = 0;
    for (; chain_points && c < n_levels; c++) {
        bool fits = true;
        for (uint32_t i = 0; i < n && fits; i++)
            for (int k = 0; k < N && fits; k++) {
                uint64_t first[4], step[4], cnt[4];
                fits = szk_region_pass_window(&gs[i], c, k, first, step, cnt) <= chain_points;
            }
        if (!fits) break;
    }
    if (chain_levels) *chain_levels = (uint32_t)c;
    // every box's buffers inside the scratch, before anything is built
    for (uint32_t i = 0; i < n; i++)
        for (int b = 0; b < nbuf; b++)
            if (gs[i].lv[b].base > scratch_elems || gs[i].lv[b].elems > scratch_elems - gs[i].lv[b].base) return -1;
    std::vector<MultiLaunch> seq;
    uint64_t w = 0;  // the table's cursor
    auto room = [&](uint64_t words) { return words <= table_words && w <= table_words - words; };
    auto put = [&](const void *rec, size_t bytes) {
        memcpy(h_table + w, rec, bytes);
        w += bytes / 8;
    };
    // a launch of `kind` whose records start at the cursor, room for `words` per box provided
    auto launch_at = [&](int kind, uint64_t words, MultiLaunch *l) {
        *l = MultiLaunch{};
        l->kind = kind;
        l->off = w;
        return room((uint64_t)n * words);
    };
    MultiLaunch l;
    if (n_vout) {
        if (!launch_at(0, nbuf * SZK_WORDS(szk_region_scatter_row), &l)) return -1;
        l.gx = region_scatter_grid(n_vout);
        for (uint32_t i = 0; i < n; i++) {
            szk_region_scatter_row rows[SZK_REGION_MAX_LEVELS];
            region_scatter_rows(gs[i], rows);
            put(rows, nbuf * sizeof(rows[0]));
        }
        seq.push_back(l);
    }
    if (g0.anchor == 0) {  // the first point, for the boxes whose coarsest window holds it
        if (!launch_at(1, SZK_WORDS(szk_region_first_box), &l)) return -1;
        bool any = false;
        for (uint32_t i = 0; i < n; i++) {
            const szk_region_first_box r = region_first_record(gs[i]);
            put(&r, sizeof(r));
            any = any || r.total;
        }
        l.gx = 1;
        l.chained = c > 0;
        if (any) seq.push_back(l);
        else w = l.off;
    }
    for (int b = 0; b < n_levels; b++) {
        uint64_t most = 0;
        if (b > 0) {
            if (!launch_at(2, SZK_WORDS(szk_region_regrid_box), &l)) return -1;
            for (uint32_t i = 0; i < n; i++) {
                szk_region_regrid_box r;
                if (region_regrid_record(gs[i], b, &r)) return -1;
                put(&r, sizeof(r));
                most = r.g.total > most ? r.g.total : most;
            }
            if (!region_grid(most, &l.gx)) return -1;
            l.chained = b < c;
            if (most) seq.push_back(l);
            else w = l.off;
        }
        szk_region_pass_shared sh;
        region_pass_level(ip, g0, b, &sh);
        for (int k = 0; k < N; k++) {
            if (!launch_at(3, SZK_WORDS(szk_region_pass_box), &l)) return -1;
            most = 0;
            for (uint32_t i = 0; i < n; i++) {
                szk_region_pass_shared si = sh;
                szk_region_pass_box r;
                if (region_pass_records(gs[i], b, k, i ? &si : &sh, &r)) return -1;
                if (i && memcmp(si.step, sh.step, sizeof(sh.step))) return -1;  // (the lattice's steps are the level's and the pass's)
                put(&r, sizeof(r));
                most = r.total > most ? r.total : most;
            }
            if (!region_grid(most, &l.gx)) return -1;
            if (most == 0) {  // (no box has a point in this pass)
                w = l.off;
                continue;
            }
            l.sh = sh;
            l.twice = region_pass_twice(sh);
            l.chained = b < c;
            seq.push_back(l);
        }
    }
    {
        const uint64_t words = outs ? SZK_WORDS(szk_region_gather_strided_box) : SZK_WORDS(szk_region_gather_box);  // (the form is the request's, chosen once)
        if (!launch_at(4, words, &l)) return -1;
        uint64_t most = 0;
        for (uint32_t i = 0; i < n; i++) {
            uint64_t rec[SZK_WORDS(szk_region_gather_strided_box)], total;
            if (region_gather_words(gs[i], outs ? nullptr : d_outs[i], outs ? &outs[i] : nullptr, rec, &total)) return -1;
            put(rec, words * 8);
            most = std::max(most, total);
        }
        if (!region_grid(most, &l.gx)) return -1;
        l.most = most;
        seq.push_back(l);
        // (a sink's per-box entries ride with every group's records; its flat words with the request's one final)
        if (!region_sink_tail(sink, n, h_table, &w, table_words, sink_final)) return -1;
    }
    // the chain's steps, behind the boxes' records: the chained launches in their order, a pass's shared part in front of its step(s)
    uint64_t steps_off = 0;
    uint32_t n_steps = 0;
    if (c > 0) {
        std::vector<szk_chain_step> steps;
        for (const MultiLaunch &cl : seq) {
            if (!cl.chained) continue;
            szk_chain_step st = {(uint64_t)cl.kind, 0, cl.off, 0};
            if (cl.kind == 3) {
                if (!room(SZK_WORDS(szk_region_pass_shared))) return -1;
                st.shared = w;
                put(&cl.sh, sizeof(cl.sh));
            }
            steps.push_back(st);
            if (cl.kind == 3 && cl.twice) {  // the deferred last point of even-length lines: a step of its own, behind a barrier
                st.subpass = 1;
                steps.push_back(st);
            }
        }
        if (!room(steps.size() * SZK_WORDS(szk_chain_step))) return -1;
        steps_off = w;
        n_steps = (uint32_t)steps.size();
        put(steps.data(), steps.size() * sizeof(szk_chain_step));
    }
    // the whole table by one copy, in front of the first launch; `copied` tells the next call's build when the pinned array may be rewritten
    if (hipMemcpyAsync(d_table, h_table, w * 8, hipMemcpyHostToDevice, s) != hipSuccess) return -2;
    if (hipEventRecord(copied, s) != hipSuccess) return -2;
    szk_region_scatter_shared ss;
    region_scatter_shared(g0, &ss);
    uint64_t off[4];
    const uint64_t num = region_code_steps(g0, off);
    uint32_t issued = 0;
    bool chain_done = false;
    for (const MultiLaunch &ml : seq) {
        if (ml.chained) {  // (the chained launches follow each other in seq: the one launch stands where the first of them stood)
            if (!chain_done && n_steps)
                region_launch(&issued, k_region_chain_multi<T>, dim3(n), 1024, s, scratch, codes, ip.eb, ip.radius, (const uint64_t *)d_table, steps_off, n_steps);
            chain_done = true;
            continue;
        }
        const dim3 grid(ml.gx, n);
        const uint64_t *rec = d_table + ml.off;
        switch (ml.kind) {
        case 0:
            region_launch(&issued, k_region_scatter_raw_multi<T>, grid, 256, s, payload, vout_idx_off, vout_val_off, n_vout, num, ss, rec, scratch);
            break;
        case 1:
            region_launch(&issued, k_region_first_multi<T>, grid, 64, s, scratch, codes, ip.eb, ip.radius, reinterpret_cast<const szk_region_first_box *>(rec));
            break;
        case 2:
            region_launch(&issued, k_region_regrid_multi<T>, grid, 256, s, scratch, reinterpret_cast<const szk_region_regrid_box *>(rec));
            break;
        case 3:
            for (int sub = 0; sub < (ml.twice ? 2 : 1); sub++) {  // (the deferred last point of even-length lines, as in run_region)
                szk_region_pass_shared sh = ml.sh;
                sh.subpass = sub;
                region_launch(&issued, k_region_pass_multi<T>, grid, 256, s, scratch, codes, sh, reinterpret_cast<const szk_region_pass_box *>(rec));
            }
            break;
        default:
            if (sink) {
                if (!outs || region_sink_launch<T>(&issued, scratch, reinterpret_cast<const szk_region_gather_strided_box *>(rec), n, ml.most, sink, sink_final, s)) return -2;
            } else if (outs) region_launch(&issued, k_region_gather_strided<T>, grid, 256, s, (const T *)scratch, reinterpret_cast<const szk_region_gather_strided_box *>(rec));
            else region_launch(&issued, k_region_gather_multi<T>, grid, 256, s, (const T *)scratch, reinterpret_cast<const szk_region_gather_box *>(rec));
        }
    }
    if (launches) *launches = issued;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int szk_launch_interp_decompress_region_multi(int dtype, const szk_interp_params *ip, const szk_region_geom *gs, uint32_t n, uint64_t scratch_elems,
                                              const uint8_t *payload, uint64_t vout_idx_off, uint64_t vout_val_off, uint64_t n_vout, const uint16_t *codes,
                                              void *scratch, void *const *d_outs, uint64_t *h_table, uint64_t *d_table, uint64_t table_words, hipEvent_t copied,
                                              hipStream_t s, uint32_t chain_points, uint32_t *chain_levels, uint32_t *launches) {
    if (chain_levels) *chain_levels = 0;
    if (launches) *launches = 0;
    if (n < 1 || n > 65535 || !gs || !d_outs || !h_table || !d_table) return -1;
    for (uint32_t i = 0; i < n; i++) {  // one level of one stream: the grid, the level count, the buffer count and the pass order are the request's
        const szk_region_geom &g = gs[i];
        if (g.N != ip->N || g.nbuf < 1 || g.shift < 0 || g.shift > 30) return -1;
        if (g.n_levels != gs[0].n_levels || g.nbuf != gs[0].nbuf || g.shift != gs[0].shift || g.anchor != gs[0].anchor || memcmp(g.perm, gs[0].perm, sizeof(g.perm))) return -1;
        for (int j = 0; j < ip->N; j++)
            if (g.full[j] != ip->dims[j] || g.dims[j] != ((ip->dims[j] - 1) >> g.shift) + 1) return -1;
        for (int b = 0; b < g.nbuf; b++)
            if (g.lv[b].s != gs[0].lv[b].s) return -1;
        if (!d_outs[i]) return -1;
    }
    return dtype == 0 ? run_region_multi<float>(*ip, gs, n, scratch_elems, payload, vout_idx_off, vout_val_off, n_vout, codes, (float *)scratch, d_outs, h_table, d_table,
                                                table_words, copied, s, chain_points, chain_levels, launches)
                      : run_region_multi<double>(*ip, gs, n, scratch_elems, payload, vout_idx_off, vout_val_off, n_vout, codes, (double *)scratch, d_outs, h_table, d_table,
                                                 table_words, copied, s, chain_points, chain_levels, launches);
}

// ---- boxes of several levels in one request ------------------------------------------------------------------------
namespace {
struct MixedLaunch {
    int kind;      // 0 scatter, 1 first, 2 regrid, 3 pass, 4 gather
    uint64_t off;  // the launch's records in the table, in words
    uint32_t gx;
    bool twice;
    szk_region_pass_level lvl;
    uint64_t most;  // gather: the largest box's points
};
// the array's level count as the boxes that run levels see it; false: two of them disagree (or differ in pass order), the sequence cannot be merged
bool request_aligned(const szk_region_geom *gs, uint32_t n) {
    int A = -1;
    for (uint32_t i = 0; i < n; i++) {
        if (memcmp(gs[i].perm, gs[0].perm, sizeof(gs[0].perm))) return false;
        if (gs[i].n_levels == 0) continue;
        if (A >= 0 && gs[i].n_levels + gs[i].shift != A) return false;
        A = gs[i].n_levels + gs[i].shift;
    }
    return true;
}
}  // namespace
uint64_t szk_region_request_table_words(const szk_region_geom *gs, uint32_t n) {
    uint64_t nl = 0, kinds = 0, words = 0;
    const uint64_t N = (uint64_t)gs[0].N;
    for (uint32_t i = 0; i < n; i++) {
        nl = std::max<uint64_t>(nl, (uint64_t)gs[i].n_levels);
        kinds |= 1ull << gs[i].shift;
    }
    for (uint32_t i = 0; i < n; i++)
        words += (uint64_t)gs[i].nbuf * SZK_WORDS(szk_region_scatter_row) + SZK_WORDS(szk_region_scatter_box) + SZK_WORDS(szk_region_first_box) +
                 nl * SZK_WORDS(szk_region_regrid_box) + nl * N * SZK_WORDS(szk_region_pass_mixed_box) + SZK_WORDS(szk_region_gather_strided_box);
    // (one level, or level group by level group: the one-level sequence's chain parts, once per level)
    return words + (uint64_t)__builtin_popcountll(kinds) * (nl * N * SZK_WORDS(szk_region_pass_shared) + (1 + nl * (1 + 2 * N)) * SZK_WORDS(szk_chain_step));
}
uint64_t szk_sink_table_words(const szk_region_sink *sink, const szk_region_geom *gs, uint32_t n) {
    const szk_sink_desc &d = szk_sink(sink);
    const uint64_t recs = (uint64_t)n * SZK_WORDS(szk_region_gather_strided_box);
    return (gs ? szk_region_request_table_words(gs, n) + (d.final_launches ? recs : 0) : recs) + (uint64_t)n * (d.box_words + d.flat_words);
}
template <typename T>
static int run_region_mixed(const szk_interp_params &ip, const szk_region_geom *gs, uint32_t n, uint64_t scratch_elems, const uint8_t *payload,
                            uint64_t vout_idx_off, uint64_t vout_val_off, uint64_t n_vout, const uint16_t *codes, T *scratch, const szk_region_out *outs,
                            uint64_t *h_table, uint64_t *d_table, uint64_t table_words, hipEvent_t copied, hipStream_t s, uint32_t *launches, uint32_t *levels,
                            const szk_region_sink *sink) {
    const int N = gs[0].N;
    int n_levels = 0;  // the array levels the sequence runs: the finest box's own count
    for (uint32_t i = 0; i < n; i++) {
        n_levels = std::max(n_levels, gs[i].n_levels);
        for (int b = 0; b < gs[i].nbuf; b++)
            if (gs[i].lv[b].base > scratch_elems || gs[i].lv[b].elems > scratch_elems - gs[i].lv[b].base) return -1;
    }
    if (levels) *levels = (uint32_t)n_levels;
    std::vector<MixedLaunch> seq;
    uint64_t w = 0;
    auto room = [&](uint64_t words) { return words <= table_words && w <= table_words - words; };
    auto put = [&](const void *rec, size_t bytes) {
        memcpy(h_table + w, rec, bytes);
        w += bytes / 8;
    };
    auto launch_at = [&](int kind, uint64_t words, MixedLaunch *l) {
        *l = MixedLaunch{};
        l->kind = kind;
        l->off = w;
        return room((uint64_t)n * words);
    };
    MixedLaunch l;
    if (n_vout) {  // every box's rows, then the boxes' records
        std::vector<szk_region_scatter_box> recs(n);
        for (uint32_t i = 0; i < n; i++) {
            szk_region_scatter_row rows[SZK_REGION_MAX_LEVELS];
            if (!room((uint64_t)gs[i].nbuf * SZK_WORDS(szk_region_scatter_row))) return -1;
            region_scatter_rows(gs[i], rows);
            recs[i] = {w, (uint32_t)gs[i].nbuf, (uint32_t)gs[i].shift};
            put(rows, gs[i].nbuf * sizeof(rows[0]));
        }
        if (!launch_at(0, SZK_WORDS(szk_region_scatter_box), &l)) return -1;
        put(recs.data(), n * sizeof(recs[0]));
        l.gx = region_scatter_grid(n_vout);
        seq.push_back(l);
    }
    {  // the first point: per box (a box whose every grid point is an anchor has none, whatever the others have)
        if (!launch_at(1, SZK_WORDS(szk_region_first_box), &l)) return -1;
        bool any = false;
        for (uint32_t i = 0; i < n; i++) {
            szk_region_first_box r = region_first_record(gs[i]);
            if (gs[i].anchor != 0) r.total = 0;
            put(&r, sizeof(r));
            any = any || r.total;
        }
        l.gx = 1;
        if (any) seq.push_back(l);
        else w = l.off;
    }
    for (int b = 0; b < n_levels; b++) {
        uint64_t most = 0;
        if (b > 0) {
            if (!launch_at(2, SZK_WORDS(szk_region_regrid_box), &l)) return -1;
            for (uint32_t i = 0; i < n; i++) {
                szk_region_regrid_box r;
                memset(&r, 0, sizeof(r));
                if (b < gs[i].n_levels && region_regrid_record(gs[i], b, &r)) return -1;
                put(&r, sizeof(r));
                most = std::max(most, r.g.total);
            }
            if (!region_grid(most, &l.gx)) return -1;
            if (most) seq.push_back(l);
            else w = l.off;
        }
        for (int k = 0; k < N; k++) {
            if (!launch_at(3, SZK_WORDS(szk_region_pass_mixed_box), &l)) return -1;
            most = 0;
            bool have = false;
            szk_region_pass_shared ref;
            for (uint32_t i = 0; i < n; i++) {
                szk_region_pass_shared sh;
                szk_region_pass_mixed_box r;
                if (region_pass_mixed_record(ip, gs[i], b, k, &sh, &r)) return -1;
                put(&r, sizeof(r));
                if (b >= gs[i].n_levels) continue;
                // (what stays a kernel argument is the array level's: the same for every box that runs it)
                // (-4, before anything is copied or launched: the caller then serves the request level group by level group)
                if (have && (sh.dir != ref.dir || sh.old_api != ref.old_api || sh.interp_id != ref.interp_id || memcmp(&sh.eb, &ref.eb, sizeof(sh.eb)))) return -4;
                if (!have) ref = sh;
                have = true;
                most = std::max(most, r.box.total);
            }
            if (!region_grid(most, &l.gx)) return -1;
            if (most == 0) {
                w = l.off;
                continue;
            }
            l.lvl = szk_region_pass_level{ref.N, ref.dir, ref.interp_id, ref.old_api, 0, ref.radius, ref.eb};
            l.twice = region_pass_twice(ref);
            seq.push_back(l);
        }
    }
    {
        if (!launch_at(4, SZK_WORDS(szk_region_gather_strided_box), &l)) return -1;
        uint64_t most = 0;
        for (uint32_t i = 0; i < n; i++) {
            szk_region_gather_strided_box r;
            if (region_gather_strided_record(gs[i], outs[i], &r)) return -1;
            put(&r, sizeof(r));
            most = std::max(most, r.total);
        }
        if (!region_grid(most, &l.gx)) return -1;
        l.most = most;
        seq.push_back(l);
        if (!region_sink_tail(sink, n, h_table, &w, table_words)) return -1;
    }
    if (hipMemcpyAsync(d_table, h_table, w * 8, hipMemcpyHostToDevice, s) != hipSuccess) return -2;
    if (hipEventRecord(copied, s) != hipSuccess) return -2;
    szk_sel4 full;
    for (int q = 0; q < 4; q++) full.v[q] = q - (4 - N) >= 0 ? gs[0].full[q - (4 - N)] : 1;
    uint64_t off[4];
    const uint64_t num = region_code_steps(gs[0], off);
    uint32_t issued = 0;
    for (const MixedLaunch &ml : seq) {
        const dim3 grid(ml.gx, n);
        const uint64_t *rec = d_table + ml.off;
        switch (ml.kind) {
        case 0:
            region_launch(&issued, k_region_scatter_raw_mixed<T>, grid, 256, s, payload, vout_idx_off, vout_val_off, n_vout, num, full, (const uint64_t *)d_table,
                          reinterpret_cast<const szk_region_scatter_box *>(rec), scratch);
            break;
        case 1:
            region_launch(&issued, k_region_first_multi<T>, grid, 64, s, scratch, codes, ip.eb, ip.radius, reinterpret_cast<const szk_region_first_box *>(rec));
            break;
        case 2:
            region_launch(&issued, k_region_regrid_multi<T>, grid, 256, s, scratch, reinterpret_cast<const szk_region_regrid_box *>(rec));
            break;
        case 3:
            for (int sub = 0; sub < (ml.twice ? 2 : 1); sub++) {
                szk_region_pass_level lvl = ml.lvl;
                lvl.subpass = sub;
                region_launch(&issued, k_region_pass_mixed<T>, grid, 256, s, scratch, codes, lvl, reinterpret_cast<const szk_region_pass_mixed_box *>(rec));
            }
            break;
        default:
            if (sink) {
                if (region_sink_launch<T>(&issued, scratch, reinterpret_cast<const szk_region_gather_strided_box *>(rec), n, ml.most, sink, true, s)) return -2;
            } else region_launch(&issued, k_region_gather_strided<T>, grid, 256, s, (const T *)scratch, reinterpret_cast<const szk_region_gather_strided_box *>(rec));
        }
    }
    if (launches) *launches = issued;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

template <typename T>
static int run_region_request(const szk_interp_params &ip, const szk_region_geom *gs, uint32_t n, uint64_t scratch_elems, const uint8_t *payload,
                              uint64_t vout_idx_off, uint64_t vout_val_off, uint64_t n_vout, const uint16_t *codes, T *scratch, const szk_region_out *outs,
                              uint64_t *h_table, uint64_t *d_table, uint64_t table_words, hipEvent_t copied, hipStream_t s, uint32_t chain_points,
                              uint32_t *chain_levels, uint32_t *launches, uint32_t *levels, const szk_region_sink *sink) {
    bool one = true;
    for (uint32_t i = 1; i < n; i++) one = one && gs[i].shift == gs[0].shift;
    if (one) {  // the one-level sequence, the chain included
        if (levels) *levels = (uint32_t)gs[0].n_levels;
        return run_region_multi<T>(ip, gs, n, scratch_elems, payload, vout_idx_off, vout_val_off, n_vout, codes, scratch, nullptr, h_table, d_table, table_words, copied, s,
                                   chain_points, chain_levels, launches, outs, sink);
    }
    if (request_aligned(gs, n) && !(szk_dbg_flags2 & SZ3HIP_DBG2_REQUEST_BY_LEVEL)) {
        const int rc = run_region_mixed<T>(ip, gs, n, scratch_elems, payload, vout_idx_off, vout_val_off, n_vout, codes, scratch, outs, h_table, d_table, table_words,
                                           copied, s, launches, levels, sink);
        if (rc != -4) return rc;  // (-4: a pass's arguments are not one for all boxes; nothing was copied or launched)
    }
    // level group by level group, every group with a stretch of the table of its own (no wait between the groups' copies)
    const szk_sink_desc &sd = szk_sink(sink);
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return gs[a].shift < gs[b].shift; });
    uint64_t used = 0;
    uint32_t total = 0, most_levels = 0;
    for (uint32_t at = 0; at < n;) {
        std::vector<szk_region_geom> gg;
        std::vector<szk_region_out> oo;
        for (; at < n && (gg.empty() || gs[order[at]].shift == gg[0].shift); at++) {
            gg.push_back(gs[order[at]]);
            oo.push_back(outs[order[at]]);
        }
        const uint64_t need = szk_region_request_table_words(gg.data(), (uint32_t)gg.size()) + gg.size() * sd.box_words;
        if (need > table_words || used > table_words - need) return -1;
        uint32_t issued = 0;
        const int rc = run_region_multi<T>(ip, gg.data(), (uint32_t)gg.size(), scratch_elems, payload, vout_idx_off, vout_val_off, n_vout, codes, scratch, nullptr,
                                           h_table + used, d_table + used, need, copied, s, 0, nullptr, &issued, oo.data(), sink, false);
        if (rc) return rc;
        used += need;
        total += issued;
        most_levels = std::max(most_levels, (uint32_t)gg[0].n_levels);
    }
    if (sd.final_launches) {  // ONE final for the request: the boxes' records once more, in the request's order, behind the groups' stretches
        uint64_t need = (uint64_t)n * SZK_WORDS(szk_region_gather_strided_box), most = 0;
        if (need > table_words || used > table_words - need) return -1;
        for (uint32_t i = 0; i < n; i++) {
            szk_region_gather_strided_box r;
            if (region_gather_strided_record(gs[i], outs[i], &r)) return -1;
            memcpy(h_table + used + (uint64_t)i * SZK_WORDS(szk_region_gather_strided_box), &r, sizeof(r));
            most = std::max(most, r.total);
        }
        need += used;  // (the cursor behind the records; the sink's flat words follow them)
        if (!region_sink_tail(sink, n, h_table, &need, table_words)) return -1;
        need -= used;
        if (hipMemcpyAsync(d_table + used, h_table + used, need * 8, hipMemcpyHostToDevice, s) != hipSuccess) return -2;
        if (hipEventRecord(copied, s) != hipSuccess) return -2;
        const szk_region_gather_strided_box *d_recs = reinterpret_cast<const szk_region_gather_strided_box *>(d_table + used);
        if (sd.final(sizeof(T) == 4 ? 0 : 1, scratch, d_recs, n, most, sink, s)) return -2;  // (the groups ran the sink's launch; its final once, over all boxes)
        for (uint32_t k = 0; k < sd.final_launches; k++) region_count(&total);
    }
    if (launches) *launches = total;
    if (levels) *levels = most_levels;
    return 0;
}

int szk_launch_interp_decompress_region_request(int dtype, const szk_interp_params *ip, const szk_region_geom *gs, uint32_t n, uint64_t scratch_elems,
                                                const uint8_t *payload, uint64_t vout_idx_off, uint64_t vout_val_off, uint64_t n_vout, const uint16_t *codes,
                                                void *scratch, const szk_region_out *outs, uint64_t *h_table, uint64_t *d_table, uint64_t table_words,
                                                hipEvent_t copied, hipStream_t s, uint32_t chain_points, uint32_t *chain_levels, uint32_t *launches, uint32_t *levels,
                                                const szk_region_sink *sink) {
    if (chain_levels) *chain_levels = 0;
    if (launches) *launches = 0;
    if (levels) *levels = 0;
    if (n < 1 || n > 65535 || !gs || !outs || !h_table || !d_table) return -1;
    const szk_sink_desc &sd = szk_sink(sink);  // (what the sink's row asks of the sink and of every box's `dst` word)
    if (sink && ((sd.entries && !sd.entries(sink)) || (sd.ready && !sd.ready(sink)))) return -1;
    for (uint32_t i = 0; i < n; i++)
        if (sd.dst == SZK_DST_VIEW ? !outs[i].dst : sd.dst == SZK_DST_INDEX && (uintptr_t)outs[i].dst != i) return -1;
    for (uint32_t i = 0; i < n; i++) {  // one stream: every box on the grid of its own level
        const szk_region_geom &g = gs[i];
        if (g.N != ip->N || g.nbuf < 1 || g.nbuf > SZK_REGION_MAX_LEVELS || g.n_levels < 0 || g.n_levels > g.nbuf || g.shift < 0 || g.shift > 30) return -1;
        for (int j = 0; j < ip->N; j++)
            if (g.full[j] != ip->dims[j] || g.dims[j] != ((ip->dims[j] - 1) >> g.shift) + 1) return -1;
        if (g.shift == gs[0].shift) {  // (the one-level sequence's conditions, for the boxes of a level)
            if (g.n_levels != gs[0].n_levels || g.nbuf != gs[0].nbuf || g.anchor != gs[0].anchor) return -1;
        }
    }
    return dtype == 0 ? run_region_request<float>(*ip, gs, n, scratch_elems, payload, vout_idx_off, vout_val_off, n_vout, codes, (float *)scratch, outs, h_table, d_table,
                                                  table_words, copied, s, chain_points, chain_levels, launches, levels, sink)
                      : run_region_request<double>(*ip, gs, n, scratch_elems, payload, vout_idx_off, vout_val_off, n_vout, codes, (double *)scratch, outs, h_table, d_table,
                                                   table_words, copied, s, chain_points, chain_levels, launches, levels, sink);
}

int szk_launch_gather_boxes(int dtype, const void *d_src, const szk_region_gather_strided_box *recs, uint32_t n, uint64_t *h_table, uint64_t *d_table,
                            uint64_t table_words, hipEvent_t copied, hipStream_t s, const szk_region_sink *sink, uint32_t *launches) {
    if (launches) *launches = 0;
    if (n < 1 || n > 65535 || !d_src || !recs || !h_table || !d_table || (uint64_t)n * SZK_WORDS(szk_region_gather_strided_box) > table_words) return -1;
    uint64_t most = 0;
    for (uint32_t i = 0; i < n; i++) most = std::max(most, recs[i].total);
    uint32_t gx;
    if (!region_grid(most, &gx)) return -1;
    memcpy(h_table, recs, (size_t)n * sizeof(recs[0]));
    uint64_t w = (uint64_t)n * SZK_WORDS(szk_region_gather_strided_box);
    if (!region_sink_tail(sink, n, h_table, &w, table_words)) return -1;
    if (hipMemcpyAsync(d_table, h_table, w * 8, hipMemcpyHostToDevice, s) != hipSuccess) return -2;
    if (hipEventRecord(copied, s) != hipSuccess) return -2;
    const szk_region_gather_strided_box *d_recs = reinterpret_cast<const szk_region_gather_strided_box *>(d_table);
    if (sink)
        return dtype == 0 ? region_sink_launch<float>(launches, (const float *)d_src, d_recs, n, most, sink, true, s)
                          : region_sink_launch<double>(launches, (const double *)d_src, d_recs, n, most, sink, true, s);
    if (dtype == 0) region_launch(launches, k_region_gather_strided<float>, dim3(gx, n), 256, s, (const float *)d_src, d_recs);
    else region_launch(launches, k_region_gather_strided<double>, dim3(gx, n), 256, s, (const double *)d_src, d_recs);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

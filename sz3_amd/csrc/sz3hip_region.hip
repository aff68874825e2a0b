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
// the buffers of all levels, extents in the last N of four places (1 in front), as the coarse decode's geometry has them
struct szk_region_bufs {
    uint64_t full[4];
    uint64_t wlo[SZK_REGION_MAX_LEVELS][4], cnt[SZK_REGION_MAX_LEVELS][4], base[SZK_REGION_MAX_LEVELS];
    uint32_t nbuf;
    uint32_t shift;  // a tile of level k: wlo / cnt are coarse coordinates, a record's are the full array's — off the coarse grid it is dropped
};
// k_scatter_raw for the region: a record goes into the buffer of the level that predicts its point — the largest stride that divides all
// its coordinates, capped at the coarsest level (whose buffer also holds the anchors / the first point) — and is dropped outside that
// buffer's window
template <typename T>
__global__ __launch_bounds__(256) void k_region_scatter_raw(const uint8_t *__restrict__ payload, uint64_t idx_off, uint64_t val_off, uint64_t cnt, uint64_t n,
                                                            szk_region_bufs g, T *__restrict__ scratch) {
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
        uint64_t o = 0;
        bool in = true;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint64_t q = (c[j] - g.wlo[b][j]) >> ls;
            in = in && c[j] >= g.wlo[b][j] && q < g.cnt[b][j];
            o = o * g.cnt[b][j] + q;
        }
        if (in) scratch[g.base[b] + o] = val[i];
    }
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
__global__ __launch_bounds__(256) void k_region_regrid(const T *__restrict__ src, T *__restrict__ dst, szk_region_regrid p) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.total) return;
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

// one directional pass over its window. first / step / cnt: the window's lattice (full coordinates); wlo / boff: the level's buffer.
struct szk_region_pass {
    int N, dir, interp_id, old_api, subpass, radius;
    uint32_t ls;  // log2 s
    uint64_t s, bsz, total, belems;
    uint64_t dims[4], off[4], first[4], step[4], cnt[4], wlo[4], boff[4];
    double eb;
};
template <typename T, typename IT>
__device__ __forceinline__ void region_point(T *__restrict__ buf, const uint16_t *__restrict__ codes, const szk_region_pass &p, uint64_t t) {
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
template <typename T>
__global__ __launch_bounds__(256) void k_region_pass(T *__restrict__ buf, const uint16_t *__restrict__ codes, szk_region_pass p) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.total) return;
    if (p.total <= 0xFFFFFFFFull) region_point<T, uint32_t>(buf, codes, p, t);  // (uniform branch; then every count fits 32 bits too)
    else region_point<T, uint64_t>(buf, codes, p, t);
}
// without anchors the first element is predicted by 0 (k_interp_first_dec)
template <typename T>
__global__ __launch_bounds__(64) void k_region_first(T *__restrict__ buf, const uint16_t *__restrict__ codes, double eb, int radius) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && codes[0]) buf[0] = ref_recover<T>((T)0, codes[0], eb, radius);
}

// ---- host: the launches ---------------------------------------------------------------------------------------------------------------
template <typename T>
static int run_region(const szk_interp_params &ip, const szk_region_geom &g, const uint8_t *payload, uint64_t vout_idx_off, uint64_t vout_val_off,
                      uint64_t n_vout, const uint16_t *codes, T *scratch, T *d_out, hipStream_t s) {
    const int N = g.N;
    uint64_t num = 1, off[4] = {0, 0, 0, 0};  // off: a step of the (coarse) grid in the FULL code array
    for (int j = N - 1; j >= 0; j--) {
        off[j] = num << g.shift;
        num *= g.full[j];
    }
    if (n_vout) {
        szk_region_bufs rb;
        memset(&rb, 0, sizeof(rb));
        rb.nbuf = (uint32_t)g.nbuf;
        rb.shift = (uint32_t)g.shift;
        for (int i = 0; i < 4; i++) {
            const int j = i - (4 - N);
            rb.full[i] = j >= 0 ? g.full[j] : 1;
            for (int b = 0; b < g.nbuf; b++) {
                rb.wlo[b][i] = j >= 0 ? g.lv[b].wlo[j] : 0;
                rb.cnt[b][i] = j >= 0 ? g.lv[b].cnt[j] : 1;
            }
        }
        for (int b = 0; b < g.nbuf; b++) rb.base[b] = g.lv[b].base;
        const uint32_t gr = (uint32_t)((n_vout + 255) / 256 < 4096 ? (n_vout + 255) / 256 : 4096);
        hipLaunchKernelGGL((k_region_scatter_raw<T>), dim3(gr), dim3(256), 0, s, payload, vout_idx_off, vout_val_off, n_vout, num, rb, scratch);
    }
    if (g.anchor == 0) {  // the first point, when the coarsest window holds it (then it is the buffer's first element)
        bool at0 = true;
        for (int j = 0; j < N; j++) at0 = at0 && g.lv[0].wlo[j] == 0;
        if (at0) hipLaunchKernelGGL((k_region_first<T>), dim3(1), dim3(64), 0, s, scratch + g.lv[0].base, codes, ip.eb, ip.radius);
    }
    for (int b = 0; b < g.n_levels; b++) {
        const szk_region_level &lv = g.lv[b];
        if (b > 0) {
            const szk_region_level &up = g.lv[b - 1];
            szk_region_regrid rg;
            memset(&rg, 0, sizeof(rg));
            rg.total = 1;
            for (int i = 0; i < 4; i++) {
                const int j = i - (4 - N);
                rg.dcnt[i] = j >= 0 ? lv.cnt[j] : 1;
                rg.scnt[i] = j >= 0 ? up.cnt[j] : 1;
                rg.ev[i] = (rg.dcnt[i] + 1) / 2;
                if (j >= 0 && lv.wlo[j] < up.wlo[j]) return -1;
                rg.shift[i] = j >= 0 ? (lv.wlo[j] - up.wlo[j]) / up.s : 0;
                rg.total *= rg.ev[i];
            }
            const uint64_t nb = (rg.total + 255) / 256;
            if (nb > 0x7FFFFFFFull) return -1;
            hipLaunchKernelGGL((k_region_regrid<T>), dim3((uint32_t)nb), dim3(256), 0, s, (const T *)(scratch + up.base), scratch + lv.base, rg);
        }
        const int level = g.n_levels - b;  // the level's number on the grid: stride 2^(level - 1); in the full array it is level + shift
        szk_region_pass p;
        memset(&p, 0, sizeof(p));
        p.N = N;
        p.interp_id = ip.interp_id;
        p.old_api = N <= 2;
        p.radius = ip.radius;
        p.s = lv.s;
        p.ls = (uint32_t)(level - 1);
        p.bsz = 32ull * lv.s;
        p.belems = lv.elems;
        p.eb = szk_interp_level_eb(ip.eb, ip.alpha, ip.beta, level + g.shift);
        for (int j = 0; j < N; j++) {
            p.dims[j] = g.dims[j];
            p.off[j] = off[j];
            p.wlo[j] = lv.wlo[j];
            p.boff[j] = lv.boff[j];
        }
        for (int k = 0; k < N; k++) {
            p.dir = g.perm[k];
            p.total = szk_region_pass_window(&g, b, k, p.first, p.step, p.cnt);
            if (p.total == 0) continue;
            for (int j = 0; j < N; j++)  // the window lies on the buffer
                if (p.first[j] < lv.wlo[j] || (p.first[j] + (p.cnt[j] - 1) * p.step[j] - lv.wlo[j]) / lv.s >= lv.cnt[j]) return -1;
            const uint64_t nb = (p.total + 255) / 256;
            if (nb > 0x7FFFFFFFull) return -1;
            p.subpass = 0;
            hipLaunchKernelGGL((k_region_pass<T>), dim3((uint32_t)nb), dim3(256), 0, s, scratch + lv.base, codes, p);
            if (!p.old_api && p.interp_id == 0) {  // the deferred last point of even-length lines, as in run_interp
                p.subpass = 1;
                hipLaunchKernelGGL((k_region_pass<T>), dim3((uint32_t)nb), dim3(256), 0, s, scratch + lv.base, codes, p);
            }
        }
    }
    // the box, out of the finest buffer (stride 1)
    const szk_region_level &fin = g.lv[g.nbuf - 1];
    szk_view v;
    memset(&v, 0, sizeof(v));
    uint64_t corner = 0;
    for (int i = 0; i < 4; i++) {
        const int j = i - (4 - N);
        v.dims[i] = j >= 0 ? g.ext[j] : 1;
        v.str[i] = j >= 0 ? (int64_t)fin.boff[j] : 0;
        if (j >= 0) corner += (g.lo[j] - fin.wlo[j]) * fin.boff[j];
    }
    v.contig = 0;
    if (szk_launch_gather(sizeof(T) == 4 ? 0 : 1, 0, scratch + fin.base + corner, &v, d_out, nullptr, s)) return -2;
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

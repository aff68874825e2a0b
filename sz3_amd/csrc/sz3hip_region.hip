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
// test hook (sz3hip_debug_region_launches): kernel launches the box reconstructions of this process issued, single and multi
static std::atomic<uint64_t> g_region_launches{0};
uint64_t szk_region_launches(void) { return g_region_launches.load(); }
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
        g_region_launches++;
    }
    if (g.anchor == 0) {  // the first point, when the coarsest window holds it (then it is the buffer's first element)
        bool at0 = true;
        for (int j = 0; j < N; j++) at0 = at0 && g.lv[0].wlo[j] == 0;
        if (at0) {
            hipLaunchKernelGGL((k_region_first<T>), dim3(1), dim3(64), 0, s, scratch + g.lv[0].base, codes, ip.eb, ip.radius);
            g_region_launches++;
        }
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
            g_region_launches++;
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
            g_region_launches++;
            if (!p.old_api && p.interp_id == 0) {  // the deferred last point of even-length lines, as in run_interp
                p.subpass = 1;
                hipLaunchKernelGGL((k_region_pass<T>), dim3((uint32_t)nb), dim3(256), 0, s, scratch + lv.base, codes, p);
                g_region_launches++;
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
    g_region_launches++;
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
struct szk_region_scatter_shared {
    uint64_t full[4];
    uint32_t nbuf, shift;
};
#define SZK_SCATTER_ROW 9  // words per buffer of a box's scatter record: wlo[4], cnt[4], base
static_assert(sizeof(szk_region_pass_box) == 19 * 8 && sizeof(szk_region_regrid_box) == 19 * 8 && sizeof(szk_region_gather_box) == 11 * 8, "table records are rows of words");

// k_region_scatter_raw per box: every box scans the whole list (as its own call would) and keeps what falls into its windows
template <typename T>
__global__ __launch_bounds__(256) void k_region_scatter_raw_multi(const uint8_t *__restrict__ payload, uint64_t idx_off, uint64_t val_off, uint64_t cnt, uint64_t n,
                                                                  szk_region_scatter_shared g, const uint64_t *__restrict__ tab, T *__restrict__ scratch) {
    const uint64_t *idx = reinterpret_cast<const uint64_t *>(payload + idx_off);
    const T *val = reinterpret_cast<const T *>(payload + val_off);
    const uint64_t *rec = tab + (uint64_t)blockIdx.y * g.nbuf * SZK_SCATTER_ROW;
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
        const uint32_t top = g.nbuf - 1;
        const uint32_t tz = any ? (uint32_t)(__ffsll((long long)any) - 1) : 64u;
        const uint32_t b = tz >= top ? 0u : top - tz;
        const uint32_t ls = top - b;
        const uint64_t *lv = rec + (uint64_t)b * SZK_SCATTER_ROW;
        uint64_t o = 0;
        bool in = true;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint64_t wlo = lv[j], bc = lv[4 + j];
            const uint64_t q = (c[j] - wlo) >> ls;
            in = in && c[j] >= wlo && q < bc;
            o = o * bc + q;
        }
        if (in) scratch[lv[8] + o] = val[i];
    }
}
template <typename T>
__global__ __launch_bounds__(64) void k_region_first_multi(T *__restrict__ scratch, const uint16_t *__restrict__ codes, double eb, int radius,
                                                           const szk_region_first_box *__restrict__ recs) {
    const szk_region_first_box &r = recs[blockIdx.y];
    if (threadIdx.x == 0 && blockIdx.x == 0 && r.total && codes[0]) scratch[r.base] = ref_recover<T>((T)0, codes[0], eb, radius);
}
template <typename T>
__global__ __launch_bounds__(256) void k_region_regrid_multi(T *__restrict__ scratch, const szk_region_regrid_box *__restrict__ recs) {
    const szk_region_regrid_box &b = recs[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= b.g.total) return;
    uint64_t r = t, so = 0, dx = 0;
    uint64_t m[4];
#pragma unroll
    for (int j = 3; j >= 0; j--) {
        m[j] = r % b.g.ev[j];
        r /= b.g.ev[j];
    }
    bool in = true;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t sq = m[j] + b.g.shift[j];
        in = in && sq < b.g.scnt[j];
        so = so * b.g.scnt[j] + sq;
        dx = dx * b.g.dcnt[j] + 2 * m[j];
    }
    if (in) scratch[b.dst + dx] = scratch[b.src + so];
}
// the pass of one box is region_point over szk_region_pass put together again from the two parts; IT by the box's own total, as k_region_pass
// chooses it
template <typename T>
__global__ __launch_bounds__(256) void k_region_pass_multi(T *__restrict__ scratch, const uint16_t *__restrict__ codes, szk_region_pass_shared sh,
                                                           const szk_region_pass_box *__restrict__ recs) {
    const szk_region_pass_box &b = recs[blockIdx.y];
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t total = b.total;
    if (t >= total) return;
    szk_region_pass_parts p;
    p.N = sh.N;
    p.dir = sh.dir;
    p.interp_id = sh.interp_id;
    p.old_api = sh.old_api;
    p.subpass = sh.subpass;
    p.radius = sh.radius;
    p.ls = sh.ls;
    p.s = sh.s;
    p.bsz = sh.bsz;
    p.total = total;
    p.belems = b.belems;
    p.eb = sh.eb;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        p.dims.v[j] = sh.dims[j];
        p.off[j] = sh.off[j];
        p.step[j] = sh.step[j];
        p.first[j] = b.first[j];
        p.cnt[j] = b.cnt[j];
        p.wlo[j] = b.wlo[j];
        p.boff.v[j] = b.boff[j];
    }
    if (total <= 0xFFFFFFFFull) region_point<T, uint32_t>(scratch + b.base, codes, p, t);
    else region_point<T, uint64_t>(scratch + b.base, codes, p, t);
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


// ---- the coarsest levels of a request in ONE launch ---------------------------------------------------------------------
// All but the finest one or two levels of a box are a few thousand points each, and every one of them costs a launch or two per pass. Here one
// workgroup per box (blockIdx.x) walks a step table — first point, regrid, pass, deferred sub-pass — over the request's coarsest levels: each
// step is a loop t = threadIdx.x, += 1024 over the body of the multi kernel it replaces (the pass: region_point<T, uint32_t> over
// szk_region_pass_parts, put together as k_region_pass_multi does), so the arithmetic is that path's by construction. A __syncthreads() follows
// every step and every thread reaches it (no return around it): the only ordering there is. The box's level buffers are written and read by
// this one workgroup, in place, with plain loads and stores; `scratch` is neither read-only nor __restrict__ here. No waiting between
// workgroups, no flags, no atomics, no LDS. A step's records are the multi kernels' own, in the request's table: `rec` is box 0's record (box
// i's follows i records on), `shared` a pass's szk_region_pass_shared (subpass as the step says), both in words from the table's start.
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
            if (threadIdx.x == 0 && r.total && codes[0]) scratch[r.base] = ref_recover<T>((T)0, codes[0], eb0, radius);
        } else if (st.kind == 2) {  // k_region_regrid_multi
            const szk_region_regrid_box &b = reinterpret_cast<const szk_region_regrid_box *>(tab + st.rec)[box];
            for (uint64_t t = threadIdx.x; t < b.g.total; t += 1024) {
                uint64_t r = t, so = 0, dx = 0;
                uint64_t m[4];
#pragma unroll
                for (int j = 3; j >= 0; j--) {
                    m[j] = r % b.g.ev[j];
                    r /= b.g.ev[j];
                }
                bool in = true;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const uint64_t sq = m[j] + b.g.shift[j];
                    in = in && sq < b.g.scnt[j];
                    so = so * b.g.scnt[j] + sq;
                    dx = dx * b.g.dcnt[j] + 2 * m[j];
                }
                if (in) scratch[b.dst + dx] = scratch[b.src + so];
            }
        } else {  // k_region_pass_multi
            const szk_region_pass_shared &sh = *reinterpret_cast<const szk_region_pass_shared *>(tab + st.shared);
            const szk_region_pass_box &b = reinterpret_cast<const szk_region_pass_box *>(tab + st.rec)[box];
            const uint64_t total = b.total;  // (at most chain_points, a 32-bit number: the host chose the levels so)
            szk_region_pass_parts p;
            p.N = sh.N;
            p.dir = sh.dir;
            p.interp_id = sh.interp_id;
            p.old_api = sh.old_api;
            p.subpass = (int)st.subpass;
            p.radius = sh.radius;
            p.ls = sh.ls;
            p.s = sh.s;
            p.bsz = sh.bsz;
            p.total = total;
            p.belems = b.belems;
            p.eb = sh.eb;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                p.dims.v[j] = sh.dims[j];
                p.off[j] = sh.off[j];
                p.step[j] = sh.step[j];
                p.first[j] = b.first[j];
                p.cnt[j] = b.cnt[j];
                p.wlo[j] = b.wlo[j];
                p.boff.v[j] = b.boff[j];
            }
            T *buf = scratch + b.base;
            for (uint64_t t = threadIdx.x; t < total; t += 1024) region_point<T, uint32_t>(buf, codes, p, t);
        }
        __syncthreads();
    }
}

// words the table of a request of n boxes takes (an upper bound: every box with every record; behind them the chain's pass parameters and steps)
uint64_t szk_region_multi_table_words(const szk_region_geom *gs, uint32_t n) {
    const uint64_t nb = (uint64_t)gs[0].nbuf, nl = (uint64_t)gs[0].n_levels, N = (uint64_t)gs[0].N;
    return (uint64_t)n * (nb * SZK_SCATTER_ROW + 2 + nl * 19 + nl * N * 19 + 11) + nl * N * 19 + (1 + nl * (1 + 2 * N)) * 4;
}

namespace {
struct MultiLaunch {
    int kind;  // 0 scatter, 1 first, 2 regrid, 3 pass, 4 gather
    uint64_t off;  // the launch's records in the table, in words
    uint32_t gx;
    bool twice;    // pass: the deferred points' launch follows
    szk_region_pass_shared sh;
    bool chained;  // the launch is a step of the chain's one launch instead
};
}  // namespace
template <typename T>
static int run_region_multi(const szk_interp_params &ip, const szk_region_geom *gs, uint32_t n, uint64_t scratch_elems, const uint8_t *payload,
                            uint64_t vout_idx_off, uint64_t vout_val_off, uint64_t n_vout, const uint16_t *codes, T *scratch, void *const *d_outs,
                            uint64_t *h_table, uint64_t *d_table, uint64_t table_words, hipEvent_t copied, hipStream_t s, uint32_t chain_points = 0,
                            uint32_t *chain_levels = nullptr, uint32_t *launches = nullptr) {
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
    uint32_t issued = 0;
    uint64_t num = 1, off[4] = {0, 0, 0, 0};
    for (int j = N - 1; j >= 0; j--) {
        off[j] = num << g0.shift;
        num *= g0.full[j];
    }
    // every box's buffers inside the scratch, before anything is built
    for (uint32_t i = 0; i < n; i++)
        for (int b = 0; b < nbuf; b++)
            if (gs[i].lv[b].base > scratch_elems || gs[i].lv[b].elems > scratch_elems - gs[i].lv[b].base) return -1;
    std::vector<MultiLaunch> seq;
    uint64_t w = 0;  // the table's cursor
    auto room = [&](uint64_t words) { return words <= table_words && w <= table_words - words; };
    auto grid_of = [](uint64_t total, uint32_t *gx) {
        const uint64_t nb = (total + 255) / 256;
        if (nb > 0x7FFFFFFFull) return false;
        *gx = (uint32_t)nb;
        return true;
    };
    if (n_vout) {
        if (!room((uint64_t)n * nbuf * SZK_SCATTER_ROW)) return -1;
        MultiLaunch l{};
        l.kind = 0;
        l.off = w;
        l.gx = (uint32_t)((n_vout + 255) / 256 < 4096 ? (n_vout + 255) / 256 : 4096);
        for (uint32_t i = 0; i < n; i++)
            for (int b = 0; b < nbuf; b++) {
                uint64_t *row = h_table + w;
                for (int q = 0; q < 4; q++) {
                    const int j = q - (4 - N);
                    row[q] = j >= 0 ? gs[i].lv[b].wlo[j] : 0;
                    row[4 + q] = j >= 0 ? gs[i].lv[b].cnt[j] : 1;
                }
                row[8] = gs[i].lv[b].base;
                w += SZK_SCATTER_ROW;
            }
        seq.push_back(l);
    }
    if (g0.anchor == 0) {  // the first point, for the boxes whose coarsest window holds it
        if (!room((uint64_t)n * 2)) return -1;
        bool any = false;
        const uint64_t at = w;
        for (uint32_t i = 0; i < n; i++) {
            bool at0 = true;
            for (int j = 0; j < N; j++) at0 = at0 && gs[i].lv[0].wlo[j] == 0;
            szk_region_first_box r = {at0 ? 1ull : 0ull, gs[i].lv[0].base};
            memcpy(h_table + w, &r, sizeof(r));
            w += 2;
            any = any || at0;
        }
        if (any) {
            MultiLaunch l{};
            l.kind = 1;
            l.off = at;
            l.gx = 1;
            l.chained = c > 0;
            seq.push_back(l);
        } else {
            w = at;
        }
    }
    for (int b = 0; b < n_levels; b++) {
        if (b > 0) {
            if (!room((uint64_t)n * 19)) return -1;
            MultiLaunch l{};
            l.kind = 2;
            l.off = w;
            uint64_t most = 0;
            for (uint32_t i = 0; i < n; i++) {
                const szk_region_level &lv = gs[i].lv[b], &up = gs[i].lv[b - 1];
                szk_region_regrid_box r;
                memset(&r, 0, sizeof(r));
                r.g.total = 1;
                for (int q = 0; q < 4; q++) {
                    const int j = q - (4 - N);
                    r.g.dcnt[q] = j >= 0 ? lv.cnt[j] : 1;
                    r.g.scnt[q] = j >= 0 ? up.cnt[j] : 1;
                    r.g.ev[q] = (r.g.dcnt[q] + 1) / 2;
                    if (j >= 0 && lv.wlo[j] < up.wlo[j]) return -1;
                    r.g.shift[q] = j >= 0 ? (lv.wlo[j] - up.wlo[j]) / up.s : 0;
                    r.g.total *= r.g.ev[q];
                }
                r.src = up.base;
                r.dst = lv.base;
                memcpy(h_table + w, &r, sizeof(r));
                w += 19;
                most = r.g.total > most ? r.g.total : most;
            }
            if (!grid_of(most, &l.gx)) return -1;
            l.chained = b < c;
            if (most) seq.push_back(l);
            else w = l.off;
        }
        const int level = n_levels - b;
        szk_region_pass_shared sh;
        memset(&sh, 0, sizeof(sh));
        sh.N = N;
        sh.interp_id = ip.interp_id;
        sh.old_api = N <= 2;
        sh.radius = ip.radius;
        sh.s = g0.lv[b].s;
        sh.ls = (uint32_t)(level - 1);
        sh.bsz = 32ull * sh.s;
        sh.eb = szk_interp_level_eb(ip.eb, ip.alpha, ip.beta, level + g0.shift);
        for (int j = 0; j < N; j++) {
            sh.dims[j] = g0.dims[j];
            sh.off[j] = off[j];
        }
        for (int k = 0; k < N; k++) {
            if (!room((uint64_t)n * 19)) return -1;
            MultiLaunch l{};
            l.kind = 3;
            l.off = w;
            sh.dir = g0.perm[k];
            uint64_t most = 0;
            for (uint32_t i = 0; i < n; i++) {
                const szk_region_level &lv = gs[i].lv[b];
                szk_region_pass_box r;
                memset(&r, 0, sizeof(r));
                uint64_t step[4] = {0, 0, 0, 0};
                r.total = szk_region_pass_window(&gs[i], b, k, r.first, step, r.cnt);
                for (int j = 0; j < N; j++) {
                    if (i == 0) sh.step[j] = step[j];
                    else if (sh.step[j] != step[j]) return -1;  // (the lattice's steps are the level's and the pass's)
                    if (r.total && (r.first[j] < lv.wlo[j] || (r.first[j] + (r.cnt[j] - 1) * step[j] - lv.wlo[j]) / lv.s >= lv.cnt[j])) return -1;  // the window lies on the buffer
                    r.wlo[j] = lv.wlo[j];
                    r.boff[j] = lv.boff[j];
                }
                r.belems = lv.elems;
                r.base = lv.base;
                memcpy(h_table + w, &r, sizeof(r));
                w += 19;
                most = r.total > most ? r.total : most;
            }
            if (!grid_of(most, &l.gx)) return -1;
            if (most == 0) {  // (no box has a point in this pass)
                w = l.off;
                continue;
            }
            l.sh = sh;
            l.twice = !sh.old_api && sh.interp_id == 0;
            l.chained = b < c;
            seq.push_back(l);
        }
    }
    {   // the boxes, out of their finest buffers (stride 1)
        if (!room((uint64_t)n * 11)) return -1;
        MultiLaunch l{};
        l.kind = 4;
        l.off = w;
        uint64_t most = 0;
        for (uint32_t i = 0; i < n; i++) {
            const szk_region_geom &g = gs[i];
            const szk_region_level &fin = g.lv[nbuf - 1];
            szk_region_gather_box r;
            memset(&r, 0, sizeof(r));
            r.total = 1;
            r.src = fin.base;
            r.dst = d_outs[i];
            for (int q = 0; q < 4; q++) {
                const int j = q - (4 - N);
                r.ext[q] = j >= 0 ? g.ext[j] : 1;
                r.str[q] = j >= 0 ? fin.boff[j] : 0;
                if (j >= 0) {
                    if (g.lo[j] < fin.wlo[j] || g.lo[j] - fin.wlo[j] + g.ext[j] > fin.cnt[j]) return -1;  // the box lies on the buffer
                    r.src += (g.lo[j] - fin.wlo[j]) * fin.boff[j];
                    r.total *= g.ext[j];
                }
            }
            memcpy(h_table + w, &r, sizeof(r));
            w += 11;
            most = r.total > most ? r.total : most;
        }
        if (!grid_of(most, &l.gx)) return -1;
        seq.push_back(l);
    }
    // the chain's steps, behind the boxes' records: the chained launches in their order, a pass's shared part in front of its step(s)
    uint64_t steps_off = 0;
    uint32_t n_steps = 0;
    if (c > 0) {
        std::vector<szk_chain_step> steps;
        for (const MultiLaunch &l : seq) {
            if (!l.chained) continue;
            szk_chain_step st = {(uint64_t)l.kind, 0, l.off, 0};
            if (l.kind == 3) {
                if (!room(19)) return -1;
                szk_region_pass_shared sh = l.sh;
                sh.subpass = 0;
                memcpy(h_table + w, &sh, sizeof(sh));
                st.shared = w;
                w += 19;
            }
            steps.push_back(st);
            if (l.kind == 3 && l.twice) {  // the deferred last point of even-length lines: a step of its own, behind a barrier
                st.subpass = 1;
                steps.push_back(st);
            }
        }
        if (!room(steps.size() * 4)) return -1;
        steps_off = w;
        n_steps = (uint32_t)steps.size();
        memcpy(h_table + w, steps.data(), steps.size() * sizeof(szk_chain_step));
        w += steps.size() * 4;
    }
    // the whole table by one copy, in front of the first launch; `copied` tells the next call's build when the pinned array may be rewritten
    if (hipMemcpyAsync(d_table, h_table, w * 8, hipMemcpyHostToDevice, s) != hipSuccess) return -2;
    if (hipEventRecord(copied, s) != hipSuccess) return -2;
    szk_region_scatter_shared ss;
    memset(&ss, 0, sizeof(ss));
    ss.nbuf = (uint32_t)nbuf;
    ss.shift = (uint32_t)g0.shift;
    for (int q = 0; q < 4; q++) ss.full[q] = q - (4 - N) >= 0 ? g0.full[q - (4 - N)] : 1;
    bool chain_done = false;
    for (const MultiLaunch &l : seq) {
        if (l.chained) {  // (the chained launches follow each other in seq: the one launch stands where the first of them stood)
            if (!chain_done && n_steps) {
                hipLaunchKernelGGL((k_region_chain_multi<T>), dim3(n), dim3(1024), 0, s, scratch, codes, ip.eb, ip.radius, (const uint64_t *)d_table, steps_off, n_steps);
                g_region_launches++;
                issued++;
            }
            chain_done = true;
            continue;
        }
        const dim3 grid(l.gx, n);
        const uint64_t *rec = d_table + l.off;
        switch (l.kind) {
        case 0:
            hipLaunchKernelGGL((k_region_scatter_raw_multi<T>), grid, dim3(256), 0, s, payload, vout_idx_off, vout_val_off, n_vout, num, ss, rec, scratch);
            break;
        case 1:
            hipLaunchKernelGGL((k_region_first_multi<T>), grid, dim3(64), 0, s, scratch, codes, ip.eb, ip.radius, reinterpret_cast<const szk_region_first_box *>(rec));
            break;
        case 2:
            hipLaunchKernelGGL((k_region_regrid_multi<T>), grid, dim3(256), 0, s, scratch, reinterpret_cast<const szk_region_regrid_box *>(rec));
            break;
        case 3: {
            szk_region_pass_shared sh = l.sh;
            sh.subpass = 0;
            hipLaunchKernelGGL((k_region_pass_multi<T>), grid, dim3(256), 0, s, scratch, codes, sh, reinterpret_cast<const szk_region_pass_box *>(rec));
            if (l.twice) {  // the deferred last point of even-length lines, as in run_region
                sh.subpass = 1;
                g_region_launches++;
                issued++;
                hipLaunchKernelGGL((k_region_pass_multi<T>), grid, dim3(256), 0, s, scratch, codes, sh, reinterpret_cast<const szk_region_pass_box *>(rec));
            }
            break;
        }
        default:
            hipLaunchKernelGGL((k_region_gather_multi<T>), grid, dim3(256), 0, s, (const T *)scratch, reinterpret_cast<const szk_region_gather_box *>(rec));
        }
        g_region_launches++;
        issued++;
    }
    if (launches) *launches = issued;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int szk_launch_interp_decompress_region_multi(int dtype, const szk_interp_params *ip, const szk_region_geom *gs, uint32_t n, uint64_t scratch_elems,
                                              const uint8_t *payload, uint64_t vout_idx_off, uint64_t vout_val_off, uint64_t n_vout, const uint16_t *codes,
                                              void *scratch, void *const *d_outs, uint64_t *h_table, uint64_t *d_table, uint64_t table_words, hipEvent_t copied,
                                              hipStream_t s) {
    return szk_launch_interp_decompress_region_chain(dtype, ip, gs, n, scratch_elems, payload, vout_idx_off, vout_val_off, n_vout, codes, scratch, d_outs, h_table, d_table,
                                                     table_words, copied, s, 0, nullptr, nullptr);
}
int szk_launch_interp_decompress_region_chain(int dtype, const szk_interp_params *ip, const szk_region_geom *gs, uint32_t n, uint64_t scratch_elems,
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

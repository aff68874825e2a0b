// sz3_amd/csrc/sz3hip_stream.cpp — an opened stream: everything of a partial decode that does not depend on the box is done
// once, at open; a request is the reconstruction alone.
//
// Open runs the existing decode chain with the request kind SZI_OPEN (sz3hip_internal.h): the chain stops behind its Huffman stage — the dense
// launch over every unit; a stock ALGO_INTERP stream: the stock decoder and k_stock_to_elem — and copies the per-element codes and the raw-value
// lists into arrays of their own. The handle keeps those, the interpolation parameters, a region scratch and the pinned / device tables: a leaner
// set than a context (no histogram, code books, outlier lists or payload). A container that is no single interpolation stream is decoded in full,
// once, into an array the handle keeps; its requests are strided gathers.
// A request (sz3hip_stream_tiles) is boxes_prepare's checks and the multi-box reconstruction (sz3hip_region.hip) against the resident arrays.
// sz3hip_stream_request takes boxes of several levels, each into a strided view of its own: the views' checks are here,
// the one launch sequence aligned by array level in sz3hip_region.hip.
// sz3hip_stream_reduce takes the same boxes without views and leaves numbers about them in device memory: the request's
// geometry and sequence with a reduction and its final fold (sz3hip_reduce.hip) in the gather's place; sz3hip_reduce_device is that reduction
// over one plain view.
// sz3hip_stream_select takes the boxes with an index and a value array each and leaves where their values lie in a
// range: the same geometry and sequence with a count, a scan and the write (sz3hip_select.hip) in the gather's place; sz3hip_select_device is
// that selection over one plain view.
// sz3hip_stream_map takes the request's own boxes and views, the views in OUTPUT elements, and leaves texels: the same
// geometry and sequence with one mapping launch (sz3hip_map.hip) in the gather's place; sz3hip_map_device is that mapping over one plain view.
// sz3hip_stream_sample takes the boxes with queries at fractional positions each and leaves the nearest point's bytes
// or the linear interpolation: the same geometry and sequence with one sampling launch (sz3hip_sample.hip) in the gather's place;
// sz3hip_sample_device is that sampling over one plain view.
// sz3hip_stream_project takes the request's own boxes and collapses each along one axis into a view of OUTPUT elements:
// the same geometry and sequence with one projecting launch (sz3hip_project.hip) in the gather's place; sz3hip_project_device is that
// projection over one plain view.
// sz3hip_stream_gradient takes the request's own boxes and leaves their derivatives by central differences — one axis,
// the squared magnitude, the magnitude or the vector — in views of OUTPUT elements: the same geometry and sequence with one differentiating
// launch (sz3hip_gradient.hip) in the gather's place; sz3hip_gradient_device is that gradient over one plain view.
// sz3hip_stream_composite takes the request's own boxes and leaves each folded front to back along one axis through an
// RGBA table — one compositing launch (sz3hip_composite.hip) in the gather's place; sz3hip_composite_device is that fold over one plain view.
// A handle serves one request at a time; it is not thread-safe.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <math.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/sz3hip.h"
#include "sz3hip_format.h"
#include "sz3hip_internal.h"
#include "sz3hip_kernels.h"

#define fail szi_fail
#define HIPCHK(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) return fail(SZ3HIP_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

struct sz3hip_stream {
    int device = 0, dtype = 0;
    int N = 0;
    uint64_t dims[4] = {0, 0, 0, 0}, num = 0;
    sz3hip_config conf;
    bool fast = false;
    szi_stream_codes codes;  // fast: the codes, the lists, the parameters
    void *d_full = nullptr;  // else: the full decode
    void *d_region = nullptr;  // the levels' compact buffers of a request's boxes: made by the first request, grown when one needs more, kept
    uint64_t region_cap = 0;
    uint64_t *h_table = nullptr, *d_table = nullptr;  // the records a request's workgroups read, pinned and on the device
    uint64_t table_cap = 0;
    hipEvent_t ev_table = nullptr;  // recorded behind the table's copy: the next request waits for it before it writes h_table
    bool table_pending = false;
    hipEvent_t ev_req = nullptr;  // recorded behind a request's last launch: a request on another stream is ordered behind it (scratch and tables are shared)
    bool req_pending = false;
    hipStream_t last_stream = nullptr;
    uint32_t huffman_stages = 0, launches_last = 0, chain_last = 0, levels_last = 0, chain_points_last = 0;
    uint64_t requests = 0;
};

namespace {
struct DeviceScope {  // the caller's current device is left as it was found
    int prev = -1;
    DeviceScope() {
        if (hipGetDevice(&prev) != hipSuccess) {
            (void)hipGetLastError();
            prev = -1;
        }
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
inline size_t tsize(int dtype) { return dtype == SZ3HIP_FLOAT ? 4 : 8; }

// the chain's threshold (sz3hip_debug_chain_points; -1: SZ3HIP_CHAIN_POINTS decides at the first request). The default is a measurement
// (DESIGN.md section 15): 0, the chain off
constexpr uint32_t CHAIN_POINTS_DEFAULT = 0;
std::atomic<int64_t> g_chain_points{-1};

int dtype_check(int dataType) {
    if (dataType < 0 || dataType > 9) return fail(SZ3HIP_EUNSUPPORTED, "dataType %d is not one of SZ_FLOAT .. SZ_INT64 (0 .. 9)", dataType);
    if (dataType > SZ3HIP_DOUBLE) return fail(SZ3HIP_EUNSUPPORTED, "the region decode reads float / double arrays; integer element types are not supported yet");
    return 0;
}
void release(sz3hip_stream *h) {
    szi_stream_codes_free(&h->codes);
    if (h->d_full) (void)hipFree(h->d_full);
    if (h->d_region) (void)hipFree(h->d_region);
    if (h->d_table) (void)hipFree(h->d_table);
    if (h->h_table) (void)hipHostFree(h->h_table);
    if (h->ev_table) (void)hipEventDestroy(h->ev_table);
    if (h->ev_req) (void)hipEventDestroy(h->ev_req);
    delete h;
}
int events(sz3hip_stream *h) {
    HIPCHK(hipEventCreateWithFlags(&h->ev_table, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_req, hipEventDisableTiming));
    return 0;
}
// the handle's scratch and table, as a context keeps them (region_reserve, table_reserve of sz3hip_api.cpp): grown when a request needs more
int region_reserve(sz3hip_stream *h, uint64_t elems) {
    if (elems <= h->region_cap) return 0;
    if (h->d_region) {
        HIPCHK(hipDeviceSynchronize());  // (an earlier request's kernels may still read it)
        HIPCHK(hipFree(h->d_region));
    }
    h->d_region = nullptr;
    h->region_cap = 0;
    if (hipMalloc(&h->d_region, elems * tsize(h->dtype) + 64) != hipSuccess) {
        (void)hipGetLastError();
        h->d_region = nullptr;
        return fail(SZ3HIP_EHIP, "no device memory for the region decode's scratch (%zu bytes)", (size_t)(elems * tsize(h->dtype)));
    }
    h->region_cap = elems;
    return 0;
}
int table_reserve(sz3hip_stream *h, uint64_t words) {
    if (words <= h->table_cap) return 0;
    if (h->d_table) {
        HIPCHK(hipDeviceSynchronize());  // (an earlier request's copy and kernels may still read them)
        (void)hipFree(h->d_table);
    }
    if (h->h_table) (void)hipHostFree(h->h_table);
    h->d_table = h->h_table = nullptr;
    h->table_cap = 0;
    h->table_pending = false;
    const uint64_t cap = std::max<uint64_t>(words, 8192);
    HIPCHK(hipHostMalloc((void **)&h->h_table, cap * 8));
    HIPCHK(hipMalloc((void **)&h->d_table, cap * 8));
    h->table_cap = cap;
    return 0;
}
// the boxes of a request against the grid of every 2^level-th point, with the multi-box calls' wording (the fallback: no geometry is made)
int boxes_on_grid(const sz3hip_stream *h, int level, const sz3hip_box *boxes, uint32_t n) {
    for (uint32_t b = 0; b < n; b++)
        for (int i = 0; i < h->N; i++) {
            const uint64_t cd = szi_coarse_extent(h->dims[i], level), lo = boxes[b].lo[i], ext = boxes[b].ext[i];
            if (ext == 0) return fail(SZ3HIP_EINVAL, "box %u: the region has extent 0 in dimension %d", b, i);
            if (lo >= cd || ext > cd - lo)
                return fail(SZ3HIP_EINVAL, "box %u: the region [%llu, %llu + %llu) leaves dimension %d (extent %llu)", b, (unsigned long long)lo, (unsigned long long)lo,
                            (unsigned long long)ext, i, (unsigned long long)cd);
        }
    return 0;
}
}  // namespace

extern "C" void sz3hip_debug_chain_points(uint32_t points) { g_chain_points.store((int64_t)points); }
extern "C" uint32_t sz3hip_debug_get_chain_points(void) {
    if (g_chain_points.load() < 0) {
        const char *e = getenv("SZ3HIP_CHAIN_POINTS");
        g_chain_points.store(e && *e ? (int64_t)std::min<unsigned long long>(strtoull(e, nullptr, 10), 0xFFFFFFFFull) : (int64_t)CHAIN_POINTS_DEFAULT);
    }
    return (uint32_t)g_chain_points.load();
}

extern "C" int sz3hip_stream_open(sz3hip_stream **out, sz3hip_config *conf, int dataType, const char *cmpData, size_t cmpSize, int device) {
    if (!out) return fail(SZ3HIP_EINVAL, "sz3hip_stream_open: NULL argument (out)");
    *out = nullptr;
    int rc = dtype_check(dataType);
    if (rc) return rc;
    sz3hip_stream *h = new sz3hip_stream();
    memset(&h->codes, 0, sizeof(h->codes));
    int fast = 0, huffman = 0;
    DeviceScope scope;
    if (device < 0) device = scope.prev >= 0 ? scope.prev : 0;
    if ((rc = szi_stream_open_container(conf, dataType, cmpData, cmpSize, device, &h->codes, &h->d_full, &fast, &huffman))) {
        release(h);
        return rc;
    }
    h->device = device;
    h->dtype = dataType;
    h->conf = *conf;
    h->fast = fast != 0;
    h->huffman_stages = (uint32_t)huffman;
    h->N = conf->N;
    h->num = conf->num;
    for (int i = 0; i < conf->N; i++) h->dims[i] = conf->dims[i];
    if (hipSetDevice(device) != hipSuccess || (rc = events(h))) {
        release(h);
        return rc ? rc : fail(SZ3HIP_EHIP, "hipSetDevice(%d) failed", device);
    }
    *out = h;
    return 0;
}

extern "C" int sz3hip_stream_open_payload(sz3hip_stream **out, int device, int dataType, const void *d_payload, size_t payload_size, void *stream) {
    if (!out) return fail(SZ3HIP_EINVAL, "sz3hip_stream_open_payload: NULL argument (out)");
    *out = nullptr;
    int rc = dtype_check(dataType);
    if (rc) return rc;
    if (!d_payload) return fail(SZ3HIP_EINVAL, "sz3hip_stream_open_payload: the payload is NULL");
    if (payload_size < sizeof(szh_header)) return fail(SZ3HIP_EFORMAT, "payload shorter than its header");
    DeviceScope scope;
    if (device < 0) device = scope.prev >= 0 ? scope.prev : 0;
    HIPCHK(hipSetDevice(device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipStreamSynchronize(s));  // (what produced the payload comes first)
    szh_header hd;
    HIPCHK(hipMemcpy(&hd, d_payload, sizeof(hd), hipMemcpyDeviceToHost));
    if (hd.magic != SZH_MAGIC) return fail(SZ3HIP_EFORMAT, "not an SZH1 payload");
    if (hd.dtype != dataType) return fail(SZ3HIP_EINVAL, "payload data type does not match the requested one");
    if (hd.n == 0 || hd.ndim < 1 || hd.ndim > 4) return fail(SZ3HIP_EFORMAT, "corrupt SZH1 header");
    // a context for the length of the open: the header's checks, the tables and the Huffman stage are its decode's; it is destroyed before this
    // returns (the handle keeps the codes and the lists, not the context)
    sz3hip_ctx *ctx = sz3hip_ctx_create(device, hd.n, dataType);
    if (!ctx) return sz3hip_last_error_code();
    sz3hip_stream *h = new sz3hip_stream();
    memset(&h->codes, 0, sizeof(h->codes));
    szi_partial q;
    memset(&q, 0, sizeof(q));
    q.kind = SZI_OPEN;
    q.open = &h->codes;
    rc = szi_decompress_device_partial(ctx, d_payload, payload_size, &q, nullptr, s);
    if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = fail(SZ3HIP_EHIP, "the opened stream's decode failed on the device");
    h->fast = rc == 0;
    h->huffman_stages = rc == 0 ? 1 : 0;
    if (rc == SZ3HIP_EUNSUPPORTED) {  // no single interpolation stream the windows nest on: the full decode, once, into an array the handle keeps
        szi_stream_codes_free(&h->codes);
        rc = 0;
        if (hipMalloc(&h->d_full, std::max<size_t>((size_t)hd.n * tsize(dataType), 16)) != hipSuccess) {
            (void)hipGetLastError();
            h->d_full = nullptr;
            rc = fail(SZ3HIP_EHIP, "no device memory for the full-size array (%zu bytes) this payload's opened stream keeps", (size_t)hd.n * tsize(dataType));
        }
        if (!rc) rc = sz3hip_decompress_device(ctx, d_payload, payload_size, h->d_full, s);
        if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = fail(SZ3HIP_EHIP, "the opened stream's full decode failed on the device");
    }
    sz3hip_ctx_destroy(ctx);
    if (!rc) rc = events(h);
    if (rc) {
        release(h);
        return rc;
    }
    h->device = device;
    h->dtype = dataType;
    h->N = (int)hd.ndim;
    h->num = hd.n;
    for (int i = 0; i < h->N; i++) h->dims[i] = hd.dims[4 - h->N + i];
    // the Config a payload implies: the header's extents as they stand (one entry per extent, also of size 1), bound and interpolation fields
    sz3hip_config_init(&h->conf, h->N, h->dims);
    h->conf.N = h->N;
    for (int i = 0; i < 4; i++) h->conf.dims[i] = i < h->N ? h->dims[i] : 0;
    h->conf.num = hd.n;
    h->conf.dataType = (uint8_t)dataType;
    h->conf.cmprAlgo = hd.predictor == 1 ? SZ3HIP_ALGO_HIP_INTERP : SZ3HIP_ALGO_HIP_LORENZO;
    h->conf.errorBoundMode = SZ3HIP_EB_ABS;
    h->conf.absErrorBound = hd.eb;
    h->conf.quantbinCnt = (int32_t)(2 * hd.radius);
    if (hd.predictor == 1) {
        h->conf.interpAlgo = (uint8_t)hd.interp_id;
        h->conf.interpDirection = (uint8_t)hd.interp_dir;
        h->conf.interpAnchorStride = (int32_t)hd.anchor_stride;
        h->conf.interpAlpha = hd.interp_alpha;
        h->conf.interpBeta = hd.interp_beta;
    }
    *out = h;
    return 0;
}

extern "C" int sz3hip_stream_config(const sz3hip_stream *h, sz3hip_config *conf) {
    if (!h || !conf) return fail(SZ3HIP_EINVAL, "sz3hip_stream_config: %s", !h ? "no handle" : "NULL argument (conf)");
    *conf = h->conf;
    return 0;
}

extern "C" int sz3hip_stream_stats(const sz3hip_stream *h, struct sz3hip_stream_stats *st) {
    if (!h || !st) return fail(SZ3HIP_EINVAL, "sz3hip_stream_stats: %s", !h ? "no handle" : "NULL argument (st)");
    memset(st, 0, sizeof(*st));
    st->fast = h->fast ? 1 : 0;
    st->huffman_stages = h->huffman_stages;
    st->launches_last_request = h->launches_last;
    st->chain_levels_last_request = h->chain_last;
    st->units_total = (h->num + SZH_UNIT_SYMS - 1) / SZH_UNIT_SYMS;
    st->requests = h->requests;
    st->scratch_elems = h->region_cap;
    st->resident_bytes = h->codes.bytes + (h->d_full ? std::max<uint64_t>(h->num * tsize(h->dtype), 16) : 0) + (h->d_region ? h->region_cap * tsize(h->dtype) + 64 : 0) +
                         h->table_cap * 8;
    st->n_levels_last_request = h->levels_last;
    st->chain_points = h->chain_points_last;
    return 0;
}

// ---- boxes of several levels in one request, into strided views ----------------------------------------------------------
namespace {
struct ReqView {
    uintptr_t lo, hi;  // the byte hull
    int64_t str[4];    // element strides as the kernels read them: the caller's, or the contiguous ones
    bool atlas;        // the caller's strides are positive and nested over ALL N dimensions: the view may be a rectangle of an atlas
};
// what comes before any geometry: the arguments, every box's reserved word and output pointer
int request_args(const char *who, const sz3hip_tile_req *reqs, uint32_t n) {
    int rc = szi_boxes_args(who, reqs, n, reqs, "reqs");
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) {
        if (reqs[i].reserved) return fail(SZ3HIP_EINVAL, "box %u: the reserved word is %u, not 0", i, reqs[i].reserved);
        if (!reqs[i].d_out) return fail(SZ3HIP_EINVAL, "box %u: the output array is NULL", i);
    }
    return 0;
}
// every view by itself, then every pair (the boxes' extents are checked by now: none is 0)
int request_views(int N, const sz3hip_tile_req *reqs, uint32_t n, size_t tsz, std::vector<ReqView> &vs) {
    vs.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        const sz3hip_tile_req &q = reqs[i];
        ReqView &v = vs[i];
        bool given = false;
        for (int j = 0; j < N; j++) given = given || q.strides[j] != 0;
        uint64_t span = 0;  // the last element's distance from the first
        if (!given) {
            uint64_t run = 1;
            for (int j = N - 1; j >= 0; j--) {
                v.str[j] = (int64_t)run;
                run *= q.box.ext[j];
            }
            span = run - 1;
            v.atlas = false;
        } else {
            int inner = -1;  // the next counted dimension
            v.atlas = true;
            for (int j = N - 1; j >= 0; j--) {
                const int64_t st = q.strides[j];
                v.str[j] = st;
                if (j < N - 1 && (st <= 0 || q.strides[j + 1] <= 0 || (uint64_t)st / (uint64_t)q.strides[j + 1] < q.box.ext[j + 1])) v.atlas = false;
                if (st <= 0) v.atlas = false;
                if (q.box.ext[j] == 1) continue;
                if (st < 0) return fail(SZ3HIP_EINVAL, "box %u: the view's stride of dimension %d is negative (%lld)", i, j, (long long)st);
                if (st == 0) return fail(SZ3HIP_EINVAL, "box %u: the view's stride of dimension %d is zero", i, j);
                if ((uint64_t)st > (1ull << 56) / q.box.ext[j])  // (the hull's byte count stays far inside 64 bits)
                    return fail(SZ3HIP_EINVAL, "box %u: the view's stride of dimension %d is too large (%lld)", i, j, (long long)st);
                if (inner >= 0 && (uint64_t)st / (uint64_t)q.strides[inner] < q.box.ext[inner])
                    return fail(SZ3HIP_EINVAL, "box %u: the view's strides are permuted or overlap: dimension %d's (%lld) is below %llu * dimension %d's (%lld); a view is nested in row-major order",
                                i, j, (long long)st, (unsigned long long)q.box.ext[inner], inner, (long long)q.strides[inner]);
                span += (q.box.ext[j] - 1) * (uint64_t)st;
                inner = j;
            }
        }
        v.lo = (uintptr_t)q.d_out;
        // (span < 4 * 2^56 elements: the byte count cannot wrap; the hull's end could, for a pointer near the top of the address space)
        if ((span + 1) * tsz > UINTPTR_MAX - v.lo) return fail(SZ3HIP_EINVAL, "box %u: the view runs past the end of the address space", i);
        v.hi = v.lo + (uintptr_t)((span + 1) * tsz);
    }
    for (uint32_t i = 1; i < n; i++)
        for (uint32_t k = 0; k < i; k++) {
            if (vs[i].hi <= vs[k].lo || vs[k].hi <= vs[i].lo) continue;  // disjoint hulls
            bool apart = false;
            if (vs[i].atlas && vs[k].atlas && !memcmp(vs[i].str, vs[k].str, N * sizeof(int64_t))) {  // two rectangles of one atlas?
                const uint32_t a = vs[i].lo >= vs[k].lo ? k : i, b = a == i ? k : i;  // b's origin is not below a's
                uint64_t d = (uint64_t)(vs[b].lo - vs[a].lo);
                bool fits = d % tsz == 0;
                d /= tsz;
                for (int j = 0; j < N && fits; j++) {
                    const uint64_t st = (uint64_t)vs[a].str[j], o = d / st;
                    d -= o * st;
                    if (j >= 1 && o + reqs[b].box.ext[j] > (uint64_t)vs[a].str[j - 1] / st) fits = false;
                    if (o >= reqs[a].box.ext[j]) apart = true;
                }
                apart = apart && fits && d == 0;
            }
            if (!apart) return fail(SZ3HIP_EINVAL, "box %u: the output overlaps box %u's, or cannot be shown not to", i, k);
        }
    return 0;
}
}  // namespace

namespace {
// a handle that keeps the full array: every box on the grid of its own level (boxes_on_grid's checks and wording)
int full_boxes_check(const sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n) {
    for (uint32_t b = 0; b < n; b++) {
        if (reqs[b].level < 0 || reqs[b].level > 30) return fail(SZ3HIP_EINVAL, "box %u: tile level %d is outside 0 .. 30", b, reqs[b].level);
        for (int i = 0; i < h->N; i++) {
            const uint64_t cd = szi_coarse_extent(h->dims[i], reqs[b].level), lo = reqs[b].box.lo[i], ext = reqs[b].box.ext[i];
            if (ext == 0) return fail(SZ3HIP_EINVAL, "box %u: the region has extent 0 in dimension %d", b, i);
            if (lo >= cd || ext > cd - lo)
                return fail(SZ3HIP_EINVAL, "box %u: the region [%llu, %llu + %llu) leaves dimension %d (extent %llu)", b, (unsigned long long)lo, (unsigned long long)lo,
                            (unsigned long long)ext, i, (unsigned long long)cd);
        }
    }
    return 0;
}
// ... and its record: the view of the resident array whose strides are multiplied by 2^level, into the caller's view (dstr null: no view — a
// reducing request)
void full_record(const sz3hip_stream *h, const sz3hip_tile_req &q, const int64_t *dstr, szk_region_gather_strided_box *r) {
    uint64_t str[4] = {0, 0, 0, 0}, corner = 0, run = 1;
    for (int i = h->N - 1; i >= 0; i--) {
        corner += (q.box.lo[i] << q.level) * run;
        str[i] = run << q.level;
        run *= h->dims[i];
    }
    szi_view_record(h->N, q.box.ext, str, corner, q.d_out, dstr, r);
}
}  // namespace

// a strided gather's record over a plain view: N extents, the source's element strides and corner, the destination and its strides (null: none)
void szi_view_record(int N, const uint64_t *ext, const uint64_t *str, uint64_t corner, void *dst, const int64_t *dstr, szk_region_gather_strided_box *r) {
    memset(r, 0, sizeof(*r));
    r->total = 1;
    r->src = corner;
    r->dst = dst;
    for (int q = 0; q < 4; q++) {
        const int i = q - (4 - N);
        r->ext[q] = i >= 0 ? ext[i] : 1;
        r->str[q] = i >= 0 && r->ext[q] > 1 ? str[i] : 0;
        r->dstr[q] = i >= 0 && r->ext[q] > 1 && dstr ? dstr[i] : 0;
        r->total *= r->ext[q];
    }
}

// ---- what every call of a kind shares: the plans' prefix, a handle's one submit path, the _device calls' view ------------
namespace {
// the plan structs' shared prefix: sz3hip_request_plan's fields in front of scratch_elems (that one is the call's own)
template <typename Plan, typename Req>
void plan_prefix(Plan *out, const Req *reqs, uint32_t n, const std::vector<szk_region_geom> &gs) {
    out->n = n;
    out->finest_level = out->coarsest_level = reqs[0].level;
    for (uint32_t i = 0; i < n; i++) {
        out->finest_level = std::min(out->finest_level, reqs[i].level);
        out->coarsest_level = std::max(out->coarsest_level, reqs[i].level);
        out->n_levels = std::max(out->n_levels, (int32_t)gs[i].n_levels);
        out->points += gs[i].points;
    }
}

// One request of a handle, whatever its sink. The handle's pinned table, scratch and device table are shared by all of them: submit_begin
// and submit_launch are the one place that orders a request behind the previous one. Between submit_boxes and submit_begin a call runs the
// checks of its own that need the dimension count; nothing is reserved, waited for or launched before all of them passed.
struct Submit {
    sz3hip_stream *h;
    hipStream_t s;
    DeviceScope scope;
    int N;                                  // the stream's dimension count
    const sz3hip_tile_req *reqs = nullptr;  // the boxes; d_out and strides count where the sink's `dst` word is the view (SZK_DST_VIEW)
    uint32_t n = 0;
    std::vector<szk_region_geom> gs;        // fast: the boxes' geometry and the level buffers' elements
    uint64_t elems = 0;
    void *const *d_outs = nullptr;          // sz3hip_stream_tiles: boxes of one level into contiguous arrays, the multi launcher's form
    Submit(sz3hip_stream *h_, void *stream) : h(h_), s((hipStream_t)stream), N(h_->fast ? h_->codes.ip.N : h_->N) {}
};
// every box on the grid of its own level: the geometry, or — a handle that keeps the full array — the checks alone
int submit_boxes(Submit &sub, const sz3hip_tile_req *reqs, uint32_t n) {
    sub.reqs = reqs;
    sub.n = n;
    if (!sub.h->fast) return full_boxes_check(sub.h, reqs, n);
    const szk_interp_params &ip = sub.h->codes.ip;
    return szi_request_geometry(ip.N, ip.dims, ip.interp_id, ip.direction, ip.anchor_stride, reqs, n, sub.gs, &sub.elems);
}
// the device; the scratch (`scratch` elements: the level buffers and what the sink keeps behind them) and the table's room (the sink
// table's); then the two waits
int submit_begin(Submit &sub, const szk_region_sink *sink, uint64_t scratch) {
    sz3hip_stream *h = sub.h;
    const uint64_t words = sub.d_outs ? szk_region_multi_table_words(sub.gs.data(), sub.n) : szk_sink_table_words(sink, h->fast ? sub.gs.data() : nullptr, sub.n);
    int rc;
    HIPCHK(hipSetDevice(h->device));
    if ((rc = region_reserve(h, scratch)) || (rc = table_reserve(h, words))) return rc;
    if (h->table_pending) {  // the previous request's copy of the pinned table, whatever stream it ran on
        HIPCHK(hipEventSynchronize(h->ev_table));
        h->table_pending = false;
    }
    if (h->req_pending && sub.s != h->last_stream) HIPCHK(hipStreamWaitEvent(sub.s, h->ev_req, 0));  // (the scratch and the device table are still the previous request's)
    return 0;
}
// the one launcher call and what follows it. vs: the boxes' views where the sink reads them (null: no strides); first: box i's first
// partial record where the `dst` word carries it (SZK_DST_PART). ev_req is recorded and the handle marked even when the launcher fails
// (part of the sequence may be issued); the statistics change on success only. what: the call's noun in the failure's message
int submit_launch(Submit &sub, const char *what, const szk_region_sink *sink, const std::vector<ReqView> *vs, const uint64_t *first) {
    sz3hip_stream *h = sub.h;
    const uint32_t n = sub.n, chain_points = sz3hip_debug_get_chain_points();
    const int dst = szk_sink(sink).dst;
    auto dst_word = [&](uint32_t i) { return dst == SZK_DST_VIEW ? sub.reqs[i].d_out : (void *)(uintptr_t)(dst == SZK_DST_INDEX ? (uint64_t)i : SZK_REDUCE_DST(first[i], i)); };
    uint32_t chain_levels = 0, launches = 0, levels = 0;
    h->table_pending = true;  // (the launchers record ev_table behind the table's copy)
    // (fast: the lists are the handle's own arrays, handed over as offsets from a null base, as a stock stream's are)
    const szi_stream_codes &c = h->codes;
    const uint64_t vidx = (uint64_t)(uintptr_t)c.d_vidx, vval = (uint64_t)(uintptr_t)c.d_vval;
    int lr;
    if (sub.d_outs) {
        levels = (uint32_t)sub.gs[0].n_levels;
        lr = szk_launch_interp_decompress_region_multi(h->dtype, &c.ip, sub.gs.data(), n, sub.elems, nullptr, vidx, vval, c.n_vout, c.d_codes, h->d_region, sub.d_outs, h->h_table,
                                                       h->d_table, h->table_cap, h->ev_table, sub.s, chain_points, &chain_levels, &launches);
    } else if (!h->fast) {
        std::vector<szk_region_gather_strided_box> full_recs(n);
        for (uint32_t i = 0; i < n; i++) {
            full_record(h, sub.reqs[i], vs ? (*vs)[i].str : nullptr, &full_recs[i]);
            full_recs[i].dst = dst_word(i);
        }
        lr = szk_launch_gather_boxes(h->dtype, h->d_full, full_recs.data(), n, h->h_table, h->d_table, h->table_cap, h->ev_table, sub.s, sink, &launches);
    } else {
        std::vector<szk_region_out> outs(n);
        for (uint32_t i = 0; i < n; i++) {
            outs[i].dst = dst_word(i);
            for (int j = 0; j < 4; j++) outs[i].str[j] = vs && j < sub.N ? (*vs)[i].str[j] : 0;
        }
        lr = szk_launch_interp_decompress_region_request(h->dtype, &c.ip, sub.gs.data(), n, sub.elems, nullptr, vidx, vval, c.n_vout, c.d_codes, h->d_region, outs.data(), h->h_table,
                                                         h->d_table, h->table_cap, h->ev_table, sub.s, chain_points, &chain_levels, &launches, &levels, sink);
    }
    HIPCHK(hipEventRecord(h->ev_req, sub.s));
    h->req_pending = true;
    h->last_stream = sub.s;
    if (lr) return fail(SZ3HIP_EHIP, "the stream's %s could not be launched (%d)", what, lr);
    h->launches_last = launches;
    h->chain_last = chain_levels;
    h->levels_last = levels;
    h->chain_points_last = chain_points;
    h->requests++;
    return 0;
}

// a _device call's arguments in front of its own: the type and the extents ...
int device_dims(int dataType, int N, const uint64_t *dims) {
    const int rc = dtype_check(dataType);
    if (rc) return rc;
    if (N < 1 || N > 4 || !dims) return fail(SZ3HIP_EINVAL, "the dimension count is %d: 1 .. 4 extents are supported", N);
    for (int i = 0; i < N; i++)
        if (dims[i] == 0) return fail(SZ3HIP_EINVAL, "dimension %d has extent 0", i);
    return 0;
}
// ... and behind them: the input view's strides, device and alignment; the output (where the call has one) as a request's view of the whole
// array at level 0, for the request's own view checks
struct DeviceView {
    uint64_t str[4] = {0, 0, 0, 0};
    int dev = 0;
    sz3hip_tile_req q;
};
int device_view(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides_in, void *d_out, const int64_t *strides_out, DeviceView *v) {
    int rc;
    if ((rc = szi_dev_view_strides(N, dims, strides_in, v->str)) || (rc = szi_dev_pointer(d_in, &v->dev))) return rc;
    if ((uintptr_t)d_in % tsize(dataType)) return fail(SZ3HIP_EINVAL, "an array is not aligned to its element size (%zu bytes)", tsize(dataType));
    memset(&v->q, 0, sizeof(v->q));
    for (int i = 0; i < N; i++) {
        v->q.box.ext[i] = dims[i];
        v->q.strides[i] = strides_out ? strides_out[i] : 0;
    }
    v->q.d_out = d_out;
    return 0;
}
}  // namespace

extern "C" int sz3hip_stream_tiles(sz3hip_stream *h, int level, const sz3hip_box *boxes, uint32_t n, void *const *d_outs, void *stream) {
    if (!h) return fail(SZ3HIP_EINVAL, "sz3hip_stream_tiles: no handle");
    if (level < 0 || level > 30) return fail(SZ3HIP_EINVAL, "tile level %d is outside 0 .. 30", level);
    int rc = szi_boxes_args("sz3hip_stream_tiles", boxes, n, d_outs, "d_outs");
    if (rc) return rc;
    Submit sub(h, stream);
    hipStream_t s = sub.s;
    if (!h->fast) {  // strided gathers out of the resident array (nothing of it is written after open: no ordering between requests is needed)
        if ((rc = boxes_on_grid(h, level, boxes, n)) || (rc = szi_boxes_outputs_check(h->N, boxes, n, d_outs, tsize(h->dtype)))) return rc;
        HIPCHK(hipSetDevice(h->device));
        uint64_t str[4] = {0, 0, 0, 0}, run = 1;
        for (int i = h->N - 1; i >= 0; i--) {
            str[i] = run;
            run *= h->dims[i];
        }
        for (uint32_t b = 0; b < n; b++) {
            szk_view gv;
            memset(&gv, 0, sizeof(gv));
            uint64_t corner = 0;
            for (int q = 0; q < 4; q++) {
                const int i = q - (4 - h->N);
                gv.dims[q] = i >= 0 ? boxes[b].ext[i] : 1;
                gv.str[q] = i >= 0 && boxes[b].ext[i] > 1 ? (int64_t)(str[i] << level) : 0;
                if (i >= 0) corner += (boxes[b].lo[i] << level) * str[i];
            }
            if (szk_launch_gather(h->dtype, 0, (const char *)h->d_full + corner * tsize(h->dtype), &gv, d_outs[b], nullptr, s)) return fail(SZ3HIP_EHIP, "gather kernel failed");
        }
        h->launches_last = n;
        h->chain_last = h->levels_last = 0;
        h->chain_points_last = sz3hip_debug_get_chain_points();
        h->requests++;
        return 0;
    }
    // every box and every output before anything is launched or written (boxes_prepare of sz3hip_api.cpp, on the handle's arrays)
    const szk_interp_params &ip = h->codes.ip;
    sub.n = n;
    sub.d_outs = d_outs;
    if ((rc = szi_boxes_geometry(ip.N, ip.dims, ip.interp_id, ip.direction, ip.anchor_stride, level, boxes, n, sub.gs, &sub.elems))) return rc;
    if ((rc = szi_boxes_outputs_check(ip.N, boxes, n, d_outs, tsize(h->dtype))) || (rc = submit_begin(sub, nullptr, sub.elems))) return rc;
    return submit_launch(sub, "reconstruction", nullptr, nullptr, nullptr);
}

extern "C" int sz3hip_request_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n, sz3hip_request_plan *out) {
    if (!conf || !out) return fail(SZ3HIP_EINVAL, "sz3hip_request_plan_for: NULL argument (%s)", !conf ? "conf" : "out");
    int rc = dtype_check(dataType);
    if (rc || (rc = request_args("sz3hip_request_plan_for", reqs, n))) return rc;
    std::vector<szk_region_geom> gs;
    std::vector<ReqView> vs;
    memset(out, 0, sizeof(*out));
    if ((rc = szi_request_geometry_conf(conf, reqs, n, gs, &out->scratch_elems)) || (rc = request_views(conf->N, reqs, n, tsize(dataType), vs))) return rc;
    plan_prefix(out, reqs, n, gs);
    return 0;
}

extern "C" int sz3hip_stream_request(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, void *stream) {
    if (!h) return fail(SZ3HIP_EINVAL, "sz3hip_stream_request: no handle");
    int rc = request_args("sz3hip_stream_request", reqs, n);
    if (rc) return rc;
    Submit sub(h, stream);
    std::vector<ReqView> vs;
    if ((rc = submit_boxes(sub, reqs, n)) || (rc = request_views(sub.N, reqs, n, tsize(h->dtype), vs)) || (rc = submit_begin(sub, nullptr, sub.elems))) return rc;
    return submit_launch(sub, "reconstruction", nullptr, &vs, nullptr);
}

// ---- numbers about boxes, no output --------------------------------------------------------------------------------------
namespace {
// the arguments before any geometry; the boxes as a request's (no view), so that the request's checks and geometry serve as they are
int reduce_args(const char *who, const sz3hip_reduce_req *reqs, uint32_t n, const void *third, const char *third_name, std::vector<sz3hip_tile_req> &tr) {
    int rc = szi_boxes_args(who, reqs, n, third, third_name);
    if (rc) return rc;
    tr.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        if (reqs[i].reserved) return fail(SZ3HIP_EINVAL, "box %u: the reserved word is %u, not 0", i, reqs[i].reserved);
        memset(&tr[i], 0, sizeof(tr[i]));
        tr[i].level = reqs[i].level;
        tr[i].box = reqs[i].box;
    }
    return 0;
}
int reduce_opts(const sz3hip_reduce_opts *opts, const uint64_t *d_hist, bool need_hist, szk_reduce_hist *hh) {
    memset(hh, 0, sizeof(*hh));
    if (!opts) return 0;
    if (opts->reserved) return fail(SZ3HIP_EINVAL, "the options' reserved word is %u, not 0", opts->reserved);
    if (opts->nbins > SZ3HIP_MAX_BINS) return fail(SZ3HIP_EINVAL, "the histogram has %u bins: at most %d are supported", opts->nbins, SZ3HIP_MAX_BINS);
    if (opts->nbins == 0) return 0;
    if (!(fabs(opts->lo) < INFINITY) || !(fabs(opts->hi) < INFINITY)) return fail(SZ3HIP_EINVAL, "the histogram's range [%g, %g) is not finite", opts->lo, opts->hi);
    if (!(opts->hi > opts->lo)) return fail(SZ3HIP_EINVAL, "the histogram's range [%g, %g) is empty: hi must be above lo", opts->lo, opts->hi);
    if (need_hist && !d_hist) return fail(SZ3HIP_EINVAL, "the histogram's array (d_hist) is NULL with %u bins", opts->nbins);
    hh->nbins = opts->nbins;
    hh->lo = opts->lo;
    hh->hi = opts->hi;
    hh->scale = (double)opts->nbins / (opts->hi - opts->lo);
    return 0;
}
// the partial records lie behind the level buffers, on an 8-byte boundary: where they start and what the scratch holds then, in elements
uint64_t reduce_part_base(uint64_t elems, size_t tsz) { return tsz == 4 ? (elems + 1) & ~1ull : elems; }
uint64_t reduce_scratch_elems(uint64_t elems, uint64_t partials, size_t tsz) { return reduce_part_base(elems, tsz) + partials * (sizeof(szk_reduce_part) / tsz); }
// box i's first partial record (the request's order), the records' number
uint64_t reduce_partials(const sz3hip_tile_req *tr, uint32_t n, int N, std::vector<uint64_t> *first) {
    uint64_t at = 0;
    if (first) first->resize(n);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t total = 1;
        for (int j = 0; j < N; j++) total *= tr[i].box.ext[j];
        if (first) (*first)[i] = at;
        at += szk_reduce_chunks(total);
    }
    return at;
}

// sz3hip_reduce_device's workspace, one per device: the partial records (grown when a view needs more) and the event that orders a call
// behind the previous one on another stream
struct ReduceWs {
    std::mutex mu;
    szk_reduce_part *d_partials = nullptr;
    uint64_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    hipStream_t last = nullptr;
};
std::mutex g_reduce_mu;
std::map<int, std::unique_ptr<ReduceWs>> g_reduce_ws;
ReduceWs *reduce_ws(int device) {
    std::lock_guard<std::mutex> l(g_reduce_mu);
    auto &p = g_reduce_ws[device];
    if (!p) p.reset(new ReduceWs);
    return p.get();
}
// room for `parts` records, and the call on s ordered behind the previous one (w->mu is held)
int reduce_ws_reserve(ReduceWs *w, uint64_t parts, hipStream_t s) {
    if (!w->ev) HIPCHK(hipEventCreateWithFlags(&w->ev, hipEventDisableTiming));
    if (parts > w->cap) {
        if (w->d_partials) {
            HIPCHK(hipDeviceSynchronize());  // (an earlier call's kernels may still use them)
            (void)hipFree(w->d_partials);
        }
        w->d_partials = nullptr;
        w->cap = 0;
        w->pending = false;
        const uint64_t cap = std::max<uint64_t>(parts, 4096);
        HIPCHK(hipMalloc((void **)&w->d_partials, cap * sizeof(szk_reduce_part)));
        w->cap = cap;
    }
    if (w->pending && s != w->last) HIPCHK(hipStreamWaitEvent(s, w->ev, 0));
    return 0;
}
}  // namespace

extern "C" int sz3hip_reduce_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_reduce_req *reqs, uint32_t n, const sz3hip_reduce_opts *opts,
                                      sz3hip_reduce_plan *out) {
    if (!conf || !out) return fail(SZ3HIP_EINVAL, "sz3hip_reduce_plan_for: NULL argument (%s)", !conf ? "conf" : "out");
    int rc = dtype_check(dataType);
    std::vector<sz3hip_tile_req> tr;
    szk_reduce_hist hh;
    if (rc || (rc = reduce_args("sz3hip_reduce_plan_for", reqs, n, reqs, "reqs", tr)) || (rc = reduce_opts(opts, nullptr, false, &hh))) return rc;
    std::vector<szk_region_geom> gs;
    uint64_t elems = 0;
    memset(out, 0, sizeof(*out));
    if ((rc = szi_request_geometry_conf(conf, tr.data(), n, gs, &elems))) return rc;
    plan_prefix(out, reqs, n, gs);
    out->partials = reduce_partials(tr.data(), n, conf->N, nullptr);
    out->scratch_elems = reduce_scratch_elems(elems, out->partials, tsize(dataType));
    out->hist_words = (uint64_t)n * (hh.nbins ? hh.nbins + 2 : 0);
    return 0;
}

extern "C" int sz3hip_stream_reduce(sz3hip_stream *h, const sz3hip_reduce_req *reqs, uint32_t n, const sz3hip_reduce_opts *opts, sz3hip_box_stats *d_stats,
                                    uint64_t *d_hist, void *stream) {
    if (!d_stats) return fail(SZ3HIP_EINVAL, "sz3hip_stream_reduce: NULL argument (d_stats)");
    if (!h) return fail(SZ3HIP_EINVAL, "sz3hip_stream_reduce: no handle");
    std::vector<sz3hip_tile_req> tr;
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    int rc = reduce_args("sz3hip_stream_reduce", reqs, n, d_stats, "d_stats", tr);
    if (rc || (rc = reduce_opts(opts, d_hist, true, &sink.hist))) return rc;
    Submit sub(h, stream);
    std::vector<uint64_t> first;
    if ((rc = submit_boxes(sub, tr.data(), n))) return rc;
    const uint64_t partials = reduce_partials(tr.data(), n, sub.N, &first);
    if (partials >= (1ull << 40)) return fail(SZ3HIP_EINVAL, "the boxes hold too many points for one reducing request");
    if ((rc = submit_begin(sub, &sink, reduce_scratch_elems(sub.elems, partials, tsize(h->dtype))))) return rc;
    sink.partials = reinterpret_cast<szk_reduce_part *>((char *)h->d_region + reduce_part_base(sub.elems, tsize(h->dtype)) * tsize(h->dtype));
    sink.d_stats = d_stats;
    sink.d_hist = sink.hist.nbins ? d_hist : nullptr;
    if (sink.hist.nbins) HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)n * (sink.hist.nbins + 2) * 8, sub.s));
    return submit_launch(sub, "reduction", &sink, nullptr, first.data());
}

extern "C" int sz3hip_reduce_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides, const sz3hip_reduce_opts *opts,
                                    sz3hip_box_stats *d_stats, uint64_t *d_hist, void *stream) {
    int rc = device_dims(dataType, N, dims);
    if (rc) return rc;
    if (!d_stats) return fail(SZ3HIP_EINVAL, "sz3hip_reduce_device: NULL argument (d_stats)");
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    if ((rc = reduce_opts(opts, d_hist, true, &sink.hist))) return rc;
    DeviceView v;
    if ((rc = device_view(dataType, N, dims, d_in, strides, nullptr, nullptr, &v))) return rc;
    szk_region_gather_strided_box rec;
    szi_view_record(N, dims, v.str, 0, nullptr, nullptr, &rec);  // (dst word 0: the view's first partial record)
    const uint64_t partials = szk_reduce_chunks(rec.total);
    if (partials >= (1ull << 40)) return fail(SZ3HIP_EINVAL, "the view holds too many points for one reduction");
    hipStream_t s = (hipStream_t)stream;
    DeviceScope scope;
    HIPCHK(hipSetDevice(v.dev));
    ReduceWs *w = reduce_ws(v.dev);
    std::lock_guard<std::mutex> lock(w->mu);
    if ((rc = reduce_ws_reserve(w, partials, s))) return rc;
    sink.partials = w->d_partials;
    sink.d_stats = d_stats;
    sink.d_hist = sink.hist.nbins ? d_hist : nullptr;
    if (sink.hist.nbins) HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)(sink.hist.nbins + 2) * 8, s));
    int lr = szk_launch_region_reduce(dataType, d_in, nullptr, &rec, 1, rec.total, &sink, s);
    if (!lr) lr = szk_launch_region_reduce_final(dataType, d_in, nullptr, &rec, 1, &sink, s);
    HIPCHK(hipEventRecord(w->ev, s));
    w->pending = true;
    w->last = s;
    if (lr) return fail(SZ3HIP_EHIP, "the reduction could not be launched (%d)", lr);
    return 0;
}

// ---- the points of boxes whose values lie in a range -----------------------------------------------------------------------
namespace {
int select_opts(const sz3hip_select_opts *opts, szk_select_opts *so) {
    memset(so, 0, sizeof(*so));
    if (!opts) return fail(SZ3HIP_EINVAL, "NULL argument (opts): a selection needs its range");
    if (opts->reserved) return fail(SZ3HIP_EINVAL, "the options' reserved word is %u, not 0", opts->reserved);
    if (opts->flags & ~(SZ3HIP_SELECT_INVERT | SZ3HIP_SELECT_NAN)) return fail(SZ3HIP_EINVAL, "the options' flags (0x%x) hold bits beyond SZ3HIP_SELECT_INVERT | SZ3HIP_SELECT_NAN", opts->flags);
    if (opts->lo != opts->lo || opts->hi != opts->hi) return fail(SZ3HIP_EINVAL, "the range's %s is NaN", opts->lo != opts->lo ? "lo" : "hi");
    so->lo = opts->lo;
    so->hi = opts->hi;
    so->flags = opts->flags;
    return 0;
}
// one output's rules (prefix: "box <i>: " or nothing)
int select_out(const char *prefix, const uint64_t *d_index, const void *d_value, uint64_t capacity, size_t tsz) {
    if (capacity > 0 && !d_index) return fail(SZ3HIP_EINVAL, "%sd_index is NULL with a capacity of %llu", prefix, (unsigned long long)capacity);
    if (capacity == 0 && d_value) return fail(SZ3HIP_EINVAL, "%sd_value is given with a capacity of 0", prefix);
    if (capacity > (1ull << 56)) return fail(SZ3HIP_EINVAL, "%sthe capacity (%llu) is too large", prefix, (unsigned long long)capacity);
    if ((uintptr_t)d_index % 8 || (uintptr_t)d_value % tsz) return fail(SZ3HIP_EINVAL, "%san output is not aligned to its element size", prefix);
    return 0;
}
// the arguments before any geometry: the boxes as a request's (no view), the outputs' rules, no two outputs of one kind meeting
int select_args(const char *who, const sz3hip_select_req *reqs, uint32_t n, size_t tsz, std::vector<sz3hip_tile_req> &tr) {
    int rc = szi_boxes_args(who, reqs, n, reqs, "reqs");
    if (rc) return rc;
    tr.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        char prefix[32];
        snprintf(prefix, sizeof(prefix), "box %u: ", i);
        if (reqs[i].reserved) return fail(SZ3HIP_EINVAL, "box %u: the reserved word is %u, not 0", i, reqs[i].reserved);
        if ((rc = select_out(prefix, reqs[i].d_index, reqs[i].d_value, reqs[i].capacity, tsz))) return rc;
        memset(&tr[i], 0, sizeof(tr[i]));
        tr[i].level = reqs[i].level;
        tr[i].box = reqs[i].box;
    }
    for (uint32_t i = 1; i < n; i++)
        for (uint32_t k = 0; k < i && reqs[i].capacity; k++) {
            if (!reqs[k].capacity) continue;
            const uintptr_t ai = (uintptr_t)reqs[i].d_index, ak = (uintptr_t)reqs[k].d_index, vi = (uintptr_t)reqs[i].d_value, vk = (uintptr_t)reqs[k].d_value;
            const bool index_meet = ai < ak + reqs[k].capacity * 8 && ak < ai + reqs[i].capacity * 8;
            const bool value_meet = vi && vk && vi < vk + reqs[k].capacity * tsz && vk < vi + reqs[i].capacity * tsz;
            if (index_meet || value_meet) return fail(SZ3HIP_EINVAL, "box %u: the output overlaps box %u's (%s)", i, k, index_meet ? "d_index" : "d_value");
        }
    return 0;
}
// the chunk records (one 64-bit word each) lie behind the level buffers, on an 8-byte boundary, as a reduce's partials do
uint64_t select_scratch_elems(uint64_t elems, uint64_t partials, size_t tsz) { return reduce_part_base(elems, tsz) + partials * (8 / tsz); }
}  // namespace

extern "C" int sz3hip_select_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_select_req *reqs, uint32_t n, const sz3hip_select_opts *opts,
                                      sz3hip_select_plan *out) {
    if (!conf || !out) return fail(SZ3HIP_EINVAL, "sz3hip_select_plan_for: NULL argument (%s)", !conf ? "conf" : "out");
    int rc = dtype_check(dataType);
    std::vector<sz3hip_tile_req> tr;
    szk_select_opts so;
    if (rc || (rc = select_args("sz3hip_select_plan_for", reqs, n, tsize(dataType), tr)) || (rc = select_opts(opts, &so))) return rc;
    std::vector<szk_region_geom> gs;
    uint64_t elems = 0;
    memset(out, 0, sizeof(*out));
    if ((rc = szi_request_geometry_conf(conf, tr.data(), n, gs, &elems))) return rc;
    plan_prefix(out, reqs, n, gs);
    out->partials = reduce_partials(tr.data(), n, conf->N, nullptr);
    out->scratch_elems = select_scratch_elems(elems, out->partials, tsize(dataType));
    return 0;
}

extern "C" int sz3hip_stream_select(sz3hip_stream *h, const sz3hip_select_req *reqs, uint32_t n, const sz3hip_select_opts *opts, sz3hip_select_head *d_heads,
                                    void *stream) {
    if (!d_heads) return fail(SZ3HIP_EINVAL, "sz3hip_stream_select: NULL argument (d_heads)");
    if (!h) return fail(SZ3HIP_EINVAL, "sz3hip_stream_select: no handle");
    std::vector<sz3hip_tile_req> tr;
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    sink.kind = SZK_SINK_SELECT;
    int rc = select_args("sz3hip_stream_select", reqs, n, tsize(h->dtype), tr);
    if (rc || (rc = select_opts(opts, &sink.sel))) return rc;
    Submit sub(h, stream);
    std::vector<uint64_t> first;
    if ((rc = submit_boxes(sub, tr.data(), n))) return rc;
    const uint64_t partials = reduce_partials(tr.data(), n, sub.N, &first);
    if (partials >= (1ull << 40)) return fail(SZ3HIP_EINVAL, "the boxes hold too many points for one selecting request");
    std::vector<uint64_t> outs((size_t)n * SZK_SELECT_OUT_WORDS);  // (every box's d_index, d_value and capacity: they ride behind the final's records)
    for (uint32_t i = 0; i < n; i++) {
        outs[i * SZK_SELECT_OUT_WORDS] = (uint64_t)(uintptr_t)reqs[i].d_index;
        outs[i * SZK_SELECT_OUT_WORDS + 1] = (uint64_t)(uintptr_t)reqs[i].d_value;
        outs[i * SZK_SELECT_OUT_WORDS + 2] = reqs[i].capacity;
    }
    if ((rc = submit_begin(sub, &sink, select_scratch_elems(sub.elems, partials, tsize(h->dtype))))) return rc;
    sink.sel_counts = reinterpret_cast<uint64_t *>((char *)h->d_region + reduce_part_base(sub.elems, tsize(h->dtype)) * tsize(h->dtype));
    sink.sel_heads = d_heads;
    sink.sel_outs = outs.data();
    return submit_launch(sub, "selection", &sink, nullptr, first.data());
}

extern "C" int sz3hip_select_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides, const sz3hip_select_opts *opts,
                                    uint64_t *d_index, void *d_value, uint64_t capacity, sz3hip_select_head *d_head, void *stream) {
    int rc = device_dims(dataType, N, dims);
    if (rc) return rc;
    if (!d_head) return fail(SZ3HIP_EINVAL, "sz3hip_select_device: NULL argument (d_head)");
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    sink.kind = SZK_SINK_SELECT;
    if ((rc = select_opts(opts, &sink.sel)) || (rc = select_out("", d_index, d_value, capacity, tsize(dataType)))) return rc;
    DeviceView v;
    if ((rc = device_view(dataType, N, dims, d_in, strides, nullptr, nullptr, &v))) return rc;
    szk_region_gather_strided_box rec;
    szi_view_record(N, dims, v.str, 0, nullptr, nullptr, &rec);  // (dst word 0: the view's first chunk record)
    const uint64_t partials = szk_reduce_chunks(rec.total);
    if (partials >= (1ull << 40)) return fail(SZ3HIP_EINVAL, "the view holds too many points for one selection");
    const uint64_t parts = (partials * 8 + sizeof(szk_reduce_part) - 1) / sizeof(szk_reduce_part);  // (the workspace counts reduce records)
    hipStream_t s = (hipStream_t)stream;
    DeviceScope scope;
    HIPCHK(hipSetDevice(v.dev));
    ReduceWs *w = reduce_ws(v.dev);
    std::lock_guard<std::mutex> lock(w->mu);
    if ((rc = reduce_ws_reserve(w, parts, s))) return rc;
    const uint64_t out3[SZK_SELECT_OUT_WORDS] = {(uint64_t)(uintptr_t)d_index, (uint64_t)(uintptr_t)d_value, capacity};
    sink.sel_counts = reinterpret_cast<uint64_t *>(w->d_partials);
    sink.sel_heads = d_head;
    sink.sel_outs = out3;
    int lr = szk_launch_region_select_count(dataType, d_in, nullptr, &rec, 1, rec.total, &sink, s);
    if (!lr) lr = szk_launch_region_select_place(dataType, d_in, nullptr, &rec, 1, rec.total, &sink, s);
    HIPCHK(hipEventRecord(w->ev, s));
    w->pending = true;
    w->last = s;
    if (lr) return fail(SZ3HIP_EHIP, "the selection could not be launched (%d)", lr);
    return 0;
}

// ---- texels out of a request: boxes mapped to u8 / u16 / f16 / f32 / RGBA8 --------------------------------------------------
namespace {
int map_opts_check(const sz3hip_map_opts *opts, szk_map_opts *mo) {
    memset(mo, 0, sizeof(*mo));
    if (!opts) return fail(SZ3HIP_EINVAL, "NULL argument (opts): a mapping needs its output type");
    if (opts->out_type < SZ3HIP_MAP_U8 || opts->out_type > SZ3HIP_MAP_LUT32)
        return fail(SZ3HIP_EINVAL, "the options' out_type (%u) is not one of SZ3HIP_MAP_U8 .. SZ3HIP_MAP_LUT32 (1 .. 5)", opts->out_type);
    if (opts->flags) return fail(SZ3HIP_EINVAL, "the options' flags are 0x%x, not 0", opts->flags);
    if (opts->reserved) return fail(SZ3HIP_EINVAL, "the options' reserved word is %llu, not 0", (unsigned long long)opts->reserved);
    const uint32_t t = opts->out_type;
    if (t == SZ3HIP_MAP_F16 || t == SZ3HIP_MAP_F32) {
        if (opts->lo != 0.0 || opts->hi != 0.0 || opts->nan_code || opts->lut_n || opts->d_lut)  // (a NaN is not 0 either)
            return fail(SZ3HIP_EINVAL, "the options hold a window, a nan_code or a table: SZ3HIP_MAP_F16 / SZ3HIP_MAP_F32 take none (lo, hi, nan_code, lut_n 0 and d_lut NULL)");
        mo->out_type = t;
        return 0;
    }
    if (!(fabs(opts->lo) < INFINITY) || !(fabs(opts->hi) < INFINITY)) return fail(SZ3HIP_EINVAL, "the window [%g, %g) is not finite", opts->lo, opts->hi);
    if (!(opts->hi > opts->lo)) return fail(SZ3HIP_EINVAL, "the window [%g, %g) is empty: hi must be above lo", opts->lo, opts->hi);
    if (!(fabs(opts->hi - opts->lo) < INFINITY)) return fail(SZ3HIP_EINVAL, "the window [%g, %g) is too wide: hi - lo is not finite", opts->lo, opts->hi);
    uint32_t M;
    if (t == SZ3HIP_MAP_LUT32) {
        if (opts->lut_n < 2 || opts->lut_n > SZ3HIP_MAX_LUT) return fail(SZ3HIP_EINVAL, "the table has %u entries: 2 .. %d are supported", opts->lut_n, SZ3HIP_MAX_LUT);
        if (!opts->d_lut) return fail(SZ3HIP_EINVAL, "the table (d_lut) is NULL");
        if ((uintptr_t)opts->d_lut % 4) return fail(SZ3HIP_EINVAL, "the table (d_lut) is not aligned to its 4-byte entries");
        M = opts->lut_n - 1;
    } else {
        if (opts->lut_n || opts->d_lut) return fail(SZ3HIP_EINVAL, "the options hold a table: only SZ3HIP_MAP_LUT32 takes one (lut_n 0 and d_lut NULL)");
        M = t == SZ3HIP_MAP_U8 ? 255u : 65535u;
        if (opts->nan_code > M) return fail(SZ3HIP_EINVAL, "nan_code (%u) is beyond the output's range (0 .. %u)", opts->nan_code, M);
    }
    mo->lo = opts->lo;
    mo->hi = opts->hi;
    mo->scale = (double)(M + 1) / (opts->hi - opts->lo);
    mo->out_type = t;
    mo->M = M;
    mo->nan_code = opts->nan_code;
    mo->lut_n = opts->lut_n;
    mo->d_lut = static_cast<const uint32_t *>(opts->d_lut);
    return 0;
}
// every output aligned to the output element; the views and their overlaps by the request's rule with that element's size
int map_views(int N, const sz3hip_tile_req *reqs, uint32_t n, size_t osz, std::vector<ReqView> &vs) {
    for (uint32_t i = 0; i < n; i++)
        if ((uintptr_t)reqs[i].d_out % osz) return fail(SZ3HIP_EINVAL, "box %u: the output is not aligned to its element size (%zu bytes)", i, osz);
    return request_views(N, reqs, n, osz, vs);
}
// the sink of a mapping call: the form (packed unless the development switch asks for a thread per point) and the lanes of the largest box
void map_sink(szk_region_sink *sink, int N, const sz3hip_tile_req *reqs, uint32_t n, const std::vector<ReqView> &vs) {
    sink->kind = SZK_SINK_MAP;
    sink->map_packed = !(szk_dbg_flags2 & SZ3HIP_DBG2_MAP_PLAIN_STORES);
    const uint32_t ob = szk_map_out_bytes(sink->map.out_type);
    sink->map_threads = 1;
    for (uint32_t i = 0; i < n; i++) {
        uint64_t total = 1;
        for (int j = 0; j < N; j++) total *= reqs[i].box.ext[j];
        sink->map_threads = std::max(sink->map_threads, szk_map_threads(total, reqs[i].box.ext[N - 1], vs[i].str[N - 1], ob, sink->map_packed));
    }
}
}  // namespace

extern "C" int sz3hip_map_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_map_opts *opts,
                                   sz3hip_map_plan *out) {
    if (!conf || !out) return fail(SZ3HIP_EINVAL, "sz3hip_map_plan_for: NULL argument (%s)", !conf ? "conf" : "out");
    int rc = dtype_check(dataType);
    szk_map_opts mo;
    if (rc || (rc = request_args("sz3hip_map_plan_for", reqs, n)) || (rc = map_opts_check(opts, &mo))) return rc;
    std::vector<szk_region_geom> gs;
    std::vector<ReqView> vs;
    memset(out, 0, sizeof(*out));
    const size_t osz = szk_map_out_bytes(mo.out_type);
    if ((rc = szi_request_geometry_conf(conf, reqs, n, gs, &out->scratch_elems)) || (rc = map_views(conf->N, reqs, n, osz, vs))) return rc;
    plan_prefix(out, reqs, n, gs);
    out->out_elem_bytes = osz;
    return 0;
}

extern "C" int sz3hip_stream_map(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_map_opts *opts, void *stream) {
    if (!h) return fail(SZ3HIP_EINVAL, "sz3hip_stream_map: no handle");
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    int rc = request_args("sz3hip_stream_map", reqs, n);
    if (rc || (rc = map_opts_check(opts, &sink.map))) return rc;
    const size_t osz = szk_map_out_bytes(sink.map.out_type);
    Submit sub(h, stream);
    std::vector<ReqView> vs;
    if ((rc = submit_boxes(sub, reqs, n)) || (rc = map_views(sub.N, reqs, n, osz, vs))) return rc;
    map_sink(&sink, sub.N, reqs, n, vs);
    if ((rc = submit_begin(sub, &sink, sub.elems))) return rc;
    return submit_launch(sub, "mapping", &sink, &vs, nullptr);
}

extern "C" int sz3hip_map_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides_in, const sz3hip_map_opts *opts,
                                 void *d_out, const int64_t *strides_out, void *stream) {
    int rc = device_dims(dataType, N, dims);
    if (rc) return rc;
    if (!d_out) return fail(SZ3HIP_EINVAL, "sz3hip_map_device: NULL argument (d_out)");
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    if ((rc = map_opts_check(opts, &sink.map))) return rc;
    DeviceView v;
    if ((rc = device_view(dataType, N, dims, d_in, strides_in, d_out, strides_out, &v))) return rc;
    std::vector<ReqView> vs;
    if ((rc = map_views(N, &v.q, 1, szk_map_out_bytes(sink.map.out_type), vs))) return rc;
    map_sink(&sink, N, &v.q, 1, vs);
    szk_region_gather_strided_box rec;
    szi_view_record(N, dims, v.str, 0, d_out, vs[0].str, &rec);
    hipStream_t s = (hipStream_t)stream;
    DeviceScope scope;
    HIPCHK(hipSetDevice(v.dev));
    if (szk_launch_region_map(dataType, d_in, nullptr, &rec, 1, &sink, s)) return fail(SZ3HIP_EHIP, "the mapping could not be launched");
    return 0;
}

// ---- boxes sampled at fractional positions: nearest and linear ---------------------------------------------------------------
namespace {
int sample_opts_check(const sz3hip_sample_opts *opts, szk_sample_opts *so) {
    memset(so, 0, sizeof(*so));
    if (!opts) return fail(SZ3HIP_EINVAL, "NULL argument (opts): a sampling needs its filter");
    if (opts->filter > SZ3HIP_SAMPLE_LINEAR) return fail(SZ3HIP_EINVAL, "the options' filter (%u) is not SZ3HIP_SAMPLE_NEAREST or SZ3HIP_SAMPLE_LINEAR (0, 1)", opts->filter);
    if (opts->coord_type > SZ3HIP_DOUBLE) return fail(SZ3HIP_EINVAL, "the options' coord_type (%u) is not SZ3HIP_FLOAT or SZ3HIP_DOUBLE (0, 1)", opts->coord_type);
    if (opts->flags & ~SZ3HIP_SAMPLE_CLAMP) return fail(SZ3HIP_EINVAL, "the options' flags (0x%x) hold bits beyond SZ3HIP_SAMPLE_CLAMP", opts->flags);
    if (opts->reserved) return fail(SZ3HIP_EINVAL, "the options' reserved word is %u, not 0", opts->reserved);
    so->filter = opts->filter;
    so->coord_type = opts->coord_type;
    so->flags = opts->flags;
    so->fill = opts->fill;
    return 0;
}
// one box's queries by themselves, before any geometry (prefix: "box <i>: " or nothing); csz: a coordinate's bytes
int sample_query_args(const char *prefix, const sz3hip_sample_req &q, size_t tsz, size_t csz) {
    if (!q.d_out) return fail(SZ3HIP_EINVAL, "%sthe output array is NULL", prefix);
    if ((uintptr_t)q.d_out % tsz) return fail(SZ3HIP_EINVAL, "%sthe output is not aligned to its element size (%zu bytes)", prefix, tsz);
    if (q.n_points < 1 || q.n_points > (1ull << 31))
        return fail(SZ3HIP_EINVAL, "%sn_points is %llu: 1 .. 2^31 queries are supported", prefix, (unsigned long long)q.n_points);
    if (q.d_coords) {
        if ((uintptr_t)q.d_coords % csz) return fail(SZ3HIP_EINVAL, "%sd_coords is not aligned to its coordinate size (%zu bytes)", prefix, csz);
        bool zero = !(q.counts[0] | q.counts[1] | q.counts[2]);
        for (int j = 0; j < 4; j++) zero = zero && q.origin[j] == 0.0 && q.steps[0][j] == 0.0 && q.steps[1][j] == 0.0 && q.steps[2][j] == 0.0;
        if (!zero) return fail(SZ3HIP_EINVAL, "%sd_coords is given with a lattice: counts, origin and steps must be 0 in the points form", prefix);
        return 0;
    }
    uint64_t product = 1;
    for (int a = 0; a < 3; a++) {
        if (q.counts[a] == 0) return fail(SZ3HIP_EINVAL, "%sthe lattice's count of axis %d is 0", prefix, a);
        product = q.counts[a] > (1ull << 31) || product > (1ull << 31) ? ~0ull : product * q.counts[a];  // (~0: beyond any n_points; nothing wraps)
    }
    if (product != q.n_points)
        return fail(SZ3HIP_EINVAL, "%sthe lattice's counts (%llu x %llu x %llu) do not multiply to n_points (%llu)", prefix, (unsigned long long)q.counts[0],
                    (unsigned long long)q.counts[1], (unsigned long long)q.counts[2], (unsigned long long)q.n_points);
    return 0;
}
// ... and what needs the dimension count: the lattice's N used entries are finite
int sample_query_lattice(const char *prefix, const sz3hip_sample_req &q, int N) {
    if (q.d_coords) return 0;
    for (int j = 0; j < N; j++) {
        if (!(fabs(q.origin[j]) < INFINITY)) return fail(SZ3HIP_EINVAL, "%sthe lattice's origin[%d] is not finite", prefix, j);
        for (int a = 0; a < 3; a++)
            if (!(fabs(q.steps[a][j]) < INFINITY)) return fail(SZ3HIP_EINVAL, "%sthe lattice's steps[%d][%d] is not finite", prefix, a, j);
    }
    return 0;
}
// the arguments before any geometry: the boxes as a request's (no view), every box's queries, no two outputs meeting
int sample_args(const char *who, const sz3hip_sample_req *reqs, uint32_t n, size_t tsz, size_t csz, std::vector<sz3hip_tile_req> &tr) {
    int rc = szi_boxes_args(who, reqs, n, reqs, "reqs");
    if (rc) return rc;
    tr.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        char prefix[32];
        snprintf(prefix, sizeof(prefix), "box %u: ", i);
        if (reqs[i].reserved) return fail(SZ3HIP_EINVAL, "box %u: the reserved word is %u, not 0", i, reqs[i].reserved);
        if ((rc = sample_query_args(prefix, reqs[i], tsz, csz))) return rc;
        memset(&tr[i], 0, sizeof(tr[i]));
        tr[i].level = reqs[i].level;
        tr[i].box = reqs[i].box;
    }
    for (uint32_t i = 1; i < n; i++)
        for (uint32_t k = 0; k < i; k++) {
            const uintptr_t a = (uintptr_t)reqs[i].d_out, b = (uintptr_t)reqs[k].d_out;
            if (a - b < reqs[k].n_points * tsz || b - a < reqs[i].n_points * tsz) return fail(SZ3HIP_EINVAL, "box %u: the output overlaps box %u's", i, k);
        }
    return 0;
}
int sample_lattices(const sz3hip_sample_req *reqs, uint32_t n, int N) {
    for (uint32_t i = 0; i < n; i++) {
        char prefix[32];
        snprintf(prefix, sizeof(prefix), "box %u: ", i);
        const int rc = sample_query_lattice(prefix, reqs[i], N);
        if (rc) return rc;
    }
    return 0;
}
// a box's queries as the kernel reads them: origin and steps in the last N of four places
void sample_query_words(const sz3hip_sample_req &q, int N, szk_sample_query *w) {
    memset(w, 0, sizeof(*w));
    w->coords = q.d_coords;
    w->out = q.d_out;
    w->n_points = q.n_points;
    for (int a = 0; a < 3; a++) w->counts[a] = q.d_coords ? 1 : q.counts[a];
    for (int j = 0; j < N && !q.d_coords; j++) {
        w->origin[4 - N + j] = q.origin[j];
        for (int a = 0; a < 3; a++) w->steps[a][4 - N + j] = q.steps[a][j];
    }
}
}  // namespace

extern "C" int sz3hip_sample_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_sample_req *reqs, uint32_t n, const sz3hip_sample_opts *opts,
                                      sz3hip_sample_plan *out) {
    if (!conf || !out) return fail(SZ3HIP_EINVAL, "sz3hip_sample_plan_for: NULL argument (%s)", !conf ? "conf" : "out");
    int rc = dtype_check(dataType);
    std::vector<sz3hip_tile_req> tr;
    szk_sample_opts so;
    if (rc || (rc = sample_opts_check(opts, &so)) || (rc = sample_args("sz3hip_sample_plan_for", reqs, n, tsize(dataType), tsize((int)so.coord_type), tr))) return rc;
    std::vector<szk_region_geom> gs;
    memset(out, 0, sizeof(*out));
    if ((rc = szi_request_geometry_conf(conf, tr.data(), n, gs, &out->scratch_elems)) || (rc = sample_lattices(reqs, n, conf->N))) return rc;
    plan_prefix(out, reqs, n, gs);
    for (uint32_t i = 0; i < n; i++) out->queries += reqs[i].n_points;
    return 0;
}

extern "C" int sz3hip_stream_sample(sz3hip_stream *h, const sz3hip_sample_req *reqs, uint32_t n, const sz3hip_sample_opts *opts, void *stream) {
    if (!h) return fail(SZ3HIP_EINVAL, "sz3hip_stream_sample: no handle");
    std::vector<sz3hip_tile_req> tr;
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    sink.kind = SZK_SINK_SAMPLE;
    int rc = sample_opts_check(opts, &sink.smp);
    if (rc || (rc = sample_args("sz3hip_stream_sample", reqs, n, tsize(h->dtype), tsize((int)sink.smp.coord_type), tr))) return rc;
    Submit sub(h, stream);
    if ((rc = submit_boxes(sub, tr.data(), n)) || (rc = sample_lattices(reqs, n, sub.N))) return rc;
    std::vector<szk_sample_query> queries(n);
    sink.smp.N = (uint32_t)sub.N;
    sink.smp_threads = 1;
    for (uint32_t i = 0; i < n; i++) {
        sample_query_words(reqs[i], sub.N, &queries[i]);
        sink.smp_threads = std::max(sink.smp_threads, reqs[i].n_points);
    }
    sink.smp_queries = queries.data();
    if ((rc = submit_begin(sub, &sink, sub.elems))) return rc;
    return submit_launch(sub, "sampling", &sink, nullptr, nullptr);
}

extern "C" int sz3hip_sample_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides, const sz3hip_sample_opts *opts,
                                    const sz3hip_sample_req *query, void *stream) {
    int rc = device_dims(dataType, N, dims);
    if (rc) return rc;
    if (!query) return fail(SZ3HIP_EINVAL, "sz3hip_sample_device: NULL argument (query)");
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    sink.kind = SZK_SINK_SAMPLE;
    if ((rc = sample_opts_check(opts, &sink.smp))) return rc;
    bool zero = query->level == 0 && query->reserved == 0;
    for (int j = 0; j < 4; j++) zero = zero && query->box.lo[j] == 0 && query->box.ext[j] == 0;
    if (!zero) return fail(SZ3HIP_EINVAL, "the query's level, reserved word and box must be 0: the view is the box");
    if ((rc = sample_query_args("", *query, tsize(dataType), tsize((int)sink.smp.coord_type))) || (rc = sample_query_lattice("", *query, N))) return rc;
    DeviceView v;
    if ((rc = device_view(dataType, N, dims, d_in, strides, nullptr, nullptr, &v))) return rc;
    szk_region_gather_strided_box rec;
    szi_view_record(N, dims, v.str, 0, nullptr, nullptr, &rec);
    szk_sample_query q;
    sample_query_words(*query, N, &q);
    sink.smp.N = (uint32_t)N;
    sink.smp_threads = query->n_points;
    sink.smp_queries = &q;
    hipStream_t s = (hipStream_t)stream;
    DeviceScope scope;
    HIPCHK(hipSetDevice(v.dev));
    if (szk_launch_region_sample(dataType, d_in, nullptr, &rec, 1, &sink, s)) return fail(SZ3HIP_EHIP, "the sampling could not be launched");
    return 0;
}

// ---- boxes projected along an axis: min, max, sum, mean, arg, count -----------------------------------------------------------
namespace {
bool project_index_op(uint32_t op) { return op == SZ3HIP_PROJECT_ARGMIN || op == SZ3HIP_PROJECT_ARGMAX || op == SZ3HIP_PROJECT_COUNT; }
size_t project_out_bytes(const szk_project_opts &po) { return project_index_op(po.op) || po.out_type == 0 ? 4 : 8; }
int project_opts_check(const sz3hip_project_opts *opts, szk_project_opts *po) {
    memset(po, 0, sizeof(*po));
    if (!opts) return fail(SZ3HIP_EINVAL, "NULL argument (opts): a projection needs its op and axis");
    if (opts->op > SZ3HIP_PROJECT_COUNT) return fail(SZ3HIP_EINVAL, "the options' op (%u) is not one of SZ3HIP_PROJECT_MIN .. SZ3HIP_PROJECT_COUNT (0 .. 6)", opts->op);
    if (opts->out_type > SZ3HIP_DOUBLE) return fail(SZ3HIP_EINVAL, "the options' out_type (%u) is not SZ3HIP_FLOAT or SZ3HIP_DOUBLE (0, 1)", opts->out_type);
    if (project_index_op(opts->op) && opts->out_type)
        return fail(SZ3HIP_EINVAL, "the options' out_type is %u: an index op (ARGMIN, ARGMAX, COUNT) writes uint32_t and takes out_type 0", opts->out_type);
    if (opts->reserved) return fail(SZ3HIP_EINVAL, "the options' reserved word is %u, not 0", opts->reserved);
    po->op = opts->op;
    po->out_type = opts->out_type;
    po->fill = opts->fill;
    return 0;
}
// ... and what needs the dimension count: the axis, counted in a record's four places from here on
int project_axis(const sz3hip_project_opts *opts, int N, szk_project_opts *po) {
    if (opts->axis >= (uint32_t)N) return fail(SZ3HIP_EINVAL, "the options' axis (%u) is not one of the %d dimensions (0 .. %d)", opts->axis, N, N - 1);
    po->axis = opts->axis + (uint32_t)(4 - N);
    po->N = (uint32_t)N;
    return 0;
}
// the views of the collapsed boxes — the requests with extent 1 at the axis, by the mapping's rules with the output element's size osz;
// *threads: the largest box's output points; *rows: the axis is every box's fastest dimension that counts; *out_points (or NULL): their sum
int collapsed_views(int N, uint32_t axis, const sz3hip_tile_req *reqs, uint32_t n, size_t osz, std::vector<ReqView> &vs, uint64_t *threads, bool *rows,
                    uint64_t *out_points) {
    std::vector<sz3hip_tile_req> flat(reqs, reqs + n);
    for (uint32_t i = 0; i < n; i++) flat[i].box.ext[axis] = 1;
    const int rc = map_views(N, flat.data(), n, osz, vs);
    if (rc) return rc;
    *threads = 1;
    *rows = true;
    if (out_points) *out_points = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint64_t outs = 1;
        for (int j = 0; j < N; j++) outs *= flat[i].box.ext[j];
        *threads = std::max(*threads, outs);
        if (out_points) *out_points += outs;
        for (int j = (int)axis + 1; j < N; j++) *rows = *rows && reqs[i].box.ext[j] == 1;
        vs[i].str[axis] = 0;  // (not read)
    }
    return 0;
}
// ... and the projecting sink: a thread per output point of the largest box; the body through LDS where the axis is the fastest that counts
int project_views(int N, uint32_t axis, const sz3hip_tile_req *reqs, uint32_t n, szk_region_sink *sink, std::vector<ReqView> &vs) {
    const bool index_op = project_index_op(sink->prj.op);
    for (uint32_t i = 0; i < n; i++)
        if (index_op && reqs[i].box.ext[axis] > 0xFFFFFFFFull)
            return fail(SZ3HIP_EINVAL, "box %u: the extent along the axis (%llu) is beyond an index op's uint32_t (2^32 - 1 at most)", i, (unsigned long long)reqs[i].box.ext[axis]);
    const int rc = collapsed_views(N, axis, reqs, n, project_out_bytes(sink->prj), vs, &sink->prj_threads, &sink->prj_rows, nullptr);
    if (rc) return rc;
    sink->kind = SZK_SINK_PROJECT;
    return 0;
}
}  // namespace

extern "C" int sz3hip_project_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_project_opts *opts,
                                       sz3hip_project_plan *out) {
    if (!conf || !out) return fail(SZ3HIP_EINVAL, "sz3hip_project_plan_for: NULL argument (%s)", !conf ? "conf" : "out");
    int rc = dtype_check(dataType);
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    if (rc || (rc = request_args("sz3hip_project_plan_for", reqs, n)) || (rc = project_opts_check(opts, &sink.prj))) return rc;
    std::vector<szk_region_geom> gs;
    std::vector<ReqView> vs;
    memset(out, 0, sizeof(*out));
    if ((rc = szi_request_geometry_conf(conf, reqs, n, gs, &out->scratch_elems)) || (rc = project_axis(opts, conf->N, &sink.prj)) ||
        (rc = project_views(conf->N, opts->axis, reqs, n, &sink, vs))) {
        memset(out, 0, sizeof(*out));
        return rc;
    }
    plan_prefix(out, reqs, n, gs);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t outs = 1;
        for (int j = 0; j < conf->N; j++) outs *= j == (int)opts->axis ? 1 : reqs[i].box.ext[j];
        out->out_points += outs;
    }
    out->out_elem_bytes = (uint32_t)project_out_bytes(sink.prj);
    return 0;
}

extern "C" int sz3hip_stream_project(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_project_opts *opts, void *stream) {
    if (!h) return fail(SZ3HIP_EINVAL, "sz3hip_stream_project: no handle");
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    int rc = request_args("sz3hip_stream_project", reqs, n);
    if (rc || (rc = project_opts_check(opts, &sink.prj))) return rc;
    Submit sub(h, stream);
    std::vector<ReqView> vs;
    if ((rc = submit_boxes(sub, reqs, n)) || (rc = project_axis(opts, sub.N, &sink.prj)) || (rc = project_views(sub.N, opts->axis, reqs, n, &sink, vs))) return rc;
    if ((rc = submit_begin(sub, &sink, sub.elems))) return rc;
    return submit_launch(sub, "projection", &sink, &vs, nullptr);
}

extern "C" int sz3hip_project_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides_in, const sz3hip_project_opts *opts,
                                     void *d_out, const int64_t *strides_out, void *stream) {
    int rc = device_dims(dataType, N, dims);
    if (rc) return rc;
    if (!d_out) return fail(SZ3HIP_EINVAL, "sz3hip_project_device: NULL argument (d_out)");
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    if ((rc = project_opts_check(opts, &sink.prj)) || (rc = project_axis(opts, N, &sink.prj))) return rc;
    DeviceView v;
    if ((rc = device_view(dataType, N, dims, d_in, strides_in, d_out, strides_out, &v))) return rc;
    std::vector<ReqView> vs;
    if ((rc = project_views(N, opts->axis, &v.q, 1, &sink, vs))) return rc;
    szk_region_gather_strided_box rec;
    szi_view_record(N, dims, v.str, 0, d_out, vs[0].str, &rec);
    hipStream_t s = (hipStream_t)stream;
    DeviceScope scope;
    HIPCHK(hipSetDevice(v.dev));
    if (szk_launch_region_project(dataType, d_in, nullptr, &rec, 1, &sink, s)) return fail(SZ3HIP_EHIP, "the projection could not be launched");
    return 0;
}

// ---- gradients of boxes: central differences, magnitude, vector --------------------------------------------------------------
namespace {
int gradient_opts_check(const sz3hip_gradient_opts *opts, szk_gradient_opts *go) {
    memset(go, 0, sizeof(*go));
    if (!opts) return fail(SZ3HIP_EINVAL, "NULL argument (opts): a gradient needs its op and spacing");
    if (opts->op > SZ3HIP_GRADIENT_VECTOR) return fail(SZ3HIP_EINVAL, "the options' op (%u) is not one of SZ3HIP_GRADIENT_DERIV .. SZ3HIP_GRADIENT_VECTOR (0 .. 3)", opts->op);
    if (opts->op != SZ3HIP_GRADIENT_DERIV && opts->axis)
        return fail(SZ3HIP_EINVAL, "the options' axis is %u: only SZ3HIP_GRADIENT_DERIV reads it, every other op takes axis 0", opts->axis);
    if (opts->out_type > SZ3HIP_DOUBLE) return fail(SZ3HIP_EINVAL, "the options' out_type (%u) is not SZ3HIP_FLOAT or SZ3HIP_DOUBLE (0, 1)", opts->out_type);
    if (opts->flags & ~SZ3HIP_GRADIENT_INTERIOR) return fail(SZ3HIP_EINVAL, "the options' flags (0x%x) hold bits beyond SZ3HIP_GRADIENT_INTERIOR", opts->flags);
    go->op = opts->op;
    go->out_type = opts->out_type;
    go->flags = opts->flags;
    return 0;
}
// ... and what needs the dimension count: the axis, counted in a record's four places from here on, and the N spacings
int gradient_axis(const sz3hip_gradient_opts *opts, int N, szk_gradient_opts *go) {
    if (opts->axis >= (uint32_t)N) return fail(SZ3HIP_EINVAL, "the options' axis (%u) is not one of the %d dimensions (0 .. %d)", opts->axis, N, N - 1);
    for (int a = 0; a < N; a++)
        if (!(opts->spacing[a] > 0.0 && opts->spacing[a] < INFINITY))
            return fail(SZ3HIP_EINVAL, "the options' spacing[%d] (%g) is not finite and above 0", a, opts->spacing[a]);
    go->axis = opts->axis + (uint32_t)(4 - N);
    go->N = (uint32_t)N;
    return 0;
}
size_t gradient_out_bytes(const szk_gradient_opts &go) { return (go.out_type == 0 ? 4 : 8) * (go.op == SZ3HIP_GRADIENT_VECTOR ? go.N : 1); }
bool gradient_differentiated(const szk_gradient_opts &go, int N, int j) { return go.op != SZ3HIP_GRADIENT_DERIV || (uint32_t)(4 - N + j) == go.axis; }
// the boxes' grid steps, the output boxes — the requests trimmed under INTERIOR — and their views by the request's rules with the output
// element's size; the sink with every box's table entry (boxes: n entries, in the request's order) and the largest box's output points
int gradient_views(int N, const sz3hip_gradient_opts *opts, const sz3hip_tile_req *reqs, uint32_t n, szk_region_sink *sink, std::vector<szk_gradient_box> &boxes,
                   uint64_t *out_points) {
    const szk_gradient_opts &go = sink->grd;
    const bool interior = (go.flags & SZ3HIP_GRADIENT_INTERIOR) != 0;
    const size_t tout = go.out_type == 0 ? 4 : 8;
    boxes.assign(n, szk_gradient_box());
    std::vector<sz3hip_tile_req> trimmed(reqs, reqs + n);
    for (uint32_t i = 0; i < n; i++) {
        memset(&boxes[i], 0, sizeof(boxes[i]));
        for (int j = 0; j < N; j++) {
            const double s = ldexp(opts->spacing[j], reqs[i].level);
            if (!(s < INFINITY))
                return fail(SZ3HIP_EINVAL, "box %u: the grid step of dimension %d, spacing (%g) * 2^%d, is not finite", i, j, opts->spacing[j], reqs[i].level);
            boxes[i].scale[4 - N + j] = s;
            if (!interior || !gradient_differentiated(go, N, j)) continue;
            if (reqs[i].box.ext[j] < 3)
                return fail(SZ3HIP_EINVAL, "box %u: the extent of dimension %d is %llu: SZ3HIP_GRADIENT_INTERIOR drops the first and the last point of a differentiated axis and needs at least 3",
                            i, j, (unsigned long long)reqs[i].box.ext[j]);
            trimmed[i].box.ext[j] -= 2;
        }
    }
    for (uint32_t i = 0; i < n; i++)
        if ((uintptr_t)reqs[i].d_out % tout) return fail(SZ3HIP_EINVAL, "box %u: the output is not aligned to its element size (%zu bytes)", i, tout);
    std::vector<ReqView> vs;
    const int rc = request_views(N, trimmed.data(), n, gradient_out_bytes(go), vs);
    if (rc) return rc;
    sink->kind = SZK_SINK_GRADIENT;
    sink->grd_threads = 1;
    if (out_points) *out_points = 0;
    for (uint32_t i = 0; i < n; i++) {
        uint64_t outs = 1;
        boxes[i].dst = reqs[i].d_out;
        for (int j = 0; j < N; j++) {
            outs *= trimmed[i].box.ext[j];
            boxes[i].dstr[4 - N + j] = trimmed[i].box.ext[j] > 1 ? vs[i].str[j] : 0;
        }
        sink->grd_threads = std::max(sink->grd_threads, outs);
        if (out_points) *out_points += outs;
    }
    sink->grd_boxes = boxes.data();
    return 0;
}
}  // namespace

extern "C" int sz3hip_gradient_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_gradient_opts *opts,
                                        sz3hip_gradient_plan *out) {
    if (!conf || !out) return fail(SZ3HIP_EINVAL, "sz3hip_gradient_plan_for: NULL argument (%s)", !conf ? "conf" : "out");
    int rc = dtype_check(dataType);
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    if (rc || (rc = request_args("sz3hip_gradient_plan_for", reqs, n)) || (rc = gradient_opts_check(opts, &sink.grd))) return rc;
    std::vector<szk_region_geom> gs;
    std::vector<szk_gradient_box> boxes;
    uint64_t out_points = 0;
    memset(out, 0, sizeof(*out));
    if ((rc = szi_request_geometry_conf(conf, reqs, n, gs, &out->scratch_elems)) || (rc = gradient_axis(opts, conf->N, &sink.grd)) ||
        (rc = gradient_views(conf->N, opts, reqs, n, &sink, boxes, &out_points))) {
        memset(out, 0, sizeof(*out));
        return rc;
    }
    plan_prefix(out, reqs, n, gs);
    out->out_points = out_points;
    out->out_elem_bytes = (uint32_t)gradient_out_bytes(sink.grd);
    return 0;
}

extern "C" int sz3hip_stream_gradient(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_gradient_opts *opts, void *stream) {
    if (!h) return fail(SZ3HIP_EINVAL, "sz3hip_stream_gradient: no handle");
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    int rc = request_args("sz3hip_stream_gradient", reqs, n);
    if (rc || (rc = gradient_opts_check(opts, &sink.grd))) return rc;
    Submit sub(h, stream);
    std::vector<szk_gradient_box> boxes;
    if ((rc = submit_boxes(sub, reqs, n)) || (rc = gradient_axis(opts, sub.N, &sink.grd)) || (rc = gradient_views(sub.N, opts, reqs, n, &sink, boxes, nullptr))) return rc;
    if ((rc = submit_begin(sub, &sink, sub.elems))) return rc;
    return submit_launch(sub, "gradient", &sink, nullptr, nullptr);
}

extern "C" int sz3hip_gradient_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides_in, const sz3hip_gradient_opts *opts,
                                      void *d_out, const int64_t *strides_out, void *stream) {
    int rc = device_dims(dataType, N, dims);
    if (rc) return rc;
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    if ((rc = gradient_opts_check(opts, &sink.grd)) || (rc = gradient_axis(opts, N, &sink.grd))) return rc;  // (the options before any pointer)
    if (!d_out) return fail(SZ3HIP_EINVAL, "sz3hip_gradient_device: NULL argument (d_out)");
    DeviceView v;
    if ((rc = device_view(dataType, N, dims, d_in, strides_in, d_out, strides_out, &v))) return rc;
    std::vector<szk_gradient_box> boxes;
    if ((rc = gradient_views(N, opts, &v.q, 1, &sink, boxes, nullptr))) return rc;
    szk_region_gather_strided_box rec;
    szi_view_record(N, dims, v.str, 0, nullptr, nullptr, &rec);
    hipStream_t s = (hipStream_t)stream;
    DeviceScope scope;
    HIPCHK(hipSetDevice(v.dev));
    if (szk_launch_region_gradient(dataType, d_in, nullptr, &rec, 1, &sink, s)) return fail(SZ3HIP_EHIP, "the gradient could not be launched");
    return 0;
}

// ---- boxes composited along an axis: front to back through an RGBA table ------------------------------------------------------
namespace {
size_t composite_out_bytes(const szk_composite_opts &co) { return co.out_type == SZ3HIP_COMPOSITE_RGBA32F ? 16 : 4; }
int composite_opts_check(const sz3hip_composite_opts *opts, szk_composite_opts *co) {
    memset(co, 0, sizeof(*co));
    if (!opts) return fail(SZ3HIP_EINVAL, "NULL argument (opts): a compositing needs its window, axis and table");
    if (opts->out_type > SZ3HIP_COMPOSITE_RGBA8)
        return fail(SZ3HIP_EINVAL, "the options' out_type (%u) is not SZ3HIP_COMPOSITE_RGBA32F or SZ3HIP_COMPOSITE_RGBA8 (0, 1)", opts->out_type);
    const uint32_t known = SZ3HIP_COMPOSITE_REVERSE | SZ3HIP_COMPOSITE_LEVEL_OPACITY | SZ3HIP_COMPOSITE_ACCUMULATE;
    if (opts->flags & ~known)
        return fail(SZ3HIP_EINVAL, "the options' flags (0x%x) hold bits beyond SZ3HIP_COMPOSITE_REVERSE | _LEVEL_OPACITY | _ACCUMULATE", opts->flags);
    if (opts->reserved) return fail(SZ3HIP_EINVAL, "the options' reserved word is %u, not 0", opts->reserved);
    if (!(fabs(opts->lo) < INFINITY) || !(fabs(opts->hi) < INFINITY)) return fail(SZ3HIP_EINVAL, "the window [%g, %g) is not finite", opts->lo, opts->hi);
    if (!(opts->hi > opts->lo)) return fail(SZ3HIP_EINVAL, "the window [%g, %g) is empty: hi must be above lo", opts->lo, opts->hi);
    if (!(fabs(opts->hi - opts->lo) < INFINITY)) return fail(SZ3HIP_EINVAL, "the window [%g, %g) is too wide: hi - lo is not finite", opts->lo, opts->hi);
    if (!(opts->cutoff > 0.0)) return fail(SZ3HIP_EINVAL, "the options' cutoff (%g) is not above 0 (+Inf never stops a column)", opts->cutoff);
    if (opts->lut_n < 2 || opts->lut_n > SZ3HIP_MAX_LUT) return fail(SZ3HIP_EINVAL, "the table has %u entries: 2 .. %d are supported", opts->lut_n, SZ3HIP_MAX_LUT);
    if (!opts->d_lut) return fail(SZ3HIP_EINVAL, "the table (d_lut) is NULL");
    if ((uintptr_t)opts->d_lut % 16) return fail(SZ3HIP_EINVAL, "the table (d_lut) is not aligned to its 16-byte entries");
    if (opts->level_bias > 30) return fail(SZ3HIP_EINVAL, "the options' level_bias is %u: an opacity is squared 30 times at most", opts->level_bias);
    if ((opts->flags & SZ3HIP_COMPOSITE_ACCUMULATE) && opts->out_type != SZ3HIP_COMPOSITE_RGBA32F)
        return fail(SZ3HIP_EINVAL, "SZ3HIP_COMPOSITE_ACCUMULATE reads the output's four floats: it takes SZ3HIP_COMPOSITE_RGBA32F, not RGBA8");
    co->win.lo = opts->lo;
    co->win.hi = opts->hi;
    co->win.M = opts->lut_n - 1;
    co->win.scale = (double)(co->win.M + 1) / (opts->hi - opts->lo);
    co->win.lut_n = opts->lut_n;
    co->cutoff = opts->cutoff;
    co->out_type = opts->out_type;
    co->flags = opts->flags;
    co->d_lut = static_cast<const float *>(opts->d_lut);
    return 0;
}
// ... and what needs the dimension count: the axis, counted in a record's four places from here on
int composite_axis(const sz3hip_composite_opts *opts, int N, szk_composite_opts *co) {
    if (opts->axis >= (uint32_t)N) return fail(SZ3HIP_EINVAL, "the options' axis (%u) is not one of the %d dimensions (0 .. %d)", opts->axis, N, N - 1);
    co->axis = opts->axis + (uint32_t)(4 - N);
    co->N = (uint32_t)N;
    return 0;
}
// every box's squarings, the views of the collapsed boxes (the projection's way) and the sink with every box's table entry (boxes: n
// entries, in the request's order)
int composite_views(int N, const sz3hip_composite_opts *opts, const sz3hip_tile_req *reqs, uint32_t n, szk_region_sink *sink, std::vector<szk_composite_box> &boxes,
                    uint64_t *out_points) {
    boxes.assign(n, szk_composite_box());
    for (uint32_t i = 0; i < n; i++) {
        memset(&boxes[i], 0, sizeof(boxes[i]));
        const uint64_t s = (uint64_t)opts->level_bias + ((opts->flags & SZ3HIP_COMPOSITE_LEVEL_OPACITY) && reqs[i].level > 0 ? (uint64_t)reqs[i].level : 0);
        if (s > 30)
            return fail(SZ3HIP_EINVAL, "box %u: level_bias (%u) and the box's level (%d) make %llu squarings: an opacity is squared 30 times at most", i, opts->level_bias,
                        reqs[i].level, (unsigned long long)s);
        boxes[i].s = s;
    }
    std::vector<ReqView> vs;
    const int rc = collapsed_views(N, opts->axis, reqs, n, composite_out_bytes(sink->cmp), vs, &sink->cmp_threads, &sink->cmp_rows, out_points);
    if (rc) return rc;
    sink->kind = SZK_SINK_COMPOSITE;
    for (uint32_t i = 0; i < n; i++) {
        boxes[i].dst = reqs[i].d_out;
        for (int j = 0; j < N; j++) boxes[i].dstr[4 - N + j] = j != (int)opts->axis && reqs[i].box.ext[j] > 1 ? vs[i].str[j] : 0;
    }
    sink->cmp_boxes = boxes.data();
    return 0;
}
}  // namespace

extern "C" int sz3hip_composite_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_composite_opts *opts,
                                         sz3hip_composite_plan *out) {
    if (!conf || !out) return fail(SZ3HIP_EINVAL, "sz3hip_composite_plan_for: NULL argument (%s)", !conf ? "conf" : "out");
    int rc = dtype_check(dataType);
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    if (rc || (rc = request_args("sz3hip_composite_plan_for", reqs, n)) || (rc = composite_opts_check(opts, &sink.cmp))) return rc;
    std::vector<szk_region_geom> gs;
    std::vector<szk_composite_box> boxes;
    uint64_t out_points = 0;
    memset(out, 0, sizeof(*out));
    if ((rc = szi_request_geometry_conf(conf, reqs, n, gs, &out->scratch_elems)) || (rc = composite_axis(opts, conf->N, &sink.cmp)) ||
        (rc = composite_views(conf->N, opts, reqs, n, &sink, boxes, &out_points))) {
        memset(out, 0, sizeof(*out));
        return rc;
    }
    plan_prefix(out, reqs, n, gs);
    out->out_points = out_points;
    out->out_elem_bytes = (uint32_t)composite_out_bytes(sink.cmp);
    return 0;
}

extern "C" int sz3hip_stream_composite(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_composite_opts *opts, void *stream) {
    if (!h) return fail(SZ3HIP_EINVAL, "sz3hip_stream_composite: no handle");
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    int rc = request_args("sz3hip_stream_composite", reqs, n);
    if (rc || (rc = composite_opts_check(opts, &sink.cmp))) return rc;
    Submit sub(h, stream);
    std::vector<szk_composite_box> boxes;
    if ((rc = submit_boxes(sub, reqs, n)) || (rc = composite_axis(opts, sub.N, &sink.cmp)) || (rc = composite_views(sub.N, opts, reqs, n, &sink, boxes, nullptr))) return rc;
    if ((rc = submit_begin(sub, &sink, sub.elems))) return rc;
    return submit_launch(sub, "compositing", &sink, nullptr, nullptr);
}

extern "C" int sz3hip_composite_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides_in, const sz3hip_composite_opts *opts,
                                       void *d_out, const int64_t *strides_out, void *stream) {
    int rc = device_dims(dataType, N, dims);
    if (rc) return rc;
    szk_region_sink sink;
    memset(&sink, 0, sizeof(sink));
    if ((rc = composite_opts_check(opts, &sink.cmp)) || (rc = composite_axis(opts, N, &sink.cmp))) return rc;  // (the options before any pointer)
    if (!d_out) return fail(SZ3HIP_EINVAL, "sz3hip_composite_device: NULL argument (d_out)");
    DeviceView v;
    if ((rc = device_view(dataType, N, dims, d_in, strides_in, d_out, strides_out, &v))) return rc;
    std::vector<szk_composite_box> boxes;
    if ((rc = composite_views(N, opts, &v.q, 1, &sink, boxes, nullptr))) return rc;
    szk_region_gather_strided_box rec;
    szi_view_record(N, dims, v.str, 0, nullptr, nullptr, &rec);
    hipStream_t s = (hipStream_t)stream;
    DeviceScope scope;
    HIPCHK(hipSetDevice(v.dev));
    if (szk_launch_region_composite(dataType, d_in, nullptr, &rec, 1, &sink, s)) return fail(SZ3HIP_EHIP, "the compositing could not be launched");
    return 0;
}

extern "C" void sz3hip_stream_close(sz3hip_stream *h) {
    if (!h) return;
    DeviceScope scope;
    if (hipSetDevice(h->device) == hipSuccess) {
        if (h->req_pending) (void)hipEventSynchronize(h->ev_req);
        if (h->table_pending) (void)hipEventSynchronize(h->ev_table);
        // (a fallback handle's gathers carry no event: everything queued on the device)
        if (!h->fast) (void)hipDeviceSynchronize();
    }
    release(h);
}

/*
 * include/sz3hip.h — C ABI of libsz3hip.so: the MI355X (gfx950) implementation of the SZ3 hot path
 *     predictor -> linear quantizer -> Huffman (-> zstd on the host side of the boundary)
 *
 * Plain pointers and sizes only; no C++/torch types.  Three groups of entry points:
 *
 *  (1) the reference's own C ABI for this path, tools/sz3c/include/sz3c.h:52-59
 *      (SZ_compress_args / SZ_decompress / free_buf) — same names, argument meaning, malloc ownership and
 *      "unsupported => printf + exit(0)" behaviour — declared in include/sz3c.h of this repository.
 *  (2) sz3hip_compress / sz3hip_decompress (+ bound / config save / load): what the reference's C++ templates
 *      SZ_compress<T>(conf, data, cmpData, cmpCap) and SZ_decompress<T>(conf, cmpData, cmpSize, decData)
 *      (include/SZ3/api/sz.hpp:43,117) do, with the full SZ3::Config passed as the POD `sz3hip_config`
 *      (mirror of include/SZ3/utils/Config.hpp:441-478).  Host pointers in, host pointers out; the stream is the
 *      reference container (16-byte header + payload + Config trailer, sz.hpp:53-81) whose trailer carries the
 *      new cmprAlgo id SZ3HIP_ALGO_LORENZO (stock SZ3 rejects it with "Unknown compression algorithm",
 *      api/impl/SZDispatcher.hpp:98 — the honest behaviour: GPU streams are not decodable by the CPU reference).
 *  (3) the device-resident API (sz3hip_ctx_*, sz3hip_*_device): input already in HBM, payload left in HBM,
 *      split into stage1 (predict+quantize+histogram) and stage2 (codebook+encode) so that a multi-GPU caller
 *      can all-reduce the histogram between them.
 *  (4) the multi-GPU exchange (sz3hip_comm_*): an RCCL communicator over xGMI — one process driving all its GPUs
 *      (what sz3hip_compress does by itself when conf.openmp is set: slabs along dims[0] like SZ_compress_OMP,
 *      api/impl/SZImplOMP.hpp:16-117) or one process per GPU — with the sum all-reduce of the code histogram and the
 *      min/max all-reduce of the value range as its two collectives.
 *
 * Error handling: functions returning int return 0 on success, a negative SZ3HIP_E* code otherwise;
 * functions returning size_t return 0 on error. sz3hip_last_error() gives the message (thread-local).
 */
#ifndef SZ3HIP_H
#define SZ3HIP_H
#include <stddef.h>
#include <stdint.h>
#include "sz3hip_debug.h"

#ifdef __cplusplus
extern "C" {
#endif

/* data types: include/SZ3/utils/Config.hpp:27-36 */
#define SZ3HIP_FLOAT 0
#define SZ3HIP_DOUBLE 1
/* host-buffer API only: integers ride the f64 pipeline (exact; 64-bit values beyond 2^53 -> the array stays lossless). The numbers
 * are the reference's SZ_UINT8 .. SZ_INT64 (include/SZ3/def.hpp:27-36), the element types of its HDF5 filter (H5Z_SZ3.cpp:195-227) */
#define SZ3HIP_UINT8 2
#define SZ3HIP_INT8 3
#define SZ3HIP_UINT16 4
#define SZ3HIP_INT16 5
#define SZ3HIP_UINT32 6
#define SZ3HIP_INT32 7
#define SZ3HIP_UINT64 8
#define SZ3HIP_INT64 9

/* error-bound modes: include/SZ3/utils/Config.hpp:66 (enum EB) */
enum { SZ3HIP_EB_ABS = 0, SZ3HIP_EB_REL, SZ3HIP_EB_PSNR, SZ3HIP_EB_L2NORM, SZ3HIP_EB_ABS_AND_REL, SZ3HIP_EB_ABS_OR_REL };

/* algorithms: include/SZ3/utils/Config.hpp:80 (enum ALGO) + the ids of the GPU stream formats */
enum {
    SZ3HIP_ALGO_LORENZO_REG = 0,
    SZ3HIP_ALGO_INTERP_LORENZO = 1,
    SZ3HIP_ALGO_INTERP = 2,
    SZ3HIP_ALGO_NOPRED = 3,
    SZ3HIP_ALGO_LOSSLESS = 4,
    SZ3HIP_ALGO_HIP_LORENZO = 16, /* dual-quantisation integer Lorenzo + chunked canonical Huffman (this library) */
    SZ3HIP_ALGO_HIP_INTERP = 17   /* the reference's multilevel interpolation, pass-parallel, same codes bit for bit */
};

enum {
    SZ3HIP_OK = 0,
    SZ3HIP_EINVAL = -1,      /* std::invalid_argument in the reference */
    SZ3HIP_ECAPACITY = -2,   /* buffer too small (SZ3_ERROR_COMP_BUFFER_NOT_LARGE_ENOUGH) */
    SZ3HIP_EFORMAT = -3,     /* bad magic / version / corrupt stream */
    SZ3HIP_EHIP = -4,        /* HIP runtime error */
    SZ3HIP_EUNSUPPORTED = -5,
    SZ3HIP_EOUTLIERS = -6,   /* outlier lists overflowed: caller falls back to lossless like SZDispatcher.hpp:44-59 */
    SZ3HIP_EZSTD = -7
};

/* POD mirror of SZ3::Config (include/SZ3/utils/Config.hpp:441-478); dims slowest first, like Config::dims */
typedef struct sz3hip_config {
    int32_t N;
    uint64_t dims[4];
    uint64_t num;
    uint8_t cmprAlgo, errorBoundMode;
    double absErrorBound, relErrorBound, psnrErrorBound, l2normErrorBound;
    uint8_t openmp; /* compress: split dims[0] into one slab per visible GPU (SZ_compress_OMP's slabs, SZImplOMP.hpp:48-55)
                     * and write the multi-slab container; trailer bit: the payload is that container */
    int32_t quantbinCnt, blockSize;
    uint8_t predDim, dataType;
    uint8_t lorenzo, lorenzo2, regression, regression2;
    uint8_t interpAlgo, interpDirection; /* interpDirection: 0 .. N! - 1, the order of the dimensions (std::next_permutation steps from the identity);
                                          * a 1-D array takes any value (one order exists); elsewhere a value beyond N! - 1 is SZ3HIP_EINVAL */
    int32_t interpAnchorStride;
    double interpAlpha, interpBeta;
} sz3hip_config;

const char *sz3hip_last_error(void);
int sz3hip_last_error_code(void); /* SZ3HIP_E* of the last failure on this thread (for wrappers that map codes to exceptions) */
const char *sz3hip_version(void);

/* ---- (2) Config + host-buffer API ------------------------------------------------------------------------ */
/* SZ3::Config(dims...) : drops size-1 dims, sets N/num/predDim/blockSize and all defaults (Config.hpp:146-177,452-478) */
void sz3hip_config_init(sz3hip_config *c, int ndims, const uint64_t *dims_slowest_first);
/* Config::save / Config::load (Config.hpp:312-413); return bytes written / consumed */
size_t sz3hip_config_save(const sz3hip_config *c, unsigned char *out);
size_t sz3hip_config_load(sz3hip_config *c, const unsigned char *in);
/* Stock-stream interoperability. READING needs no switch: sz3hip_decompress decodes stock SZ3 streams of the
 * interpolation compressor (cmprAlgo ALGO_INTERP = 2, float / double, 1-D .. 4-D — what the reference's default ALGO_INTERP_LORENZO
 * writes for anything but some 1-D arrays) and of ALGO_LOSSLESS, next to this library's own ids 16 / 17; the reconstruction is the
 * reference's bit for bit. WRITING: sz3hip_set_stock_format(1) (or SZ3HIP_STOCK_FORMAT=1 in the environment) makes sz3hip_compress —
 * and everything on top of it — write ALGO_INTERP streams stock SZ3 reads whenever the interpolation predictor is chosen (a 1-D array whose
 * default-algorithm tuner takes Lorenzo gets the reference's ALGO_LORENZO_REG container with the Config the reference goes on with); calls that
 * name ALGO_LORENZO_REG / ALGO_NOPRED get those containers; what has no stock form here keeps this library's ids. Prediction, quantisation, reconstruction and the Huffman bit stream run on the
 * GPU either way; the tree's serialisation and zstd are host stages. The tree is built with the reference's own queue (which of two
 * equal frequencies merges first, encoder/HuffmanEncoder.hpp:402-432): wherever the codes are the reference's — ALGO_INTERP, ALGO_NOPRED,
 * the default algorithm with SZ3HIP_TUNER_EXACT=1, ALGO_LORENZO_REG (round 6: the writer repeats its per-block choices against the coded array until they are the reference's) — the container
 * written IS the reference's file byte for byte, as long as its buffer leaves in one zstd frame: up to 1 MB by default (larger buffers are
 * cut into 1 MB frames for the pool's threads; stock SZ3 reads them), any size with SZ3HIP_STOCK_ONE_FRAME=1 (one host thread, ~0.4 GB/s). */
void sz3hip_set_stock_format(int on);
int sz3hip_get_stock_format(void);
/* the same over at most `avail` readable bytes: 0 when the serialised Config does not fit in them (truncated stream) */
size_t sz3hip_config_load_n(sz3hip_config *c, const unsigned char *in, size_t avail);
/* SZ_compress_size_bound<T> (api/impl/SZImpl.hpp:34-44) */
size_t sz3hip_compress_bound(const sz3hip_config *c, int dataType);
/* SZ_compress<T>(conf, data, cmpData, cmpCap) -> size (api/sz.hpp:43); `conf` is not modified (copied, sz.hpp:45).
 * conf->openmp (SZ_compress_impl, api/impl/SZImpl.hpp:10-20): dims[0] is split into independent slabs exactly like
 * SZ_compress_OMP (api/impl/SZImplOMP.hpp:48-55), one per visible GPU (SZ3HIP_GPUS caps the GPUs, SZ3HIP_SLABS sets
 * another slab count; never more slabs than dims[0]); range-based bounds use the global value range (:57-69); the code
 * histograms of all slabs are summed (RCCL all-reduce across GPUs) so that every slab is coded with the same code book;
 * the slabs are stored in the reference's multi-slab container [i32 G][Config x G][u64 size x G][blob x G] (:100-107),
 * every blob what a single-slab call would have produced.
 * Large plain calls (round 5: >= 96 MB, absolute or L2-norm bound, ALGO_LORENZO_REG / ALGO_NOPRED, no conf->openmp) are written in the
 * same container by ONE GPU as a pipeline of up to 8 pieces — the copy in of piece k + 1 beside the kernels of piece k beside the copy
 * out + zstd of piece k - 1 —, every piece with its own code book; SZ3HIP_PIECES=0 keeps them whole (INTEGRATION.md sections 6, 7).
 * The trailer's dataType field: this library's own streams (ids 16 / 17) name the element type of the call there (the decoder refuses a
 * request for another one); a stock container keeps conf->dataType as the caller left it, like the reference (Config.hpp:312-354 saves the
 * field as it finds it; neither the reference's CLI nor SZ_compress<T> sets it). */
size_t sz3hip_compress(const sz3hip_config *conf, int dataType, const void *data, char *cmpData, size_t cmpCap);
/* SZ_decompress<T>(conf, cmpData, cmpSize, decData) (api/sz.hpp:117): conf is overwritten from the trailer;
 * decData must hold conf.num elements (query with sz3hip_peek_config first). Also decodes ALGO_LOSSLESS streams and
 * multi-slab containers (trailer bit openmp; SZ_decompress_OMP, SZImplOMP.hpp:120-186), slab g on GPU g % visible GPUs; with one GPU
 * the slabs are unpacked and decoded side by side and copied out in order. Arrays of 32 MB and more leave the device through a ring
 * of pinned staging buffers whose chunks host threads copy on into decData (a fresh array's pages are faulted in by those threads). */
int sz3hip_decompress(sz3hip_config *conf, int dataType, const char *cmpData, size_t cmpSize, void *decData);
/* The two calls above for an array that lives in device memory: the container sz3hip_compress writes for the same array, byte for byte,
 * read from d_data; what sz3hip_decompress writes, bit for bit, written to d_out (conf is overwritten from the trailer). The array does not
 * cross the host link: only the payload does (zstd, header and trailer stay host stages; cmpData is host memory, its capacity rule
 * sz3hip_compress_bound). Everything between the copy in and the copy out is the host API's code: dispatcher policies (range-based bounds,
 * eb == 0, the ratio < 3 lossless check, the length_error fallback), stock format, conf->openmp slabs and the pipelined pieces (all coded
 * on the array's own device), the ten element types (integers on the f64 route, 64-bit values beyond 2^53 lossless), the tuner's decisions
 * (run in stage 1 with the host API's settings — exact pricing, deterministic — instead of beside the copy in).
 *  - d_data / d_out: device memory (hipPointerGetAttributes); the call runs on the device that owns it, not on SZ3HIP_DEVICE. Anything
 *    else is SZ3HIP_EINVAL before any launch.
 *  - strides: element strides, slowest first, one per conf->N extent (the extents left after size-1 ones are dropped); NULL: contiguous.
 *    Strides are >= 0; an output whose strides make two elements overlap is SZ3HIP_EINVAL. A contiguous f32 / f64 input is read in place
 *    (never written); integer or strided inputs are gathered into the library's buffer by a strided kernel; a contiguous f32 / f64 output
 *    of the library's own streams is decoded in place, other outputs are scattered into the view.
 *  - stream (may be NULL): compression — the library's streams wait for an event recorded on it before the array is first read, so a
 *    producer's pending kernels need no host synchronisation; decompression — what is queued on it is waited for before d_out is written.
 *    Both calls are synchronous: on return the container is written, d_data is no longer read and d_out is complete.
 * The array reaches the host only where the host API's code reads it there: the lossless stream and its fallbacks, the ratio < 3
 * comparison, the stock 1-D ALGO_LORENZO_REG chain (and, decoding, a lossless stream or that chain is decoded on the host and copied in). */
size_t sz3hip_compress_from_device(const sz3hip_config *conf, int dataType, const void *d_data, const int64_t *strides, char *cmpData, size_t cmpCap,
                                   void *stream);
int sz3hip_decompress_to_device(sz3hip_config *conf, int dataType, const char *cmpData, size_t cmpSize, void *d_out, const int64_t *strides,
                                void *stream);
/* Coarse decode: every 2^level-th point of a stream, bit for bit what a full decode puts at those positions. The
 * interpolation predictor is multilevel: a point whose coordinates are all multiples of 2^k is final before the levels of stride 2^(k-1)
 * and finer run, so a preview at 1/2, 1/4, 1/8 ... resolution needs neither the full-size array nor the finest (most expensive) levels.
 * sz3hip_coarse_dims: the coarse array's extents, ((dims[i] - 1) >> level) + 1 for each of conf->N extents, slowest first (extents of 1
 * are kept), into dims_out[conf->N]. A pure function: no device. level outside 0 .. 30, N outside 1 .. 4 or an extent of 0: SZ3HIP_EINVAL.
 * sz3hip_decompress_coarse_to_device: sz3hip_decompress_to_device for the coarse array. conf is overwritten from the trailer and stays
 * the FULL array's Config; d_out is a view of sz3hip_coarse_dims(conf, level) extents (the caller learns them from sz3hip_peek_config);
 * strides, pointer and stream rules are sz3hip_decompress_to_device's. SZ3HIP_FLOAT and SZ3HIP_DOUBLE; the integer element types are
 * SZ3HIP_EUNSUPPORTED. Level 0 is sz3hip_decompress_to_device itself. Every container that call decodes is decoded:
 *  - fast path, a single-stream interpolation container (this library's id 17 or a stock ALGO_INTERP stream): the codes and raw values of
 *    the coarse points are gathered and the level kernels run on the compact array — a contiguous output is written in place, a strided one
 *    through the slot's buffer and the strided scatter; nothing of full size is written (the Huffman stage still decodes every code);
 *  - everything else (Lorenzo and block streams, ALGO_NOPRED, ALGO_LOSSLESS, the stock 1-D chain, conf->openmp slabs and pipelined
 *    pieces): the full array is decoded as sz3hip_decompress_to_device does, into a scratch array of FULL size that the library allocates
 *    in device memory for the call, and the coarse view of it is gathered by the strided gather kernel. This path needs that much HBM. */
int sz3hip_coarse_dims(const sz3hip_config *conf, int level, uint64_t *dims_out);
int sz3hip_decompress_coarse_to_device(sz3hip_config *conf, int dataType, const char *cmpData, size_t cmpSize, int level, void *d_out,
                                       const int64_t *strides, void *stream);
/* Region decode: the values of one box of the array, bit for bit what a full decode puts there, in work sized to the box (DESIGN.md
 * section 12). A point of an interpolation stream depends on a stencil of a few strides of its own level, so a box depends on a pyramid of
 * windows, one per level, not on the array. lo / ext hold one entry per conf->N extent, slowest first; the box is [lo[j], lo[j] + ext[j]).
 * sz3hip_region_plan_for: a pure function (no device). It validates the box and says what the region decode of it touches; it reads conf->N,
 * dims, interpAlgo, interpDirection and interpAnchorStride (negative: the default of the dimension count). ext[j] == 0, a box that leaves the
 * array or a NULL argument: SZ3HIP_EINVAL; an anchor stride that is no power of two: SZ3HIP_EUNSUPPORTED.
 * sz3hip_decompress_region_to_device: sz3hip_decompress_to_device for the box. conf is overwritten from the trailer and stays the FULL
 * array's Config; d_out is a view of ext extents; strides, pointer, stream and synchrony rules are sz3hip_decompress_to_device's.
 * SZ3HIP_FLOAT and SZ3HIP_DOUBLE; the integer element types are SZ3HIP_EUNSUPPORTED. A box equal to the whole array gives the full decode's
 * array. Every container that call decodes is decoded:
 *  - fast path, a single-stream interpolation container (this library's id 17 or a stock ALGO_INTERP stream): one compact buffer per level
 *    holds the level's window, the raw values that lie in a window are scattered, the passes run over the windows and the box is gathered
 *    from the finest buffer; nothing of full size is written (the Huffman stage still decodes every code);
 *  - everything else (Lorenzo and block streams, ALGO_NOPRED, ALGO_LOSSLESS, the stock 1-D chain, conf->openmp slabs and pipelined pieces,
 *    an anchor stride that is no power of two): the full array is decoded as sz3hip_decompress_to_device does, into a scratch array of FULL
 *    size that the library allocates in device memory for the call, and the box is gathered from it. This path needs that much HBM. */
typedef struct sz3hip_region_plan {
    int32_t n_levels;      /* interpolation levels that run (0: every point of the box is an anchor / the first point) */
    uint32_t stride[32];   /* stride s of level i, coarsest first */
    uint64_t win_lo[32][4], win_hi[32][4]; /* inclusive window, full-array coordinates, that level i READS (its "input window"), per conf->N extents */
    uint64_t points;       /* predicted points over all passes */
    uint64_t scratch_elems; /* elements of T the call needs in device memory besides d_out */
} sz3hip_region_plan;
int sz3hip_region_plan_for(const sz3hip_config *conf, const uint64_t *lo, const uint64_t *ext, sz3hip_region_plan *out);
int sz3hip_decompress_region_to_device(sz3hip_config *conf, int dataType, const char *cmpData, size_t cmpSize, const uint64_t *lo, const uint64_t *ext,
                                       void *d_out, const int64_t *strides, void *stream);
/* Tile decode: one box of the grid of every 2^level-th point — the tile of an image pyramid — bit for bit the full decode's values, in work
 * sized to the box, the Huffman stage included. lo / ext are in COARSE-grid coordinates, one entry per conf->N extent,
 * slowest first; the box [lo, lo + ext) must lie inside sz3hip_coarse_dims(conf, level). d_out holds ext extents; its value at coarse
 * coordinate c is the full decode's value at c << level. Level 0 is the region decode (sz3hip_decompress_region_to_device is this call at
 * level 0); the whole coarse grid as box gives sz3hip_decompress_coarse_to_device's array.
 * sz3hip_tile_plan_for: a pure function (no device). region: the region plan of the box on the coarse grid — windows in coarse-grid
 * coordinates, level strides in coarse steps; with anchors in use and 2^level at or beyond the anchor stride every coarse point is an anchor
 * (n_levels 0, points 0). units_total: decoder units (512 codes each) of the stream's code array, ceil(num / 512). units_needed: the units
 * the tile's passes read a code from — for every line of a pass window along the fastest dimension, every unit from the one that holds the
 * code of the line's first lattice point to the one that holds its last, and unit 0 where the first point (an array without anchors) is read.
 * sz3hip_tile_units_for: those units, strictly ascending, into units[0 .. cap); *n_needed is set even when cap is too small (then
 * SZ3HIP_ECAPACITY). A pure function.
 * Errors of the three: level outside 0 .. 30, ext[j] == 0, a box that leaves the coarse grid or a NULL argument: SZ3HIP_EINVAL before any
 * launch; an anchor stride that is no power of two: SZ3HIP_EUNSUPPORTED from the two pure functions (sz3hip_decompress_tile_to_device then
 * takes the fallback).
 * sz3hip_decompress_tile_to_device: pointer, stride, stream and synchrony rules are sz3hip_decompress_region_to_device's; conf comes back as
 * the FULL array's Config; SZ3HIP_FLOAT and SZ3HIP_DOUBLE. Fast path and fallback are the region decode's: the fallback (everything that is no
 * single interpolation stream, or an anchor stride that is no power of two) decodes the full array into a scratch of the call and gathers the
 * view whose strides are multiplied by 2^level and whose base lies at lo << level.
 * Sparse decode: on the fast path of this library's own interpolation stream (container id 17) the Huffman stage decodes the needed units
 * alone when they are few — at most half of the stream's and at most max(32768, an eighth of them) —; otherwise, and for stock ALGO_INTERP streams (whose codes come through the stock
 * decoder), every unit as before. sz3hip_set_sparse_decode(0) switches it off for the process (default on; SZ3HIP_SPARSE_DECODE=0 / 1 in the
 * environment decides before the first call of either function). The values do not depend on it. */
typedef struct sz3hip_tile_plan {
    sz3hip_region_plan region; /* windows, strides, points, scratch_elems: in COARSE-grid coordinates (the grid of sz3hip_coarse_dims(conf, level)) */
    uint64_t units_total;      /* decoder units of the stream's code array: ceil(num / 512) */
    uint64_t units_needed;     /* units the tile's passes read a code from */
} sz3hip_tile_plan;
int sz3hip_tile_plan_for(const sz3hip_config *conf, int level, const uint64_t *lo, const uint64_t *ext, sz3hip_tile_plan *out);
int sz3hip_tile_units_for(const sz3hip_config *conf, int level, const uint64_t *lo, const uint64_t *ext, uint32_t *units, uint64_t cap, uint64_t *n_needed);
int sz3hip_decompress_tile_to_device(sz3hip_config *conf, int dataType, const char *cmpData, size_t cmpSize, int level, const uint64_t *lo,
                                     const uint64_t *ext, void *d_out, const int64_t *strides, void *stream);
void sz3hip_set_sparse_decode(int on);
int sz3hip_get_sparse_decode(void);
/* test hook, process-wide and cumulative: decoder units the Huffman stage of the tile / region calls' fast path decoded, and units their
 * streams held (equal where the stage ran densely) */
void sz3hip_debug_tile_units(uint64_t *decoded, uint64_t *total);
/* Several tiles of one stream in one call: n boxes of the grid of every 2^level-th point — the screenful of tiles of a
 * pyramid level, a set of probe boxes — each bit for bit what sz3hip_decompress_tile_to_device and the full decode's slice deliver. The
 * boxes share what one call pays once: the container's zstd stage and the payload's copy in, one Huffman stage over the UNION of their
 * decoder units, and one reconstruction's launch sequence in which every launch carries all boxes (the launch count does not grow with n).
 * Boxes may overlap and repeat. Level 0 is the region decode of n boxes; all boxes of a request have the one level.
 * sz3hip_box: conf->N entries of lo / ext are used, slowest first, in coordinates of the grid of every 2^level-th point.
 * sz3hip_tiles_plan_for: a pure function (no device). points: the predicted points, summed over the boxes; scratch_elems: the boxes' level
 * buffers, one after the other; units_needed: the size of the union of the boxes' unit lists (sz3hip_tile_units_for).
 * d_outs: a HOST array of n device pointers; box i's array is contiguous, ext extents of T. There are no strided views in this call (the
 * single-box call has them). Outputs that overlap one another: SZ3HIP_EINVAL.
 * Errors: n == 0, n > SZ3HIP_MAX_BOXES, a NULL array: SZ3HIP_EINVAL. Every box is validated before anything is launched or written; the first
 * bad box is refused with the code and wording of sz3hip_decompress_tile_to_device, "box <index>: " in front. An anchor stride that is no power
 * of two: SZ3HIP_EUNSUPPORTED from the plan. SZ3HIP_FLOAT and SZ3HIP_DOUBLE; the integer element types are SZ3HIP_EUNSUPPORTED.
 * sz3hip_decompress_tiles_to_device: pointer, stream and synchrony rules are sz3hip_decompress_tile_to_device's; conf comes back as the FULL
 * array's Config. A container that is no single interpolation stream (or an anchor stride that is no power of two) takes the fallback ONCE: one
 * full decode into one scratch array of the call, then n gathers. */
#define SZ3HIP_MAX_BOXES 256
typedef struct sz3hip_box {
    uint64_t lo[4], ext[4];
} sz3hip_box;
typedef struct sz3hip_tiles_plan {
    uint32_t n_boxes;
    int32_t n_levels;        /* interpolation levels that run: the grid's, the same for every box */
    uint64_t points;         /* predicted points over all passes, summed over the boxes */
    uint64_t scratch_elems;  /* elements of T the call needs in device memory besides the outputs */
    uint64_t units_total;    /* decoder units of the stream's code array: ceil(num / 512) */
    uint64_t units_needed;   /* units in the union of the boxes' unit lists */
} sz3hip_tiles_plan;
int sz3hip_tiles_plan_for(const sz3hip_config *conf, int level, const sz3hip_box *boxes, uint32_t n, sz3hip_tiles_plan *out);
int sz3hip_decompress_tiles_to_device(sz3hip_config *conf, int dataType, const char *cmpData, size_t cmpSize, int level, const sz3hip_box *boxes,
                                      uint32_t n, void *const *d_outs, void *stream);
/* (test and measurement hook) the strided gather alone: the view (N extents, element strides) of d_in into the contiguous d_out on stream,
 * integers widened to f64 as the compress call does; asynchronous (the 64-bit integer types: the call waits for the launch).
 * sz3hip_debug_scatter is its mirror, the strided scatter alone: the contiguous d_in (N extents; f64 for the integer types, narrowed by
 * rint and a clamp to the type's range as the decompress call does; the float types are copied) into the view of d_out, which passes the
 * rules of an output first (no negative stride, no elements that overlap: SZ3HIP_EINVAL before any launch); asynchronous */
int sz3hip_debug_gather(int dataType, const void *d_in, int N, const uint64_t *dims, const int64_t *strides, void *d_out, void *stream);
int sz3hip_debug_scatter(int dataType, const void *d_in, int N, const uint64_t *dims, const int64_t *strides, void *d_out, void *stream);
/* The question that follows a round trip in device memory — is the decoded array within the bound, what PSNR did it get — answered where
 * the arrays lie: the numbers of the reference's verify<T> (utils/Statistic.hpp:79-137: Min, Max, range, max absolute error, max point-wise
 * relative error, PSNR, NRMSE, normError, normErr_norm, acEff) for two arrays in device memory, each read once by one reduction kernel
 * (sz3hip_verify.hip); 152 bytes cross the host link. Nothing falls back to a host loop.
 *  - dims: the caller's own N = 1 .. 4 extents, slowest first (extents of 1 are allowed; no Config is involved). strides_ori / strides_dec:
 *    element strides of each array, one per extent; NULL: contiguous. Strides are >= 0; the views may overlap and a stride of 0 is a
 *    broadcast (both arrays are only read). The two arrays share the extents, not the strides.
 *  - d_ori / d_dec: device memory of ONE device, aligned to the element size (hipPointerGetAttributes); the call runs on that device.
 *    Anything else is SZ3HIP_EINVAL before any launch, and *out is left as it was.
 *  - stream (may be NULL): the library's stream waits for an event recorded on it before the arrays are read; the call is synchronous:
 *    on return *out is filled. Calls on one device serialise on a workspace that is made by the first of them and kept for the process
 *    (after the first call on a device, a call allocates nothing).
 *  - per element a = ori, b = dec: float types e = |(double)b - (double)a|; integer types the exact difference (the unsigned magnitude at
 *    the type's width, then converted: an int64 pair beyond 2^53 that differs by 1 reports 1.0), a and b enter the sums as (double).
 *    Every accumulator is f64.
 *  - NON-FINITE positions: a position where a or b is NaN or +-Inf is counted in n_nonfinite and left out of every other statistic; it is
 *    also counted in n_nonfinite_mismatch when the two are not of the same kind (one NaN and the other not, an infinity against anything
 *    but the same infinity). With n_nonfinite == 0 every number means what the reference's verify means; the reference's own NaN
 *    behaviour depends on the element order (Max = ori_data[0], then "<") and is not reproduced. Nothing finite at all: min = max = NaN,
 *    max_diff = 0, argmax = n.
 *  - bound: n_over counts the finite positions with e > bound (strictly), first_over is the smallest row-major index of them (n: none);
 *    a bound that is negative or NaN means "no bound given" (n_over = 0, first_over = n).
 *  - argmax: the smallest row-major index, over the extents, at which max_diff is reached. max_pw_rel: max of e / |a| over a != 0.
 *  - derived fields, the reference's formulas in IEEE double with m = n - n_nonfinite, nothing special-cased (identical arrays: psnr = +inf,
 *    a constant ori: what IEEE gives): mse = sum_sq_err / m, range = max - min, psnr = 20 log10(range) - 10 log10(mse),
 *    nrmse = sqrt(mse) / range, l2_err = sqrt(sum_sq_err), l2_err_norm = l2_err / sqrt(sum_sq_dec), acEff = the Pearson coefficient
 *    (second moments accumulated about a value of the data and merged pairwise: DESIGN.md, "Verify on the device").
 * Errors: unknown dataType SZ3HIP_EUNSUPPORTED; N outside 1 .. 4, an extent of 0, a negative stride, out == NULL, a host pointer, no device,
 * arrays of two devices: SZ3HIP_EINVAL. */
typedef struct sz3hip_verify_stats {
    uint64_t n, n_nonfinite, n_nonfinite_mismatch, n_over, first_over, argmax;
    double min, max, max_diff, max_pw_rel;
    double sum_ori, sum_dec, sum_sq_err, sum_sq_dec;
    double psnr, nrmse, l2_err, l2_err_norm, acEff;
} sz3hip_verify_stats;
int sz3hip_verify_device(int dataType, int N, const uint64_t *dims, const void *d_ori, const int64_t *strides_ori, const void *d_dec,
                         const int64_t *strides_dec, double bound, sz3hip_verify_stats *out, void *stream);
/* One algorithm of the reference's dispatcher (SZ_compress_LorenzoReg / SZ_compress_Interp / ..., SZDispatcher.hpp:28-42 and
 * their SZ_decompress_* counterparts :89-99): only the bytes between the container's 16-byte header and its Config trailer.
 * compress: returns their number (0 on error); *conf is updated like the reference updates it (absolute bound resolved,
 * cmprAlgo = id of the stream written: SZ3HIP_ALGO_HIP_LORENZO / _HIP_INTERP, or ALGO_LOSSLESS after a fallback).
 * These are what include/SZ3/api/impl/SZAlgoHip.hpp binds inside the reference's own header tree. */
size_t sz3hip_compress_blob(sz3hip_config *conf, int dataType, const void *data, char *blob, size_t cap);
int sz3hip_decompress_blob(const sz3hip_config *conf, int dataType, const char *blob, size_t size, void *decData);
/* reads only header + trailer (what SZ_decompress does before dispatching, sz.hpp:119-141) */
int sz3hip_peek_config(sz3hip_config *conf, const char *cmpData, size_t cmpSize);

/* ---- (3) device-resident API -------------------------------------------------------------------------------- */
typedef struct sz3hip_ctx sz3hip_ctx;

/* workspace for arrays of up to max_elems elements of dataType on HIP device `device`: the arrays every call uses are
 * allocated here; a few that only some paths use (the block predictor's per-block arrays, the interpolation work array, the f64
 * decoder's int32 intermediates, the decoder's carry array) with the first call that takes that path — later calls allocate nothing */
sz3hip_ctx *sz3hip_ctx_create(int device, uint64_t max_elems, int dataType);
void sz3hip_ctx_destroy(sz3hip_ctx *ctx);
/* upper bound of the device payload for n elements (outlier lists of up to n / 32 entries: a compress call that needs more
 * returns SZ3HIP_EOUTLIERS when the buffer is this size) */
size_t sz3hip_payload_bound(const sz3hip_ctx *ctx, uint64_t n);
/* the bound with the largest outlier lists the library will build (n / 8 entries: rough fields at tight bounds, small
 * quantbinCnt). With a buffer this large sz3hip_compress_device grows its lists on demand and retries instead of
 * returning SZ3HIP_EOUTLIERS (the reference keeps any number of unpredictable values, LinearQuantizer.hpp:43-66). */
size_t sz3hip_payload_bound_max(const sz3hip_ctx *ctx, uint64_t n);
/* The bound for one Config: like the two above (worst_case != 0: the second), and also sufficient for the block-composed predictor's
 * side section on thin arrays (an extent below 9), which have more blocks per element than the shape-blind bounds assume. */
size_t sz3hip_payload_bound_conf(const sz3hip_ctx *ctx, const sz3hip_config *conf, int worst_case);

/* global min/max of a device array (K0: utils/Statistic.hpp:12-21); result written to host doubles (synchronises) */
int sz3hip_minmax_device(sz3hip_ctx *ctx, const void *d_in, uint64_t n, double *min_out, double *max_out, void *stream);

/* stage 1: prequantise + integer Lorenzo + code emission + outlier capture + histogram (K1+K4).
 * conf: N/dims/absErrorBound(must already be absolute)/quantbinCnt are used. Asynchronous on `stream` — except for the paths
 * that decide on the host from a device result before going on: ALGO_INTERP_LORENZO (the auto-tuner's outcome) and
 * ALGO_LORENZO_REG with lorenzo2 / regression on 3-D arrays (the selection pass's count: a field on which only first-order Lorenzo
 * is chosen is handed to the plain Lorenzo path) synchronise the stream once inside this call.
 * d_in must stay valid and unchanged until sz3hip_compress_finish returns: a context that took a shortcut from what its
 * previous call found (the one-launch form of stage 1 assumes the previous call's code width) repeats the call from stage 1
 * inside finish() when this call's data says otherwise.
 * Predictor sets of ALGO_LORENZO_REG (api/impl/SZAlgoLorenzoReg.hpp:22-64): lorenzo alone = the plain Lorenzo stream (N = 1..4);
 * with regression: per-block choice in 1-D (blockSize 4..65535, default 128), 2-D (4..32, default 16) and 3-D (4..8, default 6);
 * lorenzo2: 3-D. Elsewhere a set that contains lorenzo is coded by it alone (the trailer records that), others are refused
 * with SZ3HIP_EUNSUPPORTED. */
int sz3hip_compress_stage1(sz3hip_ctx *ctx, const sz3hip_config *conf, const void *d_in, void *stream);
/* device pointer to the code histogram: uint64_t[sz3hip_histogram_len()] — the buffer a multi-GPU caller
 * all-reduces (sum) between stage1 and stage2 */
void *sz3hip_histogram_ptr(sz3hip_ctx *ctx);
size_t sz3hip_histogram_len(const sz3hip_ctx *ctx);
/* let the caller own the histogram buffer (uint64_t[sz3hip_histogram_len()] in device memory), e.g. a tensor that its
 * communication library can all-reduce in place; NULL restores the internal buffer */
int sz3hip_ctx_set_histogram(sz3hip_ctx *ctx, void *d_hist);
/* stage 2: canonical codebook from the histogram (K5), chunked Huffman bit-pack (K6), payload assembly into
 * d_payload (device, capacity cap bytes). Asynchronous on `stream`. */
int sz3hip_compress_stage2(sz3hip_ctx *ctx, void *d_payload, size_t cap, void *stream);
/* waits for `stream`, returns the payload size in *payload_size (host), SZ3HIP_EOUTLIERS / SZ3HIP_ECAPACITY on overflow */
int sz3hip_compress_finish(sz3hip_ctx *ctx, size_t *payload_size, void *stream);
/* stage1 + stage2 + finish */
int sz3hip_compress_device(sz3hip_ctx *ctx, const sz3hip_config *conf, const void *d_in, void *d_payload, size_t cap,
                           size_t *payload_size, void *stream);
/* inverse: payload (device) -> d_out (device, n elements). Synchronises once to read the 160-byte header. */
int sz3hip_decompress_device(sz3hip_ctx *ctx, const void *d_payload, size_t payload_size, void *d_out, void *stream);
/* the same for every 2^level-th point of an interpolation payload (predictor id 1; see sz3hip_coarse_dims above): d_out receives
 * prod(((dims[i] - 1) >> level) + 1) elements, contiguous, bit for bit the full decode's values at those points. Header parse and Huffman
 * stage are sz3hip_decompress_device's; then the coarse points' codes are gathered into a buffer of max_n / 2 + 8 codes that the
 * context's first coarse call allocates and the context keeps (later calls allocate nothing), and the level kernels run on the compact
 * array. Level 0 is sz3hip_decompress_device itself; a level outside 0 .. 30 is SZ3HIP_EINVAL. Any other predictor: SZ3HIP_EUNSUPPORTED —
 * a device context has no full-size scratch of its own; sz3hip_decompress_coarse_to_device decodes every container. */
int sz3hip_decompress_device_coarse(sz3hip_ctx *ctx, const void *d_payload, size_t payload_size, int level, void *d_out, void *stream);
/* the same for one box of an interpolation payload (predictor id 1; see sz3hip_region_plan_for above): lo / ext hold one entry per extent
 * the payload's header names, d_out receives prod(ext) elements, contiguous, bit for bit the full decode's values in the box. Header parse and
 * Huffman stage are sz3hip_decompress_device's; the box's checks come before any launch. The context's first region call allocates the levels'
 * buffers (plan.scratch_elems elements; grown when a later plan needs more) and the context keeps them: a call whose plan fits allocates
 * nothing. Any other predictor: SZ3HIP_EUNSUPPORTED — a device context has no full-size scratch of its own;
 * sz3hip_decompress_region_to_device decodes every container. */
int sz3hip_decompress_device_region(sz3hip_ctx *ctx, const void *d_payload, size_t payload_size, const uint64_t *lo, const uint64_t *ext, void *d_out,
                                    void *stream);
/* the same for a box of the grid of every 2^level-th point (see sz3hip_tile_plan_for above; level 0 is sz3hip_decompress_device_region, which
 * is this call). The context's first tile / region call also allocates the unit list — a pinned and a device array of max_n / 512 + 1 entries —
 * and keeps it; the list travels by one asynchronous copy on `stream` in front of the Huffman stage's launch. */
int sz3hip_decompress_device_tile(sz3hip_ctx *ctx, const void *d_payload, size_t payload_size, int level, const uint64_t *lo, const uint64_t *ext,
                                  void *d_out, void *stream);
/* the same for n boxes of one level in one call (see sz3hip_tiles_plan_for above): lo / ext of a box hold one entry per extent the payload's
 * header names; d_outs is a host array of n device pointers, box i's array contiguous. One Huffman stage decodes the union of the boxes' units
 * (the list form when the union is within the sparse limit, else the dense launch); the boxes' level buffers lie one after the other in the
 * context's region scratch; the records the reconstruction's workgroups read are built into a pinned array the context keeps and travel by one
 * asynchronous copy on `stream` in front of the first launch. Calls of one context may follow each other on a stream without a host
 * synchronisation in between. Any other predictor: SZ3HIP_EUNSUPPORTED, as for the single box. */
int sz3hip_decompress_device_tiles(sz3hip_ctx *ctx, const void *d_payload, size_t payload_size, int level, const sz3hip_box *boxes, uint32_t n,
                                   void *const *d_outs, void *stream);
/* test hook, process-wide and cumulative: kernel launches issued by the box reconstructions, single and multi */
uint64_t sz3hip_debug_region_launches(void);
/* test hook: the capacity of the context's region scratch, in elements (0 before its first region call) */
uint64_t sz3hip_debug_region_scratch(const sz3hip_ctx *ctx);
/* test hook: the number of region decodes of this process that ran over the box's windows (the fast path of either call; a multi-box
 * call counts once, whatever the number of its boxes); a container that went through the full-decode fallback does not count */
uint64_t sz3hip_debug_region_fast_calls(void);

/* ---- an opened stream: everything that does not depend on the box is done once ----
 * A viewer or an analysis asks one stream for many boxes. Open does, once, what every call above pays again: the zstd stage and the payload's
 * copy in, the header's round trip, the decoder tables and the DENSE Huffman launch over every unit (a stock ALGO_INTERP stream: the stock
 * decoder). Open may synchronise. When it returns the handle owns what a request reads — the per-element code array (2 bytes per element), the
 * raw-value lists, the interpolation parameters, a region scratch and the pinned and device tables — and the caller's blob or payload may be
 * freed or overwritten. A container that is no single interpolation stream (Lorenzo and block streams, ALGO_NOPRED, ALGO_LOSSLESS, the stock
 * 1-D chain, conf->openmp slabs, pipelined pieces, an anchor stride that is no power of two) takes the full decode ONCE, at open, into an array
 * the handle keeps (stats.fast == 0); its requests are strided gathers out of that array. Every container the library decodes can be opened.
 * float / double only: an integer dataType is SZ3HIP_EUNSUPPORTED, with the partial calls' wording.
 *   sz3hip_stream_open          an SZ3 container in host memory; conf comes back as the full array's Config; device < 0: the calling thread's
 *                               current device
 *   sz3hip_stream_open_payload  a device context's payload (SZH1) in device memory; `stream`: what produced the payload is waited for there
 *   sz3hip_stream_config        the full array's Config (a payload's: extents, error bound and interpolation fields)
 *   sz3hip_stream_tiles         sz3hip_decompress_device_tiles' semantics exactly — a level, 1 .. SZ3HIP_MAX_BOXES boxes in coarse coordinates,
 *                               contiguous outputs, every box and output checked before anything is launched or written, the same codes and
 *                               wording with "box <i>: " in front, overlapping and repeated boxes allowed, level 0 the region decode, the whole
 *                               grid as a box the coarse decode — but it runs the reconstruction alone: no Huffman stage, no copy of the payload,
 *                               no device-to-host copy and no host synchronisation (but the wait for the previous request's table copy, and a
 *                               scratch or table that has to grow). The request's coarsest levels may run in one launch (sz3hip_debug_chain_points).
 *   sz3hip_stream_close         waits for the handle's outstanding work, then frees everything. NULL is allowed.
 * A handle serves ONE request at a time: it is not thread-safe (two handles are independent of each other). A request on another HIP stream
 * than the previous one's is ordered behind it by an event — the scratch and the tables are shared — without a wait on the host. */
typedef struct sz3hip_stream sz3hip_stream;
/* (no typedef: the statistics call carries the struct's name, as stat(2) does — write `struct sz3hip_stream_stats`) */
struct sz3hip_stream_stats {
    uint32_t fast;                       /* 1: requests run over the boxes' windows; 0: gathers out of the resident full array */
    uint32_t huffman_stages;             /* Huffman stages behind this handle's codes: 1 after open, for its life — no request adds one (0 on a handle
                                          * that keeps the full array: the stages of that one full decode are not counted) */
    uint32_t launches_last_request;      /* kernel launches the last request issued */
    uint32_t chain_levels_last_request;  /* ... and how many of its coarsest levels ran inside the chain launch (0: chain off or no level fits) */
    uint64_t units_total;                /* decoder units (512 codes) of the stream */
    uint64_t requests;                   /* requests served */
    uint64_t scratch_elems;              /* capacity of the handle's region scratch, in elements */
    uint64_t resident_bytes;             /* device memory the handle holds: codes, lists, scratch, table (or the full array) */
    uint32_t n_levels_last_request;      /* levels the last request's reconstruction ran */
    uint32_t chain_points;               /* the threshold in force at the last request */
};
int sz3hip_stream_open(sz3hip_stream **out, sz3hip_config *conf, int dataType, const char *cmpData, size_t cmpSize, int device);
int sz3hip_stream_open_payload(sz3hip_stream **out, int device, int dataType, const void *d_payload, size_t payload_size, void *stream);
int sz3hip_stream_config(const sz3hip_stream *h, sz3hip_config *conf);
int sz3hip_stream_tiles(sz3hip_stream *h, int level, const sz3hip_box *boxes, uint32_t n, void *const *d_outs, void *stream);
int sz3hip_stream_stats(const sz3hip_stream *h, struct sz3hip_stream_stats *st);
void sz3hip_stream_close(sz3hip_stream *h);
/* ---- a frame in one request: boxes of SEVERAL levels, into strided views ----
 * A level-of-detail frame wants fine tiles near the focus and coarse ones elsewhere, each written where the viewer shows it — a rectangle of
 * its atlas or screen buffer. sz3hip_stream_request takes 1 .. SZ3HIP_MAX_BOXES boxes that each name their own level and their own output
 * view. Every box is bit for bit what sz3hip_stream_tiles delivers for that box at that level — the full decode's slice — written through
 * the view. The rest is sz3hip_stream_tiles' contract: overlapping and repeated boxes are allowed; every box and every output is checked
 * before anything is launched or written, with the existing codes and wording and "box <i>: " in front; no Huffman stage, no copy of the
 * payload, no device-to-host copy, no host synchronisation beyond a tiles request's waits, the same event ordering between requests on
 * different HIP streams. float / double handles only (there are no others). reserved != 0: SZ3HIP_EINVAL.
 * One launch sequence serves the whole request: the boxes are aligned by ARRAY level (a tile's grid level l is the array's level l + k), so
 * the request issues the launches of its finest level alone, whatever the number of boxes and of levels
 * (stats: launches_last_request; n_levels_last_request: the array levels that sequence ran). A request whose boxes all have ONE level issues
 * exactly the launches sz3hip_stream_tiles issues for them — the chain launch included where sz3hip_debug_chain_points says so — with the
 * strided gather in the gather's place. A request of two or more distinct levels does NOT take the chain: chain_levels_last_request is 0.
 * A handle that keeps the full array (stats.fast == 0) serves the request by one strided gather launch out of that array.
 * Views: strides are in elements, slowest first, one per extent of the box; all zero means contiguous. Dimensions of extent 1 are ignored.
 * Over the others a stride must be positive and the view nested in row-major order: strides[j] >= ext[j'] * strides[j'] for the next counted
 * dimension j'. A negative, zero or permuted stride is SZ3HIP_EINVAL, and the message says which. Two outputs of one request are accepted when
 * their byte hulls are disjoint, or when both have the same strides, nested over all their dimensions, and the element distance of their
 * origins decomposes without remainder into offsets o[j] along those strides with o[j] + ext_b[j] <= strides[j-1] / strides[j] for j >= 1 and
 * o[j] >= ext_a[j] for some j: two rectangles of one atlas that do not meet. Anything else: SZ3HIP_EINVAL ("box i: the output overlaps box
 * j's, or cannot be shown not to").
 * sz3hip_request_plan_for: a pure function (no device), the request's checks — all but whether a pointer is device memory — and what it
 * touches: points and scratch_elems are the sums of the boxes' sz3hip_tile_plan_for figures, n_levels the array levels the merged sequence
 * runs (the finest box's own level count). dataType: the element size of the views; an integer type is SZ3HIP_EUNSUPPORTED. */
typedef struct sz3hip_tile_req {
    int32_t level;        /* 0 .. 30: the box lies on the grid of every 2^level-th point */
    uint32_t reserved;    /* 0 */
    sz3hip_box box;       /* in that grid's coordinates, slowest first, N entries used */
    void *d_out;          /* device pointer: the view's element [0, .., 0] */
    int64_t strides[4];   /* element strides of the view, slowest first, N entries used; all zero: contiguous */
} sz3hip_tile_req;
typedef struct sz3hip_request_plan {
    uint32_t n;
    int32_t finest_level, coarsest_level, n_levels;
    uint64_t points, scratch_elems;
} sz3hip_request_plan;
int sz3hip_request_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n, sz3hip_request_plan *out);
int sz3hip_stream_request(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, void *stream);
/* ---- numbers about boxes, no output: per-box min, max, moments and histogram ----
 * An analysis that stays on one stream usually wants numbers about boxes — a brick's value range, a region's mean and variance, where the
 * maximum sits, a histogram — not the arrays. sz3hip_stream_reduce takes 1 .. SZ3HIP_MAX_BOXES boxes that each name their own level, as
 * sz3hip_stream_request does (coordinates, checks, codes and wording are that call's, "box <i>: " in front; repeated and overlapping boxes
 * are allowed; everything is checked before anything is launched or written), and runs the same launch sequence with a reduction and a
 * final fold in the strided gather's place: stats.launches_last_request is the same boxes' sz3hip_stream_request's, plus one. Nothing of a
 * box is written but its results, in DEVICE memory: d_stats[i] for box i, and row i of d_hist — n * (nbins + 2) counts, slot 0 = under,
 * slot nbins + 1 = over; ignored and allowed NULL when opts is NULL or nbins is 0. The call zeroes d_hist itself, on `stream`. No
 * device-to-host copy, no host synchronisation beyond a request's own waits; the ordering between requests is the existing one.
 * What is reduced: exactly the values sz3hip_stream_request would deliver for the box, each as x = (double)v.
 *   non-finite   a NaN or +-Inf point is counted in n_nonfinite and left out of everything else (sz3hip_verify_device's rule)
 *   min, argmin  argmin is the smallest box-local row-major index at which no finite point is smaller, min the value AT that index
 *                (-0.0 and +0.0 tie: the report carries that element's sign); max / argmax symmetric; nothing finite: NaN and n
 *   shift        K: the box's point of index 0 if finite, else 0.0
 *   sum, sum_sq  of x - K and (x - K)^2 over the finite points, each difference and square rounded once, added in a fixed order
 *   mean         K + sum / m, m = (double)(n - n_nonfinite);  variance  (sum_sq - sum * sum / m) / m  (the population's); IEEE double,
 *                no fused multiply-add; m = 0: both NaN
 *   histogram    scale = (double)nbins / (hi - lo), computed once on the host; a finite x goes to slot 0 if x < lo, to slot nbins + 1 if
 *                x >= hi, else to slot 1 + min((uint64_t)((x - lo) * scale), nbins - 1). A row sums to n - n_nonfinite.
 * Which points form a partial sum and the order of every fold depend on the box's point count ALONE (chunks of 4096 consecutive row-major
 * indices): every field is reproducible bit for bit, whatever the request's other boxes, the handle's kind or the device, and
 * sz3hip_stream_reduce is bit-identical to sz3hip_reduce_device over the same values.
 * Errors (SZ3HIP_EINVAL): nbins > SZ3HIP_MAX_BINS; nbins > 0 with lo or hi not finite or hi <= lo; opts->reserved or a request's reserved
 * not 0; d_stats NULL; d_hist NULL with nbins > 0; and sz3hip_stream_request's for the boxes. Integer types: SZ3HIP_EUNSUPPORTED.
 * sz3hip_reduce_device: the same reduction of ONE plain view in device memory into one sz3hip_box_stats and one histogram row (what a
 * handle that keeps the full array runs). N, dims, strides and the pointer's rules are sz3hip_verify_device's; float / double only. It is
 * asynchronous on `stream`; the partial records live in a per-device workspace the library keeps, calls are ordered by an event.
 * sz3hip_reduce_plan_for: a pure function (no device) with sz3hip_stream_reduce's checks. points, n_levels and the two level fields are
 * sz3hip_request_plan_for's; partials: the partial records (the sum of the boxes' ceil(points / 4096)); scratch_elems: the level buffers
 * plus the room of those records, in elements of dataType; hist_words = n * (nbins + 2). */
#define SZ3HIP_MAX_BINS 1024
typedef struct sz3hip_reduce_req {
    int32_t level;        /* 0 .. 30: the box lies on the grid of every 2^level-th point */
    uint32_t reserved;    /* 0 */
    sz3hip_box box;       /* in that grid's coordinates, slowest first, N entries used */
} sz3hip_reduce_req;
typedef struct sz3hip_reduce_opts {
    uint32_t nbins, reserved;  /* nbins 0: no histogram */
    double lo, hi;
} sz3hip_reduce_opts;
typedef struct sz3hip_box_stats {            /* 88 bytes, eleven 64-bit words */
    uint64_t n, n_nonfinite, argmin, argmax; /* points of the box; NaN / +-Inf among them; box-local row-major indices */
    double min, max;                         /* over the finite points; NaN when there is none (then argmin = argmax = n) */
    double shift, sum, sum_sq;               /* K; sum of (v - K); sum of (v - K)^2, over the finite points */
    double mean, variance;                   /* K + sum / m;  (sum_sq - sum * sum / m) / m;  m = (double)(n - n_nonfinite) */
} sz3hip_box_stats;
typedef struct sz3hip_reduce_plan {
    uint32_t n;
    int32_t finest_level, coarsest_level, n_levels;
    uint64_t points, scratch_elems, partials, hist_words;
} sz3hip_reduce_plan;
int sz3hip_reduce_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_reduce_req *reqs, uint32_t n, const sz3hip_reduce_opts *opts,
                           sz3hip_reduce_plan *out);
int sz3hip_stream_reduce(sz3hip_stream *h, const sz3hip_reduce_req *reqs, uint32_t n, const sz3hip_reduce_opts *opts, sz3hip_box_stats *d_stats,
                         uint64_t *d_hist, void *stream);
int sz3hip_reduce_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides, const sz3hip_reduce_opts *opts,
                         sz3hip_box_stats *d_stats, uint64_t *d_hist, void *stream);
/* ---- the points of boxes whose values lie in a range ----
 * Where in a box do the values lie in [lo, hi]: the cells an isosurface passes through, the candidates above a threshold, the points below
 * a floor, the NaNs. sz3hip_stream_select takes 1 .. SZ3HIP_MAX_BOXES boxes that each name their own level, as sz3hip_stream_request does
 * (coordinates, checks, codes and wording are that call's, "box <i>: " in front; repeated and overlapping boxes are allowed; everything is
 * checked before anything is launched or written), and runs the same launch sequence with three launches in the strided gather's place — a
 * count per chunk, a scan per box, the write: stats.launches_last_request is the same boxes' sz3hip_stream_request's, plus two (a handle
 * that keeps the full array: three). It counts as a request in sz3hip_stream_stats.
 * What is tested: exactly the values sz3hip_stream_request would deliver for the box, each as x = (double)v. A point is selected when
 * lo <= x && x <= hi; with SZ3HIP_SELECT_INVERT a point that is not NaN is selected when that is false. +-Inf are ordinary values (lo = hi
 * = +Inf selects the +Inf points), -0.0 and +0.0 compare equal, lo > hi is a valid empty range, a NaN point is selected only under
 * SZ3HIP_SELECT_NAN. The comparison is in double: a float 0.1f lies above a lo of 0.1.
 * What is written, all of it DEVICE memory: d_heads[i] = { n: the box's points, count: the selected ones, written = min(count, capacity),
 * capacity }; d_index[0 .. written): the `written` SMALLEST selected box-local row-major indices, ascending; d_value[r]: the raw bytes of
 * the point at d_index[r] (NaN payloads and zero signs kept; NULL: indices only). Elements from `written` on are not touched. count >
 * capacity is not an error: the caller reads the head and calls again. capacity 0 with both pointers NULL counts only. No device-to-host
 * copy, no host synchronisation beyond a request's own waits; the ordering between requests is the existing one.
 * The result depends on the box's values alone — not on the grid, on n, on the request's other boxes, on the handle's kind or on the
 * device: chunks of 4096 consecutive row-major indices are counted, a box's counts are scanned, and a hit's place is its chunk's offset
 * plus the hits in front of it in the chunk. No flags, no atomics. sz3hip_stream_select is byte-identical to sz3hip_select_device over
 * the same values.
 * Errors (SZ3HIP_EINVAL): opts NULL; lo or hi NaN; flags beyond the two; opts->reserved or a request's reserved not 0; d_heads NULL;
 * capacity > 0 with d_index NULL; d_value non-NULL with capacity 0; two boxes' output ranges overlapping ("box i: the output overlaps box
 * j's" — ranges of non-zero capacity, index against index and value against value); and sz3hip_stream_request's for the boxes. Integer
 * types: SZ3HIP_EUNSUPPORTED.
 * sz3hip_select_device: the same selection of ONE plain view in device memory (what a handle that keeps the full array runs). N, dims,
 * strides and the pointer's rules are sz3hip_verify_device's; float / double only. Asynchronous on `stream`; the chunk records live in the
 * per-device workspace sz3hip_reduce_device keeps, calls are ordered by its event.
 * sz3hip_select_plan_for: a pure function (no device) with sz3hip_stream_select's checks. points, n_levels and the two level fields are
 * sz3hip_request_plan_for's; partials: the chunk records (the sum of the boxes' ceil(points / 4096)); scratch_elems: the level buffers plus
 * the room of those records (8 bytes each, on an 8-byte boundary), in elements of dataType. */
#define SZ3HIP_SELECT_INVERT 1u   /* select the points that are NOT in [lo, hi]; a NaN point is still not selected */
#define SZ3HIP_SELECT_NAN    2u   /* NaN points are selected too (alone: with lo > hi and no INVERT) */
typedef struct sz3hip_select_req {   /* 96 bytes */
    int32_t level;        /* 0 .. 30: the box lies on the grid of every 2^level-th point */
    uint32_t reserved;    /* 0 */
    sz3hip_box box;       /* in that grid's coordinates, slowest first, N entries used */
    uint64_t *d_index;    /* device: capacity box-local row-major indices, ascending */
    void *d_value;        /* device: capacity elements of the stream's type, the points' raw bytes; NULL: indices only */
    uint64_t capacity;    /* 0 with both pointers NULL: count only */
} sz3hip_select_req;
typedef struct sz3hip_select_opts {  /* 24 bytes */
    double lo, hi;
    uint32_t flags, reserved;
} sz3hip_select_opts;
typedef struct sz3hip_select_head {  /* 32 bytes */
    uint64_t n, count, written, capacity;
} sz3hip_select_head;
typedef struct sz3hip_select_plan {  /* 40 bytes */
    uint32_t n;
    int32_t finest_level, coarsest_level, n_levels;
    uint64_t points, scratch_elems, partials;
} sz3hip_select_plan;
int sz3hip_select_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_select_req *reqs, uint32_t n, const sz3hip_select_opts *opts,
                           sz3hip_select_plan *out);
int sz3hip_stream_select(sz3hip_stream *h, const sz3hip_select_req *reqs, uint32_t n, const sz3hip_select_opts *opts, sz3hip_select_head *d_heads,
                         void *stream);
int sz3hip_select_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides, const sz3hip_select_opts *opts,
                         uint64_t *d_index, void *d_value, uint64_t capacity, sz3hip_select_head *d_head, void *stream);
/* ---- texels out of a request: boxes mapped to u8 / u16 / f16 / f32 / RGBA8 ----
 * What a renderer uploads from a frame is not raw f32 / f64 values but texels: 8- or 16-bit codes of a value window, half floats, or RGBA8
 * out of a transfer function. sz3hip_stream_map takes sz3hip_stream_request's own requests (the same struct, rules, codes and wording, "box
 * <i>: " in front; repeated and overlapping boxes are allowed; everything is checked before anything is launched or written) and runs the
 * same launch sequence with ONE mapping launch in the strided gather's place: stats.launches_last_request is the same boxes'
 * sz3hip_stream_request's (a handle that keeps the full array: 1). It counts as a request in sz3hip_stream_stats.
 * The views: d_out and strides describe a view of OUTPUT elements (1, 2, 2, 4 or 4 bytes); d_out must be aligned to the output element; the
 * output-overlap rule is the request's, evaluated with the output element's size.
 * What is mapped: exactly the values sz3hip_stream_request would deliver for the box, each as x = (double)v.
 *   U8, U16, LUT32: with M = 255, 65535 or lut_n - 1 and scale = (double)(M + 1) / (hi - lo), computed once on the host, a NaN point becomes
 *     nan_code, any other code = x < lo ? 0 : x >= hi ? M : min((uint64_t)((x - lo) * scale), M), in IEEE double without a fused multiply-add:
 *     sz3hip_stream_reduce's histogram rule with nbins = M + 1 and the two outer slots folded into the end codes — a texel's code is the bin
 *     the reduce counts the point in. +-Inf are ordinary values (-Inf -> 0, +Inf -> M); -0.0 equals +0.0. U8 and U16 store the code, LUT32
 *     stores d_lut[code] (a NaN point: nan_code itself, the raw texel).
 *   F16: (half)(float)x, both conversions rounding to nearest even — the two-step rounding is the definition; overflow gives +-Inf, half
 *     denormals are kept, a NaN stays a NaN (payload and sign unspecified).
 *   F32: (float)x; for a float handle the request's bytes, NaN payloads included.
 * The result at a point depends on that point's value and the options alone: sz3hip_stream_map is byte-identical to sz3hip_map_device over
 * the same values, on every route. No byte outside the boxes' views is written or read. No device-to-host copy, no host synchronisation
 * beyond a request's own waits; the ordering between requests is the existing one.
 * Errors (SZ3HIP_EINVAL): opts NULL; out_type not one of the five; flags or reserved not 0; for U8 / U16 / LUT32 lo or hi not finite, hi <=
 * lo or hi - lo not finite; nan_code above 255 (U8) or 65535 (U16); lut_n outside 2 .. SZ3HIP_MAX_LUT, d_lut NULL or not 4-byte aligned
 * (LUT32); lut_n or d_lut set for U8 / U16; lo, hi, nan_code, lut_n or d_lut not 0 / NULL for F16 / F32; an output not aligned to its
 * element; and sz3hip_stream_request's for the boxes and views. Integer types: SZ3HIP_EUNSUPPORTED.
 * sz3hip_map_device: the same mapping of ONE plain view in device memory into one output view (what a handle that keeps the full array
 * runs, in one launch). N, dims, strides_in and d_in's rules are sz3hip_reduce_device's; strides_out are the request's view rules (NULL or
 * all 0: contiguous). Asynchronous on `stream`; no workspace.
 * sz3hip_map_plan_for: a pure function (no device) with sz3hip_stream_map's checks. points, n_levels, the two level fields and
 * scratch_elems are sz3hip_request_plan_for's; out_elem_bytes is the output element's size. */
#define SZ3HIP_MAP_U8    1   /* 1 byte:  code of the window, M = 255   */
#define SZ3HIP_MAP_U16   2   /* 2 bytes: code of the window, M = 65535 */
#define SZ3HIP_MAP_F16   3   /* 2 bytes: IEEE half, (half)(float)x, round to nearest even both times */
#define SZ3HIP_MAP_F32   4   /* 4 bytes: (float)x — an f64 handle's values narrowed; an f32 handle's unchanged */
#define SZ3HIP_MAP_LUT32 5   /* 4 bytes: d_lut[code], M = lut_n - 1 — RGBA8 out of a transfer function */
#define SZ3HIP_MAX_LUT 1024
typedef struct sz3hip_map_opts {      /* 48 bytes */
    double lo, hi;                    /* the window (U8, U16, LUT32); 0, 0 otherwise */
    uint32_t out_type, flags;         /* SZ3HIP_MAP_*; flags 0 */
    uint32_t nan_code, lut_n;         /* what a NaN point becomes (U8: <= 255, U16: <= 65535, LUT32: the raw 32-bit texel); 2 .. SZ3HIP_MAX_LUT for LUT32, else 0 */
    const void *d_lut;                /* device, lut_n 32-bit entries, 4-byte aligned; NULL unless LUT32 */
    uint64_t reserved;                /* 0 */
} sz3hip_map_opts;
typedef struct sz3hip_map_plan {      /* 40 bytes */
    uint32_t n;
    int32_t finest_level, coarsest_level, n_levels;
    uint64_t points, scratch_elems, out_elem_bytes;
} sz3hip_map_plan;
int sz3hip_map_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_map_opts *opts,
                        sz3hip_map_plan *out);
int sz3hip_stream_map(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_map_opts *opts, void *stream);
int sz3hip_map_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides_in, const sz3hip_map_opts *opts,
                      void *d_out, const int64_t *strides_out, void *stream);
/* ---- boxes sampled at fractional positions: nearest and linear ----
 * An oblique slice plane, a tile resampled to a screen's resolution, values at probe or particle positions: none of them lies on a box's
 * own lattice. sz3hip_stream_sample takes 1 .. SZ3HIP_MAX_BOXES boxes that each name their own level, as sz3hip_stream_request does
 * (geometry, codes and wording are that call's, "box <i>: " in front; repeated and overlapping boxes are allowed; everything is checked
 * before anything is launched or written), each with queries of its own, and runs the same launch sequence with ONE sampling launch in the
 * strided gather's place: stats.launches_last_request is the same boxes' sz3hip_stream_request's (a handle that keeps the full array: 1).
 * It counts as a request in sz3hip_stream_stats. The values sampled are exactly those the request would deliver for the box.
 * Coordinates: a coordinate is box-local, in the box's level grid: c_j == q is box point q along dimension j, 0 .. ext_j - 1. All N
 *   dimensions are given, those of extent 1 too. Each coordinate is converted to double exactly.
 *   Points form (d_coords non-NULL): n_points * N coordinates of coord_type, query-major, slowest dimension first.
 *   Lattice form (d_coords NULL): query r = (i0 * counts[1] + i1) * counts[2] + i2 has
 *     c_j = ((origin[j] + (double)i0 * steps[0][j]) + (double)i1 * steps[1][j]) + (double)i2 * steps[2][j],
 *   evaluated in double, in that order, without a fused multiply-add.
 * Which queries are answered: a query is inside when every 0 <= c_j && c_j <= ext_j - 1 (so -0.0 is inside). A query with a NaN
 *   coordinate always yields (T)fill; an outside query yields (T)fill — unless SZ3HIP_SAMPLE_CLAMP is set: then each non-NaN coordinate is
 *   first clamped into [0, ext_j - 1], +-Inf to the ends.
 * NEAREST: i_j = min((uint64_t)floor(c_j + 0.5), ext_j - 1); the output is that point's raw bytes — no arithmetic, NaN payloads kept.
 * LINEAR: per dimension i = floor(c) and f = c - i. f == 0: the dimension contributes the value at i alone and i + 1 has no influence —
 *   a grid point reproduces the point's value exactly, next to an Inf or NaN neighbour too, and c = ext - 1 reads nothing outside the box.
 *   Otherwise (1.0 - f) * a + f * b in double: two multiplies and an add. The fold runs the fastest dimension first, then each slower
 *   one; the result is rounded once to T. NaN and Inf in a contributing corner propagate by IEEE rules.
 * The output depends on the box's values, the query and the options alone — not on the route, the grid, the other boxes or the handle's
 * kind: sz3hip_stream_sample is byte-identical to sz3hip_sample_device over the same values. No device-to-host copy, no host
 * synchronisation beyond a request's own waits; the ordering between requests is the existing one.
 * Errors (SZ3HIP_EINVAL): opts NULL; filter, coord_type or flags out of range; the options' reserved word not 0 (fill is not checked: any
 * double); d_out NULL or not aligned to T; n_points 0 or above 2^31; points form: d_coords not aligned to its type, or any of counts /
 * origin / steps not zero; lattice form: a count of 0, counts' product != n_points, or a non-finite origin / steps entry among the N
 * used; two boxes' output ranges overlapping ("box i: the output overlaps box j's"); and sz3hip_stream_request's for the boxes.
 * Integer types: SZ3HIP_EUNSUPPORTED. A refused call launches and writes nothing, and the handle serves the next request.
 * sz3hip_sample_device: the same sampling of ONE plain view in device memory (what a handle that keeps the full array runs, in one
 * launch): N, dims, strides and d_in's rules are sz3hip_reduce_device's; the view is the box, query->level, reserved and box must be
 * zero. Asynchronous on `stream`; no workspace.
 * sz3hip_sample_plan_for: a pure function (no device) with sz3hip_stream_sample's checks. Its fields are sz3hip_request_plan_for's, plus
 * queries, the sum of n_points. */
#define SZ3HIP_SAMPLE_NEAREST 0u
#define SZ3HIP_SAMPLE_LINEAR  1u
#define SZ3HIP_SAMPLE_CLAMP   1u      /* flags */
typedef struct sz3hip_sample_req {    /* 248 bytes */
    int32_t level;          /* 0 .. 30: the box lies on the grid of every 2^level-th point */
    uint32_t reserved;      /* 0 */
    sz3hip_box box;         /* in that grid's coordinates, slowest first, N entries used */
    const void *d_coords;   /* device: n_points * N coordinates, query-major, slowest dimension first; NULL: the lattice form */
    void *d_out;            /* device: n_points elements of the stream's type, contiguous */
    uint64_t n_points;      /* 1 .. 2^31 */
    uint64_t counts[3];     /* lattice form: queries along its three axes, slowest first, each >= 1, product == n_points */
    double origin[4];       /* lattice form: N entries used */
    double steps[3][4];     /* lattice form: axis a's step, N entries used */
} sz3hip_sample_req;
typedef struct sz3hip_sample_opts {   /* 24 bytes */
    uint32_t filter, coord_type;      /* SZ3HIP_SAMPLE_NEAREST / _LINEAR; SZ3HIP_FLOAT / SZ3HIP_DOUBLE: d_coords' type */
    uint32_t flags, reserved;         /* SZ3HIP_SAMPLE_CLAMP; 0 */
    double fill;                      /* what an unanswered query yields, as (T)fill */
} sz3hip_sample_opts;
typedef struct sz3hip_sample_plan {   /* 40 bytes */
    uint32_t n;
    int32_t finest_level, coarsest_level, n_levels;
    uint64_t points, scratch_elems, queries;
} sz3hip_sample_plan;
int sz3hip_sample_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_sample_req *reqs, uint32_t n, const sz3hip_sample_opts *opts,
                           sz3hip_sample_plan *out);
int sz3hip_stream_sample(sz3hip_stream *h, const sz3hip_sample_req *reqs, uint32_t n, const sz3hip_sample_opts *opts, void *stream);
int sz3hip_sample_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides, const sz3hip_sample_opts *opts,
                         const sz3hip_sample_req *query, void *stream);
/* ---- boxes projected along an axis: min, max, sum, mean, arg, count ----
 * A maximum-intensity projection of a brick with the depth of the maximum, a column integral or mean, a minimum along time: a box
 * collapsed along ONE axis. sz3hip_stream_project takes sz3hip_stream_request's own sz3hip_tile_req, 1 .. SZ3HIP_MAX_BOXES boxes that each
 * name their own level (geometry, codes and wording are that call's, "box <i>: " in front; repeated and overlapping boxes are allowed;
 * everything is checked before anything is launched or written), and runs the same launch sequence with ONE projecting launch in the
 * strided gather's place: stats.launches_last_request is the same boxes' sz3hip_stream_request's (a handle that keeps the full array: 1).
 * It counts as a request in sz3hip_stream_stats. One op and one axis hold for the whole call.
 * The output of a box is the box with extent 1 along `axis` (keepdim): d_out and strides[] describe a view in OUTPUT elements (4 or 8
 *   bytes), all N strides given (or none: contiguous); the stride at `axis` is not read, as the stride of any extent-1 dimension is not.
 *   The view rules, the alignment rule and the overlap rule are the request's, applied to that collapsed box with the output element's size.
 * The rule: the column of an output point is the box's values v_0 .. v_{E-1} along `axis`, ascending — exactly the values
 *   sz3hip_stream_request would deliver —, each taken as x_i = (double)v_i. A point is finite when fabs(x_i) < INFINITY; NaN and +-Inf
 *   points are left out of everything, as in sz3hip_stream_reduce.
 *   COUNT: the number of finite points (uint32_t).
 *   ARGMIN: the smallest i at which no finite point is smaller (compared in double: -0.0 and +0.0 tie, the first wins); E if none is
 *     finite. ARGMAX symmetric. E > 2^32 - 1 with an index op: SZ3HIP_EINVAL.
 *   MIN / MAX: (Tout)x_i at that index — the element's sign of zero kept; with Tout the handle's type a finite value's bytes pass
 *     unchanged; double -> float rounds to nearest even and may give Inf —, (Tout)fill if none is finite.
 *   SUM: s = 0.0; for i ascending over the finite points: s = s + x_i; then (Tout)s — the plain sequential fold in double, rounded once
 *     at the end, whichever axis is folded. A column without a finite point gives (Tout)0.0.
 *   MEAN: (Tout)(s / (double)m) with SUM's s and m the finite count; m == 0 gives (Tout)fill.
 * The output depends on the column, the op and the options alone — not on the route, the grid, the other boxes or the handle's kind:
 * sz3hip_stream_project is byte-identical to sz3hip_project_device over the same values. No device-to-host copy, no host synchronisation
 * beyond a request's own waits; no workspace. A 1-D box is one column and so one lane's work: sz3hip_stream_reduce is the call for one
 * number about a long 1-D box.
 * Errors (SZ3HIP_EINVAL): opts NULL; op above SZ3HIP_PROJECT_COUNT; axis >= N; out_type above SZ3HIP_DOUBLE, or not 0 with an index op;
 * reserved not 0 (fill is not checked: any double); d_out NULL or not aligned to the output element; the request's view and overlap cases
 * on the collapsed box; and sz3hip_stream_request's for the boxes. Integer types: SZ3HIP_EUNSUPPORTED. A refused call launches and writes
 * nothing, and the handle serves the next request.
 * sz3hip_project_device: the same projection of ONE plain view in device memory (what a handle that keeps the full array runs, in one
 * launch): N, dims, strides_in and d_in's rules are sz3hip_map_device's (x stride 2, stride-0 broadcasts and transposed views included);
 * d_out / strides_out: the view of the collapsed array in output elements (strides_out NULL: contiguous). Asynchronous on `stream`.
 * sz3hip_project_plan_for: a pure function (no device) with sz3hip_stream_project's checks. */
#define SZ3HIP_PROJECT_MIN    0u   /* value ops: the output element is out_type's */
#define SZ3HIP_PROJECT_MAX    1u
#define SZ3HIP_PROJECT_SUM    2u
#define SZ3HIP_PROJECT_MEAN   3u
#define SZ3HIP_PROJECT_ARGMIN 4u   /* index ops: the output element is uint32_t, out_type must be 0 */
#define SZ3HIP_PROJECT_ARGMAX 5u
#define SZ3HIP_PROJECT_COUNT  6u
typedef struct sz3hip_project_opts {   /* 24 bytes */
    uint32_t op, axis;                 /* SZ3HIP_PROJECT_*; 0 .. N-1, slowest first: the dimension that is folded away */
    uint32_t out_type, reserved;       /* value ops: SZ3HIP_FLOAT / SZ3HIP_DOUBLE, whatever the handle's type; 0 */
    double fill;                       /* a column without a finite point (MIN, MAX, MEAN): (Tout)fill; any double, not checked */
} sz3hip_project_opts;
typedef struct sz3hip_project_plan {   /* 48 bytes */
    uint32_t n; int32_t finest_level, coarsest_level, n_levels;
    uint64_t points, scratch_elems;    /* sz3hip_request_plan_for's */
    uint64_t out_points;               /* the sum over the boxes of points / ext[axis] */
    uint32_t out_elem_bytes, reserved; /* 4 or 8 */
} sz3hip_project_plan;
int sz3hip_project_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n,
                            const sz3hip_project_opts *opts, sz3hip_project_plan *out);
int sz3hip_stream_project(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_project_opts *opts, void *stream);
int sz3hip_project_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides_in,
                          const sz3hip_project_opts *opts, void *d_out, const int64_t *strides_out, void *stream);
/* ---- gradients of boxes: central differences, magnitude, vector ----
 * A gradient-magnitude transfer function, a shading normal, an edge or front detector: the derivative of a box along its axes.
 * sz3hip_stream_gradient takes sz3hip_stream_request's own sz3hip_tile_req, 1 .. SZ3HIP_MAX_BOXES boxes that each name their own level
 * (geometry, codes and wording are that call's, "box <i>: " in front; repeated and overlapping boxes are allowed; everything is checked
 * before anything is launched or written), and runs the same launch sequence with ONE differentiating launch in the strided gather's
 * place: stats.launches_last_request is the same boxes' sz3hip_stream_request's (a handle that keeps the full array: 1). It counts as a
 * request in sz3hip_stream_stats. One op and one set of options hold for the whole call.
 * The output of a box has the box's shape; under SZ3HIP_GRADIENT_INTERIOR the box loses its first and its last point along every
 *   differentiated axis (DERIV: `axis`; the other ops: all N), and such an extent must be at least 3. A caller who asks for a tile with a
 *   halo of one point gets the tile's own points, every one a central difference. The output element is Tout (out_type), for VECTOR N
 *   consecutive Tout, component j the derivative along axis j, slowest first. d_out and strides[] describe a view in OUTPUT ELEMENTS
 *   (sizeof(Tout), or N * sizeof(Tout) bytes), all N strides given (or none: contiguous); d_out is aligned to sizeof(Tout). The view rules
 *   and the overlap rule are the request's, applied to the output box with the output element's size.
 * The rule: v the values sz3hip_stream_request would deliver for the box, x = (double)v. Along axis a the box has extent E and the point
 *   sits at index i:
 *     ip = min(i + 1, E - 1), im = max(i, 1) - 1, s_a = ldexp(spacing[a], level)
 *     d_a = E == 1 ? +0.0 : (x[ip] - x[im]) / ((double)(ip - im) * s_a)
 *   — the two values differ in the index along a only; one subtraction, one multiplication and one division in IEEE double, nothing
 *   contracted; central inside the box, one-sided at its first and last point; only points of the box are read: numpy.gradient's
 *   edge_order=1 with a spacing that knows the level.
 *   DERIV: (Tout)d_axis. VECTOR: every (Tout)d_j. MAG2: m = 0.0; for a ascending: m = m + d_a * d_a; (Tout)m. MAG: (Tout)sqrt(m), the
 *   square root in double. Non-finite values get no special case (a NaN neighbour gives NaN, Inf - Inf gives NaN; a NaN output's sign and
 *   payload are not part of the contract); double -> float rounds to nearest even and may give Inf.
 * The output depends on the box's values, the box's level and the options alone — not on the route, the grid, the other boxes or the
 * handle's kind: sz3hip_stream_gradient is byte-identical to sz3hip_gradient_device over the same values with spacing pre-multiplied by
 * 2^level. No device-to-host copy, no host synchronisation beyond a request's own waits; no workspace.
 * Errors (SZ3HIP_EINVAL): opts NULL; op above SZ3HIP_GRADIENT_VECTOR; axis >= N, or not 0 with another op than DERIV; out_type above
 * SZ3HIP_DOUBLE; flag bits beyond SZ3HIP_GRADIENT_INTERIOR; a spacing[a], a < N, that is not finite and above 0, or whose s_a at some
 * box's level is not finite (entries at and beyond N are not read); INTERIOR with a differentiated extent below 3; d_out NULL or not
 * aligned to sizeof(Tout); the request's view and overlap cases on the output box; and sz3hip_stream_request's for the boxes. Integer
 * types: SZ3HIP_EUNSUPPORTED. A refused call launches and writes nothing, and the handle serves the next request.
 * sz3hip_gradient_device: the same gradient of ONE plain view in device memory at level 0 (what a handle that keeps the full array runs,
 * in one launch): N, dims, strides_in and d_in's rules are sz3hip_map_device's (x stride 2, stride-0 broadcasts and transposed views
 * included), the options checked before any pointer; d_out / strides_out: the view of the output box in output elements (strides_out
 * NULL: contiguous). Asynchronous on `stream`.
 * sz3hip_gradient_plan_for: a pure function (no device) with sz3hip_stream_gradient's checks. */
#define SZ3HIP_GRADIENT_DERIV  0u   /* the derivative along `axis` */
#define SZ3HIP_GRADIENT_MAG2   1u   /* the sum of the squared derivatives */
#define SZ3HIP_GRADIENT_MAG    2u   /* its square root */
#define SZ3HIP_GRADIENT_VECTOR 3u   /* all N derivatives, N consecutive Tout */
#define SZ3HIP_GRADIENT_INTERIOR 1u /* flags: drop the first and last point along every differentiated axis */
typedef struct sz3hip_gradient_opts {  /* 48 bytes */
    uint32_t op, axis;                 /* SZ3HIP_GRADIENT_*; 0 .. N-1, slowest first: read by DERIV only, 0 otherwise */
    uint32_t out_type, flags;          /* SZ3HIP_FLOAT / SZ3HIP_DOUBLE, whatever the handle's type; SZ3HIP_GRADIENT_INTERIOR or 0 */
    double spacing[4];                 /* the level-0 grid step per axis, N entries used: finite and above 0 */
} sz3hip_gradient_opts;
typedef struct sz3hip_gradient_plan {  /* 48 bytes */
    uint32_t n; int32_t finest_level, coarsest_level, n_levels;
    uint64_t points, scratch_elems;    /* sz3hip_request_plan_for's */
    uint64_t out_points;               /* output elements over the boxes, after INTERIOR */
    uint32_t out_elem_bytes, reserved; /* sizeof(Tout), times N for VECTOR */
} sz3hip_gradient_plan;
int sz3hip_gradient_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n,
                             const sz3hip_gradient_opts *opts, sz3hip_gradient_plan *out);
int sz3hip_stream_gradient(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_gradient_opts *opts, void *stream);
int sz3hip_gradient_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides_in,
                           const sz3hip_gradient_opts *opts, void *d_out, const int64_t *strides_out, void *stream);
/* ---- boxes composited along an axis: front to back through an RGBA table ----
 * The emission-absorption image of a brick: every column of a box folded front to back through a colour / opacity transfer function.
 * sz3hip_stream_composite takes sz3hip_stream_request's own sz3hip_tile_req, 1 .. SZ3HIP_MAX_BOXES boxes that each name their own level
 * (geometry, codes and wording are that call's, "box <i>: " in front; repeated and overlapping boxes are allowed; everything is checked
 * before anything is launched or written), and runs the same launch sequence with ONE compositing launch in the strided gather's place:
 * stats.launches_last_request is the same boxes' sz3hip_stream_request's (a handle that keeps the full array: 1). It counts as a request
 * in sz3hip_stream_stats. One set of options holds for the whole call.
 * The output of a box is the box with extent 1 along `axis` (keepdim): d_out and strides[] describe a view in OUTPUT elements, all N
 *   strides given (or none: contiguous); the stride at `axis` is not read, as the stride of any extent-1 dimension is not. The view
 *   rules, the alignment rule and the overlap rule are the request's, applied to that collapsed box with the output element's size.
 *   SZ3HIP_COMPOSITE_RGBA32F: an element is four floats r, g, b, a (16 bytes), d_out aligned to 16. The colours are PREMULTIPLIED by
 *   the opacity (the fold's sums as they are). SZ3HIP_COMPOSITE_RGBA8: 4 bytes, byte 0 = r .. byte 3 = a, d_out aligned to 4.
 * The table: d_lut, lut_n entries (2 .. SZ3HIP_MAX_LUT) of four floats r, g, b, a in device memory, 16-byte aligned. Its contents are not
 *   checked (as the map's are not): the rule is plain arithmetic on whatever is there.
 * The rule, bit-defined; all arithmetic is IEEE double, each operation rounded on its own, nothing contracted:
 *   1. The column of an output point is the box's values v_0 .. v_{E-1} along `axis` — exactly the values sz3hip_stream_request would
 *      deliver —, visited ascending, or descending under SZ3HIP_COMPOSITE_REVERSE, each taken as x = (double)v.
 *   2. A NaN point is skipped: it adds nothing and stops nothing. Any other point (+-Inf are ordinary values) has
 *        code = x < lo ? 0 : x >= hi ? M : min((uint64_t)((x - lo) * scale), M),   M = lut_n - 1, scale = (double)(M + 1) / (hi - lo)
 *      — the mapping's code (sz3hip_stream_map) to the letter.
 *   3. The entry at `code`: r, g, b, a widened to double (exact). The opacity after s squarings: a itself when s == 0, otherwise
 *        t = 1.0 - a; s times: t = t * t; a = 1.0 - t
 *      with s = level_bias + (SZ3HIP_COMPOSITE_LEVEL_OPACITY ? the box's level : 0): a level-k box steps 2^k times as far per sample.
 *      sz3hip_composite_device has no level: s = level_bias.
 *   4. The fold: the state (R, G, B, A) starts at +0.0 — under SZ3HIP_COMPOSITE_ACCUMULATE at the four floats already at the output
 *      element, widened. Per visited point, in this order:
 *        w = (1.0 - A) * a;  R = R + w * r;  G = G + w * g;  B = B + w * b;  A = A + w
 *      and after a point is folded the column stops if A >= cutoff (cutoff +Inf never stops).
 *   5. The store. RGBA32F: (float) of each, rounded to nearest even. RGBA8: per channel q = c * 255.0 + 0.5 and the byte is
 *        q > 0 ? (q >= 255 ? 255 : (uint8_t)q) : 0      (a NaN gives 0).
 * The output depends on the column, the box's level and the options alone — not on the route, the grid, the other boxes or the handle's
 * kind: sz3hip_stream_composite is byte-identical to sz3hip_composite_device over the same values with level_bias raised by the box's
 * level when LEVEL_OPACITY is set. A column composited in two consecutive boxes, the second under ACCUMULATE into the first's RGBA32F
 * output, is defined by the rule too; it is NOT byte-equal to the one-box result, because the carry passes through float. No
 * device-to-host copy, no host synchronisation beyond a request's own waits; no workspace.
 * Errors (SZ3HIP_EINVAL): opts NULL; out_type not one of the two; unknown flag bits; reserved not 0; axis >= N; lo or hi not finite,
 * hi <= lo, or hi - lo not finite; cutoff NaN or <= 0; lut_n outside 2 .. SZ3HIP_MAX_LUT; d_lut NULL or not 16-byte aligned; s > 30 at
 * some box's level; ACCUMULATE with RGBA8; d_out NULL or not aligned to the output element; the request's view and overlap cases on the
 * collapsed box; and sz3hip_stream_request's for the boxes. Integer types: SZ3HIP_EUNSUPPORTED. A refused call launches and writes
 * nothing, and the handle serves the next request.
 * sz3hip_composite_device: the same fold of ONE plain view in device memory (what a handle that keeps the full array runs, in one
 * launch): N, dims, strides_in and d_in's rules are sz3hip_map_device's (x stride 2, stride-0 broadcasts and transposed views included),
 * the options checked before any pointer; d_out / strides_out: the view of the collapsed array in output elements (strides_out NULL:
 * contiguous). Asynchronous on `stream`.
 * sz3hip_composite_plan_for: a pure function (no device) with sz3hip_stream_composite's checks. */
#define SZ3HIP_COMPOSITE_RGBA32F 0u
#define SZ3HIP_COMPOSITE_RGBA8   1u
#define SZ3HIP_COMPOSITE_REVERSE       1u /* flags: visit the column descending */
#define SZ3HIP_COMPOSITE_LEVEL_OPACITY 2u /*        a box of level k has its opacities squared k more times */
#define SZ3HIP_COMPOSITE_ACCUMULATE    4u /*        the fold starts at the output element's four floats (RGBA32F only) */
typedef struct sz3hip_composite_opts {  /* 56 bytes */
    double lo, hi;                      /* the window: finite, hi > lo */
    double cutoff;                      /* a column stops once A >= cutoff: above 0, +Inf never stops */
    uint32_t axis, out_type;            /* 0 .. N-1, slowest first: the dimension that is folded away; SZ3HIP_COMPOSITE_RGBA* */
    uint32_t flags, lut_n;              /* SZ3HIP_COMPOSITE_REVERSE | _LEVEL_OPACITY | _ACCUMULATE; 2 .. SZ3HIP_MAX_LUT */
    uint32_t level_bias, reserved;      /* squarings of every entry's 1 - a, 0 .. 30 together with the box's level; 0 */
    const void *d_lut;                  /* device, lut_n entries of four floats r, g, b, a; 16-byte aligned */
} sz3hip_composite_opts;
typedef struct sz3hip_composite_plan {  /* 48 bytes */
    uint32_t n; int32_t finest_level, coarsest_level, n_levels;
    uint64_t points, scratch_elems;     /* sz3hip_request_plan_for's */
    uint64_t out_points;                /* the sum over the boxes of points / ext[axis] */
    uint32_t out_elem_bytes, reserved;  /* 16 or 4 */
} sz3hip_composite_plan;
int sz3hip_composite_plan_for(const sz3hip_config *conf, int dataType, const sz3hip_tile_req *reqs, uint32_t n,
                              const sz3hip_composite_opts *opts, sz3hip_composite_plan *out);
int sz3hip_stream_composite(sz3hip_stream *h, const sz3hip_tile_req *reqs, uint32_t n, const sz3hip_composite_opts *opts, void *stream);
int sz3hip_composite_device(int dataType, int N, const uint64_t *dims, const void *d_in, const int64_t *strides_in,
                            const sz3hip_composite_opts *opts, void *d_out, const int64_t *strides_out, void *stream);
/* development switch, process-wide: a request of a handle runs its coarsest c levels in ONE launch (one workgroup per box walks first point,
 * regrids and passes with a barrier between steps), c the largest count such that for every box every pass of those levels has at most
 * `points` points. 0: off — the request issues exactly the launches sz3hip_decompress_device_tiles issues. Environment twin, read once when
 * the setter was never called: SZ3HIP_CHAIN_POINTS. The existing calls never take the chain. */
void sz3hip_debug_chain_points(uint32_t points);
uint32_t sz3hip_debug_get_chain_points(void);

/* diagnostics of the last compress on this ctx (valid after sz3hip_compress_finish) */
typedef struct sz3hip_stats {
    uint64_t n, n_value_outliers, n_delta_outliers, n_chunks, bitstream_bytes, payload_bytes;
    uint32_t n_symbols, max_code_len;
    uint32_t narrow_codes; /* 1 when stage 1 kept the intermediate codes as one byte each (internal, not a format property) */
    uint32_t reserved;
} sz3hip_stats;
int sz3hip_get_stats(sz3hip_ctx *ctx, sz3hip_stats *st);

/* what the ALGO_INTERP_LORENZO sampling auto-tuner (SZ_compress_Interp_lorenzo, api/impl/SZAlgoInterp.hpp:122-286) saw and
 * decided in the last sz3hip_compress_stage1 / sz3hip_compress_device call of this context */
typedef struct sz3hip_tuner_report {
    int32_t ran;        /* 1: the sampling trials ran; 0: skipped like the reference (:149-162, :176-179) or another cmprAlgo */
    int32_t use_interp; /* 1: interpolation chosen; 0: Lorenzo (possible in 1-D only, :232-250) */
    uint64_t sample_block_size, n_filtered, n_blocks;
    int32_t profiling;
    int32_t interpAlgo, interpDirection;
    int32_t speculated; /* 0: stage 1 waited for the tuner; 1: it had started with the previous call's outcome and the tuner confirmed it;
                         * 2: started, not confirmed, enqueued again with this call's outcome */
    double interpAlpha, interpBeta;
    double est_bytes[8]; /* priced size of the trials: linear, cubic, reversed direction, 3 x (alpha, beta), [6] Lorenzo (1-D),
                          * [7] Lorenzo with 16384 quantization bins (1-D, only when Lorenzo won: SZAlgoInterp.hpp:268-277) */
} sz3hip_tuner_report;
int sz3hip_get_tuner_report(sz3hip_ctx *ctx, sz3hip_tuner_report *rep);

/* per-stage kernel time of the last compress / decompress when profiling is on (hipEvents on `stream`):
 * names[i] / ms[i] for i < returned count; count 0 if profiling is off */
void sz3hip_set_profiling(sz3hip_ctx *ctx, int on);
int sz3hip_get_stage_times(sz3hip_ctx *ctx, const char **names, float *ms, int max);
/* What a context remembers between calls only ever changes the TIME of a call, never its payload: which form of a kernel the
 * previous call's data took, histogram windows, the auto-tuner's previous outcome (stage 1 starts with it beside the tuner) and
 * the previous code book (stage 2 packs with it while this call's is built by one workgroup of the same launch; finish() repeats
 * the encoder when the two differ and lets the next 1, 2, 4, 8 calls sit out). sz3hip_ctx_forget drops all of it: the next call
 * behaves like a context's first (bench.py's cold numbers). sz3hip_ctx_set_speculation(ctx, off): 0 on, 1 off, 2 on without the
 * back-off after a miss (tests); sz3hip_get_spec_stats counts the code-book speculation's hits / misses. */
void sz3hip_ctx_forget(sz3hip_ctx *ctx);
void sz3hip_ctx_set_speculation(sz3hip_ctx *ctx, int off);
/* Round 4: one exception to "never its payload", and the switch that removes it. The verdict on the previous call's code book
 * accepts it when it is a complete prefix code over this call's alphabet AND codes this call's symbols within 1/1024 of the size
 * this call's own book would give (the format stores code lengths, a decoder cannot tell): a series of similar but not identical
 * arrays keeps the shortcut, and a payload then depends on what the context coded before (its size by < 0.1 %, its decoded
 * values not at all). sz3hip_ctx_set_deterministic(ctx, 1): the previous book stands only when it IS this call's book — the
 * payload is a pure function of the input again (what the host API — sz3hip_compress, the CLI, the HDF5 filter — always sets;
 * the reference builds a tree per call, encoder/HuffmanEncoder.hpp:96-105). Default of a device context: 0.
 * Round 6: the streams this mattered most for no longer speculate at all. A Lorenzo stream (ALGO_LORENZO_REG with Lorenzo-1 alone,
 * ALGO_NOPRED) of an array of at least 2^22 elements in rows of whole 256-element segments (1-D ... 3-D) that turns out to have
 * one-byte codes is coded with a book built from a SAMPLE of the array (262 144 values at places the extents alone decide) — inside
 * stage 1's own launch once the context knows the stream's form, by a launch of its own otherwise. Sample and book are functions of
 * the input: such a payload is the same whatever the context coded before and whatever this switch says, in the time the speculative
 * path took on a hit (512^3 f32: 0.24 ms either way; 0.30 ms with this switch on before). Not for contexts whose histogram is
 * exchanged between the stages (sz3hip_histogram_ptr / sz3hip_ctx_set_histogram: the ranks share one book from the summed histogram).
 * The payload header's anchor_stride field of such a stream names the symbol that stands for a listed delta (sz3hip_format.h). */
void sz3hip_ctx_set_deterministic(sz3hip_ctx *ctx, int on);
/* Round 5: the ALGO_INTERP_LORENZO tuner's trials priced the reference's way. By default a trial is priced on the device from the
 * histogram of its codes (entropy + a model of the serialised tree: 0.2 ms per tuning, the reference's decision in about three of four
 * cases, a neighbouring (alpha, beta) otherwise). With this switch every trial is priced as interp_compress_test does
 * (api/impl/SZAlgoInterp.hpp:42-78): the trial kernel's per-element codes of all sampled blocks come to the host, are put into the order
 * the reference's decomposition emits them, coded with one Huffman tree built with the reference's own queue, serialised like its buffer and
 * compressed with ZSTD_compress at level 3 — est_bytes[0..5] of the tuner report are then the reference's own compressed sizes byte for
 * byte (same libzstd) and the decisions the reference's, at a few milliseconds per tuning (a host thread per trial). The 1-D Lorenzo
 * trials (est_bytes[6], [7]) are then walked on the host in the reference's own order and priced the same way. Where a trial cannot be
 * priced this way (an anchor stride that is no power of two) the tuning goes on with the estimates. The HOST API's contexts (sz3hip_compress, and through it
 * the C++ / C wrappers, the CLI, the HDF5 filter) have it ON by default — a caller of the reference's boundary gets the reference's
 * decisions; at no cost for arrays of 16 MB and more under an absolute bound: the tuner then runs from the host's copy of the array beside its copy to
 * the device (512^3 f32 host to host: 15.1 ms per call either way; SZ3HIP_NO_PRETUNE=1: inside stage 1 as before, 18.1) —, a device context (sz3hip_ctx_create)
 * OFF. Environment, read per call, for every context this function was never called on: SZ3HIP_TUNER_EXACT=1 on, =0 off. */
void sz3hip_ctx_set_tuner_exact(sz3hip_ctx *ctx, int on);
void sz3hip_get_spec_stats(const sz3hip_ctx *ctx, uint32_t *hits, uint32_t *misses);
/* 1 when the last finished compression of this context ran the fused stage 1 (round 4: a context whose previous call left a small
 * code book codes with it INSIDE the predictor kernel — one-byte codes, rows that are multiples of 256 elements, 1-D..3-D — and the
 * encoder only moves the rows' bit strings to their places; the verdict on the book is as for the unfused form, a miss repeats
 * the whole call in the two-pass form: the input must stay valid until sz3hip_compress_finish returns) */
int sz3hip_last_call_fused(const sz3hip_ctx *ctx);
/* 1 when the last finished compression of this context ran the 16-bit form of the one-byte stage-1 kernel (round 5: f32 data, 1-D ... 3-D
 * arrays, behind a call whose probe found every lattice value within +-2047 steps): same bytes out as the one-byte kernel at 13 instead
 * of 21 vector instructions per element. A lattice value beyond +-4095 (or a value that is not finite) voids the launch and the call is
 * repeated with the one-byte kernel (the input must stay valid until sz3hip_compress_finish returns, as for every one-launch form). */
int sz3hip_last_call_q16(const sz3hip_ctx *ctx);
/* opt in to (1) / out of (0, the default) that form for this context; SZ3HIP_FUSED=1 in the environment makes 1 the default of every
 * context created afterwards. It halves the encoder's HBM traffic (no code array) and is byte-identical to the two-pass form, but on
 * MI355X it measured slower ("Round 4: the single-pass encoder"): the default stays the two-pass form. */
void sz3hip_ctx_set_fused(sz3hip_ctx *ctx, int on);
/* 1: this library carries the superseded forms kept for reference — the fused stage 1 above and the decoder's multi-symbol table
 * (sz3hip_debug_flags(SZ3HIP_DBG_DEC_MULTI_SYM)) — i.e. it is the lab build (python -m sz3_amd.build --lab: sz3_amd/libsz3hip_lab.so). The product build
 * (libsz3hip.so) leaves them out: 0, and both switches do nothing. */
int sz3hip_lab_build(void);
/* test hooks: copy internal device arrays to host (quantisation codes as uint16, histogram as uint64) */
int sz3hip_debug_copy_codes(sz3hip_ctx *ctx, uint16_t *host_codes, uint64_t n);
/* test hook: which chain the last sz3hip_decompress_device took: out4[0] half-width intermediates, [1] rows that cross chunk
 * boundaries (carry pass), [2] calls left before the half-width chain is tried again after an overflow, [3] reserved */
int sz3hip_debug_decode_info(sz3hip_ctx *ctx, uint32_t *out4);
/* the last stock Huffman decode of this process: *passes = restart-point passes launched (0 if none),
   *route = 0 device, 1 host by the switch, 2 host after the pass cap, 3 single symbol (no bit stream) */
void sz3hip_debug_stock_huffman(int *passes, int *route);
/* the last block-stream decode of this process (predictor sets with Lorenzo-2 / regression): which decoder form ran, over how many
   slots, workgroups and tiles, and whether the retry was taken — out[enum sz3hip_blkdec_word], sz3hip_debug.h; all 0 before the first */
void sz3hip_debug_blkdec_last(uint32_t out[8]);
/* test hook: non-zero routes every shape through the generic (any-shape) stage-1 kernel instead of the tuned one */
void sz3hip_debug_force_generic(int on);
/* development switches (bit mask, process-wide; 0 = product behaviour): an OR of enum sz3hip_dbg, sz3hip_debug.h, which says what each bit gates */
void sz3hip_debug_flags(int flags);
/* The second word of development switches: an OR of enum sz3hip_dbg2 (include/sz3hip_debug.h). */
void sz3hip_debug_flags2(int flags);
/* Launches the encoder of the last stage 2 enqueued in this process, from the bits / segment pass to the packer (for tests). */
int sz3hip_last_encode_launches(void);

/* ---- (4) multi-GPU exchange over RCCL / xGMI ------------------------------------------------------------------- */
typedef struct sz3hip_comm sz3hip_comm;
#define SZ3HIP_COMM_ID_BYTES 128
/* one process, `ndev` GPUs (devices[i], or 0..ndev-1 when NULL; ndev <= 0: all visible): ncclCommInitAll. The
 * communicator has ndev members, all local. */
sz3hip_comm *sz3hip_comm_create_local(int ndev, const int *devices);
/* one process per GPU: rank 0 makes the id (ncclGetUniqueId), the launcher ships its SZ3HIP_COMM_ID_BYTES bytes to
 * every rank, each rank joins with its device (ncclCommInitRank). The communicator has one local member. */
int sz3hip_comm_unique_id(unsigned char *id128);
sz3hip_comm *sz3hip_comm_create_rank(int nranks, int rank, int device, const unsigned char *id128);
void sz3hip_comm_destroy(sz3hip_comm *comm);
int sz3hip_comm_size(const sz3hip_comm *comm);       /* ranks RCCL reports for the communicator */
int sz3hip_comm_rank(const sz3hip_comm *comm);       /* rank of this process's first member (0 for a local communicator) */
int sz3hip_comm_local_size(const sz3hip_comm *comm); /* members this process drives */
int sz3hip_comm_device(const sz3hip_comm *comm, int member);
/* Between stage1 and stage2: in-place sum all-reduce of the code histogram of ctxs[m] (one context per local member, on
 * that member's device), enqueued on streams[m] — stage2 on the same stream sees the global histogram, and every member
 * builds the same code book. Asynchronous. */
int sz3hip_comm_allreduce_histogram(sz3hip_comm *comm, sz3hip_ctx *const *ctxs, void *const *streams);
/* the same for any uint64 device buffers (d_bufs[m] on member m's device) */
int sz3hip_comm_allreduce_u64(sz3hip_comm *comm, void *const *d_bufs, size_t count, void *const *streams);
/* global value range for REL / PSNR / ABS_AND_REL / ABS_OR_REL bounds (api/impl/SZImplOMP.hpp:57-69): mins[m] / maxs[m]
 * hold member m's local pair on entry and the global pair on return (synchronises the streams) */
int sz3hip_comm_allreduce_minmax(sz3hip_comm *comm, double *mins, double *maxs, void *const *streams);


/* One process per GPU (communicator from sz3hip_comm_create_rank): this rank's share of SZ_compress_OMP. `global_conf`
 * describes the WHOLE array; rank r of G owns the slab [r*dims[0]/G, (r+1)*dims[0]/G) (SZImplOMP.hpp:48-50) and passes
 * a host pointer to that slab. Collective: every rank of the communicator must call it (value range for range-based
 * bounds, a status word, the code histogram). Writes this slab's blob — what the container stores for it — to `blob`
 * (capacity >= sz3hip_compress_bound of the slab's Config) and the slab's Config to *slab_conf; returns the blob size,
 * 0 on error (then on every rank). The launcher gathers blobs + Configs and rank 0 calls sz3hip_assemble_container. */
size_t sz3hip_compress_rank(sz3hip_comm *comm, const sz3hip_config *global_conf, int dataType, const void *slab_data,
                            char *blob, size_t cap, sz3hip_config *slab_conf);
/* [magic][version][u64 body][ i32 G | Config x G | u64 size x G | blob x G ][outer Config, openmp = 1] (api/sz.hpp:53-81
 * around SZImplOMP.hpp:100-107): the stream sz3hip_decompress / SZ_decompress<T> read back. Returns its size, 0 on error. */
size_t sz3hip_assemble_container(const sz3hip_config *global_conf, int dataType, int G, const sz3hip_config *slab_confs,
                                 const char *const *blobs, const size_t *blob_sizes, char *out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif

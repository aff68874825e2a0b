"""sz3_amd — host-side mirror of the SZ3 API for the MI355X (gfx950) hot path.

The product is the C-ABI shared library ``sz3_amd/libsz3hip.so`` (include/sz3hip.h, include/sz3c.h): predictor ->
quantizer -> Huffman as hand-written HIP kernels.  This module is a thin ctypes binding that mirrors the reference's
Python face ``pysz`` (tools/pysz/src/pysz/sz.pyx:185-405: ``sz.compress(ndarray, szConfig) -> (uint8 ndarray, ratio)``,
``sz.decompress(bytes, dtype, shape) -> (ndarray, szConfig)``, ``sz.verify -> (max_diff, psnr, nrmse)``) plus the
device-resident entry points used by bench.py and the multi-GPU driver.

There is no CPU implementation here: importing works anywhere, but every call needs the built library and a HIP
device and raises otherwise.
"""
import contextlib
import ctypes as C
import enum
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SZ3HIP_LIB") or os.path.join(_HERE, "libsz3hip.so")  # (SZ3HIP_LIB: A/B runs of two builds)

# include/SZ3/utils/Config.hpp:66,80,93 (enum EB / ALGO / INTERP_ALGO) + the GPU stream id (include/sz3hip.h)
EB_ABS, EB_REL, EB_PSNR, EB_L2NORM, EB_ABS_AND_REL, EB_ABS_OR_REL = range(6)
ALGO_LORENZO_REG, ALGO_INTERP_LORENZO, ALGO_INTERP, ALGO_NOPRED, ALGO_LOSSLESS = range(5)
ALGO_HIP_LORENZO = 16
ALGO_HIP_INTERP = 17
INTERP_ALGO_LINEAR, INTERP_ALGO_CUBIC = 0, 1
SZ_FLOAT, SZ_DOUBLE = 0, 1


class Dbg(enum.IntFlag):
    """The development switches of sz3hip_debug_flags: enum sz3hip_dbg of include/sz3hip_debug.h without the SZ3HIP_DBG_ prefix, same
    values (tests/test_debug_flags_cpu.py keeps the two equal). Members of equal value are one bit with several meanings: setting it
    switches all of them. The header says what each one gates."""
    CB_COMPACT_IN_WG = 1
    K1_LAB_NO_HIST = 1
    DEC_MULTI_SYM = 2
    K1_NO_CODE_STORES = 2
    BLKDEC_FORCE_RETRY = 4
    K1_V4_NO_STENCIL = 4
    K1_NO_Q16 = 8
    BLKDEC_LOCAL_EXPANDED = 16
    K1_V4_NO_PREFETCH = 16
    PACK_LAB_NO_STORES = 16
    K1_NO_MARCH = 32
    K1_NO_NARROW = 64
    INTERP_NO_VEC = 128
    K1_NO_WIDTH_SPEC = 256
    DEC_NO_FUSED_X = 512
    PACK_LAB_ONE_UNIT = 512
    CB_ONE_CLASS = 1024
    K1_NO_FUSED = 2048
    BLK_RANK_3_LAUNCHES = 2048
    BLK_SIDE_8_LAUNCHES = 2048
    K1_NO_XCD_ORDER = 4096
    CB_NO_SPEC_WIDE = 4096
    INTERP_HIST_BIG = 8192
    BLK_OFF = 16384
    PACK_OLD = 32768
    BLKDEC_GROUPS_3 = 32768
    CB_NO_SAMPLED = 65536
    BLKDEC_PER_FRONT = 65536
    CTX_NO_MEMORY = 131072
    CB_SERIAL_MERGE = 262144
    DEC_NO_STORES = 524288
    DEC_DIRECT_STORES = 1048576
    DEC_NO_HALF = 2097152
    INTERP_LEVELS_ANY_SIZE = 4194304
    K1_NO_SAMP_IN_LAUNCH = 4194304
    BLKDEC_BLOCK_PER_WAVE = 8388608
    K1_Q16_PLAIN_STORES = 8388608
    K1_NO_DEFER_FOLD = 16777216
    PACK_NO_SEG_BITS = 33554432
    BLK_FIT_TILES = 67108864
    BLK_1D_WAVE_PER_BLOCK = 134217728
    CTX_NO_PUBLISH_ZERO = 268435456
    INTERP_HANDOVER_IN_PLACE = 536870912
    DEC_CARRY_PASS = 536870912
    BLK_NO_EXIT = 1073741824
    BLK_NO_SELECT = 2147483648


class Dbg2(enum.IntFlag):
    """The second word of development switches (sz3hip_debug_flags2): enum sz3hip_dbg2 of include/sz3hip_debug.h without the
    SZ3HIP_DBG2_ prefix, same values. One bit, one meaning."""
    PACK_SCAN_LAUNCH = 1
    REQUEST_BY_LEVEL = 2
    MAP_PLAIN_STORES = 4


class BlkDecForm(enum.IntEnum):
    """The block decoder's forms (debug_blkdec_last): enum sz3hip_blkdec_form of include/sz3hip_debug.h without the
    SZ3HIP_BLKDEC_FORM_ prefix, same values."""
    NONE = 0
    FRONTS_4D = 1
    SCAN2_1D = 2
    WAVE_2D = 3
    SCAN_1D = 4
    FRONTS2_2D = 5
    GROUPS_2D = 6
    FRONTS_2D = 7
    WAVE_3D = 8
    GROUPS_3_3D = 9
    GROUPS_2_3D = 10
    FRONTS_3D = 11


class SZ3HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sz3hip error %d: %s" % (code, msg))
        self.code = code


class _CConfig(C.Structure):
    _fields_ = [
        ("N", C.c_int32), ("dims", C.c_uint64 * 4), ("num", C.c_uint64),
        ("cmprAlgo", C.c_uint8), ("errorBoundMode", C.c_uint8),
        ("absErrorBound", C.c_double), ("relErrorBound", C.c_double),
        ("psnrErrorBound", C.c_double), ("l2normErrorBound", C.c_double),
        ("openmp", C.c_uint8), ("quantbinCnt", C.c_int32), ("blockSize", C.c_int32),
        ("predDim", C.c_uint8), ("dataType", C.c_uint8),
        ("lorenzo", C.c_uint8), ("lorenzo2", C.c_uint8), ("regression", C.c_uint8), ("regression2", C.c_uint8),
        ("interpAlgo", C.c_uint8), ("interpDirection", C.c_uint8),
        ("interpAnchorStride", C.c_int32), ("interpAlpha", C.c_double), ("interpBeta", C.c_double),
    ]


class _CTunerReport(C.Structure):
    _fields_ = [("ran", C.c_int32), ("use_interp", C.c_int32), ("sample_block_size", C.c_uint64), ("n_filtered", C.c_uint64),
                ("n_blocks", C.c_uint64), ("profiling", C.c_int32), ("interpAlgo", C.c_int32), ("interpDirection", C.c_int32),
                ("speculated", C.c_int32), ("interpAlpha", C.c_double), ("interpBeta", C.c_double), ("est_bytes", C.c_double * 8)]


class _CStats(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_value_outliers", C.c_uint64), ("n_delta_outliers", C.c_uint64),
                ("n_chunks", C.c_uint64), ("bitstream_bytes", C.c_uint64), ("payload_bytes", C.c_uint64),
                ("n_symbols", C.c_uint32), ("max_code_len", C.c_uint32),
                ("narrow_codes", C.c_uint32), ("reserved", C.c_uint32)]


class _CRegionPlan(C.Structure):
    """sz3hip_region_plan (include/sz3hip.h)"""
    _fields_ = [("n_levels", C.c_int32), ("stride", C.c_uint32 * 32), ("win_lo", (C.c_uint64 * 4) * 32), ("win_hi", (C.c_uint64 * 4) * 32),
                ("points", C.c_uint64), ("scratch_elems", C.c_uint64)]


class _CTilePlan(C.Structure):
    """sz3hip_tile_plan (include/sz3hip.h)"""
    _fields_ = [("region", _CRegionPlan), ("units_total", C.c_uint64), ("units_needed", C.c_uint64)]


class _CBox(C.Structure):
    """sz3hip_box (include/sz3hip.h)"""
    _fields_ = [("lo", C.c_uint64 * 4), ("ext", C.c_uint64 * 4)]


class _CTilesPlan(C.Structure):
    """sz3hip_tiles_plan (include/sz3hip.h)"""
    _fields_ = [("n_boxes", C.c_uint32), ("n_levels", C.c_int32), ("points", C.c_uint64), ("scratch_elems", C.c_uint64), ("units_total", C.c_uint64),
                ("units_needed", C.c_uint64)]


class _CTileReq(C.Structure):
    """sz3hip_tile_req (include/sz3hip.h)"""
    _fields_ = [("level", C.c_int32), ("reserved", C.c_uint32), ("box", _CBox), ("d_out", C.c_void_p), ("strides", C.c_int64 * 4)]


class _CRequestPlan(C.Structure):
    """sz3hip_request_plan (include/sz3hip.h)"""
    _fields_ = [("n", C.c_uint32), ("finest_level", C.c_int32), ("coarsest_level", C.c_int32), ("n_levels", C.c_int32), ("points", C.c_uint64),
                ("scratch_elems", C.c_uint64)]


class _CReduceReq(C.Structure):
    # sz3hip_reduce_req (include/sz3hip.h)
    _fields_ = [("level", C.c_int32), ("reserved", C.c_uint32), ("box", _CBox)]


class _CReduceOpts(C.Structure):
    # sz3hip_reduce_opts
    _fields_ = [("nbins", C.c_uint32), ("reserved", C.c_uint32), ("lo", C.c_double), ("hi", C.c_double)]


class _CBoxStats(C.Structure):
    # sz3hip_box_stats: eleven 64-bit words
    _fields_ = ([(k, C.c_uint64) for k in ("n", "n_nonfinite", "argmin", "argmax")] +
                [(k, C.c_double) for k in ("min", "max", "shift", "sum", "sum_sq", "mean", "variance")])


class _CReducePlan(C.Structure):
    # sz3hip_reduce_plan
    _fields_ = [("n", C.c_uint32), ("finest_level", C.c_int32), ("coarsest_level", C.c_int32), ("n_levels", C.c_int32), ("points", C.c_uint64),
                ("scratch_elems", C.c_uint64), ("partials", C.c_uint64), ("hist_words", C.c_uint64)]


class _CSelectReq(C.Structure):
    # sz3hip_select_req (include/sz3hip.h)
    _fields_ = [("level", C.c_int32), ("reserved", C.c_uint32), ("box", _CBox), ("d_index", C.c_void_p), ("d_value", C.c_void_p), ("capacity", C.c_uint64)]


class _CSelectOpts(C.Structure):
    # sz3hip_select_opts
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class _CSelectHead(C.Structure):
    # sz3hip_select_head: four 64-bit words
    _fields_ = [(k, C.c_uint64) for k in ("n", "count", "written", "capacity")]


class _CSelectPlan(C.Structure):
    # sz3hip_select_plan
    _fields_ = [("n", C.c_uint32), ("finest_level", C.c_int32), ("coarsest_level", C.c_int32), ("n_levels", C.c_int32), ("points", C.c_uint64),
                ("scratch_elems", C.c_uint64), ("partials", C.c_uint64)]


class _CMapOpts(C.Structure):
    # sz3hip_map_opts: 48 bytes
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("out_type", C.c_uint32), ("flags", C.c_uint32), ("nan_code", C.c_uint32), ("lut_n", C.c_uint32),
                ("d_lut", C.c_void_p), ("reserved", C.c_uint64)]


class _CMapPlan(C.Structure):
    # sz3hip_map_plan
    _fields_ = [("n", C.c_uint32), ("finest_level", C.c_int32), ("coarsest_level", C.c_int32), ("n_levels", C.c_int32), ("points", C.c_uint64),
                ("scratch_elems", C.c_uint64), ("out_elem_bytes", C.c_uint64)]


class _CSampleReq(C.Structure):
    # sz3hip_sample_req: 248 bytes
    _fields_ = [("level", C.c_int32), ("reserved", C.c_uint32), ("box", _CBox), ("d_coords", C.c_void_p), ("d_out", C.c_void_p), ("n_points", C.c_uint64),
                ("counts", C.c_uint64 * 3), ("origin", C.c_double * 4), ("steps", (C.c_double * 4) * 3)]


class _CSampleOpts(C.Structure):
    # sz3hip_sample_opts: 24 bytes
    _fields_ = [("filter", C.c_uint32), ("coord_type", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("fill", C.c_double)]


class _CSamplePlan(C.Structure):
    # sz3hip_sample_plan
    _fields_ = [("n", C.c_uint32), ("finest_level", C.c_int32), ("coarsest_level", C.c_int32), ("n_levels", C.c_int32), ("points", C.c_uint64),
                ("scratch_elems", C.c_uint64), ("queries", C.c_uint64)]


class _CProjectOpts(C.Structure):
    # sz3hip_project_opts: 24 bytes
    _fields_ = [("op", C.c_uint32), ("axis", C.c_uint32), ("out_type", C.c_uint32), ("reserved", C.c_uint32), ("fill", C.c_double)]


class _CProjectPlan(C.Structure):
    # sz3hip_project_plan: 48 bytes
    _fields_ = [("n", C.c_uint32), ("finest_level", C.c_int32), ("coarsest_level", C.c_int32), ("n_levels", C.c_int32), ("points", C.c_uint64),
                ("scratch_elems", C.c_uint64), ("out_points", C.c_uint64), ("out_elem_bytes", C.c_uint32), ("reserved", C.c_uint32)]


class _CGradientOpts(C.Structure):
    # sz3hip_gradient_opts: 48 bytes
    _fields_ = [("op", C.c_uint32), ("axis", C.c_uint32), ("out_type", C.c_uint32), ("flags", C.c_uint32), ("spacing", C.c_double * 4)]


class _CGradientPlan(C.Structure):
    # sz3hip_gradient_plan: 48 bytes
    _fields_ = [("n", C.c_uint32), ("finest_level", C.c_int32), ("coarsest_level", C.c_int32), ("n_levels", C.c_int32), ("points", C.c_uint64),
                ("scratch_elems", C.c_uint64), ("out_points", C.c_uint64), ("out_elem_bytes", C.c_uint32), ("reserved", C.c_uint32)]


class _CCompositeOpts(C.Structure):
    # sz3hip_composite_opts: 56 bytes
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("cutoff", C.c_double), ("axis", C.c_uint32), ("out_type", C.c_uint32), ("flags", C.c_uint32),
                ("lut_n", C.c_uint32), ("level_bias", C.c_uint32), ("reserved", C.c_uint32), ("d_lut", C.c_void_p)]


class _CCompositePlan(C.Structure):
    # sz3hip_composite_plan: 48 bytes
    _fields_ = [("n", C.c_uint32), ("finest_level", C.c_int32), ("coarsest_level", C.c_int32), ("n_levels", C.c_int32), ("points", C.c_uint64),
                ("scratch_elems", C.c_uint64), ("out_points", C.c_uint64), ("out_elem_bytes", C.c_uint32), ("reserved", C.c_uint32)]


class _CStreamStats(C.Structure):
    """struct sz3hip_stream_stats (include/sz3hip.h)"""
    _fields_ = [("fast", C.c_uint32), ("huffman_stages", C.c_uint32), ("launches_last_request", C.c_uint32), ("chain_levels_last_request", C.c_uint32),
                ("units_total", C.c_uint64), ("requests", C.c_uint64), ("scratch_elems", C.c_uint64), ("resident_bytes", C.c_uint64),
                ("n_levels_last_request", C.c_uint32), ("chain_points", C.c_uint32)]


class _CVerifyStats(C.Structure):
    """sz3hip_verify_stats (include/sz3hip.h)"""
    _fields_ = ([(k, C.c_uint64) for k in ("n", "n_nonfinite", "n_nonfinite_mismatch", "n_over", "first_over", "argmax")] +
                [(k, C.c_double) for k in ("min", "max", "max_diff", "max_pw_rel", "sum_ori", "sum_dec", "sum_sq_err", "sum_sq_dec",
                                           "psnr", "nrmse", "l2_err", "l2_err_norm", "acEff")])


_lib = None


def _share_torch_hip_runtime():
    """A process must hold ONE HIP runtime. PyTorch-ROCm wheels bundle their own libamdhip64 (found by rpath): when this library
    is loaded first it brings the system's copy in, and a later `import torch` + first CUDA call then finds "No HIP GPUs" — two
    runtimes cannot share the device. If a torch with a bundled runtime is installed, that copy is loaded first (by path, without
    importing torch), so that whoever comes second binds to it; torch-first already worked that way (same soname)."""
    try:
        import importlib.util
        import sys
        if "torch" in sys.modules:
            return
        # An `import torch` that comes AFTER this library has been at work on the device (contexts, streams, kernels launched) stalled
        # for good in about one fresh process out of five on the MI355X boxes — inside torch/__init__'s load of its C extension, i.e.
        # while torch's bundled libraries register their code objects with a HIP runtime that is already busy (caught with pytest's
        # faulthandler_timeout, round 4). The cure is the ORDER — torch first — and it is the caller's to keep: programs that use
        # torch beside this package import it before the first call (tests/conftest.py, bench.py, sz3_amd.distributed do), or set
        # SZ3HIP_TORCH_PRELOAD=1 and have it imported here. By default only the runtime library is preloaded: a host that never
        # touches torch (the CLI, the HDF5 filter under h5py, CPU-side tools) does not pay torch's import or its runtime initialisation.
        if os.environ.get("SZ3HIP_TORCH_PRELOAD", "0") == "1":
            try:
                import torch  # noqa: F401
                return
            except Exception:  # noqa: BLE001 - no usable torch: fall through to the runtime library alone
                pass
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        _warn_on_late_torch_import(sys)
        libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
        for name in ("libamdhip64.so",):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:  # noqa: BLE001 - best effort: without it the library still works, only torch-after-us does not
        pass


class _LateTorchImport:
    """sys.meta_path entry that finds nothing: it only notices the first `import torch` that comes after this library has been loaded
    (the hazard described in _share_torch_hip_runtime) and says so once — the caller can then fix the order instead of meeting an
    intermittent hang."""
    warned = False

    def find_spec(self, name, path=None, target=None):
        if name == "torch" and not _LateTorchImport.warned and _lib is not None:
            _LateTorchImport.warned = True
            import warnings
            warnings.warn("`import torch` after sz3_amd has loaded libsz3hip.so: on MI355X boxes this order stalled inside torch's import in "
                          "about one fresh process out of five once the device had been used. Import torch before the first sz3_amd call, "
                          "or set SZ3HIP_TORCH_PRELOAD=1.", RuntimeWarning, stacklevel=2)
        return None


def _warn_on_late_torch_import(sys):
    if not any(isinstance(f, _LateTorchImport) for f in sys.meta_path):
        sys.meta_path.insert(0, _LateTorchImport())


def lib():
    """Loads libsz3hip.so; fails loudly when it has not been built (python -m sz3_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("sz3_amd/libsz3hip.so is missing — build it with `python -m sz3_amd.build` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    _share_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.sz3hip_last_error.restype = C.c_char_p
    L.sz3hip_version.restype = C.c_char_p
    L.sz3hip_config_init.argtypes = [P(_CConfig), C.c_int, P(C.c_uint64)]
    L.sz3hip_config_save.restype = C.c_size_t
    L.sz3hip_config_save.argtypes = [P(_CConfig), C.c_void_p]
    L.sz3hip_config_load.restype = C.c_size_t
    L.sz3hip_config_load.argtypes = [P(_CConfig), C.c_void_p]
    L.sz3hip_compress_bound.restype = C.c_size_t
    L.sz3hip_compress_bound.argtypes = [P(_CConfig), C.c_int]
    L.sz3hip_compress.restype = C.c_size_t
    L.sz3hip_compress.argtypes = [P(_CConfig), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    L.sz3hip_decompress.restype = C.c_int
    L.sz3hip_decompress.argtypes = [P(_CConfig), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.sz3hip_peek_config.restype = C.c_int
    L.sz3hip_compress_from_device.restype = C.c_size_t
    L.sz3hip_compress_from_device.argtypes = [P(_CConfig), C.c_int, C.c_void_p, P(C.c_int64), C.c_void_p, C.c_size_t, C.c_void_p]
    L.sz3hip_decompress_to_device.restype = C.c_int
    L.sz3hip_decompress_to_device.argtypes = [P(_CConfig), C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, P(C.c_int64), C.c_void_p]
    L.sz3hip_peek_config.argtypes = [P(_CConfig), C.c_void_p, C.c_size_t]
    L.sz3hip_coarse_dims.restype = C.c_int
    L.sz3hip_coarse_dims.argtypes = [P(_CConfig), C.c_int, P(C.c_uint64)]
    L.sz3hip_decompress_coarse_to_device.restype = C.c_int
    L.sz3hip_decompress_coarse_to_device.argtypes = [P(_CConfig), C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, P(C.c_int64), C.c_void_p]
    L.sz3hip_decompress_device_coarse.restype = C.c_int
    L.sz3hip_decompress_device_coarse.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    L.sz3hip_region_plan_for.restype = C.c_int
    L.sz3hip_region_plan_for.argtypes = [P(_CConfig), P(C.c_uint64), P(C.c_uint64), P(_CRegionPlan)]
    L.sz3hip_decompress_region_to_device.restype = C.c_int
    L.sz3hip_decompress_region_to_device.argtypes = [P(_CConfig), C.c_int, C.c_void_p, C.c_size_t, P(C.c_uint64), P(C.c_uint64), C.c_void_p, P(C.c_int64),
                                                     C.c_void_p]
    L.sz3hip_decompress_device_region.restype = C.c_int
    L.sz3hip_decompress_device_region.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, P(C.c_uint64), P(C.c_uint64), C.c_void_p, C.c_void_p]
    L.sz3hip_tile_plan_for.restype = C.c_int
    L.sz3hip_tile_plan_for.argtypes = [P(_CConfig), C.c_int, P(C.c_uint64), P(C.c_uint64), P(_CTilePlan)]
    L.sz3hip_tile_units_for.restype = C.c_int
    L.sz3hip_tile_units_for.argtypes = [P(_CConfig), C.c_int, P(C.c_uint64), P(C.c_uint64), C.c_void_p, C.c_uint64, P(C.c_uint64)]
    L.sz3hip_decompress_tile_to_device.restype = C.c_int
    L.sz3hip_decompress_tile_to_device.argtypes = [P(_CConfig), C.c_int, C.c_void_p, C.c_size_t, C.c_int, P(C.c_uint64), P(C.c_uint64), C.c_void_p,
                                                   P(C.c_int64), C.c_void_p]
    L.sz3hip_decompress_device_tile.restype = C.c_int
    L.sz3hip_decompress_device_tile.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, P(C.c_uint64), P(C.c_uint64), C.c_void_p, C.c_void_p]
    L.sz3hip_set_sparse_decode.restype = None
    L.sz3hip_set_sparse_decode.argtypes = [C.c_int]
    L.sz3hip_get_sparse_decode.restype = C.c_int
    L.sz3hip_get_sparse_decode.argtypes = []
    L.sz3hip_tiles_plan_for.restype = C.c_int
    L.sz3hip_tiles_plan_for.argtypes = [P(_CConfig), C.c_int, P(_CBox), C.c_uint32, P(_CTilesPlan)]
    L.sz3hip_decompress_tiles_to_device.restype = C.c_int
    L.sz3hip_decompress_tiles_to_device.argtypes = [P(_CConfig), C.c_int, C.c_void_p, C.c_size_t, C.c_int, P(_CBox), C.c_uint32, P(C.c_void_p), C.c_void_p]
    L.sz3hip_decompress_device_tiles.restype = C.c_int
    L.sz3hip_decompress_device_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, P(_CBox), C.c_uint32, P(C.c_void_p), C.c_void_p]
    L.sz3hip_debug_region_launches.restype = C.c_uint64
    L.sz3hip_debug_region_launches.argtypes = []
    L.sz3hip_debug_tile_units.restype = None
    L.sz3hip_debug_tile_units.argtypes = [P(C.c_uint64), P(C.c_uint64)]
    L.sz3hip_debug_blkdec_last.restype = None
    L.sz3hip_debug_blkdec_last.argtypes = [P(C.c_uint32)]
    L.sz3hip_debug_stock_huffman.restype = None
    L.sz3hip_debug_stock_huffman.argtypes = [P(C.c_int), P(C.c_int)]
    L.sz3hip_debug_region_fast_calls.restype = C.c_uint64
    L.sz3hip_debug_region_fast_calls.argtypes = []
    L.sz3hip_debug_region_scratch.restype = C.c_uint64
    L.sz3hip_debug_region_scratch.argtypes = [C.c_void_p]
    L.sz3hip_stream_open.restype = C.c_int
    L.sz3hip_stream_open.argtypes = [P(C.c_void_p), P(_CConfig), C.c_int, C.c_void_p, C.c_size_t, C.c_int]
    L.sz3hip_stream_open_payload.restype = C.c_int
    L.sz3hip_stream_open_payload.argtypes = [P(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.sz3hip_stream_config.restype = C.c_int
    L.sz3hip_stream_config.argtypes = [C.c_void_p, P(_CConfig)]
    L.sz3hip_stream_tiles.restype = C.c_int
    L.sz3hip_stream_tiles.argtypes = [C.c_void_p, C.c_int, P(_CBox), C.c_uint32, P(C.c_void_p), C.c_void_p]
    L.sz3hip_stream_stats.restype = C.c_int
    L.sz3hip_stream_stats.argtypes = [C.c_void_p, P(_CStreamStats)]
    L.sz3hip_stream_request.restype = C.c_int
    L.sz3hip_stream_request.argtypes = [C.c_void_p, P(_CTileReq), C.c_uint32, C.c_void_p]
    L.sz3hip_reduce_plan_for.restype = C.c_int
    L.sz3hip_reduce_plan_for.argtypes = [P(_CConfig), C.c_int, P(_CReduceReq), C.c_uint32, P(_CReduceOpts), P(_CReducePlan)]
    L.sz3hip_stream_reduce.restype = C.c_int
    L.sz3hip_stream_reduce.argtypes = [C.c_void_p, P(_CReduceReq), C.c_uint32, P(_CReduceOpts), C.c_void_p, C.c_void_p, C.c_void_p]
    L.sz3hip_reduce_device.restype = C.c_int
    L.sz3hip_reduce_device.argtypes = [C.c_int, C.c_int, P(C.c_uint64), C.c_void_p, P(C.c_int64), P(_CReduceOpts), C.c_void_p, C.c_void_p, C.c_void_p]
    L.sz3hip_select_plan_for.restype = C.c_int
    L.sz3hip_select_plan_for.argtypes = [P(_CConfig), C.c_int, P(_CSelectReq), C.c_uint32, P(_CSelectOpts), P(_CSelectPlan)]
    L.sz3hip_stream_select.restype = C.c_int
    L.sz3hip_stream_select.argtypes = [C.c_void_p, P(_CSelectReq), C.c_uint32, P(_CSelectOpts), C.c_void_p, C.c_void_p]
    L.sz3hip_select_device.restype = C.c_int
    L.sz3hip_select_device.argtypes = [C.c_int, C.c_int, P(C.c_uint64), C.c_void_p, P(C.c_int64), P(_CSelectOpts), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                       C.c_void_p]
    L.sz3hip_map_plan_for.restype = C.c_int
    L.sz3hip_map_plan_for.argtypes = [P(_CConfig), C.c_int, P(_CTileReq), C.c_uint32, P(_CMapOpts), P(_CMapPlan)]
    L.sz3hip_stream_map.restype = C.c_int
    L.sz3hip_stream_map.argtypes = [C.c_void_p, P(_CTileReq), C.c_uint32, P(_CMapOpts), C.c_void_p]
    L.sz3hip_map_device.restype = C.c_int
    L.sz3hip_map_device.argtypes = [C.c_int, C.c_int, P(C.c_uint64), C.c_void_p, P(C.c_int64), P(_CMapOpts), C.c_void_p, P(C.c_int64), C.c_void_p]
    L.sz3hip_sample_plan_for.restype = C.c_int
    L.sz3hip_sample_plan_for.argtypes = [P(_CConfig), C.c_int, P(_CSampleReq), C.c_uint32, P(_CSampleOpts), P(_CSamplePlan)]
    L.sz3hip_stream_sample.restype = C.c_int
    L.sz3hip_stream_sample.argtypes = [C.c_void_p, P(_CSampleReq), C.c_uint32, P(_CSampleOpts), C.c_void_p]
    L.sz3hip_sample_device.restype = C.c_int
    L.sz3hip_sample_device.argtypes = [C.c_int, C.c_int, P(C.c_uint64), C.c_void_p, P(C.c_int64), P(_CSampleOpts), P(_CSampleReq), C.c_void_p]
    L.sz3hip_project_plan_for.restype = C.c_int
    L.sz3hip_project_plan_for.argtypes = [P(_CConfig), C.c_int, P(_CTileReq), C.c_uint32, P(_CProjectOpts), P(_CProjectPlan)]
    L.sz3hip_stream_project.restype = C.c_int
    L.sz3hip_stream_project.argtypes = [C.c_void_p, P(_CTileReq), C.c_uint32, P(_CProjectOpts), C.c_void_p]
    L.sz3hip_project_device.restype = C.c_int
    L.sz3hip_project_device.argtypes = [C.c_int, C.c_int, P(C.c_uint64), C.c_void_p, P(C.c_int64), P(_CProjectOpts), C.c_void_p, P(C.c_int64), C.c_void_p]
    L.sz3hip_gradient_plan_for.restype = C.c_int
    L.sz3hip_gradient_plan_for.argtypes = [P(_CConfig), C.c_int, P(_CTileReq), C.c_uint32, P(_CGradientOpts), P(_CGradientPlan)]
    L.sz3hip_stream_gradient.restype = C.c_int
    L.sz3hip_stream_gradient.argtypes = [C.c_void_p, P(_CTileReq), C.c_uint32, P(_CGradientOpts), C.c_void_p]
    L.sz3hip_gradient_device.restype = C.c_int
    L.sz3hip_gradient_device.argtypes = [C.c_int, C.c_int, P(C.c_uint64), C.c_void_p, P(C.c_int64), P(_CGradientOpts), C.c_void_p, P(C.c_int64), C.c_void_p]
    L.sz3hip_composite_plan_for.restype = C.c_int
    L.sz3hip_composite_plan_for.argtypes = [P(_CConfig), C.c_int, P(_CTileReq), C.c_uint32, P(_CCompositeOpts), P(_CCompositePlan)]
    L.sz3hip_stream_composite.restype = C.c_int
    L.sz3hip_stream_composite.argtypes = [C.c_void_p, P(_CTileReq), C.c_uint32, P(_CCompositeOpts), C.c_void_p]
    L.sz3hip_composite_device.restype = C.c_int
    L.sz3hip_composite_device.argtypes = [C.c_int, C.c_int, P(C.c_uint64), C.c_void_p, P(C.c_int64), P(_CCompositeOpts), C.c_void_p, P(C.c_int64), C.c_void_p]
    L.sz3hip_request_plan_for.restype = C.c_int
    L.sz3hip_request_plan_for.argtypes = [P(_CConfig), C.c_int, P(_CTileReq), C.c_uint32, P(_CRequestPlan)]
    L.sz3hip_stream_close.restype = None
    L.sz3hip_stream_close.argtypes = [C.c_void_p]
    L.sz3hip_debug_chain_points.restype = None
    L.sz3hip_debug_chain_points.argtypes = [C.c_uint32]
    L.sz3hip_debug_get_chain_points.restype = C.c_uint32
    L.sz3hip_debug_get_chain_points.argtypes = []
    L.sz3hip_verify_device.restype = C.c_int
    L.sz3hip_verify_device.argtypes = [C.c_int, C.c_int, P(C.c_uint64), C.c_void_p, P(C.c_int64), C.c_void_p, P(C.c_int64), C.c_double,
                                       P(_CVerifyStats), C.c_void_p]
    L.sz3hip_ctx_create.restype = C.c_void_p
    L.sz3hip_ctx_create.argtypes = [C.c_int, C.c_uint64, C.c_int]
    L.sz3hip_ctx_destroy.argtypes = [C.c_void_p]
    L.sz3hip_payload_bound.restype = C.c_size_t
    L.sz3hip_payload_bound.argtypes = [C.c_void_p, C.c_uint64]
    L.sz3hip_payload_bound_max.restype = C.c_size_t
    L.sz3hip_payload_bound_max.argtypes = [C.c_void_p, C.c_uint64]
    L.sz3hip_minmax_device.restype = C.c_int
    L.sz3hip_minmax_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_double), P(C.c_double), C.c_void_p]
    L.sz3hip_compress_stage1.restype = C.c_int
    L.sz3hip_compress_stage1.argtypes = [C.c_void_p, P(_CConfig), C.c_void_p, C.c_void_p]
    L.sz3hip_histogram_ptr.restype = C.c_void_p
    L.sz3hip_histogram_ptr.argtypes = [C.c_void_p]
    L.sz3hip_histogram_len.restype = C.c_size_t
    L.sz3hip_histogram_len.argtypes = [C.c_void_p]
    L.sz3hip_ctx_set_histogram.restype = C.c_int
    L.sz3hip_ctx_set_histogram.argtypes = [C.c_void_p, C.c_void_p]
    L.sz3hip_compress_stage2.restype = C.c_int
    L.sz3hip_compress_stage2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.sz3hip_compress_finish.restype = C.c_int
    L.sz3hip_compress_finish.argtypes = [C.c_void_p, P(C.c_size_t), C.c_void_p]
    L.sz3hip_compress_device.restype = C.c_int
    L.sz3hip_compress_device.argtypes = [C.c_void_p, P(_CConfig), C.c_void_p, C.c_void_p, C.c_size_t, P(C.c_size_t), C.c_void_p]
    L.sz3hip_decompress_device.restype = C.c_int
    L.sz3hip_decompress_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.sz3hip_get_stats.restype = C.c_int
    L.sz3hip_get_stats.argtypes = [C.c_void_p, P(_CStats)]
    L.sz3hip_get_tuner_report.restype = C.c_int
    L.sz3hip_get_tuner_report.argtypes = [C.c_void_p, P(_CTunerReport)]
    L.sz3hip_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.sz3hip_ctx_forget.argtypes = [C.c_void_p]
    L.sz3hip_ctx_forget.restype = None
    L.sz3hip_ctx_set_speculation.argtypes = [C.c_void_p, C.c_int]
    L.sz3hip_ctx_set_speculation.restype = None
    L.sz3hip_ctx_set_deterministic.argtypes = [C.c_void_p, C.c_int]
    L.sz3hip_ctx_set_deterministic.restype = None
    L.sz3hip_ctx_set_tuner_exact.argtypes = [C.c_void_p, C.c_int]
    L.sz3hip_ctx_set_tuner_exact.restype = None
    L.sz3hip_set_stock_format.argtypes = [C.c_int]
    L.sz3hip_set_stock_format.restype = None
    L.sz3hip_last_call_fused.argtypes = [C.c_void_p]
    L.sz3hip_last_call_fused.restype = C.c_int
    L.sz3hip_last_call_q16.argtypes = [C.c_void_p]
    L.sz3hip_last_call_q16.restype = C.c_int
    L.sz3hip_ctx_set_fused.argtypes = [C.c_void_p, C.c_int]
    L.sz3hip_ctx_set_fused.restype = None
    L.sz3hip_get_spec_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.sz3hip_get_spec_stats.restype = None
    L.sz3hip_payload_bound_conf.restype = C.c_size_t
    L.sz3hip_payload_bound_conf.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.sz3hip_get_stage_times.restype = C.c_int
    L.sz3hip_get_stage_times.argtypes = [C.c_void_p, P(C.c_char_p), P(C.c_float), C.c_int]
    L.sz3hip_debug_copy_codes.restype = C.c_int
    L.sz3hip_debug_copy_codes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.sz3hip_debug_force_generic.argtypes = [C.c_int]
    L.sz3hip_config_load_n.restype = C.c_size_t
    L.sz3hip_config_load_n.argtypes = [P(_CConfig), C.c_void_p, C.c_size_t]
    L.sz3hip_comm_create_local.restype = C.c_void_p
    L.sz3hip_comm_create_local.argtypes = [C.c_int, P(C.c_int)]
    L.sz3hip_comm_unique_id.restype = C.c_int
    L.sz3hip_comm_unique_id.argtypes = [C.c_void_p]
    L.sz3hip_comm_create_rank.restype = C.c_void_p
    L.sz3hip_comm_create_rank.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.sz3hip_comm_destroy.argtypes = [C.c_void_p]
    for f in ("size", "rank", "local_size"):
        getattr(L, "sz3hip_comm_" + f).restype = C.c_int
        getattr(L, "sz3hip_comm_" + f).argtypes = [C.c_void_p]
    L.sz3hip_comm_device.restype = C.c_int
    L.sz3hip_comm_device.argtypes = [C.c_void_p, C.c_int]
    L.sz3hip_comm_allreduce_histogram.restype = C.c_int
    L.sz3hip_comm_allreduce_histogram.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_void_p)]
    L.sz3hip_comm_allreduce_u64.restype = C.c_int
    L.sz3hip_comm_allreduce_u64.argtypes = [C.c_void_p, P(C.c_void_p), C.c_size_t, P(C.c_void_p)]
    L.sz3hip_comm_allreduce_minmax.restype = C.c_int
    L.sz3hip_comm_allreduce_minmax.argtypes = [C.c_void_p, P(C.c_double), P(C.c_double), P(C.c_void_p)]
    L.sz3hip_compress_rank.restype = C.c_size_t
    L.sz3hip_compress_rank.argtypes = [C.c_void_p, P(_CConfig), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, P(_CConfig)]
    L.sz3hip_assemble_container.restype = C.c_size_t
    L.sz3hip_assemble_container.argtypes = [P(_CConfig), C.c_int, C.c_int, P(_CConfig), P(C.c_void_p), P(C.c_size_t), C.c_void_p, C.c_size_t]
    L.SZ_compress_args.restype = C.c_void_p
    L.SZ_compress_args.argtypes = [C.c_int, C.c_void_p, P(C.c_size_t), C.c_int, C.c_double, C.c_double, C.c_double,
                                   C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]
    L.SZ_decompress.restype = C.c_void_p
    L.SZ_decompress.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]
    L.free_buf.argtypes = [C.c_void_p]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise SZ3HipError(rc, lib().sz3hip_last_error().decode())


@contextlib.contextmanager
def debug_flags(flags):
    """``with sz3_amd.debug_flags(Dbg.X | Dbg.Y):`` sets the process-wide development switches (sz3hip_debug_flags) for the body and
    sets them back to 0 on the way out, also when the body raises. Not for nesting: the inner block's exit leaves 0, not the outer flags."""
    L = lib()
    L.sz3hip_debug_flags(int(flags))
    try:
        yield
    finally:
        L.sz3hip_debug_flags(0)


@contextlib.contextmanager
def debug_flags2(flags):
    """``with sz3_amd.debug_flags2(Dbg2.X):`` the same for the second word of switches (sz3hip_debug_flags2)."""
    L = lib()
    L.sz3hip_debug_flags2(int(flags))
    try:
        yield
    finally:
        L.sz3hip_debug_flags2(0)


def last_encode_launches():
    """launches the encoder of the last stage 2 enqueued, the packer's included (sz3hip_last_encode_launches)"""
    return int(lib().sz3hip_last_encode_launches())


_SZ_TYPES = {"float32": 0, "float64": 1, "uint8": 2, "int8": 3, "uint16": 4, "int16": 5, "uint32": 6, "int32": 7, "uint64": 8, "int64": 9}


def _dtype_id(dt):
    """SZ_FLOAT .. SZ_INT64 (include/SZ3/def.hpp:27-36); integers: host-buffer API only (compress / decompress), they ride the f64 pipeline"""
    dt = np.dtype(dt)
    if dt.name in _SZ_TYPES:
        return _SZ_TYPES[dt.name]
    raise TypeError("sz3_amd supports float32 / float64 and 8 ... 64-bit integers (got %s)" % dt)


class Config:
    """Mirror of SZ3::Config (include/SZ3/utils/Config.hpp:138-479): ``Config(d0, d1, ...)`` with dims slowest first,
    size-1 dims dropped; public fields with the reference's names and defaults."""

    _FIELDS = [f[0] for f in _CConfig._fields_ if f[0] not in ("dims",)]

    def __init__(self, *dims):
        if len(dims) == 1 and isinstance(dims[0], (tuple, list)):
            dims = tuple(dims[0])
        if not dims:
            dims = (1,)
        self._c = _CConfig()
        self.setDims(dims)

    def setDims(self, dims):
        dims = [int(d) for d in dims]
        saved = {k: getattr(self._c, k) for k in self._FIELDS} if getattr(self._c, "num", 0) else None
        arr = (C.c_uint64 * len(dims))(*dims)
        lib().sz3hip_config_init(C.byref(self._c), len(dims), arr)
        if saved:  # setDims only touches dims/N/num/predDim/blockSize (Config.hpp:161-177)
            for k, v in saved.items():
                if k not in ("N", "num", "predDim", "blockSize"):
                    setattr(self._c, k, v)
        return int(self._c.num)

    @property
    def dims(self):
        return tuple(int(self._c.dims[i]) for i in range(self._c.N))

    def __getattr__(self, k):
        if k != "_c" and k in Config._FIELDS:
            return getattr(self._c, k)
        raise AttributeError(k)

    def __setattr__(self, k, v):
        if k != "_c" and k in Config._FIELDS:
            setattr(self._c, k, v)
        else:
            object.__setattr__(self, k, v)

    def save(self):
        buf = (C.c_ubyte * 256)()
        n = lib().sz3hip_config_save(C.byref(self._c), buf)
        return bytes(buf[:n])

    @classmethod
    def load(cls, raw):
        c = cls(1)
        b = (C.c_ubyte * len(raw)).from_buffer_copy(raw)
        if lib().sz3hip_config_load_n(C.byref(c._c), b, len(raw)) == 0:
            raise ValueError("truncated serialised Config")
        return c

    def copy(self):
        c = Config(1)
        C.memmove(C.byref(c._c), C.byref(self._c), C.sizeof(_CConfig))
        return c


# ---- pysz-like host API (tools/pysz/src/pysz/sz.pyx) -----------------------------------------------------------
def set_stock_format(on=True):
    """on: compress() writes streams stock SZ3 reads wherever this library has a stock form (ALGO_INTERP, which is what the default
    ALGO_INTERP_LORENZO resolves to on most data); reading stock ALGO_INTERP / ALGO_LOSSLESS streams needs no switch"""
    lib().sz3hip_set_stock_format(int(on))


def compress_bound(conf, dtype):
    return int(lib().sz3hip_compress_bound(C.byref(conf._c), _dtype_id(dtype)))


def _gpu_tensor(x):
    """x is a torch tensor on a HIP device (without importing torch when the caller never did)"""
    import sys
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor) and x.device.type == "cuda"


def _np_dtype(dtype):
    """a NumPy dtype, also from a torch dtype (torch.float32 -> float32)"""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(dtype, torch.dtype):
        return np.dtype(str(dtype).replace("torch.", ""))
    return np.dtype(dtype)


def _view_strides(t, conf):
    """element strides of a tensor for the Config's extents: size-1 dimensions dropped the way Config drops them"""
    dims = [int(d) for d in t.shape if int(d) != 1]
    strides = [int(st) for d, st in zip(t.shape, t.stride()) if int(d) != 1]
    if tuple(dims or [1]) != tuple(conf.dims):
        raise ValueError("config dims %s do not match the tensor's shape %s" % (conf.dims, tuple(t.shape)))
    if not strides:
        strides = [1]
    return (C.c_int64 * len(strides))(*strides)


def _stream_handle(device, stream):
    if stream is not None:
        return int(getattr(stream, "cuda_stream", stream))
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)


def compress(data, conf, out=None, stream=None):
    """sz.compress (sz.pyx:185-272): returns (uint8 ndarray, ratio). `out`: a caller's uint8 buffer of at least
    compress_bound(conf, dtype) bytes — the pre-allocated form, SZ_compress(conf, data, cmpData, cmpCap) (api/sz.hpp:43-62); a buffer
    used before costs no first-touch page faults.
    `data` may be a torch tensor on a HIP device, also a strided view: it is compressed where it lies (sz3hip_compress_from_device, the
    same container as for its host copy); `stream` (a torch stream or a raw handle; default: the device's current stream) is what the
    library waits for before it reads the tensor."""
    gpu = _gpu_tensor(data)
    if gpu:
        a = data
        npdt = _np_dtype(a.dtype)
        if int(conf.num) != a.numel():
            raise ValueError("config dims do not match the array")
    else:
        a = np.ascontiguousarray(data)
        npdt = a.dtype
        if int(conf.num) != a.size:
            raise ValueError("config dims do not match the array")
    dt = _dtype_id(npdt)
    cap = compress_bound(conf, npdt)
    if out is None:
        out = np.empty(cap, dtype=np.uint8)
    elif out.dtype != np.uint8 or not out.flags.c_contiguous or out.size < cap:
        raise ValueError("out must be a contiguous uint8 array of at least compress_bound(conf, dtype) = %d bytes" % cap)
    else:
        cap = out.size
    if gpu:
        n = lib().sz3hip_compress_from_device(C.byref(conf._c), dt, a.data_ptr(), _view_strides(a, conf), out.ctypes.data, cap,
                                              _stream_handle(a.device, stream))
        nbytes = a.numel() * npdt.itemsize
    else:
        n = lib().sz3hip_compress(C.byref(conf._c), dt, a.ctypes.data, out.ctypes.data, cap)
        nbytes = a.nbytes
    if n == 0:
        raise SZ3HipError(-1, lib().sz3hip_last_error().decode())
    blob = out[:n]  # a view, like pysz (sz.pyx:230-272): the untouched rest of the bound-sized buffer is never resident
    return blob, nbytes / float(n)


def decompress(blob, dtype, shape=None, out=None, device=None, stream=None):
    """sz.decompress (sz.pyx:276-365): returns (ndarray, Config). `out`: a caller's array of the stream's element count and `dtype`
    — the pre-allocated form, SZ_decompress(conf, cmpData, cmpSize, decData) (api/sz.hpp:84-110). `dtype` may be a torch dtype.
    `out` may be a torch tensor on a HIP device, also a view (a sub-box of a larger tensor): the array is decoded into it
    (sz3hip_decompress_to_device) and (out, Config) returned. `device=`: a tensor allocated there, returned as (tensor, Config).
    `stream`: what is waited for before the tensor is written (default: the device's current stream)."""
    blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob)
    conf = Config(1)
    _check(lib().sz3hip_peek_config(C.byref(conf._c), blob.ctypes.data, blob.size))
    npdt = _np_dtype(dtype)
    if device is not None or _gpu_tensor(out):
        import torch
        if out is None:
            out = torch.empty(conf.dims, dtype=getattr(torch, npdt.name), device=device)
            if shape is not None:
                shape = tuple(shape)
        else:
            shape = None
        if not _gpu_tensor(out):
            raise ValueError("out must be a tensor on a HIP device")
        if _np_dtype(out.dtype) != npdt or out.numel() != int(conf.num):
            raise ValueError("out must be a %s tensor of %d elements" % (npdt, int(conf.num)))
        _check(lib().sz3hip_decompress_to_device(C.byref(conf._c), _dtype_id(npdt), blob.ctypes.data, blob.size, out.data_ptr(),
                                                 _view_strides(out, conf), _stream_handle(out.device, stream)))
        return (out.reshape(shape) if shape is not None else out), conf
    dtype = npdt
    if out is None:
        dec = np.empty(int(conf.num), dtype=dtype)
    else:
        if out.dtype != np.dtype(dtype) or not out.flags.c_contiguous or out.size != int(conf.num):
            raise ValueError("out must be a contiguous %s array of %d elements" % (np.dtype(dtype), int(conf.num)))
        dec = out.reshape(-1)
    _check(lib().sz3hip_decompress(C.byref(conf._c), _dtype_id(dtype), blob.ctypes.data, blob.size, dec.ctypes.data))
    if shape is None:
        shape = conf.dims
    return dec.reshape(shape), conf


def _box(conf, lo, shape):
    lo, shape = tuple(int(v) for v in lo), tuple(int(v) for v in shape)
    if len(lo) != conf.N or len(shape) != conf.N:
        raise ValueError("lo and shape need one entry per extent of the array (%d)" % conf.N)
    if any(v < 0 for v in lo) or any(v < 0 for v in shape):
        raise ValueError("lo and shape must not be negative")
    return (C.c_uint64 * 4)(*lo), (C.c_uint64 * 4)(*shape), shape


def _region_plan_dict(plan, N):
    n = int(plan.n_levels)
    return {"n_levels": n, "strides": tuple(int(plan.stride[i]) for i in range(n)),
            "windows": tuple((tuple(int(plan.win_lo[i][j]) for j in range(N)), tuple(int(plan.win_hi[i][j]) for j in range(N))) for i in range(n)),
            "points": int(plan.points), "scratch_elems": int(plan.scratch_elems)}


def region_plan(conf, lo, shape):
    """what the region decode of the box [lo, lo + shape) of conf's array touches (sz3hip_region_plan_for): a dict with n_levels, strides
    (coarsest first), windows (per level the inclusive (lo, hi) tuples of the window the level reads, full-array coordinates), points
    (predicted points over all passes) and scratch_elems. Needs no device."""
    clo, cext, _ = _box(conf, lo, shape)
    plan = _CRegionPlan()
    _check(lib().sz3hip_region_plan_for(C.byref(conf._c), clo, cext, C.byref(plan)))
    return _region_plan_dict(plan, conf.N)


def tile_plan(conf, level, lo, shape):
    """what the tile decode of the box [lo, lo + shape) of the grid of every 2**level-th point of conf's array touches
    (sz3hip_tile_plan_for): a dict with region (region_plan's dict, in coarse-grid coordinates), units_total and units_needed. Needs no
    device."""
    clo, cext, _ = _box(conf, lo, shape)
    plan = _CTilePlan()
    _check(lib().sz3hip_tile_plan_for(C.byref(conf._c), int(level), clo, cext, C.byref(plan)))
    return {"region": _region_plan_dict(plan.region, conf.N), "units_total": int(plan.units_total), "units_needed": int(plan.units_needed)}


def tile_units(conf, level, lo, shape):
    """the decoder units (512 codes each) the tile's passes read a code from, strictly ascending, as a numpy uint32 array
    (sz3hip_tile_units_for). Needs no device."""
    clo, cext, _ = _box(conf, lo, shape)
    n = C.c_uint64(0)
    rc = lib().sz3hip_tile_units_for(C.byref(conf._c), int(level), clo, cext, None, 0, C.byref(n))
    if rc != -2:  # (SZ3HIP_ECAPACITY with the count: the list's size; 0: an empty list)
        _check(rc)
    units = np.empty(int(n.value), dtype=np.uint32)
    if units.size:
        _check(lib().sz3hip_tile_units_for(C.byref(conf._c), int(level), clo, cext, units.ctypes.data, units.size, C.byref(n)))
    return units


def set_sparse_decode(on=True):
    """on (the default): the Huffman stage of a tile / region decode decodes only the units the box needs where they are few"""
    lib().sz3hip_set_sparse_decode(int(on))


def get_sparse_decode():
    return bool(lib().sz3hip_get_sparse_decode())


def debug_tile_units():
    """(decoded, total): units the Huffman stage of this process's tile / region decodes decoded, and units their streams held"""
    d, t = C.c_uint64(0), C.c_uint64(0)
    lib().sz3hip_debug_tile_units(C.byref(d), C.byref(t))
    return int(d.value), int(t.value)


def debug_stock_huffman():
    """(passes, route) of this process's last stock Huffman decode: restart-point passes launched on the device (0 if none), and
    route 0 device, 1 host by SZ3HIP_STOCK_HOST_HUFFMAN, 2 host after the pass cap, 3 single symbol (no bit stream)"""
    p, r = C.c_int(0), C.c_int(0)
    lib().sz3hip_debug_stock_huffman(C.byref(p), C.byref(r))
    return int(p.value), int(r.value)


def debug_blkdec_last():
    """what this process's last block-stream decode did (sz3hip_debug_blkdec_last; the words of enum sz3hip_blkdec_word): a dict of
    form (BlkDecForm: the branch the first pass took), nslots (groups handed out, or blocks), workgroups (of a one-launch form, else
    0), tiles (of the 1-D top scan, else 0), retried (the retry through the launch-per-front decoders followed), rows (1-D: four
    blocks per wave) and retry_form (BlkDecForm.NONE without a retry)"""
    w = (C.c_uint32 * 8)()
    lib().sz3hip_debug_blkdec_last(w)
    return dict(form=BlkDecForm(w[0]), nslots=int(w[1]), workgroups=int(w[2]), tiles=int(w[3]), retried=bool(w[4]), rows=bool(w[5]),
                retry_form=BlkDecForm(w[6]))


def _decompress_partial(name, blob, dtype, probe_args, shape_of, out, device, stream):
    """The body of decompress_coarse / decompress_region / decompress_tile (name), over the library's sz3hip_<name>_to_device.
    shape_of(conf) -> (the output's shape, the call's arguments between cmpSize and d_out); probe_args() -> those arguments for an
    integer dtype, which the library refuses before it reads a box."""
    blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob)
    npdt = _np_dtype(dtype)
    dt = _dtype_id(npdt)
    if out is None and device is None:
        raise ValueError("%s decodes into device memory: pass device= or out=" % name)
    if out is not None and not _gpu_tensor(out):
        raise ValueError("out must be a tensor on a HIP device")
    call = getattr(lib(), "sz3hip_%s_to_device" % name)
    if dt > 1:  # (the library's own refusal, before anything is parsed or allocated)
        _check(call(C.byref(Config(1)._c), dt, blob.ctypes.data, blob.size, *probe_args(), None, None, None))
    conf = Config(1)
    _check(lib().sz3hip_peek_config(C.byref(conf._c), blob.ctypes.data, blob.size))
    shape, args = shape_of(conf)
    import torch
    if out is None:
        out = torch.empty(shape, dtype=getattr(torch, npdt.name), device=device)
    if _np_dtype(out.dtype) != npdt or tuple(out.shape) != shape:
        raise ValueError("out must be a %s tensor of shape %s" % (npdt, shape))
    strides = (C.c_int64 * len(shape))(*[int(st) for st in out.stride()])
    _check(call(C.byref(conf._c), dt, blob.ctypes.data, blob.size, *args, out.data_ptr(), strides, _stream_handle(out.device, stream)))
    return out, conf


def decompress_tile(blob, dtype, level, lo, shape, out=None, device=None, stream=None):
    """The box [lo, lo + shape) of the grid of every 2**level-th point of a container — bit for bit
    ``decompress(blob, dtype, device=...)[0][::2**level, ...][box]`` — in work sized to the box where the container is a single
    interpolation stream (sz3hip_decompress_tile_to_device). lo / shape are coarse-grid coordinates. Arguments and result as for
    decompress_region, which is level 0."""
    def shape_of(conf):
        clo, cext, box = _box(conf, lo, shape)
        return box, (int(level), clo, cext)
    return _decompress_partial("decompress_tile", blob, dtype, lambda: (int(level), None, None), shape_of, out, device, stream)


def _boxes(N, boxes):
    """boxes: a sequence of (lo, shape) pairs, N entries each -> (the sz3hip_box array, the shapes)"""
    boxes = [(tuple(int(v) for v in lo), tuple(int(v) for v in shape)) for lo, shape in boxes]
    arr = (_CBox * max(len(boxes), 1))()
    for i, (lo, shape) in enumerate(boxes):
        if len(lo) != N or len(shape) != N:
            raise ValueError("box %d: lo and shape need one entry per extent of the array (%d)" % (i, N))
        if any(v < 0 for v in lo) or any(v < 0 for v in shape):
            raise ValueError("box %d: lo and shape must not be negative" % i)
        arr[i].lo[:N] = lo
        arr[i].ext[:N] = shape
    return arr, [shape for _, shape in boxes]


def tiles_plan(conf, level, boxes):
    """what one decompress_tiles call for `boxes` — (lo, shape) pairs in coordinates of the grid of every 2**level-th point of conf's array —
    touches (sz3hip_tiles_plan_for): a dict with n_boxes, n_levels, points and scratch_elems (summed over the boxes), units_total and
    units_needed (the size of the union of the boxes' unit lists). Needs no device."""
    arr, shapes = _boxes(conf.N, boxes)
    plan = _CTilesPlan()
    _check(lib().sz3hip_tiles_plan_for(C.byref(conf._c), int(level), arr, len(shapes), C.byref(plan)))
    return {k: int(getattr(plan, k)) for k in ("n_boxes", "n_levels", "points", "scratch_elems", "units_total", "units_needed")}


def decompress_tiles(blob, dtype, level, boxes, out=None, device=None, stream=None):
    """Several boxes of the grid of every 2**level-th point of a container in ONE call (sz3hip_decompress_tiles_to_device): box i — a
    (lo, shape) pair in coarse-grid coordinates — comes out bit for bit as decompress_tile delivers it. The boxes share the container's
    host stage, one Huffman stage over the union of their units and one reconstruction's launches. Device only: `device=` allocates the
    tensors, or `out=` is a list of contiguous tensors of the boxes' shapes on one HIP device, none overlapping another. float32 / float64.
    Returns (list of tensors, Config) — the Config is the FULL array's. `stream` as for decompress."""
    blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob)
    npdt = _np_dtype(dtype)
    dt = _dtype_id(npdt)
    if out is None and device is None:
        raise ValueError("decompress_tiles decodes into device memory: pass device= or out=")
    if out is not None and not all(_gpu_tensor(t) for t in out):
        raise ValueError("out must be a list of tensors on a HIP device")
    call = lib().sz3hip_decompress_tiles_to_device
    if dt > 1:  # (the library's own refusal, before anything is parsed or allocated)
        _check(call(C.byref(Config(1)._c), dt, blob.ctypes.data, blob.size, int(level), None, 0, None, None))
    conf = Config(1)
    _check(lib().sz3hip_peek_config(C.byref(conf._c), blob.ctypes.data, blob.size))
    arr, shapes = _boxes(conf.N, boxes)
    import torch
    if out is None:
        out = [torch.empty(shape, dtype=getattr(torch, npdt.name), device=device) for shape in shapes]
    out = list(out)
    if len(out) != len(shapes):
        raise ValueError("out needs one tensor per box (%d)" % len(shapes))
    for t, shape in zip(out, shapes):
        if _np_dtype(t.dtype) != npdt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("out must hold contiguous %s tensors of the boxes' shapes" % npdt)
    ptrs = (C.c_void_p * max(len(out), 1))(*[t.data_ptr() for t in out])
    handle = _stream_handle(out[0].device, stream) if out else None  # (no box: the library's refusal)
    _check(call(C.byref(conf._c), dt, blob.ctypes.data, blob.size, int(level), arr, len(shapes), ptrs, handle))
    return out, conf


def decompress_region(blob, dtype, lo, shape, out=None, device=None, stream=None):
    """The box [lo, lo + shape) of a container, bit for bit what ``decompress(blob, dtype, device=...)[0]`` holds there, in work sized to the
    box where the container is a single interpolation stream (sz3hip_decompress_region_to_device). Device only: `device=` allocates a tensor
    of `shape` there, or `out=` is a tensor of that shape on a HIP device, also a view. float32 / float64. Returns (tensor, Config) — the
    Config is the FULL array's. `stream` as for decompress."""
    def shape_of(conf):
        clo, cext, box = _box(conf, lo, shape)
        return box, (clo, cext)
    return _decompress_partial("decompress_region", blob, dtype, lambda: (None, None), shape_of, out, device, stream)


def coarse_dims(conf, level):
    """extents of the array of every 2**level-th point of conf's array (sz3hip_coarse_dims): ``len(range(0, D, 2**level))`` per extent,
    slowest first, extents of 1 kept. Needs no device."""
    out = (C.c_uint64 * 4)()
    _check(lib().sz3hip_coarse_dims(C.byref(conf._c), int(level), out))
    return tuple(int(out[i]) for i in range(conf.N))


def decompress_coarse(blob, dtype, level, out=None, device=None, stream=None):
    """Every 2**level-th point of a container, bit for bit what ``decompress(blob, dtype, device=...)[0][::2**level, ...]`` holds, without
    the full-size array where the container is a single interpolation stream (sz3hip_decompress_coarse_to_device). Device only:
    `device=` allocates a tensor of coarse_dims(conf, level) there, or `out=` is a tensor of that shape on a HIP device, also a view.
    float32 / float64. Returns (tensor, Config) — the Config is the FULL array's. `stream` as for decompress."""
    return _decompress_partial("decompress_coarse", blob, dtype, lambda: (int(level),), lambda conf: (coarse_dims(conf, level), (int(level),)), out, device, stream)


def request_plan(conf, dtype, items):
    """what one Stream.request for `items` touches (sz3hip_request_plan_for), without a device. `items` have Stream.request's form: (level, lo,
    shape) or (level, lo, shape, out), lo / shape in coordinates of the grid of every 2**level-th point of conf's array. Of a tensor `out` the
    plan reads the address and the element strides only (its shape and dtype are checked as request checks them); an item without one is
    given a contiguous placeholder that overlaps no other. The request's own checks run, views and overlaps included. Returns a dict with n,
    finest_level, coarsest_level, n_levels (the array levels the one merged launch sequence runs), points and scratch_elems (summed over
    the boxes)."""
    items = [tuple(it) for it in items]
    if any(len(it) not in (3, 4) for it in items):
        raise ValueError("an item is (level, lo, shape) or (level, lo, shape, out)")
    npdt = _np_dtype(dtype)
    arr, shapes = _boxes(conf.N, [(it[1], it[2]) for it in items])
    reqs = (_CTileReq * max(len(items), 1))()
    at = 1 << 40  # (placeholders: never read, never written)
    for i, (it, shape) in enumerate(zip(items, shapes)):
        reqs[i].level = int(it[0])
        reqs[i].box = arr[i]
        t = it[3] if len(it) == 4 else None
        if t is not None:
            if _np_dtype(t.dtype) != npdt or tuple(t.shape) != shape:
                raise ValueError("item %d: out must be a %s tensor of the box's shape %s" % (i, npdt, shape))
            reqs[i].d_out = t.data_ptr()
            reqs[i].strides[:conf.N] = [int(v) for v in t.stride()]
        else:
            reqs[i].d_out = at
            at += (int(np.prod(shape, dtype=np.uint64)) * npdt.itemsize + 255) & ~255
    plan = _CRequestPlan()
    _check(lib().sz3hip_request_plan_for(C.byref(conf._c), _dtype_id(npdt), reqs, len(items), C.byref(plan)))
    return {k: int(getattr(plan, k)) for k, _ in _CRequestPlan._fields_}


BOX_STATS_DTYPE = np.dtype([(k, np.uint64 if t is C.c_uint64 else np.float64) for k, t in _CBoxStats._fields_])


class ReduceResult:
    """what a reduction leaves in DEVICE memory: `stats`, an (n, 11) int64 tensor whose rows are sz3hip_box_stats records (raw words), and
    `hist`, an (n, bins + 2) int64 tensor of counts (slot 0 under, slot bins + 1 over; None without a histogram). Nothing here waits for the
    device; numpy() does: it synchronises and returns (structured array with the struct's field names, histogram as uint64 or None)."""

    def __init__(self, stats, hist, bins):
        self.stats = stats
        self.hist = hist
        self.bins = bins

    def numpy(self):
        st = self.stats.cpu().numpy().view(BOX_STATS_DTYPE).reshape(-1)  # (the copy to the host is the synchronisation)
        return st, None if self.hist is None else self.hist.cpu().numpy().view(np.uint64)


def _reduce_opts(bins, lo, hi):
    o = _CReduceOpts()
    o.nbins = int(bins)
    o.lo = float(lo)
    o.hi = float(hi)
    return o


def _reduce_reqs(N, items):
    items = [tuple(it) for it in items]
    if any(len(it) != 3 for it in items):
        raise ValueError("an item is (level, lo, shape)")
    arr, _ = _boxes(N, [(it[1], it[2]) for it in items])
    reqs = (_CReduceReq * max(len(items), 1))()
    for i, it in enumerate(items):
        reqs[i].level = int(it[0])
        reqs[i].box = arr[i]
    return reqs, len(items)


def _reduce_result(n, bins, device):
    import torch
    stats = torch.empty((n, C.sizeof(_CBoxStats) // 8), dtype=torch.int64, device=device)
    hist = torch.empty((n, int(bins) + 2), dtype=torch.int64, device=device) if int(bins) > 0 else None
    return ReduceResult(stats, hist, int(bins))


def reduce_plan(conf, dtype, items, bins=0, lo=0.0, hi=0.0):
    """what one Stream.reduce for `items` — (level, lo, shape) — touches (sz3hip_reduce_plan_for), without a device: the reduce call's own
    checks run. Returns a dict with n, finest_level, coarsest_level, n_levels, points, scratch_elems (the level buffers and the partial
    records' room), partials (one per 4096 points of a box) and hist_words."""
    reqs, n = _reduce_reqs(conf.N, items)
    opts = _reduce_opts(bins, lo, hi)
    plan = _CReducePlan()
    _check(lib().sz3hip_reduce_plan_for(C.byref(conf._c), _dtype_id(_np_dtype(dtype)), reqs, n, C.byref(opts), C.byref(plan)))
    return {k: int(getattr(plan, k)) for k, _ in _CReducePlan._fields_}


def _points_tensor(fn, tensor, ndim=(0, None), what="the tensor is empty"):
    """what reduce_stats, select_points and the *_points functions ask of their input first: a torch tensor on a HIP device, of a supported
    dtype, not empty and of ndim[0] .. ndim[1] dimensions (None: any number); fn: the caller's name, for the messages. Returns the dtype's name."""
    if not _is_tensor(tensor):
        raise TypeError("%s takes a torch tensor on a HIP device (got %s)" % (fn, type(tensor).__name__))
    if not _gpu_tensor(tensor):
        raise ValueError("%s: the tensor must be on a HIP device (it is on %s)" % (fn, tensor.device))
    name = str(tensor.dtype).replace("torch.", "")
    if name not in _SZ_TYPES:
        raise TypeError("sz3_amd supports float32 / float64 and 8 ... 64-bit integers (got %s)" % tensor.dtype)
    if tensor.numel() == 0 or tensor.dim() < ndim[0] or (ndim[1] is not None and tensor.dim() > ndim[1]):
        raise ValueError("%s: %s" % (fn, what))
    return name


def _points_view(fn, tensor, out=None, axis=None):
    """... and the view a _device call gets: the dimensions above size 1 (and `axis`, where one is kept whatever its size), at most 4.
    Returns their indices, N, the extents, the input's strides and (out given) the output's."""
    keep = [i for i, d in enumerate(tensor.shape) if int(d) != 1 or i == axis]
    if len(keep) > 4:
        raise ValueError("%s: %d dimensions above size 1%s (at most 4 are supported)" % (fn, len(keep), "" if axis is None else ", the axis included"))
    dims = [int(tensor.shape[i]) for i in keep] or [1]
    sin = [int(tensor.stride(i)) for i in keep] or [1]
    sout = None if out is None else [int(out.stride(i)) for i in keep] or [1]
    return keep, len(dims), dims, sin, sout


def reduce_stats(tensor, bins=0, lo=0.0, hi=0.0, stream=None):
    """min, max, their places, shifted moments and (bins > 0) a histogram over [lo, hi) of one float32 / float64 torch tensor on a HIP device
    (sz3hip_reduce_device): the reduction Stream.reduce runs per box, over a plain view — any strides that are not negative, size-1
    dimensions dropped, at most 4 left; indices are row-major over the tensor's shape. Asynchronous on `stream`; returns a ReduceResult
    of one row."""
    name = _points_tensor("reduce_stats", tensor)
    _, N, dims, strides, _ = _points_view("reduce_stats", tensor)
    res = _reduce_result(1, bins, tensor.device)
    opts = _reduce_opts(bins, lo, hi)
    _check(lib().sz3hip_reduce_device(_SZ_TYPES[name], N, (C.c_uint64 * N)(*dims), tensor.data_ptr(), (C.c_int64 * N)(*strides), C.byref(opts),
                                      res.stats.data_ptr(), None if res.hist is None else res.hist.data_ptr(), _stream_handle(tensor.device, stream)))
    return res


SELECT_INVERT = 1  # SZ3HIP_SELECT_INVERT
SELECT_NAN = 2     # SZ3HIP_SELECT_NAN


class SelectResult:
    """what a selection leaves in DEVICE memory: `heads`, an (n, 4) int64 tensor whose rows are sz3hip_select_head records (n, count,
    written, capacity); `index`, a list of int64 tensors of the boxes' capacities (box-local row-major indices, ascending; only the first
    `written` are set); `value`, the same in the array's dtype (the points' raw bytes) or None. Nothing here waits for the device; numpy()
    does: it synchronises and returns per box (count, index[:written], value[:written] or None)."""

    def __init__(self, heads, index, value):
        self.heads = heads
        self.index = index
        self.value = value

    def numpy(self):
        heads = self.heads.cpu().numpy()  # (the copy to the host is the synchronisation)
        out = []
        for i, ix in enumerate(self.index):
            written = int(heads[i, 2])
            out.append((int(heads[i, 1]), ix[:written].cpu().numpy(), None if self.value is None else self.value[i][:written].cpu().numpy()))
        return out


def _select_opts(lo, hi, invert, nan):
    o = _CSelectOpts()
    o.lo = float(lo)
    o.hi = float(hi)
    o.flags = (SELECT_INVERT if invert else 0) | (SELECT_NAN if nan else 0)
    return o


def _select_caps(capacity, n):
    caps = [int(capacity)] * n if isinstance(capacity, (int, np.integer)) else [int(c) for c in capacity]
    if len(caps) != n:
        raise ValueError("capacity is an int or one per item (%d)" % n)
    if any(c < 0 for c in caps):
        raise ValueError("a capacity is negative")
    return caps


def _select_reqs(N, items, caps=None, index=None, value=None):
    items = [tuple(it) for it in items]
    if any(len(it) != 3 for it in items):
        raise ValueError("an item is (level, lo, shape)")
    arr, _ = _boxes(N, [(it[1], it[2]) for it in items])
    reqs = (_CSelectReq * max(len(items), 1))()
    for i, it in enumerate(items):
        reqs[i].level = int(it[0])
        reqs[i].box = arr[i]
        if caps is not None:
            reqs[i].capacity = caps[i]
        if index is not None and caps[i]:
            reqs[i].d_index = index[i].data_ptr()
            reqs[i].d_value = value[i].data_ptr() if value is not None else None
    return reqs, len(items)


def _select_result(caps, values, dtype, device):
    import torch
    heads = torch.empty((max(len(caps), 1), C.sizeof(_CSelectHead) // 8), dtype=torch.int64, device=device)
    index = [torch.empty((c,), dtype=torch.int64, device=device) for c in caps]
    value = [torch.empty((c,), dtype=dtype, device=device) for c in caps] if values else None
    return SelectResult(heads, index, value)


def select_plan(conf, dtype, items, lo=0.0, hi=0.0, capacity=0, invert=False, nan=False):
    """what one Stream.select for `items` — (level, lo, shape) — touches (sz3hip_select_plan_for), without a device: the select call's own
    checks run (the outputs are laid out one behind the other, index and value apart). Returns a dict with n, finest_level,
    coarsest_level, n_levels, points, scratch_elems (the level buffers and the chunk records' room) and partials (one per 4096 points of a
    box)."""
    items = [tuple(it) for it in items]
    caps = _select_caps(capacity, len(items))
    reqs, n = _select_reqs(conf.N, items, caps)
    at = 1 << 20
    for i in range(n):  # (stand-in addresses: the plan checks the outputs' rules, not whether they are device memory)
        if caps[i]:
            reqs[i].d_index = at
            at += caps[i] * 8
    opts = _select_opts(lo, hi, invert, nan)
    plan = _CSelectPlan()
    _check(lib().sz3hip_select_plan_for(C.byref(conf._c), _dtype_id(_np_dtype(dtype)), reqs, n, C.byref(opts), C.byref(plan)))
    return {k: int(getattr(plan, k)) for k, _ in _CSelectPlan._fields_}


def select_points(tensor, lo, hi, capacity, invert=False, nan=False, values=True, stream=None):
    """the points of one float32 / float64 torch tensor on a HIP device whose values lie in [lo, hi] (sz3hip_select_device): the selection
    Stream.select runs per box, over a plain view — any strides that are not negative, size-1 dimensions dropped, at most 4 left; indices
    are row-major over the tensor's shape. invert: the points outside the range; nan: NaN points too. Asynchronous on `stream`; returns a
    SelectResult of one box."""
    name = _points_tensor("select_points", tensor)
    _, N, dims, strides, _ = _points_view("select_points", tensor)
    caps = _select_caps(capacity, 1)
    res = _select_result(caps, values, tensor.dtype, tensor.device)
    opts = _select_opts(lo, hi, invert, nan)
    _check(lib().sz3hip_select_device(_SZ_TYPES[name], N, (C.c_uint64 * N)(*dims), tensor.data_ptr(), (C.c_int64 * N)(*strides), C.byref(opts),
                                      res.index[0].data_ptr() if caps[0] else None, res.value[0].data_ptr() if values and caps[0] else None, caps[0],
                                      res.heads.data_ptr(), _stream_handle(tensor.device, stream)))
    return res


MAP_U8, MAP_U16, MAP_F16, MAP_F32, MAP_LUT32 = 1, 2, 3, 4, 5  # SZ3HIP_MAP_*
MAX_LUT = 1024  # SZ3HIP_MAX_LUT
# out_type name -> (SZ3HIP_MAP_*, the out tensor's dtype name). torch's uint16 has too few operations to be a working storage type (no
# fill, no indexing, no comparison on every build this package meets): U16 texels live in int16 tensors, the same two bytes; LUT32's
# RGBA8 texels in int32 tensors.
_MAP_TYPES = {"u8": (MAP_U8, "uint8"), "u16": (MAP_U16, "int16"), "f16": (MAP_F16, "float16"), "f32": (MAP_F32, "float32"), "lut32": (MAP_LUT32, "int32")}


def _map_type(out_type):
    if isinstance(out_type, str) and out_type.lower() in _MAP_TYPES:
        return _MAP_TYPES[out_type.lower()]
    for code, name in _MAP_TYPES.values():
        if not isinstance(out_type, str) and int(out_type) == code:
            return code, name
    raise ValueError("out_type is one of 'u8', 'u16', 'f16', 'f32', 'lut32' (got %r)" % (out_type,))


def _map_opts(code, lo, hi, nan_code, lut):
    """the options struct; `lut`: an int32 torch tensor on a HIP device holding the table's 32-bit entries (kept alive by the caller for the call)"""
    o = _CMapOpts()
    o.lo = float(lo)
    o.hi = float(hi)
    o.out_type = code
    o.nan_code = int(nan_code) & 0xFFFFFFFF
    if lut is not None:
        if not _gpu_tensor(lut) or str(lut.dtype) != "torch.int32" or lut.dim() != 1 or not lut.is_contiguous():
            raise ValueError("lut must be a contiguous 1-D int32 tensor on a HIP device")
        o.lut_n = int(lut.numel())
        o.d_lut = lut.data_ptr()
    return o


def _map_reqs(N, items, shapes, arr, name, device, alloc):
    """the request structs over out tensors of dtype `name` (uint8 / int16 / float16 / float32 / int32); alloc: missing outputs are allocated
    (else given placeholders that overlap no other, for the plan)"""
    import sys
    torch = sys.modules.get("torch")
    itemsize = np.dtype(name).itemsize
    reqs = (_CTileReq * max(len(items), 1))()
    outs = []
    at = 1 << 40
    for i, (it, shape) in enumerate(zip(items, shapes)):
        t = it[3] if len(it) == 4 else None
        if t is None and alloc:
            t = torch.empty(shape, dtype=getattr(torch, name), device=device)
        reqs[i].level = int(it[0])
        reqs[i].box = arr[i]
        if t is not None:
            if (alloc and not _gpu_tensor(t)) or str(t.dtype) != "torch." + name or tuple(t.shape) != shape or (alloc and t.device != device):
                raise ValueError("item %d: out must be a %s tensor of the box's shape %s%s" % (i, name, shape, " on %s" % device if alloc else ""))
            reqs[i].d_out = t.data_ptr()
            reqs[i].strides[:N] = [int(v) for v in t.stride()]
        else:
            reqs[i].d_out = at
            at += (int(np.prod(shape, dtype=np.uint64)) * itemsize + 255) & ~255
        outs.append(t)
    return reqs, outs


def map_plan(conf, dtype, items, out_type, lo=0.0, hi=0.0, nan_code=0, lut=None):
    """what one Stream.map for `items` touches (sz3hip_map_plan_for), without a device: `items` are Stream.map's — (level, lo, shape) or
    (level, lo, shape, out) — and the map call's own checks run, views and overlaps in OUTPUT elements included. `lut`: an int32 tensor, or
    for the plan an int (the entry count; the table's address is then a placeholder). Returns a dict with request_plan's fields and
    out_elem_bytes."""
    items = [tuple(it) for it in items]
    if any(len(it) not in (3, 4) for it in items):
        raise ValueError("an item is (level, lo, shape) or (level, lo, shape, out)")
    code, name = _map_type(out_type)
    arr, shapes = _boxes(conf.N, [(it[1], it[2]) for it in items])
    reqs, _ = _map_reqs(conf.N, items, shapes, arr, name, None, False)
    if isinstance(lut, int):
        opts = _map_opts(code, lo, hi, nan_code, None)
        opts.lut_n = lut
        opts.d_lut = 1 << 39
    else:
        opts = _map_opts(code, lo, hi, nan_code, lut)
    plan = _CMapPlan()
    _check(lib().sz3hip_map_plan_for(C.byref(conf._c), _dtype_id(_np_dtype(dtype)), reqs, len(items), C.byref(opts), C.byref(plan)))
    return {k: int(getattr(plan, k)) for k, _ in _CMapPlan._fields_}


def map_points(tensor, out_type, lo=0.0, hi=0.0, nan_code=0, lut=None, out=None, stream=None):
    """texels of one float32 / float64 torch tensor on a HIP device (sz3hip_map_device): the mapping Stream.map runs per box, over a plain
    view — any strides that are not negative, at most 4 dimensions above size 1. out_type: "u8" / "u16" (codes of the window [lo, hi), a
    NaN point becomes nan_code), "f16", "f32", or "lut32" (lut[code], `lut` an int32 tensor of 2 .. 1024 entries on the device; a NaN
    point becomes nan_code itself). `out`: a tensor of the input's shape and of dtype uint8 / int16 (u16's two bytes: torch's uint16 is
    not a working storage type) / float16 / float32 / int32, any view whose strides nest in row-major order (default: allocated,
    contiguous). Asynchronous on `stream`; returns `out`."""
    tname = _points_tensor("map_points", tensor)
    import torch
    code, name = _map_type(out_type)
    if out is None:
        out = torch.empty(tuple(tensor.shape), dtype=getattr(torch, name), device=tensor.device)
    if not _gpu_tensor(out) or str(out.dtype) != "torch." + name or tuple(out.shape) != tuple(tensor.shape) or out.device != tensor.device:
        raise ValueError("map_points: out must be a %s tensor of the input's shape %s on %s" % (name, tuple(tensor.shape), tensor.device))
    _, N, dims, sin, sout = _points_view("map_points", tensor, out)
    opts = _map_opts(code, lo, hi, nan_code, lut)
    _check(lib().sz3hip_map_device(_SZ_TYPES[tname], N, (C.c_uint64 * N)(*dims), tensor.data_ptr(), (C.c_int64 * N)(*sin), C.byref(opts), out.data_ptr(),
                                   (C.c_int64 * N)(*sout), _stream_handle(tensor.device, stream)))
    return out


SAMPLE_NEAREST, SAMPLE_LINEAR = 0, 1  # SZ3HIP_SAMPLE_*
SAMPLE_CLAMP = 1                      # SZ3HIP_SAMPLE_CLAMP
_SAMPLE_MODES = {"nearest": SAMPLE_NEAREST, "linear": SAMPLE_LINEAR}


def _sample_mode(mode):
    if isinstance(mode, str) and mode.lower() in _SAMPLE_MODES:
        return _SAMPLE_MODES[mode.lower()]
    if not isinstance(mode, str) and int(mode) in _SAMPLE_MODES.values():
        return int(mode)
    raise ValueError("mode is 'nearest' or 'linear' (got %r)" % (mode,))


def _sample_query(q, N, i, req):
    """fills box i's query words of `req` from q — a (n, N) float32 / float64 tensor, a lattice (origin, steps, counts), or (the plan only)
    an int: that many points at a placeholder address. Returns (the coordinates' dtype name or None, the output's shape)."""
    if isinstance(q, (int, np.integer)) and not isinstance(q, bool):
        req.d_coords = 1 << 38
        req.n_points = int(q)
        return None, (int(q),)
    if _is_tensor(q):
        name = str(q.dtype).replace("torch.", "")
        if name not in ("float32", "float64") or q.dim() != 2 or int(q.shape[1]) != N or not q.is_contiguous():
            raise ValueError("query %d: coordinates are a contiguous (n, %d) float32 / float64 tensor" % (i, N))
        req.d_coords = q.data_ptr()
        req.n_points = int(q.shape[0])
        return name, (int(q.shape[0]),)
    if not isinstance(q, (tuple, list)) or len(q) != 3:
        raise ValueError("query %d: a query is a coordinate tensor or a lattice (origin, steps, counts)" % i)
    origin, steps, counts = q
    origin = [float(v) for v in origin]
    steps = [[float(v) for v in st] for st in steps]
    counts = [int(c) for c in counts]
    if len(origin) != N or any(len(st) != N for st in steps):
        raise ValueError("query %d: the lattice's origin and every step need one entry per extent of the array (%d)" % (i, N))
    if not 1 <= len(counts) <= 3 or len(steps) != len(counts) or any(c < 0 for c in counts):
        raise ValueError("query %d: a lattice has 1 .. 3 axes, a step and a count each" % i)
    pad = 3 - len(counts)  # (the axes given are the fastest ones)
    req.d_coords = None
    req.origin[:N] = origin
    total = 1
    for a in range(3):
        req.counts[a] = counts[a - pad] if a >= pad else 1
        total *= int(req.counts[a])
        if a >= pad:
            req.steps[a][:N] = steps[a - pad]
    req.n_points = total
    return None, tuple(counts)


def _sample_reqs(N, items, queries):
    items = [tuple(it) for it in items]
    if any(len(it) != 3 for it in items):
        raise ValueError("an item is (level, lo, shape)")
    queries = list(queries)
    if len(queries) != len(items):
        raise ValueError("queries holds one entry per item (%d)" % len(items))
    arr, _ = _boxes(N, [(it[1], it[2]) for it in items])
    reqs = (_CSampleReq * max(len(items), 1))()
    names, shapes = set(), []
    for i, (it, q) in enumerate(zip(items, queries)):
        reqs[i].level = int(it[0])
        reqs[i].box = arr[i]
        name, shape = _sample_query(q, N, i, reqs[i])
        shapes.append(shape)
        if name:
            names.add(name)
    if len(names) > 1:
        raise ValueError("the coordinate tensors of one call are all float32 or all float64")
    return reqs, len(items), (names.pop() if names else "float64"), shapes


def _sample_opts(mode, clamp, fill, coord_name):
    o = _CSampleOpts()
    o.filter = _sample_mode(mode)
    o.coord_type = _SZ_TYPES[coord_name]
    o.flags = SAMPLE_CLAMP if clamp else 0
    o.fill = float(fill)
    return o


def sample_plan(conf, dtype, items, queries, mode="linear", clamp=False, fill=float("nan")):
    """what one Stream.sample for `items` and `queries` touches (sz3hip_sample_plan_for), without a device: the sample call's own checks run
    (the outputs are laid out one behind the other). A query is Stream.sample's, or an int: that many float64 points at a placeholder
    address. Returns a dict with request_plan's fields and queries, the sum of the queries' points."""
    reqs, n, cname, _ = _sample_reqs(conf.N, items, queries)
    dt = _np_dtype(dtype)
    at = 1 << 40
    for i in range(n):  # (stand-in addresses: the plan checks the outputs' rules, not whether they are device memory)
        reqs[i].d_out = at
        at += (int(reqs[i].n_points) * 8 + 255) & ~255
    opts = _sample_opts(mode, clamp, fill, cname)
    plan = _CSamplePlan()
    _check(lib().sz3hip_sample_plan_for(C.byref(conf._c), _dtype_id(dt), reqs, n, C.byref(opts), C.byref(plan)))
    return {k: int(getattr(plan, k)) for k, _ in _CSamplePlan._fields_}


def sample_points(tensor, query, mode="linear", clamp=False, fill=float("nan"), stream=None):
    """one float32 / float64 torch tensor on a HIP device sampled at fractional positions (sz3hip_sample_device): the sampling Stream.sample
    runs per box, over a plain view — 1 .. 4 dimensions, any strides that are not negative. `query`: a contiguous (n, tensor.dim()) float32 /
    float64 tensor of coordinates on the device — every dimension has its coordinate, those of size 1 too — or a lattice (origin, steps,
    counts). mode "nearest": the nearest point's bytes; "linear": the multilinear interpolation in double, rounded once. A query outside
    [0, size - 1] yields `fill`, or is clamped (clamp=True); a NaN coordinate always yields `fill`. Asynchronous on `stream`; returns a
    tensor of the input's dtype: (n,) for coordinates, of shape `counts` for a lattice."""
    name = _points_tensor("sample_points", tensor)
    N = tensor.dim()
    if not 1 <= N <= 4:
        raise ValueError("sample_points: %d dimensions (1 .. 4 are supported)" % N)
    import torch
    req = _CSampleReq()
    cname, shape = _sample_query(query, N, 0, req)
    if _is_tensor(query) and (not _gpu_tensor(query) or query.device != tensor.device):
        raise ValueError("sample_points: the coordinates must be on %s" % tensor.device)
    if isinstance(query, (int, np.integer)):
        raise ValueError("sample_points: a query is a coordinate tensor or a lattice (origin, steps, counts)")
    out = torch.empty(shape, dtype=tensor.dtype, device=tensor.device)
    req.d_out = out.data_ptr()
    opts = _sample_opts(mode, clamp, fill, cname or "float64")
    dims = [int(d) for d in tensor.shape]
    strides = [int(v) for v in tensor.stride()]
    _check(lib().sz3hip_sample_device(_SZ_TYPES[name], N, (C.c_uint64 * N)(*dims), tensor.data_ptr(), (C.c_int64 * N)(*strides), C.byref(opts), C.byref(req),
                                      _stream_handle(tensor.device, stream)))
    return out


PROJECT_MIN, PROJECT_MAX, PROJECT_SUM, PROJECT_MEAN, PROJECT_ARGMIN, PROJECT_ARGMAX, PROJECT_COUNT = range(7)  # SZ3HIP_PROJECT_*
_PROJECT_OPS = {"min": PROJECT_MIN, "max": PROJECT_MAX, "sum": PROJECT_SUM, "mean": PROJECT_MEAN, "argmin": PROJECT_ARGMIN, "argmax": PROJECT_ARGMAX,
                "count": PROJECT_COUNT}


def _project_opts(op, axis, N, dtype_name, out_dtype, fill):
    """the options struct and the outputs' dtype name: the handle's, or out_dtype (float32 / float64); an index op ("argmin", "argmax",
    "count") writes uint32 and takes no out_dtype — its values live in int32 tensors, the same four bytes"""
    if not isinstance(op, str) or op.lower() not in _PROJECT_OPS:
        raise ValueError("op is one of 'min', 'max', 'sum', 'mean', 'argmin', 'argmax', 'count' (got %r)" % (op,))
    code = _PROJECT_OPS[op.lower()]
    axis = int(axis)
    if not -N <= axis < N:
        raise ValueError("axis %d is not one of the %d dimensions" % (axis, N))
    o = _CProjectOpts()
    o.op = code
    o.axis = axis % N
    o.fill = float(fill)
    if code >= PROJECT_ARGMIN:
        if out_dtype is not None:
            raise ValueError("op %r writes indices: it takes no out_dtype" % op)
        return o, "int32"
    name = dtype_name if out_dtype is None else str(out_dtype).replace("torch.", "")
    if name not in ("float32", "float64") and out_dtype is not None:  # (a numpy dtype or type)
        try:
            name = np.dtype(out_dtype).name
        except TypeError:
            pass
    if name not in ("float32", "float64"):
        raise ValueError("out_dtype is float32 or float64 (got %r)" % (out_dtype,))
    o.out_type = _SZ_TYPES[name]
    return o, name


def _project_items(items):
    items = [tuple(it) for it in items]
    if any(len(it) not in (3, 4) for it in items):
        raise ValueError("an item is (level, lo, shape) or (level, lo, shape, out)")
    return [it if len(it) == 3 or it[3] is not None else it[:3] for it in items]


def project_plan(conf, dtype, items, op, axis, out_dtype=None):
    """what one Stream.project for `items` touches (sz3hip_project_plan_for), without a device: `items` are Stream.project's — (level, lo,
    shape) or (level, lo, shape, out) — and the call's own checks run, the views and overlaps of the collapsed boxes in OUTPUT elements
    included. Returns a dict with request_plan's fields, out_points and out_elem_bytes."""
    items = _project_items(items)
    dt = _np_dtype(dtype)
    opts, name = _project_opts(op, axis, conf.N, dt.name, out_dtype, float("nan"))
    arr, shapes = _boxes(conf.N, [(it[1], it[2]) for it in items])
    flat = [tuple(1 if j == opts.axis else v for j, v in enumerate(shape)) for shape in shapes]
    reqs, _ = _map_reqs(conf.N, items, flat, arr, name, None, False)
    plan = _CProjectPlan()
    _check(lib().sz3hip_project_plan_for(C.byref(conf._c), _dtype_id(dt), reqs, len(items), C.byref(opts), C.byref(plan)))
    return {k: int(getattr(plan, k)) for k, _ in _CProjectPlan._fields_ if k != "reserved"}


def project_points(tensor, op, axis, out_dtype=None, fill=float("nan"), out=None, stream=None):
    """one float32 / float64 torch tensor on a HIP device collapsed along `axis` (sz3hip_project_device): the projection Stream.project runs
    per box, over a plain view — any strides that are not negative, at most 4 dimensions above size 1 (the axis counts as one). op: "min",
    "max", "sum", "mean" (values, of the tensor's dtype or `out_dtype`), "argmin", "argmax", "count" (uint32 in an int32 tensor). NaN and
    +-Inf points are left out; a column without a finite point gives `fill` (min, max, mean), 0 (sum, count) or the axis' size (argmin,
    argmax). The sum is the sequential fold in double along the axis, rounded once. `out`: a tensor of the input's shape with 1 at `axis`,
    any view whose strides nest in row-major order (default: allocated, contiguous). Asynchronous on `stream`; returns `out`. One number
    about a long 1-D tensor is reduce_stats' work: a 1-D projection is one lane's."""
    tname = _points_tensor("project_points", tensor, (1, None), "the tensor is empty or has no dimension")
    import torch
    opts, name = _project_opts(op, axis, tensor.dim(), tname, out_dtype, fill)
    axis = int(opts.axis)
    shape = tuple(1 if i == axis else int(d) for i, d in enumerate(tensor.shape))
    if out is None:
        out = torch.empty(shape, dtype=getattr(torch, name), device=tensor.device)
    if not _gpu_tensor(out) or str(out.dtype) != "torch." + name or tuple(out.shape) != shape or out.device != tensor.device:
        raise ValueError("project_points: out must be a %s tensor of shape %s on %s" % (name, shape, tensor.device))
    keep, N, dims, sin, sout = _points_view("project_points", tensor, out, axis)
    opts.axis = keep.index(axis)
    _check(lib().sz3hip_project_device(_SZ_TYPES[tname], N, (C.c_uint64 * N)(*dims), tensor.data_ptr(), (C.c_int64 * N)(*sin), C.byref(opts), out.data_ptr(),
                                       (C.c_int64 * N)(*sout), _stream_handle(tensor.device, stream)))
    return out


GRADIENT_DERIV, GRADIENT_MAG2, GRADIENT_MAG, GRADIENT_VECTOR = range(4)  # SZ3HIP_GRADIENT_*
GRADIENT_INTERIOR = 1                                                    # SZ3HIP_GRADIENT_INTERIOR
_GRADIENT_OPS = {"deriv": GRADIENT_DERIV, "mag2": GRADIENT_MAG2, "mag": GRADIENT_MAG, "vector": GRADIENT_VECTOR}


def _gradient_opts(op, axis, N, dtype_name, spacing, out_dtype, interior):
    """the options struct and the outputs' dtype name: the input's, or out_dtype (float32 / float64). spacing: None (1.0 per axis), a
    scalar for every axis, or one value per axis"""
    if not isinstance(op, str) or op.lower() not in _GRADIENT_OPS:
        raise ValueError("op is one of 'deriv', 'mag2', 'mag', 'vector' (got %r)" % (op,))
    code = _GRADIENT_OPS[op.lower()]
    axis = int(axis)
    if not -N <= axis < N:
        raise ValueError("axis %d is not one of the %d dimensions" % (axis, N))
    if code != GRADIENT_DERIV and axis != 0:
        raise ValueError("op %r differentiates along every axis: it takes no axis" % op)
    o = _CGradientOpts()
    o.op = code
    o.axis = axis % N
    o.flags = GRADIENT_INTERIOR if interior else 0
    if spacing is None:
        steps = [1.0] * N
    elif np.ndim(spacing) == 0:
        steps = [float(spacing)] * N
    else:
        steps = [float(v) for v in spacing]
        if len(steps) != N:
            raise ValueError("spacing needs one value per extent of the array (%d), or one scalar" % N)
    o.spacing[:N] = steps
    name = dtype_name if out_dtype is None else str(out_dtype).replace("torch.", "")
    if name not in ("float32", "float64") and out_dtype is not None:  # (a numpy dtype or type)
        try:
            name = np.dtype(out_dtype).name
        except TypeError:
            pass
    if name not in ("float32", "float64"):
        raise ValueError("out_dtype is float32 or float64 (got %r)" % (out_dtype,))
    o.out_type = _SZ_TYPES[name]
    return o, name


def _gradient_shape(shape, opts):
    """a box's output shape: the box's, without the first and last point of every differentiated axis under INTERIOR (never below 0)"""
    if not opts.flags & GRADIENT_INTERIOR:
        return tuple(shape)
    return tuple(max(v - 2, 0) if opts.op != GRADIENT_DERIV or j == opts.axis else v for j, v in enumerate(shape))


def _vector_strides(t, N, what):
    """the strides of a VECTOR output in output ELEMENTS (N values each): the tensor's without the last dimension, divided by N"""
    if t.shape[-1] > 1 and int(t.stride(-1)) != 1:
        raise ValueError("%s: a vector output's last dimension (the %d components) must be contiguous (its stride is %d)" % (what, N, int(t.stride(-1))))
    strides = [int(v) for v in t.stride()[:-1]]
    if any(v % N for v, e in zip(strides, t.shape[:-1]) if int(e) != 1):
        raise ValueError("%s: a vector output's strides %s must be divisible by the component count %d: a view is counted in elements of %d values"
                         % (what, tuple(strides), N, N))
    return [v // N for v in strides]


def _gradient_reqs(N, items, shapes, arr, name, opts, device, alloc):
    """the request structs over out tensors of dtype `name` and the output boxes' shapes (VECTOR: plus a last dimension N); alloc: missing
    outputs are allocated (else given placeholders that overlap no other, for the plan)"""
    import sys
    torch = sys.modules.get("torch")
    vec = opts.op == GRADIENT_VECTOR
    elem = np.dtype(name).itemsize * (N if vec else 1)
    reqs = (_CTileReq * max(len(items), 1))()
    outs = []
    at = 1 << 40
    for i, (it, shape) in enumerate(zip(items, shapes)):
        oshape = _gradient_shape(shape, opts)
        full = oshape + (N,) if vec else oshape
        t = it[3] if len(it) == 4 else None
        if alloc and not all(oshape):
            raise ValueError("item %d: interior needs at least 3 points along every differentiated axis (the box's shape is %s)" % (i, tuple(shape)))
        if t is None and alloc:
            t = torch.empty(full, dtype=getattr(torch, name), device=device)
        reqs[i].level = int(it[0])
        reqs[i].box = arr[i]
        if t is not None:
            if str(t.dtype) != "torch." + name or tuple(t.shape) != full or (alloc and (not _gpu_tensor(t) or t.device != device)):
                raise ValueError("item %d: out must be a %s tensor of shape %s%s" % (i, name, full, " on %s" % device if alloc else ""))
            reqs[i].d_out = t.data_ptr()
            reqs[i].strides[:N] = _vector_strides(t, N, "item %d" % i) if vec else [int(v) for v in t.stride()]
        else:
            reqs[i].d_out = at
            at += (int(np.prod(oshape, dtype=np.uint64)) * elem + 255) & ~255
        outs.append(t)
    return reqs, outs


def gradient_plan(conf, dtype, items, op, axis=0, spacing=None, out_dtype=None, interior=False):
    """what one Stream.gradient for `items` touches (sz3hip_gradient_plan_for), without a device: `items` are Stream.gradient's — (level,
    lo, shape) or (level, lo, shape, out) — and the call's own checks run, the views and overlaps of the output boxes in OUTPUT elements
    included. Returns a dict with request_plan's fields, out_points (after `interior`) and out_elem_bytes."""
    items = _project_items(items)
    dt = _np_dtype(dtype)
    opts, name = _gradient_opts(op, axis, conf.N, dt.name, spacing, out_dtype, interior)
    arr, shapes = _boxes(conf.N, [(it[1], it[2]) for it in items])
    reqs, _ = _gradient_reqs(conf.N, items, shapes, arr, name, opts, None, False)
    plan = _CGradientPlan()
    _check(lib().sz3hip_gradient_plan_for(C.byref(conf._c), _dtype_id(dt), reqs, len(items), C.byref(opts), C.byref(plan)))
    return {k: int(getattr(plan, k)) for k, _ in _CGradientPlan._fields_ if k != "reserved"}


def gradient_points(tensor, op, axis=0, spacing=None, out_dtype=None, interior=False, out=None, stream=None):
    """the gradient of one float32 / float64 torch tensor of 1 .. 4 dimensions on a HIP device (sz3hip_gradient_device): what
    Stream.gradient runs per box, over a plain view — any strides that are not negative. op: "deriv" (along `axis`), "mag2" (the sum of
    the squared derivatives), "mag" (its square root) or "vector" (all derivatives: the output has a last dimension of tensor.dim()
    components, slowest axis first). Central differences inside, one-sided at the first and last point (numpy.gradient's edge_order=1),
    in IEEE double, rounded once into the tensor's dtype or `out_dtype`. spacing: the grid step, one scalar or one value per axis
    (default 1.0). interior: the output loses the first and last point of every differentiated axis, so every point is a central
    difference. `out`: a tensor of the output's shape, any view whose strides nest in row-major order (default: allocated, contiguous);
    a vector output must have its last dimension contiguous and its other strides divisible by the component count. Asynchronous on
    `stream`; returns `out`."""
    tname = _points_tensor("gradient_points", tensor, (1, 4), "the tensor is empty or does not have 1 .. 4 dimensions")
    import torch
    N = tensor.dim()
    opts, name = _gradient_opts(op, axis, N, tname, spacing, out_dtype, interior)
    vec = opts.op == GRADIENT_VECTOR
    shape = _gradient_shape(tuple(int(d) for d in tensor.shape), opts)
    full = shape + (N,) if vec else shape
    for j, e in enumerate(shape):
        if e == 0:
            raise ValueError("gradient_points: interior needs at least 3 points along every differentiated axis (dimension %d is %d)" % (j, int(tensor.shape[j])))
    if out is None:
        out = torch.empty(full, dtype=getattr(torch, name), device=tensor.device)
    if (not _gpu_tensor(out) or str(out.dtype) != "torch." + name or tuple(out.shape) != full or out.device != tensor.device):
        raise ValueError("gradient_points: out must be a %s tensor of shape %s on %s" % (name, full, tensor.device))
    dims = [int(d) for d in tensor.shape]
    sin = [int(v) for v in tensor.stride()]
    sout = _vector_strides(out, N, "gradient_points") if vec else [int(v) for v in out.stride()]
    _check(lib().sz3hip_gradient_device(_SZ_TYPES[tname], N, (C.c_uint64 * N)(*dims), tensor.data_ptr(), (C.c_int64 * N)(*sin), C.byref(opts),
                                        out.data_ptr(), (C.c_int64 * N)(*sout), _stream_handle(tensor.device, stream)))
    return out


COMPOSITE_RGBA32F, COMPOSITE_RGBA8 = 0, 1                                    # SZ3HIP_COMPOSITE_RGBA*
COMPOSITE_REVERSE, COMPOSITE_LEVEL_OPACITY, COMPOSITE_ACCUMULATE = 1, 2, 4   # SZ3HIP_COMPOSITE_* flags
_COMPOSITE_TYPES = {"rgba32f": (COMPOSITE_RGBA32F, "float32"), "rgba8": (COMPOSITE_RGBA8, "int32")}


def _composite_opts(axis, N, lut, lo, hi, out_type, reverse, level_opacity, accumulate, cutoff, level_bias):
    """the options struct and the outputs' dtype name ("float32": a last dimension of 4; "int32": the four bytes of an RGBA8 element).
    lut: a contiguous float32 tensor of shape (2 .. 1024, 4) on the device — or, for a plan, an int: the entry count (the table's address
    is then a placeholder)"""
    if not isinstance(out_type, str) or out_type.lower() not in _COMPOSITE_TYPES:
        raise ValueError("out_type is 'rgba32f' or 'rgba8' (got %r)" % (out_type,))
    code, name = _COMPOSITE_TYPES[out_type.lower()]
    axis = int(axis)
    if not -N <= axis < N:
        raise ValueError("axis %d is not one of the %d dimensions" % (axis, N))
    o = _CCompositeOpts()
    o.lo, o.hi, o.cutoff = float(lo), float(hi), float(cutoff)
    o.axis = axis % N
    o.out_type = code
    o.flags = (COMPOSITE_REVERSE if reverse else 0) | (COMPOSITE_LEVEL_OPACITY if level_opacity else 0) | (COMPOSITE_ACCUMULATE if accumulate else 0)
    o.level_bias = int(level_bias)
    if isinstance(lut, (int, np.integer)):
        o.lut_n = int(lut)
        o.d_lut = 1 << 39
    else:
        if not _is_tensor(lut) or str(lut.dtype) != "torch.float32" or lut.dim() != 2 or int(lut.shape[1]) != 4 or not lut.is_contiguous():
            raise ValueError("lut is a contiguous float32 tensor of shape (entries, 4): r, g, b, a per entry")
        if not _gpu_tensor(lut):
            raise ValueError("lut must be on a HIP device (it is on %s)" % lut.device)
        o.lut_n = int(lut.shape[0])
        o.d_lut = lut.data_ptr()
    return o, name


def _composite_reqs(N, items, shapes, arr, name, axis, device, alloc):
    """the request structs over out tensors of the collapsed boxes' shapes — float32 with a last dimension 4, or int32 —; alloc: missing
    outputs are allocated (else given placeholders that overlap no other, for the plan)"""
    import sys
    torch = sys.modules.get("torch")
    vec = name == "float32"
    elem = 16 if vec else 4
    reqs = (_CTileReq * max(len(items), 1))()
    outs = []
    at = 1 << 40
    for i, (it, shape) in enumerate(zip(items, shapes)):
        flat = tuple(1 if j == axis else int(v) for j, v in enumerate(shape))
        full = flat + (4,) if vec else flat
        t = it[3] if len(it) == 4 else None
        if t is None and alloc:
            t = torch.empty(full, dtype=getattr(torch, name), device=device)
        reqs[i].level = int(it[0])
        reqs[i].box = arr[i]
        if t is not None:
            if str(t.dtype) != "torch." + name or tuple(t.shape) != full or (alloc and (not _gpu_tensor(t) or t.device != device)):
                raise ValueError("item %d: out must be a %s tensor of shape %s%s" % (i, name, full, " on %s" % device if alloc else ""))
            reqs[i].d_out = t.data_ptr()
            reqs[i].strides[:N] = _vector_strides(t, 4, "item %d" % i) if vec else [int(v) for v in t.stride()]
        else:
            reqs[i].d_out = at
            at += (int(np.prod(flat, dtype=np.uint64)) * elem + 255) & ~255
        outs.append(t)
    return reqs, outs


def composite_plan(conf, dtype, items, axis, lut, lo, hi, out_type="rgba32f", reverse=False, level_opacity=False, accumulate=False, cutoff=float("inf"),
                   level_bias=0):
    """what one Stream.composite for `items` touches (sz3hip_composite_plan_for), without a device: `items` are Stream.composite's — (level,
    lo, shape) or (level, lo, shape, out) — and the call's own checks run, the views and overlaps of the collapsed boxes in OUTPUT elements
    included. `lut`: the table, or an int (the entry count). Returns a dict with request_plan's fields, out_points and out_elem_bytes."""
    items = _project_items(items)
    dt = _np_dtype(dtype)
    opts, name = _composite_opts(axis, conf.N, lut, lo, hi, out_type, reverse, level_opacity, accumulate, cutoff, level_bias)
    arr, shapes = _boxes(conf.N, [(it[1], it[2]) for it in items])
    reqs, _ = _composite_reqs(conf.N, items, shapes, arr, name, int(opts.axis), None, False)
    plan = _CCompositePlan()
    _check(lib().sz3hip_composite_plan_for(C.byref(conf._c), _dtype_id(dt), reqs, len(items), C.byref(opts), C.byref(plan)))
    return {k: int(getattr(plan, k)) for k, _ in _CCompositePlan._fields_ if k != "reserved"}


def composite_points(tensor, axis, lut, lo, hi, out_type="rgba32f", reverse=False, accumulate=False, cutoff=float("inf"), level_bias=0, out=None, stream=None):
    """one float32 / float64 torch tensor of 1 .. 4 dimensions on a HIP device composited front to back along `axis` through the RGBA table
    `lut` (sz3hip_composite_device): what Stream.composite runs per box, over a plain view — any strides that are not negative. A point's
    value picks an entry by the window [lo, hi) as map's codes do; per visited point w = (1 - A) * a, the colours gain w * r, g, b and A
    gains w, in IEEE double — bit-defined; NaN points are skipped; a column stops once A >= cutoff. reverse: back to front in index terms.
    level_bias: every entry's 1 - a is squared that many times first. "rgba32f": a float32 tensor of the input's shape with 1 at `axis`
    plus a last dimension 4 (premultiplied colours, opacity) — a given `out` must have that dimension contiguous and its other strides
    divisible by 4; accumulate: the fold starts from what `out` holds. "rgba8": an int32 tensor, byte 0 = r .. byte 3 = a. Asynchronous
    on `stream`; returns `out`."""
    tname = _points_tensor("composite_points", tensor, (1, 4), "the tensor is empty or does not have 1 .. 4 dimensions")
    import torch
    N = tensor.dim()
    opts, name = _composite_opts(axis, N, lut, lo, hi, out_type, reverse, False, accumulate, cutoff, level_bias)
    if isinstance(lut, (int, np.integer)) or lut.device != tensor.device:
        raise ValueError("composite_points: lut must be a tensor on %s" % tensor.device)
    vec = name == "float32"
    flat = tuple(1 if j == int(opts.axis) else int(d) for j, d in enumerate(tensor.shape))
    full = flat + (4,) if vec else flat
    if out is None:
        if accumulate:
            raise ValueError("composite_points: accumulate needs `out`, the image to go on from")
        out = torch.empty(full, dtype=getattr(torch, name), device=tensor.device)
    if not _gpu_tensor(out) or str(out.dtype) != "torch." + name or tuple(out.shape) != full or out.device != tensor.device:
        raise ValueError("composite_points: out must be a %s tensor of shape %s on %s" % (name, full, tensor.device))
    dims = [int(d) for d in tensor.shape]
    sin = [int(v) for v in tensor.stride()]
    sout = _vector_strides(out, 4, "composite_points") if vec else [int(v) for v in out.stride()]
    _check(lib().sz3hip_composite_device(_SZ_TYPES[tname], N, (C.c_uint64 * N)(*dims), tensor.data_ptr(), (C.c_int64 * N)(*sin), C.byref(opts),
                                         out.data_ptr(), (C.c_int64 * N)(*sout), _stream_handle(tensor.device, stream)))
    return out


def set_chain_points(points):
    """development switch (sz3hip_debug_chain_points): a Stream request runs its coarsest levels — those whose every pass has at most
    `points` points for every box — in one launch; 0 switches the chain off"""
    lib().sz3hip_debug_chain_points(int(points))


def get_chain_points():
    return int(lib().sz3hip_debug_get_chain_points())


class Stream:
    """An opened stream (sz3hip_stream_*): open_stream / DeviceCompressor.open_stream do, once, everything of a partial
    decode that does not depend on the box — the container's host stage, the copy in, the Huffman stage over every unit — and keep the codes
    resident on the device; tiles / tile / region / coarse are then the reconstruction alone, bit for bit what decompress_tiles delivers;
    request takes boxes of several levels, each into a view of its own, in one launch sequence (section 16).
    A container that is no single interpolation stream is decoded in full once (stats()["fast"] == 0) and its requests are gathers.
    One request at a time: a Stream is not thread-safe. Use as a context manager, or close() it."""

    def __init__(self, handle, dtype, device):
        self._h = handle
        self.dtype = np.dtype(dtype)
        self.device = device
        c = Config(1)
        _check(lib().sz3hip_stream_config(self._h, C.byref(c._c)))
        self.conf = c

    def close(self):
        if self._h:
            lib().sz3hip_stream_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def stats(self):
        st = _CStreamStats()
        _check(lib().sz3hip_stream_stats(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in _CStreamStats._fields_}

    def tiles(self, level, boxes, out=None, stream=None):
        """boxes — (lo, shape) pairs in coordinates of the grid of every 2**level-th point — in one request; `out`: a list of contiguous
        tensors of the boxes' shapes on the stream's device, none overlapping another (default: allocated). Asynchronous on `stream`
        (a torch stream or a raw handle; default: the device's current stream). Returns the list of tensors."""
        arr, shapes = _boxes(self.conf.N, boxes)
        import torch
        if out is None:
            out = [torch.empty(shape, dtype=getattr(torch, self.dtype.name), device=self.device) for shape in shapes]
        out = list(out)
        if len(out) != len(shapes):
            raise ValueError("out needs one tensor per box (%d)" % len(shapes))
        for t, shape in zip(out, shapes):
            if not _gpu_tensor(t) or _np_dtype(t.dtype) != self.dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError("out must hold contiguous %s tensors of the boxes' shapes on a HIP device" % self.dtype)
        ptrs = (C.c_void_p * max(len(out), 1))(*[t.data_ptr() for t in out])
        _check(lib().sz3hip_stream_tiles(self._h, int(level), arr, len(shapes), ptrs, _stream_handle(self.device, stream)))
        return out

    def request(self, items, stream=None):
        """boxes of SEVERAL levels in one request (sz3hip_stream_request): `items` are (level, lo, shape) or
        (level, lo, shape, out) — lo / shape in coordinates of the grid of every 2**level-th point; `out` any view of that shape and the
        stream's dtype on its device, its element strides taken from the tensor: a rectangle of an atlas, a view with a step along x.
        Missing outputs are allocated. One launch sequence serves all boxes, whatever their levels. Asynchronous on `stream`, as tiles.
        Returns the list of tensors."""
        items = [tuple(it) for it in items]
        if any(len(it) not in (3, 4) for it in items):
            raise ValueError("an item is (level, lo, shape) or (level, lo, shape, out)")
        N = self.conf.N
        arr, shapes = _boxes(N, [(it[1], it[2]) for it in items])
        reqs, outs = _map_reqs(N, items, shapes, arr, self.dtype.name, self.device, True)
        _check(lib().sz3hip_stream_request(self._h, reqs, len(items), _stream_handle(self.device, stream)))
        return outs

    def reduce(self, items, bins=0, lo=0.0, hi=0.0, stream=None):
        """numbers about boxes, no output arrays (sz3hip_stream_reduce): `items` are (level, lo, shape) as request's.
        Per box n, n_nonfinite, argmin, argmax, min, max, shift, sum, sum_sq, mean, variance over exactly the values request would deliver,
        and with bins > 0 a histogram over [lo, hi) with an under and an over slot. The request's launch sequence with a reduction in the
        gather's place; bit-reproducible. Asynchronous on `stream`, as tiles; returns a ReduceResult (device tensors; .numpy() waits)."""
        reqs, n = _reduce_reqs(self.conf.N, items)
        res = _reduce_result(max(n, 1), bins, self.device)
        opts = _reduce_opts(bins, lo, hi)
        _check(lib().sz3hip_stream_reduce(self._h, reqs, n, C.byref(opts), res.stats.data_ptr(), None if res.hist is None else res.hist.data_ptr(),
                                          _stream_handle(self.device, stream)))
        return res

    def select(self, items, lo, hi, capacity, invert=False, nan=False, values=True, stream=None):
        """where in boxes the values lie in [lo, hi] (sz3hip_stream_select): `items` are (level, lo, shape) as
        request's; `capacity` an int or one per item. Per box the count of selected points and the `capacity` smallest selected box-local
        row-major indices, ascending, with (values) the points' raw values — over exactly the values request would deliver, compared as
        doubles. invert: the points that are not in the range; nan: NaN points too. The request's launch sequence with count, scan and
        write in the gather's place; deterministic. Asynchronous on `stream`, as tiles; returns a SelectResult (device tensors; .numpy()
        waits)."""
        import torch
        items = [tuple(it) for it in items]
        caps = _select_caps(capacity, len(items))
        res = _select_result(caps, values, getattr(torch, self.dtype.name), self.device)
        reqs, n = _select_reqs(self.conf.N, items, caps, res.index, res.value)
        opts = _select_opts(lo, hi, invert, nan)
        _check(lib().sz3hip_stream_select(self._h, reqs, n, C.byref(opts), res.heads.data_ptr(), _stream_handle(self.device, stream)))
        return res

    def map(self, items, out_type, lo=0.0, hi=0.0, nan_code=0, lut=None, stream=None):
        """texels out of boxes (sz3hip_stream_map): `items` are request's — (level, lo, shape) or (level, lo, shape,
        out) — with `out` a view of OUTPUT elements: dtype uint8 ("u8"), int16 ("u16": the code's two bytes, torch's uint16 is not a
        working storage type), float16 ("f16"), float32 ("f32") or int32 ("lut32": RGBA8 out of `lut`, an int32 tensor of 2 .. 1024
        entries on the device). Codes are those of the window [lo, hi) — the bin Stream.reduce would count the point in, the outer slots
        folded into the end codes; a NaN point becomes nan_code. The request's launch sequence with one mapping launch in the gather's
        place. Missing outputs are allocated. Asynchronous on `stream`, as tiles. Returns the list of tensors."""
        items = [tuple(it) for it in items]
        if any(len(it) not in (3, 4) for it in items):
            raise ValueError("an item is (level, lo, shape) or (level, lo, shape, out)")
        items = [it if len(it) == 3 or it[3] is not None else it[:3] for it in items]
        code, name = _map_type(out_type)
        N = self.conf.N
        arr, shapes = _boxes(N, [(it[1], it[2]) for it in items])
        reqs, outs = _map_reqs(N, items, shapes, arr, name, self.device, True)
        opts = _map_opts(code, lo, hi, nan_code, lut)
        _check(lib().sz3hip_stream_map(self._h, reqs, len(items), C.byref(opts), _stream_handle(self.device, stream)))
        return outs

    def sample(self, items, queries, mode="linear", clamp=False, fill=float("nan"), stream=None):
        """boxes sampled at fractional positions (sz3hip_stream_sample): `items` are (level, lo, shape); queries[i]
        belongs to item i and is a contiguous (n_i, N) float32 / float64 tensor of box-local coordinates on the device (slowest dimension
        first; all tensors of a call of one dtype), or a lattice (origin, steps, counts): 1 .. 3 axes, slowest first, a step of N entries
        and a count each. mode "nearest": the nearest point's bytes; "linear": the multilinear interpolation in double, rounded once. A
        query outside the box yields `fill`, or is clamped into it (clamp=True); a NaN coordinate always yields `fill`. The request's
        launch sequence with one sampling launch in the gather's place. Asynchronous on `stream`, as tiles. Returns the list of tensors of
        the stream's dtype: (n_i,) for coordinates, of shape `counts` for a lattice."""
        import torch
        reqs, n, cname, shapes = _sample_reqs(self.conf.N, items, queries)
        for i, q in enumerate(queries):
            if isinstance(q, (int, np.integer)):
                raise ValueError("query %d: a query is a coordinate tensor or a lattice (origin, steps, counts)" % i)
            if _is_tensor(q) and (not _gpu_tensor(q) or q.device != self.device):
                raise ValueError("query %d: the coordinates must be on %s" % (i, self.device))
        outs = [torch.empty(shape, dtype=getattr(torch, np.dtype(self.dtype).name), device=self.device) for shape in shapes]
        for i, t in enumerate(outs):
            reqs[i].d_out = t.data_ptr()
        opts = _sample_opts(mode, clamp, fill, cname)
        _check(lib().sz3hip_stream_sample(self._h, reqs, n, C.byref(opts), _stream_handle(self.device, stream)))
        return outs

    def project(self, items, op, axis, out_dtype=None, fill=float("nan"), stream=None):
        """boxes collapsed along one axis (sz3hip_stream_project): `items` are request's — (level, lo, shape) or (level,
        lo, shape, out) — with `out` a view of OUTPUT elements of the box's shape with 1 at `axis`. op: "min", "max", "sum", "mean" (values:
        the stream's dtype, or `out_dtype` float32 / float64), "argmin", "argmax", "count" (uint32 in int32 tensors). NaN and +-Inf points are
        left out; a column without a finite point gives `fill` (min, max, mean), 0 (sum, count) or the axis' extent (argmin, argmax). The
        sum is the sequential fold in double along the axis, rounded once: bit-defined. The request's launch sequence with one projecting
        launch in the gather's place. Missing outputs are allocated. Asynchronous on `stream`, as tiles. Returns the list of tensors."""
        items = _project_items(items)
        N = self.conf.N
        opts, name = _project_opts(op, axis, N, np.dtype(self.dtype).name, out_dtype, fill)
        arr, shapes = _boxes(N, [(it[1], it[2]) for it in items])
        flat = [tuple(1 if j == opts.axis else v for j, v in enumerate(shape)) for shape in shapes]
        reqs, outs = _map_reqs(N, items, flat, arr, name, self.device, True)
        _check(lib().sz3hip_stream_project(self._h, reqs, len(items), C.byref(opts), _stream_handle(self.device, stream)))
        return outs

    def gradient(self, items, op, axis=0, spacing=None, out_dtype=None, interior=False, stream=None):
        """the derivatives of boxes by central differences (sz3hip_stream_gradient): `items` are request's — (level,
        lo, shape) or (level, lo, shape, out) — with `out` a view of OUTPUT elements of the box's shape. op: "deriv" (along `axis`),
        "mag2", "mag" or "vector" (a last dimension of N components, slowest axis first; a given `out` must have it contiguous and its
        other strides divisible by N). spacing: the level-0 grid step, one scalar or one value per axis (default 1.0); a box of level k
        is differentiated with 2**k times it. interior: every box loses its first and last point along every differentiated axis — ask
        for a tile with a halo of one point and get the tile, every point a central difference. In IEEE double, rounded once into the
        stream's dtype or `out_dtype`: bit-defined. The request's launch sequence with one differentiating launch in the gather's place.
        Missing outputs are allocated. Asynchronous on `stream`, as tiles. Returns the list of tensors."""
        items = _project_items(items)
        N = self.conf.N
        opts, name = _gradient_opts(op, axis, N, np.dtype(self.dtype).name, spacing, out_dtype, interior)
        arr, shapes = _boxes(N, [(it[1], it[2]) for it in items])
        reqs, outs = _gradient_reqs(N, items, shapes, arr, name, opts, self.device, True)
        _check(lib().sz3hip_stream_gradient(self._h, reqs, len(items), C.byref(opts), _stream_handle(self.device, stream)))
        return outs

    def composite(self, items, axis, lut, lo, hi, out_type="rgba32f", reverse=False, level_opacity=False, accumulate=False, cutoff=float("inf"),
                  level_bias=0, stream=None):
        """boxes composited front to back along one axis through an RGBA transfer function (sz3hip_stream_composite):
        `items` are request's — (level, lo, shape) or (level, lo, shape, out) — with `out` a view of OUTPUT elements of the box's shape with
        1 at `axis`. `lut`: a contiguous float32 tensor of shape (2 .. 1024, 4) on the device, r, g, b, a per entry; the window [lo, hi)
        picks a point's entry as map's codes do. Per visited point w = (1 - A) * a, the colours gain w * r, g, b and A gains w, in IEEE
        double: bit-defined. NaN points are skipped; a column stops once A >= cutoff. reverse: the column is visited descending.
        level_opacity: a box of level k has every entry's 1 - a squared k more times (it steps 2**k times as far per sample); level_bias:
        squarings for every box. "rgba32f": float32 tensors with a last dimension 4 (premultiplied colours, opacity) — a given `out` must
        have it contiguous and its other strides divisible by 4; accumulate: the fold goes on from what `out` holds. "rgba8": int32
        tensors, byte 0 = r .. byte 3 = a. The request's launch sequence with one compositing launch in the gather's place. Missing
        outputs are allocated. Asynchronous on `stream`, as tiles. Returns the list of tensors."""
        items = _project_items(items)
        N = self.conf.N
        opts, name = _composite_opts(axis, N, lut, lo, hi, out_type, reverse, level_opacity, accumulate, cutoff, level_bias)
        if isinstance(lut, (int, np.integer)) or lut.device != self.device:
            raise ValueError("lut must be a tensor on %s" % self.device)
        if accumulate and any(len(it) != 4 for it in items):
            raise ValueError("accumulate needs every item's `out`, the image to go on from")
        arr, shapes = _boxes(N, [(it[1], it[2]) for it in items])
        reqs, outs = _composite_reqs(N, items, shapes, arr, name, int(opts.axis), self.device, True)
        _check(lib().sz3hip_stream_composite(self._h, reqs, len(items), C.byref(opts), _stream_handle(self.device, stream)))
        return outs

    def tile(self, level, lo, shape, out=None, stream=None):
        """one box of the grid of every 2**level-th point (tiles with one box)"""
        return self.tiles(level, [(lo, shape)], None if out is None else [out], stream)[0]

    def region(self, lo, shape, out=None, stream=None):
        """one box of the array itself (tile at level 0)"""
        return self.tile(0, lo, shape, out, stream)

    def coarse(self, level, out=None, stream=None):
        """every 2**level-th point of the array (the whole grid as one box)"""
        dims = coarse_dims(self.conf, level)
        return self.tile(level, (0,) * len(dims), dims, out, stream)


def open_stream(blob, dtype, device=None):
    """Opens a container for many partial decodes (sz3hip_stream_open): returns a Stream. The blob may be freed or overwritten afterwards.
    `device`: a torch device, its index, or None for the current one. float32 / float64."""
    blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob)
    npdt = _np_dtype(dtype)
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("open_stream decodes into device memory: device must be a HIP device")
    index = torch.cuda.current_device() if dev.index is None else dev.index
    h = C.c_void_p()
    conf = Config(1)
    _check(lib().sz3hip_stream_open(C.byref(h), C.byref(conf._c), _dtype_id(npdt), blob.ctypes.data, blob.size, index))
    return Stream(h, npdt, torch.device("cuda", index))


class VerifyStats(dict):
    """the fields of sz3hip_verify_stats (include/sz3hip.h), as items and as attributes"""
    __getattr__ = dict.__getitem__


def _is_tensor(x):
    import sys
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor)


def verify_stats(ori, dec, bound=None, stream=None):
    """Error statistics of two torch tensors on the same HIP device with the same shape and dtype (one of the ten element types),
    reduced on that device by one kernel that reads each tensor once (sz3hip_verify_device): the tensors do not cross the host link.
    Views are welcome, each with its own strides (size-1 dimensions are dropped; at most 4 are left). `bound`: n_over / first_over count
    the positions with |dec - ori| > bound (None: no bound). `stream` (a torch stream or a raw handle; default: the device's current
    stream) is what the library waits for before it reads the tensors. Returns a VerifyStats: n, n_nonfinite, n_nonfinite_mismatch,
    n_over, first_over, argmax, min, max, max_diff, max_pw_rel, sum_ori, sum_dec, sum_sq_err, sum_sq_dec, psnr, nrmse, l2_err,
    l2_err_norm, acEff (include/sz3hip.h says what each means, also for positions that are not finite)."""
    if not (_is_tensor(ori) and _is_tensor(dec)):
        raise TypeError("verify_stats takes two torch tensors on a HIP device (got %s and %s)" % (type(ori).__name__, type(dec).__name__))
    if not (_gpu_tensor(ori) and _gpu_tensor(dec)):
        raise ValueError("verify_stats: both tensors must be on a HIP device (they are on %s and %s)" % (ori.device, dec.device))
    if ori.device != dec.device:
        raise ValueError("verify_stats: the tensors are on different devices (%s and %s)" % (ori.device, dec.device))
    if tuple(ori.shape) != tuple(dec.shape):
        raise ValueError("verify_stats: the shapes differ (%s and %s)" % (tuple(ori.shape), tuple(dec.shape)))
    if ori.dtype != dec.dtype:
        raise TypeError("verify_stats: the dtypes differ (%s and %s)" % (ori.dtype, dec.dtype))
    name = str(ori.dtype).replace("torch.", "")
    if name not in _SZ_TYPES:
        raise TypeError("sz3_amd supports float32 / float64 and 8 ... 64-bit integers (got %s)" % ori.dtype)
    if ori.numel() == 0:
        raise ValueError("verify_stats: the tensors are empty")
    keep = [i for i, d in enumerate(ori.shape) if int(d) != 1]
    if len(keep) > 4:
        raise ValueError("verify_stats: %d dimensions above size 1 (at most 4 are supported)" % len(keep))
    dims = [int(ori.shape[i]) for i in keep] or [1]
    so = [int(ori.stride(i)) for i in keep] or [1]
    sd = [int(dec.stride(i)) for i in keep] or [1]
    N = len(dims)
    st = _CVerifyStats()
    b = -1.0 if bound is None else float(bound)
    _check(lib().sz3hip_verify_device(_SZ_TYPES[name], N, (C.c_uint64 * N)(*dims), ori.data_ptr(), (C.c_int64 * N)(*so), dec.data_ptr(),
                                      (C.c_int64 * N)(*sd), b, C.byref(st), _stream_handle(ori.device, stream)))
    return VerifyStats((k, getattr(st, k)) for k, _ in _CVerifyStats._fields_)


def verify(ori, dec):
    """sz.verify (sz.pyx:368-405, utils/Statistic.hpp:80-137): (max_diff, psnr, nrmse) in float64. Two torch tensors on a HIP device
    are compared where they lie (verify_stats), with the same conventions: the same triple whichever side the arrays are on."""
    if _gpu_tensor(ori) and _gpu_tensor(dec):
        st = verify_stats(ori, dec)
        rng = st.max - st.min
        mse = st.sum_sq_err / (st.n - st.n_nonfinite) if st.n > st.n_nonfinite else float("nan")
        psnr = st.psnr if mse > 0 and rng > 0 else float("inf")
        nrmse = st.nrmse if rng > 0 else 0.0
        return float(st.max_diff), float(psnr), float(nrmse)
    o = np.asarray(ori, dtype=np.float64).ravel()
    d = np.asarray(dec, dtype=np.float64).ravel()
    err = np.abs(d - o)
    rng = o.max() - o.min()
    mse = float(np.mean(err * err))
    psnr = 20 * np.log10(rng) - 10 * np.log10(mse) if mse > 0 and rng > 0 else float("inf")
    nrmse = np.sqrt(mse) / rng if rng > 0 else 0.0
    return float(err.max()), float(psnr), float(nrmse)


# ---- device-resident API ---------------------------------------------------------------------------------------
class DeviceCompressor:
    """Workspace + entry points for arrays that already live in HBM (pointers are plain ints, e.g. tensor.data_ptr())."""

    def __init__(self, max_elems, dtype, device=0):
        self.dtype = np.dtype(dtype)
        self._h = lib().sz3hip_ctx_create(int(device), int(max_elems), _dtype_id(dtype))
        if not self._h:
            raise SZ3HipError(-4, lib().sz3hip_last_error().decode())
        self.max_elems = int(max_elems)
        self.device = int(device)

    def close(self):
        if self._h:
            lib().sz3hip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def payload_bound(self, n, worst_case=False):
        """device payload bound; worst_case=True leaves room for outlier lists of n / 8 entries (compress then grows
        its lists on demand instead of raising SZ3HIP_EOUTLIERS)"""
        if worst_case:
            return int(lib().sz3hip_payload_bound_max(self._h, int(n)))
        return int(lib().sz3hip_payload_bound(self._h, int(n)))

    def minmax(self, d_in, n, stream=0):
        mn, mx = C.c_double(), C.c_double()
        _check(lib().sz3hip_minmax_device(self._h, d_in, int(n), C.byref(mn), C.byref(mx), stream))
        return mn.value, mx.value

    def stage1(self, conf, d_in, stream=0):
        _check(lib().sz3hip_compress_stage1(self._h, C.byref(conf._c), d_in, stream))

    def histogram_ptr(self):
        return int(lib().sz3hip_histogram_ptr(self._h)), int(lib().sz3hip_histogram_len(self._h))

    def set_histogram(self, d_hist):
        _check(lib().sz3hip_ctx_set_histogram(self._h, d_hist))

    def stage2(self, d_payload, cap, stream=0):
        _check(lib().sz3hip_compress_stage2(self._h, d_payload, int(cap), stream))

    def finish(self, stream=0):
        sz = C.c_size_t()
        _check(lib().sz3hip_compress_finish(self._h, C.byref(sz), stream))
        return int(sz.value)

    def compress(self, conf, d_in, d_payload, cap, stream=0):
        sz = C.c_size_t()
        _check(lib().sz3hip_compress_device(self._h, C.byref(conf._c), d_in, d_payload, int(cap), C.byref(sz), stream))
        return int(sz.value)

    def decompress(self, d_payload, size, d_out, stream=0):
        _check(lib().sz3hip_decompress_device(self._h, d_payload, int(size), d_out, stream))

    def decompress_coarse(self, d_payload, size, level, d_out, stream=0):
        """every 2**level-th point of an interpolation payload into d_out (prod(coarse_dims) elements, contiguous)"""
        _check(lib().sz3hip_decompress_device_coarse(self._h, d_payload, int(size), int(level), d_out, stream))

    def decompress_region(self, d_payload, size, lo, shape, d_out, stream=0):
        """the box [lo, lo + shape) of an interpolation payload into d_out (prod(shape) elements, contiguous)"""
        lo, shape = tuple(int(v) for v in lo), tuple(int(v) for v in shape)
        if len(lo) != len(shape) or not 1 <= len(lo) <= 4:
            raise ValueError("lo and shape need one entry per extent of the array")
        _check(lib().sz3hip_decompress_device_region(self._h, d_payload, int(size), (C.c_uint64 * 4)(*lo), (C.c_uint64 * 4)(*shape), d_out, stream))

    def decompress_tile(self, d_payload, size, level, lo, shape, d_out, stream=0):
        """the box [lo, lo + shape) of the grid of every 2**level-th point of an interpolation payload into d_out (prod(shape) elements,
        contiguous); lo / shape are coarse-grid coordinates"""
        lo, shape = tuple(int(v) for v in lo), tuple(int(v) for v in shape)
        if len(lo) != len(shape) or not 1 <= len(lo) <= 4:
            raise ValueError("lo and shape need one entry per extent of the array")
        _check(lib().sz3hip_decompress_device_tile(self._h, d_payload, int(size), int(level), (C.c_uint64 * 4)(*lo), (C.c_uint64 * 4)(*shape), d_out, stream))

    def decompress_tiles(self, d_payload, size, level, boxes, d_outs, stream=0):
        """several boxes — (lo, shape) pairs in coarse-grid coordinates — of the grid of every 2**level-th point of an interpolation payload
        in one call; d_outs: one device pointer per box, its array contiguous"""
        boxes = list(boxes)
        N = len(boxes[0][0]) if boxes else 1
        if not 1 <= N <= 4:
            raise ValueError("lo and shape need one entry per extent of the array")
        arr, shapes = _boxes(N, boxes)
        d_outs = [int(p) for p in d_outs]
        if len(d_outs) != len(shapes):
            raise ValueError("d_outs needs one pointer per box (%d)" % len(shapes))
        ptrs = (C.c_void_p * max(len(d_outs), 1))(*d_outs)
        _check(lib().sz3hip_decompress_device_tiles(self._h, d_payload, int(size), int(level), arr, len(shapes), ptrs, stream))

    def open_stream(self, d_payload, size, stream=0):
        """Opens a payload of this context's type that lies in device memory (sz3hip_stream_open_payload): returns a Stream that owns
        everything its requests read — the payload may be freed or overwritten afterwards. `stream`: what produced the payload is waited for there."""
        import torch
        h = C.c_void_p()
        _check(lib().sz3hip_stream_open_payload(C.byref(h), int(self.device), _dtype_id(self.dtype), d_payload, int(size), stream))
        return Stream(h, self.dtype, torch.device("cuda", int(self.device)))

    def region_scratch(self):
        """capacity of the context's region scratch in elements (0 before its first region call)"""
        return int(lib().sz3hip_debug_region_scratch(self._h))

    def stats(self):
        st = _CStats()
        lib().sz3hip_get_stats(self._h, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in _CStats._fields_}

    def tuner_report(self):
        """what the ALGO_INTERP_LORENZO auto-tuner decided in the last stage1 / compress call (sz3hip_get_tuner_report)"""
        r = _CTunerReport()
        lib().sz3hip_get_tuner_report(self._h, C.byref(r))
        out = {k: getattr(r, k) for k, _ in _CTunerReport._fields_ if k not in ("est_bytes", "speculated")}
        out["est_bytes"] = [float(x) for x in r.est_bytes]
        self.speculated = int(r.speculated)  # (how stage 1 related to the tuner; not part of the decision the report describes)
        return out

    def set_profiling(self, on=True):
        lib().sz3hip_set_profiling(self._h, int(on))

    def forget(self):
        """drop what earlier calls left in the context (kernel forms, windows, tuner outcome, code book): the next call is a first call"""
        lib().sz3hip_ctx_forget(self._h)

    def set_speculation(self, on=True, backoff=True):
        """on=False: every stage 2 builds its code book first; backoff=False: a miss does not make the next calls sit out (tests)"""
        lib().sz3hip_ctx_set_speculation(self._h, (0 if backoff else 2) if on else 1)

    def set_deterministic(self, on=True):
        """on: the previous call's code book stands only when it IS this call's book — the payload is a pure function of the input
        (off, the device API's default: also when it is complete over this call's alphabet and within 1/1024 of its own book's size)"""
        lib().sz3hip_ctx_set_deterministic(self._h, int(on))

    def set_tuner_exact(self, on=True):
        """on: the ALGO_INTERP_LORENZO tuner prices its trials the reference's way (Huffman tree + bits + zstd on the host: the reference's
        own compressed sizes and decisions, milliseconds per tuning); off: the device-side estimate (include/sz3hip.h)"""
        lib().sz3hip_ctx_set_tuner_exact(self._h, int(on))

    def set_fused(self, on=True):
        """opt in to the fused stage 1 (the previous call's book codes inside the predictor kernel; off by default)"""
        lib().sz3hip_ctx_set_fused(self._h, int(on))

    @property
    def fused(self):
        """the last finished compression ran the fused stage 1 (coded with the previous call's book inside the predictor kernel)"""
        return bool(lib().sz3hip_last_call_fused(self._h))

    @property
    def q16(self):
        """the last finished compression ran the 16-bit form of the one-byte stage-1 kernel (f32, lattice values within +-4095)"""
        return bool(lib().sz3hip_last_call_q16(self._h))

    def spec_stats(self):
        h, m = C.c_uint32(), C.c_uint32()
        lib().sz3hip_get_spec_stats(self._h, C.byref(h), C.byref(m))
        return int(h.value), int(m.value)

    def payload_bound_conf(self, conf, worst_case=False):
        return int(lib().sz3hip_payload_bound_conf(self._h, C.byref(conf._c), int(bool(worst_case))))

    def stage_times(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        k = lib().sz3hip_get_stage_times(self._h, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(k)}

    def debug_codes(self, n):
        out = np.empty(int(n), dtype=np.uint16)
        _check(lib().sz3hip_debug_copy_codes(self._h, out.ctypes.data, int(n)))
        return out


# ---- multi-GPU exchange (RCCL over xGMI, in the library) --------------------------------------------------------
COMM_ID_BYTES = 128


class Comm:
    """sz3hip_comm: the RCCL communicator of the slab-parallel path. ``Comm.local(ndev)`` = one process drives ndev GPUs;
    ``Comm.rank(nranks, rank, device, id)`` = one process per GPU, ``id`` being ``Comm.unique_id()`` of rank 0 shipped by
    the launcher (sz3_amd.distributed.init_comm does that over torch.distributed)."""

    def __init__(self, handle):
        if not handle:
            raise SZ3HipError(lib().sz3hip_last_error_code(), lib().sz3hip_last_error().decode())
        self._h = handle

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * COMM_ID_BYTES)()
        _check(lib().sz3hip_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def local(cls, ndev=0, devices=None):
        arr = (C.c_int * len(devices))(*devices) if devices else None
        return cls(lib().sz3hip_comm_create_local(int(ndev if not devices else len(devices)), arr))

    @classmethod
    def rank(cls, nranks, rank, device, id_bytes):
        b = (C.c_ubyte * COMM_ID_BYTES).from_buffer_copy(bytes(id_bytes))
        return cls(lib().sz3hip_comm_create_rank(int(nranks), int(rank), int(device), b))

    def close(self):
        if self._h:
            lib().sz3hip_comm_destroy(self._h)
            self._h = None

    @property
    def size(self):
        return int(lib().sz3hip_comm_size(self._h))

    @property
    def my_rank(self):
        return int(lib().sz3hip_comm_rank(self._h))

    @property
    def local_size(self):
        return int(lib().sz3hip_comm_local_size(self._h))

    def device(self, member=0):
        return int(lib().sz3hip_comm_device(self._h, member))

    def allreduce_histogram(self, compressors, streams):
        """in-place sum of the code histograms of the local members' DeviceCompressors, enqueued on their streams"""
        m = len(compressors)
        ctxs = (C.c_void_p * m)(*[dc._h for dc in compressors])
        st = (C.c_void_p * m)(*[int(x) if x else None for x in streams])
        _check(lib().sz3hip_comm_allreduce_histogram(self._h, ctxs, st))

    def allreduce_u64(self, ptrs, count, streams):
        m = len(ptrs)
        bufs = (C.c_void_p * m)(*[int(p) for p in ptrs])
        st = (C.c_void_p * m)(*[int(x) if x else None for x in streams])
        _check(lib().sz3hip_comm_allreduce_u64(self._h, bufs, int(count), st))

    def allreduce_minmax(self, mins, maxs, streams):
        m = len(mins)
        a = (C.c_double * m)(*mins)
        b = (C.c_double * m)(*maxs)
        st = (C.c_void_p * m)(*[int(x) if x else None for x in streams])
        _check(lib().sz3hip_comm_allreduce_minmax(self._h, a, b, st))
        return list(a), list(b)


def compress_rank(comm, slab, global_conf):
    """this rank's slab of a slab-parallel compress (sz3hip_compress_rank; collective): returns (blob, slab Config)"""
    a = np.ascontiguousarray(slab)
    sc = Config(1)
    cap = int(lib().sz3hip_compress_bound(C.byref(global_conf._c), _dtype_id(a.dtype)))  # (>= the slab's own bound)
    out = np.empty(cap, dtype=np.uint8)
    n = lib().sz3hip_compress_rank(comm._h, C.byref(global_conf._c), _dtype_id(a.dtype), a.ctypes.data, out.ctypes.data, cap, C.byref(sc._c))
    if n == 0:
        raise SZ3HipError(lib().sz3hip_last_error_code(), lib().sz3hip_last_error().decode())
    return out[:n].copy(), sc


def assemble_container(global_conf, dtype, slab_confs, blobs):
    """sz3hip_assemble_container: the multi-slab SZ3 stream from the ranks' blobs and Configs (rank order)"""
    G = len(blobs)
    arrs = [np.ascontiguousarray(np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray)) else b) for b in blobs]
    confs = (_CConfig * G)()
    for i, c in enumerate(slab_confs):
        C.memmove(C.byref(confs[i]), C.byref(c._c), C.sizeof(_CConfig))
    ptrs = (C.c_void_p * G)(*[a.ctypes.data for a in arrs])
    sizes = (C.c_size_t * G)(*[a.size for a in arrs])
    cap = 16 + 4 + G * (8 + 160) + 160 + sum(a.size for a in arrs)
    out = np.empty(cap, dtype=np.uint8)
    n = lib().sz3hip_assemble_container(C.byref(global_conf._c), _dtype_id(dtype), G, confs, ptrs, sizes, out.ctypes.data, cap)
    if n == 0:
        raise SZ3HipError(lib().sz3hip_last_error_code(), lib().sz3hip_last_error().decode())
    return out[:n]

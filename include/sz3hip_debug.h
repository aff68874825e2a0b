/* sz3hip_debug.h — the development switches of sz3hip_debug_flags(), one name per meaning.
 *
 * The word is process-wide and 0 in production. All 32 bits are taken, and many carry several unrelated meanings: such a bit has
 * several enumerators of EQUAL value, listed next to each other, and setting it switches every one of them. Each comment names the
 * function the switch gates and the enumerators it shares its bit with. Unless a comment says otherwise a switch chooses between
 * two equivalent paths and leaves the results unchanged (the tests compare them).
 *   "lab build": has an effect only in the library built with -DSZ3HIP_LAB (python -m sz3_amd.build --lab);
 *   "LAB_ABLATE": only in a library compiled with -DLAB_ABLATE (tools/k1_lab.py);
 *   "WRONG RESULTS": an ablation for timing, the output is not a valid stream / array.
 * The values are ABI (tools and committed profiles quote the numbers): a new switch needs a new word, not a reused bit. */
#ifndef SZ3HIP_DEBUG_H
#define SZ3HIP_DEBUG_H

enum sz3hip_dbg {
    /* ---- bit 0 ---- */
    SZ3HIP_DBG_CB_COMPACT_IN_WG = 1,       /* szk_launch_codebook: the wide code book compacts the histogram inside its own workgroup (no k_cb_compact launch, no k_cb_assign). Shares K1_LAB_NO_HIST */
    SZ3HIP_DBG_K1_LAB_NO_HIST = 1,         /* LAB_ABLATE, WRONG RESULTS: k_lorenzo_quant_v4 and the marching body leave the histogram out. Shares CB_COMPACT_IN_WG */
    /* ---- bit 1 ---- */
    SZ3HIP_DBG_DEC_MULTI_SYM = 2,          /* lab build: sz3hip_decompress_device takes the multi-symbol lookup table for small code books. Shares K1_NO_CODE_STORES */
    SZ3HIP_DBG_K1_NO_CODE_STORES = 2,      /* WRONG RESULTS: k_lorenzo_quant_v4 does not store its codes (every build); the marching body likewise under LAB_ABLATE. Shares DEC_MULTI_SYM */
    /* ---- bit 2 ---- */
    SZ3HIP_DBG_BLKDEC_FORCE_RETRY = 4,     /* szk_launch_blk_decompress: after the one-launch block decoder, the retry through the launch-per-front decoders as if a flag poll had given up. Shares K1_V4_NO_STENCIL */
    SZ3HIP_DBG_K1_V4_NO_STENCIL = 4,       /* WRONG RESULTS: k_lorenzo_quant_v4 skips the stencil's LDS reads. Shares BLKDEC_FORCE_RETRY */
    /* ---- bit 3 ---- */
    SZ3HIP_DBG_K1_NO_Q16 = 8,              /* launch_march_w: no 16-bit form of the one-launch stage-1 kernel (k_lorenzo_quant_march3q) */
    /* ---- bit 4 ---- */
    SZ3HIP_DBG_BLKDEC_LOCAL_EXPANDED = 16, /* blk_decompress_impl, 3-D blocks of 6^3: the local pass a wave per block from an expanded copy of the deltas (k_blk_local3) instead of k_blk_local3v. Shares K1_V4_NO_PREFETCH, PACK_LAB_NO_STORES */
    SZ3HIP_DBG_K1_V4_NO_PREFETCH = 16,     /* k_lorenzo_quant_v4 fetches a tile when it starts on it, not one tile ahead (slower, same output). Shares BLKDEC_LOCAL_EXPANDED, PACK_LAB_NO_STORES */
    SZ3HIP_DBG_PACK_LAB_NO_STORES = 16,    /* lab build, WRONG RESULTS: k_pack_b does not store the bit stream (szk_launch_encode). Shares BLKDEC_LOCAL_EXPANDED, K1_V4_NO_PREFETCH */
    /* ---- bit 5 ---- */
    SZ3HIP_DBG_K1_NO_MARCH = 32,           /* launch_k1: no marching kernels (the tiled v4 / generic kernels, two-byte codes) */
    /* ---- bit 6 ---- */
    SZ3HIP_DBG_K1_NO_NARROW = 64,          /* szk_launch_k1: no one-byte codes */
    /* ---- bit 7 ---- */
    SZ3HIP_DBG_INTERP_NO_VEC = 128,        /* sz3hip_debug_flags -> szk_interp_novec: interpolation pass by pass, one point per thread (no 8-wide level-1 kernels, no level kernels) */
    /* ---- bit 8 ---- */
    SZ3HIP_DBG_K1_NO_WIDTH_SPEC = 256,     /* launch_k1 / launch_march_w: no stage-1 specialisation by code width (the run-time-width marching kernel, no k_sample) */
    /* ---- bit 9 ---- */
    SZ3HIP_DBG_DEC_NO_FUSED_X = 512,       /* sz3hip_decompress_device: the Huffman decoder without the fused x prefix sum. Shares PACK_LAB_ONE_UNIT */
    SZ3HIP_DBG_PACK_LAB_ONE_UNIT = 512,    /* lab build, WRONG RESULTS: every unit of k_pack_b reads the first unit's codes (szk_launch_encode). Shares DEC_NO_FUSED_X */
    /* ---- bit 10 ---- */
    SZ3HIP_DBG_CB_ONE_CLASS = 1024,        /* szk_launch_codebook -> codebook_wide: the one-class construction instead of the two-class one */
    /* ---- bit 11 ---- */
    SZ3HIP_DBG_K1_NO_FUSED = 2048,         /* lab build: launch_march_w does not take the fused stage 1 (k_lorenzo_quant_march3f). Shares BLK_RANK_3_LAUNCHES, BLK_SIDE_8_LAUNCHES */
    SZ3HIP_DBG_BLK_RANK_3_LAUNCHES = 2048, /* launch_blk_rank: the rank pass in three launches whatever the block count. Shares K1_NO_FUSED, BLK_SIDE_8_LAUNCHES */
    SZ3HIP_DBG_BLK_SIDE_8_LAUNCHES = 2048, /* launch_blk_side_build / szk_blk_side_small: the side section in eight launches whatever the block count. Shares K1_NO_FUSED, BLK_RANK_3_LAUNCHES */
    /* ---- bit 12 ---- */
    SZ3HIP_DBG_K1_NO_XCD_ORDER = 4096,     /* the marching kernels (device code) take their tasks in launch order, not in the XCD-aware order. Shares CB_NO_SPEC_WIDE */
    SZ3HIP_DBG_CB_NO_SPEC_WIDE = 4096,     /* stage2_launch: no speculative stage 2 for wide alphabets (this call's book on the side stream beside the encoder). Shares K1_NO_XCD_ORDER */
    /* ---- bit 13 ---- */
    SZ3HIP_DBG_INTERP_HIST_BIG = 8192,     /* stage1_interp: the interpolation histogram with the large tier and the windowed tail passes whatever the history */
    /* ---- bit 14 ---- */
    SZ3HIP_DBG_BLK_OFF = 16384,            /* sz3hip_compress_stage1: predictor sets with Lorenzo-2 / regression fall back to plain Lorenzo (no block path) */
    /* ---- bit 15 ---- */
    SZ3HIP_DBG_PACK_OLD = 32768,           /* szk_launch_encode: k_pack instead of k_pack_b for one-byte codes (a call with a sampled book keeps k_pack_b). Shares BLKDEC_GROUPS_3 */
    SZ3HIP_DBG_BLKDEC_GROUPS_3 = 32768,    /* blk_decompress_impl, 3-D blocks of 6^3: groups of 3 x 3 x 3 blocks in closed form, a launch per front (k_blk_decode_gf); also what the retry of a one-launch decoder takes. Shares PACK_OLD */
    /* ---- bit 16 ---- */
    SZ3HIP_DBG_CB_NO_SAMPLED = 65536,      /* lorenzo_k1: no sampled book (the exact histogram's book). Shares BLKDEC_PER_FRONT */
    SZ3HIP_DBG_BLKDEC_PER_FRONT = 65536,   /* blk_decompress_impl: no one-launch decoder (k_blk_wave3 / k_blkn_wave2). 2-D: groups of 4 x 4 blocks, a launch per front; 3-D: groups of 2 x 2 x 2 blocks inverted by line scans where sz3hip_regress.hip is compiled with -DSZ3HIP_LAB, else the block-per-wave form. Also ORed into the retry of a one-launch decoder. Shares CB_NO_SAMPLED */
    /* ---- bit 17 ---- */
    SZ3HIP_DBG_CTX_NO_MEMORY = 131072,     /* contexts act as if every call were their first: launch_k1 (no one-launch form by the previous code width), cb_params_from (both code-book forms launched), book_spec_ok (no stage 2 with the previous book), sz3hip_compress_stage1 (no stage 1 beside the tuner) */
    /* ---- bit 18 ---- */
    SZ3HIP_DBG_CB_SERIAL_MERGE = 262144,   /* szk_launch_codebook -> cb_small: the Huffman merge by one wave, pick by pick, instead of the round-parallel merge */
    /* ---- bit 19 ---- */
    SZ3HIP_DBG_DEC_NO_STORES = 524288,     /* WRONG RESULTS (tools/dec_lab.py): k_decode with the fused x prefix sum, without output stores */
    /* ---- bit 20 ---- */
    SZ3HIP_DBG_DEC_DIRECT_STORES = 1048576, /* experiment (tools/dec_lab.py), slower and not covered by a test, treat as WRONG RESULTS: k_decode stores from each lane directly, without the wave's cooperative stores */
    /* ---- bit 21 ---- */
    SZ3HIP_DBG_DEC_NO_HALF = 2097152,      /* sz3hip_decompress_device: no half-width intermediates (the full-width chain only) */
    /* ---- bit 22 ---- */
    SZ3HIP_DBG_INTERP_LEVELS_ANY_SIZE = 4194304, /* sz3hip_debug_flags -> szk_interp_min_blocks: the interpolation level kernels whatever the array's size (normally from 256 blocks up). Shares K1_NO_SAMP_IN_LAUNCH */
    SZ3HIP_DBG_K1_NO_SAMP_IN_LAUNCH = 4194304,   /* launch_march_w: no sampling workgroups inside stage 1's launch (k_sample behind it). Shares INTERP_LEVELS_ANY_SIZE */
    /* ---- bit 23 ---- */
    SZ3HIP_DBG_BLKDEC_BLOCK_PER_WAVE = 8388608,  /* blk_decompress_impl, 2-D / 3-D: the launch-per-front decoder with a block per wave. Shares K1_Q16_PLAIN_STORES */
    SZ3HIP_DBG_K1_Q16_PLAIN_STORES = 8388608,    /* k_lorenzo_quant_march3q stores its codes with plain instead of non-temporal stores. Shares BLKDEC_BLOCK_PER_WAVE */
    /* ---- bit 24 ---- */
    SZ3HIP_DBG_K1_NO_DEFER_FOLD = 16777216,      /* lorenzo_k1: stage 1 folds its histogram rows itself (not in the encoder's scan launch) */
    /* ---- bit 25 ---- */
    SZ3HIP_DBG_PACK_NO_SEG_BITS = 33554432,      /* stage1_lorenzo: stage 2 ignores the segment bit sums of stage 1 and runs its own bits pass */
    /* ---- bit 26 ---- */
    SZ3HIP_DBG_BLK_FIT_TILES = 67108864,         /* szk_launch_blk_compress: a given selection is coded by the tile kernels, not element by element (k_blk_rows) */
    /* ---- bit 27 ---- */
    SZ3HIP_DBG_BLK_1D_WAVE_PER_BLOCK = 134217728, /* launch_blkn_compress / blk_decompress_impl, 1-D: a wave per block instead of four blocks per wave (the *_rows kernels) */
    /* ---- bit 28 ---- */
    SZ3HIP_DBG_CTX_NO_PUBLISH_ZERO = 268435456,  /* stage2_launch / sz3hip_compress_finish: the next call's histogram and counters are zeroed in front of that call, neither by k_publish nor behind finish() */
    /* ---- bit 29 ---- */
    SZ3HIP_DBG_INTERP_HANDOVER_IN_PLACE = 536870912, /* dense2_for: the level kernels hand the grid of stride 2 over in place, not as a dense array. Shares DEC_CARRY_PASS */
    SZ3HIP_DBG_DEC_CARRY_PASS = 536870912,           /* sz3hip_decompress_device: the units' carries are added by a pass of their own (k_scan_carry), not inside the first strided scan. Shares INTERP_HANDOVER_IN_PLACE */
    /* ---- bit 30 ---- */
    SZ3HIP_DBG_BLK_NO_EXIT = 1073741824,   /* blk_all_lorenzo / szk_launch_blk_compress: the block stream even where the selection would hand the array to the plain Lorenzo path; no speculation on the previous call's decision, no rank-first coding */
    /* ---- bit 31 (2147483648 as an unsigned word; the flags travel as an int, whose sign bit it is) ---- */
    SZ3HIP_DBG_BLK_NO_SELECT = -2147483647 - 1 /* blk_all_lorenzo: no selection pass, the fit pass chooses by its own wave sums */
};

/* The second word, sz3hip_debug_flags2(): one bit, one meaning. 0 in production. */
enum sz3hip_dbg2 {
    SZ3HIP_DBG2_PACK_SCAN_LAUNCH = 1,      /* szk_launch_encode: the offset scan of the sampled stage 2 in a launch of its own (k_scan_groups) where k_pack_b would scan the groups' sums itself */
    SZ3HIP_DBG2_REQUEST_BY_LEVEL = 2,      /* run_region_request: a request of several levels runs level group by level group over the one-level sequence (the route of a request whose boxes do not align by array level), not as one merged sequence */
    SZ3HIP_DBG2_MAP_PLAIN_STORES = 4       /* szk_launch_region_map: one-byte and two-byte texels by a thread per point (k_region_map), not by the form in which a lane maps four / two consecutive x points and issues one 32-bit store (k_region_map_packed) */
};

/* What the block decoder did, sz3hip_debug_blkdec_last(): the branch of blk_decompress_impl a pass took, one name per branch. The
 * values are ABI like the switches'. */
enum sz3hip_blkdec_form {
    SZ3HIP_BLKDEC_FORM_NONE = 0,           /* no block stream has been decoded in this process */
    SZ3HIP_BLKDEC_FORM_FRONTS_4D = 1,      /* 4-D: a launch per front of blocks (k_blk4_decode) */
    SZ3HIP_BLKDEC_FORM_SCAN2_1D = 2,       /* 1-D, second-order Lorenzo in the set: the scan of affine maps (k_blkn2_tile, k_blkn2_top, k_blkn2_apply) */
    SZ3HIP_BLKDEC_FORM_WAVE_2D = 3,        /* 2-D, one launch for the chain of fronts (k_blkn_wave2) */
    SZ3HIP_BLKDEC_FORM_SCAN_1D = 4,        /* 1-D, first-order sets: the scan of the blocks' sums (k_blkn_scan_tile, k_blkn_scan_top, k_blkn_apply1*) */
    SZ3HIP_BLKDEC_FORM_FRONTS2_2D = 5,     /* 2-D, second-order Lorenzo in the set: a block per wave, a launch per front (k_blkn_decode2s) */
    SZ3HIP_BLKDEC_FORM_GROUPS_2D = 6,      /* 2-D: groups of 4 x 4 blocks, a launch per front (k_blkn_decode2g) */
    SZ3HIP_BLKDEC_FORM_FRONTS_2D = 7,      /* 2-D: a block per wave, a launch per front (k_blkn_decode2) */
    SZ3HIP_BLKDEC_FORM_WAVE_3D = 8,        /* 3-D blocks of 6^3, one launch for the chain of fronts (k_blk_wave3) */
    SZ3HIP_BLKDEC_FORM_GROUPS_3_3D = 9,    /* 3-D blocks of 6^3: groups of 3 x 3 x 3 blocks in closed form, a launch per front (k_blk_decode_gf) */
    SZ3HIP_BLKDEC_FORM_GROUPS_2_3D = 10,   /* lab build, 3-D blocks of 6^3: groups of 2 x 2 x 2 blocks, line scans, a launch per front (k_blk_decode_g) */
    SZ3HIP_BLKDEC_FORM_FRONTS_3D = 11      /* 3-D: a block per wave, a launch per front (k_blk_decode) */
};

/* The words of sz3hip_debug_blkdec_last(). [0] .. [3] and [5] describe the first pass of the last szk_launch_blk_decompress of this
 * process, under the flags the caller had set. */
enum sz3hip_blkdec_word {
    SZ3HIP_BLKDEC_WORD_FORM = 0,           /* enum sz3hip_blkdec_form */
    SZ3HIP_BLKDEC_WORD_NSLOTS = 1,         /* the groups the form hands out (WAVE_2D, GROUPS_2D, WAVE_3D, GROUPS_3_3D, GROUPS_2_3D); the blocks for every other form */
    SZ3HIP_BLKDEC_WORD_WORKGROUPS = 2,     /* WAVE_2D / WAVE_3D: the workgroups of the one launch, each taking tickets until none is left (more slots than workgroups: some take a second one); else 0 */
    SZ3HIP_BLKDEC_WORD_TILES = 3,          /* SCAN_1D / SCAN2_1D: the tiles of 1024 blocks the top scan runs over, 1024 to a step of its loop; else 0 */
    SZ3HIP_BLKDEC_WORD_RETRIED = 4,        /* 1: a one-launch form was followed by the retry through the launch-per-front decoders (a flag poll gave up, or SZ3HIP_DBG_BLKDEC_FORCE_RETRY) */
    SZ3HIP_BLKDEC_WORD_ROWS = 5,           /* SCAN_1D / SCAN2_1D: 1 four blocks per wave (the *_rows kernels), 0 a wave per block; else 0 */
    SZ3HIP_BLKDEC_WORD_RETRY_FORM = 6      /* the form the retry took, SZ3HIP_BLKDEC_FORM_NONE without one; [7] is reserved (0) */
};

#endif

"""ctypes binding of include/dark_amd.h (dark_amd/libdark_amd.so).  No fallback: if the library is missing the
import of anything that needs it raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("DARK_AMD_LIB") or os.path.join(HERE, "libdark_amd.so")  # DARK_AMD_LIB: another build of the same ABI (A/B runs)

DK_OK = 0
DK_E_ARG, DK_E_NOMEM, DK_E_HIP, DK_E_CAPACITY, DK_E_MODEL, DK_E_STREAM, DK_E_INTERNAL, DK_E_NODEVICE = -1, -2, -3, -4, -5, -6, -7, -8
FM_NO_HIT = 0xFFFFFFFF  # DK_FM_NO_HIT: a position dk_dev_fm_locate* did not fill
FM_FIND_MAX_PAIRS = 1 << 24  # DK_FM_FIND_MAX_PAIRS: most (pattern, block) pairs of one dk_dev_fm_find* call
FM_SEAM_MAX_PATTERN = 4096  # DK_FM_SEAM_MAX_PATTERN: longest pattern of one dk_dev_fm_seams* call (and prev_len stays below it)
FM_NEAR_MAX_PATTERN = 128  # DK_FM_NEAR_MAX_PATTERN: most positions of a pattern of dk_dev_fm_near*
FM_NEAR_MAX_K = 3  # DK_FM_NEAR_MAX_K: the largest budget of mismatches
FM_NEAR_NODE_LIMIT = 1 << 20  # DK_FM_NEAR_NODE_LIMIT: nodes of the search tree one (pattern, block) pair visits where node_limit is 0
ERROR_NAMES = {-1: "DK_E_ARG", -2: "DK_E_NOMEM", -3: "DK_E_HIP", -4: "DK_E_CAPACITY", -5: "DK_E_MODEL",
               -6: "DK_E_STREAM", -7: "DK_E_INTERNAL", -8: "DK_E_NODEVICE"}
MODEL_IDS = {"dark": 0, "exp": 1, "ybs": 2, "simple": 3, "rawdc": 4}
DK_MODEL_ANYBYTE = 0x100  # "<model>+ff": [u32 LE first position of byte 0xFF][the reference stream], so that every block decodes
MODEL_IDS.update({name + "+ff": mid | DK_MODEL_ANYBYTE for name, mid in list(MODEL_IDS.items()) if name != "rawdc"})
NUM_KERNEL_SLOTS = 32
DK_FLAG_HAS_FF, DK_FLAG_SINGLE_SYMBOL = 1, 2
DK_PACKED_MAX_BLOCKS, DK_PACKED_MAX_BLOCK_BYTES = 65536, 1 << 24
SA_VERDICTS = {0: "ok", 1: "bad_range", 2: "not_permutation", 3: "bad_order"}  # DK_SA_OK ... DK_SA_BAD_ORDER
PURPOSES = {"full": 0, "decoder": 1}  # DK_CTX_FULL, DK_CTX_DECODER


class FmHit(C.Structure):
    """dk_fm_hit: a record of dk_dev_fm_find* (16 bytes; context.FM_HIT_DTYPE is the same layout for numpy)"""
    _fields_ = [("pattern", C.c_uint32), ("block", C.c_uint32), ("position", C.c_uint32), ("slot", C.c_uint32)]


class SaSmem(C.Structure):
    """dk_sa_smem: a record of dk_dev_sa_smems* (16 bytes; context.SA_SMEM_DTYPE is the same layout for numpy)"""
    _fields_ = [("at", C.c_uint32), ("len", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("ms_h2d", C.c_double), ("ms_sa", C.c_double), ("ms_bwt", C.c_double), ("ms_dc", C.c_double),
                ("ms_d2h", C.c_double), ("ms_entropy", C.c_double), ("ms_ibwt", C.c_double), ("ms_total", C.c_double),
                ("rounds", C.c_uint32), ("sort_passes", C.c_uint32), ("sorted_elements", C.c_uint64),
                ("dc_runs", C.c_uint64), ("entropy_threads", C.c_uint32), ("entropy_l3_group", C.c_int32),
                ("kernel_launches", C.c_uint32 * NUM_KERNEL_SLOTS), ("kernel_ms", C.c_double * NUM_KERNEL_SLOTS),
                ("kernel_bytes", C.c_double * NUM_KERNEL_SLOTS), ("sa_route", C.c_uint32), ("entropy_l3_numa", C.c_int16), ("gpu_numa", C.c_int16),
                ("ws_peak_bytes", C.c_uint64), ("ws_size_bytes", C.c_uint64),
                ("lcp_measured", C.c_uint64), ("lcp_bytes_compared", C.c_uint64), ("lcp_passes", C.c_uint32)]
ROUTES = {"short_prefix": 0x1, "narrow_keys": 0x2, "text_round": 0x4, "isa_windows": 0x8, "isa_marked": 0x10, "isa_buckets": 0x20,
          "general_round": 0x40, "big_groups": 0x80, "inplace_rounds": 0x100, "pair_chains": 0x200, "lfirst": 0x400,
          "lfirst_big_round": 0x800, "lfirst_deep": 0x1000, "lfirst_fallback": 0x2000, "lfirst_giant": 0x4000, "period_round": 0x8000, "packed_pairs": 0x10000,
          "packed_guard": 0x20000, "lcp_long": 0x40000, "lcp_giant": 0x80000}


# every symbol include/dark_amd.h declares: name -> (restype, argtypes)
_vp, _sz, _szp, _u32p, _i = C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_int
SIGNATURES = {
    "dk_version": (C.c_char_p, []),
    "dk_ctx_create": (_i, [_i, _sz, C.POINTER(_vp)]),
    "dk_ctx_create_decoder": (_i, [_i, _sz, _sz, C.POINTER(_vp)]),
    "dk_ctx_purpose": (_i, [_vp]),
    "dk_workspace_bytes": (_sz, [_i, _sz, _sz]),
    "dk_ctx_destroy": (None, [_vp]),
    "dk_capacity": (_sz, [_vp]),
    "dk_last_consumed": (_sz, [_vp]),
    "dk_last_block_flags": (C.c_uint, [_vp]),
    "dk_last_error": (C.c_char_p, [_vp]),
    "dk_suffix_array": (_i, [_vp, _vp, _sz, _vp]),
    "dk_bwt_forward": (_i, [_vp, _vp, _sz, _vp, _u32p]),
    "dk_bwt_inverse": (_i, [_vp, _vp, _sz, C.c_uint32, _vp]),
    "dk_dc_encode": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _szp]),
    "dk_dc_decode": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _szp]),
    "dk_block_encode": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _szp]),
    "dk_block_decode": (_i, [_vp, _i, _vp, _sz, _sz, _vp]),
    "dk_raw_block_encode": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _szp, _vp, _sz, _szp]),
    "dk_raw_block_decode": (_i, [_vp, _i, _vp, _sz, _sz, _vp]),
    "dk_dev_suffix_array": (_i, [_vp, _vp, _sz, _vp]),
    "dk_dev_bwt_forward": (_i, [_vp, _vp, _sz, _vp, _u32p]),
    "dk_dev_bwt_inverse": (_i, [_vp, _vp, _sz, C.c_uint32, _vp]),
    "dk_dev_dc_encode": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _szp]),
    "dk_dev_block_encode": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _szp]),
    "dk_dev_block_decode": (_i, [_vp, _i, _vp, _sz, _sz, _vp]),
    "dk_dev_batch_encode": (_i, [_vp, _i, _sz, _vp, _vp, _vp, _vp, _vp, _i]),
    "dk_batch_begin": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "dk_batch_push": (_i, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "dk_batch_finish": (_i, [_vp]),
    "dk_dev_bwt_forward_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _u32p]),
    "dk_dev_suffix_array_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _u32p]),
    "dk_suffix_array_packed": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "dk_dev_lcp": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "dk_dev_suffix_array_lcp": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "dk_suffix_array_lcp": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "dk_dev_lcp_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_suffix_array_packed_lcp": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "dk_suffix_array_packed_lcp": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_sa_check": (_i, [_vp, _vp, _sz, _vp, _u32p, _u32p]),
    "dk_sa_check": (_i, [_vp, _vp, _sz, _vp, _u32p, _u32p]),
    "dk_dev_sa_check_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "dk_dev_sa_search": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp]),
    "dk_sa_search": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_sa_search_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "dk_dev_sa_match": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_sa_match_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp]),
    "dk_sa_match": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_sa_smems": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _sz, _sz, _vp, _vp]),
    "dk_dev_sa_smems_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _sz, _sz, _vp, _vp]),
    "dk_sa_smems": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _sz, _sz, _vp, _vp]),
    "dk_fm_index_bytes": (_sz, [_sz, _sz]),
    "dk_dev_fm_build": (_i, [_vp, _vp, _sz, C.c_uint32, _vp]),
    "dk_dev_fm_build_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_fm_count": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_fm_count_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "dk_fm_count": (_i, [_vp, _vp, _sz, C.c_uint32, _vp, _sz, _vp, _vp, _vp]),
    "dk_fm_locate_bytes": (_sz, [_sz, _sz, C.c_uint32]),
    "dk_dev_fm_locate_build": (_i, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _vp]),
    "dk_dev_fm_locate_build_packed": (_i, [_vp, _vp, _sz, _vp, _vp, C.c_uint32, _vp]),
    "dk_dev_fm_locate": (_i, [_vp, _vp, _sz, _vp, _vp, C.c_uint32, _vp, _vp, _sz, _sz, _vp]),
    "dk_dev_fm_locate_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _sz, _vp, _sz, _vp]),
    "dk_fm_locate": (_i, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "dk_fm_extract_bytes": (_sz, [_sz, _sz, C.c_uint32]),
    "dk_dev_fm_extract_build": (_i, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _vp]),
    "dk_dev_fm_extract_build_packed": (_i, [_vp, _vp, _sz, _vp, _vp, C.c_uint32, _vp]),
    "dk_dev_fm_extract": (_i, [_vp, _vp, _sz, _vp, _vp, C.c_uint32, _vp, _vp, _sz, _sz, _vp]),
    "dk_dev_fm_extract_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _sz, _vp, _sz, _vp]),
    "dk_fm_extract": (_i, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _vp, _vp, _sz, _sz, _vp]),
    "dk_dev_fm_find": (_i, [_vp, _vp, _sz, _vp, _vp, C.c_uint32, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_fm_find_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, C.c_uint32, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_fm_seams": (_i, [_vp, _vp, _sz, _vp, _vp, C.c_uint32, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_fm_seams_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, C.c_uint32, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "dk_fm_find": (_i, [_vp, _vp, _sz, C.c_uint32, C.c_uint32, _vp, _sz, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_fm_near": (_i, [_vp, _vp, _sz, _vp, _vp, C.c_uint32, _vp, _sz, _vp, C.c_uint32, C.c_uint32, _sz, _vp, _vp, _vp, _vp]),
    "dk_dev_fm_near_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, C.c_uint32, _vp, _sz, _vp, C.c_uint32, C.c_uint32, _sz, _vp, _vp, _vp, _vp]),
    "dk_dbg_dev_fm_rank": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _sz, _vp]),
    "dk_dev_dc_encode_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _szp]),
    "dk_batch_push_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "dk_dev_packed_encode": (_i, [_vp, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i]),
    "dk_dev_batch_decode": (_i, [_vp, _i, _sz, _vp, _vp, _vp, _vp, _i]),
    "dk_dev_bwt_inverse_packed": (_i, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "dk_dev_packed_decode": (_i, [_vp, _i, _sz, _vp, _vp, _vp, _vp, _i]),
    "dk_multi_block_encode": (_i, [_vp, _i, _i, _sz, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz]),
    "dk_multi_block_decode": (_i, [_vp, _i, _i, _sz, _vp, _vp, _vp, _vp, _i, _vp, _sz]),
    "dk_model_encode": (_i, [_i, _vp, _vp, _sz, _vp, _sz, _szp]),
    "dk_model_decode": (_i, [_i, _vp, _sz, _vp, _sz, _vp]),
    "dk_bitcoder_encode": (_i, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "dk_bitcoder_decode": (_i, [_vp, _sz, _vp, _sz, _vp]),
    "dk_stream_encode": (_i, [_i, _sz, _vp, _vp, _vp, _vp, _vp, _sz, C.c_uint32, _vp, _sz, _szp]),
    "dk_stream_decode": (_i, [_i, _vp, _sz, _sz, _vp, _u32p, C.POINTER(_i), _szp]),
    "dk_raw_stream_encode": (_i, [_i, _vp, _sz, C.c_uint32, _vp, _sz, _szp]),
    "dk_raw_stream_decode": (_i, [_i, _vp, _sz, _sz, _vp, _u32p, _szp]),
    "dk_set_profiling": (_i, [_vp, _i]),
    "dk_stats_reset": (_i, [_vp]),
    "dk_get_stats": (_i, [_vp, C.POINTER(Stats)]),
    "dk_kernel_name": (C.c_char_p, [_i]),
    "dk_set_entropy_threads": (_i, [_i]),
    "dk_host_l3_groups": (_i, [_i]),
    "dk_last_entropy_info": (None, [C.POINTER(_i), C.POINTER(_i)]),
    "dk_set_entropy_numa_node": (None, [_i]),
    "dk_dbg_l3_claim_order": (_i, [C.POINTER(_i), _i, _i, _i, C.POINTER(_i)]),
    "dk_dbg_stream_encode_gated": (_i, [_i, _sz, _vp, _vp, _vp, _sz, C.c_uint32, _vp, _sz, _szp, _vp, C.c_uint, _i]),
    "dk_dbg_sort_pairs": (_i, [_vp, _vp, _vp, _sz, _i, _i]),
    "dk_dbg_dev_sort_pairs": (_i, [_vp, _vp, _vp, _sz, _i, _i]),
    "dk_dbg_dev_local_sort": (_i, [_vp, _vp, _vp, _sz, _i, _i]),
    "dk_dbg_dev_sort_groups": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, C.c_uint32, _i, _i]),
    # ctx, keys, key_bytes, bucket_starts, idx, pos_in, gid_in, cmp_shift, count | rank, sa | bwt, sym_in, sym_out, origin | out_idx, out_pos, out_gid,
    # gstart, bigidx, bigoff | ls_max, counts_out[5] | reduce_tiles_per_wg, first_tiles_per_wg, sparse_max
    "dk_dbg_dev_rerank": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _sz] + [_vp] * 2 + [_vp] * 4 + [_vp] * 6 + [C.c_uint32, _vp, C.c_uint, C.c_uint, _i]),
    "dk_dbg_dev_lf_refine": (_i, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _sz, C.c_uint32, _i, _vp, _vp, _vp]),
    "dk_dbg_dev_lf_rerank": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _sz] + [_vp] * 8 + [C.c_uint32, _vp, _i, C.c_uint32, _vp, C.c_uint]),
    # ctx, n, h, count, idx, pos, gid, gstart, groups | rank, sa, bwt, sym, origin | chain_group, record_cap, max_rounds, always_compact |
    # out_idx, out_meta, out_sym, out_pos, out[8]
    "dk_dbg_dev_in_place": (_i, [_vp, _sz, C.c_uint32, _sz, _vp, _vp, _vp, _vp, _sz] + [_vp] * 5 + [_i, C.c_uint32, _i, _i] + [_vp] * 5),
    # ctx, text, n, h, count, idx, pos, gid, gstart, groups | rank, tsym, period, next_break | sa, bwt, sym, origin |
    # out_sorted_keys, out_sorted_idx, out_sorted_sym, out_idx, out_pos, out_gid, out_gstart, out_sym, out[8]
    "dk_dbg_dev_round": (_i, [_vp, _vp, _sz, C.c_uint32, _sz, _vp, _vp, _vp, _vp, _sz] + [_vp, _i, _i, _vp] + [_vp] * 4 + [_vp] * 9),
    # ctx, text, n | period, next_break | run_out[2], probe_out[8] | count_p, count_out | search_pmax, found_out[32] | m, span, cands, ncands, dups_out[4]
    "dk_dbg_dev_period": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, C.c_uint32, C.c_uint32, _vp, _i, _vp]),
    # ctx, text, n | code[256], bits, spk, inv[256], narrow | keys_out, sa, bwt, origin | bucket_starts_out[256], out[4]
    "dk_dbg_dev_initial_sort": (_i, [_vp, _vp, _sz, _vp, _i, _i, _vp, _i] + [_vp] * 4 + [_vp, _vp]),
    # ctx, text, count, n | keys, vals, rank, act | code[256], out[8]
    "dk_dbg_dev_packed_first": (_i, [_vp, _vp, _sz, _vp] + [_vp] * 4 + [_vp, _vp]),
    # ctx, count, n, h, act, c, rank | keys, vals, next_act, guard | out[8]
    "dk_dbg_dev_packed_round": (_i, [_vp, _sz, _vp, C.c_uint32, _vp, _sz, _vp] + [_vp] * 4 + [_vp]),
    "dk_dbg_dev_inverse_permutation": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "dk_dbg_mail_fill": (_i, [_vp, _i]),
    "dk_dbg_ws_peek": (_i, [_vp, _sz, _vp]),
}

_lib = None


def load():
    """dlopen the in-tree library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError("dark_amd: %s is missing -- run `python dark_amd/build.py` (hipcc, gfx950). "
                              "There is no CPU fallback." % SO_PATH)
        # PyTorch-ROCm ships its own libamdhip64 under the same soname as /opt/rocm's.  Whichever is loaded first serves the
        # whole process; if ours came first, torch would later fail to find the GPU.  So when torch is installed, load it first.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the ABI lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib

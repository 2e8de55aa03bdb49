"""ctypes view of libmillion_hip.so (include/million_hip.h).  No fallback: if the library is missing
or fails to load, importing the ops raises — the product path never runs on a CPU substitute."""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libmillion_hip.so"
if os.environ.get("MILLION_HIP_LIB"):      # development A/B builds (tools/ab_build.py); the product path uses the in-tree library
    LIB_PATH = Path(os.environ["MILLION_HIP_LIB"]).resolve()

c_i32, c_i64, c_u32, c_vp, c_sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t

MILLION_CODES_ROWMAJOR, MILLION_CODES_KPAGES, MILLION_CODES_VPAGES = 0, 1, 2
MILLION_KV_ROWMAJOR, MILLION_KV_PAGED = 0, 1


class EncodeDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("bs", c_i32), ("nh_k", c_i32), ("n", c_i32),
                ("d", c_i32), ("M", c_i32), ("C", c_i32),
                ("x_stride_b", c_i64), ("x_stride_h", c_i64), ("x_stride_n", c_i64),
                ("x_row_start", c_i32), ("x_row_mod", c_i32),
                ("dst_layout", c_i32), ("dst_token_start", c_i32),
                ("dst_stride_b", c_i64), ("dst_stride_h", c_i64),
                ("page_size", c_i32), ("n_pages_cap", c_i32), ("dev_lengths", c_vp), ("cents_prepared", c_vp)]


class AttnDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("bs", c_i32), ("nh", c_i32), ("nh_k", c_i32),
                ("d", c_i32), ("M", c_i32), ("C", c_i32),
                ("n_tokens", c_i32), ("r", c_i32), ("resid_start", c_i32), ("resid_cap", c_i32),
                ("resid_stride_b", c_i64), ("resid_stride_h", c_i64),
                ("k_layout", c_i32), ("v_layout", c_i32), ("page_size", c_i32), ("n_pages_cap", c_i32),
                ("page_ids_i64", c_i32), ("v_pages_dense", c_i32),
                ("k_stride_b", c_i64), ("k_stride_h", c_i64), ("v_stride_b", c_i64), ("v_stride_h", c_i64),
                ("dev_lengths", c_vp), ("k_pool_pages", c_i32), ("v_pool_pages", c_i32)]


class PrefillDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("bs", c_i32), ("nh", c_i32), ("nh_k", c_i32), ("d", c_i32),
                ("n_q", c_i32), ("n_kv", c_i32), ("q_pos0", c_i32), ("causal", c_i32),
                ("q_stride_b", c_i64), ("q_stride_h", c_i64), ("q_stride_n", c_i64),
                ("k_stride_b", c_i64), ("k_stride_h", c_i64), ("k_stride_n", c_i64),
                ("v_stride_b", c_i64), ("v_stride_h", c_i64), ("v_stride_n", c_i64),
                ("o_stride_b", c_i64), ("o_stride_h", c_i64), ("o_stride_n", c_i64),
                ("dev_spans", c_vp)]


class ChunkAttnDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("bs", c_i32), ("nh", c_i32), ("nh_k", c_i32), ("d", c_i32), ("M", c_i32), ("C", c_i32),
                ("n_q", c_i32), ("n_c", c_i32), ("n_tokens", c_i32), ("r", c_i32), ("resid_start", c_i32), ("resid_cap", c_i32),
                ("resid_stride_b", c_i64), ("resid_stride_h", c_i64),
                ("k_layout", c_i32), ("v_layout", c_i32), ("page_size", c_i32), ("n_pages_cap", c_i32), ("page_ids_i64", c_i32),
                ("k_stride_b", c_i64), ("k_stride_h", c_i64), ("v_stride_b", c_i64), ("v_stride_h", c_i64),
                ("q_stride_b", c_i64), ("q_stride_h", c_i64), ("q_stride_n", c_i64),
                ("kc_stride_b", c_i64), ("kc_stride_h", c_i64), ("kc_stride_n", c_i64),
                ("vc_stride_b", c_i64), ("vc_stride_h", c_i64), ("vc_stride_n", c_i64),
                ("o_stride_b", c_i64), ("o_stride_h", c_i64), ("o_stride_n", c_i64),
                ("dev_lengths", c_vp), ("dev_n_q", c_vp)]


class GatherRowsDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("bs", c_i32), ("nh_k", c_i32), ("d", c_i32), ("M", c_i32), ("C", c_i32), ("code_bytes", c_i32),
                ("t0", c_i32), ("t1", c_i32), ("r", c_i32), ("resid_start", c_i32), ("resid_cap", c_i32),
                ("resid_stride_b", c_i64), ("resid_stride_h", c_i64),
                ("k_layout", c_i32), ("v_layout", c_i32), ("page_size", c_i32), ("n_pages_cap", c_i32),
                ("k_stride_b", c_i64), ("k_stride_h", c_i64), ("v_stride_b", c_i64), ("v_stride_h", c_i64),
                ("rows_cap", c_i32), ("reserved", c_i32), ("o_stride_b", c_i64), ("o_stride_h", c_i64)]


MILLION_MERGE_MAX_PARTS = 8


class AttnMergeDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("n_parts", c_i32), ("bs", c_i32), ("nh", c_i32), ("n_q", c_i32), ("d", c_i32),
                ("out_stride", c_i64 * 3 * MILLION_MERGE_MAX_PARTS), ("lse_stride", c_i64 * 3 * MILLION_MERGE_MAX_PARTS),
                ("res_out_stride", c_i64 * 3), ("res_lse_stride", c_i64 * 3)]


class StoreRaggedDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("bs", c_i32), ("nh_k", c_i32), ("d", c_i32), ("M", c_i32), ("C", c_i32),
                ("n_bound", c_i32),
                ("kn_stride_b", c_i64), ("kn_stride_h", c_i64), ("kn_stride_n", c_i64),
                ("vn_stride_b", c_i64), ("vn_stride_h", c_i64), ("vn_stride_n", c_i64),
                ("resid_cap", c_i32), ("page_size", c_i32),
                ("resid_stride_b", c_i64), ("resid_stride_h", c_i64),
                ("n_pages_cap", c_i32)]


class BlockMergeDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("bs", c_i32), ("nh", c_i32), ("nh_k", c_i32), ("n", c_i32), ("d", c_i32),
                ("q_stride", c_i64 * 3), ("k_stride", c_i64 * 3), ("v_stride", c_i64 * 3),
                ("a_stride", c_i64 * 3), ("o_stride", c_i64 * 3),
                ("stage_stride_b", c_i64), ("stage_stride_h", c_i64)]


class SinkMergeDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("bs", c_i32), ("nh", c_i32), ("nh_k", c_i32), ("n", c_i32), ("d", c_i32),
                ("s_cap", c_i32), ("n_sink", c_i32),
                ("q_stride", c_i64 * 3), ("a_stride", c_i64 * 3), ("o_stride", c_i64 * 3),
                ("sink_stride_b", c_i64), ("sink_stride_h", c_i64)]


class WindowCommitDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("n_layers", c_i32), ("bs", c_i32), ("nh_k", c_i32), ("d", c_i32), ("M", c_i32), ("C", c_i32),
                ("n_bound", c_i32), ("page_size", c_i32), ("n_pages_cap", c_i32), ("n_pool", c_i32), ("resid_cap", c_i32),
                ("new_stride_l", c_i64), ("new_stride_b", c_i64), ("new_stride_h", c_i64), ("new_stride_n", c_i64),
                ("ids_layer_stride", c_i64), ("rows_layer_stride", c_i64), ("lengths_layer_stride", c_i64)]


MILLION_FORK_SHARE, MILLION_FORK_COPY = 0, 1


class ForkDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("n_layers", c_i32), ("bs", c_i32), ("nh_k", c_i32), ("d", c_i32), ("M", c_i32),
                ("page_size", c_i32), ("n_pages_cap", c_i32), ("n_pool", c_i32), ("resid_cap", c_i32),
                ("ids_layer_stride", c_i64), ("rows_layer_stride", c_i64), ("lengths_layer_stride", c_i64),
                ("src", c_i32), ("n_dst", c_i32), ("mode", c_i32), ("n_pages_bound", c_i32), ("prefix_tokens", c_i32)]


MILLION_SWAP_PACK, MILLION_SWAP_UNPACK = 0, 1
MILLION_REPACK_PACK, MILLION_REPACK_UNPACK = 0, 1


class SwapDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("direction", c_i32), ("n_layers", c_i32), ("bs", c_i32), ("nh_k", c_i32), ("d", c_i32),
                ("M", c_i32), ("page_size", c_i32), ("n_pages_cap", c_i32), ("n_pool", c_i32), ("resid_cap", c_i32),
                ("layer0", c_i32), ("n_layers_call", c_i32),
                ("ids_layer_stride", c_i64), ("rows_layer_stride", c_i64), ("lengths_layer_stride", c_i64), ("blob_bytes", c_i64),
                ("n_slots", c_i32), ("n_pages_bound", c_i32)]


class TrainDesc(ctypes.Structure):
    _fields_ = [("struct_size", c_u32), ("n", c_i32), ("d", c_i32), ("M", c_i32), ("C", c_i32), ("niter", c_i32),
                ("x_is_f32", c_i32), ("x_stride_n", c_i64), ("eps", ctypes.c_float)]


# every symbol include/million_hip.h declares: (restype, argtypes)
SYMBOLS = {
    "million_pq_train_workspace_bytes": (c_sz, [ctypes.POINTER(TrainDesc)]),
    "million_pq_train": (c_i32, [ctypes.POINTER(TrainDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "million_version": (c_i32, []),
    "million_last_error": (ctypes.c_char_p, []),
    "million_prepared_cents_bytes": (c_sz, [c_i32, c_i32, c_i32]),
    "million_prepare_cents": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "million_pq_encode": (c_i32, [ctypes.POINTER(EncodeDesc), c_vp, c_vp, c_vp, c_vp, c_vp]),
    "million_pq_decode": (c_i32, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp]),
    "million_pq_flush": (c_i32, [ctypes.POINTER(EncodeDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp]),
    "million_pq_flush_layers": (c_i32, [ctypes.POINTER(EncodeDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32,
                                        c_i32, c_i64, c_i64, c_i64, c_i32, c_vp]),
    "million_transpose_v_codes": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i64, c_i64, c_vp]),
    "million_attn_workspace_bytes": (c_sz, [ctypes.POINTER(AttnDesc)]),
    "million_workspace_init": (c_i32, [c_vp, c_sz, c_vp]),
    "million_pq_decode_attn": (c_i32, [ctypes.POINTER(AttnDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                       c_vp, c_vp, c_vp, c_sz, c_vp]),
    "million_pq_decode_attn_append": (c_i32, [ctypes.POINTER(AttnDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                              c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "million_pq_decode_attn_lse": (c_i32, [ctypes.POINTER(AttnDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                           c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "million_attn_kernel_kind": (c_i32, [ctypes.POINTER(AttnDesc)]),
    "million_attn_wide_workspace_bytes": (c_sz, [ctypes.POINTER(AttnDesc)]),
    "million_attn_wide_splits": (c_i32, [ctypes.POINTER(AttnDesc)]),
    "million_pq_decode_attn_wide": (c_i32, [ctypes.POINTER(AttnDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "million_pq_encode_packed": (c_i32, [ctypes.POINTER(EncodeDesc), c_vp, c_vp, c_vp, c_vp, c_vp]),
    "million_pq_decode_attn_packed": (c_i32, [ctypes.POINTER(AttnDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                              c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "million_pq_repack_pages": (c_i32, [c_i32, c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "million_prefill_attn": (c_i32, [ctypes.POINTER(PrefillDesc), c_vp, c_vp, c_vp, c_vp, c_vp]),
    "million_prefill_attn_lse": (c_i32, [ctypes.POINTER(PrefillDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "million_chunk_attn_workspace_bytes": (c_sz, [ctypes.POINTER(ChunkAttnDesc)]),
    "million_pq_chunk_attn": (c_i32, [ctypes.POINTER(ChunkAttnDesc)] + [c_vp] * 13 + [c_sz, c_vp]),
    "million_pq_chunk_attn_lse": (c_i32, [ctypes.POINTER(ChunkAttnDesc)] + [c_vp] * 14 + [c_sz, c_vp]),
    "million_chunk_attn_wide_workspace_bytes": (c_sz, [ctypes.POINTER(ChunkAttnDesc)]),
    "million_pq_chunk_attn_wide": (c_i32, [ctypes.POINTER(ChunkAttnDesc)] + [c_vp] * 14 + [c_sz, c_vp]),
    "million_pq_chunk_attn_packed": (c_i32, [ctypes.POINTER(ChunkAttnDesc)] + [c_vp] * 14 + [c_sz, c_vp]),
    "million_pq_gather_rows": (c_i32, [ctypes.POINTER(GatherRowsDesc)] + [c_vp] * 11),
    "million_pq_gather_rows_packed": (c_i32, [ctypes.POINTER(GatherRowsDesc)] + [c_vp] * 11),
    "million_attn_merge": (c_i32, [ctypes.POINTER(AttnMergeDesc), ctypes.POINTER(c_vp), ctypes.POINTER(c_vp), c_vp, c_vp, c_vp]),
    "million_attn_block_merge": (c_i32, [ctypes.POINTER(BlockMergeDesc)] + [c_vp] * 11),
    "million_attn_sink_merge": (c_i32, [ctypes.POINTER(SinkMergeDesc)] + [c_vp] * 10),
    "million_window_commit": (c_i32, [ctypes.POINTER(WindowCommitDesc)] + [c_vp] * 12),
    "million_attn_tree_merge": (c_i32, [ctypes.POINTER(BlockMergeDesc)] + [c_vp] * 12),
    "million_window_commit_rows": (c_i32, [ctypes.POINTER(WindowCommitDesc)] + [c_vp] * 13),
    "million_window_commit_wide": (c_i32, [ctypes.POINTER(WindowCommitDesc)] + [c_vp] * 11 + [c_i32, c_vp]),
    "million_window_commit_rows_wide": (c_i32, [ctypes.POINTER(WindowCommitDesc)] + [c_vp] * 12 + [c_i32, c_vp]),
    "million_pq_store_ragged": (c_i32, [ctypes.POINTER(StoreRaggedDesc)] + [c_vp] * 12),
    "million_pq_store_ragged_wide": (c_i32, [ctypes.POINTER(StoreRaggedDesc)] + [c_vp] * 11 + [c_i32, c_vp]),
    "million_pq_flush_wide": (c_i32, [ctypes.POINTER(EncodeDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "million_pq_flush_wide_layers": (c_i32, [ctypes.POINTER(EncodeDesc), c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32,
                                             c_i32, c_i64, c_i64, c_i64, c_i32, c_i32, c_i32, c_vp]),
    "million_cache_fork": (c_i32, [ctypes.POINTER(ForkDesc)] + [c_vp] * 9),
    "million_cache_swap": (c_i32, [ctypes.POINTER(SwapDesc)] + [c_vp] * 10),
    "million_cache_fork_wide": (c_i32, [ctypes.POINTER(ForkDesc)] + [c_vp] * 8 + [c_i32, c_i32, c_vp]),
    "million_cache_swap_wide": (c_i32, [ctypes.POINTER(SwapDesc)] + [c_vp] * 9 + [c_i32, c_i32, c_vp]),
    "million_set_force_generic": (None, [c_i32]),
    "million_debug_set_stamp_buffer": (None, [c_vp]),
    "million_debug_bad_page_ids": (c_i32, []),
    "million_debug_tail_faults": (c_i32, []),
    "million_debug_rows_reduce": (c_i32, [c_vp, c_vp, c_vp, c_vp]),
    "million_lengths_advance": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp]),
    "million_residual_append": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i64, c_i64,
                                        c_i32, c_i32, c_vp, c_vp]),
}

_lib = None


def load() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(f"{LIB_PATH} is missing: run `make bindings` (hipcc --offload-arch=gfx950). "
                              "There is no CPU fallback for the PQ-KV hot path.")
        # torch first: its bundled HIP runtime must be the one this library binds to.  Loaded the other way round
        # (this library pulling in the system libamdhip64 before torch brings its own) the process ends up with two
        # runtimes and the second one reports "no ROCm-capable device".
        import torch  # noqa: F401
        L = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)      # AttributeError if the ABI drifted
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().million_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")

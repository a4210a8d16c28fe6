"""ctypes binding of the C-ABI kernel library (include/emcid_hip.h -> csrc/libemcid_hip.so).

There is NO fallback: if the library is missing or a call fails, the product path raises.
torch is used here only to hand over device pointers and the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from pathlib import Path
from typing import Optional

import torch

_LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libemcid_hip.so"
_lib = None

EXPORTS = [
    "emcid_abi_version", "emcid_last_error", "emcid_gram_accumulate_f32", "emcid_symmetrize_lower_f32",
    "emcid_gather_mean_f32", "emcid_edit_workspace_bytes", "emcid_edit_layer_f64", "emcid_assemble_spd_f64",
    "emcid_cholesky_f64", "emcid_cholesky_solve_f64", "emcid_delta_w_f64", "emcid_dgemm_f64", "emcid_dgemm_ex_f64", "emcid_dgemm_batched_f64", "emcid_streamk_workspace_bytes", "emcid_dgemm_streamk_f64", "emcid_debug_streamk_stamps", "emcid_debug_step_stamps", "emcid_debug_linear_sp16_stamps", "emcid_fingerprint_store", "emcid_fingerprint_check", "emcid_fingerprint_content", "emcid_axpy_f32",
    "emcid_profile_enable", "emcid_profile_collect", "emcid_attention_f32", "emcid_edit_layer_shard_f64",
    "emcid_apply_update_f32", "emcid_inverse_workspace_doubles", "emcid_quick_gelu_f32", "emcid_add_layernorm_f32", "emcid_embed_layernorm_f32", "emcid_tree_attention_f32", "emcid_debug_leaf_stamps",
    "emcid_cov_factor_workspace_bytes", "emcid_factor_cov_f64", "emcid_cov_inverse_f64", "emcid_cov_factor_rescale_f64",
    "emcid_edit_dual_workspace_bytes",
    "emcid_edit_dual_stage1_f64", "emcid_edit_dual_pt", "emcid_edit_dual_stage2_f64",
    "emcid_edit_dual_apply_stage1_f64", "emcid_edit_dual_yt", "emcid_edit_dual_apply_stage2_f64",
    "emcid_edit_dual_apply_assemble_f64",
    "emcid_edit_dual_preserve_workspace_bytes", "emcid_edit_layer_dual_preserve_f64",
    "emcid_session_retain_workspace_bytes", "emcid_session_retain_f64", "emcid_session_step_norms_f64",
    "emcid_session_release_workspace_bytes", "emcid_session_release_f64", "emcid_session_rescale_f64",
    "emcid_cov_factor_fold_workspace_bytes", "emcid_cov_factor_fold_f64",
    "emcid_session_refold_update_f64", "emcid_cov_factor_refactor_f64",
    "emcid_score_rows_f32", "emcid_score_chains_f64", "emcid_score_chains_pair_f64", "emcid_score_pooled_f32",
    "emcid_score_chains_pair_grid_f64",
    "emcid_edit_lu_workspace_bytes", "emcid_edit_layer_lu_f64", "emcid_lu_solve_f64",
    "emcid_edit_dual_cols_stage1_f64", "emcid_edit_dual_s", "emcid_edit_dual_u", "emcid_edit_dual_cols_stage2_f64",
    "emcid_apply_update2d_f32", "emcid_linear_f32", "emcid_linear_ws_f32", "emcid_linear_workspace_bytes",
    "emcid_split_rows_f16", "emcid_linear_sp16_f32", "emcid_gram_sp16_workspace_bytes", "emcid_gram_sp16_workspace_bytes_for", "emcid_gram_accumulate_sp16_f32", "emcid_add_layernorm_sp16", "emcid_embed_layernorm_sp16",
    "emcid_tree_attention_sp16", "emcid_tree_attention_sp16_supported", "emcid_clip_workspace_bytes",
    "emcid_clip_layer_head_sp16", "emcid_clip_layer_tail_sp16", "emcid_clip_layers_sp16", "emcid_clip_edit_layer_tail_sp16",
    "emcid_edit_dual_block", "emcid_edit_dual_schur_form", "emcid_full_inverse_scratch_doubles", "emcid_full_inverse_f64",
]
DUAL_BLOCKS = ["K", "P", "Y", "R", "S", "LS", "INVS", "PT", "Y2", "V", "U", "SK", "XT", "TT", "SK_COUNTERS"]   # EMCID_DUAL_* (include/emcid_hip.h)
SCHUR_FORMS = ["xrow", "full_inverse", "substitution"]                                                         # EMCID_SCHUR_*
PROF_CLASSES = ["prep", "assemble", "chol_leaf", "chol_panel", "chol_trail", "trsm_diag", "trsm_update", "delta_w",
                "gram", "gather", "dgemm", "misc", "inv_build", "chol_inner", "inv_apply", "inv_block", "linear"]

ABI_VERSION = 16
NB = 128      # Cholesky block (csrc/common.h)
NPAD = 64     # concept padding of the f64 stacks (csrc/common.h)


class EmcidHipError(RuntimeError):
    pass


def lib_path() -> Path:
    return _LIB_PATH


def load():
    """dlopen the kernel library (works without a GPU: used by the CPU symbol-export test)."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise EmcidHipError(
            f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C {_LIB_PATH.parent}`. The MI355X path has no CPU fallback.")
    lib = C.CDLL(str(_LIB_PATH))
    p, i64, i32, f64, f32 = C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_float
    sig = {
        "emcid_abi_version": (i32, []),
        "emcid_last_error": (C.c_char_p, []),
        "emcid_gram_accumulate_f32": (i32, [p, i64, i64, i64, p, i64, i32, p]),
        "emcid_symmetrize_lower_f32": (i32, [p, i64, i64, p]),
        "emcid_gather_mean_f32": (i32, [p, i64, i64, i64, i64, i64, p, p, i64, p, i64, p]),
        "emcid_edit_workspace_bytes": (i64, [i64, i64, i64]),
        "emcid_edit_layer_f64": (i32, [p, p, p, p, i64, i64, i64, f64, f64, i32, p, p, p, p, p, p, i64, p, p]),
        "emcid_edit_layer_shard_f64": (i32, [p, p, p, p, i64, i64, i64, f64, f64, i32, i64, i64, p, p, p, p, i64, p, p]),
        "emcid_apply_update_f32": (i32, [p, p, p, p, i64, p]),
        "emcid_assemble_spd_f64": (i32, [p, i64, p, i64, i64, i64, f64, f32, p, i64, p]),
        "emcid_cholesky_f64": (i32, [p, p, i64, i64, p, p, p]),
        "emcid_inverse_workspace_doubles": (i64, [i64]),
        "emcid_debug_leaf_stamps": (i32, [p, p, p, p, p, p]),
        "emcid_cov_factor_workspace_bytes": (i64, [i64, i64]),
        "emcid_factor_cov_f64": (i32, [p, i64, i64, f64, f64, p, i64, p, p]),
        "emcid_cov_inverse_f64": (i32, [p, i64, i64, i64, i64, p]),
        "emcid_cov_factor_rescale_f64": (i32, [p, p, i64, i64, i64, f64, i32, p]),
        "emcid_edit_dual_workspace_bytes": (i64, [i64, i64, i64]),
        "emcid_edit_dual_stage1_f64": (i32, [p, p, p, i64, i64, i64, f64, i32, f64, p, i64, i64, i64, i64, i32, p, i64, p]),
        "emcid_edit_dual_pt": (p, [p, i64, i64, i64]),
        "emcid_edit_dual_block": (p, [p, i64, i64, i64, i32, C.POINTER(i64)]),
        "emcid_edit_dual_schur_form": (i32, [i64, i64, i64]),
        "emcid_full_inverse_scratch_doubles": (i64, [i64, i64]),
        "emcid_full_inverse_f64": (i32, [p, i64, i64, p, p, p, i64, p]),
        "emcid_edit_dual_stage2_f64": (i32, [i64, i64, i64, f64, p, p, p, p, p, p, i64, p, p]),
        "emcid_edit_dual_apply_stage1_f64": (i32, [p, p, p, i64, i64, i64, f64, i32, f64, p, i64, i64, i64, i64, i32, p, i64, p]),
        "emcid_edit_dual_yt": (p, [p, i64, i64, i64]),
        "emcid_edit_dual_apply_stage2_f64": (i32, [i64, i64, i64, p, i64, i64, i32, i32, p, p, p, p, i64, p, p]),
        "emcid_edit_dual_apply_assemble_f64": (i32, [i64, i64, i64, p, i64, p]),
        "emcid_edit_dual_preserve_workspace_bytes": (i64, [i64, i64, i64, i64]),
        "emcid_edit_layer_dual_preserve_f64": (i32, [p, p, p, i64, i64, i64, f64, i32, f64, p, i64, i64, p, i64, p, i64, p, i64, i64,
                                                     p, p, p, p, p, i64, p, p]),
        "emcid_session_retain_workspace_bytes": (i64, [i64, i64, i64]),
        "emcid_session_retain_f64": (i32, [p, i64, i64, f64, f64, p, i64, i64, p, i64, p, i64, p, i64, i64, p, i64, p, p]),
        "emcid_session_step_norms_f64": (i32, [p, i64, i64, i64, i64, i64, i64, p, p, p, p]),
        "emcid_session_release_workspace_bytes": (i64, [i64, i64, i64]),
        "emcid_session_release_f64": (i32, [p, i64, i64, i64, p, i64, p, i64, p, i64, i64, p, i64, p, p]),
        "emcid_session_rescale_f64": (i32, [p, p, i64, i64, i64, p, i64, p, i64, p, i64, i64, p, i64, p, p]),
        "emcid_cov_factor_fold_workspace_bytes": (i64, [i64, i64]),
        "emcid_cov_factor_fold_f64": (i32, [p, f64, p, i64, i64, i64, p, f64, f64, i32, p, i64, i64, i64, p, p, i64, p, p]),
        "emcid_session_refold_update_f64": (i32, [p, i64, i64, i64, p, i64, i64, i64, p, i64, i64, p, i64, p, p]),
        "emcid_cov_factor_refactor_f64": (i32, [p, i64, i64, i64, p, p]),
        "emcid_score_rows_f32": (i32, [p, i64, p, i64, p, i64, p, p, f32, i64, i64, p, p]),
        "emcid_score_chains_f64": (i32, [p, i64, p, i64, p, p, i64, p, p]),
        "emcid_score_chains_pair_f64": (i32, [p, i64, p, i64, p, p, p, i64, p, i64, p, p, i64, p, p]),
        "emcid_score_chains_pair_grid_f64": (i32, [p, i64, i64, p, i64, p, p, p, i64, i64, p, i64, p, p, i64, p, i64, p, p]),
        "emcid_score_pooled_f32": (i32, [p, i64, p, i64, p, p, f32, p, i64, i64, i64, i64, p, p]),
        "emcid_cholesky_solve_f64": (i32, [p, i64, i64, p, p, p, i64, i64, p]),
        "emcid_edit_dual_cols_stage1_f64": (i32, [p, p, p, i64, i64, i64, f64, i32, f64, p, i64, i64, p, i32, p, i64, p]),
        "emcid_edit_dual_s": (p, [p, i64, i64, i64]),
        "emcid_edit_dual_u": (p, [p, i64, i64, i64]),
        "emcid_edit_dual_cols_stage2_f64": (i32, [i64, i64, i64, p, i64, i64, p, i32, p, i64, p, p]),
        "emcid_apply_update2d_f32": (i32, [p, i64, p, p, p, i64, i64, p]),
        "emcid_edit_lu_workspace_bytes": (i64, [i64, i64, i64]),
        "emcid_edit_layer_lu_f64": (i32, [p, p, p, p, i64, i64, i64, f64, f64, i32, p, p, p, p, p, p, i64, p, p]),
        "emcid_lu_solve_f64": (i32, [p, i64, i64, p, i64, i64, p, p, p]),
        "emcid_delta_w_f64": (i32, [p, i64, p, i64, i64, i64, i64, p, p, i64, p, p, p]),
        "emcid_dgemm_f64": (i32, [i32, i32, i64, i64, i64, f64, p, i64, p, i64, f64, p, i64, p]),
        "emcid_dgemm_ex_f64": (i32, [i32, i32, i64, i64, i64, f64, p, i64, p, i64, f64, p, i64, i32, i32, i32, p]),
        "emcid_dgemm_batched_f64": (i32, [i32, i32, i64, i64, i64, f64, p, i64, i64, p, i64, i64, f64, p, i64, i64, i64, p]),
        "emcid_streamk_workspace_bytes": (i64, [i32]),
        "emcid_debug_streamk_stamps": (i32, [p]),
        "emcid_debug_linear_sp16_stamps": (i32, [p]),
        "emcid_fingerprint_store": (i32, [i64, p, p, p, p, i64, p]),
        "emcid_fingerprint_check": (i32, [p, i64, i64, i64, p, p, p]),
        "emcid_fingerprint_content": (i32, [i64, p, p, p, p]),
        "emcid_debug_step_stamps": (i32, [p]),
        "emcid_dgemm_streamk_f64": (i32, [i32, i64, i64, i64, f64, p, i64, p, i64, p, i64, i32, i32, f64, p, i64, p]),
        "emcid_axpy_f32": (i32, [p, p, i64, p]),
        "emcid_quick_gelu_f32": (i32, [p, p, i64, p]),
        "emcid_linear_f32": (i32, [p, i64, p, i64, p, p, i64, p, i64, i64, i64, i64, i32, i32, p]),
        "emcid_linear_ws_f32": (i32, [p, i64, p, i64, p, p, i64, p, i64, i64, i64, i64, i32, i32, p, i64, p]),
        "emcid_linear_workspace_bytes": (i64, []),
        "emcid_split_rows_f16": (i32, [p, i64, i64, i64, p, i64, p, p, p]),
        "emcid_gram_sp16_workspace_bytes": (i64, [i64]),
        "emcid_gram_sp16_workspace_bytes_for": (i64, [i64, i64]),
        "emcid_gram_accumulate_sp16_f32": (i32, [p, p, i64, i64, i64, p, i64, p, i64, p]),
        "emcid_add_layernorm_sp16": (i32, [p, i64, p, i64, p, p, C.c_float, i64, i64, p, p, p, i64, p, p, p, p]),
        "emcid_embed_layernorm_sp16": (i32, [p, i64, i64, p, i64, i64, p, p, p, p, C.c_float, i64, i64, p, p, p, i64, p, p]),
        "emcid_tree_attention_sp16_supported": (i32, [i64, i64, i64]),
        "emcid_clip_workspace_bytes": (i64, [i64, i64, i64]),
        "emcid_clip_layer_head_sp16": (i32, [p, i64, i64, i64, i64, f32, p, i64, p, p, i64, p, p, p, p, p, p, p, p, i64, p]),
        "emcid_clip_layer_tail_sp16": (i32, [p, i64, i64, i64, p, p, p, p, p, p, f32, p, p, p]),
        "emcid_clip_layers_sp16": (i32, [p, i64, i64, i64, i64, i64, f32, p, i64, p, p, p, p, p, p, f32, p, i64, p]),
        "emcid_clip_edit_layer_tail_sp16": (i32, [p, i64, i64, i64, p, p, p, p, p, p, i64, i64, p, f64, i32, f64, p, i64, i64, i32,
                                                 p, p, p, p, p, p, p, p, i64, p, p, i64, p, p, p, f32, p, p, p]),
        "emcid_tree_attention_sp16": (i32, [p, i64, p, p, i64, p, i64, p, p, i64, i64, i64, f32, p, i64, p, p]),
        "emcid_linear_sp16_f32": (i32, [p, i64, p, p, i64, p, p, p, i64, p, i64, p, i64, p, i64, i64, i64, i32, i32, p]),
        "emcid_add_layernorm_f32": (i32, [p, i64, p, i64, p, p, C.c_float, i64, i64, p, p, p]),
        "emcid_embed_layernorm_f32": (i32, [p, i64, i64, p, i64, i64, p, p, p, p, C.c_float, i64, i64, p, p, p]),
        "emcid_tree_attention_f32": (i32, [p, i64, p, p, i64, p, i64, p, p, i64, i64, i64, f32, p, i64, p]),
        "emcid_profile_enable": (i32, [C.c_uint]),
        "emcid_profile_collect": (i32, [p, p, i32]),
        "emcid_attention_f32": (i32, [p, p, p, i64, i64, i64, p, i32, i64, i64, i32, f32, i64, i64, i64, i64, p, p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if lib.emcid_abi_version() != ABI_VERSION:
        raise EmcidHipError(f"ABI mismatch: library {lib.emcid_abi_version()} vs binding {ABI_VERSION}; rebuild csrc/")
    _lib = lib
    return lib


_tls = threading.local()  # .restore: device ordinals to go back to after the call in flight (see _stream), per thread


def _check(rc: int, what: str):
    restore = getattr(_tls, "restore", None)
    if restore:
        torch.cuda.set_device(restore.pop())
    if rc != 0:
        raise EmcidHipError(f"{what} failed (rc={rc}): {load().emcid_last_error().decode()}")


def _ptr(t: Optional[torch.Tensor], dtype=None, what="tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise EmcidHipError(f"{what} must live in HBM (got device {t.device}); there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise EmcidHipError(f"{what} must be {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def _stream(t: torch.Tensor):
    """The current HIP stream of the tensor's device — and that device made current for the duration of the call
    (include/emcid_hip.h: the library keys its capture streams, cached graphs and launches by the current device; a model
    on cuda:1 while cuda:0 is current must still run on cuda:1).  Every call site is ``_check(lib.fn(..., _stream(t)), name)``:
    ``_check`` switches back."""
    idx = t.device.index
    cur = torch.cuda.current_device()
    if idx is not None and idx != cur:
        if getattr(_tls, "restore", None) is None:
            _tls.restore = []
        _tls.restore.append(cur)
        torch.cuda.set_device(idx)
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def pinned_copy(t: torch.Tensor) -> torch.Tensor:
    """``t`` on its way to page-locked host memory: the copy is queued on the current stream, not waited for."""
    out = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    out.copy_(t.detach(), non_blocking=True)
    return out


# ---- Stage 0 -----------------------------------------------------------------------------------------

GRAM_SPLIT = os.environ.get("EMCID_GRAM_SPLIT", "1") != "0"      # 0: always the exact-f32 MFMA SYRK
_GRAM_WS = {}


def gram_takes_row_weight(X: torch.Tensor, ksplit: int = 0) -> bool:
    """whether gram_accumulate_ would run this batch on the split-fp16 path (which applies a per-row weight as it reads the rows)"""
    d = X.shape[1]
    return bool(GRAM_SPLIT and ksplit != 1 and X.shape[0] >= 2048 and d % 4 == 0 and d >= 256 and X.stride(0) % 4 == 0
                and X.stride(1) == 1 and X.data_ptr() % 16 == 0 and X.dtype == torch.float32)


def gram_accumulate_(G: torch.Tensor, X: torch.Tensor, ksplit: int = 0, row_weight: Optional[torch.Tensor] = None):
    """G (d,d) fp32 lower triangle += X^T X, X (t,d) fp32 with row stride multiple of 4 (runningstats.py:493).  Long batches
    (>= 2048 tokens, ``ksplit != 1``) run on the split-fp16 path (csrc/gemm_sp16.hip: three f16 MFMAs per k-step on X^T planes
    under per-feature scales, fp32 atomics into G); ``ksplit == 1`` — the deterministic mode — and short batches on the exact-f32
    SYRK (csrc/gram_f32.hip).  ``row_weight`` (t,) fp32: row r enters as fl32(row_weight[r] * X[r]) — on the split path inside the
    kernels that read the rows, otherwise by a multiplication here."""
    assert X.dim() == 2 and G.dim() == 2 and G.shape[0] == G.shape[1] == X.shape[1]
    assert X.stride(1) == 1 and G.stride(1) == 1
    if X.shape[0] == 0:
        return G
    d = X.shape[1]
    if row_weight is not None:
        assert row_weight.shape == (X.shape[0],) and row_weight.dtype == torch.float32 and row_weight.is_contiguous()
        if not (gram_takes_row_weight(X, ksplit) and G.dtype == torch.float32):
            X, row_weight = X * row_weight.unsqueeze(1), None
    if GRAM_SPLIT and ksplit != 1 and X.shape[0] >= 2048 and d % 4 == 0 and d >= 256 and X.stride(0) % 4 == 0 \
            and X.data_ptr() % 16 == 0 and X.dtype == torch.float32 and G.dtype == torch.float32:
        key = (X.device.index if X.device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(X.device).cuda_stream, d)
        # one workspace per (device, stream, d), sized for the largest batch seen there (403 MB at d = 3072 only when a batch
        # reaches the 32 768-token chunk; a 2 048-token batch takes 25 MB)
        need = int(load().emcid_gram_sp16_workspace_bytes_for(d, X.shape[0]))
        ws = _GRAM_WS.get(key)
        if ws is None or ws.numel() < need:
            if ws is None and len(_GRAM_WS) >= 8:
                _GRAM_WS.clear()
            ws = _GRAM_WS[key] = torch.empty(need, dtype=torch.uint8, device=X.device)
        _check(load().emcid_gram_accumulate_sp16_f32(_ptr(X, torch.float32, "X"),
                                                     _ptr(row_weight, torch.float32, "row_weight") if row_weight is not None else None,
                                                     X.shape[0], d, X.stride(0),
                                                     _ptr(G, torch.float32, "G"), G.stride(0), C.c_void_p(ws.data_ptr()),
                                                     ws.numel(), _stream(G)), "emcid_gram_accumulate_sp16_f32")
        return G
    _check(load().emcid_gram_accumulate_f32(_ptr(X, torch.float32, "X"), X.shape[0], X.shape[1], X.stride(0),
                                            _ptr(G, torch.float32, "G"), G.stride(0), ksplit, _stream(G)),
           "emcid_gram_accumulate_f32")
    return G


def symmetrize_lower_(G: torch.Tensor):
    _check(load().emcid_symmetrize_lower_f32(_ptr(G, torch.float32, "G"), G.shape[0], G.stride(0), _stream(G)),
           "emcid_symmetrize_lower_f32")
    return G


# ---- K/Z assembly -------------------------------------------------------------------------------------

def gather_mean(act: torch.Tensor, idx: torch.Tensor, seg: torch.Tensor, out: Optional[torch.Tensor] = None):
    """act (B,S,c) fp32, idx (B,) int64 token position per prompt, seg (N+1,) int64 prompt offsets per request."""
    assert act.dim() == 3 and act.stride(2) == 1
    B, S, c = act.shape
    N = seg.numel() - 1
    assert idx.numel() == B
    if out is None:
        out = torch.empty(N, c, dtype=torch.float32, device=act.device)
    _check(load().emcid_gather_mean_f32(_ptr(act, torch.float32, "act"), B, S, c, act.stride(0), act.stride(1),
                                        _ptr(idx, torch.int64, "idx"), _ptr(seg, torch.int64, "seg"), N,
                                        _ptr(out, torch.float32, "out"), out.stride(0), _stream(act)),
           "emcid_gather_mean_f32")
    return out


# ---- Stage 2 ------------------------------------------------------------------------------------------

def edit_workspace_bytes(N: int, d: int, h: int) -> int:
    return int(load().emcid_edit_workspace_bytes(N, d, h))


class EditWorkspace:
    """Reusable HBM workspace (+ the device `info` word) of emcid_edit_layer_f64 / emcid_edit_layer_shard_f64, or with ``lu``
    of the pivoted-LU fallback emcid_edit_layer_lu_f64."""

    def __init__(self, N: int, d: int, h: int, device, lu: bool = False):
        self.key = (N, d, h)
        self.lu = lu
        self.nbytes = int(load().emcid_edit_lu_workspace_bytes(N, d, h)) if lu else edit_workspace_bytes(N, d, h)
        self.buf = torch.zeros(self.nbytes // 8, dtype=torch.float64, device=device)      # (zero: padding the stages never write)
        self.info = torch.zeros(1, dtype=torch.int32, device=device)


def edit_layer(K, Zc, zs_t, Cov, lam: float, edit_weight: float, layers_left: int, W0=None, W=None,
               want_factors: bool = False, want_dw: bool = True, ws: Optional[EditWorkspace] = None):
    """One edited layer of emcid_main.py:1016-1061 on the GPU.  Returns dict(Xt, Rt, dW) (entries may be None)."""
    N, d = K.shape
    h = Zc.shape[1]
    assert Cov.shape == (d, d) and zs_t.shape == (N, h) and Zc.shape == (N, h)
    for t, nm in ((K, "K"), (Zc, "Zc"), (zs_t, "zs_t"), (Cov, "C")):
        assert t.is_contiguous(), nm
    if ws is None or ws.key != (N, d, h) or ws.lu:
        ws = EditWorkspace(N, d, h, K.device)
    dev = K.device
    Xt = torch.empty(N, d, dtype=torch.float64, device=dev) if want_factors else None
    Rt = torch.empty(N, h, dtype=torch.float64, device=dev) if want_factors else None
    dW = torch.empty(h, d, dtype=torch.float32, device=dev) if want_dw else None
    if W is not None:
        assert W.is_contiguous() and W.shape == (h, d) and W0 is not None and W0.is_contiguous()
    _check(load().emcid_edit_layer_f64(
        _ptr(K, torch.float32, "K"), _ptr(Zc, torch.float32, "Zc"), _ptr(zs_t, torch.float32, "zs_t"),
        _ptr(Cov, torch.float32, "C"), N, d, h, float(lam), float(edit_weight), int(layers_left),
        _ptr(W0, torch.float32, "W0"), _ptr(W, torch.float32, "W"), _ptr(Xt), _ptr(Rt), _ptr(dW),
        _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32, "info"), _stream(K)), "emcid_edit_layer_f64")
    return {"Xt": Xt, "Rt": Rt, "dW": dW, "ws": ws}


def edit_layer_lu(K, Zc, zs_t, Cov, lam: float, edit_weight: float, layers_left: int, W0=None, W=None,
                  want_factors: bool = False, want_dw: bool = True, ws: Optional[EditWorkspace] = None):
    """One edited layer solved like the reference does (LU with partial pivoting, torch.linalg.solve's algorithm): works for
    any nonsingular lam*C' + K K^T.  Returns dict(adj_k (d, N) | None, Rt (N, h) | None, dW, ws)."""
    N, d = K.shape
    h = Zc.shape[1]
    assert Cov.shape == (d, d) and zs_t.shape == (N, h) and Zc.shape == (N, h)
    for t, nm in ((K, "K"), (Zc, "Zc"), (zs_t, "zs_t"), (Cov, "C")):
        assert t.is_contiguous(), nm
    if ws is None or ws.key != (N, d, h) or not ws.lu:
        ws = EditWorkspace(N, d, h, K.device, lu=True)
    dev = K.device
    adj_k = torch.empty(d, N, dtype=torch.float64, device=dev) if want_factors else None
    Rt = torch.empty(N, h, dtype=torch.float64, device=dev) if want_factors else None
    dW = torch.empty(h, d, dtype=torch.float32, device=dev) if want_dw else None
    if W is not None:
        assert W.is_contiguous() and W.shape == (h, d) and W0 is not None and W0.is_contiguous()
    _check(load().emcid_edit_layer_lu_f64(
        _ptr(K, torch.float32, "K"), _ptr(Zc, torch.float32, "Zc"), _ptr(zs_t, torch.float32, "zs_t"),
        _ptr(Cov, torch.float32, "C"), N, d, h, float(lam), float(edit_weight), int(layers_left),
        _ptr(W0, torch.float32, "W0"), _ptr(W, torch.float32, "W"), _ptr(adj_k), _ptr(Rt), _ptr(dW),
        _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32, "info"), _stream(K)), "emcid_edit_layer_lu_f64")
    return {"adj_k": adj_k, "Rt": Rt, "dW": dW, "ws": ws}


def lu_solve_(A: torch.Tensor, B: torch.Tensor):
    """Test hook: solves A X = B in place (A (n, n) f64 becomes P L U, B (n, nrhs) f64 becomes X) by LU with partial
    pivoting; returns (pivots int32 (n,), info int32 (1,))."""
    n = A.shape[0]
    piv = torch.zeros(n, dtype=torch.int32, device=A.device)
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    _check(load().emcid_lu_solve_f64(_ptr(A, torch.float64, "A"), A.stride(0), n, _ptr(B, torch.float64, "B"), B.stride(0),
                                     B.shape[1], _ptr(piv), _ptr(info), _stream(A)), "emcid_lu_solve_f64")
    return piv, info


def edit_layer_shard(K, Zc, zs_t, Cov, lam: float, edit_weight: float, layers_left: int, rows, want_factors=False,
                     ws: Optional[EditWorkspace] = None):
    """Concept-sharded layer: all N concepts assemble/factor A, only rows [lo, hi) are solved.
    Returns dict(U=(h,d) f64 partial, Xt, Rt (shard rows or None), ws)."""
    N, d = K.shape
    h = Zc.shape[1]
    lo, hi = rows
    assert Cov.shape == (d, d) and zs_t.shape == (N, h) and Zc.shape == (N, h) and 0 <= lo < hi <= N
    for t, nm in ((K, "K"), (Zc, "Zc"), (zs_t, "zs_t"), (Cov, "C")):
        assert t.is_contiguous(), nm
    if ws is None or ws.key != (N, d, h) or ws.lu:
        ws = EditWorkspace(N, d, h, K.device)
    dev = K.device
    U = torch.empty(h, d, dtype=torch.float64, device=dev)
    Xt = torch.empty(hi - lo, d, dtype=torch.float64, device=dev) if want_factors else None
    Rt = torch.empty(hi - lo, h, dtype=torch.float64, device=dev) if want_factors else None
    _check(load().emcid_edit_layer_shard_f64(
        _ptr(K, torch.float32, "K"), _ptr(Zc, torch.float32, "Zc"), _ptr(zs_t, torch.float32, "zs_t"),
        _ptr(Cov, torch.float32, "C"), N, d, h, float(lam), float(edit_weight), int(layers_left), lo, hi,
        _ptr(U), _ptr(Xt), _ptr(Rt), _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32, "info"), _stream(K)),
        "emcid_edit_layer_shard_f64")
    return {"U": U, "Xt": Xt, "Rt": Rt, "ws": ws}


def apply_update_(U, W0, W, want_dw=True):
    """W = W0 + float(U); returns dW = float(U) (or None)."""
    assert U.is_contiguous() and W.is_contiguous() and W0.is_contiguous() and U.shape == W.shape
    dW = torch.empty_like(W) if want_dw else None
    _check(load().emcid_apply_update_f32(_ptr(U, torch.float64, "U"), _ptr(W0, torch.float32, "W0"),
                                         _ptr(W, torch.float32, "W"), _ptr(dW), W.numel(), _stream(W)),
           "emcid_apply_update_f32")
    return dW


def dgemm(ta: int, tb: int, A, B, Cm, alpha=1.0, beta=0.0, M=None, N=None, K=None):
    """Test hook for the fp64 MFMA GEMM. ta/tb = 0: operand stored [rows][K]; 1: stored [K][rows]."""
    M = M if M is not None else (A.shape[0] if ta == 0 else A.shape[1])
    K = K if K is not None else (A.shape[1] if ta == 0 else A.shape[0])
    N = N if N is not None else (B.shape[0] if tb == 0 else B.shape[1])
    _check(load().emcid_dgemm_f64(ta, tb, M, N, K, float(alpha), _ptr(A, torch.float64), A.stride(0),
                                  _ptr(B, torch.float64), B.stride(0), float(beta), _ptr(Cm, torch.float64),
                                  Cm.stride(0), _stream(Cm)), "emcid_dgemm_f64")
    return Cm


def dgemm_ex(ta: int, tb: int, A, B, Cm, alpha=1.0, beta=0.0, flags=0, cfg=-1, ksplit=0):
    """Test hook: the GEMM with the solver's structure hints (triangular operands, lower-only, tile config, K split)."""
    M = A.shape[0] if ta == 0 else A.shape[1]
    K = A.shape[1] if ta == 0 else A.shape[0]
    N = B.shape[0] if tb == 0 else B.shape[1]
    _check(load().emcid_dgemm_ex_f64(ta, tb, M, N, K, float(alpha), _ptr(A, torch.float64), A.stride(0),
                                     _ptr(B, torch.float64), B.stride(0), float(beta), _ptr(Cm, torch.float64),
                                     Cm.stride(0), int(flags), int(cfg), int(ksplit), _stream(Cm)), "emcid_dgemm_ex_f64")
    return Cm


_streamk_ws = {}


def dgemm_streamk(tb: int, A, B, Cm, alpha=1.0, flags=1, wgs=256, diag_add=0.0):
    """Test hook: the two-phase (atomic-free, reproducible) stream-K GEMM; flags 1/2: triangular B, 16: lower-only square."""
    M, K = A.shape
    N = B.shape[0] if tb == 0 else B.shape[1]
    key = (str(A.device), wgs)
    ws = _streamk_ws.get(key)
    if ws is None:
        ws = _streamk_ws[key] = torch.zeros(int(load().emcid_streamk_workspace_bytes(wgs)) // 8, dtype=torch.float64, device=A.device)
    _check(load().emcid_dgemm_streamk_f64(tb, M, N, K, float(alpha), _ptr(A, torch.float64), A.stride(0), _ptr(B, torch.float64),
                                          B.stride(0), _ptr(Cm, torch.float64), Cm.stride(0), int(flags), int(wgs), float(diag_add),
                                          _ptr(ws), ws.numel() * 8, _stream(Cm)), "emcid_dgemm_streamk_f64")
    return Cm


def dgemm_batched(ta: int, tb: int, A, B, Cm, alpha=1.0, beta=0.0):
    """C[b] = alpha * opA(A[b]) opB(B[b]) + beta * C[b] for 3-D operands (batch, rows, cols) with unit inner stride;
    ta/tb as in `dgemm`.  A batch stride of 0 (an expanded operand) shares that operand across the batch."""
    nb = Cm.shape[0]
    M = A.shape[1] if ta == 0 else A.shape[2]
    K = A.shape[2] if ta == 0 else A.shape[1]
    N = B.shape[1] if tb == 0 else B.shape[2]
    for t_, nm in ((A, "A"), (B, "B"), (Cm, "C")):
        if t_.dim() != 3 or t_.stride(2) != 1 or t_.shape[0] != nb:
            raise EmcidHipError(f"dgemm_batched: {nm} must be (batch, rows, cols) with unit inner stride")
    if Cm.shape[1] != M or Cm.shape[2] != N or (B.shape[2] if tb == 0 else B.shape[1]) != K:
        raise EmcidHipError("dgemm_batched: shapes do not agree")
    _check(load().emcid_dgemm_batched_f64(ta, tb, M, N, K, float(alpha), _ptr(A, torch.float64), A.stride(1), A.stride(0),
                                          _ptr(B, torch.float64), B.stride(1), B.stride(0), float(beta),
                                          _ptr(Cm, torch.float64), Cm.stride(1), Cm.stride(0), nb, _stream(Cm)),
           "emcid_dgemm_batched_f64")
    return Cm


def fingerprint_store(entries, table: torch.Tensor):
    """Stale-cache guard (include/emcid_hip.h): leave {address, bytes, fingerprint of the bytes} of every ``(tensor, slot)`` of
    ``entries`` in ``table[slot]`` — one launch per 32 entries."""
    n = len(entries)
    if not n:
        return
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t, _ in entries])
    sizes = (C.c_int64 * n)(*[t.numel() * t.element_size() for t, _ in entries])
    slots = (C.c_int64 * n)(*[int(s) for _, s in entries])
    _check(load().emcid_fingerprint_store(n, ptrs, sizes, slots, _ptr(table, torch.int64, "table"), table.shape[0], _stream(table)),
           "emcid_fingerprint_store")


def fingerprint_check(table: torch.Tensor, first_slot: int, n_slots: int, flag: torch.Tensor, skip=()):
    """Recompute the fingerprints of ``table[first_slot : first_slot + n_slots]`` (empty slots and the slot offsets in ``skip``
    are not looked at); ``flag |= 1`` on a mismatch."""
    mask = (C.c_uint64 * 4)()
    for k in skip:
        mask[k >> 6] |= 1 << (k & 63)
    _check(load().emcid_fingerprint_check(_ptr(table, torch.int64, "table"), table.shape[0], int(first_slot), int(n_slots), mask,
                                          _ptr(flag, torch.int32, "flag"), _stream(table)), "emcid_fingerprint_check")


def fingerprint_content(tensors) -> torch.Tensor:
    """The guard's fingerprint of the BYTES of every tensor of ``tensors`` (all in HBM, on one device) without its address
    (include/emcid_hip.h, "content fingerprint"): an int64 tensor of len(tensors) words on that device — one launch per 32
    tensors on the current stream, no synchronisation; equal bytes give equal words in any process.  A tensor whose size is no
    multiple of 16 bytes (or that is not contiguous, or not 16-byte aligned) is fingerprinted as a contiguous copy padded with
    zeros.  A word says nothing of the shape or dtype: compare those on the host."""
    tensors = list(tensors)
    if not tensors:
        raise EmcidHipError("fingerprint_content needs at least one tensor")
    dev = tensors[0].device
    held = []
    for k, t in enumerate(tensors):
        if not t.is_cuda or t.device != dev:
            raise EmcidHipError(f"fingerprint_content: tensor {k} must live in HBM on {dev} (got {t.device}); there is no CPU path")
        t = t.detach()
        nbytes = t.numel() * t.element_size()
        if nbytes == 0:
            raise EmcidHipError(f"fingerprint_content: tensor {k} is empty")
        if nbytes % 16 or t.data_ptr() % 16 or not t.is_contiguous():
            padded = torch.zeros((nbytes + 15) // 16 * 16, dtype=torch.uint8, device=dev)
            padded[:nbytes].view(t.dtype).copy_(t.reshape(-1))
            t = padded
        held.append(t)
    n = len(held)
    out = torch.zeros(n, dtype=torch.int64, device=dev)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in held])
    sizes = (C.c_int64 * n)(*[t.numel() * t.element_size() for t in held])
    _check(load().emcid_fingerprint_content(n, ptrs, sizes, _ptr(out, torch.int64, "out"), _stream(out)), "emcid_fingerprint_content")
    return out


def axpy_(W: torch.Tensor, dW: torch.Tensor):
    """W += dW, fp32 (emcid_main.py:809)."""
    assert W.is_contiguous() and dW.is_contiguous() and W.numel() == dW.numel()
    _check(load().emcid_axpy_f32(_ptr(W, torch.float32, "W"), _ptr(dW, torch.float32, "dW"), W.numel(), _stream(W)),
           "emcid_axpy_f32")
    return W


def cholesky(A: torch.Tensor):
    """Test hook: A (dp,dp) f64 contiguous, dp % 128 == 0.  Returns (L, inverse workspace, info); the first
    ceil(dp/512) slots of 512*512 doubles of the workspace are the inverted 512-blocks of L (ld 512)."""
    dp = A.shape[0]
    L = torch.zeros_like(A)
    inv = torch.empty(int(load().emcid_inverse_workspace_doubles(dp)), dtype=torch.float64, device=A.device)
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    _check(load().emcid_cholesky_f64(_ptr(A, torch.float64), _ptr(L), dp, A.stride(0), _ptr(inv), _ptr(info), _stream(A)),
           "emcid_cholesky_f64")
    return L, inv, info


def cholesky_solve_(L, inv, Bt):
    """Test hook: Bt (Np,dp) f64 := Bt (L L^T)^{-1}."""
    Y = torch.empty_like(Bt)
    _check(load().emcid_cholesky_solve_f64(_ptr(L, torch.float64), L.shape[0], L.stride(0), _ptr(inv), _ptr(Bt), _ptr(Y),
                                           Bt.shape[0], Bt.stride(0), _stream(Bt)), "emcid_cholesky_solve_f64")
    return Bt


def delta_w_(Rt, Xt, W0, W):
    """W = W0 + float(Rt^T Xt): the dW contraction of emcid_main.py:1050,:1061 alone, for factors that are already
    there (Rt (N, h) f64 residual rows, Xt (N, d) f64 rows of adj_k^T; both contiguous)."""
    N, h = Rt.shape
    d = Xt.shape[1]
    assert Xt.shape[0] == N and W.shape == (h, d) and W0.shape == (h, d)
    for t, nm in ((Rt, "Rt"), (Xt, "Xt"), (W0, "W0"), (W, "W")):
        assert t.is_contiguous(), nm
    if h % 2 or d % 2:
        raise EmcidHipError("delta_w_: h and d must be even (16-byte aligned f64 rows)")
    _check(load().emcid_delta_w_f64(_ptr(Rt, torch.float64, "Rt"), h, _ptr(Xt, torch.float64, "Xt"), d, N, h, d,
                                    _ptr(W0, torch.float32, "W0"), _ptr(W, torch.float32, "W"), d, None, None, _stream(W)),
           "emcid_delta_w_f64")
    return W


def profile_enable(classes=()):
    """Start (or, with no classes, stop) HIP-event timing of the named kernel classes (PROF_CLASSES)."""
    mask = 0
    for c in classes:
        mask |= 1 << PROF_CLASSES.index(c)
    _check(load().emcid_profile_enable(mask), "emcid_profile_enable")


def profile_collect():
    """{class: (total_ms, launches)} for the classes that recorded launches since profile_enable."""
    n = len(PROF_CLASSES)
    ms = (C.c_double * n)()
    cnt = (C.c_int64 * n)()
    _check(load().emcid_profile_collect(ms, cnt, n), "emcid_profile_collect")
    return {PROF_CLASSES[i]: (ms[i], int(cnt[i])) for i in range(n) if cnt[i]}


def attention(q, k, v, mask=None, causal=False, scale=None):
    """q/k/v: (B, H, S, D) fp32 views with unit stride over D and identical strides; mask: None, bool keep-mask or
    additive float, shape (B|1, 1, S, S).  Returns (B, S, H, D) contiguous."""
    B, H, S, D = q.shape
    for t in (q, k, v):
        if t.stride(3) != 1 or t.stride() != q.stride() or t.shape != q.shape:
            raise EmcidHipError("attention: q/k/v must share shape/strides with unit stride over head_dim")
    out = torch.empty(B, S, H, D, dtype=torch.float32, device=q.device)
    kind, mptr, mb, mi = 0, None, 0, 0
    if mask is not None:
        if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[2] != S or mask.shape[3] != S or mask.stride(3) != 1:
            mask = mask.expand(-1, 1, S, S).contiguous() if mask.dim() == 4 and mask.shape[1] == 1 else None
            if mask is None:
                raise EmcidHipError("attention: mask must be (B|1, 1, S, S)")
        if mask.dtype == torch.bool:
            kind, mptr = 1, _ptr(mask)
        elif mask.dtype == torch.float32:
            kind, mptr = 2, _ptr(mask)
        else:
            raise EmcidHipError(f"attention: mask dtype {mask.dtype} not supported")
        mb = mask.stride(0) if mask.shape[0] > 1 else 0
        mi = mask.stride(2)
    scale = float(D ** -0.5 if scale is None else scale)
    _check(load().emcid_attention_f32(_ptr(q, torch.float32, "q"), _ptr(k, torch.float32, "k"), _ptr(v, torch.float32, "v"),
                                      q.stride(0), q.stride(1), q.stride(2), mptr, kind, mb, mi, int(bool(causal)), scale,
                                      B, H, S, D, _ptr(out), _stream(q)), "emcid_attention_f32")
    return out


def quick_gelu(x: torch.Tensor) -> torch.Tensor:
    """x * sigmoid(1.702 x), fp32, one pass."""
    x = x.contiguous()
    y = torch.empty_like(x)
    _check(load().emcid_quick_gelu_f32(_ptr(x, torch.float32, "x"), _ptr(y), x.numel(), _stream(x)), "emcid_quick_gelu_f32")
    return y


ACT_NONE, ACT_QUICK_GELU, ACT_GELU_ERF = 0, 1, 2
LINEAR_FLOPS = {"count": False, "flops": 0.0, "launches": 0}      # bench.py's roofline pass: algorithmic 2 M N K of every launch


def linear_supported(x: torch.Tensor, w: torch.Tensor) -> bool:
    """True when ``linear`` takes these operands: fp32 in HBM, K contiguous and a multiple of 16, 16-byte aligned rows."""
    return (x.is_cuda and w.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32 and x.dim() == 2 and w.dim() == 2
            and x.shape[1] == w.shape[1] and x.shape[1] % 16 == 0 and x.stride(1) == 1 and w.stride(1) == 1
            and x.stride(0) % 4 == 0 and w.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
            and x.shape[0] > 0)


_LINEAR_WS = {}       # (device index, stream handle) -> the split-K form's workspace (zeroed once; every launch leaves its counters zero)


def linear_split_cfg(parts: int, prefetch: int = 2) -> int:
    """``cfg`` of the split-K form: 128 x 128 tiles, four waves, every tile's K range over ``parts`` (2..8) workgroups."""
    return 64 + 1 + 4 * (prefetch - 1) + (int(parts) << 7)


def _linear_workspace(dev: torch.device) -> torch.Tensor:
    """Launches of one stream run one after the other and share the partial-tile slots; launches of different streams (the two
    encoders of an SDXL edit) may overlap and get their own (32 MB each)."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    ws = _LINEAR_WS.get(key)
    if ws is None:
        if len(_LINEAR_WS) >= 8:
            _LINEAR_WS.clear()
        ws = _LINEAR_WS[key] = torch.zeros(int(load().emcid_linear_workspace_bytes()), dtype=torch.uint8, device=dev)
    return ws


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
           residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, cfg: int = -1) -> torch.Tensor:
    """act(x @ w.T + bias) + residual in one launch (csrc/gemm_f32.hip): x (M, K), w (N, K) like nn.Linear.weight, bias (N,),
    residual (M, N) row views; fp32, exact-f32 MFMA.  Launches of at most 128 tiles on a K of 2048 or more are cut by K over
    several workgroups per tile (partial tiles meet in a per-stream workspace, fixed summation order)."""
    if not linear_supported(x, w):
        raise EmcidHipError("linear: fp32 HBM operands with K contiguous, K % 16 == 0 and 16-byte aligned rows")
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    if out.shape != (M, N) or out.stride(1) != 1 or out.dtype != torch.float32:
        raise EmcidHipError("linear: out must be an (M, N) fp32 row view")
    if bias is not None and (bias.shape != (N,) or not bias.is_contiguous()):
        raise EmcidHipError("linear: bias must be a contiguous (N,) vector")
    if residual is not None and (residual.shape != (M, N) or residual.stride(1) != 1):
        raise EmcidHipError("linear: residual must be an (M, N) row view")
    if LINEAR_FLOPS["count"]:
        LINEAR_FLOPS["flops"] += 2.0 * M * N * K
        LINEAR_FLOPS["launches"] += 1
    ws = None
    if (cfg >= 128 or (cfg < 0 and K >= 2048 and -(-M // 128) * -(-N // 128) <= 128)) and not torch.cuda.is_current_stream_capturing():
        ws = _linear_workspace(x.device)
    try:
        _check(load().emcid_linear_ws_f32(_ptr(x, torch.float32, "x"), x.stride(0), _ptr(w, torch.float32, "w"), w.stride(0),
                                          _ptr(bias, torch.float32, "bias"), _ptr(residual, torch.float32, "residual"),
                                          residual.stride(0) if residual is not None else 0, _ptr(out, torch.float32, "out"),
                                          out.stride(0), M, N, K, int(act), int(cfg),
                                          C.c_void_p(ws.data_ptr()) if ws is not None else None, ws.numel() if ws is not None else 0,
                                          _stream(x)), "emcid_linear_ws_f32")
    except EmcidHipError:
        # the split-K form relies on its ticket counters being zero on entry; a launch that did not complete may have left
        # some behind — later launches on this stream would then never see a "last arriver".  Start from a fresh workspace.
        if ws is not None:
            _LINEAR_WS.pop((x.device.index if x.device.index is not None else torch.cuda.current_device(),
                            torch.cuda.current_stream(x.device).cuda_stream), None)
        raise
    return out


class SplitRows:
    """An fp32 matrix (rows, K) as two fp16 planes under per-row power-of-two scales (include/emcid_hip.h, "split fp16"):
    ``planes`` int32 (rows, K) — one 4-byte unit per element, [hi x 8][lo x 8] per group of 8 k —, ``inv_scale`` fp32 (rows,).
    ``f32``: the fp32 matrix itself when the producer wrote it too; ``bound``: for a weight, the device pair
    (largest row norm, largest |bias|) ``add_layernorm_sp`` turns into the scale of the projection's own split output."""
    __slots__ = ("planes", "inv_scale", "f32", "bound", "out_scale")

    def __init__(self, planes: torch.Tensor, inv_scale: torch.Tensor, f32: Optional[torch.Tensor] = None,
                 bound: Optional[torch.Tensor] = None, out_scale: Optional[torch.Tensor] = None):
        self.planes, self.inv_scale, self.f32, self.bound = planes, inv_scale, f32, bound
        self.out_scale = out_scale        # (2, rows): scale / inverse scale for the split OUTPUT of the projection that consumes this

    @property
    def shape(self):
        return self.planes.shape

    def index_select(self, idx: torch.Tensor) -> "SplitRows":
        return SplitRows(self.planes.index_select(0, idx), self.inv_scale.index_select(0, idx),
                         self.f32.index_select(0, idx) if self.f32 is not None else None)

    def rows(self, lo: int, hi: int) -> "SplitRows":
        return SplitRows(self.planes[lo:hi], self.inv_scale[lo:hi], self.f32[lo:hi] if self.f32 is not None else None)

    def float(self) -> torch.Tensor:
        """Back to fp32: the twin when there is one, else (hi + lo) * 2^-e (22-23 significant bits)."""
        if self.f32 is not None:
            return self.f32
        r, k = self.planes.shape
        h = self.planes.contiguous().view(torch.float16).view(r, k // 8, 2, 8).float()
        return ((h[:, :, 0] + h[:, :, 1]).reshape(r, k)) * self.inv_scale[:, None]


def split_supported(x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] % 32 == 0 and x.stride(1) == 1
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and x.shape[0] > 0)


def split_rows(x: torch.Tensor, bias: Optional[torch.Tensor] = None, want_bound: bool = False) -> SplitRows:
    """fp32 rows -> split fp16 planes (csrc/gemm_sp16.hip: split_rows_kernel).  ``want_bound`` (weights): also the device pair
    (largest Euclidean row norm, largest |bias|)."""
    if not split_supported(x):
        raise EmcidHipError("split_rows: fp32 HBM rows with K contiguous, K % 32 == 0 and 16-byte aligned rows")
    rows, K = x.shape
    planes = torch.empty(rows, K, dtype=torch.int32, device=x.device)
    inv = torch.empty(rows, dtype=torch.float32, device=x.device)
    bound = None
    if want_bound:
        bound = torch.zeros(2, dtype=torch.float32, device=x.device)
        if bias is not None:
            bound[1:2] = bias.detach().abs().max()
    _check(load().emcid_split_rows_f16(_ptr(x, torch.float32, "x"), x.stride(0), rows, K, _ptr(planes), planes.stride(0), _ptr(inv),
                                       _ptr(bound), _stream(x)), "emcid_split_rows_f16")
    return SplitRows(planes, inv, None, bound)


def linear_sp(x: SplitRows, w: SplitRows, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
              residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, want_f32: bool = True,
              planes_scale: Optional[torch.Tensor] = None, cfg: int = -1):
    """act(x @ w.T + bias) + residual with both operands given as split fp16 matrices (three f16 MFMAs per k-step, fp32
    accumulate).  Returns the fp32 result, or — with ``planes_scale`` ((2, M): per-row 2^e bounding the result rows, and 2^-e) —
    the result as a SplitRows (its ``f32`` twin too unless ``want_f32=False``)."""
    M, K = x.planes.shape
    N = w.planes.shape[0]
    if w.planes.shape[1] != K or K % 32:
        raise EmcidHipError("linear_sp: operands (M, K) and (N, K) with K % 32 == 0")
    for t in (x.planes, w.planes):
        if t.stride(1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16 or t.dtype != torch.int32:
            raise EmcidHipError("linear_sp: planes must be int32 row views with 16-byte aligned rows")
    dev = x.planes.device
    y = None
    if want_f32 or planes_scale is None:
        y = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=dev)
        if y.shape != (M, N) or y.stride(1) != 1 or y.dtype != torch.float32:
            raise EmcidHipError("linear_sp: out must be an (M, N) fp32 row view")
    yp = None
    if planes_scale is not None:
        if N % 32 or planes_scale.shape != (2, M) or not planes_scale.is_contiguous():
            raise EmcidHipError("linear_sp: planes output needs N % 32 == 0 and a contiguous (2, M) scale / inverse scale")
        yp = torch.empty(M, N, dtype=torch.int32, device=dev)
    if bias is not None and (bias.shape != (N,) or not bias.is_contiguous()):
        raise EmcidHipError("linear_sp: bias must be a contiguous (N,) vector")
    if residual is not None and (residual.shape != (M, N) or residual.stride(1) != 1):
        raise EmcidHipError("linear_sp: residual must be an (M, N) row view")
    if LINEAR_FLOPS["count"]:
        LINEAR_FLOPS["flops"] += 2.0 * M * N * K
        LINEAR_FLOPS["launches"] += 1
    _check(load().emcid_linear_sp16_f32(
        _ptr(x.planes), x.planes.stride(0), _ptr(x.inv_scale, torch.float32, "x scale"), _ptr(w.planes), w.planes.stride(0),
        _ptr(w.inv_scale, torch.float32, "w scale"), _ptr(bias, torch.float32, "bias"), _ptr(residual, torch.float32, "residual"),
        residual.stride(0) if residual is not None else 0, _ptr(y), y.stride(0) if y is not None else 0, _ptr(yp),
        yp.stride(0) if yp is not None else 0, _ptr(planes_scale, torch.float32, "planes scale"), M, N, K, int(act), int(cfg),
        _stream(x.planes)), "emcid_linear_sp16_f32")
    if planes_scale is None:
        return y
    return SplitRows(yp, planes_scale[1], y)


def add_layernorm(a: torch.Tensor, b: Optional[torch.Tensor], ln: torch.nn.LayerNorm, want_sum: bool = True):
    """(a + b, LayerNorm(a + b)) in one pass; a, b (rows, cols) fp32 with unit column stride.  ``b=None``: LayerNorm(a)
    alone (returns (a, LayerNorm(a)); nothing but z is written)."""
    rows, cols = a.shape
    if a.stride(1) != 1 or (b is not None and (b.stride(1) != 1 or b.shape != a.shape)):
        raise EmcidHipError("add_layernorm: (rows, cols) operands with unit column stride")
    if ln.weight is None or ln.bias is None or tuple(ln.normalized_shape) != (cols,):
        raise EmcidHipError("add_layernorm: LayerNorm over the last dimension with affine parameters")
    y = torch.empty(rows, cols, dtype=torch.float32, device=a.device) if (b is not None and want_sum) else None
    z = torch.empty(rows, cols, dtype=torch.float32, device=a.device)
    _check(load().emcid_add_layernorm_f32(_ptr(a, torch.float32, "a"), a.stride(0), _ptr(b, torch.float32, "b"),
                                          b.stride(0) if b is not None else 0,
                                          _ptr(ln.weight, torch.float32, "gamma"), _ptr(ln.bias, torch.float32, "beta"),
                                          float(ln.eps), rows, cols, _ptr(y), _ptr(z), _stream(a)), "emcid_add_layernorm_f32")
    return (a if b is None else y), z


def add_layernorm_sp(a: torch.Tensor, b: Optional[torch.Tensor], ln: torch.nn.LayerNorm, want_sum: bool = True,
                     want_f32: bool = False, bound: Optional[torch.Tensor] = None):
    """``add_layernorm`` with the LayerNorm's output as a split-fp16 matrix for the projection that consumes it:
    returns (a + b | a, SplitRows of LayerNorm(a + b) [with .f32 when ``want_f32``]).  ``bound`` (the consuming weight's
    ``SplitRows.bound``): the result's ``out_scale`` (2, rows) = the per-row 2^e (and 2^-e) under which that projection may write its
    own output as planes (``linear_sp(planes_scale=...)``)."""
    rows, cols = a.shape
    if a.stride(1) != 1 or (b is not None and (b.stride(1) != 1 or b.shape != a.shape)):
        raise EmcidHipError("add_layernorm_sp: (rows, cols) operands with unit column stride")
    if ln.weight is None or ln.bias is None or tuple(ln.normalized_shape) != (cols,) or cols % 32 or cols > 2048:
        raise EmcidHipError("add_layernorm_sp: LayerNorm over the last dimension with affine parameters, cols % 32 == 0, <= 2048")
    dev = a.device
    y = torch.empty(rows, cols, dtype=torch.float32, device=dev) if (b is not None and want_sum) else None
    z = torch.empty(rows, cols, dtype=torch.float32, device=dev) if want_f32 else None
    planes = torch.empty(rows, cols, dtype=torch.int32, device=dev)
    inv = torch.empty(rows, dtype=torch.float32, device=dev)
    out_scale = torch.empty(2, rows, dtype=torch.float32, device=dev) if bound is not None else None
    _check(load().emcid_add_layernorm_sp16(_ptr(a, torch.float32, "a"), a.stride(0), _ptr(b, torch.float32, "b"),
                                           b.stride(0) if b is not None else 0,
                                           _ptr(ln.weight, torch.float32, "gamma"), _ptr(ln.bias, torch.float32, "beta"),
                                           float(ln.eps), rows, cols, _ptr(y), _ptr(z), _ptr(planes), planes.stride(0), _ptr(inv),
                                           _ptr(bound, torch.float32, "bound"), _ptr(out_scale), _stream(a)),
           "emcid_add_layernorm_sp16")
    return (a if b is None else y), SplitRows(planes, inv, z, None, out_scale)


def embed_layernorm_sp(tok_emb: torch.Tensor, pos_emb: torch.Tensor, token: torch.Tensor, position: torch.Tensor,
                       ln: torch.nn.LayerNorm):
    """``embed_layernorm`` with the LayerNorm's output as a split-fp16 matrix: (embeddings, SplitRows)."""
    rows, cols = token.numel(), tok_emb.shape[1]
    if tok_emb.stride(1) != 1 or pos_emb.stride(1) != 1 or pos_emb.shape[1] != cols or position.numel() != rows:
        raise EmcidHipError("embed_layernorm_sp: embedding tables with unit column stride and one index pair per row")
    if ln.weight is None or ln.bias is None or tuple(ln.normalized_shape) != (cols,) or cols % 32 or cols > 2048:
        raise EmcidHipError("embed_layernorm_sp: LayerNorm over the last dimension with affine parameters, cols % 32 == 0, <= 2048")
    y = torch.empty(rows, cols, dtype=torch.float32, device=tok_emb.device)
    planes = torch.empty(rows, cols, dtype=torch.int32, device=tok_emb.device)
    inv = torch.empty(rows, dtype=torch.float32, device=tok_emb.device)
    _check(load().emcid_embed_layernorm_sp16(_ptr(tok_emb, torch.float32, "tok_emb"), tok_emb.stride(0), tok_emb.shape[0],
                                             _ptr(pos_emb, torch.float32, "pos_emb"), pos_emb.stride(0), pos_emb.shape[0],
                                             _ptr(token, torch.int64, "token"), _ptr(position, torch.int32, "position"),
                                             _ptr(ln.weight, torch.float32, "gamma"), _ptr(ln.bias, torch.float32, "beta"),
                                             float(ln.eps), rows, cols, _ptr(y), None, _ptr(planes), planes.stride(0), _ptr(inv),
                                             _stream(tok_emb)), "emcid_embed_layernorm_sp16")
    return y, SplitRows(planes, inv)


def tree_attention_sp_supported(anc: torch.Tensor, H: int, D: int) -> bool:
    return bool(load().emcid_tree_attention_sp16_supported(anc.shape[1], H, D)) and (H * D) % 32 == 0


def tree_attention_sp(q, k, v, anc, depth, H: int, scale=None, rows=None) -> SplitRows:
    """``tree_attention`` with the result as a split-fp16 matrix for the out-projection (short chains only)."""
    U, HD = k.shape
    D = HD // H
    for t in (q, k, v):
        if t.stride(1) != 1 or t.shape[1] != HD:
            raise EmcidHipError("tree_attention_sp: q/k/v must be row-major")
    if k.stride(0) != v.stride(0):
        raise EmcidHipError("tree_attention_sp: k and v must share a leading dimension")
    n = U if rows is None else rows.numel()
    if q.shape[0] != n:
        raise EmcidHipError(f"tree_attention_sp: {q.shape[0]} query rows for {n} query nodes")
    planes = torch.empty(n, HD, dtype=torch.int32, device=q.device)
    inv = torch.empty(n, dtype=torch.float32, device=q.device)
    scale = float(D ** -0.5 if scale is None else scale)
    _check(load().emcid_tree_attention_sp16(
        _ptr(q, torch.float32, "q"), q.stride(0), _ptr(k, torch.float32, "k"), _ptr(v, torch.float32, "v"), k.stride(0),
        _ptr(anc, torch.int32, "anc"), anc.stride(0), _ptr(depth, torch.int32, "depth"),
        _ptr(rows, torch.int32, "rows") if rows is not None else None, n, H, D, scale, _ptr(planes), planes.stride(0), _ptr(inv),
        _stream(q)), "emcid_tree_attention_sp16")
    return SplitRows(planes, inv)


def embed_layernorm(tok_emb: torch.Tensor, pos_emb: torch.Tensor, token: torch.Tensor, position: torch.Tensor,
                    ln: torch.nn.LayerNorm):
    """(tok_emb[token] + pos_emb[position], LayerNorm of it) in one launch; token int64 (rows,), position int32 (rows,)."""
    rows, cols = token.numel(), tok_emb.shape[1]
    if tok_emb.stride(1) != 1 or pos_emb.stride(1) != 1 or pos_emb.shape[1] != cols or position.numel() != rows:
        raise EmcidHipError("embed_layernorm: embedding tables with unit column stride and one index pair per row")
    if ln.weight is None or ln.bias is None or tuple(ln.normalized_shape) != (cols,):
        raise EmcidHipError("embed_layernorm: LayerNorm over the last dimension with affine parameters")
    y = torch.empty(rows, cols, dtype=torch.float32, device=tok_emb.device)
    z = torch.empty_like(y)
    _check(load().emcid_embed_layernorm_f32(_ptr(tok_emb, torch.float32, "tok_emb"), tok_emb.stride(0), tok_emb.shape[0],
                                            _ptr(pos_emb, torch.float32, "pos_emb"), pos_emb.stride(0), pos_emb.shape[0],
                                            _ptr(token, torch.int64, "token"), _ptr(position, torch.int32, "position"),
                                            _ptr(ln.weight, torch.float32, "gamma"), _ptr(ln.bias, torch.float32, "beta"),
                                            float(ln.eps), rows, cols, _ptr(y), _ptr(z), _stream(tok_emb)),
           "emcid_embed_layernorm_f32")
    return y, z


def tree_attention(q, k, v, anc, depth, H: int, scale=None, rows=None):
    """k/v (U, H*D) fp32 row views sharing one leading dimension; q (n, H*D) in query order; anc (U, S) int32;
    depth (U,) int32; rows: optional (n,) int32 query nodes (None: all U nodes, q has U rows).  Returns (n, H*D)."""
    U, HD = k.shape
    D = HD // H
    for t in (q, k, v):
        if t.stride(1) != 1 or t.shape[1] != HD:
            raise EmcidHipError("tree_attention: q/k/v must be row-major")
    if k.stride(0) != v.stride(0):
        raise EmcidHipError("tree_attention: k and v must share a leading dimension")
    n = U if rows is None else rows.numel()
    if q.shape[0] != n:
        raise EmcidHipError(f"tree_attention: {q.shape[0]} query rows for {n} query nodes")
    out = torch.empty(n, HD, dtype=torch.float32, device=q.device)
    scale = float(D ** -0.5 if scale is None else scale)
    _check(load().emcid_tree_attention_f32(
        _ptr(q, torch.float32, "q"), q.stride(0), _ptr(k, torch.float32, "k"), _ptr(v, torch.float32, "v"), k.stride(0),
        _ptr(anc, torch.int32, "anc"), anc.stride(0), _ptr(depth, torch.int32, "depth"),
        _ptr(rows, torch.int32, "rows") if rows is not None else None, n, H, D, scale, _ptr(out), out.stride(0),
        _stream(q)), "emcid_tree_attention_f32")
    return out


# ---- native layer runner of the trie forward (csrc/clip_layers.hip) -----------------------------------------------------------

class ClipLayerSp16(C.Structure):
    """include/emcid_hip.h: emcid_clip_layer_sp16."""
    _fields_ = [(n, C.c_void_p) for n in (
        "ln1_gamma", "ln1_beta", "ln2_gamma", "ln2_beta", "qkv_planes", "qkv_inv_scale", "qkv_bias", "out_planes",
        "out_inv_scale", "out_bias", "fc1_planes", "fc1_inv_scale", "fc1_bias", "fc1_bound", "fc2_planes", "fc2_inv_scale",
        "fc2_bias")] + [("ln1_eps", C.c_float), ("ln2_eps", C.c_float), ("act", C.c_int32), ("reserved", C.c_int32)]


_CLIP_WS = {}       # (device index, stream handle, rows, h, d) -> workspace of the layer runner


def clip_workspace(dev: torch.device, rows: int, h: int, d: int) -> torch.Tensor:
    """Launches of one stream run one after the other and may share the runner's scratch buffers."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream,
           rows, h, d)
    ws = _CLIP_WS.get(key)
    if ws is None:
        if len(_CLIP_WS) >= 16:
            _CLIP_WS.clear()
        ws = _CLIP_WS[key] = torch.empty(int(load().emcid_clip_workspace_bytes(rows, h, d)), dtype=torch.uint8, device=dev)
    return ws


def clip_layers(layer_array, first: int, count: int, rows: int, h: int, d: int, heads: int, scale: float, anc: torch.Tensor,
                depth: torch.Tensor, hs: torch.Tensor, x: "SplitRows", next_ln: Optional[torch.nn.LayerNorm]):
    """``count`` whole layers starting at ``layer_array[first]`` on every trie node, in place on ``hs`` (rows, h) and on the
    planes of ``x`` (LN1 of hs in, the next layer's LN1 of the result out when ``next_ln`` is given)."""
    ws = clip_workspace(hs.device, rows, h, d)
    if LINEAR_FLOPS["count"]:
        LINEAR_FLOPS["flops"] += count * 2.0 * rows * h * (4 * h + 2 * d)
        LINEAR_FLOPS["launches"] += 4 * count
    base = C.addressof(layer_array) + first * C.sizeof(ClipLayerSp16)
    g = _ptr(next_ln.weight, torch.float32, "gamma") if next_ln is not None else None
    b = _ptr(next_ln.bias, torch.float32, "beta") if next_ln is not None else None
    _check(load().emcid_clip_layers_sp16(C.c_void_p(base), count, rows, h, d, heads, float(scale), _ptr(anc, torch.int32, "anc"),
                                         anc.stride(0), _ptr(depth, torch.int32, "depth"), _ptr(hs, torch.float32, "hs"),
                                         _ptr(x.planes), _ptr(x.inv_scale), g, b, float(next_ln.eps) if next_ln is not None else 0.0,
                                         C.c_void_p(ws.data_ptr()), ws.numel(), _stream(hs)), "emcid_clip_layers_sp16")


def clip_layer_head(layer_array, index: int, rows: int, h: int, d: int, heads: int, scale: float, anc: torch.Tensor,
                    depth: torch.Tensor, rows_sel: Optional[torch.Tensor], hs: torch.Tensor, x: "SplitRows", want_f32: bool):
    """Attention block + fc1 of layer ``layer_array[index]``: returns (mid (n, h), SplitRows of fc2's input (n, d) [with its
    fp32 twin when ``want_f32``]); n = every node, or the ``rows_sel`` query nodes."""
    dev = hs.device
    n = rows if rows_sel is None else rows_sel.numel()
    ws = clip_workspace(dev, rows, h, d)
    mid = torch.empty(n, h, dtype=torch.float32, device=dev)
    f_planes = torch.empty(n, d, dtype=torch.int32, device=dev)
    f_scale = torch.empty(2, n, dtype=torch.float32, device=dev)
    f_f32 = torch.empty(n, d, dtype=torch.float32, device=dev) if want_f32 else None
    if LINEAR_FLOPS["count"]:
        LINEAR_FLOPS["flops"] += 2.0 * h * (rows * (3 * h if rows_sel is None else 2 * h) + n * (h if rows_sel is not None else 0)
                                            + n * h + n * d)
        LINEAR_FLOPS["launches"] += 3 if rows_sel is None else 4
    base = C.addressof(layer_array) + index * C.sizeof(ClipLayerSp16)
    _check(load().emcid_clip_layer_head_sp16(
        C.c_void_p(base), rows, h, d, heads, float(scale), _ptr(anc, torch.int32, "anc"), anc.stride(0),
        _ptr(depth, torch.int32, "depth"), _ptr(rows_sel, torch.int32, "rows") if rows_sel is not None else None, n,
        _ptr(hs, torch.float32, "hs"), _ptr(x.planes), _ptr(x.inv_scale), _ptr(mid), _ptr(f_planes), _ptr(f_scale), _ptr(f_f32),
        C.c_void_p(ws.data_ptr()), ws.numel(), _stream(hs)), "emcid_clip_layer_head_sp16")
    return mid, SplitRows(f_planes, f_scale[1], f_f32)


def clip_layer_tail(layer_array, index: int, h: int, d: int, f: "SplitRows", mid: torch.Tensor,
                    next_ln: Optional[torch.nn.LayerNorm]):
    """fc2 + residual add of layer ``layer_array[index]`` and the next layer's LN1 as planes: (hs (n, h), SplitRows | None)."""
    dev = mid.device
    n = mid.shape[0]
    hs = torch.empty(n, h, dtype=torch.float32, device=dev)
    x = None
    if next_ln is not None:
        x = SplitRows(torch.empty(n, h, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    if LINEAR_FLOPS["count"]:
        LINEAR_FLOPS["flops"] += 2.0 * n * h * d
        LINEAR_FLOPS["launches"] += 1
    base = C.addressof(layer_array) + index * C.sizeof(ClipLayerSp16)
    _check(load().emcid_clip_layer_tail_sp16(
        C.c_void_p(base), n, h, d, _ptr(f.planes), _ptr(f.inv_scale), _ptr(mid, torch.float32, "mid"), _ptr(hs),
        _ptr(next_ln.weight, torch.float32, "gamma") if next_ln is not None else None,
        _ptr(next_ln.bias, torch.float32, "beta") if next_ln is not None else None,
        float(next_ln.eps) if next_ln is not None else 0.0, _ptr(x.planes) if x is not None else None,
        _ptr(x.inv_scale) if x is not None else None, _stream(mid)), "emcid_clip_layer_tail_sp16")
    return hs, x


def clip_edit_layer_tail(layer_array, index: int, h: int, d: int, f: "SplitRows", mid: torch.Tensor, lookup: torch.Tensor,
                         seg: torch.Tensor, zs_t: torch.Tensor, factors: "CovFactors", layer_index: int, edit_weight: float,
                         layers_left: int, W0: torch.Tensor, W: torch.Tensor, ws: "DualWorkspace", lam: Optional[float],
                         next_ln: Optional[torch.nn.LayerNorm], last: bool, want_dw: bool = True, zc_split: bool = True):
    """The rest of an edited layer behind ``clip_layer_head`` in ONE C call: keys, Zc, the apply-only dual solve (W = W0 + dW), the
    new weight's planes and — unless ``last`` — fc2 + residual + the next layer's LN1.  Returns dict(K, Zc, dW, hs, x)."""
    dev = mid.device
    n = f.f32.shape[0]
    N = seg.numel() - 1
    K = torch.empty(N, d, dtype=torch.float32, device=dev)
    Zc = torch.empty(N, h, dtype=torch.float32, device=dev)
    dW = torch.empty(h, d, dtype=torch.float32, device=dev) if want_dw else None
    # Zc = fc2(keys) on the split-fp16 kernel against the layer's own fc2 planes (scratch for the keys' planes): the caller
    # says so with zc_split — the planes in ``layer_array`` must then be those of W as it is now
    kp = torch.empty(N, d, dtype=torch.int32, device=dev) if zc_split else None
    ks = torch.empty(N, dtype=torch.float32, device=dev) if zc_split else None
    hs = x = None
    if not last:
        hs = torch.empty(n, h, dtype=torch.float32, device=dev)
        if next_ln is not None:
            x = SplitRows(torch.empty(n, h, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    lws = _linear_workspace(dev) if (d >= 2048 and -(-N // 128) * -(-h // 128) <= 128
                                     and not torch.cuda.is_current_stream_capturing()) else None
    if LINEAR_FLOPS["count"]:
        LINEAR_FLOPS["flops"] += 2.0 * N * h * d + (0.0 if last else 2.0 * n * h * d)
        LINEAR_FLOPS["launches"] += 1 if last else 2
    base = C.addressof(layer_array) + index * C.sizeof(ClipLayerSp16)
    use_inverse = layer_index in factors.have_inverse
    _check(load().emcid_clip_edit_layer_tail_sp16(
        C.c_void_p(base), n, h, d, _ptr(f.f32, torch.float32, "fc2 input"), _ptr(f.planes), _ptr(f.inv_scale),
        _ptr(mid, torch.float32, "mid"), _ptr(lookup, torch.int64, "lookup"), _ptr(seg, torch.int64, "seg"), lookup.numel(), N,
        _ptr(zs_t, torch.float32, "zs_t"), float(edit_weight), int(layers_left), factors.lam_ratio(lam), _ptr(factors.buf),
        factors.n_layers, int(layer_index), int(bool(use_inverse)), _ptr(W0, torch.float32, "W0"), _ptr(W, torch.float32, "W"),
        _ptr(dW), _ptr(K), _ptr(Zc), _ptr(kp), _ptr(ks), _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32),
        C.c_void_p(lws.data_ptr()) if lws is not None else None, lws.numel() if lws is not None else 0, _ptr(hs),
        _ptr(next_ln.weight, torch.float32, "gamma") if (next_ln is not None and not last) else None,
        _ptr(next_ln.bias, torch.float32, "beta") if (next_ln is not None and not last) else None,
        float(next_ln.eps) if (next_ln is not None and not last) else 0.0, _ptr(x.planes) if x is not None else None,
        _ptr(x.inv_scale) if x is not None else None, _stream(mid)), "emcid_clip_edit_layer_tail_sp16")
    return {"K": K, "Zc": Zc, "dW": dW, "hs": hs, "x": x}


# ---- dual (Woodbury) solver ---------------------------------------------------------------------------------------------

class CovFactors:
    """Cholesky factors of M_l = lam * C'_l for every edited layer (batched factorization, one workspace)."""

    def __init__(self, n_layers: int, d: int, device):
        self.n_layers, self.d = n_layers, d
        self.nbytes = int(load().emcid_cov_factor_workspace_bytes(n_layers, d))
        self.buf = torch.zeros(self.nbytes // 8, dtype=torch.float64, device=device)
        self.info = torch.zeros(1, dtype=torch.int32, device=device)
        self.dp = (d + NB - 1) // NB * NB
        self._inv = ((self.dp + 511) // 512) * (512 * 512 + 256 * 256)   # csrc/common.h inv_doubles
        self.have_inverse = set()                                        # layers whose X = inv(L) has been built
        self.ready = None       # HIP event after the last kernel that wrote this workspace on another stream (or None)
        self.cached = False     # True once the edit engine shares it between edits (then it is read-only)
        self.lam = None         # the lam the workspace was factored with (factor_cov); edits with another lam pass the ratio
        self.edit_weight = None

    def lam_ratio(self, lam: Optional[float]) -> float:
        """lam of an edit / the lam of the factorization: the gain the dual stages fold into Kt64 and Rt
        (include/emcid_hip.h, "lam_ratio")."""
        if lam is None or self.lam is None or float(lam) == self.lam:
            return 1.0
        if not (lam > 0.0 and self.lam > 0.0):
            raise EmcidHipError(f"mom2_update_weight must be positive for the Cholesky path (got {lam})")
        return float(lam) / float(self.lam)

    def L(self, layer: int) -> torch.Tensor:
        """(dp, dp) view of the Cholesky factor of lam*C'_layer (lower triangle valid)."""
        o = (self.n_layers + layer) * self.dp * self.dp
        return self.buf[o:o + self.dp * self.dp].view(self.dp, self.dp)

    def X(self, layer: int) -> torch.Tensor:
        """(dp, dp) view of inv(L_layer), explicit (lower triangle valid; nothing above it is ever read)."""
        o = self.n_layers * (2 * self.dp * self.dp + self._inv) + layer * self.dp * self.dp
        return self.buf[o:o + self.dp * self.dp].view(self.dp, self.dp)


def cov_inverse(factors: "CovFactors", first: int = 0, count: Optional[int] = None):
    """Build X = inv(L) for layers [first, first + count) of a factored workspace (default: all), batched.
    Asynchronous on the current stream; needs factor_cov earlier on it."""
    count = factors.n_layers - first if count is None else count
    _check(load().emcid_cov_inverse_f64(_ptr(factors.buf), factors.n_layers, factors.d, int(first), int(count),
                                        _stream(factors.buf)), "emcid_cov_inverse_f64")
    factors.have_inverse.update(range(first, first + count))


def factor_cov(covs, lam: float, edit_weight: float, factors: Optional[CovFactors] = None, inverse: bool = True) -> CovFactors:
    """covs: list of (d, d) fp32 contiguous HBM tensors (one per edited layer, forward order).  Asynchronous on the
    current stream.  ``inverse=False`` leaves the explicit inverse factors to per-layer ``cov_inverse`` calls."""
    d = covs[0].shape[0]
    for c in covs:
        assert c.shape == (d, d) and c.is_contiguous()
    if factors is None or factors.n_layers != len(covs) or factors.d != d:
        factors = CovFactors(len(covs), d, covs[0].device)
    arr = (C.c_void_p * len(covs))(*[_ptr(c, torch.float32, "C").value for c in covs])
    _check(load().emcid_factor_cov_f64(arr, len(covs), d, float(lam), float(edit_weight), _ptr(factors.buf), factors.nbytes,
                                       _ptr(factors.info, torch.int32), _stream(covs[0])), "emcid_factor_cov_f64")
    factors.have_inverse = set()
    factors.lam, factors.edit_weight = float(lam), float(edit_weight)
    if inverse:
        cov_inverse(factors)
    return factors


def cov_factor_rescale(src: CovFactors, a: float, dst: Optional[CovFactors] = None, lam: Optional[float] = None,
                       edit_weight: Optional[float] = None) -> CovFactors:
    """``dst`` (default: a new workspace; ``dst is src``: in place) = the factors of a * M for the M that ``src`` holds:
    sqrt(a) L, inverse factors / sqrt(a).  With ``src`` factored at unit scale (``factor_cov(covs, 1.0, 0.5)``: M = C) and
    a = 2 lam (1 - edit_weight), ``dst`` is the workspace of that pair; ``lam`` / ``edit_weight`` are recorded on it.
    Asynchronous on the current stream."""
    if not (a > 0.0 and a < 1e300):
        raise EmcidHipError(f"the scale of a factored workspace must be positive and finite (got {a})")
    with_inverse = len(src.have_inverse) == src.n_layers
    if dst is None or dst.n_layers != src.n_layers or dst.d != src.d or dst.buf.device != src.buf.device:
        dst = CovFactors(src.n_layers, src.d, src.buf.device)
    if dst is not src:
        dst.info.zero_()          # (a reused workspace starts every point with a clean flag word)
    _check(load().emcid_cov_factor_rescale_f64(_ptr(src.buf), _ptr(dst.buf), dst.nbytes, src.n_layers, src.d, float(a),
                                               int(with_inverse), _stream(src.buf)), "emcid_cov_factor_rescale_f64")
    dst.have_inverse = set(range(src.n_layers)) if with_inverse else set()
    dst.lam = float(lam) if lam is not None else (src.lam * float(a) if src.lam is not None else None)
    dst.edit_weight = float(edit_weight) if edit_weight is not None else src.edit_weight
    return dst


class DualWorkspace:
    def __init__(self, N: int, d: int, h: int, device):
        self.key = (N, d, h)
        self.nbytes = int(load().emcid_edit_dual_workspace_bytes(N, d, h))
        self.buf = torch.zeros(self.nbytes // 8, dtype=torch.float64, device=device)     # zero: the stream-K ticket counters
        self.info = torch.zeros(1, dtype=torch.int32, device=device)
        self.Np, self.dp = (N + NB - 1) // NB * NB, (d + NB - 1) // NB * NB
        pt = load().emcid_edit_dual_pt(_ptr(self.buf), N, d, h)
        off = (pt - self.buf.data_ptr()) // 8
        self.Pt = self.buf[off:off + self.Np * self.dp].view(self.Np, self.dp)   # the Pt stack, rows = concepts
        hp = h + (h % 2)
        off = (load().emcid_edit_dual_s(_ptr(self.buf), N, d, h) - self.buf.data_ptr()) // 8
        self.S = self.buf[off:off + self.Np * self.Np].view(self.Np, self.Np)    # N x N system (column-sharded form: partial sums)
        off = (load().emcid_edit_dual_u(_ptr(self.buf), N, d, h) - self.buf.data_ptr()) // 8
        self.U = self.buf[off:off + hp * self.dp].view(hp, self.dp)[:h]          # U (h, dp) f64 partial sums of the same form
        # the other blocks of the chain (emcid_edit_dual_block; what each holds after which stage: include/emcid_hip.h)
        self.hp = hp
        Np, dp = self.Np, self.dp
        self.Kt, self.Yt = self.block("K").view(Np, dp), self.block("Y").view(Np, dp)
        self.Rt = self.block("R").view(Np, hp)
        self.LS, self.XT = self.block("LS").view(Np, Np), self.block("XT").view(Np, Np)
        self.RT = self.block("PT").view(dp, Np)              # rows < h: Z^T (apply-only form); adj_k^T padded (adj_k form)
        self.V = self.block("V").view(hp, dp)[:h]
        self.sk_counters = self.block("SK_COUNTERS")         # every stream-K launch leaves them zero

    def block(self, name: str) -> torch.Tensor:
        """Flat f64 view of one block of the workspace (DUAL_BLOCKS)."""
        n = C.c_int64(0)
        at = load().emcid_edit_dual_block(_ptr(self.buf), *self.key, DUAL_BLOCKS.index(name), C.byref(n))
        if not at or n.value < 0:
            raise EmcidHipError(f"no block {name!r} in a dual workspace")
        off = (at - self.buf.data_ptr()) // 8
        return self.buf[off:off + n.value]

    def schur_form(self) -> str:
        """How stage 2 of the apply-only form will solve Z = S^-1 Rt here (SCHUR_FORMS)."""
        return SCHUR_FORMS[load().emcid_edit_dual_schur_form(*self.key)]


def full_inverse(L: torch.Tensor, inv: torch.Tensor, scratch: torch.Tensor):
    """Test hook: X = inv(L) (lower triangle) from ``cholesky``'s factor and inverse workspace; ``scratch``: f64,
    at least emcid_full_inverse_scratch_doubles(dp, ld) elements."""
    X = torch.zeros_like(L)
    _check(load().emcid_full_inverse_f64(_ptr(L, torch.float64), L.shape[0], L.stride(0), _ptr(inv), _ptr(X), _ptr(scratch),
                                         scratch.numel(), _stream(L)), "emcid_full_inverse_f64")
    return X


def edit_layer_dual(K, Zc, zs_t, factors: CovFactors, layer_index: int, edit_weight: float, layers_left: int,
                    W0=None, W=None, want_factors: bool = False, want_dw: bool = True, ws: Optional[DualWorkspace] = None,
                    rows=None, gather_pt=None, use_inverse: Optional[bool] = None, lam: Optional[float] = None):
    """One edited layer through the dual solver.  ``lam``: this edit's mom2_update_weight when it differs from the one
    ``factors`` was built with (None: the same).  ``rows=(lo, hi)`` + ``gather_pt(Pt_rows) -> all rows`` split the
    M-solves over ranks.  ``use_inverse``: solve against M with GEMMs on X = inv(L) (default: if cov_inverse built it)
    or by block substitution with L.  Returns dict(adj_k (d,N) | None, Rt (N,h) | None, dW, ws)."""
    if use_inverse is None:
        use_inverse = layer_index in factors.have_inverse
    N, d = K.shape
    h = Zc.shape[1]
    for t, nm in ((K, "K"), (Zc, "Zc"), (zs_t, "zs_t")):
        assert t.is_contiguous(), nm
    assert zs_t.shape == (N, h) and factors.d == d
    if ws is None or ws.key != (N, d, h):
        ws = DualWorkspace(N, d, h, K.device)
    lo, hi = rows if rows is not None else (0, N)
    lib = load()
    _check(lib.emcid_edit_dual_stage1_f64(
        _ptr(K, torch.float32, "K"), _ptr(Zc, torch.float32, "Zc"), _ptr(zs_t, torch.float32, "zs_t"), N, d, h,
        float(edit_weight), int(layers_left), factors.lam_ratio(lam), _ptr(factors.buf), factors.n_layers, int(layer_index), lo, hi,
        int(bool(use_inverse)), _ptr(ws.buf), ws.nbytes, _stream(K)), "emcid_edit_dual_stage1_f64")
    if gather_pt is not None:
        ws.Pt[:N].copy_(gather_pt(ws.Pt[lo:hi]))
    dev = K.device
    adj_k = torch.empty(d, N, dtype=torch.float64, device=dev) if want_factors else None
    Rt = torch.empty(N, h, dtype=torch.float64, device=dev) if want_factors else None
    dW = torch.empty(h, d, dtype=torch.float32, device=dev) if want_dw else None
    if W is not None:
        assert W.is_contiguous() and W.shape == (h, d) and W0 is not None and W0.is_contiguous()
    _check(lib.emcid_edit_dual_stage2_f64(N, d, h, factors.lam_ratio(lam), _ptr(W0, torch.float32, "W0"), _ptr(W, torch.float32, "W"), _ptr(adj_k),
                                          _ptr(Rt), _ptr(dW), _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32),
                                          _stream(K)), "emcid_edit_dual_stage2_f64")
    return {"adj_k": adj_k, "Rt": Rt, "dW": dW, "ws": ws}


def column_tiles(rank: int, world: int, n_tiles: int):
    """This rank's 128-wide column tiles of the d dimension for the column-sharded solve.  Tile t of the triangular factor
    costs ~(t + 1) (its contraction depth), so the tiles are dealt heaviest first, each to the least loaded rank so far
    (ties: lowest rank) — the same table on every rank, per-rank cost within a few percent of the mean (24 tiles over 8
    ranks: 36..39 of a mean 37.5)."""
    load_ = [0] * world
    owner = {}
    for t in range(n_tiles - 1, -1, -1):
        r = min(range(world), key=lambda i: (load_[i], i))
        owner[t] = r
        load_[r] += t + 1
    return [t for t in range(n_tiles) if owner[t] == rank]


class _HipColsBackend:
    """The two stages of the column-sharded solve on the C library (include/emcid_hip.h)."""

    def __init__(self, K, Zc, zs_t, factors, layer_index, edit_weight, layers_left, ws, lam=None):
        self.a = (K, Zc, zs_t, factors, layer_index, edit_weight, layers_left, ws)
        self.lam_ratio = factors.lam_ratio(lam)

    def stage1(self, tiles):
        K, Zc, zs_t, factors, layer_index, edit_weight, layers_left, ws = self.a
        N, d = K.shape
        arr = (C.c_int * len(tiles))(*tiles)
        _check(load().emcid_edit_dual_cols_stage1_f64(
            _ptr(K, torch.float32, "K"), _ptr(Zc, torch.float32, "Zc"), _ptr(zs_t, torch.float32, "zs_t"), N, d, Zc.shape[1],
            float(edit_weight), int(layers_left), self.lam_ratio, _ptr(factors.buf), factors.n_layers, int(layer_index), arr,
            len(tiles), _ptr(ws.buf), ws.nbytes, _stream(K)), "emcid_edit_dual_cols_stage1_f64")
        return ws.S

    def stage2(self, tiles):
        K, Zc, zs_t, factors, layer_index, edit_weight, layers_left, ws = self.a
        N, d = K.shape
        arr = (C.c_int * len(tiles))(*tiles)
        _check(load().emcid_edit_dual_cols_stage2_f64(N, d, Zc.shape[1], _ptr(factors.buf), factors.n_layers, int(layer_index), arr,
                                                      len(tiles), _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32), _stream(K)),
               "emcid_edit_dual_cols_stage2_f64")
        return ws.U

    def apply(self, U, W0, W, want_dw):
        K, Zc = self.a[0], self.a[1]
        h, d = Zc.shape[1], K.shape[1]
        dW = torch.empty(h, d, dtype=torch.float32, device=K.device) if want_dw else None
        _check(load().emcid_apply_update2d_f32(_ptr(U), U.stride(0), _ptr(W0, torch.float32, "W0"), _ptr(W, torch.float32, "W"),
                                               _ptr(dW), h, d, _stream(K)), "emcid_apply_update2d_f32")
        return dW


def edit_layer_dual_cols(K, Zc, zs_t, factors, layer_index: int, edit_weight: float, layers_left: int, W0, W,
                         tiles, all_reduce, want_dw: bool = True, ws: Optional["DualWorkspace"] = None, backend=None,
                         lam: Optional[float] = None):
    """Apply-only dual solver with the layer's GEMMs split over ranks by column tiles of d (include/emcid_hip.h,
    "COLUMN-SHARDED").  ``tiles``: this rank's tile indices (column_tiles); ``all_reduce(t)``: sums a tensor over the
    ranks in place (two calls: the N x N partial S, the h x dp partial U).  Needs the layer's explicit inverse factor.
    ``backend``: object with stage1/stage2/apply (default: the C library; tests/test_dist_cpu.py passes a torch-CPU
    restatement of the two stages to run this very skeleton under gloo)."""
    N, d = K.shape
    h = Zc.shape[1]
    tiles = sorted(int(t) for t in tiles)
    if not tiles:
        raise EmcidHipError("a rank without a column tile: world size exceeds d / 128")
    if backend is None:
        for t, nm in ((K, "K"), (Zc, "Zc"), (zs_t, "zs_t"), (W, "W"), (W0, "W0")):
            assert t.is_contiguous(), nm
        assert zs_t.shape == (N, h) and factors.d == d and W.shape == (h, d)
        if layer_index not in factors.have_inverse:
            raise EmcidHipError("edit_layer_dual_cols needs the explicit inverse factor of the layer (cov_inverse)")
        if ws is None or ws.key != (N, d, h):
            ws = DualWorkspace(N, d, h, K.device)
        backend = _HipColsBackend(K, Zc, zs_t, factors, layer_index, edit_weight, layers_left, ws, lam)
    S = backend.stage1(tiles)            # partial S_r = Yc Yc^T (no identity)
    all_reduce(S)
    U = backend.stage2(tiles)            # partial U_r = (Z^T Yc) X[tiles, :]
    all_reduce(U)
    dW = backend.apply(U, W0, W, want_dw)
    return {"dW": dW, "ws": ws}


def edit_layer_dual_apply(K, Zc, zs_t, factors: CovFactors, layer_index: int, edit_weight: float, layers_left: int,
                          W0, W, want_dw: bool = True, ws: Optional[DualWorkspace] = None,
                          use_inverse: Optional[bool] = None, on_factor_start=None, lam: Optional[float] = None):
    """Apply-only dual solver: W = W0 + float(U) without ever forming adj_k.  ``on_factor_start()``: called (host side)
    right after S = I + Yt Yt^T has been enqueued, i.e. the stream position where the latency-bound Cholesky of S
    begins.  Returns dict(dW, ws)."""
    if use_inverse is None:
        use_inverse = layer_index in factors.have_inverse
    N, d = K.shape
    h = Zc.shape[1]
    for t, nm in ((K, "K"), (Zc, "Zc"), (zs_t, "zs_t"), (W, "W"), (W0, "W0")):
        assert t.is_contiguous(), nm
    assert zs_t.shape == (N, h) and factors.d == d and W.shape == (h, d)
    if ws is None or ws.key != (N, d, h):
        ws = DualWorkspace(N, d, h, K.device)
    lib = load()
    _check(lib.emcid_edit_dual_apply_stage1_f64(
        _ptr(K, torch.float32, "K"), _ptr(Zc, torch.float32, "Zc"), _ptr(zs_t, torch.float32, "zs_t"), N, d, h,
        float(edit_weight), int(layers_left), factors.lam_ratio(lam), _ptr(factors.buf), factors.n_layers, int(layer_index), 0, N,
        int(bool(use_inverse)), _ptr(ws.buf), ws.nbytes, _stream(K)), "emcid_edit_dual_apply_stage1_f64")
    dW = torch.empty(h, d, dtype=torch.float32, device=K.device) if want_dw else None
    if on_factor_start is not None:
        _check(lib.emcid_edit_dual_apply_assemble_f64(N, d, h, _ptr(ws.buf), ws.nbytes, _stream(K)),
               "emcid_edit_dual_apply_assemble_f64")
        on_factor_start()
    _check(lib.emcid_edit_dual_apply_stage2_f64(N, d, h, _ptr(factors.buf), factors.n_layers, int(layer_index),
                                                int(bool(use_inverse)), int(on_factor_start is not None),
                                                _ptr(W0, torch.float32, "W0"), _ptr(W, torch.float32, "W"), _ptr(dW),
                                                _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32), _stream(K)),
           "emcid_edit_dual_apply_stage2_f64")
    return {"dW": dW, "ws": ws}


def check_preserved_state(sd, n_layers: int, d: int, capacity: int) -> int:
    """Would a state of ``n_layers`` layers of width ``d`` at ``capacity`` take ``sd`` (a ``PreservedKeys.state_dict()``)?  Returns
    its M; ``EmcidHipError`` otherwise, naming what does not fit.  Pure host code: only shapes and dtypes are looked at."""
    def bad(what):
        return EmcidHipError(f"preserved key state: {what}")

    if not isinstance(sd, dict):
        raise bad(f"a dict is expected (got {type(sd).__name__})")
    missing = [k for k in ("M", "d", "n_layers", "Yp", "Lp", "tile_inv", "row_scale") if k not in sd]
    if missing:
        raise bad(f"no entry {missing}")
    M = sd["M"]
    if isinstance(M, bool) or not isinstance(M, int) or M < 0:
        raise bad(f"M must be a non-negative integer (got {M!r})")
    if sd["d"] != d:
        raise bad(f"its rows are of width d = {sd['d']}, this state's of d = {d}")
    if sd["n_layers"] != n_layers:
        raise bad(f"it holds {sd['n_layers']} layers, this state {n_layers}")
    if M > capacity:
        raise bad(f"its M = {M} committed rows exceed this state's capacity {capacity}")
    tiles = (M + NB - 1) // NB
    for name, shape in (("Yp", (M, d)), ("Lp", (M, M)), ("tile_inv", (tiles, NB, NB))):
        ts = sd[name]
        if not isinstance(ts, (list, tuple)) or len(ts) != n_layers:
            raise bad(f"{name} must be a list of {n_layers} tensors")
        for i, t in enumerate(ts):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != shape:
                got = (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__
                raise bad(f"{name}[{i}] must be an f64 tensor of {shape} for M = {M}, d = {d} (got {got})")
    rs = sd["row_scale"]
    if not isinstance(rs, torch.Tensor) or rs.dtype != torch.float64 or tuple(rs.shape) != (M,):
        raise bad(f"row_scale must be an f64 tensor of ({M},)")
    return M


class PreservedKeys:
    """The session state of the dual solver for ``n_layers`` edited layers (include/emcid_hip.h, "PRESERVED key set"): per layer
    Yp (capacity, dp), Lp (capacity, capacity) and the inverses of Lp's diagonal 128-tiles, f64 in HBM, allocated once —
    capacity * dp + capacity^2 doubles per layer plus the tiles.  ``M`` rows of every layer are committed; ``edit_layer_dual_preserve``
    (an edit's rows) and ``session_retain`` (a retain list's) write rows behind them and ``commit(N, scale)`` makes them count.
    ``row_scale`` (capacity,) f64 on the host: the factor each committed row's raw key was multiplied by on its way in
    (sqrt(edit_weight / 0.5) / sqrt(lam_ratio) for an edited key, with the retain weight under the first root for a retained one) —
    what takes a norm in the solve's units back to raw-key units (``session_step_norms``); the same for every layer."""

    def __init__(self, n_layers: int, d: int, capacity: int, device):
        if capacity < 1:
            raise EmcidHipError(f"the capacity of a preserved key set must be positive (got {capacity})")
        self.n_layers, self.d, self.capacity, self.M = int(n_layers), int(d), int(capacity), 0
        self.dp = (d + NB - 1) // NB * NB
        self.ldl = self.capacity + (self.capacity % 2)
        tiles = (self.capacity + NB - 1) // NB
        self.Yp = [torch.zeros(self.capacity, self.dp, dtype=torch.float64, device=device) for _ in range(n_layers)]
        self.Lp = [torch.zeros(self.capacity, self.ldl, dtype=torch.float64, device=device) for _ in range(n_layers)]
        self.tile_inv = [torch.zeros(tiles, NB, NB, dtype=torch.float64, device=device) for _ in range(n_layers)]
        self.row_scale = torch.ones(self.capacity, dtype=torch.float64)

    def commit(self, N: int, scale: float = 1.0):
        assert self.M + N <= self.capacity
        self.row_scale[self.M:self.M + int(N)] = float(scale)
        self.M += int(N)

    def release_commit(self, keep):
        """Make the rows ``keep`` (ascending indices < M) the committed set, after ``session_release`` has run on every layer and
        the flag word read zero: compacts the host ``row_scale`` vector and sets ``M``."""
        keep = check_keep(keep, self.M)[0]
        self.row_scale[:len(keep)] = self.row_scale[torch.as_tensor(keep, dtype=torch.long)]
        self.M = len(keep)

    def rescale_commit(self, factors):
        """Make the committed rows count as scaled by ``factors`` (one positive finite number, or one per committed row), after
        ``session_rescale`` has run on every layer and the flag word read zero: multiplies the host ``row_scale`` vector.  The
        factors are those of the UNITS a later ``session_step_norms`` reports in; they are the device factors whenever the
        coordinates' factor workspace stays what it was (``check_factors`` refuses the rest)."""
        f = check_factors(factors, self.M)
        self.row_scale[:self.M] *= f

    def reset(self):
        self.M = 0

    def snapshot(self, first: int, end: int) -> "KeySnapshot":
        return KeySnapshot(self, first, end)

    def state_dict(self, sync: bool = True) -> dict:
        """The committed part, on the host, in a form that knows nothing of ``capacity`` (so of ``ldl`` and the tile count): per
        layer ``Yp`` (M, d) — the padding columns are zero by construction —, ``Lp`` (M, M) and ``tile_inv`` (ceil(M / 128), 128,
        128), the inverses of the diagonal tiles that rows < M touch, the last one zero outside the rows and columns below M (the
        leading block of a lower-triangular inverse is the inverse of the leading block); ``row_scale`` (M,); ``M``, ``d``,
        ``n_layers``.  What ``load_state_dict`` of a state of ANY capacity >= M takes.  The state is not changed.  From HBM the
        copies go to page-locked memory on the current stream, followed by ONE synchronisation; ``sync=False`` leaves that to
        the caller (the tensors are not to be read before)."""
        M, d, tiles = self.M, self.d, (self.M + NB - 1) // NB
        w = M - NB * (tiles - 1)                    # rows of the last tile that count

        def host(t: torch.Tensor) -> torch.Tensor:
            return pinned_copy(t) if t.is_cuda else t.clone()

        def tile_part(ti: torch.Tensor) -> torch.Tensor:
            ti = ti[:tiles].clone()
            if tiles and w < NB:
                ti[-1, w:, :] = 0
                ti[-1, :, w:] = 0
            return ti

        sd = {"M": M, "d": d, "n_layers": self.n_layers,
              "Yp": [host(y[:M, :d].contiguous()) for y in self.Yp],
              "Lp": [host(l[:M, :M].contiguous()) for l in self.Lp],
              "tile_inv": [host(tile_part(t)) for t in self.tile_inv],
              "row_scale": self.row_scale[:M].clone()}
        if sync and self.Yp[0].is_cuda:
            torch.cuda.current_stream(self.Yp[0].device).synchronize()
        return sd

    def load_state_dict(self, sd: dict):
        """Make the rows of ``sd`` (a ``state_dict()``, of a state of any capacity) this state's committed set: checked on the host
        first (``check_preserved_state``: ``EmcidHipError`` for M > capacity, another d or layer count, a tensor of another shape
        or dtype — nothing is copied then), then every row and tile is copied to where THIS capacity's layout wants it.  What lies
        behind row M stays as it is: no entry of the library reads it before writing it."""
        M = check_preserved_state(sd, self.n_layers, self.d, self.capacity)
        tiles = (M + NB - 1) // NB
        for i in range(self.n_layers):
            self.Yp[i][:M, :self.d].copy_(sd["Yp"][i])
            self.Yp[i][:M, self.d:].zero_()
            self.Lp[i][:M, :M].copy_(sd["Lp"][i])
            self.tile_inv[i][:tiles].copy_(sd["tile_inv"][i])
        self.row_scale[:M] = sd["row_scale"]
        self.M = M

    def check_layer(self, layer_index: int):
        if not 0 <= layer_index < self.n_layers:
            raise EmcidHipError(f"layer index {layer_index} outside the session state's {self.n_layers} layers")

    def layer_args(self, layer_index: int):
        """Layer ``layer_index``'s part of the state as the session entries of the library take it: (Yp, ldy, Lp, ldl, tile_inv,
        capacity, M), the tensors as checked pointers into HBM.  Raises for a layer outside the state."""
        self.check_layer(layer_index)
        Yp, Lp, Ti = self.Yp[layer_index], self.Lp[layer_index], self.tile_inv[layer_index]
        for t, nm in ((Yp, "Yp"), (Lp, "Lp"), (Ti, "tile_inv")):
            assert t.stride(-1) == 1 and (t.dim() < 3 or t.is_contiguous()), nm
        return (_ptr(Yp, torch.float64, "Yp"), Yp.stride(0), _ptr(Lp, torch.float64, "Lp"), Lp.stride(0),
                _ptr(Ti, torch.float64, "tile_inv"), self.capacity, self.M)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * 8 for ts in (self.Yp, self.Lp, self.tile_inv) for t in ts)


class KeySnapshot:
    """Copies of rows [first, end) of every layer's Yp and Lp of a ``PreservedKeys``, of the tile inverses those rows touch (tiles
    [first // NB, ceil(end / NB))) and of the host ``row_scale`` of the committed rows; ``restore()`` copies all of it back to
    where it came from.  ``Yp[i]`` is layer i's copy, a contiguous (end - first, dp) tensor.  first == end holds nothing."""

    def __init__(self, state: PreservedKeys, first: int, end: int):
        self.state, self.rows = state, slice(first, end)
        self.tiles = slice(first // NB, (end + NB - 1) // NB if end > first else first // NB)
        self.Yp = [t[self.rows].clone() for t in state.Yp]
        self.Lp = [t[self.rows].clone() for t in state.Lp]
        self.tile_inv = [t[self.tiles].clone() for t in state.tile_inv]
        self.row_scale = state.row_scale[:state.M if end > first else 0].clone()

    def restore(self):
        s = self.state
        for kept, live, part in ((self.Yp, s.Yp, self.rows), (self.Lp, s.Lp, self.rows), (self.tile_inv, s.tile_inv, self.tiles)):
            for k, t in zip(kept, live):
                t[part].copy_(k)
        s.row_scale[:self.row_scale.numel()] = self.row_scale


class _SessionWorkspace:
    """HBM workspace (+ the device `info` word) of one session entry of the library: ``size_fn(*dims.values())`` bytes, ``key``
    the dimensions it was sized for; ``fitting``: ``ws`` if it was sized for ``dims``, else a new one of this class for them."""

    @classmethod
    def fitting(cls, ws, device, *dims):
        return ws if ws is not None and ws.key == dims else cls(*dims, device)

    def __init__(self, what: str, size_fn, dims: dict, device):
        self.key = tuple(dims.values())
        self.nbytes = int(size_fn(*self.key))
        if self.nbytes <= 0:
            raise EmcidHipError(f"no {what} workspace for " + ", ".join(f"{k}={v}" for k, v in dims.items()))
        self.buf = torch.zeros(self.nbytes // 8, dtype=torch.float64, device=device)     # zero: the stream-K ticket counters
        self.info = torch.zeros(1, dtype=torch.int32, device=device)


class PreserveWorkspace(_SessionWorkspace):
    """The workspace of emcid_edit_layer_dual_preserve_f64 for steps of N rows at a given capacity."""

    def __init__(self, N: int, d: int, h: int, capacity: int, device):
        super().__init__("preserve", load().emcid_edit_dual_preserve_workspace_bytes, dict(N=N, d=d, h=h, capacity=capacity), device)


class RetainWorkspace(_SessionWorkspace):
    """The workspace of emcid_session_retain_f64 for retain calls of N rows at a given capacity."""

    def __init__(self, N: int, d: int, capacity: int, device):
        super().__init__("retain", load().emcid_session_retain_workspace_bytes, dict(N=N, d=d, capacity=capacity), device)


class ReleaseWorkspace(_SessionWorkspace):
    """The workspace of emcid_session_release_f64 for a release that rebuilds ``n_rebuilt`` rows: the retain workspace of that N."""

    def __init__(self, n_rebuilt: int, d: int, capacity: int, device):
        super().__init__("release", load().emcid_session_release_workspace_bytes, dict(n_rebuilt=n_rebuilt, d=d, capacity=capacity),
                         device)


def edit_layer_dual_preserve(K, Zc, zs_t, factors: CovFactors, layer_index: int, edit_weight: float, layers_left: int,
                             W0, W, state: PreservedKeys, want_dw: bool = True, want_u: bool = False,
                             ws: Optional[PreserveWorkspace] = None, lam: Optional[float] = None):
    """``edit_layer_dual_apply`` with the keys of the earlier steps of ``state`` preserved: W = W0 + float(U) for
    A = lam C' + P^T P + Kt^T Kt.  The step's rows land behind ``state.M`` in layer ``layer_index``'s buffers; nothing is committed
    here (``state.commit(N)`` after the flag word ``ws.info`` read zero, for all layers together).  Needs the layer's explicit
    inverse factor.  Returns dict(dW, U (h, d) f64 | None, ws)."""
    N, d = K.shape
    h = Zc.shape[1]
    for t, nm in ((K, "K"), (Zc, "Zc"), (zs_t, "zs_t")) + (((W, "W"), (W0, "W0")) if W is not None else ()):
        assert t.is_contiguous(), nm
    assert zs_t.shape == (N, h) and factors.d == d == state.d and (W is None or W.shape == (h, d))
    state.check_layer(layer_index)
    if layer_index not in factors.have_inverse:
        raise EmcidHipError("edit_layer_dual_preserve needs the explicit inverse factor of the layer (cov_inverse)")
    if state.M + N > state.capacity:
        raise EmcidHipError(f"{state.M} preserved + {N} new rows exceed the state's capacity {state.capacity}")
    ws = PreserveWorkspace.fitting(ws, K.device, N, d, h, state.capacity)
    dW = torch.empty(h, d, dtype=torch.float32, device=K.device) if want_dw else None
    U = torch.empty(h, d, dtype=torch.float64, device=K.device) if want_u else None
    _check(load().emcid_edit_layer_dual_preserve_f64(
        _ptr(K, torch.float32, "K"), _ptr(Zc, torch.float32, "Zc"), _ptr(zs_t, torch.float32, "zs_t"), N, d, h,
        float(edit_weight), int(layers_left), factors.lam_ratio(lam), _ptr(factors.buf), factors.n_layers, int(layer_index),
        *state.layer_args(layer_index), _ptr(W0, torch.float32, "W0"), _ptr(W, torch.float32, "W"), _ptr(dW), _ptr(U),
        _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32), _stream(K)), "emcid_edit_layer_dual_preserve_f64")
    return {"dW": dW, "U": U, "ws": ws}


def row_scale_of(edit_weight: float, factors: CovFactors, lam: Optional[float] = None, weight: float = 1.0) -> float:
    """The factor a raw key is multiplied by on its way into a preserved key set (``PreservedKeys.row_scale``): sqrt(weight
    edit_weight / 0.5), the ``row_scale`` of ``session_retain`` (weight 1: an edited key's), over sqrt(lam_ratio)."""
    return math.sqrt(float(weight) * float(edit_weight) / 0.5) / math.sqrt(factors.lam_ratio(lam))


def session_retain(K, factors: CovFactors, layer_index: int, row_scale: float, state: PreservedKeys,
                   ws: Optional[RetainWorkspace] = None, lam: Optional[float] = None):
    """A retain list for layer ``layer_index`` of ``state``: the rows of K (N, d) fp32, scaled by ``row_scale``, enter the
    preserved key set with a zero residual — Yk, [Lkp Lkk] and the touched tile inverses land behind ``state.M``; no weight is
    read or written (include/emcid_hip.h, emcid_session_retain_f64).  Nothing is committed here (``state.commit(N, scale)`` after the
    flag word ``ws.info`` read zero, for all layers together).  Needs the layer's explicit inverse factor.  Returns dict(ws)."""
    N, d = K.shape
    assert K.is_contiguous(), "K"
    assert factors.d == d == state.d
    state.check_layer(layer_index)
    if layer_index not in factors.have_inverse:
        raise EmcidHipError("session_retain needs the explicit inverse factor of the layer (cov_inverse)")
    if state.M + N > state.capacity:
        raise EmcidHipError(f"{state.M} preserved + {N} retained rows exceed the state's capacity {state.capacity}")
    row_scale = float(row_scale)
    if not (row_scale > 0.0 and row_scale < float("inf")):
        raise EmcidHipError(f"row_scale must be positive and finite (got {row_scale})")
    ws = RetainWorkspace.fitting(ws, K.device, N, d, state.capacity)
    _check(load().emcid_session_retain_f64(
        _ptr(K, torch.float32, "K"), N, d, row_scale, factors.lam_ratio(lam), _ptr(factors.buf), factors.n_layers, int(layer_index),
        *state.layer_args(layer_index), _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32), _stream(K)), "emcid_session_retain_f64")
    return {"ws": ws}


def check_keep(keep, M: int):
    """(keep as a list of ints, first): ``keep`` must be strictly ascending indices inside [0, M); ``first`` is the smallest index
    that is NOT kept (== len(keep): only trailing rows go, or none).  Pure host code."""
    keep = [int(i) for i in keep]
    if any(i < 0 or i >= M for i in keep) or any(b <= a for a, b in zip(keep, keep[1:])):
        raise EmcidHipError(f"keep must be strictly ascending row indices inside [0, {M})")
    first = next((j for j, i in enumerate(keep) if i != j), len(keep))
    return keep, first


def session_release(state: PreservedKeys, layer_index: int, keep, first: Optional[int] = None, ws: Optional[ReleaseWorkspace] = None):
    """Release rows of layer ``layer_index`` of ``state``: the rows ``keep`` (strictly ascending indices < ``state.M``) stay, the
    others go.  Rows below ``first`` (the smallest released index; worked out from ``keep`` when None) are not touched; the kept
    rows behind it are rebuilt in place as the key half of a step (include/emcid_hip.h, emcid_session_release_f64).  Nothing is
    committed here (``state.release_commit(keep)`` after the flag word ``ws.info`` read zero, for all layers together).  A release
    of trailing rows only, or of every row, launches nothing.  ``keep`` may be an int32 tensor on the state's device holding the
    same indices (then ``first`` must be given and nothing is checked on the host).  Returns dict(ws | None, launched, first)."""
    state.check_layer(layer_index)
    Yp = state.Yp[layer_index]
    if isinstance(keep, torch.Tensor) and keep.is_cuda:
        if first is None:
            raise EmcidHipError("session_release: a device tensor of kept rows needs `first`")
        keep_dev, n_keep, first = keep, int(keep.numel()), int(first)
        if keep_dev.dtype != torch.int32 or not keep_dev.is_contiguous() or keep_dev.device != Yp.device:
            raise EmcidHipError(f"session_release: keep must be a contiguous int32 tensor on {Yp.device}")
    else:
        rows, f = check_keep(keep.tolist() if isinstance(keep, torch.Tensor) else keep, state.M)
        if first is not None and int(first) != f:
            raise EmcidHipError(f"session_release: first = {first}, but the smallest released row of keep is {f}")
        keep_dev, n_keep, first = None, len(rows), f
    if not 0 <= first <= n_keep <= state.M:
        raise EmcidHipError(f"session_release: first = {first}, {n_keep} kept rows, {state.M} committed")
    if n_keep == state.M or first == n_keep:       # nothing goes; or only trailing rows (everything included): the set is truncated
        return {"ws": None, "launched": False, "first": first}
    if keep_dev is None:
        keep_dev = torch.tensor(rows, dtype=torch.int32, device=Yp.device)
    ws = ReleaseWorkspace.fitting(ws, Yp.device, n_keep - first, state.d, state.capacity)
    _check(load().emcid_session_release_f64(
        _ptr(keep_dev, torch.int32, "keep"), n_keep, first, state.d, *state.layer_args(layer_index),
        _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32), _stream(Yp)), "emcid_session_release_f64")
    return {"ws": ws, "launched": True, "first": first}


def check_factors(factors, M: int) -> torch.Tensor:
    """``factors`` as an (M,) f64 host tensor: one number for every row, or M of them; ``EmcidHipError`` for another length and for
    a factor that is not positive and finite.  Pure host code."""
    try:
        f = torch.as_tensor(factors, dtype=torch.float64, device="cpu").detach()
    except (TypeError, ValueError, RuntimeError) as e:
        raise EmcidHipError(f"row factors must be numbers: {e}") from e
    if f.dim() == 0:
        f = f.repeat(M)
    if f.dim() != 1 or f.numel() != M:
        raise EmcidHipError(f"{tuple(f.shape)} row factors for {M} committed rows")
    if not bool((torch.isfinite(f) & (f > 0.0)).all()):
        raise EmcidHipError("row factors must be positive and finite")
    return f.contiguous()


class RescaleWorkspace(_SessionWorkspace):
    """The workspace of emcid_session_rescale_f64 for a rescale that rebuilds ``n_rebuilt`` rows: the retain workspace of that N
    (which may equal the capacity)."""

    def __init__(self, n_rebuilt: int, d: int, capacity: int, device):
        super().__init__("rescale", load().emcid_session_retain_workspace_bytes, dict(n_rebuilt=n_rebuilt, d=d, capacity=capacity),
                         device)


def session_rescale(state: PreservedKeys, layer_index: int, factors, first: Optional[int] = None, src: Optional[torch.Tensor] = None,
                    ws: Optional[RescaleWorkspace] = None):
    """Scale the committed rows of layer ``layer_index`` of ``state`` by ``factors`` (one number, or one per committed row; all
    positive and finite) and rebuild what lies behind ``first``, the smallest row whose factor is not 1 (worked out when None; a
    smaller one may be given): rows [first, M) of ``src`` (default: the layer's own Yp; else an f64 tensor of >= M rows of the
    same width on the same device, a copy of them) times their factors become the layer's rows, Lp and the tile inverses behind
    ``first`` follow as the key half of a step (include/emcid_hip.h, emcid_session_rescale_f64).  Nothing is committed here
    (``state.rescale_commit(...)`` after the flag word ``ws.info`` read zero, for all layers together).  All factors 1 with no
    ``src``, and M = 0, launch nothing.  ``factors`` may be an (M,) f64 tensor on the state's device (then ``first`` must be
    given and nothing is checked on the host).  Returns dict(ws | None, launched, first)."""
    state.check_layer(layer_index)
    Yp, M = state.Yp[layer_index], state.M
    if isinstance(factors, torch.Tensor) and factors.is_cuda:
        if first is None:
            raise EmcidHipError("session_rescale: a device tensor of factors needs `first`")
        if factors.dtype != torch.float64 or not factors.is_contiguous() or factors.numel() != M or factors.device != Yp.device:
            raise EmcidHipError(f"session_rescale: factors must be a contiguous f64 tensor of {M} elements on {Yp.device}")
        f_dev, first = factors, int(first)
    else:
        f = check_factors(factors, M)
        changed = torch.nonzero(f != 1.0).flatten()
        lowest = int(changed[0]) if changed.numel() else M
        if first is None:
            first = 0 if src is not None else lowest
        first = int(first)
        if not 0 <= first <= M:
            raise EmcidHipError(f"session_rescale: first = {first}, {M} committed")
        if first > lowest:
            raise EmcidHipError(f"session_rescale: first = {first}, but row {lowest} has the factor {float(f[lowest])}")
        f_dev = None
    if not 0 <= first <= M:
        raise EmcidHipError(f"session_rescale: first = {first}, {M} committed")
    if first == M:
        return {"ws": None, "launched": False, "first": first}
    if not Yp.is_cuda:
        raise EmcidHipError(f"session_rescale runs on a state in HBM (got {Yp.device}); there is no CPU path")
    if src is not None:
        if not isinstance(src, torch.Tensor) or src.dtype != torch.float64 or src.dim() != 2 or src.device != Yp.device or \
                src.shape[0] < M or src.shape[1] < state.dp or src.stride(1) != 1 or src.stride(0) % 2 or src.data_ptr() % 16:
            raise EmcidHipError(f"session_rescale: src must be an f64 tensor of >= ({M}, {state.dp}) on {Yp.device}, rows contiguous")
    if f_dev is None:
        f_dev = f.to(Yp.device)
    ws = RescaleWorkspace.fitting(ws, Yp.device, M - first, state.d, state.capacity)
    s = Yp if src is None else src
    _check(load().emcid_session_rescale_f64(
        _ptr(f_dev, torch.float64, "factors"), _ptr(s, torch.float64, "src"), s.stride(0), first, state.d,
        *state.layer_args(layer_index), _ptr(ws.buf), ws.nbytes, _ptr(ws.info, torch.int32), _stream(Yp)),
        "emcid_session_rescale_f64")
    return {"ws": ws, "launched": True, "first": first}


def session_step_norms(ws: PreserveWorkspace, N: int, d: int, h: int, state: PreservedKeys, out: Optional[torch.Tensor] = None):
    """The readout of the ``edit_layer_dual_preserve`` call that has just run on ``ws`` (same N, d, h, ``state.M`` not yet
    committed, the same stream): one launch, no synchronisation.  Returns dict(drift (M,), left (N,), resid (N,)) f64 in HBM:
    ||Zp_i||, ||Zk_j||, ||Rt_j|| in the solve's scaled units — the step moved preserved key i by ||dW k_i|| = drift[i] /
    state.row_scale[i] and left the fraction left[j] / resid[j] of new residual j.  ``out``: a contiguous f64 tensor of at least
    M + 2 N elements on the device to write into (the three results are views of it)."""
    N, M = int(N), int(state.M)
    if not isinstance(ws, PreserveWorkspace) or ws.key != (N, int(d), int(h), state.capacity):
        raise EmcidHipError(f"session_step_norms reads the workspace of the preserve step of N={N}, d={d}, h={h} at capacity "
                            f"{state.capacity} (got {getattr(ws, 'key', None)})")
    if M + N > state.capacity:
        raise EmcidHipError(f"{M} preserved + {N} new rows exceed the state's capacity {state.capacity}")
    if out is None:
        out = torch.empty(M + 2 * N, dtype=torch.float64, device=ws.buf.device)
    if out.dtype != torch.float64 or not out.is_contiguous() or out.numel() < M + 2 * N or out.device != ws.buf.device:
        raise EmcidHipError(f"session_step_norms: out must be a contiguous f64 tensor of >= {M + 2 * N} elements on {ws.buf.device}")
    flat = out.view(-1)
    drift, left, resid = flat[:M], flat[M:M + N], flat[M + N:M + 2 * N]
    _check(load().emcid_session_step_norms_f64(
        _ptr(ws.buf), ws.nbytes, N, int(d), int(h), state.capacity, M, _ptr(drift, torch.float64, "drift") if M > 0 else None,
        _ptr(left, torch.float64, "left"), _ptr(resid, torch.float64, "resid"), _stream(ws.buf)), "emcid_session_step_norms_f64")
    return {"drift": drift, "left": left, "resid": resid}


# ---- the readout of an edit score (csrc/score.hip) -----------------------------------------------------------------------------

SCORE_MAX_COLS = 2048


def _f64_out(who: str, out: Optional[torch.Tensor], shape: tuple, device) -> torch.Tensor:
    """``out`` when it is a contiguous f64 tensor of ``shape`` on ``device`` (refused otherwise), a new one for ``None``."""
    if out is None:
        return torch.empty(shape, dtype=torch.float64, device=device)
    if out.dtype != torch.float64 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise EmcidHipError(f"{who}: out must be a contiguous ({', '.join(str(n) for n in shape)}) f64 tensor on {device}")
    return out


def score_rows(a: torch.Tensor, b: torch.Tensor, t: Optional[torch.Tensor] = None, ln: Optional[torch.nn.LayerNorm] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(rows, 8) f64 in HBM, one launch (include/emcid_hip.h, emcid_score_rows_f32): per row of the fp32 matrices ``a``, ``b``
    (rows, cols) — behind ``ln`` (an affine LayerNorm over cols, applied to both in fp64) when given — ||a^ - b^||^2, ||b^||^2,
    ||a^||^2, a^ . b^ in slots 0-3 and, with a target ``t`` (rows, cols), ||t - a||^2, ||t - b||^2, (a - b) . (t - b) on the raw
    rows in slots 4-6.  Row strides may differ from cols (multiples of 4); cols % 4 == 0 and <= 2048, else the library refuses
    the call before it launches anything.  ``out``: a contiguous (rows, 8) f64 tensor to write into."""
    if a.dim() != 2 or a.shape != b.shape or (t is not None and t.shape != a.shape):
        raise EmcidHipError(f"score_rows: a, b (and t) must be matrices of one shape (got {tuple(a.shape)}, {tuple(b.shape)}"
                            f"{', ' + str(tuple(t.shape)) if t is not None else ''})")
    rows, cols = a.shape
    for x, nm in ((a, "a"), (b, "b"), (t, "t")):
        if x is not None and (x.stride(1) != 1 or x.device != a.device):
            raise EmcidHipError(f"score_rows: {nm} must have unit column stride and live on {a.device}")
    if ln is not None and (ln.weight is None or ln.bias is None or tuple(ln.normalized_shape) != (cols,)
                           or not ln.weight.is_contiguous() or not ln.bias.is_contiguous()):
        raise EmcidHipError("score_rows: a LayerNorm over the last dimension with contiguous affine parameters")
    out = _f64_out("score_rows", out, (rows, 8), a.device)
    _check(load().emcid_score_rows_f32(
        _ptr(a, torch.float32, "a"), a.stride(0), _ptr(b, torch.float32, "b"), b.stride(0), _ptr(t, torch.float32, "t"),
        t.stride(0) if t is not None else 0, _ptr(ln.weight, torch.float32, "gamma") if ln is not None else None,
        _ptr(ln.bias, torch.float32, "beta") if ln is not None else None, float(ln.eps) if ln is not None else 0.0, rows, cols,
        _ptr(out, torch.float64, "out"), _stream(a)), "emcid_score_rows_f32")
    return out


def _check_chain_arrays(who: str, node: torch.Tensor, anc: torch.Tensor, depth: torch.Tensor, end_node: torch.Tensor):
    U = node.shape[0]
    if node.dim() != 2 or node.shape[1] != 8 or not node.is_contiguous():
        raise EmcidHipError(f"{who}: node must be a contiguous (U, 8) f64 tensor (got {tuple(node.shape)})")
    if anc.dim() != 2 or anc.shape[0] != U or anc.stride(1) != 1 or depth.shape != (U,) or not depth.is_contiguous():
        raise EmcidHipError(f"{who}: anc (U, S) and depth (U,) must describe the {U} nodes (got {tuple(anc.shape)}, "
                            f"{tuple(depth.shape)})")
    if end_node.dim() != 1 or end_node.numel() == 0 or not end_node.is_contiguous():
        raise EmcidHipError(f"{who}: end_node must be a non-empty contiguous (B,) int64 tensor")


def _check_chain_pair(who: str, first: tuple, second: tuple, more: tuple = ()) -> int:
    """The pairing of two tries' (node, anc, depth, end_node): each as ``_check_chain_arrays`` takes it, as many end nodes in one
    as in the other, and they and ``more`` on one device.  Returns that number B of end nodes."""
    _check_chain_arrays(who, *first)
    _check_chain_arrays(who, *second)
    B = first[3].numel()
    if second[3].numel() != B:
        raise EmcidHipError(f"{who}: {B} end nodes in the first trie, {second[3].numel()} in the second")
    if any(x.device != first[0].device for x in first[1:] + second + more):
        raise EmcidHipError(f"{who}: every operand must live on {first[0].device}")
    return B


def score_chains(node: torch.Tensor, anc: torch.Tensor, depth: torch.Tensor, end_node: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, 4) f64 in HBM, one launch (emcid_score_chains_f64): per prompt the max, the mean and the end-node value of
    sqrt(node[u, 0] / node[u, 1]) over the chain ``anc[e, 0 .. depth[e]]`` of its end node e = ``end_node[p]``, and the chain
    position of the max.  ``node`` (U, 8) f64 (``score_rows``' result), ``anc`` (U, S) int32, ``depth`` (U,) int32 — a trie's own
    arrays —, ``end_node`` (B,) int64."""
    _check_chain_arrays("score_chains", node, anc, depth, end_node)
    U = node.shape[0]
    if any(x.device != node.device for x in (anc, depth, end_node)):
        raise EmcidHipError(f"score_chains: every operand must live on {node.device}")
    B = end_node.numel()
    out = _f64_out("score_chains", out, (B, 4), node.device)
    _check(load().emcid_score_chains_f64(
        _ptr(node, torch.float64, "node"), U, _ptr(anc, torch.int32, "anc"), anc.stride(0), _ptr(depth, torch.int32, "depth"),
        _ptr(end_node, torch.int64, "end_node"), B, _ptr(out, torch.float64, "out"), _stream(node)), "emcid_score_chains_f64")
    return out


def score_chains_pair(node1: torch.Tensor, anc1: torch.Tensor, depth1: torch.Tensor, end_node1: torch.Tensor,
                      node2: torch.Tensor, anc2: torch.Tensor, depth2: torch.Tensor, end_node2: torch.Tensor,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, 4) f64 in HBM, one launch (emcid_score_chains_pair_f64): ``score_chains`` over the concatenated columns of two encoders.
    Per prompt p and chain position j, with c_e the chain ``anc_e[end_node_e[p], 0 .. depth_e[end_node_e[p]]]`` in encoder e's own
    trie, r_j = sqrt((node1[c_1[j], 0] + node2[c_2[j], 0]) / (node1[c_1[j], 1] + node2[c_2[j], 1])); the max, the mean, the value at
    the end and the chain position of the max.  A prompt whose two chains differ in length (or leave their tries) gets four NaN."""
    B = _check_chain_pair("score_chains_pair", (node1, anc1, depth1, end_node1), (node2, anc2, depth2, end_node2))
    out = _f64_out("score_chains_pair", out, (B, 4), node1.device)
    _check(load().emcid_score_chains_pair_f64(
        _ptr(node1, torch.float64, "node1"), node1.shape[0], _ptr(anc1, torch.int32, "anc1"), anc1.stride(0),
        _ptr(depth1, torch.int32, "depth1"), _ptr(end_node1, torch.int64, "end_node1"),
        _ptr(node2, torch.float64, "node2"), node2.shape[0], _ptr(anc2, torch.int32, "anc2"), anc2.stride(0),
        _ptr(depth2, torch.int32, "depth2"), _ptr(end_node2, torch.int64, "end_node2"), B, _ptr(out, torch.float64, "out"),
        _stream(node1)), "emcid_score_chains_pair_f64")
    return out


def score_chains_pair_grid(node1_bank: torch.Tensor, anc1: torch.Tensor, depth1: torch.Tensor, end_node1: torch.Tensor,
                           node2_bank: torch.Tensor, anc2: torch.Tensor, depth2: torch.Tensor, end_node2: torch.Tensor,
                           combo: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(C, B, 4) f64 in HBM, one launch (emcid_score_chains_pair_grid_f64): ``score_chains_pair`` for every row (g1, g2) of
    ``combo`` (C, 2) int32 on the device, on ``node1_bank[g1]`` and ``node2_bank[g2]`` — the banks are (G_e, U_e, 8) f64, one
    ``score_rows`` result per point of encoder e.  ``out[c]`` holds the bits ``score_chains_pair`` gives on those two slices; a
    row of ``combo`` that leaves a bank gives NaN for every prompt of that combination."""
    for bank, nm in ((node1_bank, "node1_bank"), (node2_bank, "node2_bank")):
        if bank.dim() != 3 or bank.shape[0] < 1:
            raise EmcidHipError(f"score_chains_pair_grid: {nm} must be a (G, U, 8) f64 tensor (got {tuple(bank.shape)})")
    if not node1_bank.is_contiguous() or not node2_bank.is_contiguous():
        raise EmcidHipError("score_chains_pair_grid: the banks must be contiguous")
    if combo.dim() != 2 or combo.shape[1] != 2 or combo.shape[0] < 1 or not combo.is_contiguous():
        raise EmcidHipError(f"score_chains_pair_grid: combo must be a non-empty contiguous (C, 2) int32 tensor (got {tuple(combo.shape)})")
    B = _check_chain_pair("score_chains_pair_grid", (node1_bank[0], anc1, depth1, end_node1), (node2_bank[0], anc2, depth2, end_node2),
                          (combo,))
    n_combo = combo.shape[0]
    out = _f64_out("score_chains_pair_grid", out, (n_combo, B, 4), node1_bank.device)
    _check(load().emcid_score_chains_pair_grid_f64(
        _ptr(node1_bank, torch.float64, "node1_bank"), node1_bank.shape[0], node1_bank.shape[1], _ptr(anc1, torch.int32, "anc1"),
        anc1.stride(0), _ptr(depth1, torch.int32, "depth1"), _ptr(end_node1, torch.int64, "end_node1"),
        _ptr(node2_bank, torch.float64, "node2_bank"), node2_bank.shape[0], node2_bank.shape[1], _ptr(anc2, torch.int32, "anc2"),
        anc2.stride(0), _ptr(depth2, torch.int32, "depth2"), _ptr(end_node2, torch.int64, "end_node2"), B,
        _ptr(combo, torch.int32, "combo"), n_combo, _ptr(out, torch.float64, "out"), _stream(node1_bank)),
        "emcid_score_chains_pair_grid_f64")
    return out


def score_pooled(a: torch.Tensor, b: torch.Tensor, ln: torch.nn.LayerNorm, proj_weight: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(rows, 4) f64 in HBM, one launch (emcid_score_pooled_f32): per row of the fp32 matrices ``a``, ``b`` (rows, cols), with
    a^ = ln(a), b^ = ln(b) in fp64 (``ln``: an affine LayerNorm over cols) and P = ``proj_weight`` (proj, cols) fp32, a projection
    without bias: ||P (a^ - b^)||^2, ||P b^||^2, ||P a^||^2, (P a^) . (P b^).  a^ - b^ is formed from a - b (``score_rows``):
    identical rows give an exact 0 in slot 0.  Row strides may differ from cols (multiples of 4); cols % 4 == 0 and <= 2048, else
    the library refuses the call before it launches anything."""
    if a.dim() != 2 or a.shape != b.shape:
        raise EmcidHipError(f"score_pooled: a, b must be matrices of one shape (got {tuple(a.shape)}, {tuple(b.shape)})")
    rows, cols = a.shape
    if proj_weight.dim() != 2 or proj_weight.shape[1] != cols or proj_weight.shape[0] < 1:
        raise EmcidHipError(f"score_pooled: proj_weight must be a (proj, {cols}) matrix (got {tuple(proj_weight.shape)})")
    for x, nm in ((a, "a"), (b, "b"), (proj_weight, "proj_weight")):
        if x.stride(1) != 1 or x.device != a.device:
            raise EmcidHipError(f"score_pooled: {nm} must have unit column stride and live on {a.device}")
    if not isinstance(ln, torch.nn.LayerNorm) or ln.weight is None or ln.bias is None or tuple(ln.normalized_shape) != (cols,) \
            or not ln.weight.is_contiguous() or not ln.bias.is_contiguous() or ln.weight.device != a.device:
        raise EmcidHipError("score_pooled: a LayerNorm over the last dimension with contiguous affine parameters")
    out = _f64_out("score_pooled", out, (rows, 4), a.device)
    _check(load().emcid_score_pooled_f32(
        _ptr(a, torch.float32, "a"), a.stride(0), _ptr(b, torch.float32, "b"), b.stride(0), _ptr(ln.weight, torch.float32, "gamma"),
        _ptr(ln.bias, torch.float32, "beta"), float(ln.eps), _ptr(proj_weight, torch.float32, "proj_weight"), proj_weight.stride(0),
        rows, cols, proj_weight.shape[0], _ptr(out, torch.float64, "out"), _stream(a)), "emcid_score_pooled_f32")
    return out


def cov_factor_fold(src: CovFactors, state: PreservedKeys, layer_index: int, cov: Optional[torch.Tensor], lam: float,
                    edit_weight: float, dst: CovFactors, base: torch.Tensor, ws: Optional[torch.Tensor] = None) -> CovFactors:
    """Fold the ``state.M`` preserved rows of layer ``layer_index`` into the caller's own factors (include/emcid_hip.h,
    emcid_cov_factor_fold_f64): ``base`` (n_layers, dp, dp) f64 += P^T P for the keys P = Yp L_s^T that ``state`` holds in the
    coordinates of ``src`` (lam: the session's own, any ratio to ``src.lam``), then layer ``layer_index`` of ``dst`` = the factor
    of ``base``, its block inverses and X = inv(L).  ``cov`` (d, d) fp32: the layer's statistics, from which ``base`` is filled
    first (the first fold); ``None``: ``base`` is what the previous fold left.  ``src`` is only read; ``dst is src`` folds the
    caller's own workspace in place (``src.lam`` must be ``lam`` then).  ``ws``: an f64 scratch tensor of at least
    ``state.M * dp`` elements.  Asynchronous on the current stream; ``dst.info`` reports a non-positive pivot.  Returns ``dst``
    with ``lam`` / ``edit_weight`` recorded, ``have_inverse`` updated and ``cached = False``; ``state`` is not touched."""
    lib = load()
    if src.n_layers != dst.n_layers or src.d != dst.d or state.d != src.d:
        raise EmcidHipError(f"fold: src ({src.n_layers} x {src.d}), dst ({dst.n_layers} x {dst.d}) and the state (d = {state.d}) "
                            f"must describe the same layers")
    if dst is not src and dst.cached:
        raise EmcidHipError("fold: dst is a workspace of the factor cache; a fold writes only into a workspace its caller owns")
    if dst is src and src.cached:
        raise EmcidHipError("fold: an in-place fold needs a workspace its caller owns (this one belongs to the factor cache)")
    dp = src.dp
    if base.dtype != torch.float64 or not base.is_contiguous() or base.numel() != src.n_layers * dp * dp:
        raise EmcidHipError(f"fold: base must be a contiguous f64 tensor of {src.n_layers} x {dp} x {dp}")
    if cov is not None:
        assert cov.shape == (src.d, src.d) and cov.is_contiguous()
    M = int(state.M)
    need = int(lib.emcid_cov_factor_fold_workspace_bytes(max(M, 1), src.d))
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.float64, device=src.buf.device)
    if src.ready is not None:
        torch.cuda.current_stream(src.buf.device).wait_event(src.ready)
    in_range = 0 <= layer_index < state.n_layers        # (a layer outside the state: the library refuses the call)
    Yp, ldy = state.layer_args(layer_index if in_range else 0)[:2]
    base_l = base.view(src.n_layers, dp, dp)[layer_index if in_range else 0]
    _check(lib.emcid_cov_factor_fold_f64(
        _ptr(src.buf), src.lam_ratio(lam), Yp, ldy, M, state.capacity,
        _ptr(cov, torch.float32, "C"), float(lam), float(edit_weight), int(cov is not None), _ptr(dst.buf), src.n_layers, src.d,
        int(layer_index), _ptr(base_l, torch.float64, "base"), _ptr(ws, torch.float64, "ws"), ws.numel() * 8,
        _ptr(dst.info, torch.int32), _stream(src.buf)), "emcid_cov_factor_fold_f64")
    dst.have_inverse.add(int(layer_index))
    dst.lam, dst.edit_weight, dst.cached = float(lam), float(edit_weight), False
    return dst


def _check_own_workspace(factors: CovFactors, who: str):
    if factors.cached:
        raise EmcidHipError(f"{who}: the workspace belongs to the factor cache; a refold writes only into a workspace its caller owns")


def session_refold_update(factors: CovFactors, state: PreservedKeys, layer_index: int, archive: torch.Tensor, n_archived: int,
                          rel_idx: Optional[torch.Tensor], base: torch.Tensor):
    """The update half of a release across a fold for layer ``layer_index`` (include/emcid_hip.h, emcid_session_refold_update_f64),
    in place on ``factors``, the caller's OWN workspace (never one of the factor cache) whose lam is the session's: the ``state.M``
    live rows go into rows [n_archived, n_archived + M) of ``archive`` (rows, dp) f64 as Q = Yp L^T, ``base`` (n_layers, dp, dp) f64
    += Q^T Q, then ``base`` -= the rows ``rel_idx`` names (int32 on the device, indices into the n_archived + M rows the archive
    holds by then; ``None``: no row goes) and the result lands in the layer's M region for ``cov_factor_refactor``.  L, X and the
    state are only read and ``have_inverse`` stays as it is: the workspace is whole until the refactorization runs.  Asynchronous
    on the current stream; nothing is committed here (the caller counts the archive's new rows once the flag read zero)."""
    _check_own_workspace(factors, "session_refold_update")
    if state.d != factors.d:
        raise EmcidHipError(f"refold: the workspace (d = {factors.d}) and the state (d = {state.d}) must describe the same layers")
    dp, M, n_archived = factors.dp, int(state.M), int(n_archived)
    if base.dtype != torch.float64 or not base.is_contiguous() or base.numel() != factors.n_layers * dp * dp:
        raise EmcidHipError(f"refold: base must be a contiguous f64 tensor of {factors.n_layers} x {dp} x {dp}")
    if archive.dtype != torch.float64 or archive.dim() != 2 or archive.stride(1) != 1 or archive.shape[1] < dp or \
            n_archived < 0 or archive.shape[0] < n_archived + M:
        raise EmcidHipError(f"refold: the archive must be an f64 tensor of at least {n_archived + M} rows of {dp} (got "
                            f"{tuple(archive.shape)}, {archive.dtype})")
    n_rel = 0 if rel_idx is None else int(rel_idx.numel())
    if n_rel and (rel_idx.dtype != torch.int32 or not rel_idx.is_contiguous() or rel_idx.device != archive.device):
        raise EmcidHipError(f"refold: rel_idx must be a contiguous int32 tensor on {archive.device}")
    in_range = 0 <= layer_index < state.n_layers        # (a layer outside the state: the library refuses the call)
    Yp, ldy = state.layer_args(layer_index if in_range else 0)[:2]
    base_l = base.view(factors.n_layers, dp, dp)[layer_index if in_range and layer_index < factors.n_layers else 0]
    _check(load().emcid_session_refold_update_f64(
        _ptr(factors.buf), factors.n_layers, factors.d, int(layer_index), Yp, ldy, M, state.capacity,
        _ptr(archive, torch.float64, "archive"), archive.stride(0), n_archived, _ptr(rel_idx) if n_rel else None, n_rel,
        _ptr(base_l, torch.float64, "base"), _stream(factors.buf)), "emcid_session_refold_update_f64")


def cov_factor_from_base(base: torch.Tensor, d: int, lam: float, edit_weight: float) -> CovFactors:
    """A new workspace, its caller's own, holding the factors of the systems ``base`` (n_layers, dp, dp) f64 holds in its lower
    triangles (a folded session's accumulator, ``cov_factor_fold``): every layer's system is copied into its M region, made
    symmetric from the lower triangle, and all of them are factored and inverted as the one batched chain of a release across a
    fold (``cov_factor_refactor``).  Asynchronous on the current stream; ``info`` of the result reports a non-positive pivot;
    ``base`` is only read."""
    n_layers = int(base.shape[0])
    fac = CovFactors(n_layers, int(d), base.device)
    if base.dtype != torch.float64 or tuple(base.shape) != (n_layers, fac.dp, fac.dp):
        raise EmcidHipError(f"base must be an f64 tensor of {n_layers} x {fac.dp} x {fac.dp} (got {tuple(base.shape)}, {base.dtype})")
    regions = fac.buf[:n_layers * fac.dp * fac.dp].view(n_layers, fac.dp, fac.dp)
    torch.tril(base, out=regions)
    regions += torch.tril(base, -1).transpose(1, 2)
    fac.lam, fac.edit_weight = float(lam), float(edit_weight)
    return cov_factor_refactor(fac)


def cov_factor_refactor(factors: CovFactors) -> CovFactors:
    """Factor the M regions of every layer of ``factors`` — the caller's OWN workspace, after ``session_refold_update`` on each
    layer — as one batched chain and build every X = inv(L) (emcid_cov_factor_refactor_f64, then ``cov_inverse``).  Asynchronous
    on the current stream; ``factors.info`` reports a non-positive pivot.  ``have_inverse`` is emptied by the factorization and
    filled again by the inverse build."""
    _check_own_workspace(factors, "cov_factor_refactor")
    _check(load().emcid_cov_factor_refactor_f64(_ptr(factors.buf), factors.nbytes, factors.n_layers, factors.d,
                                                _ptr(factors.info, torch.int32), _stream(factors.buf)), "emcid_cov_factor_refactor_f64")
    factors.have_inverse = set()
    cov_inverse(factors)
    return factors

"""Every exported entry that takes (workspace, workspace_bytes) refuses a workspace 8 bytes short of what its *_workspace_bytes
function asks for, with status -3 (EMCID_ERR_WORKSPACE) and a fixed message, before it touches the device: the pointers here are
host memory and no GPU is needed.  Also pins the size of the covariance-factor workspace [M | L | 512-block inverses | X] x layers."""
import ctypes as C

import pytest

from emcid_amd import hip

N, D, H, CAP, LAYERS = 5, 128, 16, 8, 1
ERR_WORKSPACE = -3

_buf = (C.c_char * 4096)()
P = (C.addressof(_buf) + 15) & ~15          # a non-null, 16-byte aligned address that no entry gets as far as reading
_tiles = (C.c_int * 1)(0)                   # the column-sharded entries read their tile list on the host before the size check
TILES = C.addressof(_tiles)

EDIT = ("emcid_edit_workspace_bytes", (N, D, H))
COV = ("emcid_cov_factor_workspace_bytes", (LAYERS, D))
DUAL = ("emcid_edit_dual_workspace_bytes", (N, D, H))
PRESERVE = ("emcid_edit_dual_preserve_workspace_bytes", (N, D, H, CAP))
RETAIN = ("emcid_session_retain_workspace_bytes", (N, D, CAP))
PLAIN = "workspace too small"

# entry -> (its size function and arguments, the arguments with "WS" where workspace_bytes goes, the message behind "<name>: ")
CASES = {
    "emcid_dgemm_streamk_f64": (("emcid_streamk_workspace_bytes", (8,)),
                                (0, 128, 128, 128, 1.0, P, 128, P, 128, P, 128, 16, 8, 0.0, P, "WS", None), None, PLAIN),
    "emcid_edit_layer_f64": (EDIT, (P, P, P, P, N, D, H, 1.0, 0.5, 1, None, None, None, None, P, P, "WS", P, None),
                             "edit_layer_impl", PLAIN + " (see emcid_edit_workspace_bytes)"),
    "emcid_edit_layer_shard_f64": (EDIT, (P, P, P, P, N, D, H, 1.0, 0.5, 1, 0, N, P, None, None, P, "WS", P, None),
                                   "edit_layer_impl", PLAIN + " (see emcid_edit_workspace_bytes)"),
    "emcid_edit_layer_lu_f64": (("emcid_edit_lu_workspace_bytes", (N, D, H)),
                                (P, P, P, P, N, D, H, 1.0, 0.5, 1, None, None, None, None, P, P, "WS", P, None), None, PLAIN),
    "emcid_factor_cov_f64": (COV, (P, LAYERS, D, 1.0, 0.5, P, "WS", P, None), None,
                             PLAIN + " (see emcid_cov_factor_workspace_bytes)"),
    "emcid_cov_factor_rescale_f64": (COV, (P, P, "WS", LAYERS, D, 2.0, 1, None), None,
                                     PLAIN + " (see emcid_cov_factor_workspace_bytes)"),
    "emcid_cov_factor_fold_f64": (("emcid_cov_factor_fold_workspace_bytes", (N, D)),
                                  (P, 1.0, P, 128, N, CAP, None, 1.0, 0.5, 0, P, LAYERS, D, 0, P, P, "WS", P, None), None,
                                  PLAIN + " (see emcid_cov_factor_fold_workspace_bytes)"),
    "emcid_edit_dual_stage1_f64": (DUAL, (P, P, P, N, D, H, 0.5, 1, 1.0, P, LAYERS, 0, 0, N, 1, P, "WS", None), None, PLAIN),
    "emcid_edit_dual_stage2_f64": (DUAL, (N, D, H, 1.0, None, None, None, None, P, P, "WS", P, None), None, PLAIN),
    "emcid_edit_dual_apply_stage1_f64": (DUAL, (P, P, P, N, D, H, 0.5, 1, 1.0, P, LAYERS, 0, 0, N, 1, P, "WS", None), None, PLAIN),
    "emcid_edit_dual_apply_assemble_f64": (DUAL, (N, D, H, P, "WS", None), None, PLAIN),
    "emcid_edit_dual_apply_stage2_f64": (DUAL, (N, D, H, P, LAYERS, 0, 1, 0, None, None, P, P, "WS", P, None), None, PLAIN),
    "emcid_edit_layer_dual_preserve_f64": (PRESERVE, (P, P, P, N, D, H, 0.5, 1, 1.0, P, LAYERS, 0, P, 128, P, CAP, P, CAP, 3,
                                                      None, None, P, None, P, "WS", P, None), None, PLAIN),
    "emcid_session_retain_f64": (RETAIN, (P, N, D, 1.0, 1.0, P, LAYERS, 0, P, 128, P, CAP, P, CAP, 3, P, "WS", P, None), None, PLAIN),
    # rows 1 .. 5 of 8 are rebuilt: n_keep = 6, first = 1
    "emcid_session_release_f64": (("emcid_session_release_workspace_bytes", (N, D, CAP)),
                                  (P, 6, 1, D, P, 128, P, CAP, P, CAP, 8, P, "WS", P, None), None, PLAIN),
    "emcid_session_step_norms_f64": (PRESERVE, (P, "WS", N, D, H, CAP, 3, P, P, P, None), None, PLAIN),
    "emcid_edit_dual_cols_stage1_f64": (DUAL, (P, P, P, N, D, H, 0.5, 1, 1.0, P, LAYERS, 0, TILES, 1, P, "WS", None), None, PLAIN),
    "emcid_edit_dual_cols_stage2_f64": (DUAL, (N, D, H, P, LAYERS, 0, TILES, 1, P, "WS", P, None), None, PLAIN),
}


def test_the_table_covers_the_solver_entries_with_a_size_function():
    """each *_workspace_bytes export of the fp64 solvers has at least one entry here that is sized by it"""
    sizers = {name for name in hip.EXPORTS if name.endswith("_workspace_bytes")} - {
        "emcid_linear_workspace_bytes", "emcid_gram_sp16_workspace_bytes", "emcid_clip_workspace_bytes"}
    assert sizers == {case[0][0] for case in CASES.values()}
    assert set(CASES) <= set(hip.EXPORTS)


@pytest.mark.parametrize("entry", sorted(CASES))
def test_a_workspace_eight_bytes_short_is_refused_by_name(entry):
    lib = hip.load()
    (size_fn, size_args), args, who, tail = CASES[entry]
    need = getattr(lib, size_fn)(*size_args)
    assert need > 8
    fn = getattr(lib, entry)
    assert len(args) == len(fn.argtypes)
    rc = fn(*[need - 8 if a == "WS" else a for a in args])
    assert rc == ERR_WORKSPACE
    assert lib.emcid_last_error().decode() == f"{who or entry}: {tail}"


@pytest.mark.parametrize("n_layers,d", [(1, 128), (4, 768), (4, 3072), (2, 5120), (3, 200)])
def test_cov_factor_workspace_is_three_squares_and_the_block_inverses_per_layer(n_layers, d):
    lib = hip.load()
    dp = -(-d // 128) * 128
    assert lib.emcid_inverse_workspace_doubles(dp) == -(-dp // 512) * (512 * 512 + 256 * 256)
    assert lib.emcid_cov_factor_workspace_bytes(n_layers, d) == 8 * n_layers * (3 * dp * dp + lib.emcid_inverse_workspace_doubles(dp))

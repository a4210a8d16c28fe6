"""CPU half of the fp64 GEMM tests: the oracle of test_gemm_f64_gpu.py (tests/gemm_f64_oracle.py) checked against a torch-fp64
stand-in of the kernel and against mutants of it, and the host-side argument checks of the three GEMM entry points (they return
before any HIP call, so no GPU is needed)."""
import numpy as np
import pytest
import torch

import gemm_f64_oracle as gx
from emcid_amd import hip

BAD_ARG, BAD_WORKSPACE = -1, -3       # EMCID_ERR_BAD_ARG, EMCID_ERR_WORKSPACE (include/emcid_hip.h)


def _run(pr, mode, flags, cfg, ta=0, mutant=None):
    pre = gx.prefill(pr, mode)
    got = gx.standin(pr.a, pr.b, pre, mode.alpha, mode.beta, flags, cfg, mode.ksplit, ta, mutant)
    ref, tol = gx.expected(pr, mode.alpha, mode.beta)
    return got, pre, ref, tol


def test_shapes_have_the_properties_the_cases_rely_on():
    c = gx._ceil
    assert (c(264, 128), c(264, 64), c(264, 32), c(264, 16)) == (3, 5, 9, 17)      # odd tile counts, a K ring of 4 that wraps
    assert (c(256, 128), c(256, 64), c(256, 32)) == (2, 4, 8)                       # even counts: every pair has two tiles
    assert c(gx.BIG_SHAPE[0], 128) * c(gx.BIG_SHAPE[1], 128) >= 512                 # the launcher's own 128 x 128 choice
    assert all(gx.resolve_cfg(M, N, -1, 0) == 2 and gx.resolve_cfg(M, N, -1, 1) == 1
               for f in gx.FLAGS for M, N, _ in gx.shapes_for(f, 0, 0))
    assert gx.resolve_cfg(*gx.BIG_SHAPE[:2], -1, 0) == 0
    # a 7-way split leaves empty splits at every K here, and an automatic split exists at K >= 256 only
    assert all(c(c(K, 16), 7) * 6 >= c(K, 16) for K in (264, 256, 151, 150, 144))
    assert {f for f in gx.FLAGS} == {0, 1, 2, 4, 8, 16, 5, 10, 33, 34, 36, 40, 32, 48} and len(gx.MODES) == 8


@pytest.mark.parametrize("flags", gx.FLAGS)
def test_standin_passes_the_oracle(flags):
    """Every shape, tile form and mode of the GPU test, on the stand-in: no element outside the bound, and under lower_only no
    element with m >= n that needs the "still holds its prefill" exemption."""
    lower = bool(flags & gx.LOWER)
    shapes = sorted(set(gx.shapes_for(flags, 0, 0)) | set(gx.shapes_for(flags, 1, 1)))
    for shape in shapes:
        pr = gx.problem(*shape, flags & 15)
        for cfg in (0, 1, 2):
            for mode in gx.MODES:
                got, pre, ref, tol = _run(pr, mode, flags, cfg)
                bad = gx.failures(got, pre, ref, tol, lower)
                assert not bad.any(), (shape, flags, cfg, mode, gx.describe(bad, got, pre, ref, tol))
                within, _ = gx.classify(got, pre, ref, tol)
                assert within[~gx.strictly_upper(*got.shape)].all(), (shape, flags, cfg, mode)
                if not lower:
                    assert within.all()


def test_standin_passes_on_the_big_tile_shape():
    M, N, K = gx.BIG_SHAPE
    pr = gx.make_problem(M, N, K, 0)
    mode = gx.Mode(-0.5, 2.0, 0, False)
    got, pre, ref, tol = _run(pr, mode, 0, -1)
    assert not gx.failures(got, pre, ref, tol, False).any()


def test_lower_only_leaves_skipped_tiles_alone_in_the_standin():
    """The exemption is used where it is meant to be: tiles wholly above the diagonal keep their prefill bits."""
    pr = gx.problem(264, 264, 264, 0)
    for mode in gx.MODES[:3]:
        got, pre, ref, tol = _run(pr, mode, gx.LOWER, 1)
        within, untouched = gx.classify(got, pre, ref, tol)
        assert untouched[:64, 64:].all() and not within[:64, 64:].any()
        assert not untouched[64:, :64].any()


MUTANTS = [
    # (mutant, flags, cfg, modes (indices into MODES))
    ("drop_k_tile", 0, 1, (0, 1, 2)),
    ("drop_k_tile", 0, 0, (1,)),
    ("tri_end_short", 1, 1, (0, 1)),          # the last column tile's K range ends at 264: 16 whole tiles and a ragged one
    ("tri_end_short", 4, 2, (0, 2)),
    ("tri_end_short", 2, 1, (1,)),
    ("tri_end_short", 8, 2, (1,)),
    ("swap_bits_1_2", 1, -1, (0,)),
    ("swap_bits_1_2", 2, -1, (1,)),
    ("swap_bits_1_2", 2 | gx.PAIR, 1, (2,)),
    ("transpose_tile", 0, 1, (0, 1)),
    ("transpose_tile", 0, 0, (0,)),
    ("beta_per_split", 0, 1, (2, 3, 4, 5, 6, 7)),
    ("pair_middle_twice", 1 | gx.PAIR, 1, (2, 4)),
    ("pair_middle_twice", 4 | gx.PAIR, 2, (2,)),
    ("pair_middle_twice", 8 | gx.PAIR, 0, (2,)),
    ("zero_upper_tile", gx.LOWER, 1, (0, 1, 2)),
    ("lower_tile_missing", gx.LOWER, 2, (0, 1, 2, 3)),
    ("lower_tile_missing", gx.LOWER, 0, (0,)),
]


@pytest.mark.parametrize("mutant,flags,cfg,modes", MUTANTS)
def test_oracle_catches_mutant(mutant, flags, cfg, modes):
    shape = (264, 264, 264)
    pr = gx.problem(*shape, flags & 15)
    lower = bool(flags & gx.LOWER)
    for mi in modes:
        mode = gx.MODES[mi]
        good = _run(pr, mode, flags, cfg)
        assert not gx.failures(*good, lower).any()
        bad_run = _run(pr, mode, flags, cfg, mutant=mutant)
        assert not torch.equal(gx.bits(bad_run[0]), gx.bits(good[0])), "the mutant changed nothing in this configuration"
        assert gx.failures(*bad_run, lower).any(), (mutant, flags, cfg, mode)


def test_bound_is_tight_enough_for_one_rounding_error_in_a_thousand():
    """Scale of the bound: an element moved by 1e-10 of its magnitude scale (a thousand times the bound at K = 264) fails."""
    pr = gx.problem(264, 264, 264, 0)
    mode = gx.MODES[1]
    got, pre, ref, tol = _run(pr, mode, 0, 1)
    assert float((tol / (pr.Pabs + pr.c0.abs())).max()) < 1e-13
    got[100, 7] += 1e-10 * float(pr.Pabs[100, 7])
    assert int(gx.failures(got, pre, ref, tol, False).sum()) == 1


# ---- argument rejection (host-side checks; nothing reaches a device) -------------------------------------------------------

@pytest.fixture(scope="module")
def ptrs():
    buf = np.zeros(16, dtype=np.float64)
    base = buf.ctypes.data
    ok = base + (-base) % 16
    return buf, ok, ok + 8


def _ex(lib, ptr, ta=0, tb=0, M=4, N=4, K=4, alpha=1.0, A="p", lda=4, B="p", ldb=4, beta=0.0, C="p", ldc=4, flags=0, cfg=-1, ksplit=0):
    pick = lambda v: ptr if v == "p" else v
    return lib.emcid_dgemm_ex_f64(ta, tb, M, N, K, alpha, pick(A), lda, pick(B), ldb, beta, pick(C), ldc, flags, cfg, ksplit, None)


def test_dgemm_ex_rejects_bad_arguments_without_gpu(ptrs):
    lib = hip.load()
    _, ok, odd = ptrs
    cases = [dict(flags=64), dict(cfg=3), dict(cfg=-2), dict(ksplit=2, beta=0.5), dict(ksplit=-2, beta=0.5), dict(lda=5), dict(ldb=5),
             dict(A=odd), dict(B=odd), dict(M=0), dict(N=0), dict(K=0), dict(C=None)]
    for kw in cases:
        assert _ex(lib, ok, **kw) == BAD_ARG, kw
        assert b"emcid_dgemm_ex_f64: bad argument" in lib.emcid_last_error(), kw


def _batched(lib, ptr, M=4, N=4, K=4, sA=16, sB=16, sC=16, batch=2):
    return lib.emcid_dgemm_batched_f64(0, 0, M, N, K, 1.0, ptr, 4, sA, ptr, 4, sB, 0.0, ptr, 4, sC, batch, None)


def test_dgemm_batched_rejects_bad_arguments_without_gpu(ptrs):
    lib = hip.load()
    _, ok, _ = ptrs
    for kw in (dict(batch=0), dict(batch=65536), dict(sA=15), dict(sC=-16)):
        assert _batched(lib, ok, **kw) == BAD_ARG, kw
        assert b"emcid_dgemm_batched_f64: bad argument" in lib.emcid_last_error(), kw


def _streamk(lib, ptr, M=256, N=256, K=64, flags=1, wgs=256, ws="p", ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.emcid_streamk_workspace_bytes(wgs) if wgs > 0 else 0
    return lib.emcid_dgemm_streamk_f64(0, M, N, K, 1.0, ptr, 64, ptr, 64, ptr, 256, flags, wgs, 0.0, ptr if ws == "p" else ws, ws_bytes, None)


def test_dgemm_streamk_rejects_bad_arguments_without_gpu(ptrs):
    lib = hip.load()
    _, ok, _ = ptrs
    for kw in (dict(flags=16, M=256, N=128), dict(flags=16 | 1), dict(flags=0), dict(wgs=0), dict(wgs=4097)):
        assert _streamk(lib, ok, **kw) == BAD_ARG, kw
        assert b"emcid_dgemm_streamk_f64: bad argument" in lib.emcid_last_error(), kw
    need = lib.emcid_streamk_workspace_bytes(256)
    assert need == (2 * 256 * 128 * 128 + 8192) * 8
    assert _streamk(lib, ok, ws_bytes=need - 1) == BAD_WORKSPACE
    assert b"workspace too small" in lib.emcid_last_error()
    assert _streamk(lib, ok, flags=16, ws_bytes=need - 1) == BAD_WORKSPACE      # the lower-only form asks for the same workspace

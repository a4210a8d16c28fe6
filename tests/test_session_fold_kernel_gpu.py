"""Folding a preserved key set into a base factor (emcid_cov_factor_fold_f64, include/emcid_hip.h) through the C ABI, no encoder:
after a fold the workspace holds the factor of lam C' + P^T P (P: the keys of the folded steps), its block inverses and its explicit
inverse, and a step on it with an empty state solves the system a never-folding session solves.  The references are formed here, on
the CPU in fp64: numpy's Cholesky of the primal matrix and torch.linalg.solve on it.

The input recipe of tests/session_kernel_helpers.py (d = 384, h = 96, lam = 50, edit_weight 0.6, nearly collinear rows, Cov with a
1 600 condition number).  The same algebra on the CPU in fp64 gives L' within 6e-16 .. 7e-16 and U within 3e-15 .. 2e-13 of these
references, six to seven orders inside the bars; the values the MI355X gives are in DESIGN.md §3."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import hip
from session_kernel_helpers import D, DEV, EW, H, LAM, LEFT, L_BAR, U_BAR, _inputs, _primal_matrix, _primal_u


def _step(inp, lo, n, fac, state):
    K, Zc, zs_t, Cov, W0 = inp
    W = torch.empty(H, K.shape[1], dtype=torch.float32, device=DEV)
    res = hip.edit_layer_dual_preserve(K[lo:lo + n].contiguous().to(DEV), Zc[lo:lo + n].contiguous().to(DEV),
                                       zs_t[lo:lo + n].contiguous().to(DEV), fac, 0, EW, LEFT, W0.to(DEV), W, state, want_u=True,
                                       lam=LAM)
    assert int(res["ws"].info.item()) == 0 and int(fac.info.item()) == 0
    state.commit(n)
    return res["U"].cpu()


def _fold(src, state, cov, dst=None, base=None):
    """One fold of the state's rows; a first fold (no dst) makes the workspace and the accumulator and fills it from ``cov``."""
    first = dst is None
    if first:
        dst = hip.CovFactors(1, src.d, DEV)
        base = torch.empty(1, dst.dp, dst.dp, dtype=torch.float64, device=DEV)
    hip.cov_factor_fold(src, state, 0, cov if first else None, LAM, EW, dst, base)
    return dst, base


def _factor_checks(dst, A, d=D):
    """(error of L' against numpy's Cholesky of A relative to its largest entry, max |X' L' - I|)"""
    Lref = torch.from_numpy(np.linalg.cholesky(A.numpy()))
    Lgot = torch.tril(dst.L(0).cpu())
    Xgot = torch.tril(dst.X(0).cpu())
    lerr = (Lgot[:d, :d] - Lref).abs().max().item() / Lref.abs().max().item()
    ierr = (Xgot @ Lgot - torch.eye(dst.dp, dtype=torch.float64)).abs().max().item()
    if dst.dp > d:       # the padding: identity, decoupled
        assert torch.equal(Lgot[d:, :d], torch.zeros(dst.dp - d, d, dtype=torch.float64))
        assert torch.equal(Lgot[d:, d:], torch.eye(dst.dp - d, dtype=torch.float64))
    return lerr, ierr


@functools.lru_cache(maxsize=None)
def _scenario(lam0):
    """Steps (130, 70) on factors made with ``lam0`` at the session's lam = 50, a fold of the 200 rows, then a step of 129 rows on
    the folded workspace with the state emptied.  Run once per lam0, shared by the tests below."""
    inp = _inputs(329)
    cov = inp[3].to(DEV)
    src = hip.factor_cov([cov], lam0, EW)
    state = hip.PreservedKeys(1, D, 207, DEV)
    _step(inp, 0, 130, src, state)
    _step(inp, 130, 70, src, state)
    before = src.buf.clone()
    dst, base = _fold(src, state, cov)
    info = int(dst.info.item())
    same = torch.equal(src.buf, before)
    checks = _factor_checks(dst, _primal_matrix(*inp[:4], 200))
    state.reset()
    U = _step(inp, 200, 129, dst, state)
    return {"info": info, "src_untouched": same, "lerr": checks[0], "ierr": checks[1], "U": U, "lam": dst.lam,
            "have_inverse": set(dst.have_inverse), "cached": dst.cached}


@functools.lru_cache(maxsize=None)
def _unfolded_u():
    """The same three steps on one state that never folds (capacity 336): U of the last one."""
    inp = _inputs(329)
    src = hip.factor_cov([inp[3].to(DEV)], LAM, EW)
    state = hip.PreservedKeys(1, D, 336, DEV)
    _step(inp, 0, 130, src, state)
    _step(inp, 130, 70, src, state)
    return _step(inp, 200, 129, src, state)


@pytest.mark.parametrize("lam0", [LAM, 20.0], ids=["lam_ratio=1", "lam_ratio=2.5"])
def test_fold_gives_the_factor_of_the_primal_matrix(lam0):
    """Cases 1 and 3: M = 200 crosses a 128 tile.  L' against numpy's Cholesky of lam C' + Kt[:200]^T Kt[:200], X' L' = I, info 0,
    the source workspace (a factor-cache entry in the product) byte for byte as before — also with the source factored at
    another lam (20 against the session's 50), where the keys come back through sqrt(lam_ratio) L."""
    s = _scenario(lam0)
    print(f"lam0 {lam0}: L' error {s['lerr']:.3e} of max|L'|, max|X' L' - I| {s['ierr']:.3e}")
    assert s["info"] == 0
    assert s["src_untouched"]
    assert s["lerr"] <= L_BAR
    assert s["ierr"] <= 1e-9
    assert s["lam"] == LAM and s["have_inverse"] == {0} and s["cached"] is False


@pytest.mark.parametrize("lam0", [LAM, 20.0], ids=["lam_ratio=1", "lam_ratio=2.5"])
def test_step_after_the_fold(lam0):
    """Cases 2 and 3: a step of 129 rows on the folded workspace with an empty state (M = 0): U against the primal solve with all
    329 rows in the system, and against the same three steps run unfolded with capacity 336."""
    inp = _inputs(329)
    ref = _primal_u(*inp[:4], 200, 329)
    scale = ref.abs().max().item()
    got = _scenario(lam0)["U"]
    err = (got - ref).abs().max().item() / scale
    gap = (got - _unfolded_u()).abs().max().item() / scale
    print(f"lam0 {lam0}: U after the fold: error {err:.3e} of max|U| against the primal solve, {gap:.3e} against the unfolded steps")
    assert err <= U_BAR
    assert gap <= U_BAR


def test_two_folds_in_a_row():
    """Case 4: steps (5), fold, (3), fold in place (src is dst), (4): the last U against the primal solve on 12 rows."""
    inp = _inputs(12)
    cov = inp[3].to(DEV)
    src = hip.factor_cov([cov], LAM, EW)
    state = hip.PreservedKeys(1, D, 8, DEV)
    _step(inp, 0, 5, src, state)
    dst, base = _fold(src, state, cov)
    state.reset()
    _step(inp, 5, 3, dst, state)
    again, _ = _fold(dst, state, None, dst, base)
    assert again is dst and int(dst.info.item()) == 0
    lerr, ierr = _factor_checks(dst, _primal_matrix(*inp[:4], 8))
    state.reset()
    U = _step(inp, 8, 4, dst, state)
    ref = _primal_u(*inp[:4], 8, 12)
    err = (U - ref).abs().max().item() / ref.abs().max().item()
    print(f"two folds: L' error {lerr:.3e}, max|X' L' - I| {ierr:.3e}, U error {err:.3e} of max|U|")
    assert lerr <= L_BAR and ierr <= 1e-9
    assert err <= U_BAR


def test_fold_at_the_edge_of_a_tile():
    """Case 5: steps (127, 2): M = 129, one row past a 128 tile; the factor, and a step of 3 rows after the fold."""
    inp = _inputs(132)
    cov = inp[3].to(DEV)
    src = hip.factor_cov([cov], LAM, EW)
    state = hip.PreservedKeys(1, D, 129, DEV)
    _step(inp, 0, 127, src, state)
    _step(inp, 127, 2, src, state)
    dst, _ = _fold(src, state, cov)
    assert int(dst.info.item()) == 0
    lerr, ierr = _factor_checks(dst, _primal_matrix(*inp[:4], 129))
    state.reset()
    U = _step(inp, 129, 3, dst, state)
    ref = _primal_u(*inp[:4], 129, 132)
    err = (U - ref).abs().max().item() / ref.abs().max().item()
    print(f"M = 129: L' error {lerr:.3e}, max|X' L' - I| {ierr:.3e}, U error {err:.3e} of max|U|")
    assert lerr <= L_BAR and ierr <= 1e-9
    assert err <= U_BAR


def test_fold_with_padding():
    """d = 200 (dp = 256): the folded factor against numpy's Cholesky, its padding rows and columns the identity's, as
    emcid_factor_cov_f64 leaves them, and a step after the fold against the same step on the unfolded state.  (Against the primal
    solve the step entry itself sits 0.7e-7 .. 1.8e-7 of max|U| away at this d, with or without a fold — d = 256 and 384: 1e-13 —
    which is the step's matter, not the fold's: the figure is printed, the fold is held to what it changes.)"""
    d = 200
    inp = _inputs(12, d)
    cov = inp[3].to(DEV)
    src = hip.factor_cov([cov], LAM, EW)
    state = hip.PreservedKeys(1, d, 12, DEV)
    _step(inp, 0, 5, src, state)
    _step(inp, 5, 3, src, state)
    dst, _ = _fold(src, state, cov)
    assert int(dst.info.item()) == 0
    lerr, ierr = _factor_checks(dst, _primal_matrix(*inp[:4], 8), d)
    unfolded = _step(inp, 8, 4, src, state)
    state.reset()
    U = _step(inp, 8, 4, dst, state)
    ref = _primal_u(*inp[:4], 8, 12)
    gap = (U - unfolded).abs().max().item() / ref.abs().max().item()
    err = (U - ref).abs().max().item() / ref.abs().max().item()
    print(f"d = 200: L' error {lerr:.3e}, max|X' L' - I| {ierr:.3e}, U after the fold {gap:.3e} of max|U| from the unfolded step "
          f"({err:.3e} from the primal solve)")
    assert lerr <= L_BAR and ierr <= 1e-9
    assert gap <= U_BAR


def test_argument_errors_launch_nothing():
    """Case 6: layer_index out of range, M = 0, M > capacity, src == dst with lam_ratio != 1 return EMCID_ERR_BAD_ARG (-1) and a
    workspace that is too small returns the library's status for exactly that argument, EMCID_ERR_WORKSPACE (-3), as in every
    other entry that takes a workspace; none of them writes dst, base or src."""
    inp = _inputs(12)
    cov = inp[3].to(DEV)
    src = hip.factor_cov([cov], LAM, EW)
    state = hip.PreservedKeys(1, D, 8, DEV)
    _step(inp, 0, 5, src, state)
    dst = hip.CovFactors(1, D, DEV)
    dp = dst.dp
    base = torch.full((dp, dp), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(8 * dp, dtype=torch.float64, device=DEV)
    lib = hip.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.emcid_cov_factor_fold_workspace_bytes(5, D) == 5 * dp * 8

    def call(src_buf=src.buf, ratio=1.0, M=5, capacity=8, dst_buf=dst.buf, layer=0, ws_bytes=ws.numel() * 8):
        return lib.emcid_cov_factor_fold_f64(p(src_buf), ratio, p(state.Yp[0]), state.Yp[0].stride(0), M, capacity, p(cov), LAM, EW, 1,
                                             p(dst_buf), 1, D, layer, p(base), p(ws), ws_bytes, p(dst.info), stream)

    keep = [t.clone() for t in (src.buf, dst.buf, base, ws)]
    assert call(layer=1) == -1 and call(layer=-1) == -1
    assert call(M=0) == -1
    assert call(M=9) == -1
    assert call(dst_buf=src.buf, ratio=2.5) == -1
    assert call(ws_bytes=5 * dp * 8 - 8) == -3
    assert b"workspace" in lib.emcid_last_error()
    torch.cuda.synchronize()
    for t, k in zip((src.buf, dst.buf, base, ws), keep):
        assert torch.equal(t, k)
    assert int(dst.info.item()) == 0
    # the binding refuses a workspace of the factor cache as a target, whichever way round
    src.cached = True
    with pytest.raises(hip.EmcidHipError, match="cache"):
        hip.cov_factor_fold(src, state, 0, cov, LAM, EW, src, base.view(1, dp, dp))
    with pytest.raises(hip.EmcidHipError, match="layer"):
        hip.cov_factor_fold(src, state, 1, cov, LAM, EW, dst, base.view(1, dp, dp))
    assert call() == 0 and int(dst.info.item()) == 0        # and the same arguments, all in range, go through

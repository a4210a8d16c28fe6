"""emcid_session_retain_f64 and emcid_session_step_norms_f64 (include/emcid_hip.h) through the binding, no encoder: a retain list
must append exactly the rows a preserve step with a zero residual appends — Yk = Kt X^T, [Lkp Lkk] of chol(I + Y Y^T), the touched
tile inverses — without touching rows below M, and the norms must be those of dW p_i = -Zp_i, Zk_j = Rt_j - dW Kt_j and Rt_j.
The references are formed here, on the CPU in fp64.  Inputs and bars are those of tests/session_kernel_helpers.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import hip
from session_kernel_helpers import DEV, EW, H, LAM, LEFT, L_BAR, U_BAR, _cp, _dev, _inputs_by_width as _inputs, _retain, _scale, _step

SAME = 1e-13                       # two fp64 chains over the same launches, relative to the largest entry
CASES = [(0, 5), (5, 3), (130, 70), (200, 129)]      # one tile; a tile boundary inside the append; a last partial tile


def _y_ref(K, Cov, scale):
    Lc = torch.linalg.cholesky(LAM * _cp(Cov))
    return torch.linalg.solve_triangular(Lc, (scale * K.double()).t(), upper=False).t()          # Kt L^-T


def _check_state(state, total, M, d, Yref):
    Y = state.Yp[0][:total].cpu()
    yerr = (Y[:, :d] - Yref).abs().max().item() / Yref.abs().max().item()
    Lref = torch.from_numpy(np.linalg.cholesky((torch.eye(total, dtype=torch.float64) + Y @ Y.t()).numpy()))
    Lgot = state.Lp[0][:total, :total].cpu()
    lerr = (Lgot - Lref).abs().max().item()
    print(f"M={M} N={total - M} d={d}: Yk error {yerr:.3e} of max|Y|, factor error {lerr:.3e}")
    assert yerr <= U_BAR
    assert torch.equal(Y[:, d:], torch.zeros_like(Y[:, d:]))               # the padding columns of the appended rows
    torch.testing.assert_close(Lgot, Lref, rtol=L_BAR, atol=L_BAR)
    for J in range((total + 127) // 128):
        w = min(128, total - 128 * J)
        blk = Lref[128 * J:128 * J + w, 128 * J:128 * J + w]
        inv = state.tile_inv[0][J, :w, :w].cpu()
        assert (inv @ blk - torch.eye(w, dtype=torch.float64)).abs().max().item() < 1e-9, J
        assert torch.equal(torch.triu(inv, 1), torch.zeros_like(inv))


@pytest.mark.parametrize("M,N", CASES, ids=[f"{m}+{n}" for m, n in CASES])
def test_retained_rows_vs_numpy(M, N):
    """After retain and commit: Lp[:M + N] is numpy's Cholesky factor of I + Y Y^T, Yk = Kt X^T against the CPU's triangular solve,
    every touched tile inverse times its tile is the identity, and rows below M are byte-identical.  The M earlier rows are a
    retain list of their own at weight 4, the N new ones go in at weight 1."""
    total = M + N
    K, _, _, Cov, _ = _inputs(total)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = hip.PreservedKeys(1, 384, total + 7, DEV)
    if M:
        assert _retain(K[:M], fac, state, weight=4.0) == 0
    assert state.M == M
    before = [t.clone() for t in (state.Yp[0], state.Lp[0], state.tile_inv[0])]
    assert _retain(K[M:], fac, state, commit=False) == 0
    assert state.M == M                                   # the entry commits nothing by itself
    state.commit(N, hip.row_scale_of(EW, fac, LAM))
    assert int(fac.info.item()) == 0
    assert torch.equal(state.Yp[0][:M], before[0][:M]) and torch.equal(state.Lp[0][:M], before[1][:M])
    full = M // 128                                       # tiles wholly below row M, and the rows < M of the tile M lies in
    assert torch.equal(state.tile_inv[0][:full], before[2][:full])
    assert torch.equal(state.tile_inv[0][full, :M - 128 * full], before[2][full, :M - 128 * full])
    Yref = torch.cat([_y_ref(K[:M], Cov, _scale(4.0)), _y_ref(K[M:], Cov, _scale())])
    _check_state(state, total, M, 384, Yref)
    assert state.row_scale[:total].tolist() == [_scale(4.0)] * M + [_scale()] * N


def test_weight_is_a_row_scale():
    """Retaining K at weight 4 and 2 K at weight 1 leave the same rows (2 K is exact in fp32; the two scales differ by the rounding
    of one square root)."""
    M, N = 5, 3
    K, _, _, Cov, _ = _inputs(M + N)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    rows = []
    for Kn, w in ((K[M:], 4.0), (2.0 * K[M:], 1.0)):
        state = hip.PreservedKeys(1, 384, 16, DEV)
        assert _retain(K[:M], fac, state) == 0
        assert _retain(Kn, fac, state, weight=w) == 0
        rows.append((state.Yp[0][M:M + N].cpu(), state.Lp[0][M:M + N, :M + N].cpu(), state.tile_inv[0][0, :M + N, :M + N].cpu()))
    for a, b, what in zip(rows[0], rows[1], ("Yk", "[Lkp Lkk]", "tile inverse")):
        err = (a - b).abs().max().item() / b.abs().max().item()
        print(f"{what}: weight 4 vs doubled keys {err:.3e}")
        assert err <= SAME, what


@pytest.mark.parametrize("M,N", [(5, 3), (130, 70)], ids=["5+3", "130+70"])
def test_retain_is_a_preserve_step_with_a_zero_residual(M, N):
    """The rows retain appends are those of emcid_edit_layer_dual_preserve_f64 with zs_t = Zc — and that step leaves W == W0."""
    total = M + N
    K, Zc, _, Cov, W0 = _inputs(total)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    a, b = hip.PreservedKeys(1, 384, total, DEV), hip.PreservedKeys(1, 384, total, DEV)
    assert _retain(K[:M], fac, a) == 0 and _retain(K[M:], fac, a) == 0
    for lo, hi in ((0, M), (M, total)):
        res = _step(K[lo:hi], Zc[lo:hi], Zc[lo:hi], W0, fac, b)
        assert torch.equal(res["W"].cpu(), W0)
        assert torch.equal(res["U"], torch.zeros_like(res["U"]))
        b.commit(hi - lo)
    for x, y, what in ((a.Yp[0], b.Yp[0], "Yk"), (a.Lp[0], b.Lp[0], "[Lkp Lkk]"), (a.tile_inv[0], b.tile_inv[0], "tile inverses")):
        err = (x - y).abs().max().item() / y.abs().max().item()
        print(f"{M}+{N} {what}: retain vs zero-residual step {err:.3e}")
        assert err <= SAME, what


@pytest.mark.parametrize("weight", [1.0, 4.0])
def test_step_after_retain_vs_primal_fp64(weight):
    """An edit step after a retain list: U against torch.linalg.solve on lam C' + P^T P + Kt^T Kt, P the scaled retained rows."""
    M, N = 130, 70
    K, Zc, zs_t, Cov, W0 = _inputs(M + N)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = hip.PreservedKeys(1, 384, M + N + 7, DEV)
    assert _retain(K[:M], fac, state, weight=weight) == 0
    res = _step(K[M:], Zc[M:], zs_t[M:], W0, fac, state)
    P = _scale(weight) * K[:M].double()
    Kt, Rt = _scale() * K[M:].double(), (_scale() * (zs_t[M:] - Zc[M:]).double()) / LEFT
    ref = torch.linalg.solve(LAM * _cp(Cov) + P.t() @ P + Kt.t() @ Kt, Kt.t() @ Rt).t()
    err = (res["U"].cpu() - ref).abs().max().item() / ref.abs().max().item()
    print(f"weight {weight}: U after a retain list, error {err:.3e} of max|U|")
    assert err <= U_BAR
    assert (res["W"].cpu() - (W0 + ref.float())).abs().max().item() <= 1e-6 * max(ref.abs().max().item(), 1.0)


def test_padded_width_rows_and_the_following_step():
    """d = 200 (dp = 256): the factor rows, and the step after the retain list against the step after the SAME rows entered by
    zero-residual preserve steps (not against the primal solve: DESIGN.md §3 records an offset of the step at this d)."""
    d, M, N = 200, 130, 70
    K, Zc, zs_t, Cov, W0 = _inputs(M + N, d)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    a, b = hip.PreservedKeys(1, d, M + N, DEV), hip.PreservedKeys(1, d, M + N, DEV)
    assert _retain(K[:5], fac, a) == 0 and _retain(K[5:M], fac, a) == 0
    _check_state(a, M, 5, d, _y_ref(K[:M], Cov, _scale()))
    for lo, hi in ((0, 5), (5, M)):
        _step(K[lo:hi], Zc[lo:hi], Zc[lo:hi], W0, fac, b)
        b.commit(hi - lo)
    ua = _step(K[M:], Zc[M:], zs_t[M:], W0, fac, a)["U"].cpu()
    ub = _step(K[M:], Zc[M:], zs_t[M:], W0, fac, b)["U"].cpu()
    err = (ua - ub).abs().max().item() / ub.abs().max().item()
    print(f"d = 200: step after retain vs step after zero-residual steps {err:.3e} of max|U|")
    assert err <= U_BAR


def test_indefinite_schur_complement_reports_and_keeps_the_state():
    """Lp spoiled as in tests/test_session_kernel_gpu.py (far too small, so T has a negative pivot: wrong input, not a fault):
    the flag is non-zero, rows < M are unchanged, and the same call passes once the state is put right."""
    M, N = 5, 3
    K, _, _, Cov, _ = _inputs(M)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = hip.PreservedKeys(1, 384, 16, DEV)
    assert _retain(K, fac, state) == 0
    g = torch.Generator().manual_seed(7)
    K2 = (K[:N] + 0.05 * torch.randn(N, 384, generator=g)).contiguous()        # close to preserved keys: B is not small
    good = (state.Lp[0].clone(), state.tile_inv[0].clone())
    state.Lp[0][:M] *= 1e-3
    state.tile_inv[0][0, :M] *= 1e3
    before = [t.clone() for t in (state.Yp[0], state.Lp[0], state.tile_inv[0])]
    assert _retain(K2, fac, state) != 0
    assert state.M == M
    assert torch.equal(state.Yp[0][:M], before[0][:M]) and torch.equal(state.Lp[0][:M], before[1][:M])
    assert torch.equal(state.tile_inv[0][0, :M], before[2][0, :M])
    state.Lp[0][:M].copy_(good[0][:M])
    state.tile_inv[0][0, :M].copy_(good[1][0, :M])
    assert _retain(K2, fac, state) == 0
    assert state.M == M + N
    Yref = torch.cat([_y_ref(K, Cov, _scale()), _y_ref(K2, Cov, _scale())])
    _check_state(state, M + N, M, 384, Yref)


def test_capacity_and_inverse_are_checked_by_the_binding():
    K, _, _, Cov, _ = _inputs(8)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = hip.PreservedKeys(1, 384, 6, DEV)
    assert _retain(K[:5], fac, state) == 0
    with pytest.raises(hip.EmcidHipError, match="capacity"):
        hip.session_retain(_dev(K[5:8]), fac, 0, _scale(), state)
    with pytest.raises(hip.EmcidHipError, match="row_scale"):
        hip.session_retain(_dev(K[5:6]), fac, 0, 0.0, state)
    with pytest.raises(hip.EmcidHipError, match="layer index"):
        hip.session_retain(_dev(K[5:6]), fac, 1, _scale(), state)
    bare = hip.factor_cov([_dev(Cov)], LAM, EW, inverse=False)
    with pytest.raises(hip.EmcidHipError, match="inverse"):
        hip.session_retain(_dev(K[5:6]), bare, 0, _scale(), state)
    assert state.M == 5


@pytest.mark.parametrize("M,N", [(0, 5), (5, 3), (130, 70)], ids=["0+5", "5+3", "130+70"])
def test_step_norms_vs_cpu(M, N):
    """drift = ||U P_i^T|| from U_out (dW p_i = -Zp_i), left = ||Rt_j - U Kt_j^T||, resid = ||Rt_j||, row by row, each within 1e-8
    of the largest value; M = 0 runs with a null drift_out.  The M preserved rows are a retain list at weight 4."""
    total = M + N
    K, Zc, zs_t, Cov, W0 = _inputs(total)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = hip.PreservedKeys(1, 384, total + 7, DEV)
    if M:
        assert _retain(K[:M], fac, state, weight=4.0) == 0
    res = _step(K[M:], Zc[M:], zs_t[M:], W0, fac, state)
    out = torch.full((M + 2 * N + 3,), -1.0, dtype=torch.float64, device=DEV)
    norms = hip.session_step_norms(res["ws"], N, 384, H, state, out=out)
    assert norms["drift"].shape == (M,) and norms["left"].shape == (N,) and norms["resid"].shape == (N,)
    assert torch.equal(out[M + 2 * N:].cpu(), torch.full((3,), -1.0, dtype=torch.float64))      # nothing past the outputs
    U = res["U"].cpu()
    Kt, Rt = _scale() * K[M:].double(), (_scale() * (zs_t[M:] - Zc[M:]).double()) / LEFT
    refs = {"drift": (U @ (_scale(4.0) * K[:M].double()).t()).norm(dim=0), "left": (Rt - Kt @ U.t()).norm(dim=1),
            "resid": Rt.norm(dim=1)}
    for name, ref in refs.items():
        got = norms[name].cpu()
        if ref.numel():
            err = (got - ref).abs().max().item() / ref.max().item()
            print(f"{M}+{N} {name}: error {err:.3e} of the largest ({ref.max().item():.3e})")
            assert err <= U_BAR, name
    if M:       # in raw-key units: ||dW k_i|| = drift_i / row_scale_i
        raw = (U @ K[:M].double().t()).norm(dim=0)
        assert ((norms["drift"].cpu() / state.row_scale[:M]) - raw).abs().max().item() <= U_BAR * raw.max().item()
    fresh = hip.session_step_norms(res["ws"], N, 384, H, state)             # the binding's own buffer
    assert torch.equal(fresh["left"], norms["left"]) and torch.equal(fresh["resid"], norms["resid"])
    with pytest.raises(hip.EmcidHipError, match="workspace"):
        hip.session_step_norms(res["ws"], N + 1, 384, H, state)

"""The dual solver with a preserved key set (emcid_edit_layer_dual_preserve_f64, include/emcid_hip.h) through the C ABI, no encoder:
a later step must solve against A = lam C' + P^T P + Kt^T Kt, P the stacked keys of the earlier steps, and append [Lkp Lkk] to the
state's Cholesky factor.  The reference is formed here, on the CPU in fp64, from the primal system."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import hip
from session_kernel_helpers import D, DEV, EW, H, LAM, LEFT, L_BAR, U_BAR, _inputs, _primal_u, _scaled


def _dual_u(K, Zc, zs_t, Cov, lo, hi):
    """The same update from the stacked dual system, on the CPU in fp64 (the second reference of the spread below)."""
    Kt, Rt = _scaled(K, Zc, zs_t)
    Cp = ((Cov * (1 - EW)) / 0.5).double()
    Lc = torch.linalg.cholesky(LAM * Cp)
    Y = torch.linalg.solve_triangular(Lc, Kt[:hi].t(), upper=False).t()          # Kt L^-T
    rhs = torch.zeros(hi, H, dtype=torch.float64)
    rhs[lo:] = Rt[lo:hi]
    Z = torch.linalg.solve(torch.eye(hi, dtype=torch.float64) + Y @ Y.t(), rhs)
    return torch.linalg.solve_triangular(Lc.t(), (Z.t() @ Y).t(), upper=True).t()        # (Z^T Y) L^-1


def _run_steps(steps, capacity, fac=None, state=None):
    """Runs the entry for consecutive steps of the given sizes; returns (state, fac, [result of every step], inputs)."""
    total = sum(steps)
    K, Zc, zs_t, Cov, W0 = _inputs(total)
    fac = fac or hip.factor_cov([Cov.to(DEV)], LAM, EW)
    state = state or hip.PreservedKeys(1, D, capacity, DEV)
    outs, lo = [], 0
    W0d = W0.to(DEV)
    for n in steps:
        W = torch.empty(H, D, dtype=torch.float32, device=DEV)
        res = hip.edit_layer_dual_preserve(K[lo:lo + n].contiguous().to(DEV), Zc[lo:lo + n].contiguous().to(DEV),
                                           zs_t[lo:lo + n].contiguous().to(DEV), fac, 0, EW, LEFT, W0d, W, state, want_u=True)
        assert int(res["ws"].info.item()) == 0 and int(fac.info.item()) == 0
        res["W"] = W
        outs.append(res)
        state.commit(n)
        lo += n
    return state, fac, outs, (K, Zc, zs_t, Cov, W0)


@pytest.mark.parametrize("steps", [(5,), (5, 3), (130, 70), (200, 129)], ids=lambda s: "+".join(map(str, s)))
def test_preserved_step_vs_primal_fp64(steps):
    """(M, N) = (0, 5), (5, 3), (130, 70) — crosses a 128 tile in M and in M + N — and (200, 129); the M > 0 states come from
    the entry's own earlier steps.  U of the last step against torch.linalg.solve on lam C' + P^T P + Kt^T Kt, the appended rows
    [Lkp Lkk] against numpy's Cholesky of I + Y Y^T of the stacked rows.

    Reference-vs-reference spread for these inputs (primal solve against the stacked dual solve, both CPU fp64, relative to
    max|U|): 5: 1.4e-13, 5+3: 1.8e-13, 130+70: 3.5e-14, 200+129: 9.1e-14 — ten times that is still four orders below the 1e-8 bar
    of the existing solve-vs-oracle tests, so that bar is kept as it is for the nearly collinear rows too."""
    total, M, N = sum(steps), sum(steps[:-1]), steps[-1]
    state, fac, outs, (K, Zc, zs_t, Cov, W0) = _run_steps(steps, capacity=total + 7)
    assert state.M == total
    ref = _primal_u(K, Zc, zs_t, Cov, M, total)
    spread = (ref - _dual_u(K, Zc, zs_t, Cov, M, total)).abs().max().item() / ref.abs().max().item()
    got = outs[-1]["U"].cpu()
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print(f"steps {steps}: U error {err:.3e} of max|U| (CPU primal-vs-dual spread {spread:.3e})")
    assert err <= U_BAR, (err, spread)
    # the weights: W0 + float(U)
    assert (outs[-1]["W"].cpu() - (W0 + ref.float())).abs().max().item() <= 1e-6 * max(ref.abs().max().item(), 1.0)
    assert (outs[-1]["dW"].cpu().double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item() + 1e-12
    # the state: Yp rows verbatim = Kt X^T, Lp = chol(I + Yp Yp^T) with the step's rows appended
    Y = state.Yp[0][:total].cpu()
    Lref = torch.from_numpy(np.linalg.cholesky((torch.eye(total, dtype=torch.float64) + Y @ Y.t()).numpy()))
    Lgot = state.Lp[0][:total, :total].cpu()
    lerr = (Lgot[M:] - Lref[M:]).abs().max().item()
    print(f"steps {steps}: appended [Lkp Lkk] error {lerr:.3e}")
    torch.testing.assert_close(Lgot[M:], Lref[M:], rtol=L_BAR, atol=L_BAR)
    torch.testing.assert_close(Lgot, Lref, rtol=L_BAR, atol=L_BAR)
    Kt, _ = _scaled(K, Zc, zs_t)
    Lc = torch.linalg.cholesky(LAM * ((Cov * (1 - EW)) / 0.5).double())
    Yref = torch.linalg.solve_triangular(Lc, Kt.t(), upper=False).t()
    assert (Y[:, :D] - Yref).abs().max().item() <= U_BAR * Yref.abs().max().item()
    # the kept inverses of the diagonal 128-tiles, the partial last one included
    for J in range((total + 127) // 128):
        w = min(128, total - 128 * J)
        blk = Lref[128 * J:128 * J + w, 128 * J:128 * J + w]
        inv = state.tile_inv[0][J, :w, :w].cpu()
        assert (inv @ blk - torch.eye(w, dtype=torch.float64)).abs().max().item() < 1e-9
        assert torch.equal(torch.triu(inv, 1), torch.zeros_like(inv))


def test_first_step_is_the_plain_dual_stage():
    """M = 0 is today's dual stage: the same weights as edit_layer_dual_apply on the same inputs.  edit_layer_dual_apply hands out
    no fp64 U (it writes float(U) straight into W and dW), so the tightest comparison its binding allows is the fp32 one: the two
    chains sum in another order, fp64 rounding apart, and their dW / W agree to the fp32 rounding of dW — 2e-7 of the scale, the
    constant tests/test_kernels_gpu.py uses between two runs of the dual stage.  The fp64 U of the new entry is held to the
    primal solve at the fp64 bar."""
    N = 70
    K, Zc, zs_t, Cov, W0 = _inputs(N)
    fac = hip.factor_cov([Cov.to(DEV)], LAM, EW)
    Kd, Zd, zd, W0d = K.to(DEV), Zc.to(DEV), zs_t.to(DEV), W0.to(DEV)
    Wa, Wb = torch.empty(H, D, device=DEV), torch.empty(H, D, device=DEV)
    a = hip.edit_layer_dual_apply(Kd, Zd, zd, fac, 0, EW, LEFT, W0d, Wa)
    state = hip.PreservedKeys(1, D, 100, DEV)
    b = hip.edit_layer_dual_preserve(Kd, Zd, zd, fac, 0, EW, LEFT, W0d, Wb, state, want_u=True)
    assert int(a["ws"].info.item()) == 0 and int(b["ws"].info.item()) == 0
    scale = a["dW"].abs().max().item()
    assert (a["dW"] - b["dW"]).abs().max().item() <= 2e-7 * scale
    assert (Wa - Wb).abs().max().item() <= 2e-7 * max(scale, 1.0)
    ref = _primal_u(K, Zc, zs_t, Cov, 0, N)
    assert (b["U"].cpu() - ref).abs().max().item() <= U_BAR * ref.abs().max().item()
    assert state.M == 0          # the entry commits nothing by itself


def test_indefinite_schur_complement_reports_and_keeps_the_state():
    """A state whose Lp is wrong — far too small, so that Lkp = B Lp^-T is far too large and T = I + Yk Yk^T - Lkp Lkp^T has a
    negative pivot (wrong input, not a fault): info != 0, and rows < M of Yp / Lp (and of the tile inverses) bit-identical."""
    state, fac, _, (K, Zc, zs_t, Cov, W0) = _run_steps((5,), capacity=16)
    M, N = 5, 3
    g = torch.Generator().manual_seed(7)
    K2 = (K[:N] + 0.05 * torch.randn(N, D, generator=g)).contiguous()         # close to preserved keys: B is not small
    state.Lp[0][:M] *= 1e-3
    state.tile_inv[0][0, :M] *= 1e3
    before = [t.clone() for t in (state.Yp[0], state.Lp[0], state.tile_inv[0])]
    W0d = W0.to(DEV)
    W = W0d.clone()
    res = hip.edit_layer_dual_preserve(K2.to(DEV), Zc[:N].contiguous().to(DEV), zs_t[:N].contiguous().to(DEV), fac, 0, EW, LEFT,
                                       W0d, W, state)
    assert int(res["ws"].info.item()) != 0
    assert state.M == M
    assert torch.equal(state.Yp[0][:M], before[0][:M]) and torch.equal(state.Lp[0][:M], before[1][:M])
    assert torch.equal(state.tile_inv[0][0, :M], before[2][0, :M])


def test_capacity_is_checked_by_the_binding():
    state, fac, _, (K, Zc, zs_t, Cov, W0) = _run_steps((5,), capacity=6)
    with pytest.raises(hip.EmcidHipError, match="capacity"):
        hip.edit_layer_dual_preserve(K[:3].contiguous().to(DEV), Zc[:3].contiguous().to(DEV), zs_t[:3].contiguous().to(DEV), fac, 0,
                                     EW, LEFT, W0.to(DEV), torch.empty(H, D, device=DEV), state)
    assert state.M == 5

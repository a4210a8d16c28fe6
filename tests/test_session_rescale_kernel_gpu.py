"""emcid_session_rescale_f64 (include/emcid_hip.h) through the binding, no encoder: after a rescale the state must be the state of
the scaled rows — Yp' the rows times their factors bit for bit (one fp64 multiply per element), Lp' = chol(I + Yp' Yp'^T), the
tile inverses those of its diagonal tiles — with rows below the smallest changed one, everything behind row M and the
covariance-factor workspace never written, the same bits whether the rows are scaled in place or out of a copy, and a step on it
must be the primal solve of the system as the device then holds it.  The references are formed here, on the CPU in fp64.  Inputs,
helpers and bars are those of tests/session_kernel_helpers.py."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import hip
from session_kernel_helpers import DEV, EW, H, LAM, LEFT, L_BAR, U_BAR, _dev, _inputs_by_width as _inputs, _retain, _scale, _step

NSTEP = 6                       # rows of the step that follows every rescale
CHUNK = 70                      # the state is seeded by retain lists of at most this many rows
# (M, {row: factor} or a uniform factor, d)
CASES = {
    "uniform": (8, 0.5, 384),                                         # first = 0: the tail's M == 0 branch, one tile
    "inside-tile": (200, {3: 2.0, 130: 2.0, 131: 2.0}, 384),          # first = 3 inside a tile, the rebuilt range crosses a tile edge
    "tile-edge": (256, {i: 0.7 for i in range(128, 256)}, 384),       # first = 128 on a tile edge: tile 0 is not touched at all
    "three-tiles": (329, math.sqrt(1.0 / 3.0), 384),                  # N = 329 from the front: three tiles, the fused-leaf schedule
    "last-row": (200, {199: 2.0}, 384),                               # N = 1
    "padded": (150, {i: 0.5 for i in range(1, 150)}, 200),            # d = 200, dp = 256: padding columns
    "ones": (200, 1.0, 384),                                          # every factor 1: no launch
}


def _factors(case):
    M, f, _ = CASES[case]
    out = torch.full((M,), float(f), dtype=torch.float64) if not isinstance(f, dict) else torch.ones(M, dtype=torch.float64)
    if isinstance(f, dict):
        for i, v in f.items():
            out[i] = v
    return out


def _seed(K, M, fac, d, capacity):
    state = hip.PreservedKeys(1, d, capacity, DEV)
    for a in range(0, M, CHUNK):
        assert _retain(K[a:min(a + CHUNK, M)], fac, state) == 0
    assert state.M == M
    return state


def _tensors(state):
    return state.Yp[0], state.Lp[0], state.tile_inv[0]


@functools.lru_cache(maxsize=None)
def _run(case):
    """One rescale per case (and its twin out of a copy), shared by the tests and never written afterwards: everything they
    compare, on the host."""
    M, _, d = CASES[case]
    f = _factors(case)
    K, Zc, zs_t, Cov, W0 = _inputs(M + NSTEP, d)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = _seed(K, M, fac, d, M + NSTEP)
    state.row_scale[:M] = torch.arange(M, dtype=torch.float64) + 1.0          # (marks to follow the host vector's commit)
    before = [t.clone() for t in _tensors(state)]
    cov_before = fac.buf.clone()
    # the twin: the same state, scaled out of a copy of its rows
    twin = hip.PreservedKeys(1, d, M + NSTEP, DEV)
    for t, s in zip(_tensors(twin), before):
        t.copy_(s)
    twin.M = M
    res = hip.session_rescale(state, 0, f)
    flag = int(res["ws"].info.item()) if res["ws"] is not None else 0
    assert state.M == M                                                       # the entry commits nothing by itself
    after = [t.clone() for t in _tensors(state)]
    res2 = hip.session_rescale(twin, 0, f, first=res["first"], src=before[0].clone())
    flag2 = int(res2["ws"].info.item()) if res2["ws"] is not None else 0
    after2 = [t.clone() for t in _tensors(twin)]
    # ... and the same in-place call once more on the same bytes: what "the same bits" can mean for Lp (see the test below)
    again = hip.PreservedKeys(1, d, M + NSTEP, DEV)
    for t, s in zip(_tensors(again), before):
        t.copy_(s)
    again.M = M
    hip.session_rescale(again, 0, f)
    after3 = [t.clone() for t in _tensors(again)]
    state.rescale_commit(f)
    scale = state.row_scale[:M].clone()
    cov_same = torch.equal(fac.buf, cov_before)
    new = slice(M, M + NSTEP)
    U = _step(K[new], Zc[new], zs_t[new], W0, fac, state)["U"].cpu()
    # the system as the device holds it: L L^T + (Yp' L^T)^T (Yp' L^T) + Kt^T Kt, L the factor of lam C' in the workspace
    L = torch.tril(fac.L(0)[:d, :d]).cpu()
    P = after[0][:M, :d].cpu() @ L.t()
    Kt = _scale() * K[new].double()
    Rt = (_scale() * (zs_t[new] - Zc[new]).double()) / LEFT
    U_ref = torch.linalg.solve(L @ L.t() + P.t() @ P + Kt.t() @ Kt, Kt.t() @ Rt).t()
    return dict(M=M, d=d, f=f, first=res["first"], launched=res["launched"], launched2=res2["launched"], flag=flag, flag2=flag2,
                scale=scale, cov_same=cov_same, before=[t.cpu() for t in before], after=[t.cpu() for t in after],
                after2=[t.cpu() for t in after2], after3=[t.cpu() for t in after3], U=U, U_ref=U_ref)


@pytest.mark.parametrize("case", list(CASES))
def test_rescaled_state_vs_numpy(case):
    """Yp' bitwise factor x Yp; Lp' against numpy's Cholesky of I + Yp' Yp'^T; every tile inverse against the inverse of its tile's
    leading part; rows < first, the tiles wholly below first, everything behind row M and the covariance-factor workspace
    byte-identical; all factors 1 launches nothing and leaves every byte as it was."""
    r = _run(case)
    M, f, first = r["M"], r["f"], r["first"]
    (Y0, L0, T0), (Y1, L1, T1) = r["before"], r["after"]
    assert r["flag"] == 0
    changed = torch.nonzero(f != 1.0).flatten()
    assert first == (int(changed[0]) if changed.numel() else M)
    assert r["launched"] == (case != "ones")
    assert r["scale"].tolist() == [(i + 1) * float(f[i]) for i in range(M)]
    assert r["cov_same"]                                             # the cov-factor workspace is only ever read by the step
    if not r["launched"]:
        assert torch.equal(Y0, Y1) and torch.equal(L0, L1) and torch.equal(T0, T1)
    assert torch.equal(Y1[:M], f[:, None] * Y0[:M])                  # one fp64 multiply per element
    assert torch.equal(Y1[:first], Y0[:first]) and torch.equal(L1[:first], L0[:first])
    full = first // 128
    assert torch.equal(T1[:full], T0[:full])
    if full < T1.shape[0]:
        assert torch.equal(T1[full, :first - 128 * full], T0[full, :first - 128 * full])
    assert torch.equal(Y1[M:], Y0[M:]) and torch.equal(L1[M:], L0[M:])          # nothing behind row M is written
    assert torch.equal(L1[:M, M:], L0[:M, M:])
    Y = Y1[:M]
    Lref = torch.from_numpy(np.linalg.cholesky((torch.eye(M, dtype=torch.float64) + Y @ Y.t()).numpy()))
    Lgot = L1[:M, :M]
    lerr = (Lgot - Lref).abs().max().item() / Lref.abs().max().item()
    terr = 0.0
    for J in range((M + 127) // 128):
        w = min(128, M - 128 * J)
        inv_ref = torch.linalg.inv(Lref[128 * J:128 * J + w, 128 * J:128 * J + w])
        inv = T1[J, :w, :w]
        terr = max(terr, (inv - inv_ref).abs().max().item() / inv_ref.abs().max().item())
        assert torch.equal(torch.triu(inv, 1), torch.zeros_like(inv)), J
    print(f"{case}: M={M}, first={first}: factor error {lerr:.3e}, tile inverse error {terr:.3e} of the largest entry")
    assert lerr <= L_BAR
    assert torch.equal(torch.triu(Lgot, 1), torch.zeros_like(Lgot))
    assert terr <= L_BAR


def _factor_errors(M, Y, Lgot, T):
    """(error of Lp, error of the tile inverses) against numpy's Cholesky of I + Y Y^T, of the largest entry"""
    Lref = torch.from_numpy(np.linalg.cholesky((torch.eye(M, dtype=torch.float64) + Y @ Y.t()).numpy()))
    lerr = (Lgot - Lref).abs().max().item() / Lref.abs().max().item()
    terr = 0.0
    for J in range((M + 127) // 128):
        w = min(128, M - 128 * J)
        inv_ref = torch.linalg.inv(Lref[128 * J:128 * J + w, 128 * J:128 * J + w])
        terr = max(terr, (T[J, :w, :w] - inv_ref).abs().max().item() / inv_ref.abs().max().item())
    return lerr, terr


@pytest.mark.parametrize("case", list(CASES))
def test_scaling_out_of_a_copy_gives_the_same_bits(case):
    """Scaled out of a separate copy of its rows, the state holds the same bits as scaled in place: asserted for Yp', rows < first
    and everything behind row M — everything the scaling pass and the copy decide.  Lp' and the tile inverses behind `first` come
    out of the tail every session entry shares, whose products add their K slices with f64 atomics (syrk_signed_kernel, the split
    B = Yk Yp^T): two runs of the SAME in-place call on the same bytes already differ in their last bits there (the figures are
    printed: on MI355X the in-place call differs from its own repetition by 3e-16 ... 1.3e-15 of the largest entry in five of
    the six launched cases, from the copy's run by 1.3e-16 ... 1.3e-15), so for them the copy's run is held to what the in-place run is held to — the bar against numpy's factor."""
    r = _run(case)
    M, first = r["M"], r["first"]
    assert r["flag2"] == 0
    assert r["launched2"] == (case != "ones")        # (`first` was handed over: with every factor 1 it is M, and nothing runs)
    (Y1, L1, T1), (Y2, L2, T2), (Y3, L3, T3) = r["after"], r["after2"], r["after3"]
    assert torch.equal(Y1, Y2)
    assert torch.equal(L1[:first], L2[:first]) and torch.equal(L1[M:], L2[M:]) and torch.equal(L1[:M, M:], L2[:M, M:])
    full = first // 128
    assert torch.equal(T1[:full], T2[:full])
    top = L1[:M, :M].abs().max().item()
    rerun, copy = (L1 - L3).abs().max().item() / top, (L1 - L2).abs().max().item() / top
    print(f"{case}: Lp' in place against the same call again {rerun:.3e}, against the run out of a copy {copy:.3e} of the largest "
          f"entry; bitwise equal: {torch.equal(L1, L3)} / {torch.equal(L1, L2)}")
    if not r["launched"]:
        assert torch.equal(L1, L2) and torch.equal(T1, T2)
        return
    lerr, terr = _factor_errors(M, Y2[:M], L2[:M, :M], T2)
    assert lerr <= L_BAR and terr <= L_BAR
    assert torch.equal(torch.triu(L2[:M, :M], 1), torch.zeros(M, M, dtype=torch.float64))


@pytest.mark.parametrize("case", list(CASES))
def test_step_after_rescale_vs_primal_fp64(case):
    """U of an edit step after the rescale against torch.linalg.solve on the system as the device holds it,
    L L^T + (Yp' L^T)^T (Yp' L^T) + Kt^T Kt with L the workspace's factor of lam C': within 1e-8 of max|U|."""
    r = _run(case)
    top = r["U_ref"].abs().max().item()
    err = (r["U"] - r["U_ref"]).abs().max().item() / top
    print(f"{case}: U after the rescale {err:.3e} of max|U| from the primal solve")
    assert err <= U_BAR


def test_a_rejected_rebuild_reports_and_rows_below_first_stay():
    """Lp spoiled below `first` as tests/test_session_release_kernel_gpu.py spoils it (far too small, so T has a negative pivot: wrong
    input, not a fault): the flag is non-zero, rows < first are untouched, and the same call passes once the state is put right."""
    M, first = 8, 4
    K, _, _, Cov, _ = _inputs(M)
    K = K.clone()
    g = torch.Generator().manual_seed(7)
    K[5:8] = K[:3] + 0.05 * torch.randn(3, 384, generator=g)           # close to rows that stay below `first`: B is not small
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = _seed(K, M, fac, 384, M)
    f = [1.0] * first + [2.0] * (M - first)
    good = [t.clone() for t in _tensors(state)]
    state.Lp[0][:first] *= 1e-3
    state.tile_inv[0][0, :first] *= 1e3
    before = [t.clone() for t in _tensors(state)]
    res = hip.session_rescale(state, 0, f)
    assert int(res["ws"].info.item()) != 0 and state.M == M and res["first"] == first
    assert torch.equal(state.Yp[0][:first], before[0][:first]) and torch.equal(state.Lp[0][:first], before[1][:first])
    assert torch.equal(state.tile_inv[0][0, :first], before[2][0, :first])
    for t, s in zip(_tensors(state), good):
        t.copy_(s)                                                     # what the session does with its copy
    res = hip.session_rescale(state, 0, f)
    assert int(res["ws"].info.item()) == 0
    Y = state.Yp[0][:M].cpu()
    assert torch.equal(Y, torch.tensor(f, dtype=torch.float64)[:, None] * good[0][:M].cpu())
    Lref = torch.from_numpy(np.linalg.cholesky((torch.eye(M, dtype=torch.float64) + Y @ Y.t()).numpy()))
    torch.testing.assert_close(state.Lp[0][:M, :M].cpu(), Lref, rtol=L_BAR, atol=L_BAR)


def test_the_whole_capacity_is_rebuilt_from_the_front():
    """N = M = capacity, one row more than a release can rebuild: the retain sizer's workspace takes it and B is not touched."""
    M = 130
    K, _, _, Cov, _ = _inputs(M)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = _seed(K, M, fac, 384, M)
    Y0 = state.Yp[0].clone()
    res = hip.session_rescale(state, 0, 0.25)
    assert int(res["ws"].info.item()) == 0 and res["first"] == 0 and res["ws"].key == (M, 384, M)
    Y = state.Yp[0].cpu()
    assert torch.equal(Y, 0.25 * Y0.cpu())
    Lref = torch.from_numpy(np.linalg.cholesky((torch.eye(M, dtype=torch.float64) + Y @ Y.t()).numpy()))
    assert (state.Lp[0][:M, :M].cpu() - Lref).abs().max().item() <= L_BAR * Lref.abs().max().item()


def test_the_binding_checks_factors_first_and_src():
    K, _, _, Cov, _ = _inputs(8)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = _seed(K, 8, fac, 384, 8)
    before = [t.clone() for t in _tensors(state)]
    for bad in (0.0, -1.0, float("nan"), [1.0] * 7 + [float("inf")]):
        with pytest.raises(hip.EmcidHipError, match="positive and finite"):
            hip.session_rescale(state, 0, bad)
    with pytest.raises(hip.EmcidHipError, match="committed rows"):
        hip.session_rescale(state, 0, [1.0, 2.0])
    with pytest.raises(hip.EmcidHipError, match="first = 5"):
        hip.session_rescale(state, 0, [1, 1, 2, 1, 1, 1, 1, 1], first=5)
    with pytest.raises(hip.EmcidHipError, match="layer index"):
        hip.session_rescale(state, 1, 0.5)
    with pytest.raises(hip.EmcidHipError, match="first"):
        hip.session_rescale(state, 0, torch.full((8,), 0.5, dtype=torch.float64, device=DEV))
    with pytest.raises(hip.EmcidHipError, match="src"):
        hip.session_rescale(state, 0, 0.5, src=state.Yp[0][:4])                  # fewer rows than are committed
    with pytest.raises(hip.EmcidHipError, match="src"):
        hip.session_rescale(state, 0, 0.5, src=state.Yp[0].float())
    assert hip.session_rescale(state, 0, 1.0)["launched"] is False
    assert state.M == 8 and all(torch.equal(a, b) for a, b in zip(before, _tensors(state)))

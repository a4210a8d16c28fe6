"""emcid_session_release_f64 (include/emcid_hip.h) through the binding, no encoder: after a release the state must be the state of
the kept rows alone — Yp' the kept rows bit for bit, Lp' = chol(I + Yp' Yp'^T), the tile inverses those of its diagonal tiles — with
rows below the smallest released index never written, and a step on it must be the primal solve without the released keys.  The
references are formed here, on the CPU in fp64.  Inputs, helpers and bars are those of tests/session_kernel_helpers.py."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import hip
from session_kernel_helpers import DEV, EW, H, LAM, LEFT, L_BAR, U_BAR, _cp, _dev, _inputs_by_width as _inputs, _retain, _scale, _step

NSTEP = 6                       # rows of the step that follows every release
CHUNK = 70                      # the state is seeded by retain lists of at most this many rows
# (M, released rows, d)
CASES = {
    "first0": (8, (0,), 384),                             # first = 0: the tail's M == 0 branch
    "tile-edge": (200, (3, 130, 131), 384),               # the rebuilt range crosses the 128-tile edge, first unaligned
    "129-gone": (329, tuple(range(100, 229)), 384),       # 129 released: the kept tail moves across two tiles
    "trailing": (200, (199,), 384),                       # no launch
    "all": (5, (0, 1, 2, 3, 4), 384),                     # M' = 0, no launch
    "padded": (150, (1, 140), 200),                       # d = 200, dp = 256: padding columns
}


def _seed(K, rows, fac, d, capacity):
    state = hip.PreservedKeys(1, d, capacity, DEV)
    for a in range(0, len(rows), CHUNK):
        assert _retain(K[rows[a:a + CHUNK]], fac, state) == 0
    assert state.M == len(rows)
    return state


@functools.lru_cache(maxsize=None)
def _run(case):
    """One release per case, shared by the tests and never written afterwards: everything they compare, on the host."""
    M, gone, d = CASES[case]
    K, Zc, zs_t, Cov, W0 = _inputs(M + NSTEP, d)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    keep = [i for i in range(M) if i not in gone]
    state = _seed(K, list(range(M)), fac, d, M + NSTEP)
    state.row_scale[:M] = torch.arange(M, dtype=torch.float64) + 1.0          # (marks to follow the host vector's compaction)
    before = [t.clone() for t in (state.Yp[0], state.Lp[0], state.tile_inv[0])]
    cov_before = fac.buf.clone()
    res = hip.session_release(state, 0, keep)
    flag = int(res["ws"].info.item()) if res["ws"] is not None else 0
    assert state.M == M                                                       # the entry commits nothing by itself
    after = [t.clone() for t in (state.Yp[0], state.Lp[0], state.tile_inv[0])]
    state.release_commit(keep)
    scale = state.row_scale[:len(keep)].clone()
    cov_same = torch.equal(fac.buf, cov_before)
    new = slice(M, M + NSTEP)
    U = _step(K[new], Zc[new], zs_t[new], W0, fac, state)["U"].cpu()
    only = _seed(K, keep, fac, d, M + NSTEP) if keep else hip.PreservedKeys(1, d, M + NSTEP, DEV)
    U_only = _step(K[new], Zc[new], zs_t[new], W0, fac, only)["U"].cpu()
    P, Kt = _scale() * K[keep].double(), _scale() * K[new].double()
    Rt = (_scale() * (zs_t[new] - Zc[new]).double()) / LEFT
    U_ref = torch.linalg.solve(LAM * _cp(Cov) + P.t() @ P + Kt.t() @ Kt, Kt.t() @ Rt).t()
    return dict(M=M, d=d, keep=keep, first=res["first"], launched=res["launched"], flag=flag, scale=scale, cov_same=cov_same,
                before=[t.cpu() for t in before], after=[t.cpu() for t in after], U=U, U_only=U_only, U_ref=U_ref)


@pytest.mark.parametrize("case", list(CASES))
def test_released_state_vs_numpy(case):
    """Yp' bitwise the kept rows; Lp' against numpy's Cholesky of I + Yp' Yp'^T; every tile inverse against the inverse of its tile's
    leading part; rows < first and the tiles wholly below first byte-identical; the launch-free cases leave every buffer as it was."""
    r = _run(case)
    M, keep, first, n = r["M"], r["keep"], r["first"], len(r["keep"])
    (Y0, L0, T0), (Y1, L1, T1) = r["before"], r["after"]
    assert r["flag"] == 0
    assert first == next((j for j, i in enumerate(keep) if i != j), n)
    assert r["launched"] == (case not in ("trailing", "all"))
    assert r["scale"].tolist() == [float(i + 1) for i in keep]
    assert r["cov_same"]                                             # the cov-factor workspace is only ever read by the step
    if not r["launched"]:
        assert torch.equal(Y0, Y1) and torch.equal(L0, L1) and torch.equal(T0, T1)
    assert torch.equal(Y1[:n], Y0[keep])
    assert torch.equal(Y1[:first], Y0[:first]) and torch.equal(L1[:first], L0[:first])
    full = first // 128
    assert torch.equal(T1[:full], T0[:full])
    assert torch.equal(T1[full, :first - 128 * full], T0[full, :first - 128 * full])
    assert torch.equal(Y1[n:], Y0[n:]) and torch.equal(L1[n:], L0[n:])          # nothing behind the rebuilt rows is written either
    if n == 0:
        return
    Y = Y1[:n]
    Lref = torch.from_numpy(np.linalg.cholesky((torch.eye(n, dtype=torch.float64) + Y @ Y.t()).numpy()))
    Lgot = L1[:n, :n]
    lerr = (Lgot - Lref).abs().max().item() / Lref.abs().max().item()
    terr = 0.0
    for J in range((n + 127) // 128):
        w = min(128, n - 128 * J)
        inv_ref = torch.linalg.inv(Lref[128 * J:128 * J + w, 128 * J:128 * J + w])
        inv = T1[J, :w, :w]
        terr = max(terr, (inv - inv_ref).abs().max().item() / inv_ref.abs().max().item())
        assert torch.equal(torch.triu(inv, 1), torch.zeros_like(inv)), J
    print(f"{case}: M={M} -> {n}, first={first}: factor error {lerr:.3e}, tile inverse error {terr:.3e} of the largest entry")
    assert lerr <= L_BAR
    assert torch.equal(torch.triu(Lgot, 1), torch.zeros_like(Lgot))
    assert terr <= L_BAR


@pytest.mark.parametrize("case", list(CASES))
def test_step_after_release_vs_primal_fp64(case):
    """U of an edit step after the release: against torch.linalg.solve on lam C' + Pkept^T Pkept + Kt^T Kt, and against the same step
    on a state that only ever received the kept rows; both within 1e-8 of max|U|.  (Measured on MI355X: 4e-14 ... 2e-13 at d = 384; at
    d = 200 the step is 8e-14 from the step on the kept rows alone and 9.3e-9 from the primal solve, the offset the step entry itself
    has at that d with or without a release — DESIGN.md section 3.)"""
    r = _run(case)
    top = r["U_ref"].abs().max().item()
    err = (r["U"] - r["U_ref"]).abs().max().item() / top
    same = (r["U"] - r["U_only"]).abs().max().item() / r["U_only"].abs().max().item()
    own = (r["U_only"] - r["U_ref"]).abs().max().item() / top
    print(f"{case}: U after the release {err:.3e} of max|U| from the primal solve, {same:.3e} from the step on the kept rows alone "
          f"(that step itself: {own:.3e} from the primal solve)")
    assert same <= U_BAR
    assert err <= U_BAR


def test_a_rejected_rebuild_reports_and_rows_below_first_stay():
    """Lp spoiled below `first` as tests/test_session_retain_kernel_gpu.py spoils it (far too small, so T has a negative pivot: wrong
    input, not a fault): the flag is non-zero, rows < first are untouched, and the same call passes once the state is put right."""
    M = 8
    K, _, _, Cov, _ = _inputs(M)
    K = K.clone()
    g = torch.Generator().manual_seed(7)
    K[5:8] = K[:3] + 0.05 * torch.randn(3, 384, generator=g)           # close to rows that stay below `first`: B is not small
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = _seed(K, list(range(M)), fac, 384, M)
    keep, first = [0, 1, 2, 3, 5, 6, 7], 4
    good = [t.clone() for t in (state.Yp[0], state.Lp[0], state.tile_inv[0])]
    state.Lp[0][:first] *= 1e-3
    state.tile_inv[0][0, :first] *= 1e3
    before = [t.clone() for t in (state.Yp[0], state.Lp[0], state.tile_inv[0])]
    res = hip.session_release(state, 0, keep, first)
    assert int(res["ws"].info.item()) != 0 and state.M == M
    assert torch.equal(state.Yp[0][:first], before[0][:first]) and torch.equal(state.Lp[0][:first], before[1][:first])
    assert torch.equal(state.tile_inv[0][0, :first], before[2][0, :first])
    for t, s in zip((state.Yp[0], state.Lp[0], state.tile_inv[0]), good):
        t.copy_(s)                                                     # what the session does with its copy
    res = hip.session_release(state, 0, keep, first)
    assert int(res["ws"].info.item()) == 0
    state.release_commit(keep)
    Y = state.Yp[0][:7].cpu()
    assert torch.equal(Y, good[0][keep].cpu())
    Lref = torch.from_numpy(np.linalg.cholesky((torch.eye(7, dtype=torch.float64) + Y @ Y.t()).numpy()))
    torch.testing.assert_close(state.Lp[0][:7, :7].cpu(), Lref, rtol=L_BAR, atol=L_BAR)


def test_the_binding_checks_keep_and_first():
    K, _, _, Cov, _ = _inputs(8)
    fac = hip.factor_cov([_dev(Cov)], LAM, EW)
    state = _seed(K, list(range(8)), fac, 384, 8)
    before = [t.clone() for t in (state.Yp[0], state.Lp[0], state.tile_inv[0])]
    with pytest.raises(hip.EmcidHipError, match="ascending"):
        hip.session_release(state, 0, [0, 2, 1])
    with pytest.raises(hip.EmcidHipError, match="ascending"):
        hip.session_release(state, 0, [0, 8])
    with pytest.raises(hip.EmcidHipError, match="first"):
        hip.session_release(state, 0, [0, 1, 3], first=1)
    with pytest.raises(hip.EmcidHipError, match="layer index"):
        hip.session_release(state, 1, [0, 1, 3])
    with pytest.raises(hip.EmcidHipError, match="first"):
        hip.session_release(state, 0, torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV))
    assert hip.session_release(state, 0, list(range(8)))["launched"] is False          # nothing goes
    assert state.M == 8 and all(torch.equal(a, b) for a, b in zip(before, (state.Yp[0], state.Lp[0], state.tile_inv[0])))

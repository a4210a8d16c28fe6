"""The COLUMN-SHARDED form of the dual solve, stage by stage in fp64 (csrc/edit_solve.hip, "COLUMN-SHARDED"; hip._HipColsBackend):

    per rank, tiles t_0 < t_1 < ... of the d / 128 column tiles, kd = 128 (t + 1), w = 128 n_tiles
    stage 1   Kt64, Rt -> Yc[:, 128 i : 128 i + 128] = Kt[:, :kd] X[128 t_i : 128 t_i + 128, :kd]^T -> partial S = Yc[:, :w] Yc[:, :w]^T
    caller    S = sum of the partial S over the ranks                                    (the all-reduce, emulated here)
    stage 2   S + I = LS LS^T [-> XT = inv(LS)^T] -> Z^T = Rt^T S^-1 -> V[:, :w] = Z^T Yc[:, :w] -> partial U = sum_i V_i X[tile rows, :kd]
    caller    U = sum of the partial U, then emcid_apply_update2d_f32: dW = float(U), W = W0 + dW

Inputs, references and the allowance rule are those of test_dual_chain_gpu.py (its _row, _check, _floor, _split_err, _dw_bound,
_poisoned_workspace, imported): correlated keys, cond(S) = 3e5, the factor built at lam0 and the edit at lam = 0.4 lam0; every
residual is allowed 8 x torch's fp64 residual of the same stage on the same device-held input by the same method plus
4 eps64 (depth) max|A| max|B|; dW is judged element by element against the oracle's fp64 LU by _dw_bound.  No constant is new.

Every rank works on its own NaN-poisoned DualWorkspace (everything but the stream-K block).  The all-reduce is emulated as the
sum of the ranks' partial S in rank order on the lower 128-tiles and NaN on every 128-tile strictly above the diagonal: stage 2
must not read there.  (Stage 1's SYRK computes 64 x 64 tiles on and below the diagonal, so inside a diagonal 128-tile the 64-tile
above the diagonal is not written; what a check excuses there is only an entry ABOVE the diagonal that still holds, bit for bit,
what it held before the call.)  The summed S is judged against I + Yt Yt^T for the Yt the ranks' Yc blocks make up.  Which form
ran is asserted from the per-class launch counts of a second, profiled run on the same workspaces, neither zeroed nor poisoned
again: that run also bypasses the cached stage-2 graph.

Branches by shape, read from emcid_edit_dual_cols_stage2_f64 / cholesky_takes_shadow / solve_schur_rhs (stage 2 passes no
full-inverse buffer, so this form NEVER builds the full inverse: xrow for 256 <= Np <= 2048, block substitution otherwise):

    N     d    h    Np    tiles  branch reached                              deals (one list per emulated rank)
    100   256  32   128   2      serial, one leaf; substitution              [[0,1]], [[1],[0]]
    130   200  48   256   2      fused, inverse rides (xrow); ragged d       [[0,1]], [[1],[0]]
    130   200  33   256   2      odd h (hp = 34)                             [[1],[0]]
    300   640  48   384   5      depth kd from 128 to 640                    column_tiles for world 2, 3, 5 (one tile per rank); [[0,2,4],[1,3]]
    600   384  48   640   3      stream-K assemble sizes                     column_tiles for world 3
    2049  256  32   2176  2      serial with short block; substitution       [[1],[0]]

Measured on MI355X: max-abs residuals, torch's / the kernel's, the line closest to its allowance over the deals, ranks and
tiles of each row.  Every line of every case, with the allowance, is printed by the run and written to the file
EMCID_DUAL_COLS_TABLE names; profiles/dual_cols_residuals.txt is that file.

    row         Yc              S part          S sum           LS              XT              Z^T             V               U               dW (vs oracle; allowed)
    100x256x32  1.4e-14/2.1e-14 1.5e-11/1.5e-11 1.5e-11/1.5e-11 4.4e-11/3.6e-11 -               9.3e-11/1.5e-10 3.1e-14/2.5e-14 7.1e-15/7.1e-15 9.4e-07 (1.5e-06)
    130x200x48  2.8e-14/2.8e-14 9.1e-13/9.1e-13 1.1e-11/1.1e-11 2.2e-11/3.6e-11 1.0e-13/9.2e-14 9.7e-11/1.0e-10 3.2e-15/4.7e-14 3.6e-15/5.3e-15 1.8e-06 (1.6e-05)
    130x200x33  5.3e-15/3.6e-15 9.1e-13/9.1e-13 1.5e-11/7.3e-12 2.2e-11/2.9e-11 1.3e-13/1.7e-13 1.1e-10/1.0e-10 1.2e-13/0       7.1e-15/0       2.2e-06 (1.6e-05)
    300x640x48  5.6e-16/8.9e-16 1.8e-12/1.8e-12 1.5e-11/2.9e-11 3.3e-11/4.7e-11 2.4e-13/2.5e-13 2.1e-10/2.2e-10 8.3e-14/7.1e-14 3.1e-15/3.1e-15 4.7e-07 (9.3e-07)
    600x384x48  1.4e-14/1.8e-14 9.1e-12/7.3e-12 7.3e-12/9.1e-12 3.6e-11/3.8e-11 2.1e-13/2.2e-13 1.8e-10/1.7e-10 7.7e-13/0       1.3e-15/6.7e-16 2.2e-07 (3.0e-07)
    2049x256x32 1.3e-15/1.8e-15 2.0e-13/2.0e-13 1.1e-11/1.3e-11 2.7e-11/2.7e-11 -               1.2e-10/1.5e-10 1.5e-12/1.4e-12 1.7e-16/8.3e-17 7.4e-09 (1.6e-08)
The kernels sit within a small factor of torch at every stage, tile and deal (a 0: the same bits as torch's product), the allowance
is the floor's almost everywhere, and dW's error is the fp32 rounding of U.  The poison found no stage that reads what it did not
write, the NaN above the lower 128-tiles of the summed S reached nothing, and every launch count is the branch table's.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import hip
from test_dual_chain_gpu import (DEV, EW, LEFT, _TABLE, _amax, _block_mask, _check, _dw_bound, _finite, _floor, _poisoned_workspace,
                                 _row, _split_err)

NAN = float("nan")
BAD_ARG, ERR_WORKSPACE = -1, -3


def _world(world, n_tiles):
    return [hip.column_tiles(r, world, n_tiles) for r in range(world)]


# (N, d, h) -> how Z = S^-1 Rt is solved, and the deals: name -> one ascending tile list per emulated rank
ROWS = {
    (100, 256, 32): ("substitution", {"one": [[0, 1]], "swap": [[1], [0]]}),
    (130, 200, 48): ("xrow", {"one": [[0, 1]], "swap": [[1], [0]]}),
    (130, 200, 33): ("xrow", {"swap": [[1], [0]]}),
    (300, 640, 48): ("xrow", {"world2": _world(2, 5), "world3": _world(3, 5), "world5": _world(5, 5), "oddeven": [[0, 2, 4], [1, 3]]}),
    (600, 384, 48): ("xrow", {"world3": _world(3, 3)}),
    (2049, 256, 32): ("substitution", {"swap": [[1], [0]]}),
}
CASES = [(N, d, h, deal) for (N, d, h), (_, deals) in ROWS.items() for deal in deals]


@pytest.fixture(scope="module", autouse=True)
def _cols_residual_table():
    first = len(_TABLE)
    yield
    table = _TABLE[first:]
    lines = [f"{'case':44s} {'stage':10s} {'ref':>10s} {'kernel':>10s} {'allowed':>10s}"]
    lines += [f"{c:44s} {s:10s} {r:10.3e} {k:10.3e} {a:10.3e}" for c, s, r, k, a in table]
    worst = {}
    for c, s, r, k, a in table:
        key = (c.split(" ")[0], s)
        if key not in worst or k / max(a, 1e-300) > worst[key][1] / max(worst[key][2], 1e-300):
            worst[key] = (r, k, a)
    lines += ["", "worst per row and stage:"] + [f"{c:18s} {s:10s} ref {r:9.3e} kernel {k:9.3e} allowed {a:9.3e}"
                                                   for (c, s), (r, k, a) in worst.items()]
    print("\n".join(lines[-len(worst) - 2:]))
    path = os.environ.get("EMCID_DUAL_COLS_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _same_bits(a, b):
    return a.contiguous().view(torch.int64) == b.contiguous().view(torch.int64)


def _all_nan(x):
    return bool(torch.isnan(x).all())


_X_CHECKED = set()


def _diag_tiles_above_diagonal(X):
    i = torch.arange(X.shape[0], device=X.device)
    return X[(i[:, None] // 128 == i[None, :] // 128) & (i[None, :] > i[:, None])]


def _lower_x(fac, layer):
    """tril(X) of the layer; once per factor workspace: the part of X's diagonal 128-tiles above the diagonal is exact zeros (the
    per-tile products of both stages take no triangular hint and read those tiles whole)."""
    X = fac.X(layer)
    if (id(fac), layer) not in _X_CHECKED:
        assert int(_diag_tiles_above_diagonal(X).count_nonzero()) == 0, "X: a diagonal 128-tile is not zero above the diagonal"
        _X_CHECKED.add((id(fac), layer))
    return torch.tril(X)


def _backend(r, ws):
    return hip._HipColsBackend(r["K"], r["Zc"], r["zs_t"], r["fac"], 1, EW, LEFT, ws, lam=r["lam"])


def _counters_zero(ws, case):
    assert int(ws.sk_counters.view(torch.int64).count_nonzero()) == 0, f"{case}: stream-K ticket counters not left zero"


def _check_stage1(case, r, ws, tiles, S_before):
    """What stage 1 left in `ws` for `tiles`.  S_before: ws.S as it was before the call.  Returns the partial S (a copy)."""
    N, d, h = r["N"], r["d"], r["h"]
    fac = r["fac"]
    Np, dp = ws.Np, ws.dp
    Xc = _lower_x(fac, 1)
    _counters_zero(ws, case)
    # ---- Kt64, Rt: bit for bit, exact zeros on the padding (as the chain test demands)
    s, g = math.sqrt(EW / 0.5), 1.0 / math.sqrt(fac.lam_ratio(r["lam"]))
    Kt, Rt_full = ws.Kt, ws.Rt
    assert torch.equal(Kt[:N, :d], (r["K"].double() * s) * g), f"{case}: stage Kt64"
    assert int(Kt[N:].count_nonzero()) == 0 and int(Kt[:, d:].count_nonzero()) == 0, f"{case}: stage Kt64: padding not zero"
    Rt_want = ((r["zs_t"].cpu() - r["Zc"].cpu()).double() * s) / LEFT * g
    assert torch.equal(Rt_full[:N, :h].cpu(), Rt_want), f"{case}: stage Rt"
    assert int(Rt_full[N:].count_nonzero()) == 0 and int(Rt_full[:, h:].count_nonzero()) == 0, f"{case}: stage Rt: padding not zero"
    # ---- Yc, block by block: position i in the list, tile index t, contraction depth kd = 128 (t + 1)
    Yc = ws.Yt
    for i, t in enumerate(tiles):
        kd = 128 * (t + 1)
        A, B = Kt[:, :kd], Xc[128 * t:128 * t + 128, :kd].T
        blk = Yc[:, 128 * i:128 * i + 128]
        _finite(blk, case, f"Yc block {i} (tile {t})")
        _check(f"{case} t{t}", "Yc", _amax(blk - A @ B), _split_err(A, B), _floor(kd, A, B))
        assert int(blk[N:].count_nonzero()) == 0, f"{case}: stage Yc: padding rows of block {i} (tile {t}) not zero"
        if 128 * (t + 1) > d:
            assert int(blk[:, d - 128 * t:].count_nonzero()) == 0, f"{case}: stage Yc: padding columns of the last tile not zero"
    # ---- partial S = Yc[:, :w] Yc[:, :w]^T on the lower 128-tiles, no identity; rows and columns >= N exact zeros
    w = 128 * len(tiles)
    Yw = Yc[:, :w]
    S = ws.S.clone()
    i = torch.arange(Np, device=DEV)
    excused = (i[None, :] > i[:, None]) & _same_bits(S, S_before)      # above the diagonal and not written by this call
    read = _block_mask(Np, lower=True) & ~excused
    got = torch.where(read, S, torch.zeros_like(S))
    _finite(got, case, "partial S (lower 128-tiles)")
    _check(case, "S part", _amax(got - torch.where(read, Yw @ Yw.T, torch.zeros_like(S))), _split_err(Yw, Yw.T), _floor(w, Yw, Yw))
    assert int(got[N:].count_nonzero()) == 0 and int(got[:, N:].count_nonzero()) == 0, f"{case}: stage S part: padding not zero"
    return S


def _all_reduce_s(partials, Np):
    """The all-reduce as stage 2 may rely on it: the sum in rank order on the lower 128-tiles, NaN strictly above them."""
    total = partials[0].clone()
    for p in partials[1:]:
        total += p
    return torch.where(_block_mask(Np, lower=True), total, torch.full_like(total, NAN))


def _check_stage2(case, r, ws, tiles, schur, Ssym):
    """What stage 2 left in `ws` for `tiles`, given the summed system Ssym (= I + the summed S, symmetric).  Returns (RT, U copy)."""
    N, d, h = r["N"], r["d"], r["h"]
    Np, dp = ws.Np, ws.dp
    Xc = _lower_x(r["fac"], 1)
    _counters_zero(ws, case)
    assert int(ws.info.item()) == 0, f"{case}: stage LS: info {int(ws.info.item())}"
    eye = torch.eye(Np, dtype=torch.float64, device=DEV)
    Rt = ws.Rt[:, :h]
    # ---- LS
    Ld = torch.tril(ws.LS)
    _finite(Ld, case, "LS (lower triangle)")
    Lt = torch.linalg.cholesky(Ssym)
    _check(case, "LS", _amax(torch.tril(Ld @ Ld.T - Ssym)), _amax(torch.tril(Lt @ Lt.T - Ssym)), _floor(Np, Ld, Ld))
    # ---- XT = inv(LS)^T where it rides in the factorization
    assert schur == ("xrow" if 256 <= Np <= 2048 else "substitution")
    XS = None
    if schur == "xrow":
        XTr = torch.where(_block_mask(Np, lower=False), ws.XT, torch.zeros_like(ws.XT))
        _finite(XTr, case, "XT (upper tiles)")
        assert int(torch.tril(XTr, -1).count_nonzero()) == 0, f"{case}: stage XT: not upper triangular inside its diagonal tiles"
        Xs_t = torch.linalg.solve_triangular(Ld, eye, upper=False)
        _check(case, "XT", _amax(XTr.T @ Ld - eye), _amax(Xs_t @ Ld - eye), _floor(Np, XTr, Ld))
        XS = XTr.T
    # ---- Z^T: RT Ssym = Rt^T, torch's own by the branch's method
    RT = ws.RT[:h]
    _finite(RT, case, "RT = Z^T")
    Zt = torch.cholesky_solve(Rt, Ld).T if schur == "substitution" else (Rt.T @ XS.T) @ XS
    _check(case, "Z^T", _amax(RT @ Ssym - Rt.T), _amax(Zt @ Ssym - Rt.T), _floor(Np, RT, Ssym))
    # ---- V[:, :w] = Z^T Yc[:, :w]
    w = 128 * len(tiles)
    Yw, Vw = ws.Yt[:, :w], ws.V[:, :w]
    _finite(Vw, case, "V[:, :w]")
    _check(case, "V", _amax(Vw - RT @ Yw), _split_err(RT, Yw), _floor(Np, RT, Yw))
    # ---- partial U = sum_i V_i tril(X)[rows of tile t_i, :kd]: one product against the tiles' rows of tril(X) stacked (a row
    # of tile t is zero from column kd on), zero from the largest kd on and on the padding columns
    Xs = torch.cat([Xc[128 * t:128 * t + 128] for t in tiles])
    U = ws.U.clone()
    _finite(U, case, "partial U")
    _check(case, "U", _amax(U - Vw @ Xs), _split_err(Vw, Xs), _floor(w, Vw, Xs))
    kd_max = 128 * (tiles[-1] + 1)
    assert int(U[:, kd_max:].count_nonzero()) == 0, f"{case}: stage U: columns from the largest kd = {kd_max} on are not zero"
    assert int(U[:, d:].count_nonzero()) == 0, f"{case}: stage U: padding columns not zero"
    return RT, U


def _profiled(fn):
    classes = ["assemble", "inv_build", "inv_apply", "trsm_update", "delta_w"]
    hip.profile_enable(classes)
    try:
        fn()
        torch.cuda.synchronize()
        counts = {k: v[1] for k, v in hip.profile_collect().items()}
    finally:
        hip.profile_enable(())
    return {k: counts.get(k, 0) for k in classes}


_SUMMED = {}       # (N, d, h) -> the emulated all-reduce of S (lower tiles, NaN above) from the first deal of the row that ran


def _check_deal(N, d, h, deal):
    r = _row(N, d, h)
    schur, deals = ROWS[(N, d, h)]
    ranks = deals[deal]
    row = f"{N}x{d}x{h}"
    wss = [_poisoned_workspace(N, d, h) for _ in ranks]
    Np, dp = wss[0].Np, wss[0].dp
    assert sorted(t for ts in ranks for t in ts) == list(range(dp // 128))
    bes = [_backend(r, ws) for ws in wss]
    Xc = _lower_x(r["fac"], 1)

    # ---- stage 1 per rank
    partials = []
    for k, (be, ws, tiles) in enumerate(zip(bes, wss, ranks)):
        before = ws.S.clone()
        be.stage1(tiles)
        torch.cuda.synchronize()
        partials.append(_check_stage1(f"{row} {deal} r{k}", r, ws, tiles, before))

    # ---- the all-reduce: lower triangle of the sum plus I against I + Yt Yt^T, Yt put together from the ranks' Yc blocks
    case = f"{row} {deal}"
    S_sum = _all_reduce_s(partials, Np)
    _SUMMED.setdefault((N, d, h), S_sum)
    Yt = torch.empty(Np, dp, dtype=torch.float64, device=DEV)
    for ws, tiles in zip(wss, ranks):
        for i, t in enumerate(tiles):
            Yt[:, 128 * t:128 * t + 128] = ws.Yt[:, 128 * i:128 * i + 128]
    eye = torch.eye(Np, dtype=torch.float64, device=DEV)
    Sl = torch.tril(S_sum) + eye
    _finite(Sl, case, "summed S (lower triangle)")
    _check(case, "S sum", _amax(Sl - torch.tril(eye + Yt @ Yt.T)), _split_err(Yt, Yt.T), _floor(dp, Yt, Yt))
    Ssym = Sl + torch.tril(Sl, -1).T

    # ---- stage 2 per rank on the summed S (NaN on the strictly upper 128-tiles)
    U_sum, RT0 = None, None
    for k, (be, ws, tiles) in enumerate(zip(bes, wss, ranks)):
        ws.S.copy_(S_sum)
        be.stage2(tiles)
        torch.cuda.synchronize()
        RT, U = _check_stage2(f"{row} {deal} r{k}", r, ws, tiles, schur, Ssym)
        RT0 = RT if RT0 is None else RT0
        U_sum = U if U_sum is None else U_sum + U

    # ---- summation (rank order, torch fp64) and apply
    W = torch.full((h, d), NAN, device=DEV)
    dW = bes[0].apply(U_sum, r["W0"], W, True)
    torch.cuda.synchronize()
    assert torch.equal(dW, U_sum[:, :d].float()), f"{case}: stage dW: not float(U)"
    assert torch.equal(W, r["W0"] + dW), f"{case}: stage W: W != W0 + dW"
    bound, t64 = _dw_bound(r, RT0, Yt, Xc)
    over = ((dW.double() - r["U_ref"]).abs() - bound).max().item()
    _TABLE.append((case, "dW", r["wood_err"], _amax(dW.double() - r["U_ref"]), 2.0 ** -24 * _amax(r["U_ref"]) + t64))
    assert over <= 0.0, f"{case}: stage dW: an entry is {over:.3e} beyond 2^-24 |U_ref| + t64 (t64 {t64:.3e}, max|U_ref| {_amax(r['U_ref']):.3e})"

    # ---- the same again on the same workspaces, neither zeroed nor poisoned again, under the per-class launch counter (which
    # also takes the cached stage-2 graph out of the path)
    counts = [_profiled(lambda be=be, tiles=tiles: be.stage1(tiles)) for be, tiles in zip(bes, ranks)]
    S2 = _all_reduce_s([ws.S.clone() for ws in wss], Np)
    U2 = None
    ob = lambda n: -(-n // 512) - 1                  # rank-512 updates of one block substitution over n columns
    for k, (be, ws, tiles) in enumerate(zip(bes, wss, ranks)):
        ws.S.copy_(S2)
        c2 = _profiled(lambda: be.stage2(tiles))
        got = {key: counts[k][key] + c2[key] for key in c2}
        want = {"assemble": 1, "inv_build": 0, "inv_apply": 2 * len(tiles),
                "trsm_update": 2 * ob(Np) if schur == "substitution" else 0, "delta_w": 1}
        assert got == want, f"{case} r{k}: launches per class {got}, the branch in the table gives {want}"
        assert int(ws.info.item()) == 0
        _counters_zero(ws, f"{case} r{k} (second run)")
        U2 = ws.U.clone() if U2 is None else U2 + ws.U
    dW2 = bes[0].apply(U2, r["W0"], W, True)
    _finite(dW2, case, "dW of the second run")
    assert ((dW2.double() - r["U_ref"]).abs() - bound).max().item() <= 0.0, f"{case}: stage dW of the second run on the same workspaces"


@pytest.mark.parametrize("N,d,h,deal", CASES)
def test_cols_stage_by_stage(N, d, h, deal):
    _check_deal(N, d, h, deal)


def test_inverse_factor_is_zero_above_the_diagonal_of_its_diagonal_tiles():
    """What the un-hinted per-tile products rely on, for a workspace factor_cov made and for one cov_factor_rescale made of it
    (which copies the diagonal tiles whole), ragged d (the last tile is part identity padding) and five tiles."""
    for N, d, h in ((130, 200, 48), (300, 640, 48)):
        fac = _row(N, d, h)["fac"]
        scaled = hip.cov_factor_rescale(fac, 0.4)
        torch.cuda.synchronize()
        for f in (fac, scaled):
            assert f.have_inverse == {0, 1}
            for layer in (0, 1):
                X = f.X(layer)
                assert int(_diag_tiles_above_diagonal(X).count_nonzero()) == 0, (d, layer, f is scaled)
                assert bool(torch.isfinite(torch.tril(X)).all()) and int(torch.tril(X).diagonal().count_nonzero()) == f.dp


def test_reuse_with_another_tile_set():
    """One workspace, poisoned once, through tiles [0,1,2,3,4], [1], [4], [0] (the last three have equal w: one cached stage-2
    graph, zeroing U inside it, the per-tile products outside): after every run the partial S and the partial U pass the checks
    of a fresh workspace, in particular U is exact zeros beyond the set's largest kd while Yc and V beyond w hold the previous
    set's values.  Stage 2 gets the row's full summed S every time."""
    N, d, h = 300, 640, 48
    r = _row(N, d, h)
    if (N, d, h) not in _SUMMED:
        _check_deal(N, d, h, "world2")
    S_sum = _SUMMED[(N, d, h)]
    ws = _poisoned_workspace(N, d, h)
    Np = ws.Np
    Sl = torch.tril(S_sum) + torch.eye(Np, dtype=torch.float64, device=DEV)
    Ssym = Sl + torch.tril(Sl, -1).T
    be = _backend(r, ws)
    for tiles in ([0, 1, 2, 3, 4], [1], [4], [0]):
        case = f"{N}x{d}x{h} reuse " + "".join(map(str, tiles))
        before = ws.S.clone()
        be.stage1(tiles)
        torch.cuda.synchronize()
        _check_stage1(case, r, ws, tiles, before)
        ws.S.copy_(S_sum)
        be.stage2(tiles)
        torch.cuda.synchronize()
        _check_stage2(case, r, ws, tiles, "xrow", Ssym)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _lib_stage(stage, r, ws, tiles, n_tiles=None):
    """The library's stage entry called directly (hip.edit_layer_dual_cols sorts its list): (status, message)."""
    lib = hip.load()
    N, d, h = r["N"], r["d"], r["h"]
    fac = r["fac"]
    arr = (C.c_int * max(len(tiles), 1))(*tiles)
    n = len(tiles) if n_tiles is None else n_tiles
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    if stage == 1:
        rc = lib.emcid_edit_dual_cols_stage1_f64(hip._ptr(r["K"]), hip._ptr(r["Zc"]), hip._ptr(r["zs_t"]), N, d, h, EW, LEFT,
                                                 fac.lam_ratio(r["lam"]), hip._ptr(fac.buf), fac.n_layers, 1, arr, n,
                                                 hip._ptr(ws.buf), ws.nbytes, st)
    else:
        rc = lib.emcid_edit_dual_cols_stage2_f64(N, d, h, hip._ptr(fac.buf), fac.n_layers, 1, arr, n, hip._ptr(ws.buf), ws.nbytes,
                                                 hip._ptr(ws.info), st)
    return rc, lib.emcid_last_error().decode()


@pytest.mark.parametrize("tiles", [[], [1, 0], [0, 0], [-1], [2], list(range(257))], ids=["empty", "unsorted", "duplicate", "negative", "past_dp", "257"])
def test_bad_tile_list_is_refused_before_any_launch(tiles):
    """dp / 128 = 2 here.  Both stages: the bad-argument status with a message, and the Y, S, V and U blocks still all NaN."""
    r = _row(100, 256, 32)
    ws = _poisoned_workspace(100, 256, 32)
    for stage in (1, 2):
        rc, msg = _lib_stage(stage, r, ws, tiles)
        torch.cuda.synchronize()
        assert rc == BAD_ARG and msg, (stage, rc, msg)
        for name in ("Y", "S", "V", "U"):
            assert _all_nan(ws.block(name)), f"stage {stage} refused {tiles[:3]} but wrote block {name}"
    _counters_zero(ws, "refused")


def test_edit_layer_dual_cols_refuses_a_rank_without_tiles_and_a_layer_without_inverse():
    r = _row(100, 256, 32)
    W = torch.empty(32, 256, device=DEV)
    with pytest.raises(hip.EmcidHipError, match="without a column tile"):
        hip.edit_layer_dual_cols(r["K"], r["Zc"], r["zs_t"], r["fac"], 1, EW, LEFT, r["W0"], W, [], lambda t: t, lam=r["lam"])
    cov = torch.eye(256, device=DEV) * 2.0
    bare = hip.factor_cov([cov, cov], r["lam0"], EW, inverse=False)
    with pytest.raises(hip.EmcidHipError, match="explicit inverse factor"):
        hip.edit_layer_dual_cols(r["K"], r["Zc"], r["zs_t"], bare, 1, EW, LEFT, r["W0"], W, [0, 1], lambda t: t, lam=r["lam"])


def _refused_h_beyond_dp():
    """N = 100, d = 128, h = 160: RT / Y2 hold dp = 128 rows of Np.  Stage 1 runs; stage 2 returns the workspace status and S, and
    every block stage 2 writes, is bit for bit what it was."""
    N, d, h = 100, 128, 160
    r = _row(N, d, h)
    ws = _poisoned_workspace(N, d, h)
    rc, msg = _lib_stage(1, r, ws, [0])
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert bool(torch.isfinite(torch.tril(ws.S)).all())
    before = ws.buf.clone()
    rc, msg = _lib_stage(2, r, ws, [0])
    torch.cuda.synchronize()
    assert rc == ERR_WORKSPACE and "h rows" in msg, (rc, msg)
    off = ws.S.data_ptr() - ws.buf.data_ptr()
    assert off >= 0 and bool(_same_bits(ws.S, before[off // 8:off // 8 + ws.S.numel()].view_as(ws.S)).all()), "a refused stage 2 rewrote S"
    assert bool(_same_bits(ws.buf, before).all()), "a refused stage 2 wrote to its workspace"
    assert int(ws.info.item()) == 0


_REFUSED_SCRIPT = r'''
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_dual_cols_gpu as t
t._refused_h_beyond_dp()
print("REFUSED_OK")
'''


def test_h_beyond_dp_is_refused_before_any_launch():
    """With the graph cache on (a refusal inside the capture discards the graph) and, in a fresh child process, with
    EMCID_GRAPH = 0 (the switch is read once per process), where the launches are issued as the entry goes: the size test of
    stage 2 stands in front of its first launch."""
    from conftest import REPO
    _refused_h_beyond_dp()
    p = subprocess.run([sys.executable, "-c", _REFUSED_SCRIPT, str(REPO)], env=dict(os.environ, EMCID_GRAPH="0"),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "REFUSED_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---- emcid_apply_update2d_f32 -----------------------------------------------------------------------------------------------------

def _apply2d(U, ldu, W0, W, dW, h, d):
    lib = hip.load()
    rc = lib.emcid_apply_update2d_f32(hip._ptr(U), ldu, hip._ptr(W0), hip._ptr(W), hip._ptr(dW), h, d,
                                      C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, lib.emcid_last_error().decode()


@pytest.mark.parametrize("h,d,ldu", [(3, 5, 8), (33, 200, 256), (2, 700, 768)])
def test_apply_update2d_vs_torch(h, d, ldu):
    """dW = float(U[:, :d]) and W = W0 + dW bit for bit against torch for U [h][ldu] f64 (ldu > d; d > 256: more than one pass
    of the row's 256 threads): random values, a column of exact ties between two neighbouring floats (1 + (2 k + 1) 2^-24:
    round to even), a column 0.3 and one 0.7 of a float spacing above a float (round down, round up).  The entry takes W and dW
    with leading dimension d, so they cannot be column blocks of a wider matrix: they are the [h][d] middle of longer buffers
    filled with 7.0, and nothing before or behind them is touched (a row written ldu or dp wide would run into the next row,
    and behind the last).  W only, dW only; the refusals write nothing."""
    g = torch.Generator().manual_seed(h + d + ldu)
    U = torch.randn(h, ldu, generator=g, dtype=torch.float64)
    base = torch.randn(h, generator=g).float()
    gap = (torch.nextafter(base, torch.full_like(base, float("inf"))) - base).double()
    U[:, 0] = 1.0 + (2.0 * torch.arange(h, dtype=torch.float64) + 1.0) * 2.0 ** -24
    U[:, 1] = base.double() + 0.3 * gap
    U[:, 2] = base.double() + 0.7 * gap
    want = U[:, :d].float()
    assert torch.equal(want[:, 1], base) and torch.equal(want[:, 2], torch.nextafter(base, torch.full_like(base, float("inf"))))
    assert torch.equal(want[:, 0].double(), 1.0 + 2.0 ** -23 * 2.0 * ((torch.arange(h, dtype=torch.float64) + 1.0) // 2))
    W0 = (torch.randn(h, d, generator=g) * 0.02).to(DEV)
    Ud, want = U.to(DEV), want.to(DEV)
    guard = 1024

    def wide():
        buf = torch.full((2 * guard + h * d,), 7.0, device=DEV)
        return buf, buf[guard:guard + h * d].view(h, d)

    def untouched(buf):
        return bool((buf[:guard] == 7.0).all()) and bool((buf[guard + h * d:] == 7.0).all())

    for with_w, with_dw in ((True, True), (True, False), (False, True)):
        (wb, W), (db, dW) = wide(), wide()
        rc, msg = _apply2d(Ud, ldu, W0, W if with_w else None, dW if with_dw else None, h, d)
        assert rc == 0, msg
        if with_dw:
            assert torch.equal(dW, want), "dW != float(U[:, :d])"
        if with_w:
            assert torch.equal(W, W0 + want), "W != W0 + float(U[:, :d])"
        assert untouched(wb) and untouched(db)
        assert with_w or bool((wb == 7.0).all())
        assert with_dw or bool((db == 7.0).all())
    (wb, W), (db, dW) = wide(), wide()
    for args in ((Ud, d - 1, W0, W, dW), (Ud, ldu, W0, None, None), (Ud, ldu, None, W, dW), (Ud, ldu, None, W, None)):
        rc, msg = _apply2d(*args, h, d)
        assert rc == BAD_ARG and msg, (rc, msg)
        assert bool((wb == 7.0).all()) and bool((db == 7.0).all()), "a refused call wrote"

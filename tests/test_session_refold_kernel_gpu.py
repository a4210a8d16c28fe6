"""Releasing rows that a fold has already taken (emcid_session_refold_update_f64 + emcid_cov_factor_refactor_f64, include/emcid_hip.h)
through the binding, no encoder: the fold leaves its rows Q in an archive, the update subtracts the released ones from ``base``
again (and folds the live rows on its way), the batched refactorization gives the factor of lam C' + P_kept^T P_kept, and a step
on it solves the system of the kept rows.  The references are formed here, on the CPU in fp64: numpy's Cholesky of the primal
matrix of the kept rows and torch.linalg.solve on it.

The input recipe and the bars of tests/session_kernel_helpers.py (d = 384, h = 96, lam = 50, edit_weight 0.6, nearly collinear rows,
Cov with a 1 600 condition number; L_BAR 1e-9, U_BAR 1e-8).  The same algebra on the CPU in fp64 gives L'' within 2e-16 .. 4e-15 of
max|L| and U within 5e-15 .. 3e-14 of max|U| of these references; a step that does NOT release lies 3e-2 (one row) to 0.74 (100
rows) of max|U| away, which is the gap the 1e-3 assertions below stand on.  The values the MI355X gives are in DESIGN.md §3."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import hip
from session_kernel_helpers import D, DEV, EW, H, LAM, LEFT, L_BAR, U_BAR, _cp, _inputs, _scaled


def _step(inp, lo, n, fac, state, layer=0):
    """A preserve step of rows [lo, lo + n) on layer ``layer``; nothing is committed.  Returns U (h, d) f64 on the host."""
    K, Zc, zs_t, Cov, W0 = inp
    W = torch.empty(H, K.shape[1], dtype=torch.float32, device=DEV)
    res = hip.edit_layer_dual_preserve(K[lo:lo + n].contiguous().to(DEV), Zc[lo:lo + n].contiguous().to(DEV),
                                       zs_t[lo:lo + n].contiguous().to(DEV), fac, layer, EW, LEFT, W0.to(DEV), W, state, want_u=True,
                                       lam=LAM)
    assert int(res["ws"].info.item()) == 0 and int(fac.info.item()) == 0
    return res["U"].cpu()


def _matrix(inp, kept):
    """lam C' + Kt[kept]^T Kt[kept]"""
    Kt, _ = _scaled(*inp[:3])
    rows = Kt[list(kept)]
    return LAM * _cp(inp[3]) + rows.t() @ rows


def _u_ref(inp, kept, lo, hi):
    """U of the step of rows [lo, hi) with the rows ``kept`` in the system"""
    Kt, Rt = _scaled(*inp[:3])
    A = _matrix(inp, kept) + Kt[lo:hi].t() @ Kt[lo:hi]
    return torch.linalg.solve(A, Kt[lo:hi].t() @ Rt[lo:hi]).t()


def _factor_checks(fac, A, d, layer=0):
    """(error of the layer's L against numpy's Cholesky of A relative to its largest entry, max |X L - I|); the padding exact"""
    Lref = torch.from_numpy(np.linalg.cholesky(A.numpy()))
    Lgot = torch.tril(fac.L(layer).cpu())
    Xgot = torch.tril(fac.X(layer).cpu())
    lerr = (Lgot[:d, :d] - Lref).abs().max().item() / Lref.abs().max().item()
    ierr = (Xgot @ Lgot - torch.eye(fac.dp, dtype=torch.float64)).abs().max().item()
    if fac.dp > d:       # the padding: identity, decoupled
        assert torch.equal(Lgot[d:, :d], torch.zeros(fac.dp - d, d, dtype=torch.float64))
        assert torch.equal(Lgot[d:, d:], torch.eye(fac.dp - d, dtype=torch.float64))
    return lerr, ierr


def _base_error(base, A, d):
    got = torch.tril(base.cpu()[:d, :d])
    return (got - torch.tril(A)).abs().max().item() / A.abs().max().item()


class _Folded:
    """Steps of ``steps`` rows on fresh factors of one layer, the first ``n_fold`` steps folded with the archive's tail as the
    fold's workspace (so Q stays there), the rest left live and committed."""

    def __init__(self, inp, steps, n_fold, d=D, capacity=207, archive_rows=336):
        self.inp, self.d = inp, d
        cov = inp[3].to(DEV)
        src = hip.factor_cov([cov], LAM, EW)
        self.state = state = hip.PreservedKeys(1, d, capacity, DEV)
        lo = 0
        for n in steps[:n_fold]:
            _step(inp, lo, n, src, state)
            state.commit(n)
            lo += n
        self.fac = hip.CovFactors(1, d, DEV)
        self.base = torch.empty(1, self.fac.dp, self.fac.dp, dtype=torch.float64, device=DEV)
        self.archive = torch.zeros(archive_rows, self.fac.dp, dtype=torch.float64, device=DEV)
        hip.cov_factor_fold(src, state, 0, cov, LAM, EW, self.fac, self.base, ws=self.archive[:lo].view(-1))
        assert int(self.fac.info.item()) == 0
        self.n_archived = lo
        state.reset()
        for n in steps[n_fold:]:
            _step(inp, lo, n, self.fac, state)
            state.commit(n)
            lo += n
        self.rows = lo

    def release(self, rel):
        rel_dev = torch.tensor(rel, dtype=torch.int32, device=DEV) if len(rel) else None
        hip.session_refold_update(self.fac, self.state, 0, self.archive, self.n_archived, rel_dev, self.base)
        hip.cov_factor_refactor(self.fac)
        return int(self.fac.info.item())


def _release_case(rel, what):
    """d = 384, steps (130, 70) folded, ``rel`` released with M = 0: every check of case 1"""
    inp = _inputs(329)
    f = _Folded(inp, (130, 70), 2)
    held = _step(inp, 200, 129, f.fac, f.state)                     # the step a session that cannot release would run
    archive = f.archive.clone()
    assert f.release(rel) == 0
    assert f.fac.have_inverse == {0}
    assert torch.equal(f.archive, archive)                          # M = 0: the archive is only read
    kept = [i for i in range(200) if i not in set(rel)]
    A = _matrix(inp, kept)
    lerr, ierr = _factor_checks(f.fac, A, D)
    berr = _base_error(f.base[0], A, D)
    U = _step(inp, 200, 129, f.fac, f.state)
    ref = _u_ref(inp, kept, 200, 329)
    top = ref.abs().max().item()
    err, gap = (U - ref).abs().max().item() / top, (held - ref).abs().max().item() / top
    print(f"{what}: L'' error {lerr:.3e} of max|L|, max|X'' L'' - I| {ierr:.3e}, base {berr:.3e} of its largest entry, U of the next "
          f"step {err:.3e} of max|U|; the same step without the release {gap:.3e}")
    assert lerr <= L_BAR
    assert ierr <= 1e-9
    assert berr <= 1e-12
    assert err <= U_BAR
    assert gap >= 1e-3
    return f


def test_release_one_folded_row():
    """Case 1: release {0} of 200 folded rows, M = 0."""
    _release_case([0], "release {0}")


def test_release_rows_on_both_sides_of_a_tile_edge():
    """Case 2: release {3, 130, 131}."""
    _release_case([3, 130, 131], "release {3, 130, 131}")


def test_release_more_than_one_chunk_of_rows():
    """Case 3: rows 100 .. 198, 99 of them: more than one LDS chunk of the downdate kernel and a multiple of no power of two."""
    _release_case(list(range(100, 199)), "release rows 100-198")


def test_release_every_folded_row():
    """Case 4: all 200 go: L'' is the Cholesky factor of lam C' again."""
    f = _release_case(list(range(200)), "release all 200")
    lerr, _ = _factor_checks(f.fac, LAM * _cp(f.inp[3]), D)
    assert lerr <= L_BAR


def test_refold_with_live_rows():
    """Case 5: 130 rows folded, a step of 70 left live; the refold releases archived row 3 and live row 5 with M = 70: the factor
    of all 200 rows less those two, the 70 live rows in the archive's tail as the scaled keys, Yp and Lp only read."""
    inp = _inputs(329)
    f = _Folded(inp, (130, 70), 1)
    assert f.state.M == 70 and f.n_archived == 130
    Yp, Lp, head = f.state.Yp[0].clone(), f.state.Lp[0].clone(), f.archive[:130].clone()
    assert f.release([3, 130 + 5]) == 0
    assert torch.equal(f.state.Yp[0], Yp) and torch.equal(f.state.Lp[0], Lp) and torch.equal(f.archive[:130], head)
    Kt, _ = _scaled(*inp[:3])
    tail = f.archive[130:200].cpu()
    terr = (tail[:, :D] - Kt[130:200]).abs().max().item() / Kt.abs().max().item()
    assert torch.equal(tail[:, D:], torch.zeros(70, f.fac.dp - D, dtype=torch.float64))
    kept = [i for i in range(200) if i not in (3, 135)]
    A = _matrix(inp, kept)
    lerr, ierr = _factor_checks(f.fac, A, D)
    berr = _base_error(f.base[0], A, D)
    f.state.reset()
    U = _step(inp, 200, 129, f.fac, f.state)
    ref = _u_ref(inp, kept, 200, 329)
    err = (U - ref).abs().max().item() / ref.abs().max().item()
    print(f"refold, M = 70: archive tail {terr:.3e} of max|Kt|, L'' error {lerr:.3e}, max|X'' L'' - I| {ierr:.3e}, base {berr:.3e}, "
          f"U of the next step {err:.3e} of max|U|")
    assert terr <= 1e-12
    assert lerr <= L_BAR and ierr <= 1e-9 and berr <= 1e-12
    assert err <= U_BAR


def test_release_with_padding():
    """Case 6: d = 200 (dp = 256), 129 rows folded (one past a 128 tile), release {1, 128}: the padding block of L'' is the exact
    identity (asserted inside _factor_checks), as emcid_factor_cov_f64 leaves it."""
    d = 200
    inp = _inputs(132, d)
    f = _Folded(inp, (127, 2), 2, d=d, capacity=129, archive_rows=129)
    assert f.fac.dp == 256
    assert f.release([1, 128]) == 0
    kept = [i for i in range(129) if i not in (1, 128)]
    A = _matrix(inp, kept)
    lerr, ierr = _factor_checks(f.fac, A, d)
    berr = _base_error(f.base[0], A, d)
    pad = f.base[0].cpu()
    assert torch.equal(torch.tril(pad[d:, d:]), torch.eye(256 - d, dtype=torch.float64)) and not pad[d:, :d].any()
    print(f"d = 200: L'' error {lerr:.3e} of max|L|, max|X'' L'' - I| {ierr:.3e}, base {berr:.3e}")
    assert lerr <= L_BAR and ierr <= 1e-9 and berr <= 1e-12


def test_two_layers_one_batched_refactor():
    """Case 7: n_layers = 2, different statistics and keys per layer, the update per layer and ONE refactor call: both layers
    hold, one flag word."""
    inps = (_inputs(329), _inputs(329, D, 77))
    covs = [inp[3].to(DEV) for inp in inps]
    src = hip.factor_cov(covs, LAM, EW)
    state = hip.PreservedKeys(2, D, 207, DEV)
    for lo, n in ((0, 130), (130, 70)):
        for layer, inp in enumerate(inps):
            _step(inp, lo, n, src, state, layer)
        state.commit(n)
    fac = hip.CovFactors(2, D, DEV)
    base = torch.empty(2, fac.dp, fac.dp, dtype=torch.float64, device=DEV)
    archives = [torch.zeros(200, fac.dp, dtype=torch.float64, device=DEV) for _ in inps]
    for layer in range(2):
        hip.cov_factor_fold(src, state, layer, covs[layer], LAM, EW, fac, base, ws=archives[layer].view(-1))
    assert int(fac.info.item()) == 0
    state.reset()
    rel = [0, 64, 199]
    rel_dev = torch.tensor(rel, dtype=torch.int32, device=DEV)
    for layer in range(2):
        hip.session_refold_update(fac, state, layer, archives[layer], 200, rel_dev, base)
    hip.cov_factor_refactor(fac)
    assert int(fac.info.item()) == 0 and fac.have_inverse == {0, 1}
    kept = [i for i in range(200) if i not in rel]
    for layer, inp in enumerate(inps):
        lerr, ierr = _factor_checks(fac, _matrix(inp, kept), D, layer)
        U = _step(inp, 200, 129, fac, state, layer)
        ref = _u_ref(inp, kept, 200, 329)
        err = (U - ref).abs().max().item() / ref.abs().max().item()
        print(f"layer {layer} of 2: L'' error {lerr:.3e} of max|L|, max|X'' L'' - I| {ierr:.3e}, U of the next step {err:.3e}")
        assert lerr <= L_BAR and ierr <= 1e-9
        assert err <= U_BAR


def test_no_released_row_is_a_fold():
    """Case 8: n_rel = 0 with M = 70 live rows: the update and the batched refactor against emcid_cov_factor_fold_f64 in place on
    a copy of the same state."""
    inp = _inputs(329)
    f = _Folded(inp, (130, 70), 1)
    twin = hip.CovFactors(1, D, DEV)
    twin.buf.copy_(f.fac.buf)
    twin.lam, twin.edit_weight, twin.have_inverse = f.fac.lam, f.fac.edit_weight, {0}
    base2 = f.base.clone()
    hip.cov_factor_fold(twin, f.state, 0, None, LAM, EW, twin, base2)
    assert int(twin.info.item()) == 0
    assert f.release([]) == 0
    Lf, Lr = torch.tril(twin.L(0).cpu()), torch.tril(f.fac.L(0).cpu())
    gap = (Lf - Lr).abs().max().item() / Lf.abs().max().item()
    bgap = (torch.tril(base2[0].cpu()) - torch.tril(f.base[0].cpu())).abs().max().item()
    lerr, ierr = _factor_checks(f.fac, _matrix(inp, range(200)), D)
    print(f"n_rel = 0: L from the refold {gap:.3e} of max|L| from the fold's, base {bgap:.3e} apart; against numpy {lerr:.3e}")
    assert gap <= L_BAR
    assert lerr <= L_BAR and ierr <= 1e-9


def test_a_row_that_was_never_added_is_reported_not_faulted():
    """Case 9: the test multiplies an archive row by 1e3 and releases it: base loses 1e6 q q^T it never held, the factorization
    reports a non-positive pivot in the flag word (no fault), and after the caller's restore from its copies (what
    EditSession.release does) the workspace and base are byte for byte the copies and a step gives what it gave before.  The
    step entry itself is not bit-reproducible from one run to the next (two runs on an untouched state differ by 2e-15 of 0.63
    on the MI355X), so "what it gave" is held to 1e-12 of max|U|: fp64's 1.1e-16 times the few hundred terms of a d = 384
    contraction, chained a few times, stays below that; U_BAR is four orders wider."""
    inp = _inputs(329)
    f = _Folded(inp, (130, 70), 2)
    before = _step(inp, 200, 129, f.fac, f.state)
    keep = (f.fac.buf.clone(), f.base.clone())
    f.archive[7] *= 1e3
    code = f.release([7])
    assert code != 0
    f.fac.buf.copy_(keep[0])
    f.base.copy_(keep[1])
    f.fac.info.zero_()
    assert torch.equal(f.fac.buf, keep[0]) and torch.equal(f.base, keep[1])
    after = _step(inp, 200, 129, f.fac, f.state)
    gap = (after - before).abs().max().item() / before.abs().max().item()
    print(f"flag word after releasing a row scaled by 1e3: {code}; the step after the restore {gap:.3e} of max|U| from the one before")
    assert gap <= 1e-12

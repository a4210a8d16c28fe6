"""EditSession.fold end to end on the toy encoder with cached v* files: a session that folds its full preserved set against an fp64
recomputation of the primal system with ALL earlier keys in it, against a session that never folds, and against plain calls; what a
fold leaves alone (the engine's factor cache, a refused fold's state) and what reset() / restore() drop.
Run on the MI355X box:  python -m pytest tests/test_session_fold_gpu.py -m gpu -q"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import emcid_amd
from emcid_amd import clip_forward as cf, edit_engine as ee, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter
import session_helpers as sh
from session_helpers import BAR, DEV, _primal_step, _ratios, _weights

_fresh_caches = sh.fresh_caches(engine=True)


def _setup(tmp_path, n_req=13, k=1):
    return sh._setup(tmp_path, n_req, k)


def _run(fx, sizes, k=1, primal=False, fold_after=(), **session_kw):
    """A session over disjoint request sets of the given sizes on a fresh toy pipe.  Returns (per-step {name: dW f64 from the GPU
    weights}, per-step primal dW | None, per-step keys | None, session, pipe); ``fold_after``: steps after which fold() is called."""
    reqs, hp_d, names, cache, stats = fx
    pipe = syn.build_pipe("toy", DEV)
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, **session_kw)
    P, got, ref, keys, lo = {}, [], [], [], 0
    for t, n in enumerate(sizes):
        step = reqs[lo:lo + n]
        if primal:
            r, _, _, kk = _primal_step(pipe.text_encoder, step, hp_d, names, cache, stats, P, k)
            ref.append(r), keys.append(kk)
        before = _weights(pipe.text_encoder, names)
        sess.apply(step, cache_name=cache)
        after = _weights(pipe.text_encoder, names)
        got.append({m: after[m] - before[m] for m in names})
        if primal:
            for m in names:
                err = (got[-1][m] - ref[-1][m]).abs().max().item()
                print(f"k={k} step {t} (N={n * k}, preserved {sess.preserved}, folded {sess.folded}) {m}: err {err:.3e} "
                      f"max|dW| {ref[-1][m].abs().max().item():.3e}")
                assert err < BAR and err <= BAR * ref[-1][m].abs().max().item(), (t, m, err)
        lo += n
        if t in fold_after:
            sess.fold()
    return got, ref, keys, sess, pipe


def _close(a, b, names, what):
    for n in names:
        err, scale = (a[n] - b[n]).abs().max().item(), b[n].abs().max().item()
        print(f"{what} {n}: {err:.3e} of max|dW| {scale:.3e}")
        assert err <= BAR * scale, (what, n, err, scale)


def test_on_full_fold_keeps_the_folded_keys_preserved(tmp_path, monkeypatch):
    """capacity 10, on_full="fold", steps of 5 + 4 + 4 concepts: the third step folds the 9 preserved rows and runs.  Its dW against the
    fp64 primal recomputation with all 9 earlier keys in the system (every step is, inside _run), against a capacity-20 session
    that never folds, and against a session that calls fold() itself after step 2; max_i ||dW3 k_i|| / ||dW1 k_i|| over step 1's
    keys agrees between the folding session, the never-folding one and the primal recomputation within 1e-3 relative and is
    below half of what three plain calls give (a preserved key is a row of the system with the weight of a new one; nothing in a
    plain call's system holds it: 0.26 against 1.31 for two steps)."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    sizes = (5, 4, 4)
    got, ref, keys, sess, pipe = _run(fx, sizes, primal=True, capacity=10, on_full="fold")
    assert sess.preserved == 4 and sess.folded == 9 and sess.folds == 1 and sess.steps == 3
    assert cf.LAST_PATHS["session_folds"] == 1 and cf.LAST_PATHS["session_folded_rows"] == 9
    assert cf.LAST_PATHS["session_preserved_rows"] == 4 and cf.LAST_PATHS["session_steps"] == 3
    assert sess.private_factors is not None and sess.private_factors.cached is False
    assert all(hit[0] is not sess.private_factors for hit in ee._FACTOR_CACHE.values())
    got_never, _, _, never, _ = _run(fx, sizes, capacity=20)
    assert never.preserved == 13 and never.folded == 0 and never.private_factors is None
    _close(got[2], got_never[2], names, "step 3, folding vs never folding")
    got_explicit, _, _, explicit, _ = _run(fx, sizes, capacity=20, fold_after=(1,))
    assert explicit.preserved == 4 and explicit.folded == 9 and explicit.folds == 1
    _close(got_explicit[2], got[2], names, "step 3, fold() vs on_full='fold'")
    # three plain calls on a fresh pipe
    plain = syn.build_pipe("toy", DEV)
    dws, lo = [], 0
    for n in sizes:
        before = _weights(plain.text_encoder, names)
        em.apply_emcid_to_text_encoder(plain, reqs[lo:lo + n], EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=stats,
                                       verbose=False)
        after = _weights(plain.text_encoder, names)
        dws.append({m: after[m] - before[m] for m in names})
        lo += n
    worst = lambda r: max(v.max().item() for v in r.values())
    r_fold, r_never, r_ref, r_plain = (worst(_ratios(a[0], a[2], keys[0], names)) for a in (got, got_never, ref, dws))
    print(f"preservation ratio max_i |dW3 k_i| / |dW1 k_i|: folding session {r_fold:.4e}, never folding {r_never:.4e}, fp64 primal "
          f"{r_ref:.4e}, three plain calls {r_plain:.4e}")
    assert abs(r_fold - r_ref) <= 1e-3 * r_ref and abs(r_never - r_ref) <= 1e-3 * r_ref and abs(r_fold - r_never) <= 1e-3 * r_ref
    assert r_fold < 0.5 * r_plain


def test_multi_token_session_folds(tmp_path):
    """num_edit_tokens = 2: rows are concepts x tokens (8, then 6); capacity 10 makes the second step fold.  Every step against the
    primal recomputation."""
    fx = _setup(tmp_path, 7, k=2)
    _, _, _, sess, _ = _run(fx, (4, 3), k=2, primal=True, capacity=10, on_full="fold")
    assert sess.preserved == 6 and sess.folded == 8 and sess.folds == 1


def test_a_fold_leaves_the_factor_cache_alone(tmp_path, monkeypatch):
    """A plain call on a fresh copy of the pipe, on the same request set, before the session has folded and after: bit-identical
    edited weights, one cache entry throughout, and the cached workspace byte for byte what it was.  (The plain calls run the
    dual solver, the form whose factors a session shares.)"""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx

    def plain_call():
        p = syn.build_pipe("toy", DEV)
        monkeypatch.setenv("EMCID_SOLVER", "dual")
        em.apply_emcid_to_text_encoder(p, reqs[:5], EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=stats, verbose=False)
        monkeypatch.delenv("EMCID_SOLVER")
        return {n: get_parameter(p.text_encoder, n + ".weight").detach().clone() for n in names}

    pipe = syn.build_pipe("toy", DEV)
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, capacity=10, on_full="fold")
    sess.apply(reqs[:5], cache_name=cache)
    sess.apply(reqs[5:9], cache_name=cache)
    w_before = plain_call()
    assert len(ee._FACTOR_CACHE) == 1
    shared = next(iter(ee._FACTOR_CACHE.values()))[0]
    bytes_before = shared.buf.clone()
    sess.apply(reqs[9:13], cache_name=cache)
    assert sess.folds == 1 and sess.folded == 9
    assert len(ee._FACTOR_CACHE) == 1 and next(iter(ee._FACTOR_CACHE.values()))[0] is shared
    assert shared.cached and torch.equal(shared.buf, bytes_before) and int(shared.info.item()) == 0
    assert sess.private_factors is not shared
    w_after = plain_call()
    for n in names:
        assert torch.equal(w_before[n], w_after[n]), n


def test_reset_and_restore_drop_the_private_factors(tmp_path):
    """After a fold, reset() followed by a step is a fresh session's first step on the encoder as it is; restore() gives the
    original weights back bit for bit; both leave no private factors, no base and folded == 0."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe = syn.build_pipe("toy", DEV)
    orig = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, capacity=10, on_full="fold")
    sess.apply(reqs[:5], cache_name=cache)
    sess.apply(reqs[5:9], cache_name=cache)
    sess.fold()
    assert sess.folded == 9 and sess.private_factors is not None
    sess.reset()
    assert (sess.preserved, sess.folded, sess.folds, sess.private_factors, sess._base) == (0, 0, 0, None, None)
    assert cf.LAST_PATHS["session_folds"] == 0 and cf.LAST_PATHS["session_folded_rows"] == 0
    twin = syn.build_pipe("toy", DEV)
    twin.text_encoder.load_state_dict(pipe.text_encoder.state_dict())
    fresh = emcid_amd.EditSession(twin, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
    b0, t0 = _weights(pipe.text_encoder, names), _weights(twin.text_encoder, names)
    sess.apply(reqs[9:13], cache_name=cache)
    fresh.apply(reqs[9:13], cache_name=cache)
    b1, t1 = _weights(pipe.text_encoder, names), _weights(twin.text_encoder, names)
    _close({n: b1[n] - b0[n] for n in names}, {n: t1[n] - t0[n] for n in names}, names, "step after reset() vs a fresh session")
    assert sess.preserved == 4 and sess.folded == 0
    sess.apply(reqs[:5], cache_name=cache)
    sess.apply(reqs[5:9], cache_name=cache)          # 4 + 5 fit, + 4 fold
    assert sess.folded == 9 and sess.preserved == 4
    sess.restore()
    assert (sess.preserved, sess.folded, sess.private_factors, sess._base) == (0, 0, None, None)
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), orig[n]), n


def test_a_refused_fold_leaves_the_state_alone(tmp_path):
    """Statistics that are not positive definite — a large negative diagonal entry written into the first edited layer's Cov, the
    tensor the session's own fold reads (wrong input, not a fault) — make the fold's factorization report a pivot:
    torch.linalg.LinAlgError from fold() and from a step that has to fold, with preserved, folded, the private factors and the
    weights unchanged; with the entry put back the same step folds and runs."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe = syn.build_pipe("toy", DEV)
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, capacity=10, on_full="fold")
    sess.apply(reqs[:5], cache_name=cache)
    sess.apply(reqs[5:9], cache_name=cache)
    cov = sess._shared[1][0]
    good = cov[0, 0].item()
    cov[0, 0] = -1e4 * cov.abs().max().item()
    before = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    gauges = dict(cf.LAST_PATHS)
    with pytest.raises(torch.linalg.LinAlgError, match="not positive definite"):
        sess.fold()
    with pytest.raises(torch.linalg.LinAlgError, match="preserved"):
        sess.apply(reqs[9:13], cache_name=cache)
    assert sess.preserved == 9 and sess.folded == 0 and sess.folds == 0 and sess.steps == 2
    assert sess.private_factors is None and sess._base is None
    assert dict(cf.LAST_PATHS) == gauges
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    cov[0, 0] = good
    sess.apply(reqs[9:13], cache_name=cache)
    assert sess.preserved == 4 and sess.folded == 9 and sess.folds == 1

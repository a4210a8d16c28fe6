"""EditSession.rescale / reweight / sweep / apply(point=) end to end on the toy encoder: after a rescale the next step is the primal
system lam' C'(e') + P^T P + Kt^T Kt with the held rows P at the scale they were committed with (recomputed on the CPU in fp64); a
reweighted concept counts like one retained at the new weight; a sweep runs trial steps at several points and leaves the session
byte for byte as it was; a failed apply(point=) takes its rescale back.  The fixture recipe, the helpers and the bar are those of
tests/session_helpers.py (toy encoder, layers 1-4, lam = 50, edit_weight 0.6).
Run on the MI355X box:  python -m pytest tests/test_session_rescale_gpu.py -m gpu -q"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter
from session_helpers import BAR, DEV, _apply_checked, _held, _keys, _primal_step, _seed, _session, _setup, _weights, fresh_caches

_fresh_caches = fresh_caches(engine=True)
HOLDOUT = ["a photo of a dog", "a painting of a house by the sea", "two people walking in the rain", "a red car"]


def _params(pipe):
    return {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}


def _same_params(pipe, ref):
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), ref[n]), n


def _buffers(sess):
    k = sess.keys
    return [t.clone() for t in k.Yp + k.Lp + k.tile_inv]


def _at(fx, lam, e):
    """The fixture with the hparams of another point."""
    reqs, hp_d, names, cache, stats = fx
    return reqs, dict(hp_d, mom2_update_weight=lam, edit_weight=e), names, cache, stats


def _apply_at(sess, pipe, step, fx, point, P, what=""):
    """sess.apply(step, point=point) against the primal recomputation at that point, at the bar; returns (GPU dW, reference dW)."""
    reqs, hp_d, names, cache, stats = _at(fx, *point)
    ref, *_ = _primal_step(pipe.text_encoder, step, hp_d, names, cache, stats, P)
    before = _weights(pipe.text_encoder, names)
    sess.apply(step, cache_name=cache, point=point)
    after = _weights(pipe.text_encoder, names)
    got = {n: after[n] - before[n] for n in names}
    for n in names:
        err = (got[n] - ref[n]).abs().max().item()
        print(f"{what} {n}: err {err:.3e} max|dW| {ref[n].abs().max().item():.3e}")
        assert err <= BAR * ref[n].abs().max().item(), (what, n, err)
    return got, ref


def _point(sess):
    return sess._fixed[:2], (float(sess.hparams.mom2_update_weight), float(sess.hparams.edit_weight))


@pytest.mark.parametrize("lam,e", [(20.0, 0.4), (20.0, 0.6)])
def test_step_after_a_rescale(tmp_path, lam, e):
    """(1) apply 0-4 at (50, 0.6), rescale, apply 5-8: within 1e-4 of max|dW| of the primal recomputation at the new point whose held
    rows keep their committed scale sqrt(0.6 / 0.5).  No parameter moves in the rescale.  Measured on MI355X:
    after rescale(20, 0.4) 1.1e-6 ... 1.8e-6 of max|dW| per layer; with lam alone changed, (20, 0.6), where the rescale is exact,
    0.85e-6 ... 2.1e-6 — both what an ordinary second step of a session shows (1.0e-6 ... 1.5e-6): the offset of the fp32-rounded C'
    that a scalar cannot reproduce lies below what the fp32 forward leaves and is not visible at this level."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, report=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1 at (50, 0.6)")
    now, scale = _params(pipe), sess.keys.row_scale[:5].clone()
    sess.rescale(lam, e)
    _same_params(pipe, now)
    assert _point(sess) == ((lam, e), (lam, e)) and sess.preserved == 5 and sess.steps == 1 and sess.report() is None
    assert cf.LAST_PATHS["session_rescales"] == len(names)        # one call per edited layer, the session's first
    assert sess._shared[0].edit_weight == e                       # the rows are coordinates of the new point's factors from now on
    g = math.sqrt(1.0 / sess._shared[0].lam_ratio(lam))
    assert sess.keys.row_scale[:5].tolist() == pytest.approx([math.sqrt(0.6 / 0.5) * g] * 5, rel=1e-14)
    assert scale.tolist() == pytest.approx([math.sqrt(0.6 / 0.5)] * 5, rel=1e-14)
    _, ref, _, _ = _apply_checked(sess, pipe, reqs[5:9], _at(fx, lam, e), P, what=f"step 2 after rescale({lam:g}, {e:g})")
    assert sess.preserved == 9 and sess.steps == 2
    # report()'s drift in RAW-key units, against ||dW k_i|| from the CPU recomputation's dW and step 1's raw keys (its Kt over the
    # scale they were committed with).  The bar: every entry of dW is within BAR max|dW|, so ||dW' k - dW k|| <= BAR max|dW| ||k||_1.
    # (A row_scale multiplied by rho = sqrt(a / a') instead would be off by the factor 1.29 at (20, 0.4) and 1.58 at (20, 0.6).)
    for n in names:
        drift = sess.report()[n + ".weight"]["drift"]
        k_raw = P[n][0] / math.sqrt(0.6 / 0.5)
        want = (ref[n] @ k_raw.t()).norm(dim=0)
        bar = BAR * ref[n].abs().max().item() * k_raw.abs().sum(dim=1)
        print(f"{n}: drift {drift.tolist()} against {want.tolist()} from the recomputation (bar {bar.max().item():.2e})")
        assert drift.shape == (5,) and bool(((drift - want).abs() <= bar).all()), n
        assert bool((0.29 * want > 2 * bar).any()), n    # (a row large enough beside the bar to tell the two units apart)
    buffers, report = _buffers(sess), sess.report()
    sess.rescale(lam, e)                                # the point it is at: no launch, and the readout stays
    assert cf.LAST_PATHS["session_rescales"] == len(names) and all(torch.equal(a, b) for a, b in zip(buffers, _buffers(sess)))
    assert sess.report() is not None and torch.equal(sess.report()[names[0] + ".weight"]["drift"], report[names[0] + ".weight"]["drift"])
    _apply_checked(sess, pipe, reqs[9:12], _at(fx, lam, e), P, what="step 3 at the new point")


def test_a_rescale_that_is_not_made_misses_the_bar(tmp_path):
    """The control of (1): the same second step at (20, 0.4) in a NEW session that re-enters rows 0-4 by a retain list keys them at
    today's edit_weight, so it is not the system whose held rows keep their committed scale."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    fx2 = _at(fx, 20.0, 0.4)
    other = emcid_amd.EditSession(pipe, EMCIDHyperParams(**fx2[1]), DEV, stats_dir=stats)
    other.retain(_held(reqs[:5]))
    ref, *_ = _primal_step(pipe.text_encoder, reqs[5:9], fx2[1], names, cache, stats, {n: list(b) for n, b in P.items()})
    before = _weights(pipe.text_encoder, names)
    other.apply(reqs[5:9], cache_name=cache)
    after = _weights(pipe.text_encoder, names)
    worst = max(((after[n] - before[n]) - ref[n]).abs().max().item() / ref[n].abs().max().item() for n in names)
    print(f"a fresh session with retained rows: {worst:.3e} of max|dW| from the recomputation with the committed scale")
    assert worst > BAR


def test_reweight_counts_like_a_retain_at_the_new_weight(tmp_path):
    """(2) retain 0-4, reweight 0-1 to 4, apply 5-8: the primal system with rows 0-1 at weight 4 and 2-4 at weight 1; report()'s
    drift of rows 0-1 is smaller than in the twin that did not reweight."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, report=True)
    keys = _keys(pipe.text_encoder, reqs[:5], names)
    now = _params(pipe)
    assert sess.retain(_held(reqs[:5])) == 5
    ledger = sess.rows()
    assert sess.reweight([reqs[0], reqs[1]["source"]], 4.0) == 2
    _same_params(pipe, now)
    assert sess.preserved == 5 and sess.retained == 5 and sess.rows() == ledger
    s = math.sqrt(0.6 / 0.5)
    assert sess.keys.row_scale[:5].tolist() == pytest.approx([2 * s, 2 * s, s, s, s], rel=1e-14)
    P = {}
    _seed(P, {n: K[:2] for n, K in keys.items()}, 4.0, hp_d)
    _seed(P, {n: K[2:] for n, K in keys.items()}, 1.0, hp_d)
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="after reweight(0-1, 4)")
    drift = sess.report()[names[0] + ".weight"]["drift"]

    pipe_t, twin = _session(fx, report=True)
    twin.retain(_held(reqs[:5]))
    twin.apply(reqs[5:9], cache_name=cache)
    drift_t = twin.report()[names[0] + ".weight"]["drift"]
    print(f"drift of rows 0-1, {names[0]}: reweighted {drift[:2].tolist()}, twin {drift_t[:2].tolist()}")
    assert bool((drift[:2] < drift_t[:2]).all())
    # a second reweight to the weight they hold launches nothing
    buffers = _buffers(sess)
    n0 = cf.LAST_PATHS["session_rescales"]
    assert sess.reweight([reqs[2]["source"]], 1.0) == 1
    assert cf.LAST_PATHS["session_rescales"] == n0 and all(torch.equal(a, b) for a, b in zip(buffers, _buffers(sess)))
    with pytest.raises(KeyError, match="c9999"):
        sess.reweight(["c9999"], 2.0)


def _scorer(pipe, fx, step):
    return emcid_amd.EditScorer(pipe, step, EMCIDHyperParams(**fx[1]), DEV, holdout=HOLDOUT, cache_name=fx[3])


def test_sweep_of_a_step(tmp_path):
    """(3) apply 0-4, then sweep 5-8 over three pairs with an EditScorer: afterwards every parameter and every state tensor is
    bit-identical and preserved / rows() / steps / the point are unchanged; per pair the weights a ``visit`` captured and the score
    are those of a twin session's apply(point=pair) — WITHIN THE BAR, not bit-equal: the sweep rescales one unit factorization
    chol(C), the twin factors the fp32-rounded C' of its point — and of the primal recomputation; select_point picks from the
    returned scores.  Measured on MI355X: 0.8e-6 ... 1.7e-6 of max|dW| from the recomputation, 1.2e-7 ... 9.9e-7 from the twin, ``left``
    within 6.6e-8 and ``drift_max`` within 1.6e-7 of the twin's."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    grid = [(50.0, 0.6), (20.0, 0.4), (100.0, 0.7)]
    step = reqs[5:9]
    pipe, sess = _session(fx, report=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    scorer = _scorer(pipe, fx, step)
    now, buffers, ledger, scale, report = _params(pipe), _buffers(sess), sess.rows(), sess.keys.row_scale.clone(), sess.report()
    base = _weights(pipe.text_encoder, names)
    seen = []

    def visit(pair, p):
        assert p is pipe
        seen.append(pair)
        return {n: w - base[n] for n, w in _weights(p.text_encoder, names).items()}

    out = sess.sweep(step, grid, cache_name=cache, scorer=scorer, visit=visit)
    _same_params(pipe, now)
    assert all(torch.equal(a, b) for a, b in zip(buffers, _buffers(sess)))
    assert sess.preserved == 5 and sess.rows() == ledger and sess.steps == 1 and _point(sess) == ((50.0, 0.6), (50.0, 0.6))
    assert torch.equal(sess.keys.row_scale, scale)
    assert all(torch.equal(sess.report()[n]["drift"], report[n]["drift"]) for n in report)
    assert seen == grid and [r["point"] for r in out] == grid and all(r["error"] is None for r in out)
    assert cf.LAST_PATHS["session_sweep_points"] == 3 and cf.LAST_PATHS["sweep_cov_factorizations"] <= len(names)
    d = base[names[0]].shape[1]
    tol = 2.0 * math.sqrt(d) * BAR        # |d left| <= ||dW' k - dW k|| / ||v* - Z0||, entries of dW within BAR max|dW|: sqrt(d) BAR (1 + left)
    for pair, r in zip(grid, out):
        pipe_t, twin = _session(fx)
        twin.apply(reqs[:5], cache_name=cache)
        scorer_t = _scorer(pipe_t, fx, step)
        Pt = {n: list(b) for n, b in P.items()}
        got_t, ref = _apply_at(twin, pipe_t, step, fx, pair, Pt, what=f"twin apply(point={pair})")
        score_t = scorer_t.score()
        for n in names:
            top = ref[n].abs().max().item()
            err, apart = (r["visit"][n] - ref[n]).abs().max().item() / top, (r["visit"][n] - got_t[n]).abs().max().item() / top
            print(f"sweep point {pair} {n}: {err:.3e} of max|dW| from the primal recomputation, {apart:.3e} from the twin's apply(point=)")
            assert err <= BAR and apart <= BAR
        dl = (r["score"].left - score_t.left).abs().max().item()
        dd = (r["score"].drift_max - score_t.drift_max).abs().max().item() / score_t.drift_max.max().item()
        print(f"sweep point {pair}: left {r['score'].left.tolist()} ({dl:.3e} from the twin's), drift_max {dd:.3e} of the largest apart")
        assert dl <= tol and dd <= tol
        assert r["report"] is not None and r["report"][names[0] + ".weight"]["drift"].shape == (5,)
    scores = [r["score"] for r in out]
    pick = em.select_point(scores, max(float(s.drift_max.max()) for s in scores))
    assert pick is not None and 0 <= pick < 3
    assert em.select_point(scores, 0.0) is None
    # the session goes on as if nothing had happened
    _apply_checked(sess, pipe, step, fx, P, what="step 2 after the sweep")


def test_a_visit_that_raises_leaves_the_session_as_it_was(tmp_path):
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    sess.apply(reqs[:5], cache_name=cache)
    now, buffers, ledger = _params(pipe), _buffers(sess), sess.rows()

    def visit(pair, p):
        raise RuntimeError("stop here")

    with pytest.raises(RuntimeError, match="stop here"):
        sess.sweep(reqs[5:9], [(20.0, 0.4), (50.0, 0.6)], cache_name=cache, visit=visit)
    _same_params(pipe, now)
    assert all(torch.equal(a, b) for a, b in zip(buffers, _buffers(sess)))
    assert sess.preserved == 5 and sess.rows() == ledger and sess.steps == 1 and _point(sess) == ((50.0, 0.6), (50.0, 0.6))


def test_a_sweep_takes_the_stale_cache_retry_a_step_takes(tmp_path):
    """A weight rewritten behind the forward's caches (param.data.copy_, as tests/test_session_gpu.py does it) makes the sweep
    prepare its plan again from the live weights — once — and go on at the point that met it: every point is visited once, each is
    the primal system's on the weights as they are, and the session is as it was."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    w = get_parameter(pipe.text_encoder, "text_model.encoder.layers.0.mlp.fc1.weight")
    v = w._version
    w.data.copy_(w.data * 1.25)
    assert w._version == v                      # invisible to the version counter
    grid = [(20.0, 0.4), (50.0, 0.6)]
    refs = [_primal_step(pipe.text_encoder, reqs[5:9], _at(fx, *pt)[1], names, cache, stats, {n: list(b) for n, b in P.items()})[0]
            for pt in grid]
    now, buffers, base = _params(pipe), _buffers(sess), _weights(pipe.text_encoder, names)
    retries = cf.LAST_PATHS.get("stale_cache_retries", 0)
    seen = []

    def visit(pair, p):
        seen.append(pair)
        return {n: x - base[n] for n, x in _weights(p.text_encoder, names).items()}

    out = sess.sweep(reqs[5:9], grid, cache_name=cache, visit=visit)
    assert cf.LAST_PATHS.get("stale_cache_retries", 0) == retries + 1
    assert seen == grid and [r["point"] for r in out] == grid and all(r["error"] is None for r in out)
    for r, ref in zip(out, refs):
        for n in names:
            err = (r["visit"][n] - ref[n]).abs().max().item() / ref[n].abs().max().item()
            print(f"sweep point {r['point']} after the retry {n}: {err:.3e} of max|dW|")
            assert err <= BAR
    _same_params(pipe, now)
    assert all(torch.equal(a, b) for a, b in zip(buffers, _buffers(sess))) and sess.preserved == 5 and sess.steps == 1


def test_a_sweep_point_with_a_bad_pivot_is_marked_and_the_walk_goes_on(tmp_path, monkeypatch):
    """``hip.edit_layer_dual_preserve`` patched to run and then set its workspace's flag word at the FIRST point only: that entry
    carries the error, the others are sound; with every point spoiled the sweep raises LinAlgError; the session is as it was."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    sess.apply(reqs[:5], cache_name=cache)
    now, buffers = _params(pipe), _buffers(sess)
    real, calls, spoil = hip.edit_layer_dual_preserve, [], [len(names)]

    def spoiled(*a, **kw):
        res = real(*a, **kw)
        calls.append(1)
        if len(calls) <= spoil[0]:
            res["ws"].info.fill_(1)
        return res

    monkeypatch.setattr(hip, "edit_layer_dual_preserve", spoiled)
    out = sess.sweep(reqs[5:9], [(20.0, 0.4), (50.0, 0.6)], cache_name=cache)
    assert out[0]["error"] is not None and "pivot" in out[0]["error"] and out[1]["error"] is None
    calls.clear()
    spoil[0] = 10 ** 6
    with pytest.raises(torch.linalg.LinAlgError, match="every one"):
        sess.sweep(reqs[5:9], [(20.0, 0.4), (50.0, 0.6)], cache_name=cache)
    monkeypatch.undo()
    _same_params(pipe, now)
    assert all(torch.equal(a, b) for a, b in zip(buffers, _buffers(sess))) and sess.preserved == 5


def test_a_failed_apply_at_a_point_takes_the_rescale_back(tmp_path, monkeypatch):
    """(4) ``hip.edit_layer_dual_preserve`` patched to run and then set its workspace's flag word, as
    tests/test_session_release_gpu.py forces its rolled-back release: apply(point=) raises LinAlgError and the point, hparams, Yp, Lp,
    the tile inverses, row_scale, the factors the rows refer to and the weights are as before; the same call then succeeds."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    buffers, now, ledger, scale, shared = _buffers(sess), _params(pipe), sess.rows(), sess.keys.row_scale.clone(), sess._shared
    real = hip.edit_layer_dual_preserve

    def spoiled(*a, **kw):
        res = real(*a, **kw)
        res["ws"].info.fill_(1)
        return res

    monkeypatch.setattr(hip, "edit_layer_dual_preserve", spoiled)
    with pytest.raises(torch.linalg.LinAlgError):
        sess.apply(reqs[5:9], cache_name=cache, point=(20.0, 0.4))
    monkeypatch.undo()
    M = 5
    got = _buffers(sess)
    L = len(names)
    for i in range(L):                                  # (rows behind M are scratch a refused step may have written)
        assert torch.equal(got[i][:M], buffers[i][:M]) and torch.equal(got[L + i][:M, :M], buffers[L + i][:M, :M])
        assert torch.equal(got[2 * L + i][0, :M, :M], buffers[2 * L + i][0, :M, :M])
    assert sess.preserved == 5 and sess.steps == 1 and sess.rows() == ledger and _point(sess) == ((50.0, 0.6), (50.0, 0.6))
    assert torch.equal(sess.keys.row_scale, scale) and sess._shared is shared
    _same_params(pipe, now)
    # a forced flag in the rescale itself: nothing of the step runs, the state is back byte for byte
    real_r, calls = hip.session_rescale, []

    def spoiled_r(*a, **kw):
        res = real_r(*a, **kw)
        res["ws"].info.fill_(1)
        calls.append(1)
        return res

    monkeypatch.setattr(hip, "session_rescale", spoiled_r)
    with pytest.raises(torch.linalg.LinAlgError, match="as they were"):
        sess.rescale(20.0, 0.4)
    monkeypatch.undo()
    assert len(calls) == L                              # all layers ran before the one flag read
    got = _buffers(sess)
    for i in range(L):
        assert torch.equal(got[i][:M], buffers[i][:M]) and torch.equal(got[L + i][:M, :M], buffers[L + i][:M, :M])
    assert _point(sess) == ((50.0, 0.6), (50.0, 0.6)) and torch.equal(sess.keys.row_scale, scale) and sess._shared is shared
    _apply_at(sess, pipe, reqs[5:9], fx, (20.0, 0.4), P, what="apply(point=(20, 0.4)) after the rollbacks")
    assert _point(sess) == ((20.0, 0.4), (20.0, 0.4)) and sess.preserved == 9 and sess.steps == 2


def test_fold_after_a_rescale_stays_exact(tmp_path):
    """(5) apply 0-4, rescale(20, 0.4), fold(), apply 5-8: the rows are coordinates of the re-pointed factors, so Q = Yp L_s^T gives
    the committed keys back and the folded system is the recomputation's."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    sess.rescale(20.0, 0.4)
    sess.fold()
    assert sess.folded == 5 and sess.preserved == 0
    fx2 = _at(fx, 20.0, 0.4)
    _apply_checked(sess, pipe, reqs[5:9], fx2, P, what="step 2 on the folded factors of the new point")
    with pytest.raises(ValueError, match="folded"):
        sess.rescale(50.0, 0.6)
    with pytest.raises(ValueError, match="folded"):
        sess.sweep(reqs[9:12], [(50.0, 0.6)], cache_name=cache)
    _apply_checked(sess, pipe, reqs[9:12], fx2, P, what="step 3")


def test_private_factors_left_by_a_refold_refuse_a_rescale(tmp_path):
    """keep_folded: apply 0-4, fold(), release every folded source — ``folded`` is 0 again, but the session still steps on the
    private factors of the point of the fold.  rescale / reweight / sweep / apply(point=) are refused with everything as it was, also
    with live rows behind the refold, and the session goes on at its own point."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, keep_folded=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    sess.fold()
    assert sess.release([r["source"] for r in reqs[:5]]) == 5
    assert sess.folded == 0 and sess.preserved == 0 and sess.private_factors is not None
    now = _params(pipe)

    def refused():
        for call in (lambda: sess.rescale(20.0, 0.4), lambda: sess.sweep(reqs[9:12], [(20.0, 0.4)], cache_name=cache),
                     lambda: sess.apply(reqs[9:12], cache_name=cache, point=(20.0, 0.4))):
            with pytest.raises(ValueError, match="has folded"):
                call()
        assert _point(sess) == ((50.0, 0.6), (50.0, 0.6))
    refused()
    _same_params(pipe, now)
    P2 = {}
    _apply_checked(sess, pipe, reqs[5:9], fx, P2, what="step 2 on the private factors, every folded row released")
    buffers, now = _buffers(sess), _params(pipe)
    refused()                                           # M = 4 live rows, coordinates of the private factors
    with pytest.raises(ValueError, match="has folded"):
        sess.reweight([reqs[5]["source"]], 4.0)
    assert all(torch.equal(a, b) for a, b in zip(buffers, _buffers(sess))) and sess.preserved == 4
    _same_params(pipe, now)
    _apply_checked(sess, pipe, reqs[9:12], fx, P2, what="step 3 at the session's own point")


def test_multi_token_rescale_and_reweight(tmp_path):
    """(6) num_edit_tokens = 2: both rows of a request are reweighted, and the step after a rescale is at the bar."""
    fx = _setup(tmp_path, 7, k=2)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    P = {}
    _apply_checked(sess, pipe, reqs[:3], fx, P, k=2, what="k=2 step 1")
    sess.rescale(20.0, 0.4)
    fx2 = _at(fx, 20.0, 0.4)
    _apply_checked(sess, pipe, reqs[3:5], fx2, P, k=2, what="k=2 step 2 after the rescale")
    assert sess.preserved == 10
    assert sess.reweight([reqs[1]["source"]], 4.0) == 2
    s_old, s_new = math.sqrt(0.6 / 0.5), math.sqrt(4.0 * 0.4 / 0.5)       # held at the first point's scale; now like a retain at 4 today
    for n in names:
        P[n][0] = P[n][0].clone()
        P[n][0][2:4] *= s_new / s_old
    _apply_checked(sess, pipe, reqs[5:7], fx2, P, k=2, what="k=2 step 3 after the reweight")


def test_save_after_a_rescale_and_load(tmp_path):
    """(7) apply 0-4, rescale(20, 0.4), save; a load with hparams at the new point carries on and its next step is bit-identical to
    the unsaved twin's; hparams that hold the old point are refused."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    fx2 = _at(fx, 20.0, 0.4)
    path = tmp_path / "session.pt"
    pipe_a, A = _session(fx)
    P = {}
    _apply_checked(A, pipe_a, reqs[:5], fx, P, what="A step 1")
    A.rescale(20.0, 0.4)
    A.save(path)
    state = em._read_session_file(path)
    assert (state["fixed"]["mom2_update_weight"], state["fixed"]["edit_weight"]) == (20.0, 0.4)
    assert torch.equal(state["keys"]["row_scale"], A.keys.row_scale[:5])
    pipe_b = syn.build_pipe("toy", DEV)
    with pytest.raises(ValueError, match="saved with"):
        emcid_amd.EditSession.load(pipe_b, EMCIDHyperParams(**hp_d), path, DEV, stats_dir=stats, weights="load")
    B = emcid_amd.EditSession.load(pipe_b, EMCIDHyperParams(**fx2[1]), path, DEV, stats_dir=stats, weights="load")
    assert _point(B) == ((20.0, 0.4), (20.0, 0.4)) and B.preserved == 5 and B.rows() == A.rows()
    assert torch.equal(B.keys.row_scale[:5], A.keys.row_scale[:5])
    for i in range(len(names)):
        assert torch.equal(A.keys.Yp[i][:5], B.keys.Yp[i][:5]) and torch.equal(A.keys.Lp[i][:5, :5], B.keys.Lp[i][:5, :5])
    before_a, before_b = _weights(pipe_a.text_encoder, names), _weights(pipe_b.text_encoder, names)
    got_b, *_ = _apply_checked(B, pipe_b, reqs[5:9], fx2, {n: list(b) for n, b in P.items()}, what="B step 2 after the load")
    got_a, *_ = _apply_checked(A, pipe_a, reqs[5:9], fx2, {n: list(b) for n, b in P.items()}, what="A step 2, never loaded")
    for n in names:
        assert torch.equal(before_a[n], before_b[n])
        apart = (got_a[n] - got_b[n]).abs().max().item()
        print(f"{n}: loaded against unsaved twin {apart:.3e}")
        assert torch.equal(got_a[n], got_b[n]), n

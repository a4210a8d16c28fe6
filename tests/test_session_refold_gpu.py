"""EditSession(keep_folded=True).release across a fold, end to end on the toy encoder: a concept whose rows a fold has taken into the
base factor leaves the system again without a weight moving, the steps after it are those of the primal system lam C' + P^T P +
Kt^T Kt with the released rows taken out of P (recomputed on the CPU in fp64, folded rows or not), and a re-edit lands where a
session that still holds the old rows cannot reach.  The fixture recipe, the helpers and the bar are those of
tests/session_helpers.py (toy encoder, layers 1-4, lam = 50, edit_weight 0.6).
Run on the MI355X box:  python -m pytest tests/test_session_refold_gpu.py -m gpu -q"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import clip_forward as cf, hip, synthetic as syn
from session_helpers import _apply_checked, _held, _keys, _seed, _session, _setup, _weights, fresh_caches

_fresh_caches = fresh_caches()


def _params(pipe):
    return {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}


def _same_params(pipe, ref):
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), ref[n]), n


def _without(P, names, step, rows):
    """P with ``rows`` of the Kt block of ``step`` taken out, for every layer."""
    keep = [i for i in range(P[names[0]][step].shape[0]) if i not in rows]
    return {n: [blk[keep] if s == step else blk for s, blk in enumerate(P[n])] for n in names}


def _src(reqs):
    return [r["source"] for r in reqs]


def test_reedit_after_a_release_across_a_fold(tmp_path):
    """(1) apply 0-4, fold(), apply 5-8, release the sources of 0-1 (folded rows): the live step is folded on the way, so preserved
    == 0, folded == 7, folds == 2, released == 2, every parameter bit-identical.  The re-edit of 0-1 towards a second set of v* rows
    is within 1e-4 of max|dW| of the primal recomputation whose P lacks the two released rows; the same third step in a session that
    did not release lies more than 0.1 of max|dW| from that reference in every edited layer (fp64 on the CPU, un-folded analogue:
    0.22 .. 0.63)."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    cache2 = str(tmp_path / "cache2") + "/"
    syn.write_vstar_cache(cache2, reqs[:2], 32, seed=7, scale=0.5)
    fx2 = (reqs, hp_d, names, cache2, stats)
    pipe, sess = _session(fx, keep_folded=True, report=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    sess.fold()
    assert sess.folded_sources() == _src(reqs[:5]) and sess.sources() == [] and sess.rows() == []
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="step 2")
    now = _params(pipe)
    assert sess.release(_src(reqs[:2])) == 2
    _same_params(pipe, now)
    assert sess.preserved == 0 and sess.folded == 7 and sess.folds == 2 and sess.released == 2 and sess.steps == 2
    assert sess.report() is None
    assert cf.LAST_PATHS["session_released_rows"] == 2 and cf.LAST_PATHS["session_folded_rows"] == 7
    assert cf.LAST_PATHS["session_preserved_rows"] == 0 and cf.LAST_PATHS["session_folds"] == 2
    assert sess.folded_sources() == _src(reqs[2:9]) and sess.sources() == []
    got, ref, _, _ = _apply_checked(sess, pipe, reqs[:2], fx2, _without(P, names, 0, (0, 1)), what="re-edit after the release")
    assert sess.preserved == 2 and sess.sources() == _src(reqs[:2])

    # the same three steps and the fold without the release
    pipe_b, held = _session(fx, keep_folded=True)
    held.apply(reqs[:5], cache_name=cache)
    held.fold()
    held.apply(reqs[5:9], cache_name=cache)
    before = _weights(pipe_b.text_encoder, names)
    held.apply(reqs[:2], cache_name=cache2)
    after = _weights(pipe_b.text_encoder, names)
    assert held.preserved == 6 and held.folded == 5
    for n in names:
        top = ref[n].abs().max().item()
        away = ((after[n] - before[n]) - ref[n]).abs().max().item() / top
        print(f"{n}: released {(got[n] - ref[n]).abs().max().item() / top:.3e}, not released {away:.3f} of max|dW| from the primal "
              f"recomputation without the two rows")
        assert away > 0.1, n


def test_one_call_releases_a_folded_and_a_live_name(tmp_path):
    """(2) apply 0-4, fold(), apply 5-8, release request 1 (folded) and request 6 (live) in one call; the next step is the primal
    system without either."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, keep_folded=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    sess.fold()
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="step 2")
    now = _params(pipe)
    assert sess.release([reqs[6], reqs[1]["source"]]) == 2             # a request dict: its source is used
    _same_params(pipe, now)
    assert sess.preserved == 0 and sess.folded == 7 and sess.folds == 2 and sess.released == 2
    assert sess.folded_sources() == _src([reqs[0]] + reqs[2:6] + reqs[7:9])
    Pk = _without(_without(P, names, 0, (1,)), names, 1, (1,))
    _apply_checked(sess, pipe, reqs[9:12], fx, Pk, what="after a release of a folded and a live name")
    assert sess.preserved == 3


def test_release_of_a_retained_folded_concept(tmp_path):
    """(3) retain 0-4 at weight 4, fold(), apply 5-8, release two of the retained: retained == 3, no weight moved, and the next step
    is the primal system seeded with the three kept rows."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, keep_folded=True)
    keys = _keys(pipe.text_encoder, reqs[:5], names)
    assert sess.retain(_held(reqs[:5]), weight=4.0) == 5
    sess.fold()
    P = {}
    _seed(P, keys, 4.0, hp_d)
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="step on the folded retain list")
    now = _params(pipe)
    assert sess.release([reqs[1], reqs[3]]) == 2
    _same_params(pipe, now)
    assert sess.retained == 3 and sess.folded == 7 and sess.preserved == 0 and cf.LAST_PATHS["session_retained_rows"] == 3
    _apply_checked(sess, pipe, reqs[9:12], fx, _without(P, names, 0, (1, 3)), what="after releasing two folded retained concepts")


def test_multi_token_release_across_a_fold(tmp_path):
    """(4) num_edit_tokens = 2: both folded rows of a released request go."""
    fx = _setup(tmp_path, 7, k=2)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, keep_folded=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:3], fx, P, k=2, what="k=2 step 1")
    sess.fold()
    _apply_checked(sess, pipe, reqs[3:5], fx, P, k=2, what="k=2 step 2")
    assert sess.release([reqs[1]["source"]]) == 2
    assert sess.preserved == 0 and sess.folded == 8 and reqs[1]["source"] not in sess.folded_sources()
    _apply_checked(sess, pipe, reqs[5:7], fx, _without(P, names, 0, (2, 3)), k=2, what="k=2 after the release")


def test_release_after_chunked_folds(tmp_path):
    """(5) on_full="fold" at capacity 4: a retain list of 9 goes in chunks of 4, 4 and 1 with a fold between them (the archive grows
    on the way); a name of the FIRST chunk is released, and the next step is the primal system with the other eight."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, keep_folded=True, capacity=4, on_full="fold")
    keys = _keys(pipe.text_encoder, reqs[:9], names)
    assert sess.retain(_held(reqs[:9])) == 9
    assert sess.folds == 2 and sess.folded == 8 and sess.preserved == 1
    assert sess.folded_sources() == _src(reqs[:8]) and sess.sources() == _src(reqs[8:9])
    now = _params(pipe)
    assert sess.release([reqs[1]["source"]]) == 1
    _same_params(pipe, now)
    assert sess.folds == 3 and sess.folded == 8 and sess.preserved == 0 and sess.retained == 8
    assert sess.folded_sources() == _src([reqs[0]] + reqs[2:9])
    P = {}
    _seed(P, {n: K[[0, 2, 3, 4, 5, 6, 7, 8]] for n, K in keys.items()}, 1.0, hp_d)
    _apply_checked(sess, pipe, reqs[9:12], fx, P, what="after a release from the first chunk")


def test_release_then_fold_then_apply(tmp_path):
    """(6) apply 0-4, fold(), apply 5-8, release 0; apply 9, fold() (the archive takes the row behind the compacted ones), release 9
    and 6 across that fold; the last step is the primal system without the three."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, keep_folded=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    sess.fold()
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="step 2")
    assert sess.release([reqs[0]["source"]]) == 1 and sess.folded == 8
    P = _without(P, names, 0, (0,))
    _apply_checked(sess, pipe, reqs[9:10], fx, P, what="step 3, after the release")
    sess.fold()
    assert sess.folded == 9 and sess.folds == 3 and sess.preserved == 0
    assert sess.folded_sources() == _src(reqs[1:10])
    assert sess.release(_src([reqs[9], reqs[6]])) == 2
    assert sess.folded == 7 and sess.folds == 4 and sess.released == 3
    assert sess.folded_sources() == _src(reqs[1:6] + reqs[7:9])
    Pk = _without(_without(P, names, 1, (1,)), names, 2, (0,))
    _apply_checked(sess, pipe, reqs[10:12], fx, Pk, what="step 4, after the second release")


def test_folded_sources_before_and_after(tmp_path):
    """(7) the archive ledger: empty before a fold, the folded names after it, without the released ones after a release; rows()
    and sources() list live rows only."""
    fx = _setup(tmp_path)
    reqs = fx[0]
    pipe, sess = _session(fx, keep_folded=True)
    sess.retain(_held(reqs[:5]))
    assert sess.folded_sources() == [] and sess.sources() == _src(reqs[:5])
    sess.fold()
    assert sess.folded_sources() == _src(reqs[:5]) and sess.sources() == [] and sess.rows() == []
    assert sess._archived == 5 and all(a.shape[0] >= 5 and a.dtype == torch.float64 for a in sess._archive)
    sess.retain(_held(reqs[5:7]))
    assert sess.release(_src(reqs[1:3])) == 2
    assert sess.folded_sources() == _src([reqs[0]] + reqs[3:7]) and sess.sources() == [] and sess._archived == 5
    assert sess.retained == 5 and sess.folded == 5


def test_an_unknown_name_changes_nothing(tmp_path):
    """(8) KeyError for a name in neither ledger, alone or beside a folded one: the private factors, base, the archive and every
    counter as before."""
    fx = _setup(tmp_path)
    reqs = fx[0]
    pipe, sess = _session(fx, keep_folded=True)
    sess.retain(_held(reqs[:5]))
    sess.fold()
    sess.retain(_held(reqs[5:7]))
    state = lambda: [sess.private_factors.buf.clone(), sess._base.clone()] + [a.clone() for a in sess._archive]
    counters = lambda: (sess.preserved, sess.folded, sess.folds, sess.released, sess.retained, sess.folded_sources(), sess.sources())
    before, n_before, now = state(), counters(), _params(pipe)
    with pytest.raises(KeyError, match="c9999"):
        sess.release(["c9999"])
    with pytest.raises(KeyError, match="c9999"):
        sess.release([reqs[0]["source"], "c9999"])
    assert all(torch.equal(a, b) for a, b in zip(before, state())) and counters() == n_before
    _same_params(pipe, now)


def test_a_default_session_still_refuses_and_keeps_no_archive(tmp_path):
    """(9) without keep_folded: fold() allocates no archive and a folded name is the ValueError it was."""
    fx = _setup(tmp_path)
    reqs = fx[0]
    pipe, sess = _session(fx)
    sess.retain(_held(reqs[:5]))
    sess.fold()
    assert sess._archive is None and sess._archived == 0 and sess.folded_sources() == [] and sess.folded == 5
    with pytest.raises(ValueError, match="folded") as e:
        sess.release([reqs[0]["source"]])
    assert "releasing across a fold is not supported" in str(e.value)
    assert sess.folded == 5 and sess.released == 0


def test_reset_and_restore_drop_the_archive(tmp_path):
    """(10) reset() and restore() empty the archive and its ledger; restore() also gives the weights back."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, keep_folded=True)
    orig = _params(pipe)
    sess.apply(reqs[:5], cache_name=cache)
    sess.fold()
    assert sess._archive is not None and sess.folded_sources() == _src(reqs[:5])
    sess.reset()
    assert sess._archive is None and sess._archived == 0 and sess.folded_sources() == [] and sess.folded == 0
    with pytest.raises(KeyError):
        sess.release([reqs[0]["source"]])
    sess.apply(reqs[5:9], cache_name=cache)
    sess.fold()
    assert sess.folded_sources() == _src(reqs[5:9])
    sess.restore()
    assert sess._archive is None and sess.folded_sources() == []
    _same_params(pipe, orig)


def test_a_refused_refold_is_rolled_back(tmp_path, monkeypatch):
    """``hip.cov_factor_refactor`` patched to run and then set the flag word: ``release`` raises LinAlgError and the private
    factors, base, the archive's length and ledger, preserved and the counters are as before; the next real release succeeds
    and the step after it is at the bar."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, keep_folded=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    sess.fold()
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="step 2")
    fac = sess.private_factors
    before, now = (fac.buf.clone(), sess._base.clone(), [a[:5].clone() for a in sess._archive]), _params(pipe)
    ledger, folded = sess.rows(), sess.folded_sources()
    real, calls = hip.cov_factor_refactor, []

    def spoiled(factors):
        real(factors)
        factors.info.fill_(1)
        calls.append(1)
        return factors

    monkeypatch.setattr(hip, "cov_factor_refactor", spoiled)
    with pytest.raises(torch.linalg.LinAlgError, match="nothing was released"):
        sess.release([reqs[1]["source"]])
    monkeypatch.undo()
    assert calls == [1]                                                # all layers in one call, before the one flag read
    assert torch.equal(fac.buf, before[0]) and torch.equal(sess._base, before[1]) and int(fac.info.item()) == 0
    assert all(torch.equal(a[:5], b) for a, b in zip(sess._archive, before[2]))
    assert sess.preserved == 4 and sess.folded == 5 and sess.folds == 1 and sess.released == 0 and sess._archived == 5
    assert sess.rows() == ledger and sess.folded_sources() == folded and fac.have_inverse == {0, 1, 2, 3}
    _same_params(pipe, now)
    assert sess.release([reqs[1]["source"]]) == 1
    assert sess.preserved == 0 and sess.folded == 8 and sess.folds == 2
    _apply_checked(sess, pipe, reqs[9:12], fx, _without(P, names, 0, (1,)), what="after a rollback and a real release")

"""EditSession.release end to end on the toy encoder: a released concept's rows leave the preserved set without a weight moving, the
steps after it are those of the primal system lam C' + P^T P + Kt^T Kt with the released rows taken out of P (recomputed on the CPU in
fp64), and a re-edit lands where a session that still holds the old rows cannot reach.  The fixture recipe, the helpers and the bar
are those of tests/session_helpers.py.
Run on the MI355X box:  python -m pytest tests/test_session_release_gpu.py -m gpu -q"""
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


def _buffers(sess):
    k = sess.keys
    return [t.clone() for t in k.Yp + k.Lp + k.tile_inv]


def _without(P, names, step, rows):
    """P with ``rows`` of the Kt block of ``step`` taken out, for every layer."""
    keep = [i for i in range(P[names[0]][step].shape[0]) if i not in rows]
    return {n: [blk[keep] if s == step else blk for s, blk in enumerate(P[n])] for n in names}


def test_reedit_after_release(tmp_path):
    """(1) apply 0-4, apply 5-8, release the sources of 0-1: preserved == 7, every parameter bit-identical.  The re-edit of 0-1
    towards a second set of v* rows is within 1e-4 of max|dW| of the primal recomputation whose P lacks the two released rows; the
    same third step in a session that did not release lies more than 0.1 of max|dW| from that reference in every edited layer
    (fp64 on the CPU: 0.35 / 0.22 / 0.54 / 0.63), and leaves more of the pair's residuals in the first edited layer (CPU: 0.40 / 0.34
    against 0.62 / 0.60)."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    cache2 = str(tmp_path / "cache2") + "/"
    syn.write_vstar_cache(cache2, reqs[:2], 32, seed=7, scale=0.5)
    fx2 = (reqs, hp_d, names, cache2, stats)
    pipe, sess = _session(fx, report=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="step 2")
    assert sess.sources() == [r["source"] for r in reqs[:9]]
    assert sess.rows()[0] == (reqs[0]["source"], "edit", 1, 0) and sess.rows()[8] == (reqs[8]["source"], "edit", 2, 0)
    now = _params(pipe)
    assert sess.release([r["source"] for r in reqs[:2]]) == 2
    _same_params(pipe, now)
    assert sess.preserved == 7 and sess.released == 2 and sess.steps == 2 and sess.report() is None
    assert cf.LAST_PATHS["session_released_rows"] == 2 and cf.LAST_PATHS["session_preserved_rows"] == 7
    assert sess.sources() == [r["source"] for r in reqs[2:9]] and len(sess.rows()) == 7
    got, ref, _, _ = _apply_checked(sess, pipe, reqs[:2], fx2, _without(P, names, 0, (0, 1)), what="re-edit after release")
    assert sess.preserved == 9 and sess.rows()[-1] == (reqs[1]["source"], "edit", 3, 0)
    left = sess.report()[names[0] + ".weight"]["left"]

    # the same three steps without the release
    pipe_b, held = _session(fx, report=True)
    held.apply(reqs[:5], cache_name=cache)
    held.apply(reqs[5:9], cache_name=cache)
    before = _weights(pipe_b.text_encoder, names)
    held.apply(reqs[:2], cache_name=cache2)
    after = _weights(pipe_b.text_encoder, names)
    assert held.preserved == 11
    left_held = held.report()[names[0] + ".weight"]["left"]
    for n in names:
        top = ref[n].abs().max().item()
        away = ((after[n] - before[n]) - ref[n]).abs().max().item() / top
        print(f"{n}: released {(got[n] - ref[n]).abs().max().item() / top:.3e}, not released {away:.3f} of max|dW| from the primal "
              f"recomputation without the two rows")
        assert away > 0.1, n
    print(f"left of the re-edited pair, {names[0]}: released {left.tolist()}, not released {left_held.tolist()}")
    assert left.shape == left_held.shape == (2,)
    assert bool((left < left_held).all())


def test_release_of_a_retained_concept(tmp_path):
    """(2) retain 0-4 at weight 4, release two of them: retained == 3, no weight moved, and the apply of 5-8 is the primal system
    seeded with the three kept rows."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    keys = _keys(pipe.text_encoder, reqs[:5], names)
    now = _params(pipe)
    assert sess.retain(_held(reqs[:5]), weight=4.0) == 5
    assert sess.rows()[3] == (reqs[3]["source"], "retain", 1, 0)
    assert sess.release([reqs[1], reqs[3]]) == 2                       # request dicts: their source is used
    _same_params(pipe, now)
    assert sess.retained == 3 and sess.preserved == 3 and cf.LAST_PATHS["session_retained_rows"] == 3
    assert sess.keys.row_scale[:3].tolist() == pytest.approx([(4.0 * 0.6 / 0.5) ** 0.5] * 3, rel=1e-15)
    P = {}
    _seed(P, {n: K[[0, 2, 4]] for n, K in keys.items()}, 4.0, hp_d)
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="after releasing two retained concepts")
    assert sess.preserved == 7 and sess.retained == 3


def test_trailing_release_launches_nothing(tmp_path, monkeypatch):
    """(3) releasing the last step's sources changes no device buffer (and never reaches the library); the next step is the primal
    system without them."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="step 2")
    buffers, now = _buffers(sess), _params(pipe)

    def boom(*a, **kw):
        raise AssertionError("a release of trailing rows launches nothing")

    monkeypatch.setattr(hip, "session_release", boom)
    assert sess.release([r["source"] for r in reqs[5:9]]) == 4
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(buffers, _buffers(sess)))
    _same_params(pipe, now)
    assert sess.preserved == 5 and sess.sources() == [r["source"] for r in reqs[:5]]
    _apply_checked(sess, pipe, reqs[9:12], fx, {n: P[n][:1] for n in names}, what="after a trailing release")
    # everything: M' = 0, again without a launch
    monkeypatch.setattr(hip, "session_release", boom)
    assert sess.release(sess.sources()) == 8
    monkeypatch.undo()
    assert sess.preserved == 0 and sess.rows() == [] and sess.released == 12


def test_multi_token_release(tmp_path):
    """(4) num_edit_tokens = 2: both rows of a released request go, and the next step is at the bar."""
    fx = _setup(tmp_path, 7, k=2)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    P = {}
    _apply_checked(sess, pipe, reqs[:3], fx, P, k=2, what="k=2 step 1")
    _apply_checked(sess, pipe, reqs[3:5], fx, P, k=2, what="k=2 step 2")
    assert sess.preserved == 10
    assert sess.rows()[2:4] == [(reqs[1]["source"], "edit", 1, 0), (reqs[1]["source"], "edit", 1, 1)]
    assert sess.release([reqs[1]["source"]]) == 2
    assert sess.preserved == 8 and reqs[1]["source"] not in sess.sources()
    _apply_checked(sess, pipe, reqs[5:7], fx, _without(P, names, 0, (2, 3)), k=2, what="k=2 after release")
    assert sess.preserved == 12


def test_release_across_a_fold_is_refused(tmp_path):
    """(5) after fold(), a folded source raises ValueError with preserved, folded and the weights unchanged; a source applied after
    the fold can be released, and the step after that is the primal system with the folded rows and the kept ones."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    P = {}
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    sess.fold()
    assert sess.folded == 5 and sess.preserved == 0 and sess.rows() == [] and sess.sources() == []
    now = _params(pipe)
    with pytest.raises(ValueError, match="folded") as e:
        sess.release([reqs[0]["source"]])
    assert "restore()" in str(e.value)
    assert sess.preserved == 0 and sess.folded == 5 and sess.released == 0
    _same_params(pipe, now)
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="step 2 on the folded factors")
    with pytest.raises(ValueError, match="folded"):                    # one folded name refuses the whole call
        sess.release([reqs[5]["source"], reqs[0]["source"]])
    assert sess.preserved == 4
    with pytest.raises(KeyError, match="c9999"):
        sess.release(["c9999"])
    assert sess.release([reqs[5]["source"]]) == 1
    assert sess.preserved == 3 and sess.folded == 5
    _apply_checked(sess, pipe, reqs[9:12], fx, _without(P, names, 1, (0,)), what="after a release behind a fold")


def test_a_refused_rebuild_is_rolled_back(tmp_path, monkeypatch):
    """(6) ``hip.session_release`` patched to run and then set the workspace's flag word: ``release`` raises LinAlgError and Yp, Lp,
    the tile inverses, preserved, the ledger and row_scale are as before; the next real release succeeds."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    P = {}
    assert sess.retain(_held(reqs[9:11]), weight=4.0) == 2
    _seed(P, _keys(pipe.text_encoder, reqs[9:11], names), 4.0, hp_d)
    _apply_checked(sess, pipe, reqs[:5], fx, P, what="step 1")
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="step 2")
    buffers, now, ledger, scale = _buffers(sess), _params(pipe), sess.rows(), sess.keys.row_scale.clone()
    real, calls = hip.session_release, []

    def spoiled(*a, **kw):
        res = real(*a, **kw)
        res["ws"].info.fill_(1)
        calls.append(1)
        return res

    monkeypatch.setattr(hip, "session_release", spoiled)
    gone = [reqs[10]["source"], reqs[1]["source"]]
    with pytest.raises(torch.linalg.LinAlgError, match="nothing was released"):
        sess.release(gone)
    monkeypatch.undo()
    assert len(calls) == len(names)                                    # all layers ran before the one flag read
    assert all(torch.equal(a, b) for a, b in zip(buffers, _buffers(sess)))
    assert sess.preserved == 11 and sess.retained == 2 and sess.released == 0 and sess.rows() == ledger
    assert torch.equal(sess.keys.row_scale, scale)
    _same_params(pipe, now)
    assert sess.release(gone) == 2
    assert sess.preserved == 9 and sess.retained == 1 and sess.released == 2
    assert sess.keys.row_scale[0].item() == pytest.approx((4.0 * 0.6 / 0.5) ** 0.5) and sess.keys.row_scale[1].item() == pytest.approx((0.6 / 0.5) ** 0.5)
    Pk = _without(_without(P, names, 0, (1,)), names, 1, (1,))
    _apply_checked(sess, pipe, reqs[11:12], fx, Pk, what="after a rollback and a real release")

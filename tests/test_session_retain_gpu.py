"""EditSession.retain and EditSession(report=True) end to end on the toy encoder: a retain list moves no weight, the steps after it
are those of the primal system lam C' + P^T P + Kt^T Kt with P seeded by the scaled held keys (recomputed on the CPU in fp64 from a
hooked forward on the weights as they are), the held keys move far less than without the list, and report() says by how much.
The fixture recipe, the helpers and the bar are those of tests/session_helpers.py.
Run on the MI355X box:  python -m pytest tests/test_session_retain_gpu.py -m gpu -q"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em
from session_helpers import BAR, _apply_checked, _held, _keys, _seed, _session, _setup, _weights, fresh_caches

_fresh_caches = fresh_caches()


def test_retain_moves_no_weight_and_needs_no_targets(tmp_path, monkeypatch):
    """(1) requests with nothing but prompts and source, no cache directory, every way to a v* made to raise: all parameters
    bit-identical, preserved == retained == 5, the gauge set."""
    fx = _setup(tmp_path)
    pipe, sess = _session(fx)

    def boom(*a, **kw):
        raise AssertionError("a retain list has no targets: v* must not be looked up, read or computed")

    for name in ("load_v_stars", "_default_stage1", "_any_vstar_missing"):
        monkeypatch.setattr(em, name, boom)
    orig = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    assert sess.retain(_held(fx[0][:5])) == 5
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), orig[n]), n
    assert sess.preserved == sess.retained == 5 and sess.steps == 0 and sess.report() is None
    assert cf.LAST_PATHS["session_retained_rows"] == 5 and cf.LAST_PATHS["session_preserved_rows"] == 5
    assert sess.keys.row_scale[:5].tolist() == [(0.6 / 0.5) ** 0.5] * 5


@pytest.mark.parametrize("weight", [1.0, 4.0])
def test_step_after_retain_matches_primal_and_holds_the_keys(tmp_path, weight):
    """(2) retain(reqs[:5], weight) then apply(reqs[5:9]): every layer within 1e-4 max|dW| of the primal recomputation with P =
    sqrt(weight) s K_held.  (3) per layer, max_i ||dW k_i|| over the held keys is at most 0.5 of what a fresh session that only
    applies gives (the CPU primal gives at most 0.31 at weight 1, 0.11 at weight 4: the reference alone meets the cap), and per
    key within 1e-4 max of the primal's.  (4) report(): drift against (W_after - W_before) k_i and left against the residuals
    recomputed on the CPU, within 1e-4 of the largest."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, report=True)
    held, step = reqs[:5], reqs[5:9]
    keys = _keys(pipe.text_encoder, held, names)
    assert sess.retain(_held(held), weight=weight) == 5
    assert sess.report() is None                   # a retain list is no step
    P = {}
    _seed(P, keys, weight, hp_d)
    got, ref, rts, kts = _apply_checked(sess, pipe, step, fx, P, what=f"weight {weight}")
    assert sess.preserved == 9 and sess.retained == 5 and sess.steps == 1
    # the same step without the list
    plain_pipe, plain = _session(fx)
    b = _weights(plain_pipe.text_encoder, names)
    plain.apply(step, cache_name=cache)
    a = _weights(plain_pipe.text_encoder, names)
    rep = sess.report()
    assert set(rep) == {n + ".weight" for n in names}
    for n in names:
        mv, mv_ref, mv_plain = ((dw @ keys[n].t()).norm(dim=0) for dw in (got[n], ref[n], a[n] - b[n]))
        print(f"weight {weight} {n}: max ||dW k|| held {mv.max().item():.4f} (primal {mv_ref.max().item():.4f}), "
              f"without the list {mv_plain.max().item():.4f}")
        assert mv.max().item() <= 0.5 * mv_plain.max().item(), n
        assert (mv - mv_ref).abs().max().item() <= BAR * mv_ref.max().item(), n
        r = rep[n + ".weight"]
        assert r["drift"].shape == (5,) and r["left"].shape == (4,)
        derr = (r["drift"] - mv).abs().max().item()
        left = (rts[n] - kts[n] @ got[n].t()).norm(dim=1) / rts[n].norm(dim=1)
        lerr = (r["left"] - left).abs().max().item()
        print(f"weight {weight} {n}: report drift err {derr:.3e} of {mv.max().item():.3e}, left err {lerr:.3e} of {left.max().item():.3e}")
        assert derr <= BAR * mv.max().item(), n
        assert lerr <= BAR * left.max().item(), n


def test_capacity_raise_and_chunked_fold(tmp_path):
    """(5) capacity 10: a retain past it raises before any launch (weights, preserved, gauges untouched).  Capacity 4 with
    on_full="fold": retain of 9 requests chunks and folds (folds >= 2, retained == 9), and the following apply of 3 requests is
    the primal solve with all 9 held keys."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, capacity=10)
    assert sess.retain(_held(reqs[:5])) == 5
    now = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    gauges = dict(cf.LAST_PATHS)
    with pytest.raises(emcid_amd.PreservedSetFull, match="capacity 10"):
        sess.retain(_held(reqs[5:11]))
    assert sess.preserved == 5 and sess.retained == 5 and dict(cf.LAST_PATHS) == gauges
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), now[n]), n
    assert sess.retain(_held(reqs[5:10])) == 5 and sess.preserved == 10

    pipe, sess = _session(fx, capacity=4, on_full="fold")
    keys = _keys(pipe.text_encoder, reqs[:9], names)
    orig = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    assert sess.retain(_held(reqs[:9])) == 9
    assert sess.folds >= 2 and sess.retained == 9 and sess.preserved + sess.folded == 9
    assert cf.LAST_PATHS["session_retained_rows"] == 9 and cf.LAST_PATHS["session_folds"] == sess.folds
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), orig[n]), n
    P = {}
    _seed(P, keys, 1.0, hp_d)
    _apply_checked(sess, pipe, reqs[9:12], fx, P, what="after a chunked retain")
    assert sess.retained == 9 and sess.steps == 1


def test_retain_between_steps_takes_the_edited_weights(tmp_path):
    """(6) apply(reqs[:4]), retain(reqs[4:8]), apply(reqs[8:12]): step 3 is the primal recomputation with the retained keys taken
    on the weights step 1 left."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, report=True)
    P = {}
    _apply_checked(sess, pipe, reqs[:4], fx, P, what="step 1")
    first = sess.report()
    keys = _keys(pipe.text_encoder, reqs[4:8], names)               # on the edited weights
    assert sess.retain(_held(reqs[4:8])) == 4
    _seed(P, keys, 1.0, hp_d)
    got, _, _, _ = _apply_checked(sess, pipe, reqs[8:12], fx, P, what="step 3")
    assert sess.preserved == 12 and sess.retained == 4 and sess.steps == 2 and cf.LAST_PATHS["session_steps"] == 2
    rep = sess.report()
    for n in names:
        assert first[n + ".weight"]["drift"].shape == (0,) and rep[n + ".weight"]["drift"].shape == (8,)
        mv = (got[n] @ keys[n].t()).norm(dim=0)          # rows 4..8 of the set are the retained keys
        assert (rep[n + ".weight"]["drift"][4:] - mv).abs().max().item() <= BAR * mv.max().item(), n


def test_retain_on_the_hooked_forward(tmp_path, monkeypatch):
    """The retain call sits at the solve seam both forwards share: on the hooked HF forward it moves no weight either, and the
    step after it (on the trie forward again) is the primal system's with the same held keys."""
    from emcid_amd import edit_engine as ee
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    keys = _keys(pipe.text_encoder, reqs[:5], names)
    orig = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    hf = cf.LAST_PATHS["forward_hf"]
    monkeypatch.setattr(ee, "FORWARD_MODE", "hf")
    assert sess.retain(_held(reqs[:5]), weight=4.0) == 5
    monkeypatch.undo()
    assert cf.LAST_PATHS["forward_hf"] == hf + 1
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), orig[n]), n
    P = {}
    _seed(P, keys, 4.0, hp_d)
    _apply_checked(sess, pipe, reqs[5:9], fx, P, what="after a retain on the hooked forward")


def test_multi_token_retain(tmp_path):
    """(7) num_edit_tokens = 2: a retain request adds two rows, and the next step matches the primal."""
    fx = _setup(tmp_path, 7, k=2)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx)
    keys = _keys(pipe.text_encoder, reqs[:4], names, k=2)
    assert sess.retain(_held(reqs[:4])) == 8
    assert sess.preserved == sess.retained == 8
    P = {}
    _seed(P, keys, 1.0, hp_d)
    _apply_checked(sess, pipe, reqs[4:7], fx, P, k=2, what="k=2")
    assert sess.preserved == 14 and sess.retained == 8


def test_reset_and_restore_zero_retained(tmp_path):
    """(8) reset() and restore() zero ``retained``; restore() gives the original weights back bit for bit."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe, sess = _session(fx, report=True)
    orig = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    sess.retain(_held(reqs[:5]), weight=2.0)
    sess.apply(reqs[5:9], cache_name=cache)
    assert sess.retained == 5 and sess.preserved == 9 and sess.report() is not None
    sess.reset()
    assert sess.retained == 0 and sess.preserved == 0 and cf.LAST_PATHS["session_retained_rows"] == 0 and sess.report() is None
    sess.retain(_held(reqs[:3]))
    assert sess.retained == 3
    sess.restore()
    assert sess.retained == 0 and sess.preserved == 0
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), orig[n]), n

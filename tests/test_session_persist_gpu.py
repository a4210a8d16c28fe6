"""EditSession.save / EditSession.load end to end on the toy encoder: a session saved to a file and loaded on a NEW pipe carries on
where the saved one stopped — its next step is the primal system lam C' + P^T P + Kt^T Kt with every earlier key and every retained
row in P (recomputed on the CPU in fp64), across folds, with a ``keep_folded`` archive, after a release and at another capacity —
and a load on another encoder, other statistics or other edited weights is refused with the encoder untouched.  The fixture
recipe, the helpers and the bar are those of tests/session_helpers.py (toy encoder, layers 1-4, lam = 50, edit_weight 0.6).
Run on the MI355X box:  python -m pytest tests/test_session_persist_gpu.py -m gpu -q"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter
from session_helpers import BAR, DEV, _apply_checked, _held, _keys, _primal_step, _seed, _session, _setup, _weights, fresh_caches

_fresh_caches = fresh_caches(engine=True)


def _params(pipe):
    return {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}


def _same_params(pipe, ref):
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), ref[n]), n


def _src(reqs):
    return [r["source"] for r in reqs]


def _copy(P):
    return {n: list(blocks) for n, blocks in P.items()}


def _without(P, names, step, rows):
    """P with ``rows`` of the Kt block of ``step`` taken out, for every layer."""
    keep = [i for i in range(P[names[0]][step].shape[0]) if i not in rows]
    return {n: [blk[keep] if s == step else blk for s, blk in enumerate(P[n])] for n in names}


def _pipe_like(other):
    """A NEW toy pipe in HBM holding ``other``'s weights as they are now."""
    pipe = syn.build_pipe("toy", DEV)
    pipe.text_encoder.load_state_dict(other.text_encoder.state_dict())
    return pipe


def _load(pipe, fx, path, **kw):
    return emcid_amd.EditSession.load(pipe, EMCIDHyperParams(**fx[1]), path, DEV, stats_dir=fx[4], **kw)


def _listing(sess):
    return dict(preserved=sess.preserved, folded=sess.folded, folds=sess.folds, retained=sess.retained, released=sess.released,
                steps=sess.steps, rows=sess.rows(), sources=sess.sources(), folded_sources=sess.folded_sources(),
                capacity=sess.capacity, on_full=sess.on_full, keep_folded=sess.keep_folded, report=sess.report_on)


def _delta(pipe, sess, step, fx, cache=None):
    names = fx[2]
    before = _weights(pipe.text_encoder, names)
    sess.apply(step, cache_name=cache or fx[3])
    after = _weights(pipe.text_encoder, names)
    return {n: after[n] - before[n] for n in names}


def _print_apart(what, a, b, names):
    worst = max((a[n] - b[n]).abs().max().item() / b[n].abs().max().item() for n in names)
    print(f"{what}: max|dW_A - dW_B| / max|dW| = {worst:.3e}")
    return worst


def test_plain_resume(tmp_path):
    """(1) A: retain 9-11, apply 0-4, save.  B: loaded on a new pipe (weights="load"); C: on a pipe that already holds the edited
    weights (weights="check").  Attributes and listings are A's; B's step 5-8 is within the bar of the primal recomputation with
    step 1's keys and the retained rows in P; A's own step 5-8 is printed beside it; a fresh session on the same weights WITHOUT the
    load misses the bar in every edited layer."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    path = tmp_path / "session.pt"
    pipe_a, A = _session(fx, report=True)
    original = _params(pipe_a)
    P = {}
    _seed(P, _keys(pipe_a.text_encoder, reqs[9:12], names), 1.0, hp_d)
    assert A.retain(_held(reqs[9:12])) == 3
    _apply_checked(A, pipe_a, reqs[:5], fx, P, what="A step 1")
    now = _params(pipe_a)
    out = A.save(path)
    assert out == {"rows": 8, "folded": 0, "archived": 0, "bytes": path.stat().st_size} and out["bytes"] > 0
    assert [p.name for p in tmp_path.glob("*session.pt*")] == ["session.pt"]
    _same_params(pipe_a, now)
    assert A.report() is not None

    pipe_b = syn.build_pipe("toy", DEV)
    _same_params(pipe_b, original)
    B = _load(pipe_b, fx, path, weights="load")
    _same_params(pipe_b, now)
    assert _listing(B) == _listing(A) and B.preserved == 8 and B.retained == 3 and B.steps == 1
    assert B.rows() == [(r["source"], "retain", 1, 0) for r in reqs[9:12]] + [(r["source"], "edit", 1, 0) for r in reqs[:5]]
    assert B.report() is None and B.report_on
    LP = cf.LAST_PATHS
    assert LP["session_loaded_rows"] == 8 and LP["session_preserved_rows"] == 8 and LP["session_steps"] == 1
    assert LP["session_retained_rows"] == 3 and LP["session_folds"] == 0 and LP["session_folded_rows"] == 0
    pipe_c = _pipe_like(pipe_a)
    C = _load(pipe_c, fx, path)
    _same_params(pipe_c, now)
    assert _listing(C) == _listing(A)
    pipe_d = _pipe_like(pipe_a)                         # the control: the same weights, no loaded rows

    got_b, ref, _, _ = _apply_checked(B, pipe_b, reqs[5:9], fx, _copy(P), what="B step 2 after the load")
    assert B.preserved == 12 and B.steps == 2 and B.report() is not None
    got_a = _delta(pipe_a, A, reqs[5:9], fx)
    _print_apart("step 2, never-saved A against loaded B", got_a, got_b, names)
    fresh = emcid_amd.EditSession(pipe_d, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
    got_d = _delta(pipe_d, fresh, reqs[5:9], fx)
    for n in names:
        top = ref[n].abs().max().item()
        away = (got_d[n] - ref[n]).abs().max().item()
        print(f"{n}: without the load {away / top:.3e} of max|dW| from the primal recomputation")
        assert away > BAR * top, n


def test_resume_across_a_fold(tmp_path):
    """(2) capacity 10, on_full="fold": apply 0-4, 5-8, 9-11 (folds first), save, load; folded / folds / preserved are as saved
    and the loaded session's step 12-14 is the primal system with every earlier key in P.  A plain call gives the same weights
    before and after the load."""
    fx = _setup(tmp_path, n_req=15)
    reqs, hp_d, names, cache, stats = fx
    path = tmp_path / "session.pt"
    pipe_a, A = _session(fx, capacity=10, on_full="fold")
    P = {}
    for k, (lo, hi) in enumerate(((0, 5), (5, 9), (9, 12))):
        _apply_checked(A, pipe_a, reqs[lo:hi], fx, P, what=f"A step {k + 1}")
    assert (A.preserved, A.folded, A.folds) == (3, 9, 1)
    A.save(path)

    def plain():
        pipe = syn.build_pipe("toy", DEV)
        em.apply_emcid_to_text_encoder(pipe, reqs[:3], EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=stats, verbose=False)
        return _params(pipe)

    before = plain()
    pipe_b = syn.build_pipe("toy", DEV)
    B = _load(pipe_b, fx, path, weights="load")
    _same_params(pipe_b, _params(pipe_a))
    assert (B.preserved, B.folded, B.folds, B.steps) == (3, 9, 1, 3) and _listing(B) == _listing(A)
    assert B.sources() == _src(reqs[9:12]) and B.folded_sources() == []
    assert B.private_factors is not None and not B.private_factors.cached
    after = plain()
    assert all(torch.equal(before[n], after[n]) for n in before)
    got_b, *_ = _apply_checked(B, pipe_b, reqs[12:15], fx, _copy(P), what="B step 4 after the load")
    assert (B.preserved, B.folded) == (6, 9)
    _print_apart("step 4 across a fold, never-saved A against loaded B", _delta(pipe_a, A, reqs[12:15], fx), got_b, names)
    B.fold()                                            # a later fold of loaded and new rows finds its factors
    assert (B.preserved, B.folded, B.folds) == (0, 15, 2)


def test_resume_with_an_archive(tmp_path):
    """(3) as (2) with keep_folded=True: after the load a folded source is released and re-edited towards a second v* set, within
    the bar of the primal recomputation without the old rows."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    cache2 = str(tmp_path / "cache2") + "/"
    syn.write_vstar_cache(cache2, reqs[:2], 32, seed=7, scale=0.5)
    path = tmp_path / "session.pt"
    pipe_a, A = _session(fx, capacity=10, on_full="fold", keep_folded=True)
    P = {}
    for k, (lo, hi) in enumerate(((0, 5), (5, 9), (9, 12))):
        _apply_checked(A, pipe_a, reqs[lo:hi], fx, P, what=f"A step {k + 1}")
    assert A.save(path)["archived"] == 9
    pipe_b = syn.build_pipe("toy", DEV)
    B = _load(pipe_b, fx, path, weights="load")
    assert _listing(B) == _listing(A) and B.folded_sources() == _src(reqs[:9]) and B.keep_folded
    now = _params(pipe_b)
    assert B.release(_src(reqs[:2])) == 2
    _same_params(pipe_b, now)
    assert (B.preserved, B.folded, B.folds, B.released) == (0, 10, 2, 2) and B.folded_sources() == _src(reqs[2:12])
    _apply_checked(B, pipe_b, reqs[:2], (reqs, hp_d, names, cache2, stats), _without(P, names, 0, (0, 1)),
                   what="re-edit after load and release across the fold")
    assert B.preserved == 2 and B.sources() == _src(reqs[:2])


def test_release_after_load(tmp_path):
    """(4) apply 0-4, 5-8, save; release of a live source of either step in the loaded session gives the rows() of the session that
    releases without a load, and the next step is the primal system without the two rows."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    path = tmp_path / "session.pt"
    pipe_a, A = _session(fx)
    P = {}
    _apply_checked(A, pipe_a, reqs[:5], fx, P, what="A step 1")
    _apply_checked(A, pipe_a, reqs[5:9], fx, P, what="A step 2")
    A.save(path)
    pipe_b = syn.build_pipe("toy", DEV)
    B = _load(pipe_b, fx, path, weights="load")
    gone = [reqs[1]["source"], reqs[6]["source"]]
    assert B.release(gone) == 2 and A.release(gone) == 2
    assert B.rows() == A.rows() and _listing(B) == _listing(A) and B.preserved == 7 and B.released == 2
    Pk = _without(_without(P, names, 0, (1,)), names, 1, (1,))
    got_b, *_ = _apply_checked(B, pipe_b, reqs[9:12], fx, _copy(Pk), what="B step 3 after load and release")
    got_a, *_ = _apply_checked(A, pipe_a, reqs[9:12], fx, _copy(Pk), what="A step 3 after release")
    _print_apart("step 3 after a release, A against loaded B", got_a, got_b, names)


def test_capacity_change(tmp_path):
    """(5) saved at capacity 10 with 9 rows: loaded at 16, a step of 3 fits (on_full="raise"); at 8 < M the load is refused on the
    host, with nothing allocated."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    path = tmp_path / "session.pt"
    pipe_a, A = _session(fx, capacity=10)
    P = {}
    _apply_checked(A, pipe_a, reqs[:5], fx, P, what="A step 1")
    _apply_checked(A, pipe_a, reqs[5:9], fx, P, what="A step 2")
    A.save(path)
    with pytest.raises(emcid_amd.PreservedSetFull):
        A.apply(reqs[9:12], cache_name=cache)
    pipe_b = _pipe_like(pipe_a)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="capacity 8"):
        _load(pipe_b, fx, path, capacity=8)
    assert torch.cuda.memory_allocated() == held
    assert _load(pipe_b, fx, path).capacity == 10           # default: the file's
    B = _load(pipe_b, fx, path, capacity=16)
    assert B.capacity == 16 and B.keys.capacity == 16 and B.preserved == 9 and B.on_full == "raise"
    _apply_checked(B, pipe_b, reqs[9:12], fx, _copy(P), what="B step 3 at capacity 16")
    assert B.preserved == 12
    C = _load(_pipe_like(pipe_a), fx, path, capacity=9, on_full="fold")         # shrunk to exactly M
    assert C.capacity == 9 and C.on_full == "fold" and C.preserved == 9


def test_refusals_on_the_device(tmp_path):
    """(6) an edited weight changed by one element (weights="check"), a LayerNorm parameter changed (both modes), statistics written
    with another seed: ValueError naming what differs, and the encoder is bit for bit as the load found it."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    path = tmp_path / "session.pt"
    pipe_a, A = _session(fx)
    A.apply(reqs[:5], cache_name=cache)
    A.save(path)

    pipe_b = _pipe_like(pipe_a)
    get_parameter(pipe_b.text_encoder, names[2] + ".weight").data[3, 7] += 1e-3
    found = _params(pipe_b)
    with pytest.raises(ValueError, match=names[2].replace(".", r"\.") + r"\.weight differs"):
        _load(pipe_b, fx, path)
    _same_params(pipe_b, found)
    assert _load(pipe_b, fx, path, weights="load").preserved == 5        # (the file's weights replace the changed one)
    _same_params(pipe_b, _params(pipe_a))

    ln = next(n for n, _ in pipe_a.text_encoder.named_parameters() if n.endswith("layer_norm1.bias"))
    for mode in ("check", "load"):
        pipe_c = syn.build_pipe("toy", DEV) if mode == "load" else _pipe_like(pipe_a)
        dict(pipe_c.text_encoder.named_parameters())[ln].data[5] += 1e-3
        found = _params(pipe_c)
        with pytest.raises(ValueError, match=f"parameter '{ln}'"):
            _load(pipe_c, fx, path, weights=mode)
        _same_params(pipe_c, found)

    other = str(tmp_path / "other_stats")
    syn.write_stats_cache(other, names, 128, 1000, seed=11, t=512)
    for mode in ("check", "load"):
        pipe_d = syn.build_pipe("toy", DEV) if mode == "load" else _pipe_like(pipe_a)
        found = _params(pipe_d)
        with pytest.raises(ValueError, match=f"layer {names[0]}: the statistics of .*other_stats"):
            emcid_amd.EditSession.load(pipe_d, EMCIDHyperParams(**hp_d), path, DEV, stats_dir=other, weights=mode)
        _same_params(pipe_d, found)


def test_restore_on_a_loaded_session(tmp_path):
    """(7) restore() of a loaded session gives the weights of before the saved session's first step, bit for bit."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    path = tmp_path / "session.pt"
    pipe_a, A = _session(fx)
    original = _params(pipe_a)
    A.apply(reqs[:5], cache_name=cache)
    A.apply(reqs[5:9], cache_name=cache)
    A.save(path)
    pipe_b = syn.build_pipe("toy", DEV)
    B = _load(pipe_b, fx, path, weights="load")
    assert not all(torch.equal(p.detach(), original[n]) for n, p in pipe_b.text_encoder.named_parameters())
    B.restore()
    _same_params(pipe_b, original)
    assert B.preserved == 0 and B.steps == 0 and B.rows() == []
    empty = tmp_path / "empty.pt"                       # a session saved before any step: nothing to restore, nothing preserved
    assert emcid_amd.EditSession(pipe_b, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats).save(empty)["rows"] == 0
    E = _load(pipe_b, fx, empty)
    assert E.preserved == 0 and E.keys is None and E._orig is None
    E.restore()
    _same_params(pipe_b, original)


def test_save_leaves_the_session_as_it_was(tmp_path):
    """(8) the state tensors are bit-identical across save(), and the step after it is the twin's that never saved."""
    fx = _setup(tmp_path)
    reqs, hp_d, names, cache, stats = fx
    pipe_a, A = _session(fx)
    pipe_t, T = _session(fx)
    P = {}
    _apply_checked(A, pipe_a, reqs[:5], fx, P, what="A step 1")
    T.apply(reqs[:5], cache_name=cache)
    state = [t.clone() for ts in (A.keys.Yp, A.keys.Lp, A.keys.tile_inv) for t in ts]
    listing, now, shared = _listing(A), _params(pipe_a), A._shared
    A.save(tmp_path / "session.pt")
    assert all(torch.equal(x, y) for x, y in zip(state, [t for ts in (A.keys.Yp, A.keys.Lp, A.keys.tile_inv) for t in ts]))
    assert _listing(A) == listing and A._shared is shared and A.keys.M == 5
    _same_params(pipe_a, now)
    got_a, *_ = _apply_checked(A, pipe_a, reqs[5:9], fx, _copy(P), what="A step 2 after save")
    got_t, *_ = _apply_checked(T, pipe_t, reqs[5:9], fx, _copy(P), what="twin step 2")
    _print_apart("step 2, saved A against its twin", got_a, got_t, names)

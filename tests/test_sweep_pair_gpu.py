"""sweep_emcid_sdxl_text_encoders end to end on the toy SDXL pair of tests/test_score_pair_gpu.py (TE1 32/128 with 5 layers edited at
1-3, TE2 48/192 with 7 layers edited at 3-5 and a text projection to 24; 12 ragged requests of which the first 8 are edited).

The grid is a 2 x 2 cross of the two mom2 weights at one edit_weight plus the first triple at another edit_weight: 3 distinct
points of TE1 (the same mom2 weight at another edit_weight is another point), 3 of TE2, 5 triples.  The factorised ``score=`` path
(each encoder walked over its own points, one grid reduction) is held against the joint path (both encoders at the triple, one
``PairEditScorer.score()`` each) and against a single ``apply_emcid_to_sdxl_text_encoders`` call on a fresh pipe, at the score bar
of tests/test_score_pair_gpu.py: 1e-4 of each vector's largest entry (``BAR``); the weights at 1e-4 of the largest entry of W - W0,
the bar of tests/test_sweep_gpu.py.  Bitwise equality is not asked for: the solve's atomic assemblies need not repeat a point's
weights to the last bit."""
import copy
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDXLHyperParams
from emcid_amd.nethook import get_parameter
from session_helpers import BAR, DEV, fresh_caches
from test_score_gpu import _holdout
from test_score_pair_gpu import PROJ, _assert_params, _assert_within_bar, _params, _setup_pair, _vectors

_fresh_caches = fresh_caches(engine=True)
LA, LB, LC, LD, E, E2 = 50.0, 400.0, 80.0, 600.0, 0.5, 0.3
GRID = [(LA, LC, E), (LA, LD, E), (LB, LC, E), (LB, LD, E), (LA, LC, E2)]


def _fx(tmp_path, proj=PROJ):
    reqs, hp_d, names, cache, stats = _setup_pair(tmp_path)
    pipe = syn.build_pipe("toy", DEV, sdxl=True, projection_dim=proj)
    return reqs[:8], hp_d, names, cache, stats, _holdout(reqs), pipe


def _sweep(pipe, edit, hp_d, cache, stats, grid=GRID, **kw):
    return em.sweep_emcid_sdxl_text_encoders(pipe, edit, EMCIDXLHyperParams(**hp_d), grid, DEV, cache_name=cache, stat_dir=stats[0],
                                             stat_dir_2=stats[1], **kw)


def _gauges():
    return tuple(cf.LAST_PATHS[k] for k in ("sweep_pair_points_1", "sweep_pair_points_2", "sweep_pair_combos"))


def _edited(pipe, names):
    """Per encoder {layer name: its edited fc2 weight as it is now, a copy}."""
    return [{n: get_parameter(te, n + ".weight").detach().clone() for n in ns}
            for te, ns in zip((pipe.text_encoder, pipe.text_encoder_2), names)]


def _deltas(pipe, names, w0):
    """Per encoder {layer name: W - W0 in fp64} against ``w0`` = ``_edited`` of the original weights."""
    return [{n: w.double() - w0[i][n].double() for n, w in now.items()} for i, now in enumerate(_edited(pipe, names))]


def _distance(a, b):
    """The largest distance of two scores over their vectors, each relative to the largest entry of ``b``'s."""
    return max(float((x - y).abs().max() / y.abs().max()) for (_, x), (_, y) in zip(_vectors(a), _vectors(b)))


def _cpu_pick(scores, budget):
    """select_point's rule recomputed from the summaries' definitions on the host: among the scores whose largest pair-level
    drift_max is within the budget, the smallest median of ``left`` over the rows of both encoders (middle two averaged)."""
    best = None
    for i, s in enumerate(scores):
        if not max(s.drift_max.tolist()) <= budget:
            continue
        left = sorted(s.te1.left.tolist() + s.te2.left.tolist())
        n = len(left)
        med = left[n // 2] if n % 2 else 0.5 * (left[n // 2 - 1] + left[n // 2])
        if best is None or med < best[1]:
            best = (i, med)
    return None if best is None else best[0]


@pytest.mark.parametrize("proj", [PROJ, None])
def test_factorised_against_joint(tmp_path, proj):
    """The ``score=`` sweep: five PairEditScores from 3 + 3 encoder points and one grid launch; every vector of every score within
    the bar of the joint path's, which edits both encoders per triple and scores them together; hparams untouched, every parameter
    bit-identical afterwards; ``select_point`` on the list picks what the host recomputation picks.
    Observed on the MI355X: every vector of every triple bit-equal between the two paths, with and without the projection (at the
    toy's sizes the solve repeated each point's weights to the last bit, and the pair ratio is the same fp64 reduction in both) — the
    bar is 1e-4.  At SDXL's dimensions the summaries of this path and of one call + ``score()`` per triple agree to 3.0e-7."""
    edit, hp_d, names, cache, stats, holdout, pipe = _fx(tmp_path, proj)
    hp = EMCIDXLHyperParams(**hp_d)
    hp_before = copy.deepcopy(hp.__dict__)
    params = _params(pipe)
    replays0 = cf.LAST_PATHS["score_replays"]
    fact = em.sweep_emcid_sdxl_text_encoders(pipe, edit, hp, GRID, DEV, score=holdout, cache_name=cache, stat_dir=stats[0], stat_dir_2=stats[1])
    assert _gauges() == (3, 3, 5) and cf.LAST_PATHS["sweep_points"] == 6 and cf.LAST_PATHS["sweep_prefix_runs"] == 2
    assert cf.LAST_PATHS["score_replays"] == replays0 + 2 + 6          # the scorer's construction, then one replay per encoder point
    assert hp.__dict__ == hp_before
    _assert_params(pipe, params)
    assert len(fact) == 5 and all(isinstance(s, em.PairEditScore) for s in fact)
    assert all((s.drift_pooled is None) == (proj is None) for s in fact)
    joint = _sweep(pipe, edit, hp_d, cache, stats, visit=lambda *_: None, score=holdout)
    assert _gauges() == (3, 5, 5)          # TE1: a, b, a at e'; TE2 changes at every triple
    _assert_params(pipe, params)
    assert [v for v, _ in joint] == [None] * 5
    worst = 0.0
    for g, (s, (_, ref)) in enumerate(zip(fact, joint)):
        _assert_within_bar(s, ref, f"triple {g} factorised against joint")
        worst = max(worst, _distance(s, ref))
        assert s.sources == ref.sources and s.holdout == holdout
    print(f"[pair sweep] projection {proj}: largest distance factorised against joint {worst:.3e}")
    # the same encoder point read for two triples is the same read: bit for bit
    assert torch.equal(fact[0].te1.left, fact[1].te1.left) and torch.equal(fact[0].te2.left, fact[2].te2.left)
    assert not torch.equal(fact[0].te1.left, fact[4].te1.left)          # the same mom2 weight at another edit_weight is another point
    assert not torch.equal(fact[0].drift_max, fact[1].drift_max)
    # select_point takes the list unchanged
    drifts = sorted(float(s.drift_max.max()) for s in fact)
    for budget in (drifts[0] * 0.5, drifts[2], drifts[-1] * 2):
        assert em.select_point(fact, budget) == _cpu_pick(fact, budget), budget
    assert em.select_point(fact, drifts[0] * 0.5) is None and em.select_point(fact, drifts[-1] * 2) is not None


def test_against_a_single_call(tmp_path):
    """Inside ``visit`` both encoders hold the triple's weights: W - W0 of TE1 and of TE2 (= 2 dW) within 1e-4 of the largest entry
    of what apply_emcid_to_sdxl_text_encoders leaves on a fresh copy of the pipe at the same triple, and the triple's score within
    the bar of a PairEditScorer's around that call.
    Observed on the MI355X: at edit_weight 0.5 weights and scores bit-equal; at 0.3 — where a single call factors the fp32-rounded
    C (1 - e) / 0.5 of the reference and the sweep rescales chol(C) — weights within 9.6e-7 of the largest entry, scores 4.5e-7."""
    edit, hp_d, names, cache, stats, holdout, pipe = _fx(tmp_path)
    params, w0 = _params(pipe), _edited(pipe, names)
    seen = []

    def visit(triple, p):
        assert p is pipe
        seen.append(triple)
        return _deltas(p, names, w0)

    out = _sweep(pipe, edit, hp_d, cache, stats, visit=visit, score=holdout)
    assert seen == GRID and len(out) == 5
    _assert_params(pipe, params)
    for g in (1, 4):
        l1, l2, e = GRID[g]
        fresh = syn.build_pipe("toy", DEV, sdxl=True, projection_dim=PROJ)
        f0 = _edited(fresh, names)
        scorer = emcid_amd.PairEditScorer(fresh, edit, EMCIDXLHyperParams(**hp_d), DEV, holdout=holdout, cache_name=cache)
        em.apply_emcid_to_sdxl_text_encoders(fresh, edit, EMCIDXLHyperParams(**hp_d), DEV, mom2_weight=l1, mom2_weight_2=l2, edit_weight=e,
                                             cache_name=cache, stat_dir=stats[0], stat_dir_2=stats[1], verbose=False)
        want = _deltas(fresh, names, f0)
        for i in (0, 1):
            for n in names[i]:
                err, top = float((out[g][0][i][n] - want[i][n]).abs().max()), float(want[i][n].abs().max())
                print(f"[pair sweep] triple {g} encoder {i + 1} {n}: |sweep - call| {err:.3e}, max|W - W0| {top:.3e}")
                assert top > 0 and err <= 1e-4 * top, (g, i, n, err, top)
        _assert_within_bar(out[g][1], scorer.score(), f"triple {g} against a single call")


def test_second_apply_follows_the_flag(tmp_path, monkeypatch):
    """TE2 holds W + 2 dW at a point while SDXL_TE2_DOUBLE_APPLY holds (``left_2`` overshoots) and W + dW without it: half the
    step — within 1e-4 of its largest entry, two solves of one point — and every ``left_2`` below 1."""
    edit, hp_d, names, cache, stats, holdout, pipe = _fx(tmp_path)
    params, w0 = _params(pipe), _edited(pipe, names)
    grid = GRID[:2]
    visit = lambda triple, p: _deltas(p, names, w0)[1]
    twice = _sweep(pipe, edit, hp_d, cache, stats, grid=grid, visit=visit, score=holdout)
    monkeypatch.setattr(em, "SDXL_TE2_DOUBLE_APPLY", False)
    once = _sweep(pipe, edit, hp_d, cache, stats, grid=grid, visit=visit, score=holdout)
    fact = _sweep(pipe, edit, hp_d, cache, stats, grid=grid, score=holdout)
    _assert_params(pipe, params)
    for g in range(len(grid)):
        for n in names[1]:
            top = float(twice[g][0][n].abs().max())
            assert top > 0 and float((2.0 * once[g][0][n] - twice[g][0][n]).abs().max()) <= 1e-4 * top, (g, n)
        for s in (once[g][1], fact[g]):
            assert float(s.te2.left.max()) < 1.0, g
        _assert_within_bar(fact[g], once[g][1], f"triple {g} without the second apply")
        assert float((once[g][1].te2.left - twice[g][1].te2.left).abs().max()) > 1e-3          # (the flag is seen by the score)


def test_weights_are_restored_when_visit_raises(tmp_path):
    edit, hp_d, names, cache, stats, holdout, pipe = _fx(tmp_path)
    params, w0 = _params(pipe), _edited(pipe, names)
    calls = []

    def visit(triple, p):
        calls.append(triple)
        for i, now in enumerate(_edited(p, names)):          # both edits ARE in place here
            assert not torch.equal(now[names[i][0]], w0[i][names[i][0]])
        if len(calls) == 3:
            raise KeyError("stop at the third triple")

    with pytest.raises(KeyError):
        _sweep(pipe, edit, hp_d, cache, stats, visit=visit)
    assert calls == GRID[:3]
    _assert_params(pipe, params)
    # without visit and score: the edited weights of both encoders on the host, per triple
    out = _sweep(pipe, edit, hp_d, cache, stats, grid=GRID[:2])
    _assert_params(pipe, params)
    assert [sorted(d) for d in out[0]] == [sorted(n + ".weight" for n in ns) for ns in names]
    w = out[1][1][names[1][0] + ".weight"]
    assert w.device.type == "cpu" and w.dtype == torch.float32 and not torch.equal(w, w0[1][names[1][0]].cpu())
    assert torch.equal(out[0][0][names[0][0] + ".weight"], out[1][0][names[0][0] + ".weight"])          # TE1 was not edited again


def test_a_reported_pivot_reruns_that_encoder_point_alone(tmp_path, monkeypatch):
    """On the dual form (EMCID_SOLVER=dual) a pivot is REPORTED for TE2's second point, as
    tests/test_sweep_gpu.py::test_a_reported_pivot_on_the_dual_form_reruns_that_point_alone does it: the flag word of its rescaled
    workspace is set after the rescale (the factorised path rescales for TE1's three points, then for TE2's).  That point is
    rerun on the pivoted LU — TE2's second apply adds the rerun's own dW —, lu_fallbacks rises by one, every score stays within the
    bar of an undisturbed sweep's, and every parameter is bit-identical afterwards."""
    edit, hp_d, names, cache, stats, holdout, pipe = _fx(tmp_path)
    monkeypatch.setenv("EMCID_SOLVER", "dual")
    params = _params(pipe)
    clean = _sweep(pipe, edit, hp_d, cache, stats, score=holdout)
    real, seen, lu_calls = hip.cov_factor_rescale, [], []

    def rescale(src, a, dst=None, **k):
        out = real(src, a, dst, **k)
        seen.append(out)
        if len(seen) == 5:
            out.info.fill_(3)
        return out

    real_lu = hip.edit_layer_lu

    def edit_layer_lu(*a, **k):
        lu_calls.append(_gauges()[:2])
        return real_lu(*a, **k)

    monkeypatch.setattr(hip, "cov_factor_rescale", rescale)
    monkeypatch.setattr(hip, "edit_layer_lu", edit_layer_lu)
    lu0 = cf.LAST_PATHS.get("lu_fallbacks", 0)
    got = _sweep(pipe, edit, hp_d, cache, stats, score=holdout)
    assert cf.LAST_PATHS.get("lu_fallbacks", 0) == lu0 + 1
    assert lu_calls == [(3, 1)] * len(names[1]) and len(seen) == 6          # the LU ran for TE2's second point only
    assert _gauges() == (3, 3, 5)
    _assert_params(pipe, params)
    for g, (s, ref) in enumerate(zip(got, clean)):
        _assert_within_bar(s, ref, f"triple {g} with TE2's second point on the LU")


def test_instruction_driver_prints_one_summary_per_triple(tmp_path, capsys):
    from emcid_amd import run_emcid
    edit, hp_d, names, cache, stats, holdout, pipe = _fx(tmp_path)
    (tmp_path / "hp").mkdir()
    (tmp_path / "hp" / "toyxl.json").write_text(json.dumps(hp_d))
    ins = {"requests": edit, "hparams": "toyxl", "model_ckpt": "sdxl-1.0", "mom2_weight": 50, "mom2_weight_2": 80, "edit_weight": 0.5,
           "holdout_prompts": holdout, "sweep": [list(t) for t in GRID]}
    path = tmp_path / "ins.json"
    path.write_text(json.dumps(ins))
    want = [s.summary() for s in _sweep(pipe, edit, hp_d, cache, stats, score=holdout)]
    params = _params(pipe)
    capsys.readouterr()
    res = run_emcid.run(str(path), DEV, pipe=pipe, hparams_dir=str(tmp_path / "hp"), cache_name=cache, stats_dir=stats[0],
                        stats_dir_2=stats[1], verbose=False)
    _assert_params(pipe, params)
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == len(GRID) == len(res[3])
    for rec, triple, summary in zip(lines, GRID, want):
        assert (rec["mom2_weight"], rec["mom2_weight_2"], rec["edit_weight"]) == triple
        assert set(rec["score"]) == set(summary) and "drift_pooled_max" in rec["score"]
        for key in summary:
            assert abs(rec["score"][key] - summary[key]) <= BAR * abs(summary[key]), (triple, key)


def test_without_the_trie_forward_every_triple_is_an_ordinary_call(tmp_path, monkeypatch):
    """edit_engine.FORWARD_MODE = "hf": no stored prefix state to replay.  The sweep says so (forward_hf_fallback rises), runs one
    ordinary call per triple and encoder on the hooked forward — the weights inside ``visit`` within 1e-4 of the largest entry of
    the trie sweep's at the same triple —, sets the pair gauges to one point per triple, restores both encoders bit for bit, and
    refuses ``score=``, which has no such fallback."""
    from emcid_amd import edit_engine
    edit, hp_d, names, cache, stats, holdout, pipe = _fx(tmp_path)
    params, w0 = _params(pipe), _edited(pipe, names)
    grid = GRID[:3]
    visit = lambda triple, p: _deltas(p, names, w0)
    want = _sweep(pipe, edit, hp_d, cache, stats, grid=grid, visit=visit)
    monkeypatch.setattr(edit_engine, "FORWARD_MODE", "hf")
    p0 = dict(cf.LAST_PATHS)
    got = _sweep(pipe, edit, hp_d, cache, stats, grid=grid, visit=visit)
    assert cf.LAST_PATHS["forward_hf_fallback"] == p0["forward_hf_fallback"] + 1
    assert cf.LAST_PATHS["forward_hf"] == p0["forward_hf"] + 2 * len(grid) and cf.LAST_PATHS["forward_trie"] == p0["forward_trie"]
    assert _gauges() == (3, 3, 3)
    _assert_params(pipe, params)
    for g in range(len(grid)):
        for i in (0, 1):
            for n in names[i]:
                err, top = float((got[g][i][n] - want[g][i][n]).abs().max()), float(want[g][i][n].abs().max())
                assert top > 0 and err <= 1e-4 * top, (g, i, n, err, top)
    with pytest.raises(cf.UnsupportedEncoder):
        _sweep(pipe, edit, hp_d, cache, stats, grid=grid, score=holdout)
    _assert_params(pipe, params)

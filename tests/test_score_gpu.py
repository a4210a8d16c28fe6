"""EditScorer end to end on the toy encoder (layers 1-4, edit_weight 0.6, 12 ragged requests of which the first 8 are edited; the
holdout is the prompts of requests 8-11 plus six captions).  The reference is the HF encoder on the CPU in fp64 on copies of the
GPU's weights: ``left`` / ``cos`` from ``oracle.module_input_output_at_words`` at the last edited layer, drift from
``te(**inputs)[0]`` over each prompt's attended tokens.  Every score vector is held to the project's end-to-end bar, 1e-4 of its
largest reference entry (``BAR`` of tests/session_helpers.py).  Run on the MI355X box:  python -m pytest tests/test_score_gpu.py -m gpu -q -s"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import emcid_amd
import session_helpers as sh
from emcid_amd import clip_forward as cf, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from oracle import emcid_oracle as orc
from session_helpers import BAR, DEV, _setup, fresh_caches

_fresh_caches = fresh_caches(engine=True)
VECTORS = ("left", "cos", "drift_max", "drift_mean", "drift_eos")
GRID = [(50.0, 0.6), (500.0, 0.6), (5000.0, 0.6), (50000.0, 0.6)]


def _holdout(reqs):
    return [p.format(r["source"]) for r in reqs[8:] for p in r["prompts"]] + [c["caption"] for c in syn.make_captions(6)]


def _state(te):
    return {n: v.detach().cpu().clone() for n, v in te.state_dict().items()}


def _hf_read(state, reqs, name, holdout, k=1, dtype=torch.float64):
    """(Z (N k, h), [F_p (tokens of prompt p, h)]) in fp64 from the HF encoder on the CPU, run in ``dtype`` on the weights ``state``."""
    cpu = syn.build_pipe("toy", "cpu")
    te, tok = cpu.text_encoder, cpu.tokenizer
    te.load_state_dict(state)
    te = te.to(dtype)
    with torch.no_grad():
        if k > 1:
            Z = orc.module_input_output_at_words_multi(te, tok, reqs, name, k)[1]
            Z = Z.reshape(-1, Z.shape[-1])
        else:
            Z = orc.module_input_output_at_words(te, tok, reqs, name)[1]
        inp = orc.tokenize_prompts(holdout, tok, "cpu")
        out = te(**inp)[0]
    n = inp["attention_mask"].sum(1)
    return Z.double(), [out[p, :int(n[p])].double() for p in range(len(holdout))]


def _scores(now, base, vstar):
    """{vector: fp64} by the definitions of EditScore from two ``_hf_read`` results and the (N k, h) targets."""
    (Z, F), (Z0, F0) = now, base
    t = vstar.double()
    left = (t - Z).norm(dim=1) / (t - Z0).norm(dim=1)
    moved = (Z - Z0).norm(dim=1) * (t - Z0).norm(dim=1)
    cos = torch.where(moved > 0, ((Z - Z0) * (t - Z0)).sum(1) / moved.clamp(min=1e-300), torch.zeros_like(moved))
    ratio = [(f - f0).norm(dim=1) / f0.norm(dim=1) for f, f0 in zip(F, F0)]
    return {"left": left, "cos": cos, "drift_max": torch.stack([r.max() for r in ratio]),
            "drift_mean": torch.stack([r.mean() for r in ratio]), "drift_eos": torch.stack([r[-1] for r in ratio])}


def _errors(got, ref):
    """{vector: max |got - ref| / max |ref|}; ``got``: an EditScore or a dict like ``ref``"""
    vec = (lambda v: got[v]) if isinstance(got, dict) else (lambda v: getattr(got, v))
    return {v: float((vec(v) - ref[v]).abs().max() / ref[v].abs().max()) for v in VECTORS}


def _assert_within_bar(score, ref, what, f32=None):
    e = _errors(score, ref)
    for v in VECTORS:
        line = f"[score] {what} {v}: e_score {e[v]:.3e} (max |ref| {float(ref[v].abs().max()):.4g})"
        if f32 is not None:
            e32 = _errors(f32, ref)[v]
            line += f"  e_f32 {e32:.3e}  ratio {e[v] / e32 if e32 > 0 else float('inf'):.2f}"
        print(line)
    for v in VECTORS:
        assert e[v] <= BAR, (what, v, e[v])
    return e


def _vstar(cache, reqs, k=1):
    return orc.load_vstars(cache, reqs, use_new_compute_z=k > 1).t().contiguous()


def _fixture(tmp_path, k=1):
    reqs, hp_d, names, cache, stats = _setup(tmp_path, 12, k)
    holdout = _holdout(reqs)
    assert len(holdout) == sum(len(r["prompts"]) for r in reqs[8:]) + 6
    pipe = syn.build_pipe("toy", DEV)
    base_state = _state(pipe.text_encoder)
    scorer = emcid_amd.EditScorer(pipe, reqs[:8], EMCIDHyperParams(**hp_d), DEV, holdout=holdout, cache_name=cache)
    return reqs, hp_d, names, cache, stats, holdout, pipe, base_state, scorer


def test_score_after_a_plain_call(tmp_path):
    """apply_emcid_to_text_encoder at lam = 50: every score vector within the bar of the fp64 HF reference; the same scores from
    the fp32 HF forward on the CPU printed beside them (e_f32: the distance an fp32 forward has from the reference anyway).
    Observed on the MI355X, e_score / e_f32 relative to the largest reference entry: left 3.4e-6 / 1.1e-6, cos 1.1e-7 / 4.1e-8,
    drift_max 1.8e-7 / 1.5e-7, drift_mean 7.5e-8 / 1.3e-7, drift_eos 2.0e-7 / 1.6e-7 — the bar is 1e-4."""
    reqs, hp_d, names, cache, stats, holdout, pipe, base_state, scorer = _fixture(tmp_path)
    edit = reqs[:8]
    em.apply_emcid_to_text_encoder(pipe, edit, EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=stats, verbose=False)
    s = scorer.score()
    assert s.sources == [(r["source"], 0) for r in edit] and s.holdout == holdout
    assert all(getattr(s, v).dtype == torch.float64 and not getattr(s, v).is_cuda for v in VECTORS)
    now = _state(pipe.text_encoder)
    vs = _vstar(cache, edit)
    ref = _scores(_hf_read(now, edit, names[-1], holdout), _hf_read(base_state, edit, names[-1], holdout), vs)
    f32 = _scores(_hf_read(now, edit, names[-1], holdout, dtype=torch.float32),
                  _hf_read(base_state, edit, names[-1], holdout, dtype=torch.float32), vs)
    _assert_within_bar(s, ref, "plain call lam=50", f32)
    print(f"[score] summary {s.summary()}")
    assert 0.0 < s.summary()["left_median"] < 0.5 and s.summary()["drift_max"] > 0.1        # the edit took, and it moved the holdout
    assert torch.equal(s.drift_argmax, s.drift_argmax.round()) and bool((s.drift_argmax >= 0).all())


def test_trade_off_over_a_grid(tmp_path):
    """A ``score=`` sweep over lam in {50, 500, 5 000, 50 000}: efficacy falls and drift falls with lam, ``select_point`` under a
    drift budget of 0.6 picks lam = 5 000, every point equals a plain call + ``score()`` at that pair within the bar, and the
    encoder is bit-identical afterwards.  fp64 CPU values for this set-up (HF forward, the oracle's edit): median left — the mean
    of the middle two of the eight rows — 0.153 / 0.632 / 0.845 / 0.920, drift_max.max() 1.62 / 1.03 / 0.52 / 0.20; the MI355X
    reads the same digits.  The gaps are orders of magnitude above the bar."""
    reqs, hp_d, names, cache, stats = _setup(tmp_path, 12)
    holdout, edit = _holdout(reqs), reqs[:8]
    pipe = syn.build_pipe("toy", DEV)
    before = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    scores = em.sweep_emcid_text_encoder(pipe, edit, EMCIDHyperParams(**hp_d), GRID, DEV, cache_name=cache, stat_dir=stats, score=holdout)
    assert len(scores) == len(GRID) and all(isinstance(s, em.EditScore) for s in scores)
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    lefts = [s.summary()["left_median"] for s in scores]
    drifts = [float(s.drift_max.max()) for s in scores]
    print(f"[score] sweep median left {lefts}  drift_max.max() {drifts}")
    assert all(a < b for a, b in zip(lefts, lefts[1:])), lefts
    assert all(a > b for a, b in zip(drifts, drifts[1:])), drifts
    assert em.select_point(scores, 0.6) == 2
    for (lam, e), s in zip(GRID, scores):
        plain = syn.build_pipe("toy", DEV)
        scorer = emcid_amd.EditScorer(plain, edit, EMCIDHyperParams(**hp_d), DEV, holdout=holdout, cache_name=cache)
        em.apply_emcid_to_text_encoder(plain, edit, EMCIDHyperParams(**hp_d), DEV, mom2_weight=lam, edit_weight=e, cache_name=cache,
                                       stats_dir=stats, verbose=False)
        ref = scorer.score()
        _assert_within_bar(s, {v: getattr(ref, v) for v in VECTORS}, f"sweep point lam={lam:g} against a plain call")
    # with a visit as well: (visit's value, EditScore) per point
    both = em.sweep_emcid_text_encoder(pipe, edit, EMCIDHyperParams(**hp_d), GRID[:1], DEV, visit=lambda point, p: point,
                                       cache_name=cache, stat_dir=stats, score=holdout)
    assert both[0][0] == GRID[0] and torch.equal(both[0][1].left, scores[0].left)


def _assert_identity(s, what):
    exact = bool((s.left == 1).all()) and all(bool((getattr(s, v) == 0).all()) for v in ("cos", "drift_max", "drift_mean", "drift_eos"))
    print(f"[score] identity {what}: max |left - 1| {float((s.left - 1).abs().max()):.3e}  max drift {float(s.drift_max.max()):.3e}  "
          f"exactly 1 and 0: {exact}")
    assert float((s.left - 1).abs().max()) <= 1e-6 and float(s.drift_max.max()) <= 1e-6 and float(s.drift_mean.max()) <= 1e-6


def test_identity_and_determinism(tmp_path):
    """Before any edit, and again after the weights were put back (``plan.restore_weights()``, ``sess.restore()``): left = 1 and
    drift = 0 to 1e-6 (exactly, if the replay is deterministic: printed); two ``score()`` calls in a row are bit-identical, also
    after an edit; every parameter is bit-identical across ``score()``."""
    reqs, hp_d, names, cache, stats, holdout, pipe, base_state, scorer = _fixture(tmp_path)
    edit = reqs[:8]
    params = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    s1, s2 = scorer.score(), scorer.score()
    _assert_identity(s1, "before any edit")
    for v in VECTORS + ("resid", "resid0", "drift_argmax"):
        assert torch.equal(getattr(s1, v), getattr(s2, v)), v
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), params[n]), n
    plan = em.prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, edit, EMCIDHyperParams(**hp_d), hp_d["layers"],
                                        hp_d["mom2_update_weight"], stats, cache, verbose=False)
    em.run_checked(plan)
    edited = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    a, b = scorer.score(), scorer.score()
    assert float(a.left.max()) < 0.9
    for v in VECTORS + ("resid", "resid0", "drift_argmax"):
        assert torch.equal(getattr(a, v), getattr(b, v)), v
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), edited[n]), n
    plan.restore_weights()
    _assert_identity(scorer.score(), "after plan.restore_weights()")
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
    sess.apply(edit, cache_name=cache)
    assert float(scorer.score().left.max()) < 0.9
    sess.restore()
    _assert_identity(scorer.score(), "after sess.restore()")
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), params[n]), n


def test_two_edit_tokens(tmp_path):
    """num_edit_tokens = 2: 16 rows in "rq num" order, values within the bar of the fp64 reference."""
    reqs, hp_d, names, cache, stats, holdout, pipe, base_state, scorer = _fixture(tmp_path, k=2)
    edit = reqs[:8]
    em.apply_emcid_to_text_encoder(pipe, edit, EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=stats, verbose=False)
    s = scorer.score()
    assert s.sources == [(r["source"], t) for r in edit for t in range(2)] and s.left.shape == (16,)
    vs = _vstar(cache, edit, 2)
    ref = _scores(_hf_read(_state(pipe.text_encoder), edit, names[-1], holdout, 2), _hf_read(base_state, edit, names[-1], holdout, 2), vs)
    _assert_within_bar(s, ref, "num_edit_tokens=2")


def test_session_step(tmp_path):
    """An ``EditSession.apply`` step scored within the bar.  The session's own readout of its last edited layer, ``left`` =
    ||v* - Z|| / ||v* - Zc|| with Zc that layer's output just before ITS solve (the earlier layers already edited), shares the
    numerator with the score's ``left`` = ||v* - Z|| / ||v* - Z0|| (Z0: nothing edited); on the common denominator ||v* - Zc||,
    taken from the fp64 recomputation of the step, the two agree to 1e-4."""
    reqs, hp_d, names, cache, stats, holdout, pipe, base_state, scorer = _fixture(tmp_path)
    edit = reqs[:8]
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, report=True)
    _, _, rts, _ = sh._apply_checked(sess, pipe, edit, (reqs, hp_d, names, cache, stats), {}, what="session step")
    s = scorer.score()
    ref = _scores(_hf_read(_state(pipe.text_encoder), edit, names[-1], holdout), _hf_read(base_state, edit, names[-1], holdout),
                  _vstar(cache, edit))
    _assert_within_bar(s, ref, "session step")
    scale = (float(hp_d["edit_weight"]) / 0.5) ** 0.5
    resid_before_last = rts[names[-1]].norm(dim=1) / scale            # ||v* - Zc|| of the last edited layer (its residual is not divided)
    mine = s.resid / resid_before_last
    theirs = sess.report()[names[-1] + ".weight"]["left"]
    print(f"[score] session: score's left on the layer's denominator {mine.tolist()}\n        report's left {theirs.tolist()}")
    assert float((mine - theirs).abs().max()) <= 1e-4


def test_refusals_launch_nothing(tmp_path):
    reqs, hp_d, names, cache, stats, holdout, pipe, base_state, scorer = _fixture(tmp_path)
    edit = reqs[:8]
    hp = lambda **kw: EMCIDHyperParams(**dict(hp_d, **kw))
    params = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    gauges = dict(cf.LAST_PATHS)
    with pytest.raises(cf.UnsupportedEncoder):          # layer modules the trie forward cannot find
        emcid_amd.EditScorer(pipe, edit, hp(layer_module_tmp="text_model.encoder.nolayers.{}"), DEV, holdout=holdout, cache_name=cache)
    half = syn.build_pipe("toy", DEV)
    half.text_encoder.half()
    with pytest.raises(cf.UnsupportedEncoder, match="fp32 in HBM"):
        emcid_amd.EditScorer(half, edit, hp(), DEV, holdout=holdout, cache_name=cache)
    with pytest.raises(ValueError, match="SDXL"):
        emcid_amd.EditScorer(syn.build_pipe("toy", DEV, sdxl=True), edit, hp(), DEV, holdout=holdout, cache_name=cache)
    with pytest.raises(ValueError, match="cross-attention"):
        emcid_amd.EditScorer(pipe, edit, hp(rewrite_module_tmp="unet.down_blocks.{}.attn2.to_k"), DEV, holdout=holdout, cache_name=cache)
    with pytest.raises(ValueError, match="collective"):
        emcid_amd.EditScorer(pipe, edit, hp(), DEV, holdout=holdout, cache_name=cache, shard=em.ConceptShard(0, 2))
    with pytest.raises(FileNotFoundError, match="v\\*"):
        emcid_amd.EditScorer(pipe, edit, hp(), DEV, holdout=holdout, cache_name=str(tmp_path / "nowhere") + "/")
    assert dict(cf.LAST_PATHS) == gauges
    # a parameter other than the edited fc2 weights written in place, then replaced: score() refuses on the host
    ln = scorer.graph.final_layer_norm
    with torch.no_grad():
        ln.bias.add_(0.0)                                # (same values: only the version counter moved)
    with pytest.raises(ValueError, match="final_layer_norm.bias"):
        scorer.score()
    assert dict(cf.LAST_PATHS) == gauges
    fresh = emcid_amd.EditScorer(pipe, edit, hp(), DEV, holdout=holdout, cache_name=cache)
    gauges = dict(cf.LAST_PATHS)
    pos = fresh.graph.position_embedding
    pos.weight = torch.nn.Parameter(pos.weight.detach().clone())
    with pytest.raises(ValueError, match="position_embedding"):
        fresh.score()
    assert dict(cf.LAST_PATHS) == gauges
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), params[n]), n


def test_instruction_driver_with_holdout_prompts(tmp_path, capsys):
    """run_emcid.run on an instruction with "holdout_prompts": a plain edit prints the summary of a scorer built BEFORE the edit;
    with a "sweep" every pair's record carries its score's summary.  Both against the scorer used directly."""
    import json
    from emcid_amd import run_emcid
    reqs, hp_d, names, cache, stats = _setup(tmp_path, 12)
    holdout, edit = _holdout(reqs), reqs[:8]
    (tmp_path / "hp").mkdir()
    (tmp_path / "hp" / "toy.json").write_text(json.dumps(hp_d))
    ins = {"requests": edit, "hparams": "toy", "model_ckpt": "sd-v1.4", "mom2_weight": 50, "edit_weight": 0.6, "holdout_prompts": holdout}
    path = tmp_path / "ins.json"
    path.write_text(json.dumps(ins))
    # the same edit scored directly
    twin = syn.build_pipe("toy", DEV)
    scorer = emcid_amd.EditScorer(twin, edit, EMCIDHyperParams(**hp_d), DEV, holdout=holdout, cache_name=cache)
    em.apply_emcid_to_text_encoder(twin, edit, EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=stats, verbose=False)
    want = scorer.score().summary()
    capsys.readouterr()
    pipe = syn.build_pipe("toy", DEV)
    run_emcid.run(str(path), DEV, pipe=pipe, hparams_dir=str(tmp_path / "hp"), cache_name=cache, stats_dir=stats, verbose=False)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("edit score over")]
    assert len(line) == 1 and line[0].startswith(f"edit score over {len(holdout)} holdout prompts: ")
    got = json.loads(line[0].split(": ", 1)[1])
    assert set(got) == {"left_median", "left_max", "drift_max", "drift_median"}
    for key in want:
        assert abs(got[key] - want[key]) <= BAR * abs(want[key]), (key, got[key], want[key])
    assert 0.0 < got["left_median"] < 0.5
    # a sweep: one record per pair, each with its score
    ins["sweep"] = [list(p) for p in GRID[:3]]
    path.write_text(json.dumps(ins))
    pipe = syn.build_pipe("toy", DEV)
    before = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    direct = em.sweep_emcid_text_encoder(syn.build_pipe("toy", DEV), edit, EMCIDHyperParams(**hp_d), GRID[:3], DEV, cache_name=cache,
                                         stat_dir=stats, score=holdout)
    out = run_emcid.run(str(path), DEV, pipe=pipe, hparams_dir=str(tmp_path / "hp"), cache_name=cache, stats_dir=stats, verbose=True)
    reports = out[3]
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(reports) == 3 and printed == reports                      # one line per pair
    for rec, point, s in zip(reports, GRID[:3], direct):
        assert (rec["mom2_weight"], rec["edit_weight"]) == point and set(rec["layers"]) == {n + ".weight" for n in names}
        for key, v in s.summary().items():
            assert abs(rec["score"][key] - v) <= BAR * abs(v), (point, key)
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), before[n]), n


def test_sweep_with_score_takes_the_sweeps_own_plan(tmp_path):
    """``score=`` tokenizes and runs the request trie once (the sweep's prefix run), a missing v* file is handled by the sweep's own
    loader (here: no Stage 1 available, the loader's own error, not the scorer's), and what the scorer refuses regardless of the
    encoder is refused before the preparation."""
    reqs, hp_d, names, cache, stats = _setup(tmp_path, 12)
    holdout, edit = _holdout(reqs), reqs[:8]
    pipe = syn.build_pipe("toy", DEV)
    em.sweep_emcid_text_encoder(pipe, edit, EMCIDHyperParams(**hp_d), GRID[:2], DEV, cache_name=cache, stat_dir=stats, score=holdout)
    assert cf.LAST_PATHS["sweep_prefix_runs"] == 1 and cf.LAST_PATHS["sweep_points"] == 2
    gauges = dict(cf.LAST_PATHS)
    with pytest.raises(ValueError, match="one rank"):
        em.sweep_emcid_text_encoder(pipe, edit, EMCIDHyperParams(**hp_d), GRID[:2], DEV, cache_name=cache, stat_dir=stats, score=holdout,
                                    shard=em.ConceptShard(0, 2))
    with pytest.raises(ValueError, match="prompt strings"):
        em.sweep_emcid_text_encoder(pipe, edit, EMCIDHyperParams(**hp_d), GRID[:2], DEV, cache_name=cache, stat_dir=stats, score=[])
    assert dict(cf.LAST_PATHS) == gauges
    with pytest.raises(NotImplementedError, match="no cached v"):
        em.sweep_emcid_text_encoder(pipe, edit, EMCIDHyperParams(**hp_d), GRID[:2], DEV, cache_name=str(tmp_path / "nowhere") + "/",
                                    stat_dir=stats, score=holdout)

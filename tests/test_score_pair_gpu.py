"""PairEditScorer end to end on the toy SDXL pair (TE1 32/128 with 5 layers, edited at 1-3; TE2 48/192 with 7 layers and a text
projection to 24, edited at 3-5: the last edited layer is each encoder's penultimate one, as in the shipped SDXL configuration; 12
ragged requests of which the first 8 are edited; the holdout is the prompts of requests 8-11 plus six captions).  The reference is
the two HF encoders on the CPU in fp64 on copies of the GPU's weights: ``left`` / ``cos`` from
``oracle.module_input_output_at_words`` at the last edited layer of each encoder, drift from ``hidden_states[-2]`` of both
(``output_hidden_states=True``), each encoder's own and their concatenation, over each prompt's attended tokens, and the pooled
drift from TE2's ``text_embeds``.  Every score vector is held to the project's end-to-end bar, 1e-4 of its largest reference entry
(``BAR`` of tests/session_helpers.py); the same scores from the fp32 HF forward are printed beside it."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams, EMCIDXLHyperParams
from oracle import emcid_oracle as orc
from session_helpers import BAR, DEV, fresh_caches
from test_score_gpu import _holdout, _state

_fresh_caches = fresh_caches(engine=True)
PROJ = 24
ENCODER = ("left", "cos", "drift_max", "drift_mean", "drift_eos")
PAIR = ("drift_max", "drift_mean", "drift_eos")


def _setup_pair(tmp_path):
    reqs = syn.make_requests(12, ragged=True)
    hp_d = syn.sdxl_hparams_dict(layers=(1, 2, 3), layers_2=(3, 4, 5), mom2_update_weight=50, mom2_update_weight_2=80, mom2_n_samples=1000)
    n1 = [hp_d["rewrite_module_tmp"].format(l) for l in hp_d["layers"]]
    n2 = [hp_d["rewrite_module_tmp"].format(l) for l in hp_d["layers_2"]]
    cache, s1, s2 = str(tmp_path / "cache") + "/", str(tmp_path / "s1"), str(tmp_path / "s2")
    syn.write_vstar_cache(cache, reqs, 32, seed=1, scale=0.5)
    syn.write_vstar_cache(cache, reqs, 48, seed=5, scale=0.5, suffix="_2")
    syn.write_stats_cache(s1, n1, 128, 1000, seed=2, t=512)
    syn.write_stats_cache(s2, n2, 192, 1000, seed=3, t=768)
    return reqs, hp_d, (n1, n2), cache, (s1, s2)


def _fixture(tmp_path, proj=PROJ):
    reqs, hp_d, names, cache, stats = _setup_pair(tmp_path)
    holdout = _holdout(reqs)
    pipe = syn.build_pipe("toy", DEV, sdxl=True, projection_dim=proj)
    base = _states(pipe)
    scorer = emcid_amd.PairEditScorer(pipe, reqs[:8], EMCIDXLHyperParams(**hp_d), DEV, holdout=holdout, cache_name=cache)
    assert [len(e.graph.layers) for e in scorer.encoders] == [5, 7]          # the edited layers end at each encoder's penultimate one
    return reqs, hp_d, names, cache, stats, holdout, pipe, base, scorer


def _states(pipe):
    return _state(pipe.text_encoder), _state(pipe.text_encoder_2)


def _params(pipe):
    return {(i, n): p.detach().clone() for i, te in enumerate((pipe.text_encoder, pipe.text_encoder_2)) for n, p in te.named_parameters()}


def _assert_params(pipe, want):
    for key, p in _params(pipe).items():
        assert torch.equal(p, want[key]), key


def _apply(pipe, reqs, hp_d, cache, stats):
    em.apply_emcid_to_sdxl_text_encoders(pipe, reqs, EMCIDXLHyperParams(**hp_d), DEV, cache_name=cache, stat_dir=stats[0],
                                         stat_dir_2=stats[1], verbose=False)


def _hf_read(states, reqs, names, holdout, proj, dtype=torch.float64):
    """Per encoder (Z (N, h), [hidden_states[-2] of prompt p (tokens, h)]) and TE2's text_embeds (B, proj) | None, in fp64, from
    the HF encoders on the CPU run in ``dtype`` on the weights ``states``."""
    cpu = syn.build_pipe("toy", "cpu", sdxl=True, projection_dim=proj)
    out = []
    pooled = None
    for te, tok, state, name in ((cpu.text_encoder, cpu.tokenizer, states[0], names[0][-1]),
                                 (cpu.text_encoder_2, cpu.tokenizer_2, states[1], names[1][-1])):
        te.load_state_dict(state)
        te = te.to(dtype)
        with torch.no_grad():
            Z = orc.module_input_output_at_words(te, tok, reqs, name)[1]
            inp = orc.tokenize_prompts(holdout, tok, "cpu")
            res = te(**inp, output_hidden_states=True)
        n = inp["attention_mask"].sum(1)
        out.append((Z.double(), [res.hidden_states[-2][p, :int(n[p])].double() for p in range(len(holdout))]))
        if te is not cpu.text_encoder and proj:
            pooled = res.text_embeds.double()
    return out[0], out[1], pooled


def _reduce(ratio):
    return {"drift_max": torch.stack([r.max() for r in ratio]), "drift_mean": torch.stack([r.mean() for r in ratio]),
            "drift_eos": torch.stack([r[-1] for r in ratio])}


def _scores(now, base, vstars):
    """{"te1" | "te2" | "pair": {vector: fp64}, "drift_pooled": fp64 | None} by the definitions of PairEditScore."""
    out = {}
    for key, (Z, H), (Z0, H0), t in (("te1", now[0], base[0], vstars[0].double()), ("te2", now[1], base[1], vstars[1].double())):
        left = (t - Z).norm(dim=1) / (t - Z0).norm(dim=1)
        moved = (Z - Z0).norm(dim=1) * (t - Z0).norm(dim=1)
        cos = torch.where(moved > 0, ((Z - Z0) * (t - Z0)).sum(1) / moved.clamp(min=1e-300), torch.zeros_like(moved))
        out[key] = dict(left=left, cos=cos, **_reduce([(h - h0).norm(dim=1) / h0.norm(dim=1) for h, h0 in zip(H, H0)]))
    cat = lambda i: [torch.cat([h1, h2], dim=1) for h1, h2 in zip(i[0][1], i[1][1])]
    out["pair"] = _reduce([(h - h0).norm(dim=1) / h0.norm(dim=1) for h, h0 in zip(cat(now), cat(base))])
    out["drift_pooled"] = None if now[2] is None else (now[2] - base[2]).norm(dim=1) / base[2].norm(dim=1)
    return out


def _vectors(x, skip=()):
    """[(label, vector)] of a PairEditScore or of a ``_scores`` dict, in one order."""
    get = (lambda o, v: o[v]) if isinstance(x, dict) else getattr
    part = (lambda k: x[k]) if isinstance(x, dict) else (lambda k: x if k == "pair" else getattr(x, k))
    vs = [(f"{k}.{v}", get(part(k), v)) for k, names in (("te1", ENCODER), ("te2", ENCODER), ("pair", PAIR)) if k not in skip for v in names]
    pooled = x["drift_pooled"] if isinstance(x, dict) else x.drift_pooled
    return vs + ([("drift_pooled", pooled)] if pooled is not None else [])


def _assert_within_bar(score, ref, what, f32=None, skip=()):
    got, want = _vectors(score, skip), _vectors(ref, skip)
    low = dict(_vectors(f32, skip)) if f32 is not None else {}
    assert [k for k, _ in got] == [k for k, _ in want]
    errs = {}
    for (k, g), (_, r) in zip(got, want):
        errs[k] = float((g - r).abs().max() / r.abs().max())
        line = f"[pair score] {what} {k}: e_score {errs[k]:.3e} (max |ref| {float(r.abs().max()):.4g})"
        if k in low:
            line += f"  e_f32 {float((low[k] - r).abs().max() / r.abs().max()):.3e}"
        print(line)
    for k, e in errs.items():
        assert e <= BAR, (what, k, e)


def _vstars(cache, reqs):
    return orc.load_vstars(cache, reqs).t().contiguous(), orc.load_vstars(cache, reqs, "_2").t().contiguous()


def _all_drifts(s):
    return [s.drift_max, s.drift_mean, s.drift_eos, s.drift_argmax] + [getattr(e, v) for e in (s.te1, s.te2)
                                                                        for v in ("drift_max", "drift_mean", "drift_eos", "drift_argmax")]


def _bits(s):
    return [v for _, v in _vectors(s)] + [s.left, s.cos, s.resid, s.resid0, s.drift_argmax, s.te1.drift_argmax, s.te2.drift_argmax]


def test_before_any_edit(tmp_path):
    """On the weights of construction: left = 1 exactly for both encoders, every drift — pair, per encoder, pooled — exactly 0,
    two ``score()`` calls bit-identical, every parameter bit-identical afterwards."""
    reqs, hp_d, names, cache, stats, holdout, pipe, base, scorer = _fixture(tmp_path)
    params = _params(pipe)
    s1, s2 = scorer.score(), scorer.score()
    assert s1.sources == [(r["source"], 0, 1) for r in reqs[:8]] + [(r["source"], 0, 2) for r in reqs[:8]] and s1.holdout == holdout
    assert s1.left.shape == (16,) and s1.drift_max.shape == (len(holdout),) and s1.drift_pooled.shape == (len(holdout),)
    assert all(v.dtype == torch.float64 and not v.is_cuda for v in _bits(s1))
    assert bool((s1.te1.left == 1).all()) and bool((s1.te2.left == 1).all()) and bool((s1.cos == 0).all())
    for d in _all_drifts(s1) + [s1.drift_pooled]:
        assert bool((d == 0).all())
    for a, b in zip(_bits(s1), _bits(s2)):
        assert torch.equal(a, b)
    _assert_params(pipe, params)


def test_after_apply(tmp_path):
    """apply_emcid_to_sdxl_text_encoders (TE1 at W + dW, TE2 at W + 2 dW): every vector of te1, te2, the pair drift and the pooled
    drift within the bar of the fp64 HF reference; two calls bit-identical; parameters untouched by ``score()``.
    Observed on the MI355X, e_score / e_f32 relative to the largest reference entry: te1.left 2.2e-6 / 1.1e-6, te2.left 7.4e-7 /
    9.5e-7, pair drift_max 1.2e-7 / 1.6e-7, drift_pooled 3.7e-7 / 2.0e-7, every other vector below 3.3e-7 — the bar is 1e-4."""
    reqs, hp_d, names, cache, stats, holdout, pipe, base, scorer = _fixture(tmp_path)
    edit = reqs[:8]
    _apply(pipe, edit, hp_d, cache, stats)
    params = _params(pipe)
    s, again = scorer.score(), scorer.score()
    _assert_params(pipe, params)
    for a, b in zip(_bits(s), _bits(again)):
        assert torch.equal(a, b)
    now, vs = _states(pipe), _vstars(cache, edit)
    ref = _scores(_hf_read(now, edit, names, holdout, PROJ), _hf_read(base, edit, names, holdout, PROJ), vs)
    f32 = _scores(_hf_read(now, edit, names, holdout, PROJ, torch.float32), _hf_read(base, edit, names, holdout, PROJ, torch.float32), vs)
    _assert_within_bar(s, ref, "after apply", f32)
    print(f"[pair score] summary {s.summary()}")
    assert s.summary()["left_median_1"] < 1 and float(s.drift_max.max()) > 0 and float(s.drift_pooled.max()) > 0
    assert set(s.summary()) == {"left_median", "left_max", "drift_max", "drift_median", "left_median_1", "left_median_2", "drift_pooled_max"}
    assert torch.equal(s.drift_argmax, s.drift_argmax.round()) and bool((s.drift_argmax >= 0).all())
    assert torch.equal(s.left, torch.cat([s.te1.left, s.te2.left]))
    assert em.select_point([s], 1e9) == 0 and em.select_point([s], 0.0) is None


def test_after_execute_only_the_second_encoder_moved(tmp_path):
    """execute_emcid_sd_xl_text_encoders restores TE1 and leaves TE2 edited: te1 reads left = 1 and drift 0 exactly, while the pair
    drift — TE2's numerator over BOTH encoders' denominator — and the pooled drift are non-zero and within the bar."""
    reqs, hp_d, names, cache, stats, holdout, pipe, base, scorer = _fixture(tmp_path)
    edit = reqs[:8]
    em.execute_emcid_sd_xl_text_encoders(pipe, edit, EMCIDXLHyperParams(**hp_d), cache_name=cache, verbose=False, stat_dir=stats[0],
                                         stat_dir_2=stats[1])
    s = scorer.score()
    assert bool((s.te1.left == 1).all()) and bool((s.te1.cos == 0).all())
    for v in ("drift_max", "drift_mean", "drift_eos", "drift_argmax"):
        assert bool((getattr(s.te1, v) == 0).all()), v
    assert float(s.drift_max.min()) > 0 and float(s.drift_pooled.min()) > 0 and float(s.te2.left.max()) < 1
    assert bool((s.drift_max < s.te2.drift_max).all())             # (the same numerator over a larger denominator)
    ref = _scores(_hf_read(_states(pipe), edit, names, holdout, PROJ), _hf_read(base, edit, names, holdout, PROJ), _vstars(cache, edit))
    assert float(ref["te1"]["drift_max"].max()) == 0.0
    _assert_within_bar(s, ref, "after execute", skip=("te1",))


def test_without_a_text_projection(tmp_path):
    reqs, hp_d, names, cache, stats, holdout, pipe, base, scorer = _fixture(tmp_path, proj=None)
    assert not hasattr(pipe.text_encoder_2, "text_projection")
    edit = reqs[:8]
    _apply(pipe, edit, hp_d, cache, stats)
    s = scorer.score()
    assert s.drift_pooled is None and "drift_pooled_max" not in s.summary()
    ref = _scores(_hf_read(_states(pipe), edit, names, holdout, None), _hf_read(base, edit, names, holdout, None), _vstars(cache, edit))
    _assert_within_bar(s, ref, "no projection")
    assert s.summary()["left_median_1"] < 1 and float(s.drift_max.max()) > 0


def test_refusals(tmp_path):
    reqs, hp_d, names, cache, stats, holdout, pipe, base, scorer = _fixture(tmp_path)
    edit = reqs[:8]
    hp = lambda **kw: EMCIDXLHyperParams(**dict(hp_d, **kw))
    params = _params(pipe)
    gauges = dict(cf.LAST_PATHS)
    half = syn.build_pipe("toy", DEV, sdxl=True, projection_dim=PROJ)
    half.text_encoder_2.half()
    with pytest.raises(cf.UnsupportedEncoder, match="fp32 in HBM"):
        emcid_amd.PairEditScorer(half, edit, hp(), DEV, holdout=holdout, cache_name=cache)
    with pytest.raises(cf.UnsupportedEncoder):          # layer modules the trie forward cannot find
        emcid_amd.PairEditScorer(pipe, edit, hp(layer_module_tmp="text_model.encoder.nolayers.{}"), DEV, holdout=holdout, cache_name=cache)
    only_first = str(tmp_path / "first") + "/"
    syn.write_vstar_cache(only_first, reqs, 32, seed=1, scale=0.5)
    with pytest.raises(FileNotFoundError, match="_2"):
        emcid_amd.PairEditScorer(pipe, edit, hp(), DEV, holdout=holdout, cache_name=only_first)
    # two tokenizers that disagree on a prompt's length: refused on the host
    short = syn.build_pipe("toy", DEV, sdxl=True, projection_dim=PROJ)
    short.tokenizer_2 = syn.build_tokenizer(model_max_length=5)
    with pytest.raises(ValueError, match="cannot be concatenated"):
        emcid_amd.PairEditScorer(short, edit, hp(), DEV, holdout=holdout, cache_name=cache)
    with pytest.raises(ValueError, match="SDXL"):
        emcid_amd.EditScorer(pipe, edit, EMCIDHyperParams(**{k: v for k, v in hp_d.items() if not k.endswith("_2")}), DEV,
                             holdout=holdout, cache_name=cache)
    assert dict(cf.LAST_PATHS) == gauges
    # a parameter other than the edited fc2 weights written in place: score() refuses on the host, whichever encoder it is
    with torch.no_grad():
        pipe.text_encoder_2.text_projection.weight.add_(0.0)          # (same values: only the version counter moved)
    with pytest.raises(ValueError, match="text encoder 2.*text_projection.weight"):
        scorer.score()
    fresh = emcid_amd.PairEditScorer(pipe, edit, hp(), DEV, holdout=holdout, cache_name=cache)
    gauges = dict(cf.LAST_PATHS)
    with torch.no_grad():
        fresh.encoders[0].graph.final_layer_norm.bias.add_(0.0)
    with pytest.raises(ValueError, match="text encoder 1.*final_layer_norm.bias"):
        fresh.score()
    assert dict(cf.LAST_PATHS) == gauges
    _assert_params(pipe, params)


def test_instruction_driver_with_holdout_prompts(tmp_path, capsys):
    """run_emcid.run on an sdxl-1.0 instruction with "holdout_prompts" prints the summary of a PairEditScorer built BEFORE the
    edit: the one a scorer used directly around the same call gives."""
    from emcid_amd import run_emcid
    reqs, hp_d, names, cache, stats = _setup_pair(tmp_path)
    holdout, edit = _holdout(reqs), reqs[:8]
    (tmp_path / "hp").mkdir()
    (tmp_path / "hp" / "toyxl.json").write_text(json.dumps(hp_d))
    ins = {"requests": edit, "hparams": "toyxl", "model_ckpt": "sdxl-1.0", "mom2_weight": 50, "mom2_weight_2": 80, "edit_weight": 0.5,
           "holdout_prompts": holdout}
    path = tmp_path / "ins.json"
    path.write_text(json.dumps(ins))
    twin = syn.build_pipe("toy", DEV, sdxl=True, projection_dim=PROJ)
    scorer = emcid_amd.PairEditScorer(twin, edit, EMCIDXLHyperParams(**hp_d), DEV, holdout=holdout, cache_name=cache)
    _apply(twin, edit, hp_d, cache, stats)
    want = scorer.score().summary()
    capsys.readouterr()
    pipe = syn.build_pipe("toy", DEV, sdxl=True, projection_dim=PROJ)
    run_emcid.run(str(path), DEV, pipe=pipe, hparams_dir=str(tmp_path / "hp"), cache_name=cache, stats_dir=stats[0], stats_dir_2=stats[1],
                  verbose=False)
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("edit score over")]
    assert len(line) == 1 and line[0].startswith(f"edit score over {len(holdout)} holdout prompts: ")
    got = json.loads(line[0].split(": ", 1)[1])
    assert set(got) == set(want) and "drift_pooled_max" in got
    for key in want:
        assert abs(got[key] - want[key]) <= BAR * abs(want[key]), (key, got[key], want[key])
    assert 0.0 < got["left_median_1"] < 1 and got["drift_max"] > 0

"""The host side of the SDXL pair's edit score (emcid_main.PairEditScorer / PairEditScore), no GPU: the two entry points in the
header, the library and the binding (their argument checks run on real buffers in tests/test_score_pair_kernel_gpu.py), a
PairEditScore built by hand, ``select_point`` on a list of them, and the refusals that need no device."""
import re
from pathlib import Path

import pytest
import torch

import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDXLHyperParams
from session_helpers import _hp

REPO = Path(__file__).resolve().parents[1]
NEW = {"emcid_score_chains_pair_f64": 15, "emcid_score_pooled_f32": 14}


def _xl(**kw):
    d = syn.sdxl_hparams_dict(layers=(1, 2, 3), layers_2=(3, 4, 5), mom2_update_weight=50, mom2_update_weight_2=80, mom2_n_samples=1000)
    d.update(kw)
    return EMCIDXLHyperParams(**d)


def _f64(x):
    return torch.tensor(x, dtype=torch.float64)


def _one(left, drift_max):
    left, drift_max = _f64(left), _f64(drift_max)
    z = torch.zeros_like(left)
    return em.EditScore([(f"c{i}", 0) for i in range(len(left))], left, z + 0.5, left * 2, z + 2, ["p"] * len(drift_max), drift_max,
                        drift_max / 2, drift_max / 3, torch.zeros_like(drift_max))


def _pair(left1, left2, drift_max, pooled=None):
    d = _f64(drift_max)
    return em.PairEditScore(_one(left1, [9.0] * len(d)), _one(left2, [7.0] * len(d)), ["p"] * len(d), d, d / 2, d / 3,
                            torch.zeros_like(d), None if pooled is None else _f64(pooled))


def test_symbols_are_declared_exported_and_bound():
    header = (REPO / "include" / "emcid_hip.h").read_text()
    lib = hip.load()
    for name, n_args in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in hip.EXPORTS
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert callable(hip.score_chains_pair) and callable(hip.score_pooled)
    # entry points were added, the ABI number stays
    assert int(re.search(r"#define\s+EMCID_ABI_VERSION\s+(\d+)", header).group(1)) == hip.ABI_VERSION == lib.emcid_abi_version() == 16


def test_names_are_exported():
    assert emcid_amd.PairEditScorer is em.PairEditScorer and emcid_amd.PairEditScore is em.PairEditScore


def test_a_pair_score_built_by_hand():
    s = _pair([0.2, 0.9, 0.4], [0.1, 0.3, 0.8], [0.5, 0.1, 0.3, 0.2], pooled=[0.01, 0.04, 0.02, 0.03])
    # the rows of TE1, then those of TE2; the sources say which encoder
    assert torch.equal(s.left, _f64([0.2, 0.9, 0.4, 0.1, 0.3, 0.8])) and torch.equal(s.cos, _f64([0.5] * 6))
    assert torch.equal(s.resid, s.left * 2) and torch.equal(s.resid0, _f64([2.0] * 6))
    assert s.sources == [("c0", 0, 1), ("c1", 0, 1), ("c2", 0, 1), ("c0", 0, 2), ("c1", 0, 2), ("c2", 0, 2)]
    assert torch.equal(s.te1.left, _f64([0.2, 0.9, 0.4])) and torch.equal(s.te2.left, _f64([0.1, 0.3, 0.8]))
    # EditScore.summary()'s keys on the pair-level fields (not on an encoder's own drift: 9 and 7 above), and three more
    assert s.summary() == pytest.approx({"left_median": 0.35, "left_max": 0.9, "drift_max": 0.5, "drift_median": 0.25,
                                         "left_median_1": 0.4, "left_median_2": 0.3, "drift_pooled_max": 0.04}, rel=1e-14)
    assert "left_median_2=0.3" in repr(s)
    no_pool = _pair([0.2], [0.4], [0.5])
    assert no_pool.drift_pooled is None and set(no_pool.summary()) == {"left_median", "left_max", "drift_max", "drift_median",
                                                                        "left_median_1", "left_median_2"}
    assert abs(no_pool.summary()["left_median"] - 0.3) < 1e-15


def test_select_point_on_pair_scores():
    """The smallest median ``left`` (over the rows of BOTH encoders) among the scores whose largest pair-level ``drift_max`` is
    within the budget, the first of equals; a NaN drift is within no budget."""
    scores = [_pair([0.1, 0.2], [0.1, 0.2], [0.9, 1.5]),          # best left, over the budget
              _pair([0.5, 0.6], [0.7, 0.7], [0.2, 0.59]),
              _pair([0.2, 0.3], [0.9, 0.9], [0.6, 0.1]),          # median of (0.2, 0.3, 0.9, 0.9) = 0.6: drift at the budget counts
              _pair([0.8, 0.9], [1.0, 1.0], [0.1, 0.1])]
    assert em.select_point(scores, 0.6) == 2
    assert em.select_point(scores, 0.59) == 1
    assert em.select_point(scores, 10.0) == 0
    assert em.select_point(scores, 0.05) is None
    assert em.select_point([_pair([0.5], [0.5], [float("nan")])], 1.0) is None
    assert em.select_point([_pair([0.5], [0.5], [0.3]), _pair([0.25], [0.75], [0.1])], 1.0) == 0
    # a list may mix the two kinds: only ``left`` and ``drift_max`` are read
    assert em.select_point([_one([0.7], [0.1]), _pair([0.5], [0.5], [0.3])], 1.0) == 1


def test_refusals_that_need_no_device(tmp_path):
    pair = syn.build_pipe("toy", "cpu", sdxl=True, projection_dim=24)
    one = syn.build_pipe("toy", "cpu")
    reqs = syn.make_requests(2, ragged=True)
    cache = str(tmp_path) + "/"
    before = dict(emcid_amd.LAST_PATHS)
    params = {(i, n): p.detach().clone() for i, te in enumerate((pair.text_encoder, pair.text_encoder_2)) for n, p in te.named_parameters()}
    with pytest.raises(TypeError, match="EMCIDXLHyperParams"):
        emcid_amd.PairEditScorer(pair, reqs, _hp(), holdout=["a dog"], cache_name=cache)
    with pytest.raises(ValueError, match="text_encoder_2"):
        emcid_amd.PairEditScorer(one, reqs, _xl(), holdout=["a dog"], cache_name=cache)
    with pytest.raises(ValueError, match="num_edit_tokens"):
        emcid_amd.PairEditScorer(pair, reqs, _xl(num_edit_tokens=2), holdout=["a dog"], cache_name=cache)
    with pytest.raises(ValueError, match="collective"):
        emcid_amd.PairEditScorer(pair, reqs, _xl(), holdout=["a dog"], cache_name=cache, shard=em.ConceptShard(0, 2))
    with pytest.raises(ValueError, match="holdout"):
        emcid_amd.PairEditScorer(pair, reqs, _xl(), holdout=[], cache_name=cache)
    with pytest.raises(ValueError, match="at least one request"):
        emcid_amd.PairEditScorer(pair, [], _xl(), holdout=["a dog"], cache_name=cache)
    with pytest.raises(ValueError, match="forward order"):
        emcid_amd.PairEditScorer(pair, reqs, _xl(layers_2=[5, 3]), holdout=["a dog"], cache_name=cache)
    with pytest.raises(cf.UnsupportedEncoder, match="fp32 in HBM"):              # CPU encoders: no prefix-trie forward
        emcid_amd.PairEditScorer(pair, reqs, _xl(), holdout=["a dog"], cache_name=cache)
    with pytest.raises(cf.UnsupportedEncoder, match="layer_module_tmp"):
        emcid_amd.PairEditScorer(pair, reqs, _xl(layer_module_tmp=None), holdout=["a dog"], cache_name=cache)
    # EditScorer goes on refusing the pair
    with pytest.raises(ValueError, match="SDXL"):
        emcid_amd.EditScorer(pair, reqs, _hp(), holdout=["a dog"])
    assert dict(emcid_amd.LAST_PATHS) == before
    for i, te in enumerate((pair.text_encoder, pair.text_encoder_2)):
        for n, p in te.named_parameters():
            assert torch.equal(p.detach(), params[(i, n)]), (i, n)

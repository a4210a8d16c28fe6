"""The edit_score module without a GPU: the moved names are the same objects under ``emcid_main`` in either import order, the
replay callback, the signature expression and the row-sums-to-``EditScore`` conversion are written once, and the shared
per-encoder host check and the two list validators refuse what the scorers and the sweeps refuse (tests/test_score*_cpu.py), in
each class's wording."""
import inspect
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import emcid_amd
from emcid_amd import clip_forward as cf, edit_score as sc, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDXLHyperParams
from session_helpers import LAYERS, _hp, pipe  # noqa: F401  (pipe: a module-scoped fixture)

REPO = Path(__file__).resolve().parents[1]
MOVED = ("_median", "EditScore", "score_row_sources", "SCORE_MAX_CHAIN", "holdout_tokens", "holdout_trie", "select_point",
         "EditScorer", "PairEditScore", "PairEditScorer")

_SAME = "; import emcid_amd.edit_score as s, emcid_amd.emcid_main as m; assert all(getattr(m, n) is getattr(s, n) for n in %r)" % (MOVED,)


@pytest.mark.parametrize("code", [
    "import emcid_amd.edit_score" + _SAME,
    "import emcid_amd.emcid_main as m; m.EditScorer" + _SAME,
    "import emcid_amd.edit_session, emcid_amd.edit_score" + _SAME,
    "import emcid_amd; emcid_amd.PairEditScorer; emcid_amd.select_point",
], ids=["edit_score first", "emcid_main first", "edit_session first", "the package"])
def test_either_import_order_works_in_a_fresh_interpreter(code):
    done = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=str(REPO)), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_moved_names_are_one_object_under_both_modules():
    for name in MOVED:
        assert getattr(em, name) is getattr(sc, name), name
        assert name not in vars(em), name                       # reached through the module's __getattr__, not defined there
    for name in ("EditScorer", "EditScore", "select_point", "PairEditScorer", "PairEditScore"):
        assert getattr(emcid_amd, name) is getattr(sc, name), name
    main = inspect.getsource(em)
    for name in MOVED:
        assert not re.search(rf"^(class|def) {name}\b|^{name} =", main, re.M), name
    assert len(re.findall(r"^def __getattr__\(", main, re.M)) == 1          # one mechanism for sessions and scores
    assert em.EditSession is emcid_amd.EditSession
    with pytest.raises(AttributeError):
        em.no_such_name


def test_the_replay_the_signature_and_the_conversion_are_written_once():
    src = inspect.getsource(sc)
    assert len(re.findall(r"def on_fc2\(", src)) == 1 and len(re.findall(r"hip\.gather_mean\(", src)) == 1
    assert len(re.findall(r"p\.data_ptr\(\), p\._version", src)) == 1 and len(re.findall(r"named_parameters\(\)", src)) == 1
    assert len(re.findall(r"resid02\.clamp\(", src)) == 1 and len(re.findall(r"return EditScore\(", src)) == 1      # _score_from_sums
    assert len(re.findall(r"changed since this", src)) == 1                                                       # check_frozen
    assert len(re.findall(r"\"score_replays\"\]\s*=", src)) == 1
    assert len(re.findall(r"hip\.score_chains\(", src)) == 1 and len(re.findall(r"hip\.score_rows\(", src)) == 2    # _half
    assert len(re.findall(r"did not take the prefix-trie forward", src)) == 1                                      # the plan test
    assert len(re.findall(r"a non-empty list of prompt strings\"", src)) == 1 and "prompt strings" not in inspect.getsource(em).split('"""')[-1]
    for cls in (sc.EditScorer, sc.PairEditScorer):
        assert "run_layers_from" not in inspect.getsource(cls).split('"""', 2)[2]         # the scorers own replays; they run none


def test_score_from_sums_is_the_definition_and_aliases_nothing():
    rows = torch.zeros(3, 8, dtype=torch.float64)
    #                moved2            resid2  resid02  dot
    rows[0, [0, 4, 5, 6]] = torch.tensor([4.0, 1.0, 9.0, 6.0], dtype=torch.float64)      # left 1/3, cos 6 / sqrt(36) = 1
    rows[1, [0, 4, 5, 6]] = torch.tensor([0.0, 4.0, 4.0, 0.0], dtype=torch.float64)      # nothing moved: left 1, cos 0
    rows[2, [0, 4, 5, 6]] = torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64)      # started on target: left 0, cos 0
    chains = torch.arange(8, dtype=torch.float64).view(2, 4)
    s = sc._score_from_sums([("a", 0), ("b", 0), ("c", 0)], ["p", "q"], rows, chains)
    assert torch.equal(s.left, torch.tensor([1.0 / 3.0, 1.0, 0.0], dtype=torch.float64))
    assert torch.equal(s.cos, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64))
    assert torch.equal(s.resid, torch.tensor([1.0, 2.0, 1.0], dtype=torch.float64))
    assert torch.equal(s.resid0, torch.tensor([3.0, 2.0, 0.0], dtype=torch.float64))
    assert [float(x[1]) for x in (s.drift_max, s.drift_mean, s.drift_eos, s.drift_argmax)] == [4.0, 5.0, 6.0, 7.0]
    assert s.sources == [("a", 0), ("b", 0), ("c", 0)] and s.holdout == ["p", "q"]
    rows.fill_(-1.0)
    chains.fill_(-1.0)
    assert float(s.left[0]) == 1.0 / 3.0 and float(s.drift_max[1]) == 4.0 and float(s.resid[0]) == 1.0


@pytest.mark.parametrize("bad", [None, [], "a dog", ["a dog", 3], [b"a dog"]])
def test_holdout_list_refuses_what_the_scorers_and_the_sweeps_refuse(bad):
    if bad == "a dog":          # (a string is a list of one-letter prompts, as before)
        assert sc._holdout_list(bad) == list("a dog")
        return
    with pytest.raises(ValueError) as err:
        sc._holdout_list(bad)
    assert str(err.value) == "holdout must be a non-empty list of prompt strings"
    with pytest.raises(ValueError) as err:
        sc._holdout_list(bad, "score= takes the holdout:")
    assert str(err.value) == "score= takes the holdout: a non-empty list of prompt strings"


def test_holdout_list_returns_a_list():
    assert sc._holdout_list(("a dog", "a cat")) == ["a dog", "a cat"] and sc._holdout_list(iter(["x"])) == ["x"]


@pytest.mark.parametrize("who", ["EditScorer", "PairEditScorer", "score="])
def test_one_rank_refuses_a_collective_shard(who):
    assert sc._one_rank(None, who) is None and sc._one_rank(em.ConceptShard(), who) is None
    with pytest.raises(ValueError) as err:
        sc._one_rank(em.ConceptShard(0, 2), who)
    assert str(err.value) == f"{who} runs on one rank: a collective ConceptShard is not supported"


def _xl(**kw):
    d = syn.sdxl_hparams_dict(layers=(1, 2, 3), layers_2=(3, 4, 5), mom2_update_weight=50, mom2_update_weight_2=80, mom2_n_samples=1000)
    d.update(kw)
    return EMCIDXLHyperParams(**d)


def test_check_encoder_refuses_a_cpu_encoder_in_each_class_wording(pipe):
    te, hp = pipe.text_encoder, _hp()
    with pytest.raises(cf.UnsupportedEncoder) as err:
        sc._check_encoder(te, list(LAYERS), hp, None, ["a dog"])
    assert str(err.value) == "the prefix-trie forward runs fp32 in HBM (got torch.float32 on cpu)"
    for which in (1, 2):
        with pytest.raises(cf.UnsupportedEncoder) as err:
            sc._check_encoder(te, list(LAYERS), hp, None, ["a dog"], which)
        assert str(err.value) == f"the prefix-trie forward runs fp32 in HBM (text encoder {which}: torch.float32 on cpu)"
    # ... and, before that, in the scorers' order: the weight names, the device, the holdout, layer_module_tmp
    xattn = _hp(rewrite_module_tmp="unet.down_blocks.{}.attn2.to_k")
    with pytest.raises(ValueError, match=r"^EditScorer scores edits of the text encoder's MLP projections; .* names no weight of "
                                         r"pipe\.text_encoder \(cross-attention edits are not supported\): "):
        sc._check_encoder(te, list(LAYERS), xattn, None, ["a dog"])
    with pytest.raises(ValueError, match=r"^'unet\.down_blocks.*' names no weight of text encoder 2: "):
        sc._check_encoder(te, list(LAYERS), xattn, None, ["a dog"], 2)
    with pytest.raises(ValueError) as err:
        sc._check_encoder(te, list(LAYERS), hp, "cuda:0", [])
    assert str(err.value) == "device 'cuda:0' but the text encoder's weights live on cpu"
    with pytest.raises(ValueError) as err:
        sc._check_encoder(te, list(LAYERS), hp, "cuda:0", [], 1)
    assert str(err.value) == "device 'cuda:0' but the weights of text encoder 1 live on cpu"
    with pytest.raises(ValueError, match="^holdout must be a non-empty list of prompt strings$"):
        sc._check_encoder(te, list(LAYERS), hp, "cpu", [])
    with pytest.raises(cf.UnsupportedEncoder, match="^hparams.layer_module_tmp is not set: no prefix-trie forward$"):
        sc._check_encoder(te, list(LAYERS), _hp(layer_module_tmp=None), None, ["a dog"], 1)


def test_the_scorers_raise_the_shared_check_for_a_cpu_encoder(pipe):
    with pytest.raises(cf.UnsupportedEncoder) as one:
        emcid_amd.EditScorer(pipe, syn.make_requests(2), _hp(), holdout=["a dog"])
    assert str(one.value) == "the prefix-trie forward runs fp32 in HBM (got torch.float32 on cpu)"
    with pytest.raises(cf.UnsupportedEncoder) as two:
        emcid_amd.PairEditScorer(syn.build_pipe("toy", "cpu", sdxl=True, projection_dim=24), syn.make_requests(2), _xl(), holdout=["a dog"])
    assert str(two.value) == "the prefix-trie forward runs fp32 in HBM (text encoder 1: torch.float32 on cpu)"


def test_check_frozen_raises_each_class_wording():
    enc = object.__new__(sc._EncoderReplay)
    enc.frozen = (("a.weight", 1, 2, 0), ("b.bias", 3, 4, 0))
    enc.signature = lambda: (("a.weight", 1, 2, 1), ("b.bias", 3, 4, 0))
    with pytest.raises(ValueError) as err:
        enc.check_frozen()
    assert str(err.value) == ("parameters other than the edited fc2 weights changed since this EditScorer was built (a.weight): its kept "
                              "states are no longer this encoder's; build a new EditScorer")
    with pytest.raises(ValueError) as err:
        enc.check_frozen(2)
    assert str(err.value) == ("parameters of text encoder 2 other than the edited fc2 weights changed since this PairEditScorer was built "
                              "(a.weight): its kept states are no longer this encoder's; build a new one")
    enc.signature = lambda: enc.frozen
    assert enc.check_frozen() is None and enc.check_frozen(1) is None

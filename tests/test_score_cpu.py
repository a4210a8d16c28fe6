"""The host side of edit scores (emcid_main.EditScorer / EditScore / select_point), no GPU: the selection rule, the summary, the
holdout trie's end nodes against a brute-force walk, the row order of ``sources``, the refusals that need no device, and the two
new entry points in the header, the library and the binding (their argument checks run on real buffers in
tests/test_score_kernel_gpu.py)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em, hip, synthetic as syn
from session_helpers import _hp, pipe  # noqa: F401  (pipe: a module-scoped fixture)

REPO = Path(__file__).resolve().parents[1]
NEW = ("emcid_score_rows_f32", "emcid_score_chains_f64")


def _score(left, drift_max):
    left, drift_max = torch.tensor(left, dtype=torch.float64), torch.tensor(drift_max, dtype=torch.float64)
    z = torch.zeros_like(left)
    return em.EditScore([("c", 0)] * len(left), left, z, z, z, ["p"] * len(drift_max), drift_max, drift_max / 2, drift_max / 3,
                        torch.zeros_like(drift_max))


def test_names_are_exported():
    assert emcid_amd.EditScorer is em.EditScorer and emcid_amd.EditScore is em.EditScore and emcid_amd.select_point is em.select_point
    assert "score_replays" in emcid_amd.LAST_PATHS


def test_select_point_takes_the_smallest_median_left_within_the_budget():
    scores = [_score([0.1, 0.2, 0.3], [0.9, 1.5]),        # best left, over the budget
              _score([0.5, 0.6, 0.7], [0.2, 0.59]),
              _score([0.4, 0.5, 0.9], [0.6, 0.1]),        # drift exactly at the budget counts
              _score([0.8, 0.9, 1.0], [0.1, 0.1])]
    assert em.select_point(scores, 0.6) == 2
    assert em.select_point(scores, 0.59) == 1
    assert em.select_point(scores, 10.0) == 0
    # the median decides, not the mean or the max: [0.0, 0.55, 0.56] (median 0.55) loses to [0.5, 0.5, 5.0] (median 0.5)
    assert em.select_point([_score([0.0, 0.55, 0.56], [0.1]), _score([0.5, 0.5, 5.0], [0.1])], 1.0) == 1


def test_select_point_ties_nothing_under_the_budget_and_an_empty_list():
    tie = [_score([0.5, 0.5], [0.3]), _score([0.5, 0.5], [0.1]), _score([0.7, 0.3], [0.2])]
    assert em.select_point(tie, 1.0) == 0                  # the first of equals
    assert em.select_point(tie[1:], 1.0) == 0
    assert em.select_point(tie, 0.05) is None
    assert em.select_point([], 1.0) is None
    assert em.select_point([_score([0.5], [float("nan")])], 1.0) is None      # a NaN drift is not within any budget


def test_summary():
    s = _score([0.2, 0.9, 0.4, 0.1, 0.3], [0.5, 0.1, 0.3])
    assert s.summary() == {"left_median": 0.3, "left_max": 0.9, "drift_max": 0.5, "drift_median": 0.3}
    assert "left_median=0.3" in repr(s)


def test_sources_row_order():
    reqs = syn.make_requests(3, ragged=True)
    assert em.score_row_sources(reqs, 1) == [("c0000", 0), ("c0001", 0), ("c0002", 0)]
    assert em.score_row_sources(reqs, 2) == [("c0000", 0), ("c0000", 1), ("c0001", 0), ("c0001", 1), ("c0002", 0), ("c0002", 1)]
    # the order of EditSession.rows(): request by request, its tokens in turn
    assert [(s, t) for s, t in em.score_row_sources(reqs, 2)] == [(r["source"], t) for r in reqs for t in range(2)]


def test_holdout_trie_end_nodes_against_a_brute_force_walk(pipe):
    reqs = syn.make_requests(12, ragged=True)
    prompts = [p.format(r["source"]) for r in reqs[8:] for p in r["prompts"]] + [c["caption"] for c in syn.make_captions(6)]
    prompts.append(prompts[0])                              # a repeated prompt ends where its twin ends
    trie, eos = em.holdout_trie(pipe.tokenizer, prompts, "cpu")
    enc = pipe.tokenizer(prompts, padding=True, truncation=True)
    ids, mask = np.asarray(enc["input_ids"]), np.asarray(enc["attention_mask"])
    assert np.array_equal(eos, mask.sum(1) - 1)
    end, anc, depth, token = trie.lookup_node.numpy(), trie.anc.numpy(), trie.depth.numpy(), trie.token.numpy()
    assert end.shape == (len(prompts),) and end[-1] == end[0]
    node_of = {}                                            # prefix -> node, filled by walking every prompt from its root
    for p, e in enumerate(end):
        n = int(eos[p]) + 1
        assert depth[e] == n - 1 and n <= anc.shape[1]
        chain = anc[e, :n]
        assert chain[-1] == e and np.array_equal(token[chain], ids[p, :n])          # the chain spells BOS ... EOS
        assert ids[p, n - 1] == pipe.tokenizer.eos_token_id
        for j, u in enumerate(chain):
            assert depth[u] == j and np.array_equal(anc[u, :j + 1], chain[:j + 1])
            assert node_of.setdefault(tuple(ids[p, :j + 1]), int(u)) == int(u)      # one node per distinct prefix
    assert len(set(node_of.values())) == len(node_of) == trie.n_nodes               # ... and one prefix per node: nothing else is in the trie


def test_holdout_must_be_prompt_strings(pipe):
    for bad in ([], [{"caption": "a dog"}], None):
        with pytest.raises(ValueError, match="holdout"):
            em.holdout_trie(pipe.tokenizer, bad or [], "cpu")


def test_refusals_that_need_no_device(pipe, tmp_path):
    reqs = syn.make_requests(2, ragged=True)
    before = dict(emcid_amd.LAST_PATHS)
    sd = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    with pytest.raises(cf.UnsupportedEncoder, match="fp32 in HBM"):              # a CPU encoder: no prefix-trie forward
        emcid_amd.EditScorer(pipe, reqs, _hp(), holdout=["a dog"], cache_name=str(tmp_path) + "/")
    with pytest.raises(ValueError, match="SDXL"):
        emcid_amd.EditScorer(syn.build_pipe("toy", "cpu", sdxl=True), reqs, _hp(), holdout=["a dog"])
    with pytest.raises(ValueError, match="cross-attention"):
        emcid_amd.EditScorer(pipe, reqs, _hp(rewrite_module_tmp="unet.down_blocks.{}.attn2.to_k"), holdout=["a dog"])
    with pytest.raises(ValueError, match="collective"):
        emcid_amd.EditScorer(pipe, reqs, _hp(), holdout=["a dog"], shard=em.ConceptShard(0, 2))
    with pytest.raises(ValueError, match="holdout"):
        emcid_amd.EditScorer(pipe, reqs, _hp(), holdout=[])
    assert dict(emcid_amd.LAST_PATHS) == before
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), sd[n]), n


def test_symbols_are_declared_exported_and_bound():
    header = (REPO / "include" / "emcid_hip.h").read_text()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert set(NEW) <= set(hip.EXPORTS)
    lib = hip.load()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name            # bound with a signature, not ctypes' default
    assert len(lib.emcid_score_rows_f32.argtypes) == 13 and len(lib.emcid_score_chains_f64.argtypes) == 9
    assert callable(hip.score_rows) and callable(hip.score_chains)
    # entry points were added, the ABI number stays
    assert int(re.search(r"#define\s+EMCID_ABI_VERSION\s+(\d+)", header).group(1)) == hip.ABI_VERSION == lib.emcid_abi_version() == 16


def test_a_holdout_chain_the_readout_or_the_position_table_cannot_take_is_refused_on_the_host(pipe):
    long_tok = syn.build_tokenizer(model_max_length=200)
    words = " ".join(["painting"] * 150)
    with pytest.raises(cf.UnsupportedEncoder, match="128"):
        em.holdout_tokens(long_tok, ["a dog", words])
    ids, eos = em.holdout_tokens(pipe.tokenizer, ["a dog", words], 77)           # (truncated to the tokenizer's 77: fine)
    assert int(eos.max()) + 1 <= 77
    with pytest.raises(ValueError, match="position embeddings"):
        em.holdout_tokens(pipe.tokenizer, ["a dog", words], 40)

"""The host side of the sweep over the SDXL pair of text encoders (emcid_main.sweep_emcid_sdxl_text_encoders), no GPU: the grid of
(mom2_weight, mom2_weight_2, edit_weight) triples and its factorisation into the two encoders' distinct points, the instruction
file's "sweep" list for sdxl-1.0, the new C-ABI symbol in the header, the library and the binding, and every host-side refusal of
its entry point (called the way tests/test_sweep_cpu.py calls the library: on host buffers, nothing can launch)."""
import copy
import json
import re
from pathlib import Path

import numpy as np
import pytest

import emcid_amd
from emcid_amd import edit_engine, emcid_main as em, hip, run_emcid, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDXLHyperParams

REPO = Path(__file__).resolve().parents[1]
NAME = "emcid_score_chains_pair_grid_f64"


def _xl(**kw):
    d = syn.sdxl_hparams_dict(layers=(1, 2, 3), layers_2=(3, 4, 5), mom2_update_weight=50, mom2_update_weight_2=80, mom2_n_samples=1000)
    d.update(kw)
    return EMCIDXLHyperParams(**d)


@pytest.mark.parametrize("grid", [[], [(4000, 4000, 1.0)], [(4000, 4000, 0.0)], [(4000, 4000, 1.5)], [(4000, 4000, -0.1)],
                                  [(0, 4000, 0.5)], [(4000, 0, 0.5)], [(-3, 4000, 0.5)], [(4000, -3, 0.5)],
                                  [(4000, 4000, 0.5), (float("nan"), 4000, 0.5)], [(4000, float("nan"), 0.5)],
                                  [(float("inf"), 4000, 0.5)], [(4000, float("inf"), 0.5)], [(4000, 4000, float("nan"))],
                                  [(4000, 0.5)], [(4000,)], [4000, 4000, 0.5], [(4000, 4000, 0.5, 1)],
                                  [(4000, 4000, 0.5), (4000, 0.5)], [("a", 4000, 0.5)]])
def test_bad_grids_raise_before_anything_runs(grid):
    """validate_grid's refusals per component, and an entry that is not a triple — a pair included: ValueError from the public
    entry point before the pipe is looked at (``pipe=None`` would be an AttributeError otherwise); hparams untouched."""
    hp = _xl()
    before = copy.deepcopy(hp.__dict__)
    with pytest.raises(ValueError):
        edit_engine.validate_pair_grid(grid)
    with pytest.raises(ValueError):
        em.sweep_emcid_sdxl_text_encoders(None, syn.make_requests(2), hp, grid)
    assert hp.__dict__ == before


def test_valid_grid_is_returned_as_float_triples_in_order():
    got = edit_engine.validate_pair_grid([(4000, 8000, 0.5), [1, 2, 0.25], (2.5, 3, 0.999)])
    assert got == [(4000.0, 8000.0, 0.5), (1.0, 2.0, 0.25), (2.5, 3.0, 0.999)]
    assert all(isinstance(x, float) for t in got for x in t)


def test_plan_order_of_first_appearance_and_repeated_triples():
    triples = [(2.0, 9.0, 0.5), (1.0, 9.0, 0.5), (2.0, 7.0, 0.5), (2.0, 9.0, 0.5), (1.0, 7.0, 0.5), (1.0, 9.0, 0.5)]
    pts1, pts2, combos = edit_engine.pair_grid_plan(triples)
    assert pts1 == [(2.0, 0.5), (1.0, 0.5)] and pts2 == [(9.0, 0.5), (7.0, 0.5)]
    assert combos == [(0, 0), (1, 0), (0, 1), (0, 0), (1, 1), (1, 0)]
    for (l1, l2, e), (i, j) in zip(triples, combos):
        assert pts1[i] == (l1, e) and pts2[j] == (l2, e)


def test_plan_of_a_4_by_4_cross_is_4_plus_4_points():
    lams1, lams2 = [500.0, 1000.0, 2000.0, 4000.0], [1000.0, 2000.0, 4000.0, 8000.0]
    triples = [(a, b, 0.5) for a in lams1 for b in lams2]
    pts1, pts2, combos = edit_engine.pair_grid_plan(triples)
    assert pts1 == [(a, 0.5) for a in lams1] and pts2 == [(b, 0.5) for b in lams2]
    assert len(combos) == 16 and combos == [(i, j) for i in range(4) for j in range(4)]


def test_plan_two_edit_weights_do_not_merge_points_that_share_a_lambda():
    """TE1's weights depend on (lam1, e), not on lam1 alone: the same lam at another edit_weight is another point, for both."""
    triples = [(1000.0, 2000.0, 0.5), (1000.0, 3000.0, 0.5), (1000.0, 2000.0, 0.25)]
    pts1, pts2, combos = edit_engine.pair_grid_plan(triples)
    assert pts1 == [(1000.0, 0.5), (1000.0, 0.25)]
    assert pts2 == [(2000.0, 0.5), (3000.0, 0.5), (2000.0, 0.25)]
    assert combos == [(0, 0), (0, 1), (1, 2)]
    # the grid of tests/test_sweep_pair_gpu.py: 3 + 3 points, 5 combos
    a, b, c, d, e, e2 = 50.0, 400.0, 80.0, 600.0, 0.5, 0.3
    pts1, pts2, combos = edit_engine.pair_grid_plan([(a, c, e), (a, d, e), (b, c, e), (b, d, e), (a, c, e2)])
    assert (len(pts1), len(pts2), combos) == (3, 3, [(0, 0), (0, 1), (1, 0), (1, 1), (2, 2)])


def test_instruction_file_takes_triples_for_sdxl_and_pairs_for_sd(tmp_path):
    (tmp_path / "hp").mkdir()
    (tmp_path / "hp" / "toyxl.json").write_text(json.dumps(syn.sdxl_hparams_dict(layers=(1, 2, 3), layers_2=(3, 4, 5), mom2_update_weight=50,
                                                                                 mom2_update_weight_2=80, mom2_n_samples=1000)))
    (tmp_path / "hp" / "toy.json").write_text(json.dumps(syn.sd_hparams_dict(layers=(1, 2), mom2_update_weight=50, edit_weight=0.6,
                                                                             mom2_n_samples=1000)))
    ins = {"requests": syn.make_requests(2), "hparams": "toyxl", "model_ckpt": "sdxl-1.0", "mom2_weight": 50, "mom2_weight_2": 80,
           "edit_weight": 0.5, "sweep": [[50, 80, 0.5], [50, 600, 0.5], [400, 80, 0.25]]}
    p = tmp_path / "ins.json"
    p.write_text(json.dumps(ins))
    got, hp, cache = run_emcid.load_instruction(p, tmp_path / "hp")
    assert got["sweep"] == [(50.0, 80.0, 0.5), (50.0, 600.0, 0.5), (400.0, 80.0, 0.25)]
    assert isinstance(hp, EMCIDXLHyperParams) and cache == "cache/toyxl/"
    for bad in ([[50, 0.5]], [[50, 80, 1.0]], [[50, 0, 0.5]], []):          # a pair; edit_weight = 1; mom2_weight_2 = 0; empty
        ins["sweep"] = bad
        p.write_text(json.dumps(ins))
        with pytest.raises(ValueError):
            run_emcid.load_instruction(p, tmp_path / "hp")
    ins.update(sweep=[[50, 80, 0.5]], hparams="toy", model_ckpt="sd-v1.4")          # triples are not for sd-v1.4
    p.write_text(json.dumps(ins))
    with pytest.raises(ValueError):
        run_emcid.load_instruction(p, tmp_path / "hp")


def test_names_are_exported():
    assert emcid_amd.sweep_emcid_sdxl_text_encoders is em.sweep_emcid_sdxl_text_encoders
    assert callable(edit_engine.SweepWalk) and callable(hip.score_chains_pair_grid)


def test_symbol_is_declared_exported_and_bound():
    header = (REPO / "include" / "emcid_hip.h").read_text()
    lib = hip.load()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header)
    assert NAME in hip.EXPORTS and len(getattr(lib, NAME).argtypes) == 19
    # an entry point was added, the ABI number stays
    assert int(re.search(r"#define\s+EMCID_ABI_VERSION\s+(\d+)", header).group(1)) == hip.ABI_VERSION == lib.emcid_abi_version() == 16


def test_entry_refuses_bad_arguments_without_a_device():
    """A null pointer, G_e, U_e, B or C < 1, a bank or ``out`` that is not 16-byte aligned: non-zero, "bad argument", before any
    launch (the buffers are the host's: a launch could not even read them)."""
    lib = hip.load()
    buf = np.zeros(64, dtype=np.float64)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    ints_buf = np.zeros(16, dtype=np.int64)
    ints = ints_buf.ctypes.data
    good = dict(node1=base, G1=1, U1=1, anc1=ints, ld1=1, depth1=ints, end1=ints, node2=base, G2=1, U2=1, anc2=ints, ld2=1, depth2=ints,
                end2=ints, B=1, combo=ints, C=1, out=base + 64)

    def call(**kw):
        a = dict(good, **kw)
        return lib.emcid_score_chains_pair_grid_f64(a["node1"], a["G1"], a["U1"], a["anc1"], a["ld1"], a["depth1"], a["end1"], a["node2"],
                                                    a["G2"], a["U2"], a["anc2"], a["ld2"], a["depth2"], a["end2"], a["B"], a["combo"],
                                                    a["C"], a["out"], None)

    for key in ("node1", "anc1", "depth1", "end1", "node2", "anc2", "depth2", "end2", "combo", "out"):
        assert call(**{key: None}) != 0 and b"bad argument" in lib.emcid_last_error(), key
    for key in ("G1", "U1", "G2", "U2", "B", "C", "ld1", "ld2"):
        for v in (0, -1):
            assert call(**{key: v}) != 0 and b"bad argument" in lib.emcid_last_error(), (key, v)
    for key in ("node1", "node2", "out"):
        assert call(**{key: good[key] + 8}) != 0 and b"bad argument" in lib.emcid_last_error(), key


def test_refusals_that_need_no_device(tmp_path):
    pair = syn.build_pipe("toy", "cpu", sdxl=True, projection_dim=24)
    one = syn.build_pipe("toy", "cpu")
    reqs = syn.make_requests(2, ragged=True)
    cache = str(tmp_path) + "/"
    grid = [(50, 80, 0.5)]
    before = dict(emcid_amd.LAST_PATHS)
    from session_helpers import _hp
    with pytest.raises(TypeError, match="EMCIDXLHyperParams"):
        em.sweep_emcid_sdxl_text_encoders(pair, reqs, _hp(), grid)
    with pytest.raises(ValueError, match="text_encoder_2"):
        em.sweep_emcid_sdxl_text_encoders(one, reqs, _xl(), grid)
    with pytest.raises(AssertionError, match="num_edit_tokens"):          # (_sdxl_plans' own refusal, reference :1246)
        em.sweep_emcid_sdxl_text_encoders(pair, reqs, _xl(num_edit_tokens=2), grid)
    with pytest.raises(ValueError, match="collective"):
        em.sweep_emcid_sdxl_text_encoders(pair, reqs, _xl(), grid, score=["a dog"], cache_name=cache, shard=em.ConceptShard(0, 2))
    with pytest.raises(ValueError, match="holdout"):
        em.sweep_emcid_sdxl_text_encoders(pair, reqs, _xl(), grid, score=[], cache_name=cache)
    with pytest.raises(ValueError, match="at least one request"):
        em.sweep_emcid_sdxl_text_encoders(pair, [], _xl(), grid, score=["a dog"], cache_name=cache)
    with pytest.raises(em.clip_forward.UnsupportedEncoder, match="fp32 in HBM"):          # CPU encoders: score= has no fallback
        em.sweep_emcid_sdxl_text_encoders(pair, reqs, _xl(), grid, score=["a dog"], cache_name=cache)
    with pytest.raises(ValueError, match="not on"):
        em.sweep_emcid_sdxl_text_encoders(pair, reqs, _xl(), grid, device="cuda:0")
    assert dict(emcid_amd.LAST_PATHS) == before

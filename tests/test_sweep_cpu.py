"""CPU tests of the (mom2_weight, edit_weight) sweep: grid validation, the scaling identity the sweep rests on (and that it is the
reference's scaling, through the oracle), the new C-ABI symbol, the instruction file's "sweep" list."""
import copy
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_golden, pipe_from_golden, write_cov_npz, write_vstars
from emcid_amd import edit_engine, emcid_main as em, hip, run_emcid, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from oracle import emcid_oracle as orc

REPO = Path(__file__).resolve().parents[1]


def _ab(lam, e):
    return 2.0 * lam * (1.0 - e), 2.0 * e


@pytest.mark.parametrize("grid", [[], [(4000, 1.0)], [(4000, 0.0)], [(4000, 1.5)], [(4000, -0.1)], [(0, 0.5)], [(-3, 0.5)],
                                  [(4000, 0.5), (float("nan"), 0.5)], [(float("inf"), 0.5)], [(4000,)], [4000, 0.5],
                                  [(4000, 0.5, 1)], [(4000, float("nan"))]])
def test_bad_grids_raise_before_anything_runs(grid):
    """Every bad grid is a ValueError from the public entry point, raised before the pipe is even looked at (``pipe=None`` would
    be an AttributeError otherwise), and the caller's hparams is untouched."""
    hp = EMCIDHyperParams(**syn.sd_hparams_dict(layers=(1, 2), mom2_update_weight=50, edit_weight=0.6, mom2_n_samples=1000))
    before = copy.deepcopy(hp.__dict__)
    with pytest.raises(ValueError):
        em.sweep_emcid_text_encoder(None, syn.make_requests(2), hp, grid)
    assert hp.__dict__ == before
    with pytest.raises(ValueError):
        edit_engine.validate_grid(grid)


def test_valid_grid_is_returned_as_float_pairs_in_order():
    assert edit_engine.validate_grid([(4000, 0.5), [1, 0.25], (2.5, 0.999)]) == [(4000.0, 0.5), (1.0, 0.25), (2.5, 0.999)]


def test_sweep_is_exported():
    import emcid_amd
    assert emcid_amd.sweep_emcid_text_encoder is em.sweep_emcid_text_encoder
    assert {"sweep_points", "sweep_cov_factorizations", "sweep_prefix_runs"} <= set(emcid_amd.LAST_PATHS)


def test_sweep_factor_key_has_neither_lam_nor_edit_weight():
    c = [torch.eye(4), torch.eye(4)]
    key = edit_engine.sweep_factor_cache_key(c)
    assert key == edit_engine.sweep_factor_cache_key(c) and key[0] == "sweep"
    assert key != edit_engine.factor_cache_key(c, 4000.0, 0.5)       # never collides with a single call's entry
    flat = repr(key)
    assert "4000" not in flat and "0.5" not in flat


def test_scaling_identity_fp64():
    """chol(a C) = sqrt(a) chol(C), and the dual (Woodbury) solve built from the RESCALED unit factor and the scalar b / a equals
    the direct solve of (a C + b K K^T) X = sqrt(b) K, to 1e-12 relative.  The pairs span the reference's range of
    mom2_update_weight (hparams files: 50 .. 8000) and edit_weight: there cond(A) <= (a + b |K|^2) / (a lambda_min(C)) stays below
    1e3 for this C (spectrum 1 .. 1e-2) and K (|K|^2 ~ 1e2), so np.linalg.solve itself, the yardstick, is good to eps * cond ~ 1e-13;
    a lam far below that range (0.25: cond 4e5) would measure the yardstick's own 4e-11, not the identity."""
    rng = np.random.default_rng(7)
    d, n = 64, 10
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    C = (q * np.logspace(0, -2, d)) @ q.T
    C = (C + C.T) / 2
    K = rng.standard_normal((d, n))
    L = np.linalg.cholesky(C)
    X = np.linalg.inv(L)
    for lam, e in [(4000.0, 0.5), (50.0, 0.6), (1000.0, 0.9), (8000.0, 0.05)]:
        a, b = _ab(lam, e)
        La = np.sqrt(a) * L                       # what the rescale kernel writes
        Xa = X / np.sqrt(a)
        ref_L = np.linalg.cholesky(a * C)
        assert np.abs(La - ref_L).max() <= 1e-12 * np.abs(ref_L).max()
        # the engine's chain on the rescaled factors: Kt = sqrt(b) K^T, Yt = Kt Xa^T, S = I + Yt Yt^T, adj^T = S^-1 Yt Xa
        Yt = (np.sqrt(b) * K.T) @ Xa.T
        S = np.eye(n) + Yt @ Yt.T
        adj = (np.linalg.solve(S, Yt) @ Xa).T
        want = np.linalg.solve(a * C + b * K @ K.T, np.sqrt(b) * K)
        assert np.abs(adj - want).max() <= 1e-12 * np.abs(want).max(), (lam, e)
        # and S is I + (b / a) Yc Yc^T with the pair-independent whitened keys Yc = K^T X^T
        Yc = K.T @ X.T
        assert np.abs(S - (np.eye(n) + (b / a) * Yc @ Yc.T)).max() <= 1e-12 * np.abs(S).max()


def test_oracle_agrees_with_the_a_b_formula(tmp_path):
    """a = 2 lam (1 - e), b = 2 e are the REFERENCE's scaling: the oracle's layer loop on the toy SD fixture, at two pairs, returns
    for its first edited layer the adj_k of (a C + b K K^T) adj_k = sqrt(b) K with the keys it traced.  Both pairs have (1 - e) a
    power of two, so the oracle's fp32 C (1 - e) / 0.5 is exact and the two sides differ by fp64 solve rounding only: eps 1.1e-16
    times the condition number of A (the fixture's statistics span three decades, lam C dominates: < 1e6) — bar 1e-8 of max|adj_k|."""
    z, meta = load_golden("toy_sd")
    cache = str(tmp_path / "cache") + "/"
    write_vstars(cache, meta["requests"], z["vstar"])
    for li, ln in enumerate(meta["layer_names"]):
        write_cov_npz(tmp_path / "stats", ln, z[f"cov/{li}"], meta["hparams"]["mom2_n_samples"])
    C = z["cov/0"].astype(np.float64)
    for lam, e in [(float(meta["lam"]), 0.5), (7.0, 0.75)]:
        pipe = syn.SyntheticPipe(text_encoder=pipe_from_golden(z, meta["kind"]), tokenizer=syn.build_tokenizer())
        trace = []
        orc.apply_emcid_to_text_encoder(pipe, meta["requests"], copy.deepcopy(meta["hparams"]), mom2_weight=lam, edit_weight=e,
                                        cache_name=cache, stats_dir=str(tmp_path / "stats"), trace=trace)
        K = trace[0]["K"].double().numpy().T                  # (d, N)
        a, b = _ab(lam, e)
        want = np.linalg.solve(a * C + b * K @ K.T, np.sqrt(b) * K)
        got = trace[0]["adj_k"].numpy()
        assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max(), (lam, e)


def test_library_and_header_declare_the_rescale_entry():
    header = (REPO / "include" / "emcid_hip.h").read_text()
    assert re.search(r"\bint\s+emcid_cov_factor_rescale_f64\s*\(", header)
    assert "emcid_cov_factor_rescale_f64" in hip.EXPORTS
    lib = hip.load()
    assert hasattr(lib, "emcid_cov_factor_rescale_f64")
    assert int(re.search(r"#define\s+EMCID_ABI_VERSION\s+(\d+)", header).group(1)) == hip.ABI_VERSION == lib.emcid_abi_version()
    assert hip.ABI_VERSION >= 15          # moved with the new entry (14 before it)


def test_rescale_entry_rejects_bad_arguments_without_gpu():
    lib = hip.load()
    buf = np.zeros(4, dtype=np.float64)
    ptr = buf.ctypes.data
    assert lib.emcid_cov_factor_rescale_f64(None, ptr, 32, 1, 128, 2.0, 1, None) != 0           # no source
    assert lib.emcid_cov_factor_rescale_f64(ptr, ptr, 32, 1, 128, 0.0, 1, None) != 0            # a = 0 has no factor
    assert lib.emcid_cov_factor_rescale_f64(ptr, ptr, 32, 1, 128, -1.0, 1, None) != 0
    assert lib.emcid_cov_factor_rescale_f64(ptr, ptr, 32, 0, 128, 2.0, 1, None) != 0
    if ptr % 16 == 0:
        assert lib.emcid_cov_factor_rescale_f64(ptr, ptr, 32, 1, 128, 2.0, 1, None) != 0        # workspace too small


def test_instruction_file_with_sweep_parses(tmp_path):
    hp_d = syn.sd_hparams_dict(layers=(1, 2), mom2_update_weight=50, edit_weight=0.6, mom2_n_samples=1000)
    (tmp_path / "hp").mkdir()
    (tmp_path / "hp" / "toy.json").write_text(json.dumps(hp_d))
    ins = {"requests": syn.make_requests(2), "hparams": "toy", "model_ckpt": "sd-v1.4", "mom2_weight": 50, "edit_weight": 0.6,
           "sweep": [[50, 0.6], [4000, 0.5], [100, 0.25]]}
    p = tmp_path / "ins.json"
    p.write_text(json.dumps(ins))
    got, hp, cache = run_emcid.load_instruction(p, tmp_path / "hp")
    assert got["sweep"] == [(50.0, 0.6), (4000.0, 0.5), (100.0, 0.25)]
    assert hp.mom2_update_weight == 50 and hp.edit_weight == 0.6 and cache == "cache/toy/"
    ins["sweep"] = [[50, 1.0]]
    p.write_text(json.dumps(ins))
    with pytest.raises(ValueError):
        run_emcid.load_instruction(p, tmp_path / "hp")
    ins.update(sweep=[[50, 0.5]], model_ckpt="sdxl-1.0")
    p.write_text(json.dumps(ins))
    with pytest.raises(ValueError):
        run_emcid.load_instruction(p, tmp_path / "hp")

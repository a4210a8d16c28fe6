"""GPU tests of sweep_emcid_text_encoder: every point of a (mom2_weight, edit_weight) grid against the oracle (toy fixture) and
against a standalone apply_emcid_to_text_encoder at that pair (real dimensions), the sharing counters, the weight restore, the
per-point LU fallback, the factor-rescale kernel on its own, and the collective code path.
Run on the MI355X box:  python -m pytest tests/test_sweep_gpu.py -m gpu -q"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from conftest import load_golden, pipe_from_golden, write_cov_npz, write_vstars
from emcid_amd import emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter
from oracle import emcid_oracle as orc

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _fresh_caches():
    em.clear_caches()
    yield
    em.clear_caches()


def _toy(tmp_path):
    z, meta = load_golden("toy_sd")
    cache = str(tmp_path / "cache") + "/"
    write_vstars(cache, meta["requests"], z["vstar"])
    for li, ln in enumerate(meta["layer_names"]):
        write_cov_npz(tmp_path / "stats", ln, z[f"cov/{li}"], meta["hparams"]["mom2_n_samples"])
    pipe = syn.SyntheticPipe(text_encoder=pipe_from_golden(z, meta["kind"]).to(DEV), tokenizer=syn.build_tokenizer())
    return z, meta, pipe, cache, str(tmp_path / "stats")


def _toy_grid(meta):
    return [(50.0, 0.6), (float(meta["lam"]), float(meta["ew"])), (4000.0, 0.3), (meta["hparams"]["mom2_update_weight"], 0.9)]


def _oracle_dw(z, meta, cache, stats, lam, e):
    cpu = syn.SyntheticPipe(text_encoder=pipe_from_golden(z, meta["kind"]), tokenizer=syn.build_tokenizer())
    w0 = {ln: orc.get_parameter(cpu.text_encoder, ln + ".weight").clone() for ln in meta["layer_names"]}
    orc.apply_emcid_to_text_encoder(cpu, meta["requests"], copy.deepcopy(meta["hparams"]), mom2_weight=lam, edit_weight=e,
                                    cache_name=cache, stats_dir=stats)
    return {ln: orc.get_parameter(cpu.text_encoder, ln + ".weight").double() - w0[ln].double() for ln in meta["layer_names"]}, w0


def _params(te):
    return {n: p.detach().clone() for n, p in te.named_parameters()}


def _assert_bit_equal(te, before):
    for n, p in te.named_parameters():
        assert torch.equal(p.detach(), before[n]), n


def test_toy_sweep_matches_oracle_at_every_point(tmp_path):
    """Toy fixture, 4 pairs (the hparams' own among them): each point against the oracle run at that pair, at the bar of the toy
    tests (err < 1e-4 and <= 1e-4 max|dW|); hparams untouched; the encoder bit-equal to its state before the sweep."""
    z, meta, pipe, cache, stats = _toy(tmp_path)
    hp = EMCIDHyperParams(**meta["hparams"])
    hp_before = copy.deepcopy(hp.__dict__)
    before = _params(pipe.text_encoder)
    grid = _toy_grid(meta)
    seen = []

    def visit(point, p):
        assert p is pipe
        seen.append(point)
        return {ln: get_parameter(p.text_encoder, ln + ".weight").detach().cpu().double() for ln in meta["layer_names"]}

    out = em.sweep_emcid_text_encoder(pipe, meta["requests"], hp, grid, DEV, visit=visit, cache_name=cache, stat_dir=stats)
    assert seen == [(float(a), float(b)) for a, b in grid] and len(out) == len(grid)
    assert hp.__dict__ == hp_before
    _assert_bit_equal(pipe.text_encoder, before)
    assert em.clip_forward.LAST_PATHS["sweep_points"] == len(grid) and em.clip_forward.LAST_PATHS["sweep_prefix_runs"] == 1
    for (lam, e), got in zip(grid, out):
        ref, w0 = _oracle_dw(z, meta, cache, stats, lam, e)
        for ln in meta["layer_names"]:
            err = ((got[ln] - w0[ln].double()) - ref[ln]).abs().max().item()
            print(f"toy sweep point ({lam}, {e}) {ln}: err {err:.3e} max|dW| {ref[ln].abs().max().item():.3e}")
            assert err < 1e-4 and err <= 1e-4 * ref[ln].abs().max().item(), (lam, e, ln, err)


def test_toy_sweep_default_result_is_the_edited_weights_on_the_host(tmp_path):
    z, meta, pipe, cache, stats = _toy(tmp_path)
    grid = _toy_grid(meta)[:2]
    out = em.sweep_emcid_text_encoder(pipe, meta["requests"], EMCIDHyperParams(**meta["hparams"]), grid, DEV, cache_name=cache,
                                      stat_dir=stats)
    single = syn.SyntheticPipe(text_encoder=pipe_from_golden(z, meta["kind"]).to(DEV), tokenizer=syn.build_tokenizer())
    em.apply_emcid_to_text_encoder(single, meta["requests"], EMCIDHyperParams(**meta["hparams"]), DEV, mom2_weight=grid[1][0],
                                   edit_weight=grid[1][1], cache_name=cache, stats_dir=stats, verbose=False)
    for ln in meta["layer_names"]:
        w = out[1][ln + ".weight"]
        assert w.device.type == "cpu" and w.dtype == torch.float32
        w0 = torch.from_numpy(z[f"w_orig/{meta['layer_names'].index(ln)}"]).double()
        dw = get_parameter(single.text_encoder, ln + ".weight").cpu().double() - w0
        assert ((w.double() - w0) - dw).abs().max().item() <= 1e-4 * dw.abs().max().item()


def _real_setup(tmp_path, n_req):
    reqs = syn.make_requests(n_req, names="syllable")
    hp_d = syn.sd_hparams_dict(prefix="text_model.")
    names = [hp_d["rewrite_module_tmp"].format(l) for l in hp_d["layers"]]
    cache = str(tmp_path / "cache") + "/"
    syn.write_vstar_cache(cache, reqs, 768, seed=1, scale=0.5)
    syn.write_stats_cache(tmp_path / "stats", names, 3072, hp_d["mom2_n_samples"], seed=2, t=6144)
    return reqs, hp_d, names, cache, str(tmp_path / "stats")


def _sweep_vs_standalone(tmp_path, n_req, grid):
    reqs, hp_d, names, cache, stats = _real_setup(tmp_path, n_req)
    pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)
    before = _params(pipe.text_encoder)
    orig = {ln: get_parameter(pipe.text_encoder, ln + ".weight").detach().cpu().double() for ln in names}
    paths0 = dict(em.clip_forward.LAST_PATHS)
    out = em.sweep_emcid_text_encoder(pipe, reqs, EMCIDHyperParams(**hp_d), grid, DEV, cache_name=cache, stat_dir=stats)
    counters = {k: v for k, v in em.clip_forward.LAST_PATHS.items() if k.startswith("sweep_")}
    moved = {k: em.clip_forward.LAST_PATHS.get(k, 0) - paths0.get(k, 0)
             for k in ("fused_edit_layers", "forward_trie", "forward_hf", "forward_hf_fallback", "lu_fallbacks")}
    # every point ran the hot path of a warm single call: the fused edit-layer call on the rescaled factors, on the trie forward
    assert moved == {"fused_edit_layers": len(grid) * len(names), "forward_trie": len(grid), "forward_hf": 0,
                     "forward_hf_fallback": 0, "lu_fallbacks": 0}, moved
    _assert_bit_equal(pipe.text_encoder, before)
    del pipe
    for (lam, e), got in zip(grid, out):
        fresh = syn.build_pipe("sd-v1.4", DEV, syllables=True)
        em.apply_emcid_to_text_encoder(fresh, reqs, EMCIDHyperParams(**hp_d), DEV, mom2_weight=lam, edit_weight=e,
                                       cache_name=cache, stats_dir=stats, verbose=False)
        for ln in names:
            w0 = orig[ln]
            dw = get_parameter(fresh.text_encoder, ln + ".weight").cpu().double() - w0
            err = ((got[ln + ".weight"].double() - w0) - dw).abs().max().item()
            print(f"N={n_req} point ({lam}, {e}) {ln}: |sweep - standalone| {err:.3e}, max|dW| {dw.abs().max().item():.3e}")
            assert err <= 1e-4 * dw.abs().max().item(), (lam, e, ln, err, dw.abs().max().item())
        del fresh
    return counters, len(names)


def test_real_dims_n100_sweep_matches_standalone_calls(tmp_path):
    """SD-v1.4 dimensions, 100 concepts, 4 pairs: each point within 1e-4 max|dW| (elementwise) of a standalone call on a fresh copy."""
    _sweep_vs_standalone(tmp_path, 100, [(4000.0, 0.5), (1000.0, 0.3), (8000.0, 0.7), (4000.0, 0.9)])


def test_real_dims_n1000_sweep_matches_standalone_calls_and_shares_the_work(tmp_path):
    """1 000 concepts, 3 pairs, same bar; one covariance factorization per edited layer, one prefix run, three points."""
    counters, n_layers = _sweep_vs_standalone(tmp_path, 1000, [(4000.0, 0.5), (2000.0, 0.4), (6000.0, 0.8)])
    assert counters == {"sweep_points": 3, "sweep_cov_factorizations": n_layers, "sweep_prefix_runs": 1}, counters


def test_weights_are_restored_when_visit_raises(tmp_path):
    z, meta, pipe, cache, stats = _toy(tmp_path)
    before = _params(pipe.text_encoder)
    calls = []

    def visit(point, p):
        calls.append(point)
        w = get_parameter(p.text_encoder, meta["layer_names"][0] + ".weight")
        assert not torch.equal(w.detach(), before[meta["layer_names"][0] + ".weight"])       # the edit IS in place here
        if len(calls) == 2:
            raise KeyError("stop at the second point")

    with pytest.raises(KeyError):
        em.sweep_emcid_text_encoder(pipe, meta["requests"], EMCIDHyperParams(**meta["hparams"]), _toy_grid(meta), DEV, visit=visit,
                                    cache_name=cache, stat_dir=stats)
    assert len(calls) == 2
    _assert_bit_equal(pipe.text_encoder, before)
    # and the same after a sweep that ran to its end on the dual solver (factors rescaled per point)
    em.clear_caches()
    os.environ["EMCID_SOLVER"] = "dual"
    try:
        out = em.sweep_emcid_text_encoder(pipe, meta["requests"], EMCIDHyperParams(**meta["hparams"]), _toy_grid(meta), DEV,
                                          cache_name=cache, stat_dir=stats)
    finally:
        del os.environ["EMCID_SOLVER"]
    _assert_bit_equal(pipe.text_encoder, before)
    assert em.clip_forward.LAST_PATHS["sweep_cov_factorizations"] == len(meta["layer_names"])
    for (lam, e), got in zip(_toy_grid(meta), out):      # the rescaled-factor path against the oracle, toy bar
        ref, w0 = _oracle_dw(z, meta, cache, stats, lam, e)
        for ln in meta["layer_names"]:
            err = ((got[ln + ".weight"].double() - w0[ln].double()) - ref[ln]).abs().max().item()
            assert err < 1e-4 and err <= 1e-4 * ref[ln].abs().max().item(), (lam, e, ln, err)


def test_a_non_spd_middle_point_takes_the_lu_rerun_alone(tmp_path, monkeypatch):
    """a C + b K K^T with the sweep's shared C is positive definite for every pair or for none, so ONE point can only be made
    non-SPD by handing its factorization other statistics: the middle point's first direct solve gets the indefinite matrix of
    test_apply_falls_back_to_pivoted_lu_* (nothing more is provoked than there: a reported pivot).  That point reruns on the
    pivoted LU — from the plan's own, sound statistics, so it still equals the oracle — lu_fallbacks rises by exactly one, and
    the point after it runs on the Cholesky path again and equals the oracle too."""
    from test_kernels_gpu import _indefinite_cov
    z, meta, pipe, cache, stats = _toy(tmp_path)
    n_layers = len(meta["layer_names"])
    grid = _toy_grid(meta)[:3]
    bad = _indefinite_cov(z["cov/0"].shape[0], seed=20).to(DEV)
    real, calls, lu_calls = hip.edit_layer, [], []

    def edit_layer(K, Zc, zs_t, Cov, *a, **k):
        calls.append(len(calls))
        return real(K, Zc, zs_t, bad if len(calls) - 1 == n_layers else Cov, *a, **k)

    real_lu = hip.edit_layer_lu

    def edit_layer_lu(*a, **k):
        lu_calls.append(em.clip_forward.LAST_PATHS["sweep_points"])
        return real_lu(*a, **k)

    monkeypatch.setattr(hip, "edit_layer", edit_layer)
    monkeypatch.setattr(hip, "edit_layer_lu", edit_layer_lu)
    before = _params(pipe.text_encoder)
    lu0 = em.clip_forward.LAST_PATHS.get("lu_fallbacks", 0)
    out = em.sweep_emcid_text_encoder(pipe, meta["requests"], EMCIDHyperParams(**meta["hparams"]), grid, DEV, cache_name=cache,
                                      stat_dir=stats)
    assert em.clip_forward.LAST_PATHS.get("lu_fallbacks", 0) == lu0 + 1
    assert lu_calls == [1] * n_layers                       # the LU ran for the middle point (one point done before it) only
    assert len(calls) == 3 * n_layers                       # the direct path: all of point 0, all of point 1 (failed), all of point 2
    _assert_bit_equal(pipe.text_encoder, before)
    for (lam, e), got in zip(grid, out):
        ref, w0 = _oracle_dw(z, meta, cache, stats, lam, e)
        for ln in meta["layer_names"]:
            err = ((got[ln + ".weight"].double() - w0[ln].double()) - ref[ln]).abs().max().item()
            assert err < 1e-4 and err <= 1e-4 * ref[ln].abs().max().item(), (lam, e, ln, err)


def test_a_reported_pivot_on_the_dual_form_reruns_that_point_alone(tmp_path, monkeypatch):
    """The same on the dual form (EMCID_SOLVER=dual), whose points run on the rescaled factors.  S = I + Yt Yt^T is positive definite
    whatever the factors hold, so the pivot is REPORTED for the middle point: the flag word of its rescaled workspace is set after
    the rescale.  That point is restored and rerun on the pivoted LU (lu_fallbacks + 1), the next point rescales into the same
    workspace again, runs on the Cholesky path and all three equal the oracle."""
    z, meta, pipe, cache, stats = _toy(tmp_path)
    n_layers = len(meta["layer_names"])
    grid = _toy_grid(meta)[:3]
    monkeypatch.setenv("EMCID_SOLVER", "dual")
    real, seen, lu_calls = hip.cov_factor_rescale, [], []

    def rescale(src, a, dst=None, **k):
        out = real(src, a, dst, **k)
        seen.append(out)
        if len(seen) == 2:
            out.info.fill_(3)
        return out

    real_lu = hip.edit_layer_lu

    def edit_layer_lu(*a, **k):
        lu_calls.append(em.clip_forward.LAST_PATHS["sweep_points"])
        return real_lu(*a, **k)

    monkeypatch.setattr(hip, "cov_factor_rescale", rescale)
    monkeypatch.setattr(hip, "edit_layer_lu", edit_layer_lu)
    before = _params(pipe.text_encoder)
    lu0 = em.clip_forward.LAST_PATHS.get("lu_fallbacks", 0)
    out = em.sweep_emcid_text_encoder(pipe, meta["requests"], EMCIDHyperParams(**meta["hparams"]), grid, DEV, cache_name=cache,
                                      stat_dir=stats)
    assert em.clip_forward.LAST_PATHS.get("lu_fallbacks", 0) == lu0 + 1
    assert lu_calls == [1] * n_layers and len(seen) == 3
    assert seen[1] is seen[2] and int(seen[2].info.item()) == 0          # the reused workspace, its flag word clean again
    assert em.clip_forward.LAST_PATHS["sweep_cov_factorizations"] == n_layers and em.clip_forward.LAST_PATHS["sweep_points"] == 3
    _assert_bit_equal(pipe.text_encoder, before)
    for (lam, e), got in zip(grid, out):
        ref, w0 = _oracle_dw(z, meta, cache, stats, lam, e)
        for ln in meta["layer_names"]:
            err = ((got[ln + ".weight"].double() - w0[ln].double()) - ref[ln]).abs().max().item()
            assert err < 1e-4 and err <= 1e-4 * ref[ln].abs().max().item(), (lam, e, ln, err)


def test_without_the_trie_forward_every_point_is_an_ordinary_call(tmp_path, monkeypatch):
    """edit_engine.FORWARD_MODE = "hf": no stored prefix state to replay.  The sweep says so (forward_hf_fallback rises), runs one
    ordinary call per point on the hooked forward, each equal to the oracle at the toy bar, and restores the weights bit for bit."""
    from emcid_amd import edit_engine
    z, meta, pipe, cache, stats = _toy(tmp_path)
    monkeypatch.setattr(edit_engine, "FORWARD_MODE", "hf")
    grid = _toy_grid(meta)[:3]
    before = _params(pipe.text_encoder)
    hp = EMCIDHyperParams(**meta["hparams"])
    hp_before = copy.deepcopy(hp.__dict__)
    p0 = dict(em.clip_forward.LAST_PATHS)
    out = em.sweep_emcid_text_encoder(pipe, meta["requests"], hp, grid, DEV, cache_name=cache, stat_dir=stats)
    lp = em.clip_forward.LAST_PATHS
    assert lp["forward_hf_fallback"] == p0["forward_hf_fallback"] + 1
    assert lp["forward_hf"] == p0["forward_hf"] + len(grid) and lp["forward_trie"] == p0["forward_trie"]
    assert hp.__dict__ == hp_before and len(out) == len(grid)
    _assert_bit_equal(pipe.text_encoder, before)
    for (lam, e), got in zip(grid, out):
        ref, w0 = _oracle_dw(z, meta, cache, stats, lam, e)
        for ln in meta["layer_names"]:
            err = ((got[ln + ".weight"].double() - w0[ln].double()) - ref[ln]).abs().max().item()
            assert err < 1e-4 and err <= 1e-4 * ref[ln].abs().max().item(), (lam, e, ln, err)


@pytest.mark.parametrize("d", [3072, 5120])
def test_factor_rescale_kernel_against_host_factorization(d):
    """emcid_cov_factor_rescale_f64 alone: chol(C) of a seeded C factored once on the GPU, rescaled by a in {0.5, 8000} into a second
    workspace (and in place), against torch.linalg.cholesky(a C) and its inverse in fp64 on the host: 1e-12 of the largest entry —
    two orders above the ~1e-14 of one fp64 multiply, because the inverse factor compounds it.  (C = G G^T / 2d + I, spectrum within
    [1, 4]: the two factorizations themselves then agree to a few eps.)"""
    g = torch.Generator(device=DEV).manual_seed(1234 + d)
    G = torch.randn(d, 2 * d, generator=g, device=DEV, dtype=torch.float32)
    C = (G @ G.t()) / (2 * d)
    C = ((C + C.t()) / 2 + torch.eye(d, device=DEV)).contiguous()
    del G
    unit = hip.factor_cov([C], 1.0, 0.5, None, inverse=True)
    assert int(unit.info.item()) == 0
    Lu, Xu = unit.L(0).clone(), unit.X(0).clone()
    C64 = C.double().cpu()
    tril = torch.ones(d, d, dtype=torch.bool).tril()
    scaled = None
    for a in (0.5, 8000.0):
        scaled = hip.cov_factor_rescale(unit, a, scaled, lam=a, edit_weight=0.5)
        assert scaled is not unit and scaled.have_inverse == {0} and scaled.lam == a
        torch.cuda.synchronize()
        assert torch.equal(unit.L(0), Lu) and torch.equal(unit.X(0), Xu)        # the source is left alone
        Ls, Xs = scaled.L(0)[:d, :d].cpu(), scaled.X(0)[:d, :d].cpu()
        # the kernel itself: one multiply per entry (by the rounded 1 / sqrt(a) for the inverses: two roundings, < 1e-15)
        wantL, wantX = Lu[:d, :d].cpu() * np.sqrt(a), Xu[:d, :d].cpu() / np.sqrt(a)
        assert (Ls - wantL)[tril].abs().max().item() <= 1e-15 * wantL.abs().max().item()
        assert (Xs - wantX)[tril].abs().max().item() <= 1e-15 * wantX.abs().max().item()
        inv_lo = 2 * unit.dp * unit.dp
        assert torch.allclose(scaled.buf[inv_lo:inv_lo + unit._inv], unit.buf[inv_lo:inv_lo + unit._inv] / np.sqrt(a), rtol=1e-15, atol=0)
        # against the host's factorization of a C
        Lref = torch.linalg.cholesky(a * C64)
        errL = (Ls - Lref)[tril].abs().max().item() / Lref.abs().max().item()
        Xref = torch.linalg.solve_triangular(Lref, torch.eye(d, dtype=torch.float64), upper=False)
        errX = (Xs - Xref)[tril].abs().max().item() / Xref.abs().max().item()
        print(f"rescale d={d} a={a}: L rel err {errL:.3e}, inverse factor rel err {errX:.3e}")
        assert errL <= 1e-12 and errX <= 1e-12, (d, a, errL, errX)
    # in place: the same numbers as into a second workspace
    twin = hip.cov_factor_rescale(unit, 1.0, None)
    again = hip.cov_factor_rescale(twin, 8000.0, twin)
    torch.cuda.synchronize()
    assert again is twin
    assert torch.equal(twin.L(0)[:d, :d].cpu()[tril], scaled.L(0)[:d, :d].cpu()[tril])
    assert torch.equal(twin.X(0)[:d, :d].cpu()[tril], scaled.X(0)[:d, :d].cpu()[tril])
    with pytest.raises(hip.EmcidHipError):
        hip.cov_factor_rescale(unit, 0.0)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _toy_dist_setup(tmp):
    reqs = syn.make_requests(9, ragged=True)
    hp_d = syn.sd_hparams_dict(layers=(1, 2, 3, 4), mom2_update_weight=50, edit_weight=0.6, mom2_n_samples=1000)
    names = [hp_d["rewrite_module_tmp"].format(l) for l in hp_d["layers"]]
    cache = tmp + "/cache/"
    if not os.path.exists(cache):
        syn.write_vstar_cache(cache, reqs, 32, seed=1, scale=0.5)
        syn.write_stats_cache(tmp + "/stats", names, 128, 1000, seed=2, t=512)
    return reqs, hp_d, names, cache


DIST_GRID = [(50.0, 0.6), (4000.0, 0.5), (200.0, 0.25)]


def _collective_worker(rank, world, port, tmp):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", EMCID_FORCE_COLLECTIVES="1",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        assert em._shard_from_env(None).collective
        reqs, hp_d, names, cache = _toy_dist_setup(tmp)
        pipe = syn.build_pipe("toy", "cuda:0")
        out = em.sweep_emcid_text_encoder(pipe, reqs, EMCIDHyperParams(**hp_d), DIST_GRID, "cuda:0", cache_name=cache,
                                          stat_dir=tmp + "/stats")
        np.savez(f"{tmp}/collective.npz", **{f"{i}/{n}": out[i][n + ".weight"].numpy() for i in range(len(out)) for n in names})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("solver", ["dual", "direct"])
def test_sweep_through_the_collective_code_path(tmp_path, solver, monkeypatch):
    """EMCID_FORCE_COLLECTIVES=1 in a one-rank RCCL group (K all-gather, column-sharded / row-sharded solve and their all-reduces
    per point) over the toy encoder, against the plain single-rank sweep at the bar of tests/test_dist_gpu.py's RCCL tests:
    1e-5 max|dW|."""
    tmp = str(tmp_path)
    reqs, hp_d, names, cache = _toy_dist_setup(tmp)
    monkeypatch.setenv("EMCID_SOLVER", solver)
    mp.spawn(_collective_worker, args=(1, _free_port(), tmp), nprocs=1, join=True)
    em.clear_caches()
    pipe = syn.build_pipe("toy", DEV)
    w0 = {n: get_parameter(pipe.text_encoder, n + ".weight").cpu().double() for n in names}
    out = em.sweep_emcid_text_encoder(pipe, reqs, EMCIDHyperParams(**hp_d), DIST_GRID, DEV, cache_name=cache, stat_dir=tmp + "/stats")
    got = np.load(f"{tmp}/collective.npz")
    for i in range(len(DIST_GRID)):
        for n in names:
            dw = (out[i][n + ".weight"].double() - w0[n]).numpy()
            err = np.abs((got[f"{i}/{n}"].astype(np.float64) - w0[n].numpy()) - dw).max()
            assert err <= 1e-5 * np.abs(dw).max(), (i, n, err)

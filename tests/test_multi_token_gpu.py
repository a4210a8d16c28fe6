"""num_edit_tokens = k > 1 on the library's own forward: the prefix trie with query-only leaves behind each prompt's EOS, the
(request, num) pseudo-segments of the key gather, and the concept-sharded solve over k x the request ranges.  Run on the MI355X
box:  python -m pytest tests/test_multi_token_gpu.py -m gpu -q"""
import datetime
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from conftest import load_golden, pipe_from_golden, write_cov_npz, write_vstars
from emcid_amd import clip_forward as cf, edit_engine as ee, emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter

DEV = "cuda:0"
RANK_TIMEOUT = 240          # seconds: every rank's process group (and so every collective) gives up after this


@pytest.fixture(autouse=True)
def _fresh_caches():
    em.clear_caches()
    yield
    em.clear_caches()


def _toy_fixture(tmp):
    """toy_multi_token (minted by the reference: k = 3, ragged prompt counts) with its (3, hidden) v* files and statistics."""
    z, meta = load_golden("toy_multi_token")
    cache = tmp + "/cache/"
    if not os.path.exists(cache):
        write_vstars(cache, meta["requests"], [z[f"vstar/{i}"] for i in range(len(meta["requests"]))])
        for li, ln in enumerate(meta["layer_names"]):
            write_cov_npz(tmp + "/stats", ln, z[f"cov/{li}"], meta["hparams"]["mom2_n_samples"])
    return z, meta, cache


def _dw_error(te, z, meta):
    worst = 0.0
    for li, ln in enumerate(meta["layer_names"]):
        dw_ref = z[f"w_final/{li}"].astype(np.float64) - z[f"w_orig/{li}"]
        dw = get_parameter(te, ln + ".weight").double().cpu().numpy() - z[f"w_orig/{li}"]
        worst = max(worst, np.abs(dw - dw_ref).max() / np.abs(dw_ref).max())
    return worst


def test_multi_token_edit_on_the_trie_matches_reference(tmp_path, monkeypatch):
    """The reference's own (3, hidden) v* files through execute_* and apply_* on the prefix-trie forward (no hooked HF forward):
    the factors and final weights of the REAL reference, on the staged path (cold call) and on the fused edit-layer call (warm)."""
    tmp = str(tmp_path)
    z, meta, cache = _toy_fixture(tmp)
    k, n = meta["k"], len(meta["requests"])
    te = pipe_from_golden(z, meta["kind"]).to(DEV)
    pipe = syn.SyntheticPipe(text_encoder=te, tokenizer=syn.build_tokenizer())
    hp = lambda: EMCIDHyperParams(**meta["hparams"])
    paths0 = dict(cf.LAST_PATHS)
    deltas = em.execute_emcid_text_encoder(pipe, meta["requests"], hp(), cache_name=cache, mom2_weight=meta["lam"],
                                           edit_weight=meta["ew"], verbose=False, stat_dir=tmp + "/stats")
    assert cf.LAST_PATHS["forward_trie"] > paths0["forward_trie"]
    assert cf.LAST_PATHS["forward_hf"] == paths0["forward_hf"] and cf.LAST_PATHS["forward_hf_fallback"] == paths0["forward_hf_fallback"]
    for li, ln in enumerate(meta["layer_names"]):
        adj_k, resid = deltas[ln + ".weight"]
        ref_a, ref_r = z[f"adj_k/{li}"], z[f"resid/{li}"]
        assert adj_k.shape == ref_a.shape == (ref_a.shape[0], n * k) and resid.shape == ref_r.shape
        np.testing.assert_allclose(adj_k.numpy(), ref_a, rtol=0, atol=2e-4 * np.abs(ref_a).max())
        np.testing.assert_allclose(resid.numpy(), ref_r, rtol=0, atol=2e-5 * np.abs(ref_r).max())
    w0 = {ln: get_parameter(te, ln + ".weight").detach().clone() for ln in meta["layer_names"]}
    fused0 = cf.LAST_PATHS.get("fused_edit_layers", 0)
    for call, solver in enumerate(("auto", "dual", "dual")):
        # the default solver of this size (direct), then the dual one cold and warm: the warm call finds the factors in HBM and
        # takes the fused edit-layer call (keys, Zc, solve, fc2 in one C call per layer)
        if solver == "auto":
            monkeypatch.delenv("EMCID_SOLVER", raising=False)
        else:
            monkeypatch.setenv("EMCID_SOLVER", solver)
        with torch.no_grad():
            for ln, w in w0.items():
                get_parameter(te, ln + ".weight").copy_(w)
        em.apply_emcid_to_text_encoder(pipe, meta["requests"], hp(), DEV, mom2_weight=meta["lam"], edit_weight=meta["ew"],
                                       cache_name=cache, stats_dir=tmp + "/stats", verbose=False)
        assert _dw_error(te, z, meta) <= 1e-4, call
    assert cf.LAST_PATHS.get("fused_edit_layers", 0) > fused0
    assert cf.LAST_PATHS["forward_hf"] == paths0["forward_hf"] and cf.LAST_PATHS["forward_hf_fallback"] == paths0["forward_hf_fallback"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _too_long(meta):
    """The fixture's requests with one prompt of the LAST request (rank 1's share at 2 ranks) padded beyond the position table:
    longest (77 after truncation) + k - 2 > 77."""
    reqs = [dict(r) for r in meta["requests"]]
    reqs[-1]["prompts"] = list(reqs[-1]["prompts"]) + ["painting by {}" + " artwork" * 90]
    return reqs


def _dist_worker(rank, world, port, tmp, force):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      EMCID_FORCE_COLLECTIVES="1" if force else "0")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=RANK_TIMEOUT))
    try:
        z, meta, cache = _toy_fixture(tmp)
        te = pipe_from_golden(z, meta["kind"]).to(DEV)
        pipe = syn.SyntheticPipe(text_encoder=te, tokenizer=syn.build_tokenizer())
        hp = lambda: EMCIDHyperParams(**meta["hparams"])
        try:
            em.apply_emcid_to_text_encoder(pipe, _too_long(meta), hp(), DEV, mom2_weight=meta["lam"], edit_weight=meta["ew"],
                                           cache_name=cache, stats_dir=tmp + "/stats", verbose=False)
            too_long = "no error"
        except ValueError as e:
            too_long = "ValueError" if "max_position_embeddings" in str(e) else f"other ValueError: {e}"
        w_untouched = all(torch.equal(get_parameter(te, ln + ".weight").cpu(), torch.from_numpy(z[f"w_orig/{li}"]))
                          for li, ln in enumerate(meta["layer_names"]))
        paths0 = dict(cf.LAST_PATHS)
        em.apply_emcid_to_text_encoder(pipe, meta["requests"], hp(), DEV, mom2_weight=meta["lam"], edit_weight=meta["ew"],
                                       cache_name=cache, stats_dir=tmp + "/stats", verbose=False)
        np.savez(f"{tmp}/rank{rank}_w{world}.npz", err=_dw_error(te, z, meta), too_long=too_long, untouched=w_untouched,
                 trie=cf.LAST_PATHS["forward_trie"] - paths0["forward_trie"], hf=cf.LAST_PATHS["forward_hf"] - paths0["forward_hf"],
                 **{ln: get_parameter(te, ln + ".weight").cpu().numpy() for ln in meta["layer_names"]})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 1])
def test_multi_token_edit_sharded_matches_reference(tmp_path, world):
    """The same fixture concept-sharded: 2 ranks sharing the GPU over gloo (4 requests: 2 | 2 requests, 6 | 6 concept rows), and
    world 1 through the collective code path (EMCID_FORCE_COLLECTIVES=1).  Every rank ends with the reference's final weights;
    a request set padded beyond the position table fails with ValueError on EVERY rank (one rank's prompts are short), and none
    hangs (every rank's process group times out)."""
    tmp = str(tmp_path)
    _toy_fixture(tmp)
    mp.spawn(_dist_worker, args=(world, _free_port(), tmp, world == 1), nprocs=world, join=True)
    outs = [np.load(f"{tmp}/rank{r}_w{world}.npz") for r in range(world)]
    for o in outs:
        assert str(o["too_long"]) == "ValueError" and bool(o["untouched"])
        assert float(o["err"]) <= 1e-4
        assert int(o["trie"]) == 1 and int(o["hf"]) == 0
    if world == 2:
        for ln in load_golden("toy_multi_token")[1]["layer_names"]:
            assert np.array_equal(outs[0][ln], outs[1][ln])


def _real_dims(tmp, k, n_req=200, long_prompts=False):
    reqs = syn.make_requests(n_req, names="syllable")
    if long_prompts:     # chains over 16 nodes: the general tree-attention kernel, outside the native runner
        reqs = [dict(r, prompts=["a quiet river scene at dusk painted by {}", "study of light by {}", "by {}"]) for r in reqs]
    hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
    layers = (7, 8, 9, 10)
    hp_d = dict(syn.sd_hparams_dict(layers=layers, mom2_update_weight=60, mom2_n_samples=100), num_edit_tokens=k,
                use_new_compute_z=True)
    names = [hp_d["rewrite_module_tmp"].format(l) for l in layers]
    cache = tmp + f"/cache{k}/"
    rng = np.random.default_rng(k)
    for r in reqs:
        p = syn.vstar_cache_path(cache, r)
        p.parent.mkdir(parents=True, exist_ok=True)
        np.savez(p, v_star=(0.5 * rng.standard_normal((k, hidden))).astype(np.float32))
    if not os.path.exists(tmp + "/stats"):
        syn.write_stats_cache(tmp + "/stats", names, inter, 100, seed=2, t=2 * inter)
    return reqs, hp_d, names, cache


def _traced_edit(pipe, reqs, hp, cache, tmp):
    plan = em.prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, reqs, hp, hp.layers, hp.mom2_update_weight,
                                        tmp + "/stats", cache, verbose=False)
    edits = ee.run_encoder_edit(plan, trace=True, restore=True)
    ee.check_info(plan)
    return plan, [(e.dW.double().cpu(), e.K.cpu(), e.Zc.cpu()) for e in edits]


@pytest.mark.parametrize("k,long_prompts", [(2, False), (3, False), (3, True), (6, False)])
def test_real_dims_trie_equals_hooked_forward(tmp_path, monkeypatch, k, long_prompts):
    """SD-v1.4-sized encoder, 200 artist-shaped requests x 3 prompts: per edited layer the trie forward's K / Zc rows and dW against
    the hooked HF forward (forward_mode "hf") on the same plan inputs."""
    tmp = str(tmp_path)
    reqs, hp_d, names, cache = _real_dims(tmp, k, long_prompts=long_prompts)
    pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)
    hp = EMCIDHyperParams(**hp_d)
    plan, trie = _traced_edit(pipe, reqs, hp, cache, tmp)
    assert plan.graph is not None and plan.n_total == len(reqs) * k
    if long_prompts:
        assert plan.trie.anc.shape[1] > 16 and cf.native_of(plan.graph, plan.trie, 0, 1) is None
    else:
        assert cf.native_of(plan.graph, plan.trie, 0, 1) is not None
    monkeypatch.setattr(ee, "FORWARD_MODE", "hf")
    em.clear_caches()
    plan_hf, hooked = _traced_edit(pipe, reqs, hp, cache, tmp)
    assert plan_hf.graph is None
    for (dw, K, Zc), (dw_h, K_h, Zc_h) in zip(trie, hooked):
        assert K.shape == K_h.shape == (len(reqs) * k, K.shape[1])
        # (fp32 rounding of two different forwards through up to 11 layers, split-fp16 projections on the trie)
        assert (K - K_h).abs().max().item() <= 1e-4 * K_h.abs().max().item()
        assert (Zc - Zc_h).abs().max().item() <= 1e-4 * Zc_h.abs().max().item()
        # k = 6: four of every request's six rows are padding positions behind one EOS, nearly collinear keys — the N k = 1 200
        # row system amplifies the forwards' fp32 differences to 1.02e-4 of max |dW| (measured on the MI355X); k <= 3: the 1e-4 bar
        assert (dw - dw_h).abs().max().item() <= (1e-4 if k <= 3 else 2e-4) * dw_h.abs().max().item()


def test_real_dims_multi_token_matches_oracle(tmp_path):
    """k = 3 at N = 40 on the SD-v1.4-sized encoder: the product's edited weights elementwise against the oracle's (the reference's
    algorithm in fp32 / fp64 on the CPU)."""
    from oracle import emcid_oracle as orc
    tmp = str(tmp_path)
    reqs, hp_d, names, cache = _real_dims(tmp, 3, n_req=40)
    cpu = syn.build_pipe("sd-v1.4", "cpu", syllables=True)
    w0 = {n: orc.get_parameter(cpu.text_encoder, n + ".weight").clone().double() for n in names}
    orc.apply_emcid_to_text_encoder(cpu, reqs, dict(hp_d), cache_name=cache, stats_dir=tmp + "/stats")
    gpu = syn.build_pipe("sd-v1.4", DEV, syllables=True)
    em.apply_emcid_to_text_encoder(gpu, reqs, EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=tmp + "/stats",
                                   verbose=False)
    for n in names:
        ref = orc.get_parameter(cpu.text_encoder, n + ".weight").double() - w0[n]
        got = get_parameter(gpu.text_encoder, n + ".weight").cpu().double() - w0[n]
        assert (got - ref).abs().max().item() <= 1e-4 * ref.abs().max().item(), n


def _dense_reference(q, k, v, ids_len, lk, eos, rows_of, H, scale):
    """fp64 dense masked attention of every prompt padded behind its EOS (causal mask AND key <= EOS, as HF's CLIP with its
    attention mask): the output at each of the prompt's lookup positions."""
    out = {}
    for i in range(len(eos)):
        S = int(lk[i].max()) + 1
        node = rows_of(i, S)                                    # node of every position 0 .. S-1 of prompt i
        Q, K, V = (t[node].double().view(S, H, -1).transpose(0, 1) for t in (q, k, v))
        s = Q @ K.transpose(1, 2) * scale
        keep = (torch.arange(S)[None, :] <= torch.arange(S)[:, None]) & (torch.arange(S)[None, :] <= int(eos[i]))
        s = s.masked_fill(~keep.to(s.device), float("-inf"))
        o = (torch.softmax(s, -1) @ V).transpose(0, 1).reshape(S, -1)
        for j in range(lk.shape[1]):
            out[(i, j)] = o[int(lk[i, j])]
    return out


@pytest.mark.parametrize("S,k", [(7, 3), (15, 2), (14, 6), (40, 4)])
def test_tree_attention_with_leaves_equals_dense_masked(S, k):
    """Tree attention on a trie with query-only leaves, in every form the dispatch picks (chains <= 8 and <= 16: the short-chain
    kernel, fp32 and split-fp16 output; longer: the general kernel) against fp64 dense masked attention of the padded prompts."""
    rng = np.random.default_rng(S * 10 + k)
    B, H, D = 24, 12, 64
    ids = rng.integers(0, 5, size=(B, S)).astype(np.int64)
    ids[:, 0] = 7
    eos = rng.integers(max(1, S - 4), S, size=B).astype(np.int64)
    last = np.array([rng.integers(0, e) for e in eos], dtype=np.int64)
    from emcid_amd.compute_z import multi_token_lookup
    lk = multi_token_lookup(last, eos, k)
    trie = cf.build_trie(ids, lk, DEV, eos=eos, pad_token=9)
    U = trie.token.numel()
    g = torch.Generator().manual_seed(S + k)
    q, kk, v = (torch.randn(U, H * D, generator=g).to(DEV) for _ in range(3))
    ln = trie.lookup_node.view(B, k).cpu()
    anc = trie.anc.cpu()

    def rows_of(i, n):       # chain node at positions <= EOS, the leaf at EOS + j (only the lookups are compared)
        node = [int(anc[int(ln[i, 1]), p]) for p in range(int(eos[i]) + 1)]
        leaf = {int(lk[i, j]): int(ln[i, j]) for j in range(k)}
        return torch.tensor([node[p] if p <= eos[i] else leaf.get(p, node[-1]) for p in range(n)])

    ref = _dense_reference(q.cpu(), kk.cpu(), v.cpu(), S, lk, eos, rows_of, H, D ** -0.5)
    rows = trie.query_rows
    forms = {"f32": hip.tree_attention(q[rows.long()], kk, v, trie.anc, trie.depth, H, None, rows)}
    if hip.tree_attention_sp_supported(trie.anc, H, D):
        forms["sp16"] = hip.tree_attention_sp(q[rows.long()], kk, v, trie.anc, trie.depth, H, None, rows).float()
        assert trie.anc.shape[1] <= 16
    else:
        assert trie.anc.shape[1] > 16
    for name, out in forms.items():
        out = out.cpu().double()
        tol = 1e-5 if name == "f32" else 1e-4
        liq = trie.lookup_in_query.view(B, k).cpu()
        for (i, j), want in ref.items():
            got = out[int(liq[i, j])]
            assert (got - want).abs().max().item() <= tol * max(1.0, want.abs().max().item()), (name, i, j)

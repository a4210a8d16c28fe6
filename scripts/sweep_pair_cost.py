"""What a scored sweep over the SDXL pair costs (emcid_main.sweep_emcid_sdxl_text_encoders), by the method of scripts/score_pair_cost.py
and scripts/sweep_vs_calls.py: the synthetic pair at SDXL's dimensions (TE1 768 / 12 layers edited at 8-10, TE2 1280 / 32 layers
edited at 26-30, text projection 1280 -> 1280), 3 prompts per concept, 100 caption prompts held out; N = 100 and N = 1 000 requests;
crosses of 2 x 2 and 4 x 4 (mom2_weight, mom2_weight_2) at one edit_weight.  Arms, alternated after one warm-up of each, REPS
repetitions, device-synchronised wall ms PER TRIPLE, median [min, max]; every repetition of either arm starts from empty factor caches:
    A   the factorised ``score=`` sweep: one call
    B   what existed before it: a PairEditScorer built once, then per triple apply_emcid_to_sdxl_text_encoders + scorer.score() +
        restore of both encoders' edited weights
Recorded as well: arm A's encoder-point counts (LAST_PATHS) and, by device events, ``hip.score_chains_pair_grid`` alone at C = 4 and
C = 16 on banks of the last case's shape.
    timeout -k 10 900 python scripts/sweep_pair_cost.py        [OUT=dir, default profiles/] -> OUT/sweep_pair.json"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import torch
from emcid_amd import clip_forward as cf, edit_engine as ee, emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDXLHyperParams
from emcid_amd.nethook import get_parameter

DEV, REPS, PROJ, M, E = "cuda:0", 5, 1280, 100, 0.5
LAMS1, LAMS2 = [1000.0, 2000.0, 4000.0, 8000.0], [2500.0, 5000.0, 10000.0, 20000.0]
hp_d = syn.sdxl_hparams_dict()
(h1, i1), (h2, i2) = syn.ENCODER_DIMS["sdxl-te1"][:2], syn.ENCODER_DIMS["sdxl-te2"][:2]
n1 = [hp_d["rewrite_module_tmp"].format(l) for l in hp_d["layers"]]
n2 = [hp_d["rewrite_module_tmp"].format(l) for l in hp_d["layers_2"]]
tmp = tempfile.mkdtemp()
s1, s2 = tmp + "/s1", tmp + "/s2"
syn.write_stats_cache(s1, n1, i1, hp_d["mom2_n_samples"], seed=2, t=2 * i1)
syn.write_stats_cache(s2, n2, i2, hp_d["mom2_n_samples"], seed=7, t=2 * i2)
holdout = [c["caption"] for c in syn.make_captions(M, seed=11)]
pipe = syn.build_pipe("sdxl", DEV, sdxl=True, syllables=True, projection_dim=PROJ)
hp = lambda: EMCIDXLHyperParams(**hp_d)
w0 = [{n: get_parameter(te, n + ".weight").detach().clone() for n in ns}
      for te, ns in ((pipe.text_encoder, n1), (pipe.text_encoder_2, n2))]


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


def restore():
    with torch.no_grad():
        for te, ws in zip((pipe.text_encoder, pipe.text_encoder_2), w0):
            for n, w in ws.items():
                get_parameter(te, n + ".weight").copy_(w)


def measure(n_concepts, k):
    reqs = syn.make_requests(n_concepts, names="syllable", name_seed=3)
    cache = f"{tmp}/cache{n_concepts}/"
    if not os.path.exists(cache):
        syn.write_vstar_cache(cache, reqs, h1, seed=1, scale=0.5)
        syn.write_vstar_cache(cache, reqs, h2, seed=5, scale=0.5, suffix="_2")
    grid = [(a, b, E) for a in LAMS1[:k] for b in LAMS2[:k]]
    kw = dict(cache_name=cache, stat_dir=s1, stat_dir_2=s2, verbose=False)
    last = {}

    def arm_a():
        ee.clear_engine_caches()
        torch.cuda.synchronize()
        t = time.perf_counter()
        last["a"] = em.sweep_emcid_sdxl_text_encoders(pipe, reqs, hp(), grid, DEV, score=holdout, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def arm_b():
        ee.clear_engine_caches()
        torch.cuda.synchronize()
        t = time.perf_counter()
        scorer = em.PairEditScorer(pipe, reqs, hp(), DEV, holdout=holdout, cache_name=cache)
        scores = []
        for l1, l2, e in grid:
            em.apply_emcid_to_sdxl_text_encoders(pipe, reqs, hp(), DEV, mom2_weight=l1, mom2_weight_2=l2, edit_weight=e, **kw)
            scores.append(scorer.score())
            restore()
        torch.cuda.synchronize()
        last["b"] = scores
        return (time.perf_counter() - t) * 1e3

    arm_a(), arm_b()                                           # warm-up of both (kernels loaded, graphs captured, files cached)
    ms = {"a": [], "b": []}
    for i in range(REPS):
        for arm in (("a", "b") if i % 2 == 0 else ("b", "a")):
            ms[arm].append((arm_a if arm == "a" else arm_b)() / len(grid))
        if i == 0:
            counters = {key: cf.LAST_PATHS[key] for key in ("sweep_pair_points_1", "sweep_pair_points_2", "sweep_pair_combos", "sweep_points",
                                                            "sweep_cov_factorizations", "sweep_prefix_runs")}
    # the two arms read the same edits: the largest distance of their summaries
    agree = max(abs(x - y) / max(abs(y), 1e-300) for sa, sb in zip(last["a"], last["b"])
                for x, y in zip(sa.summary().values(), sb.summary().values()))
    rec = {"n_concepts": n_concepts, "cross": f"{k} x {k}", "triples": len(grid), "holdout": M, "a_factorised_sweep_ms_per_triple": spread(ms["a"]),
           "b_call_score_restore_ms_per_triple": spread(ms["b"]), "a_counters": counters, "max_rel_difference_of_summaries_a_vs_b": agree}
    a, b = rec["a_factorised_sweep_ms_per_triple"], rec["b_call_score_restore_ms_per_triple"]
    rec["ranges_disjoint_a_faster"] = a["max"] < b["min"]
    rec["b_over_a_medians"] = b["median"] / a["median"]
    print(json.dumps(rec), flush=True)
    return rec


def by_events(fn):
    """device ms of what ``fn`` launches, REPS times after one warm-up"""
    fn()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return spread(ms)


records = [measure(n, k) for n in (100, 1000) for k in (2, 4)]
# the grid kernel alone, on banks of a 4 x 4 cross's shape over the holdout tries of a scorer
scorer = em.PairEditScorer(pipe, syn.make_requests(100, names="syllable", name_seed=3), hp(), DEV, holdout=holdout, cache_name=f"{tmp}/cache100/")
e1, e2 = scorer.encoders
banks = [torch.rand(4, e.H0.shape[0], 8, dtype=torch.float64, device=DEV) + 0.05 for e in (e1, e2)]
kernel = {}
for k in (2, 4):
    combo = torch.tensor([(i, j) for i in range(k) for j in range(k)], dtype=torch.int32, device=DEV)
    out = torch.empty(k * k, M, 4, dtype=torch.float64, device=DEV)
    kernel[f"C={k * k}"] = by_events(lambda: hip.score_chains_pair_grid(banks[0], e1.trie_h.anc, e1.trie_h.depth, e1.trie_h.lookup_node,
                                                                        banks[1], e2.trie_h.anc, e2.trie_h.depth, e2.trie_h.lookup_node,
                                                                        combo, out=out))
out = {"what": "sweep_emcid_sdxl_text_encoders(score=) [A] against a PairEditScorer + per triple apply_emcid_to_sdxl_text_encoders, "
               "scorer.score(), restore [B]; synthetic SDXL-dimension pair, layers 8-10 and 26-30, projection 1280, 3 prompts per concept, "
               "100 caption prompts held out; wall ms per triple, device-synchronised, arms alternated after a warm-up of each, factor "
               "caches emptied before every repetition of either arm, median [min, max]; score_chains_pair_grid alone by device events",
       "device": torch.cuda.get_device_name(0), "reps": REPS, "mom2_weights": LAMS1, "mom2_weights_2": LAMS2, "edit_weight": E,
       "holdout_trie_rows": [e.trie_h.n_nodes for e in scorer.encoders], "records": records, "score_chains_pair_grid_device_ms": kernel}
out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "sweep_pair.json"), "w"), indent=1)
print(json.dumps({"score_chains_pair_grid_device_ms": kernel}), flush=True)

"""One sweep_emcid_text_encoder call against one apply_emcid_to_text_encoder call (+ restore) per pair, over grids of 4 and 8
distinct (mom2_weight, edit_weight) pairs, bench.py's 1 000-concept synthetic SD-v1.4 set and N = 100: alternated, device-
synchronised, three repetitions each after a warm-up of both, medians and spread (profiles/sweep_vs_calls.json).  Every
repetition starts from empty factor caches: a grid is walked once, each pair is new to the process, as in the user's search.
python scripts/sweep_vs_calls.py  [OUT=dir, default profiles/]"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import torch
from emcid_amd import clip_forward as cf, edit_engine as ee, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter

DEV, REPS, LAYERS = "cuda:0", 3, (7, 8, 9, 10)
GRID8 = [(4000.0, 0.5), (2000.0, 0.4), (6000.0, 0.8), (1000.0, 0.3), (8000.0, 0.6), (3000.0, 0.7), (5000.0, 0.2), (500.0, 0.9)]
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=4000, edit_weight=0.5)
names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
tmp = tempfile.mkdtemp()
stats = tmp + "/stats"
syn.write_stats_cache(stats, names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)
w0 = {n: get_parameter(pipe.text_encoder, n + ".weight").detach().clone() for n in names}


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "spread": max(ms) - min(ms), "all": ms}


def measure(n_concepts, grid):
    reqs = syn.make_requests(n_concepts, names="syllable", name_seed=3)
    cache = f"{tmp}/cache{n_concepts}/"
    if not os.path.exists(cache):
        syn.write_vstar_cache(cache, reqs, hidden, seed=1, scale=0.5)

    def sweep():
        ee.clear_engine_caches()
        ee.TIMING.clear()
        torch.cuda.synchronize()
        t = time.perf_counter()
        em.sweep_emcid_text_encoder(pipe, reqs, EMCIDHyperParams(**hp_d), grid, DEV, visit=lambda point, p: None, cache_name=cache,
                                    stat_dir=stats)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def calls():
        ee.clear_engine_caches()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for lam, e in grid:
            em.apply_emcid_to_text_encoder(pipe, reqs, EMCIDHyperParams(**hp_d), DEV, mom2_weight=lam, edit_weight=e, cache_name=cache,
                                           stats_dir=stats, verbose=False)
            with torch.no_grad():
                for n, w in w0.items():
                    get_parameter(pipe.text_encoder, n + ".weight").copy_(w)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    sweep(), calls()                                           # warm-up of both (kernels loaded, graphs captured, files cached)
    ms = {"sweep": [], "calls": []}
    for i in range(REPS):
        for arm in (("sweep", "calls") if i % 2 == 0 else ("calls", "sweep")):
            ms[arm].append((sweep if arm == "sweep" else calls)() / len(grid))
    host = {k: round(v * 1e3, 3) for k, v in ee.TIMING.items() if k.startswith("sweep")}
    rec = {"n_concepts": n_concepts, "grid_points": len(grid), "sweep_ms_per_point": spread(ms["sweep"]),
           "calls_ms_per_point": spread(ms["calls"]), "host_ms_of_last_sweep": host,
           "counters": {k: cf.LAST_PATHS[k] for k in ("sweep_points", "sweep_cov_factorizations", "sweep_prefix_runs")}}
    gap = rec["calls_ms_per_point"]["median"] - rec["sweep_ms_per_point"]["median"]
    rec["gap_ms"], rec["spreads_combined_ms"] = gap, rec["sweep_ms_per_point"]["spread"] + rec["calls_ms_per_point"]["spread"]
    rec["sweep_accepted"] = gap > rec["spreads_combined_ms"]
    return rec


records = []
for n in (1000, 100):
    r4, r8 = measure(n, GRID8[:4]), measure(n, GRID8)
    # total(G) = shared + G * per_point, from the two grid lengths
    t4, t8 = 4 * r4["sweep_ms_per_point"]["median"], 8 * r8["sweep_ms_per_point"]["median"]
    per_point = (t8 - t4) / 4
    split = {"n_concepts": n, "sweep_per_point_ms": per_point, "sweep_shared_ms": t4 - 4 * per_point}
    records += [r4, r8, {"shared_vs_per_point_from_G4_and_G8": split}]
    print(json.dumps([{k: v for k, v in r.items()} for r in (r4, r8)] + [split]), flush=True)
out = {"what": "sweep_emcid_text_encoder vs one apply_emcid_to_text_encoder + restore per pair; synthetic SD-v1.4 encoder, layers 7-10, "
               "3 prompts per concept; per-point wall ms, device-synchronised; factor caches emptied before every repetition of either arm; "
               "first-layer chains run per point (no batched chain in this build)",
       "device": torch.cuda.get_device_name(0), "reps": REPS, "grid": GRID8, "records": records}
out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "sweep_vs_calls.json"), "w"), indent=1)

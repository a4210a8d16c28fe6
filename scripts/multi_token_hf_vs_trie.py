"""hf vs trie forward at k = 3, 1 000 requests, SD-v1.4 dims: alternated device-synchronised apply_ calls, medians, dW diff
(profiles/multi_token_hf_vs_trie.json).  python scripts/multi_token_hf_vs_trie.py  [OUT=dir]"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import numpy as np, torch
from emcid_amd import clip_forward as cf, edit_engine as ee, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter

DEV, K, N, REPS = "cuda:0", 3, 1000, 12
tmp = tempfile.mkdtemp()
reqs = syn.make_requests(N, names="syllable")
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
layers = (7, 8, 9, 10)
hp_d = dict(syn.sd_hparams_dict(layers=layers, mom2_update_weight=60, mom2_n_samples=100), num_edit_tokens=K, use_new_compute_z=True)
names = [hp_d["rewrite_module_tmp"].format(l) for l in layers]
cache = tmp + "/cache/"
rng = np.random.default_rng(K)
for r in reqs:
    p = syn.vstar_cache_path(cache, r); p.parent.mkdir(parents=True, exist_ok=True)
    np.savez(p, v_star=(0.5 * rng.standard_normal((K, hidden))).astype(np.float32))
syn.write_stats_cache(tmp + "/stats", names, inter, 100, seed=2, t=2 * inter)
pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)
w0 = {n: get_parameter(pipe.text_encoder, n + ".weight").detach().clone() for n in names}

def call(mode):
    ee.FORWARD_MODE = mode
    with torch.no_grad():
        for n, w in w0.items():
            get_parameter(pipe.text_encoder, n + ".weight").copy_(w)
    torch.cuda.synchronize()
    t = time.perf_counter()
    em.apply_emcid_to_text_encoder(pipe, reqs, EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=tmp + "/stats", verbose=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return dt, {n: (get_parameter(pipe.text_encoder, n + ".weight").double() - w0[n].double()).cpu() for n in names}

times = {"hf": [], "trie": []}
for warm in range(2):
    for mode in ("hf", "trie"):
        call(mode)
p0 = dict(cf.LAST_PATHS)
dws = {}
for i in range(REPS):
    for mode in (("hf", "trie") if i % 2 == 0 else ("trie", "hf")):
        dt, dws[mode] = call(mode)
        times[mode].append(dt * 1e3)
diff = max((dws["trie"][n] - dws["hf"][n]).abs().max().item() / dws["hf"][n].abs().max().item() for n in names)
out = {"what": "apply_emcid_to_text_encoder, SD-v1.4-sized synthetic encoder, 1000 requests x 3 prompts, k=3 (3000 concepts), layers 7-10, warm calls, alternated",
       "device": torch.cuda.get_device_name(0), "reps": REPS,
       "hf_ms_median": statistics.median(times["hf"]), "trie_ms_median": statistics.median(times["trie"]),
       "hf_ms": times["hf"], "trie_ms": times["trie"], "dW_max_rel_diff_trie_vs_hf": diff,
       "paths": {k: cf.LAST_PATHS[k] - p0.get(k, 0) for k in ("forward_trie", "forward_hf", "forward_hf_fallback", "fused_edit_layers")},
       "trie_rows": list(cf.LAST_PATHS.get("last_trie_rows", 0) for _ in [0]) + [cf.LAST_PATHS.get("last_trie_tokens", 0)]}
out_dir = os.environ.get("OUT", "bench_out"); os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "multi_token_hf_vs_trie.json"), "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if not k.endswith("_ms")}, indent=1))

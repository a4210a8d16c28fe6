"""What an edit score costs (emcid_main.EditScorer), on the set-up of scripts/sweep_vs_calls.py: the synthetic SD-v1.4 encoder, layers
7-10, 3 prompts per concept, N concepts edited and M caption prompts held out.  Arms, alternated after a warm-up of all of them,
REPS device-synchronised repetitions each, reported as median [min, max] wall ms:
    score        scorer.score() on the edited weights
    hf           the same numbers the way a sweep's ``visit`` has to get them without it: two pipe.text_encoder(...) forwards (the
                 request prompts with a hook on the last edited fc2, the holdout prompts), torch reductions on the GPU against
                 baselines kept from before the edit, one read-back
    sweep        a 4-point sweep's per-point time with visit=lambda: None
    sweep_score  the same sweep with score=holdout
ONE case per process, each under its own time limit, chained so that a failing case ends the chain:
    timeout -k 10 600 python scripts/score_cost.py 100 100 && timeout -k 10 600 python scripts/score_cost.py 100 1000 && \
    timeout -k 10 600 python scripts/score_cost.py 1000 100 && timeout -k 10 600 python scripts/score_cost.py 1000 1000 && \
    python scripts/score_cost.py merge
``merge`` (no GPU) joins the cases' files into OUT/edit_score.json  [OUT=dir, default profiles/]."""
import glob, json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())

out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
if len(sys.argv) == 2 and sys.argv[1] == "merge":
    parts = sorted(glob.glob(os.path.join(out_dir, "edit_score_case_*.json")))
    cases = [json.load(open(p)) for p in parts]
    out = {"what": "EditScorer.score() against two HF forwards + torch reductions, and a sweep's per-point time with and without score=; "
                   "synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per concept, caption prompts held out; wall ms, device-synchronised, "
                   "arms alternated after a warm-up, median [min, max]",
           "device": cases[0]["device"] if cases else None, "cases": cases}
    json.dump(out, open(os.path.join(out_dir, "edit_score.json"), "w"), indent=1)
    for p in parts:
        os.remove(p)
    print(f"{len(cases)} cases -> {os.path.join(out_dir, 'edit_score.json')}")
    sys.exit(0)

import torch
from emcid_amd import compute_z, edit_engine as ee, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_module, get_parameter

N, M = int(sys.argv[1]), int(sys.argv[2])
DEV, REPS, LAYERS = "cuda:0", 5, (7, 8, 9, 10)
GRID = [(4000.0, 0.5), (2000.0, 0.4), (6000.0, 0.8), (1000.0, 0.3)]
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=4000, edit_weight=0.5)
names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
tmp = tempfile.mkdtemp()
stats, cache = tmp + "/stats", tmp + "/cache/"
syn.write_stats_cache(stats, names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
reqs = syn.make_requests(N, names="syllable", name_seed=3)
syn.write_vstar_cache(cache, reqs, hidden, seed=1, scale=0.5)
holdout = [c["caption"] for c in syn.make_captions(M, seed=11)]
pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)
te, tok = pipe.text_encoder, pipe.tokenizer
hp = lambda: EMCIDHyperParams(**hp_d)


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


# ---- the HF arm: baselines from before the edit, then per call two forwards and the reductions ----------------------------------
batch = compute_z.build_prompt_batch(tok, reqs, DEV)
hold = compute_z.tokenize_prompts(holdout, tok, DEV)
hold_mask = hold["attention_mask"].bool()
hold_eos = hold["attention_mask"].sum(1) - 1
last_fc2 = get_module(te, names[-1])
vstar = em.load_v_stars(reqs, hp(), cache).to(DEV)


def hf_read():
    box = {}
    handle = last_fc2.register_forward_hook(lambda mod, args, out: box.__setitem__("out", out))
    try:
        with torch.no_grad():
            te(**batch.inputs)
            Z = compute_z.gather_request_means(box["out"], batch)
            F = te(**hold)[0]
    finally:
        handle.remove()
    return Z, F


def hf_scores(base):
    Z, F = hf_read()
    Z0, F0 = base
    with torch.no_grad():
        Z, Z0, t, F, F0 = Z.double(), Z0.double(), vstar.double(), F.double(), F0.double()
        left = (t - Z).norm(dim=1) / (t - Z0).norm(dim=1)
        cos = ((Z - Z0) * (t - Z0)).sum(1) / ((Z - Z0).norm(dim=1) * (t - Z0).norm(dim=1)).clamp(min=1e-300)
        ratio = ((F - F0).norm(dim=2) / F0.norm(dim=2)).masked_fill(~hold_mask, 0.0)
        dmax, dmean = ratio.max(dim=1).values, ratio.sum(1) / hold_mask.sum(1)
        deos = ratio.gather(1, hold_eos[:, None])[:, 0]
        return torch.cat([left, cos, dmax, dmean, deos]).cpu()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


base = hf_read()
base = (base[0].clone(), base[1].clone())
t0 = time.perf_counter()
scorer = em.EditScorer(pipe, reqs, hp(), DEV, holdout=holdout, cache_name=cache)
torch.cuda.synchronize()
build_ms = (time.perf_counter() - t0) * 1e3
em.apply_emcid_to_text_encoder(pipe, reqs, hp(), DEV, cache_name=cache, stats_dir=stats, verbose=False)
s = scorer.score()
ref = hf_scores(base)
n = len(reqs)
agree = {"left": float((s.left - ref[:n]).abs().max()), "drift_max": float((s.drift_max - ref[2 * n:2 * n + M]).abs().max())}
arms = {"score": lambda: scorer.score(), "hf": lambda: hf_scores(base)}
for fn in arms.values():
    fn(), fn()                                               # warm-up
ms = {k: [] for k in arms}
for i in range(REPS):
    for arm in (("score", "hf") if i % 2 == 0 else ("hf", "score")):
        ms[arm].append(timed(arms[arm]))
# the edited weights go back before the sweeps (a sweep starts from the original ones)
fresh = syn.build_pipe("sd-v1.4", DEV, syllables=True)
with torch.no_grad():
    for nme in names:
        get_parameter(te, nme + ".weight").copy_(get_parameter(fresh.text_encoder, nme + ".weight"))
del fresh


def sweep(score):
    ee.clear_engine_caches()
    return timed(lambda: em.sweep_emcid_text_encoder(pipe, reqs, hp(), GRID, DEV, visit=None if score else (lambda point, p: None),
                                                     cache_name=cache, stat_dir=stats, score=holdout if score else None)) / len(GRID)


sweep(False), sweep(True)
sw = {"sweep": [], "sweep_score": []}
for i in range(REPS):
    for arm in (("sweep", "sweep_score") if i % 2 == 0 else ("sweep_score", "sweep")):
        sw[arm].append(sweep(arm == "sweep_score"))
rec = {"n_concepts": N, "n_holdout": M, "device": torch.cuda.get_device_name(0), "reps": REPS,
       "request_trie_rows": scorer.chunk.trie.n_nodes, "holdout_trie_rows": scorer.trie_h.n_nodes,
       "holdout_tokens_dense": int(hold["attention_mask"].numel()), "scorer_construction_ms": build_ms,
       "score_ms": spread(ms["score"]), "hf_two_forwards_ms": spread(ms["hf"]),
       "sweep_ms_per_point": spread(sw["sweep"]), "sweep_with_score_ms_per_point": spread(sw["sweep_score"]),
       "max_abs_difference_score_vs_hf_fp32": agree, "summary_after_the_edit": s.summary()}
json.dump(rec, open(os.path.join(out_dir, f"edit_score_case_{N:05d}_{M:05d}.json"), "w"), indent=1)
print(json.dumps(rec), flush=True)

"""What an edit score of the SDXL pair costs (emcid_main.PairEditScorer), by the method of scripts/score_cost.py: the synthetic pair at
SDXL's dimensions (TE1 768 / 12 layers edited at 8-10, TE2 1280 / 32 layers edited at 26-30, text projection 1280 -> 1280), 3 prompts
per concept, N concepts edited and M caption prompts held out.  Arms, alternated after a warm-up of both, REPS device-synchronised
repetitions each, reported as median [min, max] wall ms:
    score   scorer.score() on the edited weights
    hf      the same numbers without it: per encoder two ``output_hidden_states=True`` forwards (the request prompts with a hook on
            the last edited fc2; the holdout prompts for hidden_states[-2] and TE2's text_embeds), torch reductions on the GPU
            against baselines kept from before the edit, one read-back
and, bracketed by device events on the tensors a score() has just used, REPS times each: the two kernels that exist for the pair
(``hip.score_chains_pair``, ``hip.score_pooled``) and, to hold the second against, TE2's last-layer replay on the EOS rows.
ONE case per process, each under its own time limit, chained so that a failing case ends the chain:
    timeout -k 10 600 python scripts/score_pair_cost.py 100 100 && timeout -k 10 600 python scripts/score_pair_cost.py 100 1000 && \
    timeout -k 10 600 python scripts/score_pair_cost.py 1000 100 && timeout -k 10 600 python scripts/score_pair_cost.py 1000 1000 && \
    python scripts/score_pair_cost.py merge
``merge`` (no GPU) joins the cases' files into OUT/edit_score_pair.json  [OUT=dir, default profiles/; STATS=dir keeps the synthetic
statistics between the cases instead of writing them anew]."""
import glob, json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())

out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
if len(sys.argv) == 2 and sys.argv[1] == "merge":
    parts = sorted(glob.glob(os.path.join(out_dir, "edit_score_pair_case_*.json")))
    cases = [json.load(open(p)) for p in parts]
    out = {"what": "PairEditScorer.score() against two output_hidden_states=True HF forwards per encoder + torch reductions; synthetic "
                   "SDXL-dimension pair, layers 8-10 and 26-30, projection 1280, 3 prompts per concept, caption prompts held out; wall "
                   "ms, device-synchronised, arms alternated after a warm-up, median [min, max]; the pair's two kernels and TE2's "
                   "last-layer replay on the EOS rows by device events",
           "device": cases[0]["device"] if cases else None, "cases": cases}
    json.dump(out, open(os.path.join(out_dir, "edit_score_pair.json"), "w"), indent=1)
    for p in parts:
        os.remove(p)
    print(f"{len(cases)} cases -> {os.path.join(out_dir, 'edit_score_pair.json')}")
    sys.exit(0)

import torch
from emcid_amd import clip_forward, compute_z, emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDXLHyperParams
from emcid_amd.nethook import get_module

N, M = int(sys.argv[1]), int(sys.argv[2])
DEV, REPS, PROJ = "cuda:0", 5, 1280
hp_d = syn.sdxl_hparams_dict()
(h1, i1), (h2, i2) = syn.ENCODER_DIMS["sdxl-te1"][:2], syn.ENCODER_DIMS["sdxl-te2"][:2]
n1 = [hp_d["rewrite_module_tmp"].format(l) for l in hp_d["layers"]]
n2 = [hp_d["rewrite_module_tmp"].format(l) for l in hp_d["layers_2"]]
tmp = tempfile.mkdtemp()
stats_root = os.environ.get("STATS", tmp)
s1, s2, cache = stats_root + "/s1", stats_root + "/s2", tmp + "/cache/"
if not os.path.isdir(s2):
    syn.write_stats_cache(s1, n1, i1, hp_d["mom2_n_samples"], seed=2, t=2 * i1)
    syn.write_stats_cache(s2, n2, i2, hp_d["mom2_n_samples"], seed=7, t=2 * i2)
reqs = syn.make_requests(N, names="syllable", name_seed=3)
syn.write_vstar_cache(cache, reqs, h1, seed=1, scale=0.5)
syn.write_vstar_cache(cache, reqs, h2, seed=5, scale=0.5, suffix="_2")
holdout = [c["caption"] for c in syn.make_captions(M, seed=11)]
pipe = syn.build_pipe("sdxl", DEV, sdxl=True, syllables=True, projection_dim=PROJ)
hp = lambda: EMCIDXLHyperParams(**hp_d)
encoders = ((pipe.text_encoder, pipe.tokenizer, n1[-1], ""), (pipe.text_encoder_2, pipe.tokenizer_2, n2[-1], "_2"))


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


# ---- the HF arm: baselines from before the edit, then per call two forwards per encoder and the reductions ------------------------
prep = []
for te, tok, last_name, suffix in encoders:
    hold = compute_z.tokenize_prompts(holdout, tok, DEV)
    prep.append((te, compute_z.build_prompt_batch(tok, reqs, DEV), hold, get_module(te, last_name),
                 em.load_v_stars(reqs, hp(), cache, suffix).to(DEV)))
hold_mask = prep[0][2]["attention_mask"].bool()
hold_eos = prep[0][2]["attention_mask"].sum(1) - 1


def hf_read():
    out = []
    for te, batch, hold, last_fc2, _ in prep:
        box = {}
        handle = last_fc2.register_forward_hook(lambda mod, args, o, box=box: box.__setitem__("out", o))
        try:
            with torch.no_grad():
                te(**batch.inputs, output_hidden_states=True)
                Z = compute_z.gather_request_means(box["out"], batch)
                res = te(**hold, output_hidden_states=True)
        finally:
            handle.remove()
        out.append((Z, res.hidden_states[-2], getattr(res, "text_embeds", None)))
    return out


def hf_scores(base):
    now = hf_read()
    with torch.no_grad():
        parts, num, den = [], 0.0, 0.0
        for (Z, H, _), (Z0, H0, _), (_, _, _, _, vstar) in zip(now, base, prep):
            Z, Z0, t, H, H0 = Z.double(), Z0.double(), vstar.double(), H.double(), H0.double()
            parts.append((t - Z).norm(dim=1) / (t - Z0).norm(dim=1))
            parts.append(((Z - Z0) * (t - Z0)).sum(1) / ((Z - Z0).norm(dim=1) * (t - Z0).norm(dim=1)).clamp(min=1e-300))
            n2_, d2_ = (H - H0).pow(2).sum(2), H0.pow(2).sum(2)
            num, den = num + n2_, den + d2_
            own = (n2_ / d2_).sqrt().masked_fill(~hold_mask, 0.0)
            parts += [own.max(dim=1).values, own.sum(1) / hold_mask.sum(1), own.gather(1, hold_eos[:, None])[:, 0]]
        ratio = (num / den).sqrt().masked_fill(~hold_mask, 0.0)
        parts += [ratio.max(dim=1).values, ratio.sum(1) / hold_mask.sum(1), ratio.gather(1, hold_eos[:, None])[:, 0]]
        e, e0 = now[1][2].double(), base[1][2].double()
        parts.append((e - e0).norm(dim=1) / e0.norm(dim=1))
        return [p.cpu() for p in parts]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


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


base = [tuple(None if x is None else x.clone() for x in enc) for enc in hf_read()]
t0 = time.perf_counter()
scorer = em.PairEditScorer(pipe, reqs, hp(), DEV, holdout=holdout, cache_name=cache)
torch.cuda.synchronize()
build_ms = (time.perf_counter() - t0) * 1e3
em.apply_emcid_to_sdxl_text_encoders(pipe, reqs, hp(), DEV, cache_name=cache, stat_dir=s1, stat_dir_2=s2, verbose=False)
s = scorer.score()
ref = hf_scores(base)
# parts: per encoder (left, cos, own max, mean, eos), then the pair's (max, mean, eos), then the pooled drift
agree = {"left_1": float((s.te1.left - ref[0]).abs().max()), "left_2": float((s.te2.left - ref[5]).abs().max()),
         "drift_max": float((s.drift_max - ref[10]).abs().max()), "drift_eos": float((s.drift_eos - ref[12]).abs().max()),
         "drift_pooled": float((s.drift_pooled - ref[13]).abs().max())}
arms = {"score": lambda: scorer.score(), "hf": lambda: hf_scores(base)}
for fn in arms.values():
    fn(), fn()                                               # warm-up
ms = {k: [] for k in arms}
for i in range(REPS):
    for arm in (("score", "hf") if i % 2 == 0 else ("hf", "score")):
        ms[arm].append(timed(arms[arm]))

# ---- the pair's own two kernels, and the replay the second is held against, by device events ------------------------------------
e1, e2 = scorer.encoders
with torch.no_grad():
    g, L = e2.graph, len(e2.graph.layers)
    state = clip_forward.run_layers_from(g, e2.trie_h, e2._state_h, e2.layers[0], L - 2, None, last_rows_only=False)
    rows = clip_forward.run_layers_from(g, e2.trie_h, state, L - 1, L - 1, None, last_rows_only=True)[0]
    h_last = rows.index_select(0, e2.trie_h.lookup_in_query)
    out4 = torch.empty(M, 4, dtype=torch.float64, device=DEV)
    kernels = {
        "score_chains_pair": by_events(lambda: hip.score_chains_pair(
            e1.node, e1.trie_h.anc, e1.trie_h.depth, e1.trie_h.lookup_node,
            e2.node, e2.trie_h.anc, e2.trie_h.depth, e2.trie_h.lookup_node, out=out4)),
        "score_pooled": by_events(lambda: hip.score_pooled(h_last, e2.H0last, scorer.ln2, scorer.proj.weight, out=out4)),
        "te2_last_layer_replay_on_eos_rows": by_events(
            lambda: clip_forward.run_layers_from(g, e2.trie_h, state, L - 1, L - 1, None, last_rows_only=True)),
    }
rec = {"n_concepts": N, "n_holdout": M, "device": torch.cuda.get_device_name(0), "reps": REPS,
       "request_trie_rows": [e.chunk.trie.n_nodes for e in scorer.encoders], "holdout_trie_rows": [e.trie_h.n_nodes for e in scorer.encoders],
       "holdout_eos_rows": int(e2.trie_h.query_rows.numel()), "holdout_tokens_dense": int(hold_mask.numel()),
       "scorer_construction_ms": build_ms, "score_ms": spread(ms["score"]), "hf_four_forwards_ms": spread(ms["hf"]),
       "device_ms_by_events": kernels, "max_abs_difference_score_vs_hf_fp32": agree, "summary_after_the_edit": s.summary()}
json.dump(rec, open(os.path.join(out_dir, f"edit_score_pair_case_{N:05d}_{M:05d}.json"), "w"), indent=1)
print(json.dumps(rec), flush=True)

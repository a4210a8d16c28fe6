"""What rescale, reweight and a session sweep cost, each against the only earlier way to the same state (profiles/session_rescale.json).
The set-up of scripts/session_release_cost.py: synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per concept, one process, a warm-up of
every arm, REPS device-synchronised repetitions per arm, the arms alternated; median [min, max] wall ms per call.

  rescale    EditSession.rescale between (4000, 0.5) and (2000, 0.4) at M = 100 / 1 000 / 1 800 held rows, the factors of both points
             warm in the factor cache.  Against: a FRESH session at the new point whose rows are re-entered by retain lists (its state
             allocated outside the timed window) — an arm that exists for RETAINED rows only: an edited row cannot be re-entered.
  reweight   EditSession.reweight of 10 rows at the front / at row 500 of 1 000, weight 1 <-> 4.  Against: release + retain of the
             same 10 concepts at the new weight (the rows then sit at the end of the set).
  sweep      EditSession.sweep of 100 new concepts over 4 and 8 pairs at M = 100 / 1 000 with an EditScorer of 100 holdout prompts,
             per point.  Against, per point: a fresh session at that point — retain rebuild of the M rows, apply, score(), restore().

Between repetitions the state is put back from a copy, outside the timed window — a measurement device, not an interface.
python scripts/session_rescale_cost.py  [OUT=dir, default profiles/]"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import torch
import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams

DEV, REPS, LAYERS = "cuda:0", 5, (7, 8, 9, 10)
A, B, CHUNK = (4000.0, 0.5), (2000.0, 0.4), 1000
GRID8 = [(4000.0, 0.5), (2000.0, 0.5), (4000.0, 0.4), (8000.0, 0.6), (1000.0, 0.5), (2000.0, 0.4), (8000.0, 0.5), (4000.0, 0.6)]
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=int(A[0]), edit_weight=A[1])
names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
tmp = tempfile.mkdtemp()
stats, cache = tmp + "/stats", tmp + "/cache/"
syn.write_stats_cache(stats, names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
reqs = syn.make_requests(1800 + 100, names="syllable", name_seed=3)
held = [{"source": r["source"], "prompts": list(r["prompts"])} for r in reqs[:1800]]
new = reqs[1800:]
syn.write_vstar_cache(cache, new, hidden, seed=1, scale=0.5)
holdout = [c["caption"] for c in syn.make_captions(100, seed=11)]
pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)


def hp(point=A):
    return EMCIDHyperParams(**dict(hp_d, mom2_update_weight=point[0], edit_weight=point[1]))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


def session_at(M, point=A, rows=None):
    sess = emcid_amd.EditSession(pipe, hp(point), DEV, stats_dir=stats)
    rows = held[:M] if rows is None else rows
    for a in range(0, len(rows), CHUNK):
        sess.retain(rows[a:a + CHUNK])
    return sess


def snapshot(sess):
    k = sess.keys
    return ([t.clone() for t in k.Yp + k.Lp + k.tile_inv], k.row_scale.clone(), k.M, sess.rows(), sess.retained, sess._retains,
            sess._fixed, sess._shared)


def put_back(sess, c):
    k = sess.keys
    for t, s in zip(k.Yp + k.Lp + k.tile_inv, c[0]):
        t.copy_(s)
    k.row_scale.copy_(c[1])
    k.M, sess._ledger, sess.retained, sess._retains, sess.released = c[2], list(c[3]), c[4], c[5], 0
    sess._fixed, sess._shared = c[6], c[7]
    sess.hparams.mom2_update_weight, sess.hparams.edit_weight = c[6][0], c[6][1]


def fresh_rebuild(M, point, fresh):
    """the comparison arm of rescale: ``fresh`` (a session at ``point`` with its state allocated) takes the M rows by retain lists"""
    fresh.reset()
    for a in range(0, M, CHUNK):
        fresh.retain(held[a:min(a + CHUNK, M)])


def alternate(arms):
    """warm every arm once, then REPS repetitions alternated; {arm: [ms]}"""
    for fn in arms.values():
        fn()
    runs = {a: [] for a in arms}
    order = list(arms)
    for i in range(REPS):
        for a in (order if i % 2 == 0 else order[::-1]):
            runs[a].append(arms[a]())
    return runs


records = {"rescale": [], "reweight": [], "sweep": []}
gauges = {}      # LAST_PATHS right after the arm they belong to: reset() / restore() of ANY session zeroes the session_* entries

# ---- rescale --------------------------------------------------------------------------------------------------------------------
for M in (100, 1000, 1800):
    sess = session_at(M)
    sess.rescale(*B)            # (both points' factors into the factor cache)
    sess.rescale(*A)
    copy = snapshot(sess)
    fresh = emcid_amd.EditSession(pipe, hp(B), DEV, stats_dir=stats)
    fresh._ensure_keys()

    def arm_rescale():
        ms = timed(lambda: sess.rescale(*B))
        gauges[f"rescale M={M}"] = {"session_rescales": cf.LAST_PATHS["session_rescales"]}     # (this session's calls so far)
        put_back(sess, copy)
        return ms

    runs = alternate({"rescale": arm_rescale, "fresh_retain": lambda: timed(lambda: fresh_rebuild(M, B, fresh))})
    records["rescale"].append({"preserved": M, **{a + "_ms": spread(v) for a, v in runs.items()}})
    print(json.dumps({"rescale M": M, **{a: round(statistics.median(v), 3) for a, v in runs.items()}}), flush=True)
    del sess, copy, fresh
    torch.cuda.empty_cache()

# ---- reweight -------------------------------------------------------------------------------------------------------------------
sess = session_at(1000)
copy = snapshot(sess)
for first in (0, 500):
    rows = held[first:first + 10]
    gone = [r["source"] for r in rows]

    def arm_reweight():
        ms = timed(lambda: sess.reweight(gone, 4.0))
        put_back(sess, copy)
        return ms

    def arm_release_retain():
        ms = timed(lambda: (sess.release(gone), sess.retain(rows, weight=4.0)))
        put_back(sess, copy)
        return ms

    runs = alternate({"reweight": arm_reweight, "release_retain": arm_release_retain})
    records["reweight"].append({"preserved": 1000, "rows": 10, "first": first, **{a + "_ms": spread(v) for a, v in runs.items()}})
    print(json.dumps({"reweight first": first, **{a: round(statistics.median(v), 3) for a, v in runs.items()}}), flush=True)
del sess, copy
torch.cuda.empty_cache()

# ---- sweep ----------------------------------------------------------------------------------------------------------------------
scorer = em.EditScorer(pipe, new, hp(), DEV, holdout=holdout, cache_name=cache)
for M in (100, 1000):
    sess = session_at(M)
    fresh = {pt: emcid_amd.EditSession(pipe, hp(pt), DEV, stats_dir=stats) for pt in GRID8[:2]}
    for f in fresh.values():
        f._ensure_keys()
    for n_pairs in (4, 8):
        grid = GRID8[:n_pairs]

        def arm_sweep():
            ms = timed(lambda: sess.sweep(new, grid, cache_name=cache, scorer=scorer)) / len(grid)
            gauges[f"sweep M={M} pairs={len(grid)}"] = {k: cf.LAST_PATHS[k] for k in ("session_sweep_points", "sweep_cov_factorizations",
                                                                                  "sweep_prefix_runs")}
            return ms

        def arm_fresh():
            def points():
                for pt, f in fresh.items():        # two of the grid's points: the arm's cost does not depend on the pair
                    fresh_rebuild(M, pt, f)
                    f.apply(new, cache_name=cache)
                    scorer.score()
                    f.restore()
            return timed(points) / len(fresh)

        runs = alternate({"sweep_per_point": arm_sweep, "fresh_session_per_point": arm_fresh})
        records["sweep"].append({"preserved": M, "pairs": n_pairs, "new_concepts": len(new), "holdout": len(holdout),
                                 **{a + "_ms": spread(v) for a, v in runs.items()}})
        print(json.dumps({"sweep M": M, "pairs": n_pairs, **{a: round(statistics.median(v), 3) for a, v in runs.items()}}), flush=True)
    del sess, fresh
    torch.cuda.empty_cache()

out = {"what": "EditSession.rescale / reweight / sweep against the earlier way to the same state (see scripts/session_rescale_cost.py); "
               "synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per concept; wall ms per call (sweep: per point), device-synchronised, "
               "arms alternated in one process after a warm-up of each",
       "device": torch.cuda.get_device_name(0), "reps": REPS, "capacity": int(0.6 * inter), "records": records,
       "paths": {k: cf.LAST_PATHS.get(k, 0) for k in ("forward_trie", "forward_hf_fallback")}, "gauges": gauges}
out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "session_rescale.json"), "w"), indent=1)

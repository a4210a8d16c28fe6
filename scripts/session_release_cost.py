"""What a release costs: EditSession.release of R rows out of P preserved ones, the smallest released row at `first`, against an
EditSession.retain of as many requests as the release rebuilds rows (P - R - first of them, behind `first` preserved rows) — the
operation that existed before and runs the same chain plus a forward, a key gather and the product against X.  The set-up of
scripts/session_retain_cost.py: synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per concept, one process, a warm-up of every arm,
seven device-synchronised repetitions per arm, the arms alternated; median [min, max] wall ms per call
(profiles/session_release.json).  Cases (P, R, first): (1 000, 10, 0), (1 000, 10, 500), (1 000, 100, 0), (1 800, 10, 0) and the last
10 of 1 000 (trailing rows: nothing is launched, there is no comparison arm).

Between repetitions the state (Yp, Lp, the tile inverses, M, the row scales, the ledger) is put back from a copy, outside the timed
window — a measurement device, not an interface.
python scripts/session_release_cost.py  [OUT=dir, default profiles/]"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import torch
import emcid_amd
from emcid_amd import clip_forward as cf, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams

DEV, REPS, LAYERS = "cuda:0", 7, (7, 8, 9, 10)
LAM, EW, CHUNK = 4000.0, 0.5, 1000
CASES = ((1000, 10, 0), (1000, 10, 500), (1000, 100, 0), (1800, 10, 0), (1000, 10, 990))
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=int(LAM), edit_weight=EW)
names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
tmp = tempfile.mkdtemp()
stats = tmp + "/stats"
syn.write_stats_cache(stats, names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
reqs = syn.make_requests(1800 + 1790, names="syllable", name_seed=3)
held = [{"source": r["source"], "prompts": list(r["prompts"])} for r in reqs[:1800]]
new = [{"source": r["source"], "prompts": list(r["prompts"])} for r in reqs[1800:]]
pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


def session_at(P):
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
    for a in range(0, P, CHUNK):
        sess.retain(held[a:min(a + CHUNK, P)])
    assert sess.preserved == P
    k = sess.keys
    copy = ([t.clone() for t in k.Yp + k.Lp + k.tile_inv], k.row_scale.clone(), sess.rows(), sess.retained, sess._retains)
    return sess, copy


def put_back(sess, copy, P):
    k = sess.keys
    for t, c in zip(k.Yp + k.Lp + k.tile_inv, copy[0]):
        t.copy_(c)
    k.row_scale.copy_(copy[1])
    k.M, sess._ledger, sess.retained, sess._retains, sess.released = P, list(copy[2]), copy[3], copy[4], 0


def call(sess, copy, P, R, first, arm):
    """one timed call of ``arm``, then the state back where it was"""
    if arm == "release":
        gone = [r["source"] for r in held[first:first + R]]
        ms = timed(lambda: sess.release(gone))
        assert sess.preserved == P - R
    else:                                       # the rows a release rebuilds, entered the way that existed before: a retain list
        sess.keys.M, sess._ledger = first, sess._ledger[:first]
        n = P - R - first
        ms = timed(lambda: sess.retain(new[:n]))
        assert sess.preserved == P - R
    put_back(sess, copy, P)
    return ms


records = []
for P, R, first in CASES:
    sess, copy = session_at(P)
    rebuilt = P - R - first
    arms = ("release", "retain") if rebuilt > 0 else ("release",)
    for arm in arms:                            # warm-up of every arm at this shape (kernels loaded, workspaces allocated)
        call(sess, copy, P, R, first, arm)
    runs = {a: [] for a in arms}
    for i in range(REPS):
        for arm in (arms if i % 2 == 0 else arms[::-1]):
            runs[arm].append(call(sess, copy, P, R, first, arm))
    records.append({"preserved": P, "released": R, "first": first, "rebuilt": rebuilt, **{a + "_ms": spread(v) for a, v in runs.items()}})
    print(json.dumps({"preserved": P, "released": R, "first": first, "rebuilt": rebuilt,
                      **{a: round(statistics.median(v), 3) for a, v in runs.items()}}), flush=True)
    del sess, copy
    torch.cuda.empty_cache()

out = {"what": "EditSession.release(R rows of P preserved, the smallest at `first`) vs EditSession.retain(as many requests as the release "
               "rebuilds rows, behind `first` preserved rows); synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per concept; wall ms per "
               "call, device-synchronised, arms alternated in one process after a warm-up of each; rebuilt = 0: trailing rows, no launch",
       "device": torch.cuda.get_device_name(0), "reps": REPS, "capacity": int(0.6 * inter), "records": records,
       "paths": {k: cf.LAST_PATHS.get(k, 0) for k in ("forward_trie", "forward_hf_fallback", "session_released_rows")}}
out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "session_release.json"), "w"), indent=1)

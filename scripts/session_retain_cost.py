"""What a retain list costs: EditSession.retain of N requests against EditSession.apply of the same N at the same M, and a step with
report=True against one without.  The set-up of scripts/session_vs_refactor.py: synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per
concept, one process, a warm-up of every arm, seven device-synchronised repetitions per arm, the arms alternated; median [min, max]
wall ms per call (profiles/session_retain.json).  N = 100 and 1 000 at M = 0 and 800 preserved rows (a retain list of 800).

A retain call runs a strict subset of a step's launches (no Zc, no v* read, no Zk / Zp / U half, no weight update and no re-split of
the new weight), so it should never be the slower arm; the file says by how much it is the faster one.

Between repetitions the session is rewound to M rows (``sess.keys.M = M``: the rows a call wrote behind M are simply written again)
and an apply's weights are put back, both outside the timed window — a measurement device, not an interface.
python scripts/session_retain_cost.py  [OUT=dir, default profiles/]"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import torch
import emcid_amd
from emcid_amd import clip_forward as cf, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter

DEV, REPS, LAYERS = "cuda:0", 7, (7, 8, 9, 10)
LAM, EW, HELD, CASES = 4000.0, 0.5, 800, ((100, 0), (100, 800), (1000, 0), (1000, 800))
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=int(LAM), edit_weight=EW)
names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
tmp = tempfile.mkdtemp()
stats, cache = tmp + "/stats", tmp + "/cache/"
syn.write_stats_cache(stats, names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
reqs = syn.make_requests(HELD + 1000, names="syllable", name_seed=3)
held, new = reqs[:HELD], reqs[HELD:]
syn.write_vstar_cache(cache, new, hidden, seed=1, scale=0.5)
pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)
te = pipe.text_encoder
w0 = {n: get_parameter(te, n + ".weight").detach().clone() for n in names}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def restore():
    with torch.no_grad():
        for n, w in w0.items():
            get_parameter(te, n + ".weight").copy_(w)


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


def session_at(M):
    restore()
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
    if M:
        sess.retain(held[:M])
    assert sess.preserved == M
    return sess


def call(sess, M, arm, step):
    """one timed call of ``arm`` at M preserved rows, then the session and the weights back where they were"""
    sess.report_on = arm == "apply+report"
    ms = timed((lambda: sess.retain(step)) if arm == "retain" else (lambda: sess.apply(step, cache_name=cache)))
    assert sess.preserved == M + len(step)
    sess.keys.M = M
    if arm != "retain":
        restore()
    return ms


ARMS = ("retain", "apply", "apply+report")
records = []
for N, M in CASES:
    sess, step = session_at(M), new[:N]
    for arm in ARMS:                          # warm-up of every arm at this shape (kernels loaded, workspaces allocated, files cached)
        call(sess, M, arm, step)
    runs = {a: [] for a in ARMS}
    for i in range(REPS):
        for arm in (ARMS if i % 2 == 0 else ARMS[::-1]):
            runs[arm].append(call(sess, M, arm, step))
    rec = {"N": N, "M": M, **{a.replace("+", "_") + "_ms": spread(v) for a, v in runs.items()}}
    records.append(rec)
    print(json.dumps({"N": N, "M": M, **{a: round(statistics.median(v), 3) for a, v in runs.items()}}), flush=True)

out = {"what": "EditSession.retain(N requests) vs EditSession.apply(the same N) at M preserved rows, and apply with report=True; "
               "synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per concept; wall ms per call, device-synchronised, arms alternated "
               "in one process after a warm-up of each",
       "device": torch.cuda.get_device_name(0), "reps": REPS, "capacity": sess.capacity, "records": records,
       "paths": {k: cf.LAST_PATHS.get(k, 0) for k in ("forward_trie", "forward_hf_fallback", "session_retained_rows")}}
out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "session_retain.json"), "w"), indent=1)

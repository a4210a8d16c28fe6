"""What EditSession.fold costs (profiles/session_fold.json).  Synthetic SD-v1.4 encoder, layers 7-10, one MI355X, arms alternated in
one process, seven repetitions each after a warm-up, device-synchronised wall ms, median [min, max].  No threshold.
 1. one fold (all four layers, the flag read included) at M = 460, 1 000, 1 800 preserved rows against a cold factor_cov +
    cov_inverse of the same four layers: the fold is that plus one M x d x d triangular product and one SYRK per layer, run layer
    by layer where the cold factorization is batched over the layers.
 2. a session step of N = 100 at M = 100 on the private factors (after a fold) against the same step at M = 100 before any fold,
    each in a session of its own; (3)'s per-step medians give the same pair inside one session (step 1 against the step after a
    folding one).
 3. a 40-step session of N = 100 per step with on_full="fold" at the default capacity, per step (folds included), against the
    refactor-every-step arm of scripts/session_vs_refactor.py (C_eff = C + P^T P / lam as a new statistics tensor, cold factors)
    over the same 40 steps.
python scripts/session_fold_cost.py  [OUT=dir, default profiles/]"""
import gc, json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import torch
import emcid_amd
from emcid_amd import clip_forward as cf, edit_engine as ee, emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter

DEV, REPS, LAYERS, N, STEPS = "cuda:0", 7, (7, 8, 9, 10), 100, 40
LAM, EW = 4000.0, 0.5
FOLD_AT = (460, 1000, 1800)
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=int(LAM), edit_weight=EW)
names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
tmp = tempfile.mkdtemp()
stats, cache = tmp + "/stats", tmp + "/cache/"
syn.write_stats_cache(stats, names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
reqs = syn.make_requests(N * STEPS, names="syllable", name_seed=3)
vstars = torch.from_numpy(syn.write_vstar_cache(cache, reqs, hidden, seed=1, scale=0.5)).to(DEV)
pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)
te, tok = pipe.text_encoder, pipe.tokenizer
w0 = {n: get_parameter(te, n + ".weight").detach().clone() for n in names}
covs = {l: em.get_cov_text_encoder(te, tok, hp_d["rewrite_module_tmp"].format(l), hp_d["mom2_dataset"], hp_d["mom2_n_samples"],
                                   hp_d["mom2_dtype"], stat_dir=stats, verbose=False).to(DEV).float().contiguous() for l in LAYERS}


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


def session(**kw):
    restore()
    return emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, **kw)


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


# ---- 1. one fold against a cold factorization -------------------------------------------------------------------------------------
cold_ws = hip.CovFactors(len(LAYERS), inter, DEV)


def cold_factor():
    cold_ws.info.zero_()
    hip.factor_cov([covs[l] for l in LAYERS], LAM, EW, cold_ws, inverse=True)
    assert int(cold_ws.info.item()) == 0


def fold_and_undo(sess, M):
    """one fold of the M preserved rows, timed; then the session put back to M unfolded rows (a fold never writes Yp)"""
    ms = timed(sess.fold)
    assert sess.preserved == 0 and sess.folded == M
    sess.keys.M, sess.folded, sess.folds, sess.private_factors, sess._base = M, 0, 0, None, None
    return ms


fold_records = []
sess, lo = session(), 0
for M in FOLD_AT:
    while sess.preserved < M:
        n = min(N, M - sess.preserved)
        sess.apply(reqs[lo:lo + n], cache_name=cache)
        lo += n
    fold_and_undo(sess, M), cold_factor()                  # warm-up of both
    f, c = [], []
    for i in range(REPS):
        for arm in (("fold", "cold") if i % 2 == 0 else ("cold", "fold")):
            (f if arm == "fold" else c).append(fold_and_undo(sess, M) if arm == "fold" else timed(cold_factor))
    fold_records.append({"M": M, "fold_ms": spread(f), "cold_factor_ms": spread(c)})
    print(json.dumps({"M": M, "fold_ms": statistics.median(f), "cold_factor_ms": statistics.median(c)}), flush=True)
state_bytes = sess.keys.nbytes
del sess

# ---- 2. a step on the private factors against the same step on the cached ones -------------------------------------------------------


def step_at_100(folded):
    s = session()
    s.apply(reqs[:N], cache_name=cache)
    if folded:
        s.fold()
        s.apply(reqs[N:2 * N], cache_name=cache)
    assert s.preserved == N and (s.private_factors is not None) == folded
    gc.collect()                # (the sessions of earlier repetitions: not inside the window)
    return timed(lambda: s.apply(reqs[2 * N:3 * N], cache_name=cache))


step_at_100(False), step_at_100(True)
steps = {False: [], True: []}
for i in range(REPS):
    for folded in ((False, True) if i % 2 == 0 else (True, False)):
        steps[folded].append(step_at_100(folded))
print(json.dumps({"step_M100_ms": statistics.median(steps[False]), "step_M100_after_fold_ms": statistics.median(steps[True])}), flush=True)

# ---- 3. 40 steps with on_full="fold" against refactoring every step ----------------------------------------------------------------


def folding_arm():
    s = session(on_full="fold")
    ms, folded_at = [], []
    for k in range(STEPS):
        before = s.folds
        ms.append(timed(lambda: s.apply(reqs[k * N:(k + 1) * N], cache_name=cache)))
        if s.folds != before:
            folded_at.append(k)
    assert s.preserved + s.folded == N * STEPS
    return ms, folded_at


def refactor_arm():
    restore()
    eff = {l: c.clone() for l, c in covs.items()}
    ms = []
    s_gain = EW / 0.5
    for k in range(STEPS):
        step, kept = reqs[k * N:(k + 1) * N], {}

        def call():
            plan = ee.prepare_encoder_edit(te, tok, step, list(LAYERS), hp_d["rewrite_module_tmp"], LAM, EW, vstars[k * N:(k + 1) * N],
                                           {l: eff[l] for l in LAYERS}, layer_module_tmp=hp_d["layer_module_tmp"])
            plan.solver = "dual"
            kept["edits"] = ee.run_encoder_edit(plan, trace=True)
            ee.check_info(plan)
        ms.append(timed(call))
        eff = {e.layer: eff[e.layer] + (e.K.t() @ e.K) * (s_gain * 0.5 / ((1.0 - EW) * LAM)) for e in kept["edits"]}
    return ms


folding_arm(), refactor_arm()
per_step = {"fold": [], "refactor": []}
fold_steps, folds, by_index = [], [], []
for i in range(REPS):
    for arm in (("fold", "refactor") if i % 2 == 0 else ("refactor", "fold")):
        if arm == "fold":
            ms, folds = folding_arm()
            fold_steps += [ms[k] for k in folds]
            by_index.append(ms)
            per_step["fold"].append(sum(ms) / STEPS)
        else:
            per_step["refactor"].append(sum(refactor_arm()) / STEPS)
print(json.dumps({"per_step_fold_ms": statistics.median(per_step["fold"]), "per_step_refactor_ms": statistics.median(per_step["refactor"]),
                  "folds": folds}), flush=True)
capacity = int(0.6 * inter)
out = {"what": "EditSession.fold: (1) one fold of M preserved rows over four layers vs a cold factor_cov + cov_inverse of the same layers; "
               "(2) a step of N = 100 at M = 100 before any fold vs after one (private factors); (3) ms per step of a 40-step session, "
               "N = 100, on_full='fold', default capacity, folds included, vs C_eff = C + P^T P / lam refactored every step; synthetic "
               "SD-v1.4 encoder, layers 7-10, wall ms, device-synchronised, arms alternated in one process",
       "device": torch.cuda.get_device_name(0), "reps": REPS, "d": inter, "capacity": capacity, "fold": fold_records,
       "step_M100_ms": spread(steps[False]), "step_M100_after_fold_ms": spread(steps[True]),
       "forty_steps": {"per_step_fold_ms": spread(per_step["fold"]), "per_step_refactor_ms": spread(per_step["refactor"]), "folds": folds,
                       "steps_that_folded_ms": spread(fold_steps) if fold_steps else None,
                       # step k of the folding arm, median over the repetitions: k = 1 runs at M = 100 on the cached factors, the
                       # step after a folding one at M = 100 on the private factors, inside the same session
                       "fold_arm_ms_by_step": [statistics.median(r[k] for r in by_index) for k in range(STEPS)]},
       "session_state_bytes": state_bytes,
       "fold_state_bytes": int(hip.load().emcid_cov_factor_workspace_bytes(len(LAYERS), inter)) + len(LAYERS) * cold_ws.dp ** 2 * 8,
       "paths": {k: cf.LAST_PATHS.get(k, 0) for k in ("session_steps", "session_folds", "session_folded_rows", "forward_trie",
                                                      "forward_hf_fallback")}}
restore()
out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "session_fold.json"), "w"), indent=1)

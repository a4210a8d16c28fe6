"""An EditSession step against the only route to the same update without a session: fold the earlier keys into the statistics,
C_eff = C + P^T P / lam (a NEW statistics tensor, so the factor cache misses and lam C_eff' is refactored every step), then a
plain call.  Synthetic SD-v1.4 encoder, layers 7-10, steps of N = 100 new concepts at M = 0, 100, ... 1 000 preserved ones; the two
arms alternate within one process, seven repetitions each after a warm-up of both, device-synchronised wall time per step; median,
min and max per M (profiles/session_vs_refactor.json).  No threshold: the file confirms or refutes "a step stays near a warm call
while the refactor route pays the cold-factor cost".  A third figure per repetition, "warm_plain_ms": one plain
apply_emcid_to_text_encoder call on 100 unseen concepts with warm factors (the fused edit-layer call a session step does not take).
The arms are not quite like for like, and both differences favour the refactor arm: its window holds only the engine's prepare / run /
check on v* rows that are already in HBM (the session arm reads the v* files through emcid_main's loader, as a user's call does),
and forming the next step's C_eff (K^T K and a 3072 x 3072 add per layer) happens outside it.
python scripts/session_vs_refactor.py  [OUT=dir, default profiles/]"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import torch
import emcid_amd
from emcid_amd import clip_forward as cf, edit_engine as ee, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter

DEV, REPS, LAYERS, N, STEPS = "cuda:0", 7, (7, 8, 9, 10), 100, 11
LAM, EW = 4000.0, 0.5
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=int(LAM), edit_weight=EW)
names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
tmp = tempfile.mkdtemp()
stats, cache = tmp + "/stats", tmp + "/cache/"
syn.write_stats_cache(stats, names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
reqs = syn.make_requests(N * (STEPS + 1), names="syllable", name_seed=3)          # the last N: the warm plain call's
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


def session_arm():
    """(i) EditSession.apply per step; the factors of lam C' stay in the factor cache throughout"""
    restore()
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
    ms = [timed(lambda s=s: sess.apply(reqs[s * N:(s + 1) * N], cache_name=cache)) for s in range(STEPS)]
    assert sess.preserved == N * STEPS
    return ms


def refactor_arm():
    """(ii) C_eff = C + P^T P 0.5 / ((1 - e) lam) per layer as a new tensor, then the engine's plain call on it: cold factors"""
    restore()
    eff = {l: c.clone() for l, c in covs.items()}
    ms = []
    s_gain = EW / 0.5
    for s in range(STEPS):
        step, kept = reqs[s * N:(s + 1) * N], {}

        def call():
            plan = ee.prepare_encoder_edit(te, tok, step, list(LAYERS), hp_d["rewrite_module_tmp"], LAM, EW, vstars[s * N:(s + 1) * N],
                                           {l: eff[l] for l in LAYERS}, layer_module_tmp=hp_d["layer_module_tmp"])
            plan.solver = "dual"
            kept["edits"] = ee.run_encoder_edit(plan, trace=True)          # (trace: keeps the K rows the kernels made anyway)
            ee.check_info(plan)
        ms.append(timed(call))
        # the next step's statistics, a new tensor per layer — outside the timed window
        eff = {e.layer: eff[e.layer] + (e.K.t() @ e.K) * (s_gain * 0.5 / ((1.0 - EW) * LAM)) for e in kept["edits"]}
    return ms


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


def warm_plain():
    """a plain call on N concepts with the factors of lam C' warm (the call before it left them in the cache)"""
    restore()
    hp = lambda: EMCIDHyperParams(**hp_d)
    em.apply_emcid_to_text_encoder(pipe, reqs[:N], hp(), DEV, cache_name=cache, stats_dir=stats, verbose=False)
    return timed(lambda: em.apply_emcid_to_text_encoder(pipe, reqs[STEPS * N:], hp(), DEV, cache_name=cache, stats_dir=stats, verbose=False))


session_arm(), refactor_arm(), warm_plain()                     # warm-up of all (kernels loaded, files cached)
runs = {"session": [], "refactor": []}
warm = []
for i in range(REPS):
    warm.append(warm_plain())
    for arm in (("session", "refactor") if i % 2 == 0 else ("refactor", "session")):
        runs[arm].append((session_arm if arm == "session" else refactor_arm)())
records = [{"M": s * N, "N": N, "session_ms": spread([r[s] for r in runs["session"]]),
            "refactor_ms": spread([r[s] for r in runs["refactor"]])} for s in range(STEPS)]
for r in records:
    print(json.dumps({"M": r["M"], "session_ms": r["session_ms"]["median"], "refactor_ms": r["refactor_ms"]["median"]}), flush=True)
out = {"what": "EditSession.apply per step vs C_eff = C + P^T P / lam as a new statistics tensor + a plain dual call (factors cold every "
               "step); synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per concept, N = 100 new concepts per step; wall ms per step, "
               "device-synchronised, arms alternated in one process",
       "device": torch.cuda.get_device_name(0), "reps": REPS, "session_state_bytes": None, "warm_plain_ms": spread(warm),
       "asymmetry": "refactor arm: v* rows already in HBM, engine entry points, C_eff formed outside the window; session arm: "
                    "emcid_main's loader reads the v* files inside the window — both favour the refactor arm",
       "records": records}
restore()
sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
sess.apply(reqs[:N], cache_name=cache)
out["session_state_bytes"], out["capacity"] = sess.keys.nbytes, sess.capacity
out["paths"] = {k: cf.LAST_PATHS.get(k, 0) for k in ("session_steps", "session_preserved_rows", "forward_trie", "forward_hf_fallback")}
out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "session_vs_refactor.json"), "w"), indent=1)

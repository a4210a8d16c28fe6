"""What a release across a fold costs (profiles/session_refold.json).  The set-up of scripts/session_fold_cost.py: synthetic SD-v1.4
encoder, layers 7-10, one MI355X, one process, every arm warmed up once, seven device-synchronised repetitions, arms alternated,
the state put back outside the window, wall ms as median [min, max].  No threshold.
 1. EditSession(keep_folded=True).release of archived rows, the flag read included:
      (a) 10 of 1 800 archived rows at M = 0        (b) the same at M = 800 live rows        (c) 1 000 of 1 800 at M = 0
    each beside fold() at the same live M — the one refactorization the session already pays; the launches of the parent's fold, Q
    written to the archive's tail instead of a scratch buffer; at M = 0 a fold is a no-op, so (a) and (c) stand beside the fold of
    one step's 100 rows — and beside the cold factor_cov + cov_inverse of the same four layers, the floor.
 2. the downdate kernel alone (hip.session_refold_update at M = 0, one layer, HIP events over 20 back-to-back launches) at n_rel =
    10, 100, 1 000 against the route it replaces on the same buffers: gather the rows, one lower-only fp64 GEMM with alpha = -1,
    copy base to the M region (torch's index_select and copy_ stand in for the two element-wise kernels; the copy moves the whole
    square where the fold's copy moves the lower tiles).
python scripts/session_refold_cost.py  [OUT=dir, default profiles/]"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import torch
import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter

DEV, REPS, LAYERS, N = "cuda:0", 7, (7, 8, 9, 10), 100
LAM, EW = 4000.0, 0.5
FOLDED, LIVE = 1800, 800
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=int(LAM), edit_weight=EW)
names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
tmp = tempfile.mkdtemp()
stats, cache = tmp + "/stats", tmp + "/cache/"
syn.write_stats_cache(stats, names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
reqs = syn.make_requests(FOLDED + LIVE, names="syllable", name_seed=3)
syn.write_vstar_cache(cache, reqs, hidden, seed=1, scale=0.5)
pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)
te, tok = pipe.text_encoder, pipe.tokenizer
covs = {l: em.get_cov_text_encoder(te, tok, hp_d["rewrite_module_tmp"].format(l), hp_d["mom2_dataset"], hp_d["mom2_n_samples"],
                                   hp_d["mom2_dtype"], stat_dir=stats, verbose=False).to(DEV).float().contiguous() for l in LAYERS}


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


class Snapshot:
    """everything a release or a fold of the session changes, to put back outside the timed window (neither writes Yp or a weight)"""

    def __init__(self, s):
        self.s = s
        self.buf, self.base = s.private_factors.buf.clone(), s._base.clone()
        self.rows = s._archived
        self.archive = [a[:self.rows].clone() for a in s._archive]
        self.host = (s.keys.M, list(s._ledger), list(s._archive_ledger), s._archived, s.folded, s.folds, s.released, s.retained)

    def restore(self):
        s = self.s
        s.private_factors.buf.copy_(self.buf)
        s._base.copy_(self.base)
        for a, b in zip(s._archive, self.archive):
            a[:self.rows].copy_(b)
        s.keys.M, s._ledger, s._archive_ledger, s._archived, s.folded, s.folds, s.released, s.retained = \
            self.host[0], list(self.host[1]), list(self.host[2]), *self.host[3:]
        s.private_factors.have_inverse = set(range(len(LAYERS)))


cold_ws = hip.CovFactors(len(LAYERS), inter, DEV)


def cold_factor():
    cold_ws.info.zero_()
    hip.factor_cov([covs[l] for l in LAYERS], LAM, EW, cold_ws, inverse=True)
    assert int(cold_ws.info.item()) == 0


def arms(sess, gone, fold_M):
    """release of ``gone`` against fold() and the cold factorization, alternated; the session as it was afterwards"""
    snap = Snapshot(sess)
    M = sess.preserved

    def release():
        assert sess.release(gone) == len(gone) and sess.preserved == 0
        snap.restore()

    def fold():
        assert sess.preserved == fold_M
        sess.fold()
        snap.restore()

    def one(arm):
        if arm == "release":
            ms = timed(lambda: sess.release(gone))
        elif arm == "fold":
            ms = timed(sess.fold)
        else:
            return timed(cold_factor)
        snap.restore()
        return ms

    release(), cold_factor()
    if fold_M == M:
        fold()
    out = {"release": [], "fold": [], "cold": []}
    order = ["release", "fold", "cold"] if fold_M == M else ["release", "cold"]
    for i in range(REPS):
        for arm in (order if i % 2 == 0 else order[::-1]):
            out[arm].append(one(arm))
    return {k: spread(v) for k, v in out.items() if v}


sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, keep_folded=True)
for lo in range(0, FOLDED, N):
    sess.apply(reqs[lo:lo + N], cache_name=cache)
sess.fold()
assert sess.folded == FOLDED and sess.preserved == 0
src = [r["source"] for r in reqs]
ten = src[5:FOLDED:180]
thousand = src[0:FOLDED:2][:900] + src[1:200:2]
assert len(ten) == 10 and len(set(thousand)) == 1000
records = {}
records["a_10_of_1800_M0"] = arms(sess, ten, -1)
print(json.dumps({"a": {k: v["median"] for k, v in records["a_10_of_1800_M0"].items()}}), flush=True)
records["c_1000_of_1800_M0"] = arms(sess, thousand, -1)
print(json.dumps({"c": {k: v["median"] for k, v in records["c_1000_of_1800_M0"].items()}}), flush=True)
# the fold beside the M = 0 arms: one step's rows
sess.apply(reqs[FOLDED:FOLDED + N], cache_name=cache)
snap = Snapshot(sess)
f100 = []
for i in range(REPS + 1):
    ms = timed(sess.fold)
    snap.restore()
    if i:
        f100.append(ms)
records["fold_M100"] = spread(f100)
print(json.dumps({"fold_M100": statistics.median(f100)}), flush=True)
for lo in range(FOLDED + N, FOLDED + LIVE, N):
    sess.apply(reqs[lo:lo + N], cache_name=cache)
assert sess.preserved == LIVE
records["b_10_of_1800_M800"] = arms(sess, ten, LIVE)
print(json.dumps({"b": {k: v["median"] for k, v in records["b_10_of_1800_M800"].items()}}), flush=True)

# ---- 2. the downdate kernel alone against gather + GEMM(alpha = -1) + copy ----------------------------------------------------------
fac, base, archive = sess.private_factors, sess._base, sess._archive[0]
dp, INNER = fac.dp, 20
sess.keys.M = 0
Mb = fac.buf[:dp * dp].view(dp, dp)


def events(fn):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(INNER):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / INNER


kernel = {}
for n_rel in (10, 100, 1000):
    idx = torch.arange(0, FOLDED, FOLDED // n_rel, device=DEV)[:n_rel]
    idx32 = idx.to(torch.int32)

    def fused():
        hip.session_refold_update(fac, sess.keys, 0, archive, FOLDED, idx32, base)

    def three():
        G = archive.index_select(0, idx)
        hip.dgemm_ex(1, 1, G, G, base[0], alpha=-1.0, beta=1.0, flags=16)
        Mb.copy_(base[0])

    k, t = [], []
    for i in range(REPS):
        for arm in (("k", "t") if i % 2 == 0 else ("t", "k")):
            (k if arm == "k" else t).append(events(fused if arm == "k" else three))
    kernel[str(n_rel)] = {"fold_downdate_kernel_ms": spread(k), "gather_gemm_copy_ms": spread(t)}
    print(json.dumps({"n_rel": n_rel, "kernel_ms": statistics.median(k), "gather_gemm_copy_ms": statistics.median(t)}), flush=True)

out = {"what": "EditSession(keep_folded=True).release across a fold: (1) the release (all four layers, the flag read included) of 10 / "
               "1 000 of 1 800 archived rows at M = 0 and of 10 at M = 800 live rows, beside fold() at the same live M (M = 0: beside "
               "the fold of one step's 100 rows) and the cold factor_cov + cov_inverse of the same layers; (2) the downdate kernel "
               "alone, one layer, per launch by HIP events over 20 launches, against index_select + lower-only GEMM(alpha = -1) + a "
               "copy of the whole square; synthetic SD-v1.4 encoder, layers 7-10, wall ms, device-synchronised, arms alternated in "
               "one process",
       "device": torch.cuda.get_device_name(0), "reps": REPS, "d": inter, "capacity": int(0.6 * inter), "release": records,
       "kernel_alone": kernel,
       "archive_bytes_per_layer": FOLDED * dp * 8,
       "paths": {k: cf.LAST_PATHS.get(k, 0) for k in ("session_steps", "session_folds", "session_folded_rows", "session_released_rows",
                                                      "forward_trie", "forward_hf_fallback")}}
out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "session_refold.json"), "w"), indent=1)

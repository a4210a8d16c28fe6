"""What saving and resuming a session costs: EditSession.save and EditSession.load at M preserved rows — file size, wall ms — against
the only alternative there was, rebuilding the same rows by ``retain`` in a fresh session (which needs the requests; a load does
not).  The set-up of scripts/session_retain_cost.py: synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per concept, one process, a
warm-up of every arm, device-synchronised repetitions, the arms alternated; median [min, max] wall ms per call
(profiles/session_persist.json).  Unfolded sessions of M = 100 / 1 000 / 1 800 rows; sessions that folded 1 000 rows once and hold
100 live ones, with and without ``keep_folded``.

``read`` is ``torch.load`` of the file alone (page cache warm: the file was just written), so ``load - read`` is what a load costs
once file I/O is excluded: fingerprints, the factor cache hit (a folded session: the batched refactorization of ``base``), the
uploads.  The rows are retained, so no weight moves and every load runs with ``weights="check"`` on the same pipe.
python scripts/session_persist_cost.py  [OUT=dir, default profiles/]"""
import json, os, statistics, sys, tempfile, time
sys.path.insert(0, os.getcwd())
import torch
import emcid_amd
from emcid_amd import clip_forward as cf, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams

DEV, REPS, LAYERS = "cuda:0", 5, (7, 8, 9, 10)
LAM, EW = 4000.0, 0.5
CASES = (("unfolded", 100, 0, False), ("unfolded", 1000, 0, False), ("unfolded", 1800, 0, False),
         ("folded once", 100, 1000, False), ("folded once, keep_folded", 100, 1000, True))      # (what, live rows, folded rows, keep_folded)
hidden, inter = syn.ENCODER_DIMS["sd-v1.4"][:2]
hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=int(LAM), edit_weight=EW)
names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
tmp = tempfile.mkdtemp()
stats = tmp + "/stats"
syn.write_stats_cache(stats, names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
reqs = syn.make_requests(1800, names="syllable", name_seed=3)
held = [{"source": r["source"], "prompts": list(r["prompts"])} for r in reqs]
pipe = syn.build_pipe("sd-v1.4", DEV, syllables=True)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "all": ms}


def build(M, folded, keep):
    """the rows by retain lists in a fresh session: what a process without the file has to do"""
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, keep_folded=keep)
    if folded:
        sess.retain(held[:folded])
        sess.fold()
    sess.retain(held[folded:folded + M])
    assert (sess.preserved, sess.folded) == (M, folded)
    return sess


ARMS = ("save", "read", "load", "replay")
records = []
for what, M, folded, keep in CASES:
    path = os.path.join(tmp, "session.pt")
    sess = build(M, folded, keep)

    def call(arm):
        if arm == "save":
            ms, out = timed(lambda: sess.save(path))
            return ms, out["bytes"]
        if arm == "read":
            return timed(lambda: em._read_session_file(path))[0], None
        if arm == "load":
            ms, got = timed(lambda: emcid_amd.EditSession.load(pipe, EMCIDHyperParams(**hp_d), path, DEV, stats_dir=stats))
            assert (got.preserved, got.folded, got.rows()) == (sess.preserved, sess.folded, sess.rows())
            return ms, None
        ms, got = timed(lambda: build(M, folded, keep))
        return ms, None

    nbytes = None
    for arm in ARMS:                          # warm-up of every arm at this shape; the save first, the others need its file
        nbytes = call(arm)[1] or nbytes
    runs = {a: [] for a in ARMS}
    for i in range(REPS):
        for arm in (ARMS if i % 2 == 0 else ("save",) + ARMS[:0:-1]):
            runs[arm].append(call(arm)[0])
    med = {a: statistics.median(v) for a, v in runs.items()}
    rec = {"what": what, "M": M, "folded": folded, "keep_folded": keep, "file_bytes": nbytes,
           **{a + "_ms": spread(v) for a, v in runs.items()}, "load_minus_read_ms": med["load"] - med["read"]}
    records.append(rec)
    print(json.dumps({"what": what, "M": M, "folded": folded, "MB": round(nbytes / 2 ** 20, 1),
                      **{a: round(v, 2) for a, v in med.items()}, "load-read": round(med["load"] - med["read"], 2)}), flush=True)
    del sess
    os.remove(path)

out = {"what": "EditSession.save / EditSession.load at M live (+ folded) rows against rebuilding the same rows by retain lists in a "
               "fresh session; synthetic SD-v1.4 encoder, layers 7-10, 3 prompts per concept; wall ms per call, device-synchronised, "
               "arms alternated in one process after a warm-up of each; read = torch.load of the file alone (page cache warm)",
       "device": torch.cuda.get_device_name(0), "reps": REPS, "capacity": int(0.6 * inter), "records": records,
       "paths": {k: cf.LAST_PATHS.get(k, 0) for k in ("forward_trie", "forward_hf_fallback", "session_loaded_rows")}}
out_dir = os.environ.get("OUT", "profiles")
os.makedirs(out_dir, exist_ok=True)
json.dump(out, open(os.path.join(out_dir, "session_persist.json"), "w"), indent=1)

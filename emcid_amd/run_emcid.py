"""Instruction-file driver of the mass-edit path (counterpart of the reference's scripts/run_emcid.py:27-134).

Same instruction JSON (reference: test_examples/*.json) — ``requests``, ``hparams`` (name of ``{hparams_dir}/{name}.json``),
``model_ckpt`` ("sd-v1.4" | "sdxl-1.0"), ``mom2_weight``, ``edit_weight``, optional ``mom2_weight_2``, optional ``sweep`` (sd-v1.4:
a list of [mom2_weight, edit_weight] pairs run over the requests in one ``sweep_emcid_text_encoder`` call; sdxl-1.0: a list of
[mom2_weight, mom2_weight_2, edit_weight] triples run over the pair in one ``sweep_emcid_sdxl_text_encoders`` call), optional
``holdout_prompts`` (a list of prompt strings; the edit is scored on them by ``emcid_main.EditScorer`` — sdxl-1.0: by
``emcid_main.PairEditScorer`` — and the summary — median and largest ``left`` over the concepts, largest and median ``drift_max``
over the prompts; for the pair also each encoder's median ``left`` and the largest pooled drift — is printed, with a ``sweep`` one
line per pair or triple); ``val_prompts``,
``out_dir`` and ``sample_num`` are read and ignored: the reference generates pre/post images with the diffusion pipeline
around the edit, this driver runs the edit only, reports its wall clock like experiments/emcid_test.py:1171-1180 and
writes the edited fc2 matrices to a safetensors file.

The pipeline: ``--pipe diffusers`` loads Stable Diffusion like the reference (needs the ``diffusers`` package and the
checkpoints); ``--pipe synthetic`` builds the random-init encoders of the same dimensions with the in-memory tokenizer
(emcid_amd/synthetic.py) — the configuration the parity fixtures and the benchmark use, v* and statistics caches
included when ``--synthetic_caches`` is given.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path
from typing import Optional

import torch

from .emcid_hparams import EMCIDHyperParams, EMCIDXLHyperParams
from .globals import HPARAMS_DIR, STATS_DIR, XL_STATS_DIR1, XL_STATS_DIR2


def set_weights(hparams, mom2_weight, edit_weight):
    """reference: experiments/emcid_test.py:924-930"""
    hparams.mom2_update_weight = hparams.mom2_update_weight if mom2_weight is None else mom2_weight
    hparams.edit_weight = hparams.edit_weight if edit_weight is None else edit_weight
    return hparams


def load_instruction(path, hparams_dir=HPARAMS_DIR):
    """(instructions dict, hparams object, cache_name) exactly as the reference derives them (:39-63)."""
    with open(path, "r") as f:
        ins = json.load(f)
    ckpt = ins["model_ckpt"]
    if ckpt == "sd-v1.4":
        cls = EMCIDHyperParams
    elif ckpt == "sdxl-1.0":
        cls = EMCIDXLHyperParams
    else:
        raise ValueError("Invalid model_ckpt")
    if "sweep" in ins:
        from .edit_engine import validate_grid, validate_pair_grid
        # sd-v1.4: [mom2_weight, edit_weight] pairs; sdxl-1.0: [mom2_weight, mom2_weight_2, edit_weight] triples
        ins["sweep"] = validate_grid(ins["sweep"]) if ckpt == "sd-v1.4" else validate_pair_grid(ins["sweep"])
    hparams = set_weights(cls.from_json(Path(hparams_dir) / f"{ins['hparams']}.json"), ins["mom2_weight"], ins["edit_weight"])
    return ins, hparams, f"cache/{ins['hparams']}/"


def sweep_report(point, pipe, hparams, originals):
    """What ``run`` keeps of a sweep point: the pair and, per edited layer, max|dW| and the Frobenius norm of dW."""
    from .nethook import get_parameter
    rec = {"mom2_weight": point[0], "edit_weight": point[1], "layers": {}}
    for name, w0 in originals.items():
        dw = get_parameter(pipe.text_encoder, name).detach() - w0
        rec["layers"][name] = {"dw_maxabs": float(dw.abs().max()), "dw_fro": float(dw.norm())}
    return rec


def build_pipe(kind: str, model_ckpt: str, device: str):
    if kind == "diffusers":
        try:
            from diffusers import StableDiffusionPipeline, StableDiffusionXLPipeline
        except ImportError as e:
            raise SystemExit(f"--pipe diffusers needs the diffusers package ({e}); use --pipe synthetic") from e
        if model_ckpt == "sd-v1.4":
            return StableDiffusionPipeline.from_pretrained("CompVis/stable-diffusion-v1-4", torch_dtype=torch.float32,
                                                           safety_checker=None, requires_safety_checker=False).to(device)
        return StableDiffusionXLPipeline.from_pretrained("stabilityai/stable-diffusion-xl-base-1.0", torch_dtype=torch.float32,
                                                         use_safetensors=True, variant="fp16").to(device)
    from . import synthetic as syn
    return syn.build_pipe("sd-v1.4", device, sdxl=(model_ckpt == "sdxl-1.0"))


def run(instruction_path, device="cuda:0", pipe=None, pipe_kind="synthetic", hparams_dir=HPARAMS_DIR, cache_name: Optional[str] = None,
        stats_dir=None, stats_dir_2=None, out: Optional[str] = None, verbose=True):
    """Apply the instruction's edit; returns (pipe, hparams, seconds).  For sdxl-1.0 a ``sweep`` list holds triples, and with
    ``holdout_prompts`` the score summary of every triple is printed, one JSON line each.  An instruction with a ``sweep`` list
    runs every pair or triple of it over the requests instead (the encoder is left unedited): per point the report of ``sweep_report``, printed and — ``out`` —
    written as JSON; returns (pipe, hparams, seconds, reports)."""
    from . import emcid_main as em
    ins, hparams, default_cache = load_instruction(instruction_path, hparams_dir)
    cache_name = default_cache if cache_name is None else cache_name
    pipe = build_pipe(pipe_kind, ins["model_ckpt"], device) if pipe is None else pipe
    if device.startswith("cuda"):
        torch.cuda.synchronize()
    t0 = time.time()
    holdout = ins.get("holdout_prompts")
    if ins.get("sweep") and ins["model_ckpt"] == "sdxl-1.0":
        kw = dict(cache_name=cache_name, stat_dir=XL_STATS_DIR1 if stats_dir is None else stats_dir,
                  stat_dir_2=XL_STATS_DIR2 if stats_dir_2 is None else stats_dir_2, verbose=verbose)
        head = [dict(mom2_weight=t[0], mom2_weight_2=t[1], edit_weight=t[2]) for t in ins["sweep"]]
        if holdout:     # the factorised path: one PairEditScore per triple, no weight leaves the device
            scores = em.sweep_emcid_sdxl_text_encoders(pipe, ins["requests"], hparams, ins["sweep"], device, score=list(holdout), **kw)
            reports = [dict(h, score=s.summary()) for h, s in zip(head, scores)]
        else:           # per triple and encoder the figures of ``sweep_report``
            from .nethook import get_parameter
            encoders = (("layers", pipe.text_encoder, hparams.layers), ("layers_2", pipe.text_encoder_2, hparams.layers_2))
            w0 = {key: {n: get_parameter(te, n).detach().clone() for n in (f"{hparams.rewrite_module_tmp.format(l)}.weight" for l in ls)}
                  for key, te, ls in encoders}

            def report(triple, p):
                rec = {}
                for key, te, _ in encoders:
                    dws = {n: get_parameter(te, n).detach() - w for n, w in w0[key].items()}
                    rec[key] = {n: {"dw_maxabs": float(dw.abs().max()), "dw_fro": float(dw.norm())} for n, dw in dws.items()}
                return rec

            recs = em.sweep_emcid_sdxl_text_encoders(pipe, ins["requests"], hparams, ins["sweep"], device, visit=report, **kw)
            reports = [dict(h, **rec) for h, rec in zip(head, recs)]
        if device.startswith("cuda"):
            torch.cuda.synchronize()
        dt = time.time() - t0
        if verbose:
            print(f"sweep of {len(reports)} triples takes {dt} seconds ({1e3 * dt / len(reports):.1f} ms per triple).")
        if verbose or holdout:
            for rec in reports:
                print(json.dumps(rec))
        if out:
            Path(out).write_text(json.dumps(reports, indent=1))
        return pipe, hparams, dt, reports
    if ins.get("sweep"):
        from .nethook import get_parameter
        names = [f"{hparams.rewrite_module_tmp.format(l)}.weight" for l in hparams.layers]
        originals = {n: get_parameter(pipe.text_encoder, n).detach().clone() for n in names}
        reports = em.sweep_emcid_text_encoder(pipe, ins["requests"], hparams, ins["sweep"], device,
                                              visit=lambda point, p: sweep_report(point, p, hparams, originals),
                                              cache_name=cache_name, stat_dir=STATS_DIR if stats_dir is None else stats_dir,
                                              verbose=verbose, score=list(holdout) if holdout else None)
        if holdout:     # (report, EditScore) per point: the score's summary joins the point's record
            reports = [dict(rec, score=s.summary()) for rec, s in reports]
        if device.startswith("cuda"):
            torch.cuda.synchronize()
        dt = time.time() - t0
        if verbose:
            print(f"sweep of {len(reports)} points takes {dt} seconds ({1e3 * dt / len(reports):.1f} ms per point).")
            for rec in reports:
                print(json.dumps(rec))
        if out:
            Path(out).write_text(json.dumps(reports, indent=1))
        return pipe, hparams, dt, reports
    if ins["model_ckpt"] == "sd-v1.4":
        # (the scorer is built on the weights of BEFORE the edit; its construction is inside the reported wall clock)
        scorer = em.EditScorer(pipe, ins["requests"], hparams, device, holdout=list(holdout), cache_name=cache_name) if holdout else None
        em.apply_emcid_to_text_encoder(pipe, ins["requests"], hparams, device, cache_name=cache_name,
                                       stats_dir=STATS_DIR if stats_dir is None else stats_dir, verbose=verbose)
        if scorer is not None:
            print(f"edit score over {len(holdout)} holdout prompts: {json.dumps(scorer.score().summary())}")
    else:
        scorer = em.PairEditScorer(pipe, ins["requests"], hparams, device, holdout=list(holdout), cache_name=cache_name) if holdout else None
        em.apply_emcid_to_sdxl_text_encoders(pipe, ins["requests"], hparams, device, mom2_weight=ins["mom2_weight"],
                                             mom2_weight_2=ins.get("mom2_weight_2", None), edit_weight=ins["edit_weight"],
                                             cache_name=cache_name, stat_dir=XL_STATS_DIR1 if stats_dir is None else stats_dir,
                                             stat_dir_2=XL_STATS_DIR2 if stats_dir_2 is None else stats_dir_2, verbose=verbose)
        if scorer is not None:
            print(f"edit score over {len(holdout)} holdout prompts: {json.dumps(scorer.score().summary())}")
    if device.startswith("cuda"):
        torch.cuda.synchronize()
    dt = time.time() - t0
    if verbose:
        print(f"apply_emcid takes {dt} seconds ({len(ins['requests']) / dt:.1f} concept-edits/s).")
    if out:
        em.export_edited_weights(pipe.text_encoder, hparams, out)
        if ins["model_ckpt"] == "sdxl-1.0":
            p = Path(out)
            em.export_edited_weights(pipe.text_encoder_2, hparams, p.with_name(p.stem + "_2" + p.suffix), layers=hparams.layers_2)
    return pipe, hparams, dt


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--instruction_path", type=str, required=True)
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--pipe", choices=["synthetic", "diffusers"], default="synthetic")
    ap.add_argument("--hparams_dir", default=str(HPARAMS_DIR))
    ap.add_argument("--cache_name", default=None, help="v* cache prefix (default cache/{hparams}/ like the reference)")
    ap.add_argument("--stats_dir", default=None)
    ap.add_argument("--stats_dir_2", default=None)
    ap.add_argument("--out", default=None, help="write the edited fc2 weights here (safetensors)")
    ap.add_argument("--synthetic_caches", action="store_true",
                    help="with --pipe synthetic: write synthetic v* / statistics caches for the instruction first")
    a = ap.parse_args(argv)
    os.environ.setdefault("EMCID_MANAGE_THREADS", "1")      # this process exists to edit: thread pools sized to the CPU quota
    if a.synthetic_caches:
        if a.pipe != "synthetic":
            raise SystemExit("--synthetic_caches only makes sense with --pipe synthetic")
        from . import synthetic as syn
        ins, hp, default_cache = load_instruction(a.instruction_path, a.hparams_dir)
        cache = default_cache if a.cache_name is None else a.cache_name
        sdxl = ins["model_ckpt"] == "sdxl-1.0"
        syn.write_vstar_cache(cache, ins["requests"], 768, seed=1, scale=0.5)
        s1 = a.stats_dir or str(XL_STATS_DIR1 if sdxl else STATS_DIR)
        syn.write_stats_cache(s1, [hp.rewrite_module_tmp.format(l) for l in hp.layers], 3072, hp.mom2_n_samples, seed=2, t=6144)
        if sdxl:
            syn.write_vstar_cache(cache, ins["requests"], 1280, seed=5, scale=0.5, suffix="_2")
            syn.write_stats_cache(a.stats_dir_2 or str(XL_STATS_DIR2), [hp.rewrite_module_tmp.format(l) for l in hp.layers_2],
                                  5120, hp.mom2_n_samples, seed=7, t=10240)
    run(a.instruction_path, a.device, None, a.pipe, a.hparams_dir, a.cache_name, a.stats_dir, a.stats_dir_2, a.out)
    print("Done")


if __name__ == "__main__":
    main(sys.argv[1:])

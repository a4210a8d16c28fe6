#!/usr/bin/env python3
"""bench.py — concept-edits/sec of the closed-form mass-edit path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N --steps K --warmup W]     (N > 1 without a launcher: re-launches itself under
                                                         torch.distributed.run before anything touches a GPU)
                    [--dump-outputs DIR] [--full]

A plain run sets up, makes the first call, warms up, times the K steps and prints the line.  `--dump-outputs DIR` writes what the
last timed step computed (the four edited fc2 weights, float32 .npy; the inputs are seeded, so two builds compare output for
output).  `--full` adds the other records described below: the replay / new-weight calls, the GEMM A/B, the host/device split, the roofline
pass, the secondary records, the CPU baseline and Stage 0 (the --no-* switches leave parts of it out); with N > 1 also
`per_rank` and `weak_replicas`.

Workload (config.workload): the 1 000-concept batch on SD-v1.4 dims the metric is quoted on — CLIP ViT-L/14 text
encoder (768 / 3072 / 12 layers, random init), layers [7, 8, 9, 10], lambda = 4000, edit_weight 0.5, 3 prompts per
concept, synthetic v* npz files and synthetic second-moment npz files on disk (no network for real weights/captions).

A STEP is ONE CALL of the drop-in entry point, timed from outside exactly like the reference's own timer
(experiments/emcid_test.py:1172-1179):

    apply_emcid_to_text_encoder(pipe, requests, hparams, device, cache_name=..., stats_dir=...)

with the model resident in HBM, the v* files on disk and C_l in the covariance cache ("all v* and C
pre-cached").  EVERY warm-up and timed step edits a request set the process has NOT seen before (1 000 other names, its
own v* directory of 1 000 npz files; up to 32 sets, cycled beyond that) — the reference's harness never repeats a call
either (experiments/emcid_test.py:1168-1179 shuffles, :924-930 sweeps the weights).  Reported beside it:
`replay_ms_per_call` (the same 1 000 requests again and again), `new_lambda_ms_per_call` / `new_edit_weight_ms_per_call`
(same requests, a mom2_update_weight / edit_weight never used before), `cold_process` (a CHILD process making one call:
what the reference's one-call CLI user gets), and the records `n100` (BASELINE config 2) and `sdxl` (config 4).  Inside the call: tokenizer, subject search, prefix trie, v* reads (host), then one partial
prefix-deduplicated encoder forward that runs gather -> assemble -> Cholesky -> TRSM -> dW on the HIP kernels at each
edited layer's fc2 (device), then the not-SPD flag read (one sync).  Before every call the four fc2 weights are put
back to their original values (four device copies, inside the timed region), so every step performs the same edit.
`value` = concepts * K / wall.  The FIRST call of the process (statistics npz -> HBM, cold v* reads, Cholesky of the
four lam*C' and their inverse factors, GEMM selection) is timed separately as `first_call_ms`; warm calls reuse what
is a pure function of (statistics, lambda, edit_weight) — `config.caches` says what was warm.

Secondary fields: `device_ms_per_step` (run_encoder_edit on an HBM-resident plan: what round 1 reported as the step),
`host_prepare_ms` (prepare_text_encoder_edit alone, median), `forward_gemm` (the call with the other GEMM path: A/B).

`roofline`: the same K device steps once more with every kernel class of the solve bracketed by HIP events on the
launch stream (emcid_profile_*); `kernel_classes` lists every class with its ALGORITHMIC flops (SURVEY.md §8d counts),
`solve` aggregates all fp64 classes, and the headline object is the class with the most time.
`cpu_baseline`: the oracle (op-for-op CPU port of the reference path) on the host cores, 100-concept sample of the same
workload, median of up to 3 runs, host/compute split; the same run yields `dw_max_abs_err`.
`stage0`: BASELINE config 5 on this GPU (100 000 synthetic captions, 12 layers, one pass) — tokens/s and the Gram
kernel's fraction of the fp32 MFMA peak.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

F64_MFMA_PEAK_TFLOPS = 78.6   # MI355X fp64 matrix peak [external: AMD MI355X datasheet; MI355X_MICROARCH.md lists no fp64 row]
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md
F16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: BF16 / F16 MFMA, dense
LAYERS = (7, 8, 9, 10)
LAM, EW = 4000, 0.5
KIND = "sd-v1.4"


MAX_REQUEST_SETS = 32
_T0 = time.perf_counter()


def log(msg):
    """Progress line on stderr (the JSON line on stdout stays alone): a long silent run looks hung to the GPU box's watchdog."""
    print(f"[bench {time.perf_counter() - _T0:7.1f} s] {msg}", file=sys.stderr, flush=True)


def request_set(n_concepts, workdir, index=0, write=True):
    """Request set `index` of the workload: n_concepts 3-syllable names drawn with their own seed (set 0 = the names of the
    reference-minted N = 1000 golden) and the directory holding their v* npz files."""
    from emcid_amd import synthetic as syn

    reqs = syn.make_requests(n_concepts, names="syllable", name_seed=3 + 101 * index)   # 3-token names, 7-token prompts like real CLIP BPE
    cache = str(Path(workdir) / (f"cache_{n_concepts}" if index == 0 else f"cache_{n_concepts}_set{index}")) + "/"
    done = Path(cache) / ".complete"
    if write and not done.exists():
        syn.write_vstar_cache(cache, reqs, syn.ENCODER_DIMS[KIND][0], seed=1 + index, scale=0.5)
        done.touch()
    return reqs, cache


def write_inputs(n_concepts, workdir):
    """Request set 0 with its v* files and the statistics files of the edited layers (written once per workdir).
    Returns (requests, cache, hparams dict, stats dir, layer names)."""
    from emcid_amd import synthetic as syn

    inter = syn.ENCODER_DIMS[KIND][1]
    hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=LAM, edit_weight=EW)
    reqs, cache = request_set(n_concepts, workdir, 0)
    stats = Path(workdir) / "stats"
    layer_names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
    if not (stats / ".complete").exists():
        syn.write_stats_cache(stats, layer_names, inter, hp_d["mom2_n_samples"], seed=2, t=2 * inter)
        (stats / ".complete").touch()
    return reqs, cache, hp_d, str(stats), layer_names


def build_inputs(n_concepts, device, workdir):
    from emcid_amd import synthetic as syn

    pipe = syn.build_pipe(KIND, device, syllables=True)
    reqs, cache, hp_d, stats, layer_names = write_inputs(n_concepts, workdir)
    return pipe, reqs, hp_d, cache, stats, layer_names


def dump_outputs(out_dir, pipe, layer_names):
    """What the caller of the timed path receives from its last step: the edited fc2 weights (the only parameters the call
    changes), one float32 .npy per weight (4 x 768 x 3072 x 4 B = 38 MB)."""
    import numpy as np
    import torch
    from emcid_amd.nethook import get_parameter

    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    for n in layer_names:
        w = get_parameter(pipe.text_encoder, n + ".weight").detach().to("cpu", torch.float32).numpy()
        np.save(out / f"{n}.weight.npy", w)


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start N ranks under torch.distributed.run as a CHILD process (never
    exec from a process that may touch the GPU) and exit with its code.  Nothing here has initialised HIP."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.call(cmd, env=env))


# ---- algorithmic flop counts (SYRK = n^2 k, Cholesky = n^3/3, triangular solve = rows * n^2 per direction,
# GEMM = 2 m n k) for the launches each solver makes, per class and STEP ---------------------------------------------------

def chol_flops(n):
    """Cholesky of one n x n matrix with the two-level schedule of csrc/spd_solve.hip (NB 128 inside OB 512)."""
    nbk, nob = n // 128, n // 512
    inner = sum(((n - (j + 1) * 128) * w - w * w // 2) * 128
                for j in range(nbk - 1) for w in [(j // 4 + 1) * 512 - (j + 1) * 128] if w > 0)
    trail = sum(((n - J * 512) * 512 - 512 * 512 // 2) * (J * 512) for J in range(1, nob))
    panel = sum((n - (j + 1) * 128) * 128 * 128 for j in range(nbk - 1))
    leaf = nbk * 2 * 128 ** 3 // 3                      # factor (128^3/3) + inverse of the triangular block (128^3/3)
    block_inv = nob * (512 ** 3 - 4 * 128 ** 3) // 3    # 512-block inverses from the 128-block inverses
    return {"chol_inner": inner, "chol_trail": trail, "chol_panel": panel, "chol_leaf": leaf, "inv_block": block_inv}


def trsm_flops(rows, n, directions=2):
    """Right-sided two-level TRSM of `rows` rows against an n x n factor."""
    nob = n // 512
    return {"trsm_update": directions * (2 * rows * 512 * sum(n - (J + 1) * 512 for J in range(nob))),
            "trsm_diag": directions * (rows * nob * 512 * 512)}


def step_flops(N, n_rows, d, h, L, dual, apply_only, factors_cached, first_x):
    f = {c: 0 for c in ("assemble", "chol_leaf", "chol_inner", "chol_trail", "chol_panel", "inv_block", "trsm_update",
                        "trsm_diag", "delta_w", "inv_apply", "inv_build")}

    def add(table, times=1):
        for c, v in table.items():
            f[c] += times * v

    Np = -(-N // 128) * 128
    if not dual:
        add(chol_flops(d), L)
        add(trsm_flops(n_rows, d, 2), L)
        f["assemble"] = L * N * d * d
        f["delta_w"] = L * 2 * h * n_rows * d
        return f
    if not factors_cached:      # this step factors lam*C' (d x d) for the L layers and builds X = inv(L) for those that use it
        add(chol_flops(d), L)
        f["inv_build"] = (L - first_x) * (d ** 3 // 3 - (d // 512) * 512 ** 3 // 3)
    n_x = L if factors_cached else L - first_x           # layers whose M-solves are GEMMs against X
    add(chol_flops(Np), L)                               # the N x N system S = I + Yt Yt^T
    f["assemble"] += L * N * N * d                       # SYRK count of S
    if apply_only:
        if Np <= 4096:
            # Z^T = (Rt^T XS^T) XS with XS = inv(LS) explicit: two triangular GEMMs on h rows + the halving level(s) above 512
            f["trsm_diag"] += L * 2 * h * Np * Np
            f["inv_build"] += L * (Np ** 3 // 3 - (Np // 512) * 512 ** 3 // 3)
        else:
            add(trsm_flops(h, Np, 2), L)                 # Z = S^-1 Rt by block substitution: h right-hand sides
        f["delta_w"] += L * 2 * h * N * d                # V = Z^T Yt
        shadow = (os.environ.get("EMCID_SHADOW_P", "1") != "0"
                  and 256 <= Np <= 2048)
        if shadow and os.environ.get("EMCID_SHADOW_P", "1") == "1":      # the library's own fit estimate (emcid_edit_dual_apply_stage2_f64)
            ntl, nb = -(-d // 128), Np // 128
            steps = -(-(ntl + 1) * 8 // nb)
            rounds = -(-(Np // 64) * ((ntl + 1) // 2) // 240)
            shadow = rounds * (9.0 + 1.5 * steps) <= 50.0
        if shadow:
            # P = Yt X rides in the Cholesky's leaf launches (csrc/spd_solve.hip ShadowJob); U = Z^T P is the delta_w GEMM
            f["inv_apply"] += n_x * n_rows * d * d       # Yt = Kt X^T on the concept rows
            f["chol_leaf"] += n_x * N * d * d            # P = Yt X: N x d x d against a triangle
        else:
            f["inv_apply"] += n_x * (n_rows + h) * d * d     # Yt = Kt X^T on the concept rows, U = V X on h rows
        add(trsm_flops(n_rows, d, 1), L - n_x)
        add(trsm_flops(h, d, 1), L - n_x)
    else:
        add(trsm_flops(d, Np, 2), L)                     # adj_k = (S^-1 Pt)^T: d right-hand sides
        f["delta_w"] += L * 2 * h * N * d
        f["inv_apply"] += n_x * 2 * n_rows * d * d
        add(trsm_flops(n_rows, d, 2), L - n_x)
    return f


KERNEL_OF_CLASS = {
    "assemble": "gemm_f64_streamk_kernel / gemm_f64_kernel launched as SYRK (S = I + Yt Yt^T, or K^T K in the direct solver)",
    "chol_leaf": "chol_step_leaf_kernel: workgroup 0 = 128 x 128 diagonal block (factor + inverse, matrix-pipe pivots), the others = "
                 "the previous step's trailing tiles and one K slice of the shadow product P = Yt X (64 x 128 tiles)",
    "chol_trail": "gemm_f64_kernel<KC,KC,*,*,16,EpiAxpby> launched as left-looking Cholesky block-column update",
    "chol_inner": "gemm_f64_kernel<KC,KC,*,64,16,2,2,EpiAxpby> launched as in-block Cholesky trailing update",
    "chol_panel": "gemm_f64_kernel<KC,KC,32,64,16,2,2,EpiAxpby> launched as Cholesky panel solve",
    "chol_fused": "chol_fused_kernel (whole N x N Cholesky + its block inverses in one cooperative launch)",
    "inv_block": "gemm_f64_kernel (batched) building the 512-block inverses from the leaf's 128-block inverses",
    "trsm_update": "gemm_f64_kernel<KC,*,*,*,16,EpiAxpby> launched as rank-512 TRSM update",
    "trsm_diag": "gemm_f64_kernel<KC,*,32,64,16,2,2,EpiAxpby> launched as TRSM diagonal-block multiply",
    "delta_w": "gemm_f64_kernel (V = Z^T Yt in the dual solver, dW = R^T X in the direct one)",
    "inv_apply": "GEMM against the explicit inverse factor (Yt = Kt X^T; triangular K range): gemm_f64_kernel<KC,KC,32,64,16,2,2> on "
                 "mirrored tile pairs where their count fills the chip evenly (N = 1000, d = 3072), else gemm_f64_streamk2_kernel "
                 "<KC,*,128,128,16,2,4>",
    "inv_build": "gemm_f64_kernel<KC,!KC,*,*,16,*> launched as recursive-halving build of X = inv(L)",
    "linear": "linear_f32_kernel (csrc/gemm_f32.hip): the forward's projections Y = act(X W^T + b) + residual on v_mfma_f32_32x32x2_f32, "
              "128 x 128 tiles on 4 waves or 160 x 128 on 8 waves (K split inside the workgroup) by the launch's fill of the chip",
    "linear_sp16": "linear_sp16_dma16_kernel (csrc/gemm_sp16.hip): the forward's projections Y = act(X W^T + b) + residual at fp32 accuracy on "
                   "v_mfma_f32_16x16x32_f16 — operands as hi + lo fp16 planes under per-row power-of-two scales, three MFMAs per k-step "
                   "(hi.hi + hi.lo + lo.hi), fp32 accumulate; operands staged by LDS-DMA (buffer_load ... lds, XOR-swizzled image), "
                   "epilogue through LDS (whole-row stores); four waves per workgroup, two workgroups per compute unit; by the launch's "
                   "shape 128 x 128 tiles (q|k|v, fc1 at ~6 300 rows), 80 x 128 (out, fc2), 64 x 64 or 160 x 128; launches of less than one "
                   "tile per compute unit on the register-staged 64 x 64 kernel (linear_sp16_kernel, v_mfma_f32_32x32x16_f16)",
}
FP64_CLASSES = ["assemble", "chol_leaf", "chol_panel", "chol_trail", "chol_inner", "chol_fused", "inv_block", "trsm_diag",
                "trsm_update", "delta_w", "inv_build", "inv_apply"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--concepts", type=int, default=1000)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (the edited fc2 weights) as DIR/<name>.npy, float32")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: replay / new-weight calls, GEMM A/B, host/device split, roofline, "
                         "the secondary records, the CPU baseline, Stage 0 (the --no-* switches below act inside it)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-stage0", action="store_true")
    ap.add_argument("--gc-freeze", action="store_true", help="gc.freeze() once the inputs exist (default: the collector as it is)")
    ap.add_argument("--no-variants", action="store_true", help="skip the n100 / sdxl / cold_process records")
    ap.add_argument("--no-cpu-full", action="store_true", help="skip the full 1 000-concept runs of the CPU baseline (~1 min each)")
    ap.add_argument("--cpu-full-runs", type=int, default=3, help="full-size runs of the CPU baseline (median reported)")
    ap.add_argument("--no-gemm-ab", action="store_true", help="skip the calls on the OTHER forward-GEMM path (keeps a profiler trace "
                                                              "of this run free of that path's kernels)")
    ap.add_argument("--cold-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--stage0-captions", type=int, default=100000)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.cold_child:
        return cold_child(args.cold_child, args.concepts)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world == 1 and "RANK" not in os.environ:
        self_launch(args)
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import torch
    import torch.distributed as dist
    from emcid_amd import clip_forward, emcid_main as em, hip, edit_engine
    from emcid_amd.edit_engine import ConceptShard, run_encoder_edit, check_info
    from emcid_amd.emcid_hparams import EMCIDHyperParams
    from emcid_amd.nethook import get_parameter

    backend = os.environ.get("EMCID_BENCH_BACKEND", "nccl")      # "gloo": functional test of this script on a 1-GPU box
    if backend == "gloo":
        local = 0                                                 # every rank shares cuda:0, collectives staged via host
    torch.cuda.set_device(local)
    device = f"cuda:{local}"
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(device))
        else:
            dist.init_process_group(backend)
        assert dist.get_backend() == backend and dist.get_world_size() == world
    shard = ConceptShard(rank, world, None)

    # the forward's projections run on the library's own GEMM (no selection step); under EMCID_OWN_GEMM=0 they are torch's
    # F.linear with library-default selection
    os.environ.setdefault("EMCID_MANAGE_THREADS", "1")      # an editing process of its own: thread pools sized to the CPU quota
    os.environ.setdefault("EMCID_FACTOR_CACHE", "8")        # the edit_weight sweep below must not evict the workload's own factors
    workdir = Path(tempfile.gettempdir()) / f"emcid_bench_{os.getuid()}"
    n_sets = min(MAX_REQUEST_SETS, 1 + args.warmup + args.steps)      # set 0: the first call; then one per warm-up / timed step
    if rank == 0:
        workdir.mkdir(exist_ok=True, mode=0o700)
        write_inputs(args.concepts, workdir)            # writes the synthetic v*/stats caches once
        for j in range(1, n_sets):
            request_set(args.concepts, workdir, j)
    if world > 1:
        dist.barrier()
    pipe, reqs, hp_d, cache, stats, layer_names = build_inputs(args.concepts, device, workdir)
    sets = [(reqs, cache)] + [request_set(args.concepts, workdir, j, write=False) for j in range(1, n_sets)]
    hp = EMCIDHyperParams(**hp_d)
    originals = {n: get_parameter(pipe.text_encoder, n + ".weight").detach().clone() for n in layer_names}

    def restore_weights():
        with torch.no_grad():
            for n in layer_names:
                get_parameter(pipe.text_encoder, n + ".weight").copy_(originals[n])

    def call(which=0, hparams=None, **kw):
        r, c = sets[which % len(sets)]
        restore_weights()
        em.apply_emcid_to_text_encoder(pipe, r, hparams or hp, device, cache_name=c, stats_dir=stats, verbose=False, shard=shard, **kw)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_calls(k, first_set=None, **kw):
        """k calls bracketed by barrier + synchronize; call i edits request set first_set + i (None: set 0 every time).
        Returns (total seconds, per-call seconds)."""
        per = []
        sync()
        t0 = time.perf_counter()
        for i in range(k):
            t1 = time.perf_counter()
            call(0 if first_set is None else first_set + i, **kw)
            per.append(time.perf_counter() - t1)
            call_marks.append((dict(edit_engine.TIMING), dict(clip_forward.LAST_PATHS)))      # two small dict copies: ~2 us
        sync()
        return time.perf_counter() - t0, per

    call_marks = []

    def cpu_throttle_counters():
        """the container's CPU-quota throttling counters (cgroup v2 cpu.stat, or v1), None where they cannot be read"""
        for f in ("/sys/fs/cgroup/cpu.stat", "/sys/fs/cgroup/cpu/cpu.stat", "/sys/fs/cgroup/cpu,cpuacct/cpu.stat"):
            try:
                kv = dict(ln.split()[:2] for ln in open(f).read().splitlines() if len(ln.split()) >= 2)
                out = {k: int(v) for k, v in kv.items() if k in ("nr_periods", "nr_throttled", "throttled_usec", "throttled_time", "usage_usec")}
                if out:
                    return out
            except Exception:
                continue
        return None

    def slowest_call(per, marks, first_set):
        """host phases and path counters of the slowest of a series of calls, as differences of the running totals"""
        i = max(range(len(per)), key=lambda j: per[j])
        (t_a, p_a), (t_b, p_b) = (marks[i - 1] if i > 0 else ({}, {})), marks[i]
        return {"index": i, "request_set": first_set + i, "ms": per[i] * 1e3,
                "host_phases_ms": {k: round((v - t_a.get(k, 0.0)) * 1e3, 3) for k, v in t_b.items()} if i > 0 else None,
                "path_counters": {k: v - p_a.get(k, 0) for k, v in p_b.items() if isinstance(v, (int, float)) and v != p_a.get(k, 0)} if i > 0 else None,
                "over_median": per[i] / statistics.median(per)}

    def each_synced(k, fn):
        """k single calls, each between two synchronisations: milliseconds per call."""
        out = []
        for i in range(k):
            sync()
            t1 = time.perf_counter()
            fn(i)
            sync()
            out.append((time.perf_counter() - t1) * 1e3)
        return out

    # ---- the interpreter's cyclic collector: every collection inside the timed region is recorded ------------------------------
    # (the process holds 26 000 request dicts and a model; a full collection would walk all of it.  Measured: two generation-0
    # collections, 0.4 ms, in the twenty timed steps, frozen or not — profiles/r05_outlier.txt; --gc-freeze is there to repeat that.)
    import gc
    gc.collect()
    if args.gc_freeze:
        gc.freeze()
    gc_events = []

    def _gc_cb(phase, info, _t=[0.0]):
        if phase == "start":
            _t[0] = time.perf_counter()
        else:
            gc_events.append((info.get("generation"), (time.perf_counter() - _t[0]) * 1e3))
    gc.callbacks.append(_gc_cb)
    # ---- the first call of the process: everything cold ------------------------------------------------------------------
    log(f"inputs ready ({len(sets)} request sets); first call")
    first_s, _ = timed_calls(1)
    log(f"first call {first_s * 1e3:.0f} ms; warm-up + {args.steps} timed steps")
    # ---- warm-up and the K timed steps: every call a request set this process has never seen ------------------------------
    for i in range(args.warmup):
        call(1 + i)
    edit_engine.TIMING.clear()
    call_marks.clear()
    gc_events.clear()
    thr0 = cpu_throttle_counters()
    elapsed, per_call = timed_calls(args.steps, first_set=1 + args.warmup)
    thr1 = cpu_throttle_counters()
    # did the container's CPU quota freeze the process inside the timed region?  (a frozen process shows as a call whose host
    # phases are ALL stretched, profiles/r05_quick_noisy_box.json)
    cpu_throttle = None if thr0 is None or thr1 is None else {k: thr1[k] - thr0.get(k, 0) for k in thr1}
    gc_in_timed = {"frozen": bool(args.gc_freeze), "collections": len(gc_events),
                   "by_generation_ms": {str(g): round(sum(ms for gg, ms in gc_events if gg == g), 3) for g in sorted({g for g, _ in gc_events})},
                   "longest_ms": round(max((ms for _, ms in gc_events), default=0.0), 3)}
    slowest = slowest_call(per_call, list(call_marks), 1 + args.warmup)
    host_phases = {k: round(v / args.steps * 1e3, 4) for k, v in edit_engine.TIMING.items()}      # host wall-clock per phase and call
    last_paths = dict(clip_forward.LAST_PATHS)       # the path counters and trie gauges as the timed steps left them
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, pipe, layer_names)      # before any other call touches the weights
    per_rank = None
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=device if backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        rank_elapsed, elapsed = elapsed, float(tmax.item())
    if world > 1 and args.full:
        # per-rank phase times (a few more calls OUTSIDE the timed region, with event brackets around the collectives and the
        # solves): what a scaling curve is read with
        try:
            per_rank = _per_rank_phases(edit_engine, dist, timed_calls, args, rank, world, device, shard, rank_elapsed, host_phases)
        except Exception as e:         # diagnostics must never cost the line
            edit_engine.DIST_TIMING["enabled"] = False
            per_rank = {"error": repr(e)}
    value = args.concepts * args.steps / elapsed
    # ---- companion record for N > 1: the SAME call as G independent replicas (every rank edits its own 1 000-concept request
    # sets on its own GPU, no collective on the data path — SURVEY.md §8e: what actually uses 8 GPUs when there are 8 lists to
    # edit), beside the strong-scaling number above (ONE list cut across the ranks, whose replicated N x N chain and per-layer
    # all-reduces do not divide) -------------------------------------------------------------------------------------------
    weak = None
    if world > 1 and args.full:
        try:
            solo = ConceptShard(0, 1, None)

            def replica_call(i):
                r, c = sets[(1 + args.warmup + rank * 5 + i) % len(sets)]
                restore_weights()
                em.apply_emcid_to_text_encoder(pipe, r, hp, device, cache_name=c, stats_dir=stats, verbose=False, shard=solo)

            for i in range(2):
                replica_call(i)
            sync()
            t0 = time.perf_counter()
            for i in range(args.steps):
                replica_call(2 + i)
            sync()
            wt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=device if backend == "nccl" else "cpu")
            dist.all_reduce(wt, op=dist.ReduceOp.MAX)
            weak = {"scaling": "weak", "value": world * args.concepts * args.steps / float(wt.item()), "unit": "concept-edits/s",
                    "ms_per_step": float(wt.item()) / args.steps * 1e3, "steps": args.steps,
                    "note": f"{world} replicas, one process per GPU, each editing its own {args.concepts}-concept request sets with no "
                            f"collective on the data path; barrier + synchronize on both sides, max over ranks"}
        except Exception as e:         # diagnostics must never cost the line
            weak = {"error": repr(e)}

    # ---- the headline line: what the timed steps themselves measured -------------------------------------------------------
    own_gemm = bool(clip_forward.OWN_GEMM)
    split_gemm = own_gemm and bool(clip_forward.SPLIT_GEMM)
    fresh_ms = statistics.median(per_call) * 1e3
    out = {
        "metric": "concept-edits/sec (1 000-concept batch, SD-v1.4)", "value": value, "unit": "concept-edits/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": ("f32 forward (2 x fp16 split MFMA, fp32 accumulate) + f64 solve" if split_gemm else "f32 forward + f64 solve"), "data": "synthetic",
        "config": {"workload": f"{args.concepts}-concept edit, SD-v1.4 text-encoder dims (768/3072/12L), layers 7-10, "
                               f"lambda 4000, 3 prompts/concept; one step = one apply_emcid_to_text_encoder call, timer "
                               f"around the call (v* npz on disk, C_l in the covariance cache, model in HBM); every step "
                               f"edits a request set the process has not seen before",
                   "concepts": args.concepts,
                   "request_sets": {"distinct": len(sets), "used_by_first_warmup_timed": 1 + args.warmup + args.steps,
                                    "note": "set i = 1 000 other syllable names + its own directory of 1 000 v* npz files; "
                                            "cycled when warmup + steps exceed the distinct sets"},
                   "forward": ("prefix-trie: %d unique rows of %d tokens (last timed step)"
                               % (last_paths["last_trie_rows"], last_paths["last_trie_tokens"]))
                   if "last_trie_rows" in last_paths else "hooked HF forward",
                   "caches": {"covariance_in_hbm": True,
                              "vstar_files": "read from the files in every call (native batch reader, no in-process copy)",
                              "gemm_selection": "none needed (own GEMM)" if own_gemm else "torch F.linear, library-default selection"},
                   "backend": (dist.get_backend() if world > 1 else None),
                   "world_size_seen": (dist.get_world_size() if world > 1 else 1),
                   "parallelism": f"concept-shard x{world}"},
        "ms_per_call_median": fresh_ms,
        "ms_per_call_min": min(per_call) * 1e3,
        "ms_per_call": [round(t * 1e3, 3) for t in per_call],
        "fresh_requests_ms": fresh_ms,                   # = the timed steps themselves
        "first_call_ms": first_s * 1e3,
        "host_phases_ms_per_call": host_phases, "slowest_call": slowest, "gc_in_timed_region": gc_in_timed, "cpu_throttle_in_timed_region": cpu_throttle,
        "outputs_dumped_to": args.dump_outputs,
        "full": bool(args.full),
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(out))
        if world > 1:
            dist.destroy_process_group()
        return

    # ---- the same 1 000 requests again and again (what rounds 1-2 reported as the step) ------------------------------------
    log(f"{elapsed / args.steps * 1e3:.2f} ms per step; replay / new-weight variants")
    call(0)
    replay_s, replay_per = timed_calls(max(5, args.steps // 2))
    # ---- same requests, weights never used before: a new mom2_update_weight reuses the cached factor of C' (chol(lam C') =
    # sqrt(lam) chol(C')); a new edit_weight changes C' itself (fp32 rounding per entry) and is refactored -------------------
    import copy
    lam_list = [2500, 3000, 5000, 6000, 8000]
    ew_list = [0.35, 0.4, 0.45, 0.55, 0.6]
    new_lam_ms = each_synced(len(lam_list), lambda i: call(0, copy.deepcopy(hp), mom2_weight=lam_list[i]))
    new_ew_ms = each_synced(len(ew_list), lambda i: call(0, copy.deepcopy(hp), edit_weight=ew_list[i]))
    call(0)        # (lam, e_w) of the workload again (its factors are still cached)

    log("GEMM A/B, host/device split, roofline pass")
    # ---- the forward's projections on torch's F.linear (hipBLASLt, library-default selection, element-wise passes unfused)
    # instead of the library's own fp32-MFMA GEMM with fused epilogues (csrc/gemm_f32.hip): a few calls -----------------------
    other_gemm_ms = None
    if not args.no_gemm_ab:
        # the A/B path: the exact-f32 MFMA kernel (csrc/gemm_f32.hip) when this run is on the split-fp16 kernel, else torch
        if split_gemm:
            clip_forward.SPLIT_GEMM = False
        else:
            clip_forward.OWN_GEMM = not own_gemm
        call()
        other_s, _ = timed_calls(max(3, args.steps // 2))
        other_gemm_ms = other_s / max(3, args.steps // 2) * 1e3
        clip_forward.OWN_GEMM, clip_forward.SPLIT_GEMM = own_gemm, (split_gemm or clip_forward.SPLIT_GEMM)
        call()

    # ---- host / device split: prepare alone (median), then run_encoder_edit on the HBM-resident plan ---------------------
    prep_ms = []
    plan = None
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = em.prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, reqs, hp, hp.layers, hp.mom2_update_weight,
                                            stats, cache, "", verbose=False, shard=shard)
        prep_ms.append((time.perf_counter() - t0) * 1e3)      # host time until prepare returns (it LAUNCHES the leading layers)
        torch.cuda.synchronize()

    def device_step():
        restore_weights()
        return run_encoder_edit(plan, keep_factors=False, restore=False)

    for _ in range(2):
        device_step()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        device_step()
    sync()
    device_ms = (time.perf_counter() - t0) / args.steps * 1e3
    check_info(plan)

    # ---- roofline: the same K device steps once more with every kernel class bracketed by HIP events on the launch stream
    # (emcid_profile_*; graph replay is bypassed while events are recorded, kernels and arguments are identical) ------------
    hip.LINEAR_FLOPS.update(count=True, flops=0.0, launches=0)
    prof, left = {}, args.steps
    while left > 0:                         # (the library's event pool holds ~25 steps of brackets: collected in slices)
        hip.profile_enable([c for c in hip.PROF_CLASSES])
        for _ in range(min(left, 20)):
            device_step()
        sync()
        for c, (ms, launches) in hip.profile_collect().items():
            prof[c] = (prof.get(c, (0.0, 0))[0] + ms, prof.get(c, (0.0, 0))[1] + launches)
        hip.profile_enable([])
        left -= 20
    hip.LINEAR_FLOPS["count"] = False
    d, h = 3072, 768
    N, L = args.concepts, len(LAYERS)
    dual = plan.dual_ws is not None
    flops = step_flops(N, N, d, h, L, dual, True, plan.factors_from_cache,
                       min(L, 1))
    classes = {}
    for c, (ms, launches) in prof.items():
        rec = {"ms_per_step": ms / args.steps, "launches_per_step": launches / args.steps}
        if c in flops or c in FP64_CLASSES:
            fl = flops.get(c, 0)
            rec["algorithmic_flops_per_step"] = fl
            rec["tflops"] = fl * args.steps / (ms * 1e-3) / 1e12 if ms > 0 else None
            rec["frac_f64_mfma_peak"] = rec["tflops"] / F64_MFMA_PEAK_TFLOPS if rec["tflops"] is not None else None
        classes[c] = rec
    f64 = [c for c in prof if c in FP64_CLASSES]
    solve_ms = sum(prof[c][0] for c in f64) / args.steps
    solve_flops = sum(flops.get(c, 0) for c in f64)
    survey_flops = L * (N * d * d + d ** 3 // 3 + 2 * N * d * d + 2 * h * N * d)     # 4.27e10 per layer
    solve = {"classes": f64, "ms_per_step": solve_ms, "algorithmic_flops_per_step": solve_flops,
             "tflops": solve_flops / (solve_ms * 1e-3) / 1e12 if solve_ms else None,
             "frac_f64_mfma_peak": solve_flops / (solve_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS if solve_ms else None,
             "survey_8d_flops_per_step": survey_flops,
             "survey_8d_frac_over_solve_time": survey_flops / (solve_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS if solve_ms else None,
             "survey_8d_frac_over_device_step": survey_flops / (device_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS}
    # the forward's projections (class "linear", fp32 MFMA): algorithmic 2 M N K of every launch of the profiled steps (a device
    # step on a plan whose prepared state has been used runs the leading layers itself, so all of the forward is in here)
    lin = None
    if "linear" in prof and hip.LINEAR_FLOPS["flops"] > 0:
        lin_ms, lin_launches = prof["linear"]
        tot_ms, tot_flops, tot_launches = lin_ms / args.steps, hip.LINEAR_FLOPS["flops"] / args.steps, lin_launches / args.steps
        lin = {"ms_per_step": tot_ms, "launches_per_step": tot_launches, "algorithmic_flops_per_step": tot_flops,
               "tflops": tot_flops / (tot_ms * 1e-3) / 1e12, "frac_f32_mfma_peak": tot_flops / (tot_ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS}
        classes["linear"] = lin
    roofline = None
    top = max(f64, key=lambda c: prof[c][0]) if f64 else None
    if lin is not None and (top is None or lin["ms_per_step"] >= prof[top][0] / args.steps):
        # the class with the most time of a call is the forward's GEMM kernel
        pmc = REPO / "profiles" / "r03_pmc_linear.json"
        traffic = traffic_note = None
        if pmc.exists():
            with open(pmc) as fh:
                rec = json.load(fh)
            traffic, traffic_note = rec.get("traffic_bytes_per_launch"), rec.get("note")
        if split_gemm:
            # three f16 MFMAs per algorithmic multiply-add: the rate at which this algorithm's 2 M N K can execute is a third of
            # the dense f16 MFMA peak
            peak = F16_MFMA_PEAK_TFLOPS / 3.0
            lin["frac_f16_mfma_peak"] = lin["tflops"] / peak
            lin["mfma_tflops_executed"] = 3.0 * lin["tflops"]
            held_clock = None
            pmc = REPO / "profiles" / "r06_pmc_linear_sp16.json"          # (this round's counter passes of the same kernels)
            if not pmc.exists():
                pmc = REPO / "profiles" / "r05_pmc_linear_sp16.json"
            traffic = traffic_note = None
            if pmc.exists():
                with open(pmc) as fh:
                    rec = json.load(fh)
                traffic = rec.get("traffic_bytes_per_launch")
                traffic_note = f"STORED value from {pmc.relative_to(REPO)} (counter passes of the same kernels, not of this run): " + str(rec.get("note"))
                # the clock the chip HELD in those launches (GRBM_GUI_ACTIVE / 8 / wall, MI355X_MICROARCH.md "DVFS give-back"),
                # weighted by each shape's launch time: informational — `frac` stays against the 2.4 GHz peak
                shapes_ = [v for v in (rec.get("per_shape") or {}).values() if v.get("clock_ghz") and v.get("avg_us")]
                if shapes_:
                    held_clock = sum(v["clock_ghz"] * v["avg_us"] for v in shapes_) / sum(v["avg_us"] for v in shapes_)
            roofline = {"bound": "mfma", "kernel": KERNEL_OF_CLASS["linear_sp16"], "class": "linear", "achieved": lin["tflops"],
                        "peak": peak, "unit": "TFLOP/s", "frac": lin["tflops"] / peak,
                        "dtype": "f32 (2 x fp16 split: 3 f16 MFMAs per k-step, fp32 accumulate)",
                        "peak_note": "algorithmic 2 M N K against a third of the dense f16 MFMA peak (2.5 PFLOP/s, "
                                     "MI355X_MICROARCH.md): every multiply-add is three MFMA multiply-adds",
                        "mfma_tflops_executed": 3.0 * lin["tflops"], "f16_mfma_peak": F16_MFMA_PEAK_TFLOPS,
                        "over_f32_mfma_peak": lin["tflops"] / F32_MFMA_PEAK_TFLOPS,
                        "traffic": traffic, "traffic_unit": "bytes/launch", "traffic_note": traffic_note,
                        "avg_launch_us": lin["ms_per_step"] * 1e3 / lin["launches_per_step"],
                        "launches_per_step": lin["launches_per_step"],
                        "flops_per_launch": lin["algorithmic_flops_per_step"] / lin["launches_per_step"],
                        "selection": "the kernel class with the most time per call over ALL classes (forward GEMMs and fp64 solve)",
                        "held_clock_ghz": held_clock,
                        "frac_at_held_clock": (lin["tflops"] / peak * 2.4 / held_clock) if held_clock else None,
                        "held_clock_note": "informational: the shader clock the chip held in these kernels' counter passes (it lowers its "
                                           "clock under MFMA load on random data; launch-time-weighted over the four shapes) and the same "
                                           "fraction against the peak AT that clock; `frac` is against the 2.4 GHz peak.  The GRBM quotient reads HIGH on "
                                           "dispatches this short (MI355X_MICROARCH.md): in-kernel stamps of the same loops read 1.75-1.93 GHz "
                                           "(profiles/r05_mb_linear_sp16_rounds.txt), so this fraction is a lower bound of the at-clock one",
                        "next": (None if top is None else {"class": top, "ms_per_step": prof[top][0] / args.steps,
                                                           "frac_f64_mfma_peak": classes[top].get("frac_f64_mfma_peak")})}
        else:
            roofline = {"bound": "mfma", "kernel": KERNEL_OF_CLASS["linear"], "class": "linear", "achieved": lin["tflops"],
                        "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": lin["frac_f32_mfma_peak"], "dtype": "f32",
                        "traffic": traffic, "traffic_unit": "bytes/launch", "traffic_note": traffic_note,
                        "avg_launch_us": lin["ms_per_step"] * 1e3 / lin["launches_per_step"], "launches_per_step": lin["launches_per_step"],
                        "flops_per_launch": lin["algorithmic_flops_per_step"] / lin["launches_per_step"],
                        "selection": "the kernel class with the most time per call over ALL classes (forward GEMMs and fp64 solve)",
                        "next": (None if top is None else {"class": top, "ms_per_step": prof[top][0] / args.steps,
                                                           "frac_f64_mfma_peak": classes[top].get("frac_f64_mfma_peak")})}
    elif top is not None:
        ms, launches = prof[top]
        achieved = flops.get(top, 0) * args.steps / (ms * 1e-3) / 1e12      # = flops per launch / average launch duration
        traffic, traffic_note = None, None
        pmc = REPO / "profiles" / f"r02_pmc_{top}.json"
        if pmc.exists():
            with open(pmc) as fh:
                rec = json.load(fh)
            traffic = rec.get("traffic_bytes_per_launch")
            traffic_note = rec.get("note")
        roofline = {"bound": "mfma", "kernel": KERNEL_OF_CLASS.get(top, top), "class": top, "achieved": achieved,
                    "peak": F64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / F64_MFMA_PEAK_TFLOPS,
                    "traffic": traffic, "traffic_unit": "bytes/launch", "traffic_note": traffic_note,
                    "avg_launch_us": ms * 1e3 / launches, "launches": launches,
                    "flops_per_launch": flops.get(top, 0) * args.steps / launches,
                    "selection": "the kernel class with the most time per call over ALL classes (forward GEMMs and fp64 solve)",
                    "solver": "dual" if dual else "direct"}

    replay_ms = statistics.median(replay_per) * 1e3
    out["config"].update(
        prompts_per_rank=plan.n_prompts,
        forward=("prefix-trie: %d unique rows of %d tokens in %d slice(s)" % (*plan.trie_rows, len(plan.chunks)))
        if plan.chunks is not None else "hooked HF forward")
    out["config"]["caches"]["cov_factor_cache"] = ("warm (keyed by statistics + edit_weight; any mom2_update_weight)"
                                                   if plan.factors_from_cache else "off")
    out.update({
        "replay_ms_per_call": replay_ms, "replay_ms_per_call_all": [round(t * 1e3, 3) for t in replay_per],
        "fresh_over_replay": fresh_ms / replay_ms,
        "new_weights_ms": {"new_lambda_ms_per_call": statistics.median(new_lam_ms), "lambdas": lam_list,
                           "new_lambda_ms_all": [round(t, 3) for t in new_lam_ms],
                           "new_edit_weight_ms_per_call": statistics.median(new_ew_ms), "edit_weights": ew_list,
                           "new_edit_weight_ms_all": [round(t, 3) for t in new_ew_ms],
                           "note": "same requests as the replay; a new lambda reuses the cached factor of C' (lam_ratio), a new "
                                   "edit_weight refactors the four 3072 x 3072 matrices on the side stream under the forward"},
        "forward_gemm": {"this_run": ("emcid_linear_sp16_f32 (split-fp16 MFMA GEMM at fp32 accuracy, fused bias / activation / residual, "
                                       "native layer runner)" if split_gemm else
                                       "emcid_linear_f32 (own fp32-MFMA GEMM, fused bias / activation / residual)") if own_gemm
                         else "torch F.linear (hipBLASLt)",
                         "other_path_ms_per_step": other_gemm_ms,
                         "other_path": ("emcid_linear_f32 (exact-f32 MFMA GEMM, EMCID_SPLIT_GEMM=0)" if split_gemm else
                                        "torch F.linear (hipBLASLt, library-default selection) + separate element-wise passes")
                         if own_gemm else "emcid_linear_f32",
                         "paths": dict(clip_forward.LAST_PATHS),
                         "note": "replay calls (same 1 000 requests); compare with replay_ms_per_call"},
        "host_prepare_ms": statistics.median(prep_ms),
        "device_ms_per_step": device_ms,
        "roofline": roofline,
        "solve": solve,
        "kernel_classes": classes,
        "per_rank": per_rank,
        "weak_replicas": weak,
    })

    if rank == 0 and world == 1 and not args.no_variants:
        log("secondary records: n100, latency, realistic_names, n1500, no_shared_prefix, sdxl, stage1, cold_process")
        for name, fn in (("n100", lambda: n100_record(workdir, device)),
                         ("n125", lambda: n100_record(workdir, device, n=125, calls=5)),      # a rank's share of the 8-GPU concept-sharded config
                         ("latency_n1000", lambda: latency_record(workdir, device, args.concepts)),
                         ("latency_n100", lambda: latency_record(workdir, device, 100)),
                         ("realistic_names", lambda: realistic_names_record(workdir, device)),
                         ("n1500", lambda: n1500_record(workdir, device)),
                         ("no_shared_prefix", lambda: no_shared_prefix_record(workdir, device)),
                         ("sdxl", lambda: sdxl_record(workdir, device)),
                         ("stage1", lambda: stage1_record(device)),
                         ("cold_process", lambda: cold_process_record(workdir, device))):
            try:
                out[name] = fn()
            except Exception as e:     # the headline line must survive a problem in a secondary record
                out[name] = {"error": repr(e)}
            log(f"{name} done")
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        log("cpu_baseline (oracle on the host cores)")
        out.update(cpu_baseline_and_error(workdir, device, full_n=0 if args.no_cpu_full else args.concepts,
                                          full_runs=max(1, args.cpu_full_runs)))
    if rank == 0 and world == 1:
        # what the headline assumes, stated in `config` (review of round 5, item 1): the trie of its 3-syllable names, against a
        # request list shaped like the reference's 1 000-artist list and one without shared prefixes; warm factors of lam C'
        rn, ns = out.get("realistic_names") or {}, out.get("no_shared_prefix") or {}
        for rec_, shape in ((rn, "artist"), (ns, "own_prompts")):
            chk = (out.get("shape_checks") or {}).get(shape)
            if chk is not None and "error" not in rec_:
                rec_["dw_check"] = chk
        out["config"]["assumes"] = {
            "headline_trie_rows": plan.trie_rows[0] if plan.chunks is not None else None,
            "names": "3-syllable names from 90 syllables (first tokens shared 11-fold) under three shared templates",
            "factor_cache": "the d x d factors of lam C' of the four edited layers warm (a long-running editing service)",
            "call_with_cold_factor_cache_ms": statistics.median(new_ew_ms),
            "first_call_of_process_ms": first_s * 1e3,
            "realistic_names": {k: rn.get(k) for k in ("ms_per_call_median", "concept_edits_per_s", "trie_rows_of_tokens")} if rn else None,
            "no_shared_prefix": {k: ns.get(k) for k in ("ms_per_call_median", "concept_edits_per_s", "trie_rows_of_tokens")} if ns else None,
            "n100": {k: (out.get("n100") or {}).get(k) for k in ("ms_per_call_median", "concept_edits_per_s")} if out.get("n100") else None,
        }
    if rank == 0 and world == 1 and not args.no_stage0:
        log("stage0")
        try:
            out["stage0"] = stage0_record(workdir, device, args.stage0_captions)
        except Exception as e:     # the headline line must survive a Stage-0 problem
            out["stage0"] = {"error": repr(e)}
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


def _per_rank_phases(edit_engine, dist, timed_calls, args, rank, world, device, shard, rank_elapsed, host_phases):
    """A few more calls OUTSIDE the timed region with event brackets around the collectives and the solves, gathered from every rank."""
    edit_engine.DIST_TIMING["enabled"] = True
    edit_engine.dist_timing_collect()
    k_diag = max(2, min(5, args.steps))
    diag_s, _ = timed_calls(k_diag, first_set=1 + args.warmup)
    phases = {k: {"ms_per_call": v[0] / k_diag, "brackets_per_call": v[1] / k_diag}
              for k, v in edit_engine.dist_timing_collect().items()}
    edit_engine.DIST_TIMING["enabled"] = False
    coll = sum(v["ms_per_call"] for k, v in phases.items() if k.startswith(("all_reduce", "k_all_gather")))
    lo, hi = shard.bounds(args.concepts)
    mine = {"rank": rank, "device": str(device), "timed_region_s": rank_elapsed, "ms_per_call": diag_s / k_diag * 1e3,
            "phases_ms_per_call": phases, "collectives_ms_per_call": coll,
            "forward_and_host_ms_per_call": diag_s / k_diag * 1e3 - phases.get("solve (incl. its collectives)", {}).get("ms_per_call", 0.0),
            "host_phases_ms_per_call": host_phases, "concepts_of_this_rank": hi - lo}
    gathered = [None] * world
    dist.all_gather_object(gathered, mine)
    return gathered


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline_and_error(workdir, device, n_sample=100, budget_s=40.0, full_n=0, full_runs=3, full_budget_s=200.0):
    """Oracle on the host cores over a 100-concept sample of the workload (median of up to 3 runs inside `budget_s`) +
    dW error of the HIP path on the same sample; with `full_n`, ONE more run on the full request set of the GPU number
    ("same request sets"; about a minute).  host_s = tokenizer, subject search, v*/C reads inside the call."""
    import copy
    import torch
    from emcid_amd import effective_cpu_count, emcid_main as em, synthetic as syn
    from emcid_amd.emcid_hparams import EMCIDHyperParams
    from emcid_amd.nethook import get_parameter
    from oracle import emcid_oracle as orc

    cores = torch.get_num_threads()
    host_acc = [0.0]

    def timed(fn):
        def wrapper(*a, **k):
            t = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                host_acc[0] += time.perf_counter() - t
        return wrapper

    host_fns = ("tokenize_prompts", "find_token_range", "load_vstars", "load_cov")
    saved = {n: getattr(orc, n) for n in host_fns}

    def oracle_runs(n_concepts, max_runs, budget):
        pipe_c, reqs, hp_d, cache, stats, layer_names = build_inputs(n_concepts, "cpu", workdir)
        w0 = {ln: orc.get_parameter(pipe_c.text_encoder, ln + ".weight").clone() for ln in layer_names}
        runs = []
        try:
            for n in host_fns:
                setattr(orc, n, timed(saved[n]))
            t_all = time.perf_counter()
            while len(runs) < max_runs and (not runs or time.perf_counter() - t_all + runs[-1][0] < budget):
                with torch.no_grad():
                    for ln in layer_names:
                        orc.get_parameter(pipe_c.text_encoder, ln + ".weight").copy_(w0[ln])
                host_acc[0] = 0.0
                t0 = time.perf_counter()
                orc.apply_emcid_to_text_encoder(pipe_c, reqs, copy.deepcopy(hp_d), cache_name=cache, stats_dir=stats)
                runs.append((time.perf_counter() - t0, host_acc[0]))
        finally:
            for n in host_fns:
                setattr(orc, n, saved[n])
        runs.sort()
        return runs, (pipe_c, reqs, hp_d, cache, stats, layer_names, w0)

    def dw_error(ctx):
        pipe_c, reqs, hp_d, cache, stats, layer_names, w0 = ctx
        pipe_g = syn.build_pipe(KIND, device, syllables=True)
        em.apply_emcid_to_text_encoder(pipe_g, reqs, EMCIDHyperParams(**hp_d), device, cache_name=cache, stats_dir=stats,
                                       verbose=False)
        err_abs, err_rel = 0.0, 0.0
        for ln in layer_names:
            ref = orc.get_parameter(pipe_c.text_encoder, ln + ".weight").double() - w0[ln].double()
            got = get_parameter(pipe_g.text_encoder, ln + ".weight").cpu().double() - w0[ln].double()
            e = (got - ref).abs().max().item()
            err_abs = max(err_abs, e)
            err_rel = max(err_rel, e / ref.abs().max().item())
        return err_abs, err_rel

    runs, ctx = oracle_runs(n_sample, 3, budget_s)
    cpu_s, host_s = runs[len(runs) // 2]
    log(f"cpu_baseline: {n_sample}-concept sample {cpu_s:.1f} s per run")
    err_abs, err_rel = dw_error(ctx)
    rec = {"value": n_sample / cpu_s, "unit": "concept-edits/s", "cores": cores, "kind": "port",
           "cores_note": f"torch intra-op threads = the CPUs this process may use (cgroup quota / affinity: "
                         f"{effective_cpu_count()}; the machine shows {os.cpu_count()} hardware threads); bench.py runs under "
                         f"EMCID_MANAGE_THREADS=1, which lowers PyTorch's default pool to that number",
           "cpu_model": cpu_model(), "runs": len(runs), "seconds_per_run": [r[0] for r in runs],
           "host_s": host_s, "compute_s": cpu_s - host_s,
           "sample": f"{n_sample}-concept edit (300 prompts), same dims/layers/lambda through the oracle's "
                     f"op-for-op port of apply_emcid_to_text_encoder, timer around the call (median "
                     f"{cpu_s:.1f} s of {len(runs)} runs; the cost is ~linear in the concept count: 2 full "
                     f"encoder forwards per edited layer over all prompts)"}
    out = {"cpu_baseline": rec, "dw_max_abs_err": err_abs, "dw_max_rel_err": err_rel}
    # ---- the same check on the two request shapes the syllable names do not exercise (a 100-concept sample each, same leg: the
    # oracle is the checker): two-word artist-like names under the shared templates; every request's own prompts ---------------
    shape_checks = {}
    for shape in ("artist", "own_prompts"):
        try:
            vocab = "wide" if shape == "artist" else True
            reqs = syn.make_requests(n_sample, names="artist" if shape == "artist" else "syllable", name_seed=7)
            if shape == "own_prompts":
                reqs = syn.own_prompt_requests(reqs, seed=978)
            _, _, hp_d, _, stats, layer_names = build_inputs(n_sample, "cpu", workdir)
            cache = str(Path(workdir) / f"cache_check_{shape}_{n_sample}") + "/"
            syn.write_vstar_cache(cache, reqs, syn.ENCODER_DIMS[KIND][0], seed=11, scale=0.5)
            pipe_c = syn.build_pipe(KIND, "cpu", syllables=vocab)
            w0 = {ln: orc.get_parameter(pipe_c.text_encoder, ln + ".weight").clone() for ln in layer_names}
            t0 = time.perf_counter()
            orc.apply_emcid_to_text_encoder(pipe_c, reqs, copy.deepcopy(hp_d), cache_name=cache, stats_dir=stats)
            cpu_shape_s = time.perf_counter() - t0
            pipe_g = syn.build_pipe(KIND, device, syllables=vocab)
            em.apply_emcid_to_text_encoder(pipe_g, reqs, EMCIDHyperParams(**hp_d), device, cache_name=cache, stats_dir=stats, verbose=False)
            from emcid_amd import clip_forward
            ea, er = 0.0, 0.0
            for ln in layer_names:
                ref = orc.get_parameter(pipe_c.text_encoder, ln + ".weight").double() - w0[ln].double()
                got = get_parameter(pipe_g.text_encoder, ln + ".weight").cpu().double() - w0[ln].double()
                e = (got - ref).abs().max().item()
                ea, er = max(ea, e), max(er, e / ref.abs().max().item())
            shape_checks[shape] = {"concepts": n_sample, "dw_max_abs_err": ea, "dw_max_rel_err": er,
                                   "trie_rows_of_tokens": [clip_forward.LAST_PATHS.get("last_trie_rows"), clip_forward.LAST_PATHS.get("last_trie_tokens")],
                                   "oracle_seconds": cpu_shape_s, "against": "oracle/emcid_oracle.py on the host cores, same requests"}
            del pipe_g, pipe_c
        except Exception as e:      # a diagnostic must never cost the line
            shape_checks[shape] = {"error": repr(e)}
    out["shape_checks"] = shape_checks
    if full_n and full_n != n_sample:
        log(f"cpu_baseline: full {full_n}-concept run (about {cpu_s * full_n / n_sample:.0f} s)")
        # median of 3 runs after a warm-up (the sample runs above are the warm-up); a third run is dropped
        # when the first two already took more than `full_budget_s` (a slow host must not push the bench past its minutes)
        runs_f, ctx_f = oracle_runs(full_n, full_runs, full_budget_s)
        fa, fr = dw_error(ctx_f)
        med_s, med_host = runs_f[len(runs_f) // 2]
        full = {"value": full_n / med_s, "unit": "concept-edits/s", "seconds": med_s, "host_s": med_host,
                "runs": len(runs_f), "seconds_per_run": [r[0] for r in runs_f],
                "sample": f"the full {full_n}-concept request set of the GPU number (set 0), median of {len(runs_f)} run(s)",
                "dw_max_abs_err": fa, "dw_max_rel_err": fr}
        # the like-for-like figure leads: `value` is the full request set of the GPU number; the bounded sample moves below it
        rec["sample_run"] = {k: rec[k] for k in ("value", "runs", "seconds_per_run", "host_s", "compute_s", "sample")}
        rec.update(value=full["value"], sample=full["sample"], seconds=full["seconds"], host_s=full["host_s"], runs=len(runs_f),
                   seconds_per_run=full["seconds_per_run"], compute_s=full["seconds"] - full["host_s"])
        rec["full"] = full
    return out


def profiled_classes(steps, step_fn, flops):
    """`steps` runs of step_fn with every kernel class bracketed by HIP events on the launch stream: ({class: record},
    solve record).  flops: {class: algorithmic flops per step}."""
    import torch
    from emcid_amd import hip
    hip.profile_enable([c for c in hip.PROF_CLASSES])
    for _ in range(steps):
        step_fn()
    torch.cuda.synchronize()
    prof = hip.profile_collect()
    hip.profile_enable([])
    classes = {}
    for c, (ms, launches) in prof.items():
        rec = {"ms_per_step": ms / steps, "launches_per_step": launches / steps}
        if c in flops or c in FP64_CLASSES:
            fl = flops.get(c, 0)
            rec["algorithmic_flops_per_step"] = fl
            rec["tflops"] = fl * steps / (ms * 1e-3) / 1e12 if ms > 0 else None
            rec["frac_f64_mfma_peak"] = rec["tflops"] / F64_MFMA_PEAK_TFLOPS if rec["tflops"] is not None else None
        classes[c] = rec
    f64 = [c for c in prof if c in FP64_CLASSES]
    solve_ms = sum(prof[c][0] for c in f64) / steps
    solve_flops = sum(flops.get(c, 0) for c in f64)
    solve = {"ms_per_step": solve_ms, "algorithmic_flops_per_step": solve_flops,
             "tflops": solve_flops / (solve_ms * 1e-3) / 1e12 if solve_ms else None,
             "frac_f64_mfma_peak": solve_flops / (solve_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS if solve_ms else None}
    top = max(f64, key=lambda c: prof[c][0]) if f64 else None
    roofline = None
    if top is not None:
        ms, launches = prof[top]
        ach = flops.get(top, 0) * steps / (ms * 1e-3) / 1e12
        roofline = {"bound": "mfma", "class": top, "kernel": KERNEL_OF_CLASS.get(top, top), "achieved": ach,
                    "peak": F64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / F64_MFMA_PEAK_TFLOPS, "traffic": None,
                    "avg_launch_us": ms * 1e3 / launches, "launches": launches}
    return classes, solve, roofline


def n100_record(workdir, device, n=100, calls=9):
    """BASELINE config 2: the 100-concept batch on SD-v1.4 dims, one GPU: wall of apply_emcid_to_text_encoder (median; every
    call a request set the process has not seen before)."""
    import torch
    from emcid_amd import emcid_main as em
    from emcid_amd.emcid_hparams import EMCIDHyperParams
    from emcid_amd.nethook import get_parameter

    pipe, reqs, hp_d, cache, stats, layer_names = build_inputs(n, device, workdir)
    sets = [(reqs, cache)] + [request_set(n, workdir, j) for j in range(1, calls + 3)]
    hp = EMCIDHyperParams(**hp_d)
    w0 = {ln: get_parameter(pipe.text_encoder, ln + ".weight").detach().clone() for ln in layer_names}
    from emcid_amd import edit_engine
    ms = []
    for i, (r, c) in enumerate(sets):
        with torch.no_grad():
            for ln in layer_names:
                get_parameter(pipe.text_encoder, ln + ".weight").copy_(w0[ln])
        torch.cuda.synchronize()
        if i == 3:
            edit_engine.TIMING.clear()
        t0 = time.perf_counter()
        em.apply_emcid_to_text_encoder(pipe, r, hp, device, cache_name=c, stats_dir=stats, verbose=False)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    timed = ms[3:]
    med = statistics.median(timed)
    host_phases = {k: round(v / len(timed) * 1e3, 4) for k, v in edit_engine.TIMING.items()}
    # ---- where the device time of this latency-bound call goes (review of round 5, item 5): the plan's device step alone, then
    # the same step with every kernel class bracketed by HIP events (graph replay bypassed while events are recorded) ----------
    from emcid_amd import hip
    from emcid_amd.edit_engine import run_encoder_edit, check_info
    plan = em.prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, reqs, hp, hp.layers, hp.mom2_update_weight,
                                        stats, cache, "", verbose=False)

    def device_step():
        with torch.no_grad():
            for ln in layer_names:
                get_parameter(pipe.text_encoder, ln + ".weight").copy_(w0[ln])
        return run_encoder_edit(plan, keep_factors=False, restore=False)

    for _ in range(3):
        device_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        device_step()
    torch.cuda.synchronize()
    device_ms = (time.perf_counter() - t0) / 20 * 1e3
    flops = step_flops(n, n, 3072, 768, len(LAYERS), plan.dual_ws is not None, True, plan.factors_from_cache, 1)
    hip.LINEAR_FLOPS.update(count=True, flops=0.0, launches=0)
    classes, solve, _ = profiled_classes(10, device_step, flops)
    hip.LINEAR_FLOPS["count"] = False
    check_info(plan)
    bracketed = sum(r["ms_per_step"] for r in classes.values())
    return {"workload": f"{n}-concept edit, SD-v1.4 dims, layers 7-10, lambda 4000 (BASELINE config 2), one GPU; every call a "
                        f"never-seen request set", "ms_per_call_median": med, "ms_per_call": [round(t, 3) for t in timed],
            "host_phases_ms_per_call": host_phases,
            "concept_edits_per_s": n / (med * 1e-3), "first_call_ms_this_shape": ms[0], "calls": len(timed),
            "trie_rows_of_tokens": list(plan.trie_rows) if plan.chunks is not None else None,
            "device_ms_per_step": device_ms, "device_ms_in_bracketed_kernels": bracketed,
            "launches_per_step": sum(r["launches_per_step"] for r in classes.values()),
            "solve_ms_per_step": solve["ms_per_step"],
            "kernel_classes": {c: {k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items()
                                   if k in ("ms_per_step", "launches_per_step", "frac_f64_mfma_peak")} for c, r in classes.items()}}


def percentiles(ms):
    """p50 / p95 / p99 / max of a list of per-call milliseconds (nearest-rank on the sorted list)."""
    v = sorted(ms)
    def q(p):
        return v[min(len(v) - 1, max(0, int(round(p * (len(v) - 1)))))]
    return {"calls": len(v), "p50": q(0.50), "p95": q(0.95), "p99": q(0.99), "max": v[-1], "min": v[0],
            "over_1p3x_median": sum(1 for t in v if t > 1.3 * q(0.50))}


def latency_record(workdir, device, n, calls=200, kind="syllable"):
    """Per-call wall-clock distribution of `calls` warm apply_emcid_to_text_encoder calls on `n`-concept request sets (cycled over
    the distinct sets on disk; each call synchronised, weights restored before it, as in the headline)."""
    import torch
    from emcid_amd import emcid_main as em
    from emcid_amd.emcid_hparams import EMCIDHyperParams
    from emcid_amd.nethook import get_parameter

    pipe, reqs, hp_d, cache, stats, layer_names = build_inputs(n, device, workdir)
    sets = [(reqs, cache)] + [request_set(n, workdir, j) for j in range(1, 12)]
    hp = EMCIDHyperParams(**hp_d)
    w0 = {ln: get_parameter(pipe.text_encoder, ln + ".weight").detach().clone() for ln in layer_names}
    ms = []
    for i in range(calls + 5):
        r, c = sets[i % len(sets)]
        with torch.no_grad():
            for ln in layer_names:
                get_parameter(pipe.text_encoder, ln + ".weight").copy_(w0[ln])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        em.apply_emcid_to_text_encoder(pipe, r, hp, device, cache_name=c, stats_dir=stats, verbose=False)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    rec = percentiles(ms[5:])
    rec["workload"] = f"{n}-concept edit, SD-v1.4 dims, layers 7-10: {calls} warm calls over {len(sets)} request sets, each between two synchronisations"
    return rec


def realistic_names_record(workdir, device, n=1000, calls=7):
    """The headline edit on a request list with the first-word statistics of the reference's artist lists
    (data/artists/info/erased-1000artists-....txt: two-word names of 3-5 tokens, ~650 distinct first words of 1 000, the
    commonest ~21 times) instead of the 3-syllable names drawn from 90 syllables (which share first tokens 11-fold): how many trie
    rows the three shared templates leave, and what the call costs.  Synthetic names of that shape (emcid_amd.synthetic.
    artist_names, `syllables="wide"` vocabulary: its own model object, same dims); the list itself is not shipped."""
    import torch
    from emcid_amd import emcid_main as em, synthetic as syn
    from emcid_amd.emcid_hparams import EMCIDHyperParams
    from emcid_amd.nethook import get_parameter

    pipe = syn.build_pipe(KIND, device, syllables="wide")
    hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=LAM, edit_weight=EW)
    hp = EMCIDHyperParams(**hp_d)
    layer_names = [hp_d["rewrite_module_tmp"].format(l) for l in LAYERS]
    _, _, _, _, stats, _ = build_inputs(n, "cpu", workdir)
    w0 = {ln: get_parameter(pipe.text_encoder, ln + ".weight").detach().clone() for ln in layer_names}
    ms, rows, tok_hist = [], None, None
    for j in range(calls + 2):
        reqs = syn.make_requests(n, names="artist", name_seed=3 + 101 * j)
        cache = str(Path(workdir) / f"cache_artist_{n}_set{j}") + "/"
        if not (Path(cache) / ".complete").exists():
            syn.write_vstar_cache(cache, reqs, syn.ENCODER_DIMS[KIND][0], seed=1 + j, scale=0.5)
            (Path(cache) / ".complete").touch()
        with torch.no_grad():
            for ln in layer_names:
                get_parameter(pipe.text_encoder, ln + ".weight").copy_(w0[ln])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        em.apply_emcid_to_text_encoder(pipe, reqs, hp, device, cache_name=cache, stats_dir=stats, verbose=False)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if rows is None:
            plan = em.prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, reqs, hp, hp.layers, hp.mom2_update_weight,
                                                stats, cache, "", verbose=False)
            rows = list(plan.trie_rows) if getattr(plan, "trie_rows", None) else None
            torch.cuda.synchronize()
            lens = [len(pipe.tokenizer(r["source"])["input_ids"]) - 2 for r in reqs]
            firsts = len({r["source"].split()[0] for r in reqs})
            tok_hist = {"tokens_per_name_mean": sum(lens) / len(lens), "tokens_per_name_min_max": [min(lens), max(lens)],
                        "distinct_first_words": firsts}
    timed = ms[2:]
    med = statistics.median(timed)
    return {"workload": f"{n}-concept edit, SD-v1.4 dims, layers 7-10, lambda 4000, the three shared templates, two-word names with "
                        f"the first-word sharing of the reference's 1 000-artist list (synthetic names of that shape); every call a "
                        f"never-seen name list", "names": tok_hist, "trie_rows_of_tokens": rows, "ms_per_call_median": med,
            "ms_per_call": [round(t, 3) for t in timed], "concept_edits_per_s": n / (med * 1e-3), "calls": len(timed)}


def n1500_record(workdir, device, n=1500, calls=7):
    """The reference's largest shipped request list (data/artists/info/erased-1500artists-....txt through
    dsets/artist_requests.py:27-46): 1 500 concepts, Np = 1536 — other tile / stream-K / shadow-fit decisions than Np = 1024."""
    import torch
    from emcid_amd import emcid_main as em
    from emcid_amd.emcid_hparams import EMCIDHyperParams
    from emcid_amd.nethook import get_parameter

    pipe, reqs, hp_d, cache, stats, layer_names = build_inputs(n, device, workdir)
    sets = [(reqs, cache)] + [request_set(n, workdir, j) for j in range(1, calls + 2)]
    hp = EMCIDHyperParams(**hp_d)
    w0 = {ln: get_parameter(pipe.text_encoder, ln + ".weight").detach().clone() for ln in layer_names}
    ms = []
    for r, c in sets:
        with torch.no_grad():
            for ln in layer_names:
                get_parameter(pipe.text_encoder, ln + ".weight").copy_(w0[ln])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        em.apply_emcid_to_text_encoder(pipe, r, hp, device, cache_name=c, stats_dir=stats, verbose=False)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    timed = ms[2:]
    med = statistics.median(timed)
    return {"workload": f"{n}-concept edit (the reference's largest shipped list size), SD-v1.4 dims, layers 7-10, lambda 4000, one GPU; "
                        f"every call a never-seen request set", "ms_per_call_median": med, "ms_per_call": [round(t, 3) for t in timed],
            "concept_edits_per_s": n / (med * 1e-3), "first_call_ms_this_shape": ms[0], "calls": len(timed)}


def no_shared_prefix_record(workdir, device, n=1000, calls=5):
    """How much of the headline is the workload's shape: the same 1 000-concept edit with request lists whose prompts share
    NOTHING but the start token — every request brings its own three prompts with three words of its own (>= 8 tokens) in front
    of the subject, so the prefix trie has (almost) one row per token — against the headline's three templates shared by all
    concepts (6 292 rows for 21 000 tokens)."""
    import torch
    from emcid_amd import emcid_main as em, synthetic as syn
    from emcid_amd.emcid_hparams import EMCIDHyperParams
    from emcid_amd.nethook import get_parameter

    pipe, reqs0, hp_d, cache0, stats, layer_names = build_inputs(n, device, workdir)
    hp = EMCIDHyperParams(**hp_d)
    w0 = {ln: get_parameter(pipe.text_encoder, ln + ".weight").detach().clone() for ln in layer_names}
    ms, rows = [], None
    for j in range(calls + 2):
        reqs, cache = request_set(n, workdir, 40 + j)
        reqs = syn.own_prompt_requests(reqs, seed=977 + j)
        with torch.no_grad():
            for ln in layer_names:
                get_parameter(pipe.text_encoder, ln + ".weight").copy_(w0[ln])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        em.apply_emcid_to_text_encoder(pipe, reqs, hp, device, cache_name=cache, stats_dir=stats, verbose=False)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        if rows is None:
            plan = em.prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, reqs, hp, hp.layers, hp.mom2_update_weight,
                                                stats, cache, "", verbose=False)
            rows = list(plan.trie_rows) if getattr(plan, "trie_rows", None) else None
            torch.cuda.synchronize()
    timed = ms[2:]
    med = statistics.median(timed)
    return {"workload": f"{n}-concept edit, SD-v1.4 dims, layers 7-10, lambda 4000, three prompts per concept with three words of "
                        f"the request's own (9+ tokens) in front of the subject: no shared prefixes beyond the start token",
            "trie_rows_of_tokens": rows, "ms_per_call_median": med, "ms_per_call": [round(t, 3) for t in timed],
            "concept_edits_per_s": n / (med * 1e-3), "calls": len(timed)}


def sdxl_record(workdir, device, n=1000, calls=5):
    """BASELINE config 4 on one GPU: SDXL dual text-encoder edit (TE1 768/3072/12L layers 8-10, TE2 1280/5120/32L layers
    26-30), N = 1000: wall of apply_emcid_to_sdxl_text_encoders, TE1 / TE2 device steps alone, roofline of the dominant
    class of the two encoders' solves."""
    import torch
    from emcid_amd import emcid_main as em, synthetic as syn
    from emcid_amd.edit_engine import check_info, run_encoder_edit
    from emcid_amd.emcid_hparams import EMCIDXLHyperParams
    from emcid_amd.nethook import get_parameter

    tmp = Path(workdir) / "sdxl"
    pipe = syn.build_pipe("sd-v1.4", device, sdxl=True, syllables=True)
    reqs = syn.make_requests(n, names="syllable")
    hp_d = syn.sdxl_hparams_dict()
    hp = EMCIDXLHyperParams(**hp_d)
    cache = str(tmp / f"cache_{n}") + "/"
    n1 = [hp.rewrite_module_tmp.format(l) for l in hp.layers]
    n2 = [hp.rewrite_module_tmp.format(l) for l in hp.layers_2]
    if not (tmp / ".complete").exists():
        syn.write_vstar_cache(cache, reqs, 768, seed=1, scale=0.5)
        syn.write_vstar_cache(cache, reqs, 1280, seed=5, scale=0.5, suffix="_2")
        syn.write_stats_cache(tmp / "s1", n1, 3072, hp.mom2_n_samples, seed=2, t=6144)
        syn.write_stats_cache(tmp / "s2", n2, 5120, hp.mom2_n_samples, seed=7, t=10240)
        (tmp / ".complete").touch()
    w1 = {nm: get_parameter(pipe.text_encoder, nm + ".weight").detach().clone() for nm in n1}
    w2 = {nm: get_parameter(pipe.text_encoder_2, nm + ".weight").detach().clone() for nm in n2}

    def restore():
        with torch.no_grad():
            for nm, w in w1.items():
                get_parameter(pipe.text_encoder, nm + ".weight").copy_(w)
            for nm, w in w2.items():
                get_parameter(pipe.text_encoder_2, nm + ".weight").copy_(w)

    def apply_call():
        restore()
        em.apply_emcid_to_sdxl_text_encoders(pipe, reqs, hp, device, cache_name=cache, stat_dir=str(tmp / "s1"),
                                             stat_dir_2=str(tmp / "s2"), verbose=False)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    apply_call()
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    apply_call()
    ms = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        apply_call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms)
    p1, p2 = em._sdxl_plans(pipe, reqs, hp, cache, str(tmp / "s1"), str(tmp / "s2"), False, None, None)

    def alone(p, k=3):
        def f():
            restore()
            run_encoder_edit(p)
        f()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(k):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / k * 1e3

    t1, t2 = alone(p1), alone(p2)
    first_x = 1
    f1 = step_flops(n, n, 3072, 768, len(hp.layers), p1.dual_ws is not None, True, p1.factors_from_cache, min(len(hp.layers), first_x))
    f2 = step_flops(n, n, 5120, 1280, len(hp.layers_2), p2.dual_ws is not None, True, p2.factors_from_cache,
                    min(len(hp.layers_2), first_x))
    flops = {c: f1.get(c, 0) + f2.get(c, 0) for c in set(f1) | set(f2)}

    def both():
        restore()
        run_encoder_edit(p1)
        run_encoder_edit(p2)

    classes, solve, roofline = profiled_classes(2, both, flops)
    check_info(p1)
    check_info(p2)
    survey = len(hp.layers) * (n * 3072 ** 2 + 3072 ** 3 // 3 + 2 * n * 3072 ** 2 + 2 * 768 * n * 3072) \
        + len(hp.layers_2) * (n * 5120 ** 2 + 5120 ** 3 // 3 + 2 * n * 5120 ** 2 + 2 * 1280 * n * 5120)
    return {"workload": f"SDXL dual text-encoder edit, {n} concepts, TE1 768/3072/12L layers 8-10 (lambda 4000) + TE2 "
                        f"1280/5120/32L layers 26-30 (lambda_2 10000), one GPU, two HIP streams (BASELINE config 4); timer around "
                        f"apply_emcid_to_sdxl_text_encoders, same request set every call",
            "ms_per_call_median": med, "ms_per_call": [round(t, 3) for t in ms], "concept_edits_per_s": n / (med * 1e-3),
            "first_call_ms": first_ms, "te1_device_ms": t1, "te2_device_ms": t2,
            "trie_rows": [p1.trie.n_nodes, p2.trie.n_nodes], "survey_8d_flops_per_step": survey,
            "roofline": roofline, "solve": solve,
            "kernel_classes": {c: r for c, r in classes.items() if c in FP64_CLASSES}}


def stage1_record(device, n=16, steps=10, batch=8):
    """Stage 1 (compute_z_text_encoder: the Adam optimisation of v* through the UNet) on this GPU: concepts/s
    one concept at a time and `batch` concepts per Adam step.  SD-v1.4 text encoder (768 / 12 layers, random init); the UNet /
    VAE are the synthetic stand-ins (the 32 cross-attention projections at their real widths; no conv stack — there is no
    diffusers package or checkpoint here), so this prices the text-encoder side and the per-step overheads, not a real UNet."""
    import torch
    from emcid_amd import synthetic as syn
    from emcid_amd.compute_z import compute_z_text_encoder, compute_z_text_encoder_batched
    from emcid_amd.emcid_hparams import EMCIDHyperParams

    pipe = syn.add_diffusion(syn.build_pipe(KIND, device, syllables=True), KIND)
    reqs = [dict(r, images=syn.make_images(len(r["prompts"]), 64, seed=90 + i))
            for i, r in enumerate(syn.make_requests(n, names="syllable"))]
    hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=LAM, edit_weight=EW)
    hp_d.update(v_num_grad_steps=steps, cal_text_repr_loss=True)
    hp = EMCIDHyperParams(**hp_d)
    kw = dict(noise_scheduler=syn.DDPMNoiseSchedule(), resolution=64)
    compute_z_text_encoder(pipe, reqs[0], hp, LAYERS[-1], **kw)                    # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.manual_seed(3)
    seq = [compute_z_text_encoder(pipe, r, hp, LAYERS[-1], **kw) for r in reqs]
    torch.cuda.synchronize()
    t_seq = time.perf_counter() - t0
    compute_z_text_encoder_batched(pipe, reqs[:batch], hp, LAYERS[-1], batch_size=batch, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.manual_seed(3)
    bat = compute_z_text_encoder_batched(pipe, reqs, hp, LAYERS[-1], batch_size=batch, **kw)
    torch.cuda.synchronize()
    t_bat = time.perf_counter() - t0
    dev_err = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(bat, seq))
    return {"workload": f"{n} concepts x 3 prompts, {steps} Adam steps each (shipped: 100), SD-v1.4 text encoder, synthetic UNet / VAE "
                        f"stand-ins, 64 x 64 images",
            "concepts_per_s_sequential": n / t_seq, "concepts_per_s_batched": n / t_bat, "batch": batch,
            "seconds_sequential": t_seq, "seconds_batched": t_bat, "speedup": t_seq / t_bat,
            "max_rel_deviation_batched_vs_sequential": dev_err}


def cold_child(workdir, n):
    """Child-process mode (`bench.py --cold-child WORKDIR`): ONE call in a process that has never edited — the reference's
    one-call CLI user (scripts/run_emcid.py:99); then the pieces of that
    call one at a time.  Prints one JSON line."""
    t_start = time.perf_counter()
    os.environ.setdefault("EMCID_MANAGE_THREADS", "1")
    import torch
    t_torch = time.perf_counter()
    from emcid_amd import edit_engine, emcid_main as em, hip, host_text
    from emcid_amd.emcid_hparams import EMCIDHyperParams
    from emcid_amd.nethook import get_parameter
    hip.load()
    host_text.load()
    t_lib = time.perf_counter()
    device = "cuda:0"
    torch.cuda.set_device(0)
    torch.zeros(1, device=device)
    torch.cuda.synchronize()
    t_ctx = time.perf_counter()
    pipe, reqs, hp_d, cache, stats, layer_names = build_inputs(n, device, workdir)
    hp = EMCIDHyperParams(**hp_d)
    w0 = {ln: get_parameter(pipe.text_encoder, ln + ".weight").detach().clone() for ln in layer_names}
    torch.cuda.synchronize()
    t_model = time.perf_counter()

    def one(which=0):
        r, c = request_set(n, workdir, which, write=False) if which else (reqs, cache)
        with torch.no_grad():
            for ln in layer_names:
                get_parameter(pipe.text_encoder, ln + ".weight").copy_(w0[ln])
        torch.cuda.synchronize()
        edit_engine.TIMING.clear()
        t0 = time.perf_counter()
        em.apply_emcid_to_text_encoder(pipe, r, hp, device, cache_name=c, stats_dir=stats, verbose=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, {k: round(v * 1e3, 3) for k, v in edit_engine.TIMING.items()}

    first_ms, first_phases = one(0)
    from emcid_amd import clip_forward
    warm = [one(1 + i)[0] for i in range(3)]
    with edit_engine.ENGINE_LOCK:
        edit_engine._FACTOR_CACHE.clear()
    cold_factor_ms, _ = one(4)
    em.clear_caches()
    edit_engine.clear_engine_caches()
    cold_stats_ms, stats_phases = one(5)
    warm_ms = statistics.median(warm)
    print(json.dumps({
        "cold_process_ms": first_ms, "host_phases_ms_first_call": first_phases,
        "before_the_call_ms": {"import_torch": (t_torch - t_start) * 1e3, "import_package_and_load_libraries": (t_lib - t_torch) * 1e3,
                               "gpu_context": (t_ctx - t_lib) * 1e3, "synthetic_model_to_hbm": (t_model - t_ctx) * 1e3},
        "second_to_fourth_call_ms": [round(t, 3) for t in warm], "warm_call_ms": warm_ms,
        "call_with_cold_factor_cache_ms": cold_factor_ms, "factor_and_inverses_ms": cold_factor_ms - warm_ms,
        "call_with_cold_statistics_and_factors_ms": cold_stats_ms,
        "statistics_npz_to_hbm_ms": stats_phases.get("statistics"),
        "vstar_reads_ms_first_call": first_phases.get("vstar join + h2d"),
        "first_call_minus_warm_ms": first_ms - warm_ms,
        "libraries_and_kernels_first_use_ms": first_ms - cold_stats_ms,
        "note": "cold_process_ms = wall of the ONE apply_emcid_to_text_encoder call of a fresh process (model already in HBM); "
                "call_with_cold_statistics_and_factors = the same work in a process whose libraries and kernels have run before; "
                "the difference is first-use cost (code objects, graph captures, allocator growth)"}))
    return 0


def cold_process_record(workdir, device):
    """Runs cold_child as a CHILD process (never an exec from this GPU-touching process) and returns its JSON."""
    env = dict(os.environ)
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--cold-child", str(workdir)], env=env,
                       capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": f"child exited {r.returncode}", "stderr_tail": r.stderr[-800:]}
    return json.loads(lines[-1])


def stage0_record(workdir, device, n_captions):
    """BASELINE config 5 on one GPU: second moment of the fc2 inputs of all 12 layers over `n_captions` synthetic captions in
    one pass (layer_stats_text_encoder_multi); tokens/s over the whole job and the Gram kernel against the fp32 MFMA peak."""
    import shutil
    import torch
    from emcid_amd import hip, synthetic as syn, layer_stats as ls

    tmp = Path(workdir) / "stage0"
    data = tmp / "data" / f"ccs_{n_captions}.json"
    if not data.exists():
        syn.write_captions(data, n_captions, seed=2)
    pipe = syn.build_pipe(KIND, device)
    names = [f"text_model.encoder.layers.{i}.mlp.fc2" for i in range(12)]
    d = syn.ENCODER_DIMS[KIND][1]
    for sub in ("warm", "stats"):
        shutil.rmtree(tmp / sub, ignore_errors=True)
    ls.layer_stats_text_encoder_multi(pipe.text_encoder, pipe.tokenizer, names[:2], tmp / "warm", sample_size=500,
                                      data_path=str(data), progress=None, num_workers=0)
    torch.cuda.synchronize()
    hip.profile_enable(["gram"])
    t0 = time.perf_counter()
    st = ls.layer_stats_text_encoder_multi(pipe.text_encoder, pipe.tokenizer, names, tmp / "stats", sample_size=n_captions,
                                           data_path=str(data), progress=None, num_workers=0)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    prof = hip.profile_collect()
    hip.profile_enable([])
    tokens = int(st[names[0]].mom2.count)
    gram_ms, launches = prof.get("gram", (0.0, 0))
    rows = ls.LAST_RUN.get("rows", tokens)
    alg = float(tokens) * d * d * len(names)
    exe = float(rows) * d * d * len(names)
    split = bool(hip.GRAM_SPLIT)
    peak = F16_MFMA_PEAK_TFLOPS / 3.0 if split else F32_MFMA_PEAK_TFLOPS
    kernel = ("gram_sp16_kernel (csrc/gemm_sp16.hip: the projection kernel's K loop — v_mfma_f32_16x16x32_f16, operands by LDS-DMA — on "
              "X^T planes under per-feature scales, lower 128 x 128 tiles, fp32 atomics) + gram_colmax_kernel + "
              "gram_transpose_split_kernel (both apply the packed forward's row weights as they read the rows)") if split else \
        "gram_f32_kernel (v_mfma_f32_32x32x2_f32 SYRK)"
    shutil.rmtree(tmp / "stats", ignore_errors=True)
    return {"workload": f"{n_captions} synthetic captions, SD-v1.4 dims, 12 layers in one pass (BASELINE config 5, one GPU), "
                        f"npz written", "tokens": tokens, "wall_s": wall, "tokens_per_s": tokens / wall,
            "layer_tokens_per_s": tokens * len(names) / wall, "forward": ls.LAST_RUN.get("forward", "hooked-hf"),
            "gram_rows": rows, "gram_ms": gram_ms, "gram_launches": launches,
            "gram_tflops_algorithmic": alg / (gram_ms * 1e-3) / 1e12 if gram_ms else None,
            "gram_tflops_executed": exe / (gram_ms * 1e-3) / 1e12 if gram_ms else None,
            "gram_over_f32_mfma_peak": exe / (gram_ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS if gram_ms else None,
            "gram_path": "split-fp16 (emcid_gram_accumulate_sp16_f32)" if split else "exact-f32 SYRK (emcid_gram_accumulate_f32)",
            "roofline": {"bound": "mfma", "kernel": kernel, "unit": "TFLOP/s",
                         "achieved": exe / (gram_ms * 1e-3) / 1e12 if gram_ms else None, "peak": peak,
                         "frac": exe / (gram_ms * 1e-3) / 1e12 / peak if gram_ms else None,
                         "dtype": "f32 (2 x fp16 split: 3 f16 MFMAs per k-step, fp32 accumulate)" if split else "f32",
                         "flops_counted": "rows pushed through the kernel x d^2 (SYRK count) x layers; the launches include the "
                                          "column-maximum and transpose-split passes of every 32 768-token chunk" if split else
                                          "rows pushed through the kernel x d^2 (SYRK count) x layers",
                         "peak_note": ("SYRK count (one multiply-add per lower-triangle entry and token = 2 flop counted as d^2 per "
                                       "token) against a third of the dense f16 MFMA peak: three MFMA multiply-adds each") if split
                         else "fp32 MFMA peak"}}


if __name__ == "__main__":
    main()

"""The restructured Stage-2 pass: ONE forward per encoder, the closed form solved inside the fc2 hooks.

The reference's layer loop (emcid/emcid_main.py:981-1073) runs the whole text encoder twice per edited layer
(once for the keys :987, once more for the current fc2 outputs :1004) on all N*P prompts — 98 % of its
wall-clock.  Layers are sequentially dependent: layer l+1's keys must see layer l's new
weights.  That dependency is exactly the order of a single forward pass, so here:

    forward(prompts)                                   # once
      └─ at each edited layer's fc2 (forward hook, in layer order):
           K  = gather_mean(fc2 input)                 # HIP, csrc/gram_f32.hip
           Zc = gather_mean(fc2 output)                # pre-edit output, bias included (as :1002-1016)
           [all-gather K, Zc over concept shards]      # RCCL, multi-GPU only
           W  = W0 + float(R X^T)                      # HIP fp64 MFMA solve, csrc/edit_solve.hip on csrc/spd_solve.hip
           return fc2(input) with the NEW W            # the rest of the pass sees the edited layer
      └─ the hook of the last edited layer aborts the pass (nothing downstream is needed)

Same K, Zc, A, X, R, dW as the reference's loop (same inputs to every step), 1 partial forward instead of
2*L full ones.  Host work (tokenizing, subject search, v*/C loading) happens once in ``prepare``; ``run``
touches only HBM-resident inputs — that is the region bench.py times.
"""
import logging
import math
import os
import threading
import time
import weakref
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence


import numpy as np
import torch
import torch.nn.functional as F

from . import hip
from . import clip_forward
from .clip_attention import hip_attention
from .compute_z import PromptBatch, build_prompt_batch, build_prompt_batch_multi, gather_request_means, prompt_chunk
from .nethook import StopForward, get_module, get_parameter


@dataclass
class ConceptShard:
    """This rank's contiguous slice [lo, hi) of the request list (concept sharding)."""
    rank: int = 0
    world: int = 1
    group: object = None
    force_collectives: bool = False      # run the multi-rank code path (collectives, column-sharded solve) even at world size 1:
                                         # lets ONE GPU exercise the RCCL calls on HBM buffers (tests/test_dist_gpu.py)

    @property
    def collective(self) -> bool:
        return self.world > 1 or self.force_collectives

    def bounds(self, n: int, r: Optional[int] = None):
        r = self.rank if r is None else r
        return (n * r) // self.world, (n * (r + 1)) // self.world


@dataclass
class LayerEdit:
    layer: int
    weight_name: str
    dW: torch.Tensor                       # (h, d) fp32 in HBM: float(resid @ adj_k^T)
    Xt: Optional[torch.Tensor] = None      # (N, d) f64: adj_k^T
    Rt: Optional[torch.Tensor] = None      # (N, h) f64: resid^T
    K: Optional[torch.Tensor] = None       # (N, d) fp32 keys (kept when trace=True)
    Zc: Optional[torch.Tensor] = None      # (N, h) fp32 current fc2 outputs


@dataclass
class TrieChunk:
    """This rank's requests on the prefix-trie forward: their trie, the request -> prompt offsets and, when prepare already
    ran the unedited leading layers, the state that enters the first edited layer."""
    trie: clip_forward.TokenTrie
    seg: torch.Tensor                      # (n_requests + 1,) int64 prompt offsets
    n_requests: int
    n_prompts: int
    state: Optional[tuple] = None          # (layer index, residual stream, LN1 of it | None)
    # the gather of the keys: one segment per CONCEPT.  k = 1: the trie's own lookup arrays and ``seg``.  k > 1: the B k lookups
    # reordered into (request, num) pseudo-segments of the request's P prompts each, concept rq k + num (the reference's
    # "rq num" order, emcid_main.py:993-1014), so that the one gather-mean kernel yields the N k rows in that order
    lookup_node: Optional[torch.Tensor] = None     # (B k,) int64 node of every lookup, concept order (edited layers before the last)
    lookup_query: Optional[torch.Tensor] = None    # (B k,) int64 its index among the trie's query rows (the last edited layer)
    cseg: Optional[torch.Tensor] = None            # (n_requests k + 1,) int64 offsets of the concepts' segments

    def __post_init__(self):
        if self.lookup_node is None:
            self.lookup_node, self.lookup_query, self.cseg = self.trie.lookup_node, self.trie.lookup_in_query, self.seg


def concept_bounds(plan, r: Optional[int] = None):
    """``EncoderEditPlan.concept_bounds`` for anything with ``shard``, ``n_total`` (and ``num_edit_tokens``, default 1)."""
    k = int(getattr(plan, "num_edit_tokens", 1) or 1)
    lo, hi = plan.shard.bounds(plan.n_total // k, r)
    return lo * k, hi * k


def concept_segments(counts, k: int):
    """(perm (B k,), cseg (N k + 1,)) of the pseudo-segments: concept rq k + num gathers the lookups p k + num of the request's
    prompts p, in prompt order (position k s_rq + num c_rq + (p - s_rq) of ``perm``; s: prompt offsets, c: prompt counts)."""
    c = np.asarray(counts, dtype=np.int64)
    s = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    B = int(s[-1])
    req = np.repeat(np.arange(c.size), c)
    w = np.arange(B, dtype=np.int64) - s[req]
    num = np.arange(k, dtype=np.int64)
    perm = np.empty(B * k, dtype=np.int64)
    perm[(k * s[req] + w)[:, None] + num[None, :] * c[req][:, None]] = np.arange(B, dtype=np.int64)[:, None] * k + num[None, :]
    cseg = np.empty(c.size * k + 1, dtype=np.int64)
    cseg[:-1] = (k * s[:-1, None] + num[None, :] * c[:, None]).reshape(-1)
    cseg[-1] = B * k
    return perm, cseg


@dataclass
class EncoderEditPlan:
    """Everything one encoder's Stage-2 pass needs, resident in HBM."""
    text_encoder: torch.nn.Module
    layers: List[int]
    rewrite_module_tmp: str
    lam: float
    edit_weight: float
    batch: Optional[PromptBatch]           # this rank's prompts as one padded batch (hooked-HF forward; built on demand)
    zs_t: torch.Tensor                     # (N, h) fp32: v* of ALL requests, row per request
    covs: Dict[int, torch.Tensor]          # layer -> (d, d) fp32 second moment C
    n_total: int                           # N over all ranks
    shard: ConceptShard = field(default_factory=ConceptShard)
    ws: Optional[hip.EditWorkspace] = None
    dual_ws: Optional[hip.DualWorkspace] = None          # dual (Woodbury) solver state, see run_encoder_edit
    cov_factors: Optional[hip.CovFactors] = None
    side_stream: Optional[torch.cuda.Stream] = None
    solver: str = "auto"                                 # "direct" | "dual" | "auto" (dual when N is well below d)
    graph: Optional[clip_forward.ClipTextGraph] = None   # set -> prefix-deduplicated forward (clip_forward.py)
    chunk: Optional[TrieChunk] = None                    # the prompts on the trie forward (None: hooked-HF forward)
    tokenizer: object = None
    local_requests: Optional[List[Dict]] = None
    zs_pending: object = None
    backups: Optional[Dict[int, torch.Tensor]] = None    # W0 of the edited layers of the last run (failure recovery)
    factor_key: Optional[tuple] = None   # set by a run that factored lam*C' itself: check_info caches the factors if sound
    factors_from_cache: bool = False
    num_edit_tokens: int = 1             # k > 1: k key / value rows per request (last subject token, EOS, padding), n_total = N k
    sweep_factors: Optional[hip.CovFactors] = None       # set by run_sweep: the point's rescaled factors, used as they are
    session: object = None               # set by edit_session.EditSession: the preserved keys (``.keys``: hip.PreservedKeys) of the earlier steps
    retain_weight: Optional[float] = None    # set by EditSession.retain: the pass only ENTERS its keys into the session's set (no targets, no weight written)

    def weight_name(self, layer):
        return f"{self.rewrite_module_tmp.format(layer)}.weight"

    def concept_bounds(self, r: Optional[int] = None):
        """Rank ``r``'s (default: this rank's) rows [lo, hi) of the N k concepts: k times its request range — the request
        split decides everything (a rank's concepts come from its own prompts), so this, not bounds(n_total), sizes every
        K / Zc / v* row block and row-sharded solve."""
        return concept_bounds(self, r)

    @property
    def trie(self):                        # the trie of the prefix-deduplicated forward, None on the hooked-HF path
        return self.chunk.trie if self.chunk is not None and self.graph is not None else None

    @trie.setter
    def trie(self, value):                 # ``plan.graph = plan.trie = None`` switches a plan to the hooked-HF forward
        if value is not None:
            raise AttributeError("assign plan.chunk instead")
        self.chunk = None

    @property
    def chunks(self) -> Optional[List[TrieChunk]]:       # (read-only, for reports that count prompt slices: always one)
        return None if self.chunk is None else [self.chunk]

    @property
    def n_prompts(self) -> int:
        return self.chunk.n_prompts if self.chunk is not None else self.ensure_batch().n_prompts

    @property
    def trie_rows(self):
        return (self.chunk.trie.n_nodes, self.chunk.trie.n_tokens_dense) if self.chunk is not None else None

    def restore_weights(self):
        """Put the edited weights back to the values they had before the last run (W0, kept in ``backups``)."""
        if self.backups is None:
            return
        with torch.no_grad():
            for l, w0 in self.backups.items():
                get_parameter(self.text_encoder, self.weight_name(l)).copy_(w0)

    def resolve_targets(self) -> torch.Tensor:
        """(N, h) fp32 v* rows in HBM.  When prepare was handed the reader thread's future, this is where it is joined:
        at the first solve, i.e. after the forward up to the first edited layer has been launched."""
        if self.zs_pending is not None:
            with phase("vstar join + h2d"):
                with phase("vstar join (wait for the reader)"):
                    zs = self.zs_pending.result() if hasattr(self.zs_pending, "result") else self.zs_pending
                dev = next(self.text_encoder.parameters()).device
                if dev.type == "cuda" and not zs.is_cuda:
                    # through a page-locked staging buffer, asynchronously: a pageable copy would make the host wait for
                    # everything already queued on the stream (the encoder forward this call is meant to run underneath)
                    zs = _pinned_like(zs.to(torch.float32)).to(dev, non_blocking=True)
                else:
                    zs = zs.to(device=dev, dtype=torch.float32).contiguous()
                if zs.shape[0] != self.n_total:
                    raise ValueError(f"v* stack has {zs.shape[0]} rows for {self.n_total} requests")
                self.zs_t, self.zs_pending = zs, None
        return self.zs_t

    def ensure_batch(self) -> PromptBatch:
        if self.batch is None:
            dev = next(self.text_encoder.parameters()).device
            if self.num_edit_tokens > 1:
                self.batch = build_prompt_batch_multi(self.tokenizer, self.local_requests, dev, self.num_edit_tokens)
            else:
                self.batch = build_prompt_batch(self.tokenizer, self.local_requests, dev)
        return self.batch


# ---- state kept across calls (every access under ENGINE_LOCK) --------------------------------------------------------
ENGINE_LOCK = threading.RLock()
_WS_CACHE: "OrderedDict[tuple, list]" = OrderedDict()          # (kind, device, N, d, h) -> reusable f64 workspaces of that shape
_FACTOR_CACHE: "OrderedDict[tuple, tuple]" = OrderedDict()     # see factor_cache_key -> (CovFactors, cov tensors)
WS_CACHE_SIZE = 4
WS_PER_SHAPE = 2


def _factor_cache_size() -> int:
    return int(os.environ.get("EMCID_FACTOR_CACHE", "4"))


def _workspace(kind: str, N: int, d: int, h: int, dev, plan):
    """A workspace (buffers + its device `info` word) LEASED to ``plan`` until its check_info: two plans in flight —
    prepare(A), prepare(B), run(A), run(B), check_info(A) — or two threads never share buffers or a flag word; a plan that
    runs again gets its own workspace back.  A lease whose plan is gone (never checked) is free again."""
    key = (kind, str(dev), N, d, h)
    with ENGINE_LOCK:
        pool = _WS_CACHE.get(key)
        if pool is None:
            pool = _WS_CACHE[key] = []
            while len(_WS_CACHE) > WS_CACHE_SIZE:
                _WS_CACHE.popitem(last=False)
        else:
            _WS_CACHE.move_to_end(key)
        free = None
        for ws in pool:
            holder = ws.lease() if getattr(ws, "lease", None) is not None else None
            if holder is plan:
                return ws
            if holder is None and free is None:
                free = ws
        if free is None:
            free = hip.DualWorkspace(N, d, h, dev) if kind == "dual" else hip.EditWorkspace(N, d, h, dev, lu=kind == "lu")
            if len(pool) < WS_PER_SHAPE:      # beyond that the workspace lives as long as its plan
                pool.append(free)
        free.lease = weakref.ref(plan)
        return free


def _release_workspaces(plan):
    with ENGINE_LOCK:
        for ws in (plan.ws, plan.dual_ws):
            if ws is not None and getattr(ws, "lease", None) is not None and ws.lease() is plan:
                ws.lease = None


def _pinned_like(t: torch.Tensor) -> torch.Tensor:
    """``t`` in page-locked memory: itself when it already is (the native v* reader fills pinned rows), else a copy in a
    buffer from torch's caching host allocator — which keeps a block alive until the asynchronous copies issued from it have
    finished (it records an event per stream use), so two plans prepared back to back never share a staging buffer."""
    if t.is_pinned():
        return t
    buf = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    buf.copy_(t)
    return buf


def factor_cache_key(covs: Sequence[torch.Tensor], lam: float, edit_weight: float) -> tuple:
    """The Cholesky factor of lam*C'_l and its explicit inverse are functions of (the statistics, edit_weight) up to a scalar:
    chol(lam C') = sqrt(lam) chol(C'), so ``lam`` is NOT part of the key — an edit with another mom2_update_weight (the
    reference's most common sweep, experiments/emcid_test.py:924-930, ablation.py:80-83) reuses the factors and hands the
    library the ratio (include/emcid_hip.h, "lam_ratio").  edit_weight stays in the key: C' = fl32(fl32(C (1 - e_w)) / 0.5)
    is rounded per entry in fp32 (reference :1037), which a scalar cannot reproduce.  The statistics are identified by the
    identity and version counter of the HBM-resident C tensors (the entries of emcid_main's covariance cache).
    Reusing a factor across lam changes the weights at fp64-rounding level against a process that factors lam C' itself;
    (A process that wants bit-stable output across runs keeps lam fixed.)"""
    return (tuple((c.device.index, c.data_ptr(), c._version, tuple(c.shape)) for c in covs), float(edit_weight))


def clear_engine_caches():
    with ENGINE_LOCK:
        _WS_CACHE.clear()
        _FACTOR_CACHE.clear()


TIMING: Dict[str, float] = {}      # host seconds per phase of the last prepare/run (diagnostic; scripts/host_profile.py)


class phase:
    """with phase("name"): ... accumulates host wall-clock into TIMING[name]."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.t = time.perf_counter()

    def __exit__(self, *exc):
        TIMING[self.name] = TIMING.get(self.name, 0.0) + time.perf_counter() - self.t
        return False


FORWARD_MODE = "trie"   # "trie": prefix-deduplicated forward when the encoder is a HF CLIP text model; "hf": hooked HF forward
SOLVER = None           # None: plan.solver decides; "direct" / "dual" force it (tests, experiments; env EMCID_SOLVER too)


def _solver_mode(plan) -> str:
    if plan.solver == "lu":          # the fallback after a failed Cholesky overrides every preference
        return "lu"
    return SOLVER or os.environ.get("EMCID_SOLVER") or plan.solver


DUAL_FORMS = ("dual", "dual_apply", "dual_cols", "dual_preserve")


def solver_form(plan, d: int, keep_factors: bool) -> str:
    """Which closed form solves every edited layer of a run:
      "direct"       A = lam C' + K^T K (d x d) factored and solved (edit_layer), optionally keeping adj_k and resid
      "direct_rows"  the same, sharded: every rank factors A, the solves and dW are split by concept rows (edit_layer_shard)
      "lu"           the reference's LU with partial pivoting, the fallback after a failed Cholesky (edit_layer_lu)
      "dual"         the Woodbury form on the factors of lam C' (N x N systems), adj_k and resid kept (edit_layer_dual)
      "dual_apply"   the Woodbury form that only writes the new weights (edit_layer_dual_apply)
      "dual_cols"    dual_apply split by 128-wide column tiles of d over the ranks (edit_layer_dual_cols)
      "dual_preserve" dual_apply of an edit session: the keys of its earlier steps stay preserved (edit_layer_dual_preserve)"""
    mode = _solver_mode(plan)
    if plan.session is not None:
        # (EditSession.apply has already refused what a session does not run: ranks, a forced direct / lu solver, kept factors)
        if mode in ("lu", "direct") or keep_factors or plan.shard.collective:
            raise ValueError(f"an edit session runs the dual solver on one rank (solver {mode!r}, keep_factors={keep_factors})")
        return "dual_preserve"
    if mode == "lu":
        return "lu"
    if mode in ("dual", "direct"):
        dual = mode == "dual"
    else:
        np_, dp = -(-plan.n_total // hip.NB) * hip.NB, -(-d // hip.NB) * hip.NB
        dual = np_ * 5 <= dp * 3      # N x N system + two extra solves pay off when N is well below d
    if dual:
        if keep_factors:
            return "dual"
        # (fewer 128-column tiles than ranks: every rank runs the whole layer itself)
        return "dual_cols" if plan.shard.collective and -(-d // hip.NB) >= plan.shard.world else "dual_apply"
    return "direct_rows" if plan.shard.collective and not keep_factors else "direct"


def prepare_encoder_edit(text_encoder, tokenizer, requests: Sequence[Dict], layers, rewrite_module_tmp, lam,
                         edit_weight, zs_t: torch.Tensor, covs: Dict[int, torch.Tensor],
                         shard: Optional[ConceptShard] = None, layer_module_tmp: Optional[str] = None,
                         forward_mode: Optional[str] = None, num_edit_tokens: int = 1, _defer_checks: bool = True) -> EncoderEditPlan:
    from . import manage_threads
    manage_threads()                    # acts once per process, and only under EMCID_MANAGE_THREADS=1
    shard = shard or ConceptShard()
    device = next(text_encoder.parameters()).device
    lo, hi = shard.bounds(len(requests))
    if len(requests) < shard.world:     # the same verdict on every rank, before any collective can be entered
        raise ValueError(f"{len(requests)} request(s) cannot be sharded over {shard.world} ranks (every rank needs one)")
    local = list(requests[lo:hi])
    mode = forward_mode or FORWARD_MODE
    graph = None
    k = int(num_edit_tokens)
    if k < 1:
        raise ValueError(f"num_edit_tokens must be >= 1, got {k}")
    # k > 1: k rows per request ([last subject token, EOS, k - 2 padding positions], reference compute_z.py:2329-2382 and
    # emcid_main.py:993-1014), N k concepts.  On the trie the rows behind the EOS are query-only leaves (clip_forward.build_trie);
    # the one batch-wide effect of the padding, the padded length longest + k - 2 against the position table, is checked on
    # every rank before anything is launched (_check_padded_length)
    length_checked = k == 1
    if mode == "trie" and layer_module_tmp is not None and device.type == "cuda":
        try:
            with phase("graph"):
                graph = clip_forward.discover_cached(text_encoder, layer_module_tmp)
                for l in layers:   # the edited weights must be the very tensors the explicit forward multiplies with
                    if graph.layers[l].fc2.weight is not get_parameter(text_encoder, f"{rewrite_module_tmp.format(l)}.weight"):
                        raise clip_forward.UnsupportedEncoder("rewrite_module_tmp is not the layer's mlp.fc2")
                if sorted(layers) != list(layers):
                    raise clip_forward.UnsupportedEncoder("layers not in forward order")
        except (clip_forward.UnsupportedEncoder, IndexError, LookupError) as e:
            clip_forward.note_fallback("prepare_encoder_edit", e)
            graph = None
    plan = EncoderEditPlan(text_encoder, list(layers), rewrite_module_tmp, float(lam), float(edit_weight), None,
                           None, covs, len(requests) * k, shard, tokenizer=tokenizer, local_requests=local, num_edit_tokens=k)
    if graph is not None:
        # As soon as the prompts are tokenized their prefix trie is built and the unedited leading layers are LAUNCHED here,
        # so the GPU runs them underneath the rest of the host preparation (v* reads, statistics lookups).  (Cutting the prompt
        # list into slices, each launched before the next is tokenized, measured slower on 2 x EPYC 9575F: every extra tokenizer
        # call costs 3-4 ms of fixed overhead, waking the backend's thread pool, more than the 2.9 ms of GPU time a second
        # slice hides.)
        first_edit = plan.layers[0]
        try:
            # (k > 1: every check of the tokenization up front — a restarted preparation on one rank would pair its collective
            # with another rank's next one)
            with phase("tokenize+lookup"):
                pc = prompt_chunk(tokenizer, local, defer_probe=_defer_checks and k == 1, num_edit_tokens=k)
            if k > 1:
                _check_padded_length(shard, int(pc.eos.max()) + 1, k, graph.position_embedding.num_embeddings, device)
                length_checked = True
                with phase("trie"):
                    pad = getattr(tokenizer, "pad_token_id", None)
                    if pad is None and k > 2:
                        raise ValueError("num_edit_tokens > 2 pads the prompts: the tokenizer has no pad token")
                    perm, cseg = concept_segments(pc.counts, k)
                    offs = pc.request_offsets()
                    trie = clip_forward.build_trie(pc.ids, pc.lookup, device, tail=np.concatenate([offs, cseg, perm]),
                                                   eos=pc.eos, pad_token=int(pad or 0))
                    n1, n2 = offs.size, offs.size + cseg.size
                    seg, cseg_d, perm_d = trie.tail[:n1], trie.tail[n1:n2], trie.tail[n2:]
                    chunk = TrieChunk(trie, seg, pc.n_requests, len(pc.lookup), None, trie.lookup_node.index_select(0, perm_d),
                                      trie.lookup_in_query.index_select(0, perm_d), cseg_d)
            else:
                with phase("trie"):
                    trie = clip_forward.build_trie(pc.ids, pc.lookup, device, tail=pc.request_offsets())
                    chunk = TrieChunk(trie, trie.tail, pc.n_requests, len(pc.lookup))
            with phase("prefix launches"), torch.no_grad():
                hs, x_ln1 = clip_forward.run_prefix(graph, trie, first_edit)
            chunk.state = (first_edit, hs, x_ln1)
            if pc.verify is not None:
                # the checks of the templated tokenization that need not hold the first launch back — the native tokenizer's
                # cross-check against the public tokenizer call, the reference's subject walk against the lookup positions
                # known from the construction of the rows — run now that the GPU has the leading layers to work on.
                # If one says no (a name that also occurs earlier in its prompt; a tokenizer disagreement retires the native
                # twin for good), the preparation starts over with every check up front; what was launched is abandoned.
                with phase("tokenize+lookup"):
                    agreed = pc.verify()
                if not agreed:
                    return prepare_encoder_edit(text_encoder, tokenizer, requests, layers, rewrite_module_tmp, lam, edit_weight,
                                                zs_t, covs, shard, layer_module_tmp, forward_mode, num_edit_tokens,
                                                _defer_checks=False)
            plan.graph, plan.chunk = graph, chunk
            # gauges (not counters): the trie of the last prepared call — rows run per layer and the tokens they stand for
            clip_forward.LAST_PATHS["last_trie_rows"], clip_forward.LAST_PATHS["last_trie_tokens"] = plan.trie_rows
        except (clip_forward.UnsupportedEncoder, IndexError) as e:
            clip_forward.note_fallback("prepare_encoder_edit (prompt batch)", e)
            plan.graph = plan.chunk = None
    if plan.chunk is None:
        with phase("tokenize+lookup"):
            batch = plan.ensure_batch()
        if not length_checked:
            # (the hooked forward pads this rank's prompts to ITS longest + k - 2; the reference pads every prompt to the global one)
            n_pos = getattr(getattr(text_encoder, "config", None), "max_position_embeddings", None)
            _check_padded_length(shard, int(batch.inputs["attention_mask"].sum(dim=1).max().item()), k, n_pos, device)
    # ``zs_t`` / ``covs`` may be callables: the caller's v* cache check and statistics lookups, run HERE — after the leading
    # layers have been launched, so that these host milliseconds too pass underneath the GPU (v* first, as the reference)
    if callable(zs_t) and not hasattr(zs_t, "result"):
        with phase("vstar check"):
            zs_t = zs_t()
    if callable(covs):
        with phase("statistics"):
            covs = covs()
    plan.covs = {l: c.to(device=device, dtype=torch.float32).contiguous() for l, c in covs.items()}
    plan.zs_pending = zs_t          # a tensor, or the caller's reader-thread future: resolved where the first solve needs it
    if not hasattr(zs_t, "result"):
        plan.resolve_targets()
    return plan


def _check_padded_length(shard: ConceptShard, longest: int, k: int, n_positions: Optional[int], device):
    """The reference pads every prompt of a k > 1 edit to (longest + k - 2) tokens (compute_z.py:2329-2360) — the longest over
    ALL requests — and HF's CLIP embeddings refuse a sequence longer than the position table.  Raised on every rank, the same
    verdict everywhere (one MAX all-reduce of the local longest under a collective shard), before anything is launched."""
    if shard.collective:
        import torch.distributed as dist
        dev = torch.device(device)
        t = torch.tensor([int(longest)], dtype=torch.int64,
                         device=dev if dev.type == "cuda" and not _staged(shard.group) else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=shard.group)
        longest = int(t.item())
    if n_positions is not None and longest + k - 2 > int(n_positions):
        raise ValueError(f"Sequence length must be less than max_position_embeddings (got `sequence length`: {longest + k - 2} "
                         f"and max_position_embeddings: {int(n_positions)}): num_edit_tokens = {k} pads the longest prompt "
                         f"({longest} tokens) by {k - 2}")


def _staged(group) -> bool:
    """True when the process group cannot take HBM tensors (gloo): collectives are then staged through host
    memory.  RCCL ("nccl") — the production backend — works on the device buffers directly."""
    import torch.distributed as dist
    return dist.get_backend(group) == "gloo"


# Per-rank phase times of a sharded edit (bench.py --gpus N reports them for every rank, so that a bad scaling curve can be read):
# EMCID_DIST_TIMING=1 (or DIST_TIMING["enabled"] = True) brackets the collectives and every layer's solve with event pairs on
# the launch stream; dist_timing_collect() synchronises and returns {phase: (total ms, count)}.
DIST_TIMING = {"enabled": os.environ.get("EMCID_DIST_TIMING", "0") == "1", "events": []}


class _dist_phase:
    def __init__(self, name: str, dev):
        self.name, self.dev = name, dev
        self.on = DIST_TIMING["enabled"] and torch.device(dev).type == "cuda"

    def __enter__(self):
        if self.on:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        if self.on:
            b = torch.cuda.Event(enable_timing=True)
            b.record(torch.cuda.current_stream(self.dev))
            DIST_TIMING["events"].append((self.name, self.a, b))
        return False


def dist_timing_collect() -> Dict[str, tuple]:
    """{phase: (milliseconds in total, number of brackets)} since the last collect (synchronises the device)."""
    out: Dict[str, list] = {}
    evs, DIST_TIMING["events"] = DIST_TIMING["events"], []
    if evs:
        torch.cuda.synchronize()
    for name, a, b in evs:
        rec = out.setdefault(name, [0.0, 0])
        rec[0] += a.elapsed_time(b)
        rec[1] += 1
    return {k: (v[0], v[1]) for k, v in out.items()}


def _all_reduce_sum(t: torch.Tensor, group):
    import torch.distributed as dist
    # the two all-reduces of the column-sharded solve: the N x N partial S (square) and the h x d partial U
    name = "all_reduce_S" if t.dim() == 2 and t.shape[0] == t.shape[1] else "all_reduce_U"
    with _dist_phase(name, t.device):
        if t.is_cuda and _staged(group):
            host = t.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            t.copy_(host)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


def _all_gather_rows(local: torch.Tensor, plan: EncoderEditPlan) -> torch.Tensor:
    """Concatenate per-rank row blocks (uneven shards allowed) in rank order == request order."""
    sh = plan.shard
    if not sh.collective:
        return local
    import torch.distributed as dist

    with _dist_phase("k_all_gather", local.device):
        return _all_gather_rows_timed(local, plan, sh, dist)


def _all_gather_rows_timed(local, plan, sh, dist):
    sizes = [b - a for a, b in (concept_bounds(plan, r) for r in range(sh.world))]
    nmax = max(sizes)
    padded = local
    if local.shape[0] < nmax:
        padded = torch.zeros(nmax, local.shape[1], dtype=local.dtype, device=local.device)
        padded[:local.shape[0]] = local
    out = torch.empty(sh.world * nmax, local.shape[1], dtype=local.dtype, device=local.device)
    if local.is_cuda and _staged(sh.group):
        host = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(host, padded.cpu().contiguous(), group=sh.group)
        out.copy_(host)
    else:
        dist.all_gather_into_tensor(out, padded.contiguous(), group=sh.group)
    if all(s == nmax for s in sizes):
        return out
    return torch.cat([out[r * nmax:r * nmax + s] for r, s in enumerate(sizes)], dim=0)


def _touch(w: torch.Tensor):
    """The kernels write an edited weight through its raw pointer, which torch's in-place version counter does not see; caches
    keyed by (tensor, version) — the split-fp16 copies of the weights, clip_forward.ClipLayer.split_of — must."""
    torch.autograd.graph.increment_version(w)


def _dual_factors(plan: EncoderEditPlan, form: str, dev):
    """The factors of lam * C'_l of every edited layer for a dual form: L L^T, and the explicit inverses X_l = inv(L_l) that
    turn a layer's two M-solves into two GEMMs.  Returns (fac_done, lazy): per edited layer the event its solve waits for
    (None: the factors came from the cache, nothing to wait for), and whether the solve of layer i builds X of layer i + 1."""
    L = len(plan.layers)
    if plan.sweep_factors is not None:
        # a point of run_sweep: the unit-scale factors of the sweep, rescaled to this point's lam and edit_weight, inverses included
        plan.cov_factors, plan.factors_from_cache = plan.sweep_factors, True
        return None, False
    private = plan.session.private_factors if plan.session is not None else None
    if private is not None:
        # a session that has folded its preserved keys: the factors of lam C' + P^T P, the session's own (edit_session.EditSession.fold)
        plan.cov_factors, plan.factors_from_cache = private, True
        return None, False
    fkey = factor_cache_key([plan.covs[l] for l in plan.layers], plan.lam, plan.edit_weight)
    with ENGINE_LOCK:
        hit = _FACTOR_CACHE.get(fkey) if _factor_cache_size() > 0 and plan.lam > 0 else None
        if hit is not None and not (hit[0].lam and hit[0].lam > 0):
            hit = None
        if hit is not None:
            _FACTOR_CACHE.move_to_end(fkey)
    if hit is not None:
        # lam0 * C'_l = L L^T and X = inv(L) of every edited layer are already in HBM from an earlier edit with the
        # same statistics and edit_weight (any lam0: the solve stages take lam / lam0): every M-solve of this pass is a
        # GEMM against X, nothing is factored but the N x N systems
        plan.cov_factors, plan.factors_from_cache = hit[0], True
        if plan.cov_factors.ready is not None:
            torch.cuda.current_stream(dev).wait_event(plan.cov_factors.ready)
        return None, False
    # lam * C'_l does not depend on the concepts: factor it for ALL edited layers in one batched pass on a side
    # stream, underneath the encoder forward that produces the first layer's keys
    if plan.side_stream is None:
        # high priority: the factorization is a long chain of small dependent kernels; each must get the next
        # free CU ahead of the forward's wide GEMMs or the chain stretches to several times its own length
        plan.side_stream = torch.cuda.Stream(device=dev, priority=-1)
    plan.side_stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(plan.side_stream):
        if plan.cov_factors is not None and plan.cov_factors.cached:
            plan.cov_factors = None        # never refactor into a workspace the cache hands to other edits
        if plan.cov_factors is not None:
            plan.cov_factors.info.zero_()
        plan.cov_factors = hip.factor_cov([plan.covs[l] for l in plan.layers], plan.lam, plan.edit_weight,
                                          plan.cov_factors, inverse=False)
        plan.factor_key = fkey
        chol_done = torch.cuda.Event()
        chol_done.record(plan.side_stream)
        fac_done = [chol_done] * L
        # The first edited layer solves against M by block substitution with L as soon as the factorization is there.
        # The apply-only form builds the explicit inverse of each LATER layer one layer ahead, on the side stream, exactly
        # while the previous layer's solve sits in the latency-bound Cholesky of its N x N system (the chip is idle there).
        # (Building them all right after the factorization, batched underneath the forward, cost the forward more than it
        # hid: HISTORY.md §5.)  The other forms build them here in one batch; the column-sharded solve multiplies by X in
        # every layer, the first one included.
        lazy = form == "dual_apply" and L > 1
        first_x = 0 if form in ("dual_cols", "dual_preserve") else 1      # (these multiply by X in every layer)
        if not lazy and first_x < L:
            hip.cov_inverse(plan.cov_factors, first_x, L - first_x)
            ev = torch.cuda.Event()
            ev.record(plan.side_stream)
            fac_done[first_x:] = [ev] * (L - first_x)
    return fac_done, lazy


def _cache_own_factors(plan: EncoderEditPlan):
    """Hand the factors a plan made itself (``factor_key`` set) to the factor cache, once their flag word read zero."""
    if plan.factor_key is not None and plan.cov_factors is not None and _factor_cache_size() > 0:
        with ENGINE_LOCK:
            plan.cov_factors.cached = True
            _FACTOR_CACHE[plan.factor_key] = (plan.cov_factors, [plan.covs[l] for l in plan.layers])
            while len(_FACTOR_CACHE) > _factor_cache_size():
                _FACTOR_CACHE.popitem(last=False)
        plan.factor_key = None


def session_factors(text_encoder, layers, rewrite_module_tmp: str, lam: float, edit_weight: float, covs: Dict[int, torch.Tensor], dev):
    """The factors of lam C' of every edited layer with their explicit inverses, obtained the way a session step obtains them
    (``_dual_factors``: the factor cache under the key plain calls use, else one batched factorization on the side stream) but
    without a pass — what ``edit_session.EditSession.load`` takes as the coordinates of the rows it loads.  The current stream waits
    for them.  Returns (factors, commit): ``commit()``, to be called once the caller has read ``factors.info`` as zero, hands
    factors made here to the cache as ``check_info`` does (nothing to do after a cache hit)."""
    plan = EncoderEditPlan(text_encoder, list(layers), rewrite_module_tmp, float(lam), float(edit_weight), None, None, covs, 0)
    fac_done, _ = _dual_factors(plan, "dual_preserve", dev)
    if fac_done is not None:
        torch.cuda.current_stream(dev).wait_stream(plan.side_stream)
    return plan.cov_factors, lambda: _cache_own_factors(plan)


def _finish_inverse_factors(plan: EncoderEditPlan, dev):
    """After a pass that factored lam * C' itself: build the explicit inverse factors it did not need (off the critical path,
    on the side stream) so that check_info can hand the complete set to later edits."""
    if plan.factor_key is None or _factor_cache_size() <= 0:
        return
    missing = [i for i in range(len(plan.layers)) if i not in plan.cov_factors.have_inverse]
    if missing:
        plan.side_stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(plan.side_stream):
            for i in missing:
                hip.cov_inverse(plan.cov_factors, i, 1)
            plan.cov_factors.ready = torch.cuda.Event()
            plan.cov_factors.ready.record(plan.side_stream)


def run_encoder_edit(plan: EncoderEditPlan, keep_factors: bool = False, trace: bool = False,
                     restore: bool = False) -> List[LayerEdit]:
    """Device-only Stage 2 for one encoder.  On return the edited fc2 weights hold W0 + dW (``restore=False``)
    or their original values (``restore=True``, the reference's execute_* invariant, emcid_main.py:1076-1078)."""
    te = plan.text_encoder
    L = len(plan.layers)
    mods = {l: get_module(te, plan.rewrite_module_tmp.format(l)) for l in plan.layers}
    weights = {l: get_parameter(te, plan.weight_name(l)) for l in plan.layers}
    for l, w in weights.items():
        if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()):
            raise hip.EmcidHipError(f"{plan.weight_name(l)} must be a contiguous fp32 tensor in HBM "
                                    f"(got {w.dtype} on {w.device})")
    backups = {l: w.detach().clone() for l, w in weights.items()}
    plan.backups = backups
    guard = plan.graph.guard if plan.graph is not None else None
    if guard is not None:
        # the caches this pass runs on (stacked q | k | v, split planes, layer structs) against the BYTES of the live weights:
        # one launch, read back by check_info with the solver's flags (clip_forward.WeightGuard)
        guard.check(plan.graph.layers, plan.layers[-1] + 1)
    d, h = weights[plan.layers[0]].shape[1], weights[plan.layers[0]].shape[0]
    dev = weights[plan.layers[0]].device
    form = solver_form(plan, d, keep_factors)
    edits: List[LayerEdit] = []
    last = plan.layers[-1]
    fac_done, lazy = None, False
    plan.factor_key, plan.factors_from_cache = None, False
    if form in DUAL_FORMS:
        # (a session brings its own workspace, sized by its capacity)
        plan.dual_ws = plan.session.workspace(plan.n_total, d, h, dev, retain=plan.retain_weight is not None) \
            if form == "dual_preserve" else _workspace("dual", plan.n_total, d, h, dev, plan)
        plan.dual_ws.info.zero_()
        fac_done, lazy = _dual_factors(plan, form, dev)
    else:
        plan.ws = _workspace("lu" if form == "lu" else "direct", plan.n_total, d, h, dev, plan)
        plan.ws.info.zero_()
        if form == "lu":
            plan.dual_ws = None

    def solve(i, layer, K_local, Zc_local):
        """All-gather the shard's K/Zc rows, run the closed form, leave W0 + dW in the live weight.  ``Zc_local`` may be
        a callable K -> Zc (fc2 applied to the gathered keys): then only K crosses the links."""
        if plan.retain_weight is not None:
            # a retain list (EditSession.retain): the keys enter the session's preserved set with a zero residual — no Zc, no targets,
            # and the layer's weight is neither read by the solver nor written, so the forward goes on with it as it is
            if fac_done is not None:
                torch.cuda.current_stream(dev).wait_event(fac_done[i])
            hip.session_retain(K_local, plan.cov_factors, i, math.sqrt(plan.retain_weight * plan.edit_weight / 0.5), plan.session.keys,
                               ws=plan.dual_ws, lam=plan.lam)
            edits.append(LayerEdit(layer, plan.weight_name(layer), None, None, None, K_local if trace else None, None))
            return
        try:
            with _dist_phase("solve (incl. its collectives)", dev):
                K = _all_gather_rows(K_local, plan)
                Zc = Zc_local(K) if callable(Zc_local) else _all_gather_rows(Zc_local, plan)
                plan.resolve_targets()
                if fac_done is not None:
                    torch.cuda.current_stream(dev).wait_event(fac_done[i])
                dW, Xt, Rt = _solve(i, layer, K, Zc)
                edits.append(LayerEdit(layer, plan.weight_name(layer), dW, Xt, Rt, K if trace else None, Zc if trace else None))
        finally:
            _touch(weights[layer])

    def _solve(i, layer, K, Zc):
        """The closed form of ``form`` for edited layer ``i``: (dW, adj_k^T | None, resid^T | None)."""
        W0, W = backups[layer], weights[layer].data
        if form == "dual_cols":
            # Every rank holds all N key rows (the K all-gather above).  The layer's GEMMs are split by 128-wide
            # column tiles of d: a rank forms its columns of Yt = Kt X^T and its share of S = I + Yt Yt^T and of
            # U = (Z^T Yt) X; S (N x N) and U (h x d) are summed over the ranks (two all-reduces over xGMI), the
            # N x N Cholesky and the h-row solves are repeated by everyone (latency-bound, no d^2 work in them).
            res = hip.edit_layer_dual_cols(
                K, Zc, plan.zs_t, plan.cov_factors, i, plan.edit_weight, L - i, W0, W,
                hip.column_tiles(plan.shard.rank, plan.shard.world, -(-d // hip.NB)),
                lambda t: _all_reduce_sum(t, plan.shard.group), ws=plan.dual_ws, lam=plan.lam)
            return res["dW"], None, None
        if form == "dual_apply":     # only the edited weights are wanted: the form that never builds adj_k
            def lazy_inverse(nxt=i + 1):
                # stream position: S of layer i is assembled, its Cholesky starts now -> build X of the next layer
                start = torch.cuda.Event()
                start.record(torch.cuda.current_stream(dev))
                plan.side_stream.wait_event(start)
                with torch.cuda.stream(plan.side_stream):
                    hip.cov_inverse(plan.cov_factors, nxt, 1)
                    fac_done[nxt] = torch.cuda.Event()
                    fac_done[nxt].record(plan.side_stream)

            res = hip.edit_layer_dual_apply(K, Zc, plan.zs_t, plan.cov_factors, i, plan.edit_weight, L - i, W0, W,
                                            ws=plan.dual_ws, on_factor_start=lazy_inverse if lazy and i + 1 < L else None,
                                            lam=plan.lam)
            return res["dW"], None, None
        if form == "dual_preserve":
            # the rows of this step land behind the committed ones of the session's state; EditSession.apply commits them
            # for all layers at once after check_info
            res = hip.edit_layer_dual_preserve(K, Zc, plan.zs_t, plan.cov_factors, i, plan.edit_weight, L - i, W0, W,
                                               plan.session.keys, ws=plan.dual_ws, lam=plan.lam)
            if plan.session.report_on:      # the step's readout, from what it left in its workspace: one more launch per layer
                hip.session_step_norms(plan.dual_ws, K.shape[0], d, h, plan.session.keys, out=plan.session.report_row(i, K.shape[0]))
            return res["dW"], None, None
        if form == "dual":
            sharded = plan.shard.collective
            res = hip.edit_layer_dual(
                K, Zc, plan.zs_t, plan.cov_factors, i, plan.edit_weight, L - i, W0=W0, W=W, want_factors=keep_factors,
                ws=plan.dual_ws, rows=plan.concept_bounds() if sharded else None,
                gather_pt=(lambda rows_: _all_gather_rows(rows_.contiguous(), plan)) if sharded else None, lam=plan.lam)
            return res["dW"], (res["adj_k"].t() if res["adj_k"] is not None else None), res["Rt"]
        if form == "lu":
            # the reference's own algorithm (LU with partial pivoting) for a system the Cholesky paths rejected; every
            # rank holds all N key rows here and solves the whole layer itself (rare path, never sharded)
            res = hip.edit_layer_lu(K, Zc, plan.zs_t, plan.covs[layer], plan.lam, plan.edit_weight, L - i,
                                    W0=W0, W=W, want_factors=keep_factors, ws=plan.ws)
            return res["dW"], (res["adj_k"].t() if res["adj_k"] is not None else None), res["Rt"]
        if form == "direct_rows":
            # every rank assembles and factors A from all N concepts; the triangular solves and the dW
            # contraction are split by concept rows and the partial U summed over xGMI (fp64, h*d*8 bytes)
            res = hip.edit_layer_shard(K, Zc, plan.zs_t, plan.covs[layer], plan.lam, plan.edit_weight, L - i,
                                       plan.concept_bounds(), ws=plan.ws)
            _all_reduce_sum(res["U"], plan.shard.group)
            return hip.apply_update_(res["U"], W0, W), None, None
        res = hip.edit_layer(K, Zc, plan.zs_t, plan.covs[layer], plan.lam, plan.edit_weight, L - i,
                             W0=W0, W=W, want_factors=keep_factors, ws=plan.ws)
        return res["dW"], res["Xt"], res["Rt"]

    if plan.chunk is not None and plan.graph is not None:
        ch, order = plan.chunk, {l: i for i, l in enumerate(plan.layers)}
        if sorted(plan.layers) != plan.layers:
            raise RuntimeError("hparams.layers must be in forward order")
        first_edit = plan.layers[0]
        lin = clip_forward.linear
        # the one-call form of an edited layer: single rank, the apply-only dual solver on factors that are already in HBM
        # (a warm call), the split-fp16 forward with its native runner
        fused_run = os.environ.get("EMCID_FUSED_EDIT_LAYER", "1") != "0" and form == "dual_apply" \
            and not plan.shard.collective and plan.factors_from_cache and clip_forward.NATIVE_RUNNER

        def keys(li, x):           # this rank's (N_local k, d) key rows: per-concept means at the lookup rows of its prompts
            if isinstance(x, hip.SplitRows):       # split-fp16 path: the keys come from the fp32 twin fc1's epilogue wrote
                x = x.float()
            idx = ch.lookup_query if li == last else ch.lookup_node
            return hip.gather_mean(x.unsqueeze(0).expand(idx.numel(), -1, -1), idx, ch.cseg)

        def fused_layer_ok(li, x):
            if not (fused_run and isinstance(x, hip.SplitRows) and x.f32 is not None and x.f32.is_contiguous()):
                return False
            gl = plan.graph.layers[li]
            if gl.fc2 is not mods[li] or gl.fc2.bias is None:
                return False
            return clip_forward.native_of(plan.graph, ch.trie, li, li + 1) is not None

        def on_fc2(li, x, out, mid=None, next_ln=None):
            """fc2 of an edited layer: keys -> closed form -> fc2(x) + mid with the NEW weight (the add riding in the GEMM's
            epilogue); with the native layer runner the (hs, LN1 planes of the next layer) pair from ONE C call (``next_ln``:
            that LayerNorm, or None)."""
            if li not in order:
                return out
            m = mods[li]
            if fused_layer_ok(li, x):
                # keys, Zc, the solve, the new weight's planes and fc2 + residual + the next LN1: ONE C call
                # (csrc/clip_layers.hip: emcid_clip_edit_layer_tail_sp16)
                i = order[li]
                nat = clip_forward.native_of(plan.graph, ch.trie, li, li + 1)
                plan.resolve_targets()
                w = weights[li]
                try:
                    res = hip.clip_edit_layer_tail(
                        nat.array, li, nat.h, nat.d, x, mid, ch.lookup_query if li == last else ch.lookup_node,
                        ch.cseg, plan.zs_t, plan.cov_factors, i, plan.edit_weight, L - i, backups[li], w.data, plan.dual_ws,
                        plan.lam, next_ln, last=li == last)
                finally:
                    _touch(w)
                if li != last:      # the layer's fc2 planes were re-split in place from the new weight: keep the cache entry
                    gl = plan.graph.layers[li]
                    gl.splits["fc2"] = ((id(gl.fc2.weight), gl.fc2.weight._version, gl.fc2.weight.data_ptr()), gl.splits["fc2"][1])
                    if gl.guard is not None:
                        gl.guard.store(gl.index, "fc2", gl.fc2.weight)
                edits.append(LayerEdit(li, plan.weight_name(li), res["dW"], None, None, res["K"] if trace else None,
                                       res["Zc"] if trace else None))
                clip_forward.LAST_PATHS["fused_edit_layers"] = clip_forward.LAST_PATHS.get("fused_edit_layers", 0) + 1
                return None if li == last else (res["hs"], res["x"])
            # fc2 is affine, so the mean over a request's prompts of its output at the lookup rows IS fc2 of the mean
            # key: Zc = K W^T + b on N rows (to fp32 rounding) instead of fc2 over every node followed by a gather
            # (on the split-fp16 kernel against the planes of the weight as it is now, like the fused call above)
            solve(order[li], li, keys(li, x), lambda K_all: lin(K_all, m.weight, m.bias, wsp=plan.graph.layers[li].split_of("fc2")))
            if li == last:
                return None
            wsp = plan.graph.layers[li].split_of("fc2")          # of the NEW weight (solve() bumped its version counter)
            if wsp is not None and isinstance(x, hip.SplitRows):
                nat = clip_forward.native_of(plan.graph, ch.trie, li, li + 1)
                if nat is not None:        # fc2 + residual add + the next layer's LN1: one C call
                    return hip.clip_layer_tail(nat.array, li, nat.h, nat.d, x, mid, next_ln)
            return lin(x, m.weight, m.bias, residual=mid, wsp=wsp)

        with torch.no_grad():
            # the unedited leading layers: already launched by prepare (underneath the host's tokenization), else here
            if ch.state is not None and ch.state[0] == first_edit:
                state = ch.state[1:]
            else:
                state = clip_forward.run_prefix(plan.graph, ch.trie, first_edit)
            ch.state = None         # single use: the residual stream below belongs to the weights of this very call
            clip_forward.LAST_PATHS["forward_trie"] += 1
            clip_forward.run_layers_from(plan.graph, ch.trie, state, first_edit, last, on_fc2, fc2_by_callback=order,
                                         edit_callback=True)
    else:
        def make_hook(i, layer):
            def hook(mod, inputs, output):
                x = inputs[0]
                solve(i, layer, gather_request_means(x, plan.ensure_batch()),
                      None if plan.retain_weight is not None else gather_request_means(output, plan.ensure_batch()))
                if layer == last:
                    raise StopForward()
                return clip_forward.linear(x.reshape(-1, x.shape[-1]), mod.weight, mod.bias).reshape(*x.shape[:-1], -1) \
                    if x.is_cuda and x.dtype == torch.float32 else F.linear(x, mod.weight, mod.bias)
            return hook

        clip_forward.LAST_PATHS["forward_hf"] += 1
        handles = [mods[l].register_forward_hook(make_hook(i, l)) for i, l in enumerate(plan.layers)]
        try:
            with torch.no_grad(), hip_attention(te):
                try:
                    te(**plan.ensure_batch().inputs)
                except StopForward:
                    pass
        finally:
            for hd in handles:
                hd.remove()
    if len(edits) != L:
        raise RuntimeError(f"only {len(edits)} of {L} edited layers were reached by the forward pass "
                           f"(hparams.layers must be in forward order)")
    _finish_inverse_factors(plan, dev)
    if restore:
        plan.restore_weights()
    if guard is not None:
        guard.flush()       # fingerprints of every weight a cache entry was made from in this pass (the edited fc2's as they are NOW)
    return edits


# ---- many (mom2_update_weight, edit_weight) pairs over one prepared plan ------------------------------------------------------------
# The system of a pair is A = a C + b K K^T with a = 2 lam (1 - e), b = 2 e (reference emcid_main.py:1030-1050: C (1 - e) / 0.5, keys
# and residuals times sqrt(e / 0.5)).  Nothing of the preparation depends on the pair, nor does chol(C): chol(a C) = sqrt(a) chol(C).

def sweep_factor_cache_key(covs: Sequence[torch.Tensor]) -> tuple:
    """The key of a sweep's unit-scale factors chol(C_l), inv(chol(C_l)) in the factor cache: the statistics alone — neither lam nor
    edit_weight (``factor_cache_key`` keeps edit_weight: a single call factors the fp32-rounded C' of the reference)."""
    return ("sweep", tuple((c.device.index, c.data_ptr(), c._version, tuple(c.shape)) for c in covs))


def validate_grid(grid) -> List[tuple]:
    """``grid`` as a list of (mom2_update_weight, edit_weight) float pairs, or ValueError: empty, not pairs, mom2_update_weight <= 0
    or not finite, edit_weight outside (0, 1) (e = 1 makes a = 0: no Cholesky factor to rescale; e = 0 edits nothing)."""
    try:
        pts = [(float(p[0]), float(p[1])) for p in grid] if all(len(p) == 2 for p in grid) else None
    except (TypeError, ValueError, IndexError) as e:
        raise ValueError(f"grid must be a sequence of (mom2_weight, edit_weight) pairs: {e}") from e
    if pts is None:
        raise ValueError("grid must be a sequence of (mom2_weight, edit_weight) pairs")
    if not pts:
        raise ValueError("grid is empty")
    for lam, e in pts:
        if not (np.isfinite(lam) and lam > 0.0):
            raise ValueError(f"mom2_weight must be positive and finite in a sweep (got {lam})")
        if not (0.0 < e < 1.0):
            raise ValueError(f"edit_weight must lie inside (0, 1) in a sweep (got {e})")
    return pts


def _sweep_unit_factors(plan: EncoderEditPlan, dev) -> Optional[hip.CovFactors]:
    """chol(C_l) and its explicit inverse for every edited layer, from the factor cache or factored here (lam = 1, edit_weight = 0.5:
    C' = fl32(fl32(C 0.5) / 0.5) = C exactly), checked with one host synchronisation per sweep.  None: C is not positive definite."""
    covs = [plan.covs[l] for l in plan.layers]
    key = sweep_factor_cache_key(covs)
    with ENGINE_LOCK:
        hit = _FACTOR_CACHE.get(key) if _factor_cache_size() > 0 else None
        if hit is not None:
            _FACTOR_CACHE.move_to_end(key)
    if hit is not None:
        if hit[0].ready is not None:
            torch.cuda.current_stream(dev).wait_event(hit[0].ready)
        return hit[0]
    unit = hip.factor_cov(covs, 1.0, 0.5, None, inverse=True)
    clip_forward.LAST_PATHS["sweep_cov_factorizations"] += len(covs)
    if int(unit.info.item()) != 0:
        return None
    if _factor_cache_size() > 0:
        with ENGINE_LOCK:
            unit.cached = True
            _FACTOR_CACHE[key] = (unit, covs)
            while len(_FACTOR_CACHE) > _factor_cache_size():
                _FACTOR_CACHE.popitem(last=False)
    return unit


def validate_pair_grid(grid) -> List[tuple]:
    """``grid`` as a list of (mom2_update_weight, mom2_update_weight_2, edit_weight) float triples for the SDXL pair of encoders,
    or ValueError: ``validate_grid``'s refusals per component — empty, an entry that is not a triple (a pair included), a
    mom2_update_weight of either encoder <= 0 or not finite, edit_weight outside (0, 1)."""
    try:
        pts = [(float(p[0]), float(p[1]), float(p[2])) for p in grid] if all(len(p) == 3 for p in grid) else None
    except (TypeError, ValueError, IndexError) as e:
        raise ValueError(f"grid must be a sequence of (mom2_weight, mom2_weight_2, edit_weight) triples: {e}") from e
    if pts is None:
        raise ValueError("grid must be a sequence of (mom2_weight, mom2_weight_2, edit_weight) triples")
    if not pts:
        raise ValueError("grid is empty")
    for lam1, lam2, e in pts:
        validate_grid([(lam1, e), (lam2, e)])
    return pts


def pair_grid_plan(triples):
    """(pts1, pts2, combos) of a validated grid of triples: the two encoders are independent models, so TE1's weights depend on
    (lam1, e) alone and TE2's on (lam2, e).  ``pts1``: the distinct (lam1, e) in order of first appearance, ``pts2``: the distinct
    (lam2, e); ``combos[g]`` = (index in pts1, index in pts2) of triple g.  Host only."""
    pts1, pts2, combos = [], [], []
    seen1, seen2 = {}, {}
    for lam1, lam2, e in triples:
        i = seen1.setdefault((lam1, e), len(pts1))
        if i == len(pts1):
            pts1.append((lam1, e))
        j = seen2.setdefault((lam2, e), len(pts2))
        if j == len(pts2):
            pts2.append((lam2, e))
        combos.append((i, j))
    return pts1, pts2, combos


class SweepWalk:
    """The points of a sweep over ONE prepared plan, one at a time (``run_sweep`` is a loop over this; a sweep over the SDXL pair
    steps two of them side by side).

        with SweepWalk(plan) as walk:            # the shared part: solver form, the state entering the first edited layer,
            edits = walk.point(lam, e)           # chol(C) at unit scale; then per point: rescale, run, check, LU rerun if need be
            ...                                  # the point's weights are in place; ``edits`` are its LayerEdits (dW per layer)
            plan.restore_weights()               # before the next point
                                                 # on exit, also by an exception: weights, lam, edit_weight, solver put back

    ``point`` returns the LayerEdits of the run whose weights are in place — those of the LU rerun when the point took it.  It
    counts LAST_PATHS sweep_points / sweep_cov_factorizations / sweep_prefix_runs up; whoever walks resets them."""

    def __init__(self, plan: EncoderEditPlan):
        if plan.chunk is None or plan.graph is None:
            raise clip_forward.UnsupportedEncoder("run_sweep replays the prefix-trie forward's state")
        self.plan, self.saved = plan, (plan.lam, plan.edit_weight, plan.solver)
        self.unit = self.scaled = self.state = self.form = self.pinned = None

    def __enter__(self):
        plan, LP = self.plan, clip_forward.LAST_PATHS
        ch, first_edit = plan.chunk, plan.layers[0]
        w0 = get_parameter(plan.text_encoder, plan.weight_name(first_edit))
        dev, d = w0.device, w0.shape[1]
        try:
            with phase("sweep: shared"), torch.no_grad():
                form = solver_form(plan, d, False)          # once: N, d and the shard decide, not the pair
                pinned = "dual" if form in DUAL_FORMS else form if form == "lu" else "direct"
                self.state = ch.state if ch.state is not None and ch.state[0] == first_edit else \
                    (first_edit,) + tuple(clip_forward.run_prefix(plan.graph, ch.trie, first_edit))
                LP["sweep_prefix_runs"] += 1
                self.unit = _sweep_unit_factors(plan, dev) if form in DUAL_FORMS else None
                if form in DUAL_FORMS and self.unit is None:
                    # C itself has a non-positive pivot: so has a C for every pair.  Every point is a single call's fallback.
                    logging.getLogger("emcid_amd").warning("the statistics are not positive definite: every point of the sweep runs "
                                                           "on the pivoted-LU solver")
                    if os.environ.get("EMCID_LU_FALLBACK", "1") == "0":
                        raise FloatingPointError("the statistics are not positive definite (non-positive pivot in chol(C))")
                    pinned = "lu"
                self.form, self.pinned = form, pinned
        except BaseException:
            self.close()
            raise
        return self

    def point(self, lam: float, e: float) -> List[LayerEdit]:
        plan, LP = self.plan, clip_forward.LAST_PATHS
        with phase("sweep: points"):
            plan.lam, plan.edit_weight, plan.solver = lam, e, self.pinned
            if self.unit is not None:
                self.scaled = hip.cov_factor_rescale(self.unit, 2.0 * lam * (1.0 - e), self.scaled, lam=lam, edit_weight=e)
                plan.sweep_factors = self.scaled
            elif self.pinned == "lu" and self.form != "lu":
                LP["lu_fallbacks"] = LP.get("lu_fallbacks", 0) + 1
            plan.chunk.state = self.state
            edits = run_encoder_edit(plan)
            try:
                check_info(plan)
            except FloatingPointError as err:
                plan.sweep_factors = None
                plan.chunk.state = self.state
                edits = rerun_with_lu(plan, err)
            LP["sweep_points"] += 1
        return edits

    def close(self):
        plan = self.plan
        plan.restore_weights()
        plan.lam, plan.edit_weight, plan.solver = self.saved
        plan.sweep_factors = plan.cov_factors = None
        plan.chunk.state = None

    def __exit__(self, *exc):
        self.close()
        return False


def run_sweep(plan: EncoderEditPlan, grid, visit=None) -> list:
    """Stage 2 of ONE prepared plan at every (mom2_update_weight, edit_weight) pair of ``grid``, in order.  While a point's edited
    weights are in place ``visit(index, (lam, e))`` is called; its return values are the result.  The weights are back at their
    original values between the points and on return (also when ``visit`` raises).

    Shared by the points: the plan (tokenization, trie, v* rows), the residual stream entering the first edited layer (the prefix
    launched by prepare, replayed: run_layers_from only reads it), the choice of the solver, and one factorization of the statistics
    at unit scale — a point rescales it into its own workspace (hip.cov_factor_rescale) and then runs the chain of a single call on
    warm factors: run_layers_from, the fused edit-layer call, check_info, rerun_with_lu for a point whose Cholesky reports a pivot
    (that point only).  The per-point body is ``SweepWalk``.  LAST_PATHS gauges of the last sweep: sweep_points,
    sweep_cov_factorizations (len(layers) for a dual form on a cold cache, 0 on cached unit factors or for the direct form, which
    assembles A from C itself), sweep_prefix_runs (1)."""
    pts = validate_grid(grid)
    walk = SweepWalk(plan)
    LP = clip_forward.LAST_PATHS
    LP["sweep_points"] = LP["sweep_cov_factorizations"] = LP["sweep_prefix_runs"] = 0
    for key in ("sweep_pair_points_1", "sweep_pair_points_2", "sweep_pair_combos"):      # (a pair sweep's gauges: not of this sweep)
        LP.pop(key, None)
    results = []
    with walk:
        for index, (lam, e) in enumerate(pts):
            walk.point(lam, e)
            results.append(visit(index, (lam, e)) if visit is not None else None)
            plan.restore_weights()
    return results


def solver_info(plan: EncoderEditPlan) -> int:
    """One host sync: 0, or 1 + the column of the first non-positive pivot any factorization of the last run met."""
    infos = [holder.info for holder in (plan.ws, plan.dual_ws, plan.cov_factors) if holder is not None]
    guard = plan.graph.guard if getattr(plan, "graph", None) is not None else None
    plan.stale_weights = False
    if guard is not None:
        if infos and infos[0].is_cuda and infos[0].device == guard.flag.device:
            infos = infos + [guard.flag]          # the stale-cache flag rides in the same read-back
        else:
            plan.stale_weights = bool(int(guard.flag.item()))
            guard = None
    if not infos:
        return 0
    if len(infos) == 1 or not infos[0].is_cuda:
        vals = [int(t.item()) for t in infos]
    else:       # all the flag words through ONE synchronisation: asynchronous copies into a pinned buffer, then one stream sync
        dev = infos[0].device
        host = torch.empty(len(infos), dtype=infos[0].dtype, pin_memory=True)
        for i, t in enumerate(infos):
            host[i:i + 1].copy_(t.reshape(-1)[:1], non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        vals = [int(v) for v in host.tolist()]
    if guard is not None:
        plan.stale_weights = bool(vals.pop())
    return next((v for v in vals if v != 0), 0)


def run_checked(plan: EncoderEditPlan, keep_factors: bool = False, restore: bool = False) -> List[LayerEdit]:
    """run_encoder_edit + check_info with the reference's fallback semantics (``rerun_with_lu``)."""
    edits = run_encoder_edit(plan, keep_factors=keep_factors, restore=restore)
    try:
        check_info(plan)
    except FloatingPointError as err:
        edits = rerun_with_lu(plan, err, keep_factors=keep_factors, restore=restore)
    return edits


def rerun_with_lu(plan: EncoderEditPlan, err: FloatingPointError, keep_factors: bool = False,
                  restore: bool = False) -> List[LayerEdit]:
    """After check_info raised ``err`` (a Cholesky factorization met a non-positive pivot: lam*C' + K K^T not positive
    definite, e.g. statistics that lost definiteness in fp32; the weights are already back): rerun the whole pass with LU +
    partial pivoting — torch.linalg.solve's algorithm (reference emcid_main.py:1045), which returns numbers for any
    nonsingular system — and check it.  EMCID_LU_FALLBACK=0 raises ``err`` instead."""
    if os.environ.get("EMCID_LU_FALLBACK", "1") == "0" or plan.solver == "lu":
        raise err
    plan.solver = "lu"
    plan.cov_factors = None
    clip_forward.LAST_PATHS["lu_fallbacks"] = clip_forward.LAST_PATHS.get("lu_fallbacks", 0) + 1
    logging.getLogger("emcid_amd").warning("a Cholesky factorization met a non-positive pivot: the pass is rerun with the pivoted-LU solver")
    edits = run_encoder_edit(plan, keep_factors=keep_factors, restore=restore)
    check_info(plan)
    return edits


def check_info(plan: EncoderEditPlan, restore_on_failure: bool = True):
    """One host sync at the very end: did any factorization meet a non-positive pivot?  If so the edited weights hold
    garbage: they are put back to the values they had before the run, then FloatingPointError is raised (callers that can
    retry — emcid_main — catch it and rerun with the pivoted-LU solver, the reference's own semantics)."""
    code = solver_info(plan)          # (a host synchronisation: nothing of this plan's run is still using its workspaces)
    _release_workspaces(plan)
    if getattr(plan, "stale_weights", False):
        # a weight was rewritten without its version counter moving: this pass ran on planes of the OLD bytes
        plan.restore_weights()
        clip_forward.invalidate_weight_caches(plan.text_encoder)
        plan.factor_key, plan.graph = None, None
        raise clip_forward.StaleWeightCacheError(
            "an encoder weight was written in a way torch's version counter does not see (param.data.copy_/add_, a raw pointer) "
            "after the forward's caches were made from it; the edited weights have been put back and the caches dropped — call "
            "again (emcid_main's entry points do so by themselves), and bump the counter or call "
            "emcid_amd.invalidate_weight_caches(text_encoder) after such writes")
    if code != 0 and plan.solver == "lu":
        if restore_on_failure:
            plan.restore_weights()
        raise torch.linalg.LinAlgError(
            f"lam*C + K K^T is singular to working precision (zero pivot at column {code - 1} of the pivoted LU): "
            f"torch.linalg.solve (reference emcid_main.py:1045) raises for this system too; the edited weights have been restored")
    if code == 0:
        _cache_own_factors(plan)
        return
    if plan.factor_key is not None:
        plan.factor_key = None
        plan.cov_factors = None
    if restore_on_failure:
        plan.restore_weights()
    raise FloatingPointError(
        f"lam*C + K K^T is not positive definite (non-positive pivot at column {code - 1}); the reference's LU "
        f"(torch.linalg.solve, emcid_main.py:1045) returns numbers for an indefinite system — the edited weights have been "
        f"restored; rerun with solver='lu' (emcid_main does so by itself) or check the statistics file / mom2_update_weight")

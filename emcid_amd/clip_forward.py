"""Prefix-deduplicated ("trie") forward of a HF CLIP text encoder for the K/Z assembly.

The reference forwards every prompt of every request in full, twice per edited layer
(emcid/compute_z.py:2296-2308 via emcid/emcid_main.py:987,:1004).  Mass-edit prompts are a handful of templates
times many concept names, so most token positions are shared causal prefixes ("<bos> painting by ...").  A causal
text encoder's state at a token depends only on the tokens before it; here every DISTINCT prefix is a node of a
trie and is computed once:

    rows            = trie nodes (unique (prefix, token) pairs up to each prompt's lookup token)
    embeddings      = token_embedding[token[u]] + position_embedding[depth[u]]
    per layer       = LN1 -> q/k/v projections (row-wise GEMMs) -> attention over the ancestor chain
                      (csrc/attention.hip: tree_attention_f32) -> out_proj -> +res -> LN2 -> fc1 -> act -> fc2 -> +res
    edited layer    = K / Zc gathered at the prompts' lookup nodes, closed form solved, fc2 recomputed with W_new
    last edited one = only the lookup nodes go through q/attention/out_proj/MLP (k/v still for every node)

Same arithmetic as the HF module tree (its own weights, LayerNorm eps, activation), only fewer rows; results
match the hooked HF forward to fp32 rounding (tests/test_e2e_gpu.py).  Encoders that do not look like HF's
CLIPTextModel raise ``UnsupportedEncoder`` and the engine falls back to the hooked HF forward.
"""
import os
import weakref
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import hip
from .nethook import get_module


class UnsupportedEncoder(Exception):
    pass


OWN_GEMM = os.environ.get("EMCID_OWN_GEMM", "1") != "0"     # 0: torch's F.linear (hipBLASLt) + separate element-wise passes
# 1 (default): the projections run on the split-fp16 kernel (csrc/gemm_sp16.hip: fp32 operands as hi + lo fp16 planes, three f16
# MFMAs per k-step, fp32 accumulate — fp32-level accuracy at 3/16 of the f32-MFMA issue time); 0: the exact-f32 MFMA kernel
SPLIT_GEMM = os.environ.get("EMCID_SPLIT_GEMM", "1") != "0"
# Which path ran (counters of this process; ``emcid_amd.LAST_PATHS`` is this dict): projections on the split-fp16 kernel / the
# exact-f32 kernel / torch's F.linear; layers issued by the native runner; forwards that took the trie / the hooked HF encoder;
# trie forwards that had to FALL BACK to the hooked HF encoder (each one is also logged once per reason).  sweep_*: gauges of the
# last sweep_emcid_text_encoder (edit_engine.run_sweep): its points, the covariance factorizations it ran, its prefix runs.
# session_*: gauges of the last EditSession operation (edit_session.EditSession, written by its _publish alone from the table
# edit_session._GAUGES): its steps so far and preserved concept rows; its folds and the rows they took into the session's base
# factor; the rows its retain lists added (EditSession.retain), folded ones included; session_loaded_rows appears with a load.
# session_rescales: hip.session_rescale calls of the session so far (rescale, reweight, the points of a sweep; one per edited layer);
# session_sweep_points: the points the last EditSession.sweep ran.
# score_replays: replays of the trie forward made by an emcid_main.EditScorer (its construction and every score()).
# sweep_pair_points_1, sweep_pair_points_2, sweep_pair_combos: present while the last sweep was a sweep_emcid_sdxl_text_encoders —
# the encoder edits it ran on TE1 and on TE2, and its triples; edit_engine.run_sweep takes them out again.
LAST_PATHS = {"linear_sp16": 0, "linear_f32": 0, "linear_torch": 0, "native_layers": 0, "fused_edit_layers": 0, "forward_trie": 0,
              "forward_hf": 0, "forward_hf_fallback": 0, "sweep_points": 0, "sweep_cov_factorizations": 0, "sweep_prefix_runs": 0,
              "session_steps": 0, "session_preserved_rows": 0, "session_folds": 0, "session_folded_rows": 0,
              "session_retained_rows": 0, "session_released_rows": 0, "score_replays": 0,
              "session_rescales": 0, "session_sweep_points": 0}
_FALLBACK_SEEN = set()


def note_fallback(where: str, why: Exception):
    """A trie forward that could not run and took the hooked HF forward instead: counted, and logged once per (place, reason)."""
    import logging
    LAST_PATHS["forward_hf_fallback"] += 1
    key = (where, type(why).__name__, str(why))
    if key not in _FALLBACK_SEEN:
        _FALLBACK_SEEN.add(key)
        logging.getLogger("emcid_amd").warning("%s: the prefix-trie forward is not available (%s: %s); using the hooked HF "
                                               "forward (its projections still run on the library's GEMM)", where,
                                               type(why).__name__, why)


def split_ok(w: torch.Tensor) -> bool:
    return SPLIT_GEMM and OWN_GEMM and hip.split_supported(w)


def linear(x, w: torch.Tensor, b: Optional[torch.Tensor] = None, act=None, act_code: Optional[int] = None,
           residual: Optional[torch.Tensor] = None, wsp: Optional["hip.SplitRows"] = None,
           planes_scale: Optional[torch.Tensor] = None, want_f32: bool = True):
    """act(x @ w.T + b) + residual for the row-wise projections of the forward.  ``wsp`` (the weight as a split-fp16 matrix,
    ``ClipLayer.split_of``): the split-fp16 kernel (csrc/gemm_sp16.hip), x an fp32 row matrix (split here) or already a
    ``hip.SplitRows``; ``planes_scale`` asks for the result as a SplitRows for the next projection (with its fp32 twin
    unless ``want_f32=False``).
    Otherwise the library's exact-f32 MFMA GEMM (csrc/gemm_f32.hip) with bias / activation / residual add in its epilogue
    whenever the operands allow it (fp32, HBM, K % 16 == 0); otherwise — and under EMCID_OWN_GEMM=0 — torch's F.linear and
    separate passes."""
    fusable = (b is None or b.is_contiguous()) and (act is None or act_code is not None) and \
        (residual is None or (residual.stride(1) == 1 and residual.dtype == torch.float32))
    if wsp is not None and fusable and (isinstance(x, hip.SplitRows) or hip.split_supported(x)):
        xs = x if isinstance(x, hip.SplitRows) else hip.split_rows(x)
        LAST_PATHS["linear_sp16"] += 1
        return hip.linear_sp(xs, wsp, b, act=act_code if act is not None else hip.ACT_NONE, residual=residual,
                             planes_scale=planes_scale, want_f32=want_f32)
    if isinstance(x, hip.SplitRows):
        x = x.float()
    if OWN_GEMM and hip.linear_supported(x, w) and (b is None or b.is_contiguous()) and \
            (residual is None or (residual.stride(1) == 1 and residual.dtype == torch.float32)):
        LAST_PATHS["linear_f32"] += 1
        if act is None or act_code is not None:
            return hip.linear(x, w, b, act=act_code if act is not None else hip.ACT_NONE, residual=residual)
        y = act(hip.linear(x, w, b))
        return y if residual is None else residual + y
    LAST_PATHS["linear_torch"] += 1
    y = F.linear(x, w, b)
    if act is not None:
        y = act(y)
    return y if residual is None else residual + y


def norm_of(x: torch.Tensor, ln, wsp: Optional["hip.SplitRows"] = None, want_f32: bool = False, scale_output: bool = False):
    """LayerNorm(x) on the library's kernel when it fits, else the module itself.  ``wsp`` (the split weight of the projection
    that consumes the result): the result as a ``hip.SplitRows`` written by the LayerNorm kernel itself (``scale_output``: with
    the per-row scale under which that projection may write its own output as planes)."""
    if _fusable(ln) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1:
        if wsp is not None and _sp_ln_ok(ln):
            return hip.add_layernorm_sp(x, None, ln, want_f32=want_f32, bound=wsp.bound if scale_output else None)[1]
        return hip.add_layernorm(x, None, ln)[1]
    return ln(x)


def _sp_ln_ok(ln) -> bool:
    return ln.normalized_shape[0] % 32 == 0 and ln.normalized_shape[0] <= 2048


class StaleWeightCacheError(RuntimeError):
    """An encoder weight was rewritten behind the caches' back (``param.data.copy_(...)``, a raw-pointer write): the planes
    the forward just ran on were stale.  The edit engine restores the edited weights, drops the encoder's caches and raises
    this; the public entry points of ``emcid_main`` catch it once and redo the call (single process)."""


WEIGHT_GUARD = os.environ.get("EMCID_WEIGHT_GUARD", "1") != "0"
GUARD_SLOTS = 6            # per layer: q, k, v (the stacked snapshot is cut from them), out, fc1, fc2
_GUARD_SLOT = {"q": 0, "k": 1, "v": 2, "out": 3, "fc1": 4, "fc2": 5}


class WeightGuard:
    """Content guard of the weight-derived caches of ONE encoder (include/emcid_hip.h, "stale-cache guard"): a device table with
    one {address, bytes, fingerprint} entry per cached weight, written when a cache entry is made (``store``), and a device flag
    that ``check`` raises when a cached weight's BYTES no longer match — torch's version counter, which the caches are keyed by,
    does not see ``param.data`` writes.  The check is one launch per edit call; the flag is read back with the call's final
    synchronisation (``edit_engine.check_info``).  Host side: the address and size every slot was stored with, so that a slot
    whose tensor has since been replaced is emptied instead of dereferenced.
    Scope: the WEIGHTS of the six projections per layer, on the edit entry points (``edit_engine.run_encoder_edit``), whose graph
    is cached across calls.  Stage 0 (``layer_stats``) and UCE (``uce_train``) build a fresh graph per call
    (``clip_forward.discover``), so their cache entries are made from the live weights inside the call and need no guard.
    Biases, LayerNorm parameters and embeddings are read live by every launch (nothing is cached from them but the stacked
    q|k|v bias and fc1's row bound, which follow the weights' version counters): a ``.data`` write to a bias alone is the one
    case not covered."""

    def __init__(self, n_layers: int, device):
        self.n = n_layers * GUARD_SLOTS
        self.table = torch.zeros(self.n, 4, dtype=torch.int64, device=device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = [None] * self.n          # (data_ptr, bytes, version counter) of the tensor each filled slot was stored from
        self.pending = {}                    # slot -> tensor: fingerprints still to be taken (``flush``)

    def store(self, layer: int, name: str, w: torch.Tensor):
        """Note that a cache entry was just made from ``w``.  The fingerprint itself is taken by ``flush`` — ONE launch for
        everything noted since the last one, at the end of the forward / edit that made the entries (an edited layer's fc2
        is noted twice per call, before and after its edit: the later note wins, and the bytes are read after both)."""
        nbytes = w.numel() * w.element_size()
        slot = layer * GUARD_SLOTS + _GUARD_SLOT[name]
        self.pending.pop(slot, None)
        if not (w.is_cuda and w.is_contiguous() and nbytes % 16 == 0 and w.data_ptr() % 16 == 0 and w.device == self.table.device):
            self.host[slot] = None
            return
        self.pending[slot] = w
        self.host[slot] = (w.data_ptr(), nbytes, w._version)

    def flush(self):
        if self.pending:
            hip.fingerprint_store([(w.detach(), slot) for slot, w in self.pending.items()], self.table)
            self.pending.clear()

    def check(self, layers, hi: int):
        """Zero the flag and launch the comparison for the slots of layers [0, hi) whose cache entries this call will TRUST: the
        tensor a slot was stored from is still the live parameter, at the same address, with the same version counter.  Any other
        slot is masked out — its cache entry misses on the counter (or identity) anyway and is rebuilt, with a fresh
        fingerprint, before it is used; its table entry may point at memory that is no longer there and is never looked at."""
        self.flush()        # (entries made earlier in this very call, by the leading layers' launches)
        self.flag.zero_()
        n = min(hi, len(layers)) * GUARD_SLOTS
        skip = []
        for i in range(min(hi, len(layers))):
            l = layers[i]
            for k, m in enumerate((l.q, l.k, l.v, l.out, l.fc1, l.fc2)):
                slot = i * GUARD_SLOTS + k
                h = self.host[slot]
                if h is None:
                    skip.append(slot)
                    continue
                w = m._parameters.get("weight")      # None: re-parametrized / wrapped since (weight-norm, LoRA, pruning)
                if w is None or not w.is_cuda or w.data_ptr() != h[0] or w.numel() * w.element_size() != h[1] or w._version != h[2]:
                    skip.append(slot)
        for first in range(0, n, 256):
            cnt = min(256, n - first)
            hip.fingerprint_check(self.table, first, cnt, self.flag, [s - first for s in skip if first <= s < first + cnt])


@dataclass
class ClipLayer:
    ln1: torch.nn.LayerNorm
    q: torch.nn.Linear
    k: torch.nn.Linear
    v: torch.nn.Linear
    out: torch.nn.Linear
    ln2: torch.nn.LayerNorm
    fc1: torch.nn.Linear
    act: object
    fc2: torch.nn.Linear
    heads: int
    scale: float
    qkv_w: Optional[torch.Tensor] = None   # [3h, h] rows of q, k, v stacked: one projection GEMM instead of three
    qkv_b: Optional[torch.Tensor] = None
    act_code: Optional[int] = None         # hip.ACT_* when the activation can ride in the fc1 GEMM's epilogue
    splits: Optional[dict] = None          # name -> (weight id, version, data_ptr, hip.SplitRows): the weights as split-fp16 planes
    guard: Optional[object] = None         # WeightGuard of the encoder + this layer's index: every cache entry made from a
    index: int = -1                        # weight leaves the fingerprint of the weight's bytes there

    def fuse_qkv(self):
        """Snapshot q/k/v into one stacked weight (they are never edited by this path; call again if they change)."""
        with torch.no_grad():
            self.qkv_w = torch.cat([self.q.weight, self.k.weight, self.v.weight], 0).contiguous()
            if self.q.bias is not None and self.k.bias is not None and self.v.bias is not None:
                self.qkv_b = torch.cat([self.q.bias, self.k.bias, self.v.bias], 0).contiguous()
        if self.splits is not None:
            self.splits.pop("qkv", None)
        if self.guard is not None:
            for name in ("q", "k", "v"):
                self.guard.store(self.index, name, getattr(self, name).weight)

    def split_of(self, name: str) -> Optional["hip.SplitRows"]:
        """The weight ``name`` (qkv | q | k | v | out | fc1 | fc2) as a split-fp16 matrix, made once per weight version: the
        cache entry is checked against the tensor's identity, in-place version counter and address (code that writes a
        weight through its raw pointer — the edit engine — bumps the counter, ``edit_engine._touch``).  None: the split
        kernel does not take this weight (EMCID_SPLIT_GEMM=0, K % 32, not fp32 in HBM)."""
        w = self.qkv_w if name == "qkv" else getattr(self, name).weight
        if w is None or not split_ok(w):
            return None
        if self.splits is None:
            self.splits = {}
        sig = (id(w), w._version, w.data_ptr())
        hit = self.splits.get(name)
        if hit is not None and hit[0] == sig:
            return hit[1]
        b = self.qkv_b if name == "qkv" else getattr(self, name).bias
        with torch.no_grad():        # the (max row norm, max |bias|) pair only where a LayerNorm turns it into an output scale: fc1
            sp = hip.split_rows(w.detach(), b if b is not None and b.is_contiguous() else None, want_bound=name == "fc1")
        self.splits[name] = (sig, sp)
        if self.guard is not None and name in ("out", "fc1", "fc2"):
            self.guard.store(self.index, name, w)
        return sp


@dataclass
class ClipTextGraph:
    token_embedding: torch.nn.Embedding
    position_embedding: torch.nn.Embedding
    layers: List[ClipLayer]
    final_layer_norm: Optional[torch.nn.LayerNorm] = None
    native: Optional[object] = None        # NativeLayers: the layers as the C structs of the layer runner (csrc/clip_layers.hip)
    guard: Optional[WeightGuard] = None    # content guard of everything cached from this encoder's weights


NATIVE_RUNNER = os.environ.get("EMCID_NATIVE_LAYERS", "1") != "0"     # 0: one ctypes call per launch (the A/B path)


class NativeLayers:
    """The encoder's layers as an array of ``emcid_clip_layer_sp16`` for the native layer runner: ONE C call per run of layers
    instead of one ctypes call (and two tensor allocations) per launch.  ``ready(lo, hi)`` (re)fills the entries of layers
    [lo, hi) whose weights changed (ClipLayer.split_of's version check) and says whether all of them can take the runner: split
    weights for q | k | v (stacked), out, fc1, fc2; affine LayerNorms the fused kernel takes; an activation the GEMM epilogue
    knows.  The tensors the structs point to are kept alive here."""

    def __init__(self, graph: "ClipTextGraph"):
        self.n = len(graph.layers)
        self.array = (hip.ClipLayerSp16 * self.n)()
        self.sigs = [None] * self.n
        self.quick = [None] * self.n       # identity / version / address of everything a filled struct was made from
        self.keep = [None] * self.n
        l0 = graph.layers[0]
        self.h, self.d, self.heads, self.scale = l0.q.out_features, l0.fc1.out_features, l0.heads, l0.scale

    def _fill(self, i: int, layer: ClipLayer) -> bool:
        if layer.qkv_w is None or layer.act_code is None and layer.act is not None:
            return False
        # nothing the struct was made from has moved or been written since it was filled (a call checks 7-12 layers before its
        # first launch: 4 us each this way, 36 through the checks below)
        quick = tuple((id(w), w._version, w.data_ptr()) for w in (layer.qkv_w, layer.out.weight, layer.fc1.weight, layer.fc2.weight)) + \
            tuple(t.data_ptr() if t is not None else 0 for t in (layer.qkv_b, layer.out.bias, layer.fc1.bias, layer.fc2.bias,
                                                                 layer.ln1.weight, layer.ln1.bias, layer.ln2.weight, layer.ln2.bias)) + \
            (layer.act_code, layer.ln1.eps, layer.ln2.eps)
        if self.quick[i] == quick and self.sigs[i] is not None:
            return True
        self.quick[i] = None
        if not (_fusable(layer.ln1) and _fusable(layer.ln2) and _sp_ln_ok(layer.ln1) and _sp_ln_ok(layer.ln2)):
            return False
        if (layer.q.out_features, layer.fc1.out_features, layer.heads, layer.scale) != (self.h, self.d, self.heads, self.scale):
            return False
        sps = [layer.split_of(n) for n in ("qkv", "out", "fc1", "fc2")]
        if any(sp is None for sp in sps):
            return False
        biases = [layer.qkv_b, layer.out.bias, layer.fc1.bias, layer.fc2.bias]
        if any(b is not None and not (b.is_contiguous() and b.dtype == torch.float32 and b.is_cuda) for b in biases):
            return False
        lns = [layer.ln1.weight, layer.ln1.bias, layer.ln2.weight, layer.ln2.bias]
        if any(t.dtype != torch.float32 or not t.is_contiguous() for t in lns):
            return False
        sig = tuple((sp.planes.data_ptr(), sp.inv_scale.data_ptr(), sp.bound.data_ptr() if sp.bound is not None else 0) for sp in sps) + \
            tuple(t.data_ptr() if t is not None else 0 for t in biases + lns) + (layer.act_code,)
        if self.sigs[i] == sig:
            self.quick[i] = quick
            return True
        e = self.array[i]
        ptr = lambda t: t.data_ptr() if t is not None else None
        e.ln1_gamma, e.ln1_beta, e.ln2_gamma, e.ln2_beta = (ptr(t) for t in lns)
        e.ln1_eps, e.ln2_eps = float(layer.ln1.eps), float(layer.ln2.eps)
        for name, sp, b in zip(("qkv", "out", "fc1", "fc2"), sps, biases):
            setattr(e, name + "_planes", ptr(sp.planes))
            setattr(e, name + "_inv_scale", ptr(sp.inv_scale))
            setattr(e, name + "_bias", ptr(b))
        e.fc1_bound = ptr(sps[2].bound)
        e.act = int(layer.act_code) if layer.act is not None else 0
        self.keep[i] = (sps, biases, lns)
        self.sigs[i] = sig
        self.quick[i] = quick
        return True

    def ready(self, graph: "ClipTextGraph", lo: int, hi: int) -> bool:
        if not (NATIVE_RUNNER and SPLIT_GEMM and OWN_GEMM):
            return False
        return all(self._fill(i, graph.layers[i]) for i in range(lo, hi))


def native_of(graph: ClipTextGraph, trie: "TokenTrie", lo: int, hi: int) -> Optional[NativeLayers]:
    """The graph's NativeLayers when layers [lo, hi) and this trie can take the native runner, else None."""
    if not (NATIVE_RUNNER and SPLIT_GEMM and OWN_GEMM) or hi <= lo or not graph.layers:
        return None
    if graph.native is None:
        graph.native = NativeLayers(graph)
    nat = graph.native
    if trie.anc.dtype != torch.int32 or trie.depth.dtype != torch.int32 or \
            not hip.tree_attention_sp_supported(trie.anc, nat.heads, nat.h // nat.heads):
        return None
    return nat if nat.ready(graph, lo, hi) else None


def discover(text_encoder, layer_module_tmp: str) -> ClipTextGraph:
    """Resolve the sub-modules by the hparams' own name templates (``layer_module_tmp``) and HF CLIP attribute names."""
    try:
        root = getattr(text_encoder, "text_model", text_encoder)
        emb = root.embeddings
        tok_e, pos_e = emb.token_embedding, emb.position_embedding
        n_layers = len(root.encoder.layers)
        layers = []
        for i in range(n_layers):
            lm = get_module(text_encoder, layer_module_tmp.format(i))
            at, mlp = lm.self_attn, lm.mlp
            heads = int(at.num_heads)
            hd = at.q_proj.out_features // heads
            if hd > 64 or hd % 4:
                raise UnsupportedEncoder(f"head_dim {hd} not supported by the tree-attention kernel")
            act = mlp.activation_fn
            act_code = None
            if type(act).__name__ == "QuickGELUActivation":
                act, act_code = hip.quick_gelu, hip.ACT_QUICK_GELU
            elif type(act).__name__ == "GELUActivation" and getattr(act, "act", None) is F.gelu:
                act_code = hip.ACT_GELU_ERF            # transformers' "gelu": torch's exact (erf) form
            layers.append(ClipLayer(lm.layer_norm1, at.q_proj, at.k_proj, at.v_proj, at.out_proj, lm.layer_norm2,
                                    mlp.fc1, act, mlp.fc2, heads, float(getattr(at, "scale", hd ** -0.5)), act_code=act_code))
        for l in layers:
            for m in (l.q, l.k, l.v, l.out, l.fc1, l.fc2):
                if not isinstance(m, torch.nn.Linear):
                    raise UnsupportedEncoder("projection is not nn.Linear")
        guard = None
        if WEIGHT_GUARD and layers and layers[0].q.weight.is_cuda:
            guard = WeightGuard(n_layers, layers[0].q.weight.device)
            for i, l in enumerate(layers):
                l.guard, l.index = guard, i
        for l in layers:
            if (l.q.bias is None) == (l.k.bias is None) == (l.v.bias is None) and l.q.weight.is_cuda:
                l.fuse_qkv()
        return ClipTextGraph(tok_e, pos_e, layers, getattr(root, "final_layer_norm", None), guard=guard)
    except (AttributeError, LookupError, TypeError) as e:
        raise UnsupportedEncoder(str(e))


_GRAPHS = weakref.WeakKeyDictionary()      # text_encoder -> (layer_module_tmp, signature, ClipTextGraph)


def _graph_signature(graph: ClipTextGraph) -> tuple:
    """Identity + in-place version of the tensors the stacked q|k|v snapshots were cut from."""
    sig = []
    for l in graph.layers:
        for m in (l.q, l.k, l.v):
            params = m._parameters          # (nn.Module.__getattr__ costs ~1 us per access; this runs on every edit call)
            w, b = params["weight"], params.get("bias")
            sig.append((id(w), w._version, w.data_ptr()))
            if b is not None:
                sig.append((id(b), b._version, b.data_ptr()))
    return tuple(sig)


def invalidate_weight_caches(text_encoder=None):
    """Forget everything derived from an encoder's weights — the stacked q | k | v snapshots, the split-fp16 planes and the native
    runner's structs (all encoders when ``text_encoder`` is None).  The caches follow a weight by tensor identity, address and
    torch's in-place version counter; code that rewrites a weight in a way the counter does not see (``param.data.add_(...)``, a raw
    pointer) calls this afterwards — or bumps the counter itself (``torch.autograd.graph.increment_version``), as the edit
    engine does for the weights its kernels write."""
    if text_encoder is None:
        _GRAPHS.clear()
        return
    try:
        _GRAPHS.pop(text_encoder, None)
    except TypeError:
        pass


def discover_cached(text_encoder, layer_module_tmp: str) -> ClipTextGraph:
    """``discover`` once per encoder object: the module walk and the stacked q|k|v copies are reused by later edits as long
    as the q/k/v parameters are the same tensors and have not been written in place (their version counters)."""
    try:
        hit = _GRAPHS.get(text_encoder)
    except TypeError:
        return discover(text_encoder, layer_module_tmp)
    if hit is not None and hit[0] == layer_module_tmp:
        try:
            if _graph_signature(hit[2]) == hit[1]:
                return hit[2]
        except AttributeError:
            pass
    graph = discover(text_encoder, layer_module_tmp)
    _GRAPHS[text_encoder] = (layer_module_tmp, _graph_signature(graph), graph)
    return graph


@dataclass
class TokenTrie:
    """Unique causal prefixes of a prompt batch (host-built, device-resident index arrays)."""
    token: torch.Tensor        # (U,) int64
    depth: torch.Tensor        # (U,) int32  position id of the node
    anc: torch.Tensor          # (U, Dmax) int32 ancestor chain root..node (padded with 0)
    lookup_node: torch.Tensor  # (B,) int64 node of each prompt's lookup token
    query_rows: torch.Tensor   # (R,) int32 distinct lookup nodes (sorted)
    lookup_in_query: torch.Tensor  # (B,) int64 index of each prompt's lookup node inside query_rows
    n_nodes: int               # distinct prefixes (the arrays above are padded to a multiple of ROW_BUCKET rows)
    n_tokens_dense: int        # B * S the dense forward would process
    tail: Optional[torch.Tensor] = None   # the caller's own int64 array uploaded with the trie (build_trie(tail=...))
    max_token: int = -1        # largest token id (host copy; -1: not recorded) — range check of the fused embedding kernel
    position: Optional[torch.Tensor] = None   # (U,) int32 own position of every node: ``depth`` itself except on the query-only
                                              # leaves of a multi-token trie (build_trie(eos=...)), where it is EOS + j
    max_position: int = -1     # largest position (host copy; -1: not recorded)

    def __post_init__(self):
        if self.position is None:
            self.position = self.depth
        if self.max_position < 0:
            self.max_position = int(self.anc.shape[1]) - 1


ROW_BUCKET = 256   # node / query-row counts are padded to a multiple of this: a few GEMM shapes per encoder, not one per batch


def build_trie(input_ids, lookup: Sequence[int], device, bucket: int = ROW_BUCKET, tail: Optional[np.ndarray] = None,
               eos: Optional[np.ndarray] = None, pad_token: int = 0) -> TokenTrie:
    """Trie of the prompts' prefixes up to each lookup token.  ``input_ids``: (B, S) array (or equal-length rows).
    Nodes are numbered by depth, then by (parent, token).  Built by ``libemcid_host.so`` (``emcid_trie_build``: one packed image
    in pinned memory, ONE asynchronous upload) when that library is there, else level by level with numpy
    (``build_trie_numpy``: six pageable uploads) — same arrays either way (tests/test_host_cpu.py).
    ``eos`` (B,) given: the num_edit_tokens = k > 1 trie (``emcid_trie_build_leaves``): ``lookup`` is (B, k), every prompt's
    chain runs through its EOS, and lookups behind the EOS are query-only leaves (token ``pad_token``, the EOS node's chain and
    depth, own position EOS + j; include/emcid_host.h).  ``lookup_node`` / ``lookup_in_query`` then have B k entries, row-major."""
    if eos is not None:
        return _build_trie_leaves(input_ids, lookup, device, bucket, tail, eos, pad_token)
    tok = np.asarray(input_ids, dtype=np.int64)
    if tok.ndim != 2:
        raise UnsupportedEncoder("prompt rows of unequal length")
    lk = np.asarray(lookup, dtype=np.int64)
    B = tok.shape[0]
    dmax = int(lk.max()) + 1
    if dmax > 128:
        raise UnsupportedEncoder("prompt longer than 128 tokens")
    from . import host_text
    if host_text.available() and B > 0 and int(lk.min()) >= 0 and dmax <= tok.shape[1] and int(tok[:, :dmax].min()) >= 0:
        dev = torch.device(device)

        extra = np.ascontiguousarray(tail, dtype=np.int64) if tail is not None else None
        sizes = {}

        def alloc(nbytes):
            # ``tail`` (the caller's own int64 index array, e.g. the request segment offsets) rides behind the trie image in the
            # same pinned buffer: one upload for everything
            sizes["trie"] = (nbytes + 7) // 8 * 8
            buf = torch.empty(sizes["trie"] + (extra.nbytes if extra is not None else 0), dtype=torch.uint8,
                              pin_memory=(dev.type == "cuda"))
            return buf, buf.data_ptr()

        host, z = host_text.build_trie_packed(tok, lk, bucket, alloc)
        if extra is not None:
            host[sizes["trie"]:].view(torch.int64).copy_(torch.from_numpy(extra))
        img = host.to(dev, non_blocking=True)
        U, n, R, D = z["U"], z["n"], z["R_pad"], z["dmax"]
        o32 = 8 * (U + 2 * n)
        tail_dev = img[sizes["trie"]:].view(torch.int64) if extra is not None else None
        return TokenTrie(img[:8 * U].view(torch.int64), img[o32:o32 + 4 * U].view(torch.int32),
                         img[o32 + 4 * (U + R):o32 + 4 * (U + R + U * D)].view(torch.int32).view(U, D),
                         img[8 * U:8 * (U + n)].view(torch.int64), img[o32 + 4 * U:o32 + 4 * (U + R)].view(torch.int32),
                         img[8 * (U + n):o32].view(torch.int64), z["n_real"], B * tok.shape[1], tail_dev,
                         int(tok[:, :dmax].max()))
    t = build_trie_numpy(tok, lk, device, bucket)
    t.max_token = int(tok[:, :dmax].max())
    if tail is not None:
        t.tail = torch.from_numpy(np.ascontiguousarray(tail, dtype=np.int64)).to(device)
    return t


def _build_trie_leaves(input_ids, lookup, device, bucket: int, tail: Optional[np.ndarray], eos, pad_token: int) -> TokenTrie:
    tok = np.asarray(input_ids, dtype=np.int64)
    if tok.ndim != 2:
        raise UnsupportedEncoder("prompt rows of unequal length")
    lk = np.asarray(lookup, dtype=np.int64)
    eos = np.asarray(eos, dtype=np.int64).reshape(-1)
    B = tok.shape[0]
    if lk.ndim != 2 or lk.shape[0] != B or eos.shape[0] != B or B == 0:
        raise ValueError("a multi-token trie takes (B, k) lookups and (B,) EOS positions")
    dmax = int(eos.max()) + 1
    if dmax > 128:
        raise UnsupportedEncoder("prompt longer than 128 tokens")
    if int(eos.min()) < 0 or dmax > tok.shape[1] or int(lk.min()) < 0 or int(pad_token) < 0:
        raise ValueError("EOS or lookup position outside the prompt rows")
    read = tok[:, :dmax][np.arange(dmax)[None, :] <= eos[:, None]]          # the tokens of the chains
    max_token = max(int(read.max()), int(pad_token)) if (lk > eos[:, None]).any() else int(read.max())
    max_position = int(max(int(lk.max()), dmax - 1))
    from . import host_text
    if host_text.available() and int(read.min()) >= 0:
        dev = torch.device(device)
        extra = np.ascontiguousarray(tail, dtype=np.int64) if tail is not None else None
        sizes = {}

        def alloc(nbytes):
            sizes["trie"] = (nbytes + 7) // 8 * 8
            buf = torch.empty(sizes["trie"] + (extra.nbytes if extra is not None else 0), dtype=torch.uint8,
                              pin_memory=(dev.type == "cuda"))
            return buf, buf.data_ptr()

        host, z = host_text.build_trie_packed(tok, lk, bucket, alloc, eos=eos, pad_token=int(pad_token))
        if extra is not None:
            host[sizes["trie"]:].view(torch.int64).copy_(torch.from_numpy(extra))
        img = host.to(dev, non_blocking=True)
        U, n, R, D = z["U"], z["n"], z["R_pad"], z["dmax"]
        o32 = 8 * (U + 2 * n)
        op = o32 + 4 * (U + R + U * D)
        return TokenTrie(img[:8 * U].view(torch.int64), img[o32:o32 + 4 * U].view(torch.int32),
                         img[o32 + 4 * (U + R):op].view(torch.int32).view(U, D),
                         img[8 * U:8 * (U + n)].view(torch.int64), img[o32 + 4 * U:o32 + 4 * (U + R)].view(torch.int32),
                         img[8 * (U + n):o32].view(torch.int64), z["n_real"], B * tok.shape[1],
                         img[sizes["trie"]:].view(torch.int64) if extra is not None else None, max_token,
                         img[op:op + 4 * U].view(torch.int32), max_position)
    t = build_trie_numpy(tok, lk, device, bucket, eos=eos, pad_token=pad_token)
    t.max_token, t.max_position = max_token, max_position
    if tail is not None:
        t.tail = torch.from_numpy(np.ascontiguousarray(tail, dtype=np.int64)).to(device)
    return t


def build_trie_numpy(tok: np.ndarray, lk: np.ndarray, device, bucket: int = ROW_BUCKET, eos: Optional[np.ndarray] = None,
                     pad_token: int = 0) -> TokenTrie:
    """``build_trie`` with numpy: one ``np.unique`` over (parent, token) keys per position."""
    if eos is not None:
        return _build_trie_leaves_numpy(tok, lk, device, bucket, eos, pad_token)
    B = tok.shape[0]
    dmax = int(lk.max()) + 1
    vocab = int(tok[:, :dmax].max()) + 1
    node_of = np.full(B, -1, dtype=np.int64)
    tokens, parents, levels = [], [], []
    total = 0
    for p in range(dmax):
        alive = np.nonzero(lk >= p)[0] if p else np.arange(B)
        key = (node_of[alive] + 1) * vocab + tok[alive, p]
        uniq, inverse = np.unique(key, return_inverse=True)
        node_of[alive] = total + inverse
        tokens.append(uniq % vocab)
        parents.append(uniq // vocab - 1)
        levels.append(np.arange(total, total + uniq.size))
        total += uniq.size
    n_real = total
    pad = (-n_real) % bucket if bucket > 1 else 0
    U = n_real + pad
    token = np.concatenate(tokens + [np.full(pad, tokens[0][0], dtype=np.int64)])
    parent = np.concatenate(parents)
    depth = np.zeros(U, dtype=np.int32)
    anc = np.zeros((U, dmax), dtype=np.int32)
    for p, ids in enumerate(levels):          # parents of level p are complete: copy their chains, append self
        depth[ids] = p
        if p:
            anc[ids, :p] = anc[parent[ids], :p]
        anc[ids, p] = ids
    # padding nodes: copies of the root token at depth 0 that attend to themselves; nothing ever looks them up
    anc[n_real:, 0] = np.arange(n_real, U)
    ln = node_of                                   # node of each prompt's lookup token (its last alive level)
    q_rows, inverse = np.unique(ln, return_inverse=True)
    if bucket > 1 and len(q_rows) % bucket:       # query rows of the last layer: repeat the first one as padding
        q_rows = np.concatenate([q_rows, np.full((-len(q_rows)) % bucket, q_rows[0], dtype=q_rows.dtype)])
    return TokenTrie(torch.from_numpy(token).to(device), torch.from_numpy(depth).to(device),
                     torch.from_numpy(anc).to(device), torch.from_numpy(ln).to(device),
                     torch.from_numpy(q_rows.astype(np.int32)).to(device),
                     torch.from_numpy(inverse.astype(np.int64)).to(device), n_real, B * tok.shape[1])


def _build_trie_leaves_numpy(tok: np.ndarray, lk: np.ndarray, device, bucket: int, eos: np.ndarray, pad_token: int) -> TokenTrie:
    """The numpy twin of ``emcid_trie_build_leaves`` (same numbering: the chains level by level, then the leaves by (EOS node,
    j), then the padding nodes)."""
    tok = np.asarray(tok, dtype=np.int64)
    lk = np.asarray(lk, dtype=np.int64)
    eos = np.asarray(eos, dtype=np.int64).reshape(-1)
    B, k = lk.shape
    dmax = int(eos.max()) + 1
    vocab = int(tok[:, :dmax][np.arange(dmax)[None, :] <= eos[:, None]].max()) + 1
    node_of = np.full(B, -1, dtype=np.int64)
    node_at = np.full((B, dmax), -1, dtype=np.int64)      # node of every prompt at every level of its chain
    tokens, parents, levels = [], [], []
    total = 0
    for p in range(dmax):
        alive = np.nonzero(eos >= p)[0]
        key = (node_of[alive] + 1) * vocab + tok[alive, p]
        uniq, inverse = np.unique(key, return_inverse=True)
        node_of[alive] = total + inverse
        node_at[alive, p] = node_of[alive]
        tokens.append(uniq % vocab)
        parents.append(uniq // vocab - 1)
        levels.append(np.arange(total, total + uniq.size))
        total += uniq.size
    n_chain = total
    behind = lk > eos[:, None]
    j = np.where(behind, lk - eos[:, None], 0)
    lf_key = node_of[:, None] * (int(j.max()) + 1) + j          # (EOS node, distance), ordered as the pair
    lf_uniq, lf_inv = np.unique(lf_key[behind], return_inverse=True)
    n_leaf = lf_uniq.size
    lf_eos = lf_uniq // (int(j.max()) + 1)
    lf_j = lf_uniq % (int(j.max()) + 1)
    n_real = n_chain + n_leaf
    pad = (-n_real) % bucket if bucket > 1 else 0
    U = n_real + pad
    token = np.concatenate(tokens + [np.full(n_leaf, pad_token, dtype=np.int64), np.full(pad, tokens[0][0], dtype=np.int64)])
    parent = np.concatenate(parents)
    depth = np.zeros(U, dtype=np.int32)
    anc = np.zeros((U, dmax), dtype=np.int32)
    for p, ids in enumerate(levels):
        depth[ids] = p
        if p:
            anc[ids, :p] = anc[parent[ids], :p]
        anc[ids, p] = ids
    leaf_ids = np.arange(n_chain, n_real)
    depth[leaf_ids] = depth[lf_eos]
    anc[leaf_ids] = anc[lf_eos]
    position = depth.copy()
    position[leaf_ids] = depth[lf_eos] + lf_j
    anc[n_real:, 0] = np.arange(n_real, U)
    ln = np.where(behind, 0, node_at[np.arange(B)[:, None], np.minimum(lk, dmax - 1)])
    ln[behind] = n_chain + lf_inv
    ln = ln.reshape(-1)
    q_rows, inverse = np.unique(ln, return_inverse=True)
    if bucket > 1 and len(q_rows) % bucket:
        q_rows = np.concatenate([q_rows, np.full((-len(q_rows)) % bucket, q_rows[0], dtype=q_rows.dtype)])
    return TokenTrie(torch.from_numpy(token).to(device), torch.from_numpy(depth).to(device),
                     torch.from_numpy(anc).to(device), torch.from_numpy(ln).to(device),
                     torch.from_numpy(q_rows.astype(np.int32)).to(device),
                     torch.from_numpy(inverse.reshape(-1).astype(np.int64)).to(device), n_real, B * tok.shape[1],
                     position=torch.from_numpy(position).to(device), max_position=int(position.max()))


def build_trie_packed(seqs: Sequence[Sequence[int]], device, bucket: int = ROW_BUCKET, return_nodes: bool = False):
    """Trie over WHOLE token sequences (Stage 0: every attended token of every caption is a lookup), built level by level
    with numpy — the Python loop of ``build_trie`` costs ~1 us per token, too slow for millions of caption tokens.

    Returns (TokenTrie, count): ``count[u]`` = number of sequences that pass through node u, i.e. how many (caption,
    position) pairs the node's row stands for; the rows are a multiset of size ``count.sum()`` = total tokens.
    ``lookup_node`` / ``query_rows`` / ``lookup_in_query`` are empty: every node is wanted.
    ``return_nodes``: also return the (n, lmax) int64 array of the node of every (sequence, position), -1 past the end."""
    n = len(seqs)
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=n)
    lmax = int(lens.max())
    if lmax > 128:
        raise UnsupportedEncoder("sequence longer than 128 tokens")
    tok = np.zeros((n, lmax), dtype=np.int64)
    for i, s in enumerate(seqs):
        tok[i, :len(s)] = s
    vocab = int(tok.max()) + 1
    node_of = np.full(n, -1, dtype=np.int64)          # node of each sequence at the previous level
    nodes = np.full((n, lmax), -1, dtype=np.int64) if return_nodes else None
    tokens, parents, depths, counts, level_nodes = [], [], [], [], []
    total = 0
    for p in range(lmax):
        alive = np.nonzero(lens > p)[0]
        if alive.size == 0:
            break
        key = (node_of[alive] + 1) * vocab + tok[alive, p]           # (parent, token) as one integer
        uniq, inverse, cnt = np.unique(key, return_inverse=True, return_counts=True)
        ids = total + np.arange(uniq.size)
        node_of[alive] = ids[inverse]
        if return_nodes:
            nodes[alive, p] = node_of[alive]
        tokens.append(uniq % vocab)
        parents.append(uniq // vocab - 1)
        depths.append(np.full(uniq.size, p, dtype=np.int32))
        counts.append(cnt)
        level_nodes.append(ids)
        total += uniq.size
    token = np.concatenate(tokens)
    parent = np.concatenate(parents)
    depth = np.concatenate(depths)
    count = np.concatenate(counts)
    n_real = total
    pad = (-n_real) % bucket if bucket > 1 else 0
    U = n_real + pad
    anc = np.zeros((U, lmax), dtype=np.int32)
    for p, ids in enumerate(level_nodes):             # parents of level p are complete: copy their chains, append self
        if p:
            anc[ids, :p] = anc[parent[ids], :p]
        anc[ids, p] = ids
    if pad:
        token = np.concatenate([token, np.full(pad, token[0])])
        depth = np.concatenate([depth, np.zeros(pad, dtype=np.int32)])
        anc[n_real:, 0] = np.arange(n_real, U)
    empty64 = torch.zeros(0, dtype=torch.int64, device=device)

    def up(a):
        # through page-locked memory, asynchronously: a pageable upload makes the host wait for everything already queued on the
        # stream — the previous pool's forward and Gram launches, under which the host is meant to prepare this pool
        t = torch.from_numpy(np.ascontiguousarray(a))
        if torch.device(device).type == "cuda":
            return t.pin_memory().to(device, non_blocking=True)
        return t.to(device)

    trie = TokenTrie(up(token), up(depth.astype(np.int32)), up(anc), empty64, torch.zeros(0, dtype=torch.int32, device=device),
                     empty64, n_real, n * lmax)
    count_t = up(count.astype(np.float32))
    return (trie, count_t, nodes) if return_nodes else (trie, count_t)


def _check_fp32(graph: ClipTextGraph):
    w = graph.layers[0].fc2.weight
    if not (w.is_cuda and w.dtype == torch.float32):
        raise hip.EmcidHipError(f"the trie forward runs fp32 in HBM (got {w.dtype} on {w.device})")


def embed(graph: ClipTextGraph, trie: TokenTrie) -> torch.Tensor:
    return graph.token_embedding(trie.token) + graph.position_embedding(trie.position.long())


def _fusable(ln) -> bool:
    return isinstance(ln, torch.nn.LayerNorm) and ln.weight is not None and ln.bias is not None and \
        ln.weight.is_cuda and ln.normalized_shape[0] % 4 == 0 and ln.normalized_shape[0] <= 8192


def layer_attention_block(layer: ClipLayer, hs: torch.Tensor, trie: TokenTrie, rows: Optional[torch.Tensor],
                          x_ln1=None, want_f32: bool = False):
    """hs (U, h) -> (residual stream after the attention block, LN2 of it), for every node (rows None) or the query
    rows only.  ``x_ln1``: LN1(hs) when the previous layer's residual add already produced it (fp32, or a ``hip.SplitRows``
    on the split-fp16 path).  On that path LN2's result is a SplitRows as well (``want_f32``: with its fp32 twin), carrying the
    scale for fc1's split output."""
    qkv_sp = layer.split_of("qkv") if layer.qkv_w is not None else None
    if x_ln1 is None:
        x = norm_of(hs, layer.ln1, qkv_sp) if qkv_sp is not None else layer.ln1(hs)
    else:
        x = x_ln1
    out_sp = layer.split_of("out")
    hdim = layer.q.out_features
    ctx_sp = out_sp is not None and hip.tree_attention_sp_supported(trie.anc, layer.heads, hdim // layer.heads)
    attn = hip.tree_attention_sp if ctx_sp else hip.tree_attention
    if rows is None and layer.qkv_w is not None:
        qkv = linear(x, layer.qkv_w, layer.qkv_b, wsp=qkv_sp)     # (U, 3h): q | k | v as strided row views
        ctx = attn(qkv[:, :hdim], qkv[:, hdim:2 * hdim], qkv[:, 2 * hdim:], trie.anc, trie.depth, layer.heads,
                   layer.scale, None)
        res = hs
    else:
        if layer.qkv_w is not None:
            # every node's k | v in ONE projection (the stacked weight's k and v rows), q for the query rows only
            sp = qkv_sp
            if sp is not None and not isinstance(x, hip.SplitRows) and hip.split_supported(x):
                x = hip.split_rows(x)              # once for both projections below
            kv = linear(x, layer.qkv_w[hdim:], layer.qkv_b[hdim:] if layer.qkv_b is not None else None,
                        wsp=sp.rows(hdim, 3 * hdim) if sp is not None else None)
            k, v = kv[:, :hdim], kv[:, hdim:]
            qw, qb = layer.qkv_w[:hdim], (layer.qkv_b[:hdim] if layer.qkv_b is not None else None)
            qsp = sp.rows(0, hdim) if sp is not None else None
        else:
            k = linear(x, layer.k.weight, layer.k.bias, wsp=layer.split_of("k"))
            v = linear(x, layer.v.weight, layer.v.bias, wsp=layer.split_of("v"))
            qw, qb, qsp = layer.q.weight, layer.q.bias, layer.split_of("q")
        if rows is None:
            q = linear(x, qw, qb, wsp=qsp)
            res = hs
        else:
            idx = rows.long()
            q = linear(x.index_select(idx) if isinstance(x, hip.SplitRows) else x.index_select(0, idx), qw, qb, wsp=qsp)
            res = hs.index_select(0, idx)
        ctx = attn(q, k, v, trie.anc, trie.depth, layer.heads, layer.scale, rows)
    if OWN_GEMM:
        mid = linear(ctx, layer.out.weight, layer.out.bias, residual=res, wsp=out_sp)     # residual add in the GEMM's epilogue
        fc1_sp = layer.split_of("fc1")
        scale_out = fc1_sp is not None and layer.split_of("fc2") is not None and layer.act_code is not None
        return mid, norm_of(mid, layer.ln2, fc1_sp, want_f32=want_f32, scale_output=scale_out)
    o = layer.out(ctx)
    if _fusable(layer.ln2):
        return hip.add_layernorm(res, o, layer.ln2)          # residual add + LN2 in one pass
    mid = res + o
    return mid, layer.ln2(mid)


def mlp_hidden(layer: ClipLayer, ln2_mid, want_f32: bool = True):
    """fc2 INPUT (the "key" space): act(fc1(LN2(hs_mid))).  On the split-fp16 path (``ln2_mid`` a SplitRows carrying the output
    scale) the result is a SplitRows written by fc1's epilogue, with its fp32 twin when ``want_f32``."""
    ps = ln2_mid.out_scale if isinstance(ln2_mid, hip.SplitRows) else None
    return linear(ln2_mid, layer.fc1.weight, layer.fc1.bias, act=layer.act, act_code=layer.act_code, wsp=layer.split_of("fc1"),
                  planes_scale=ps, want_f32=want_f32 or ps is None)


def run_layers(graph: ClipTextGraph, trie: TokenTrie, upto: int, on_fc2=None, last_rows_only: bool = True,
               fc2_by_callback=()):
    """Layers 0..upto (inclusive).  ``on_fc2(i, x, out) -> out'`` is called with the fc2 input/output of every layer
    (rows = all nodes, or the query rows at layer ``upto`` when ``last_rows_only``); whatever it returns is used
    as fc2's output.  Returns the residual stream after layer ``upto`` (query rows only if ``last_rows_only``)."""
    res = run_layers_from(graph, trie, None, 0, upto, on_fc2, last_rows_only, fc2_by_callback)
    if graph.guard is not None:
        graph.guard.flush()
    return None if res is None else res[0]


def run_prefix(graph: ClipTextGraph, trie: TokenTrie, stop: int):
    """Layers 0..stop-1 on every node: the state (residual stream, LN1 of it or None) that enters layer ``stop``.  Cache entries
    made on the way (first call, or after a weight changed) are fingerprinted before this returns, i.e. from the bytes the
    entries were made from, not from whatever is live when the edit's run starts."""
    try:
        return _run_prefix(graph, trie, stop)
    finally:
        if graph.guard is not None:
            graph.guard.flush()          # no launch unless entries were made


def _run_prefix(graph: ClipTextGraph, trie: TokenTrie, stop: int):
    _check_fp32(graph)
    if trie.position is not trie.depth and trie.max_position >= graph.position_embedding.num_embeddings:
        # (a leaf behind the EOS past the position table: refused here, on the host, like HF's CLIP embeddings)
        raise ValueError(f"Sequence length must be less than max_position_embeddings (position {trie.max_position} of "
                         f"{graph.position_embedding.num_embeddings})")
    ln0 = graph.layers[0].ln1 if stop > 0 and graph.layers else None
    te, pe = graph.token_embedding, graph.position_embedding
    if ln0 is not None and _fusable(ln0) and te.weight.is_cuda and te.weight.dtype == torch.float32 \
            and te.weight.stride(1) == 1 and pe.weight.stride(1) == 1 and te.padding_idx is None and te.max_norm is None \
            and pe.max_norm is None and trie.position.dtype == torch.int32 and trie.token.dtype == torch.int64 \
            and 0 <= trie.max_token < te.num_embeddings and trie.max_position < pe.num_embeddings:
        # embeddings + the first layer's LN1 in one launch; token and position ranges are checked on the host copies
        # (anything out of range takes the torch path, which raises like the reference's forward)
        sp0 = graph.layers[0].split_of("qkv") if graph.layers[0].qkv_w is not None else None
        if sp0 is not None and _sp_ln_ok(ln0):
            hs, x_ln1 = hip.embed_layernorm_sp(te.weight, pe.weight, trie.token, trie.position, ln0)
            nat = native_of(graph, trie, 0, stop)
            if nat is not None:
                # every layer of the prefix in ONE C call (csrc/clip_layers.hip), in place on hs / the LN1 planes
                nxt = graph.layers[stop].ln1 if stop < len(graph.layers) else None
                if nxt is not None and not (_fusable(nxt) and _sp_ln_ok(nxt) and graph.layers[stop].split_of("qkv") is not None):
                    nxt = None
                hip.clip_layers(nat.array, 0, stop, hs.shape[0], nat.h, nat.d, nat.heads, nat.scale, trie.anc, trie.depth,
                                hs, x_ln1, nxt)
                LAST_PATHS["native_layers"] += stop
                return hs, (x_ln1 if nxt is not None else None)
        else:
            hs, x_ln1 = hip.embed_layernorm(te.weight, pe.weight, trie.token, trie.position, ln0)
    else:
        hs, x_ln1 = embed(graph, trie), None
    for i in range(stop):
        hs, x_ln1 = _layer_full(graph, i, trie, hs, x_ln1, stop)
    return hs, x_ln1


def _next_ln1(graph, nxt_index: int, hs: torch.Tensor, nxt):
    """LN1 of the next layer on the residual stream (a SplitRows for its q | k | v projection on the split-fp16 path)."""
    if nxt is None or not _fusable(nxt):
        return None
    nl = graph.layers[nxt_index]
    return norm_of(hs, nxt, nl.split_of("qkv") if nl.qkv_w is not None else None)


def _layer_full(graph, i, trie, hs, x_ln1, n_layers_needed):
    layer = graph.layers[i]
    mid, ln2_mid = layer_attention_block(layer, hs, trie, None, x_ln1)
    nxt = graph.layers[i + 1].ln1 if i + 1 < len(graph.layers) and i + 1 <= n_layers_needed else None
    if OWN_GEMM:
        hs = linear(mlp_hidden(layer, ln2_mid, want_f32=False), layer.fc2.weight, layer.fc2.bias, residual=mid,
                    wsp=layer.split_of("fc2"))     # fc2 + residual add
        return hs, _next_ln1(graph, i + 1, hs, nxt)
    out = layer.fc2(mlp_hidden(layer, ln2_mid))
    if nxt is not None and _fusable(nxt):
        return hip.add_layernorm(mid, out, nxt)          # residual add + the next layer's LN1 in one pass
    return mid + out, None


def _tail_ln(graph: ClipTextGraph, i: int, nxt):
    """The next layer's LN1 when the native fc2 tail can produce it as planes (None: it is computed separately)."""
    return nxt if nxt is not None and _fusable(nxt) and _sp_ln_ok(nxt) and \
        graph.layers[i + 1].qkv_w is not None and graph.layers[i + 1].split_of("qkv") is not None else None


def run_layers_from(graph: ClipTextGraph, trie: TokenTrie, state, start: int, upto: int, on_fc2=None,
                    last_rows_only: bool = True, fc2_by_callback=(), edit_callback: bool = False):
    """Layers start..upto (inclusive).  ``state``: (residual stream, LN1 of it | None) entering layer ``start`` (None: start
    from the embeddings, start == 0).  ``on_fc2(i, x, out) -> out'`` gets plain fp32 fc2 inputs.  ``edit_callback`` (the edit
    engine): ``on_fc2(i, x, out, mid, next_ln)`` instead, where ``x`` may be a ``hip.SplitRows`` with its fp32 twin (the engine
    feeds the planes to fc2 and gathers the keys from the twin) and ``mid`` is the residual stream: for a layer in
    ``fc2_by_callback`` it returns fc2(x) + mid, or the pair (hs, LN1 planes of the next layer) when it also took that LayerNorm
    (``next_ln``: that LayerNorm, or None) off our hands.  Returns the final state, or None if the callback ended the pass."""
    _check_fp32(graph)
    by_cb = set(fc2_by_callback)
    hs, x_ln1 = (embed(graph, trie), None) if state is None else state
    for i in range(start, upto + 1):
        layer = graph.layers[i]
        rows = trie.query_rows if (last_rows_only and i == upto) else None
        nat = native_of(graph, trie, i, i + 1) if isinstance(x_ln1, hip.SplitRows) else None
        if nat is not None:
            # attention block + fc1 in ONE C call (csrc/clip_layers.hip)
            mid, x = hip.clip_layer_head(nat.array, i, hs.shape[0], nat.h, nat.d, nat.heads, nat.scale, trie.anc,
                                         trie.depth, rows, hs, x_ln1, want_f32=on_fc2 is not None)
            LAST_PATHS["native_layers"] += 1
        else:
            mid, ln2_mid = layer_attention_block(layer, hs, trie, rows, x_ln1)
            x = mlp_hidden(layer, ln2_mid, want_f32=on_fc2 is not None)
        # layers in ``fc2_by_callback``: the callback produces fc2's output itself (out is passed as None), so an
        # edited layer's projection is computed once, with the new weight, instead of twice
        nxt = graph.layers[i + 1].ln1 if i < upto else None
        summed = False
        tail_state = None
        if i in by_cb or not OWN_GEMM:
            out = None if i in by_cb else layer.fc2(x.float() if isinstance(x, hip.SplitRows) else x)
        elif on_fc2 is None and nat is not None:
            # fc2 + residual add + the next layer's LN1 in ONE C call
            nl = _tail_ln(graph, i, nxt)
            tail_state = hip.clip_layer_tail(nat.array, i, nat.h, nat.d, x, mid, nl)
            if nl is None and nxt is not None:
                tail_state = (tail_state[0], _next_ln1(graph, i + 1, tail_state[0], nxt))
            out = tail_state[0]
            summed = True
        else:
            out = linear(x, layer.fc2.weight, layer.fc2.bias, residual=mid, wsp=layer.split_of("fc2"))
            summed = True
        if on_fc2 is not None:
            if edit_callback and not summed:
                nl = _tail_ln(graph, i, nxt)
                out = on_fc2(i, x, out, mid, nl)
                if isinstance(out, tuple):
                    tail_state = (out[0], out[1] if nl is not None else _next_ln1(graph, i + 1, out[0], nxt))
                    out = out[0]
                summed = out is not None and i in by_cb
            else:
                out = on_fc2(i, x if edit_callback else (x.float() if isinstance(x, hip.SplitRows) else x), out)
            if out is None:
                return None
        if tail_state is not None:
            hs, x_ln1 = tail_state
        elif summed:
            hs, x_ln1 = out, _next_ln1(graph, i + 1, out, nxt)
        elif nxt is not None and _fusable(nxt):
            hs, x_ln1 = hip.add_layernorm(mid, out, nxt)
        else:
            hs, x_ln1 = mid + out, None
    return hs, x_ln1


def last_hidden_at_lookup(graph: ClipTextGraph, trie: TokenTrie) -> torch.Tensor:
    """``text_encoder(**inputs)[0]`` (final LayerNorm applied) at every prompt's lookup token, (B, h), through the trie:
    the whole encoder on the distinct prefixes, the last layer and the final norm on the lookup nodes only."""
    if graph.final_layer_norm is None:
        raise UnsupportedEncoder("no final_layer_norm")
    hs = run_layers(graph, trie, len(graph.layers) - 1, None, last_rows_only=True)      # (R, h) query rows
    return graph.final_layer_norm(hs).index_select(0, trie.lookup_in_query)

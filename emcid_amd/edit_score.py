"""Edit scores: did an edit take, and what did it move — per-concept efficacy and held-out drift read on the device from the text
encoder's own output (``EditScorer`` for one encoder, ``PairEditScorer`` for the SDXL pair), their results and ``select_point``.
The reference chooses its weights by generating and classifying images, so none of this mirrors it; every name here stays
reachable as an attribute of ``emcid_main``, whose sweeps build the scorers on their own prepared plans."""
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import clip_forward, emcid_main, hip, nethook      # (emcid_main.<name> is looked up at call time, like hip.<entry>)
from .edit_engine import ConceptShard, EncoderEditPlan, prepare_encoder_edit
from .emcid_hparams import EMCIDHyperParams, EMCIDXLHyperParams


def _median(x: torch.Tensor) -> float:
    """The median of a vector: of an even number of values, the mean of the middle two (``torch.median`` takes the lower one)."""
    return float(torch.quantile(x.double(), 0.5))


class EditScore:
    """What ``EditScorer.score`` read, as fp64 tensors on the host.

    Per concept row, in the order of ``EditSession.rows()`` (request by request, its num_edit_tokens rows in turn):
        sources   [(request["source"], token index)]
        left      ||v* - Z|| / ||v* - Z0||: the fraction of the way to the target that is still to go (1: nothing moved, 0: on target)
        cos       cos(Z - Z0, v* - Z0): whether what moved went towards the target (0 where nothing moved)
        resid, resid0   the two norms ``left`` is the ratio of
    Per holdout prompt, in the order given:
        holdout     the prompt strings
        drift_max, drift_mean   max and mean over the prompt's tokens BOS ... EOS of ||f - f0|| / ||f0||, f the encoder's output
                    (final LayerNorm applied) at the token, f0 the same before the edit
        drift_eos   that ratio at the EOS token
        drift_argmax    the token position of the max (the first one on a tie)"""

    def __init__(self, sources, left, cos, resid, resid0, holdout, drift_max, drift_mean, drift_eos, drift_argmax):
        self.sources, self.left, self.cos, self.resid, self.resid0 = list(sources), left, cos, resid, resid0
        self.holdout, self.drift_max, self.drift_mean, self.drift_eos = list(holdout), drift_max, drift_mean, drift_eos
        self.drift_argmax = drift_argmax

    def summary(self) -> Dict[str, float]:
        return {"left_median": _median(self.left), "left_max": float(self.left.max()),
                "drift_max": float(self.drift_max.max()), "drift_median": _median(self.drift_max)}

    def __repr__(self):
        return "EditScore(" + ", ".join(f"{k}={v:.4g}" for k, v in self.summary().items()) + ")"


def _score_from_sums(sources, holdout, rows: torch.Tensor, chains: torch.Tensor) -> EditScore:
    """The ``EditScore`` of one encoder from its (N, 8) row sums (``hip.score_rows`` with a target) and (B, 4) chain values
    (``hip.score_chains``) on the host.  Nothing of the result aliases the two inputs."""
    tiny = torch.finfo(torch.float64).tiny
    moved2, resid2, resid02, dot = rows[:, 0], rows[:, 4], rows[:, 5], rows[:, 6]
    left = torch.where(resid02 > 0, (resid2 / resid02.clamp(min=tiny)).sqrt(), torch.zeros_like(resid2))
    den = (moved2 * resid02).sqrt()
    cos = torch.where(den > 0, dot / den.clamp(min=tiny), torch.zeros_like(dot))
    return EditScore(sources, left, cos, resid2.sqrt(), resid02.sqrt(), holdout, *(chains[:, i].clone() for i in range(4)))


def score_row_sources(requests: Sequence[Dict], num_edit_tokens: int = 1) -> List[tuple]:
    """[(source, token index)] in the row order of an edit's concept stack: row rq * k + num (the reference's "rq num")."""
    k = int(num_edit_tokens)
    return [(r["source"], num) for r in requests for num in range(k)]


SCORE_MAX_CHAIN = 128       # nodes per holdout chain the readout takes (csrc/score.hip; the trie forward's own limit too)


def _holdout_list(prompts, what: str = "holdout must be") -> List[str]:
    """``prompts`` as a list, refused unless it is a non-empty list of prompt strings (``what`` opens the refusal)."""
    prompts = list(prompts) if prompts is not None else []
    if not prompts or not all(isinstance(p, str) for p in prompts):
        raise ValueError(f"{what} a non-empty list of prompt strings")
    return prompts


def _one_rank(shard, who: str):
    if emcid_main._shard_from_env(shard).collective:
        raise ValueError(f"{who} runs on one rank: a collective ConceptShard is not supported")


def holdout_tokens(tokenizer, prompts: Sequence[str], n_positions: Optional[int] = None):
    """Generic prompts tokenized for the holdout trie, host only: ((B, S) int64 ids, (B,) int64 EOS positions).  A chain BOS ... EOS
    longer than ``SCORE_MAX_CHAIN`` nodes, or than the encoder's ``n_positions`` position embeddings, is refused here."""
    from .compute_z import tokenize_lists
    enc = tokenize_lists(tokenizer, _holdout_list(prompts))
    ids, mask = np.asarray(enc["input_ids"], dtype=np.int64), np.asarray(enc["attention_mask"], dtype=np.int64)
    eos = mask.sum(axis=1) - 1
    if int(eos.min()) < 0:
        raise ValueError("a holdout prompt tokenizes to nothing")
    longest = int(eos.max()) + 1
    if longest > SCORE_MAX_CHAIN:
        raise clip_forward.UnsupportedEncoder(f"a holdout prompt has {longest} tokens: the score's readout takes chains of up to "
                                              f"{SCORE_MAX_CHAIN} nodes")
    if n_positions is not None and longest > int(n_positions):
        raise ValueError(f"a holdout prompt has {longest} tokens for {int(n_positions)} position embeddings")
    return ids, eos


def holdout_trie(tokenizer, prompts: Sequence[str], device, n_positions: Optional[int] = None):
    """The prefix trie of generic prompts whose lookup is each prompt's EOS, so that every chain runs BOS ... EOS: (TokenTrie,
    (B,) int64 EOS positions on the host).  ``trie.lookup_node[p]`` is prompt p's end node; its chain is
    ``trie.anc[end, 0 .. trie.depth[end]]``."""
    ids, eos = holdout_tokens(tokenizer, prompts, n_positions)
    return clip_forward.build_trie(ids, eos, device), eos


def select_point(scores: Sequence[EditScore], max_drift: float) -> Optional[int]:
    """The index of the score with the smallest median ``left`` among those whose largest ``drift_max`` is within ``max_drift``
    (the first of equals), or None when there is none.  Host only."""
    best, best_left = None, None
    for i, s in enumerate(scores):
        if not float(s.drift_max.max()) <= float(max_drift):
            continue
        m = _median(s.left)
        if best is None or m < best_left:
            best, best_left = i, m
    return best


def _layer_module_tmp(hparams) -> str:
    layer_tmp = getattr(hparams, "layer_module_tmp", None)
    if layer_tmp is None:
        raise clip_forward.UnsupportedEncoder("hparams.layer_module_tmp is not set: no prefix-trie forward")
    return layer_tmp


def _check_encoder(te, layers, hparams, device, holdout, which: Optional[int] = None):
    """The host-side refusals of ONE encoder, in the order both scorers make them, before anything is launched: (holdout as a list,
    the encoder's graph, h).  ``which``: None in ``EditScorer``'s wording, 1 | 2 in ``PairEditScorer``'s."""
    tmp = hparams.rewrite_module_tmp
    try:
        weights = [nethook.get_parameter(te, f"{tmp.format(l)}.weight") for l in layers]
    except LookupError as e:
        what = f"{tmp!r} names no weight of text encoder {which}" if which is not None else \
            f"EditScorer scores edits of the text encoder's MLP projections; {tmp!r} names no weight of pipe.text_encoder " \
            f"(cross-attention edits are not supported)"
        raise ValueError(f"{what}: {e}") from e
    w = weights[0]
    if device is not None and torch.device(device).type != w.device.type:
        whose = f"the weights of text encoder {which}" if which is not None else "the text encoder's weights"
        raise ValueError(f"device {device!r} but {whose} live on {w.device}")
    holdout = _holdout_list(holdout)
    layer_tmp = _layer_module_tmp(hparams)
    if not (w.is_cuda and w.dtype == torch.float32):
        got = f"text encoder {which}: {w.dtype}" if which is not None else f"got {w.dtype}"
        raise clip_forward.UnsupportedEncoder(f"the prefix-trie forward runs fp32 in HBM ({got} on {w.device})")
    try:
        graph = clip_forward.discover_cached(te, layer_tmp)
        if any(graph.layers[l].fc2.weight is not wl for l, wl in zip(layers, weights)):
            raise clip_forward.UnsupportedEncoder("rewrite_module_tmp is not the layer's mlp.fc2")
    except (IndexError, LookupError) as e:
        raise clip_forward.UnsupportedEncoder(str(e)) from e
    return holdout, graph, int(w.shape[0])


def _affine_fp32_ln(ln, h: int) -> bool:
    return isinstance(ln, torch.nn.LayerNorm) and ln.weight is not None and ln.bias is not None and ln.weight.is_cuda \
        and ln.weight.dtype == torch.float32 and tuple(ln.normalized_shape) == (h,)


class _EncoderReplay:
    """What a scorer keeps of ONE encoder, and the replay it scores by: the request chunk and v*, the two states entering
    ``layers[0]`` (request trie, holdout trie), Z0, H0 (and H0last), a buffer for the holdout's node sums, and the signature of the
    parameters at construction.  ``holdout_last``: the layer after which the holdout is read on every node (the last one for
    ``EditScorer``, the penultimate one — ``hidden_states[-2]`` — for the pair); ``pooled``: (final LayerNorm, projection weight) of a
    pooled embedding, for which the last layer is continued on the EOS rows as well; ``keep_state``: the plan is a sweep's own, whose points replay its state too (dropped from the plan otherwise);
    ``k``: the num_edit_tokens the plan must have been prepared with."""

    def __init__(self, te, graph, layers, plan: EncoderEditPlan, ids_h, eos_h, holdout_last: int, pooled: Optional[tuple] = None,
                 keep_state: bool = False, k: Optional[int] = None):
        if plan.chunk is None or plan.graph is not graph or plan.chunk.state is None or plan.chunk.state[0] != layers[0] \
                or plan.layers != layers or (k is not None and plan.num_edit_tokens != k):
            raise clip_forward.UnsupportedEncoder("the requests did not take the prefix-trie forward")
        self.te, self.graph, self.layers, self.holdout_last, self.pooled = te, graph, layers, holdout_last, pooled
        self.chunk, self.zs = plan.chunk, plan.resolve_targets()
        self._state = tuple(plan.chunk.state[1:])
        if not keep_state:
            plan.chunk.state = None
        dev = self.zs.device
        with torch.no_grad():
            self.trie_h = clip_forward.build_trie(ids_h, eos_h, dev)
            self._state_h = tuple(clip_forward.run_prefix(graph, self.trie_h, layers[0]))
            self.frozen = self.signature()
            Z0, self.H0, self.H0last = self.forward()
        self.Z0 = Z0.clone()
        if tuple(self.zs.shape) != tuple(self.Z0.shape):
            raise ValueError(f"{self.Z0.shape[0]} concept rows of width {self.Z0.shape[1]} and v* of shape {tuple(self.zs.shape)}")
        self.node = torch.empty(self.H0.shape[0], 8, dtype=torch.float64, device=dev)

    def signature(self):
        """(name, identity, address, in-place version) of every parameter but the edited fc2 weights — of those: identity alone."""
        edited = {id(self.graph.layers[l].fc2.weight) for l in self.layers}
        return tuple((n, id(p)) if id(p) in edited else (n, id(p), p.data_ptr(), p._version) for n, p in self.te.named_parameters())

    def check_frozen(self, which: Optional[int] = None):
        """Refuse (``ValueError``) when a parameter other than the edited fc2 weights is not the tensor, at the address, with the
        version counter of construction.  ``which`` as in ``_check_encoder``."""
        now = self.signature()
        if now == self.frozen:
            return
        now = dict((s[0], s) for s in now)
        moved = [s[0] for s in self.frozen if now.get(s[0]) != s]
        of, cls, new = ("", "EditScorer", "a new EditScorer") if which is None else (f" of text encoder {which}", "PairEditScorer", "a new one")
        raise ValueError(f"parameters{of} other than the edited fc2 weights changed since this {cls} was built "
                         f"({', '.join(moved[:4]) or 'the parameter list'}{', ...' if len(moved) > 4 else ''}): its kept states "
                         f"are no longer this encoder's; build {new}")

    def forward(self):
        """(Z (N k, h), H (holdout nodes, h) after layer ``holdout_last``, H_last (B, h) at the EOS rows | None), fp32, on the
        weights as they are: the replay from the two kept states (``run_layers_from`` only reads them)."""
        g, ch, first, last = self.graph, self.chunk, self.layers[0], self.layers[-1]
        box = []

        def on_fc2(li, x, out, mid=None, next_ln=None):
            # the engine's own Zc of its last layer: fc2 is affine, so the mean output at the lookup rows is fc2 of the mean key
            if li != last:
                return out
            layer = g.layers[li]
            xf = x.float() if isinstance(x, hip.SplitRows) else x
            K = hip.gather_mean(xf.unsqueeze(0).expand(ch.lookup_query.numel(), -1, -1), ch.lookup_query, ch.cseg)
            box.append(clip_forward.linear(K, layer.fc2.weight, layer.fc2.bias, wsp=layer.split_of("fc2")))
            return None

        clip_forward.run_layers_from(g, ch.trie, self._state, first, last, on_fc2, fc2_by_callback=(last,), edit_callback=True)
        # every node, raw; a layer that lies before the first edited one is the kept state itself
        state = self._state_h if first > self.holdout_last else \
            clip_forward.run_layers_from(g, self.trie_h, self._state_h, first, self.holdout_last, None, last_rows_only=False)
        h_last = None
        if self.pooled:       # the last layer continued on the distinct EOS nodes, then one row per prompt
            n_layers = len(g.layers)
            rows = clip_forward.run_layers_from(g, self.trie_h, state, n_layers - 1, n_layers - 1, None, last_rows_only=True)[0]
            h_last = rows.index_select(0, self.trie_h.lookup_in_query)
        if g.guard is not None:
            g.guard.flush()          # (fingerprints of the weights that cache entries were made from in this replay, if any)
        clip_forward.LAST_PATHS["score_replays"] = clip_forward.LAST_PATHS.get("score_replays", 0) + 1
        return box[0], state[0], h_last

    def _half(self, rows, node, chains, ln=None, pooled=None):
        """This encoder's half of a score on its weights as they are, issued on the current stream — the one statement of it: the
        replay, ``score_rows`` into ``rows`` (N, 8) and — behind ``ln`` when given — into ``node`` (holdout nodes, 8),
        ``score_chains`` into ``chains`` (B, 4) and, with a pooled embedding, ``score_pooled`` into ``pooled`` (B, 4)."""
        Z, H, h_last = self.forward()
        hip.score_rows(Z, self.Z0, t=self.zs, out=rows)
        hip.score_rows(H, self.H0, ln=ln, out=node)
        hip.score_chains(node, self.trie_h.anc, self.trie_h.depth, self.trie_h.lookup_node, out=chains)
        if self.pooled:
            hip.score_pooled(h_last, self.H0last, *self.pooled, out=pooled)


class EditScorer:
    """Scores edits of ONE text encoder by the encoder's own output, on the device.

        scorer = EditScorer(pipe, requests, hparams, device, holdout=[prompt strings], cache_name=...)    # on the BASELINE weights
        ... any edit of the fc2 weights of hparams.layers: a plain call, a session step, a sweep point ...
        s = scorer.score()                                                                               # -> EditScore

    Efficacy is read where the closed form acts: Z is the mean over a concept's prompts of the LAST edited layer's fc2 output (bias
    included) at the lookup rows — the engine's Zc of that layer —, Z0 the same on the baseline weights, and
    ``left = ||v* - Z|| / ||v* - Z0||``, ``cos = cos(Z - Z0, v* - Z0)`` per concept row.  (The reference takes its residual
    against this very quantity, emcid_main.py:1002-1016; the residual stream at that layer carries the attention branch and the
    skip path as well, which the edit does not steer.)  Drift is read where the UNet is conditioned: with H the residual stream
    after the last encoder layer at every token of every holdout prompt and f = final_layer_norm(H), the ratio
    ``||f - f0|| / ||f0||`` per token, reduced per prompt to its max, mean and EOS value (``EditScore``).  Positions behind a
    prompt's EOS — the padding a pipeline feeds the UNet too — are not scored.

    The constructor tokenizes ``requests`` like a plain call (same trie, same lookups, for num_edit_tokens = k > 1 the same leaves
    and (request, num) rows), reads their v* rows with the call's loader (a missing file is an error: Stage 1 never runs here),
    builds a second trie over ``holdout`` whose lookups are the prompts' EOS tokens, runs the unedited leading layers on both
    (``clip_forward.run_prefix``) and keeps the two states, then runs the rest once and keeps Z0 (N k, h) and H0 (holdout nodes, h),
    raw — all of it in ``self.enc``, an ``_EncoderReplay``.  State held: the two entering states, Z0, H0, v*, fp32 in HBM.

    ``score()`` replays layers[0] ... from the two kept states: the request trie to layers[-1], the holdout trie to the last layer
    on every node; Z by the engine's own gather; then TWO launches (``hip.score_rows`` on (Z, Z0, v*) and, behind the final
    LayerNorm in fp64, on (H, H0); ``hip.score_chains`` over the holdout chains) and ONE pinned readback, the only host
    synchronisation.  Everything is issued eagerly on the current stream; no weight is moved and every parameter is bit-identical
    afterwards; the forward's weight-derived caches refresh themselves as in any forward.  Two calls in a row return the same bits.

    Refused before anything is launched: an encoder the prefix-trie forward does not take (``clip_forward.UnsupportedEncoder``,
    as ``edit_engine.run_sweep``: not HF CLIP, not fp32 in HBM, no final LayerNorm the readout takes, a holdout prompt of more than
    ``SCORE_MAX_CHAIN`` = 128 tokens); a holdout prompt longer than the position table (``ValueError``); the SDXL pair, a
    cross-attention ``rewrite_module_tmp``, a collective ``ConceptShard`` (``ValueError``); and a ``score()`` when a parameter other
    than the edited fc2 weights is not the tensor, at the address, with the in-place version counter it had at construction
    (``ValueError``: the kept states would no longer be this encoder's).  That check is host-only: a write through ``.data`` or a
    raw pointer to such a parameter is not seen and is the caller's responsibility.  Not done here: the SDXL pair (that is
    ``PairEditScorer``), sharded calls, scoring on the hooked-HF forward, positions behind the EOS."""

    def __init__(self, pipe, requests: List[Dict], hparams: EMCIDHyperParams, device: Optional[str] = None, holdout=None,
                 cache_name: Optional[str] = None, shard=None, _plan: Optional[EncoderEditPlan] = None):
        if isinstance(hparams, EMCIDXLHyperParams) or getattr(pipe, "text_encoder_2", None) is not None:
            raise ValueError("EditScorer scores one CLIP text encoder: the SDXL pair (EMCIDXLHyperParams / text_encoder_2) is not supported")
        if not isinstance(hparams, EMCIDHyperParams):
            raise TypeError(f"hparams must be EMCIDHyperParams, got {type(hparams).__name__}")
        _one_rank(shard, "EditScorer")
        if len(requests) == 0:
            raise ValueError("EditScorer needs at least one request")
        layers = list(hparams.layers)
        if not layers or sorted(layers) != layers:
            raise ValueError(f"hparams.layers must be a non-empty list in forward order (got {hparams.layers})")
        te, tok = pipe.text_encoder, pipe.tokenizer
        holdout, graph, h = _check_encoder(te, layers, hparams, device, holdout)
        if not (_affine_fp32_ln(graph.final_layer_norm, h) and h % 4 == 0 and h <= hip.SCORE_MAX_COLS):
            raise clip_forward.UnsupportedEncoder(f"the score's readout takes an affine fp32 final LayerNorm over h = {h} columns "
                                                  f"(h % 4 == 0, h <= {hip.SCORE_MAX_COLS})")
        # (host only: a holdout chain the readout or the position table cannot take is refused before anything is launched)
        ids_h, eos_h = holdout_tokens(tok, holdout, graph.position_embedding.num_embeddings)
        if _plan is None and emcid_main._any_vstar_missing(requests, hparams, cache_name, ""):
            raise FileNotFoundError(f"a v* file of the {len(requests)} requests is missing under {cache_name!r}: an EditScorer reads "
                                    f"the targets an edit was made towards and never runs Stage 1")
        k = int(getattr(hparams, "num_edit_tokens", 1) or 1)
        self.pipe, self.hparams, self.layers, self.graph, self.k = pipe, hparams, layers, graph, k
        self.sources, self.holdout, self.eos = score_row_sources(requests, k), holdout, eos_h
        # ``_plan`` (sweep_emcid_text_encoder): the sweep's own prepared plan of these very requests — its trie, its v* rows (read,
        # or computed by Stage 1, the way a call does) and the state its prefix run left, which the sweep's points replay as well
        plan = _plan if _plan is not None else prepare_encoder_edit(
            te, tok, requests, layers, hparams.rewrite_module_tmp, float(hparams.mom2_update_weight), float(hparams.edit_weight),
            lambda: emcid_main.load_v_stars(requests, hparams, cache_name, "", None, width=h, pin=True),
            lambda: {}, ConceptShard(), layer_module_tmp=hparams.layer_module_tmp, num_edit_tokens=k)
        self.enc = enc = _EncoderReplay(te, graph, layers, plan, ids_h, eos_h, len(graph.layers) - 1, keep_state=_plan is not None, k=k)
        self.chunk, self.trie_h = enc.chunk, enc.trie_h          # (what scripts/score_cost.py reports the sizes of)
        n, B = enc.Z0.shape[0], len(holdout)
        if n != len(self.sources):
            raise ValueError(f"{n} concept rows for {len(self.sources)} (source, token) pairs and v* of shape {tuple(enc.zs.shape)}")
        self._out = torch.empty(n * 8 + B * 4, dtype=torch.float64, device=enc.Z0.device)
        self._host = torch.empty(n * 8 + B * 4, dtype=torch.float64, pin_memory=True)

    def score(self) -> EditScore:
        """Score the weights as they are against the baseline of construction (class docstring): one replay, two launches, one
        pinned readback."""
        self.enc.check_frozen()
        n, B = self.enc.Z0.shape[0], len(self.holdout)
        with torch.no_grad():
            self.enc._half(self._out[:n * 8].view(n, 8), self.enc.node, self._out[n * 8:].view(B, 4), ln=self.graph.final_layer_norm)
            self._host.copy_(self._out, non_blocking=True)
            torch.cuda.current_stream(self._out.device).synchronize()
        host = self._host.clone()
        return _score_from_sums(self.sources, self.holdout, host[:n * 8].view(n, 8), host[n * 8:].view(B, 4))


class PairEditScore:
    """What ``PairEditScorer.score`` read of the SDXL pair of text encoders, as fp64 tensors on the host.

        te1, te2    one ``EditScore`` per encoder: its concept rows (``left``, ``cos``, ``resid``, ``resid0``) and, per holdout
                    prompt, the drift over that encoder's own columns of ``hidden_states[-2]`` (no final LayerNorm)
        sources, left, cos, resid, resid0   the rows of te1, then those of te2; sources are (source, token index, encoder 1 | 2)
    Per holdout prompt, where the UNet is conditioned:
        drift_max, drift_mean, drift_eos, drift_argmax   as in ``EditScore``, of the ratio over the CONCATENATED token state
                    [hidden_states[-2] of TE1 ; hidden_states[-2] of TE2]: sqrt((|dh_1|^2 + |dh_2|^2) / (|h0_1|^2 + |h0_2|^2))
        drift_pooled    ||P (a^ - b^)|| / ||P b^|| of the pooled embedding text_projection(final_layer_norm(H_last[EOS])) of TE2
                    (a^ now, b^ at construction), or None when text_encoder_2 has no text_projection
    ``select_point`` takes a list of these as it takes ``EditScore``s: it reads ``left`` and ``drift_max``."""

    def __init__(self, te1: EditScore, te2: EditScore, holdout, drift_max, drift_mean, drift_eos, drift_argmax, drift_pooled=None):
        self.te1, self.te2, self.holdout = te1, te2, list(holdout)
        self.sources = [(s, t, 1) for s, t in te1.sources] + [(s, t, 2) for s, t in te2.sources]
        self.left, self.cos = torch.cat([te1.left, te2.left]), torch.cat([te1.cos, te2.cos])
        self.resid, self.resid0 = torch.cat([te1.resid, te2.resid]), torch.cat([te1.resid0, te2.resid0])
        self.drift_max, self.drift_mean, self.drift_eos, self.drift_argmax = drift_max, drift_mean, drift_eos, drift_argmax
        self.drift_pooled = drift_pooled

    def summary(self) -> Dict[str, float]:
        out = {"left_median": _median(self.left), "left_max": float(self.left.max()),
               "drift_max": float(self.drift_max.max()), "drift_median": _median(self.drift_max),
               "left_median_1": _median(self.te1.left), "left_median_2": _median(self.te2.left)}
        if self.drift_pooled is not None:
            out["drift_pooled_max"] = float(self.drift_pooled.max())
        return out

    def __repr__(self):
        return "PairEditScore(" + ", ".join(f"{k}={v:.4g}" for k, v in self.summary().items()) + ")"


class PairEditScorer:
    """Scores edits of the SDXL PAIR of text encoders, on the device, where an SDXL UNet is conditioned.

        scorer = PairEditScorer(pipe, requests, hparams, device, holdout=[prompt strings], cache_name=...)   # on the BASELINE weights
        ... apply_emcid_to_sdxl_text_encoders, or any other edit of the fc2 weights of hparams.layers / hparams.layers_2 ...
        s = scorer.score()                                                                                  # -> PairEditScore

    For encoder e in {1, 2} — layers ``hparams.layers`` / ``hparams.layers_2``, v* files with suffix "" / "_2" — efficacy is
    ``EditScorer``'s: Z_e the mean over a concept's prompts of the LAST edited layer's fc2 output at the lookup rows, Z0_e the same
    on the baseline weights, ``left_e = ||v*_e - Z_e|| / ||v*_e - Z0_e||``, ``cos_e = cos(Z_e - Z0_e, v*_e - Z0_e)``.  The weights are
    read as they are: after ``apply_emcid_to_sdxl_text_encoders`` TE2 holds W + 2 dW (the reference's double apply,
    ``SDXL_TE2_DOUBLE_APPLY``) and ``left_2`` reports that overshoot.  Drift follows the conditioning of an SDXL UNet, which takes
    NO final LayerNorm on the token states but, per token, [hidden_states[-2] of TE1 ; hidden_states[-2] of TE2], and the pooled
    embedding of TE2: with h_e(u) the raw residual stream after encoder e's penultimate layer at token u of BOS ... EOS and h0_e the
    same at construction, the token ratio is r(u) = sqrt((|h_1 - h0_1|^2 + |h_2 - h0_2|^2) / (|h0_1|^2 + |h0_2|^2)) (0 when both
    sums are 0), reduced per prompt as in ``EditScore``; each encoder's own ratio over its own columns is in ``te1`` / ``te2``; and
    ``drift_pooled = ||P (a^ - b^)|| / ||P b^||`` with a^ = final_layer_norm(H_last[EOS]) of TE2, b^ the same at construction and
    P = ``text_projection.weight`` — None when text_encoder_2 has no ``text_projection``.  Positions behind the EOS are not scored.

    The constructor prepares each encoder as a call does (same trie, same lookups, v* through ``load_v_stars`` with the encoder's
    suffix and width; a missing file is an error: Stage 1 never runs), builds a holdout trie per encoder whose lookups are the EOS
    tokens, runs the unedited leading layers on both tries of both encoders and keeps the four states, then replays once and
    keeps, per encoder (``self.encoders``, two ``_EncoderReplay``), Z0_e (N, h_e) and the penultimate H0_e (holdout nodes of that
    trie, h_e), and for TE2 with a projection H0last (B, h_2) at the EOS rows — all fp32 in HBM.

    ``score()`` replays both encoders from the kept states (request trie to the last edited layer; holdout trie to the penultimate
    layer on every node and, for the pooled embedding, the last layer on the EOS rows), then per encoder ``hip.score_rows`` on
    (Z, Z0, v*) and on (H, H0) without a LayerNorm and ``hip.score_chains``, once ``hip.score_chains_pair`` and once
    ``hip.score_pooled``, and ONE pinned readback, the only host synchronisation.  Everything is issued on the current stream.  No
    weight is moved, every parameter is bit-identical afterwards, two calls in a row return the same bits.

    Refused before anything is launched: ``hparams`` that is not ``EMCIDXLHyperParams`` (``TypeError``); a pipe without
    ``text_encoder_2``, ``num_edit_tokens != 1``, a collective ``ConceptShard``, two tokenizers that give a holdout prompt different
    BOS ... EOS lengths, a holdout prompt longer than a position table (``ValueError``); an encoder the prefix-trie forward does not
    take — not HF CLIP, not fp32 in HBM, fewer than two layers, h % 4 != 0 or h > 2048, a ``text_projection`` with a bias —, a
    holdout prompt of more than ``SCORE_MAX_CHAIN`` tokens (``clip_forward.UnsupportedEncoder``); a missing v* file
    (``FileNotFoundError``); and, as in ``EditScorer``, a ``score()`` when a parameter of either encoder other than its edited fc2
    weights is not the tensor, at the address, with the version counter it had at construction (``ValueError``).

    A grid of (mom2_weight, mom2_weight_2, edit_weight) triples is ``sweep_emcid_sdxl_text_encoders``: with ``score=`` it builds
    one scorer on its own prepared plans and reads every triple through ``score_points`` — each encoder's half of ``score()``
    (``_EncoderReplay._half``: the one statement of it) once per DISTINCT point of that encoder, one ``hip.score_chains_pair_grid`` for all the
    triples' pair drifts, one pinned read.  Not done here: sessions, sharded calls, the hooked-HF forward, positions behind the
    EOS."""

    @staticmethod
    def _host_checks(pipe, requests, hparams, device, holdout, shard):
        """Every refusal of the constructor that needs neither a launch nor a file, and what it found on the way: (holdout, per
        encoder (te, tok, layers, v* suffix, graph, h, holdout ids, EOS positions), text_projection | None, TE2's final LayerNorm)."""
        if not isinstance(hparams, EMCIDXLHyperParams):
            raise TypeError(f"hparams must be EMCIDXLHyperParams, got {type(hparams).__name__}")
        if getattr(pipe, "text_encoder_2", None) is None or getattr(pipe, "tokenizer_2", None) is None:
            raise ValueError("PairEditScorer scores the SDXL pair: the pipe has no text_encoder_2 / tokenizer_2 (EditScorer scores one encoder)")
        if int(getattr(hparams, "num_edit_tokens", 1) or 1) != 1:
            raise ValueError("num_edit_tokens should be 1 for the SDXL pair")       # (as _sdxl_plans, reference :1246)
        _one_rank(shard, "PairEditScorer")
        if len(requests) == 0:
            raise ValueError("PairEditScorer needs at least one request")
        holdout = _holdout_list(holdout)
        _layer_module_tmp(hparams)
        for which, layers in ((1, list(hparams.layers)), (2, list(hparams.layers_2))):
            if not layers or sorted(layers) != layers:
                raise ValueError(f"the layers of text encoder {which} must be a non-empty list in forward order (got {layers})")
        found = []
        for which, te, tok, layers, suffix in ((1, pipe.text_encoder, pipe.tokenizer, list(hparams.layers), ""),
                                               (2, pipe.text_encoder_2, pipe.tokenizer_2, list(hparams.layers_2), "_2")):
            _, graph, h = _check_encoder(te, layers, hparams, device, holdout, which)
            if len(graph.layers) < 2 or h % 4 or h > hip.SCORE_MAX_COLS:
                raise clip_forward.UnsupportedEncoder(f"the pair's readout takes encoders of two or more layers and h % 4 == 0, h <= "
                                                      f"{hip.SCORE_MAX_COLS} (text encoder {which}: {len(graph.layers)} layers, h = {h})")
            ids_h, eos_h = holdout_tokens(tok, holdout, graph.position_embedding.num_embeddings)
            found.append((te, tok, layers, suffix, graph, h, ids_h, eos_h))
        if not np.array_equal(found[0][7], found[1][7]):
            p = int(np.nonzero(found[0][7] != found[1][7])[0][0])
            raise ValueError(f"holdout prompt {p} ({holdout[p]!r}) has {int(found[0][7][p]) + 1} tokens BOS ... EOS in the first "
                             f"tokenizer and {int(found[1][7][p]) + 1} in the second: their token states cannot be concatenated")
        proj = getattr(pipe.text_encoder_2, "text_projection", None)
        ln2 = found[1][4].final_layer_norm
        if proj is not None:
            h2 = found[1][5]
            if not (isinstance(proj, torch.nn.Linear) and proj.bias is None and proj.weight.is_cuda and proj.weight.dtype == torch.float32
                    and proj.weight.shape[1] == h2 and proj.weight.stride(1) == 1 and proj.weight.stride(0) % 4 == 0
                    and _affine_fp32_ln(ln2, h2)):
                raise clip_forward.UnsupportedEncoder("the pooled readout takes text_projection as an fp32 nn.Linear without bias over an "
                                                      f"affine fp32 final LayerNorm of h = {h2} columns")
        return holdout, found, proj, ln2

    def __init__(self, pipe, requests: List[Dict], hparams: EMCIDXLHyperParams, device: Optional[str] = None, holdout=None,
                 cache_name: Optional[str] = None, shard=None, _plans=None, _checked=None):
        # ``_plans`` (sweep_emcid_sdxl_text_encoders): the sweep's own prepared plans of these very requests — their tries, v* rows
        # (read, or computed by Stage 1, the way a call does) and the states their prefix runs left, which the sweep's points replay
        # as well; ``_checked``: what the sweep's own call of ``_host_checks`` returned before it prepared them
        holdout, found, proj, ln2 = _checked if _checked is not None else self._host_checks(pipe, requests, hparams, device, holdout, shard)
        for te, tok, layers, suffix, graph, h, ids_h, eos_h in found:
            if _plans is None and emcid_main._any_vstar_missing(requests, hparams, cache_name, suffix):
                raise FileNotFoundError(f"a v* file (suffix {suffix!r}) of the {len(requests)} requests is missing under {cache_name!r}: "
                                        f"a PairEditScorer reads the targets an edit was made towards and never runs Stage 1")
        self.pipe, self.hparams, self.holdout, self.proj, self.ln2 = pipe, hparams, holdout, proj, ln2
        self.sources = score_row_sources(requests, 1)
        self.encoders = []
        with torch.no_grad():
            for i, ((te, tok, layers, suffix, graph, h, ids_h, eos_h), lam) in enumerate(zip(found, (hparams.mom2_update_weight,
                                                                                                     hparams.mom2_update_weight_2))):
                plan = _plans[i] if _plans is not None else prepare_encoder_edit(
                    te, tok, requests, layers, hparams.rewrite_module_tmp, float(lam), float(hparams.edit_weight),
                    lambda suffix=suffix, h=h: emcid_main.load_v_stars(requests, hparams, cache_name, suffix, None, width=h, pin=True),
                    lambda: {}, ConceptShard(), layer_module_tmp=hparams.layer_module_tmp, num_edit_tokens=1)
                self.encoders.append(_EncoderReplay(te, graph, layers, plan, ids_h, eos_h, len(graph.layers) - 2, keep_state=_plans is not None,
                                                    pooled=(ln2, proj.weight) if proj is not None and suffix == "_2" else None))
        e1, e2 = self.encoders
        n1, n2, B = e1.Z0.shape[0], e2.Z0.shape[0], len(holdout)
        if n1 != len(self.sources) or n2 != len(self.sources):
            raise ValueError(f"{n1} and {n2} concept rows for {len(self.sources)} requests")
        # one result buffer, one readback: [rows of TE1 | rows of TE2 | chains of TE1 | of TE2 | of the pair | pooled]
        self._cuts = np.cumsum([0, n1 * 8, n2 * 8, B * 4, B * 4, B * 4, B * 4 if proj is not None else 0]).tolist()
        self._out = torch.empty(self._cuts[-1], dtype=torch.float64, device=e1.Z0.device)
        self._host = torch.empty(self._cuts[-1], dtype=torch.float64, pin_memory=True)

    def _part(self, buf, i, width):
        return buf[self._cuts[i]:self._cuts[i + 1]].view(-1, width)

    def _check_frozen(self):
        for which, enc in enumerate(self.encoders, 1):
            enc.check_frozen(which)

    @staticmethod
    def _pooled_drift(sums):
        tiny = torch.finfo(torch.float64).tiny
        return torch.where(sums[:, 0] > 0, (sums[:, 0] / sums[:, 1].clamp(min=tiny)).sqrt(), torch.zeros_like(sums[:, 0]))

    def score(self) -> PairEditScore:
        """Score the weights of both encoders as they are against the baseline of construction (class docstring)."""
        self._check_frozen()
        e1, e2 = self.encoders
        out = self._out
        with torch.no_grad():
            for i, enc in enumerate(self.encoders):
                enc._half(self._part(out, i, 8), enc.node, self._part(out, 2 + i, 4), pooled=self._part(out, 5, 4) if enc.pooled else None)
            hip.score_chains_pair(e1.node, e1.trie_h.anc, e1.trie_h.depth, e1.trie_h.lookup_node,
                                  e2.node, e2.trie_h.anc, e2.trie_h.depth, e2.trie_h.lookup_node, out=self._part(out, 4, 4))
            self._host.copy_(out, non_blocking=True)
            torch.cuda.current_stream(out.device).synchronize()
        host = self._host.clone()
        pair = self._part(host, 4, 4)
        pooled = self._pooled_drift(self._part(host, 5, 4)) if self.proj is not None else None
        te1, te2 = (_score_from_sums(self.sources, self.holdout, self._part(host, i, 8), self._part(host, 2 + i, 4)) for i in (0, 1))
        return PairEditScore(te1, te2, self.holdout, *(pair[:, i].clone() for i in range(4)), pooled)

    def score_points(self, n1: int, n2: int, combos, place) -> List[PairEditScore]:
        """The factorised readout of a sweep (``sweep_emcid_sdxl_text_encoders``): ``with place(i, g):`` holds point g < n1 / n2 of
        encoder i = 0 / 1 in place; inside, that encoder's half of a score runs into the point's slot of one output buffer and of
        the encoder's bank of node sums — TE1 over all its points, then TE2 over its own.  Then ONE
        ``hip.score_chains_pair_grid`` over ``combos`` [(point of TE1, point of TE2)] and ONE pinned read: one ``PairEditScore``
        per combination — ``te1`` from its TE1 point, ``te2`` and ``drift_pooled`` from its TE2 point, the pair drift from the
        grid kernel."""
        self._check_frozen()
        e1, e2 = self.encoders
        N, B, C = len(self.sources), len(self.holdout), len(combos)
        dev = e1.Z0.device
        per = [N * 8 + B * 4, N * 8 + B * 4 + (B * 4 if self.proj is not None else 0)]
        cuts = [0, n1 * per[0], n1 * per[0] + n2 * per[1]]
        out = torch.empty(cuts[2] + C * B * 4, dtype=torch.float64, device=dev)
        host = torch.empty(out.numel(), dtype=torch.float64, pin_memory=True)
        banks = [torch.empty(n, enc.H0.shape[0], 8, dtype=torch.float64, device=dev) for n, enc in ((n1, e1), (n2, e2))]
        combo = torch.tensor([list(c) for c in combos], dtype=torch.int32).reshape(C, 2).to(dev)

        def slot(buf, i, g):
            s = buf[cuts[i] + g * per[i]:cuts[i] + (g + 1) * per[i]]
            return s[:N * 8].view(N, 8), s[N * 8:N * 8 + B * 4].view(B, 4), s[N * 8 + B * 4:].view(-1, 4)

        with torch.no_grad():
            for i, n in enumerate((n1, n2)):
                for g in range(n):
                    with place(i, g):
                        rows, chains, pooled = slot(out, i, g)
                        self.encoders[i]._half(rows, banks[i][g], chains, pooled=pooled if self.encoders[i].pooled else None)
            hip.score_chains_pair_grid(banks[0], e1.trie_h.anc, e1.trie_h.depth, e1.trie_h.lookup_node,
                                       banks[1], e2.trie_h.anc, e2.trie_h.depth, e2.trie_h.lookup_node, combo,
                                       out=out[cuts[2]:].view(C, B, 4))
            host.copy_(out, non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
        halves = [[slot(host, i, g) for g in range(n)] for i, n in ((0, n1), (1, n2))]
        pair = host[cuts[2]:].view(C, B, 4)
        scores = []
        for c, (g1, g2) in enumerate(combos):
            (r1, c1, _), (r2, c2, p2) = halves[0][g1], halves[1][g2]
            scores.append(PairEditScore(_score_from_sums(self.sources, self.holdout, r1, c1),
                                        _score_from_sums(self.sources, self.holdout, r2, c2), self.holdout,
                                        *(pair[c, :, i].clone() for i in range(4)),
                                        self._pooled_drift(p2) if self.proj is not None else None))
        return scores

"""Edit sessions: a sequence of text-encoder edits in which later ones preserve the keys of earlier ones (``EditSession``), the
pure host halves of its operations and its file format.  The reference has nothing like a session, so none of this mirrors it;
every name here stays reachable as an attribute of ``emcid_main``, whose entry points a session's steps are built from."""
import math
import os
from copy import deepcopy
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import clip_forward, edit_engine, emcid_main, hip, nethook      # (emcid_main.<name> is looked up at call time, like hip.<entry>)
from .edit_engine import check_info, phase, run_encoder_edit
from .emcid_hparams import EMCIDHyperParams, EMCIDXLHyperParams
from .globals import STATS_DIR


class PreservedSetFull(RuntimeError):
    """A step of an ``EditSession`` would take the preserved key set past the session's capacity; nothing was launched."""


def release_plan(ledger, folded_sources, sources):
    """The host half of ``EditSession.release``, pure: ``ledger`` is the session's row ledger (one ``(source, kind, ordinal, token
    index)`` tuple per live row, in row order), ``folded_sources`` the names whose rows a fold took, ``sources`` the names to
    release.  Returns (keep: ascending indices of the rows that stay, first: the smallest released index, retained: how many of
    the released rows a retain list had added).  ``ValueError`` for an empty list and for a folded source, ``KeyError`` for an
    unknown one — folded is looked at first only for names without live rows, so a name re-entered after a fold can go."""
    names = list(sources)
    if not names:
        raise ValueError("a release needs at least one source")
    live = {row[0] for row in ledger}
    for name in names:
        if name in live:
            continue
        if name in folded_sources:
            raise ValueError(f"source {name!r} was folded: its keys live inside the session's base factor and the session no longer "
                             f"has their rows; releasing across a fold is not supported — restore() gives the original weights back "
                             f"and forgets every key")
        raise KeyError(f"source {name!r} has no preserved row in this session")
    gone = set(names)
    keep = [i for i, row in enumerate(ledger) if row[0] not in gone]
    first = next((j for j, i in enumerate(keep) if i != j), len(keep))
    retained = sum(1 for row in ledger if row[0] in gone and row[1] == "retain")
    return keep, first, retained


def refold_plan(ledger, archive_ledger, sources):
    """The host half of a release that reaches across a fold (``EditSession(keep_folded=True).release``), pure: ``ledger`` as in
    ``release_plan``, ``archive_ledger`` the same tuples for the rows the folds archived, in archive order, ``sources`` the names
    to release.  Returns (archived: ascending indices into the archive of the rows that go, live: ascending indices into the ledger
    of the rows that go, retained: how many of either a retain list had added).  A name with live AND archived rows loses all of
    them.  ``ValueError`` for an empty list, ``KeyError`` for a name found in neither ledger."""
    names = list(sources)
    if not names:
        raise ValueError("a release needs at least one source")
    known = {row[0] for row in ledger} | {row[0] for row in archive_ledger}
    for name in names:
        if name not in known:
            raise KeyError(f"source {name!r} has no preserved row in this session, live or folded")
    gone = set(names)
    archived = [i for i, row in enumerate(archive_ledger) if row[0] in gone]
    live = [i for i, row in enumerate(ledger) if row[0] in gone]
    retained = sum(1 for rows in (ledger, archive_ledger) for row in rows if row[0] in gone and row[1] == "retain")
    return archived, live, retained


SESSION_FORMAT = 1     # of the file EditSession.save writes ("session file"); load refuses any other
_SESSION_ENTRIES = ("fixed", "rewrite_module_tmp", "d", "h", "capacity", "on_full", "report", "keep_folded", "counters", "ledger",
                    "folded_sources", "archive_ledger", "keys", "weights", "orig", "base", "archive", "fingerprints")
_SESSION_COUNTERS = ("steps", "folds", "folded", "retained", "released", "retains")
_COUNTER_ATTRS = {k: "_retains" if k == "retains" else k for k in _SESSION_COUNTERS}     # counter of the file -> attribute of the session
# gauge of clip_forward.LAST_PATHS -> the session attribute it shows (EditSession._publish)
_GAUGES = {"session_steps": "steps", "session_preserved_rows": "preserved", "session_folds": "folds", "session_folded_rows": "folded",
           "session_retained_rows": "retained", "session_released_rows": "released", "session_rescales": "_rescales",
           "session_sweep_points": "_swept", "session_loaded_rows": "preserved"}
# what a session is opened with; ``rescale`` alone replaces the first two.  Equal to the plain 4-tuple.
_Fixed = NamedTuple("_Fixed", [("lam", float), ("edit_weight", float), ("layers", tuple), ("num_edit_tokens", int)])


def _positive_weight(weight) -> float:
    try:
        w = float(weight)
    except (TypeError, ValueError) as e:
        raise ValueError(f"weight must be a positive finite number (got {weight!r})") from e
    if not (np.isfinite(w) and w > 0.0):
        raise ValueError(f"weight must be a positive finite number (got {weight!r})")
    return w


def _check_point(lam: float, e: float):
    if not (np.isfinite(lam) and lam > 0.0):
        raise ValueError(f"mom2_update_weight must be positive and finite in a session (got {lam}): the dual solver factors lam C'")
    if not (0.0 < e < 1.0):
        raise ValueError(f"edit_weight must lie inside (0, 1) in a session (got {e})")


def _source_names(sources) -> list:
    """``request["source"]`` strings, or request dicts, as a list of names."""
    return [s["source"] if isinstance(s, dict) else s for s in sources]


def check_session_state(state, fixed=None, rewrite_module_tmp=None, d=None, h=None, capacity=None) -> int:
    """The host half of ``EditSession.load``, pure: is ``state`` (the dict of a session file) whole and consistent in itself —
    format version, every tensor's shape and dtype against M / d / h / the layers, the ledger's length against M, the archive and
    its ledger against ``folded``, ``base`` present exactly when rows were folded — and, for the arguments that are given, does it
    agree with the session it is to continue: ``fixed`` (mom2_update_weight, edit_weight, layers, num_edit_tokens),
    ``rewrite_module_tmp``, ``d``, ``h``, and ``capacity`` >= M (default: the file's own).  Returns M; ``ValueError`` naming what is
    wrong otherwise.  No tensor's contents are read."""
    if not isinstance(state, dict) or "format" not in state:
        raise ValueError("not a session file: a dict with a 'format' entry is expected")
    if state["format"] != SESSION_FORMAT:
        raise ValueError(f"session file of unknown format {state['format']!r} (this version reads format {SESSION_FORMAT})")
    missing = [k for k in _SESSION_ENTRIES if k not in state]
    if missing:
        raise ValueError(f"session file without the entries {missing}")
    fx = state["fixed"]
    saved = (float(fx["mom2_update_weight"]), float(fx["edit_weight"]), tuple(fx["layers"]), int(fx["num_edit_tokens"]))
    if fixed is not None and tuple(fixed) != saved:
        raise ValueError(f"the session was saved with (mom2_update_weight, edit_weight, layers, num_edit_tokens) = {saved}, the hparams "
                         f"say {tuple(fixed)}: a loaded session continues with the values it was opened with")
    if rewrite_module_tmp is not None and rewrite_module_tmp != state["rewrite_module_tmp"]:
        raise ValueError(f"the session was saved for the weights {state['rewrite_module_tmp']!r}, the hparams name {rewrite_module_tmp!r}")
    for name, given in (("d", d), ("h", h)):
        if isinstance(state[name], bool) or not isinstance(state[name], int) or state[name] < 1:
            raise ValueError(f"session file: {name} must be a positive integer (got {state[name]!r})")
        if given is not None and int(given) != state[name]:
            raise ValueError(f"the session was saved for edited weights with {name} = {state[name]}, this encoder's have {name} = {given}")
    L, sd, sh = len(saved[2]), state["d"], state["h"]
    dp = (sd + hip.NB - 1) // hip.NB * hip.NB
    cap = state["capacity"] if capacity is None else capacity
    try:
        M = hip.check_preserved_state(state["keys"], L, sd, cap)
    except hip.EmcidHipError as e:
        raise ValueError(f"session file: {e}") from e
    counters = state["counters"]
    for k in _SESSION_COUNTERS:
        if isinstance(counters.get(k), bool) or not isinstance(counters.get(k), int) or counters[k] < 0:
            raise ValueError(f"session file: counter {k!r} must be a non-negative integer (got {counters.get(k)!r})")
    folded = counters["folded"]
    if len(state["ledger"]) != M:
        raise ValueError(f"session file: the ledger lists {len(state['ledger'])} rows, the state holds M = {M}")

    def tensors(name, shape, dtype, rows_at_least=None):
        ts = state[name]
        if not isinstance(ts, (list, tuple)) or len(ts) != L:
            raise ValueError(f"session file: {name} must be a list of {L} tensors, one per edited layer")
        for i, t in enumerate(ts):
            ok = isinstance(t, torch.Tensor) and t.dtype == dtype and t.dim() == len(shape) and tuple(t.shape[1:]) == tuple(shape[1:])
            if ok and rows_at_least is None:
                ok = t.shape[0] == shape[0]
            if not ok:
                got = (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"session file: {name}[{i}] must be a {dtype} tensor of {tuple(shape)} (got {got})")
            if rows_at_least is not None and t.shape[0] < rows_at_least:
                raise ValueError(f"session file: {name}[{i}] holds {t.shape[0]} rows, {rows_at_least} were folded")

    tensors("weights", (sh, sd), torch.float32)
    if state["orig"] is not None:
        tensors("orig", (sh, sd), torch.float32)
    base = state["base"]
    if (base is None) != (counters["folds"] == 0):
        raise ValueError(f"session file: {counters['folds']} folds, but the folded systems (base) are {'missing' if base is None else 'there'}")
    if base is not None and not (isinstance(base, torch.Tensor) and base.dtype == torch.float64 and tuple(base.shape) == (L, dp, dp)):
        raise ValueError(f"session file: base must be an f64 tensor of {(L, dp, dp)}")
    if state["keep_folded"]:
        if len(state["archive_ledger"]) != folded:
            raise ValueError(f"session file: the archive's ledger lists {len(state['archive_ledger'])} rows, {folded} were folded")
        if folded > 0 or state["archive"] is not None:
            tensors("archive", (folded, dp), torch.float64, rows_at_least=folded)
    elif state["archive"] is not None or len(state["archive_ledger"]):
        raise ValueError("session file: an archive on a session that does not keep what its folds added")
    return M


def _read_session_file(path) -> dict:
    """The dict of a session file: tensors and plain Python values only (``weights_only``), all on the host."""
    return torch.load(str(path), map_location="cpu", weights_only=True)


def _write_session_file(state: dict, path) -> int:
    """``torch.save`` to a temporary name beside ``path``, then renamed over it: an interrupted save leaves the previous file
    whole.  Returns the bytes written."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    tmp = path.with_name(f".{path.name}.{os.getpid()}.tmp")
    try:
        torch.save(state, str(tmp))
        os.replace(tmp, path)
    finally:
        if tmp.exists():
            tmp.unlink()
    return path.stat().st_size


class EditSession:
    """A sequence of ``apply_emcid_to_text_encoder`` calls on ONE text encoder in which every later edit keeps the keys of the
    earlier ones: step t solves against lam C' + P^T P + Kt^T Kt, P the stacked (scaled) keys of steps < t, where two plain calls
    solve the second one against lam C' alone and are free to move what the first call wrote.

        sess = EditSession(pipe, hparams, device, stats_dir=..., capacity=None)
        sess.apply(requests, cache_name=...)      # same mutations / return as apply_emcid_to_text_encoder
        sess.retain(requests, weight=1.0)         # "leave these where they are": their keys join the preserved set, no weight moves
        sess.preserved                            # M: preserved concept rows (requests x num_edit_tokens so far)
        sess.retained                             # rows added by retain() (folded ones included)
        sess.report()                             # report=True: what the last step did to the preserved keys and left of its residuals
        sess.release(sources)                     # take the rows of these request["source"] names out of the set again
        sess.rows(); sess.sources()               # the ledger: (source, "edit" | "retain", ordinal, token) per row; what release() can take
        sess.rescale(mom2_weight, edit_weight)    # the session's lam / edit_weight from now on; held rows keep their committed scale
        sess.apply(requests, point=(lam, e))      # ... rescale and step as ONE operation: a failed step takes the rescale back
        sess.reweight(sources, weight)            # these concepts count from now on like keys retained now at `weight`
        sess.sweep(requests, grid, scorer=...)    # trial steps at every (lam, e) of grid, nothing committed -> select_point
        sess.fold()                               # take the M preserved rows into the session's own base factor: M -> 0
        sess.folded                               # rows folded so far (still preserved, exactly)
        sess.folded_sources()                     # keep_folded=True: the names release() can take back out of the folds
        sess.reset()                              # forget the preserved keys (the weights stay as they are)
        sess.restore()                            # the weights of before the first step back, and the keys forgotten
        sess.save(path)                           # everything above to ONE file, between any two operations
        EditSession.load(pipe, hparams, path)     # ... and a session that carries on from it, in another process

    A step is a warm call's chain with the dual stage swapped for ``hip.edit_layer_dual_preserve``: the factors of lam C' come
    from the engine's factor cache under the key plain calls use (a session never refactors), the earlier keys live in factor
    coordinates per edited layer (``hip.PreservedKeys``: capacity x d + capacity^2 doubles per layer, allocated at the first
    step), and a step costs O(N (M + N) d).  All edited layers commit their rows together, after the one flag read at the end
    found every factorization sound; a failed or retried step leaves ``preserved`` where it was.

    A full set is FOLDED instead of dropped: ``fold()`` forms A0' = A0 + P^T P per edited layer (A0 = lam C' at the first fold, the
    previous fold's system afterwards; P = Yp L^T, the preserved keys back from factor coordinates), factors it once (d^3 / 3 per
    layer, ``hip.cov_factor_fold``) and goes on with M = 0 on these private factors — every folded key is still preserved exactly,
    since the system a later step solves is the same sum.  All layers are folded, then ONE pinned flag read decides: zero commits
    (M -> 0, ``folded`` += M, the session's steps take the private factors from now on), non-zero leaves ``preserved``, the
    private factors and the weights as they were and raises ``torch.linalg.LinAlgError``.  The private workspace is the
    session's alone: never put into the engine's factor cache, never handed to plain calls, never rescaled in place; plain
    calls, sweeps and other sessions keep the cached factors of lam C', which a fold only reads.  ``on_full="fold"`` makes a step
    that would pass ``capacity`` fold first (``"raise"``, the default: ``PreservedSetFull``).  State cost of a session that has
    folded, allocated at its first fold: one factored workspace (``emcid_cov_factor_workspace_bytes(n_layers, d)``) plus
    n_layers x dp^2 doubles of ``base``, the fp64 accumulator of the folded systems (dp = d rounded up to 128); a later fold
    keeps a copy of both for the time of the fold, so that a refused one leaves them as they were.  ``reset()`` and
    ``restore()`` drop the private factors and ``base`` and zero ``folded``.

    A RETAIN list (``retain``) names concepts no step may move: a retained key is a preserved row with a zero residual, so it takes
    the key half of a step (``hip.session_retain``: Yk, B, Lkp, T, its Cholesky, the append) and nothing else — no v* file, no
    Stage 1, no weight read by the solver or written; every parameter is bit-identical afterwards.  The keys are the mean fc2
    inputs at the requests' lookup rows under the weights AS THEY ARE NOW (the forward, lookups and num_edit_tokens rule of an edit
    step), scaled by sqrt(weight edit_weight / 0.5): weight 1 counts a retained key like an edited one.  A request needs
    ``prompts`` (or ``source_prompts``) and ``source`` only.  Capacity, ``fold()`` and ``on_full`` treat retained rows like any
    other; with ``on_full="fold"`` a list longer than ``capacity`` is taken in chunks of at most ``capacity`` rows with a fold
    between chunks (the weights do not change, so every chunk sees the same keys).

    RELEASE (``release``) takes named concepts out of the set again — to change an edit made twenty steps ago, whose own preserved
    row would otherwise hold the re-edit about half-way back, or to stop holding a retained concept.  No downdating: rows below
    the smallest released index already are the state of the reduced set, and the kept rows behind it re-enter as the key half of
    a step on the rows the session already holds in factor coordinates (``hip.session_release``: a gather, then B, Lkp, T, its
    Cholesky, the append) — no forward, no X, no statistics, no weight read or written; every parameter is bit-identical
    afterwards.  Releasing only the last rows (the last step, the last retain list) or all of them launches nothing.  Rows
    [first, M) and the touched tile inverses of every layer are copied first; all layers run, ONE pinned flag read decides, and a
    non-zero flag puts the copy back and raises ``torch.linalg.LinAlgError`` with nothing released.  ``retained`` drops by the
    retained rows released; a stored ``report()`` readout is dropped (``None`` until the next step).  A fold empties the ledger:
    folded sources live inside the base factor and cannot be released (``ValueError``; ``restore()`` starts over) — unless the
    session keeps what its folds added:

    ``keep_folded=True`` makes every fold (``fold()``, the automatic one of ``on_full="fold"``, the chunked ones of ``retain``)
    ARCHIVE its rows: a fold adds q_i q_i^T to ``base`` for the rows Q = Yp L^T, and writes Q into the tail of a session-owned fp64
    archive (n_layers tensors [rows, dp], grown geometrically) instead of a scratch buffer — no further launch, no copy; the ledger
    entries move into an archive ledger (``folded_sources()``) while ``rows()`` / ``sources()`` still list live rows only.
    ``release`` of a name with archived rows is then a REFOLD, with no Cholesky downdate: per edited layer the M live rows join the
    archive as Q and ``base`` += Q^T Q (``hip.session_refold_update``: a fold's first two stages), ``base`` -= q_i q_i^T for the
    released rows, archived and just-added live ones alike, and ``base`` is factored again — all layers in ONE batched chain
    (``hip.cov_factor_refactor``) where a fold runs one serial chain per layer.  ONE pinned flag read decides, like ``fold()``:
    zero commits everything together (M -> 0: the live set is folded as a side effect, exactly preserved and still releasable;
    the archive and its ledger are compacted; ``folded`` = folded + M_kept - released archived rows; ``folds`` += 1; ``released`` /
    ``retained`` adjusted; the stored ``report()`` dropped), non-zero puts the private workspace and ``base`` back from the copies
    taken first, leaves the archive's length alone and raises ``torch.linalg.LinAlgError`` with nothing released.  No weight is
    read or written.  A release that names live rows only is the plain one above.  Subtracting q_i q_i^T reverses the addition up to
    the rounding of ``base``: ~1e-15 of max|L| on the factor when lam C' carries the system, ~1e-13 when the keys outweigh it 30 x
    (DESIGN.md §3).  Cost of the archive: folded x dp doubles per edited layer — 45 MB per layer per full fold (1 843 rows) at
    d = 3 072 — held until ``reset()`` / ``restore()``, which drop it.  The default (``False``) allocates and launches what it did.

    RESCALE / REWEIGHT / SWEEP change how strongly the session edits and holds, from evidence.  The held rows live in factor
    coordinates Yp = P L_s^-T, L_s = chol(lam C'); with a = 2 lam (1 - e) the base term is a C and chol(a' C) = sqrt(a' / a) chol(a C),
    so another (lam', e') multiplies every row of Yp by rho = sqrt(a / a') and another weight w' of a concept held at w multiplies its
    rows by sqrt(w' / w); Lp = chol(I + Yp Yp^T) and the tile inverses behind the first changed row are rebuilt by the key half a
    release runs (``hip.session_rescale``: one scaling pass, then B, Lkp, T, its Cholesky, the append) — no forward, no X, no
    statistics, no weight read or written.  ``rescale`` keeps P (a held row keeps the raw scale it was committed with; only the base
    term moves) and re-points the factors later steps, ``fold()`` and ``save`` refer to at those of the new point, from the factor
    cache as a step takes them; the scalar cannot reproduce the fp32 rounding of C (1 - e) / 0.5 (the reference's C'), an offset far
    below the bar, and with e unchanged it is exact.  ``reweight`` takes its factors from the host ``row_scale``.
    Both are atomic like ``release`` (copy, all layers, ONE pinned flag read, commit or put back and ``torch.linalg.LinAlgError``).
    ``sweep`` prepares the requests once, copies the held state once, and per pair scales the live state out of the copy, runs the
    step's chain on one unit factorization rescaled to the pair (``hip.cov_factor_rescale``), fills the pair's entry
    (``EditScorer.score()``, ``report()``, ``visit``) and puts the weights back; in a ``finally`` the state goes back byte for byte.
    All three refuse a session that has folded (its base a C + Pf^T Pf is a sum no scalar rescales), a collective shard and
    EMCID_SOLVER=direct|lu before anything is launched or allocated.

    SAVE / LOAD carry a session across processes.  ``save(path)`` writes the fixed set-up, counters and ledgers, the COMMITTED rows
    of every layer without their padding or anything of the capacity (``hip.PreservedKeys.state_dict``: Yp[:M, :d], Lp[:M, :M], the
    tile inverses rows < M touch), the edited weights as they are and as they were before the first step, ``base`` of a folded
    session — not its factored workspace, four times the size and rebuilt by one batched chain (``hip.cov_factor_from_base``) —, the
    counted rows of the archive, and a content fingerprint (``hip.fingerprint_content``: the stale-cache guard's word without the
    address) of every other parameter of the encoder and of each edited layer's statistics; one synchronising copy, one file,
    renamed into place.  ``load`` checks the file on the host (``check_session_state``), refuses another encoder, other statistics
    or — ``weights="check"`` — other edited weights with ``ValueError`` and the encoder untouched, takes the factors of lam C' from
    the engine's factor cache as a step does, allocates the state at ITS capacity (any value >= M) and copies the rows and tiles to
    where that layout wants them; ONE pinned read decides.  The stored ``report()`` readout is not saved (``None`` until the next
    step).  A session that is never saved or loaded allocates and launches what it did.

    ``report=True`` adds one launch per edited layer to a step (``hip.session_step_norms``, from what the step left in its
    workspace: with Z = (I + Y Y^T)^-1 [0; Rt] the step moves preserved key i by dW p_i = -Zp_i and leaves Zk_j of residual j);
    ``report()`` reads the session's buffer (one synchronisation) and returns {weight name: {"drift": (rows preserved before the
    step,) ||dW k_i|| in raw-key units, in the order the rows were added since the last fold — folded rows stay preserved but
    are no longer listed —, "left": (N,) ||Zk_j|| / ||Rt_j||}}, ``None`` before any step.  ``report=False``: a step issues exactly
    the launches it issued before.

    ``device``: as in apply_emcid_to_text_encoder; the state lives on the encoder's own device, ``device`` is only checked against it.
    ``capacity``: the largest M + N (default floor(0.6 d), the engine's dual / direct threshold); a step past it raises
    ``PreservedSetFull`` before anything is launched (with ``on_full="fold"``: only a step that exceeds it by itself).
    layers and num_edit_tokens are fixed at construction, mom2_update_weight and edit_weight change through ``rescale`` alone
    (``hparams`` may be mutated by hand afterwards, a step then refuses).  Not run by a session: several ranks (a collective
    ``ConceptShard``), SDXL, cross-attention edits, EMCID_SOLVER=direct|lu; there is no pivoted-LU fallback either — a
    non-positive pivot restores the weights and raises ``torch.linalg.LinAlgError``."""

    def __init__(self, pipe, hparams: EMCIDHyperParams, device: Optional[str] = None, stats_dir=STATS_DIR,
                 capacity: Optional[int] = None, verbose: bool = False, on_full: str = "raise", report: bool = False,
                 keep_folded: bool = False):
        if on_full not in ("raise", "fold"):
            raise ValueError(f"on_full must be 'raise' or 'fold' (got {on_full!r})")
        if isinstance(hparams, EMCIDXLHyperParams) or getattr(pipe, "text_encoder_2", None) is not None:
            raise NotImplementedError("EditSession edits one CLIP text encoder: the SDXL pair (EMCIDXLHyperParams / text_encoder_2) "
                                      "is not supported")
        if not isinstance(hparams, EMCIDHyperParams):
            raise TypeError(f"hparams must be EMCIDHyperParams, got {type(hparams).__name__}")
        if not hparams.layers or sorted(hparams.layers) != list(hparams.layers):
            raise ValueError(f"hparams.layers must be a non-empty list in forward order (got {hparams.layers})")
        ws = []
        for layer in hparams.layers:
            try:
                ws.append(nethook.get_parameter(pipe.text_encoder, f"{hparams.rewrite_module_tmp.format(layer)}.weight"))
            except LookupError as e:
                raise NotImplementedError(f"EditSession edits the text encoder's MLP projections; {hparams.rewrite_module_tmp!r} names "
                                          f"no weight of pipe.text_encoder (cross-attention edits are not supported): {e}") from e
        if any(w.dim() != 2 or w.shape != ws[0].shape for w in ws):
            raise ValueError("the edited weights must be matrices of one shape")
        lam, e = float(hparams.mom2_update_weight), float(hparams.edit_weight)
        _check_point(lam, e)
        self.h, self.d = int(ws[0].shape[0]), int(ws[0].shape[1])
        if capacity is None:
            capacity = int(0.6 * self.d)
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer (got {capacity!r})")
        if device is not None and torch.device(device).type != ws[0].device.type:
            raise ValueError(f"device {device!r} but the text encoder's weights live on {ws[0].device}")
        self.pipe, self.hparams, self.stats_dir, self.verbose = pipe, hparams, stats_dir, verbose
        self.capacity, self.on_full = int(capacity), on_full
        self._fixed = _Fixed(lam, e, tuple(hparams.layers), int(getattr(hparams, "num_edit_tokens", 1)))
        self.keys: Optional[hip.PreservedKeys] = None       # allocated at the first step
        self._orig: Optional[Dict[int, torch.Tensor]] = None
        self._ws: Dict[tuple, hip.PreserveWorkspace] = {}
        self.report_on, self.keep_folded = bool(report), bool(keep_folded)
        self._forget()

    def _forget(self):
        """The state of a session that holds no key: what ``__init__`` starts from and ``reset()`` goes back to."""
        # steps; folds, folded: how often and how many rows went into the private base factor; retained: rows added by retain(),
        # folded ones included; released: rows released so far; _retains: retain() calls so far (the ordinal of a retained row)
        for attr in _COUNTER_ATTRS.values():
            setattr(self, attr, 0)
        self.private_factors: Optional[hip.CovFactors] = None    # the factors of lam C' + (folded P)^T P: this session's steps only
        self._base: Optional[torch.Tensor] = None            # (n_layers, dp, dp) f64: the folded systems themselves
        self._shared = None     # (factors, covs) of the last sound step: what the preserved rows' coordinates refer to
        self._report = self._report_pending = None           # (buffer (n_layers, M + 2 N) f64 in HBM, M, N, row scales) of the last sound step
        self._ledger: List[tuple] = []                       # per live row since the last fold: (source, "edit" | "retain", ordinal, token)
        self._folded_sources: set = set()                    # sources whose rows a fold took: no longer releasable
        self._release_ws: Optional[hip.ReleaseWorkspace] = None
        self._rescale_ws: Optional[hip.RescaleWorkspace] = None
        self._rescales = 0                                   # hip.session_rescale calls so far (LAST_PATHS session_rescales)
        self._swept = 0                                      # points the last sweep ran (LAST_PATHS session_sweep_points)
        self._archive: Optional[List[torch.Tensor]] = None   # keep_folded: per edited layer (rows, dp) f64, the Q rows every fold added
        self._archived = 0                                   # rows of the archive that count (== folded on a keep_folded session)
        self._archive_ledger: List[tuple] = []               # their ledger entries, in archive order

    @property
    def preserved(self) -> int:
        return self.keys.M if self.keys is not None else 0

    def fold(self):
        """Take the ``preserved`` rows of every edited layer into the session's private base factor and go on with M = 0; the
        folded keys stay preserved exactly.  A no-op without preserved rows.  One flag read; a non-positive pivot leaves
        ``preserved``, ``folded``, the private factors and the weights as they were and raises ``torch.linalg.LinAlgError``."""
        M = self.preserved
        if M == 0:
            return
        dev = self.keys.Yp[0].device
        if not self.keys.Yp[0].is_cuda or self._shared is None:
            raise hip.EmcidHipError(f"a fold runs on the factors of the session's last step in HBM (state on {dev}); there is no CPU path")
        fx, n = self._fixed, len(self._fixed.layers)
        first = self.private_factors is None
        src = self._shared[0] if first else self.private_factors
        if first:
            dst = hip.CovFactors(n, self.d, dev)
            base = torch.empty(n, dst.dp, dst.dp, dtype=torch.float64, device=dev)
        else:
            dst, base = src, self._base
        undo = None if first else self._keep_private(dst, base)     # (a refused first fold just drops its dst and base)
        if self.keep_folded:                        # Q lands in the archive's tail: the fold entry leaves it there
            self._archive_room(M, dst.dp, dev)
            tails = [a[self._archived:self._archived + M].view(-1) for a in self._archive]
        else:
            tails = [torch.empty(M * dst.dp, dtype=torch.float64, device=dev)] * n

        def launch():
            for i in range(n):
                hip.cov_factor_fold(src, self.keys, i, self._shared[1][i] if first else None, fx.lam, fx.edit_weight, dst, base,
                                    ws=tails[i])

        self._atomic(dst.info, launch, undo, lambda code: (
            f"fold after step {self.steps}: lam C' plus the {self.folded} folded and {M} preserved keys is not positive definite "
            f"(non-positive pivot at column {code - 1}): check the statistics; the {M} preserved rows, the private factors and "
            f"the weights are as they were"))
        self.private_factors, self._base = dst, base
        self.keys.reset()
        if self.keep_folded:
            self._archive_ledger += self._ledger
            self._archived += M
        else:
            self._folded_sources.update(row[0] for row in self._ledger)
        self._ledger = []
        self.folded += M
        self.folds += 1
        self._publish("session_folds", "session_folded_rows", "session_preserved_rows")
        self._say(f"Session fold {self.folds}: {M} preserved rows folded into the base factor, {self.folded} folded so far")

    def _say(self, text: str):
        if self.verbose:
            print(text)

    def _publish(self, *names):
        for name in names:
            clip_forward.LAST_PATHS[name] = getattr(self, _GAUGES[name])

    @classmethod
    def _atomic(cls, info: torch.Tensor, launch, undo, refuse, also: Optional[torch.Tensor] = None):
        """All layers or nothing: zero the flag word ``info``, ``launch()``, ONE pinned flag read (``also``: a second word read with it,
        the larger counts); zero returns, non-zero: ``undo()`` if any, ``info`` zeroed, ``torch.linalg.LinAlgError(refuse(code))``."""
        info.zero_()
        launch()
        code, = cls._read_flag(info if also is None else torch.maximum(info, also.to(info.device)))
        if code != 0:
            if undo is not None:
                undo()
            info.zero_()
            raise torch.linalg.LinAlgError(refuse(code))

    @staticmethod
    def _keep_private(fac, base: torch.Tensor):
        """Copy a folded session's private workspace and ``base`` now; returns ``undo()``, which puts both back."""
        kept = (fac.buf.clone(), base.clone())

        def undo():
            fac.buf.copy_(kept[0])
            base.copy_(kept[1])
            fac.have_inverse = set(range(fac.n_layers))

        return undo

    def _rebuild_ws(self, slot: str, cls, n_rebuilt: int):
        """The workspace in ``slot`` for a rebuild of ``n_rebuilt`` rows; one of another size is freed BEFORE its successor is allocated."""
        dims = (n_rebuilt, self.keys.d, self.keys.capacity)
        if getattr(self, slot) is None or getattr(self, slot).key != dims:
            setattr(self, slot, None)
            setattr(self, slot, cls(*dims, self.keys.Yp[0].device))
        return getattr(self, slot)

    def _archive_room(self, M: int, dp: int, dev):
        """Make the archive of every edited layer hold ``M`` more rows: at least doubled when it has to grow (the rows that count
        are copied over), allocated at the first fold that keeps its rows."""
        need = self._archived + M
        if self._archive is None:
            self._archive = [torch.zeros(need, dp, dtype=torch.float64, device=dev) for _ in self._fixed.layers]
        elif self._archive[0].shape[0] < need:
            rows = max(need, 2 * self._archive[0].shape[0])
            for i, old in enumerate(self._archive):
                new = torch.zeros(rows, dp, dtype=torch.float64, device=dev)
                new[:self._archived].copy_(old[:self._archived])
                self._archive[i] = new

    def workspace(self, N: int, d: int, h: int, dev, retain: bool = False):
        """(engine side) the workspace of a step (``retain``: of a retain call) of N rows; the two most recent sizes keep theirs"""
        key = (N, d, h, str(dev), bool(retain))
        ws = self._ws.pop(key, None)
        if ws is None:
            ws = hip.RetainWorkspace(N, d, self.capacity, dev) if retain else hip.PreserveWorkspace(N, d, h, self.capacity, dev)
            while len(self._ws) >= 2:
                self._ws.pop(next(iter(self._ws)))
        self._ws[key] = ws
        return ws

    def report_row(self, i: int, N: int) -> torch.Tensor:
        """(engine side) where edited layer ``i`` of the step in flight writes its M + 2 N norms"""
        if self._report_pending is None:
            M = self.preserved
            buf = torch.empty(len(self._fixed.layers), M + 2 * N, dtype=torch.float64, device=self.keys.Yp[0].device)
            self._report_pending = (buf, M, N, self.keys.row_scale[:M].clone())
        return self._report_pending[0][i]

    def report(self):
        """The readout of the last sound step of a ``report=True`` session (class docstring), ``None`` before any."""
        if self._report is None:
            return None
        buf, M, N, scale = self._report
        host = buf.cpu()                            # the one synchronising read
        out = {}
        for i, l in enumerate(self._fixed.layers):
            row = host[i]
            resid = row[M + N:M + 2 * N]
            out[f"{self.hparams.rewrite_module_tmp.format(l)}.weight"] = {
                "drift": row[:M] / scale,
                "left": torch.where(resid > 0, row[M:M + N] / resid.clamp(min=torch.finfo(torch.float64).tiny), torch.zeros_like(resid))}
        return out

    def _check_call(self, requests, shard, what="a session step"):
        hp = self.hparams
        now = (float(hp.mom2_update_weight), float(hp.edit_weight), tuple(hp.layers), int(getattr(hp, "num_edit_tokens", 1)))
        if now != self._fixed:
            raise ValueError(f"a session's mom2_update_weight, edit_weight, layers and num_edit_tokens are fixed: it was opened with "
                             f"{tuple(self._fixed)}, the hparams now say {now}; open a new EditSession")
        if emcid_main._shard_from_env(shard).collective:
            raise NotImplementedError("EditSession runs on one rank: a multi-rank ConceptShard is not supported")
        forced = edit_engine.SOLVER or os.environ.get("EMCID_SOLVER")
        if forced in ("direct", "lu"):
            raise ValueError(f"EMCID_SOLVER={forced} inside a session: the preserved keys live in the dual solver's coordinates")
        if len(requests) == 0:
            raise ValueError(f"{what} needs at least one request")

    def _check_step(self, requests, shard):
        self._check_call(requests, shard)
        n = len(requests) * self._fixed.num_edit_tokens
        if self.preserved + n > self.capacity and not (self.on_full == "fold" and n <= self.capacity):    # (else apply() folds first)
            raise PreservedSetFull(f"{self.preserved} preserved + {n} new concept rows exceed the session's capacity {self.capacity}; "
                                   f"open a session with a larger capacity, or with on_full='fold' (sess.fold() takes a full set into "
                                   f"the session's base factor)")
        return n

    def _weights(self):
        return {l: nethook.get_parameter(self.pipe.text_encoder, f"{self.hparams.rewrite_module_tmp.format(l)}.weight")
                for l in self._fixed.layers}

    def _weights_in_hbm(self):
        """(``_weights()``, their device), which must be a GPU."""
        weights = self._weights()
        w = next(iter(weights.values()))
        if not w.is_cuda:
            raise hip.EmcidHipError(f"the text encoder must live in HBM (got {w.device}); there is no CPU path")
        return weights, w.device

    def _prepare(self, requests, shard, cache_name=None, stage1=None, **kw):
        hp = self.hparams
        return emcid_main.prepare_text_encoder_edit(self.pipe.text_encoder, self.pipe.tokenizer, requests, hp, hp.layers, hp.mom2_update_weight,
                                                    self.stats_dir, cache_name, "", self.verbose, shard, stage1, **kw)

    def _ensure_keys(self):
        """Allocate the preserved key set at the first step or retain list, on the encoder's device (HBM only)."""
        if self.keys is None:
            self.keys = hip.PreservedKeys(len(self._fixed.layers), self.d, self.capacity, self._weights_in_hbm()[1])

    @staticmethod
    def _read_flag(info: torch.Tensor) -> List[int]:
        """The ONE synchronising read of an operation: the device flag words ``info`` (int32) through pinned memory, after
        everything queued on the current stream of their device."""
        flag = hip.pinned_copy(info)
        torch.cuda.current_stream(info.device).synchronize()
        return flag.tolist()

    def _run_plan(self, make_plan, restore_weights: bool, method: str, redo: str, keys: str, where: str, undone: str = ""):
        """Run the plan ``make_plan()`` returns as this session's and return it once every factorization was sound; nothing is
        committed here.  Any failure releases the plan's workspaces (``restore_weights``: and puts the edited weights back); a
        weight rewritten behind the forward's caches (``StaleWeightCacheError``) has the plan made and run again once, from the live
        weights, M unchanged; a non-positive pivot becomes ``torch.linalg.LinAlgError``.  The other arguments word the messages."""
        LP = clip_forward.LAST_PATHS
        for attempt in (0, 1):
            plan = make_plan()
            plan.session = self
            stats_flag = None
            self._report_pending = None
            try:
                try:
                    with phase("run + final sync"):
                        run_encoder_edit(plan, keep_factors=False, restore=False)
                except BaseException:
                    if restore_weights:
                        plan.restore_weights()
                    edit_engine._release_workspaces(plan)
                    raise
                # (check_info drops a failed plan's own factors: keep their flag word to tell which factorization said no)
                stats_flag = plan.cov_factors.info if plan.cov_factors is not None else None
                check_info(plan)                    # restores the weights itself before it raises
                return plan
            except clip_forward.StaleWeightCacheError as e:
                if attempt == 1:
                    raise
                emcid_main._note_stale(f"EditSession.{method}", e, redo)
                LP["stale_cache_retries"] = LP.get("stale_cache_retries", 0) + 1
            except FloatingPointError as e:
                what = "the statistics lam C' themselves are not positive definite" if stats_flag is not None and int(stats_flag.item()) \
                    else f"the system of the {keys} keys given the {self.preserved} preserved ones is not positive definite"
                raise torch.linalg.LinAlgError(
                    f"{where}: {what} ({e}); {undone}nothing was added to the {self.preserved} preserved rows") from e

    def apply(self, requests: List[Dict], cache_name: Optional[str] = None, return_orig_text_encoder: bool = False, shard=None,
              stage1=None, point=None):
        """One step: edit ``requests`` with every earlier step's keys preserved.  Returns what apply_emcid_to_text_encoder does.
        ``point=(mom2_weight, edit_weight)``: ``rescale`` to that pair, then the step, as ONE operation — a step that fails (a
        non-positive pivot, a stale-cache retry that fails again, any exception) takes the rescale back with it."""
        n = self._check_step(requests, shard)       # raises before anything is launched or allocated
        if point is not None:
            (lam_p, e_p), = edit_engine.validate_grid([point])
            self._refuse_rescale(shard, "apply(point=)")
            if self.preserved + n > self.capacity:
                raise ValueError(f"apply(point=): {self.preserved} preserved + {n} new rows would fold the set first, and a session "
                                 f"that has folded (one that steps on private factors) cannot be rescaled; fold() and keep the "
                                 f"session's point, or rescale() before the set is full")
            undo = self._rescale(lam_p, e_p, shard, "apply(point=)")
            try:
                return self.apply(requests, cache_name, return_orig_text_encoder, shard, stage1)
            except BaseException:
                undo()
                raise
        if self.preserved + n > self.capacity:      # (on_full="fold": the step fits once the preserved rows are folded)
            self.fold()
        origin_text_encoder = deepcopy(self.pipe.text_encoder) if return_orig_text_encoder else None
        if self._orig is None:
            self._orig = {l: w.detach().clone() for l, w in self._weights().items()}
        self._ensure_keys()
        emcid_main._announce(requests, self.verbose)
        plan = self._run_plan(lambda: self._prepare(requests, shard, cache_name, emcid_main._default_stage1(self.pipe, self.hparams, stage1)),
                              True, "apply", "step", "new", f"session step {self.steps}", "the edited weights have been restored and ")
        self._commit_rows(plan, n, "edit", self.steps + 1, requests)
        self.steps += 1
        if self._report_pending is not None:
            self._report, self._report_pending = self._report_pending, None
        self._publish("session_steps", "session_preserved_rows", "session_folds", "session_folded_rows")
        self._say(f"Session step {self.steps}: {n} concept rows inserted, {self.keys.M} preserved")
        return self.pipe, origin_text_encoder

    def _commit_rows(self, plan, n: int, kind: str, ordinal: int, requests, weight: float = 1.0):
        """The ``n`` rows a sound plan left behind row M count from now on, in all edited layers together, as ``kind`` rows."""
        fx = self._fixed
        self.keys.commit(n, hip.row_scale_of(fx.edit_weight, plan.cov_factors, fx.lam, weight))
        self._ledger += [(r.get("source"), kind, ordinal, t) for r in requests for t in range(fx.num_edit_tokens)]
        if self.private_factors is None:            # the workspace these rows are coordinates of, and its statistics
            self._shared = (plan.cov_factors, [plan.covs[l] for l in plan.layers])

    def retain(self, requests: List[Dict], weight: float = 1.0, shard=None) -> int:
        """Enter the keys of ``requests`` into the preserved set with a zero residual: later steps leave these concepts where they
        are (class docstring).  ``weight``: how much a retained key counts against an edited one (finite, > 0).  No parameter of the
        encoder changes.  Returns the rows added (len(requests) x num_edit_tokens).  Refuses what ``apply`` refuses; with
        ``on_full="raise"`` a list that does not fit raises ``PreservedSetFull`` before anything is launched, with ``"fold"`` the set
        is folded first, and a list longer than ``capacity`` goes in chunks with a fold between them.  A non-positive pivot raises
        ``torch.linalg.LinAlgError`` with nothing committed (of the chunk in flight)."""
        w = _positive_weight(weight)
        self._check_call(requests, shard, "a retain list")
        k = self._fixed.num_edit_tokens
        n, per = len(requests) * k, self.capacity // k
        if self.preserved + n <= self.capacity:
            chunks = [list(requests)]
        elif self.on_full == "fold" and per >= 1:
            chunks = [list(requests[a:a + per]) for a in range(0, len(requests), per)]
        else:
            raise PreservedSetFull(f"{self.preserved} preserved + {n} retained concept rows exceed the session's capacity "
                                   f"{self.capacity}; open a session with a larger capacity, or with on_full='fold' (the list is "
                                   f"then taken in chunks, the set folded into the session's base factor between them)")
        self._retains += 1
        for chunk in chunks:
            self._retain_chunk(chunk, w, shard)
        return n

    def _retain_chunk(self, requests, w, shard):
        n = len(requests) * self._fixed.num_edit_tokens
        if self.preserved + n > self.capacity:
            self.fold()
        self._ensure_keys()

        def make_plan():
            plan = self._prepare(requests, shard, with_targets=False)
            plan.retain_weight = w
            return plan

        plan = self._run_plan(make_plan, False, "retain", "call", "retained", f"retain after step {self.steps}")   # (writes no weight)
        self._commit_rows(plan, n, "retain", self._retains, requests, w)
        self.retained += n
        self._publish("session_preserved_rows", "session_retained_rows", "session_folds", "session_folded_rows")
        self._say(f"Session retain: {n} concept rows retained at weight {w:g}, {self.keys.M} preserved")

    def rows(self) -> List[tuple]:
        """The ledger: one ``(source, "edit" | "retain", step or retain ordinal, token index)`` per preserved row, in row order since
        the last fold."""
        return list(self._ledger)

    def sources(self) -> List[str]:
        """The distinct sources that ``release`` can take, in the order they first entered."""
        return list(dict.fromkeys(row[0] for row in self._ledger))

    def folded_sources(self) -> List[str]:
        """The distinct sources whose rows the folds of a ``keep_folded`` session archived, in the order they first entered: what
        ``release`` can take back out of the base factor.  Empty on a default session."""
        return list(dict.fromkeys(row[0] for row in self._archive_ledger))

    def release(self, sources, shard=None) -> int:
        """Take every live row of ``sources`` (``request["source"]`` strings, or request dicts) out of the preserved set — all
        ``num_edit_tokens`` rows of a request, every occurrence of a source entered more than once — so that the concept can be
        edited again, or is no longer held (class docstring).  No weight changes.  Returns the rows released.  ``KeyError``: a source
        without a preserved row; ``ValueError``: a folded source, an empty list, and what ``apply`` refuses; all before anything is
        launched or allocated.  A non-positive pivot raises ``torch.linalg.LinAlgError`` with the state as it was.  On a
        ``keep_folded`` session a folded source goes too: the release is then a refold of every edited layer (class docstring),
        which takes the live rows into the base factor on its way (``preserved`` is 0 afterwards)."""
        names = _source_names(sources)
        self._check_call(names or [None], shard, "a release")
        if self.keep_folded and names and not {row[0] for row in self._archive_ledger}.isdisjoint(names):
            return self._release_refold(names)
        keep, first, n_retained = release_plan(self._ledger, self._folded_sources, names)
        M, kept = self.preserved, len(keep)
        assert M == len(self._ledger)
        if first < kept:                            # (trailing rows only, or every row: the set is truncated, nothing to launch)
            self._release_rebuild(keep, first, M)
        self.keys.release_commit(keep)
        self._ledger = [self._ledger[i] for i in keep]
        self.retained -= n_retained
        self.released += M - kept
        self._report = self._report_pending = None  # (its drift order is the old ledger's)
        self._publish("session_released_rows", "session_preserved_rows", "session_retained_rows")
        self._say(f"Session release: {M - kept} rows of {len(set(names))} sources released, {kept} preserved")
        return M - kept

    def _release_rebuild(self, keep, first, M):
        """The device half of a release: rows [first, len(keep)) of every edited layer rebuilt in place from the kept rows
        (``hip.session_release``), atomically (``_atomic``): a refused one puts rows [first, M) and their tile inverses back."""
        keys, n_rebuilt = self.keys, len(keep) - first
        ws = self._rebuild_ws("_release_ws", hip.ReleaseWorkspace, n_rebuilt)
        keep_dev = torch.tensor(keep, dtype=torch.int32, device=keys.Yp[0].device)
        snap = keys.snapshot(first, M)

        def launch():
            for i in range(keys.n_layers):
                hip.session_release(keys, i, keep_dev, first, ws=ws)

        self._atomic(ws.info, launch, snap.restore, lambda code: (
            f"release after step {self.steps}: the system of the {n_rebuilt} kept rows behind row {first} is not positive definite "
            f"(non-positive pivot at column {code - 1}); the {M} preserved rows are as they were and nothing was released"))

    def _release_refold(self, names) -> int:
        """A release that names archived rows: update every edited layer's ``base`` (``hip.session_refold_update``), factor all of
        them in one batched chain (``hip.cov_factor_refactor``), ONE pinned flag read, then commit or put everything back."""
        arch, live, n_retained = refold_plan(self._ledger, self._archive_ledger, names)
        keys, fac, base, n0 = self.keys, self.private_factors, self._base, self._archived
        M = self.preserved
        assert M == len(self._ledger) and n0 == len(self._archive_ledger) and fac is not None
        dev = fac.buf.device
        rel = arch + [n0 + i for i in live]
        if M > 0:
            self._archive_room(M, fac.dp, dev)
        rel_dev = torch.tensor(rel, dtype=torch.int32, device=dev)
        undo = self._keep_private(fac, base)                # (a refused refold puts both back)

        def launch():
            for i in range(keys.n_layers):
                hip.session_refold_update(fac, keys, i, self._archive[i], n0, rel_dev, base)
            hip.cov_factor_refactor(fac)

        self._atomic(fac.info, launch, undo, lambda code: (
            f"release after step {self.steps}: the folded system without the {len(rel)} released rows is not positive definite "
            f"(non-positive pivot at column {code - 1}); the {M} preserved and {n0} folded rows, the private factors and the "
            f"weights are as they were and nothing was released"))
        del undo                                            # (and the copies with it)
        gone = set(rel)
        stay = [k for k in range(rel[0], n0 + M) if k not in gone]      # (rows below the first released one stay where they are)
        if stay:
            idx = torch.tensor(stay, dtype=torch.long, device=dev)
            for a in self._archive:
                a[rel[0]:rel[0] + len(stay)] = a.index_select(0, idx)
        both = self._archive_ledger + self._ledger
        self._archive_ledger = both[:rel[0]] + [both[k] for k in stay]
        self._archived = len(self._archive_ledger)
        self._ledger = []
        keys.reset()
        self.folded += (M - len(live)) - len(arch)
        self.folds += 1
        self.retained -= n_retained
        self.released += len(rel)
        self._report = self._report_pending = None
        self._publish("session_released_rows", "session_preserved_rows", "session_retained_rows", "session_folds", "session_folded_rows")
        self._say(f"Session release: {len(arch)} folded and {len(live)} live rows of {len(set(names))} sources released by a refold, "
                  f"{self.folded} folded")
        return len(rel)

    # ---- another point, another weight, a sweep of one step -------------------------------------------------------------------

    def _refuse_rescale(self, shard, what: str):
        """What rescale / reweight / sweep refuse before anything is launched or allocated, on top of ``_check_call``."""
        self._check_call([None], shard, what)
        if self.private_factors is not None or self.folded > 0:
            # (private factors outlive their rows: a keep_folded session that released every folded source still steps on them)
            raise ValueError(f"{what} on a session that has folded ({self.folded} folded rows, {self.folds} folds): its steps run on "
                             f"private factors of a C + Pf^T Pf at the point of the fold, a sum no scalar rescales (base += (a' - a) C "
                             f"and a refactorization is not implemented); restore() starts over")

    def _scale_rows(self, dev_factors: torch.Tensor, first: int, what: str, extra_info: Optional[torch.Tensor] = None):
        """The device half of rescale / reweight: rows [first, M) of every edited layer scaled by ``dev_factors`` (M,) and rebuilt
        (``hip.session_rescale``), atomically (``extra_info``: a second flag word).  Returns ``undo()``, which puts the snapshot back."""
        keys, M = self.keys, self.preserved
        ws = self._rebuild_ws("_rescale_ws", hip.RescaleWorkspace, M - first)
        snap = keys.snapshot(first, M)

        def launch():
            for i in range(keys.n_layers):
                hip.session_rescale(keys, i, dev_factors, first, ws=ws)
            self._rescales += keys.n_layers
            self._publish("session_rescales")

        self._atomic(ws.info, launch, snap.restore, lambda code: (
            f"{what} after step {self.steps}: the system of the {M - first} scaled rows behind row {first} (or lam C' at the new "
            f"point) is not positive definite (non-positive pivot at column {code - 1}); the {M} preserved rows, the session's "
            f"point and the weights are as they were"), also=extra_info)
        return snap.restore

    def _rescale(self, mom2_weight, edit_weight, shard, what: str):
        """``rescale`` proper; returns ``undo()``, which makes the session what it was before (``apply(point=)`` calls it when its
        step fails)."""
        lam0, e0, layers, k = self._fixed
        try:
            lam = lam0 if mom2_weight is None else float(mom2_weight)
            e = e0 if edit_weight is None else float(edit_weight)
        except (TypeError, ValueError) as err:
            raise ValueError(f"mom2_weight and edit_weight must be numbers (got {mom2_weight!r}, {edit_weight!r})") from err
        _check_point(lam, e)
        self._refuse_rescale(shard, what)
        if (lam, e) == (lam0, e0):                  # (the point it is at: nothing to scale, nothing to drop)
            return lambda: None
        hp, M = self.hparams, self.preserved
        before = (self._fixed, hp.mom2_update_weight, hp.edit_weight, self._shared, self._report)
        undo_rows = None
        if M > 0:
            keys = self.keys
            dev = keys.Yp[0].device
            old, covs = self._shared
            # the factors of (lam', e') the later steps, fold() and save / load take the rows as coordinates of: the factor cache's,
            # or one batched factorization handed to it
            fac, commit = edit_engine.session_factors(self.pipe.text_encoder, layers, hp.rewrite_module_tmp, lam, e,
                                                      dict(zip(layers, covs)), dev)
            rho = math.sqrt((lam0 * (1.0 - e0)) / (lam * (1.0 - e)))
            undo_rows = self._scale_rows(torch.full((M,), rho, dtype=torch.float64, device=dev), 0, what, fac.info)
            commit()
            # report() divides by row_scale = (raw scale) / sqrt(lam_ratio of the factors in use): P keeps its raw scale, the unit moves
            keys.rescale_commit(math.sqrt(old.lam_ratio(lam0) / fac.lam_ratio(lam)))
            self._shared = (fac, covs)
        self._fixed = _Fixed(lam, e, layers, k)
        hp.mom2_update_weight, hp.edit_weight = lam, e
        self._report = self._report_pending = None
        self._publish("session_preserved_rows")

        def undo():
            if undo_rows is not None:
                undo_rows()                         # (rows, tiles and row_scale)
            self._fixed, hp.mom2_update_weight, hp.edit_weight, self._shared, self._report = before

        return undo

    def rescale(self, mom2_weight=None, edit_weight=None, shard=None):
        """The session's mom2_update_weight and edit_weight from now on (``None``: as it is); the held rows become coordinates of the
        new point's factor as the class docstring says (RESCALE), atomically: zero commits all layers together with ``hparams`` (the
        two fields the constructor read), the factors later steps, ``fold()`` and ``save`` refer to and ``row_scale``; non-zero puts
        everything back and raises ``torch.linalg.LinAlgError``.  A stored ``report()`` readout is dropped.  With no preserved row
        only the numbers change; the point the session is at already changes nothing.  ``ValueError`` before anything is
        launched: a bad value (the constructor's rules), a session that has folded, and what ``apply`` refuses."""
        self._rescale(mom2_weight, edit_weight, shard, "rescale")
        self._say(f"Session rescale: mom2_update_weight {self._fixed.lam:g}, edit_weight {self._fixed.edit_weight:g}, {self.preserved} preserved")

    def reweight(self, sources, weight: float, shard=None) -> int:
        """Every live row of ``sources`` (``request["source"]`` strings, or request dicts) counts from now on like a key retained now
        at ``weight``: its rows are multiplied by (that row scale) / (the one they hold) — 1 for every other row — and everything
        behind the smallest changed row is rebuilt (``hip.session_rescale``), atomically as in ``rescale``.  No weight of the
        encoder moves.  Returns the rows changed.  Errors are ``release``'s (``KeyError``: a source without a live row;
        ``ValueError``: a folded source, an empty list, a weight that is not positive and finite, a folded session, what ``apply``
        refuses), all before anything is launched or allocated."""
        w = _positive_weight(weight)
        names = _source_names(sources)
        self._refuse_rescale(shard, "a reweight")
        keep, _, _ = release_plan(self._ledger, self._folded_sources, names)
        kept = set(keep)
        rows = [i for i in range(len(self._ledger)) if i not in kept]
        M = self.preserved
        assert M == len(self._ledger) and rows
        target = hip.row_scale_of(self._fixed.edit_weight, self._shared[0], self._fixed.lam, w)
        f = torch.ones(M, dtype=torch.float64)
        idx = torch.tensor(rows, dtype=torch.long)
        f[idx] = target / self.keys.row_scale[idx]
        changed = [i for i in rows if float(f[i]) != 1.0]
        if changed:
            self._scale_rows(f.to(self.keys.Yp[0].device), changed[0], "reweight")
            self.keys.rescale_commit(f)
        self._report = self._report_pending = None
        self._say(f"Session reweight: {len(rows)} rows of {len(set(names))} sources at weight {w:g}")
        return len(rows)

    def sweep(self, requests: List[Dict], grid, cache_name: Optional[str] = None, scorer=None, visit=None, shard=None,
              stage1=None) -> List[Dict]:
        """Trial steps of ``requests`` at every (mom2_weight, edit_weight) pair of ``grid`` (``edit_engine.validate_grid``), nothing
        committed: the sweep -> score -> ``select_point`` workflow on ONE step of a session, run as the class docstring says (SWEEP;
        the shared part is ``edit_engine.SweepWalk``'s, the step's rows land behind row M, M is not bumped).  Returns one dict per
        pair: ``point``, ``score`` (``scorer.score()`` of an ``EditScorer`` built on the baseline weights; ``None`` without one),
        ``report`` (``report()``'s dict on a ``report=True`` session), ``visit`` (``visit(pair, pipe)``'s result) and ``error``
        (``None``, or the message of the non-positive pivot that point met — the walk goes on; ``torch.linalg.LinAlgError`` only if
        every point failed).  On return, also when ``visit`` raises, the state is back from the copy byte for byte and weights,
        ``preserved``, ledger, ``steps``, the point and ``hparams`` are as before.  A weight rewritten behind the forward's caches
        (``StaleWeightCacheError``) has the plan made again once, as for a step, and the walk goes on at the point that met it.  One
        pinned flag read per point.  Refuses what ``rescale`` refuses, an empty grid or request list, and a step that does not fit."""
        pts = edit_engine.validate_grid(grid)
        n = self._check_step(requests, shard)
        self._refuse_rescale(shard, "a sweep")
        if self.preserved + n > self.capacity:
            raise PreservedSetFull(f"{self.preserved} preserved + {n} new concept rows exceed the session's capacity {self.capacity}: "
                                   f"a sweep does not fold")
        LP = clip_forward.LAST_PATHS
        self._swept = 0
        self._publish("session_sweep_points")
        LP["sweep_points"] = LP["sweep_cov_factorizations"] = LP["sweep_prefix_runs"] = 0
        self._ensure_keys()
        results: List[Dict] = []
        for attempt in (0, 1):
            try:
                self._sweep_points(requests, pts, n, results, cache_name, scorer, visit, shard, stage1)
                break
            except clip_forward.StaleWeightCacheError as e:
                # (as a step: the plan is made again from the live weights, once; the walk goes on at the point that met it)
                if attempt == 1:
                    raise
                emcid_main._note_stale("EditSession.sweep", e, "point")
                LP["stale_cache_retries"] = LP.get("stale_cache_retries", 0) + 1
            except FloatingPointError as e:         # (EMCID_LU_FALLBACK=0 and statistics that are not positive definite)
                raise torch.linalg.LinAlgError(f"sweep after step {self.steps}: {e}; nothing was run and the session is as it was") from e
        if all(r["error"] is not None for r in results):
            raise torch.linalg.LinAlgError(f"sweep after step {self.steps}: every one of the {len(pts)} points met a non-positive pivot "
                                           f"(the first: {results[0]['error']}); the session is as it was")
        return results

    def _sweep_points(self, requests, pts, n, results, cache_name, scorer, visit, shard, stage1):
        """The walk of ``sweep`` over ``pts[len(results):]`` on a freshly prepared plan; a finished point's entry is appended to
        ``results``.  Whatever ends it, the held state, ``row_scale``, the stored readout and the weights are put back."""
        lam0, e0 = self._fixed.lam, self._fixed.edit_weight
        keys, M = self.keys, self.preserved
        plan = self._prepare(requests, shard, cache_name, emcid_main._default_stage1(self.pipe, self.hparams, stage1))
        plan.session = self
        snap, report0 = keys.snapshot(0, M + n), self._report       # (the held rows and the ones the trial steps write behind them)
        rws = own_info = None
        if M > 0:
            rws = self._rebuild_ws("_rescale_ws", hip.RescaleWorkspace, M)
            own_info = rws.info
        factor = torch.empty(max(M, 1), dtype=torch.float64, device=keys.Yp[0].device)[:M]
        walk = edit_engine.SweepWalk(plan)
        try:
            with walk:
                if walk.unit is None:
                    raise torch.linalg.LinAlgError("sweep: the statistics C themselves are not positive definite; nothing was run")
                for lam, e in pts[len(results):]:
                    entry = {"point": (lam, e), "score": None, "report": None, "visit": None, "error": None}
                    with phase("sweep: points"):
                        plan.lam, plan.edit_weight, plan.solver = lam, e, walk.pinned
                        walk.scaled = hip.cov_factor_rescale(walk.unit, 2.0 * lam * (1.0 - e), walk.scaled, lam=lam, edit_weight=e)
                        plan.sweep_factors = walk.scaled
                        if M > 0:
                            # the rescale reports into the flag word of the point's factors (just zeroed), which check_info reads
                            # with the step's own: ONE pinned read per point
                            rws.info = walk.scaled.info
                            factor.fill_(math.sqrt((lam0 * (1.0 - e0)) / (lam * (1.0 - e))))
                            for i in range(keys.n_layers):
                                hip.session_rescale(keys, i, factor, 0, src=snap.Yp[i], ws=rws)
                            self._rescales += keys.n_layers
                            # (the point's factors are at its own lam: a preserved row's unit is its raw scale)
                            keys.row_scale[:M] = snap.row_scale * math.sqrt(self._shared[0].lam_ratio(lam0))
                        plan.chunk.state = walk.state
                        self._report_pending = None
                        try:
                            edit_engine.run_encoder_edit(plan, keep_factors=False, restore=False)
                            check_info(plan)            # (puts the weights back itself before it raises)
                        except FloatingPointError as err:
                            entry["error"] = str(err)
                        self._swept += 1
                        self._publish("session_sweep_points")
                    if entry["error"] is None:
                        if scorer is not None:
                            entry["score"] = scorer.score()
                        if self.report_on and self._report_pending is not None:
                            self._report = self._report_pending
                            entry["report"] = self.report()
                        if visit is not None:
                            entry["visit"] = visit((lam, e), self.pipe)
                        plan.restore_weights()
                    results.append(entry)
        finally:
            edit_engine._release_workspaces(plan)
            if rws is not None:
                rws.info = own_info
            snap.restore()
            self._report, self._report_pending = report0, None
            self._publish("session_rescales")

    def reset(self):
        """Forget the preserved keys; the weights stay as they are, the next step starts a fresh set (M = 0)."""
        if self.keys is not None:
            self.keys.reset()
        self._forget()
        self._publish(*(g for g in _GAUGES if g != "session_loaded_rows"))

    def restore(self):
        """The edited weights back at their values of before the session's first step (bit-identical), and the keys forgotten."""
        if self._orig is not None:
            with torch.no_grad():
                for l, w in self._weights().items():
                    w.copy_(self._orig[l])
        self.reset()

    # ---- save to a file, resume in another process --------------------------------------------------------------------------

    def _other_parameters(self):
        """[(name, parameter)] of the text encoder outside the edited weights, in ``named_parameters`` order."""
        edited = {id(w) for w in self._weights().values()}      # (by identity: nethook resolves names more freely than equality)
        return [(n, p) for n, p in self.pipe.text_encoder.named_parameters() if id(p) not in edited]

    def _statistics(self):
        """[(layer name, statistics file, C in HBM)] per edited layer: the matrices a step of this session reads."""
        from .layer_stats import stats_filename
        hp, te = self.hparams, self.pipe.text_encoder
        out = []
        for l in self._fixed.layers:
            name = hp.rewrite_module_tmp.format(l)
            c = emcid_main.get_cov_text_encoder(te, self.pipe.tokenizer, name, hp.mom2_dataset, hp.mom2_n_samples, hp.mom2_dtype,
                                                stat_dir=self.stats_dir, verbose=self.verbose)
            out.append((name, str(stats_filename(self.stats_dir, "text_encoder", hp.mom2_dataset, name, hp.mom2_dtype, ["mom2"],
                                                 3 * 1024, hp.mom2_n_samples)), c))
        return out

    def save(self, path) -> dict:
        """Write everything a later process needs to carry this session on to ONE file (``torch.save`` of CPU tensors and plain
        values; what it holds: class docstring, SAVE / LOAD, and INTEGRATION.md, "session file").  May be called between any two
        operations; the session is not changed.  One synchronising copy to the host; the file is written under a temporary name
        beside ``path`` and renamed.  Returns {"rows", "folded", "archived", "bytes"}."""
        (weights, dev), (lam, e, layers, k) = self._weights_in_hbm(), self._fixed
        host = hip.pinned_copy                      # (what it returns is held by `state` or `words` until the copies have landed)
        keys = self.keys if self.keys is not None else hip.PreservedKeys(len(layers), self.d, 1, "cpu")
        others = self._other_parameters()
        # (a session that has not run anything yet has read no statistics: nothing of it depends on them)
        stats = self._statistics() if self._shared is not None or self.private_factors is not None else None
        words = host(hip.fingerprint_content([p for _, p in others] + [c for _, _, c in stats or ()]))
        state = {
            "format": SESSION_FORMAT,
            "fixed": {"mom2_update_weight": lam, "edit_weight": e, "layers": list(layers), "num_edit_tokens": k},
            "rewrite_module_tmp": self.hparams.rewrite_module_tmp, "d": self.d, "h": self.h, "capacity": self.capacity,
            "on_full": self.on_full, "report": self.report_on, "keep_folded": self.keep_folded,
            "counters": {k: getattr(self, attr) for k, attr in _COUNTER_ATTRS.items()},
            "ledger": [tuple(r) for r in self._ledger], "folded_sources": sorted(self._folded_sources, key=repr),
            "archive_ledger": [tuple(r) for r in self._archive_ledger],
            "keys": keys.state_dict(sync=False),
            "weights": [host(weights[l]) for l in layers],
            "orig": [host(self._orig[l]) for l in layers] if self._orig is not None else None,
            "base": host(self._base) if self._base is not None else None,
            "archive": [host(a[:self._archived]) for a in self._archive] if self._archive is not None else None,
        }
        torch.cuda.current_stream(dev).synchronize()        # the ONE synchronisation: every copy above has landed
        words = words.tolist()
        state["fingerprints"] = {
            "encoder": [(n, list(p.shape), str(p.dtype), words[i]) for i, (n, p) in enumerate(others)],
            "statistics": None if stats is None else
            [(n, f, list(c.shape), words[len(others) + i]) for i, (n, f, c) in enumerate(stats)]}
        nbytes = _write_session_file(state, path)
        self._say(f"Session saved to {path}: {self.preserved} preserved and {self.folded} folded rows, {nbytes} bytes")
        return {"rows": self.preserved, "folded": self.folded, "archived": self._archived, "bytes": nbytes}

    @classmethod
    def load(cls, pipe, hparams: EMCIDHyperParams, path, device: Optional[str] = None, stats_dir=STATS_DIR,
             capacity: Optional[int] = None, weights: str = "check", verbose: bool = False, on_full: Optional[str] = None,
             report: Optional[bool] = None) -> "EditSession":
        """The session ``save`` wrote to ``path``, carried on in this process on ``pipe``: every public attribute and listing is the
        saved session's, the next step preserves what its next step would have preserved, ``restore()`` gives the weights of before
        its first step.  The first four arguments are the constructor's; ``hparams`` must agree with the file's fixed set-up.
        ``capacity``: default the file's; any value >= the saved M (the rows and tiles go where the new layout wants them).
        ``on_full`` / ``report``: default the file's; ``keep_folded`` is the file's.  ``weights="check"``: the encoder's edited weights
        must equal the file's bit for bit (``ValueError`` naming the first that differs); ``"load"``: the file's are copied into the
        encoder, last of all.  In both modes every other parameter of the encoder and every edited layer's statistics must have the
        fingerprint the file recorded (``ValueError`` naming the parameter, or the layer and its statistics file). Factors and the ONE
        pinned read: class docstring, SAVE / LOAD; a non-positive pivot raises ``torch.linalg.LinAlgError``.  Whatever is refused, the
        encoder's weights are as they were.  Refuses what ``apply`` refuses; everything the file alone can show to be wrong is refused
        before any device call (``check_session_state``)."""
        if weights not in ("check", "load"):
            raise ValueError(f"weights must be 'check' or 'load' (got {weights!r})")
        state = _read_session_file(path)
        check_session_state(state)                  # (whole in itself, before anything of it is used)
        sess = cls(pipe, hparams, device, stats_dir, state["capacity"] if capacity is None else capacity, verbose,
                   state["on_full"] if on_full is None else on_full, state["report"] if report is None else report,
                   keep_folded=state["keep_folded"])
        M = check_session_state(state, sess._fixed, hparams.rewrite_module_tmp, sess.d, sess.h, sess.capacity)
        sess._check_call([None], None, "a load")
        (live, dev), (lam, e, layers, _) = sess._weights_in_hbm(), sess._fixed
        counters, prints = state["counters"], state["fingerprints"]
        others = sess._other_parameters()
        saved = [(n, tuple(s), dt) for n, s, dt, _ in prints["encoder"]]
        found = [(n, tuple(p.shape), str(p.dtype)) for n, p in others]
        if saved != found:
            odd = next((a[0] for a, b in zip(saved, found) if a != b), None)
            if odd is None:                         # (one list is the other's beginning)
                odd = max(saved, found, key=len)[min(len(saved), len(found))][0]
            raise ValueError(f"the session was saved on another text encoder: parameter {odd!r} differs in name, shape or dtype")
        stats = sess._statistics() if prints["statistics"] is not None else None
        for (n, f, c), (sn, sf, shape, _) in zip(stats or (), prints["statistics"] or ()):
            if n != sn or list(c.shape) != list(shape):
                raise ValueError(f"layer {n}: the statistics of {f} have shape {tuple(c.shape)}, the session was saved with "
                                 f"{tuple(shape)} for {sn} ({sf})")
        # everything the device has to say, queued on the current stream and read back once
        words = hip.fingerprint_content([p for _, p in others] + [c for _, _, c in stats or ()])
        want = torch.tensor([w for *_, w in prints["encoder"]] + [w for *_, w in prints["statistics"] or ()], dtype=torch.int64)
        differs = [words != want.to(dev, non_blocking=True)]
        if weights == "check":
            differs.append(torch.stack([(live[l].detach().view(torch.int32) != state["weights"][i].to(dev).view(torch.int32)).any()
                                        for i, l in enumerate(layers)]))
        private = base = commit = None
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        if state["base"] is not None:
            base = state["base"].to(dev)
            private = hip.cov_factor_from_base(base, sess.d, lam, e)
            shared, info = (private, [c for _, _, c in stats]), private.info
        elif stats is not None:
            fac, commit = edit_engine.session_factors(pipe.text_encoder, layers, hparams.rewrite_module_tmp, lam, e,
                                                      {l: c for l, (_, _, c) in zip(layers, stats)}, dev)
            shared, info = (fac, [c for _, _, c in stats]), fac.info
        else:
            shared = None
        host = cls._read_flag(torch.cat([d.to(torch.int32) for d in differs] + [info]))
        for i, (n, *_ ) in enumerate(prints["encoder"]):
            if host[i]:
                raise ValueError(f"the session was saved on another text encoder: the contents of parameter {n!r} differ from the "
                                 f"fingerprint in {path}; the encoder's weights are as they were")
        for i, (n, f, *_ ) in enumerate(prints["statistics"] or ()):
            if host[len(others) + i]:
                raise ValueError(f"layer {n}: the statistics of {stats[i][1]} are not the ones the session's rows were computed "
                                 f"under (saved from {f}); the encoder's weights are as they were")
        if weights == "check":
            at = len(words)
            for i, l in enumerate(layers):
                if host[at + i]:
                    raise ValueError(f"{hparams.rewrite_module_tmp.format(l)}.weight differs from the edited weight in {path}: load "
                                     f"the saved weights first (load_edited_weights, or weights='load')")
        if host[-1] != 0:
            raise torch.linalg.LinAlgError(
                f"load of {path}: " + (f"the folded system of {counters['folded']} rows" if private is not None else "lam C'") +
                f" is not positive definite (non-positive pivot at column {host[-1] - 1}); no session was made and the encoder's "
                f"weights are as they were")
        if commit is not None:
            commit()
        # sound: the state moves in
        if M > 0:
            sess.keys = hip.PreservedKeys(len(layers), sess.d, sess.capacity, dev)
            sess.keys.load_state_dict(state["keys"])
        for k, attr in _COUNTER_ATTRS.items():
            setattr(sess, attr, counters[k])
        sess._ledger = [tuple(r) for r in state["ledger"]]
        sess._folded_sources = set(state["folded_sources"])
        sess._archive_ledger = [tuple(r) for r in state["archive_ledger"]]
        sess._shared, sess.private_factors, sess._base = shared, private, base
        if state["archive"] is not None:
            sess._archived = counters["folded"]
            sess._archive = [a[:sess._archived].to(dev) for a in state["archive"]]
        if state["orig"] is not None:
            sess._orig = {l: state["orig"][i].to(dev) for i, l in enumerate(layers)}
        if weights == "load":
            with torch.no_grad():
                for i, l in enumerate(layers):
                    live[l].copy_(state["weights"][i])
        sess._publish("session_steps", "session_preserved_rows", "session_loaded_rows", "session_folds", "session_folded_rows",
                      "session_retained_rows", "session_released_rows")
        sess._say(f"Session loaded from {path}: {M} preserved and {sess.folded} folded rows after {sess.steps} steps")
        return sess

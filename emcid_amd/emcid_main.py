"""Drop-in boundary of the closed-form mass-edit path on MI355X.

Mirrors the reference's entry points with the same names, argument meaning, side effects and returns
(reference: emcid/emcid_main.py):
    apply_emcid_to_text_encoder         :769-815      execute_emcid_text_encoder         :818-1082
    apply_emcid_to_sdxl_text_encoders   :38-106       execute_emcid_sd_xl_text_encoders  :1085-1425
    get_cov_text_encoder                :2239-2276    upd_matrix_match_shape             :2279-2298
    apply_emcid_to_cross_attn           :511-548      execute_emcid_cross_attn           :314-508
    get_cov_cross_attn                  :2203-2236    cal_insert_deltas                  :1969-2052
plus ``apply_emcid_to_model`` (the name BASELINE.json uses; dispatches on the hparams type).

What runs where: tokenizing, subject search, v*/C cache reads are host Python (once per call); everything
between "inputs are in HBM" and "fc2 weights are edited" is edit_engine.run_encoder_edit -> HIP kernels.
Kept reference behaviours: ``hparams`` is mutated in place by the mom2/edit weight overrides (:846-847);
``requests`` is never written (the reference deep-copies it for that, :850); ``execute_*`` leaves TE1 weights untouched (:1076-1078); the SDXL path
leaves TE2 edited and ``apply_*`` then adds the deltas again, so TE2 ends at W + 2*dW (:1410 vs :93-99) —
reproduced by default (``SDXL_TE2_DOUBLE_APPLY``).  Deliberate differences: ``COV_CACHE`` is keyed by the
statistics directory too (the reference's key ignores it and silently reuses a stale C);
per-request progress prints obey ``verbose``; a v* cache miss runs Stage 1 (compute_z.compute_z_text_encoder) when the
pipeline carries a UNet and a VAE (SDXL: compute_z.compute_z_sdxl_text_encoders, both vectors in one optimisation), and raises
otherwise.
"""
import functools
import logging
import math
import os
import time
from copy import deepcopy
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import clip_forward, edit_engine, hip, nethook
from .edit_engine import (ConceptShard, EncoderEditPlan, LayerEdit, check_info, phase, prepare_encoder_edit,
                          rerun_with_lu, run_checked, run_encoder_edit)
from .emcid_hparams import EMCIDHyperParams, EMCIDXLHyperParams
from .globals import STATS_DIR, XL_STATS_DIR1, XL_STATS_DIR2
from .compute_ks import get_layers_input_output_at_words_cross_attn
from .layer_stats import get_all_cross_attn_kv_layer_names, layer_stats_cross_attn_kv, layer_stats_text_encoder

COV_CACHE: Dict[tuple, object] = {}                # key -> (d, d) fp32 on cpu, like the reference's (:36), or a _HostMoment that makes it on demand
_COV_DEVICE_CACHE: Dict[tuple, torch.Tensor] = {}  # (key, device) -> the same matrix resident in HBM
_VSTAR_CACHE: Dict[tuple, np.ndarray] = {}         # (path, mtime_ns, size) -> v_star
SDXL_TE2_DOUBLE_APPLY = True                       # reference quirk, see module docstring

Stage1Fn = Callable[..., torch.Tensor]


# ---- statistics ---------------------------------------------------------------------------------------

_RESOLVED_DIRS: Dict[Tuple[str, str], str] = {}     # (cwd, stat_dir as given) -> resolved path (Path.resolve is a chain of readlinks)


def _resolved(stat_dir) -> str:
    k = (os.getcwd(), str(stat_dir))
    r = _RESOLVED_DIRS.get(k)
    if r is None:
        if len(_RESOLVED_DIRS) > 256:
            _RESOLVED_DIRS.clear()
        r = _RESOLVED_DIRS[k] = str(Path(stat_dir).resolve())
    return r


def _cov_key(model, layer_name, stat_dir, mom2_n_samples, mom2_dtype):
    model_name = model.config._name_or_path.replace("/", "_")
    return (model_name, layer_name, _resolved(stat_dir), mom2_n_samples, mom2_dtype)


class _HostMoment:
    """COV_CACHE entry of a statistic that went from its file straight to the GPU (``_cov_from_file``): the host tensor the
    reference keeps there (mom2 / count, fp32) is fetched back from the device copy if anyone ever asks for it."""

    def __init__(self, on_device: torch.Tensor):
        self.on_device, self._c = on_device, None

    def tensor(self) -> torch.Tensor:
        if self._c is None:
            self._c = self.on_device.cpu()
        return self._c


def _host_cov(entry) -> torch.Tensor:
    return entry.tensor() if isinstance(entry, _HostMoment) else entry


def _cov_from_file(path, sample_size, device):
    """(C on ``device``, COV_CACHE entry) of a float32 second-moment file in the reference's npz format, or None (no such file,
    another layout or dtype, recorded sample_size differs: the general path then loads — or computes — it).  The file is read
    into ONE page-locked buffer (no zipfile, no CRC pass: runningstats.read_npz_stored), its mom2 member uploaded from there
    and divided by the count on the GPU — element-wise IEEE division by a device scalar, the same fp32 quotients as the
    host's ``mom2 / count`` (tests/test_e2e_gpu.py) — instead of: read, divide into a fresh 37.7 MB host tensor, pageable
    upload, each paying first-touch page faults (27 ms per layer in a cold process on the test box; 5 ms this way)."""
    from . import runningstats as rs
    if torch.device(device).type != "cuda" or not rs.global_load_cache_enabled or os.environ.get("EMCID_COV_FAST", "1") == "0":
        return None
    keep = {}

    def alloc(nbytes):
        keep["t"] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return keep["t"].numpy()

    try:
        dat = rs.read_npz_stored(path, alloc=alloc)
    except RuntimeError:            # no page-locked memory to be had: the general path reads into pageable memory
        return None
    if dat is None:
        return None
    try:
        dat = rs.unbox_numpy_null(dat)
        m, count = dat["mom2.mom2"], int(dat["mom2.count"])
        if sample_size is not None and dat.get("sample_size") != sample_size:
            return None
    except (KeyError, TypeError, ValueError):
        return None
    if m.dtype != np.float32 or m.ndim != 2 or m.shape[0] != m.shape[1] or count <= 0:
        return None
    # m is a view of the page-locked image: its bytes are uploaded as a slice of that very tensor (so the caching host allocator
    # knows the block is in use until the copy has run) and re-typed on the device, where the allocation is aligned
    image = keep["t"]
    off = m.__array_interface__["data"][0] - image.data_ptr()
    if off < 0 or off + m.nbytes > image.numel() or not m.flags.c_contiguous:
        return None
    dev = image[off:off + m.nbytes].to(device, non_blocking=True).view(torch.float32).reshape(m.shape)
    c = torch.div(dev, torch.full((), float(count), dtype=torch.float32, device=device))
    return c, _HostMoment(c)


def get_cov_text_encoder(model, tok, layer_name: str, mom2_dataset: str, mom2_n_samples: int, mom2_dtype: str,
                         inv: bool = False, force_recompute: bool = False, verbose: bool = True,
                         stat_dir=STATS_DIR) -> torch.Tensor:
    """Second moment C = mom2 / count of ``layer_name``'s input as fp32 on the model's device (loaded from the
    npz cache, else computed by Stage 0 over ./data/ccs_filtered.json)."""
    key = _cov_key(model, layer_name, stat_dir, mom2_n_samples, mom2_dtype)
    device = next(model.parameters()).device
    if verbose:
        print(f"Retrieving covariance statistics for {key[0]} @ {layer_name}.")
    dkey = (key, device)
    if key not in COV_CACHE or force_recompute:
        fast = None
        if not force_recompute and mom2_dtype == "float32":
            from .layer_stats import stats_filename
            fast = _cov_from_file(stats_filename(stat_dir, "text_encoder", mom2_dataset, layer_name, mom2_dtype, ["mom2"], 3 * 1024,
                                                 mom2_n_samples), mom2_n_samples, device)
        if fast is not None:
            _COV_DEVICE_CACHE[dkey], COV_CACHE[key] = fast
        else:
            stat = layer_stats_text_encoder(model, tok, layer_name, stat_dir, mom2_dataset, to_collect=["mom2"],
                                            sample_size=mom2_n_samples, precision=mom2_dtype,
                                            force_recompute=force_recompute)
            COV_CACHE[key] = stat.mom2.moment().float().to("cpu")
            _COV_DEVICE_CACHE.pop(dkey, None)
    if dkey not in _COV_DEVICE_CACHE:
        _COV_DEVICE_CACHE[dkey] = _host_cov(COV_CACHE[key]).to(device)
    c = _COV_DEVICE_CACHE[dkey]
    return torch.inverse(c) if inv else c


def clear_caches():
    COV_CACHE.clear()
    _COV_DEVICE_CACHE.clear()
    _VSTAR_CACHE.clear()


def upd_matrix_match_shape(matrix: torch.Tensor, shape: torch.Size) -> torch.Tensor:
    if matrix.shape == shape:
        return matrix
    if matrix.T.shape == shape:
        return matrix.T
    if matrix.dim() == 2 and len(shape) == 4:
        return matrix.reshape(shape[0], shape[1], *shape[2:])
    raise ValueError(f"Update matrix of shape {tuple(matrix.shape)} does not match the weight shape {tuple(shape)}")


# ---- v* cache -----------------------------------------------------------------------------------------

def vstar_cache_name(cache_name: Optional[str], request: Dict, hparams, idx: int, suffix: str = "") -> Optional[str]:
    """Cache path of one request's v* (reference :873-890 SD; :1157-1166 SDXL with suffix ``_2``)."""
    if cache_name is None:
        return None
    if "esd" in hparams.objective:
        return f"{cache_name}source_{request['source']}{suffix}.npz"
    if getattr(hparams, "sld_supervision", False):
        return f"{cache_name}source_{request['source_cat']}_{idx}{suffix}.npz"
    return f"{cache_name}source_{request['source']}_dest_{request['dest']}{suffix}.npz"


def vstar_cache_file(cache_name: Optional[str], request: Dict, hparams, idx: int, suffix: str = "") -> Optional[Path]:
    name = vstar_cache_name(cache_name, request, hparams, idx, suffix)
    return None if name is None else Path(name)


def _npz_single_array(blob: bytes, key: str) -> Optional[np.ndarray]:
    """The array of an npz whose FIRST member is ``{key}.npy``, stored uncompressed, little-endian f4/f8, C order — the
    file ``np.savez(f, v_star=...)`` writes (reference :951-968) — parsed straight from the bytes: the zip local header,
    then the npy header, then the data.  ``zipfile`` + ``np.load`` cost ~130 us per file, 1 000 files per mass edit.
    Returns None for anything else (the caller then uses ``np.load``)."""
    try:
        if blob[:4] != b"PK\x03\x04" or blob[8:10] != b"\x00\x00":          # local file header, method 0 = stored
            return None
        n_name, n_extra = int.from_bytes(blob[26:28], "little"), int.from_bytes(blob[28:30], "little")
        if blob[30:30 + n_name] != (key + ".npy").encode():
            return None
        o = 30 + n_name + n_extra
        if blob[o:o + 6] != b"\x93NUMPY":
            return None
        major = blob[o + 6]
        if major == 1:
            hlen, o = int.from_bytes(blob[o + 8:o + 10], "little"), o + 10
        elif major in (2, 3):
            hlen, o = int.from_bytes(blob[o + 8:o + 12], "little"), o + 12
        else:
            return None
        header = blob[o:o + hlen].decode("latin1")
        o += hlen
        import ast
        meta = ast.literal_eval(header)
        descr, shape = meta["descr"], tuple(meta["shape"])
        if meta["fortran_order"] and len(shape) > 1 or descr not in ("<f4", "<f8"):
            return None
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        dt = np.dtype(descr)
        if o + n * dt.itemsize > len(blob):
            return None
        return np.frombuffer(blob, dtype=dt, count=n, offset=o).reshape(shape).copy()
    except Exception:
        return None


_VSTAR_CACHE_MAX = 4096     # entries of the per-file memo below (the numpy path only); oldest dropped first


def _read_vstar(path: str) -> np.ndarray:
    """``np.load(path)["v_star"]`` for ONE file — the path of every file the native batch reader does not serve (other npz
    layouts, compressed members) and of processes without libemcid_host.so; memoised on (path, mtime, size), bounded."""
    st = os.stat(path)
    key = (path, st.st_mtime_ns, st.st_size)
    v = _VSTAR_CACHE.get(key)
    if v is None:
        with open(path, "rb") as f:
            blob = f.read()
        v = _npz_single_array(blob, "v_star")
        if v is None:
            with np.load(path) as z:
                v = np.asarray(z["v_star"])
        while len(_VSTAR_CACHE) >= _VSTAR_CACHE_MAX:
            _VSTAR_CACHE.pop(next(iter(_VSTAR_CACHE)))
        _VSTAR_CACHE[key] = v
    return v


def _read_threads() -> int:
    n = os.environ.get("EMCID_READ_THREADS", "")
    if n:
        return max(1, int(n))
    from . import effective_cpu_count
    return max(1, min(8, effective_cpu_count() // 2))


def _vstar_file_rows(hparams) -> int:
    """Rows per v* cache file: num_edit_tokens under ``use_new_compute_z`` (files (k, hidden), reference :946-957), else 1."""
    k = int(getattr(hparams, "num_edit_tokens", 1) or 1)
    return k if bool(getattr(hparams, "use_new_compute_z", False)) and k > 1 else 1


def _native_vstar_rows(names: Sequence[Optional[str]], width: int, pin: bool, k: int = 1):
    """All cache files in one native call (csrc/host_io.cpp: a few threads, open/read/parse straight into the row buffer —
    page-locked when the rows go to a GPU next, so the upload needs no staging copy).  Returns (rows (N, width) fp32 tensor —
    (N, k, width) for files of k > 1 rows —, status uint8 array: 0 = file read, 1 = no such file, 2 = a file for numpy), or None
    without the host library."""
    from . import host_text
    if os.environ.get("EMCID_NATIVE_VSTAR", "1") == "0" or not host_text.available() or any(n is None for n in names):
        return None
    lib = host_text.load()
    n = len(names)
    blob, off = host_text.pack_strings(names)
    rows = torch.empty((n, width) if k == 1 else (n, k, width), dtype=torch.float32, pin_memory=bool(pin))
    status = np.empty(n, dtype=np.uint8)
    if k == 1:
        rc = lib.emcid_read_npz_rows_f32(blob, off.ctypes.data, n, b"v_star", width, rows.data_ptr(), width,
                                         status.ctypes.data, _read_threads())
    else:
        rc = lib.emcid_read_npz_rows_k_f32(blob, off.ctypes.data, n, b"v_star", k, width, rows.data_ptr(), k * width,
                                           status.ctypes.data, _read_threads())
    if rc < 0:
        return None
    return rows, status


def load_v_stars(requests: Sequence[Dict], hparams, cache_name: Optional[str], suffix: str = "",
                 stage1: Optional[Stage1Fn] = None, width: Optional[int] = None, pin: bool = False, native=None) -> torch.Tensor:
    """(N, hidden) fp32 on the host: one row per request, the transpose of the reference's ``zs`` (:977) — (N k, hidden), row
    ``rq * k + num``, for ``use_new_compute_z`` files of k = num_edit_tokens rows each (:972-975).  ``width``: the
    encoder's hidden size when the caller knows it (then every cache file is read by the native batch reader; files it does
    not serve, and every miss, take the per-file path below, which is the reference's: np.load, recompute on an unreadable
    file :903-904, Stage 1 on a miss :905-969).  ``native``: (rows, status) of a native batch read of these very names that has
    already been made (the early reader's), so that a miss does not read the hits a second time."""
    names = [vstar_cache_name(cache_name, request, hparams, idx, suffix) for idx, request in enumerate(requests)]
    k_file = _vstar_file_rows(hparams)
    if native is None:
        native = _native_vstar_rows(names, int(width), pin, k_file) if (width and cache_name is not None and len(names)) else None
    if native is not None and not native[1].any():
        # every file was read natively: (width,) or (1, width) rows, or — use_new_compute_z with k > 1 — (k, width) files, whose
        # stack flattens to the reference's "rq num" row order (:972-975)
        return native[0].reshape(-1, native[0].shape[-1])
    rows: List[Optional[np.ndarray]] = [None] * len(requests)
    missing: List[int] = []
    for idx, request in enumerate(requests):
        f = names[idx]
        if native is not None and native[1][idx] == 0:
            rows[idx] = native[0][idx].numpy()
            continue
        v = None
        if f is not None and not (native is not None and native[1][idx] == 1):
            try:
                v = _read_vstar(f)
            except FileNotFoundError:
                v = None
            except Exception as e:  # unreadable cache -> recompute, as the reference (:903-904)
                print(f"Error reading cache file due to {e}. Recomputing...")
                v = None
        if v is None:
            if stage1 is None:
                raise NotImplementedError(
                    f"no cached v* for request {idx} ([{request['source']}] -> [{request['dest']}]) at {f}: "
                    f"pass cache_name pointing at v_star npz files (reference emcid_main.py:873-890) or a stage1= "
                    f"callable (emcid_amd.compute_z.compute_z_text_encoder is the reference's Stage 1)")
            missing.append(idx)
            continue
        rows[idx] = v
    if missing:
        # Stage 1 for every miss, in request order like the reference's loop (:871-969) — through the callable's ``batch``
        # attribute when it has one (compute_z.stage1_for: several concepts per Adam step), else one request at a time
        with torch.enable_grad():      # Stage 1 is an optimisation through the UNet, whatever mode the caller is in
            if hasattr(stage1, "batch") and len(missing) > 1:
                found = stage1.batch([requests[i] for i in missing], suffix)
            else:
                found = [stage1(requests[i], suffix) for i in missing]
        for idx, v in zip(missing, found):
            v = v.detach().float().cpu().numpy()
            if names[idx] is not None:
                Path(names[idx]).parent.mkdir(exist_ok=True, parents=True)
                np.savez(names[idx], v_star=v)
            rows[idx] = v
    new_z = bool(getattr(hparams, "use_new_compute_z", False))
    for idx, v in enumerate(rows):
        if v.dtype != np.float32:
            v = v.astype(np.float32)
        if new_z:         # files of shape (num_edit_tokens, hidden) (:946-957); zs = "rq num c_i -> c_i (rq num)" of their stack (:972-975)
            if v.ndim == 1:
                v = v[None, :]
            if v.ndim != 2 or v.shape[0] != int(hparams.num_edit_tokens):
                raise ValueError(f"v* of request {idx} has shape {tuple(v.shape)}; use_new_compute_z with num_edit_tokens = "
                                 f"{hparams.num_edit_tokens} expects ({hparams.num_edit_tokens}, hidden)")
        elif v.ndim == 2:
            if v.shape[0] != 1:
                raise ValueError(f"v* of request {idx} has {v.shape[0]} rows: a multi-token v* needs hparams.use_new_compute_z "
                                 f"(reference emcid_main.py:898-900, :972-977)")
            v = v[0]
        rows[idx] = v
    out = np.stack(rows, axis=0)
    return torch.from_numpy(out.reshape(-1, out.shape[-1]) if new_z else out)


# ---- plans --------------------------------------------------------------------------------------------

def _shard_from_env(shard: Optional[ConceptShard]) -> ConceptShard:
    if shard is not None:
        return shard
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        force = os.environ.get("EMCID_FORCE_COLLECTIVES", "0") == "1"
        if dist.get_world_size() > 1 or force:
            return ConceptShard(dist.get_rank(), dist.get_world_size(), None, force_collectives=force)
    return ConceptShard()


_DIR_LISTINGS: Dict[str, Tuple[int, frozenset]] = {}      # directory -> (its st_mtime_ns, its entries): a listing is re-read only
                                                           # when the directory changed (a file added or removed bumps mtime)


def _dir_entries(d: str) -> Optional[frozenset]:
    try:
        m = os.stat(d or ".").st_mtime_ns
        hit = _DIR_LISTINGS.get(d)
        if hit is None or hit[0] != m:
            hit = _DIR_LISTINGS[d] = (m, frozenset(os.listdir(d or ".")))
            if len(_DIR_LISTINGS) > 64:
                _DIR_LISTINGS.pop(next(iter(_DIR_LISTINGS)))
        return hit[1]
    except OSError:
        return None


def _any_vstar_missing(requests: Sequence[Dict], hparams, cache_name: Optional[str], suffix: str) -> bool:
    """True when some request has no v* file: one directory listing per cache directory (re-read only when the directory's
    mtime moved) instead of a stat per request; the per-file validation by mtime/size happens later, underneath the GPU's
    forward.  A stale answer is harmless either way: "missing" takes the eager path, which opens the files; "present" takes
    the lazy one, which handles a file that is gone exactly like the eager one, just later."""
    if cache_name is None:
        return True
    pre = str(cache_name)
    try:
        if "esd" in hparams.objective:
            tails = [f"source_{r['source']}{suffix}.npz" for r in requests]
        elif getattr(hparams, "sld_supervision", False):
            tails = [f"source_{r['source_cat']}_{i}{suffix}.npz" for i, r in enumerate(requests)]
        else:
            tails = [f"source_{r['source']}_dest_{r['dest']}{suffix}.npz" for r in requests]
    except KeyError:
        return True                                        # the eager path raises the reference's KeyError
    if any("/" in t for t in tails):                       # a source with a path separator: per-file check
        return not all(os.path.exists(pre + t) for t in tails)
    pre_dir, pre_base = os.path.split(pre)
    names = _dir_entries(pre_dir)
    if names is None:
        return True
    return not names.issuperset(pre_base + t for t in tails) if pre_base else not names.issuperset(tails)


_VSTAR_READER = None          # (pid, executor): one helper thread per process, created at first use


class _EarlyVstars:
    """The v* rows of a request list, read by the native batch reader ON A HELPER THREAD from the moment prepare has launched the
    unedited leading layers: the reader is one ctypes call that does not hold the interpreter lock, so it runs beside the host's
    remaining preparation and is (nearly) done when the first solve asks — with the GPU twice as fast as in round 3 the read had
    moved onto the critical path (profiles/r04_g_call_events.txt: the host reached the first solve 0.2 ms before the device).
    Anything the native reader does not serve (a miss, a file for numpy) falls back to load_v_stars at result().
    The rows are a SNAPSHOT of the files as they are when ``prepare`` runs: a plan prepared early and run after its cache files were
    rewritten edits towards the old targets (the lazy reader, EMCID_EARLY_VSTAR=0, reads at the first solve)."""

    def __init__(self, args, kwargs, future, rows, keep):
        self.args, self.kwargs, self.future, self.rows, self.keep = args, kwargs, future, rows, keep

    @classmethod
    def start(cls, requests, hparams, cache_name, suffix, stage1, width=None, pin=False):
        from . import host_text
        if (not width or cache_name is None or not len(requests) or os.environ.get("EMCID_NATIVE_VSTAR", "1") == "0"
                or os.environ.get("EMCID_EARLY_VSTAR", "1") == "0" or not host_text.available()):
            return None
        names = [vstar_cache_name(cache_name, request, hparams, idx, suffix) for idx, request in enumerate(requests)]
        if any(n is None for n in names):
            return None
        global _VSTAR_READER
        if _VSTAR_READER is None or _VSTAR_READER[0] != os.getpid():      # (a forked child does not inherit the worker thread)
            from concurrent.futures import ThreadPoolExecutor
            _VSTAR_READER = (os.getpid(), ThreadPoolExecutor(max_workers=1, thread_name_prefix="emcid-vstar"))
        lib = host_text.load()
        n = len(names)
        blob, off = host_text.pack_strings(names)
        k = _vstar_file_rows(hparams)        # (k, width) files of use_new_compute_z: the rows of file i at rows[i], "rq num" order
        rows = torch.empty((n, int(width)) if k == 1 else (n, k, int(width)), dtype=torch.float32, pin_memory=bool(pin))
        status = np.empty(n, dtype=np.uint8)
        threads = _read_threads()

        times = [time.perf_counter(), 0.0, 0.0]      # submitted, started, finished (edit_engine.TIMING: "vstar reader ...")

        def read(blob=blob, off=off, rows=rows, status=status, times=times):
            # (the buffers belong to this task, not to the object that waits for it: a plan that is dropped unrun must not free
            #  memory the reader is still writing)
            times[1] = time.perf_counter()
            rc = lib.emcid_read_npz_rows_k_f32(blob, off.ctypes.data, n, b"v_star", k, int(width), rows.data_ptr(), k * int(width),
                                               status.ctypes.data, threads)
            times[2] = time.perf_counter()
            return rc

        fut = _VSTAR_READER[1].submit(read)
        self = cls((requests, hparams, cache_name, suffix, stage1), dict(width=width, pin=pin), fut, rows, (blob, off, status))
        self.times = times
        return self

    def wait(self):
        try:
            rc = self.future.result()
        except Exception as e:       # the per-file path below serves the call; say why the batch read did not
            logging.getLogger("emcid_amd").warning("native v* batch read failed (%r): reading the cache files one by one", e)
            return -1
        t = getattr(self, "times", None)
        if t is not None and t[2] > 0.0:       # where a slow join comes from: the worker thread starting late, or the reads themselves
            edit_engine.TIMING["vstar reader queued"] = edit_engine.TIMING.get("vstar reader queued", 0.0) + (t[1] - t[0])
            edit_engine.TIMING["vstar reader reading"] = edit_engine.TIMING.get("vstar reader reading", 0.0) + (t[2] - t[1])
            self.times = None
        return rc

    def result(self):
        rc = self.wait()
        if rc is not None and rc >= 0 and not self.keep[2].any():
            return self.rows.reshape(-1, self.rows.shape[-1])
        # a miss or a file for numpy: the rows the batch read did serve are handed on (no second read of 999 hits for one miss)
        native = (self.rows, self.keep[2]) if rc is not None and rc >= 0 else None
        return load_v_stars(*self.args, **self.kwargs, native=native)


class _LazyVstars:
    """The v* rows of a request list, read when first asked for.  prepare hands this to the engine, which asks at the first
    edited layer's solve — by then the encoder forward up to that layer is queued on the GPU, so the file-system calls of
    the cache reads (and Stage 1 on a miss) cost no wall-clock of their own."""

    def __init__(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs

    def result(self):
        return load_v_stars(*self.args, **self.kwargs)


def prepare_text_encoder_edit(text_encoder, tokenizer, requests, hparams, layers, lam, stat_dir, cache_name,
                              suffix="", verbose=True, shard=None, stage1=None, with_targets=True) -> EncoderEditPlan:
    """Host side of one encoder's edit: v* rows, C per layer (HBM-resident), tokenized prompts + lookup.  ``with_targets=False``
    (a session's retain list): no v* is looked up, read or computed, ``cache_name`` and ``stage1`` are not touched."""
    w = None
    for layer in layers:   # resolve every edited weight now: LookupError before any GPU work, like the reference (:858-863)
        w = nethook.get_parameter(text_encoder, f"{hparams.rewrite_module_tmp.format(layer)}.weight")
    # v* rows have the encoder's hidden size = the rows of the edited projection (h, d); known here, it lets the cache files be
    # read natively, in one call, into page-locked rows (load_v_stars)
    how = dict(width=int(w.shape[0]) if w is not None and w.dim() == 2 else None, pin=bool(w is not None and w.is_cuda))

    def targets():
        # the files start coming in on the helper thread at once; whether one is missing is looked up meanwhile
        early = _EarlyVstars.start(requests, hparams, cache_name, suffix, stage1, **how)
        # a cache miss is handled FIRST, as the reference does (:873-969 come before the layer loop's covariance reads): Stage 1
        # runs (or the miss is reported) before statistics are read or computed
        if _any_vstar_missing(requests, hparams, cache_name, suffix):
            if early is not None:
                return early.result()   # waits for the reader, hands the rows it did read to load_v_stars (Stage 1 for the misses)
            return load_v_stars(requests, hparams, cache_name, suffix, stage1, **how)
        return early if early is not None else _LazyVstars(requests, hparams, cache_name, suffix, stage1, **how)

    def statistics():
        return {layer: get_cov_text_encoder(text_encoder, tokenizer, hparams.rewrite_module_tmp.format(layer),
                                            hparams.mom2_dataset, hparams.mom2_n_samples, hparams.mom2_dtype,
                                            stat_dir=stat_dir, verbose=verbose)
                for layer in layers}

    # both run inside prepare_encoder_edit right AFTER it has launched the unedited leading layers (they need nothing but the
    # prompts), in this order
    return prepare_encoder_edit(text_encoder, tokenizer, requests, layers, hparams.rewrite_module_tmp, lam,
                                hparams.edit_weight, targets if with_targets else None, statistics, _shard_from_env(shard),
                                layer_module_tmp=getattr(hparams, "layer_module_tmp", None),
                                num_edit_tokens=int(getattr(hparams, "num_edit_tokens", 1)))


def _default_stage1(pipe, hparams, stage1):
    """Stage 1 on a v* cache miss, like the reference (:905-969): when the caller gave no ``stage1=`` and the pipeline
    carries a UNet and a VAE, the missing v* is optimised by compute_z.compute_z_text_encoder at z_layer =
    hparams.layers[-1] (:868) and written to the cache — by compute_z_text_encoder_global under ``sld_supervision`` (:911-918:
    a global concept at "[CLS]" / "[EOS]" under the safe-latent-diffusion supervision), by compute_z_text_encoder_v1 when
    ``txt_img_align_scale_factor != 0`` (:919-926: CLIP's text tower with projection + the image-alignment term; its towers come
    from the hub like the reference's — ``stage1=compute_z.stage1_for(pipe, hparams, layer, clip_towers=...)`` hands over local
    ones), by compute_z_text_encoder_v2, (num_edit_tokens, hidden) per concept, under ``use_new_compute_z`` (:927-936)."""
    if stage1 is not None or getattr(pipe, "unet", None) is None or getattr(pipe, "vae", None) is None:
        return stage1
    from .compute_z import stage1_for
    return stage1_for(pipe, hparams, hparams.layers[-1])


def _default_stage1_sdxl(pipe, hparams, stage1):
    """Stage 1 of the SDXL pair on a v* cache miss, like the reference (:1157-1230): without a caller-supplied ``stage1=`` and
    with a UNet and a VAE in the pipeline, compute_z.compute_z_sdxl_text_encoders optimises (v*, v*_2) together at the last
    edited layer of each encoder; each encoder's loader writes its own cache file."""
    if stage1 is not None or getattr(pipe, "unet", None) is None or getattr(pipe, "vae", None) is None:
        return stage1
    from .compute_z import stage1_for_sdxl
    return stage1_for_sdxl(pipe, hparams)


def _deltas_to_host(edits: List[LayerEdit]) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """Reference return format: {weight_name: (adj_k (d, N) f64 cpu, resid (h, N) f64 cpu)} (:1062-1065)."""
    return {e.weight_name: (e.Xt.t().contiguous().cpu(), e.Rt.t().contiguous().cpu()) for e in edits}


def _announce(requests, verbose):
    if verbose:
        for request in requests:
            print(f"EMCID request sample: [{request['source']}] -> [{request['dest']}]")


def _any_rank(flag: bool, device) -> bool:
    """True on every rank of the default group if ``flag`` is set on any of them (one MAX all-reduce of a word)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return bool(flag)
    t = torch.tensor([1 if flag else 0], dtype=torch.int32,
                     device=device if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return bool(int(t.item()))


def _note_stale(who: str, e, what: str = "call"):
    """Before a call is repeated after ``StaleWeightCacheError``: say so and drop the forward's weight-derived caches."""
    logging.getLogger("emcid_amd").warning("%s: %s; redoing the %s from the live weights", who, e, what)
    clip_forward.invalidate_weight_caches(None)


def _retry_if_stale(fn):
    """The forward's weight-derived caches carry a content guard (clip_forward.WeightGuard): when an edit finds that a weight was
    rewritten behind them (``param.data.copy_(...)`` between two calls), the engine puts the edited weights back, drops the caches
    and raises ``StaleWeightCacheError`` — the call is redone once, from the live weights.  A multi-rank job raises instead: one
    rank repeating its call alone would leave the others inside their collectives."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        try:
            return fn(*args, **kwargs)
        except clip_forward.StaleWeightCacheError as e:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise
            _note_stale(fn.__name__, e)
            clip_forward.LAST_PATHS["stale_cache_retries"] = clip_forward.LAST_PATHS.get("stale_cache_retries", 0) + 1
            return fn(*args, **kwargs)
    return wrapper


# ---- SD ------------------------------------------------------------------------------------------------

@_retry_if_stale
def execute_emcid_text_encoder(pipe, requests: List[Dict], hparams: EMCIDHyperParams, cache_name: Optional[str] = None,
                               mom2_weight: Optional[int] = None, edit_weight: Optional[float] = None,
                               verbose: bool = True, stat_dir=STATS_DIR, shard=None, stage1=None
                               ) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """Computes the per-layer factors; the model is unchanged on return (invariant of the reference)."""
    hparams.mom2_update_weight = mom2_weight if mom2_weight is not None else hparams.mom2_update_weight
    hparams.edit_weight = edit_weight if edit_weight is not None else hparams.edit_weight
    _announce(requests, verbose)
    plan = prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, requests, hparams, hparams.layers,
                                     hparams.mom2_update_weight, stat_dir, cache_name, "", verbose, shard,
                                     _default_stage1(pipe, hparams, stage1))
    edits = run_checked(plan, keep_factors=True, restore=True)
    if verbose:
        print(f"Deltas successfully computed for {[e.weight_name for e in edits]}")
    return _deltas_to_host(edits)


@_retry_if_stale
def apply_emcid_to_text_encoder(pipe, requests: List[Dict], hparams: EMCIDHyperParams, device: str,
                                mom2_weight: Optional[int] = None, edit_weight: Optional[float] = None,
                                return_orig_text_encoder=False, cache_name: Optional[str] = None,
                                stats_dir=STATS_DIR, verbose: bool = True, shard=None, stage1=None):
    """Returns (pipe with the edited text encoder, the original text encoder or None)."""
    origin_text_encoder = deepcopy(pipe.text_encoder) if return_orig_text_encoder else None
    hparams.mom2_update_weight = mom2_weight if mom2_weight is not None else hparams.mom2_update_weight
    hparams.edit_weight = edit_weight if edit_weight is not None else hparams.edit_weight
    _announce(requests, verbose)
    plan = prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, requests, hparams, hparams.layers,
                                     hparams.mom2_update_weight, stats_dir, cache_name, "", verbose, shard,
                                     _default_stage1(pipe, hparams, stage1))
    # The engine leaves each fc2 at W0 + float(U): the value the reference reaches by restoring W0 (:1076-1078)
    # and adding float(adj_k @ resid^T) again (:802-809).
    with phase("run + final sync"):
        edits = run_checked(plan, keep_factors=False, restore=False)
    if verbose:
        print(f"New weights successfully inserted into {[e.weight_name for e in edits]}")
    return pipe, origin_text_encoder


# ---- edit sessions: later edits preserve the keys of earlier ones -------------------------------------------------------------

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
        if not (np.isfinite(lam) and lam > 0.0):
            raise ValueError(f"mom2_update_weight must be positive and finite in a session (got {lam}): the dual solver factors lam C'")
        if not (0.0 < e < 1.0):
            raise ValueError(f"edit_weight must lie inside (0, 1) in a session (got {e})")
        self.h, self.d = int(ws[0].shape[0]), int(ws[0].shape[1])
        if capacity is None:
            capacity = int(0.6 * self.d)
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 1:
            raise ValueError(f"capacity must be a positive integer (got {capacity!r})")
        if device is not None and torch.device(device).type != ws[0].device.type:
            raise ValueError(f"device {device!r} but the text encoder's weights live on {ws[0].device}")
        self.pipe, self.hparams, self.stats_dir, self.verbose = pipe, hparams, stats_dir, verbose
        self.capacity, self.on_full = int(capacity), on_full
        self._fixed = (lam, e, tuple(hparams.layers), int(getattr(hparams, "num_edit_tokens", 1)))
        self.keys: Optional[hip.PreservedKeys] = None       # allocated at the first step
        self.steps = 0
        self._orig: Optional[Dict[int, torch.Tensor]] = None
        self._ws: Dict[tuple, hip.PreserveWorkspace] = {}
        self.folded, self.folds = 0, 0                       # rows taken into the private base factor, and how often
        self.private_factors: Optional[hip.CovFactors] = None    # the factors of lam C' + (folded P)^T P: this session's steps only
        self._base: Optional[torch.Tensor] = None            # (n_layers, dp, dp) f64: the folded systems themselves
        self._shared = None     # (factors, covs) of the last sound step: what the preserved rows' coordinates refer to
        self.retained = 0                                    # rows added by retain(), folded ones included
        self.report_on = bool(report)
        self._report = self._report_pending = None           # (buffer (n_layers, M + 2 N) f64 in HBM, M, N, row scales) of the last sound step
        self._ledger: List[tuple] = []                       # per live row since the last fold: (source, "edit" | "retain", ordinal, token)
        self._folded_sources: set = set()                    # sources whose rows a fold took: no longer releasable
        self._retains = 0                                    # retain() calls so far (the ordinal of a retained row)
        self._release_ws: Optional[hip.ReleaseWorkspace] = None
        self._rescale_ws: Optional[hip.RescaleWorkspace] = None
        self._rescales = 0                                   # hip.session_rescale calls so far (LAST_PATHS session_rescales)
        self.released = 0                                    # rows released so far
        self.keep_folded = bool(keep_folded)
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
        lam, e, layers, _ = self._fixed
        first = self.private_factors is None
        src = self._shared[0] if first else self.private_factors
        if first:
            dst = hip.CovFactors(len(layers), self.d, dev)
            base = torch.empty(len(layers), dst.dp, dst.dp, dtype=torch.float64, device=dev)
            keep = None
        else:
            dst, base = src, self._base
            keep = (dst.buf.clone(), base.clone())          # (a refused fold puts both back)
        dst.info.zero_()
        if self.keep_folded:                        # Q lands in the archive's tail: the fold entry leaves it there
            self._archive_room(M, dst.dp, dev)
            tails = [a[self._archived:self._archived + M].view(-1) for a in self._archive]
        else:
            tails = [torch.empty(M * dst.dp, dtype=torch.float64, device=dev)] * len(layers)
        for i in range(len(layers)):
            hip.cov_factor_fold(src, self.keys, i, self._shared[1][i] if first else None, lam, e, dst, base, ws=tails[i])
        code = self._read_flag(dst.info)
        if code != 0:
            if keep is not None:
                dst.buf.copy_(keep[0])
                base.copy_(keep[1])
                dst.info.zero_()
            raise torch.linalg.LinAlgError(
                f"fold after step {self.steps}: lam C' plus the {self.folded} folded and {M} preserved keys is not positive definite "
                f"(non-positive pivot at column {code - 1}): check the statistics; the {M} preserved rows, the private factors and "
                f"the weights are as they were")
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
        LP = clip_forward.LAST_PATHS
        LP["session_folds"], LP["session_folded_rows"], LP["session_preserved_rows"] = self.folds, self.folded, 0
        if self.verbose:
            print(f"Session fold {self.folds}: {M} preserved rows folded into the base factor, {self.folded} folded so far")

    def _archive_room(self, M: int, dp: int, dev):
        """Make the archive of every edited layer hold ``M`` more rows: at least doubled when it has to grow (the rows that count
        are copied over), allocated at the first fold that keeps its rows."""
        need = self._archived + M
        if self._archive is None:
            self._archive = [torch.zeros(need, dp, dtype=torch.float64, device=dev) for _ in self._fixed[2]]
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
            buf = torch.empty(len(self._fixed[2]), M + 2 * N, dtype=torch.float64, device=self.keys.Yp[0].device)
            self._report_pending = (buf, M, N, self.keys.row_scale[:M].clone())
        return self._report_pending[0][i]

    def report(self):
        """The readout of the last sound step of a ``report=True`` session (class docstring), ``None`` before any."""
        if self._report is None:
            return None
        buf, M, N, scale = self._report
        host = buf.cpu()                            # the one synchronising read
        out = {}
        for i, l in enumerate(self._fixed[2]):
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
                             f"{self._fixed}, the hparams now say {now}; open a new EditSession")
        if _shard_from_env(shard).collective:
            raise NotImplementedError("EditSession runs on one rank: a multi-rank ConceptShard is not supported")
        forced = edit_engine.SOLVER or os.environ.get("EMCID_SOLVER")
        if forced in ("direct", "lu"):
            raise ValueError(f"EMCID_SOLVER={forced} inside a session: the preserved keys live in the dual solver's coordinates")
        if len(requests) == 0:
            raise ValueError(f"{what} needs at least one request")

    def _check_step(self, requests, shard):
        self._check_call(requests, shard)
        n = len(requests) * self._fixed[3]
        if self.preserved + n > self.capacity and self.on_full == "fold" and n <= self.capacity:
            return n                                # apply() folds first
        if self.preserved + n > self.capacity:
            raise PreservedSetFull(f"{self.preserved} preserved + {n} new concept rows exceed the session's capacity {self.capacity}; "
                                   f"open a session with a larger capacity, or with on_full='fold' (sess.fold() takes a full set into "
                                   f"the session's base factor)")
        return n

    def _weights(self):
        return {l: nethook.get_parameter(self.pipe.text_encoder, f"{self.hparams.rewrite_module_tmp.format(l)}.weight")
                for l in self._fixed[2]}

    def _ensure_keys(self):
        """Allocate the preserved key set at the first step or retain list, on the encoder's device (HBM only)."""
        if self.keys is None:
            w = next(iter(self._weights().values()))
            if not w.is_cuda:
                raise hip.EmcidHipError(f"the text encoder must live in HBM (got {w.device}); there is no CPU path")
            self.keys = hip.PreservedKeys(len(self._fixed[2]), self.d, self.capacity, w.device)

    @staticmethod
    def _read_flag(info: torch.Tensor) -> int:
        """The ONE synchronising read of an operation: the device flag word ``info`` through a pinned word, after everything
        queued on the current stream of its device."""
        flag = torch.empty(1, dtype=torch.int32, pin_memory=True)
        flag.copy_(info, non_blocking=True)
        torch.cuda.current_stream(info.device).synchronize()
        return int(flag.item())

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
                _note_stale(f"EditSession.{method}", e, redo)
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
        hp, te = self.hparams, self.pipe.text_encoder
        weights = self._weights()
        if self._orig is None:
            self._orig = {l: w.detach().clone() for l, w in weights.items()}
        self._ensure_keys()
        _announce(requests, self.verbose)
        plan = self._run_plan(
            lambda: prepare_text_encoder_edit(te, self.pipe.tokenizer, requests, hp, hp.layers, hp.mom2_update_weight, self.stats_dir,
                                              cache_name, "", self.verbose, shard, _default_stage1(self.pipe, hp, stage1)),
            True, "apply", "step", "new", f"session step {self.steps}", "the edited weights have been restored and ")
        LP = clip_forward.LAST_PATHS
        # all edited layers together: their rows are already behind row M
        self.keys.commit(n, hip.row_scale_of(self._fixed[1], plan.cov_factors, self._fixed[0]))
        self.steps += 1
        self._ledger += [(r.get("source"), "edit", self.steps, t) for r in requests for t in range(self._fixed[3])]
        if self._report_pending is not None:
            self._report, self._report_pending = self._report_pending, None
        if self.private_factors is None:            # the workspace this step's rows are coordinates of, and its statistics
            self._shared = (plan.cov_factors, [plan.covs[l] for l in plan.layers])
        LP["session_steps"], LP["session_preserved_rows"] = self.steps, self.keys.M
        LP["session_folds"], LP["session_folded_rows"] = self.folds, self.folded
        if self.verbose:
            print(f"Session step {self.steps}: {n} concept rows inserted, {self.keys.M} preserved")
        return self.pipe, origin_text_encoder

    def retain(self, requests: List[Dict], weight: float = 1.0, shard=None) -> int:
        """Enter the keys of ``requests`` into the preserved set with a zero residual: later steps leave these concepts where they
        are (class docstring).  ``weight``: how much a retained key counts against an edited one (finite, > 0).  No parameter of the
        encoder changes.  Returns the rows added (len(requests) x num_edit_tokens).  Refuses what ``apply`` refuses; with
        ``on_full="raise"`` a list that does not fit raises ``PreservedSetFull`` before anything is launched, with ``"fold"`` the set
        is folded first, and a list longer than ``capacity`` goes in chunks with a fold between them.  A non-positive pivot raises
        ``torch.linalg.LinAlgError`` with nothing committed (of the chunk in flight)."""
        try:
            w = float(weight)
        except (TypeError, ValueError) as e:
            raise ValueError(f"weight must be a positive finite number (got {weight!r})") from e
        if not (np.isfinite(w) and w > 0.0):
            raise ValueError(f"weight must be a positive finite number (got {weight!r})")
        self._check_call(requests, shard, "a retain list")
        k = self._fixed[3]
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
        n = len(requests) * self._fixed[3]
        if self.preserved + n > self.capacity:
            self.fold()
        hp, te = self.hparams, self.pipe.text_encoder
        self._ensure_keys()

        def make_plan():
            plan = prepare_text_encoder_edit(te, self.pipe.tokenizer, requests, hp, hp.layers, hp.mom2_update_weight, self.stats_dir,
                                             None, "", self.verbose, shard, None, with_targets=False)
            plan.retain_weight = w
            return plan

        plan = self._run_plan(make_plan, False, "retain", "call", "retained", f"retain after step {self.steps}")   # (writes no weight)
        LP = clip_forward.LAST_PATHS
        self.keys.commit(n, hip.row_scale_of(self._fixed[1], plan.cov_factors, self._fixed[0], w))
        self.retained += n
        self._ledger += [(r.get("source"), "retain", self._retains, t) for r in requests for t in range(self._fixed[3])]
        if self.private_factors is None:
            self._shared = (plan.cov_factors, [plan.covs[l] for l in plan.layers])
        LP["session_preserved_rows"], LP["session_retained_rows"] = self.keys.M, self.retained
        LP["session_folds"], LP["session_folded_rows"] = self.folds, self.folded
        if self.verbose:
            print(f"Session retain: {n} concept rows retained at weight {w:g}, {self.keys.M} preserved")

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
        names = [s["source"] if isinstance(s, dict) else s for s in sources]
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
        LP = clip_forward.LAST_PATHS
        LP["session_released_rows"], LP["session_preserved_rows"], LP["session_retained_rows"] = self.released, kept, self.retained
        if self.verbose:
            print(f"Session release: {M - kept} rows of {len(set(names))} sources released, {kept} preserved")
        return M - kept

    def _release_rebuild(self, keep, first, M):
        """The device half of a release: rows [first, len(keep)) of every edited layer rebuilt in place from the kept rows
        (``hip.session_release``), ONE pinned flag read, and on a non-zero flag rows [first, M) and the touched tile inverses put back."""
        keys, n_rebuilt = self.keys, len(keep) - first
        dev = keys.Yp[0].device
        ws = self._release_ws
        if ws is None or ws.key != (n_rebuilt, keys.d, keys.capacity):
            self._release_ws = None                 # (drop the old one first: the largest is of the order of the state itself)
            ws = self._release_ws = hip.ReleaseWorkspace(n_rebuilt, keys.d, keys.capacity, dev)
        keep_dev = torch.tensor(keep, dtype=torch.int32, device=dev)
        t0, t1 = first // hip.NB, (M + hip.NB - 1) // hip.NB
        snap = [(keys.Yp[i][first:M].clone(), keys.Lp[i][first:M].clone(), keys.tile_inv[i][t0:t1].clone())
                for i in range(keys.n_layers)]
        ws.info.zero_()
        for i in range(keys.n_layers):
            hip.session_release(keys, i, keep_dev, first, ws=ws)
        code = self._read_flag(ws.info)
        if code != 0:
            for i, (y, l, t) in enumerate(snap):
                keys.Yp[i][first:M].copy_(y)
                keys.Lp[i][first:M].copy_(l)
                keys.tile_inv[i][t0:t1].copy_(t)
            ws.info.zero_()
            raise torch.linalg.LinAlgError(
                f"release after step {self.steps}: the system of the {n_rebuilt} kept rows behind row {first} is not positive definite "
                f"(non-positive pivot at column {code - 1}); the {M} preserved rows are as they were and nothing was released")

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
        keep = (fac.buf.clone(), base.clone())              # (a refused refold puts both back)
        fac.info.zero_()
        for i in range(keys.n_layers):
            hip.session_refold_update(fac, keys, i, self._archive[i], n0, rel_dev, base)
        hip.cov_factor_refactor(fac)
        code = self._read_flag(fac.info)
        if code != 0:
            fac.buf.copy_(keep[0])
            base.copy_(keep[1])
            fac.info.zero_()
            fac.have_inverse = set(range(fac.n_layers))
            raise torch.linalg.LinAlgError(
                f"release after step {self.steps}: the folded system without the {len(rel)} released rows is not positive definite "
                f"(non-positive pivot at column {code - 1}); the {M} preserved and {n0} folded rows, the private factors and the "
                f"weights are as they were and nothing was released")
        del keep
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
        LP = clip_forward.LAST_PATHS
        LP["session_released_rows"], LP["session_preserved_rows"], LP["session_retained_rows"] = self.released, 0, self.retained
        LP["session_folds"], LP["session_folded_rows"] = self.folds, self.folded
        if self.verbose:
            print(f"Session release: {len(arch)} folded and {len(live)} live rows of {len(set(names))} sources released by a refold, "
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
        """The device half of rescale / reweight: rows [first, M) of every edited layer scaled in place by ``dev_factors`` (M,) and
        everything behind ``first`` rebuilt (``hip.session_rescale``), after rows [first, M) of Yp, Lp and the touched tile inverses
        were copied; ONE pinned flag read (``extra_info``: a second flag word read with it), and on a non-zero flag the copy put
        back and ``torch.linalg.LinAlgError``.  Returns ``undo()``, which puts the copy back later."""
        keys, M = self.keys, self.preserved
        dev = keys.Yp[0].device
        ws = self._rescale_ws
        if ws is None or ws.key != (M - first, keys.d, keys.capacity):
            self._rescale_ws = None                 # (drop the old one first: the largest is of the order of the state itself)
            ws = self._rescale_ws = hip.RescaleWorkspace(M - first, keys.d, keys.capacity, dev)
        t0, t1 = first // hip.NB, (M + hip.NB - 1) // hip.NB
        snap = [(keys.Yp[i][first:M].clone(), keys.Lp[i][first:M].clone(), keys.tile_inv[i][t0:t1].clone())
                for i in range(keys.n_layers)]

        def undo():
            for i, (y, l, t) in enumerate(snap):
                keys.Yp[i][first:M].copy_(y)
                keys.Lp[i][first:M].copy_(l)
                keys.tile_inv[i][t0:t1].copy_(t)

        ws.info.zero_()
        for i in range(keys.n_layers):
            hip.session_rescale(keys, i, dev_factors, first, ws=ws)
        self._rescales += keys.n_layers
        clip_forward.LAST_PATHS["session_rescales"] = self._rescales
        code = self._read_flag(ws.info if extra_info is None else torch.maximum(ws.info, extra_info.to(ws.info.device)))
        if code != 0:
            undo()
            ws.info.zero_()
            raise torch.linalg.LinAlgError(
                f"{what} after step {self.steps}: the system of the {M - first} scaled rows behind row {first} (or lam C' at the new "
                f"point) is not positive definite (non-positive pivot at column {code - 1}); the {M} preserved rows, the session's "
                f"point and the weights are as they were")
        return undo

    def _rescale(self, mom2_weight, edit_weight, shard, what: str):
        """``rescale`` proper; returns ``undo()``, which makes the session what it was before (``apply(point=)`` calls it when its
        step fails)."""
        lam0, e0, layers, k = self._fixed
        try:
            lam = lam0 if mom2_weight is None else float(mom2_weight)
            e = e0 if edit_weight is None else float(edit_weight)
        except (TypeError, ValueError) as err:
            raise ValueError(f"mom2_weight and edit_weight must be numbers (got {mom2_weight!r}, {edit_weight!r})") from err
        if not (np.isfinite(lam) and lam > 0.0):
            raise ValueError(f"mom2_update_weight must be positive and finite in a session (got {lam}): the dual solver factors lam C'")
        if not (0.0 < e < 1.0):
            raise ValueError(f"edit_weight must lie inside (0, 1) in a session (got {e})")
        self._refuse_rescale(shard, what)
        if (lam, e) == (lam0, e0):                  # (the point it is at: nothing to scale, nothing to drop)
            return lambda: None
        hp, M = self.hparams, self.preserved
        before = (self._fixed, hp.mom2_update_weight, hp.edit_weight, self._shared, self._report)
        undo_rows, scale0 = None, None
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
            scale0 = keys.row_scale[:M].clone()
            keys.rescale_commit(math.sqrt(old.lam_ratio(lam0) / fac.lam_ratio(lam)))
            self._shared = (fac, covs)
        self._fixed = (lam, e, layers, k)
        hp.mom2_update_weight, hp.edit_weight = lam, e
        self._report = self._report_pending = None
        clip_forward.LAST_PATHS["session_preserved_rows"] = M

        def undo():
            if undo_rows is not None:
                undo_rows()
                self.keys.row_scale[:M] = scale0
            self._fixed, hp.mom2_update_weight, hp.edit_weight, self._shared, self._report = before

        return undo

    def rescale(self, mom2_weight=None, edit_weight=None, shard=None):
        """The session's mom2_update_weight and edit_weight from now on (``None``: as it is).  Held rows keep the raw scale they were
        committed with — P does not change, only the base term a C, a = 2 lam (1 - e), does — so per edited layer ONE
        ``hip.session_rescale`` call with the uniform factor sqrt(a / a') and first = 0 makes the rows coordinates of the new
        point's factor and rebuilds Lp and the tile inverses: no forward, no statistics read by the rows, no weight moved.  Atomic
        like ``release``: rows [0, M) of every layer are copied first, all layers run, ONE pinned flag read decides; zero commits
        all layers together with ``hparams`` (the same two fields the constructor read), the factors later steps, ``fold()`` and
        ``save`` refer to (those of the new point, from the factor cache as a step takes them) and ``row_scale``; non-zero puts
        everything back and raises ``torch.linalg.LinAlgError``.  A stored ``report()`` readout is dropped.  With no preserved row
        only the numbers change; the point the session is at already changes nothing.  ``ValueError`` before anything is
        launched: a bad value (the constructor's rules), a session that has folded, and what ``apply`` refuses."""
        self._rescale(mom2_weight, edit_weight, shard, "rescale")
        if self.verbose:
            print(f"Session rescale: mom2_update_weight {self._fixed[0]:g}, edit_weight {self._fixed[1]:g}, {self.preserved} preserved")

    def reweight(self, sources, weight: float, shard=None) -> int:
        """Every live row of ``sources`` (``request["source"]`` strings, or request dicts) counts from now on like a key retained now
        at ``weight``: its rows are multiplied by (that row scale) / (the one they hold) — 1 for every other row — and everything
        behind the smallest changed row is rebuilt (``hip.session_rescale``), atomically as in ``rescale``.  No weight of the
        encoder moves.  Returns the rows changed.  Errors are ``release``'s (``KeyError``: a source without a live row;
        ``ValueError``: a folded source, an empty list, a weight that is not positive and finite, a folded session, what ``apply``
        refuses), all before anything is launched or allocated."""
        try:
            w = float(weight)
        except (TypeError, ValueError) as e:
            raise ValueError(f"weight must be a positive finite number (got {weight!r})") from e
        if not (np.isfinite(w) and w > 0.0):
            raise ValueError(f"weight must be a positive finite number (got {weight!r})")
        names = [s["source"] if isinstance(s, dict) else s for s in sources]
        self._refuse_rescale(shard, "a reweight")
        keep, _, _ = release_plan(self._ledger, self._folded_sources, names)
        kept = set(keep)
        rows = [i for i in range(len(self._ledger)) if i not in kept]
        M = self.preserved
        assert M == len(self._ledger) and rows
        lam, e, _, _ = self._fixed
        target = hip.row_scale_of(e, self._shared[0], lam, w)
        f = torch.ones(M, dtype=torch.float64)
        idx = torch.tensor(rows, dtype=torch.long)
        f[idx] = target / self.keys.row_scale[idx]
        changed = [i for i in rows if float(f[i]) != 1.0]
        if changed:
            self._scale_rows(f.to(self.keys.Yp[0].device), changed[0], "reweight")
            self.keys.rescale_commit(f)
        self._report = self._report_pending = None
        if self.verbose:
            print(f"Session reweight: {len(rows)} rows of {len(set(names))} sources at weight {w:g}")
        return len(rows)

    def sweep(self, requests: List[Dict], grid, cache_name: Optional[str] = None, scorer=None, visit=None, shard=None,
              stage1=None) -> List[Dict]:
        """Trial steps of ``requests`` at every (mom2_weight, edit_weight) pair of ``grid`` (``edit_engine.validate_grid``), nothing
        committed: the sweep -> score -> ``select_point`` workflow on ONE step of a session.  The held rows are copied once and the
        requests prepared once (tokenization, trie, prefix launches, v* rows: ``edit_engine.SweepWalk``'s shared part, with the
        statistics factored at unit scale at most once per edited layer); per pair the live state is scaled OUT OF THE COPY to the
        pair (``hip.session_rescale`` with ``src``), the factors are the unit ones rescaled (``hip.cov_factor_rescale``), the
        step's chain runs as ``apply`` runs it with its rows behind row M (M is not bumped), the flags are read, the entry is
        filled and the weights are put back.  Returns one dict per pair: ``point``, ``score`` (``scorer.score()`` of an
        ``EditScorer`` built on the baseline weights; ``None`` without one), ``report`` (``report()``'s dict on a ``report=True``
        session), ``visit`` (``visit(pair, pipe)``'s result) and ``error`` (``None``, or the message of the non-positive pivot that
        point met — the walk goes on; ``torch.linalg.LinAlgError`` only if every point failed).  On return, also when ``visit``
        raises, the state is back from the copy byte for byte and weights, ``preserved``, ledger, ``steps``, the point and
        ``hparams`` are as before.  A weight rewritten behind the forward's caches (``StaleWeightCacheError``) has the plan made again
        once, as for a step, and the walk goes on at the point that met it.  One pinned flag read per point.  Refuses what
        ``rescale`` refuses, an empty grid or request list, and a step that does not fit."""
        pts = edit_engine.validate_grid(grid)
        n = self._check_step(requests, shard)
        self._refuse_rescale(shard, "a sweep")
        if self.preserved + n > self.capacity:
            raise PreservedSetFull(f"{self.preserved} preserved + {n} new concept rows exceed the session's capacity {self.capacity}: "
                                   f"a sweep does not fold")
        LP = clip_forward.LAST_PATHS
        LP["session_sweep_points"] = 0
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
                _note_stale("EditSession.sweep", e, "point")
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
        hp, te, LP = self.hparams, self.pipe.text_encoder, clip_forward.LAST_PATHS
        lam0, e0, _, _ = self._fixed
        keys, M = self.keys, self.preserved
        dev = keys.Yp[0].device
        rows, t1 = min(M + n, keys.capacity), (M + n + hip.NB - 1) // hip.NB
        plan = prepare_text_encoder_edit(te, self.pipe.tokenizer, requests, hp, hp.layers, hp.mom2_update_weight, self.stats_dir,
                                         cache_name, "", self.verbose, shard, _default_stage1(self.pipe, hp, stage1))
        plan.session = self
        snap = [(keys.Yp[i][:rows].clone(), keys.Lp[i][:rows].clone(), keys.tile_inv[i][:t1].clone()) for i in range(keys.n_layers)]
        scale0, report0 = keys.row_scale[:M].clone(), self._report
        rws = own_info = None
        if M > 0:
            rws = self._rescale_ws
            if rws is None or rws.key != (M, keys.d, keys.capacity):
                self._rescale_ws = None             # (drop the old one first: the largest is of the order of the state itself)
                rws = self._rescale_ws = hip.RescaleWorkspace(M, keys.d, keys.capacity, dev)
            own_info = rws.info
        factor = torch.empty(max(M, 1), dtype=torch.float64, device=dev)[:M]
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
                                hip.session_rescale(keys, i, factor, 0, src=snap[i][0], ws=rws)
                            self._rescales += keys.n_layers
                            # (the point's factors are at its own lam: a preserved row's unit is its raw scale)
                            keys.row_scale[:M] = scale0 * math.sqrt(self._shared[0].lam_ratio(lam0))
                        plan.chunk.state = walk.state
                        self._report_pending = None
                        try:
                            edit_engine.run_encoder_edit(plan, keep_factors=False, restore=False)
                            check_info(plan)            # (puts the weights back itself before it raises)
                        except FloatingPointError as err:
                            entry["error"] = str(err)
                        LP["session_sweep_points"] += 1
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
            for i, (y, l, t) in enumerate(snap):
                keys.Yp[i][:rows].copy_(y)
                keys.Lp[i][:rows].copy_(l)
                keys.tile_inv[i][:t1].copy_(t)
            keys.row_scale[:M] = scale0
            self._report, self._report_pending = report0, None
            LP["session_rescales"] = self._rescales

    def reset(self):
        """Forget the preserved keys; the weights stay as they are, the next step starts a fresh set (M = 0)."""
        if self.keys is not None:
            self.keys.reset()
        self.steps = 0
        self.private_factors = self._base = self._shared = None
        self.folded = self.folds = self.retained = self.released = self._retains = 0
        self._report = self._report_pending = None
        self._ledger, self._folded_sources, self._release_ws, self._rescale_ws = [], set(), None, None
        self._archive, self._archived, self._archive_ledger = None, 0, []
        LP = clip_forward.LAST_PATHS
        LP["session_steps"] = LP["session_preserved_rows"] = LP["session_folds"] = LP["session_folded_rows"] = 0
        LP["session_retained_rows"] = LP["session_released_rows"] = 0
        LP["session_rescales"] = LP["session_sweep_points"] = self._rescales = 0

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
        for l in self._fixed[2]:
            name = hp.rewrite_module_tmp.format(l)
            c = get_cov_text_encoder(te, self.pipe.tokenizer, name, hp.mom2_dataset, hp.mom2_n_samples, hp.mom2_dtype,
                                     stat_dir=self.stats_dir, verbose=self.verbose)
            out.append((name, str(stats_filename(self.stats_dir, "text_encoder", hp.mom2_dataset, name, hp.mom2_dtype, ["mom2"],
                                                 3 * 1024, hp.mom2_n_samples)), c))
        return out

    def save(self, path) -> dict:
        """Write everything a later process needs to carry this session on to ONE file (``torch.save`` of CPU tensors and plain
        values; INTEGRATION.md, "session file"): the fixed set-up, the counters and ledgers, the committed rows of every layer in a
        form that knows nothing of the capacity (``hip.PreservedKeys.state_dict``), the edited weights as they are and as they were
        before the first step, ``base`` of a folded session (not its factored workspace: four times the size, and rebuilt by
        ``load``), the counted rows of a ``keep_folded`` archive, and content fingerprints of every other parameter of the encoder
        and of the statistics, so that ``load`` can refuse another encoder or other statistics.  May be called between any two
        operations; the session is not changed.  One synchronising copy to the host; the file is written under a temporary name
        beside ``path`` and renamed.  Returns {"rows", "folded", "archived", "bytes"}."""
        weights = self._weights()
        w0 = next(iter(weights.values()))
        if not w0.is_cuda:
            raise hip.EmcidHipError(f"the text encoder must live in HBM (got {w0.device}); there is no CPU path")
        dev, (lam, e, layers, k) = w0.device, self._fixed
        pending = []

        def host(t: torch.Tensor) -> torch.Tensor:
            out = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            out.copy_(t.detach(), non_blocking=True)
            pending.append(out)
            return out

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
            "counters": {"steps": self.steps, "folds": self.folds, "folded": self.folded, "retained": self.retained,
                         "released": self.released, "retains": self._retains},
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
        del pending
        nbytes = _write_session_file(state, path)
        if self.verbose:
            print(f"Session saved to {path}: {self.preserved} preserved and {self.folded} folded rows, {nbytes} bytes")
        return {"rows": self.preserved, "folded": self.folded, "archived": self._archived, "bytes": nbytes}

    @classmethod
    def load(cls, pipe, hparams: EMCIDHyperParams, path, device: Optional[str] = None, stats_dir=STATS_DIR,
             capacity: Optional[int] = None, weights: str = "check", verbose: bool = False, on_full: Optional[str] = None,
             report: Optional[bool] = None) -> "EditSession":
        """The session ``save`` wrote to ``path``, carried on in this process on ``pipe``: every public attribute and listing is
        the saved session's, the next step preserves what its next step would have preserved, ``restore()`` gives the weights of
        before its first step.  The first four arguments are the constructor's; ``hparams`` must agree with the file's fixed set-up.
        ``capacity``: default the file's; any value >= the saved M (the rows and tiles go where the new layout wants them).
        ``on_full`` / ``report``: default the file's; ``keep_folded`` is the file's.  ``weights="check"``: the encoder's edited
        weights must equal the file's bit for bit (``ValueError`` naming the first that differs); ``"load"``: the file's are copied
        into the encoder, last of all.  In both modes every other parameter of the encoder and every edited layer's statistics
        must have the fingerprint the file recorded (``ValueError`` naming the parameter, or the layer and its statistics file).
        The factors of lam C' come from the engine's factor cache as for a step; a folded session's private factors are rebuilt
        from ``base`` in one batched chain.  ONE pinned read of fingerprints, comparisons and flag follows; a non-positive pivot
        raises ``torch.linalg.LinAlgError``.  Whatever is refused, the encoder's weights are as they were.  Refuses what ``apply``
        refuses; everything the file alone can show to be wrong is refused before any device call (``check_session_state``)."""
        if weights not in ("check", "load"):
            raise ValueError(f"weights must be 'check' or 'load' (got {weights!r})")
        state = _read_session_file(path)
        check_session_state(state)                  # (whole in itself, before anything of it is used)
        sess = cls(pipe, hparams, device, stats_dir, state["capacity"] if capacity is None else capacity, verbose,
                   state["on_full"] if on_full is None else on_full, state["report"] if report is None else report,
                   keep_folded=state["keep_folded"])
        M = check_session_state(state, sess._fixed, hparams.rewrite_module_tmp, sess.d, sess.h, sess.capacity)
        sess._check_call([None], None, "a load")
        live = sess._weights()
        w0 = next(iter(live.values()))
        if not w0.is_cuda:
            raise hip.EmcidHipError(f"the text encoder must live in HBM (got {w0.device}); there is no CPU path")
        dev, (lam, e, layers, _) = w0.device, sess._fixed
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
        flags = torch.cat([d.to(torch.int32) for d in differs] + [info])
        host = torch.empty(flags.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(flags, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()        # the ONE synchronising read
        host = host.tolist()
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
        sess.steps, sess.folds, sess.folded = counters["steps"], counters["folds"], counters["folded"]
        sess.retained, sess.released, sess._retains = counters["retained"], counters["released"], counters["retains"]
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
        LP = clip_forward.LAST_PATHS
        LP["session_steps"], LP["session_preserved_rows"], LP["session_loaded_rows"] = sess.steps, M, M
        LP["session_folds"], LP["session_folded_rows"] = sess.folds, sess.folded
        LP["session_retained_rows"], LP["session_released_rows"] = sess.retained, sess.released
        if verbose:
            print(f"Session loaded from {path}: {M} preserved and {sess.folded} folded rows after {sess.steps} steps")
        return sess


# ---- edit scores: did the edit take, and what did it move --------------------------------------------------------------------

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


def score_row_sources(requests: Sequence[Dict], num_edit_tokens: int = 1) -> List[tuple]:
    """[(source, token index)] in the row order of an edit's concept stack: row rq * k + num (the reference's "rq num")."""
    k = int(num_edit_tokens)
    return [(r["source"], num) for r in requests for num in range(k)]


SCORE_MAX_CHAIN = 128       # nodes per holdout chain the readout takes (csrc/score.hip; the trie forward's own limit too)


def holdout_tokens(tokenizer, prompts: Sequence[str], n_positions: Optional[int] = None):
    """Generic prompts tokenized for the holdout trie, host only: ((B, S) int64 ids, (B,) int64 EOS positions).  A chain BOS ... EOS
    longer than ``SCORE_MAX_CHAIN`` nodes, or than the encoder's ``n_positions`` position embeddings, is refused here."""
    from .compute_z import tokenize_lists
    prompts = list(prompts)
    if not prompts or not all(isinstance(p, str) for p in prompts):
        raise ValueError("holdout must be a non-empty list of prompt strings")
    enc = tokenize_lists(tokenizer, prompts)
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
    raw.  State held: the two entering states, Z0, H0, v*, fp32 in HBM.

    ``score()`` replays layers[0] ... from the two kept states (``run_layers_from`` only reads them): the request trie to
    layers[-1], the holdout trie to the last layer on every node; Z by the engine's own gather; then TWO launches
    (``hip.score_rows`` on (Z, Z0, v*) and, behind the final LayerNorm in fp64, on (H, H0); ``hip.score_chains`` over the holdout
    chains) and ONE pinned readback, the only host synchronisation.  Everything is issued eagerly on the current stream; no weight
    is moved and every parameter is bit-identical afterwards; the forward's weight-derived caches refresh themselves as in any
    forward.  Two calls in a row return the same bits.

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
        if _shard_from_env(shard).collective:
            raise ValueError("EditScorer runs on one rank: a collective ConceptShard is not supported")
        if len(requests) == 0:
            raise ValueError("EditScorer needs at least one request")
        layers = list(hparams.layers)
        if not layers or sorted(layers) != layers:
            raise ValueError(f"hparams.layers must be a non-empty list in forward order (got {hparams.layers})")
        te, tok = pipe.text_encoder, pipe.tokenizer
        try:
            weights = [nethook.get_parameter(te, f"{hparams.rewrite_module_tmp.format(l)}.weight") for l in layers]
        except LookupError as e:
            raise ValueError(f"EditScorer scores edits of the text encoder's MLP projections; {hparams.rewrite_module_tmp!r} names no "
                             f"weight of pipe.text_encoder (cross-attention edits are not supported): {e}") from e
        w = weights[0]
        if device is not None and torch.device(device).type != w.device.type:
            raise ValueError(f"device {device!r} but the text encoder's weights live on {w.device}")
        holdout = list(holdout) if holdout is not None else []
        if not holdout or not all(isinstance(p, str) for p in holdout):
            raise ValueError("holdout must be a non-empty list of prompt strings")
        layer_tmp = getattr(hparams, "layer_module_tmp", None)
        if layer_tmp is None:
            raise clip_forward.UnsupportedEncoder("hparams.layer_module_tmp is not set: no prefix-trie forward")
        if not (w.is_cuda and w.dtype == torch.float32):
            raise clip_forward.UnsupportedEncoder(f"the prefix-trie forward runs fp32 in HBM (got {w.dtype} on {w.device})")
        try:
            graph = clip_forward.discover_cached(te, layer_tmp)
            if any(graph.layers[l].fc2.weight is not wl for l, wl in zip(layers, weights)):
                raise clip_forward.UnsupportedEncoder("rewrite_module_tmp is not the layer's mlp.fc2")
        except (IndexError, LookupError) as e:
            raise clip_forward.UnsupportedEncoder(str(e)) from e
        ln = graph.final_layer_norm
        h = int(w.shape[0])
        if not (isinstance(ln, torch.nn.LayerNorm) and ln.weight is not None and ln.bias is not None and ln.weight.is_cuda
                and ln.weight.dtype == torch.float32 and tuple(ln.normalized_shape) == (h,) and h % 4 == 0 and h <= hip.SCORE_MAX_COLS):
            raise clip_forward.UnsupportedEncoder(f"the score's readout takes an affine fp32 final LayerNorm over h = {h} columns "
                                                  f"(h % 4 == 0, h <= {hip.SCORE_MAX_COLS})")
        # (host only: a holdout chain the readout or the position table cannot take is refused before anything is launched)
        ids_h, eos_h = holdout_tokens(tok, holdout, graph.position_embedding.num_embeddings)
        if _plan is None and _any_vstar_missing(requests, hparams, cache_name, ""):
            raise FileNotFoundError(f"a v* file of the {len(requests)} requests is missing under {cache_name!r}: an EditScorer reads "
                                    f"the targets an edit was made towards and never runs Stage 1")
        k = int(getattr(hparams, "num_edit_tokens", 1) or 1)
        self.pipe, self.hparams, self.layers, self.graph, self.k = pipe, hparams, layers, graph, k
        self.sources, self.holdout = score_row_sources(requests, k), holdout
        dev = w.device
        # ``_plan`` (sweep_emcid_text_encoder): the sweep's own prepared plan of these very requests — its trie, its v* rows (read,
        # or computed by Stage 1, the way a call does) and the state its prefix run left, which the sweep's points replay as well
        plan = _plan if _plan is not None else prepare_encoder_edit(
            te, tok, requests, layers, hparams.rewrite_module_tmp, float(hparams.mom2_update_weight), float(hparams.edit_weight),
            lambda: load_v_stars(requests, hparams, cache_name, "", None, width=h, pin=True),
            lambda: {}, ConceptShard(), layer_module_tmp=layer_tmp, num_edit_tokens=k)
        if plan.chunk is None or plan.graph is not graph or plan.chunk.state is None or plan.chunk.state[0] != layers[0] \
                or plan.layers != layers or plan.num_edit_tokens != k:
            raise clip_forward.UnsupportedEncoder("the requests did not take the prefix-trie forward")
        self.chunk, self.zs = plan.chunk, plan.resolve_targets()
        self._state = tuple(plan.chunk.state[1:])
        if _plan is None:
            plan.chunk.state = None
        with torch.no_grad():
            self.trie_h, self.eos = clip_forward.build_trie(ids_h, eos_h, dev), eos_h
            self._state_h = tuple(clip_forward.run_prefix(graph, self.trie_h, layers[0]))
            self._frozen = self._signature()
            Z0, H0 = self._forward()
        self.Z0, self.H0 = Z0.clone(), H0
        n, B = self.Z0.shape[0], len(holdout)
        if n != len(self.sources) or tuple(self.zs.shape) != tuple(self.Z0.shape):
            raise ValueError(f"{n} concept rows for {len(self.sources)} (source, token) pairs and v* of shape {tuple(self.zs.shape)}")
        self._out = torch.empty(n * 8 + B * 4, dtype=torch.float64, device=dev)
        self._node = torch.empty(H0.shape[0], 8, dtype=torch.float64, device=dev)
        self._host = torch.empty(n * 8 + B * 4, dtype=torch.float64, pin_memory=True)

    def _signature(self):
        """(name, identity, address, in-place version) of every parameter but the edited fc2 weights — of those: identity alone."""
        edited = {id(self.graph.layers[l].fc2.weight) for l in self.layers}
        return tuple((n, id(p)) if id(p) in edited else (n, id(p), p.data_ptr(), p._version)
                     for n, p in self.pipe.text_encoder.named_parameters())

    def _forward(self):
        """(Z (N k, h), H (holdout nodes, h)) fp32 on the weights as they are: the replay from the two kept states."""
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
        H = clip_forward.run_layers_from(g, self.trie_h, self._state_h, first, len(g.layers) - 1, None, last_rows_only=False)[0]
        if g.guard is not None:
            g.guard.flush()          # (fingerprints of the weights that cache entries were made from in this replay, if any)
        clip_forward.LAST_PATHS["score_replays"] = clip_forward.LAST_PATHS.get("score_replays", 0) + 1
        return box[0], H

    def score(self) -> EditScore:
        """Score the weights as they are against the baseline of construction (class docstring): one replay, two launches, one
        pinned readback."""
        if self._signature() != self._frozen:
            now = dict((s[0], s) for s in self._signature())
            moved = [s[0] for s in self._frozen if now.get(s[0]) != s]
            raise ValueError(f"parameters other than the edited fc2 weights changed since this EditScorer was built "
                             f"({', '.join(moved[:4]) or 'the parameter list'}{', ...' if len(moved) > 4 else ''}): its kept states "
                             f"are no longer this encoder's; build a new EditScorer")
        n, B = self.Z0.shape[0], len(self.holdout)
        with torch.no_grad():
            Z, H = self._forward()
            hip.score_rows(Z, self.Z0, t=self.zs, out=self._out[:n * 8].view(n, 8))
            hip.score_rows(H, self.H0, ln=self.graph.final_layer_norm, out=self._node)
            hip.score_chains(self._node, self.trie_h.anc, self.trie_h.depth, self.trie_h.lookup_node,
                             out=self._out[n * 8:].view(B, 4))
            self._host.copy_(self._out, non_blocking=True)
            torch.cuda.current_stream(self._out.device).synchronize()
        rows, chains = self._host[:n * 8].view(n, 8).clone(), self._host[n * 8:].view(B, 4).clone()
        moved2, resid2, resid02, dot = rows[:, 0], rows[:, 4], rows[:, 5], rows[:, 6]
        tiny = torch.finfo(torch.float64).tiny
        left = torch.where(resid02 > 0, (resid2 / resid02.clamp(min=tiny)).sqrt(), torch.zeros_like(resid2))
        den = (moved2 * resid02).sqrt()
        cos = torch.where(den > 0, dot / den.clamp(min=tiny), torch.zeros_like(dot))
        return EditScore(self.sources, left, cos, resid2.sqrt(), resid02.sqrt(), self.holdout, chains[:, 0].clone(),
                         chains[:, 1].clone(), chains[:, 2].clone(), chains[:, 3].clone())


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


class _PairEncoder:
    """One encoder of a ``PairEditScorer``: what ``EditScorer`` keeps of its one encoder, with the holdout read one layer earlier
    (``hidden_states[-2]``, raw) and, ``pooled``, the last layer continued on the EOS rows."""

    def __init__(self, te, graph, layers, plan, ids_h, eos_h, pooled: bool, keep_state: bool = False):
        self.te, self.graph, self.layers, self.pooled = te, graph, layers, pooled
        self.chunk, self.zs = plan.chunk, plan.resolve_targets()
        self._state = tuple(plan.chunk.state[1:])
        if not keep_state:          # (a sweep's own plan: its points replay the state as well)
            plan.chunk.state = None
        dev = self.zs.device
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

    def forward(self):
        """(Z (N, h), H (holdout nodes, h) after the penultimate layer, H_last (B, h) at the EOS rows | None), fp32, on the weights
        as they are: the replay from the two kept states."""
        g, ch, first, last = self.graph, self.chunk, self.layers[0], self.layers[-1]
        box = []

        def on_fc2(li, x, out, mid=None, next_ln=None):
            # the engine's own Zc of its last layer (EditScorer._forward)
            if li != last:
                return out
            layer = g.layers[li]
            xf = x.float() if isinstance(x, hip.SplitRows) else x
            K = hip.gather_mean(xf.unsqueeze(0).expand(ch.lookup_query.numel(), -1, -1), ch.lookup_query, ch.cseg)
            box.append(clip_forward.linear(K, layer.fc2.weight, layer.fc2.bias, wsp=layer.split_of("fc2")))
            return None

        clip_forward.run_layers_from(g, ch.trie, self._state, first, last, on_fc2, fc2_by_callback=(last,), edit_callback=True)
        n_layers = len(g.layers)
        # hidden_states[-2]: every node, raw; when it lies before the first edited layer it is the kept state itself
        state = self._state_h if first > n_layers - 2 else \
            clip_forward.run_layers_from(g, self.trie_h, self._state_h, first, n_layers - 2, None, last_rows_only=False)
        h_last = None
        if self.pooled:       # the last layer continued on the distinct EOS nodes, then one row per prompt
            rows = clip_forward.run_layers_from(g, self.trie_h, state, n_layers - 1, n_layers - 1, None, last_rows_only=True)[0]
            h_last = rows.index_select(0, self.trie_h.lookup_in_query)
        if g.guard is not None:
            g.guard.flush()
        clip_forward.LAST_PATHS["score_replays"] = clip_forward.LAST_PATHS.get("score_replays", 0) + 1
        return box[0], state[0], h_last


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
    keeps, per encoder, Z0_e (N, h_e) and the penultimate H0_e (holdout nodes of that trie, h_e), and for TE2 with a projection
    H0last (B, h_2) at the EOS rows — all fp32 in HBM.

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
    (``_half``: the one statement of it) once per DISTINCT point of that encoder, one ``hip.score_chains_pair_grid`` for all the
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
        if _shard_from_env(shard).collective:
            raise ValueError("PairEditScorer runs on one rank: a collective ConceptShard is not supported")
        if len(requests) == 0:
            raise ValueError("PairEditScorer needs at least one request")
        holdout = list(holdout) if holdout is not None else []
        if not holdout or not all(isinstance(p, str) for p in holdout):
            raise ValueError("holdout must be a non-empty list of prompt strings")
        layer_tmp = getattr(hparams, "layer_module_tmp", None)
        if layer_tmp is None:
            raise clip_forward.UnsupportedEncoder("hparams.layer_module_tmp is not set: no prefix-trie forward")
        for which, layers in ((1, list(hparams.layers)), (2, list(hparams.layers_2))):
            if not layers or sorted(layers) != layers:
                raise ValueError(f"the layers of text encoder {which} must be a non-empty list in forward order (got {layers})")
        found = []
        for which, te, tok, layers, suffix in ((1, pipe.text_encoder, pipe.tokenizer, list(hparams.layers), ""),
                                               (2, pipe.text_encoder_2, pipe.tokenizer_2, list(hparams.layers_2), "_2")):
            try:
                weights = [nethook.get_parameter(te, f"{hparams.rewrite_module_tmp.format(l)}.weight") for l in layers]
            except LookupError as e:
                raise ValueError(f"{hparams.rewrite_module_tmp!r} names no weight of text encoder {which}: {e}") from e
            w = weights[0]
            if device is not None and torch.device(device).type != w.device.type:
                raise ValueError(f"device {device!r} but the weights of text encoder {which} live on {w.device}")
            if not (w.is_cuda and w.dtype == torch.float32):
                raise clip_forward.UnsupportedEncoder(f"the prefix-trie forward runs fp32 in HBM (text encoder {which}: {w.dtype} on {w.device})")
            try:
                graph = clip_forward.discover_cached(te, layer_tmp)
                if any(graph.layers[l].fc2.weight is not wl for l, wl in zip(layers, weights)):
                    raise clip_forward.UnsupportedEncoder("rewrite_module_tmp is not the layer's mlp.fc2")
            except (IndexError, LookupError) as e:
                raise clip_forward.UnsupportedEncoder(str(e)) from e
            h = int(w.shape[0])
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
                    and isinstance(ln2, torch.nn.LayerNorm) and ln2.weight is not None and ln2.bias is not None
                    and ln2.weight.is_cuda and ln2.weight.dtype == torch.float32 and tuple(ln2.normalized_shape) == (h2,)):
                raise clip_forward.UnsupportedEncoder("the pooled readout takes text_projection as an fp32 nn.Linear without bias over an "
                                                      f"affine fp32 final LayerNorm of h = {h2} columns")
        return holdout, found, proj, ln2

    def __init__(self, pipe, requests: List[Dict], hparams: EMCIDXLHyperParams, device: Optional[str] = None, holdout=None,
                 cache_name: Optional[str] = None, shard=None, _plans=None, _checked=None):
        # ``_plans`` (sweep_emcid_sdxl_text_encoders): the sweep's own prepared plans of these very requests — their tries, v* rows
        # (read, or computed by Stage 1, the way a call does) and the states their prefix runs left, which the sweep's points replay
        # as well; ``_checked``: what the sweep's own call of ``_host_checks`` returned before it prepared them
        holdout, found, proj, ln2 = _checked if _checked is not None else self._host_checks(pipe, requests, hparams, device, holdout, shard)
        layer_tmp = hparams.layer_module_tmp
        for te, tok, layers, suffix, graph, h, ids_h, eos_h in found:
            if _plans is None and _any_vstar_missing(requests, hparams, cache_name, suffix):
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
                    lambda suffix=suffix, h=h: load_v_stars(requests, hparams, cache_name, suffix, None, width=h, pin=True),
                    lambda: {}, ConceptShard(), layer_module_tmp=layer_tmp, num_edit_tokens=1)
                if plan.chunk is None or plan.graph is not graph or plan.chunk.state is None or plan.chunk.state[0] != layers[0] \
                        or plan.layers != layers:
                    raise clip_forward.UnsupportedEncoder("the requests did not take the prefix-trie forward")
                self.encoders.append(_PairEncoder(te, graph, layers, plan, ids_h, eos_h, pooled=proj is not None and suffix == "_2",
                                                  keep_state=_plans is not None))
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
            now = enc.signature()
            if now != enc.frozen:
                now = dict((s[0], s) for s in now)
                moved = [s[0] for s in enc.frozen if now.get(s[0]) != s]
                raise ValueError(f"parameters of text encoder {which} other than the edited fc2 weights changed since this "
                                 f"PairEditScorer was built ({', '.join(moved[:4]) or 'the parameter list'}"
                                 f"{', ...' if len(moved) > 4 else ''}): its kept states are no longer this encoder's; build a new one")

    def _half(self, i, rows, node, chains, pooled=None):
        """Encoder i's half of a score on its weights as they are, issued on the current stream: its replay, ``score_rows`` into
        ``rows`` (N, 8) and into ``node`` (holdout nodes, 8), ``score_chains`` into ``chains`` (B, 4) and, for TE2 with a
        projection, ``score_pooled`` into ``pooled`` (B, 4)."""
        enc = self.encoders[i]
        Z, H, h_last = enc.forward()
        hip.score_rows(Z, enc.Z0, t=enc.zs, out=rows)
        hip.score_rows(H, enc.H0, out=node)
        hip.score_chains(node, enc.trie_h.anc, enc.trie_h.depth, enc.trie_h.lookup_node, out=chains)
        if enc.pooled:
            hip.score_pooled(h_last, enc.H0last, self.ln2, self.proj.weight, out=pooled)

    def _encoder_score(self, rows, chains) -> EditScore:
        """The ``EditScore`` of one encoder from its (N, 8) row sums and (B, 4) chain values on the host."""
        tiny = torch.finfo(torch.float64).tiny
        moved2, resid2, resid02, dot = rows[:, 0], rows[:, 4], rows[:, 5], rows[:, 6]
        left = torch.where(resid02 > 0, (resid2 / resid02.clamp(min=tiny)).sqrt(), torch.zeros_like(resid2))
        den = (moved2 * resid02).sqrt()
        cos = torch.where(den > 0, dot / den.clamp(min=tiny), torch.zeros_like(dot))
        return EditScore(self.sources, left, cos, resid2.sqrt(), resid02.sqrt(), self.holdout, chains[:, 0].clone(),
                         chains[:, 1].clone(), chains[:, 2].clone(), chains[:, 3].clone())

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
                self._half(i, self._part(out, i, 8), enc.node, self._part(out, 2 + i, 4), self._part(out, 5, 4) if enc.pooled else None)
            hip.score_chains_pair(e1.node, e1.trie_h.anc, e1.trie_h.depth, e1.trie_h.lookup_node,
                                  e2.node, e2.trie_h.anc, e2.trie_h.depth, e2.trie_h.lookup_node, out=self._part(out, 4, 4))
            self._host.copy_(out, non_blocking=True)
            torch.cuda.current_stream(out.device).synchronize()
        host = self._host.clone()
        pair = self._part(host, 4, 4)
        pooled = self._pooled_drift(self._part(host, 5, 4)) if self.proj is not None else None
        return PairEditScore(self._encoder_score(self._part(host, 0, 8), self._part(host, 2, 4)),
                             self._encoder_score(self._part(host, 1, 8), self._part(host, 3, 4)), self.holdout, pair[:, 0].clone(),
                             pair[:, 1].clone(), pair[:, 2].clone(), pair[:, 3].clone(), pooled)

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
                        self._half(i, rows, banks[i][g], chains, pooled if self.encoders[i].pooled else None)
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
            scores.append(PairEditScore(self._encoder_score(r1, c1), self._encoder_score(r2, c2), self.holdout, pair[c, :, 0].clone(),
                                        pair[c, :, 1].clone(), pair[c, :, 2].clone(), pair[c, :, 3].clone(),
                                        self._pooled_drift(p2) if self.proj is not None else None))
        return scores


def sweep_emcid_text_encoder(pipe, requests: List[Dict], hparams: EMCIDHyperParams, grid, device: Optional[str] = None,
                             visit=None, cache_name: Optional[str] = None, stat_dir=STATS_DIR, shard=None, stage1=None,
                             verbose: bool = False, score=None) -> list:
    """One request set at every (mom2_weight, edit_weight) pair of ``grid`` (the reference sets them per run, experiments/
    emcid_test.py:924-930, and walks lists of them, ablation.py::edit_weight_ablation) in ONE call.  For each pair, in order, the
    text encoder holds the weights ``apply_emcid_to_text_encoder(..., mom2_weight=, edit_weight=)`` would have left from the
    original ones, ``visit(point, pipe)`` is called, and its return value collected; ``visit=None`` collects {weight name: the
    edited fc2 weight, fp32 on the host}.  On return — also when ``visit`` raises — the encoder holds its original weights.

    The pairs share the preparation (tokenization, prefix trie, the unedited leading layers, the v* reads) and ONE factorization of
    the statistics per edited layer (edit_engine.run_sweep); ``hparams`` is NOT mutated.  Against a single call at the same pair
    the weights differ by the fp32 rounding of the reference's C' (:1037), far below 1e-4 max|dW|.  An encoder the trie forward
    cannot take gets one ordinary call per point (counted by clip_forward.note_fallback).  Invalid grids raise ValueError first.
    When the engine finds a weight rewritten behind the forward's caches (StaleWeightCacheError, see _retry_if_stale) the sweep is
    redone once from its first point: ``visit`` is then called again for points it has already seen, and only the second pass's
    return values are kept — a ``visit`` with side effects should be idempotent per point.

    ``score=[holdout prompt strings]`` scores every point on the device (``EditScorer``, built once on the original weights before
    the first point): with ``visit=None`` the result is one ``EditScore`` per point and no weight is copied to the host, with a
    ``visit`` it is ``(visit(point, pipe), EditScore)`` per point; ``select_point`` picks among them.  The scorer takes the sweep's
    own prepared plan — the request trie, the state after the unedited leading layers, and the v* rows as the sweep's loader got
    them (a missing v* file runs Stage 1 as without ``score=``) — so only the holdout prompts are tokenized and run in addition.
    It needs the prefix-trie forward (``UnsupportedEncoder`` otherwise, raised after the preparation) and one rank (``ValueError``).
    Without ``score=`` nothing changes."""
    from .edit_engine import run_sweep, validate_grid
    pts = validate_grid(grid)
    hp = deepcopy(hparams)
    hp.mom2_update_weight, hp.edit_weight = pts[0]
    if device is not None and torch.device(device) != next(pipe.text_encoder.parameters()).device:
        raise ValueError(f"the text encoder is on {next(pipe.text_encoder.parameters()).device}, not on {device}")
    names = [f"{hp.rewrite_module_tmp.format(layer)}.weight" for layer in hp.layers]

    scorer = None
    if score is not None:       # what a scorer refuses whatever the encoder, before the preparation launches anything
        if _shard_from_env(shard).collective:
            raise ValueError("score= runs on one rank: a collective ConceptShard is not supported")
        score = list(score)
        if not score or not all(isinstance(p, str) for p in score):
            raise ValueError("score= takes the holdout: a non-empty list of prompt strings")

    def collect(point):
        if scorer is not None:
            return scorer.score() if visit is None else (visit(point, pipe), scorer.score())
        if visit is not None:
            return visit(point, pipe)
        return {n: nethook.get_parameter(pipe.text_encoder, n).detach().to("cpu", torch.float32).clone() for n in names}

    _announce(requests, verbose)
    for attempt in (0, 1):
        plan = prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, requests, hp, hp.layers, hp.mom2_update_weight,
                                         stat_dir, cache_name, "", verbose, shard, _default_stage1(pipe, hp, stage1))
        if plan.chunk is None or plan.graph is None:
            if score is not None:
                raise clip_forward.UnsupportedEncoder("score= needs the prefix-trie forward, which this encoder or request set did not take")
            break
        if score is not None:
            # on the sweep's own plan (its trie, v* rows and prefix state: nothing is tokenized or run twice), before the first point,
            # on the original weights; again after a stale-cache retry, whose new plan belongs to a new graph
            scorer = EditScorer(pipe, requests, hp, device, holdout=score, cache_name=cache_name, shard=shard, _plan=plan)
        try:
            return run_sweep(plan, pts, lambda index, point: collect(point))
        except clip_forward.StaleWeightCacheError as e:
            # (as _retry_if_stale: the engine has put the weights back and dropped the caches; a multi-rank job raises)
            import torch.distributed as dist
            if attempt or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
                raise
            _note_stale("sweep_emcid_text_encoder", e, "sweep")
    # the hooked-HF forward has no stored state to replay: one ordinary call per point, restored after each
    clip_forward.note_fallback("sweep_emcid_text_encoder", clip_forward.UnsupportedEncoder("no prefix-trie forward: one call per point"))
    results = []
    for index, (lam, e) in enumerate(pts):
        if index:         # (the plan prepared above is the first point's)
            hp_i = deepcopy(hparams)
            hp_i.mom2_update_weight, hp_i.edit_weight = lam, e
            plan = prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, requests, hp_i, hp_i.layers, lam, stat_dir,
                                             cache_name, "", verbose, shard, _default_stage1(pipe, hp_i, stage1))
        try:
            run_checked(plan, keep_factors=False, restore=False)
            results.append(collect((lam, e)))
        finally:
            plan.restore_weights()
    return results


@_retry_if_stale
def cal_insert_deltas(pipe, weights: Dict[str, torch.Tensor], hparams: EMCIDHyperParams, requests: List[Dict],
                      zs: torch.Tensor, verbose: bool = True, stat_dir=STATS_DIR, shard=None):
    """The Stage-2 layer loop for targets the caller already has (reference: :1969-2052, used by the debias driver):
    ``zs`` is (hidden, N), one column per request.  Returns {weight_name: (adj_k, resid)} and, like the reference, LEAVES
    the edited weights in the model (its callers restore from their own copies); ``weights`` must be the live
    ``rewrite_module_tmp`` parameters of ``pipe.text_encoder`` (it is what the reference indexes, :2031-2039)."""
    for layer in hparams.layers:
        name = f"{hparams.rewrite_module_tmp.format(layer)}.weight"
        if weights[name] is not nethook.get_parameter(pipe.text_encoder, name):
            raise ValueError(f"weights[{name!r}] is not the text encoder's live parameter")
    zs_t = zs.detach().t().contiguous().float().cpu()
    covs = {layer: get_cov_text_encoder(pipe.text_encoder, pipe.tokenizer, hparams.rewrite_module_tmp.format(layer),
                                        hparams.mom2_dataset, hparams.mom2_n_samples, hparams.mom2_dtype,
                                        stat_dir=stat_dir, verbose=verbose) for layer in hparams.layers}
    plan = prepare_encoder_edit(pipe.text_encoder, pipe.tokenizer, requests, hparams.layers, hparams.rewrite_module_tmp,
                                hparams.mom2_update_weight, hparams.edit_weight, zs_t, covs, _shard_from_env(shard),
                                layer_module_tmp=getattr(hparams, "layer_module_tmp", None))
    edits = run_checked(plan, keep_factors=True, restore=False)
    return _deltas_to_host(edits)


# ---- cross-attention K/V of the UNet (reference: :314-548) -------------------------------------------------------

def get_cov_cross_attn(pipe, layer_name: str, mom2_dataset: str, sample_size: int, mom2_dtype: str, inv: bool = False,
                       force_recompute: bool = False, verbose: bool = False, stats_dir=STATS_DIR) -> torch.Tensor:
    """Second moment of a cross-attention projection's input (the text embedding), fp32 on the UNet's device
    (reference: :2203-2236; its cache key ignores the statistics directory, this one includes it)."""
    model_name = pipe.unet.config._name_or_path.replace("/", "_")
    key = (model_name, layer_name, str(Path(stats_dir).resolve()), sample_size, mom2_dtype)
    device = next(pipe.unet.parameters()).device
    if verbose:
        print(f"Retrieving covariance statistics for {model_name} @ {layer_name}.")
    if key not in COV_CACHE or force_recompute:
        stat = layer_stats_cross_attn_kv(pipe, layer_name, stats_dir, mom2_dataset, to_collect=["mom2"],
                                         sample_size=sample_size, precision=mom2_dtype, force_recompute=force_recompute)
        COV_CACHE[key] = stat.mom2.moment().float().to("cpu")
        _COV_DEVICE_CACHE.pop((key, device), None)
    dkey = (key, device)
    if dkey not in _COV_DEVICE_CACHE:
        _COV_DEVICE_CACHE[dkey] = COV_CACHE[key].to(device)
    c = _COV_DEVICE_CACHE[dkey]
    return torch.inverse(c) if inv else c


def load_v_stars_cross_attn(requests: Sequence[Dict], cache_name: Optional[str], layer_names: Sequence[str],
                            stage1: Optional[Callable[[Dict], Dict[str, torch.Tensor]]] = None) -> Dict[str, torch.Tensor]:
    """{layer_name: (N, out) fp32 on the host}.  Cache: one npz per request, ``source_{source}.npz``, whose entries are
    pickled ``{"v_star": array}`` per layer name (reference: :373-391 read, :411-420 write)."""
    rows = {n: [] for n in layer_names}
    for idx, request in enumerate(requests):
        f = Path(cache_name + f"source_{request['source']}.npz") if cache_name is not None else None
        got = None
        if f is not None and f.exists():
            try:
                data = np.load(f, allow_pickle=True)
                got = {n: np.asarray(data[n].item()["v_star"], dtype=np.float32) for n in layer_names}
            except Exception as e:   # unreadable cache -> recompute, as the reference (:392-393)
                print(f"Error reading cache file due to {e}. Recomputing...")
        if got is None:
            if stage1 is None:
                raise NotImplementedError(
                    f"no cached cross-attention v* for request {idx} ([{request['source']}]) at {f} and no way to compute it: "
                    f"Stage 1 (compute_z_unet_x_kv) needs a pipeline with a UNet and a VAE — pass cache_name pointing at "
                    f"the reference's npz files or a stage1= callable")
            got = {n: v.detach().float().cpu().numpy() for n, v in stage1(request).items()}
            if f is not None:
                f.parent.mkdir(exist_ok=True, parents=True)
                np.savez(f, **{n: {"v_star": got[n]} for n in layer_names})
        for n in layer_names:
            rows[n].append(got[n])
    return {n: torch.from_numpy(np.stack(v, axis=0)) for n, v in rows.items()}


def _edit_cross_attn(pipe, requests, hparams, cache_name, stats_dir, keep_factors, restore, verbose, stage1):
    """Closed form for every cross-attention K/V projection.  Same keys for all of them (the text embedding at the last
    subject token), own targets, own statistics, residual NOT split over layers (:473).  Each projection is one
    ``emcid_edit_layer_f64`` call: d = text hidden size (768), N concepts, h = the block's channel count.

    One reference behaviour is NOT reproduced: ``apply_emcid_to_cross_attn`` forms ``adj_k @ resid^T`` (hidden x out) and
    relies on ``upd_matrix_match_shape`` to transpose it (:540-543); for a SQUARE projection the shape test passes
    untransposed and the reference adds U^T.  No Stable Diffusion UNet has channels == text hidden size (768 vs
    320/640/1280; 2048 vs 640/1280 for SDXL); here such a projection gets the intended U."""
    names = get_all_cross_attn_kv_layer_names(pipe)
    weights = {n: nethook.get_parameter(pipe.unet, f"{n}.weight") for n in names}
    device = next(pipe.unet.parameters()).device
    for n, w in weights.items():
        if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous()):
            raise hip.EmcidHipError(f"{n}.weight must be a contiguous fp32 tensor in HBM (got {w.dtype} on {w.device})")
    if stage1 is None and getattr(pipe, "unet", None) is not None and getattr(pipe, "vae", None) is not None:
        # a v* miss runs Stage 1 of this sibling on the caller's UNet / VAE, like the reference (:398)
        from .compute_z import compute_z_unet_x_kv
        device = next(pipe.unet.parameters()).device
        stage1 = lambda request: compute_z_unet_x_kv(pipe, request, hparams, device)
    zs = load_v_stars_cross_attn(requests, cache_name, names, stage1)
    covs = {n: get_cov_cross_attn(pipe, n, hparams.mom2_dataset, hparams.mom2_n_samples, hparams.mom2_dtype,
                                  verbose=verbose, stats_dir=stats_dir) for n in names}
    ks, cur = get_layers_input_output_at_words_cross_attn(pipe, requests, names,
                                                          layer_module_tmp=getattr(hparams, "layer_module_tmp", None))
    out, infos = {}, []
    # The keys are the same for every projection, and so is the system matrix lam*C' + K K^T whenever two projections
    # share their statistics (they all see the same text embeddings: the reference's files differ in name only).  Such
    # projections share ONE assembly + factorization + solve (adj_k); each then costs its residual and one dW GEMM.
    groups: List[Tuple[torch.Tensor, List[str]]] = []
    for n in names:
        for rep, members in groups:
            if rep is covs[n] or (rep.shape == covs[n].shape and torch.equal(rep, covs[n])):
                members.append(n)
                break
        else:
            groups.append((covs[n], [n]))
    s_ = (hparams.edit_weight / 0.5) ** 0.5
    for cov, members in groups:
        lead = members[0]
        w = weights[lead]
        K = ks[lead].contiguous()
        w0 = w.detach().clone()
        if verbose:
            print(f"Writing {K.shape[0]} key/value pair(s) into layer {lead}")
        res = hip.edit_layer(K, cur[lead].contiguous(), zs[lead].to(device).contiguous(), cov, hparams.mom2_update_weight,
                             hparams.edit_weight, 1, W0=w0, W=w.data, want_factors=True, want_dw=False)
        infos.append(res["ws"].info)
        Xt = res["Xt"]                                             # (N, hidden) f64 = adj_k^T, shared by the group
        adj_k_host = Xt.t().contiguous().cpu() if keep_factors else None
        if keep_factors:
            out[f"{lead}.weight"] = (adj_k_host, res["Rt"].t().contiguous().cpu())
        if restore:
            w.data.copy_(w0)
        for n in members[1:]:
            w = weights[n]
            if verbose:
                print(f"Writing {K.shape[0]} key/value pair(s) into layer {n}")
            # resid^T = double(zs - Zc) * sqrt(e_w / 0.5)  (fp32 difference first, as :440 and :466)
            Rt = ((zs[n].to(device) - cur[n]).double() * s_).contiguous()
            if keep_factors:
                out[f"{n}.weight"] = (adj_k_host, Rt.t().contiguous().cpu())
            if not restore:
                hip.delta_w_(Rt, Xt, w.detach().clone(), w.data)
    out = {f"{n}.weight": out[f"{n}.weight"] for n in names if f"{n}.weight" in out}     # reference key order
    code = int(torch.stack(infos).max().item()) if infos else 0
    if code != 0:
        raise FloatingPointError(f"lam*C + K K^T is not positive definite (non-positive pivot at column {code - 1})")
    return names, out


def execute_emcid_cross_attn(pipe, requests: List[Dict], hparams: EMCIDHyperParams, cache_name: Optional[str] = None,
                             mom2_weight: Optional[int] = None, edit_weight: Optional[float] = None, verbose: bool = True,
                             stats_dir=STATS_DIR, stage1=None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """{weight_name: (adj_k (hidden, N) f64 cpu, resid (out, N) f64 cpu)}; the UNet is unchanged on return (:314-508)."""
    hparams.mom2_update_weight = mom2_weight if mom2_weight is not None else hparams.mom2_update_weight
    hparams.edit_weight = edit_weight if edit_weight is not None else hparams.edit_weight
    requests = deepcopy(requests)
    if verbose:
        for request in requests:
            print(f"EMCID request sample: [{request['source']}] -> [{request['dest']}]" if "dest" in request
                  else f"EMCID request sample: erasing [{request['source']}]")
    names, deltas = _edit_cross_attn(pipe, requests, hparams, cache_name, stats_dir, True, True, verbose, stage1)
    if verbose:
        print(f"Deltas successfully computed for {[f'{n}.weight' for n in names]}")
    return deltas


def apply_emcid_to_cross_attn(pipe, requests: List[Dict], hparams: EMCIDHyperParams, device: str,
                              mom2_weight: Optional[int] = None, edit_weight: Optional[float] = None,
                              return_orig_text_model=False, cache_name: Optional[str] = None, stats_dir=STATS_DIR,
                              verbose: bool = True, stage1=None):
    """Returns (pipe with the edited UNet projections, the original UNet or None) (:511-548)."""
    orig_unet = deepcopy(pipe.unet) if return_orig_text_model else None
    hparams.mom2_update_weight = mom2_weight if mom2_weight is not None else hparams.mom2_update_weight
    hparams.edit_weight = edit_weight if edit_weight is not None else hparams.edit_weight
    requests = deepcopy(requests)
    # each projection is left at W0 + float(U): what the reference reaches by restoring W0 and adding
    # float(adj_k @ resid^T) (:538-545)
    names, _ = _edit_cross_attn(pipe, requests, hparams, cache_name, stats_dir, False, False, verbose, stage1)
    if verbose:
        print(f"New weights successfully inserted into {[f'{n}.weight' for n in names]}")
    return pipe, orig_unet


# ---- SDXL ----------------------------------------------------------------------------------------------

def _sdxl_overrides(hparams, mom2_weight, mom2_weight_2, edit_weight):
    hparams.mom2_update_weight = mom2_weight if mom2_weight is not None else hparams.mom2_update_weight
    hparams.mom2_update_weight_2 = mom2_weight_2 if mom2_weight_2 is not None else hparams.mom2_update_weight_2
    hparams.edit_weight = edit_weight if edit_weight is not None else hparams.edit_weight


SDXL_TE1_COST_SHARE = 0.14     # TE1 alone 16 ms, TE2 alone 102 ms per 1 000 concepts on one MI355X: share of the ranks TE1 gets
_SDXL_GROUPS: Dict[tuple, tuple] = {}


def sdxl_rank_split(rank: int, world: int):
    """(encoder this rank edits, its rank inside that encoder's group, group sizes (g1, g2)).  The two SDXL text encoders
    are independent models (reference :1233-1320 vs :1333-1422): TE1 goes to the first g1 ranks, TE2 to the rest, in
    proportion to their cost (at least one rank each)."""
    g1 = max(1, min(world - 1, int(round(world * SDXL_TE1_COST_SHARE))))
    return (1, rank, (g1, world - g1)) if rank < g1 else (2, rank - g1, (g1, world - g1))


def _sdxl_split(shard: ConceptShard):
    """Process groups of the TE1 / TE2 rank split, or None when the split does not apply (one rank, a caller-supplied
    group, or EMCID_SDXL_SPLIT=0: then both encoders are edited on every rank, concept-sharded, on two streams)."""
    import torch.distributed as dist
    if shard.world < 2 or shard.group is not None or os.environ.get("EMCID_SDXL_SPLIT", "1") == "0":
        return None
    which, sub_rank, (g1, g2) = sdxl_rank_split(shard.rank, shard.world)
    key = (shard.world, g1)
    if key not in _SDXL_GROUPS:       # collective: every rank creates both groups, in the same order
        _SDXL_GROUPS[key] = (dist.new_group(list(range(g1))), dist.new_group(list(range(g1, shard.world))))
    grp = _SDXL_GROUPS[key][which - 1]
    return {"which": which, "shard": ConceptShard(sub_rank, g1 if which == 1 else g2, grp), "roots": (0, g1)}


def _axpy_weight_(w: torch.Tensor, dW: torch.Tensor):
    """``w += dW`` on an encoder weight (the kernel writes through the raw pointer) with the in-place version counter of the
    PARAMETER bumped: the caches derived from a weight (split-fp16 planes, native layer structs) follow that counter, and a
    write through ``w.data`` alone leaves it where it was (``.data`` has a counter of its own)."""
    hip.axpy_(w.data, dW)
    edit_engine._touch(w)


def _broadcast_(t: torch.Tensor, src: int):
    """In-place broadcast over the default group (RCCL on device buffers; gloo stages HBM tensors through the host).  ``t`` may
    be a Parameter: the bytes go through ``t.data`` and the parameter's version counter is bumped (see ``_axpy_weight_``)."""
    import torch.distributed as dist
    raw = t.data
    if raw.is_cuda and dist.get_backend() == "gloo":
        host = raw.cpu()
        dist.broadcast(host, src=src)
        raw.copy_(host)
    else:
        dist.broadcast(raw, src=src)
    edit_engine._touch(t)


def _sdxl_plans(pipe, requests, hparams, cache_name, stat_dir, stat_dir_2, verbose, shard, stage1):
    if hparams.num_edit_tokens != 1:
        raise AssertionError("num_edit_tokens should be 1")   # reference :1246
    p1 = prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, requests, hparams, hparams.layers,
                                   hparams.mom2_update_weight, stat_dir, cache_name, "", verbose, shard, stage1)
    p2 = prepare_text_encoder_edit(pipe.text_encoder_2, pipe.tokenizer_2, requests, hparams, hparams.layers_2,
                                   hparams.mom2_update_weight_2, stat_dir_2, cache_name, "_2", verbose, shard, stage1)
    return p1, p2


@_retry_if_stale
def execute_emcid_sd_xl_text_encoders(pipe, requests: List[Dict], hparams: EMCIDXLHyperParams,
                                      cache_name: Optional[str] = None, mom2_weight: Optional[int] = None,
                                      mom2_weight_2: Optional[int] = None, edit_weight: Optional[float] = None,
                                      verbose: bool = True, stat_dir="data/stats/sdxl/text1",
                                      stat_dir_2="data/stats/sdxl/text2", shard=None, stage1=None):
    """(deltas, deltas_2).  TE1 is restored; TE2 is left at W + dW exactly as the reference leaves it (:1410)."""
    _sdxl_overrides(hparams, mom2_weight, mom2_weight_2, edit_weight)
    _announce(requests, verbose)
    stage1 = _default_stage1_sdxl(pipe, hparams, stage1)
    p1, p2 = _sdxl_plans(pipe, requests, hparams, cache_name, stat_dir, stat_dir_2, verbose, shard, stage1)
    e1 = run_checked(p1, keep_factors=True, restore=True)
    e2 = run_checked(p2, keep_factors=True, restore=not SDXL_TE2_DOUBLE_APPLY)
    return _deltas_to_host(e1), _deltas_to_host(e2)


@_retry_if_stale
def apply_emcid_to_sdxl_text_encoders(pipe, requests: List[Dict], hparams: EMCIDXLHyperParams, device: str,
                                      mom2_weight: Optional[int] = None, mom2_weight_2: Optional[int] = None,
                                      edit_weight: Optional[float] = None, return_orig_text_encoder=False,
                                      cache_name: Optional[str] = None, stat_dir=XL_STATS_DIR1,
                                      stat_dir_2=XL_STATS_DIR2, verbose: bool = True, shard=None, stage1=None):
    """Returns (pipe, original text_encoder | None, original text_encoder_2 | None)."""
    o1 = deepcopy(pipe.text_encoder) if return_orig_text_encoder else None
    o2 = deepcopy(pipe.text_encoder_2) if return_orig_text_encoder else None
    _sdxl_overrides(hparams, mom2_weight, mom2_weight_2, edit_weight)
    _announce(requests, verbose)
    stage1 = _default_stage1_sdxl(pipe, hparams, stage1)
    split = _sdxl_split(_shard_from_env(shard))
    if split is not None:
        # TE1 || TE2 on disjoint GPU groups (BASELINE config 4): this rank edits ONE encoder, concept-sharded
        # inside its group, then the groups' roots broadcast the edited fc2 weights so every rank ends with the whole pipe
        if hparams.num_edit_tokens != 1:
            raise AssertionError("num_edit_tokens should be 1")   # reference :1246
        stale = None
        try:
            if split["which"] == 1:
                plan = prepare_text_encoder_edit(pipe.text_encoder, pipe.tokenizer, requests, hparams, hparams.layers,
                                                 hparams.mom2_update_weight, stat_dir, cache_name, "", verbose, split["shard"], stage1)
                run_checked(plan, keep_factors=False, restore=False)
            else:
                plan = prepare_text_encoder_edit(pipe.text_encoder_2, pipe.tokenizer_2, requests, hparams, hparams.layers_2,
                                                 hparams.mom2_update_weight_2, stat_dir_2, cache_name, "_2", verbose, split["shard"], stage1)
                edits = run_checked(plan, keep_factors=False, restore=False)
                if SDXL_TE2_DOUBLE_APPLY:   # execute left TE2 edited, apply adds the update once more (:93-99)
                    for e in edits:
                        _axpy_weight_(nethook.get_parameter(pipe.text_encoder_2, e.weight_name), e.dW)
        except clip_forward.StaleWeightCacheError as e:
            stale = e              # (this group's weights are back: every rank of a group reads the same flag)
        # one group's stale caches must not leave the other group waiting in the broadcasts below: every rank learns of it
        if _any_rank(stale is not None, next(pipe.text_encoder.parameters()).device):
            if stale is None:      # the sound group's encoder is edited (TE2 sits at W + 2 dW): put it back before everybody raises
                plan.restore_weights()
            raise stale if stale is not None else clip_forward.StaleWeightCacheError(
                "the other encoder's rank group ran on stale weight caches; this group's weights were restored")
        names = []
        for enc, layers, root in ((pipe.text_encoder, hparams.layers, split["roots"][0]),
                                  (pipe.text_encoder_2, hparams.layers_2, split["roots"][1])):
            for layer in layers:
                name = f"{hparams.rewrite_module_tmp.format(layer)}.weight"
                _broadcast_(nethook.get_parameter(enc, name), root)
                names.append(name)
        if verbose:
            print(f"New weights successfully inserted into {names}")
        return pipe, o1, o2
    p1, p2 = _sdxl_plans(pipe, requests, hparams, cache_name, stat_dir, stat_dir_2, verbose, shard, stage1)
    # The two encoders are independent models (:1233 vs :1333): two HIP streams on one GPU.  Measured for the 1 000-concept edit (scripts/bench_sdxl.py): 83.0 ms against 84.9 ms per apply call — TE2's
    # 26-layer prefix forward is 3/4 of the call and leaves little for TE1 to hide under.  With more ranks the encoders go to
    # disjoint rank groups instead (_sdxl_split above).
    dev2 = next(pipe.text_encoder_2.parameters()).device      # (v* may still be a pending upload: plan.zs_t is set lazily)
    two_streams = True
    s2 = torch.cuda.Stream(device=dev2) if two_streams else torch.cuda.current_stream(dev2)
    if two_streams:
        s2.wait_stream(torch.cuda.current_stream(dev2))
    e1 = run_encoder_edit(p1, keep_factors=False, restore=False)
    with torch.cuda.stream(s2):
        e2 = run_encoder_edit(p2, keep_factors=False, restore=False)
        if SDXL_TE2_DOUBLE_APPLY:   # execute left TE2 edited, apply adds the update once more (:93-99)
            for e in e2:
                _axpy_weight_(nethook.get_parameter(pipe.text_encoder_2, e.weight_name), e.dW)
    if two_streams:
        torch.cuda.current_stream(dev2).wait_stream(s2)

    def double_apply(edits):
        for e in edits:
            _axpy_weight_(nethook.get_parameter(pipe.text_encoder_2, e.weight_name), e.dW)

    stale = None
    for plan, redo in ((p1, None), (p2, double_apply if SDXL_TE2_DOUBLE_APPLY else None)):
        try:
            try:
                check_info(plan)                   # restores the encoder's weights if a factorization failed
            except FloatingPointError as err:
                again = rerun_with_lu(plan, err)   # the reference's own solver semantics, as run_checked
                if redo is not None:
                    redo(again)
        except clip_forward.StaleWeightCacheError as e:
            stale = e                              # (this encoder's weights are back; the other one's follow below)
    if stale is not None:      # one encoder ran on stale planes: put BOTH back (TE2 sits at W + 2 dW) and let the call be redone
        p1.restore_weights()
        p2.restore_weights()
        raise stale
    if verbose:
        print(f"New weights successfully inserted into {[e.weight_name for e in e1 + e2]}")
    return pipe, o1, o2


def sweep_emcid_sdxl_text_encoders(pipe, requests: List[Dict], hparams: EMCIDXLHyperParams, grid, device: Optional[str] = None,
                                   visit=None, score=None, cache_name: Optional[str] = None, stat_dir=XL_STATS_DIR1,
                                   stat_dir_2=XL_STATS_DIR2, shard=None, stage1=None, verbose: bool = False) -> list:
    """One request set at every (mom2_weight, mom2_weight_2, edit_weight) triple of ``grid`` on the SDXL PAIR of text encoders, in
    ONE call: ``sweep_emcid_text_encoder`` for the pair.  At a triple TE1 holds W + dW(mom2_weight, edit_weight) and TE2 holds what
    ``apply_emcid_to_sdxl_text_encoders`` leaves, W + 2 dW(mom2_weight_2, edit_weight) while ``SDXL_TE2_DOUBLE_APPLY`` holds (W + dW
    otherwise).  The preparation is a call's (``_sdxl_plans``: tokenization, tries, the unedited leading layers, the v* reads, Stage
    1 on a cache miss), made once; each encoder's statistics are factored once (``edit_engine.SweepWalk``); ``hparams`` is NOT
    mutated; on return — also when ``visit`` raises — both encoders hold their original weights.  Invalid grids raise ValueError
    first (``edit_engine.validate_pair_grid``).

    The two encoders are independent models: TE1's weights and everything read of them depend on (mom2_weight, edit_weight) alone,
    TE2's on (mom2_weight_2, edit_weight); only the pair drift couples them, and it is a function of the per-node sums each
    encoder's readout leaves (``PairEditScorer``).  ``edit_engine.pair_grid_plan`` gives the distinct points of each encoder.

    ``score=[holdout prompt strings]`` with ``visit=None`` — the factorised path: a ``PairEditScorer`` is built once on the two
    prepared plans (nothing is tokenized, read or run twice), TE1 is walked over ITS distinct points and TE2 over its own — a 4 x 4
    cross of the two mom2 weights at one edit_weight is 4 + 4 encoder edits and replays, not 2 x 16 —, each point's half of a
    score runs into its slot of a bank of node sums, then ONE ``hip.score_chains_pair_grid`` launch reduces every triple's pair
    drift and ONE pinned read brings everything to the host (``PairEditScorer.score_points``).  The result is one ``PairEditScore``
    per triple, in grid order; ``select_point`` takes the list.

    With a ``visit`` — the joint path: the triples are walked in grid order and ``visit(triple, pipe)`` is called while BOTH
    encoders hold the triple's weights; an encoder whose own point equals the previous triple's is not edited again.  The result
    per triple is ``visit``'s return value, or ``(visit(...), PairEditScore)`` with ``score=``.  ``visit=None, score=None``
    collects ``({weight name: edited fc2 weight of TE1}, {the same of TE2})``, fp32 on the host, per triple.

    A point whose Cholesky reports a non-positive pivot is rerun alone on the pivoted LU (TE2's second apply then adds the rerun's
    own dW).  A stale-cache verdict (``_retry_if_stale``) puts both encoders back and redoes the sweep once from its first point.
    Refused before anything is launched: what ``PairEditScorer`` and ``_sdxl_plans`` refuse; ``score=`` on a collective shard
    (``ValueError``) or on an encoder the prefix-trie forward does not take (``UnsupportedEncoder``).  Without ``score=`` such an
    encoder gets one ordinary call per triple (counted by ``clip_forward.note_fallback``).

    LAST_PATHS gauges of the last sweep: sweep_pair_points_1, sweep_pair_points_2 (encoder edits run; on the fallback one per
    triple each), sweep_pair_combos (triples), and ``run_sweep``'s own, summed over both encoders.  Unlike every other gauge the
    three ``sweep_pair_*`` keys are NOT always in ``LAST_PATHS``: they are set by this function and taken out again by the next
    ``sweep_emcid_text_encoder`` (``edit_engine.run_sweep``), whose gauges are all the ``sweep_*`` keys of the last sweep — read
    them with ``LAST_PATHS.get(key)`` unless a pair sweep has just run.

    ``PairEditScorer.score_points`` allocates its output buffer, its pinned host buffer and the two banks of node sums per call
    (their sizes follow the grid, not the scorer); ``score()`` keeps its own preallocated pair."""
    import contextlib
    from .edit_engine import SweepWalk, pair_grid_plan, validate_pair_grid
    triples = validate_pair_grid(grid)
    if not isinstance(hparams, EMCIDXLHyperParams):
        raise TypeError(f"hparams must be EMCIDXLHyperParams, got {type(hparams).__name__}")
    if getattr(pipe, "text_encoder_2", None) is None or getattr(pipe, "tokenizer_2", None) is None:
        raise ValueError("sweep_emcid_sdxl_text_encoders sweeps the SDXL pair: the pipe has no text_encoder_2 / tokenizer_2")
    hp = deepcopy(hparams)
    hp.mom2_update_weight, hp.mom2_update_weight_2, hp.edit_weight = triples[0]
    if hp.num_edit_tokens != 1:
        raise AssertionError("num_edit_tokens should be 1")   # (as _sdxl_plans, reference :1246)
    for te in (pipe.text_encoder, pipe.text_encoder_2):
        if device is not None and torch.device(device) != next(te.parameters()).device:
            raise ValueError(f"a text encoder is on {next(te.parameters()).device}, not on {device}")
    pts = pair_grid_plan(triples)
    checked = None
    if score is not None:       # every host-side refusal of a scorer, before the preparation launches anything
        if _shard_from_env(shard).collective:
            raise ValueError("score= runs on one rank: a collective ConceptShard is not supported")
        score = list(score)
        if not score or not all(isinstance(p, str) for p in score):
            raise ValueError("score= takes the holdout: a non-empty list of prompt strings")
        checked = PairEditScorer._host_checks(pipe, requests, hp, device, score, shard)
    names = [[f"{hp.rewrite_module_tmp.format(l)}.weight" for l in layers] for layers in (hp.layers, hp.layers_2)]
    encoders = (pipe.text_encoder, pipe.text_encoder_2)
    LP = clip_forward.LAST_PATHS
    scorer = None

    def second_apply(edits):
        if SDXL_TE2_DOUBLE_APPLY:   # execute left TE2 edited, apply adds the update once more (:93-99)
            for e in edits:
                _axpy_weight_(nethook.get_parameter(pipe.text_encoder_2, e.weight_name), e.dW)

    def collect(triple):
        if scorer is not None:
            return (visit(triple, pipe), scorer.score())
        if visit is not None:
            return visit(triple, pipe)
        return tuple({n: nethook.get_parameter(te, n).detach().to("cpu", torch.float32).clone() for n in ns}
                     for te, ns in zip(encoders, names))

    _announce(requests, verbose)
    stage1 = _default_stage1_sdxl(pipe, hp, stage1)
    for attempt in (0, 1):
        plans = _sdxl_plans(pipe, requests, hp, cache_name, stat_dir, stat_dir_2, verbose, shard, stage1)
        if any(p.chunk is None or p.graph is None for p in plans):
            if score is not None:
                raise clip_forward.UnsupportedEncoder("score= needs the prefix-trie forward, which an encoder or the request set did not take")
            break
        LP["sweep_points"] = LP["sweep_cov_factorizations"] = LP["sweep_prefix_runs"] = 0
        LP["sweep_pair_points_1"] = LP["sweep_pair_points_2"] = 0
        LP["sweep_pair_combos"] = len(triples)
        try:
            if score is not None:
                # on the sweep's own plans, before the first point, on the original weights; again after a stale-cache retry
                scorer = PairEditScorer(pipe, requests, hp, device, holdout=score, cache_name=cache_name, shard=shard, _plans=plans,
                                        _checked=checked)
            with SweepWalk(plans[0]) as w1, SweepWalk(plans[1]) as w2:
                walks = (w1, w2)

                def put(i, point):
                    edits = walks[i].point(*point)
                    if i == 1:
                        second_apply(edits)
                    LP[f"sweep_pair_points_{i + 1}"] += 1

                if scorer is not None and visit is None:
                    @contextlib.contextmanager
                    def place(i, g):
                        put(i, pts[i][g])
                        try:
                            yield
                        finally:
                            plans[i].restore_weights()

                    return scorer.score_points(len(pts[0]), len(pts[1]), pts[2], place)
                results, held = [], [None, None]
                for triple, combo in zip(triples, pts[2]):
                    for i in (0, 1):
                        if held[i] != combo[i]:       # (an encoder whose own point is the previous triple's stays as it is)
                            if held[i] is not None:
                                plans[i].restore_weights()
                            held[i] = None
                            put(i, pts[i][combo[i]])
                            held[i] = combo[i]
                    results.append(collect(triple))
                return results
        except clip_forward.StaleWeightCacheError as e:
            # (as _retry_if_stale: the engine put the stale encoder's weights back, the walks' exit the other's; a multi-rank job raises)
            import torch.distributed as dist
            if attempt or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
                raise
            _note_stale("sweep_emcid_sdxl_text_encoders", e, "sweep")
            if score is not None:       # (the dropped caches took the encoders' graphs with them: the scorer's checks name the new ones)
                checked = PairEditScorer._host_checks(pipe, requests, hp, device, score, shard)
    # the hooked-HF forward has no stored state to replay: one ordinary call per triple, both encoders restored after each
    clip_forward.note_fallback("sweep_emcid_sdxl_text_encoders", clip_forward.UnsupportedEncoder("no prefix-trie forward: one call per triple"))
    LP["sweep_pair_points_1"] = LP["sweep_pair_points_2"] = LP["sweep_pair_combos"] = len(triples)      # (every triple edits both)
    results = []
    for index, triple in enumerate(triples):
        if index:         # (the plans prepared above are the first triple's)
            hp_i = deepcopy(hparams)
            hp_i.mom2_update_weight, hp_i.mom2_update_weight_2, hp_i.edit_weight = triple
            plans = _sdxl_plans(pipe, requests, hp_i, cache_name, stat_dir, stat_dir_2, verbose, shard, stage1)
        try:
            run_checked(plans[0], keep_factors=False, restore=False)
            second_apply(run_checked(plans[1], keep_factors=False, restore=False))
            results.append(collect(triple))
        finally:
            plans[0].restore_weights()
            plans[1].restore_weights()
    return results


# ---- edited-weight export (the reference never saves its edits) --------------------------------

def export_edited_weights(text_encoder, hparams, path, layers: Optional[Sequence[int]] = None) -> List[str]:
    """Write the (edited) fc2 weights of ``layers`` (default ``hparams.layers``) to a safetensors file keyed by
    the parameter names of ``hparams.rewrite_module_tmp``; returns the names written."""
    from safetensors.torch import save_file
    layers = list(hparams.layers if layers is None else layers)
    names = [f"{hparams.rewrite_module_tmp.format(l)}.weight" for l in layers]
    tensors = {n: nethook.get_parameter(text_encoder, n).detach().to("cpu").contiguous() for n in names}
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    save_file(tensors, str(path), metadata={"format": "pt", "producer": "emcid_amd"})
    return names


def load_edited_weights(text_encoder, path) -> List[str]:
    """Copy the tensors of an ``export_edited_weights`` file into the encoder (shape-checked, in place)."""
    from safetensors.torch import load_file
    tensors = load_file(str(path))
    with torch.no_grad():
        for n, t in tensors.items():
            w = nethook.get_parameter(text_encoder, n)
            if w.shape != t.shape:
                raise ValueError(f"{n}: file has {tuple(t.shape)}, model has {tuple(w.shape)}")
            w.copy_(t.to(w.device, w.dtype))
    return list(tensors)


def apply_emcid_to_model(pipe, requests, hparams, device, **kwargs):
    """Dispatching alias (the entry-point name used by BASELINE.json; absent from the reference)."""
    if isinstance(hparams, EMCIDXLHyperParams) or hasattr(hparams, "layers_2"):
        return apply_emcid_to_sdxl_text_encoders(pipe, requests, hparams, device, **kwargs)
    return apply_emcid_to_text_encoder(pipe, requests, hparams, device, **kwargs)

"""Shared helpers of the EditSession tests.  For the end-to-end ones (tests/test_session_gpu.py, _fold_gpu, _retain_gpu,
_release_gpu): the toy encoder's fixture recipe with cached v* files, the fp64 recomputation of a step from the primal system on
the CPU, and a checked ``sess.apply``.  For the ones without a GPU (tests/test_session*_cpu.py): ``_hp`` and the ``pipe`` fixture.
A plain module, imported by name like tests/gemm_f64_oracle.py."""
import numpy as np
import pytest
import torch

import emcid_amd
from emcid_amd import edit_engine as ee, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter
from oracle import emcid_oracle as orc

DEV = "cuda:0"
BAR = 1e-4          # the project's end-to-end bar: err <= 1e-4 max|dW| (tests/test_e2e_gpu.py, __graft_entry__.smoke)
LAYERS = (1, 2, 3, 4)


def _hp(**kw):
    d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=50, edit_weight=0.6, mom2_n_samples=1000)
    d.update(kw)
    return EMCIDHyperParams(**d)


@pytest.fixture(scope="module")
def pipe():
    return syn.build_pipe("toy", "cpu")


def fresh_caches(engine=False):
    """An autouse fixture for a test module (assign it to a module-level name): the weight-derived caches — ``engine``: and the
    engine's factor cache — dropped before and after every test."""
    def clear():
        em.clear_caches()
        if engine:
            ee.clear_engine_caches()

    @pytest.fixture(autouse=True)
    def _fresh_caches():
        clear()
        yield
        clear()
    return _fresh_caches


def _setup(tmp_path, n_req=12, k=1):
    reqs = syn.make_requests(n_req, ragged=True)
    hp_d = syn.sd_hparams_dict(layers=LAYERS, mom2_update_weight=50, edit_weight=0.6, mom2_n_samples=1000)
    if k > 1:
        hp_d.update(num_edit_tokens=k, use_new_compute_z=True)
    names = [hp_d["rewrite_module_tmp"].format(l) for l in hp_d["layers"]]
    cache, stats = str(tmp_path / "cache") + "/", str(tmp_path / "stats")
    if k > 1:
        rng = np.random.default_rng(1)
        for r in reqs:
            p = syn.vstar_cache_path(cache, r)
            p.parent.mkdir(parents=True, exist_ok=True)
            np.savez(p, v_star=(rng.standard_normal((k, 32)) * 0.5).astype(np.float32))
    else:
        syn.write_vstar_cache(cache, reqs, 32, seed=1, scale=0.5)
    syn.write_stats_cache(stats, names, 128, 1000, seed=2, t=512)
    return reqs, hp_d, names, cache, stats


def _held(reqs):
    """What a retain request needs: the prompts and the subject."""
    return [{"source": r["source"], "prompts": list(r["prompts"])} for r in reqs]


def _weights(te, names):
    return {n: get_parameter(te, n + ".weight").detach().cpu().double() for n in names}


def _cpu_twin(gpu_te):
    cpu = syn.build_pipe("toy", "cpu")
    cpu.text_encoder.load_state_dict({n: v.detach().cpu() for n, v in gpu_te.state_dict().items()})
    return cpu.text_encoder, cpu.tokenizer


def _keys(gpu_te, reqs, names, k=1):
    """{name: (N k, d) f64}: the mean fc2 inputs at the requests' lookup rows, hooked CPU forward on the weights as they are now."""
    te, tok = _cpu_twin(gpu_te)
    out = {}
    with torch.no_grad():
        for n in names:
            K = orc.module_input_output_at_words_multi(te, tok, reqs, n, k)[0] if k > 1 else orc.module_input_output_at_words(te, tok, reqs, n)[0]
            out[n] = K.reshape(-1, K.shape[-1]).double()
    return out


def _seed(P, keys, weight, hp_d):
    """The retained rows of the primal system: sqrt(weight) s K_held."""
    s = (float(hp_d["edit_weight"]) / 0.5) ** 0.5
    for n, K in keys.items():
        P.setdefault(n, []).append(weight ** 0.5 * s * K)


def _primal_step(gpu_te, reqs, hp_d, names, cache, stats, P, k=1):
    """One step recomputed in fp64 from the primal system, layer by layer, on a CPU copy of the encoder AS IT IS NOW: the keys of
    every edited layer come from a hooked forward on the current weights (the earlier layers of this step already updated);
    A = lam C' + sum_{P} P^T P + Kt^T Kt with EVERY earlier step's keys (folded or not) and every retained row in ``P``.  Appends
    this step's Kt to ``P``; returns ({name: dW f64}, {name: Rt f64 (N k, h)}, {name: Kt f64}, {name: K f64})."""
    te, tok = _cpu_twin(gpu_te)
    lam, e, L = float(hp_d["mom2_update_weight"]), float(hp_d["edit_weight"]), len(names)
    zs = orc.load_vstars(cache, reqs, use_new_compute_z=k > 1)          # (h, N k)
    s = (e / 0.5) ** 0.5
    dws, rts, kts, keys = {}, {}, {}, {}
    with torch.no_grad():
        for i, n in enumerate(names):
            if k > 1:
                K, Zc = orc.module_input_output_at_words_multi(te, tok, reqs, n, k)
                K, Zc = K.reshape(-1, K.shape[-1]), Zc.reshape(-1, Zc.shape[-1])
            else:
                K, Zc = orc.module_input_output_at_words(te, tok, reqs, n)
            C = orc.load_cov(stats, n, hp_d["mom2_n_samples"], hp_d["mom2_dtype"])
            Cp = (C * (1 - e) / 0.5).double()
            Kt, Rt = s * K.double(), (s * (zs.t() - Zc).double()) / (L - i)
            A = lam * Cp + Kt.t() @ Kt
            for Pk in P.setdefault(n, []):
                A = A + Pk.t() @ Pk
            upd = torch.linalg.solve(A, Kt.t() @ Rt).t()
            w = orc.get_parameter(te, n + ".weight")
            w[...] = w + upd.float()
            P[n].append(Kt)
            dws[n], rts[n], kts[n], keys[n] = upd, Rt, Kt, K.double()
    return dws, rts, kts, keys


def _apply_checked(sess, pipe, step, fx, P, k=1, what=""):
    """sess.apply(step) against the primal recomputation at the bar; returns (GPU dW, reference dW, Rt, Kt) per name."""
    reqs, hp_d, names, cache, stats = fx
    ref, rts, kts, _ = _primal_step(pipe.text_encoder, step, hp_d, names, cache, stats, P, k)
    before = _weights(pipe.text_encoder, names)
    sess.apply(step, cache_name=cache)
    after = _weights(pipe.text_encoder, names)
    got = {n: after[n] - before[n] for n in names}
    for n in names:
        err = (got[n] - ref[n]).abs().max().item()
        print(f"{what} {n}: err {err:.3e} max|dW| {ref[n].abs().max().item():.3e}")
        assert err < BAR and err <= BAR * ref[n].abs().max().item(), (what, n, err)
    return got, ref, rts, kts


def _session(fx, **kw):
    pipe = syn.build_pipe("toy", DEV)
    return pipe, emcid_amd.EditSession(pipe, EMCIDHyperParams(**fx[1]), DEV, stats_dir=fx[4], **kw)


def _ratios(dw1, dw2, keys1, names):
    """per layer and key of step 1: ||dW2 k|| / ||dW1 k||"""
    return {n: (dw2[n] @ keys1[n].t()).norm(dim=0) / (dw1[n] @ keys1[n].t()).norm(dim=0) for n in names}

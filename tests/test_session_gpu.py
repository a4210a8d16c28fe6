"""EditSession end to end on the toy encoder with cached v* files: a step against apply_emcid_to_text_encoder, several steps
against an fp64 recomputation of the primal system lam C' + sum P^T P + Kt^T Kt on the CPU, what a session preserves that plain
calls do not, and its bookkeeping.  Run on the MI355X box:  python -m pytest tests/test_session_gpu.py -m gpu -q"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import emcid_amd
from emcid_amd import clip_forward as cf, edit_engine as ee, emcid_main as em, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from emcid_amd.nethook import get_parameter
from session_helpers import BAR, DEV, _primal_step, _ratios, _setup, _weights, fresh_caches

_fresh_caches = fresh_caches()


def _session_steps(tmp_path, sizes, k=1, capacity=None):
    """A session over disjoint request sets of the given sizes; every step checked against the primal recomputation at the bar.
    Returns (per-step {name: dW f64 from the GPU weights}, per-step reference dW, per-step keys, session, pipe, fixture)."""
    fx = _setup(tmp_path, sum(sizes), k)
    reqs, hp_d, names, cache, stats = fx
    pipe = syn.build_pipe("toy", DEV)
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, capacity=capacity)
    P, got, ref, keys, lo = {}, [], [], [], 0
    for t, n in enumerate(sizes):
        step = reqs[lo:lo + n]
        r, _, _, kk = _primal_step(pipe.text_encoder, step, hp_d, names, cache, stats, P, k)
        before = _weights(pipe.text_encoder, names)
        out = sess.apply(step, cache_name=cache)
        assert out[0] is pipe and out[1] is None
        after = _weights(pipe.text_encoder, names)
        g = {m: after[m] - before[m] for m in names}
        for m in names:
            err = (g[m] - r[m]).abs().max().item()
            print(f"k={k} step {t} (M={lo * k}, N={n * k}) {m}: err {err:.3e} max|dW| {r[m].abs().max().item():.3e}")
            assert err < BAR and err <= BAR * r[m].abs().max().item(), (t, m, err)
        got.append(g), ref.append(r), keys.append(kk)
        lo += n
        assert sess.preserved == lo * k and cf.LAST_PATHS["session_steps"] == t + 1
        assert cf.LAST_PATHS["session_preserved_rows"] == lo * k
    return got, ref, keys, sess, pipe, fx


def test_first_step_equals_plain_apply(tmp_path):
    """(a) one step on a fresh session = apply_emcid_to_text_encoder on a copy of the pipe, at the end-to-end bar."""
    reqs, hp_d, names, cache, stats = _setup(tmp_path, 8)
    plain, pipe = syn.build_pipe("toy", DEV), syn.build_pipe("toy", DEV)
    w0 = _weights(plain.text_encoder, names)
    em.apply_emcid_to_text_encoder(plain, reqs, EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=stats, verbose=False)
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
    assert sess.capacity == int(0.6 * 128) and sess.preserved == 0
    sess.apply(reqs, cache_name=cache)
    a, b = _weights(plain.text_encoder, names), _weights(pipe.text_encoder, names)
    for n in names:
        ref = a[n] - w0[n]
        err = ((b[n] - w0[n]) - ref).abs().max().item()
        assert err < BAR and err <= BAR * ref.abs().max().item(), (n, err)
    assert sess.preserved == 8


@pytest.mark.parametrize("sizes", [(5, 4), (5, 4, 3)], ids=["two-steps", "three-steps"])
def test_steps_match_fp64_primal_recomputation(tmp_path, sizes):
    """(b) two and three steps of disjoint request sets, every step against lam C' + sum P^T P + Kt^T Kt solved on the CPU."""
    _session_steps(tmp_path, sizes)


def test_multi_token_session_matches_primal(tmp_path):
    """(e) num_edit_tokens = 2: rows are concepts (N k per step), one two-step session against the primal recomputation."""
    _, _, _, sess, _, _ = _session_steps(tmp_path, (4, 3), k=2)
    assert sess.preserved == 14


def test_session_preserves_what_plain_calls_move(tmp_path):
    """(c) after step 2, max_i ||dW2 k_i|| / ||dW1 k_i|| over step 1's keys: the session's ratio is below that of two plain
    calls, and agrees per key with the ratio of the fp64 primal recomputation within the 1e-4 bar: |r - r_ref| <= 1e-4 max(r_ref, 1).
    Measured on MI355X (toy encoder, 5 + 4 concepts): see DESIGN.md §3."""
    sizes = (5, 4)
    got, ref, keys, sess, pipe, (reqs, hp_d, names, cache, stats) = _session_steps(tmp_path, sizes)
    plain = syn.build_pipe("toy", DEV)
    steps = [reqs[:5], reqs[5:9]]
    dws = []
    for st in steps:
        before = _weights(plain.text_encoder, names)
        em.apply_emcid_to_text_encoder(plain, st, EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=stats, verbose=False)
        after = _weights(plain.text_encoder, names)
        dws.append({n: after[n] - before[n] for n in names})
    r_sess, r_ref, r_plain = (_ratios(a, b, keys[0], names) for a, b in ((got[0], got[1]), (ref[0], ref[1]), (dws[0], dws[1])))
    for n in names:
        gap = (r_sess[n] - r_ref[n]).abs()
        print(f"{n}: ratios per key {[f'{v:.4e}' for v in r_sess[n].tolist()]}, largest |r - r_ref| {gap.max().item():.3e}")
        assert (gap <= BAR * r_ref[n].clamp(min=1.0)).all(), (n, r_sess[n], r_ref[n])
    worst = lambda r: max(v.max().item() for v in r.values())
    print(f"preservation ratio max_i |dW2 k_i| / |dW1 k_i|: session {worst(r_sess):.4e} (fp64 primal {worst(r_ref):.4e}), "
          f"two plain calls {worst(r_plain):.4e}")
    assert worst(r_sess) < worst(r_plain)


def test_full_set_restore_and_shared_factors(tmp_path, monkeypatch):
    """(d) PreservedSetFull before any launch (weights, preserved and the launch gauges untouched); restore() gives the original
    weights back bit for bit; a 3-step session leaves as many factor-cache entries as one plain call on the dual solver (the
    form whose factors a session shares; 5 concepts at d = 128 would take the direct one by themselves): it never refactored."""
    reqs, hp_d, names, cache, stats = _setup(tmp_path, 12)
    ee.clear_engine_caches()
    plain = syn.build_pipe("toy", DEV)
    monkeypatch.setenv("EMCID_SOLVER", "dual")
    em.apply_emcid_to_text_encoder(plain, reqs[:5], EMCIDHyperParams(**hp_d), DEV, cache_name=cache, stats_dir=stats, verbose=False)
    monkeypatch.delenv("EMCID_SOLVER")
    entries_plain = len(ee._FACTOR_CACHE)
    em.clear_caches()
    ee.clear_engine_caches()
    pipe = syn.build_pipe("toy", DEV)
    orig = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    w_orig = {n: get_parameter(pipe.text_encoder, n + ".weight").detach().clone() for n in names}
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats, capacity=10)
    sess.apply(reqs[:5], cache_name=cache)
    sess.apply(reqs[5:9], cache_name=cache)
    now = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    gauges = dict(cf.LAST_PATHS)
    with pytest.raises(emcid_amd.PreservedSetFull, match="capacity 10"):
        sess.apply(reqs[9:12], cache_name=cache)
    assert sess.preserved == 9 and dict(cf.LAST_PATHS) == gauges
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), now[n]), n
    sess.apply(reqs[9:10], cache_name=cache)
    assert sess.preserved == 10 and sess.steps == 3
    assert len(ee._FACTOR_CACHE) == entries_plain == 1
    sess.restore()
    assert sess.preserved == 0
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), orig[n]), n
    # a reset session starts over: its first step is a plain call's again
    sess.apply(reqs[:5], cache_name=cache)
    for n in names:
        a = get_parameter(plain.text_encoder, n + ".weight")
        b = get_parameter(pipe.text_encoder, n + ".weight")
        d = (a - w_orig[n]).abs().max().item()
        assert (a - b).abs().max().item() <= BAR * d, n


def test_stale_cache_retry_leaves_the_preserved_count(tmp_path):
    """The content guard inside a session: a weight rewritten behind the forward's caches (param.data.copy_) makes the step run
    again from the live weights — once, with M unchanged by the abandoned attempt — and the redone step is still the primal
    system's, step 1's keys preserved as they were when step 1 ran."""
    reqs, hp_d, names, cache, stats = _setup(tmp_path, 9)
    pipe = syn.build_pipe("toy", DEV)
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
    P = {}
    _primal_step(pipe.text_encoder, reqs[:5], hp_d, names, cache, stats, P)
    sess.apply(reqs[:5], cache_name=cache)
    w = get_parameter(pipe.text_encoder, "text_model.encoder.layers.0.mlp.fc1.weight")
    v = w._version
    w.data.copy_(w.data * 1.25)
    assert w._version == v                      # invisible to the version counter
    ref = _primal_step(pipe.text_encoder, reqs[5:9], hp_d, names, cache, stats, P)[0]
    retries = cf.LAST_PATHS.get("stale_cache_retries", 0)
    before = _weights(pipe.text_encoder, names)
    sess.apply(reqs[5:9], cache_name=cache)
    assert cf.LAST_PATHS.get("stale_cache_retries", 0) == retries + 1
    assert sess.preserved == 9 and sess.steps == 2
    after = _weights(pipe.text_encoder, names)
    for n in names:
        err = ((after[n] - before[n]) - ref[n]).abs().max().item()
        assert err < BAR and err <= BAR * ref[n].abs().max().item(), (n, err)


def test_indefinite_step_raises_restores_and_commits_nothing(tmp_path):
    """A step whose Schur complement is not positive definite — the session's Lp made far too small behind its back, so that
    Lkp = B Lp^-T is far too large (wrong state, not a fault) — raises torch.linalg.LinAlgError, leaves the weights as they were
    before the step and ``preserved`` where it was; with the state put right the same step goes through."""
    reqs, hp_d, names, cache, stats = _setup(tmp_path, 9)
    pipe = syn.build_pipe("toy", DEV)
    sess = emcid_amd.EditSession(pipe, EMCIDHyperParams(**hp_d), DEV, stats_dir=stats)
    sess.apply(reqs[:5], cache_name=cache)
    good = [(L.clone(), T.clone()) for L, T in zip(sess.keys.Lp, sess.keys.tile_inv)]
    for L, T in zip(sess.keys.Lp, sess.keys.tile_inv):
        L[:5] *= 1e-3
        T[0, :5] *= 1e3
    before = {n: p.detach().clone() for n, p in pipe.text_encoder.named_parameters()}
    with pytest.raises(torch.linalg.LinAlgError, match="preserved"):
        sess.apply(reqs[5:9], cache_name=cache)
    assert sess.preserved == 5 and sess.steps == 1 and cf.LAST_PATHS["session_preserved_rows"] == 5
    for n, p in pipe.text_encoder.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    for (L, T), Ld, Td in zip(good, sess.keys.Lp, sess.keys.tile_inv):
        Ld[:5].copy_(L[:5])
        Td[0, :5].copy_(T[0, :5])
    sess.apply(reqs[5:9], cache_name=cache)
    assert sess.preserved == 9 and sess.steps == 2

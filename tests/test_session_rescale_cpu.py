"""EditSession.rescale / reweight / sweep / apply(point=) without a GPU: the export and its binding, the unchanged ABI version and
sizer set, the workspace bound at N = capacity, the host commit of the row scales, the wrapper's launch-free and refusal cases on a
CPU state, and everything the session refuses before any device use (a CPU pipe never reaches a launch)."""
import re
from pathlib import Path

import pytest
import torch

import emcid_amd
from emcid_amd import edit_engine as ee, emcid_main as em, hip, synthetic as syn
from session_helpers import _hp, pipe  # noqa: F401  (pipe: a module-scoped fixture)

NEW = "emcid_session_rescale_f64"
SIZERS = {"emcid_edit_workspace_bytes", "emcid_cov_factor_workspace_bytes", "emcid_edit_dual_workspace_bytes",
          "emcid_edit_dual_preserve_workspace_bytes", "emcid_session_retain_workspace_bytes", "emcid_session_release_workspace_bytes",
          "emcid_cov_factor_fold_workspace_bytes", "emcid_edit_lu_workspace_bytes", "emcid_streamk_workspace_bytes",
          "emcid_linear_workspace_bytes", "emcid_gram_sp16_workspace_bytes", "emcid_clip_workspace_bytes"}
LEDGER = [("a", "edit", 1, 0), ("b", "edit", 1, 0), ("c", "retain", 1, 0), ("a", "edit", 2, 0)]


def test_symbol_is_exported_bound_and_declared():
    assert NEW in hip.EXPORTS
    fn = getattr(hip.load(), NEW)
    p, i64 = hip.C.c_void_p, hip.C.c_int64
    assert fn.restype is hip.C.c_int32 or fn.restype is hip.C.c_int
    assert list(fn.argtypes) == [p, p, i64, i64, i64, p, i64, p, i64, p, i64, i64, p, i64, p, p]
    header = (Path(hip.__file__).resolve().parents[1] / "include" / "emcid_hip.h").read_text()
    decl = re.search(rf"\bint {NEW}\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == len(fn.argtypes)
    for name in ("session_rescale", "RescaleWorkspace", "check_factors"):
        assert hasattr(hip, name), name
    assert hasattr(hip.PreservedKeys, "rescale_commit")
    assert {"session_rescales", "session_sweep_points"} <= set(emcid_amd.LAST_PATHS)
    for name in ("rescale", "reweight", "sweep"):
        assert hasattr(emcid_amd.EditSession, name), name


def test_abi_version_is_still_16_and_no_sizer_was_added():
    header = (Path(hip.__file__).resolve().parents[1] / "include" / "emcid_hip.h").read_text()
    assert re.search(r"#define\s+EMCID_ABI_VERSION\s+16\b", header)
    assert hip.ABI_VERSION == 16 and hip.load().emcid_abi_version() == 16
    assert {n for n in hip.EXPORTS if n.endswith("_workspace_bytes")} == SIZERS
    assert set(re.findall(r"\b(emcid_\w+_workspace_bytes)\(", header)) == SIZERS


def test_workspace_blocks_hold_a_rebuild_of_the_whole_capacity():
    """N = capacity (first = 0, one more row than a release can rebuild), sized by the retain sizer: every block the shared tail
    addresses lies inside the workspace.  The blocks, in doubles (csrc/session.hip, RetainWorkspace): K and Y [Np, dp], S, LS, XT
    [Np, Np], TT [Np, 128], B [Np, cp] with Np == cp — with first = 0 the tail never touches B, and at first > 0 it writes columns
    < first = capacity - N of N <= Np rows of it; the total is at least their sum."""
    lib = hip.load()
    for cap, d in ((200, 384), (129, 200), (1843, 3072), (256, 128), (257, 128)):
        for n in (cap, cap - 1, 1):
            Np, dp, cp = -(-n // 128) * 128, -(-d // 128) * 128, -(-cap // 128) * 128
            assert Np <= cp
            floor = 2 * Np * dp + 3 * Np * Np + Np * 128 + Np * cp
            assert lib.emcid_session_retain_workspace_bytes(n, d, cap) >= 8 * floor, (cap, d, n)
        assert lib.emcid_session_retain_workspace_bytes(cap + 1, d, cap) == 0


def test_check_factors_and_rescale_commit_on_the_host():
    assert hip.check_factors(0.5, 3).tolist() == [0.5, 0.5, 0.5]
    assert hip.check_factors([1, 2, 4], 3).tolist() == [1.0, 2.0, 4.0]
    assert hip.check_factors(2.0, 0).numel() == 0
    for bad in (0.0, -1.0, float("inf"), float("nan"), [1.0, float("nan"), 1.0], [1.0, 0.0, 1.0]):
        with pytest.raises(hip.EmcidHipError, match="positive and finite"):
            hip.check_factors(bad, 3)
    with pytest.raises(hip.EmcidHipError, match="committed rows"):
        hip.check_factors([1.0, 2.0], 3)
    st = hip.PreservedKeys(1, 128, 7, "cpu")
    st.commit(3, 1.5)
    st.commit(2, 2.5)
    st.rescale_commit(2.0)
    assert st.M == 5 and st.row_scale.tolist() == [3.0, 3.0, 3.0, 5.0, 5.0, 1.0, 1.0]        # rows behind M are not scaled
    st.rescale_commit([1, 1, 0.5, 1, 2])
    assert st.row_scale[:5].tolist() == [3.0, 3.0, 1.5, 5.0, 10.0]
    with pytest.raises(hip.EmcidHipError, match="positive and finite"):
        st.rescale_commit([1, 1, -1, 1, 1])
    assert st.row_scale[:5].tolist() == [3.0, 3.0, 1.5, 5.0, 10.0]


def test_the_wrapper_without_a_launch_and_its_refusals_on_a_cpu_state():
    st = hip.PreservedKeys(2, 128, 7, "cpu")
    st.commit(5)
    before = [t.clone() for t in st.Yp + st.Lp + st.tile_inv]
    assert hip.session_rescale(st, 1, 1.0) == {"ws": None, "launched": False, "first": 5}
    assert hip.session_rescale(st, 0, [1, 1, 1, 1, 1]) == {"ws": None, "launched": False, "first": 5}
    assert st.M == 5 and all(torch.equal(a, b) for a, b in zip(before, st.Yp + st.Lp + st.tile_inv))
    assert st.row_scale[:5].tolist() == [1.0] * 5                                # the entry commits nothing by itself
    for bad in (0.0, -2.0, float("nan"), float("inf"), [1, 1, 0, 1, 1]):
        with pytest.raises(hip.EmcidHipError, match="positive and finite"):
            hip.session_rescale(st, 0, bad)
    with pytest.raises(hip.EmcidHipError, match="committed rows"):
        hip.session_rescale(st, 0, [1.0, 2.0])
    with pytest.raises(hip.EmcidHipError, match="first = 3"):                    # a changed row below `first` would be skipped
        hip.session_rescale(st, 0, [1, 2, 1, 1, 1], first=3)
    for first in (6, -1):                                                        # outside [0, M], whatever the factors are
        with pytest.raises(hip.EmcidHipError, match="5 committed"):
            hip.session_rescale(st, 0, 1.0, first=first)
        with pytest.raises(hip.EmcidHipError, match="5 committed"):
            hip.session_rescale(st, 0, 0.5, first=first)
    with pytest.raises(hip.EmcidHipError, match="HBM"):                          # a rebuild has no CPU path
        hip.session_rescale(st, 0, 0.5)
    with pytest.raises(hip.EmcidHipError, match="HBM"):
        hip.session_rescale(st, 0, [1, 1, 1, 2, 1])
    with pytest.raises(hip.EmcidHipError, match="layer index"):
        hip.session_rescale(st, 2, 0.5)
    empty = hip.PreservedKeys(1, 128, 7, "cpu")
    assert hip.session_rescale(empty, 0, 0.5)["launched"] is False               # M = 0


def test_rescale_without_rows_only_changes_the_numbers(pipe):
    hp = _hp()
    sess = emcid_amd.EditSession(pipe, hp, "cpu")
    layers, k = sess._fixed[2:]
    sess.rescale(20, 0.4)
    assert sess._fixed == (20.0, 0.4, layers, k) and (float(hp.mom2_update_weight), float(hp.edit_weight)) == (20.0, 0.4)
    sess.rescale(edit_weight=0.7)
    assert sess._fixed == (20.0, 0.7, layers, k) and float(hp.mom2_update_weight) == 20.0
    sess.rescale(mom2_weight=5)
    assert sess._fixed == (5.0, 0.7, layers, k)
    sess.rescale()
    assert sess._fixed == (5.0, 0.7, layers, k)
    assert sess.keys is None and sess.preserved == 0 and sess._shared is None
    sess._check_call([None], None)                                               # the session agrees with its hparams again


@pytest.mark.parametrize("bad", [dict(mom2_weight=0), dict(mom2_weight=-3), dict(mom2_weight=float("inf")),
                                 dict(mom2_weight=float("nan")), dict(edit_weight=0.0), dict(edit_weight=1.0),
                                 dict(edit_weight=1.5), dict(mom2_weight="much")])
def test_rescale_refuses_bad_values(pipe, bad):
    hp = _hp()
    sess = emcid_amd.EditSession(pipe, hp, "cpu")
    with pytest.raises(ValueError):
        sess.rescale(**bad)
    with pytest.raises(ValueError):
        sess.apply(syn.make_requests(2), point=(bad.get("mom2_weight", 50), bad.get("edit_weight", 0.6)))
    assert sess._fixed[:2] == (50.0, 0.6) and (float(hp.mom2_update_weight), float(hp.edit_weight)) == (50.0, 0.6)


def test_a_folded_session_is_refused(pipe):
    gauges = dict(emcid_amd.LAST_PATHS)
    hp = _hp()
    sess = emcid_amd.EditSession(pipe, hp, "cpu")
    sess.folded, sess._ledger, sess._folded_sources = 5, list(LEDGER), {"old"}
    with pytest.raises(ValueError, match="folded"):
        sess.rescale(20, 0.4)
    with pytest.raises(ValueError, match="folded"):
        sess.reweight(["a"], 2.0)
    with pytest.raises(ValueError, match="folded"):
        sess.sweep(syn.make_requests(2), [(20, 0.4)])
    with pytest.raises(ValueError, match="folded"):
        sess.apply(syn.make_requests(2), point=(20, 0.4))
    assert sess._fixed[:2] == (50.0, 0.6) and sess.keys is None and dict(emcid_amd.LAST_PATHS) == gauges


def test_private_factors_without_folded_rows_are_refused_too(pipe):
    """A ``keep_folded`` session that folded and then released every folded source has ``folded == 0`` but still steps on its private
    factors, which are those of the point of the fold: no scalar rescales them, and a rescale that only changed the numbers would
    leave every later step on the old edit_weight's base."""
    hp = _hp()
    sess = emcid_amd.EditSession(pipe, hp, "cpu", keep_folded=True)
    sess.private_factors, sess.folds, sess.folded = object(), 2, 0           # (never looked into before the refusal)
    gauges = dict(emcid_amd.LAST_PATHS)
    for call in (lambda: sess.rescale(20, 0.4), lambda: sess.rescale(edit_weight=0.4), lambda: sess.reweight(["a"], 2.0),
                 lambda: sess.sweep(syn.make_requests(2), [(20, 0.4)]), lambda: sess.apply(syn.make_requests(2), point=(20, 0.4))):
        with pytest.raises(ValueError, match="has folded"):
            call()
    assert sess._fixed[:2] == (50.0, 0.6) and (float(hp.mom2_update_weight), float(hp.edit_weight)) == (50.0, 0.6)
    assert sess.keys is None and dict(emcid_amd.LAST_PATHS) == gauges
    sess.reset()                                                                 # drops the private factors: a fresh start may rescale
    sess.rescale(20, 0.4)
    assert sess._fixed[:2] == (20.0, 0.4)


def test_reweight_refusals(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    sess._ledger, sess._folded_sources = list(LEDGER), {"old"}
    for bad in (0, -1.0, float("nan"), float("inf"), "heavy", None):
        with pytest.raises(ValueError, match="weight"):
            sess.reweight(["a"], bad)
    with pytest.raises(KeyError, match="'zebra'"):
        sess.reweight(["a", "zebra"], 2.0)
    with pytest.raises(ValueError, match="folded"):
        sess.reweight(["old"], 2.0)
    with pytest.raises(ValueError, match="at least one source"):
        sess.reweight([], 2.0)
    assert sess.keys is None and sess.rows() == LEDGER


def test_sweep_refusals(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    with pytest.raises(ValueError, match="grid is empty"):
        sess.sweep(syn.make_requests(2), [])
    with pytest.raises(ValueError, match="edit_weight"):
        sess.sweep(syn.make_requests(2), [(20, 1.0)])
    with pytest.raises(ValueError, match="at least one request"):
        sess.sweep([], [(20, 0.4)])
    small = emcid_amd.EditSession(pipe, _hp(), "cpu", capacity=3)
    with pytest.raises(em.PreservedSetFull):
        small.sweep(syn.make_requests(4), [(20, 0.4)])
    assert sess.keys is None and small.keys is None


def test_they_refuse_what_apply_refuses(pipe, monkeypatch):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    sess._ledger = list(LEDGER)
    calls = (lambda **kw: sess.rescale(20, 0.4, **kw), lambda **kw: sess.reweight(["a"], 2.0, **kw),
             lambda **kw: sess.sweep(syn.make_requests(2), [(20, 0.4)], **kw),
             lambda **kw: sess.apply(syn.make_requests(2), point=(20, 0.4), **kw))
    for call in calls:
        with pytest.raises(NotImplementedError, match="one rank"):
            call(shard=ee.ConceptShard(0, 2))
    for solver in ("direct", "lu"):
        monkeypatch.setenv("EMCID_SOLVER", solver)
        for call in calls:
            with pytest.raises(ValueError, match="EMCID_SOLVER"):
                call()
    monkeypatch.delenv("EMCID_SOLVER")
    assert sess.keys is None and sess._fixed[:2] == (50.0, 0.6)


@pytest.mark.parametrize("change", [dict(mom2_update_weight=60), dict(edit_weight=0.5), dict(layers=[1, 2, 3])])
def test_hand_mutated_hparams_are_still_fixed(pipe, change):
    hp = _hp()
    sess = emcid_amd.EditSession(pipe, hp, "cpu")
    sess.rescale(20, 0.4)                                   # the session's own way to another point ...
    for k, v in change.items():
        setattr(hp, k, v)                                   # ... is not a licence to set the fields by hand
    for call in (lambda: sess.rescale(30, 0.5), lambda: sess.reweight(["a"], 2.0), lambda: sess.sweep(syn.make_requests(2), [(20, 0.4)]),
                 lambda: sess.apply(syn.make_requests(2)), lambda: sess.apply(syn.make_requests(2), point=(30, 0.5))):
        with pytest.raises(ValueError, match="fixed"):
            call()
    assert sess._fixed[:2] == (20.0, 0.4) and sess.keys is None


def test_a_saved_point_is_the_rescaled_one(pipe):
    """``save`` writes ``_fixed``: after a rescale the file's fixed set-up is the new point, and ``check_session_state`` refuses
    hparams that still hold the old one (the full round trip runs on the GPU: tests/test_session_rescale_gpu.py)."""
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    sess.rescale(20, 0.4)
    lam, e, layers, k = sess._fixed
    fixed = {"mom2_update_weight": lam, "edit_weight": e, "layers": list(layers), "num_edit_tokens": k}
    keys = hip.PreservedKeys(len(layers), sess.d, 1, "cpu").state_dict()
    state = {"format": em.SESSION_FORMAT, "fixed": fixed, "rewrite_module_tmp": sess.hparams.rewrite_module_tmp, "d": sess.d, "h": sess.h,
             "capacity": sess.capacity, "on_full": "raise", "report": False, "keep_folded": False,
             "counters": {c: 0 for c in em._SESSION_COUNTERS}, "ledger": [], "folded_sources": [], "archive_ledger": [], "keys": keys,
             "weights": [torch.zeros(sess.h, sess.d)] * len(layers), "orig": None, "base": None, "archive": None, "fingerprints": {}}
    assert em.check_session_state(state, sess._fixed) == 0
    with pytest.raises(ValueError, match="saved with"):
        em.check_session_state(state, (50.0, 0.6, layers, k))

"""EditSession.retain / report without a GPU: the exports, the unchanged ABI version, and everything ``retain`` refuses before any
device use (a CPU pipe never reaches a launch)."""
import re
from pathlib import Path

import pytest

import emcid_amd
from emcid_amd import hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from session_helpers import _hp, pipe  # noqa: F401  (pipe: a module-scoped fixture)

NEW = ("emcid_session_retain_workspace_bytes", "emcid_session_retain_f64", "emcid_session_step_norms_f64")


def test_symbols_are_exported_and_bound():
    assert set(NEW) <= set(hip.EXPORTS)
    lib = hip.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name            # bound with a signature, not ctypes' default
    assert len(lib.emcid_session_retain_f64.argtypes) == 19 and len(lib.emcid_session_step_norms_f64.argtypes) == 11
    header = (Path(hip.__file__).resolve().parents[1] / "include" / "emcid_hip.h").read_text()
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
    for fn in ("session_retain", "session_step_norms", "RetainWorkspace", "row_scale_of"):
        assert hasattr(hip, fn), fn
    assert "session_retained_rows" in emcid_amd.LAST_PATHS


def test_retain_workspace_size():
    lib = hip.load()
    assert lib.emcid_session_retain_workspace_bytes(5, 128, 4) == 0             # capacity below the call
    assert lib.emcid_session_retain_workspace_bytes(0, 128, 4) == 0
    small = lib.emcid_session_retain_workspace_bytes(5, 128, 76)
    # the key half of a step's workspace: smaller than the step's, whatever h is
    assert 0 < small < lib.emcid_edit_dual_preserve_workspace_bytes(5, 128, 32, 76)
    assert lib.emcid_session_retain_workspace_bytes(5, 128, 300) > small         # B = Yk Yp^T grows with the capacity


def test_abi_version_is_still_16():
    header = (Path(hip.__file__).resolve().parents[1] / "include" / "emcid_hip.h").read_text()
    assert re.search(r"#define\s+EMCID_ABI_VERSION\s+16\b", header)
    assert hip.ABI_VERSION == 16
    assert hip.load().emcid_abi_version() == 16


def test_row_scale_of_a_preserved_row():
    class F:                        # (CovFactors.lam_ratio without a device)
        lam = 50.0
        lam_ratio = hip.CovFactors.lam_ratio
    assert hip.row_scale_of(0.6, F(), 50.0) == (0.6 / 0.5) ** 0.5
    assert hip.row_scale_of(0.6, F(), 50.0, 4.0) == pytest.approx(2 * (0.6 / 0.5) ** 0.5, rel=1e-15)
    assert hip.row_scale_of(0.6, F(), 200.0) == pytest.approx((0.6 / 0.5) ** 0.5 / 2, rel=1e-15)
    st = hip.PreservedKeys(1, 128, 7, "cpu")
    st.commit(3, 1.5)
    st.commit(2)
    assert st.row_scale.tolist() == [1.5, 1.5, 1.5, 1.0, 1.0, 1.0, 1.0] and st.M == 5


def test_report_is_none_on_a_fresh_session(pipe):
    assert emcid_amd.EditSession(pipe, _hp(), "cpu").report() is None
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu", report=True)
    assert sess.report() is None and sess.retained == 0
    sess.reset()
    assert sess.report() is None and sess.retained == 0


def test_an_empty_list_is_refused(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    with pytest.raises(ValueError, match="at least one request"):
        sess.retain([])
    assert sess.keys is None


@pytest.mark.parametrize("weight", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "heavy", None])
def test_weight_must_be_positive_and_finite(pipe, weight):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    with pytest.raises(ValueError, match="weight"):
        sess.retain(syn.make_requests(2), weight=weight)
    assert sess.keys is None and sess.retained == 0


def test_a_full_set_raises_before_any_device_use(pipe):
    gauges = dict(emcid_amd.LAST_PATHS)
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu", capacity=4)            # on_full="raise"
    with pytest.raises(emcid_amd.PreservedSetFull, match="capacity 4"):
        sess.retain(syn.make_requests(5))
    assert sess.keys is None and sess.preserved == 0 and sess.retained == 0 and dict(emcid_amd.LAST_PATHS) == gauges
    # two rows per request: 3 requests are 6 rows
    sess = emcid_amd.EditSession(pipe, _hp(num_edit_tokens=2), "cpu", capacity=5)
    with pytest.raises(emcid_amd.PreservedSetFull, match="6 retained"):
        sess.retain(syn.make_requests(3))
    # on_full="fold" with a capacity below one request's rows cannot chunk either
    sess = emcid_amd.EditSession(pipe, _hp(num_edit_tokens=2), "cpu", capacity=1, on_full="fold")
    with pytest.raises(emcid_amd.PreservedSetFull):
        sess.retain(syn.make_requests(1))
    assert sess.keys is None


@pytest.mark.parametrize("change", [dict(mom2_update_weight=60), dict(edit_weight=0.5), dict(layers=[1, 2, 3]),
                                    dict(num_edit_tokens=2)])
def test_retain_refuses_changed_hparams(pipe, change):
    hp = _hp()
    sess = emcid_amd.EditSession(pipe, hp, "cpu")
    for k, v in change.items():
        setattr(hp, k, v)
    with pytest.raises(ValueError, match="fixed"):
        sess.retain(syn.make_requests(2))


def test_retain_refuses_what_apply_refuses(pipe, monkeypatch):
    from emcid_amd import edit_engine as ee
    reqs = syn.make_requests(3)
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    with pytest.raises(NotImplementedError, match="one rank"):
        sess.retain(reqs, shard=ee.ConceptShard(0, 2))
    for solver in ("direct", "lu"):
        monkeypatch.setenv("EMCID_SOLVER", solver)
        with pytest.raises(ValueError, match="EMCID_SOLVER"):
            sess.retain(reqs)
    monkeypatch.delenv("EMCID_SOLVER")
    with pytest.raises(hip.EmcidHipError, match="HBM"):          # a CPU encoder has no path
        sess.retain(reqs)
    assert sess.keys is None and sess.retained == 0

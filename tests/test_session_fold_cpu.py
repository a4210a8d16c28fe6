"""Folding an EditSession's preserved keys, without a GPU: the ABI of the new entry, the ``on_full`` argument, and what ``fold()``
does before any GPU work."""
import inspect
import re
from pathlib import Path

import pytest

import emcid_amd
from emcid_amd import hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from session_helpers import _hp, pipe  # noqa: F401  (pipe: a module-scoped fixture)

ROOT = Path(__file__).resolve().parents[1]


def test_abi_16_carries_the_fold_entry():
    header = (ROOT / "include" / "emcid_hip.h").read_text()
    lib = hip.load()
    assert int(re.search(r"#define\s+EMCID_ABI_VERSION\s+(\d+)", header).group(1)) == 16
    assert hip.ABI_VERSION == 16 and lib.emcid_abi_version() == 16
    assert "emcid_cov_factor_fold_f64" in header
    assert {"emcid_cov_factor_fold_f64", "emcid_cov_factor_fold_workspace_bytes"} <= set(hip.EXPORTS)
    fn = lib.emcid_cov_factor_fold_f64          # AttributeError if the built library does not export it
    assert fn.argtypes is not None and len(fn.argtypes) == 19
    # the scratch is the M x dp block of recovered keys, nothing else
    assert lib.emcid_cov_factor_fold_workspace_bytes(460, 768) == 460 * 768 * 8
    assert lib.emcid_cov_factor_fold_workspace_bytes(5, 100) == 5 * 128 * 8
    assert lib.emcid_cov_factor_fold_workspace_bytes(0, 768) == 0
    assert list(inspect.signature(hip.cov_factor_fold).parameters) == ["src", "state", "layer_index", "cov", "lam", "edit_weight", "dst",
                                                                       "base", "ws"]
    assert {"session_folds", "session_folded_rows"} <= set(emcid_amd.LAST_PATHS)
    assert not hasattr(emcid_amd, "cov_factor_fold") and not hasattr(emcid_amd, "fold")      # nothing new is exported: a method


def test_on_full_is_validated(pipe):
    assert emcid_amd.EditSession(pipe, _hp(), "cpu").on_full == "raise"
    assert emcid_amd.EditSession(pipe, _hp(), "cpu", on_full="fold").on_full == "fold"
    for bad in ("Fold", "drop", None, 1, ""):
        with pytest.raises(ValueError, match="on_full"):
            emcid_amd.EditSession(pipe, _hp(), "cpu", on_full=bad)


def test_fold_on_a_fresh_session_is_a_no_op(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu", on_full="fold")
    gauges = dict(emcid_amd.LAST_PATHS)
    sess.fold()
    assert sess.preserved == 0 and sess.folded == 0 and sess.folds == 0
    assert sess.keys is None and sess.private_factors is None
    assert dict(emcid_amd.LAST_PATHS) == gauges


def test_fold_has_no_cpu_path(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu", capacity=10)
    sess.keys = hip.PreservedKeys(4, sess.d, 10, "cpu")
    sess.keys.commit(3)                 # (a CPU session never gets this far by itself)
    assert sess.preserved == 3
    with pytest.raises(hip.EmcidHipError, match="no CPU path"):
        sess.fold()
    assert sess.preserved == 3 and sess.folded == 0 and sess.private_factors is None


@pytest.mark.parametrize("on_full", ["raise", "fold"])
def test_a_step_larger_than_the_capacity_still_raises(pipe, on_full):
    """on_full="raise" is the session of before; on_full="fold" raises as well when the step ALONE exceeds the capacity — both
    before anything is allocated or launched."""
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu", capacity=4, on_full=on_full)
    with pytest.raises(emcid_amd.PreservedSetFull, match="capacity 4"):
        sess.apply(syn.make_requests(5))
    assert sess.preserved == 0 and sess.keys is None and sess.folded == 0


def test_on_full_raise_keeps_raising_on_a_full_set(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu", capacity=4)
    sess.keys = hip.PreservedKeys(4, sess.d, 4, "cpu")
    sess.keys.commit(3)
    with pytest.raises(emcid_amd.PreservedSetFull, match="capacity 4"):
        sess.apply(syn.make_requests(2))
    assert sess.preserved == 3
    # the same full set with on_full="fold" goes to the fold instead — which has no CPU path
    sess.on_full = "fold"
    with pytest.raises(hip.EmcidHipError, match="no CPU path"):
        sess.apply(syn.make_requests(2))
    assert sess.preserved == 3 and sess.folded == 0

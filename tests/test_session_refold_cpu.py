"""Releasing across a fold without a GPU: the two exports and their argument counts, the unchanged ABI version, ``refold_plan`` (a
pure function), what the two entries refuse before they touch the device (the pointers here are host memory), and the session
surface of ``keep_folded`` that never reaches a launch."""
import ctypes as C
import re
from pathlib import Path

import pytest

import emcid_amd
from emcid_amd import emcid_main as em, hip
from session_helpers import _hp, pipe  # noqa: F401  (pipe: a module-scoped fixture)

NEW = ("emcid_session_refold_update_f64", "emcid_cov_factor_refactor_f64")
BAD_ARG, ERR_WORKSPACE = -1, -3
D, CAP, LAYERS = 128, 8, 2

_buf = (C.c_char * 4096)()
P = (C.addressof(_buf) + 15) & ~15          # a non-null, 16-byte aligned address that no entry gets as far as reading


def test_symbols_are_exported_and_bound():
    assert set(NEW) <= set(hip.EXPORTS)
    lib = hip.load()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.emcid_session_refold_update_f64.argtypes) == 15 and len(lib.emcid_cov_factor_refactor_f64.argtypes) == 6
    header = (Path(hip.__file__).resolve().parents[1] / "include" / "emcid_hip.h").read_text()
    for name, n_args in zip(NEW, (15, 6)):
        decl = re.search(rf"\b{name}\(([^;]*)\);", header)
        assert decl and decl.group(1).count(",") + 1 == n_args, name           # the header's count is the binding's
    for fn in ("session_refold_update", "cov_factor_refactor"):
        assert hasattr(hip, fn), fn
    for fn in ("folded_sources", "release"):
        assert hasattr(emcid_amd.EditSession, fn), fn
    assert hasattr(em, "refold_plan")


def test_abi_version_is_still_16_and_no_sizer_was_added():
    header = (Path(hip.__file__).resolve().parents[1] / "include" / "emcid_hip.h").read_text()
    assert re.search(r"#define\s+EMCID_ABI_VERSION\s+16\b", header)
    assert hip.ABI_VERSION == 16 and hip.load().emcid_abi_version() == 16
    assert not [n for n in hip.EXPORTS if "refold" in n or "refactor" in n if n.endswith("_workspace_bytes")]


LEDGER = [("e", "edit", 3, 0), ("a", "edit", 3, 0), ("f", "retain", 2, 0)]
ARCHIVE = [("a", "edit", 1, 0), ("b", "edit", 1, 0), ("c", "retain", 1, 0), ("d", "retain", 1, 0), ("b", "edit", 2, 0)]


def test_refold_plan_on_hand_filled_ledgers():
    assert em.refold_plan(LEDGER, ARCHIVE, ["b"]) == ([1, 4], [], 0)            # folded only, every occurrence
    assert em.refold_plan(LEDGER, ARCHIVE, ["c", "e"]) == ([2], [0], 1)         # live and folded mixed
    assert em.refold_plan(LEDGER, ARCHIVE, ["a"]) == ([0], [1], 0)              # a name in both ledgers loses all its rows
    assert em.refold_plan(LEDGER, ARCHIVE, ["c", "d", "f"]) == ([2, 3], [2], 3)  # retained rows of either are counted
    assert em.refold_plan(LEDGER, ARCHIVE, ["d", "d"]) == ([3], [], 1)          # a name given twice
    assert em.refold_plan(LEDGER, ARCHIVE, (s for s in "abcdef")) == ([0, 1, 2, 3, 4], [0, 1, 2], 3)     # any iterable
    assert em.refold_plan([], ARCHIVE, ["d"]) == ([3], [], 1)                   # M = 0
    assert em.refold_plan(LEDGER, [], ["e"]) == ([], [0], 0)
    two_a = [(s, k, o, t) for (s, k, o, _) in ARCHIVE[:2] for t in (0, 1)]       # num_edit_tokens = 2: both rows of a request
    two_l = [(s, k, o, t) for (s, k, o, _) in LEDGER[:1] for t in (0, 1)]
    assert em.refold_plan(two_l, two_a, ["b"]) == ([2, 3], [], 0)
    assert em.refold_plan(two_l, two_a, ["a", "e"]) == ([0, 1], [0, 1], 0)


def test_refold_plan_refusals():
    with pytest.raises(ValueError, match="at least one source"):
        em.refold_plan(LEDGER, ARCHIVE, [])
    with pytest.raises(KeyError, match="'zebra'"):
        em.refold_plan(LEDGER, ARCHIVE, ["b", "zebra"])
    with pytest.raises(KeyError):
        em.refold_plan([], [], ["a"])
    # release_plan is as it was: a folded name is still a ValueError there
    with pytest.raises(ValueError, match="restore"):
        em.release_plan(LEDGER, {"b"}, ["b"])


def _update(cov_ws=P, n_layers=LAYERS, layer=0, Yp=P, ldy=128, M=3, capacity=CAP, archive=P, lda=128, n_archived=4, rel=P, n_rel=2,
            base=P):
    return hip.load().emcid_session_refold_update_f64(cov_ws, n_layers, D, layer, Yp, ldy, M, capacity, archive, lda, n_archived, rel,
                                                      n_rel, base, None)


def test_update_entry_refuses_bad_arguments_before_the_device():
    """every call returns EMCID_ERR_BAD_ARG from the checks at the top of the entry: the pointers are host memory, a launch that
    read them would not return at all"""
    lib = hip.load()
    for kw in (dict(cov_ws=None), dict(archive=None), dict(base=None), dict(Yp=None), dict(rel=None),
               dict(layer=LAYERS), dict(layer=-1), dict(M=CAP + 1), dict(M=-1), dict(lda=129), dict(lda=126), dict(ldy=129),
               dict(M=0, n_rel=0), dict(n_rel=-1), dict(n_archived=-1), dict(archive=P + 8), dict(base=P + 8), dict(n_layers=0)):
        assert _update(**kw) == BAD_ARG, kw
        assert lib.emcid_last_error().decode().startswith("emcid_session_refold_update_f64: bad argument"), kw


def test_refactor_entry_refuses_a_short_workspace_and_null_pointers():
    lib = hip.load()
    need = lib.emcid_cov_factor_workspace_bytes(LAYERS, D)
    assert need > 8
    assert lib.emcid_cov_factor_refactor_f64(P, need - 8, LAYERS, D, P, None) == ERR_WORKSPACE
    assert lib.emcid_last_error().decode() == "emcid_cov_factor_refactor_f64: workspace too small (see emcid_cov_factor_workspace_bytes)"
    assert lib.emcid_cov_factor_refactor_f64(None, need, LAYERS, D, P, None) == BAD_ARG
    assert lib.emcid_cov_factor_refactor_f64(P, need, LAYERS, D, None, None) == BAD_ARG
    assert lib.emcid_cov_factor_refactor_f64(P, need, 0, D, P, None) == BAD_ARG
    assert lib.emcid_cov_factor_refactor_f64(P + 8, need, LAYERS, D, P, None) == BAD_ARG


def test_bindings_refuse_a_workspace_of_the_factor_cache():
    fac = hip.CovFactors(1, D, "cpu")
    fac.cached = True
    state = hip.PreservedKeys(1, D, CAP, "cpu")
    with pytest.raises(hip.EmcidHipError, match="cache"):
        hip.cov_factor_refactor(fac)
    with pytest.raises(hip.EmcidHipError, match="cache"):
        hip.session_refold_update(fac, state, 0, None, 0, None, None)


def test_keep_folded_session_surface_without_a_device(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu", keep_folded=True)
    assert sess.keep_folded is True and sess.folded_sources() == [] and sess._archive is None
    assert emcid_amd.EditSession(pipe, _hp(), "cpu").keep_folded is False
    with pytest.raises(KeyError, match="never seen"):
        sess.release(["never seen"])
    with pytest.raises(ValueError, match="at least one source"):
        sess.release([])
    # hand-filled ledgers: an unknown name beside a folded one is refused by refold_plan, before any device use
    sess._archive_ledger, sess._archived = list(ARCHIVE), len(ARCHIVE)
    assert sess.folded_sources() == ["a", "b", "c", "d"] and sess.sources() == [] and sess.rows() == []
    with pytest.raises(KeyError, match="'zebra'"):
        sess.release(["b", "zebra"])
    hp = _hp()
    changed = emcid_amd.EditSession(pipe, hp, "cpu", keep_folded=True)
    changed._archive_ledger = list(ARCHIVE)
    hp.edit_weight = 0.5
    with pytest.raises(ValueError, match="fixed"):                               # what _check_call refuses comes first
        changed.release(["b"])
    sess.reset()
    assert sess.folded_sources() == [] and sess._archive is None and sess._archived == 0
    assert sess.keys is None and sess.released == 0 and sess.folded == 0

"""EditSession.release without a GPU: the exports, the unchanged ABI version, the workspace size, the ledger's compaction (a pure
function) and everything ``release`` refuses before any device use (a CPU pipe never reaches a launch)."""
import re
from pathlib import Path

import pytest
import torch

import emcid_amd
from emcid_amd import emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams
from session_helpers import _hp, pipe  # noqa: F401  (pipe: a module-scoped fixture)

NEW = ("emcid_session_release_workspace_bytes", "emcid_session_release_f64")


def test_symbols_are_exported_and_bound():
    assert set(NEW) <= set(hip.EXPORTS)
    lib = hip.load()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name            # bound with a signature, not ctypes' default
    assert len(lib.emcid_session_release_f64.argtypes) == 15 and len(lib.emcid_session_release_workspace_bytes.argtypes) == 3
    header = (Path(hip.__file__).resolve().parents[1] / "include" / "emcid_hip.h").read_text()
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
    for fn in ("session_release", "ReleaseWorkspace", "check_keep"):
        assert hasattr(hip, fn), fn
    assert hasattr(hip.PreservedKeys, "release_commit")
    assert "session_released_rows" in emcid_amd.LAST_PATHS
    for fn in ("release", "rows", "sources"):
        assert hasattr(emcid_amd.EditSession, fn), fn


def test_abi_version_is_still_16():
    header = (Path(hip.__file__).resolve().parents[1] / "include" / "emcid_hip.h").read_text()
    assert re.search(r"#define\s+EMCID_ABI_VERSION\s+16\b", header)
    assert hip.ABI_VERSION == 16 and hip.load().emcid_abi_version() == 16


def test_release_workspace_is_the_retain_workspace_of_the_rebuilt_rows():
    lib = hip.load()
    assert lib.emcid_session_release_workspace_bytes(5, 128, 4) == 0             # more rebuilt rows than the capacity
    assert lib.emcid_session_release_workspace_bytes(0, 128, 4) == 0
    assert lib.emcid_session_release_workspace_bytes(-3, 128, 4) == 0
    for n, d, cap in ((5, 128, 76), (75, 128, 76), (199, 384, 200), (1842, 3072, 1843), (1790, 3072, 1843), (128, 200, 129)):
        got = lib.emcid_session_release_workspace_bytes(n, d, cap)
        assert got > 0 and got == lib.emcid_session_retain_workspace_bytes(n, d, cap), (n, d, cap)


def test_workspace_blocks_hold_a_rebuild_close_to_the_capacity():
    """N = capacity - 1: every block the shared tail addresses lies inside the workspace.  The blocks, in doubles (csrc/session.hip,
    RetainWorkspace): K and Y [Np, dp], S, LS, XT [Np, Np], TT [Np, 128], B [Np, cp] with Np <= cp — B's rows are cp wide and the tail
    writes columns < first <= capacity - N of N <= Np rows; the total is at least their sum."""
    lib = hip.load()
    for cap, d in ((200, 384), (129, 200), (1843, 3072), (256, 128), (257, 128)):
        n = cap - 1
        Np, dp, cp = -(-n // 128) * 128, -(-d // 128) * 128, -(-cap // 128) * 128
        assert Np <= cp
        floor = 2 * Np * dp + 3 * Np * Np + Np * 128 + Np * cp
        assert lib.emcid_session_release_workspace_bytes(n, d, cap) >= 8 * floor, (cap, d)


def test_check_keep_and_release_commit_on_the_host():
    assert hip.check_keep([0, 1, 2, 4, 7], 8) == ([0, 1, 2, 4, 7], 3)
    assert hip.check_keep([1, 2], 3) == ([1, 2], 0)
    assert hip.check_keep([0, 1, 2], 5) == ([0, 1, 2], 3)                        # trailing rows go: first == len(keep)
    assert hip.check_keep([], 5) == ([], 0)
    for bad in ([0, 0], [2, 1], [0, 8], [-1, 0]):
        with pytest.raises(hip.EmcidHipError, match="ascending"):
            hip.check_keep(bad, 8)
    st = hip.PreservedKeys(1, 128, 7, "cpu")
    st.commit(3, 1.5)
    st.commit(2, 2.5)
    st.commit(1)
    st.release_commit([0, 2, 3, 5])
    assert st.M == 4 and st.row_scale[:4].tolist() == [1.5, 1.5, 2.5, 1.0]
    with pytest.raises(hip.EmcidHipError, match="ascending"):
        st.release_commit([0, 4])
    assert st.M == 4
    # the launch-free cases never reach the library: a CPU state is enough to see it
    st2 = hip.PreservedKeys(2, 128, 7, "cpu")
    st2.commit(5)
    before = [t.clone() for t in st2.Yp + st2.Lp + st2.tile_inv]
    assert hip.session_release(st2, 1, [0, 1, 2]) == {"ws": None, "launched": False, "first": 3}
    assert hip.session_release(st2, 0, []) == {"ws": None, "launched": False, "first": 0}
    assert st2.M == 5 and all(torch.equal(a, b) for a, b in zip(before, st2.Yp + st2.Lp + st2.tile_inv))
    with pytest.raises(hip.EmcidHipError, match="HBM"):                          # a rebuild has no CPU path
        hip.session_release(st2, 0, [0, 2])
    with pytest.raises(hip.EmcidHipError, match="layer index"):
        hip.session_release(st2, 2, [0, 1])


LEDGER = [("a", "edit", 1, 0), ("b", "edit", 1, 0), ("c", "retain", 1, 0), ("d", "retain", 1, 0), ("a", "edit", 2, 0), ("e", "edit", 2, 0)]


def test_release_plan_on_a_hand_filled_ledger():
    assert em.release_plan(LEDGER, set(), ["b"]) == ([0, 2, 3, 4, 5], 1, 0)
    assert em.release_plan(LEDGER, set(), ["a"]) == ([1, 2, 3, 5], 0, 0)          # every occurrence of a source goes
    assert em.release_plan(LEDGER, set(), ["c", "d"]) == ([0, 1, 4, 5], 2, 2)     # retained rows are counted
    assert em.release_plan(LEDGER, set(), ["e"]) == ([0, 1, 2, 3, 4], 5, 0)       # trailing: first == len(keep)
    assert em.release_plan(LEDGER, set(), ["e", "e"]) == ([0, 1, 2, 3, 4], 5, 0)  # a name given twice
    assert em.release_plan(LEDGER, set(), (s for s in "abcde")) == ([], 0, 2)     # everything; any iterable
    two = [(s, k, o, t) for (s, k, o, _) in LEDGER[:2] for t in (0, 1)]           # num_edit_tokens = 2: both rows of a request
    assert em.release_plan(two, set(), ["a"]) == ([2, 3], 0, 0)
    assert em.release_plan(two, set(), ["b"]) == ([0, 1], 2, 0)


def test_release_plan_refusals():
    with pytest.raises(ValueError, match="at least one source"):
        em.release_plan(LEDGER, set(), [])
    with pytest.raises(KeyError, match="'zebra'"):
        em.release_plan(LEDGER, {"old"}, ["a", "zebra"])
    with pytest.raises(ValueError, match="restore") as e:
        em.release_plan(LEDGER, {"old"}, ["a", "old"])
    assert "folded" in str(e.value) and "'old'" in str(e.value)
    # a source folded once and entered again has live rows: those can go
    assert em.release_plan(LEDGER, {"b"}, ["b"]) == ([0, 2, 3, 4, 5], 1, 0)
    with pytest.raises(KeyError):
        em.release_plan([], set(), ["a"])


def test_release_on_a_session_without_rows_raises_keyerror(pipe):
    gauges = dict(emcid_amd.LAST_PATHS)
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    assert sess.rows() == [] and sess.sources() == []
    with pytest.raises(KeyError, match="never seen"):
        sess.release(["never seen"])
    with pytest.raises(KeyError, match=syn.make_requests(1)[0]["source"]):
        sess.release(syn.make_requests(1))                  # request dicts: their source is used
    assert sess.keys is None and sess.preserved == 0 and sess.released == 0 and dict(emcid_amd.LAST_PATHS) == gauges


def test_an_empty_list_is_refused(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    with pytest.raises(ValueError, match="at least one source"):
        sess.release([])
    with pytest.raises(ValueError, match="at least one source"):
        sess.release(iter(()))
    assert sess.keys is None


@pytest.mark.parametrize("change", [dict(mom2_update_weight=60), dict(edit_weight=0.5), dict(layers=[1, 2, 3]),
                                    dict(num_edit_tokens=2)])
def test_release_refuses_changed_hparams(pipe, change):
    hp = _hp()
    sess = emcid_amd.EditSession(pipe, hp, "cpu")
    for k, v in change.items():
        setattr(hp, k, v)
    with pytest.raises(ValueError, match="fixed"):
        sess.release(["anything"])
    with pytest.raises(ValueError, match="fixed"):
        sess.apply(syn.make_requests(2))                    # as apply refuses them
    assert sess.keys is None


def test_release_refuses_what_apply_refuses(pipe, monkeypatch):
    from emcid_amd import edit_engine as ee
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    with pytest.raises(NotImplementedError, match="one rank"):
        sess.release(["x"], shard=ee.ConceptShard(0, 2))
    for solver in ("direct", "lu"):
        monkeypatch.setenv("EMCID_SOLVER", solver)
        with pytest.raises(ValueError, match="EMCID_SOLVER"):
            sess.release(["x"])
    monkeypatch.delenv("EMCID_SOLVER")
    assert sess.keys is None


def test_reset_clears_the_ledger_and_the_gauge(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    sess._ledger, sess._folded_sources, sess.released = list(LEDGER), {"old"}, 3
    assert sess.sources() == ["a", "b", "c", "d", "e"] and sess.rows() == LEDGER
    sess.reset()
    assert sess.rows() == [] and sess.sources() == [] and sess._folded_sources == set() and sess.released == 0
    assert emcid_amd.LAST_PATHS["session_released_rows"] == 0

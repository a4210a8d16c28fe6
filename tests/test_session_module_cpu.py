"""The edit_session module without a GPU: ``hip.PreservedKeys.snapshot`` puts back exactly what it copied, the moved names are the
same objects under ``emcid_main`` in either import order, ``_fixed`` still is the plain tuple, the gauge table names gauges, and
the three validators refuse what ``retain`` / ``reweight`` / ``rescale`` / the constructor refuse (tests/test_session*_cpu.py)."""
import inspect
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import emcid_amd
from emcid_amd import clip_forward as cf, edit_session as es, emcid_main as em, hip
from session_helpers import LAYERS, _hp, pipe  # noqa: F401  (pipe: a module-scoped fixture)

REPO = Path(__file__).resolve().parents[1]
MOVED = ("PreservedSetFull", "release_plan", "refold_plan", "SESSION_FORMAT", "_SESSION_ENTRIES", "_SESSION_COUNTERS",
         "check_session_state", "_read_session_file", "_write_session_file", "EditSession")
NB = 128


def _filled(value=None):
    """PreservedKeys(2 layers, d = 8, capacity 300) on the host with M = 200: random contents, or ``value`` everywhere."""
    st = hip.PreservedKeys(2, 8, 300, "cpu")
    g = torch.Generator().manual_seed(3)
    for t in st.Yp + st.Lp + st.tile_inv + [st.row_scale]:
        if value is None:
            t.copy_(torch.randn(t.shape, dtype=torch.float64, generator=g))
        else:
            t.fill_(value)
    st.M = 200
    return st


@pytest.mark.parametrize("first,end", [(130, 200), (0, 203), (128, 129), (200, 200)])
def test_snapshot_restores_its_rows_and_tiles_and_nothing_else(first, end):
    st = _filled()
    assert NB == hip.NB
    orig = {"Yp": [t.clone() for t in st.Yp], "Lp": [t.clone() for t in st.Lp], "tile_inv": [t.clone() for t in st.tile_inv],
            "row_scale": st.row_scale.clone()}
    snap = st.snapshot(first, end)
    for i in range(st.n_layers):
        y = snap.Yp[i]
        assert y.dtype == torch.float64 and y.is_contiguous() and tuple(y.shape) == (end - first, st.dp)
        assert y.data_ptr() != st.Yp[i].data_ptr() and torch.equal(y, orig["Yp"][i][first:end])
    for t in st.Yp + st.Lp + st.tile_inv + [st.row_scale]:
        t.fill_(-7.0)
    snap.restore()
    held = end > first
    t0, t1 = (first // NB, -(-end // NB)) if held else (0, 0)
    for i in range(st.n_layers):
        for name, lo, hi in (("Yp", first, end), ("Lp", first, end), ("tile_inv", t0, t1)):
            got, was = getattr(st, name)[i], orig[name][i]
            assert torch.equal(got[lo:hi], was[lo:hi]), (name, i)
            assert bool((got[:lo] == -7.0).all()) and bool((got[hi:] == -7.0).all()), (name, i)
    m = st.M if held else 0
    assert torch.equal(st.row_scale[:m], orig["row_scale"][:m]) and bool((st.row_scale[m:] == -7.0).all())


_SAME = "; import emcid_amd.edit_session as s, emcid_amd.emcid_main as m; assert all(getattr(m, n) is getattr(s, n) for n in %r)" % (MOVED,)


@pytest.mark.parametrize("code", [
    "import emcid_amd.edit_session" + _SAME,
    "import emcid_amd.emcid_main as m; m.EditSession" + _SAME,
    "import emcid_amd; emcid_amd.EditSession",
], ids=["edit_session first", "emcid_main first", "the package"])
def test_either_import_order_works_in_a_fresh_interpreter(code):
    done = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=str(REPO)), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


def test_moved_names_are_one_object_under_both_modules():
    for name in MOVED:
        assert getattr(em, name) is getattr(es, name), name
        assert name not in vars(em), name                       # reached through the module's __getattr__, not defined there
    assert emcid_amd.EditSession is es.EditSession and emcid_amd.PreservedSetFull is es.PreservedSetFull
    with pytest.raises(AttributeError):
        em.no_such_name


def test_session_code_copies_rows_and_writes_gauges_in_one_place_each():
    src = inspect.getsource(es.EditSession)
    assert not re.search(r"(Yp|Lp|tile_inv)\[[^\n]*\]\.clone\(\)", src)         # hip.PreservedKeys.snapshot does
    assert not re.search(r"\[\"session_\w+\"\]\s*\+?=[^=]", src)                # EditSession._publish does
    main = inspect.getsource(em)
    for name in MOVED:
        assert not re.search(rf"^(class|def) {name}\b|^{name} =", main, re.M), name


def test_fixed_is_still_the_plain_tuple(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    fx = sess._fixed
    assert fx == (50.0, 0.6, tuple(LAYERS), 1) and tuple(fx) == (50.0, 0.6, tuple(LAYERS), 1)
    assert fx[:2] == (50.0, 0.6) and fx[2:] == (tuple(LAYERS), 1) and fx[3] == 1
    assert (fx.lam, fx.edit_weight, fx.layers, fx.num_edit_tokens) == tuple(fx)
    lam, e, layers, k = fx
    keys = hip.PreservedKeys(len(layers), sess.d, 1, "cpu").state_dict()
    state = {"format": es.SESSION_FORMAT, "rewrite_module_tmp": sess.hparams.rewrite_module_tmp, "d": sess.d, "h": sess.h,
             "fixed": {"mom2_update_weight": lam, "edit_weight": e, "layers": list(layers), "num_edit_tokens": k},
             "capacity": sess.capacity, "on_full": "raise", "report": False, "keep_folded": False,
             "counters": {c: 0 for c in es._SESSION_COUNTERS}, "ledger": [], "folded_sources": [], "archive_ledger": [], "keys": keys,
             "weights": [torch.zeros(sess.h, sess.d)] * len(layers), "orig": None, "base": None, "archive": None, "fingerprints": {}}
    assert es.check_session_state(state, fx) == 0
    with pytest.raises(ValueError, match=r"the hparams say \(20\.0, 0\.6, \(1, 2, 3, 4\), 1\)"):
        es.check_session_state(state, es._Fixed(20.0, 0.6, layers, k))


def test_counters_go_through_one_map(pipe):
    assert tuple(es._COUNTER_ATTRS) == es._SESSION_COUNTERS
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    for k, attr in es._COUNTER_ATTRS.items():
        assert attr == ("_retains" if k == "retains" else k) and getattr(sess, attr) == 0
        setattr(sess, attr, 3)
    sess.reset()
    assert (sess.steps, sess.folds, sess.folded, sess.retained, sess.released, sess._retains) == (0,) * 6


def test_gauge_table_names_gauges(pipe):
    for name in es._GAUGES:
        assert name in cf.LAST_PATHS or name == "session_loaded_rows", name
    assert {k for k in cf.LAST_PATHS if k.startswith("session_")} <= set(es._GAUGES)
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    sess.steps = 4
    before = dict(cf.LAST_PATHS)
    sess._publish("session_steps")
    assert cf.LAST_PATHS["session_steps"] == 4
    assert {k: v for k, v in cf.LAST_PATHS.items() if k != "session_steps"} == {k: v for k, v in before.items() if k != "session_steps"}
    sess.reset()
    assert all(cf.LAST_PATHS[k] == 0 for k in es._GAUGES if k != "session_loaded_rows")


@pytest.mark.parametrize("weight", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "heavy", None])
def test_positive_weight_refuses_what_retain_and_reweight_refuse(weight):
    with pytest.raises(ValueError) as err:
        es._positive_weight(weight)
    assert str(err.value) == f"weight must be a positive finite number (got {weight!r})"


def test_positive_weight_returns_the_float():
    assert es._positive_weight(4) == 4.0 and isinstance(es._positive_weight(4), float) and es._positive_weight("2.5") == 2.5


@pytest.mark.parametrize("lam,e,text", [
    (0.0, 0.6, "mom2_update_weight must be positive and finite in a session (got 0.0): the dual solver factors lam C'"),
    (-3.0, 0.6, "mom2_update_weight must be positive and finite in a session (got -3.0): the dual solver factors lam C'"),
    (float("inf"), 0.6, "mom2_update_weight must be positive and finite in a session (got inf): the dual solver factors lam C'"),
    (float("nan"), 0.6, "mom2_update_weight must be positive and finite in a session (got nan): the dual solver factors lam C'"),
    (50.0, 0.0, "edit_weight must lie inside (0, 1) in a session (got 0.0)"),
    (50.0, 1.0, "edit_weight must lie inside (0, 1) in a session (got 1.0)"),
    (50.0, 1.5, "edit_weight must lie inside (0, 1) in a session (got 1.5)"),
    (50.0, float("nan"), "edit_weight must lie inside (0, 1) in a session (got nan)"),
])
def test_check_point_refuses_what_the_constructor_and_rescale_refuse(pipe, lam, e, text):
    with pytest.raises(ValueError) as err:
        es._check_point(lam, e)
    assert str(err.value) == text
    with pytest.raises(ValueError) as ctor:
        emcid_amd.EditSession(pipe, _hp(mom2_update_weight=lam, edit_weight=e), "cpu")
    with pytest.raises(ValueError) as resc:
        emcid_amd.EditSession(pipe, _hp(), "cpu").rescale(lam, e)
    assert str(ctor.value) == str(resc.value) == text


def test_check_point_accepts_a_sound_point():
    assert es._check_point(50.0, 0.6) is None and es._check_point(1e-3, 0.999) is None


def test_source_names_takes_strings_and_request_dicts():
    assert es._source_names(["a", {"source": "b", "prompts": ["x"]}, "c"]) == ["a", "b", "c"]
    assert es._source_names([]) == [] and es._source_names(iter(["a"])) == ["a"]
    with pytest.raises(KeyError):
        es._source_names([{"prompts": ["x"]}])

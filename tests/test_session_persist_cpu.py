"""EditSession.save / EditSession.load without a GPU: the host validators of the session file (emcid_main.check_session_state,
hip.check_preserved_state) on a synthetic state at the toy encoder's dimensions, the marshalling of hip.PreservedKeys between two
capacities on host tensors, the file's round trip through ``torch.load(weights_only=True)``, and what ``load`` refuses before any
device call."""
import pytest
import torch

import emcid_amd
from emcid_amd import emcid_main as em, hip
from session_helpers import LAYERS, _hp, pipe  # noqa: F401  (pipe: the module-scoped CPU toy pipe)

D, H, DP = 128, 32, 128      # the toy encoder's fc2: (h, d) = (32, 128)


def _keys_state(M, d=D, n_layers=len(LAYERS), seed=0):
    g = torch.Generator().manual_seed(seed)
    tiles = (M + 127) // 128
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)      # noqa: E731
    return {"M": M, "d": d, "n_layers": n_layers, "Yp": [rnd(M, d) for _ in range(n_layers)],
            "Lp": [torch.tril(rnd(M, M)) for _ in range(n_layers)], "tile_inv": [rnd(tiles, 128, 128) for _ in range(n_layers)],
            "row_scale": torch.full((M,), 1.0954451150103321, dtype=torch.float64)}


def _state(M=5, folded=0, keep_folded=False, capacity=76):
    """A session file's dict as ``EditSession.save`` lays it out, with made-up numbers."""
    L = len(LAYERS)
    ledger = [(f"src{i}", "edit" if i % 2 else "retain", 1, 0) for i in range(M)]
    arch = [(f"old{i}", "edit", 1, 0) for i in range(folded)]
    return {
        "format": em.SESSION_FORMAT,
        "fixed": {"mom2_update_weight": 50.0, "edit_weight": 0.6, "layers": list(LAYERS), "num_edit_tokens": 1},
        "rewrite_module_tmp": _hp().rewrite_module_tmp, "d": D, "h": H, "capacity": capacity, "on_full": "fold", "report": False,
        "keep_folded": keep_folded,
        "counters": {"steps": 2, "folds": 1 if folded else 0, "folded": folded, "retained": (M + 1) // 2, "released": 0, "retains": 1},
        "ledger": ledger, "folded_sources": [] if keep_folded else [r[0] for r in arch], "archive_ledger": arch if keep_folded else [],
        "keys": _keys_state(M),
        "weights": [torch.randn(H, D) for _ in range(L)], "orig": [torch.randn(H, D) for _ in range(L)],
        "base": torch.randn(L, DP, DP, dtype=torch.float64) if folded else None,
        "archive": [torch.randn(folded, DP, dtype=torch.float64) for _ in range(L)] if keep_folded and folded else None,
        "fingerprints": {"encoder": [("text_model.final_layer_norm.weight", [H], "torch.float32", -123456789012345)],
                         "statistics": [("text_model.encoder.layers.1.mlp.fc2", "stats.npz", [D, D], 2 ** 62 + 1)]},
    }


FIXED = (50.0, 0.6, LAYERS, 1)


@pytest.mark.parametrize("kw", [dict(), dict(M=0), dict(M=5, folded=7), dict(M=3, folded=130, keep_folded=True), dict(M=76)],
                         ids=["plain", "empty", "folded", "keep_folded", "full"])
def test_a_synthetic_state_passes_the_validators(kw):
    st = _state(**kw)
    assert em.check_session_state(st) == st["keys"]["M"]
    assert em.check_session_state(st, FIXED, _hp().rewrite_module_tmp, D, H, 200) == st["keys"]["M"]
    assert hip.check_preserved_state(st["keys"], len(LAYERS), D, 76) == st["keys"]["M"]


def _refused(change, match, exc=ValueError, **args):
    st = _state(M=5, folded=7, keep_folded=True)
    change(st)
    with pytest.raises(exc, match=match):
        em.check_session_state(st, **args)


def test_an_unknown_format_is_refused():
    _refused(lambda st: st.update(format=em.SESSION_FORMAT + 1), "unknown format")
    _refused(lambda st: st.pop("format"), "not a session file")
    with pytest.raises(ValueError, match="not a session file"):
        em.check_session_state([1, 2])


def test_more_rows_than_the_capacity_are_refused():
    _refused(lambda st: None, "M = 5 committed rows exceed this state's capacity 4", capacity=4)
    _refused(lambda st: st.update(capacity=4), "capacity 4")
    with pytest.raises(hip.EmcidHipError, match="capacity 4"):
        hip.check_preserved_state(_keys_state(5), len(LAYERS), D, 4)


def test_a_ledger_of_another_length_is_refused():
    _refused(lambda st: st["ledger"].pop(), "ledger lists 4 rows, the state holds M = 5")
    _refused(lambda st: st["ledger"].append(("x", "edit", 3, 0)), "ledger lists 6 rows")


def test_another_width_is_refused():
    _refused(lambda st: None, "d = 128, this encoder's have d = 3072", d=3072)
    _refused(lambda st: None, "h = 32, this encoder's have h = 768", h=768)
    _refused(lambda st: st["keys"].update(d=256), "width d = 256")
    _refused(lambda st: st["keys"]["Yp"].__setitem__(2, torch.zeros(5, 127, dtype=torch.float64)), r"Yp\[2\]")
    _refused(lambda st: st["keys"]["Lp"].__setitem__(0, torch.zeros(5, 5)), r"Lp\[0\]")         # (fp32)
    _refused(lambda st: st["weights"].__setitem__(1, torch.zeros(H, D + 1)), r"weights\[1\]")
    with pytest.raises(hip.EmcidHipError, match="d = 128, this state's of d = 200"):
        hip.check_preserved_state(_keys_state(5), len(LAYERS), 200, 76)


def test_another_fixed_set_up_is_refused():
    _refused(lambda st: None, "a loaded session continues", fixed=(50.0, 0.6, (1, 2, 3), 1))
    _refused(lambda st: None, "a loaded session continues", fixed=(50.0, 0.5, LAYERS, 1))
    _refused(lambda st: None, "saved for the weights", rewrite_module_tmp="text_model.encoder.layers.{}.mlp.fc1")
    _refused(lambda st: st["keys"].update(n_layers=3), "holds 3 layers")
    with pytest.raises(hip.EmcidHipError, match="holds 4 layers, this state 2"):
        hip.check_preserved_state(_keys_state(5), 2, D, 76)


def test_an_archive_shorter_than_folded_is_refused():
    _refused(lambda st: st["archive"].__setitem__(3, st["archive"][3][:6]), r"archive\[3\] holds 6 rows, 7 were folded")
    _refused(lambda st: st["archive_ledger"].pop(), "archive's ledger lists 6 rows, 7 were folded")
    _refused(lambda st: st.update(archive=None), "archive must be a list")
    _refused(lambda st: st.update(base=None), "base")
    _refused(lambda st: st.update(keep_folded=False), "does not keep")


def test_preserved_keys_marshal_between_capacities_on_the_host():
    """state_dict -> a state of another capacity (another ldl, another tile count) -> state_dict: equal bit for bit; the refusals of
    load_state_dict leave the target as it was."""
    M, d = 130, 200
    a = hip.PreservedKeys(2, d, 200, "cpu")
    src = _keys_state(M, d, 2, seed=3)
    src["tile_inv"][0][1, 2:, :] = 0        # (as state_dict leaves the last tile: zero outside the rows and columns below M)
    src["tile_inv"][0][1, :, 2:] = 0
    src["tile_inv"][1][1, 2:, :] = 0
    src["tile_inv"][1][1, :, 2:] = 0
    a.load_state_dict(src)
    assert a.M == M and a.ldl == 200 and a.tile_inv[0].shape[0] == 2
    assert torch.equal(a.Yp[1][:M, d:], torch.zeros(M, 56, dtype=torch.float64))
    a.tile_inv[0][1, 5, 5] = 7.0            # what an uncommitted row left behind row M: not part of the state
    one = a.state_dict()
    b = hip.PreservedKeys(2, d, 261, "cpu")
    assert b.ldl == 262 and b.tile_inv[0].shape[0] == 3
    b.load_state_dict(one)
    two = b.state_dict()
    assert one["M"] == two["M"] == M and one["d"] == two["d"] == d and one["n_layers"] == two["n_layers"] == 2
    for name in ("Yp", "Lp", "tile_inv"):
        for x, y, z in zip(src[name], one[name], two[name]):
            assert torch.equal(x, y) and torch.equal(y, z), name
    assert torch.equal(one["row_scale"], two["row_scale"]) and torch.equal(b.row_scale[:M], src["row_scale"])
    small = hip.PreservedKeys(2, d, 129, "cpu")
    for target, sd, match in ((small, one, "capacity 129"), (hip.PreservedKeys(2, 201, 200, "cpu"), one, "d = 200"),
                              (hip.PreservedKeys(3, d, 200, "cpu"), one, "2 layers")):
        with pytest.raises(hip.EmcidHipError, match=match):
            target.load_state_dict(sd)
        assert target.M == 0 and not target.Yp[0].any()


def test_the_file_round_trips_through_weights_only(tmp_path):
    st = _state(M=3, folded=130, keep_folded=True)
    path = tmp_path / "deep" / "sess.pt"
    path.parent.mkdir()
    path.write_bytes(b"the previous file")
    n = em._write_session_file(st, path)
    assert n == path.stat().st_size > 0 and [p.name for p in path.parent.iterdir()] == ["sess.pt"]      # no temporary left
    back = torch.load(str(path), weights_only=True)
    assert em._read_session_file(path).keys() == back.keys() == st.keys()
    assert em.check_session_state(back, FIXED, _hp().rewrite_module_tmp, D, H) == 3

    def same(x, y):
        if isinstance(x, torch.Tensor):
            return isinstance(y, torch.Tensor) and x.dtype == y.dtype and torch.equal(x, y)
        if isinstance(x, dict):
            return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
        if isinstance(x, (list, tuple)):
            return type(x) is type(y) and len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        return type(x) is type(y) and x == y

    assert same(st, back)


def test_an_interrupted_save_leaves_the_previous_file(tmp_path, monkeypatch):
    path = tmp_path / "sess.pt"
    em._write_session_file(_state(), path)
    before = path.read_bytes()

    def dies(obj, f):
        with open(f, "wb") as fh:
            fh.write(b"half a fi")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", dies)
    with pytest.raises(OSError, match="disk full"):
        em._write_session_file(_state(M=7), path)
    assert path.read_bytes() == before and [p.name for p in tmp_path.iterdir()] == ["sess.pt"]


def test_load_refuses_on_the_host_what_the_file_shows(pipe, tmp_path):
    path = tmp_path / "sess.pt"
    em._write_session_file(_state(M=5), path)
    with pytest.raises(ValueError, match="weights must be"):
        emcid_amd.EditSession.load(pipe, _hp(), path, weights="copy")
    with pytest.raises(ValueError, match="capacity 4"):
        emcid_amd.EditSession.load(pipe, _hp(), path, capacity=4)
    with pytest.raises(ValueError, match="a loaded session continues"):
        emcid_amd.EditSession.load(pipe, _hp(edit_weight=0.5), path)
    with pytest.raises(ValueError, match="a loaded session continues"):
        emcid_amd.EditSession.load(pipe, _hp(layers=[1, 2, 3]), path)
    with pytest.raises(ValueError, match="on_full"):
        emcid_amd.EditSession.load(pipe, _hp(), path, on_full="drop")
    bad = _state(M=5)
    bad["format"] = 99
    em._write_session_file(bad, path)
    with pytest.raises(ValueError, match="unknown format 99"):
        emcid_amd.EditSession.load(pipe, _hp(), path)


def test_load_on_a_cpu_pipe_raises_what_apply_raises(pipe, tmp_path, monkeypatch):
    path = tmp_path / "sess.pt"
    em._write_session_file(_state(M=5), path)
    with pytest.raises(hip.EmcidHipError, match="HBM"):
        emcid_amd.EditSession.load(pipe, _hp(), path)
    with pytest.raises(hip.EmcidHipError, match="HBM"):
        emcid_amd.EditSession(pipe, _hp()).save(tmp_path / "other.pt")
    assert not (tmp_path / "other.pt").exists()
    monkeypatch.setenv("EMCID_SOLVER", "lu")
    with pytest.raises(ValueError, match="EMCID_SOLVER"):
        emcid_amd.EditSession.load(pipe, _hp(), path)


def test_the_new_entry_is_exported_under_the_same_abi():
    assert "emcid_fingerprint_content" in hip.EXPORTS and hip.ABI_VERSION == 16
    lib = hip.load()
    assert lib.emcid_fingerprint_content(1, None, None, None, None) == -1 and b"bad argument" in lib.emcid_last_error()
    assert lib.emcid_fingerprint_content(0, None, None, None, None) == 0

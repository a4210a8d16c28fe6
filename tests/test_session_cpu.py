"""EditSession without a GPU: the export, argument validation and the out-of-scope errors (all raised before any GPU work)."""
import pytest

import emcid_amd
from emcid_amd import edit_engine as ee, emcid_main as em, hip, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams, EMCIDXLHyperParams
from session_helpers import _hp, pipe  # noqa: F401  (pipe: a module-scoped fixture)


def test_package_exports_the_session():
    assert emcid_amd.EditSession is em.EditSession and emcid_amd.PreservedSetFull is em.PreservedSetFull
    assert issubclass(emcid_amd.PreservedSetFull, RuntimeError)
    assert {"session_steps", "session_preserved_rows"} <= set(emcid_amd.LAST_PATHS)
    assert "dual_preserve" in ee.DUAL_FORMS
    assert {"emcid_edit_layer_dual_preserve_f64", "emcid_edit_dual_preserve_workspace_bytes"} <= set(hip.EXPORTS)
    lib = hip.load()
    assert lib.emcid_edit_dual_preserve_workspace_bytes(5, 128, 32, 4) == 0          # capacity below the step
    assert lib.emcid_edit_dual_preserve_workspace_bytes(5, 128, 32, 76) > lib.emcid_edit_dual_workspace_bytes(5, 128, 32)


def test_defaults_and_state(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    assert sess.capacity == int(0.6 * 128) and sess.preserved == 0 and sess.steps == 0 and sess.keys is None
    assert emcid_amd.EditSession(pipe, _hp(), "cpu", capacity=20).capacity == 20
    sess.reset()
    sess.restore()          # nothing applied yet: both are no-ops
    assert sess.preserved == 0


@pytest.mark.parametrize("capacity", [0, -3, 2.5, "10", True])
def test_capacity_must_be_a_positive_integer(pipe, capacity):
    with pytest.raises(ValueError, match="capacity"):
        emcid_amd.EditSession(pipe, _hp(), "cpu", capacity=capacity)


def test_hparams_are_validated(pipe):
    with pytest.raises(ValueError, match="mom2_update_weight"):
        emcid_amd.EditSession(pipe, _hp(mom2_update_weight=0), "cpu")
    with pytest.raises(ValueError, match="edit_weight"):
        emcid_amd.EditSession(pipe, _hp(edit_weight=1.0), "cpu")
    with pytest.raises(ValueError, match="forward order"):
        emcid_amd.EditSession(pipe, _hp(layers=[3, 1]), "cpu")
    with pytest.raises(TypeError, match="EMCIDHyperParams"):
        emcid_amd.EditSession(pipe, dict(layers=[1]), "cpu")
    with pytest.raises(ValueError, match="device"):
        emcid_amd.EditSession(pipe, _hp(), "cuda:0")          # the encoder is on the CPU
    assert emcid_amd.EditSession(pipe, _hp()).capacity == 76   # device is optional


def test_out_of_scope_is_refused_with_a_reason(pipe, monkeypatch):
    xl = EMCIDXLHyperParams(**syn.sdxl_hparams_dict())
    with pytest.raises(NotImplementedError, match="SDXL"):
        emcid_amd.EditSession(pipe, xl, "cpu")
    two = syn.build_pipe("toy", "cpu", sdxl=True)
    with pytest.raises(NotImplementedError, match="SDXL"):
        emcid_amd.EditSession(two, _hp(), "cpu")
    with pytest.raises(NotImplementedError, match="cross-attention"):
        emcid_amd.EditSession(pipe, _hp(rewrite_module_tmp="down_blocks.{}.attentions.0.transformer_blocks.0.attn2.to_k"), "cpu")
    reqs = syn.make_requests(3)
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu", capacity=4)
    with pytest.raises(NotImplementedError, match="one rank"):
        sess.apply(reqs, shard=ee.ConceptShard(0, 2))
    with pytest.raises(NotImplementedError, match="one rank"):
        sess.apply(reqs, shard=ee.ConceptShard(0, 1, force_collectives=True))
    for solver in ("direct", "lu"):
        monkeypatch.setenv("EMCID_SOLVER", solver)
        with pytest.raises(ValueError, match="EMCID_SOLVER"):
            sess.apply(reqs)
    monkeypatch.delenv("EMCID_SOLVER")
    with pytest.raises(ValueError, match="at least one request"):
        sess.apply([])
    with pytest.raises(emcid_amd.PreservedSetFull, match="capacity 4"):
        sess.apply(syn.make_requests(5))
    assert sess.preserved == 0 and sess.keys is None            # nothing was allocated, let alone launched


@pytest.mark.parametrize("change", [dict(mom2_update_weight=60), dict(edit_weight=0.5), dict(layers=[1, 2, 3]),
                                    dict(num_edit_tokens=2)])
def test_a_step_refuses_changed_hparams(pipe, change):
    hp = _hp()
    sess = emcid_amd.EditSession(pipe, hp, "cpu")
    for k, v in change.items():
        setattr(hp, k, v)
    with pytest.raises(ValueError, match="fixed"):
        sess.apply(syn.make_requests(2))


def test_a_cpu_encoder_has_no_path(pipe):
    sess = emcid_amd.EditSession(pipe, _hp(), "cpu")
    with pytest.raises(hip.EmcidHipError, match="HBM"):
        sess.apply(syn.make_requests(2))


def test_preserved_keys_bookkeeping_needs_no_kernel():
    with pytest.raises(hip.EmcidHipError, match="capacity"):
        hip.PreservedKeys(1, 128, 0, "cpu")
    st = hip.PreservedKeys(2, 100, 7, "cpu")
    assert st.dp == 128 and st.ldl == 8 and st.M == 0
    assert [tuple(t.shape) for t in (st.Yp[1], st.Lp[1], st.tile_inv[1])] == [(7, 128), (7, 8), (1, 128, 128)]
    assert st.nbytes == 2 * 8 * (7 * 128 + 7 * 8 + 128 * 128)
    st.commit(5)
    assert st.M == 5
    with pytest.raises(AssertionError):
        st.commit(3)
    st.reset()
    assert st.M == 0

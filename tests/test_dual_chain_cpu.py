"""The host side of the dual chain's test access (include/emcid_hip.h): emcid_edit_dual_block names every block of a dual
workspace, emcid_full_inverse_scratch_doubles states what the explicit-inverse build writes into its scratch, and
emcid_edit_dual_schur_form reports which solve of Z = S^-1 Rt a shape gets.  Nothing here launches a kernel: the library is
loaded without a GPU and every call returns from its argument checks or from host arithmetic."""
import ctypes as C
import re
from pathlib import Path

import pytest

from emcid_amd import hip

REPO = Path(__file__).resolve().parents[1]
NEW = ["emcid_edit_dual_block", "emcid_edit_dual_schur_form", "emcid_full_inverse_scratch_doubles", "emcid_full_inverse_f64"]


def _up(x, m):
    return -(-x // m) * m


def test_the_new_entries_are_exported_under_the_same_abi():
    header = (REPO / "include" / "emcid_hip.h").read_text()
    assert int(re.search(r"#define\s+EMCID_ABI_VERSION\s+(\d+)", header).group(1)) == hip.ABI_VERSION == 16
    lib = hip.load()
    for name in NEW:
        assert name in hip.EXPORTS and name in header and hasattr(lib, name)
    # the names of the binding are the constants of the header, in order
    for i, name in enumerate(hip.DUAL_BLOCKS):
        assert re.search(rf"EMCID_DUAL_{name}\s*=\s*{i}\b", header), name
    for i, name in enumerate(hip.SCHUR_FORMS):
        assert re.search(rf"EMCID_SCHUR_{name.upper()}\s*=\s*{i}\b", header), name


def test_block_accessor_refuses_bad_arguments():
    lib = hip.load()
    buf = (C.c_double * 2)()
    base = C.addressof(buf)
    n = C.c_int64(7)
    for args in ((None, 100, 256, 32, 0), (base, 0, 256, 32, 0), (base, 100, -1, 32, 0), (base, 100, 256, 0, 0),
                 (base, 100, 256, 32, -1), (base, 100, 256, 32, len(hip.DUAL_BLOCKS))):
        n.value = 7
        assert lib.emcid_edit_dual_block(*args, C.byref(n)) is None and n.value == -1, args
    assert lib.emcid_edit_dual_block(None, 100, 256, 32, 0, None) is None          # the length is optional
    assert lib.emcid_edit_dual_schur_form(0, 256, 32) == -1 and lib.emcid_edit_dual_schur_form(100, 256, -3) == -1
    assert lib.emcid_full_inverse_scratch_doubles(0, 128) == -1 and lib.emcid_full_inverse_scratch_doubles(200, 256) == -1
    assert lib.emcid_full_inverse_scratch_doubles(256, 128) == -1


@pytest.mark.parametrize("N,d,h", [(100, 256, 32), (130, 200, 48), (600, 384, 48), (2049, 1152, 64), (4100, 256, 33)])
def test_blocks_tile_the_workspace_in_order(N, d, h):
    """Every block starts where the one before it ends, the last one ends with the workspace, and the shapes the binding's
    views assume are the lengths the library reports (only addresses are formed: the base is never dereferenced)."""
    lib = hip.load()
    Np, dp, hp = _up(N, 128), _up(d, 128), _up(h, 2)
    base = 1 << 20
    n = C.c_int64(0)
    at = base
    got = {}
    for i, name in enumerate(hip.DUAL_BLOCKS[:-1]):
        p = lib.emcid_edit_dual_block(base, N, d, h, i, C.byref(n))
        assert p == at and n.value > 0, name
        got[name] = n.value
        at += 8 * n.value
    assert at - base == lib.emcid_edit_dual_workspace_bytes(N, d, h)
    for name in ("K", "P", "Y", "PT", "Y2"):
        assert got[name] == Np * dp, name
    for name in ("S", "LS", "XT"):
        assert got[name] == Np * Np, name
    assert got["R"] == Np * hp and got["V"] == got["U"] == hp * dp and got["TT"] == Np * 128
    assert got["INVS"] == lib.emcid_inverse_workspace_doubles(Np)
    assert 8 * got["SK"] == lib.emcid_streamk_workspace_bytes(256)
    # the ticket counters are the tail of the stream-K block
    p = lib.emcid_edit_dual_block(base, N, d, h, hip.DUAL_BLOCKS.index("SK_COUNTERS"), C.byref(n))
    assert n.value == 8192 and p + 8 * n.value == lib.emcid_edit_dual_block(base, N, d, h, hip.DUAL_BLOCKS.index("XT"), None)
    # the accessors that were there before name the same blocks
    for fn, name in (("emcid_edit_dual_pt", "P"), ("emcid_edit_dual_yt", "Y"), ("emcid_edit_dual_s", "S"), ("emcid_edit_dual_u", "U")):
        assert getattr(lib, fn)(base, N, d, h) == lib.emcid_edit_dual_block(base, N, d, h, hip.DUAL_BLOCKS.index(name), None)


def _scratch_by_hand(dp, lda):
    """What the recursive-halving build writes into its scratch, worked out from its description alone: the 512-blocks
    [b0, b1) split at mid = b0 + n // 2; the step forms T = L21 X11 with m = rows below the split (the last block may be
    short) and nn = columns left of it, copy c of `reps` at row c * m, leading dimension lda.  Halves that are the same problem
    (dp a multiple of 512, equal block counts) run once with reps doubled."""
    nob = -(-dp // 512)
    regular = dp % 512 == 0
    need = 0

    def rec(b0, b1, reps, stride):
        nonlocal need
        n = b1 - b0
        if n <= 1:
            return
        mid = b0 + n // 2
        left, right = mid - b0, b1 - mid
        if regular and left == right and (reps == 1 or stride == 2 * left):
            rec(b0, mid, reps * 2, left)
        else:
            rec(b0, mid, reps, stride)
            rec(mid, b1, reps, stride)
        m, nn = min(b1 * 512, dp) - mid * 512, (mid - b0) * 512
        need = max(need, (reps * m - 1) * lda + nn)

    rec(0, nob, 1, 0)
    return need


@pytest.mark.parametrize("dp", [128, 512, 640, 1024, 1408, 1536, 2048, 2176, 3072, 4096, 4224, 5120])
def test_full_inverse_scratch_arithmetic(dp):
    lib = hip.load()
    for lda in (dp, dp + 64):
        need = lib.emcid_full_inverse_scratch_doubles(dp, lda)
        assert need == _scratch_by_hand(dp, lda)
        if dp <= 512:
            assert need == 0                       # one block: only the diagonal inverse is copied
        elif dp % 512 == 0 and (dp // 512) & (dp // 512 - 1) == 0:
            assert need == (dp // 2 - 1) * lda + dp // 2      # a power of two of blocks: dp / 2 rows at every level
        assert need <= dp * lda                    # the covariance workspace's M region always holds it
    # the figures of the dual solve at 2049 concepts: the top split leaves 1152 rows below 1024 columns
    assert lib.emcid_full_inverse_scratch_doubles(2176, 2176) == 1151 * 2176 + 1024 == 2505600


def test_schur_form_follows_the_scratch():
    """Z = S^-1 Rt goes against the explicit inverse only where the workspace's [dp][Np] scratch holds the build's; d = 768
    keys with 2100 concepts (768 * 2176 < 1151 * 2176 + 1024) is the shape that used to write past it."""
    lib = hip.load()
    form = lambda N, d, h: hip.SCHUR_FORMS[lib.emcid_edit_dual_schur_form(N, d, h)]
    assert form(100, 256, 32) == "full_inverse"                    # Np = 128: one block, no scratch
    assert form(130, 200, 48) == form(2000, 256, 32) == "xrow"     # 256 <= Np <= 2048: the inverse rides in the factorization
    assert form(2049, 1152, 64) == "full_inverse" and 1152 * 2176 >= 2505600
    assert form(2049, 1024, 64) == form(2100, 768, 768) == form(2049, 256, 32) == "substitution"
    assert form(2100, 3072, 768) == form(4096, 3072, 768) == "full_inverse"
    assert form(4097, 3072, 768) == form(4100, 256, 32) == "substitution"          # beyond Np = 4096
    for N in range(2049, 4097, 128):                               # the branch is exactly the scratch condition
        Np = _up(N, 128)
        for d in (128, Np // 2 - 128, Np // 2, Np // 2 + 128, Np):
            d = _up(max(d, 128), 128)
            fits = lib.emcid_full_inverse_scratch_doubles(Np, Np) <= d * Np
            assert form(N, d, 64) == ("full_inverse" if fits else "substitution"), (N, d)


def test_a_scratch_that_is_too_small_is_refused_before_any_launch():
    """emcid_full_inverse_f64 checks its scratch against the same arithmetic before its first launch, so the call returns
    EMCID_ERR_WORKSPACE from the host (the pointers are never dereferenced: no GPU is needed to see it)."""
    lib = hip.load()
    fake = 1 << 20
    need = lib.emcid_full_inverse_scratch_doubles(2176, 2176)
    for have in (0, 256 * 2176, need - 1):
        assert lib.emcid_full_inverse_f64(fake, 2176, 2176, fake, fake, fake, have, None) == -3
        assert b"full_inverse_scratch_doubles" in lib.emcid_last_error()
    assert lib.emcid_full_inverse_f64(fake, 2176, 2176, fake, fake, None, need, None) == -1
    assert lib.emcid_full_inverse_f64(fake, 2100, 2176, fake, fake, fake, need, None) == -1

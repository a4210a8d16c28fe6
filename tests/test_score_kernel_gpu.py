"""emcid_score_rows_f32 and emcid_score_chains_f64 (include/emcid_hip.h, csrc/score.hip) through the binding, no encoder, against
numpy fp64 on the same fp32 inputs.

The bounds are derived, not measured.  Every value is converted exactly and every operation is an fp64 one, so a sum of n <= 2048
non-negative terms, each the product of values that carry a few roundings, is good to a small multiple of 2^-53 log2(n): 1e-12 of
the sum leaves three orders of magnitude; the signed sum a^ . b^ of slot 3 is held to 1e-12 of its own magnitude as well (on these
inputs it falls to 1e-3 of ||a^|| ||b^||, which still leaves two orders).  The cancelling slot 6 is a sum of signed products bounded by ||a - b|| ||t - b||
(Cauchy-Schwarz), so its error is at most n 2^-53 < 2.3e-13 of that product.  One case needs more than fp64 from the REFERENCE:
with b one ulp from a, LayerNorm(a) - LayerNorm(b) formed from the two normalised rows in fp64 carries their roundings (1e-16 of
values of order 1) in a difference of order 1e-7 — 1e-9 relative, three orders above the bound, whatever the kernel does — so
that case's reference is the same formula in 40-digit arithmetic (mpmath) on the same fp32 inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import forward_refs as fr
from emcid_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
SHAPES = [(1, 32), (5, 200), (257, 768), (6, 1280), (3, 2048)]
EPS = 1e-5


def _inputs(rows, cols, seed=0):
    """(a, b, t, gamma, beta) fp32 on the CPU: rows riding on an offset of 500, rows with one channel 1000 times the rest, a zero and
    a constant row (forward_refs.trained_rows); b an independent draw plus noise, so that no row of b equals its row of a."""
    a, gamma, beta = fr.trained_rows(rows, cols, seed=seed)
    g = torch.Generator().manual_seed(991 + rows + cols + seed)
    b = fr.trained_rows(rows, cols, seed=seed + 1)[0] + 0.1 * torch.randn(rows, cols, generator=g)
    t = 2.0 * torch.randn(rows, cols, generator=g)
    return a, b, t, gamma, beta


def _ln64(x, gamma, beta, eps):
    x = x.astype(np.float64)
    c = x - x.mean(axis=1, keepdims=True)
    return c / np.sqrt((c * c).mean(axis=1, keepdims=True) + np.float64(np.float32(eps))) * gamma.astype(np.float64) + beta.astype(np.float64)


def _ref(a, b, t, gamma, beta, ln, with_t):
    """(rows, 8) fp64 by the definition, and the bound's scale per slot."""
    a64, b64 = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
    ah, bh = (_ln64(a.numpy(), gamma.numpy(), beta.numpy(), EPS), _ln64(b.numpy(), gamma.numpy(), beta.numpy(), EPS)) if ln else (a64, b64)
    ref = np.zeros((a.shape[0], 8))
    ref[:, 0], ref[:, 1], ref[:, 2], ref[:, 3] = ((ah - bh) ** 2).sum(1), (bh ** 2).sum(1), (ah ** 2).sum(1), (ah * bh).sum(1)
    scale = np.abs(ref).copy()          # every sum to 1e-12 of itself (a sum that is exactly 0 must come out exactly 0) ...
    if with_t:
        t64 = t.numpy().astype(np.float64)
        ref[:, 4], ref[:, 5], ref[:, 6] = ((t64 - a64) ** 2).sum(1), ((t64 - b64) ** 2).sum(1), ((a64 - b64) * (t64 - b64)).sum(1)
        scale[:, 4], scale[:, 5] = ref[:, 4], ref[:, 5]
        scale[:, 6] = np.sqrt(((a64 - b64) ** 2).sum(1) * ref[:, 5])          # ... but the cancelling one: of ||a - b|| ||t - b||
    return ref, scale


def _run(a, b, t, gamma, beta, ln, with_t):
    mod = None
    if ln:
        mod = torch.nn.LayerNorm(a.shape[1], eps=EPS).to(DEV)
        with torch.no_grad():
            mod.weight.copy_(gamma)
            mod.bias.copy_(beta)
    out = hip.score_rows(a.to(DEV), b.to(DEV), t.to(DEV) if with_t else None, mod)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(got, ref, scale, what):
    worst = 0.0
    for k in range(8):
        e = np.abs(got[:, k] - ref[:, k])
        rel = float(np.max(e / np.where(scale[:, k] > 0, scale[:, k], 1.0)))
        worst = max(worst, rel)
        assert np.all(e <= TOL * scale[:, k]), (what, k, rel)
    print(f"[score_rows] {what}: worst relative error {worst:.3e} (bound {TOL:.0e})")


@pytest.mark.parametrize("with_t", [False, True])
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_rows_against_numpy_fp64(rows, cols, ln, with_t):
    a, b, t, gamma, beta = _inputs(rows, cols)
    got = _run(a, b, t, gamma, beta, ln, with_t)
    ref, scale = _ref(a, b, t, gamma, beta, ln, with_t)
    assert np.all(got[:, 7] == 0.0)
    if not with_t:
        assert np.all(got[:, 4:7] == 0.0)         # slots not asked for
    _check(got, ref, scale, f"{rows}x{cols} ln={ln} t={with_t}")


@pytest.mark.parametrize("ln", [False, True])
def test_identical_rows_give_exact_zeros(ln):
    a, _, t, gamma, beta = _inputs(5, 200)
    got = _run(a, a.clone(), t, gamma, beta, ln, True)
    assert np.all(got[:, 0] == 0.0) and np.all(got[:, 6] == 0.0)
    assert np.array_equal(got[:, 1], got[:, 2]) and np.array_equal(got[:, 4], got[:, 5])
    ref, scale = _ref(a, a, t, gamma, beta, ln, True)
    _check(got, ref, scale, f"a == b ln={ln}")


def _ulp_ref_slot0(a, b, gamma, beta):
    """||LayerNorm(a) - LayerNorm(b)||^2 per row by the definition in 40-digit arithmetic."""
    import mpmath as mp
    out = []
    with mp.workdps(40):
        eps = mp.mpf(float(np.float32(EPS)))
        for ra, rb in zip(a.numpy(), b.numpy()):
            hats = []
            for r in (ra, rb):
                x = [mp.mpf(float(v)) for v in r]
                m = mp.fsum(x) / len(x)
                var = mp.fsum((v - m) ** 2 for v in x) / len(x)
                rstd = 1 / mp.sqrt(var + eps)
                hats.append([(v - m) * rstd * mp.mpf(float(g)) + mp.mpf(float(e)) for v, g, e in zip(x, gamma.numpy(), beta.numpy())])
            out.append(float(mp.fsum((p - q) ** 2 for p, q in zip(*hats))))
    return np.array(out)


@pytest.mark.parametrize("ln", [False, True])
def test_b_one_ulp_from_a(ln):
    rows, cols = 5, 200
    a, _, t, gamma, beta = _inputs(rows, cols)
    b = torch.from_numpy(np.nextafter(a.numpy(), np.float32(np.inf)))
    assert not torch.equal(a, b)
    got = _run(a, b, t, gamma, beta, ln, True)
    ref, scale = _ref(a, b, t, gamma, beta, ln, True)
    if ln:
        ref[:, 0] = scale[:, 0] = _ulp_ref_slot0(a, b, gamma, beta)
    assert np.all(ref[:3, 0] > 0)          # (the constant and the zero row stay constant: their difference is an exact 0)
    _check(got, ref, scale, f"b = a + 1 ulp ln={ln}")


def test_row_strides_other_than_cols():
    rows, cols = 5, 200
    a, b, t, gamma, beta = _inputs(rows, cols, seed=3)
    wide = [torch.full((rows, cols + 4 * (i + 1)), 7.0) for i in range(3)]
    for w, x in zip(wide, (a, b, t)):
        w[:, :cols] = x
    da, db, dt = (w.to(DEV)[:, :cols] for w in wide)
    assert da.stride(0) == cols + 4 and db.stride(0) == cols + 8 and dt.stride(0) == cols + 12
    mod = torch.nn.LayerNorm(cols, eps=EPS).to(DEV)
    with torch.no_grad():
        mod.weight.copy_(gamma)
        mod.bias.copy_(beta)
    got = hip.score_rows(da, db, dt, mod).cpu().numpy()
    ref, scale = _ref(a, b, t, gamma, beta, True, True)
    _check(got, ref, scale, "strided rows")


@pytest.mark.parametrize("cols", [30, 2052, 0])
def test_bad_cols_is_an_error_status_and_launches_nothing(cols):
    lib = hip.load()
    buf = torch.ones(4, 2056, device=DEV)
    out = torch.full((4, 8), -3.0, dtype=torch.float64, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = lib.emcid_score_rows_f32(p(buf), 2056, p(buf), 2056, None, 0, None, None, 0.0, 4, cols, p(out),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1 and b"bad argument" in lib.emcid_last_error()
    assert bool((out == -3.0).all())
    with pytest.raises(hip.EmcidHipError):
        hip.score_rows(buf[:, :30], buf[:, :30])


def test_other_bad_arguments_are_an_error_status_and_launch_nothing():
    """gamma without beta, a row stride below cols, no nodes, no prompts: refused on the host, on real buffers."""
    lib = hip.load()
    buf = torch.ones(4, 2056, device=DEV)
    out = torch.full((4, 8), -3.0, dtype=torch.float64, device=DEV)
    anc, depth = torch.zeros(4, 8, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    ends = torch.zeros(1, dtype=torch.int64, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.emcid_score_rows_f32(p(buf), 2056, p(buf), 2056, None, 0, p(buf), None, 0.0, 4, 32, p(out), st) == -1
    assert lib.emcid_score_rows_f32(p(buf), 28, p(buf), 2056, None, 0, None, None, 0.0, 4, 32, p(out), st) == -1
    assert lib.emcid_score_chains_f64(p(out), 0, p(anc), 8, p(depth), p(ends), 1, p(out), st) == -1
    assert lib.emcid_score_chains_f64(p(out), 4, p(anc), 8, p(depth), p(ends), 0, p(out), st) == -1
    assert b"bad argument" in lib.emcid_last_error()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


# ---- chains ----------------------------------------------------------------------------------------------------------------------

def _chains_ref(node, anc, depth, ends):
    out = np.zeros((len(ends), 4))
    for p, e in enumerate(ends):
        chain = anc[e, :depth[e] + 1]
        num, den = node[chain, 0], node[chain, 1]
        r = np.where((num == 0) & (den == 0), 0.0, np.sqrt(num / np.where(den == 0, 1.0, den)))
        out[p] = r.max(), r.mean(), r[-1], int(np.argmax(r))        # (argmax: the first of equals)
    return out


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("longest", [2, 16, 17, 64, 65, 77, 128])
def test_chains_against_numpy(longest, B):
    rng = np.random.default_rng(100 + longest)
    U = longest + 60
    anc, depth = fr.random_trie(U, longest, rng)        # nodes 0 .. longest - 1 are one path; the others branch off it: shared prefixes
    node = rng.random((U, 8)) + 0.05
    node[:, 0] *= rng.random(U) * 4.0
    end_long = longest - 1
    node[0] = 0.0                                        # the root: both sums zero -> ratio 0 on every chain
    # a tie for the max on the longest chain: the same pair of sums at its last node and one before (its first position wins)
    tie = max(1, longest // 2)
    node[tie, :2] = node[end_long, :2] = (900.0, 0.25)
    ends = [end_long] + [int(x) for x in rng.integers(longest, U, size=B - 1)]
    got = hip.score_chains(torch.from_numpy(node).to(DEV), anc.to(DEV), depth.to(DEV), torch.tensor(ends, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    ref = _chains_ref(node, anc.numpy(), depth.numpy(), ends)
    assert ref[0, 0] == 60.0 and ref[0, 3] == min(tie, end_long) and depth[end_long] == longest - 1
    assert np.array_equal(got[:, 3], ref[:, 3])
    rel = np.abs(got[:, :3] - ref[:, :3]) / np.where(ref[:, :3] != 0, np.abs(ref[:, :3]), 1.0)
    print(f"[score_chains] longest {longest} B {B}: worst relative error {rel.max():.3e}")
    assert np.all(rel <= 1e-14)


def test_chains_of_all_zero_nodes_and_an_end_node_out_of_range():
    rng = np.random.default_rng(5)
    anc, depth = fr.random_trie(40, 9, rng)
    node = torch.zeros(40, 8, dtype=torch.float64, device=DEV)
    ends = torch.tensor([8, 40, 20], dtype=torch.int64, device=DEV)          # 40: not a node -> NaN, nothing read
    got = hip.score_chains(node, anc.to(DEV), depth.to(DEV), ends).cpu().numpy()
    assert np.array_equal(got[0], [0.0, 0.0, 0.0, 0.0]) and np.all(np.isnan(got[1])) and np.array_equal(got[2][:3], [0.0, 0.0, 0.0])

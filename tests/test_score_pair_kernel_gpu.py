"""emcid_score_pooled_f32 and emcid_score_chains_pair_f64 (include/emcid_hip.h, csrc/score.hip) through the binding, no encoder,
against numpy fp64 on the same fp32 inputs, at the bar tests/test_score_kernel_gpu.py holds the other two entry points to.

The bounds are derived, not measured.  Every input is converted exactly and every operation is an fp64 one.  A pooled slot is a sum
over the proj rows P_j of P of products of two dot products u_j = P_j . x, each a SIGNED sum of cols terms: its error is at most
g S_j(x), S_j(x) = sum_k |P_jk| |x_k|, with g the summation's constant — (cols / 64 + 6) 2^-53 < 4.3e-15 for a lane's chunk followed
by six shuffle steps — so a slot sum_j u_j v_j is good to g sum_j (|u_j| S_j(y) + |v_j| S_j(x)) plus the few roundings the
normalised rows carry.  The bound is 1e-12 of that scale (two orders left), which for slots 0-2 is never below the slot itself;
the error relative to the slot is printed beside it.  The kernel takes P a^ as P (a^ - b^) + P b^, so S_j(a^) is taken as
S_j(a^ - b^) + S_j(b^).  One case needs more than fp64 from the REFERENCE: with b one ulp from a, a^ - b^ formed from the two
normalised rows in fp64 carries their roundings in a difference of order 1e-7, whatever the kernel does — that case's a^ - b^ is
made in 40-digit arithmetic (mpmath) from the same fp32 inputs, as tests/test_score_kernel_gpu.py does.  The chain ratios are one
correctly rounded division and square root of a sum of two values: 1e-14, as there."""
import ctypes as C

import numpy as np
import pytest
import torch

import forward_refs as fr
from emcid_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
EPS = 1e-5
# (rows, cols, proj): the smallest call; a toy pair's own; the widest row; SDXL's TE2; more rows than one workgroup's four, ragged
SHAPES = [(1, 4, 1), (3, 48, 24), (2, 2048, 7), (5, 1280, 1280), (67, 48, 24)]


def _inputs(rows, cols, proj, seed=0):
    """(a, b, gamma, beta, P) fp32 on the CPU: a, b as tests/test_score_kernel_gpu.py draws them (forward_refs.trained_rows: rows
    riding on an offset of 500, one channel 1000 times the rest, a zero and a constant row; b an independent draw plus noise), P a
    projection with entries of order cols^-1/2."""
    a, gamma, beta = fr.trained_rows(rows, cols, seed=seed)
    g = torch.Generator().manual_seed(4242 + rows + cols + proj + seed)
    b = fr.trained_rows(rows, cols, seed=seed + 1)[0] + 0.1 * torch.randn(rows, cols, generator=g)
    P = torch.randn(proj, cols, generator=g) / cols ** 0.5
    return a, b, gamma, beta, P


def _ln64(x, gamma, beta):
    x = x.astype(np.float64)
    c = x - x.mean(axis=1, keepdims=True)
    return c / np.sqrt((c * c).mean(axis=1, keepdims=True) + np.float64(np.float32(EPS))) * gamma.astype(np.float64) + beta.astype(np.float64)


def _ref(a, b, gamma, beta, P, dh=None):
    """((rows, 4) fp64 by the definition, the bound's scale per slot).  ``dh``: a^ - b^ when fp64 cannot form it."""
    ah, bh = _ln64(a.numpy(), gamma.numpy(), beta.numpy()), _ln64(b.numpy(), gamma.numpy(), beta.numpy())
    dh = ah - bh if dh is None else dh
    P64 = P.numpy().astype(np.float64)
    u, v, w = dh @ P64.T, bh @ P64.T, ah @ P64.T
    Su, Sv = np.abs(dh) @ np.abs(P64).T, np.abs(bh) @ np.abs(P64).T
    Sw = Su + Sv
    ref = np.stack([(u * u).sum(1), (v * v).sum(1), (w * w).sum(1), (w * v).sum(1)], axis=1)
    scale = np.stack([2 * (np.abs(u) * Su).sum(1), 2 * (np.abs(v) * Sv).sum(1), 2 * (np.abs(w) * Sw).sum(1),
                      (np.abs(w) * Sv + np.abs(v) * Sw).sum(1)], axis=1)
    return ref, scale


def _ln_module(cols, gamma, beta):
    mod = torch.nn.LayerNorm(cols, eps=EPS).to(DEV)
    with torch.no_grad():
        mod.weight.copy_(gamma)
        mod.bias.copy_(beta)
    return mod


def _run(a, b, gamma, beta, P):
    out = hip.score_pooled(a.to(DEV), b.to(DEV), _ln_module(a.shape[1], gamma, beta), P.to(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(got, ref, scale, what):
    worst, worst_own = 0.0, 0.0
    for k in range(4):
        e = np.abs(got[:, k] - ref[:, k])
        worst = max(worst, float(np.max(e / np.where(scale[:, k] > 0, scale[:, k], 1.0))))
        worst_own = max(worst_own, float(np.max(e / np.where(ref[:, k] != 0, np.abs(ref[:, k]), 1.0))))
    print(f"[score_pooled] {what}: worst error {worst:.3e} of the scale (bound {TOL:.0e}), {worst_own:.3e} of the slot itself")
    for k in range(4):
        assert np.all(np.abs(got[:, k] - ref[:, k]) <= TOL * scale[:, k]), (what, k)


@pytest.mark.parametrize("rows,cols,proj", SHAPES)
def test_pooled_against_numpy_fp64(rows, cols, proj):
    a, b, gamma, beta, P = _inputs(rows, cols, proj)
    got = _run(a, b, gamma, beta, P)
    ref, scale = _ref(a, b, gamma, beta, P)
    _check(got, ref, scale, f"{rows}x{cols} proj {proj}")
    again = _run(a, b, gamma, beta, P)
    assert np.array_equal(got, again)                      # two calls: the same bits


def test_pooled_row_strides_other_than_cols():
    rows, cols, proj = 3, 48, 24
    a, b, gamma, beta, P = _inputs(rows, cols, proj, seed=3)
    wide = [torch.full((n, cols + 4 * (i + 1)), 7.0) for i, n in enumerate((rows, rows, proj))]
    for w, x in zip(wide, (a, b, P)):
        w[:, :cols] = x
    da, db, dP = (w.to(DEV)[:, :cols] for w in wide)
    assert da.stride(0) == cols + 4 and db.stride(0) == cols + 8 and dP.stride(0) == cols + 12
    got = hip.score_pooled(da, db, _ln_module(cols, gamma, beta), dP).cpu().numpy()
    ref, scale = _ref(a, b, gamma, beta, P)
    _check(got, ref, scale, "strided rows")


@pytest.mark.parametrize("rows,cols,proj", [(3, 48, 24), (67, 48, 24), (5, 1280, 1280)])
def test_pooled_identical_rows_give_an_exact_zero(rows, cols, proj):
    a, _, gamma, beta, P = _inputs(rows, cols, proj)
    got = _run(a, a.clone(), gamma, beta, P)
    assert np.all(got[:, 0] == 0.0)
    assert np.array_equal(got[:, 1], got[:, 2]) and np.array_equal(got[:, 1], got[:, 3])
    ref, scale = _ref(a, a, gamma, beta, P)
    _check(got, ref, scale, f"a == b {rows}x{cols} proj {proj}")


def _ulp_dhat(a, b, gamma, beta):
    """LayerNorm(a) - LayerNorm(b) per entry by the definition in 40-digit arithmetic, rounded once to fp64."""
    import mpmath as mp
    out = np.zeros(a.shape, dtype=np.float64)
    with mp.workdps(40):
        eps = mp.mpf(float(np.float32(EPS)))
        for r, (ra, rb) in enumerate(zip(a.numpy(), b.numpy())):
            hats = []
            for row in (ra, rb):
                x = [mp.mpf(float(v)) for v in row]
                m = mp.fsum(x) / len(x)
                var = mp.fsum((v - m) ** 2 for v in x) / len(x)
                rstd = 1 / mp.sqrt(var + eps)
                hats.append([(v - m) * rstd * mp.mpf(float(g)) + mp.mpf(float(e)) for v, g, e in zip(x, gamma.numpy(), beta.numpy())])
            out[r] = [float(p - q) for p, q in zip(*hats)]
    return out


def test_pooled_b_one_ulp_from_a():
    rows, cols, proj = 5, 48, 24
    a, _, gamma, beta, P = _inputs(rows, cols, proj)
    b = torch.from_numpy(np.nextafter(a.numpy(), np.float32(np.inf)))
    assert not torch.equal(a, b)
    got = _run(a, b, gamma, beta, P)
    ref, scale = _ref(a, b, gamma, beta, P, dh=_ulp_dhat(a, b, gamma, beta))
    assert np.all(ref[:3, 0] > 0)          # (the constant and the zero row stay constant: their difference is an exact 0)
    assert np.all(ref[:3, 0] < 1e-6 * ref[:3, 1])         # ... and the others' is tiny: the case that is meant
    _check(got, ref, scale, "b = a + 1 ulp")


def test_pooled_bad_arguments_are_an_error_status_and_launch_nothing():
    """cols % 4 != 0, cols = 2052, proj = 0, lda < cols, a pointer 4 bytes off: EMCID_ERR_BAD_ARG, ``out`` untouched."""
    lib = hip.load()
    buf = torch.ones(4, 2056, device=DEV)
    vec = torch.ones(2056, device=DEV)
    out = torch.full((4, 4), float("nan"), dtype=torch.float64, device=DEV)
    p = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(a=p(buf), lda=2056, b=p(buf), ldb=2056, P=p(buf), ldp=2056, rows=4, cols=32, proj=4, o=p(out)):
        return lib.emcid_score_pooled_f32(a, lda, b, ldb, p(vec), p(vec), 1e-5, P, ldp, rows, cols, proj, o, st)

    for kw in (dict(cols=30), dict(cols=2052), dict(cols=0), dict(proj=0), dict(lda=28), dict(ldp=28), dict(ldb=2058),
               dict(a=p(buf, 4)), dict(P=p(buf, 4)), dict(o=p(out, 8)), dict(rows=0)):
        assert call(**kw) == -1 and b"bad argument" in lib.emcid_last_error(), kw
    assert lib.emcid_score_pooled_f32(p(buf), 2056, p(buf), 2056, None, p(vec), 1e-5, p(buf), 2056, 4, 32, 4, p(out), st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0                                       # (the same call with nothing wrong runs)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    with pytest.raises(hip.EmcidHipError):
        hip.score_pooled(buf[:, :30], buf[:, :30], torch.nn.LayerNorm(30).to(DEV), buf[:, :30])
    with pytest.raises(hip.EmcidHipError, match="proj_weight"):
        hip.score_pooled(buf[:, :32], buf[:, :32], torch.nn.LayerNorm(32).to(DEV), buf[:, :36])


# ---- pair chains -----------------------------------------------------------------------------------------------------------------

def _renumbered(anc, depth, extra, rng):
    """The same trie under another numbering with ``extra`` more slots: (anc2, depth2, new index of every node).  The slots no
    node moves to are roots of their own; entries behind a chain's end are random valid indices, as forward_refs.random_trie's."""
    U, S = anc.shape
    U2 = U + extra
    new = rng.permutation(U2)[:U]
    anc2 = rng.integers(0, U2, size=(U2, S)).astype(np.int32)
    depth2 = np.zeros(U2, dtype=np.int32)
    anc2[:, 0] = np.arange(U2)
    for u in range(U):
        n = depth[u] + 1
        anc2[new[u], :n] = new[anc[u, :n]]
        depth2[new[u]] = depth[u]
    return anc2, depth2, new


def _pair_ref(node1, anc1, depth1, end1, node2, anc2, depth2, end2):
    out = np.zeros((len(end1), 4))
    for p, (e1, e2) in enumerate(zip(end1, end2)):
        c1, c2 = anc1[e1, :depth1[e1] + 1], anc2[e2, :depth2[e2] + 1]
        num, den = node1[c1, 0] + node2[c2, 0], node1[c1, 1] + node2[c2, 1]
        r = np.where((num == 0) & (den == 0), 0.0, np.sqrt(num / np.where(den == 0, 1.0, den)))
        out[p] = r.max(), r.mean(), r[-1], int(np.argmax(r))        # (argmax: the first of equals)
    return out


def _pair_setup(seed=11):
    """Two numberings of one random trie whose longest chain has 128 nodes (U1 = 188, U2 = 195), node sums for both, the root's
    four sums all zero, and the same ratio — the largest — at positions 64 and 127 of the longest chain."""
    rng = np.random.default_rng(seed)
    longest, U1 = 128, 188
    anc1, depth1 = (x.numpy() for x in fr.random_trie(U1, longest, rng))
    anc2, depth2, new = _renumbered(anc1, depth1, 7, rng)
    node1, node2 = rng.random((U1, 8)) + 0.05, rng.random((U1 + 7, 8)) + 0.05
    node1[:, 0] *= rng.random(U1) * 4.0
    node2[:, 0] *= rng.random(U1 + 7) * 4.0
    node1[0] = 0.0
    node2[new[0]] = 0.0
    for u in (64, 127):                                    # sqrt((600 + 300) / (0.125 + 0.125)) = 60 at both
        node1[u, :2] = (600.0, 0.125)
        node2[new[u], :2] = (300.0, 0.125)
    return rng, (node1, anc1, depth1), (node2, anc2, depth2), new


def _pair_run(t1, end1, t2, end2):
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(DEV)
    args = []
    for (node, anc, depth), end in ((t1, end1), (t2, end2)):
        args += [dev(node, torch.float64), dev(anc, torch.int32), dev(depth, torch.int32), dev(np.asarray(end), torch.int64)]
    a, b = hip.score_chains_pair(*args), hip.score_chains_pair(*args)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))          # two calls: the same bits, NaN included
    return a.cpu().numpy()


@pytest.mark.parametrize("B", [1, 5, 300])
def test_pair_chains_against_numpy(B):
    rng, t1, t2, new = _pair_setup()
    assert t1[0].shape[0] != t2[0].shape[0] and not np.array_equal(new, np.arange(len(new)))
    end1 = ([127, 0, 1, 76, 64] + [int(x) for x in rng.integers(0, 188, size=max(0, B - 5))])[:B]          # chains of 128, 1, 2, 77, 65 nodes
    end2 = [int(new[e]) for e in end1]
    got = _pair_run(t1, end1, t2, end2)
    ref = _pair_ref(*t1, end1, *t2, end2)
    assert ref[0, 0] == 60.0 and ref[0, 3] == 64 and ref[0, 2] == 60.0          # the tie: its first position
    if B >= 2:
        assert np.array_equal(got[1], [0.0, 0.0, 0.0, 0.0])                     # the root alone: all four sums zero -> r = 0
    assert np.array_equal(got[:, 3], ref[:, 3])
    rel = np.abs(got[:, :3] - ref[:, :3]) / np.where(ref[:, :3] != 0, np.abs(ref[:, :3]), 1.0)
    print(f"[score_chains_pair] B {B}: worst relative error {rel.max():.3e}")
    assert np.all(rel <= 1e-14)


def test_pair_chains_that_do_not_match_or_leave_a_trie_are_nan_for_that_prompt_only():
    rng, t1, t2, new = _pair_setup(seed=12)
    (node1, anc1, depth1), (node2, anc2, depth2) = t1, t2
    U1 = node1.shape[0]
    anc2 = anc2.copy()
    anc2[new[100], 1] = -1                                 # a chain entry of -1, in the row of node 100 only
    assert depth1[100] >= 1 and depth1[76] != depth1[77]
    end1 = [127, 76, U1, 100, 50, 150]
    end2 = [int(new[127]), int(new[77]), int(new[3]), int(new[100]), int(new[50]), node2.shape[0]]
    #        fine          lengths differ  end1 = U1     entry -1          fine          end2 = U2
    got = _pair_run(t1, end1, (node2, anc2, depth2), end2)
    for p in (1, 2, 3, 5):
        assert np.all(np.isnan(got[p])), p
    ref = _pair_ref(node1, anc1, depth1, [127, 50], node2, anc2, depth2, [end2[0], end2[4]])
    assert np.array_equal(got[[0, 4], 3], ref[:, 3])
    assert np.all(np.abs(got[[0, 4], :3] - ref[:, :3]) <= 1e-14 * np.abs(ref[:, :3]))


def test_pair_chains_bad_arguments_are_an_error_status_and_launch_nothing():
    lib = hip.load()
    out = torch.full((4, 8), float("nan"), dtype=torch.float64, device=DEV)
    anc, depth = torch.zeros(4, 8, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    ends = torch.zeros(1, dtype=torch.int64, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    one = (p(out), 4, p(anc), 8, p(depth), p(ends))
    assert lib.emcid_score_chains_pair_f64(*one, p(out), 0, p(anc), 8, p(depth), p(ends), 1, p(out), st) == -1
    assert lib.emcid_score_chains_pair_f64(*one, *one, 0, p(out), st) == -1
    assert lib.emcid_score_chains_pair_f64(*one, p(out), 4, p(anc), 0, p(depth), p(ends), 1, p(out), st) == -1
    assert lib.emcid_score_chains_pair_f64(*one, p(out), 4, p(anc), 8, None, p(ends), 1, p(out), st) == -1
    assert b"bad argument" in lib.emcid_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(hip.EmcidHipError, match="end nodes"):
        hip.score_chains_pair(out, anc, depth, ends, out, anc, depth, torch.zeros(2, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("longest", [2, 65, 128])          # 65: one position in a lane's second slot; 128: both slots of every lane
@pytest.mark.parametrize("B", [1, 5])
def test_single_chains_have_the_bits_of_pair_chains_with_a_zero_second_encoder(B, longest):
    """score_chains(node, ...) against score_chains_pair(node, ..., zeros_like(node) on the same trie, ...): the node sums are
    non-negative, so x + 0.0 == x exactly, and both kernels reduce through the same helpers — the same bits, the position of the
    max and the four NaN of a prompt whose end node is out of range included."""
    rng = np.random.default_rng(100 * B + longest)
    U = longest + 9
    anc, depth = fr.random_trie(U, longest, rng)
    node = rng.random((U, 8)) + 0.05
    node[:, 0] *= rng.random(U) * 4.0
    node[0] = 0.0                                           # the root: r = 0
    node[longest - 1, :2] = node[longest // 2, :2] = (600.0, 0.125)          # the largest ratio twice along the longest chain
    ends = ([longest - 1] + [int(x) for x in rng.integers(0, U, size=4)])[:B]
    if B > 1:
        ends[3] = U                                         # out of range: four NaN
    node_d = torch.from_numpy(node).to(DEV)
    trie = (anc.to(DEV), depth.to(DEV))
    for end in [ends] + ([[U], [-1]] if B == 1 else []):
        end_d = torch.tensor(end, dtype=torch.int64, device=DEV)
        single = hip.score_chains(node_d, *trie, end_d)
        pair = hip.score_chains_pair(node_d, *trie, end_d, torch.zeros_like(node_d), *trie, end_d)
        torch.cuda.synchronize()
        assert torch.equal(single.view(torch.int64), pair.view(torch.int64)), end
        bad = torch.tensor([not 0 <= e < U for e in end])
        assert bool(torch.isnan(single.cpu()[bad]).all()) and not bool(torch.isnan(single.cpu()[~bad]).any()), end
        if not bad[0]:
            assert float(single[0, 3]) == longest // 2 and float(single[0, 0]) == float(single[0, 2])       # the tie: its first position

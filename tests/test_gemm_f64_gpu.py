"""The fp64 MFMA GEMM (csrc/gemm_f64.h) against a plain fp64 host product, through every structure hint of emcid_dgemm_ex_f64:
triangular operands, lower-only, paired tiles, the three tile forms, even / fixed-run / automatic K splits, all four layouts, at
the smallest shapes where each path can still go wrong; then the batched entry point (with the split that shares blockIdx.z
with the batch) and the dW contraction with its fp32 epilogue.

The bound is derived, not measured (tests/gemm_f64_oracle.py: `expected`), and is element-wise:
    |got - ref| <= 2 (K + 4) 2^-53 (|alpha| (|a| |b|)[m, n] + |beta| |c0[m, n]|).
Run on the MI355X box:  python -m pytest tests/test_gemm_f64_gpu.py -m gpu -x -q"""
import time

import pytest
import torch

import gemm_f64_oracle as gx
from emcid_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
_TOTAL = {"cases": 0, "worst": 0.0, "where": None}


@pytest.fixture(scope="module", autouse=True)
def _summary():
    t0 = time.perf_counter()
    yield
    print(f"\n[gemm_f64] {_TOTAL['cases']} cases, largest |got - ref| / tol = {_TOTAL['worst']:.4f} at {_TOTAL['where']}, "
          f"{time.perf_counter() - t0:.1f} s")


def _note(ratio, where):
    _TOTAL["cases"] += 1
    if ratio > _TOTAL["worst"]:
        _TOTAL["worst"], _TOTAL["where"] = ratio, where


def _dev_view(x, t, extra=0):
    """x[rows][K] in layout t on the device, as the view of its true extent inside a NaN-padded buffer."""
    buf, c = gx.pack(x, t, extra)
    return buf.to(DEV)[:, :c]


def _same_bits(x, y):
    return torch.equal(x.view(torch.int64), y.view(torch.int64))


@pytest.mark.parametrize("ta,tb", gx.LAYOUTS)
@pytest.mark.parametrize("flags", gx.FLAGS)
def test_dgemm_ex_hints(flags, ta, tb):
    lower = bool(flags & gx.LOWER)
    worst, cases = 0.0, 0
    for shape in gx.shapes_for(flags, ta, tb):
        M, N, K = shape
        pr = gx.problem(M, N, K, flags & 15)
        pad = shape == (264, 264, 264)          # this shape runs with ld > extent for A, B and C
        Ad = _dev_view(pr.a, ta, 6 if pad else 0)
        Bd = _dev_view(pr.b.t(), tb, 10 if pad else 0)
        cextra = 3 if pad else 0
        want = {}
        for mode in gx.MODES:
            key = (mode.alpha, mode.beta)
            if key not in want:
                pre = gx.prefill(pr, mode)
                want[key] = (pre, gx.pack_c(pre, cextra).to(DEV)) + gx.expected(pr, mode.alpha, mode.beta)
        for cfg in gx.CFGS:
            for mode in gx.MODES:
                pre, pre_dev, ref, tol = want[(mode.alpha, mode.beta)]
                where = (shape, flags, (ta, tb), cfg, tuple(mode))
                Cd = pre_dev.clone()
                hip.dgemm_ex(ta, tb, Ad, Bd, Cd[:, :N], mode.alpha, mode.beta, flags, cfg, mode.ksplit)
                if not gx.may_split(mode, cfg, K):
                    C2 = pre_dev.clone()
                    hip.dgemm_ex(ta, tb, Ad, Bd, C2[:, :N], mode.alpha, mode.beta, flags, cfg, mode.ksplit)
                    assert _same_bits(Cd, C2), ("two runs differ", where)
                full = Cd.cpu()
                got = full[:, :N].contiguous()
                assert bool((full[:, N:] == gx.SENTINEL).all()), ("the padding of C was written", where)
                bad = gx.failures(got, pre, ref, tol, lower)
                ratio = gx.worst_ratio(got, ref, tol)
                print(where, f"ratio {ratio:.4f} bad {int(bad.sum())}")
                assert not bad.any(), (where, gx.describe(bad, got, pre, ref, tol))
                if mode.beta == 0.0 and not lower:
                    assert not torch.isnan(got).any(), where
                _note(ratio, where)
                worst, cases = max(worst, ratio), cases + 1
    print(f"flags {flags} layout ({ta}, {tb}): {cases} cases, largest |got - ref| / tol = {worst:.4f}")


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 1)])
def test_dgemm_big_tiles(ta, tb):
    """Plain hip.dgemm at 23 x 23 tiles of 128 x 128: the launcher itself picks the 8-wave form (no cfg is passed)."""
    M, N, K = gx.BIG_SHAPE
    pr = gx.make_problem(M, N, K, 0)
    alpha, beta = -0.5, 2.0
    ref, tol = gx.expected(pr, alpha, beta)
    Ad, Bd = _dev_view(pr.a, ta), _dev_view(pr.b.t(), tb)
    pre_dev = gx.pack_c(pr.c0, 2).to(DEV)
    runs = []
    for _ in range(2):
        Cd = pre_dev.clone()
        hip.dgemm(ta, tb, Ad, Bd, Cd[:, :N], alpha=alpha, beta=beta, M=M, N=N, K=K)
        runs.append(Cd)
    assert _same_bits(*runs)
    full = runs[0].cpu()
    got = full[:, :N].contiguous()
    assert bool((full[:, N:] == gx.SENTINEL).all())
    bad = gx.failures(got, pr.c0, ref, tol, False)
    ratio = gx.worst_ratio(got, ref, tol)
    print(f"big tiles ({ta}, {tb}): ratio {ratio:.4f} bad {int(bad.sum())}")
    assert not bad.any(), gx.describe(bad, got, pr.c0, ref, tol)
    _note(ratio, (gx.BIG_SHAPE, "dgemm", (ta, tb)))


def _batch_operand(x, t, shared, nb):
    """(nb, rows, cols) device view of the per-member operands x[b][rows][K] in layout t, with a batch stride larger than one
    matrix and ld larger than a row (NaN in between); `shared`: member 0 for everybody through a batch stride of 0."""
    src = x if t == 0 else x.transpose(1, 2)
    _, r, c = src.shape
    if shared:
        buf = torch.full((r + 1, c + c % 2 + 4), NAN, dtype=gx.F64)
        buf[:r, :c] = src[0]
        return buf.to(DEV)[:r, :c].unsqueeze(0).expand(nb, r, c)
    buf = torch.full((nb, r + 1, c + c % 2 + 4), NAN, dtype=gx.F64)
    buf[:, :r, :c] = src
    return buf.to(DEV)[:, :r, :c]


@pytest.mark.parametrize("ta,tb", [(0, 1), (1, 0)])
@pytest.mark.parametrize("M,N,K,alpha,beta", [(70, 50, 36, 0.75, -1.0), (40, 72, 272, -0.5, 1.0)])
def test_dgemm_batched_strided(ta, tb, M, N, K, alpha, beta):
    """Batch of 5, strides larger than the matrices, one operand shared.  At K = 272 with beta == 1 the launcher splits K, so
    blockIdx.z carries (batch, split): every member must receive its own product exactly once."""
    nb = 5
    g = torch.Generator().manual_seed(11 * M + K)
    a = torch.randn(nb, M, K, generator=g, dtype=gx.F64)
    b = torch.randn(nb, K, N, generator=g, dtype=gx.F64)
    c0 = torch.randn(nb, M, N, generator=g, dtype=gx.F64)
    share_a = ta == 1                       # A shared in layout (1, 0), B shared in layout (0, 1)
    if share_a: a = a[:1].expand(nb, M, K).contiguous()
    else: b = b[:1].expand(nb, K, N).contiguous()
    Ad = _batch_operand(a, ta, share_a, nb)
    Bd = _batch_operand(b.transpose(1, 2), tb, not share_a, nb)
    assert (Ad.stride(0) == 0) == share_a and (Bd.stride(0) == 0) == (not share_a)
    cbuf = torch.full((nb, M + 2, N + 3), gx.SENTINEL, dtype=gx.F64)
    cbuf[:, :M, :N] = c0
    Cd = cbuf.to(DEV)
    hip.dgemm_batched(ta, tb, Ad, Bd, Cd[:, :M, :N], alpha=alpha, beta=beta)
    full = Cd.cpu()
    keep = torch.ones(M + 2, N + 3, dtype=torch.bool)
    keep[:M, :N] = False
    assert bool((full[:, keep] == gx.SENTINEL).all()), "the padding of C was written"
    for i in range(nb):
        pr = gx.Problem(a[i], b[i], c0[i], a[i] @ b[i], a[i].abs() @ b[i].abs())
        ref, tol = gx.expected(pr, alpha, beta)
        got = full[i, :M, :N].contiguous()
        bad = gx.failures(got, c0[i], ref, tol, False)
        ratio = gx.worst_ratio(got, ref, tol)
        print(f"batched ({ta}, {tb}) {(M, N, K)} member {i}: ratio {ratio:.4f} bad {int(bad.sum())}")
        assert not bad.any(), (i, gx.describe(bad, got, c0[i], ref, tol))
        _note(ratio, ((M, N, K), "batched", (ta, tb), i))


@pytest.mark.parametrize("N,h,d", [(5, 6, 130), (37, 64, 384), (300, 48, 192)])
def test_delta_w(N, h, d):
    """W = fl32(W0 + fl32(Rt^T Xt)) with the product in fp64.  Another fp64 summation order can move the fp32 rounding of dW by
    one unit and the rounded sum by one more: 2 * 2^-23 * max(|W_ref|, |dW_ref|) element-wise."""
    g = torch.Generator().manual_seed(100 * N + h)
    Rt = torch.randn(N, h, generator=g, dtype=gx.F64)
    Xt = torch.randn(N, d, generator=g, dtype=gx.F64)
    W0 = torch.randn(h, d, generator=g, dtype=torch.float32)
    dW = (Rt.t() @ Xt).float()
    W_ref = W0 + dW
    tol = 2.0 * 2.0 ** -23 * torch.maximum(W_ref.abs(), dW.abs()).double()
    W0d = W0.to(DEV)
    Wd = torch.full((h, d), NAN, dtype=torch.float32, device=DEV)
    hip.delta_w_(Rt.to(DEV), Xt.to(DEV), W0d, Wd)
    got = Wd.cpu()
    assert torch.equal(W0d.cpu(), W0), "W0 was written"
    err = (got.double() - W_ref.double()).abs()
    print(f"delta_w {(N, h, d)}: largest error / tol = {float((err / tol).max()):.4f}")
    assert bool((err <= tol).all()), (int((~(err <= tol)).sum()), float(err.max()))

"""Oracle of the fp64 MFMA GEMM tests (csrc/gemm_f64.h through emcid_dgemm_ex_f64): the case lists, the host operands with their
promised zeros, the derived element-wise bound, the lower-only predicate, and a torch-fp64 stand-in of the kernel that walks the
same tiles, K ranges and splits.  test_gemm_f64_cpu.py checks the oracle against the stand-in and against mutants of it (no GPU);
test_gemm_f64_gpu.py checks the kernel with it."""
import functools
from collections import namedtuple

import torch

F64 = torch.float64
BK = 16                      # depth of a K tile
UNIT = 2.0 ** -53            # unit roundoff of fp64
SENTINEL = -1234.5625        # what the ld padding of C holds before and after a launch

LOWER, PAIR = 16, 32
FLAGS = (0, 1, 2, 4, 8, LOWER, 1 | 4, 2 | 8, 1 | PAIR, 2 | PAIR, 4 | PAIR, 8 | PAIR, PAIR, LOWER | PAIR)
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
CFGS = (-1, 0, 1, 2)
Mode = namedtuple("Mode", "alpha beta ksplit nan_prefill")
# the split counts: 7 is more than the K tiles of some output tile (empty splits); -1 / -3 are fixed runs of 1 / 3 K tiles
MODES = (Mode(1.0, 0.0, 0, True), Mode(0.5, -1.5, 0, False)) + tuple(Mode(-0.5, 1.0, ks, False) for ks in (0, 2, 3, 7, -1, -3))
TILE = {0: (128, 128), 1: (64, 64), 2: (32, 64)}
BIG_SHAPE = (2900, 2890, 34)         # 23 x 23 tiles of 128 x 128: the launcher's own choice is the 8-wave form


def shapes_for(flags, ta, tb):
    """(M, N, K) of the hinted GEMM for one (flags, layout)."""
    tri = flags & 15
    out = [(264, 264, 264), (256, 256, 256)]
    if flags in (0, LOWER):
        out.append((200, 136, 151))              # odd K; lower-only on a trapezoid
        if ta == 1 and tb == 1:
            out.append((201, 137, 150))          # odd extents along the contiguous (row) dimension of both operands
    if tri in (1, 2):
        out += [(72, 264, 144), (72, 136, 264)]  # triangular B with N > K (empty K ranges under bit 2) and with K > N
    if tri in (4, 8):
        out += [(264, 72, 144), (136, 72, 264)]  # the A-side mirror
    if flags == 0:
        out += [(1, 2, 4), (3, 2, 2)]
    return out


Problem = namedtuple("Problem", "a b c0 P Pabs")


def make_problem(M, N, K, tri):
    """a (M, K), b (K, N), c0 (M, N) from a seeded generator (asymmetric), the zeros that the `tri` bits promise really zero,
    and the dense fp64 products a b and |a| |b|."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    a = torch.randn(M, K, generator=g, dtype=F64)
    b = torch.randn(K, N, generator=g, dtype=F64)
    c0 = torch.randn(M, N, generator=g, dtype=F64)
    k = torch.arange(K)
    kb, nb = k[:, None], torch.arange(N)[None, :]
    ma, ka = torch.arange(M)[:, None], k[None, :]
    if tri & 1: b[kb > nb] = 0.0
    if tri & 2: b[kb < nb] = 0.0
    if tri & 4: a[ka > ma] = 0.0
    if tri & 8: a[ka < ma] = 0.0
    return Problem(a, b, c0, a @ b, a.abs() @ b.abs())


problem = functools.lru_cache(maxsize=None)(make_problem)


def expected(pr, alpha, beta):
    """ref = alpha a b + beta c0 and the bound 2 (K + 4) u (|alpha| |a| |b| + |beta| |c0|): gamma_K of a K-term dot product in
    any order, once for the kernel and once for the host product, plus the roundings of the axpby.  beta == 0 never reads C."""
    K = pr.a.shape[1]
    if beta == 0.0:
        ref, mag = alpha * pr.P, abs(alpha) * pr.Pabs
    else:
        ref, mag = alpha * pr.P + beta * pr.c0, abs(alpha) * pr.Pabs + abs(beta) * pr.c0.abs()
    return ref, 2.0 * (K + 4) * UNIT * mag


def prefill(pr, mode):
    return torch.full_like(pr.c0, float("nan")) if mode.nan_prefill else pr.c0.clone()


def pack(x, t, extra=0):
    """Storage of the operand whose logical form is x[rows][K]: t = 0 -> [rows][ld], t = 1 -> [K][ld]; ld is the contiguous
    extent rounded up to even plus `extra`, the padding is NaN.  Returns (buffer, contiguous extent)."""
    src = x if t == 0 else x.t()
    r, c = src.shape
    buf = torch.full((r, c + c % 2 + extra), float("nan"), dtype=F64)
    buf[:, :c] = src
    return buf, c


def pack_c(c, extra=0):
    buf = torch.full((c.shape[0], c.shape[1] + extra), SENTINEL, dtype=F64)
    buf[:, :c.shape[1]] = c
    return buf


def bits(x):
    return x.contiguous().view(torch.int64)


def classify(got, pre, ref, tol):
    """(within, untouched): |got - ref| <= tol (false for a NaN), and got bit-identical to its prefill value."""
    return (got - ref).abs() <= tol, bits(got) == bits(pre)


def strictly_upper(M, N):
    return torch.arange(M)[:, None] < torch.arange(N)[None, :]


def failures(got, pre, ref, tol, lower_only):
    """Mask of the elements that break the contract.  Every element must be within the bound; the one exemption is an element
    with m < n under lower_only, which may instead still hold its prefill bits."""
    within, untouched = classify(got, pre, ref, tol)
    ok = within | (untouched & strictly_upper(*got.shape)) if lower_only else within
    return ~ok


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol over the elements inside the bound (how far inside it the kernel sits; not a threshold)."""
    d = (got - ref).abs()
    r = torch.where((d <= tol) & (tol > 0), d / tol, torch.zeros_like(d))
    return float(r.max()) if r.numel() else 0.0


def describe(bad, got, pre, ref, tol):
    m, n = (int(v) for v in bad.nonzero()[0])
    return (f"{int(bad.sum())} elements outside the contract; first (m={m}, n={n}): got {got[m, n].item()!r}, ref {ref[m, n].item()!r}, "
            f"tol {tol[m, n].item():.3e}, prefill {pre[m, n].item()!r}")


def may_split(mode, cfg, K):
    """A launch whose partials may be added with atomics (no bit-reproducibility asked of it)."""
    return mode.beta == 1.0 and (mode.ksplit != 0 or (cfg != 0 and K >= 256))


# ---- torch stand-in of the kernel ------------------------------------------------------------------------------------

def _ceil(a, b):
    return -(-a // b)


def _tiles(M, N, bm, bn, lower):
    tm, tn = _ceil(M, bm), _ceil(N, bn)
    sq = min(tn * bn, tm * bm)
    return tm * tn - ((sq // bm) * (sq // bn) // 2 if lower else 0)


def resolve_cfg(M, N, cfg, ta, lower=False):
    if cfg < 0:
        cfg = 0 if _tiles(M, N, 128, 128, lower) >= 512 else (2 if ta == 0 else 1)
    return 1 if (cfg == 2 and ta != 0) else cfg


def _lower_tiles(gy, r, total):
    """Tiles of a lower-only square output from their linear id: row group q holds r rows of q + 1 tiles each."""
    for L in range(total):
        q = int(((8.0 * L / r + 1.0) ** 0.5 - 1.0) * 0.5)
        while r * (q + 1) * (q + 2) // 2 <= L: q += 1
        while r * q * (q + 1) // 2 > L: q -= 1
        rem = L - r * q * (q + 1) // 2
        yield r * q + rem // (q + 1), rem % (q + 1)


def standin(a, b, c, alpha, beta, flags=0, cfg=-1, ksplit=0, ta=0, mutant=None):
    """What the kernel computes, in torch fp64 on the host: per output tile of the chosen form, the 16-deep K tiles of the range
    that `tri` leaves, cut by ksplit (> 0: even split, < 0: fixed runs, 0: the launcher's own rule), partials of a split added in
    reverse order.  `mutant` plants one of the faults the oracle has to catch."""
    M, K = a.shape
    N = b.shape[1]
    tri, lower = flags & 15, bool(flags & LOWER)
    pair = bool(flags & PAIR) and tri != 0 and not lower
    cfg = resolve_cfg(M, N, cfg, ta, lower)
    BM, BN = TILE[cfg]
    KT = _ceil(K, BK)
    tm, tn = _ceil(M, BM), _ceil(N, BN)
    accum = beta == 1.0
    nsplit, kchunk = (ksplit, 0) if ksplit > 0 else (1, 0)
    if ksplit == 0 and accum and cfg != 0 and _tiles(M, N, BM, BN, lower) < 512 and KT >= 16:
        nsplit = max(1, min(_ceil(768, _tiles(M, N, BM, BN, lower)), KT // 8))
    if ksplit < 0:
        kchunk = -ksplit
        nsplit = _ceil(KT, kchunk) if accum else 1
        if nsplit == 1: kchunk = 0
    ap = torch.zeros(M, KT * BK, dtype=F64); ap[:, :K] = a
    bp = torch.zeros(KT * BK, N, dtype=F64); bp[:K] = b
    out = c.clone()
    kbits = tri
    if mutant == "swap_bits_1_2":
        kbits = (tri & 12) | ((tri & 1) << 1) | ((tri & 2) >> 1)

    # the product of every 16-deep K tile, once for the whole output where that fits (KT x M x N doubles), else per output tile
    whole = None
    if KT * M * N <= 1 << 22:
        whole = torch.bmm(ap.reshape(M, KT, BK).permute(1, 0, 2), bp.reshape(KT, BK, N))

    def ksum(ms, ns, s0, s1):
        if whole is not None:
            return whole[s0:s1, ms, ns].sum(0)
        A3 = ap[ms, s0 * BK:s1 * BK].reshape(-1, s1 - s0, BK).permute(1, 0, 2)
        B3 = bp[s0 * BK:s1 * BK, ns].reshape(s1 - s0, BK, -1)
        return torch.bmm(A3, B3).sum(0)

    def tile(bm, bn):
        m0, n0 = bm * BM, bn * BN
        if lower and n0 > m0 + BM - 1:
            return
        up = (lambda x: x // BK) if mutant == "tri_end_short" else (lambda x: _ceil(x, BK))
        t0, t1 = 0, KT
        if kbits & 1: t1 = min(t1, up(min(K, n0 + BN)))
        if kbits & 2: t0 = max(t0, min(n0, K) // BK + (1 if mutant == "tri_end_short" and bn == tn - 1 else 0))
        if kbits & 4: t1 = min(t1, up(min(K, m0 + BM)))
        if kbits & 8: t0 = max(t0, min(m0, K) // BK + (1 if mutant == "tri_end_short" and bm == tm - 1 else 0))
        if mutant == "drop_k_tile" and (bm, bn) == (1, 1) and t1 > t0:
            t1 -= 1
        ms, ns = slice(m0, min(M, m0 + BM)), slice(n0, min(N, n0 + BN))
        if nsplit == 1:
            v = alpha * ksum(ms, ns, t0, t1) if t1 > t0 else torch.zeros_like(out[ms, ns])
            new = v + beta * out[ms, ns] if beta != 0.0 else v
            if mutant == "transpose_tile" and (bm, bn) == (1, 0):
                new = new.t()
            out[ms, ns] = new
            return
        per = _ceil(t1 - t0, nsplit)
        wrong = torch.zeros_like(out[ms, ns])
        for zs in reversed(range(nsplit)):
            s0 = t0 + zs * (kchunk if kchunk else per)
            s1 = min(t1, s0 + (kchunk if kchunk else per))
            if s0 >= s1:
                continue
            part = alpha * ksum(ms, ns, s0, s1)
            if mutant == "beta_per_split":
                wrong += part + beta * c[ms, ns]
            else:
                out[ms, ns] += part
        if mutant == "beta_per_split":
            out[ms, ns] = wrong

    if pair:
        by_n = (tri & 3) != 0
        nt = tn if by_n else tm
        for j in range((nt + 1) // 2):
            first = nt - 1 - j if (tri & (1 if by_n else 4)) else j
            second = nt - 1 - first
            both = [first] + ([second] if second != first or mutant == "pair_middle_twice" else [])
            for other in range(tm if by_n else tn):
                for i in both:
                    tile(*((other, i) if by_n else (i, other)))
    elif lower and tri == 0 and M == N:
        r = BN // BM
        q, s = tm // r, tm % r
        total = r * q * (q + 1) // 2 + s * (q + 1)
        if mutant == "lower_tile_missing":
            total -= 1
        for bm, bn in _lower_tiles(tm, r, total):
            tile(bm, bn)
    else:
        for bm in range(tm):
            for bn in range(tn):
                tile(bm, bn)
    if mutant == "zero_upper_tile":
        bm, bn = next((i, j) for i in range(tm) for j in range(tn) if j * BN > i * BM + BM - 1)
        out[bm * BM:(bm + 1) * BM, bn * BN:(bn + 1) * BN] = 0.0
    return out

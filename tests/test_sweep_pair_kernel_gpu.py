"""emcid_score_chains_pair_grid_f64 (include/emcid_hip.h, csrc/score.hip) through the binding, no encoder.

PRIMARY: bitwise equality with ``hip.score_chains_pair`` called once per combination on the bank slices — the grid kernel states the
same operations in the same order.  SECONDARY: numpy fp64 at 1e-14, the figure tests/test_score_pair_kernel_gpu.py holds the pair
kernel to (a ratio is one correctly rounded division and square root of a sum of two values).  ``out`` is a window of a buffer
filled with a sentinel: nothing outside [C][B][4] may be written.

The tries are two numberings of ONE path 0 - 1 - ... - 128 (node u's chain is the u + 1 nodes 0 .. u) with spare nodes beside it:
U1 = 133 and ld_anc1 = 129, U2 = 140 and ld_anc2 = 136 (rows of a wider array), so end nodes 0, 63, 64, 127, 128 give chains of 1, 64,
65, 128 and 129 nodes — one lane, a full first half, the first lane of the second half, every lane twice, and one node too many.
Banks: G1 = 3, G2 = 2.  In every bank entry the path's root has all sums 0 (r = 0 there) and positions 64 and 127 share the largest
ratio, 60 (the first one must be reported).  GRID_CHUNK is 16 combinations per blockIdx.y: C = 17 runs a second one."""
import ctypes as C

import numpy as np
import pytest
import torch

from emcid_amd import hip
from test_score_pair_kernel_gpu import _pair_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATH, U1, U2, LD1, LD2, G1, G2 = 129, 133, 140, 129, 136, 3, 2
SENTINEL = -12345.0
PAD = 8          # doubles of sentinel on either side of ``out`` (64 bytes: the window stays 16-byte aligned)


def _tries(seed=5):
    """((anc1, depth1), (anc2 — a (U2, LD2) array, depth2), new: node u of trie 1 is node new[u] of trie 2)."""
    rng = np.random.default_rng(seed)
    new = rng.permutation(U2)[:U1]
    anc1 = rng.integers(0, U1, size=(U1, LD1)).astype(np.int32)          # (behind a chain's end: random valid indices)
    anc2 = rng.integers(0, U2, size=(U2, LD2)).astype(np.int32)
    depth1, depth2 = np.zeros(U1, dtype=np.int32), np.zeros(U2, dtype=np.int32)
    anc1[:, 0] = np.arange(U1)                                           # every node a root of its own ...
    anc2[:, 0] = np.arange(U2)
    for u in range(PATH):                                                # ... but the path's
        anc1[u, :u + 1] = np.arange(u + 1)
        anc2[new[u], :u + 1] = new[:u + 1]
        depth1[u] = depth2[new[u]] = u
    return (anc1, depth1), (anc2, depth2), new


def _banks(new, seed=6):
    rng = np.random.default_rng(seed)
    b1, b2 = rng.random((G1, U1, 8)) + 0.05, rng.random((G2, U2, 8)) + 0.05
    b1[:, :, 0] *= rng.random((G1, U1)) * 4.0
    b2[:, :, 0] *= rng.random((G2, U2)) * 4.0
    b1[:, 0] = 0.0
    b2[:, new[0]] = 0.0
    for u in (64, 127):                                                  # sqrt((600 + 300) / (0.125 + 0.125)) = 60 at both
        b1[:, u, :2] = (600.0, 0.125)
        b2[:, new[u], :2] = (300.0, 0.125)
    return b1, b2


def _dev(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(DEV)


def _run(t1, t2, b1, b2, end1, end2, combos):
    """(grid (C, B, 4), [score_chains_pair on the slices of combination c | None when c leaves a bank]) as numpy, after checking
    that nothing outside the window was written and that two launches give the same bits."""
    (anc1, depth1), (anc2, depth2) = t1, t2
    d_anc2 = _dev(anc2, torch.int32)
    wide = torch.zeros(U2, LD2 + 4, dtype=torch.int32, device=DEV)
    wide[:, :LD2] = d_anc2
    a1, a2 = _dev(anc1, torch.int32), wide[:, :LD2]                      # ld_anc2 = 140 != the 136 columns, != ld_anc1
    assert a2.stride(0) == LD2 + 4 and a1.stride(0) == LD1
    args1 = (a1, _dev(depth1, torch.int32), _dev(np.asarray(end1), torch.int64))
    args2 = (a2, _dev(depth2, torch.int32), _dev(np.asarray(end2), torch.int64))
    d1, d2 = _dev(b1, torch.float64), _dev(b2, torch.float64)
    n_c, B = len(combos), len(end1)
    combo = torch.tensor(combos, dtype=torch.int32, device=DEV).reshape(n_c, 2)
    outs = []
    for _ in range(2):
        big = torch.full((2 * PAD + n_c * B * 4,), SENTINEL, dtype=torch.float64, device=DEV)
        win = big[PAD:PAD + n_c * B * 4].view(n_c, B, 4)
        got = hip.score_chains_pair_grid(d1, *args1, d2, *args2, combo, out=win)
        torch.cuda.synchronize()
        assert got is win
        assert bool((big[:PAD] == SENTINEL).all()) and bool((big[PAD + n_c * B * 4:] == SENTINEL).all())
        assert not bool((win == SENTINEL).any())                         # ... and every entry inside it was
        outs.append(win.clone())
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))
    singles = []
    for g1, g2 in combos:
        ok = 0 <= g1 < G1 and 0 <= g2 < G2
        singles.append(hip.score_chains_pair(d1[g1], *args1, d2[g2], *args2).cpu().numpy() if ok else None)
    return outs[0].cpu().numpy(), singles


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _check(got, singles, combos, t1, t2, b1, b2, end1, end2, nan_prompts):
    (anc1, depth1), (anc2, depth2) = t1, t2
    fine = [p for p in range(len(end1)) if p not in nan_prompts]
    worst = 0.0
    for c, ((g1, g2), single) in enumerate(zip(combos, singles)):
        if single is None:
            assert np.all(np.isnan(got[c])), ("a combination outside the banks", c)
            continue
        assert np.array_equal(_bits(got[c]), _bits(single)), ("not the bits of score_chains_pair", c, g1, g2)          # PRIMARY
        for p in nan_prompts:
            assert np.all(np.isnan(got[c, p])), (c, p)
        if fine:
            ref = _pair_ref(b1[g1], anc1, depth1, [end1[p] for p in fine], b2[g2], anc2, depth2, [end2[p] for p in fine])
            assert np.array_equal(got[c, fine, 3], ref[:, 3]), c
            rel = np.abs(got[c, fine, :3] - ref[:, :3]) / np.where(ref[:, :3] != 0, np.abs(ref[:, :3]), 1.0)
            worst = max(worst, float(rel.max()))
            assert np.all(rel <= 1e-14), (c, rel.max())                                                                  # SECONDARY
    print(f"[score_chains_pair_grid] B {len(end1)} C {len(combos)}: worst relative error against numpy {worst:.3e}")


ENDS = [127, 0, 63, 64, 128]          # chains of 128, 1, 64, 65 and 129 nodes
ALL = [(g1, g2) for g1 in range(G1) for g2 in range(G2)]
COMBOS = {1: [(2, 1)], 3: [(0, 0), (2, 1), (1, 0)], 17: (ALL + ALL[::-1] + ALL)[:17]}


@pytest.mark.parametrize("B,n_c", [(1, 1), (1, 3), (5, 1), (5, 3), (5, 17)])
def test_grid_is_the_pair_kernel_per_combination(B, n_c):
    t1, t2, new = _tries()
    b1, b2 = _banks(new)
    end1 = ENDS[:B]
    end2 = [int(new[e]) for e in end1]
    combos = COMBOS[n_c]
    got, singles = _run(t1, t2, b1, b2, end1, end2, combos)
    _check(got, singles, combos, t1, t2, b1, b2, end1, end2, nan_prompts=[4] if B == 5 else [])
    for c in range(n_c):
        assert got[c, 0, 0] == 60.0 and got[c, 0, 3] == 64 and got[c, 0, 2] == 60.0          # the tie: its first position
        if B == 5:
            assert np.array_equal(got[c, 1], [0.0, 0.0, 0.0, 0.0])                            # the root alone: both sums 0 -> r = 0
            assert got[c, 2, 3] != 64 and got[c, 3, 3] == 64 and got[c, 3, 2] == 60.0          # 64 nodes end before the tie, 65 on it


def test_a_combination_outside_the_banks_is_nan_for_that_combination_only():
    t1, t2, new = _tries()
    b1, b2 = _banks(new)
    end1 = ENDS
    end2 = [int(new[e]) for e in end1]
    combos = [(0, 1), (G1, 0), (1, 1), (0, -1), (2, G2), (2, 0)] + ALL * 2          # 18: the bad ones in the first chunk, more behind it
    got, singles = _run(t1, t2, b1, b2, end1, end2, combos)
    assert [s is None for s in singles[:6]] == [False, True, False, True, True, False]
    _check(got, singles, combos, t1, t2, b1, b2, end1, end2, nan_prompts=[4])
    assert not np.isnan(got[[0, 2, 5]][:, :4]).any()


def test_a_bad_chain_is_nan_for_that_prompt_only():
    """A chain entry outside [0, U2) (in the row of path node 100 only), a pair of chains of different lengths, end nodes outside
    their tries: four NaN for that prompt in EVERY combination, the prompts beside them as the pair kernel gives them."""
    t1, (anc2, depth2), new = _tries()
    b1, b2 = _banks(new)
    anc2 = anc2.copy()
    anc2[new[100], 70] = U2                               # position 70: the second load of lane 6
    end1 = [127, 100, 50, 51, U1, 20, 90]
    end2 = [int(new[127]), int(new[100]), int(new[51]), int(new[51]), int(new[3]), -1, int(new[90])]
    #        fine           entry = U2      lengths differ  fine         end1 = U1    end2 = -1  fine
    combos = COMBOS[17]
    got, singles = _run(t1, (anc2, depth2), b1, b2, end1, end2, combos)
    _check(got, singles, combos, t1, (anc2, depth2), b1, b2, end1, end2, nan_prompts=[1, 2, 4, 5])
    assert not np.isnan(got[:, [0, 3, 6]]).any()


def test_bad_arguments_are_an_error_status_and_launch_nothing():
    lib = hip.load()
    out = torch.full((4, 8), float("nan"), dtype=torch.float64, device=DEV)
    bank = torch.ones(2, 4, 8, dtype=torch.float64, device=DEV)
    anc, depth = torch.zeros(4, 8, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    ends = torch.zeros(1, dtype=torch.int64, device=DEV)
    combo = torch.zeros(2, 2, dtype=torch.int32, device=DEV)
    p = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(node1=p(bank), G1_=2, U1_=4, node2=p(bank), G2_=2, U2_=4, B=1, cmb=p(combo), n_c=2, o=p(out), depth2=p(depth)):
        return lib.emcid_score_chains_pair_grid_f64(node1, G1_, U1_, p(anc), 8, p(depth), p(ends), node2, G2_, U2_, p(anc), 8, depth2,
                                                    p(ends), B, cmb, n_c, o, st)

    for kw in (dict(G1_=0), dict(G2_=0), dict(U1_=0), dict(U2_=-1), dict(B=0), dict(n_c=0), dict(node1=p(bank, 8)), dict(node2=p(bank, 8)),
               dict(o=p(out, 8)), dict(cmb=None), dict(node1=None), dict(o=None), dict(depth2=None)):
        assert call(**kw) == -1 and b"bad argument" in lib.emcid_last_error(), kw
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0                                       # (the same call with nothing wrong runs)
    torch.cuda.synchronize()
    assert bool((out.view(-1)[:8] == torch.tensor([1.0, 1.0, 1.0, 0.0] * 2, dtype=torch.float64, device=DEV)).all())          # [C = 2][B = 1][4]
    assert bool(torch.isnan(out.view(-1)[8:]).all())
    with pytest.raises(hip.EmcidHipError, match="combo"):
        hip.score_chains_pair_grid(bank, anc, depth, ends, bank, anc, depth, ends, combo.view(4))
    with pytest.raises(hip.EmcidHipError, match="G, U, 8"):
        hip.score_chains_pair_grid(bank[0], anc, depth, ends, bank, anc, depth, ends, combo)
    with pytest.raises(hip.EmcidHipError, match="end nodes"):
        hip.score_chains_pair_grid(bank, anc, depth, ends, bank, anc, depth, torch.zeros(2, dtype=torch.int64, device=DEV), combo)

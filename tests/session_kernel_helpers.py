"""Shared helpers of the kernel-level session tests (tests/test_session_kernel_gpu.py, _fold_kernel_gpu, _retain_kernel_gpu,
_release_kernel_gpu), which drive the entries of include/emcid_hip.h through the binding with no encoder: one seeded input recipe
(d = 384, h = 96, lam = 50, edit_weight 0.6, a few nearly collinear rows, Cov with a 1 600 condition number), the primal system in
fp64 on the CPU, and a retain list / a preserve step on one layer.  A plain module, imported by name like tests/gemm_f64_oracle.py."""
import functools
import math

import torch

from emcid_amd import hip

DEV = "cuda:0"
D, H, LAM, EW, LEFT = 384, 96, 50.0, 0.6, 2
# the bars of the existing fp64 solve-vs-oracle tests (tests/test_kernels_gpu.py): 1e-8 of the largest entry for an fp64 solve
# result (adj_k there; U, Yk here), 1e-9 for a Cholesky factor
U_BAR, L_BAR = 1e-8, 1e-9


@functools.lru_cache(maxsize=None)
def _inputs(total, d=D, seed=None):
    """`total` key rows (a few of them nearly collinear: inside the first step, the last row with two rows of the first step, and
    a later row with one of them), targets and statistics; computed once per (size, width, seed) and shared, never written.
    ``seed``: 1000 + total when None."""
    g = torch.Generator().manual_seed(1000 + total if seed is None else seed)
    K = torch.randn(total, d, generator=g) * 0.3
    K[1] = K[0] + 1e-4 * torch.randn(d, generator=g)
    K[total - 1] = K[0] * 0.5 + K[2] * 0.5 + 1e-4 * torch.randn(d, generator=g)
    if total > 140:
        K[135] = K[3] + 1e-4 * torch.randn(d, generator=g)
    Zc = torch.randn(total, H, generator=g)
    zs_t = torch.randn(total, H, generator=g)
    x = torch.randn(2 * d, d, generator=g) * torch.exp(torch.linspace(0, -3, d))
    Cov = (x.t() @ x) / (2 * d)
    W0 = torch.randn(H, d, generator=g) * 0.02
    return K, Zc, zs_t, Cov, W0


def _inputs_by_width(total, d=D):
    """The recipe with the width in the seed too (the retain and release tests)."""
    return _inputs(total, d, 1000 + total + d)


def _dev(t):
    return t.contiguous().to(DEV)


def _cp(Cov):
    return ((Cov * (1 - EW)) / 0.5).double()


def _scale(weight=1.0):
    return math.sqrt(weight * EW / 0.5)


def _scaled(K, Zc, zs_t):
    s = (EW / 0.5) ** 0.5
    return s * K.double(), (s * (zs_t - Zc).double()) / LEFT


def _primal_matrix(K, Zc, zs_t, Cov, hi):
    Kt, _ = _scaled(K, Zc, zs_t)
    return LAM * _cp(Cov) + Kt[:hi].t() @ Kt[:hi]


def _primal_u(K, Zc, zs_t, Cov, lo, hi):
    """U = Rt^T Kt (lam C' + P^T P + Kt^T Kt)^-1 for the step of rows [lo, hi) with rows [0, lo) preserved (in the system)."""
    Kt, Rt = _scaled(K, Zc, zs_t)
    return torch.linalg.solve(_primal_matrix(K, Zc, zs_t, Cov, hi), Kt[lo:hi].t() @ Rt[lo:hi]).t()


def _retain(K, fac, state, weight=1.0, commit=True):
    res = hip.session_retain(_dev(K), fac, 0, _scale(weight), state)
    flag = int(res["ws"].info.item())
    if commit and flag == 0:
        state.commit(K.shape[0], hip.row_scale_of(EW, fac, LAM, weight))
    return flag


def _step(K, Zc, zs_t, W0, fac, state):
    W = torch.empty(H, K.shape[1], dtype=torch.float32, device=DEV)
    res = hip.edit_layer_dual_preserve(_dev(K), _dev(Zc), _dev(zs_t), fac, 0, EW, LEFT, _dev(W0), W, state, want_u=True)
    assert int(res["ws"].info.item()) == 0
    res["W"] = W
    return res

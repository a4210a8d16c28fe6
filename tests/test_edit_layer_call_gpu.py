"""The one-call edited layer, emcid_clip_edit_layer_tail_sp16 (csrc/clip_layers.hip, reached through hip.clip_edit_layer_tail from
edit_engine.on_fc2), against fp64, stage by stage:

    f (fc2's input, fp32 twin) -> K = per-request means -> Zc = fc2(K) with the CURRENT weight -> both stages of the apply-only dual
    solve -> dW = float(U), W = W0 + dW -> the layer's own fc2 planes re-split from W, in place -> hs_out = fc2 + residual with the
    NEW planes -> the next layer's LN1 planes

Every stage is judged on ITS OWN inputs as the device holds them, so a failure names the stage (the convention of
test_dual_chain_gpu.py): K against the fp64 mean of the device's f, Zc against fp64 K_dev W0^T + b2, dW against the oracle's fp64 LU
on K_dev and Zc_dev, the planes against split_rows of the device's W, hs_out and the next LN1 against the fp64 layer
(forward_refs.clip_layer_ref) with fc2's weight replaced by the device's W.  tests/test_edit_layer_ref_cpu.py holds that reference
(forward_refs.edited_layer_ref) to a hooked Hugging Face forward whose weight was edited.

No bar is new.  K, Zc, hs_out and the planes: e_kernel <= 4 e_f32 + 2^-22 (forward_refs.assert_within_bar; hs_out over all rows and
over the plain rows, the planes per row: test_forward_kernels_gpu.test_clip_layer_tail).  dW, element by element:
|dW - U_ref| <= 2^-24 |U_ref| + t64, t64 = 8 max|U_woodbury - U_ref| + 4 eps64 Np max|Z^T| max|Yt X| (test_dual_chain_gpu._dw_bound), U_woodbury
the same closed form in torch fp64 in the Woodbury order.  Bitwise: K = hip.gather_mean, Zc (split) = hip.linear_sp on split_rows(K)
against the planes the layer held before the call, W = W0 + dW, planes = hip.split_rows(W), (hs, x) = hip.clip_layer_tail issued
afterwards on the same struct array.

The models are test_forward_kernels_gpu's (h64 / d160 quick_gelu, h96 / d224 erf-gelu: dp = 256, no linear workspace; h768 / d3072
with trained-like outliers: the d >= 2048 linear-workspace rule and few_rows_ksplit at dp >= 1024), the residual rows its
``trained_rows``, the trie its random trie.  Requests: 1 to 4 prompts each, lookup rows drawn with repetition from the trie's nodes,
one request whose prompts all name one row; N = 1, 40 (Np = 128), 130 (Np = 256: two leaves).  Statistics as test_kernels_gpu.
_edit_inputs at the model's d with a second layer's in the same factor_cov batch (the edited layer is index 1 of it), factored
at lam0 = lam / 0.4; edit_weight 0.6, layers_left 3, zs_t = Zc_ref + 0.5 randn.  lam is chosen on the host for cond(S) = 1e3, S = I +
Yt Yt^T as the device factors it (Np x Np, the identity on the padding rows — N < Np in every case, so its smallest eigenvalue is 1
and cond(S) = 1 + max eig(Yt Yt^T)), asserted within [10, 1e4]: the edit is neither negligible nor a conditioning test
(test_dual_chain_gpu owns that one).  Per case the fp64 reference computed with the OLD weight is asserted (on the CPU alone) to lie
more than 100 bars from the one with the new weight: a call whose fc2 still read the old planes cannot pass.

The call overwrites the layer's fc2 planes in place: every test clones them, passes W0 and W as clones of the weight, restores the
planes in a ``finally`` and asserts that they again equal hip.split_rows(original weight) bit for bit.

Every case runs on a NaN-poisoned DualWorkspace (test_dual_chain_gpu._poisoned_workspace): info == 0, the stream-K ticket counters
zero, everything read back finite.

Measured on MI355X (the run prints every line; EMCID_EDIT_CALL_TABLE names a file for them).  dW: max|U_woodbury - U_ref| /
max|dW - U_ref| / 2^-24 max|U_ref| + t64; the others e_kernel / e_f32 / bar:

    h64 N=1 stale weight against new, all rows: distance 2.504e-04  bar 3.718e-07  cond(S) 1.00e+03
    h64 N=1 stale weight against new, plain rows: distance 1.351e-02  bar 6.923e-07  cond(S) 1.00e+03
    h64 N=1 s1 i1 l0 K  e_kernel 6.401e-08  e_f32 6.401e-08  bar 4.945e-07
    h64 N=1 s1 i1 l0 Zc  e_kernel 1.613e-07  e_f32 1.128e-07  bar 6.896e-07
    h64 N=1 s1 i1 l0 dW  reference 2.012e-14  kernel 1.817e-09  allowed 5.086e-09
    h64 N=1 s1 i1 l0 hs_out  e_kernel 3.335e-08  e_f32 3.335e-08  bar 3.718e-07
    h64 N=1 s1 i1 l0 next LN1 planes  e_kernel 1.442e-06  e_f32 2.979e-06  bar 1.216e-05
    h64 N=40 stale weight against new, all rows: distance 3.790e-04  bar 4.857e-07  cond(S) 1.00e+03
    h64 N=40 stale weight against new, plain rows: distance 7.151e-03  bar 8.605e-07  cond(S) 1.00e+03
    h64 N=40 s1 i1 l0 K  e_kernel 8.405e-08  e_f32 8.405e-08  bar 5.746e-07
    h64 N=40 s1 i1 l0 Zc  e_kernel 2.453e-07  e_f32 4.472e-07  bar 2.027e-06
    h64 N=40 s1 i1 l0 dW  reference 1.502e-14  kernel 1.464e-08  allowed 2.724e-08
    h64 N=40 s1 i1 l0 hs_out  e_kernel 6.179e-08  e_f32 6.179e-08  bar 4.856e-07
    h64 N=40 s1 i1 l0 next LN1 planes  e_kernel 1.094e-06  e_f32 2.139e-06  bar 8.796e-06
    h64 N=130 stale weight against new, all rows: distance 2.102e-04  bar 4.328e-07  cond(S) 1.00e+03
    h64 N=130 stale weight against new, plain rows: distance 3.730e-03  bar 6.832e-07  cond(S) 1.00e+03
    h64 N=130 s0 i0 l0 K  e_kernel 7.005e-08  e_f32 7.005e-08  bar 5.186e-07
    h64 N=130 s0 i0 l0 Zc  e_kernel 4.245e-07  e_f32 4.628e-07  bar 2.090e-06
    h64 N=130 s0 i0 l0 dW  reference 1.729e-14  kernel 6.858e-09  allowed 1.276e-08
    h64 N=130 s0 i0 l0 hs_out  e_kernel 4.863e-08  e_f32 4.863e-08  bar 4.329e-07
    h64 N=130 s0 i0 l0 next LN1 planes  e_kernel 1.336e-06  e_f32 2.315e-06  bar 9.498e-06
    h64 N=40 s1 i1 l1 K  e_kernel 8.405e-08  e_f32 8.405e-08  bar 5.746e-07
    h64 N=40 s1 i1 l1 Zc  e_kernel 2.453e-07  e_f32 4.472e-07  bar 2.027e-06
    h64 N=40 s1 i1 l1 dW  reference 1.502e-14  kernel 1.464e-08  allowed 2.724e-08
    h96 N=1 stale weight against new, all rows: distance 1.548e-04  bar 3.637e-07  cond(S) 1.00e+03
    h96 N=1 stale weight against new, plain rows: distance 8.471e-04  bar 6.154e-07  cond(S) 1.00e+03
    h96 N=1 s1 i1 l0 K  e_kernel 3.747e-08  e_f32 3.747e-08  bar 3.883e-07
    h96 N=1 s1 i1 l0 Zc  e_kernel 2.190e-07  e_f32 2.068e-07  bar 1.066e-06
    h96 N=1 s1 i1 l0 dW  reference 5.271e-14  kernel 2.841e-09  allowed 5.014e-09
    h96 N=1 s1 i1 l0 hs_out  e_kernel 3.133e-08  e_f32 3.133e-08  bar 3.637e-07
    h96 N=1 s1 i1 l0 next LN1 planes  e_kernel 1.303e-06  e_f32 3.373e-06  bar 1.373e-05
    h96 N=40 stale weight against new, all rows: distance 3.512e-04  bar 3.681e-07  cond(S) 1.00e+03
    h96 N=40 stale weight against new, plain rows: distance 1.062e-02  bar 9.767e-07  cond(S) 1.00e+03
    h96 N=40 s1 i1 l0 K  e_kernel 6.444e-08  e_f32 6.444e-08  bar 4.962e-07
    h96 N=40 s1 i1 l0 Zc  e_kernel 3.228e-07  e_f32 4.620e-07  bar 2.086e-06
    h96 N=40 s1 i1 l0 dW  reference 1.776e-14  kernel 1.485e-08  allowed 2.511e-08
    h96 N=40 s1 i1 l0 hs_out  e_kernel 3.248e-08  e_f32 3.248e-08  bar 3.683e-07
    h96 N=40 s1 i1 l0 next LN1 planes  e_kernel 1.271e-06  e_f32 3.124e-06  bar 1.273e-05
    h96 N=130 stale weight against new, all rows: distance 2.967e-04  bar 4.300e-07  cond(S) 1.00e+03
    h96 N=130 stale weight against new, plain rows: distance 6.451e-03  bar 8.194e-07  cond(S) 1.00e+03
    h96 N=130 s0 i0 l0 K  e_kernel 6.713e-08  e_f32 6.713e-08  bar 5.069e-07
    h96 N=130 s0 i0 l0 Zc  e_kernel 6.053e-07  e_f32 4.483e-07  bar 2.032e-06
    h96 N=130 s0 i0 l0 dW  reference 1.302e-14  kernel 1.414e-08  allowed 1.719e-08
    h96 N=130 s0 i0 l0 hs_out  e_kernel 4.792e-08  e_f32 4.792e-08  bar 4.301e-07
    h96 N=130 s0 i0 l0 next LN1 planes  e_kernel 1.140e-06  e_f32 3.314e-06  bar 1.349e-05
    h96 N=40 s1 i1 l1 K  e_kernel 6.444e-08  e_f32 6.444e-08  bar 4.962e-07
    h96 N=40 s1 i1 l1 Zc  e_kernel 3.228e-07  e_f32 4.620e-07  bar 2.086e-06
    h96 N=40 s1 i1 l1 dW  reference 1.776e-14  kernel 1.485e-08  allowed 2.511e-08
    h768 N=40 stale weight against new, all rows: distance 4.329e-04  bar 3.818e-07  cond(S) 1.00e+03
    h768 N=40 stale weight against new, plain rows: distance 2.068e-02  bar 1.367e-06  cond(S) 1.00e+03
    h768 N=40 s1 i1 l0 K  e_kernel 5.128e-08  e_f32 5.128e-08  bar 4.435e-07
    h768 N=40 s1 i1 l0 Zc  e_kernel 3.807e-07  e_f32 3.617e-07  bar 1.685e-06
    h768 N=40 s1 i1 l0 dW  reference 6.595e-15  kernel 2.826e-09  allowed 3.741e-09
    h768 N=40 s1 i1 l0 hs_out  e_kernel 3.587e-08  e_f32 3.587e-08  bar 3.819e-07
    h768 N=40 s1 i1 l0 next LN1 planes  e_kernel 3.067e-05  e_f32 6.120e-05  bar 2.450e-04
    h768 N=40 s0 i1 l0 K  e_kernel 5.128e-08  e_f32 5.128e-08  bar 4.435e-07
    h768 N=40 s0 i1 l0 Zc  e_kernel 4.586e-07  e_f32 3.617e-07  bar 1.685e-06
    h768 N=40 s0 i1 l0 dW  reference 6.554e-15  kernel 2.735e-09  allowed 3.741e-09
    h768 N=40 s0 i1 l0 hs_out  e_kernel 3.587e-08  e_f32 3.587e-08  bar 3.819e-07
    h768 N=40 s0 i1 l0 next LN1 planes  e_kernel 3.049e-05  e_f32 6.131e-05  bar 2.455e-04
    h768 N=130 stale weight against new, all rows: distance 3.284e-04  bar 3.918e-07  cond(S) 1.00e+03
    h768 N=130 stale weight against new, plain rows: distance 1.376e-02  bar 1.416e-06  cond(S) 1.00e+03
    h768 N=130 s1 i1 l1 K  e_kernel 4.884e-08  e_f32 4.884e-08  bar 4.338e-07
    h768 N=130 s1 i1 l1 Zc  e_kernel 5.182e-07  e_f32 3.277e-07  bar 1.549e-06
    h768 N=130 s1 i1 l1 dW  reference 4.883e-15  kernel 1.859e-09  allowed 3.277e-09
    h64 N=40 sequence: layer 1 cond(S) 1.00e+03, lam / lam0 1.754e-01
    h64 N=40 sequence layer 1 K against the fp64 chain  e_kernel 2.434e-06  e_f32 4.897e-06  bar 1.983e-05
    h64 N=40 sequence layer 1 K  e_kernel 5.217e-08  e_f32 5.217e-08  bar 4.471e-07
    h64 N=40 sequence layer 1 Zc  e_kernel 2.219e-07  e_f32 3.682e-07  bar 1.711e-06
    h64 N=40 sequence layer 1 dW  reference 2.745e-14  kernel 1.709e-08  allowed 3.033e-08
    h96 N=40 sequence: layer 1 cond(S) 1.00e+03, lam / lam0 2.096e-01
    h96 N=40 sequence layer 1 K against the fp64 chain  e_kernel 3.998e-06  e_f32 5.743e-06  bar 2.321e-05
    h96 N=40 sequence layer 1 K  e_kernel 5.964e-08  e_f32 5.964e-08  bar 4.770e-07
    h96 N=40 sequence layer 1 Zc  e_kernel 3.437e-07  e_f32 3.100e-07  bar 1.478e-06
    h96 N=40 sequence layer 1 dW  reference 2.404e-14  kernel 2.516e-08  allowed 3.838e-08
    (s / i / l: zc_split / use_inverse / last.)
The keys and hs_out are the fp32 formula's own bits or within a rounding of it; dW's error is the fp32 rounding of U.

One stage missed its bar when this file was written, and the kernel was changed for it: Zc on the split-fp16 kernel at h768 read
e_kernel 1.269e-06 at N = 40 (bar 1.685e-06) and 1.589e-06 at N = 130 (e_f32 3.277e-07, bar 1.549e-06: red), against 4.6e-07 on the
exact-f32 kernel on the same keys.  The planes hold the operands to 7e-08 (emulated on the CPU: representation and the dropped
lo x lo product, summed exactly); the rest was the few-tile form's single fp32 accumulator over K = 3072, 576 MFMA roundings at its
full magnitude.  From K = 2048 on such launches now run the form that keeps the small products and the two k16 steps of a stage in
accumulators of their own (csrc/gemm_sp16.hip: sp_accumulate with SA, cfg 5; test_linear_sp16_few_tiles_sum_over_three_accumulators
below); the lines above are measured with it.  Below K = 2048 the one-accumulator form stays: taken everywhere, the other cost
bench.py 1 to 3 % per call.
"""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from emcid_amd import clip_forward as cf
from emcid_amd import hip
from oracle import emcid_oracle as orc

import forward_refs as fr
from test_dual_chain_gpu import _amax, _floor, _poisoned_workspace
from test_forward_kernels_gpu import MODELS, PLAIN_ROWS, U_D, _bar_all_and_plain, _Model
from test_kernels_gpu import _edit_inputs

DEV = "cuda:0"
EW, LEFT, RATIO, COND, NOISE = 0.6, 3, 0.4, 1e3, 0.5

_TABLE = []
_EDITED = {}


def _line(text):
    _TABLE.append(text)
    print(text)


def _bar(what, got, ref, fn32, per_row=False):
    """forward_refs.assert_within_bar, with the three figures kept for the table."""
    e_f = fr.f32_err(fn32, ref, per_row)
    _TABLE.append(f"{what:58s} e_kernel {fr.err(got, ref, per_row):9.3e}  e_f32 {e_f:9.3e}  bar {fr.FACTOR * e_f + fr.FLOOR:9.3e}")
    return fr.assert_within_bar("F", what, got, ref, fn32, per_row)


class _Edited:
    """One model of test_forward_kernels_gpu with what every case of it shares: the head of layer 0 on the device (mid, fc2's
    input with its fp32 twin — only ever read), the statistics of two layers and their fp64 Cholesky factors for the references."""

    def __init__(self, name):
        self.name = name
        m = self.m = _Model(name)
        assert m.nat is not None, "the native runner does not take this model: nothing below would run the call"
        self.h, self.d = m.h, m.d
        self.hs_d = m.hs.to(DEV)
        x0 = hip.add_layernorm_sp(self.hs_d, None, m.graph.layers[0].ln1)[1]
        self.mid, self.f = m.head(0, self.hs_d, x0)
        assert self.f.f32 is not None and self.f.f32.is_contiguous()
        cov = _edit_inputs(1, m.d, m.h, seed=m.d + m.h)[3]
        self.covs = [(cov * 1.5 + torch.eye(m.d) * 1e-3).contiguous(), cov]           # index 1: the edited layer's, as _row has it
        self.covs_d = [c.to(DEV) for c in self.covs]
        self.Lc = [torch.linalg.cholesky((c * (1 - EW) / 0.5).double().to(DEV)) for c in self.covs]
        self.cases = {}

    def fc2(self, i):
        return self.m.graph.layers[i].fc2

    def ln1_of(self, i):
        return self.m.graph.layers[i].ln1


@pytest.fixture(scope="module")
def em(request):
    """The three models, built once each (kept across the parametrised tests of this module whatever order they run in)."""
    if request.param not in _EDITED:
        _EDITED[request.param] = _Edited(request.param)
    return _EDITED[request.param]


@pytest.fixture(scope="module", autouse=True)
def _models_and_table():
    yield
    for e in _EDITED.values():
        cf.invalidate_weight_caches(e.m.model)
    _EDITED.clear()
    print("\n".join(_TABLE))
    path = os.environ.get("EMCID_EDIT_CALL_TABLE")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(_TABLE) + "\n")


@contextlib.contextmanager
def _planes_kept(em, i):
    """Layer i's fc2 planes and inverse scales, as the struct array points at them: cloned, handed to the body as (live, copy),
    put back whatever the body did, and then again split_rows(original weight) bit for bit."""
    lay = em.m.graph.layers[i]
    sp = lay.split_of("fc2")
    e = em.m.nat.array[i]
    assert e.fc2_planes == sp.planes.data_ptr() and e.fc2_inv_scale == sp.inv_scale.data_ptr()
    before = hip.SplitRows(sp.planes.clone(), sp.inv_scale.clone())
    w_before = lay.fc2.weight.detach().clone()
    try:
        yield sp, before
    finally:
        sp.planes.copy_(before.planes)
        sp.inv_scale.copy_(before.inv_scale)
        torch.cuda.synchronize()
    assert torch.equal(lay.fc2.weight.detach(), w_before), "a test wrote the model's own weight"
    want = hip.split_rows(lay.fc2.weight.detach())
    assert torch.equal(sp.planes, want.planes) and torch.equal(sp.inv_scale, want.inv_scale)


def _requests(N, n_rows, seed):
    """(lookup [B], seg [N + 1]) int64: 1 to 4 prompts per request, rows drawn with repetition; request N // 2 has three prompts
    that all name one row."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 5, size=N)
    j = N // 2
    counts[j] = 3
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    lookup = rng.integers(0, n_rows, size=int(seg[-1])).astype(np.int64)
    lookup[seg[j]:seg[j + 1]] = lookup[seg[j]]
    return torch.from_numpy(lookup), torch.from_numpy(seg)


def _lam_for(em, K64, cov_index, Np):
    """lam with cond(S) = COND for the keys K64 (fp64), and that cond(S) in fp64: S = I + Yt Yt^T on the Np x Np padded system."""
    s = math.sqrt(EW / 0.5)
    Y1 = torch.linalg.solve_triangular(em.Lc[cov_index], (K64.to(DEV) * s).T, upper=False).T
    ev = torch.linalg.eigvalsh(Y1 @ Y1.T).clamp_min(0.0)
    lam = ev[-1].item() / (COND - 1.0)
    N = K64.shape[0]
    assert N < Np
    eig_s = torch.cat([1.0 + ev / lam, torch.ones(Np - N, dtype=torch.float64, device=DEV)])
    cond = (eig_s.max() / eig_s.min()).item()
    assert 10.0 <= cond <= 1e4, cond
    return lam, cond


def _case(em, N):
    """Requests, targets, lam and the fp64 / fp32 CPU references of layer 0 for N requests (computed once, shared, never written)."""
    if N in em.cases:
        return em.cases[N]
    m = em.m
    lookup, seg = _requests(N, U_D, seed=1000 + 7 * em.h + N)
    W0, b2 = em.fc2(0).weight.detach().cpu(), em.fc2(0).bias.detach().cpu()
    mid_ref, f_ref, hs_old = m.layer_ref(0)
    mid32, f32_, _ = m.layer_ref(0, dtype=torch.float32)
    K_ref = fr.request_means(f_ref, lookup, seg)
    Zc_ref = K_ref @ W0.double().T + b2.double()
    g = torch.Generator().manual_seed(2000 + em.h + N)
    zs_t = (Zc_ref + NOISE * torch.randn(N, em.h, generator=g, dtype=torch.float64)).float()
    Np = -(-N // 128) * 128
    lam, cond = _lam_for(em, K_ref, 1, Np)
    ln1 = m.w[1]["ln1"]
    ref = fr.edited_layer_ref(f_ref, mid_ref, lookup, seg, W0, b2, zs_t, em.covs[1], lam, EW, LEFT, ln1)
    ref32 = fr.edited_layer_ref(f32_, mid32, lookup, seg, W0, b2, zs_t, em.covs[1], lam, EW, LEFT, ln1, dtype=torch.float32)
    assert torch.equal(ref[0], K_ref) and torch.equal(ref[1], Zc_ref)
    # the discriminating assert, on the CPU references alone: the layer with the OLD weight lies more than 100 bars from the one
    # with the new weight, over all rows and over the plain rows (the two bars hs_out is held to)
    for what, rows in (("all rows", slice(None)), ("plain rows", PLAIN_ROWS)):
        bar = fr.FACTOR * fr.err(ref32[3][rows], ref[3][rows]) + fr.FLOOR
        dist = fr.err(hs_old[rows], ref[3][rows])
        _line(f"h{em.h} N={N} stale weight against new, {what}: distance {dist:9.3e}  bar {bar:9.3e}  cond(S) {cond:8.2e}")
        assert dist > 100.0 * bar, f"h{em.h} N={N} {what}: a stale weight is only {dist / bar:.1f} bars away"
    c = dict(N=N, Np=Np, lookup=lookup, seg=seg, zs_t=zs_t, lam=lam, lam0=lam / RATIO, cond=cond, ref=ref, W0=W0, b2=b2,
             lookup_d=lookup.to(DEV), seg_d=seg.to(DEV), zs_t_d=zs_t.to(DEV))
    em.cases[N] = c
    return c


def _finite(x, case, what):
    assert bool(torch.isfinite(x).all()), f"{case}: {what} holds a value no stage wrote (NaN poison) or a non-finite result"


def _check_k_zc(case, f, lookup, seg, W0_d, b2_d, out, zc_split, planes_before):
    """Items 1 and 2: K on the device's f, Zc on the device's K and the weight the call was given."""
    K, Zc = out["K"], out["Zc"]
    _finite(K, case, "K")
    _finite(Zc, case, "Zc")
    B = lookup.numel()
    assert torch.equal(K, hip.gather_mean(f.f32.unsqueeze(0).expand(B, -1, -1), lookup.to(DEV), seg.to(DEV))), f"{case}: stage K"
    f_cpu = f.f32.cpu()
    _bar(f"{case} K", K, fr.request_means(f_cpu, lookup, seg), lambda: fr.request_means(f_cpu, lookup, seg, torch.float32))
    K_cpu, W0c, b2c = K.cpu(), W0_d.cpu(), b2_d.cpu()
    _bar(f"{case} Zc", Zc, K_cpu.double() @ W0c.double().T + b2c.double(), lambda: F.linear(K_cpu, W0c, b2c))
    if zc_split:
        assert torch.equal(Zc, hip.linear_sp(hip.split_rows(K), planes_before, b2_d)), f"{case}: stage Zc: not fc2 of the keys' planes"


def _check_dw(case, em, cov_index, out, zs_t, lam, left, ws, fac, fac_layer, use_inverse, W0_d, W0_before, W_d):
    """Items 3 and 4: dW element by element against the oracle's fp64 LU on the device's K and Zc; W = W0 + dW; W0 untouched."""
    K, Zc, dW = out["K"], out["Zc"], out["dW"]
    N, d = K.shape
    h = Zc.shape[1]
    assert int(ws.info.item()) == 0, f"{case}: info {int(ws.info.item())}"
    assert int(ws.sk_counters.view(torch.int64).count_nonzero()) == 0, f"{case}: stream-K ticket counters not left zero"
    _finite(dW, case, "dW")
    _finite(W_d, case, "W")
    RT, Yt = ws.RT[:h], ws.Yt
    _finite(RT, case, "RT = Z^T")
    _finite(Yt, case, "Yt")
    _, resid, upd = orc.closed_form_layer(K.cpu(), Zc.cpu(), zs_t.t(), em.covs[cov_index], lam, EW, left)
    U_ref = upd.to(DEV)
    # the same closed form in torch fp64 in the Woodbury order, on the same K and Zc: the reference's own error
    s, Lc = math.sqrt(EW / 0.5), em.Lc[cov_index]
    Yw = torch.linalg.solve_triangular(Lc, (K.double() * s).T, upper=False).T / math.sqrt(lam)
    Sw = torch.eye(N, dtype=torch.float64, device=DEV) + Yw @ Yw.T
    Zw = torch.cholesky_solve(resid.t().contiguous().to(DEV), torch.linalg.cholesky(Sw))
    U_wood = torch.linalg.solve_triangular(Lc.T * math.sqrt(lam), (Zw.T @ Yw).T, upper=True).T
    wood_err = _amax(U_wood - U_ref)
    if use_inverse:
        Xc = torch.tril(fac.X(fac_layer))
    else:       # (never built; the floor takes its magnitude from torch's)
        Xc = torch.linalg.solve_triangular(torch.tril(fac.L(fac_layer)), torch.eye(fac.dp, dtype=torch.float64, device=DEV), upper=False)
    t64 = 8.0 * wood_err + _floor(RT.shape[1], RT, Yt @ Xc)
    bound = 2.0 ** -24 * U_ref.abs() + t64
    over = ((dW.double() - U_ref).abs() - bound).max().item()
    _line(f"{case + ' dW':58s} reference {wood_err:9.3e}  kernel {_amax(dW.double() - U_ref):9.3e}  "
          f"allowed {2.0 ** -24 * _amax(U_ref) + t64:9.3e}")
    assert over <= 0.0, f"{case}: stage dW: an entry is {over:.3e} beyond 2^-24 |U_ref| + t64 (t64 {t64:.3e}, max|U_ref| {_amax(U_ref):.3e})"
    assert torch.equal(W_d, W0_d + dW), f"{case}: stage W: W != W0 + dW"
    assert torch.equal(W0_d, W0_before), f"{case}: W0 was written"


def _run_layer0(em, N, zc_split, use_inverse, last, monkeypatch=None):
    """Layer 0 through the call, items 1 to 6."""
    c = _case(em, N)
    m, n = em.m, em.m.nat
    case = f"h{em.h} N={N} split={int(zc_split)} inv={int(use_inverse)} last={int(last)}"
    fac = hip.factor_cov(em.covs_d, c["lam0"], EW, inverse=use_inverse)
    assert (1 in fac.have_inverse) == use_inverse
    ws = _poisoned_workspace(N, em.d, em.h)
    lws_seen = []
    if monkeypatch is not None:
        real = hip._linear_workspace
        monkeypatch.setattr(hip, "_linear_workspace", lambda dev: lws_seen.append(real(dev)) or lws_seen[-1])
    next_ln = em.ln1_of(1)
    with _planes_kept(em, 0) as (sp, before):
        W0_d = em.fc2(0).weight.detach().clone()
        W_d, W0_before = W0_d.clone(), W0_d.clone()
        mid_before = em.mid.clone()
        out = hip.clip_edit_layer_tail(n.array, 0, n.h, n.d, em.f, em.mid, c["lookup_d"], c["seg_d"], c["zs_t_d"], fac, 1, EW, LEFT,
                                       W0_d, W_d, ws, c["lam"], next_ln, last=last, zc_split=zc_split)
        torch.cuda.synchronize()
        assert int(fac.info.item()) == 0
        if monkeypatch is not None:
            assert (len(lws_seen) == 1 and lws_seen[0] is not None and lws_seen[0].numel() > 0) == (em.d >= 2048), \
                f"{case}: the linear workspace was {'not ' if not lws_seen else ''}passed"
        _check_k_zc(case, em.f, c["lookup"], c["seg"], W0_before, em.fc2(0).bias.detach(), out, zc_split, before)
        _check_dw(case, em, 1, out, c["zs_t"], c["lam"], LEFT, ws, fac, 1, use_inverse, W0_d, W0_before, W_d)
        assert torch.equal(em.mid, mid_before)
        if last:
            # item 5, last: nothing of the forward is touched, nothing of it comes back
            assert torch.equal(sp.planes, before.planes) and torch.equal(sp.inv_scale, before.inv_scale), f"{case}: planes written"
            assert out["hs"] is None and out["x"] is None
            return
        # item 5: the layer's own planes are those of the new weight
        want = hip.split_rows(W_d)
        assert torch.equal(sp.planes, want.planes) and torch.equal(sp.inv_scale, want.inv_scale), f"{case}: stage planes"
        # item 6: fc2 + residual with the new planes and the next LN1, against the fp64 layer under the device's new W
        hs, x = out["hs"], out["x"]
        _finite(hs, case, "hs_out")
        xf = fr.sp_float(x.planes, x.inv_scale)
        _finite(xf, case, "next LN1 planes")
        Wn = W_d.cpu()
        mid_ref, f_ref, _ = m.layer_ref(0)
        mid32, f32_, _ = m.layer_ref(0, dtype=torch.float32)
        hs_ref = f_ref @ Wn.double().T + c["b2"].double() + mid_ref
        hs32 = F.linear(f32_, Wn, c["b2"]) + mid32
        _TABLE.append(f"{case + ' hs_out':58s} e_kernel {fr.err(hs, hs_ref):9.3e}  e_f32 {fr.err(hs32, hs_ref):9.3e}  "
                      f"bar {fr.FACTOR * fr.err(hs32, hs_ref) + fr.FLOOR:9.3e}")
        _bar_all_and_plain(f"{case} hs_out", hs, hs_ref, hs32)
        ln1 = m.w[1]["ln1"]
        _bar(f"{case} next LN1 planes", xf, m.ln(ln1, hs_ref), lambda: m.ln(ln1, hs32, torch.float32), per_row=True)
        hs2, x2 = hip.clip_layer_tail(n.array, 0, n.h, n.d, em.f, em.mid, next_ln)
        assert torch.equal(hs, hs2) and torch.equal(x.planes, x2.planes) and torch.equal(x.inv_scale, x2.inv_scale), \
            f"{case}: not the tail's own launches on the new planes"


SMALL = [(name, N, split, inv, last) for name in ("h64", "h96")
         for N, split, inv, last in ((1, True, True, False), (40, True, True, False), (130, False, False, False), (40, True, True, True))]
LARGE = [("h768", 40, True, True, False), ("h768", 40, False, True, False), ("h768", 130, True, True, True)]
assert set(MODELS) == {"h64", "h96", "h768"}


@pytest.mark.parametrize("em,N,zc_split,use_inverse,last", SMALL + LARGE, indirect=["em"])
def test_edited_layer_call_stage_by_stage(em, N, zc_split, use_inverse, last, monkeypatch):
    """Items 1 to 6 of the module docstring on layer 0.  zc_split = False: Zc on the exact-f32 kernel against W (at d >= 2048 with
    the linear workspace, which is asserted to have been handed over; below, asserted absent); use_inverse = False: the factors
    without X = inv(L); last = True: the planes, their scales and mid bit-identical afterwards, hs and x None."""
    _run_layer0(em, N, zc_split, use_inverse, last, monkeypatch)


@pytest.mark.parametrize("em", ["h64", "h96"], indirect=True)
def test_two_edited_layers_in_sequence(em):
    """Layer 0 through the call (not last), its (hs, x) into the head of layer 1 on an unsorted row selection with a repeated
    index, layer 1 through the call with last = True and ``lookup`` indexing the SELECTED rows.  Layer 1's keys against
    clip_layer_ref of layer 1 fed with the fp64 output of layer 0 under the device's edited weight (bar from the fp32 eager chain of
    the same two layers); its Zc and dW by items 2 and 3 on the device's own K and Zc.  The selection holds every node but one
    (that no prompt names) and one node twice, so every row index a prompt can name, as a node or as a query row, lies inside f."""
    N = 40
    c = _case(em, N)
    m, n = em.m, em.m.nat
    case = f"h{em.h} N={N} sequence"
    lookup, seg = c["lookup"], c["seg"]
    rng = np.random.default_rng(3000 + em.h)
    named = set(lookup.tolist())
    drop = next(u for u in range(U_D - 3, 0, -1) if u not in named)
    dup = int(lookup[0])
    order = [int(u) for u in rng.permutation(U_D) if u != drop]
    order.insert(int(rng.integers(0, len(order))), dup)
    rows_sel = torch.tensor(order, dtype=torch.int32)
    assert rows_sel.numel() == U_D and sorted(order) != order and order.count(dup) == 2
    where = {}
    for q, u in enumerate(order):
        where.setdefault(u, []).append(q)
    lookup_q = torch.tensor([where[int(u)][b % len(where[int(u)])] for b, u in enumerate(lookup)], dtype=torch.int64)
    assert bool((rows_sel[lookup_q].long() == lookup).all()) and not torch.equal(lookup_q, lookup)
    fac = hip.factor_cov(em.covs_d, c["lam0"], EW)
    with _planes_kept(em, 0) as (sp0, before0), _planes_kept(em, 1) as (sp1, before1):
        W0a = em.fc2(0).weight.detach().clone()
        Wa = W0a.clone()
        out0 = hip.clip_edit_layer_tail(n.array, 0, n.h, n.d, em.f, em.mid, c["lookup_d"], c["seg_d"], c["zs_t_d"], fac, 1, EW, LEFT,
                                        W0a, Wa, _poisoned_workspace(N, em.d, em.h), c["lam"], em.ln1_of(1), last=False)
        mid1, f1 = m.head(1, out0["hs"], out0["x"], rows_sel)
        torch.cuda.synchronize()
        # layer 1's references: the fp64 (fp32) layer 0 under the device's new weight, then clip_layer_ref of layer 1
        Wn = Wa.cpu()
        mid_ref, f_ref, _ = m.layer_ref(0)
        mid32, f32_, _ = m.layer_ref(0, dtype=torch.float32)
        hs0_ref = f_ref @ Wn.double().T + c["b2"].double() + mid_ref
        hs0_32 = F.linear(f32_, Wn, c["b2"]) + mid32
        f1_ref = fr.clip_layer_ref(m.w[1], hs0_ref, m.anc, m.depth, rows_sel)[1]
        f1_32 = fr.clip_layer_ref(m.w[1], hs0_32, m.anc, m.depth, rows_sel, torch.float32)[1]
        K1_ref = fr.request_means(f1_ref, lookup_q, seg)
        W1, b1 = em.fc2(1).weight.detach(), em.fc2(1).bias.detach()
        Zc1_ref = K1_ref @ W1.cpu().double().T + b1.cpu().double()
        g = torch.Generator().manual_seed(4000 + em.h)
        zs_t1 = (Zc1_ref + NOISE * torch.randn(N, em.h, generator=g, dtype=torch.float64)).float()
        lam1, cond1 = _lam_for(em, K1_ref, 0, c["Np"])
        ws1 = _poisoned_workspace(N, em.d, em.h)
        W0b = W1.clone()
        Wb, W0b_before = W0b.clone(), W0b.clone()
        mid1_before = mid1.clone()
        out1 = hip.clip_edit_layer_tail(n.array, 1, n.h, n.d, f1, mid1, lookup_q.to(DEV), c["seg_d"], zs_t1.to(DEV), fac, 0, EW, LEFT - 1,
                                        W0b, Wb, ws1, lam1, None, last=True)
        torch.cuda.synchronize()
        assert int(fac.info.item()) == 0
        _line(f"{case}: layer 1 cond(S) {cond1:8.2e}, lam / lam0 {lam1 / c['lam0']:.3e}")
        _bar(f"{case} layer 1 K against the fp64 chain", out1["K"], K1_ref, lambda: fr.request_means(f1_32, lookup_q, seg, torch.float32))
        _check_k_zc(case + " layer 1", f1, lookup_q, seg, W0b_before, b1, out1, True, before1)
        _check_dw(case + " layer 1", em, 0, out1, zs_t1, lam1, LEFT - 1, ws1, fac, 0, True, W0b, W0b_before, Wb)
        assert out1["hs"] is None and out1["x"] is None and torch.equal(mid1, mid1_before)
        assert torch.equal(sp1.planes, before1.planes) and torch.equal(sp1.inv_scale, before1.inv_scale), f"{case}: layer 1's planes written"
        want = hip.split_rows(Wa)
        assert torch.equal(sp0.planes, want.planes) and torch.equal(sp0.inv_scale, want.inv_scale), f"{case}: layer 0's planes"


# ---- refusals: before anything is launched ------------------------------------------------------------------------------------------

def _raw_call(em, a):
    """The C entry itself with the arguments of ``a`` (hip.clip_edit_layer_tail assembles the same list): (rc, message)."""
    p = hip._ptr
    rc = hip.load().emcid_clip_edit_layer_tail_sp16(
        C.c_void_p(C.addressof(em.m.nat.array)), a["n"], a["h"], a["d"], p(a["f_f32"]), p(a["f_planes"]), p(a["f_inv"]), p(a["mid"]),
        p(a["lookup"]), p(a["seg"]), a["lookup"].numel(), a["seg"].numel() - 1, p(a["zs_t"]), EW, LEFT, RATIO, p(a["fac"].buf),
        a["fac"].n_layers, 1, 1, p(a["W0"]), p(a["W"]), p(a["dW"]), p(a["K"]), p(a["Zc"]), p(a["kp"]), p(a["ks"]), p(a["ws"].buf),
        a["ws_bytes"], p(a["ws"].info), None, 0, p(a["hs"]), None, None, 0.0, None, None,
        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, hip.load().emcid_last_error().decode()


@pytest.mark.parametrize("em", ["h64"], indirect=True)
@pytest.mark.parametrize("what", ["ragged h", "k_planes without k_inv_scale", "dual workspace one byte short", "hs_out without f_planes"])
def test_edited_layer_call_refuses_before_any_launch(em, what):
    """Each refusal returns an error and leaves every output as it was: K, Zc, dW, W, hs_out and the keys' planes pre-filled with a
    sentinel, the dual workspace's poison and the layer's planes bit for bit.  (k_planes without k_inv_scale and the short dual
    workspace used to be refused only after the keys — and, for the workspace, Zc — had been written: the checks now stand in front
    of the first launch.)"""
    N = 40
    c = _case(em, N)
    h, d = em.h, em.d
    fac = hip.factor_cov(em.covs_d, c["lam0"], EW)
    ws = _poisoned_workspace(N, d, h)
    ws_before = ws.buf.view(torch.int64).clone()
    full = lambda *shape: torch.full(shape, 7.0, device=DEV)
    with _planes_kept(em, 0) as (sp, before):
        W0_d = em.fc2(0).weight.detach().clone()
        a = dict(n=U_D, h=h, d=d, f_f32=em.f.f32, f_planes=em.f.planes, f_inv=em.f.inv_scale, mid=em.mid, lookup=c["lookup_d"],
                 seg=c["seg_d"], zs_t=c["zs_t_d"], fac=fac, W0=W0_d, W=full(h, d), dW=full(h, d), K=full(N, d), Zc=full(N, h),
                 kp=torch.full((N, d), 7, dtype=torch.int32, device=DEV), ks=full(N), ws=ws, ws_bytes=ws.nbytes, hs=full(U_D, h))
        if what == "ragged h":
            a["h"] = 48                          # no multiple of 32 (every buffer is larger than such a call would need)
        elif what == "k_planes without k_inv_scale":
            a["ks"] = None
        elif what == "dual workspace one byte short":
            a["ws_bytes"] = ws.nbytes - 1
        else:
            a["f_planes"] = None
        rc, msg = _raw_call(em, a)
        assert rc != 0, f"{what}: accepted"
        with pytest.raises(hip.EmcidHipError):
            hip._check(rc, "emcid_clip_edit_layer_tail_sp16")
        for name in ("W", "dW", "K", "Zc", "hs"):
            assert bool((a[name] == 7.0).all()), f"{what}: {name} was written ({msg})"
        assert bool((a["kp"] == 7).all()) and (a["ks"] is None or bool((a["ks"] == 7.0).all())), f"{what}: the keys' planes were written"
        assert torch.equal(ws.buf.view(torch.int64), ws_before), f"{what}: the dual workspace was written"
        assert torch.equal(sp.planes, before.planes) and torch.equal(sp.inv_scale, before.inv_scale), f"{what}: the planes were written"
        if what == "dual workspace one byte short":
            # the same arguments with the full size are taken
            rc, msg = _raw_call(em, dict(a, ws_bytes=ws.nbytes))
            assert rc == 0, msg
            assert not bool((a["K"] == 7.0).all()) and int(ws.info.item()) == 0


# ---- the primal form at N > d (Np > dp in EditWorkspace) ---------------------------------------------------------------------------

PRIMAL = [(129, 128, 32), (300, 128, 64), (520, 384, 48)]


@pytest.mark.parametrize("N,d,h", PRIMAL)
def test_primal_edit_layer_vs_oracle_with_more_concepts_than_columns(N, d, h):
    """test_kernels_gpu.test_edit_layer_vs_oracle's assertions where N > d: the stacks have more rows than the system has columns
    (Np = 192 / 320 / 576 against dp = 128 / 128 / 384), the assemble contracts over more than dp rows."""
    lam, ew, left = 50.0, 0.6, 3
    K, Zc, zs, Cov, W0 = _edit_inputs(N, d, h, seed=N + d)
    adj_k, resid, upd = orc.closed_form_layer(K, Zc, zs, Cov, lam, ew, left)
    Wd = torch.empty(h, d, dtype=torch.float32, device=DEV)
    out = hip.edit_layer(K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), Cov.to(DEV), lam, ew, left, W0=W0.to(DEV), W=Wd, want_factors=True)
    assert int(out["ws"].info.item()) == 0
    scale = upd.abs().max().item()
    torch.testing.assert_close(out["Rt"].cpu(), resid.t().contiguous(), rtol=1e-14, atol=0)
    assert (out["Xt"].cpu() - adj_k.t()).abs().max().item() <= 1e-9 * adj_k.abs().max().item()
    dw_err = (out["dW"].cpu().double() - upd).abs().max().item()
    print(f"primal {N}x{d}x{h}: dW error {dw_err:.3e} at scale {scale:.3e}")
    assert dw_err <= 1e-6 * scale + 1e-12, (dw_err, scale)
    assert dw_err < 1e-4
    w_ref = W0 + upd.float()
    assert (Wd.cpu() - w_ref).abs().max().item() <= 1e-6 * max(scale, 1.0)


@pytest.mark.parametrize("N,d,h", PRIMAL)
def test_primal_concept_shards_sum_to_full_with_more_concepts_than_columns(N, d, h):
    """hip.edit_layer_shard over three row ranges sums to the full U, at the bar of test_edit_layer_concept_shards_sum_to_full."""
    lam, ew, left, parts = 50.0, 0.6, 3, 3
    K, Zc, zs, Cov, W0 = _edit_inputs(N, d, h, seed=3 * N + d)
    Kd, Zd, zd, Cd, W0d = K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), Cov.to(DEV), W0.to(DEV)
    Wfull = torch.empty_like(W0d)
    full = hip.edit_layer(Kd, Zd, zd, Cd, lam, ew, left, W0=W0d, W=Wfull, want_factors=True)
    U = torch.zeros(h, d, dtype=torch.float64, device=DEV)
    xs = []
    for r in range(parts):
        lo, hi = (N * r) // parts, (N * (r + 1)) // parts
        part = hip.edit_layer_shard(Kd, Zd, zd, Cd, lam, ew, left, (lo, hi), want_factors=True)
        assert int(part["ws"].info.item()) == 0
        U += part["U"]
        xs.append(part["Xt"])
    Wsh = torch.empty_like(W0d)
    dW = hip.apply_update_(U, W0d, Wsh)
    torch.testing.assert_close(torch.cat(xs), full["Xt"], rtol=1e-12, atol=1e-14)
    scale = full["dW"].abs().max().item()
    assert (dW - full["dW"]).abs().max().item() <= 2e-7 * scale
    assert (Wsh - Wfull).abs().max().item() <= 2e-7 * max(scale, 1.0)


# ---- the few-tile split-fp16 form that Zc runs on -------------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,N", [(130, 3072, 768), (37, 2048, 200), (129, 96, 257), (40, 2016, 96)])
def test_linear_sp16_few_tiles_sum_over_three_accumulators(M, K, N):
    """cfg 5 of emcid_linear_sp16_f32 (64 x 64 register-staged tiles, the sum kept in three accumulators) at the tolerance of
    test_kernels_gpu.test_linear_sp16_vs_torch, ragged edges and epilogues included; the automatic choice is this form from
    K = 2048 on and the one-accumulator form 4 below (bit for bit), so Zc of an edited layer at d >= 2048 runs on it."""
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K + 4, generator=g).to(DEV)[:, :K]
    w = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    r = torch.randn(M, N, generator=g).to(DEV)
    ref = F.linear(x.double(), w.double(), b.double())
    tol = 3e-6 * ref.abs().max().item() * max(1.0, (K / 768) ** 0.5) + 1e-6
    xs, ws_ = hip.split_rows(x), hip.split_rows(w)
    y = hip.linear_sp(xs, ws_, b, cfg=5)
    assert (y.double() - ref).abs().max().item() <= tol
    assert torch.equal(hip.linear_sp(xs, ws_, b, cfg=5), y)
    assert torch.equal(hip.linear_sp(xs, ws_, b), hip.linear_sp(xs, ws_, b, cfg=5 if K >= 2048 else 4))
    yr = hip.linear_sp(xs, ws_, b, residual=r, cfg=5)
    torch.testing.assert_close(yr, (ref + r.double()).float(), rtol=0, atol=tol)
    yq = hip.linear_sp(xs, ws_, b, act=hip.ACT_QUICK_GELU, cfg=5)
    torch.testing.assert_close(yq, (ref * torch.sigmoid(1.702 * ref)).float(), rtol=2e-6, atol=tol)
    wide = torch.full((M, N + 8), 7.0, device=DEV)
    hip.linear_sp(xs, ws_, b, out=wide[:, :N], cfg=5)
    assert torch.equal(wide[:, :N], y) and bool((wide[:, N:] == 7.0).all())

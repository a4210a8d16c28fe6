"""GPU parity tests of the HIP kernels, called through the C ABI (emcid_amd.hip -> libemcid_hip.so).
Run on the MI355X box:  python -m pytest tests -m gpu -x -q"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from emcid_amd import hip
from oracle import emcid_oracle as orc

DEV = "cuda:0"


def _rand(*shape, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=dtype)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 136, 50), (64, 320, 128), (1, 2, 3), (513, 129, 257)])
def test_dgemm_layouts(ta, tb, M, N, K):
    """All four operand layouts, ragged sizes, asymmetric data (catches a transposed C write)."""
    Kp = K + (K % 2)
    Mp, Np_ = M + (M % 2), N + (N % 2)
    a = _rand(M, K, seed=1)
    b = _rand(K, N, seed=2)
    A = torch.zeros(M, Kp, dtype=torch.float64) if ta == 0 else torch.zeros(K, Mp, dtype=torch.float64)
    B = torch.zeros(N, Kp, dtype=torch.float64) if tb == 0 else torch.zeros(K, Np_, dtype=torch.float64)
    if ta == 0: A[:, :K] = a
    else: A[:, :M] = a.t()
    if tb == 0: B[:, :K] = b.t()
    else: B[:, :N] = b
    c0 = _rand(M, N, seed=3)
    Cd = c0.clone().to(DEV)
    hip.dgemm(ta, tb, A.to(DEV), B.to(DEV), Cd, alpha=-0.5, beta=2.0, M=M, N=N, K=K)
    ref = -0.5 * (a @ b) + 2.0 * c0
    torch.testing.assert_close(Cd.cpu(), ref, rtol=1e-12, atol=1e-12 * K)


def test_dgemm_identity_asymmetric():
    """A = I with an asymmetric B: catches row<->col swaps in the MFMA C/D map."""
    n = 256
    Bm = torch.arange(n * n, dtype=torch.float64).reshape(n, n)
    out = torch.zeros(n, n, dtype=torch.float64, device=DEV)
    hip.dgemm(0, 1, torch.eye(n, dtype=torch.float64, device=DEV), Bm.to(DEV), out)
    assert torch.equal(out.cpu(), Bm)


@pytest.mark.parametrize("dp", [128, 256, 384, 512, 640, 1024, 1408])
def test_cholesky_and_solve(dp):
    x = _rand(dp + 64, dp, seed=4)
    A = x.t() @ x + 0.5 * torch.eye(dp, dtype=torch.float64)
    L, inv, info = hip.cholesky(A.clone().to(DEV))
    assert int(info.item()) == 0
    Lref = torch.linalg.cholesky(A)
    torch.testing.assert_close(torch.tril(L.cpu()), Lref, rtol=1e-9, atol=1e-9)
    for J in range((dp + 511) // 512):
        w = min(512, dp - 512 * J)
        blk = Lref[J * 512:J * 512 + w, J * 512:J * 512 + w]
        got = inv[J * 512 * 512:(J + 1) * 512 * 512].view(512, 512)[:w, :w].cpu()
        torch.testing.assert_close(got @ blk, torch.eye(w, dtype=torch.float64), rtol=0, atol=1e-9)
        assert torch.equal(got, torch.tril(got))
    Bt = _rand(192, dp, seed=5)
    X = hip.cholesky_solve_(L, inv, Bt.clone().to(DEV)).cpu()
    ref = torch.linalg.solve(A, Bt.t()).t()
    torch.testing.assert_close(X, ref, rtol=1e-8, atol=1e-10)


def test_cholesky_reports_non_spd():
    dp = 256
    A = torch.eye(dp, dtype=torch.float64)
    A[130, 130] = -1.0
    _, _, info = hip.cholesky(A.to(DEV))
    assert int(info.item()) == 131


def _edit_inputs(N, d, h, seed):
    g = torch.Generator().manual_seed(seed)
    K = torch.randn(N, d, generator=g) * 0.3
    Zc = torch.randn(N, h, generator=g)
    zs = torch.randn(h, N, generator=g)
    x = torch.randn(2 * d, d, generator=g) * torch.exp(torch.linspace(0, -3, d))
    Cov = (x.t() @ x) / (2 * d)
    W0 = torch.randn(h, d, generator=g) * 0.02
    return K, Zc, zs, Cov, W0


@pytest.mark.parametrize("N,d,h,lam,ew,left", [(8, 128, 32, 50.0, 0.6, 3), (5, 192, 48, 90.0, 0.5, 1),
                                              (50, 1400, 96, 300.0, 0.5, 2),     # dp = 1408: short last 512-block
                                              (100, 3072, 768, 4000.0, 0.5, 4), (1000, 3072, 768, 4000.0, 0.5, 2),
                                              (1, 3072, 768, 4000.0, 0.5, 1), (130, 5120, 1280, 10000.0, 0.5, 5),
                                              (1000, 5120, 1280, 10000.0, 0.5, 5),       # BASELINE config 4 (SDXL TE2) at its full size
                                              (1500, 3072, 768, 4000.0, 0.5, 3),         # the reference's largest shipped list (Np = 1536)
                                              (2000, 3072, 768, 4000.0, 0.5, 1)])        # Np = 2048: the last size the fused steps take
def test_edit_layer_vs_oracle(N, d, h, lam, ew, left):
    """The whole per-layer closed form against the oracle's fp64 LU restatement on identical inputs.
    Bar (BASELINE.json): dW max-abs error < 1e-4 and <= 1e-4 relative; observed ~1e-12."""
    K, Zc, zs, Cov, W0 = _edit_inputs(N, d, h, seed=N + d)
    adj_k, resid, upd = orc.closed_form_layer(K, Zc, zs, Cov, lam, ew, left)
    Wd = torch.empty(h, d, dtype=torch.float32, device=DEV)
    out = hip.edit_layer(K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), Cov.to(DEV), lam, ew, left,
                         W0=W0.to(DEV), W=Wd, want_factors=True)
    assert int(out["ws"].info.item()) == 0
    scale = upd.abs().max().item()
    torch.testing.assert_close(out["Rt"].cpu(), resid.t().contiguous(), rtol=1e-14, atol=0)
    assert (out["Xt"].cpu() - adj_k.t()).abs().max().item() <= 1e-9 * adj_k.abs().max().item()
    dw_err = (out["dW"].cpu().double() - upd).abs().max().item()
    assert dw_err <= 1e-6 * scale + 1e-12, (dw_err, scale)        # fp32 rounding of U only
    assert dw_err < 1e-4
    w_ref = W0 + upd.float()
    assert (Wd.cpu() - w_ref).abs().max().item() <= 1e-6 * max(scale, 1.0)


@pytest.mark.parametrize("t,d,ksplit", [(300, 128, 1), (1000, 3072, 1), (3072, 3072, 0), (17, 200, 1), (4097, 5120, 0)])
def test_gram_accumulate(t, d, ksplit):
    """G += X^T X (lower) then mirrored; twice, to check accumulation.  fp32: toleranced, not bitwise."""
    X1 = _rand(t, d, seed=6, dtype=torch.float32)
    X2 = _rand(t, d, seed=7, dtype=torch.float32)
    G = torch.zeros(d, d, dtype=torch.float32, device=DEV)
    hip.gram_accumulate_(G, X1.to(DEV), ksplit)
    hip.gram_accumulate_(G, X2.to(DEV), ksplit)
    hip.symmetrize_lower_(G)
    ref = X1.double().t() @ X1.double() + X2.double().t() @ X2.double()
    err = (G.cpu().double() - ref).abs().max().item()
    assert err <= 2e-6 * ref.abs().max().item() * np.sqrt(t / 100 + 1), err
    assert torch.equal(G, G.t())


def test_gram_empty_batch_is_noop():
    G = torch.ones(128, 128, dtype=torch.float32, device=DEV)
    hip.gram_accumulate_(G, torch.empty(0, 128, dtype=torch.float32, device=DEV))
    assert torch.equal(G.cpu(), torch.ones(128, 128))


def test_gather_mean_bitwise_vs_torch_cpu():
    """Ragged prompt counts; bit-exact against torch-CPU's stack(...).mean(0) (compute_z.py:2311-2325)."""
    g = torch.Generator().manual_seed(8)
    B, S, c = 23, 11, 3072
    act = torch.randn(B, S, c, generator=g)
    idx = torch.randint(0, S, (B,), generator=g)
    counts = [1, 3, 2, 5, 3, 1, 8]
    seg = torch.tensor(np.cumsum([0] + counts))
    rows = torch.stack([act[i, idx[i]] for i in range(B)])
    ref = torch.stack([rows[seg[i]:seg[i + 1]].mean(0) for i in range(len(counts))])
    out = hip.gather_mean(act.to(DEV), idx.to(DEV), seg.to(DEV))
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("B,H,S,D", [(7, 4, 9, 64), (3, 12, 17, 64), (2, 20, 77, 64), (5, 2, 1, 16), (4, 3, 33, 24)])
@pytest.mark.parametrize("mask_kind", ["none", "bool", "float"])
def test_attention_vs_torch_fp32(B, H, S, D, mask_kind):
    """Fused attention vs the plain-PyTorch fp32 eager formula (floating point: tolerance 2e-6 abs on O(1) values)."""
    g = torch.Generator().manual_seed(9)
    hidden = torch.randn(B, S, 3, H, D, generator=g).to(DEV)
    q, k, v = (hidden[:, :, i].transpose(1, 2) for i in range(3))       # strided (B,H,S,D) views like HF's
    lens = torch.randint(1, S + 1, (B,), generator=g)
    keep = (torch.arange(S)[None, :] < lens[:, None])                    # right padding
    causal = torch.ones(S, S, dtype=torch.bool).tril()
    keep4 = (keep[:, None, None, :] & causal[None, None]).to(DEV)
    if mask_kind == "none":
        mask, ref_mask = None, causal.to(DEV)[None, None]
    elif mask_kind == "bool":
        mask, ref_mask = keep4, keep4
    else:
        mask = torch.zeros(B, 1, S, S, device=DEV).masked_fill(~keep4, float("-inf"))
        ref_mask = keep4
    scale = D ** -0.5
    w = torch.matmul(q, k.transpose(-1, -2)) * scale
    w = w.masked_fill(~ref_mask, float("-inf"))
    ref = torch.matmul(torch.softmax(w, dim=-1), v).transpose(1, 2).contiguous()
    out = hip.attention(q, k, v, mask, causal=True, scale=scale)
    assert out.shape == (B, S, H, D)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=2e-6)


def test_hip_attention_inside_hf_forward():
    """Encoder forward with the registered HIP attention == the same forward with HF's own attention."""
    from emcid_amd import synthetic as syn
    from emcid_amd.clip_attention import hip_attention
    pipe = syn.build_pipe("toy", DEV)
    enc = pipe.tokenizer(["painting by c0001", "a photo of tench in the style of vincent"], return_tensors="pt", padding=True)
    enc = {k: v.to(DEV) for k, v in enc.items()}
    with torch.no_grad():
        ref = pipe.text_encoder(**enc).last_hidden_state
        with hip_attention(pipe.text_encoder) as on:
            assert on
            got = pipe.text_encoder(**enc).last_hidden_state
    keep = enc["attention_mask"].bool()
    torch.testing.assert_close(got[keep], ref[keep], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("N,d,h,parts", [(100, 3072, 768, 2), (37, 384, 64, 3), (1000, 3072, 768, 8)])
def test_edit_layer_concept_shards_sum_to_full(N, d, h, parts):
    """The multi-GPU split emulated on one GPU: per-shard partial U summed == the unsharded layer."""
    K, Zc, zs, Cov, W0 = _edit_inputs(N, d, h, seed=3 * N + d)
    Kd, Zd, zd, Cd, W0d = K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), Cov.to(DEV), W0.to(DEV)
    Wfull = torch.empty_like(W0d)
    full = hip.edit_layer(Kd, Zd, zd, Cd, 4000.0, 0.5, 2, W0=W0d, W=Wfull, want_factors=True)
    U = torch.zeros(h, d, dtype=torch.float64, device=DEV)
    xs = []
    for r in range(parts):
        lo, hi = (N * r) // parts, (N * (r + 1)) // parts
        part = hip.edit_layer_shard(Kd, Zd, zd, Cd, 4000.0, 0.5, 2, (lo, hi), want_factors=True)
        U += part["U"]
        xs.append(part["Xt"])
    Wsh = torch.empty_like(W0d)
    dW = hip.apply_update_(U, W0d, Wsh)
    torch.testing.assert_close(torch.cat(xs), full["Xt"], rtol=1e-12, atol=1e-14)
    scale = full["dW"].abs().max().item()
    assert (dW - full["dW"]).abs().max().item() <= 2e-7 * scale          # fp64 sum order, then one fp32 rounding
    assert (Wsh - Wfull).abs().max().item() <= 2e-7 * max(scale, 1.0)


def test_quick_gelu_vs_torch():
    x = torch.randn(1237, 3072, generator=torch.Generator().manual_seed(10)).to(DEV) * 3
    torch.testing.assert_close(hip.quick_gelu(x), x * torch.sigmoid(1.702 * x), rtol=2e-6, atol=1e-6)
    y = torch.randn(7, device=DEV)
    torch.testing.assert_close(hip.quick_gelu(y), y * torch.sigmoid(1.702 * y), rtol=2e-6, atol=1e-6)


@pytest.mark.parametrize("U,H,D,max_depth", [(300, 3, 16, None), (300, 12, 64, 9), (400, 20, 64, 15), (300, 5, 32, 16),
                                             (700, 12, 64, 6), (300, 20, 64, 7), (300, 12, 64, 2), (300, 1, 8, 4),   # <= 8 nodes
                                             (300, 12, 64, 40), (300, 20, 64, 30), (300, 24, 32, 30)])                # general kernel (3 / 5 / 6 rounds of four heads)
def test_tree_attention_vs_dense_reference(U, H, D, max_depth):
    """Random trie: every node attends to its ancestor chain; compare with per-node dense softmax in torch.
    Short chains (mass-edit prompts) and long ones, CLIP-L and bigG head shapes."""
    import numpy as np
    rng = np.random.default_rng(11 + U + H)
    parent = [-1]
    dep = [0]
    for u in range(1, U):
        cands = [c for c in range(max(0, u - 40), u) if max_depth is None or dep[c] < max_depth] or [0]
        p_ = cands[int(rng.integers(0, len(cands)))]
        parent.append(p_)
        dep.append(dep[p_] + 1)
    depth, anc = [], []
    for u in range(U):
        chain = [u]
        while parent[chain[-1]] >= 0:
            chain.append(parent[chain[-1]])
        chain = chain[::-1]
        depth.append(len(chain) - 1)
        anc.append(chain)
    dmax = max(depth) + 1
    anc_t = torch.zeros(U, dmax, dtype=torch.int32)
    for u, ch in enumerate(anc):
        anc_t[u, :len(ch)] = torch.tensor(ch, dtype=torch.int32)
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(U, 3, H * D, generator=g).to(DEV)
    q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]                    # strided row views
    out = hip.tree_attention(q, k, v, anc_t.to(DEV), torch.tensor(depth, dtype=torch.int32, device=DEV), H)
    rows = torch.tensor([5, 17, 299, 0, 123], dtype=torch.int32, device=DEV)
    out_rows = hip.tree_attention(q[rows.long()].contiguous(), k, v, anc_t.to(DEV),
                                  torch.tensor(depth, dtype=torch.int32, device=DEV), H, rows=rows)
    ref = torch.empty(U, H * D)
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    for u, ch in enumerate(anc):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            w = torch.softmax((kc[ch][:, sl] @ qc[u, sl]) * D ** -0.5, dim=0)
            ref[u, sl] = w @ vc[ch][:, sl]
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=2e-6)
    torch.testing.assert_close(out_rows.cpu(), ref[rows.cpu().long()], rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("N,d,h,lam,ew,left", [(8, 128, 32, 50.0, 0.6, 3), (5, 192, 48, 90.0, 0.5, 1),
                                              (50, 1400, 96, 300.0, 0.5, 2),     # dp = 1408: short last 512-block
                                              (100, 3072, 768, 4000.0, 0.5, 4), (1000, 3072, 768, 4000.0, 0.5, 2),
                                              (300, 5120, 1280, 10000.0, 0.5, 5),
                                              (1000, 5120, 1280, 10000.0, 0.5, 5),       # config 4 full size: Np = 1024 at dp = 5120 (no shadow
                                                                                         # product: two rounds of stream-K / paired tiles)
                                              (1500, 3072, 768, 4000.0, 0.5, 3),         # data/artists/info/erased-1500artists-...: Np = 1536
                                              (2000, 3072, 768, 4000.0, 0.5, 1),
                                              (2100, 3072, 768, 4000.0, 0.5, 2)])        # Np = 2176: past the fused steps (serial chain,
                                                                                         # short last 512-block, inverse of LS built after it)
def test_dual_solver_vs_oracle(N, d, h, lam, ew, left):
    """The Woodbury form (batched factor of lam*C', N x N system per layer) against the oracle's fp64 LU."""
    K, Zc, zs, Cov, W0 = _edit_inputs(N, d, h, seed=N + d)
    Cov2 = Cov * 1.5 + torch.eye(d) * 1e-3                       # a second layer's statistics in the same batch
    adj_k, resid, upd = orc.closed_form_layer(K, Zc, zs, Cov, lam, ew, left)
    fac = hip.factor_cov([Cov2.to(DEV), Cov.to(DEV)], lam, ew)
    # the explicit inverse factor the per-layer GEMMs run against: X L = I on the lower triangles
    for l in (0, 1):
        Lm, Xm = torch.tril(fac.L(l)), torch.tril(fac.X(l))
        eye = torch.eye(fac.dp, dtype=torch.float64, device=DEV)
        assert (Xm @ Lm - eye).abs().max().item() < 1e-9
    Wd = torch.empty(h, d, dtype=torch.float32, device=DEV)
    out = hip.edit_layer_dual(K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), fac, 1, ew, left,
                              W0=W0.to(DEV), W=Wd, want_factors=True)
    assert int(fac.info.item()) == 0 and int(out["ws"].info.item()) == 0
    torch.testing.assert_close(out["Rt"].cpu(), resid.t().contiguous(), rtol=1e-14, atol=0)
    assert (out["adj_k"].cpu() - adj_k).abs().max().item() <= 1e-8 * adj_k.abs().max().item()
    scale = upd.abs().max().item()
    dw_err = (out["dW"].cpu().double() - upd).abs().max().item()
    assert dw_err <= 1e-6 * scale + 1e-12 and dw_err < 1e-4, (dw_err, scale)
    assert (Wd.cpu() - (W0 + upd.float())).abs().max().item() <= 1e-6 * max(scale, 1.0)
    # apply-only form (adj_k never formed): same weights
    Wa = torch.empty(h, d, dtype=torch.float32, device=DEV)
    oa = hip.edit_layer_dual_apply(K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), fac, 1, ew, left, W0.to(DEV), Wa)
    assert int(oa["ws"].info.item()) == 0
    dwa_err = (oa["dW"].cpu().double() - upd).abs().max().item()
    assert dwa_err <= 1e-6 * scale + 1e-12 and dwa_err < 1e-4, (dwa_err, scale)
    assert (Wa.cpu() - (W0 + upd.float())).abs().max().item() <= 1e-6 * max(scale, 1.0)
    # block substitution with L instead of GEMMs against X = inv(L) (what the first edited layer runs): same weights
    Wt = torch.empty(h, d, dtype=torch.float32, device=DEV)
    ot = hip.edit_layer_dual_apply(K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), fac, 1, ew, left, W0.to(DEV), Wt,
                                   use_inverse=False)
    dwt_err = (ot["dW"].cpu().double() - upd).abs().max().item()
    assert dwt_err <= 1e-6 * scale + 1e-12 and dwt_err < 1e-4, (dwt_err, scale)
    ofull = hip.edit_layer_dual(K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), fac, 1, ew, left, want_factors=True,
                                use_inverse=False)
    assert (ofull["adj_k"].cpu() - adj_k).abs().max().item() <= 1e-8 * adj_k.abs().max().item()
    # row-sharded M-solves (multi-GPU split) give the same Pt rows
    ws2 = hip.DualWorkspace(N, d, h, DEV)
    if N >= 4:
        parts = []
        for lo, hi in ((0, N // 2), (N // 2, N)):
            hip.edit_layer_dual(K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), fac, 1, ew, left, ws=ws2, rows=(lo, hi),
                                want_dw=False)
            parts.append(ws2.Pt[lo:hi].clone())
        torch.testing.assert_close(torch.cat(parts), out["ws"].Pt[:N], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("N,d,h,lam0,lam,left", [(8, 128, 32, 50.0, 7.5, 3), (100, 3072, 768, 4000.0, 20000.0, 4),
                                                 (1000, 3072, 768, 4000.0, 1000.0, 2), (300, 5120, 1280, 10000.0, 6000.0, 5)])
def test_dual_solver_reuses_factor_for_another_lambda(N, d, h, lam0, lam, left):
    """chol(lam C') = sqrt(lam) chol(C'): a workspace factored at lam0 serves an edit at lam through `lam_ratio` (the stage-1
    gain on Kt64 / Rt; include/emcid_hip.h).  Every dual form against the oracle's fp64 LU AT lam, and against a workspace
    factored at lam itself; the returned adj_k / resid are in the caller's scale."""
    ew = 0.5
    K, Zc, zs, Cov, W0 = _edit_inputs(N, d, h, seed=N + d + 1)
    adj_k, resid, upd = orc.closed_form_layer(K, Zc, zs, Cov, lam, ew, left)
    scale = upd.abs().max().item()
    Kd, Zd, zd, W0d = K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), W0.to(DEV)
    fac0 = hip.factor_cov([Cov.to(DEV)], lam0, ew)
    assert fac0.lam == lam0 and fac0.lam_ratio(lam) == lam / lam0 and fac0.lam_ratio(None) == 1.0
    full = hip.edit_layer_dual(Kd, Zd, zd, fac0, 0, ew, left, W0=W0d, W=torch.empty(h, d, device=DEV), want_factors=True, lam=lam)
    assert int(fac0.info.item()) == 0 and int(full["ws"].info.item()) == 0
    torch.testing.assert_close(full["Rt"].cpu(), resid.t().contiguous(), rtol=1e-14, atol=0)
    assert (full["adj_k"].cpu() - adj_k).abs().max().item() <= 1e-8 * adj_k.abs().max().item()
    assert (full["dW"].cpu().double() - upd).abs().max().item() <= 1e-6 * scale + 1e-12
    own = hip.factor_cov([Cov.to(DEV)], lam, ew)
    for use_inv in (True, False):
        W = torch.empty(h, d, device=DEV)
        got = hip.edit_layer_dual_apply(Kd, Zd, zd, fac0, 0, ew, left, W0d, W, use_inverse=use_inv, lam=lam)
        assert int(got["ws"].info.item()) == 0
        err = (got["dW"].cpu().double() - upd).abs().max().item()
        assert err <= 1e-6 * scale + 1e-12 and err < 1e-4, (use_inv, err, scale)
        assert (W.cpu() - (W0 + upd.float())).abs().max().item() <= 1e-6 * max(scale, 1.0)
        ref = hip.edit_layer_dual_apply(Kd, Zd, zd, own, 0, ew, left, W0d, torch.empty(h, d, device=DEV), use_inverse=use_inv)
        assert (got["dW"] - ref["dW"]).abs().max().item() <= 2e-7 * scale      # same numbers up to the fp32 rounding of dW
    # the column-sharded form (one rank owning every tile)
    W = torch.empty(h, d, device=DEV)
    cols = hip.edit_layer_dual_cols(Kd, Zd, zd, fac0, 0, ew, left, W0d, W, list(range(fac0.dp // 128)), lambda t: t, lam=lam)
    assert (cols["dW"].cpu().double() - upd).abs().max().item() <= 1e-6 * scale + 1e-12
    # lam_ratio = 1 is the call without lam: the same launches with the same arguments — bit-identical where the schedule is
    # reproducible (from 512 padded concepts the N x N SYRK is the two-phase stream-K; below, its K split adds with f64 atomics)
    a = hip.edit_layer_dual_apply(Kd, Zd, zd, fac0, 0, ew, left, W0d, torch.empty(h, d, device=DEV))
    b = hip.edit_layer_dual_apply(Kd, Zd, zd, fac0, 0, ew, left, W0d, torch.empty(h, d, device=DEV), lam=lam0)
    if N > 384:
        assert torch.equal(a["dW"], b["dW"])
    assert (a["dW"] - b["dW"]).abs().max().item() <= 2e-7 * a["dW"].abs().max().item()


@pytest.mark.parametrize("N,d,h,lam,world", [(1000, 5120, 1280, 10000.0, 2), (300, 5120, 1280, 10000.0, 7), (1000, 3072, 768, 4000.0, 8)])
def test_column_sharded_solve_ranks_emulated(N, d, h, lam, world):
    """The column-sharded solve (multi-GPU form, include/emcid_hip.h) with its ranks emulated on one GPU: every rank's
    stage 1 on its own tiles and workspace, the partial S summed as the all-reduce would, every rank's stage 2, the partial
    U summed — against the oracle.  TE2 width (40 tiles over 2 and 7 ranks) and the headline shape over 8."""
    ew, left = 0.5, 3
    K, Zc, zs, Cov, W0 = _edit_inputs(N, d, h, seed=N + d + world)
    _, _, upd = orc.closed_form_layer(K, Zc, zs, Cov, lam, ew, left)
    Kd, Zd, zd, W0d = K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), W0.to(DEV)
    fac = hip.factor_cov([Cov.to(DEV)], lam, ew)
    n_tiles = fac.dp // 128
    tiles = [hip.column_tiles(r, world, n_tiles) for r in range(world)]
    assert sorted(t for ts in tiles for t in ts) == list(range(n_tiles))
    backends = [hip._HipColsBackend(Kd, Zd, zd, fac, 0, ew, left, hip.DualWorkspace(N, d, h, DEV)) for _ in range(world)]
    S = sum(b.stage1(ts).clone() for b, ts in zip(backends, tiles))
    U = None
    for b, ts in zip(backends, tiles):
        b.a[-1].S.copy_(S)
        u = b.stage2(ts).clone()
        U = u if U is None else U + u
        assert int(b.a[-1].info.item()) == 0
    W = torch.empty(h, d, device=DEV)
    dW = backends[0].apply(U, W0d, W, True)
    scale = upd.abs().max().item()
    err = (dW.cpu().double() - upd).abs().max().item()
    assert err <= 1e-6 * scale + 1e-12 and err < 1e-4, (err, scale)
    assert (W.cpu() - (W0 + upd.float())).abs().max().item() <= 1e-6 * max(scale, 1.0)


@pytest.mark.parametrize("rows,cols", [(5, 32), (300, 768), (6400, 768), (77, 1280), (3, 8192)])
def test_add_layernorm_vs_torch(rows, cols):
    """Fused residual add + LayerNorm against torch's two kernels (fp32 reference of the same op)."""
    g = torch.Generator().manual_seed(rows + cols)
    a = torch.randn(rows, cols + 4, generator=g).to(DEV)[:, :cols]          # strided rows
    b = (torch.randn(rows, cols, generator=g) * 3).to(DEV)
    ln = torch.nn.LayerNorm(cols, eps=1e-5).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(cols, generator=g).to(DEV))
        ln.bias.copy_(torch.randn(cols, generator=g).to(DEV))
        y, z = hip.add_layernorm(a, b, ln)
        ref_y = a + b
        ref_z = ln(ref_y)
    torch.testing.assert_close(y, ref_y, rtol=0, atol=0)
    torch.testing.assert_close(z, ref_z, rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("M,N,K,tri,tb,wgs", [(1024, 3072, 3072, 1, 0, 256), (768, 3072, 3072, 2, 1, 256), (100, 384, 384, 1, 0, 7),
                                               (130, 500, 500, 2, 1, 512), (1000, 1408, 1408, 1, 0, 64), (37, 128, 128, 2, 1, 3),
                                               (1024, 5120, 5120, 1, 0, 256), (1280, 5120, 5120, 2, 1, 256)])
def test_streamk_two_phase_triangular_gemm(M, N, K, tri, tb, wgs):
    """The atomic-free stream-K form (partial tiles to a workspace, the last ticket holder sums them in run order):
    against a plain fp64 matmul on the same shapes as the atomic form, the output never pre-initialised, and
    BIT-IDENTICAL from call to call (the atomic form is not)."""
    g = torch.Generator().manual_seed(M + N + wgs)
    A = torch.randn(M, K, generator=g, dtype=torch.float64).to(DEV)
    T = torch.tril(torch.randn(N, K, generator=g, dtype=torch.float64)).to(DEV)
    ref = A @ (T.t() if tb == 0 else T)
    outs = []
    for rep in range(3):
        C = torch.full((M, N), float("nan"), dtype=torch.float64, device=DEV)
        hip.dgemm_streamk(tb, A, T, C, flags=tri, wgs=wgs)
        assert (C - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
        outs.append(C)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("n,k,wgs", [(1024, 3072, 256), (512, 3072, 256), (640, 5120, 256), (1000, 200, 16), (128, 64, 256)])
def test_streamk_two_phase_syrk_plus_identity(n, k, wgs):
    """S = I + Y Y^T on the lower 128-tiles (the N x N system of the dual solver), identity added by the epilogue."""
    g = torch.Generator().manual_seed(n + k)
    Y = torch.randn(n, k, generator=g, dtype=torch.float64).to(DEV)
    ref = torch.eye(n, dtype=torch.float64, device=DEV) + Y @ Y.t()
    outs = []
    for rep in range(2):
        S = torch.full((n, n), float("nan"), dtype=torch.float64, device=DEV)
        hip.dgemm_streamk(0, Y, Y, S, flags=16, wgs=wgs, diag_add=1.0)
        low = torch.tril(torch.ones(n, n, dtype=torch.bool, device=DEV))
        assert ((S - ref)[low]).abs().max().item() <= 1e-12 * ref.abs().max().item()
        outs.append(S[low])
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("n,nrhs,kind", [(64, 5, "general"), (200, 130, "general"), (1000, 64, "indefinite"),
                                         (1536, 300, "indefinite"), (96, 2, "spd")])
def test_lu_solve_matches_lapack(n, nrhs, kind):
    """Blocked LU with partial pivoting + two substitutions (the reference's torch.linalg.solve = getrf + getrs) against
    LAPACK on the same matrix: same pivot rows (no ties in random data), solution to fp64 rounding."""
    g = torch.Generator().manual_seed(n + nrhs)
    A = torch.randn(n, n, generator=g, dtype=torch.float64)
    if kind == "indefinite":       # symmetric, eigenvalues of both signs
        q, _ = torch.linalg.qr(A)
        ev = torch.linspace(-2.0, 3.0, n, dtype=torch.float64)
        ev[ev.abs() < 0.05] = 0.05
        A = (q * ev) @ q.t()
        A = (A + A.t()) / 2
    elif kind == "spd":
        A = A @ A.t() + n * torch.eye(n, dtype=torch.float64)
    B = torch.randn(n, nrhs + (nrhs % 2), generator=g, dtype=torch.float64)
    ref = torch.linalg.solve(A, B)
    _, ipiv = torch.linalg.lu_factor(A)
    Ad, Bd = A.clone().to(DEV), B.clone().to(DEV)
    piv, info = hip.lu_solve_(Ad, Bd)
    assert int(info.item()) == 0
    assert torch.equal(piv.cpu() + 1, ipiv.to(torch.int32))
    err = (Bd.cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err <= 1e-9 * max(1.0, float(torch.linalg.cond(A))) * 1e-3 + 1e-11, err


def test_lu_reports_singular_matrix():
    n = 128
    A = torch.randn(n, n, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    A[:, 40] = 0.0                                  # an exactly zero column: pivot 40 is zero whatever the row order
    piv, info = hip.lu_solve_(A.to(DEV), torch.ones(n, 2, dtype=torch.float64, device=DEV))
    assert int(info.item()) == 41


def _indefinite_cov(d, seed, neg=3):
    """A symmetric fp32 'second moment' with a few NEGATIVE eigenvalues: lam*C' + K K^T is then not positive definite
    (the Cholesky paths report a pivot) but perfectly nonsingular, which is all torch.linalg.solve needs."""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(d, d, generator=g, dtype=torch.float64))
    ev = torch.logspace(0, -3, d, dtype=torch.float64)
    ev[-neg:] = -0.05
    C = ((q * ev) @ q.t())
    return ((C + C.t()) / 2).float().contiguous()


@pytest.mark.parametrize("N,d,h", [(12, 256, 64), (200, 3072, 768)])
def test_edit_layer_lu_on_indefinite_system_vs_oracle(N, d, h):
    """Where the reference's LU returns numbers and Cholesky cannot: the LU fallback against the oracle's
    torch.linalg.solve on the same indefinite system; the Cholesky entry points flag the same input."""
    K, Zc, zs, _, W0 = _edit_inputs(N, d, h, seed=11)
    Cov = _indefinite_cov(d, seed=5)
    lam, ew, left = 40.0, 0.5, 2
    adj_k, resid, upd = orc.closed_form_layer(K, Zc, zs, Cov, lam, ew, left)
    args = (K.to(DEV), Zc.to(DEV), zs.t().contiguous().to(DEV), Cov.to(DEV), lam, ew, left)
    chol = hip.edit_layer(*args, W0=W0.to(DEV), W=torch.empty(h, d, device=DEV))
    assert int(chol["ws"].info.item()) > 0                      # not positive definite
    Wd = torch.empty(h, d, dtype=torch.float32, device=DEV)
    out = hip.edit_layer_lu(*args, W0=W0.to(DEV), W=Wd, want_factors=True)
    assert int(out["ws"].info.item()) == 0
    assert out["adj_k"].shape == (d, N)
    assert (out["adj_k"].cpu() - adj_k).abs().max().item() <= 1e-8 * adj_k.abs().max().item()
    torch.testing.assert_close(out["Rt"].cpu(), resid.t().contiguous(), rtol=1e-14, atol=0)
    scale = upd.abs().max().item()
    assert (out["dW"].cpu().double() - upd).abs().max().item() <= 1e-6 * scale
    assert (Wd.cpu() - (W0 + upd.float())).abs().max().item() <= 1e-6 * max(scale, 1.0)


@pytest.mark.parametrize("decades", [2, 4, 6, 8])
@pytest.mark.parametrize("form", ["dual_inverse", "dual_substitution", "direct"])
def test_ill_conditioned_statistics(decades, form):
    """Statistics with a log-uniform spectrum over `decades` decades (cond(C) = 1e2 ... 1e8), d = 3072: dW of every solver
    form against an fp64 LU of the full system lam*C' + K K^T on identical inputs (the reference's computation,
    emcid_main.py:1040-1050).  Bar: 1e-4 relative (BASELINE.json); the dual forms factor lam*C' alone, the matrix
    whose conditioning is worst."""
    N, d, h, lam, ew = 200, 3072, 768, 4000.0, 0.5
    g = torch.Generator().manual_seed(decades)
    Q, _ = torch.linalg.qr(torch.randn(d, d, dtype=torch.float64, generator=g))
    sp = torch.logspace(0, -decades, d, dtype=torch.float64)
    C = ((Q * sp) @ Q.t())
    C = ((C + C.t()) * 0.5).float().contiguous()
    K = (torch.randn(N, d, generator=g) * 0.3)
    Zc = torch.randn(N, h, generator=g)
    zs_t = torch.randn(N, h, generator=g)
    W0 = torch.randn(h, d, generator=g)
    _, _, upd = orc.closed_form_layer(K, Zc, zs_t.t().contiguous(), C, lam, ew, 1)
    Kd, Zd, zd, Cd, W0d = K.to(DEV), Zc.to(DEV), zs_t.to(DEV), C.to(DEV), W0.to(DEV)
    W = torch.empty(h, d, device=DEV)
    if form == "direct":
        res = hip.edit_layer(Kd, Zd, zd, Cd, lam, ew, 1, W0=W0d, W=W)
        info = int(res["ws"].info.item())
    else:
        use_inv = form == "dual_inverse"
        fac = hip.factor_cov([Cd], lam, ew, inverse=use_inv)
        res = hip.edit_layer_dual_apply(Kd, Zd, zd, fac, 0, ew, 1, W0d, W, use_inverse=use_inv)
        info = max(int(fac.info.item()), int(res["ws"].info.item()))
    assert info == 0
    err = (res["dW"].cpu().double() - upd).abs().max().item() / upd.abs().max().item()
    assert err <= 1e-4, err
    assert err <= 2e-6, err           # observed: the fp32 rounding of dW itself (3-4e-8) at every condition number


@pytest.mark.parametrize("decades", [2, 4, 6, 8])
def test_edit_weight_as_a_scalar_on_ill_conditioned_statistics(decades):
    """edit_weight treated as a scalar on C (factors built for edit_weight 0.5 serving an edit at 0.7 through
    lam_eff = lam (1 - 0.7)/(1 - 0.5), handed to the apply-only kernel's ``lam``).  Against the oracle's exact form at 0.7
    (C' = fl32(fl32(0.3 C)/0.5), reference emcid_main.py:1037) the weights differ by the effect of one fp32 rounding per entry
    of C', amplified by the condition of the statistics: 3e-7 at cond 1e2, 1e-5 at 1e4 — inside BASELINE.json's 1e-4 — and
    6e-4 at 1e6, 5e-2 at 1e8: OUTSIDE it.  That is why the engine keys its cached factors by edit_weight and refactors for
    another one; the bound asserted here is the measured envelope 1e-6 + 2e-9 * cond."""
    N, d, h, lam, ew0, ew = 200, 3072, 768, 4000.0, 0.5, 0.7
    g = torch.Generator().manual_seed(decades)
    Q, _ = torch.linalg.qr(torch.randn(d, d, dtype=torch.float64, generator=g))
    sp = torch.logspace(0, -decades, d, dtype=torch.float64)
    C = ((Q * sp) @ Q.t())
    C = ((C + C.t()) * 0.5).float().contiguous()
    K = (torch.randn(N, d, generator=g) * 0.3)
    Zc = torch.randn(N, h, generator=g)
    zs_t = torch.randn(N, h, generator=g)
    W0 = torch.randn(h, d, generator=g)
    _, _, upd = orc.closed_form_layer(K, Zc, zs_t.t().contiguous(), C, lam, ew, 1)
    Kd, Zd, zd, Cd, W0d = K.to(DEV), Zc.to(DEV), zs_t.to(DEV), C.to(DEV), W0.to(DEV)
    W = torch.empty(h, d, device=DEV)
    fac = hip.factor_cov([Cd], lam, ew0)
    res = hip.edit_layer_dual_apply(Kd, Zd, zd, fac, 0, ew, 1, W0d, W, lam=lam * (1 - ew) / (1 - ew0))
    assert max(int(fac.info.item()), int(res["ws"].info.item())) == 0
    err = (res["dW"].cpu().double() - upd).abs().max().item() / upd.abs().max().item()
    print(f"edit_weight as a scalar, cond 1e{decades}: dW rel err {err:.3e}")
    assert err <= 1e-6 + 2e-9 * 10.0 ** decades, err
    if decades <= 4:
        assert err <= 1e-4, err


_SHADOW_SCRIPT = r'''
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from emcid_amd import hip
from oracle import emcid_oracle as orc
from test_kernels_gpu import _edit_inputs
worst = 0.0
for N, d, h, lam in ((200, 3072, 768, 4000.0), (300, 5120, 1280, 10000.0), (260, 1400, 96, 300.0), (640, 1152, 64, 500.0),
                     (1000, 3072, 768, 4000.0), (1000, 5120, 1280, 10000.0)):
    K, Zc, zs, Cov, W0 = _edit_inputs(N, d, h, seed=N + d)
    _, _, upd = orc.closed_form_layer(K, Zc, zs, Cov, lam, 0.5, 2)
    fac = hip.factor_cov([Cov.cuda()], lam, 0.5)
    W = torch.empty(h, d, device="cuda")
    out = hip.edit_layer_dual_apply(K.cuda(), Zc.cuda(), zs.t().contiguous().cuda(), fac, 0, 0.5, 2, W0.cuda(), W)
    assert int(fac.info.item()) == 0 and int(out["ws"].info.item()) == 0
    err = (out["dW"].cpu().double() - upd).abs().max().item() / upd.abs().max().item()
    worst = max(worst, err)
    assert err <= 2e-6, (N, d, err)
print("SHADOW_OK", worst)
'''


def test_shadow_product_forced_and_off():
    """The product P = Yt X riding in the Cholesky leaf launches (EMCID_SHADOW_P=2: forced for every shape, i.e. 2 / 3 / 5 / 8
    leaf launches, an odd number of column tiles, every XCD-block grid) and the path without it (=0) against the oracle; the
    switch is read once per process, hence the child processes."""
    import os, subprocess, sys
    from conftest import REPO
    for mode in ("2", "0"):      # one after the other: side by side the two children's host-side fp64 references fight for the cores (26 s against 18)
        r = subprocess.run([sys.executable, "-c", _SHADOW_SCRIPT, str(REPO)], env=dict(os.environ, EMCID_SHADOW_P=mode),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "SHADOW_OK" in r.stdout, (mode, r.stdout[-2000:] + r.stderr[-4000:])


@pytest.mark.parametrize("M,K,N", [(6400, 768, 2304), (6400, 768, 768), (6400, 3072, 768), (3072, 768, 3072), (1000, 3072, 768),
                                   (6300, 768, 3000), (9000, 32, 2304),
                                   (777, 1280, 3840), (37, 48, 200), (1, 16, 1), (300, 5120, 1280), (161, 32, 129)])
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4, 5, 6, 7, 64, 65 + 4, 66, 67 + 8, 64 + 8])   # tile + 4 (prefetch - 1) + 64 (4 waves)
def test_linear_f32_vs_torch(M, K, N, cfg):
    """emcid_linear_f32 (csrc/gemm_f32.hip) against torch: the plain projection to fp32 rounding of an exact-f32 accumulation
    (reference of the same op: F.linear in fp64 rounded, and torch's own fp32 F.linear), every tile configuration, ragged
    edges; the fused epilogues (bias, quick_gelu, erf-gelu, residual — also in place) against the unfused torch ops."""
    if cfg >= 0 and M * N * K > 6400 * 768 * 2304 // 2 and (cfg & 3) == 3:
        pytest.skip("64 x 64 tiles on the large shapes: covered by the smaller ones")
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K + 4, generator=g).to(DEV)[:, :K]                 # row stride K + 4: a strided row view
    w = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    r = torch.randn(M, N, generator=g).to(DEV)
    ref = F.linear(x.double(), w.double(), b.double())
    scale = ref.abs().max().item()
    tol = 3e-6 * scale * max(1.0, (K / 768) ** 0.5) + 1e-6         # fp32 accumulation over K terms (torch's own: the same size)
    y = hip.linear(x, w, b, cfg=cfg)
    assert (y.double() - ref).abs().max().item() <= tol
    assert (y - F.linear(x, w, b)).abs().max().item() <= 2 * tol
    y0 = hip.linear(x, w, None, cfg=cfg)
    assert (y0.double() - F.linear(x.double(), w.double())).abs().max().item() <= tol
    yq = hip.linear(x, w, b, act=hip.ACT_QUICK_GELU, cfg=cfg)
    torch.testing.assert_close(yq, (ref * torch.sigmoid(1.702 * ref)).float(), rtol=2e-6, atol=tol)
    ye = hip.linear(x, w, b, act=hip.ACT_GELU_ERF, cfg=cfg)
    torch.testing.assert_close(ye, F.gelu(ref).float(), rtol=2e-6, atol=tol)
    yr = hip.linear(x, w, b, residual=r, cfg=cfg)
    torch.testing.assert_close(yr, (ref + r.double()).float(), rtol=0, atol=tol)
    rr = r.clone()
    hip.linear(x, w, b, residual=rr, out=rr, cfg=cfg)                     # in place on the residual stream
    assert torch.equal(rr, yr)
    # an output that is a column block of a wider buffer (leading dimension > N)
    wide = torch.full((M, N + 8), 7.0, device=DEV)
    hip.linear(x, w, b, out=wide[:, :N], cfg=cfg)
    assert torch.equal(wide[:, :N], y) and bool((wide[:, N:] == 7.0).all())


@pytest.mark.parametrize("M,K,N", [(1000, 3072, 768), (640, 3072, 768), (640, 768, 2304), (800, 2048, 768), (1000, 5120, 1280),
                                   (129, 4096, 257), (37, 2048, 200)])
def test_linear_split_k_is_reproducible_and_leaves_its_workspace_clean(M, K, N):
    """The split-K form of the 128 x 128 kernel for launches of few tiles (every tile's K range over 2..8 workgroups; partial
    tiles meet in a per-stream workspace; the last arriver sums them in part order): fp32-rounding close to the fp64 product for
    every part count, the same bits call after call, picked by the automatic choice where K is long, the fused epilogues intact,
    the ticket counters back at zero, a second stream gets a second workspace."""
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    r = torch.randn(M, N, generator=g).to(DEV)
    ref = F.linear(x.double(), w.double(), b.double())
    tol = 3e-6 * ref.abs().max().item() * max(1.0, (K / 768) ** 0.5) + 1e-6
    tiles = -(-M // 128) * -(-N // 128)
    for parts in (2, 3, 5, 8):
        if tiles * parts > 512:
            continue
        cfg = hip.linear_split_cfg(parts)
        y = hip.linear(x, w, b, cfg=cfg)
        assert (y.double() - ref).abs().max().item() <= tol
        for _ in range(3):
            assert torch.equal(hip.linear(x, w, b, cfg=cfg), y)
        yq = hip.linear(x, w, b, act=hip.ACT_QUICK_GELU, residual=r, cfg=cfg)
        torch.testing.assert_close(yq, ((ref * torch.sigmoid(1.702 * ref)) + r.double()).float(), rtol=2e-6, atol=tol)
    auto = hip.linear(x, w, b)
    assert (auto.double() - ref).abs().max().item() <= tol and torch.equal(hip.linear(x, w, b), auto)
    ws = hip._linear_workspace(torch.device(DEV))
    torch.cuda.synchronize()
    assert int(ws[:1024].view(torch.int32).abs().sum().item()) == 0
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ys = [hip.linear(x, w, b) for _ in range(4)]
        assert hip._linear_workspace(torch.device(DEV)) is not ws
    ym = [hip.linear(x, w, b) for _ in range(4)]
    torch.cuda.synchronize()
    assert all(torch.equal(t, auto) for t in ys + ym)


def test_linear_f32_rejects_unsupported_operands():
    x = torch.randn(8, 24, device=DEV)
    w = torch.randn(4, 24, device=DEV)
    assert not hip.linear_supported(x, w)                                 # K % 16 != 0
    with pytest.raises(hip.EmcidHipError):
        hip.linear(x, w)
    assert not hip.linear_supported(torch.randn(8, 32, device=DEV).double(), torch.randn(4, 32, device=DEV).double())


# ---- split-fp16 projections (csrc/gemm_sp16.hip) ----------------------------------------------------------------------------------

def test_split_rows_keeps_22_bits_under_a_per_row_scale():
    """emcid_split_rows_f16: x = (hi + lo) 2^-e with the row's largest magnitude in [2^14, 2^15) before the fp16 rounding; rows
    spanning 60 binades between them, zero rows, tiny and large elements inside a row."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 768, generator=g)
    x *= torch.exp2(torch.randint(-30, 30, (300, 1), generator=g).float())       # rows on very different scales
    x[:, ::7] *= 1e-4                                                              # small elements inside a row
    x[17] = 0.0
    x[18, 5:] = 0.0
    xd = x.to(DEV)
    sp = hip.split_rows(xd)
    back = sp.float().cpu()
    amax = x.abs().amax(1, keepdim=True)
    # element-wise: 2^-22 of the element, or 2^-38 of the row's maximum where lo has left the fp16 normal range
    tol = torch.maximum(x.abs() * 2.0 ** -22, amax * 2.0 ** -38)
    assert bool(((back - x).abs() <= tol).all())
    inv = sp.inv_scale.cpu()
    live = amax[:, 0] > 0
    top = amax[live, 0] / inv[live]
    assert bool((top >= 2.0 ** 14).all()) and bool((top < 2.0 ** 15).all())
    assert bool((torch.log2(inv) == torch.log2(inv).round()).all())             # powers of two
    assert bool((back[17] == 0).all())
    # a strided row view
    wide = torch.randn(64, 136, generator=g).to(DEV)
    sp2 = hip.split_rows(wide[:, :128])
    assert (sp2.float() - wide[:, :128]).abs().max().item() <= wide.abs().max().item() * 2.0 ** -21


@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4])      # auto; 128 x 128, 80 x 128, 64 x 64, 160 x 128 (LDS-DMA, 16x16x32); register-staged 64 x 64
@pytest.mark.parametrize("M,K,N", [(6400, 768, 2304), (6400, 3072, 768), (1000, 3072, 768), (640, 768, 3072), (300, 1280, 1280),
                                   (129, 96, 257), (37, 2048, 200), (256, 32, 32), (330, 192, 130)])
def test_linear_sp16_vs_torch(M, K, N, cfg):
    """emcid_linear_sp16_f32 against the fp64 product at the UNCHANGED tolerance of the exact-f32 kernel's test
    (test_linear_f32_vs_torch): every tile form, ragged edges, the fused epilogues, the split-fp16 output for the next
    projection."""
    if cfg in (2, 4) and M * N * K > 6400 * 768 * 2304 // 2:
        pytest.skip("64 x 64 tiles on the large shapes: covered by the smaller ones")
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K + 4, generator=g).to(DEV)[:, :K]
    w = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    r = torch.randn(M, N, generator=g).to(DEV)
    ref = F.linear(x.double(), w.double(), b.double())
    scale = ref.abs().max().item()
    tol = 3e-6 * scale * max(1.0, (K / 768) ** 0.5) + 1e-6
    xs, ws_ = hip.split_rows(x), hip.split_rows(w)
    y = hip.linear_sp(xs, ws_, b, cfg=cfg)
    assert (y.double() - ref).abs().max().item() <= tol
    assert (y - F.linear(x, w, b)).abs().max().item() <= 2 * tol
    if cfg in (1, 2, 3):       # the LDS-DMA forms contract every element over k in the same order whatever the tile: the same bits
        assert torch.equal(y, hip.linear_sp(xs, ws_, b, cfg=0))
    assert torch.equal(hip.linear_sp(xs, ws_, b, cfg=cfg), y)                   # the same bits call after call
    y0 = hip.linear_sp(xs, ws_, None, cfg=cfg)
    assert (y0.double() - F.linear(x.double(), w.double())).abs().max().item() <= tol
    yq = hip.linear_sp(xs, ws_, b, act=hip.ACT_QUICK_GELU, cfg=cfg)
    torch.testing.assert_close(yq, (ref * torch.sigmoid(1.702 * ref)).float(), rtol=2e-6, atol=tol)
    ye = hip.linear_sp(xs, ws_, b, act=hip.ACT_GELU_ERF, cfg=cfg)
    torch.testing.assert_close(ye, F.gelu(ref).float(), rtol=2e-6, atol=tol)
    yr = hip.linear_sp(xs, ws_, b, residual=r, cfg=cfg)
    torch.testing.assert_close(yr, (ref + r.double()).float(), rtol=0, atol=tol)
    rr = r.clone()
    hip.linear_sp(xs, ws_, b, residual=rr, out=rr, cfg=cfg)                      # in place on the residual stream
    assert torch.equal(rr, yr)
    wide = torch.full((M, N + 8), 7.0, device=DEV)
    hip.linear_sp(xs, ws_, b, out=wide[:, :N], cfg=cfg)
    assert torch.equal(wide[:, :N], y) and bool((wide[:, N:] == 7.0).all())
    if N % 32 == 0:
        # the result as a split matrix under a caller-given bound: the Cauchy-Schwarz bound the forward uses
        bound = x.norm(dim=1) * w.norm(dim=1).max() + b.abs().max()
        ps = torch.exp2(14 - torch.ceil(torch.log2(bound)))
        ps2 = torch.stack([ps, 1.0 / ps]).contiguous()
        yp = hip.linear_sp(xs, ws_, b, act=hip.ACT_QUICK_GELU, planes_scale=ps2, cfg=cfg)
        assert torch.equal(yp.f32, yq)
        back = hip.SplitRows(yp.planes, yp.inv_scale).float()
        # 2^-22 of the element, or the fp16 floor under the bound's scale
        assert bool(((back - yq).abs() <= torch.maximum(yq.abs() * 2.0 ** -21, (2.0 ** -24 / ps)[:, None])).all())
        yp2 = hip.linear_sp(xs, ws_, b, act=hip.ACT_QUICK_GELU, planes_scale=ps2, want_f32=False, cfg=cfg)
        assert yp2.f32 is None and torch.equal(yp2.planes, yp.planes)


@pytest.mark.parametrize("cfg", [-1, 0, 1, 4])
def test_linear_sp16_heavy_tailed_operands(cfg):
    """Operands with the statistics of a trained encoder rather than a Gaussian init: a few channels 10^3 times the rest, rows with
    Cauchy tails, outlier weight rows.  The split keeps 22-23 bits relative to each ROW's largest magnitude, so the error of an
    output element is bounded by 2^-23 (max|x_m| ||w_n||_1 + max|w_n| ||x_m||_1) plus the fp32 accumulation — held with a factor
    of two; and the per-row output scale the LayerNorm hands to fc1 (LnPlanes.out_scale, a Cauchy-Schwarz bound) stays within
    2^10 of the row's true maximum, i.e. the output planes keep >= 12 of their 22 bits even on these rows."""
    g = torch.Generator().manual_seed(77)
    M, K, N = 1500, 768, 3072
    x = torch.randn(M, K, generator=g)
    x[:, torch.randperm(K, generator=g)[:6]] *= 1000.0                        # massive channels
    x[::7] *= torch.distributions.Cauchy(0.0, 1.0).sample((x[::7].shape[0], 1)).abs().clamp(0.1, 500.0)
    w = torch.randn(N, K, generator=g) * 0.05
    w[torch.randperm(N, generator=g)[:8]] *= 50.0
    b = torch.randn(N, generator=g)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    ref = F.linear(xd.double(), wd.double(), bd.double())
    xs, ws_ = hip.split_rows(xd), hip.split_rows(wd)
    y = hip.linear_sp(xs, ws_, bd, cfg=cfg)
    bound = 2.0 ** -23 * (xd.abs().amax(1, keepdim=True).double() * wd.abs().sum(1).double()[None, :] +
                          wd.abs().amax(1).double()[None, :] * xd.abs().sum(1, keepdim=True).double()) + \
        2.0 ** -23 * (xd.abs().double() @ wd.abs().double().t()) + 1e-6
    err = (y.double() - ref).abs()
    assert bool((err <= 2.0 * bound).all()), float((err / bound).max())
    # the exact-f32 kernel is held to the same bound (it rounds every accumulate; the split drops 2^-23 of a row's maximum)
    assert bool(((hip.linear(xd, wd, bd).double() - ref).abs() <= 2.0 * bound).all())
    if cfg == -1:
        # LayerNorm with outlier gains writing x as planes + the fc1 output scale: |act(z W^T + b)| * 2^e < 2^15 (no overflow of
        # the planes) and >= 2^5 on every row (the bound is within 2^10 of the row's true maximum)
        ln = torch.nn.LayerNorm(K).to(DEV)
        with torch.no_grad():
            ln.weight.copy_((torch.rand(K, generator=g) + 0.5).to(DEV))
            ln.weight[torch.randperm(K, generator=g)[:6].to(DEV)] *= 300.0
            ln.bias.copy_((torch.randn(K, generator=g) * 0.2).to(DEV))
        wsp = hip.split_rows(wd, bd, want_bound=True)
        _, zsp = hip.add_layernorm_sp(xd, None, ln, want_f32=True, bound=wsp.bound)
        out = F.linear(zsp.f32, wd, bd)
        top = out.abs().amax(1) * zsp.out_scale[0]
        assert bool((top < 2.0 ** 15).all()) and bool((top >= 2.0 ** 5).all()), (top.min().item(), top.max().item())
        hq = hip.linear_sp(zsp, wsp, bd, act=hip.ACT_QUICK_GELU, planes_scale=zsp.out_scale)
        back = hip.SplitRows(hq.planes, hq.inv_scale).float()
        rowmax = hq.f32.abs().amax(1, keepdim=True)
        assert bool(((back - hq.f32).abs() <= rowmax * 2.0 ** -11 * 2.0 ** -10 + hq.f32.abs() * 2.0 ** -21).all())


def test_producers_write_split_rows_directly():
    """LayerNorm (with and without the residual add, with the embedding gather) and tree attention writing their result as a
    split-fp16 matrix: the planes are exactly what emcid_split_rows_f16 makes of the fp32 kernel's result, and the scale the
    LayerNorm hands to the consuming projection bounds that projection's rows."""
    g = torch.Generator().manual_seed(11)
    rows, cols = 777, 768
    a = torch.randn(rows, cols, generator=g).to(DEV) * 3
    b = torch.randn(rows, cols, generator=g).to(DEV)
    ln = torch.nn.LayerNorm(cols).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(cols, generator=g).abs() + 0.2)
        ln.bias.copy_(torch.randn(cols, generator=g) * 0.1)
    w = (torch.randn(3072, cols, generator=g) * 0.05).to(DEV)
    wb = torch.randn(3072, generator=g).to(DEV)
    wsp = hip.split_rows(w, wb, want_bound=True)
    assert abs(wsp.bound[0].item() / w.norm(dim=1).max().item() - 1.0001) < 1e-5 and wsp.bound[1].item() == wb.abs().max().item()
    for bb in (b, None):
        y_ref, z_ref = hip.add_layernorm(a, bb, ln)
        y, zsp = hip.add_layernorm_sp(a, bb, ln, want_f32=True, bound=wsp.bound)
        assert torch.equal(y, y_ref) and torch.equal(zsp.f32, z_ref)
        ref_sp = hip.split_rows(z_ref)
        assert torch.equal(zsp.planes, ref_sp.planes) and torch.equal(zsp.inv_scale, ref_sp.inv_scale)
        # the projection's rows stay under the bound the LayerNorm derived: |act(z W^T + b)| * 2^e < 2^15
        out = F.linear(z_ref, w, wb)
        assert bool(((out.abs() * zsp.out_scale[0][:, None]) < 2.0 ** 15).all())
        assert torch.equal(zsp.out_scale[0] * zsp.out_scale[1], torch.ones(rows, device=DEV))
        _, zsp2 = hip.add_layernorm_sp(a, bb, ln)
        assert zsp2.f32 is None and zsp2.out_scale is None and torch.equal(zsp2.planes, ref_sp.planes)
        hq = hip.linear_sp(zsp, wsp, wb, act=hip.ACT_QUICK_GELU, planes_scale=zsp.out_scale)
        assert (hq.f32 - hip.linear(z_ref, w, wb, act=hip.ACT_QUICK_GELU)).abs().max().item() <= 3e-6 * out.abs().max().item()
    # embedding gather + LayerNorm
    tok_e = torch.randn(500, cols, generator=g).to(DEV)
    pos_e = torch.randn(16, cols, generator=g).to(DEV)
    token = torch.randint(0, 500, (rows,), generator=g).to(DEV)
    pos = torch.randint(0, 16, (rows,), generator=g).int().to(DEV)
    y_ref, z_ref = hip.embed_layernorm(tok_e, pos_e, token, pos, ln)
    y, zsp = hip.embed_layernorm_sp(tok_e, pos_e, token, pos, ln)
    ref_sp = hip.split_rows(z_ref)
    assert torch.equal(y, y_ref) and torch.equal(zsp.planes, ref_sp.planes) and torch.equal(zsp.inv_scale, ref_sp.inv_scale)
    # tree attention over a small trie: chains of up to 7 and up to 13 nodes, all nodes and a row subset
    for S in (7, 13):
        U, H, D = 300, 12, 64
        depth = torch.randint(0, S, (U,), generator=g).int()
        anc = torch.zeros(U, S, dtype=torch.int32)
        for u in range(U):
            anc[u, :depth[u]] = torch.randint(0, U, (int(depth[u]),), generator=g).int()
            anc[u, depth[u]] = u
        q, k, v = (torch.randn(U, H * D, generator=g).to(DEV) for _ in range(3))
        anc_d, depth_d = anc.to(DEV), depth.to(DEV)
        assert hip.tree_attention_sp_supported(anc_d, H, D)
        ref = hip.tree_attention(q, k, v, anc_d, depth_d, H)
        sp = hip.tree_attention_sp(q, k, v, anc_d, depth_d, H)
        ref_sp = hip.split_rows(ref)
        assert torch.equal(sp.planes, ref_sp.planes) and torch.equal(sp.inv_scale, ref_sp.inv_scale)
        rows_sel = torch.tensor([5, 17, 17, 299, 0], dtype=torch.int32, device=DEV)
        ref = hip.tree_attention(q[rows_sel.long()], k, v, anc_d, depth_d, H, rows=rows_sel)
        sp = hip.tree_attention_sp(q[rows_sel.long()], k, v, anc_d, depth_d, H, rows=rows_sel)
        assert torch.equal(sp.planes, hip.split_rows(ref).planes)


@pytest.mark.parametrize("t,d", [(2048, 256), (3000, 328), (40000, 3072), (33000, 1280)])
def test_gram_accumulate_split_fp16_path(t, d):
    """emcid_gram_accumulate_sp16_f32 (what gram_accumulate_ takes for long batches): X^T as split-fp16 planes under per-feature
    scales per 32 768-token chunk, lower tiles, fp32 atomics — against the fp64 Gram at the exact-f32 kernel's tolerance; features
    on very different scales, a zero feature, a ragged token count crossing a chunk boundary; accumulation over two batches; and
    the exact-f32 SYRK (ksplit = 1) agrees."""
    g = torch.Generator().manual_seed(t + d)
    X1 = torch.randn(t, d, generator=g)
    X1 *= torch.exp2(torch.randint(-12, 12, (1, d), generator=g).float())        # features on very different scales
    X1[:, 7] = 0.0
    X1[::5, 11] *= 1e-5
    X2 = torch.randn(t // 2 + 3, d, generator=g)
    X2[:, 7] = 0.0
    G = torch.zeros(d, d, dtype=torch.float32, device=DEV)
    hip.gram_accumulate_(G, X1.to(DEV), 0)
    hip.gram_accumulate_(G, X2.to(DEV), 0)
    hip.symmetrize_lower_(G)
    ref = X1.double().t() @ X1.double() + X2.double().t() @ X2.double()
    # per entry: relative to the two features' own scales (sqrt of the diagonal), like a correlation
    dd = ref.diagonal().clamp_min(1e-300).sqrt()
    rel = ((G.cpu().double() - ref).abs() / (dd[:, None] * dd[None, :] + 1e-300)).max().item()
    assert rel <= 2e-6 * np.sqrt(t / 100 + 1), rel
    assert torch.equal(G, G.t()) and bool((G[7] == 0).all())
    G1 = torch.zeros(d, d, dtype=torch.float32, device=DEV)
    hip.gram_accumulate_(G1, X1.to(DEV), 1)
    hip.gram_accumulate_(G1, X2.to(DEV), 1)
    hip.symmetrize_lower_(G1)
    rel1 = ((G1.cpu().double() - ref).abs() / (dd[:, None] * dd[None, :] + 1e-300)).max().item()
    print(f"gram t={t} d={d}: split-fp16 {rel:.2e}, exact-f32 {rel1:.2e} (relative to the features' scales)")


@pytest.mark.parametrize("t,d", [(2500, 256), (40000, 768)])
def test_gram_row_weights_inside_the_split_kernels(t, d):
    """row_weight (ABI 14): the packed Stage-0 forward's square-root multiplicities applied where the Gram's kernels read the rows
    (emcid_amd/layer_stats.py `_collect_packed`) — against the fp64 Gram of the weighted rows, against the Gram of rows multiplied
    beforehand (the form before; same tolerance, sums in no fixed order), through SecondMoment.add directly and through its staging
    buffer (short batches multiply in Python), and with a weight that makes a small feature the chunk's largest."""
    from emcid_amd import runningstats
    g = torch.Generator().manual_seed(3 * t + d)
    X = torch.randn(t, d, generator=g)
    X *= torch.exp2(torch.randint(-8, 8, (1, d), generator=g).float())
    w = torch.randint(1, 400, (t,), generator=g).float().sqrt()
    w[5] = 3.0e4                                         # one heavy row: the column maxima come from w x, not from x
    Xd, wd = X.to(DEV), w.to(DEV)
    ref = (X.double() * w.double()[:, None]).t() @ (X.double() * w.double()[:, None])
    dd = ref.diagonal().clamp_min(1e-300).sqrt()
    tol = 2e-6 * np.sqrt(t / 100 + 1)

    def err(G):
        return ((G.cpu().double() - ref).abs() / (dd[:, None] * dd[None, :] + 1e-300)).max().item()

    assert hip.gram_takes_row_weight(Xd)
    G = torch.zeros(d, d, dtype=torch.float32, device=DEV)
    hip.gram_accumulate_(G, Xd, 0, row_weight=wd)
    hip.symmetrize_lower_(G)
    G0 = torch.zeros(d, d, dtype=torch.float32, device=DEV)
    hip.gram_accumulate_(G0, Xd * wd[:, None], 0)
    hip.symmetrize_lower_(G0)
    assert err(G) <= tol and err(G0) <= tol, (err(G), err(G0))
    assert ((G - G0).abs().cpu().double() / (dd[:, None] * dd[None, :] + 1e-300)).max().item() <= tol
    # the deterministic exact-f32 path (ksplit = 1) takes the weights by a multiplication in hip.gram_accumulate_: same bits as
    # the rows multiplied beforehand
    G1 = torch.zeros(d, d, dtype=torch.float32, device=DEV)
    hip.gram_accumulate_(G1, Xd, 1, row_weight=wd)
    G1b = torch.zeros(d, d, dtype=torch.float32, device=DEV)
    hip.gram_accumulate_(G1b, Xd * wd[:, None], 1)
    assert torch.equal(G1, G1b)
    # SecondMoment: one long batch (direct), then the same rows in short pieces (staged: multiplied in Python)
    for piece in (t, 700):
        sm = runningstats.SecondMoment(stage_tokens=2048)
        for r0 in range(0, t, piece):
            sm.add(Xd[r0:r0 + piece], count=int((wd[r0:r0 + piece] ** 2).sum().item()), row_weight=wd[r0:r0 + piece])
        assert err(sm.mom2) <= tol, (piece, err(sm.mom2))
        assert sm.count == sum(int((wd[r0:r0 + piece] ** 2).sum().item()) for r0 in range(0, t, piece))
    cs = runningstats.CombinedStat(mom2=runningstats.SecondMoment(stage_tokens=2048))
    cs.add(Xd, count=7, row_weight=wd)
    assert err(cs.mom2.mom2) <= tol and cs.mom2.count == 7

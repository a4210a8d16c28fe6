"""The forward's kernels against fp64 evaluations of the SAME fp32 inputs, at the statistics of a trained encoder: logits in the
tens to hundreds with a start-token sink, LayerNorm rows whose mean dwarfs their spread or which one channel dominates, tries whose
``anc`` holds arbitrary valid indices behind ``depth[u]`` — and the native layer runner (csrc/clip_layers.hip) called directly.

No tolerance is fixed in advance: every compared tensor is held to e_kernel <= 4 e_f32 + 2^-22 (tests/forward_refs.py), where
e_f32 is the error of the plain fp32 torch formula on the CPU on the same inputs, and both figures are printed.  Bitwise
assertions are the library's existing contracts (y = a + b; planes = split_rows of the fp32 kernel's result)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from emcid_amd import clip_forward as cf
from emcid_amd import hip

import forward_refs as fr

DEV = "cuda:0"


def _report(section):
    print(f"[{section}] largest e_kernel / bar so far: {fr.RATIOS.get(section, 0.0):.3f}")


# ---- A. tree attention -----------------------------------------------------------------------------------------------------------

def _tree_arm(anc_ld: int, H: int) -> str:
    """The dispatch of emcid_tree_attention_f32 (csrc/attention.hip): rounds = ceil(H / 4); anc_ld <= 16 and rounds <= 5 take the
    short kernel (KPS = 2 keys per 16-lane group for anc_ld <= 8, else KPS = 4), everything else the general kernel."""
    rounds = (H + 3) // 4
    if anc_ld <= 16 and rounds <= 5:
        return "short2" if anc_ld <= 8 else "short4"
    return "general"


TREE_CASES = [
    # (U, H, D, max_nodes, arm): anc has exactly max_nodes columns (random_trie), which is the kernels' anc_ld
    (203, 12, 64, 8, "short2"),      # anc_ld = 8: the last width of KPS = 2; rounds = 3
    (203, 20, 64, 8, "short2"),      # rounds = 5: the last round count the short kernel is instantiated for
    (150, 1, 8, 8, "short2"),        # one head (three idle waves), D = 8: only lanes dl < 2 of a 16-lane group carry data
    (150, 3, 16, 8, "short2"),       # H no multiple of 4: the fourth wave's head is dead
    (203, 12, 64, 9, "short4"),      # anc_ld = 9: the first width of KPS = 4
    (203, 20, 64, 9, "short4"),
    (150, 5, 32, 9, "short4"),       # rounds = 2 with three dead heads in the second round
    (203, 12, 64, 16, "short4"),     # anc_ld = 16: the last width of the short kernels (every key slot of KPS = 4 used)
    (203, 20, 64, 16, "short4"),
    (150, 5, 32, 16, "short4"),
    (203, 12, 64, 17, "general"),    # anc_ld = 17 > 16: the general kernel, two 16-key steps, the second with one key
    (203, 21, 64, 16, "general"),    # rounds = 6 > 5 sends short chains to the general kernel; the last round has one live head
    (203, 24, 64, 16, "general"),    # rounds = 6, every wave live
    (320, 12, 64, 77, "general"),    # CLIP's full context: nk > 64, the softmax's lane loop takes a second trip
    (300, 2, 64, 128, "general"),    # a chain of exactly 128 nodes: all of pth[128] and sc[4][128]
]


def _tree_inputs(U, H, D, max_nodes, gain):
    q, k, v = fr.sink_qkv(U, H, D, float(gain))
    anc, depth = fr.random_trie(U, max_nodes, np.random.default_rng(100 * U + 10 * H + max_nodes), lone_root=True)
    v = v.clone()
    v[U - 1] = 0.0                       # the lone root's whole chain: an all-zero output row (the per-row scale of amax = 0)
    return q, k, v, anc, depth


@pytest.mark.parametrize("gain", [1, 8, 30])
@pytest.mark.parametrize("U,H,D,max_nodes,arm", TREE_CASES)
def test_tree_attention_vs_fp64(U, H, D, max_nodes, arm, gain):
    """emcid_tree_attention_f32 / _sp16 on sink inputs: every dispatch arm at its edge, all rows and a row subset with a repeated
    index, chains whose ``anc`` tail holds random valid indices."""
    q, k, v, anc, depth = _tree_inputs(U, H, D, max_nodes, gain)
    assert anc.shape[1] == max_nodes and int(depth.max()) == max_nodes - 1 and _tree_arm(anc.shape[1], H) == arm
    scale = fr.f32(D ** -0.5)
    qd, kd, vd, ad, dd = q.to(DEV), k.to(DEV), v.to(DEV), anc.to(DEV), depth.to(DEV)
    tag = f"tree U{U} H{H} D{D} S{max_nodes} g{gain}"
    ref = fr.tree_attention_ref(q, k, v, anc, depth, H, scale)
    ref32 = fr.tree_attention_ref(q, k, v, anc, depth, H, scale, dtype=torch.float32)
    out = hip.tree_attention(qd, kd, vd, ad, dd, H, scale=scale)
    assert bool(torch.isfinite(out).all())
    fr.assert_within_bar("A", tag + " all rows", out, ref, ref32)
    assert bool((out[U - 1] == 0).all())
    rows = torch.tensor([5, 17, U - 1, 0, 17, max_nodes - 1], dtype=torch.int32)
    q_sel = q[rows.long()].contiguous()
    ref_sel = fr.tree_attention_ref(q_sel, k, v, anc, depth, H, scale, rows)
    out_sel = hip.tree_attention(q_sel.to(DEV), kd, vd, ad, dd, H, scale=scale, rows=rows.to(DEV))
    assert bool(torch.isfinite(out_sel).all()) and torch.equal(out_sel[1], out_sel[4])
    fr.assert_within_bar("A", tag + " row subset", out_sel, ref_sel,
                         lambda: fr.tree_attention_ref(q_sel, k, v, anc, depth, H, scale, rows, dtype=torch.float32))
    gh = fr.gaussian_heads(H)
    if gh:
        # the Gaussian heads hold the same numbers at every gain: as accurate next to saturated heads as on their own
        cols = torch.cat([torch.arange(h * D, (h + 1) * D) for h in gh])
        fr.assert_within_bar("A", tag + " Gaussian heads", out[:, cols.to(DEV)], ref[:, cols], ref32[:, cols])
    if hip.tree_attention_sp_supported(ad, H, D):
        # the existing contract of test_producers_write_split_rows_directly, on these inputs
        assert arm != "general"
        want = hip.split_rows(out)
        sp = hip.tree_attention_sp(qd, kd, vd, ad, dd, H, scale=scale)
        assert torch.equal(sp.planes, want.planes) and torch.equal(sp.inv_scale, want.inv_scale)
        assert bool((sp.planes[U - 1] == 0).all()) and bool(torch.isfinite(sp.inv_scale).all())
        want = hip.split_rows(out_sel)
        sp = hip.tree_attention_sp(q_sel.to(DEV), kd, vd, ad, dd, H, scale=scale, rows=rows.to(DEV))
        assert torch.equal(sp.planes, want.planes) and torch.equal(sp.inv_scale, want.inv_scale)
    else:
        assert arm == "general" or (H * D) % 32 or D % 8
    _report("A")


def test_tree_attention_refuses_chains_past_128_nodes():
    """anc_ld = 129 is past pth[128] / sc[4][128]: both entries refuse it before launching and write nothing."""
    U, H, D = 140, 2, 64
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(U, H * D, generator=g).to(DEV) for _ in range(3))
    anc = torch.randint(0, U, (U, 129), generator=g).int()
    anc[:, 0] = torch.arange(U)
    anc, depth = anc.to(DEV), torch.zeros(U, dtype=torch.int32, device=DEV)        # every index valid, every chain one node
    out = torch.full((U, H * D), 7.0, device=DEV)
    lib = hip.load()
    with pytest.raises(hip.EmcidHipError):
        hip._check(lib.emcid_tree_attention_f32(hip._ptr(q), q.stride(0), hip._ptr(k), hip._ptr(v), k.stride(0), hip._ptr(anc),
                                                anc.stride(0), hip._ptr(depth), None, U, H, D, 0.125, hip._ptr(out), out.stride(0),
                                                hip._stream(q)), "emcid_tree_attention_f32")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(hip.EmcidHipError):
        hip.tree_attention(q, k, v, anc, depth, H)
    assert not hip.tree_attention_sp_supported(anc, H, D)
    planes = torch.full((U, H * D), 7, dtype=torch.int32, device=DEV)
    inv = torch.full((U,), 7.0, device=DEV)
    with pytest.raises(hip.EmcidHipError):
        hip._check(lib.emcid_tree_attention_sp16(hip._ptr(q), q.stride(0), hip._ptr(k), hip._ptr(v), k.stride(0), hip._ptr(anc),
                                                 anc.stride(0), hip._ptr(depth), None, U, H, D, 0.125, hip._ptr(planes),
                                                 planes.stride(0), hip._ptr(inv), hip._stream(q)), "emcid_tree_attention_sp16")
    torch.cuda.synchronize()
    assert bool((planes == 7).all()) and bool((inv == 7.0).all())


# ---- B. dense attention ----------------------------------------------------------------------------------------------------------

def _dense_form(S: int, D: int) -> str:
    """emcid_attention_f32 (csrc/attention.hip): per_wave = 4 (3 S (D + 1) + S (S + 1)) bytes of LDS; four waves per workgroup
    while 4 per_wave <= 64 KiB, else one wave with the large-LDS attribute (per_wave <= 160 KiB, else refused)."""
    per_wave = 4 * (3 * S * (D + 1) + S * (S + 1))
    return "4-wave" if 4 * per_wave <= 64 * 1024 else ("1-wave" if per_wave <= 160 * 1024 else "refused")


DENSE_SHAPES = [
    # (B, H, S, D, form)
    (3, 2, 9, 64, "4-wave"),         # 4 * 7 380 B; six (prompt, head) pairs: the second workgroup has two idle waves
    (2, 2, 20, 128, "1-wave"),       # D > 64: the staging and output loops' second trip; 4 * 32 640 B > 64 KiB
    (2, 1, 77, 128, "1-wave"),       # 143 220 B: the largest CLIP image, under the 160 KiB limit; S > 64: two trips over the rows
    (5, 3, 33, 24, "4-wave"),        # 4 * 14 388 = 57 552 B <= 65 536
    (5, 3, 37, 24, "1-wave"),        # 4 * 16 724 = 66 896 B > 65 536
]


def _dense_mask(kind, B, S, g):
    if kind == "none":
        return None
    if kind == "key_padding":            # (B, 1, 1, S): the expand branch of hip.attention; key 0 stays live
        lens = torch.randint(1, S + 1, (B,), generator=g)
        return (torch.arange(S)[None, :] < lens[:, None])[:, None, None, :]
    keep = torch.rand(B, 1, S, S, generator=g) < 0.7
    keep |= torch.eye(S, dtype=torch.bool)[None, None]      # the diagonal: one live key per query row, causal or not
    if kind == "bool_b1ss":
        return keep
    if kind == "bool_11ss":              # batch stride 0
        return keep[:1].contiguous()
    assert kind == "float_b1ss"          # additive: -inf on dropped keys, a finite bias on the others
    return (torch.randn(B, 1, S, S, generator=g) * 2.0).masked_fill(~keep, float("-inf"))


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("mask_kind", ["none", "bool_b1ss", "float_b1ss", "bool_11ss", "key_padding"])
@pytest.mark.parametrize("gain", [1, 30])
@pytest.mark.parametrize("B,H,S,D,form", DENSE_SHAPES)
def test_dense_attention_vs_fp64(B, H, S, D, form, gain, mask_kind, causal):
    """emcid_attention_f32: both LDS forms, D > 64, every mask layout, causal or not, on sink inputs.  Sink keys dropped by a
    mask put -inf slots next to the row's large finite logits.
    Closest to its bar: (3, 2, 9, 64) at gain 30, causal, no mask — e_kernel 1.02e-6 against e_f32 2.0e-7 on the GPU box's host,
    1.01e-6 on an AVX-512 host (the fp32 formula's error on a near-tie of two keys depends on the BLAS's summation order; the
    kernel's logit is one sequential D-term FMA chain).  Every other case stays under 0.4 of its bar."""
    assert _dense_form(S, D) == form
    hidden = fr.sink_hidden(B, H, S, D, float(gain))
    q, k, v = (hidden[:, :, i].transpose(1, 2) for i in range(3))
    mask = _dense_mask(mask_kind, B, S, torch.Generator().manual_seed(B + S + D))
    scale = fr.f32(D ** -0.5)
    ref = fr.attention_ref(q, k, v, mask, causal, scale)
    hd = hidden.to(DEV)
    qd, kd, vd = (hd[:, :, i].transpose(1, 2) for i in range(3))
    out = hip.attention(qd, kd, vd, None if mask is None else mask.to(DEV), causal=causal, scale=scale)
    assert out.shape == (B, S, H, D) and bool(torch.isfinite(out).all())
    fr.assert_within_bar("B", f"dense B{B} H{H} S{S} D{D} g{gain} {mask_kind} causal={causal} ({form})", out, ref,
                         lambda: fr.attention_ref(q, k, v, mask, causal, scale, dtype=torch.float32))
    _report("B")


def test_dense_attention_refuses_an_image_past_the_lds():
    """(1, 1, 128, 128): per_wave = 264 192 B > 160 KiB is refused before launching."""
    assert _dense_form(128, 128) == "refused"
    q = torch.zeros(1, 1, 128, 128, device=DEV)
    with pytest.raises(hip.EmcidHipError):
        hip.attention(q, q, q, causal=True)


# ---- C. LayerNorm family ---------------------------------------------------------------------------------------------------------

def _ln_module(gamma, beta, eps=1e-5):
    ln = torch.nn.LayerNorm(gamma.numel(), eps=eps).to(DEV)
    with torch.no_grad():
        ln.weight.copy_(gamma.to(DEV))
        ln.bias.copy_(beta.to(DEV))
    return ln


def _heavy_weight(cols, g, n=256):
    """An fc1-like weight with heavy rows (x 50) and its bias."""
    w = torch.randn(n, cols, generator=g) * 0.05
    w[torch.randperm(n, generator=g)[:8]] *= 50.0
    return w, torch.randn(n, generator=g)


def _check_sp(what, zsp, z, w, wb):
    """The split-fp16 form of a LayerNorm result ``z`` (fp32, from the fp32 entry): the planes are split_rows(z), and the output
    scale bounds the consuming projection's rows."""
    want = hip.split_rows(z)
    assert torch.equal(zsp.planes, want.planes) and torch.equal(zsp.inv_scale, want.inv_scale), what
    if zsp.out_scale is not None:
        rows = z.shape[0]
        assert zsp.out_scale.shape == (2, rows)
        assert torch.equal(zsp.out_scale[0] * zsp.out_scale[1], torch.ones(rows, device=DEV))
        pre = F.linear(z.double().cpu(), w.double(), wb.double())
        act = pre * torch.sigmoid(1.702 * pre)
        top = act.abs().amax(1) * zsp.out_scale[0].double().cpu()
        assert bool((top < 2.0 ** 15).all()), (what, float(top.max()))


LN_SHAPES = [(5, 8), (7, 32), (301, 768), (77, 1280), (9, 2048),      # the wave kernel: 2048 is its last width; rows % 4 != 0
             (3, 2052), (3, 8192), (5, 4096)]                          # the block kernel (three rows hold no +500 row: (5, 4096) does)


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("rows,cols", LN_SHAPES)
def test_add_layernorm_vs_fp64(rows, cols, with_b):
    """add_layernorm / add_layernorm_sp on ``trained_rows``: y bitwise, z against fp64 per row — over all rows, and over each
    kind of row against the fp32 formula's error on that kind; the all-zero row gives beta exactly and the constant row within the
    bar, which is 2^-22 of max |beta| there (F.layer_norm returns beta exactly).
    The +500 rows are what showed the kernels' plain two-pass mean losing digits: at (5, 4096) e_kernel was 1.7e-5 against
    e_f32 2.4e-7 and at (5, 8) 1.2e-6 against 1.5e-7 — the fp32 sum of cols values near 500 is good to a few ulp of cols * 500,
    and that error over the spread is the error of every output.  The kernels now correct the mean by the sum of the centred
    values (csrc/attention.hip: add_layernorm_wave_kernel)."""
    x, gamma, beta = fr.trained_rows(rows, cols)
    g = torch.Generator().manual_seed(rows + cols)
    if with_b:
        b = torch.randn(rows, cols, generator=g) * 3
        b[rows - 1] = 0.0
        b[rows - 2] = 0.0
        a = x - b
    else:
        a, b = x, None
    wide = torch.zeros(rows, cols + 4)
    wide[:, :cols] = a
    ad = wide.to(DEV)[:, :cols]                                        # strided rows
    bd = None if b is None else b.to(DEV)
    ln = _ln_module(gamma, beta)
    y_ref, z_ref = fr.add_layernorm_ref(a, b, gamma, beta, ln.eps)
    z32 = lambda: fr.add_layernorm_ref(a, b, gamma, beta, ln.eps, dtype=torch.float32)[1]
    tag = f"layernorm {rows}x{cols} b={with_b}"
    y, z = hip.add_layernorm(ad, bd, ln)
    assert torch.equal(y.cpu(), y_ref)
    fr.assert_within_bar("C", tag, z, z_ref, z32, per_row=True)
    # each kind of row against the fp32 formula's error on that kind alone: the +500 rows, where F.layer_norm itself loses
    # digits (it forms x rstd - mean rstd), do not set the bar of the others
    z32v = z32()
    for kind, first in (("heavy-channel rows", 0), ("offset rows", 1), ("plain rows", 2)):
        sel = torch.arange(first, max(first, rows - 2), 3)
        if sel.numel():
            fr.assert_within_bar("C", f"{tag} {kind}", z[sel.to(DEV)], z_ref[sel], z32v[sel], per_row=True)
    assert torch.equal(z[rows - 1].cpu(), beta)
    fr.assert_within_bar("C", tag + " constant row", z[rows - 2:rows - 1], beta[None].double(), beta[None], per_row=True)
    if cols % 32 == 0 and cols <= 2048:          # what the binding and split_rows take (the C entry: cols % 8 == 0)
        w, wb = _heavy_weight(cols, g)
        wsp = hip.split_rows(w.to(DEV), wb.to(DEV), want_bound=True)
        y2, zsp = hip.add_layernorm_sp(ad, bd, ln, want_f32=True, bound=wsp.bound)
        assert torch.equal(y2.cpu(), y_ref) and torch.equal(zsp.f32, z)
        _check_sp(tag, zsp, z, w, wb)
        _, zsp2 = hip.add_layernorm_sp(ad, bd, ln)
        assert zsp2.f32 is None and zsp2.out_scale is None and torch.equal(zsp2.planes, zsp.planes)
    else:
        with pytest.raises(hip.EmcidHipError):
            hip.add_layernorm_sp(ad, bd, ln)
    _report("C")


@pytest.mark.parametrize("rows,cols", [(7, 32), (77, 768), (9, 2048), (3, 2052)])
def test_embed_layernorm_vs_fp64(rows, cols):
    """embed_layernorm / embed_layernorm_sp: token and position tables with the outlier model's +25 .. 40 position channels,
    indices hitting the first and last rows of both tables."""
    g = torch.Generator().manual_seed(rows + cols)
    n_tok, n_pos = 50, 77
    tok = torch.randn(n_tok, cols, generator=g) * 0.02
    pos = torch.randn(n_pos, cols, generator=g) * 0.01
    pos[:, torch.randperm(cols, generator=g)[:2]] += 25.0 + 15.0 * torch.rand(2, generator=g)
    _, gamma, beta = fr.trained_rows(rows, cols)
    token = torch.randint(0, n_tok, (rows,), generator=g)
    position = torch.randint(0, n_pos, (rows,), generator=g).int()
    token[0], token[1], position[0], position[1] = 0, n_tok - 1, n_pos - 1, 0
    ln = _ln_module(gamma, beta)
    a, b = tok[token], pos[position.long()]
    y_ref, z_ref = fr.add_layernorm_ref(a, b, gamma, beta, ln.eps)
    tag = f"embed_layernorm {rows}x{cols}"
    args = (tok.to(DEV), pos.to(DEV), token.to(DEV), position.to(DEV), ln)
    y, z = hip.embed_layernorm(*args)
    assert torch.equal(y.cpu(), y_ref)
    fr.assert_within_bar("C", tag, z, z_ref, lambda: fr.add_layernorm_ref(a, b, gamma, beta, ln.eps, dtype=torch.float32)[1],
                         per_row=True)
    if cols % 32 == 0 and cols <= 2048:
        y2, zsp = hip.embed_layernorm_sp(*args)
        assert torch.equal(y2.cpu(), y_ref)
        _check_sp(tag, zsp, z, None, None)
    else:
        with pytest.raises(hip.EmcidHipError):
            hip.embed_layernorm_sp(*args)
    _report("C")


# ---- D. the native layer runner, directly ----------------------------------------------------------------------------------------

U_D, NODES_D = 203, 9
MODELS = {"h64": (64, 160, 4, "quick_gelu", False), "h96": (96, 224, 3, "gelu", False), "h768": (768, 3072, 12, "quick_gelu", True)}


class _Model:
    """A two-layer CLIP text model on the GPU, resolved by ``clip_forward.discover``, with a random trie, trained-like residual
    rows, the native runner's struct array and the fp64 / fp32 references of both layers (computed once, never written)."""

    def __init__(self, name):
        from transformers import CLIPTextConfig, CLIPTextModel
        from emcid_amd import synthetic as syn
        h, d, heads, act, outliers = MODELS[name]
        cfg = CLIPTextConfig(hidden_size=h, intermediate_size=d, num_hidden_layers=2, num_attention_heads=heads, vocab_size=64,
                             max_position_embeddings=77, hidden_act=act, bos_token_id=62, eos_token_id=63, pad_token_id=63)
        state = torch.random.get_rng_state()
        torch.manual_seed(21)
        model = CLIPTextModel(cfg).eval()
        torch.random.set_rng_state(state)
        for p in model.parameters():
            p.requires_grad_(False)
        if outliers:
            syn.add_trained_like_outliers(model, seed=26)
        self.h, self.d, self.heads = h, d, heads
        self.model = model.to(DEV)
        self.graph = cf.discover(self.model, "text_model.encoder.layers.{}")
        anc, depth = fr.random_trie(U_D, NODES_D, np.random.default_rng(h))
        self.anc, self.depth = anc, depth
        self.anc_d, self.depth_d = anc.to(DEV), depth.to(DEV)
        z = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.trie = cf.TokenTrie(token=torch.zeros(U_D, dtype=torch.int64, device=DEV), depth=self.depth_d, anc=self.anc_d,
                                 lookup_node=z, query_rows=z.int(), lookup_in_query=z, n_nodes=U_D, n_tokens_dense=U_D)
        self.nat = cf.native_of(self.graph, self.trie, 0, 2)
        self.hs = fr.trained_rows(U_D, h)[0]
        self.w = [fr.layer_weights(l) for l in self.graph.layers]
        self.ref, self.ref32 = {}, {}

    def layer_ref(self, i, rows_sel=None, dtype=torch.float64):
        """(mid, f, hs_out) of layer i on the references' own input: hs for layer 0, layer 0's hs_out (same dtype) for layer 1."""
        cache = self.ref if dtype == torch.float64 else self.ref32
        key = (i, None if rows_sel is None else tuple(rows_sel.tolist()))
        if key not in cache:
            hs = self.hs if i == 0 else self.layer_ref(0, None, dtype)[2]
            cache[key] = fr.clip_layer_ref(self.w[i], hs, self.anc, self.depth, rows_sel, dtype)
        return cache[key]

    def ln(self, which, x, dtype=torch.float64):
        g, b, eps = which
        return F.layer_norm(x.to(dtype), (x.shape[1],), g.to(dtype), b.to(dtype), eps)

    def head(self, i, hs_d, x, rows_sel=None, want_f32=True):
        n = self.nat
        return hip.clip_layer_head(n.array, i, U_D, n.h, n.d, n.heads, n.scale, self.anc_d, self.depth_d,
                                   None if rows_sel is None else rows_sel.to(DEV), hs_d, x, want_f32)


@pytest.fixture(scope="module", params=list(MODELS))
def model(request):
    m = _Model(request.param)
    yield m
    cf.invalidate_weight_caches(m.model)


def test_native_runner_is_available(model):
    """The struct array exists for these layers and this trie: nothing below can pass by taking another path."""
    assert model.nat is not None and (model.nat.h, model.nat.d, model.nat.heads) == (model.h, model.d, model.heads)
    assert hip.tree_attention_sp_supported(model.anc_d, model.heads, model.h // model.heads)


PLAIN_ROWS = torch.arange(2, U_D - 2, 3)        # the rows of ``trained_rows`` with neither the x 1000 channel nor the +500 offset


def _bar_all_and_plain(what, got, ref, ref32):
    """The bar over all rows — relative to the largest entry, which a x 1000 channel of the residual stream sets — and over the
    plain rows alone, whose largest entry is about 35: there an error of the attention block is not hidden behind the residual."""
    fr.assert_within_bar("D", what, got, ref, ref32)
    fr.assert_within_bar("D", what + " (plain rows)", got[PLAIN_ROWS.to(got.device)], ref[PLAIN_ROWS], ref32[PLAIN_ROWS])


def _x_of(model, i, hs_d):
    return hip.add_layernorm_sp(hs_d, None, model.graph.layers[i].ln1)[1]


def _check_f_planes(f):
    """The planes of fc2's input, decoded with their inverse scale, against the fp32 twin: 2^-21 of the element, or the fp16
    floor under the row's scale (the tolerance of test_linear_sp16_vs_torch)."""
    scales = f.inv_scale._base                   # the entry's f_scale [2, n]: scale, then inverse scale
    n = f.planes.shape[0]
    assert scales.shape == (2, n) and torch.equal(scales[1], f.inv_scale)
    assert torch.equal(scales[0] * scales[1], torch.ones(n, device=DEV)) and fr.log2_is_integer(scales[0])
    back = fr.sp_float(f.planes, f.inv_scale)
    assert bool(((back - f.f32).abs() <= torch.maximum(f.f32.abs() * 2.0 ** -21, (2.0 ** -24 * f.inv_scale)[:, None])).all())
    assert bool((f.f32.abs().amax(1) * scales[0] < 2.0 ** 15).all())


def test_clip_layer_head_all_rows(model):
    """emcid_clip_layer_head_sp16 with rows_sel = NULL: mid and fc2's input against one fp64 layer."""
    assert model.nat is not None
    hs_d = model.hs.to(DEV)
    mid, f = model.head(0, hs_d, _x_of(model, 0, hs_d))
    mid_ref, f_ref, _ = model.layer_ref(0)
    mid32, f32_, _ = model.layer_ref(0, dtype=torch.float32)
    _bar_all_and_plain(f"head h{model.h} mid", mid, mid_ref, mid32)
    _bar_all_and_plain(f"head h{model.h} f", f.f32, f_ref, f32_)
    _check_f_planes(f)
    _, f2 = model.head(0, hs_d, _x_of(model, 0, hs_d), want_f32=False)
    assert f2.f32 is None and torch.equal(f2.planes, f.planes)
    _report("D")


@pytest.mark.parametrize("sel", ["subset", "arange"])
def test_clip_layer_head_selected_rows(model, sel):
    """The rows_sel branch: k | v for every node, q / attention / MLP for an unsorted subset with a repeated index (and for
    arange(U)); the [2, n_sel] scale layout; hs and the planes of x are only read."""
    assert model.nat is not None
    rows = torch.tensor([57, 3, 202, 57, 0, 120, 9], dtype=torch.int32) if sel == "subset" else torch.arange(U_D, dtype=torch.int32)
    hs_d = model.hs.to(DEV)
    x = _x_of(model, 0, hs_d)
    hs0, p0, s0 = hs_d.clone(), x.planes.clone(), x.inv_scale.clone()
    mid, f = model.head(0, hs_d, x, rows)
    assert mid.shape == (rows.numel(), model.h) and f.f32.shape == (rows.numel(), model.d)
    assert torch.equal(hs_d, hs0) and torch.equal(x.planes, p0) and torch.equal(x.inv_scale, s0)
    mid_ref, f_ref, _ = model.layer_ref(0, rows)
    mid32, f32_, _ = model.layer_ref(0, rows, dtype=torch.float32)
    fr.assert_within_bar("D", f"head h{model.h} rows_sel={sel} mid", mid, mid_ref, mid32)
    fr.assert_within_bar("D", f"head h{model.h} rows_sel={sel} f", f.f32, f_ref, f32_)
    _check_f_planes(f)
    if sel == "subset":
        assert torch.equal(mid[0], mid[3]) and torch.equal(f.f32[0], f.f32[3]) and torch.equal(f.planes[0], f.planes[3])
        assert torch.equal(f.inv_scale[0], f.inv_scale[3])
    _report("D")


def test_clip_layer_tail(model):
    """emcid_clip_layer_tail_sp16 behind the head: hs_out and the next layer's LN1 planes; no planes without next_ln."""
    assert model.nat is not None
    n = model.nat
    hs_d = model.hs.to(DEV)
    mid, f = model.head(0, hs_d, _x_of(model, 0, hs_d))
    hs1, x1 = hip.clip_layer_tail(n.array, 0, n.h, n.d, f, mid, model.graph.layers[1].ln1)
    out_ref, out32 = model.layer_ref(0)[2], model.layer_ref(0, dtype=torch.float32)[2]
    _bar_all_and_plain(f"tail h{model.h} hs_out", hs1, out_ref, out32)
    ln1 = model.w[1]["ln1"]
    fr.assert_within_bar("D", f"tail h{model.h} next LN1 planes", fr.sp_float(x1.planes, x1.inv_scale), model.ln(ln1, out_ref),
                         lambda: model.ln(ln1, out32, torch.float32), per_row=True)
    hs2, x2 = hip.clip_layer_tail(n.array, 0, n.h, n.d, f, mid, None)
    assert x2 is None and torch.equal(hs2, hs1)
    _report("D")


@pytest.mark.parametrize("with_next_ln", [True, False])
def test_clip_layers_two_layers_in_place(model, with_next_ln):
    """emcid_clip_layers_sp16 over both layers in place against two applications of the fp64 layer; the bar comes from the fp32
    eager evaluation of the same two layers.  Without next_ln the planes of x are left as LN1 of the last layer's input."""
    assert model.nat is not None
    n = model.nat
    hs_d = model.hs.to(DEV)
    x = _x_of(model, 0, hs_d)
    nxt = model.graph.final_layer_norm if with_next_ln else None
    hip.clip_layers(n.array, 0, 2, U_D, n.h, n.d, n.heads, n.scale, model.anc_d, model.depth_d, hs_d, x, nxt)
    out_ref, out32 = model.layer_ref(1)[2], model.layer_ref(1, dtype=torch.float32)[2]
    _bar_all_and_plain(f"layers h{model.h} hs", hs_d, out_ref, out32)
    if with_next_ln:
        ln = (nxt.weight.detach().cpu(), nxt.bias.detach().cpu(), float(nxt.eps))
        x_ref, x32 = model.ln(ln, out_ref), model.ln(ln, out32, torch.float32)
    else:
        ln = model.w[1]["ln1"]
        x_ref, x32 = model.ln(ln, model.layer_ref(0)[2]), model.ln(ln, model.layer_ref(0, dtype=torch.float32)[2], torch.float32)
    fr.assert_within_bar("D", f"layers h{model.h} x planes next_ln={with_next_ln}", fr.sp_float(x.planes, x.inv_scale), x_ref, x32,
                         per_row=True)
    _report("D")


def test_clip_runner_refuses_a_short_workspace_and_a_ragged_width(model, monkeypatch):
    """A workspace one byte short of emcid_clip_workspace_bytes and an h that is no multiple of 32 are refused."""
    assert model.nat is not None
    n = model.nat
    hs_d = model.hs.to(DEV)
    x = _x_of(model, 0, hs_d)
    need = int(hip.load().emcid_clip_workspace_bytes(U_D, n.h, n.d))
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    monkeypatch.setattr(hip, "clip_workspace", lambda dev, rows, h, d: buf[:need - 1])
    hs0 = hs_d.clone()
    with pytest.raises(hip.EmcidHipError):
        model.head(0, hs_d, x)
    with pytest.raises(hip.EmcidHipError):
        hip.clip_layers(n.array, 0, 2, U_D, n.h, n.d, n.heads, n.scale, model.anc_d, model.depth_d, hs_d, x, None)
    torch.cuda.synchronize()
    assert torch.equal(hs_d, hs0)
    monkeypatch.setattr(hip, "clip_workspace", lambda dev, rows, h, d: buf)
    model.head(0, hs_d, x)                                    # the full size is taken
    monkeypatch.undo()
    h_bad, heads_bad = 48, 3
    hs_bad = torch.zeros(U_D, h_bad, device=DEV)
    x_bad = hip.SplitRows(torch.zeros(U_D, h_bad, dtype=torch.int32, device=DEV), torch.ones(U_D, device=DEV))
    with pytest.raises(hip.EmcidHipError):
        hip.clip_layer_head(n.array, 0, U_D, h_bad, 64, heads_bad, 0.25, model.anc_d, model.depth_d, None, hs_bad, x_bad, True)
    with pytest.raises(hip.EmcidHipError):
        hip.clip_layers(n.array, 0, 1, U_D, h_bad, 64, heads_bad, 0.25, model.anc_d, model.depth_d, hs_bad, x_bad, None)


# ---- E. small related pieces -----------------------------------------------------------------------------------------------------

def _gather_mean_case(c, counts, S, g, grid=None):
    B = sum(counts)
    wide = torch.randn(B, S + 2, c + 4, generator=g) if grid is None else \
        torch.randint(-grid, grid + 1, (B, S + 2, c + 4), generator=g).float() / grid
    idx = torch.randint(0, S, (B,), generator=g)
    seg = torch.tensor(np.cumsum([0] + list(counts)))
    act = wide.to(DEV)[:, :S, :c]                                      # ldb and lds_ larger than the dense ones
    assert act.stride(0) > S * c and act.stride(1) > c
    rows = [wide[i, idx[i], :c] for i in range(B)]
    return act, idx, seg, rows


@pytest.mark.parametrize("c", [1, 255, 257, 3072])
def test_gather_mean_bitwise_at_ragged_widths(c):
    """Bitwise against torch.stack(...).mean(0) on the CPU with a strided ``act``, widths around the 256-column workgroup and
    segments of one to three prompts.  (Up to three addends every summation order torch's CPU reduction uses — sequential,
    cascaded in blocks of 16 rows, four interleaved accumulators on a width's ragged tail — is the kernel's prompt order.)"""
    counts = [1, 3, 2, 1, 3, 3, 2]
    act, idx, seg, rows = _gather_mean_case(c, counts, 5, torch.Generator().manual_seed(c))
    ref = torch.stack([torch.stack(rows[int(seg[i]):int(seg[i + 1])]).mean(0) for i in range(len(counts))])
    out = hip.gather_mean(act, idx.to(DEV), seg.to(DEV))
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("c", [257, 3072])
def test_gather_mean_with_a_77_prompt_request(c):
    """A batch where one request has 77 prompts, bitwise against torch.stack(...).mean(0).  torch's CPU sum cascades over blocks
    of 16 rows and the kernel adds in prompt order, so on arbitrary floats the two differ in the last bit from 18 prompts on
    (measured on the CPU: sequential fp32 sum / n against mean(0)); the bitwise inputs therefore lie on a 2^-6 grid in [-1, 1],
    where every partial sum of 77 addends is exact in fp32 and every order gives the same bits — indexing, segment bounds and the
    count are what this checks.  Gaussian inputs are held to the fp64 mean within the bound of an fp32 sum in any order,
    (n - 1) 2^-24 sum |x| / n, plus half an ulp for the division."""
    counts = [2, 77, 1]
    act, idx, seg, rows = _gather_mean_case(c, counts, 3, torch.Generator().manual_seed(c + 1), grid=64)
    ref = torch.stack([torch.stack(rows[int(seg[i]):int(seg[i + 1])]).mean(0) for i in range(len(counts))])
    assert torch.equal(hip.gather_mean(act, idx.to(DEV), seg.to(DEV)).cpu(), ref)
    act, idx, seg, rows = _gather_mean_case(c, counts, 3, torch.Generator().manual_seed(c + 2))
    out = hip.gather_mean(act, idx.to(DEV), seg.to(DEV)).cpu().double()
    for i, n in enumerate(counts):
        part = torch.stack(rows[int(seg[i]):int(seg[i + 1])]).double()
        mean = part.mean(0)
        bound = (n - 1) * 2.0 ** -24 * part.abs().sum(0) / n + 2.0 ** -24 * mean.abs()
        assert bool(((out[i] - mean).abs() <= bound).all())


def test_gather_mean_refuses_65536_requests():
    """N = 65536 is past the grid's y extent: refused (N <= 65535) before launching."""
    N = 65536
    act = torch.zeros(N, 1, 1, device=DEV)
    out = torch.full((N, 1), 7.0, device=DEV)
    with pytest.raises(hip.EmcidHipError):
        hip.gather_mean(act, torch.zeros(N, dtype=torch.int64, device=DEV), torch.arange(N + 1, device=DEV), out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    ok = hip.gather_mean(act[:N - 1], torch.zeros(N - 1, dtype=torch.int64, device=DEV), torch.arange(N, device=DEV))
    assert ok.shape == (N - 1, 1) and bool((ok == 0).all())


def test_quick_gelu_at_the_edges_of_expf():
    """x sigmoid(1.702 x) where 1.702 x straddles expf's overflow (|x| = 51.7 / 52.3: e^88.0 / e^89.0), at +-0, +-1e-30 and
    +-1e4, on a length that is no multiple of 4 (the scalar tail), against the fp64 formula rounded to fp32.
    Bound per element, for any fp32 evaluation of x / (1 + e^t), t = -1.702 x: the product t is rounded (2^-24 |t| relative in
    e^t), expf, the add, the divide and the multiply add half an ulp to two ulp each: (|t| + 4) 2^-23 |y| holds that with a
    factor of two.  Where e^t overflows fp32 the kernel returns x / inf = +-0 for a true |y| < |x| / FLT_MAX: |x| 2^-127 absolute."""
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 51.7, -51.7, 52.3, -52.3, 1e4, -1e4])
    g = torch.Generator().manual_seed(10)
    x = torch.cat([special, torch.randn(1013, generator=g) * 20, special])          # 1033 = 4 * 258 + 1: specials in the tail too
    assert x.numel() % 4 == 1
    y = hip.quick_gelu(x.to(DEV)).cpu()
    ref = fr.quick_gelu_ref(x)
    assert bool(torch.isfinite(y).all())
    t = (fr.f32(1.702) * x.double()).abs()
    tol = (t + 4.0) * 2.0 ** -23 * ref.double().abs() + x.double().abs() * 2.0 ** -127
    bad = (y.double() - ref.double()).abs() > tol
    assert not bool(bad.any()), (x[bad], y[bad], ref[bad])
    neg = x <= -52.3
    assert bool((y[neg] == 0).all())                                   # -0.0 or 0.0, never NaN
    assert bool((y[x == 1e4] == 1e4).all()) and bool((y[x.abs() == 1e-30] == x[x.abs() == 1e-30] * 0.5).all())

"""The reference that judges the one-call edited layer (tests/test_edit_layer_call_gpu.py) against the thing it restates: a hooked
Hugging Face forward in fp64 whose fc2 weight is replaced, between two forwards, by W + float(closed_form_layer(...)) — the body
of the reference's sequential layer loop (keys and current values from forward hooks at the lookup tokens, the closed form, the
weight written into the live model, the NEXT layer then sees the edit).  No GPU.

``forward_refs.clip_layer_ref`` + ``forward_refs.edited_layer_ref`` on the trie of dense prompts (one chain per prompt) must give
the same keys, current values, update, residual stream behind the edited layer and LN1 of the next layer to 1e-12 relative;
the same chain with the OLD weight in fc2 ("stale weight": what a call that forgot to re-split the new weight computes) must be
more than 1e-6 away, so the reference can tell the two apart."""
import torch

from emcid_amd import clip_forward as cf
from oracle import emcid_oracle as orc

import forward_refs as fr

B, S, H, D, HEADS = 9, 7, 64, 160, 4
EW, LEFT = 0.6, 3


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _root(model):
    return getattr(model, "text_model", model)          # (transformers 4.x nests the text tower, 5.x does not)


def _model():
    from transformers import CLIPTextConfig, CLIPTextModel
    cfg = CLIPTextConfig(hidden_size=H, intermediate_size=D, num_hidden_layers=2, num_attention_heads=HEADS, vocab_size=64,
                         max_position_embeddings=77, hidden_act="quick_gelu", bos_token_id=62, eos_token_id=63, pad_token_id=63)
    state = torch.random.get_rng_state()
    torch.manual_seed(21)
    model = CLIPTextModel(cfg).eval()
    torch.random.set_rng_state(state)
    root = _root(model)
    with torch.no_grad():
        # every parameter is an fp32 value held in fp64, and the residual stream entering layer 0 is the token embedding alone:
        # the references take fp32 tensors and widen them, which loses nothing here
        root.embeddings.position_embedding.weight.zero_()
        root.embeddings.token_embedding.weight.mul_(8.0)
    for p in model.parameters():
        p.requires_grad_(False)
    return model.double()


def _forward(model, ids):
    """One hooked forward: (input of layer 0, fc2 input and output of layer 0, input of layer 1, LN1 output of layer 1), rows b S + s."""
    got = {}
    l0, l1 = _root(model).encoder.layers
    flat = lambda t: t.detach().reshape(-1, t.shape[-1]).clone()
    hooks = [
        l0.register_forward_pre_hook(lambda m, a, kw: got.__setitem__("hs", flat(a[0] if a else kw["hidden_states"])), with_kwargs=True),
        l0.mlp.fc2.register_forward_hook(lambda m, a, out: got.update(f=flat(a[0]), z=flat(out))),
        l1.register_forward_pre_hook(lambda m, a, kw: got.__setitem__("hs1", flat(a[0] if a else kw["hidden_states"])), with_kwargs=True),
        l1.layer_norm1.register_forward_hook(lambda m, a, out: got.__setitem__("x1", flat(out))),
    ]
    try:
        with torch.no_grad():
            model(input_ids=ids)
    finally:
        for h in hooks:
            h.remove()
    return got


def test_layer_and_edit_refs_reproduce_the_hooked_forward_with_the_edited_weight():
    model = _model()
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 62, (B, S), generator=g)
    # requests of 1 to 3 prompts; the lookup token of a prompt is any position of it
    counts = [1, 3, 2, 3]
    assert sum(counts) == B
    seg = torch.tensor([0, 1, 4, 6, 9])
    N = len(counts)
    pos = torch.randint(0, S, (B,), generator=g)
    lookup = torch.arange(B) * S + pos                      # node index of every prompt's lookup token
    x = torch.randn(2 * D, D, generator=g) * torch.exp(torch.linspace(0, -3, D))
    Cov = (x.t() @ x) / (2 * D)
    fc2 = _root(model).encoder.layers[0].mlp.fc2
    W, b2 = fc2.weight.detach().clone(), fc2.bias.detach().clone()

    # ---- the hooked forward, the closed form, the weight written into the live model, the forward again
    first = _forward(model, ids)
    K_hf = fr.request_means(first["f"], lookup, seg)
    Zc_hf = fr.request_means(first["z"], lookup, seg)       # the reference averages fc2's OUTPUT rows
    zs_t = Zc_hf.float() + 0.5 * torch.randn(N, H, generator=g)
    # lam for cond(lam C' + Ks Ks^T) of about 100 relative to lam C': an edit that moves the weight, solved to fp64 rounding
    s = (EW / 0.5) ** 0.5
    cov64 = (Cov * (1 - EW) / 0.5).double()
    Y = torch.linalg.solve_triangular(torch.linalg.cholesky(cov64), (K_hf * s).T, upper=False)
    lam = float(torch.linalg.eigvalsh(Y.T @ Y)[-1]) / 100.0
    _, _, U_hf = orc.closed_form_layer(K_hf, Zc_hf, zs_t.t(), Cov, lam, EW, LEFT)
    assert _rel(W + U_hf.float().double(), W) > 1e-3, "the edit does not move the weight"
    with torch.no_grad():
        fc2.weight.copy_(W + U_hf.float().double())
    try:
        second = _forward(model, ids)
    finally:
        with torch.no_grad():
            fc2.weight.copy_(W)
    assert torch.equal(second["f"], first["f"]) and torch.equal(second["hs"], first["hs"])

    # ---- the references on the trie of those prompts
    graph = cf.discover(model, "text_model.encoder.layers.{}")
    w0, w1 = (fr.layer_weights(l) for l in graph.layers)
    assert torch.equal(w0["fc2"][0].double(), W) and torch.equal(first["hs"].float().double(), first["hs"])
    anc, depth = fr.chain_trie(B, S)
    mid, f, hs_stale = fr.clip_layer_ref(w0, first["hs"], anc, depth)
    K, Zc, U, hs_out, x_next = fr.edited_layer_ref(f, mid, lookup, seg, W, b2, zs_t, Cov, lam, EW, LEFT, w1["ln1"])
    for name, got, want in (("f", f, first["f"]), ("K", K, K_hf), ("Zc", Zc, Zc_hf), ("U", U, U_hf), ("hs_out", hs_out, second["hs1"]),
                            ("x_next", x_next, second["x1"])):
        e = _rel(got, want)
        print(f"{name:7s} {e:.3e}")
        assert e <= 1e-12, (name, e)
    # ---- the stale weight: the unedited layer's own output, and its LN1, are far from what the next layer must see
    x_stale = torch.nn.functional.layer_norm(hs_stale, (H,), w1["ln1"][0].double(), w1["ln1"][1].double(), w1["ln1"][2])
    assert _rel(hs_stale, first["hs1"]) <= 1e-12                        # (it IS the unedited forward)
    e_hs, e_x = _rel(hs_stale, second["hs1"]), _rel(x_stale, second["x1"])
    print(f"stale weight: hs_out {e_hs:.3e}  x_next {e_x:.3e}")
    assert e_hs > 1e-6 and e_x > 1e-6, (e_hs, e_x)


def test_edited_layer_ref_in_fp32_is_the_same_formula():
    """The dtype argument: the fp32 evaluation (what sets the bars of the GPU test) is within fp32 rounding of the fp64 one and
    not identical to it, and the keys are torch's own stack(...).mean(0)."""
    g = torch.Generator().manual_seed(6)
    n, N = 23, 5
    f, mid = torch.randn(n, D, generator=g), torch.randn(n, H, generator=g)
    W, b2 = torch.randn(H, D, generator=g) * 0.05, torch.randn(H, generator=g)
    lookup = torch.randint(0, n, (11,), generator=g)
    seg = torch.tensor([0, 1, 4, 6, 10, 11])
    x = torch.randn(2 * D, D, generator=g) * torch.exp(torch.linspace(0, -3, D))
    Cov = (x.t() @ x) / (2 * D)
    zs_t = torch.randn(N, H, generator=g)
    ln = (torch.rand(H, generator=g) + 0.5, torch.randn(H, generator=g), 1e-5)
    r64 = fr.edited_layer_ref(f, mid, lookup, seg, W, b2, zs_t, Cov, 5.0, EW, LEFT, ln)
    r32 = fr.edited_layer_ref(f, mid, lookup, seg, W, b2, zs_t, Cov, 5.0, EW, LEFT, ln, dtype=torch.float32)
    assert torch.equal(r32[0], torch.stack([f[lookup[int(seg[i]):int(seg[i + 1])]].mean(0) for i in range(N)]))
    assert r64[2].dtype == torch.float64 and r32[2].dtype == torch.float64
    for a, b in zip(r32, r64):
        assert 0.0 < _rel(a, b) <= 1e-4
    for a, dt in ((r32, torch.float32), (r64, torch.float64)):
        assert all(t.dtype == dt for t in (a[0], a[1], a[3], a[4]))
    assert fr.edited_layer_ref(f, mid, lookup, seg, W, b2, zs_t, Cov, 5.0, EW, LEFT)[4] is None

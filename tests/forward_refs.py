"""fp64 references, input generators and the error bar of the forward-kernel tests (tests/test_forward_kernels_gpu.py).  A plain
module, imported by name like tests/session_kernel_helpers.py.

Every reference is the DEFINITION of the operation in plain torch on the CPU — a per-node chain gather and ``softmax``, the dense
softmax(q k^T scale + mask) v, LayerNorm, one CLIP layer on trie rows — and takes the dtype it runs in: float64 is the reference,
float32 is "the plain fp32 torch formula on the same fp32 inputs", whose own distance from the fp64 result sets the bar
(``assert_within_bar``: e_kernel <= 4 e_f32 + 2^-22).  The CPU path is true fp32 and deterministic.

The generators are seeded and give the statistics a trained CLIP text encoder has and ``randn`` lacks: logits in the tens to
hundreds with a start-token sink (``sink_qkv``), residual-stream rows whose mean dwarfs their spread or which one channel dominates
(``trained_rows``), and tries whose ``anc`` entries behind ``depth[u]`` hold random VALID node indices (``random_trie``)."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 2.0 ** -22        # two ulp of the output's largest value: for outputs the fp32 formula gets exactly
FACTOR = 4.0              # summation order, expf against exp, the maximum of two independent error samples
RATIOS = {}               # section -> largest e_kernel / (FACTOR e_f32 + FLOOR) seen in this process (printed by the tests)


def f32(x) -> float:
    """A Python float rounded to fp32 — what a kernel receives when the binding passes it as a C float."""
    return float(np.float32(x))


# ---- errors and the bar ----------------------------------------------------------------------------------------------------------

def err(got: torch.Tensor, ref: torch.Tensor, per_row: bool = False) -> float:
    """max |got - ref| / max |ref|; ``per_row`` (LayerNorm outputs): per row against the row's largest reference magnitude,
    maximised over rows — a row's scale is what the split-fp16 consumers see.  NaN / inf in ``got`` give nan (no bar holds)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("nan")
    d = (got - ref).abs()
    if per_row:
        d2, r2 = d.reshape(d.shape[0], -1), ref.abs().reshape(ref.shape[0], -1)
        top = r2.amax(1)
        return float((d2.amax(1) / torch.where(top > 0, top, torch.ones_like(top))).max())
    top = float(ref.abs().max())
    return float(d.max()) / (top if top > 0 else 1.0)


def f32_err(fn32, ref: torch.Tensor, per_row: bool = False) -> float:
    """``err`` of the plain fp32 torch formula (``fn32()`` or a tensor, evaluated on the CPU on the same fp32 inputs)."""
    val = fn32() if callable(fn32) else fn32
    assert val.dtype == torch.float32 and val.device.type == "cpu"
    return err(val, ref, per_row)


def assert_within_bar(section: str, what: str, got: torch.Tensor, ref: torch.Tensor, fn32, per_row: bool = False) -> float:
    """e_kernel <= 4 e_f32 + 2^-22, with the three figures printed first.  Returns e_kernel."""
    e_k, e_f = err(got, ref, per_row), f32_err(fn32, ref, per_row)
    bar = FACTOR * e_f + FLOOR
    ratio = e_k / e_f if e_f > 0 else float("inf") if e_k > 0 else 0.0
    print(f"[{section}] {what}: e_kernel {e_k:.3e}  e_f32 {e_f:.3e}  ratio {ratio:.2f}  (bar {bar:.3e})")
    if e_k == e_k:
        RATIOS[section] = max(RATIOS.get(section, 0.0), e_k / bar)
    assert e_k <= bar, f"{what}: e_kernel {e_k:.3e} > 4 * {e_f:.3e} + 2^-22"
    return e_k


# ---- references ------------------------------------------------------------------------------------------------------------------

def tree_attention_ref(q, k, v, anc, depth, H: int, scale: float, rows=None, dtype=torch.float64) -> torch.Tensor:
    """Every query node attends to its ancestor chain anc[u][0 .. depth[u]] (root .. u).  q (n, H D) in query order, k / v (U, H D);
    ``rows``: the n query nodes (None: all U).  Nothing behind depth[u] is read."""
    q, k, v = (t.detach().cpu().to(dtype) for t in (q, k, v))
    anc, depth = anc.cpu().long(), depth.cpu().long()
    nodes = range(k.shape[0]) if rows is None else [int(r) for r in rows.cpu()]
    D = k.shape[1] // H
    out = torch.empty(len(nodes), H * D, dtype=dtype)
    for i, u in enumerate(nodes):
        chain = anc[u, :int(depth[u]) + 1]
        kc, vc = k[chain].view(-1, H, D), v[chain].view(-1, H, D)
        p = torch.softmax(torch.einsum("hd,jhd->hj", q[i].view(H, D), kc) * scale, dim=1)
        out[i] = torch.einsum("hj,jhd->hd", p, vc).reshape(-1)
    return out


def attention_ref(q, k, v, mask, causal: bool, scale: float, dtype=torch.float64) -> torch.Tensor:
    """softmax(q k^T scale + mask) v for q / k / v (B, H, S, D); mask: None, a bool keep-mask or an additive float mask,
    broadcastable to (B, 1, S, S); ``causal`` drops keys j > i.  Returns (B, S, H, D) like ``hip.attention``."""
    q, k, v = (t.detach().cpu().to(dtype) for t in (q, k, v))
    S = q.shape[2]
    w = torch.matmul(q, k.transpose(-1, -2)) * scale
    if mask is not None:
        m = mask.detach().cpu()
        w = w.masked_fill(~m, float("-inf")) if m.dtype == torch.bool else w + m.to(dtype)
    if causal:
        w = w.masked_fill(~torch.ones(S, S, dtype=torch.bool).tril(), float("-inf"))
    return torch.matmul(torch.softmax(w, dim=-1), v).transpose(1, 2).contiguous()


def add_layernorm_ref(a, b, gamma, beta, eps: float, dtype=torch.float64):
    """(y, z): y = a + b rounded to fp32 first (the kernel's y is an fp32 sum, asserted bitwise), z = LayerNorm(y) from
    y in ``dtype``.  b None: y = a as it is (an fp64 ``a`` — the residual stream of ``clip_layer_ref`` — is not rounded)."""
    a = a.detach().cpu()
    y = a if b is None else a.float() + b.detach().cpu().float()
    z = F.layer_norm(y.to(dtype), (y.shape[1],), gamma.detach().cpu().to(dtype), beta.detach().cpu().to(dtype), eps)
    return y, z


def layer_weights(layer) -> dict:
    """The tensors of one ``clip_forward.ClipLayer`` as fp32 CPU copies for ``clip_layer_ref``."""
    c = lambda t: t.detach().cpu().float().clone()
    lin = lambda m: (c(m.weight), c(m.bias))
    return {"ln1": (c(layer.ln1.weight), c(layer.ln1.bias), float(layer.ln1.eps)), "q": lin(layer.q), "k": lin(layer.k),
            "v": lin(layer.v), "out": lin(layer.out), "ln2": (c(layer.ln2.weight), c(layer.ln2.bias), float(layer.ln2.eps)),
            "fc1": lin(layer.fc1), "fc2": lin(layer.fc2), "heads": int(layer.heads), "scale": f32(layer.scale),
            "act": {1: "quick_gelu", 2: "gelu"}[int(layer.act_code)]}


def clip_layer_ref(weights: dict, hs, anc, depth, rows_sel=None, dtype=torch.float64):
    """One CLIP text-encoder layer on trie rows: LN1, q | k | v, attention over the ancestor chain, out-projection + residual
    (``mid``), LN2, fc1 + activation (``f``, fc2's input), fc2 + residual (``hs_out``).  ``rows_sel``: k | v for every node,
    everything else for those query nodes only.  Returns (mid, f, hs_out) in ``dtype``."""
    t = lambda x: x.to(dtype)
    lin = lambda x, wb: F.linear(x, t(wb[0]), t(wb[1]))
    hs = hs.detach().cpu().float().to(dtype)
    g, b, eps = weights["ln1"]
    x = F.layer_norm(hs, (hs.shape[1],), t(g), t(b), eps)
    sel = None if rows_sel is None else rows_sel.cpu().long()
    xq, res = (x, hs) if sel is None else (x[sel], hs[sel])
    ctx = tree_attention_ref(lin(xq, weights["q"]), lin(x, weights["k"]), lin(x, weights["v"]), anc, depth, weights["heads"],
                             weights["scale"], rows_sel, dtype)
    mid = lin(ctx, weights["out"]) + res
    g, b, eps = weights["ln2"]
    pre = lin(F.layer_norm(mid, (mid.shape[1],), t(g), t(b), eps), weights["fc1"])
    f = pre * torch.sigmoid(1.702 * pre) if weights["act"] == "quick_gelu" else F.gelu(pre)
    return mid, f, lin(f, weights["fc2"]) + mid


def request_means(rows, lookup, seg, dtype=torch.float64) -> torch.Tensor:
    """Per-request mean of rows[lookup[seg[i] : seg[i + 1]]] in ``dtype`` (torch's stack(...).mean(0), like the reference)."""
    rows, lookup, seg = rows.detach().cpu().to(dtype), lookup.cpu().long(), seg.cpu().long()
    picked = rows[lookup]
    return torch.stack([picked[int(seg[i]):int(seg[i + 1])].mean(0) for i in range(seg.numel() - 1)])


def edited_layer_ref(f, mid, lookup, seg, W, b2, zs_t, Cov, lam: float, edit_weight: float, layers_left: int, next_ln=None,
                     dtype=torch.float64):
    """The body of the reference's sequential layer loop behind ``clip_layer_ref``'s (mid, f): the keys K = per-request means of
    f's lookup rows, the current values Zc = K W^T + b2, the closed form U on those K and Zc (the oracle's fp64 LU:
    ``closed_form_layer``; Cov stays fp32, the reference rounds C' there), W_new = W + float(U), fc2 + residual WITH THE NEW
    WEIGHT, hs_out = f W_new^T + b2 + mid, and the next layer's LN1 of that.  ``zs_t`` (N, h): the targets; ``next_ln``:
    (gamma, beta, eps) or None.  Returns (K, Zc, U, hs_out, x_next) — U in fp64, everything else in ``dtype``."""
    from oracle import emcid_oracle as orc
    t = lambda x: x.detach().cpu().to(dtype)
    f, mid, W, b2 = t(f), t(mid), t(W), t(b2)
    K = request_means(f, lookup, seg, dtype)
    Zc = K @ W.T + b2
    _, _, U = orc.closed_form_layer(K, Zc, zs_t.detach().cpu().t(), Cov.detach().cpu().float(), lam, edit_weight, layers_left)
    W_new = W + U.float().to(dtype)
    hs_out = f @ W_new.T + b2 + mid
    x_next = None
    if next_ln is not None:
        g, b, eps = next_ln
        x_next = F.layer_norm(hs_out, (hs_out.shape[1],), t(g), t(b), eps)
    return K, Zc, U, hs_out, x_next


def chain_trie(B: int, S: int):
    """(anc (B S, S) int32, depth (B S,) int32) of B dense prompts of S tokens as a trie that shares nothing: node b S + s is
    token s of prompt b and its chain is the prompt's tokens 0 .. s — causal attention inside the prompt."""
    anc = torch.zeros(B * S, S, dtype=torch.int32)
    for b in range(B):
        for s in range(S):
            anc[b * S + s, :s + 1] = torch.arange(b * S, b * S + s + 1, dtype=torch.int32)
    return anc, torch.arange(S, dtype=torch.int32).repeat(B)


def quick_gelu_ref(x: torch.Tensor) -> torch.Tensor:
    """x sigmoid(1.702 x) in fp64, rounded to fp32.  1.702 is the fp32 constant the kernel multiplies by."""
    xd = x.detach().cpu().double()
    return (xd / (1.0 + torch.exp(-f32(1.702) * xd))).float()


# ---- input generators ------------------------------------------------------------------------------------------------------------

def gaussian_heads(H: int):
    """The heads ``sink_qkv`` leaves Gaussian: the last two (the last one of two heads, none of a single head)."""
    return list(range(H - min(2, H - 1), H)) if H > 1 else []


@functools.lru_cache(maxsize=None)
def sink_qkv(U: int, H: int, D: int, gain: float, seed: int = 0):
    """q, k, v (U, H D) fp32 with trained-encoder attention statistics: randn; on every head but ``gaussian_heads(H)`` q times
    ``gain`` with three of its channels shifted by 3 gain, and the root node's (node 0) k times 4 and v times 20 — a start-token
    sink carrying a massive value.  The Gaussian heads hold the same numbers whatever the gain.  Shared, never written."""
    g = torch.Generator().manual_seed(4000 + 131 * U + 17 * H + D + seed)
    q, k, v = (torch.randn(U, H, D, generator=g) for _ in range(3))
    sink = [h for h in range(H) if h not in gaussian_heads(H)]
    q[:, sink] *= gain
    for c in sorted({0, D // 2, D - 1}):
        q[:, sink, c] += 3.0 * gain
    k[0, sink] *= 4.0
    v[0, sink] *= 20.0
    return tuple(t.reshape(U, H * D).contiguous() for t in (q, k, v))


@functools.lru_cache(maxsize=None)
def sink_hidden(B: int, H: int, S: int, D: int, gain: float, seed: int = 0) -> torch.Tensor:
    """The same statistics for the dense kernel: (B, S, 3, H, D) fp32 whose [:, :, i].transpose(1, 2) are q, k, v as strided
    (B, H, S, D) views like HF's; token 0 is the sink.  Shared, never written."""
    g = torch.Generator().manual_seed(5000 + 131 * B + 17 * H + 7 * S + D + seed)
    hidden = torch.randn(B, S, 3, H, D, generator=g)
    sink = [h for h in range(H) if h not in gaussian_heads(H)]
    hidden[:, :, 0, sink] *= gain
    for c in sorted({0, D // 2, D - 1}):
        hidden[:, :, 0, sink, c] += 3.0 * gain
    hidden[:, 0, 1, sink] *= 4.0
    hidden[:, 0, 2, sink] *= 20.0
    return hidden


@functools.lru_cache(maxsize=None)
def trained_rows(rows: int, cols: int, seed: int = 0):
    """(x, gamma, beta): residual-stream rows and LayerNorm parameters with the statistics a Gaussian init lacks.  In this order:
    randn rows with two channels shifted by +35; one channel times 1000 on every third row (r % 3 == 0); a constant offset of 500
    on another third (r % 3 == 1); then row rows - 1 all zero and row rows - 2 constant (1.2345 everywhere, set after the
    per-channel edits: a value whose fp32 sums are NOT exact).  gamma = rand + 0.5 with six entries times 300, beta = randn.
    Shared, never written."""
    g = torch.Generator().manual_seed(7000 + 13 * rows + cols + seed)
    x = torch.randn(rows, cols, generator=g)
    ch = torch.randperm(cols, generator=g)[:3]
    x[:, ch[:2]] += 35.0
    x[0::3, ch[2]] *= 1000.0
    x[1::3] += 500.0
    x[rows - 1] = 0.0
    x[rows - 2] = 1.2345
    gamma = torch.rand(cols, generator=g) + 0.5
    gamma[torch.randperm(cols, generator=g)[:6]] *= 300.0
    beta = torch.randn(cols, generator=g)
    return x, gamma, beta


def random_trie(U: int, max_nodes: int, rng: np.random.Generator, lone_root: bool = False):
    """(anc (U, max_nodes) int32, depth (U,) int32) of a random trie with chains of at most ``max_nodes`` nodes.  Nodes
    0 .. max_nodes - 1 form one path, so one chain has EXACTLY max_nodes nodes and ``anc`` exactly that many columns; every other
    node draws its parent among the 40 nodes before it, as tests/test_kernels_gpu.py::test_tree_attention_vs_dense_reference does.
    Every ``anc`` entry behind depth[u] is a random valid node index in [0, U), not zero: a kernel that read one would get wrong
    numbers, never an out-of-range address.  ``lone_root``: the last node is a root of its own (chain = itself)."""
    assert 1 <= max_nodes <= U
    parent, dep = [-1], [0]
    n_tree = U - 1 if lone_root else U
    for u in range(1, n_tree):
        if u < max_nodes:
            p = u - 1
        else:
            cands = [c for c in range(max(0, u - 40), u) if dep[c] < max_nodes - 1] or [0]
            p = cands[int(rng.integers(0, len(cands)))]
        parent.append(p)
        dep.append(dep[p] + 1)
    if lone_root and U > 1:
        parent.append(-1)
        dep.append(0)
    anc = rng.integers(0, U, size=(U, max_nodes)).astype(np.int32)
    for u in range(U):
        chain = [u]
        while parent[chain[-1]] >= 0:
            chain.append(parent[chain[-1]])
        anc[u, :len(chain)] = chain[::-1]
    assert max(dep) == max_nodes - 1
    return torch.from_numpy(anc), torch.tensor(dep, dtype=torch.int32)


def sp_float(planes: torch.Tensor, inv_scale: torch.Tensor) -> torch.Tensor:
    """Split-fp16 planes back to fp32: (hi + lo) 2^-e, as ``hip.SplitRows.float`` without the twin."""
    r, k = planes.shape
    h = planes.contiguous().view(torch.float16).view(r, k // 8, 2, 8).float()
    return (h[:, :, 0] + h[:, :, 1]).reshape(r, k) * inv_scale[:, None]


def log2_is_integer(x: torch.Tensor) -> bool:
    return bool((torch.log2(x) == torch.log2(x).round()).all()) and math.isfinite(float(x.abs().max()))

"""What EditSession.save / load stand on, through the binding with no encoder: emcid_fingerprint_content (include/emcid_hip.h) —
address-free, sensitive to one bit, the very word emcid_fingerprint_store leaves in its table — and the marshalling of
hip.PreservedKeys between two capacities (another ldl, another tile count), bit for bit, with a preserve step on the loaded state
against the primal system in fp64.  Inputs and bars are those of tests/session_kernel_helpers.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from emcid_amd import hip
from session_kernel_helpers import DEV, EW, LAM, U_BAR, _dev, _inputs_by_width as _inputs, _primal_u, _scale, _step

# elements of fp32: one element (4 bytes: padded), no multiple of the 16-byte vector (padded), one vector, 4 096 vectors (the last
# size read whole), one vector more and 40 000 vectors (sampled: 4 096 of them are read)
SIZES = [1, 1001, 4, 4 * 4096, 4 * 4097, 160000]


def _tensor(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _stored_word(t):
    """The fingerprint field emcid_fingerprint_store leaves for ``t`` (bytes % 16 == 0), and the entry's other fields."""
    table = torch.zeros(4, 4, dtype=torch.int64, device=DEV)
    hip.fingerprint_store([(t, 2)], table)
    entry = table.cpu()
    assert entry[2, 0].item() == t.data_ptr() and entry[2, 1].item() == t.numel() * t.element_size()
    assert not entry[[0, 1, 3]].any()
    return entry[2, 2].item()


@pytest.mark.parametrize("n", SIZES)
def test_equal_bytes_at_two_addresses_give_equal_words(n):
    a = _tensor(n, n)
    b = a.clone()
    shifted = torch.cat([a.new_zeros(1), a])[1:]                # the same bytes 4 bytes off a vector boundary
    assert a.data_ptr() != b.data_ptr() and shifted.data_ptr() % 16 != 0
    strided = torch.stack([a, a], 1)[:, 0]                      # the same values, every other element of a buffer
    w = hip.fingerprint_content([a, b, shifted, strided]).cpu()
    assert w.dtype == torch.int64 and w.shape == (4,)
    assert w[0] == w[1] == w[2] == w[3] and w[0] != 0
    assert torch.equal(hip.fingerprint_content([b]).cpu(), w[:1])          # alone as in a batch


@pytest.mark.parametrize("n", SIZES)
def test_one_flipped_bit_gives_another_word(n):
    a = _tensor(n, n)
    before = hip.fingerprint_content([a]).cpu()
    for at, bit in ((0, 0), (n - 1, 31)) if n <= 4 * 4096 else ((0, 12),):       # (a sampled tensor: inside a vector that is read)
        b = a.clone()
        b.view(torch.int32)[at] ^= (1 << bit) - (1 << 32 if bit == 31 else 0)
        assert (a.view(torch.int32) != b.view(torch.int32)).sum().item() == 1
        assert not torch.equal(hip.fingerprint_content([b]).cpu(), before), (at, bit)
    assert torch.equal(hip.fingerprint_content([a]).cpu(), before)


@pytest.mark.parametrize("n", SIZES)
def test_the_word_is_the_one_the_guard_stores(n):
    a = _tensor(n, n)
    if (4 * n) % 16:                         # the guard takes whole vectors only: the word of the bytes padded with zeros
        whole = torch.zeros((4 * n + 15) // 16 * 4, device=DEV)
        whole[:n] = a
    else:
        whole = a
    assert hip.fingerprint_content([a]).cpu().item() == _stored_word(whole)


def test_thirty_three_tensors_take_two_launches():
    ts = [_tensor(4 * (i + 1) if i % 3 else 3 * i + 1, 100 + i) for i in range(33)]
    ts[7] = ts[5].clone()
    words = hip.fingerprint_content(ts).cpu()
    singly = torch.cat([hip.fingerprint_content([t]).cpu() for t in ts])
    assert torch.equal(words, singly)
    assert words[7] == words[5] and len(set(words.tolist())) == 32
    for i in (0, 31, 32):                    # the last of the first launch and the one of the second
        if (4 * ts[i].numel()) % 16 == 0:
            assert words[i].item() == _stored_word(ts[i])


def test_what_is_refused():
    with pytest.raises(hip.EmcidHipError, match="at least one"):
        hip.fingerprint_content([])
    with pytest.raises(hip.EmcidHipError, match="HBM"):
        hip.fingerprint_content([torch.zeros(4)])
    with pytest.raises(hip.EmcidHipError, match="empty"):
        hip.fingerprint_content([torch.zeros(0, device=DEV)])


# ---- PreservedKeys: state_dict -> another capacity -> state_dict ------------------------------------------------------------------

D200, M, N = 200, 130, 5


@pytest.fixture(scope="module")
def built():
    """Two layers of d = 200 (dp = 256) at capacity 200 with M = 130 rows from two retain lists (70, then 60 across the 128 tile);
    each layer has its own inputs.  Shared, never written.  The statistics are the helpers' with the upper triangle replaced by
    the lower one's mirror image (``_symmetric``)."""
    ins = [_symmetric(_inputs(M + N, D200)), _symmetric(_inputs(M + N + 1, D200))]
    fac = hip.factor_cov([_dev(i[3]) for i in ins], LAM, EW)
    state = hip.PreservedKeys(2, D200, 200, DEV)
    for lo, hi in ((0, 70), (70, M)):
        for layer, (K, *_ ) in enumerate(ins):
            res = hip.session_retain(_dev(K[lo:hi]), fac, layer, _scale(), state)
            assert int(res["ws"].info.item()) == 0
        state.commit(hi - lo, hip.row_scale_of(EW, fac, LAM))
    assert state.M == M and int(fac.info.item()) == 0
    return ins, fac, state


def test_state_round_trip_across_capacities(built):
    ins, fac, a = built
    before = [t.clone() for ts in (a.Yp, a.Lp, a.tile_inv) for t in ts]
    one = a.state_dict()
    assert all(torch.equal(x, y) for x, y in zip(before, [t for ts in (a.Yp, a.Lp, a.tile_inv) for t in ts]))     # save changes nothing
    assert one["M"] == M and one["d"] == D200 and one["n_layers"] == 2
    assert [tuple(t.shape) for t in one["Yp"] + one["Lp"] + one["tile_inv"]] == [(M, D200)] * 2 + [(M, M)] * 2 + [(2, 128, 128)] * 2
    assert all(not t.is_cuda for t in one["Yp"] + one["Lp"] + one["tile_inv"]) and one["row_scale"].tolist() == [_scale()] * M
    for i in range(2):
        assert torch.equal(one["Yp"][i], a.Yp[i][:M, :D200].cpu()) and torch.equal(one["Lp"][i], a.Lp[i][:M, :M].cpu())
        assert torch.equal(one["tile_inv"][i][0], a.tile_inv[i][0].cpu())
        assert torch.equal(one["tile_inv"][i][1, :2, :2], a.tile_inv[i][1, :2, :2].cpu())
        assert one["tile_inv"][i][1].abs().sum() == one["tile_inv"][i][1, :2, :2].abs().sum() > 0
    b = hip.PreservedKeys(2, D200, 260, DEV)
    assert (a.ldl, a.tile_inv[0].shape[0]) == (200, 2) and (b.ldl, b.tile_inv[0].shape[0]) == (260, 3)
    b.load_state_dict(one)
    assert b.M == M and torch.equal(b.row_scale[:M], a.row_scale[:M])
    two = b.state_dict()
    for name in ("Yp", "Lp", "tile_inv"):
        for x, y in zip(one[name], two[name]):
            assert x.dtype == y.dtype == torch.float64 and torch.equal(x, y), name
    assert torch.equal(one["row_scale"], two["row_scale"])
    for target, match in ((hip.PreservedKeys(2, D200, 129, DEV), "capacity 129"), (hip.PreservedKeys(2, 384, 200, DEV), "d = 200"),
                          (hip.PreservedKeys(1, D200, 200, DEV), "2 layers")):
        with pytest.raises(hip.EmcidHipError, match=match):
            target.load_state_dict(one)
        assert target.M == 0 and not target.Yp[0].any() and not target.Lp[0].any()


def _symmetric(inputs):
    """The helpers' inputs with statistics that ARE symmetric: the upper triangle of Cov replaced by the mirror image of the lower
    one.  The recipe forms Cov = x^T x / 2d by an fp32 matrix product, and on the CPUs of the MI355X hosts that product is not
    symmetric at d = 200 or 136 (its (i, j) and (j, i) entries differ by fp32 roundings; it is at 256, 320, 384, and everywhere
    on the build machine).  The library factors lam C' by Cholesky and so reads the lower triangle only, while the helpers'
    reference hands the full matrix to an LU solve: the two then solve systems 1e-7 apart, and U differs by 1.2e-8 of max|U| at
    M = 130 (1.9e-7 at M = 0) — that is the "offset of the step at d = 200" DESIGN.md §3 recorded for the retain and release tests,
    neither the step's nor the solver's (an fp64 Cholesky, conjugate gradients and the LU solve with refinement all leave the same
    1.1e-8 of max|B| when the residual is formed with the full matrix).  Second moments are symmetric; with inputs that are, the
    helpers' reference and bar apply as they stand."""
    K, Zc, zs_t, Cov, W0 = inputs
    Cov = torch.tril(Cov) + torch.tril(Cov, -1).t()
    return K, Zc, zs_t, Cov.contiguous(), W0


@pytest.mark.parametrize("capacity", [260, 135], ids=["grown", "shrunk"])
def test_a_step_on_the_loaded_state_vs_primal_fp64(built, capacity):
    """N = 5 rows on the state loaded at another capacity: U against torch.linalg.solve on lam C' + P^T P + Kt^T Kt (the helpers'
    reference and bar), and the difference to the same step on the state the rows were built in (printed)."""
    ins, fac, a = built
    K, Zc, zs_t, Cov, W0 = ins[0]
    b = hip.PreservedKeys(2, D200, capacity, DEV)
    b.load_state_dict(a.state_dict())
    twin = hip.PreservedKeys(2, D200, 200, DEV)              # the original state, tensor for tensor (the shared one stays unwritten)
    for dst, src in zip(twin.Yp + twin.Lp + twin.tile_inv, a.Yp + a.Lp + a.tile_inv):
        dst.copy_(src)
    twin.row_scale.copy_(a.row_scale)
    twin.M = a.M
    ub = _step(K[M:], Zc[M:], zs_t[M:], W0, fac, b)["U"].cpu()
    ua = _step(K[M:], Zc[M:], zs_t[M:], W0, fac, twin)["U"].cpu()
    ref = _primal_u(K, Zc, zs_t, Cov, M, M + N)
    err = (ub - ref).abs().max().item() / ref.abs().max().item()
    same = (ub - ua).abs().max().item() / ref.abs().max().item()
    print(f"capacity {capacity}: U of a step on the loaded state {err:.3e} of max|U| from the primal solve, {same:.3e} from the step "
          f"at capacity 200")
    assert err <= U_BAR
    b.commit(N, hip.row_scale_of(EW, fac, LAM))
    assert b.M == M + N and b.state_dict()["Lp"][0].shape == (M + N, M + N)

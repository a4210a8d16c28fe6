"""num_edit_tokens = k > 1 on the prefix-trie forward, host side: the trie with query-only leaves (native builder and its numpy
twin), the pseudo-segments of the key gather, the per-rank concept ranges, the tokenization through the EOS and the k-row
v* reads.  No GPU needed."""
import hashlib
import os

import numpy as np
import pytest
import torch

from emcid_amd import clip_forward as cf, compute_z as cz, edit_engine as ee, emcid_main as em, host_text, synthetic as syn
from emcid_amd.emcid_hparams import EMCIDHyperParams

FIELDS = ("token", "depth", "anc", "lookup_node", "query_rows", "lookup_in_query", "position")


def _need_host():
    if not host_text.available():
        pytest.skip("libemcid_host.so not built")


def _random_multi(seed, B, S, k, vocab):
    """(ids, (B, k) lookups, eos) shaped like a k-token edit: a subject token before every EOS, then EOS, EOS + 1, ..."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, vocab, size=(B, S)).astype(np.int64)
    ids[:, 0] = 7
    eos = rng.integers(1, S, size=B).astype(np.int64)
    ids[np.arange(B), eos] = vocab + 1            # (the EOS token itself; rows behind it are never read)
    last = np.array([rng.integers(0, e) for e in eos], dtype=np.int64)
    return ids, cz.multi_token_lookup(last, eos, k), eos


@pytest.mark.parametrize("B,S,k,vocab,bucket,seed", [(1, 3, 2, 2, 1, 0), (40, 9, 3, 4, 1, 1), (200, 12, 6, 3, 256, 2),
                                                     (64, 20, 4, 30, 4, 3), (300, 6, 5, 2, 64, 4), (17, 30, 2, 50, 256, 5)])
def test_native_leaf_trie_equals_numpy_twin(B, S, k, vocab, bucket, seed):
    """emcid_trie_build_leaves (what the edit path runs) and build_trie_numpy's leaf form give the same arrays, positions
    included."""
    _need_host()
    ids, lk, eos = _random_multi(seed, B, S, k, vocab)
    a = cf.build_trie(ids, lk, "cpu", bucket=bucket, eos=eos, pad_token=vocab + 2)
    b = cf.build_trie_numpy(ids, lk, "cpu", bucket=bucket, eos=eos, pad_token=vocab + 2)
    assert a.n_nodes == b.n_nodes and a.max_position == b.max_position == int(max(lk.max(), eos.max()))
    assert a.max_token == (max(vocab + 1, 7, vocab + 2) if k > 2 else max(vocab + 1, 7))
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), f
    t = cf.build_trie(ids, lk, "cpu", bucket=bucket, eos=eos, pad_token=vocab + 2, tail=np.arange(5) * 3)
    assert t.tail.tolist() == [0, 3, 6, 9, 12] and torch.equal(t.anc, b.anc)


@pytest.mark.parametrize("native", [True, False])
def test_leaf_invariants(native):
    """Every lookup behind an EOS is a leaf: pad token, the EOS node's ancestor row and depth, own position EOS + j, one leaf
    per (EOS node, j); every other node has position == depth and ends its own chain; the query rows cover all B k lookups."""
    if native:
        _need_host()
    ids, lk, eos = _random_multi(11, 120, 10, 5, 3)
    ids[60:] = ids[:60]                      # duplicate prompts: their leaves are shared
    eos[60:], lk[60:] = eos[:60], lk[:60]
    build = cf.build_trie if native else cf.build_trie_numpy
    t = build(ids, lk, "cpu", bucket=64, eos=eos, pad_token=99)
    B, k = lk.shape
    ln = t.lookup_node.view(B, k)
    tok, depth, pos, anc = t.token, t.depth, t.position, t.anc
    leaves = set()
    for i in range(B):
        e_node = int(ln[i, 1])
        assert int(depth[e_node]) == eos[i] == int(pos[e_node]) and int(anc[e_node, eos[i]]) == e_node
        assert int(tok[e_node]) == ids[i, eos[i]]
        s = int(ln[i, 0])
        assert int(depth[s]) == lk[i, 0] and int(anc[e_node, lk[i, 0]]) == s
        for j in range(2, k):
            u = int(ln[i, j])
            assert int(tok[u]) == 99
            assert torch.equal(anc[u], anc[e_node]) and int(depth[u]) == int(depth[e_node])
            assert int(pos[u]) == eos[i] + j - 1
            leaves.add(u)
        if i < 60:
            assert torch.equal(ln[i + 60], ln[i])
    ordinary = [u for u in range(t.n_nodes) if u not in leaves]
    assert all(int(pos[u]) == int(depth[u]) and int(anc[u, int(depth[u])]) == u for u in ordinary)
    assert min(leaves) > max(ordinary)        # leaves numbered after every chain node
    assert len(leaves) == len({(int(ln[i, 1]), j) for i in range(B) for j in range(2, k)})
    q = t.query_rows[t.lookup_in_query]
    assert torch.equal(q.long(), t.lookup_node)


# sha256 of emcid_trie_export's image of the k = 1 builder before query-only leaves existed: the k = 1 bytes are unchanged
K1_IMAGES = {(40, 9, 5, 1, 0): (7120, "feba73533da251036f966e7a754b7c0675104ddf0ad077529c95630d31efe0eb"),
             (300, 12, 30, 256, 1): (99008, "01137d067c581c82497e52b4194eb748d6d1d76710c034bb4dfe79f013572df8"),
             (7, 4, 3, 4, 2): (480, "ebf3e78ae4a028ead74e38aac51bf56f08ac9e1edba3bba317471e70705909be")}


@pytest.mark.parametrize("key", list(K1_IMAGES))
def test_k1_trie_bytes_unchanged(key):
    _need_host()
    B, S, vocab, bucket, seed = key
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, vocab, size=(B, S)).astype(np.int64)
    ids[:, 0] = 7
    lk = rng.integers(0, S, size=B).astype(np.int64)
    def alloc(n):
        buf = np.zeros(n, dtype=np.uint8)
        return buf, buf.ctypes.data

    img, _ = host_text.build_trie_packed(ids, lk, bucket, alloc)
    assert (img.size, hashlib.sha256(img.tobytes()).hexdigest()) == K1_IMAGES[key]
    t = cf.build_trie(ids, lk, "cpu", bucket=bucket)
    assert t.position is t.depth and t.max_position == int(lk.max())


def test_concept_ranges_are_k_times_request_ranges():
    for world in range(1, 9):
        for n in (world, world + 1, 2 * world + 3, 5, 37):
            if n < world:
                continue
            for k in (1, 2, 3, 6):
                plan = ee.EncoderEditPlan(None, [0], "{}", 1.0, 0.5, None, None, {}, n * k, ee.ConceptShard(0, world),
                                          num_edit_tokens=k)
                covered = []
                for r in range(world):
                    lo, hi = plan.concept_bounds(r)
                    rlo, rhi = plan.shard.bounds(n, r)
                    assert (lo, hi) == (rlo * k, rhi * k)
                    covered.extend(range(lo, hi))
                assert covered == list(range(n * k))
    # the example of the issue: 5 requests, k = 3, 2 ranks -> 2 | 3 requests, 6 | 9 concept rows (not bounds(15) = 7 | 8)
    plan = ee.EncoderEditPlan(None, [0], "{}", 1.0, 0.5, None, None, {}, 15, ee.ConceptShard(0, 2), num_edit_tokens=3)
    assert [plan.concept_bounds(r) for r in range(2)] == [(0, 6), (6, 15)]


@pytest.mark.parametrize("k", [1, 2, 3, 6])
def test_pseudo_segments_rq_num_order(k):
    """Concept rq k + num is the mean over request rq's prompts (in prompt order) of their lookup num."""
    counts = [3, 1, 4, 2, 5]
    perm, cseg = ee.concept_segments(counts, k)
    off = np.concatenate([[0], np.cumsum(counts)])
    B = int(off[-1])
    assert sorted(perm.tolist()) == list(range(B * k)) and cseg.size == len(counts) * k + 1 and cseg[-1] == B * k
    for rq in range(len(counts)):
        for num in range(k):
            c = rq * k + num
            want = [p * k + num for p in range(off[rq], off[rq + 1])]
            assert perm[cseg[c]:cseg[c + 1]].tolist() == want
    # against the hooked path's gather (per-lookup means stacked, then "rq num" rows)
    vals = np.random.default_rng(0).standard_normal((B, k, 3))
    ours = np.stack([vals.reshape(B * k, 3)[perm[cseg[c]:cseg[c + 1]]].mean(0) for c in range(len(counts) * k)])
    ref = np.stack([np.stack([vals[off[r]:off[r + 1], num].mean(0) for num in range(k)]) for r in range(len(counts))])
    np.testing.assert_array_equal(ours, ref.reshape(-1, 3))


def _chunk_arrays(ch):
    return ch.ids, np.asarray(ch.lookup), ch.counts, None if ch.eos is None else np.asarray(ch.eos)


@pytest.mark.parametrize("k", [2, 3, 6])
def test_templated_path_equals_generic_path_multi_token(monkeypatch, k):
    """Rows kept through their EOS and the (B, k) lookups: the templated fast path (which serves this shape) and the generic one
    give the same ids, lookups, EOS positions and counts, and the lookups are those of the hooked path's padded batch."""
    _need_host()
    tok = syn.build_tokenizer(*syn.synthetic_vocab(syllables=True))
    if host_text.NativeClipBpe.for_tokenizer(tok) is None:
        pytest.skip("no native twin for the synthetic tokenizer")
    for reqs in (syn.make_requests(300, names="syllable"), syn.make_requests(40, ragged=True, names="syllable")):
        assert cz.templated_prompt_chunk(tok, reqs, reqs[0], num_edit_tokens=k) is not None
        monkeypatch.setenv("EMCID_TEMPLATED", "1")
        a = cz.prompt_chunk(tok, reqs, num_edit_tokens=k)
        monkeypatch.setenv("EMCID_TEMPLATED", "0")
        b = cz.prompt_chunk(tok, reqs, num_edit_tokens=k)
        ia, la, ca, ea = _chunk_arrays(a)
        ib, lb, cb, eb = _chunk_arrays(b)
        assert la.shape == lb.shape == (ia.shape[0], k) and list(ca) == list(cb)
        np.testing.assert_array_equal(la, lb)
        np.testing.assert_array_equal(ea, eb)
        assert ia.shape == ib.shape == (ia.shape[0], int(ea.max()) + 1)
        for i in range(ia.shape[0]):                      # (behind a row's EOS: whatever padding the route wrote, never read)
            assert ia[i, :ea[i] + 1].tolist() == ib[i, :eb[i] + 1].tolist()
        batch = cz.build_prompt_batch_multi(tok, reqs, "cpu", k)
        np.testing.assert_array_equal(batch.lookup_multi.numpy().T, la)
        for i in range(ia.shape[0]):
            assert batch.ids_host[i, :ea[i] + 1].tolist() == ia[i, :ea[i] + 1].tolist()


def test_padded_length_check():
    sh = ee.ConceptShard()
    ee._check_padded_length(sh, 75, 4, 77, "cpu")          # 77: the position table's size is allowed
    with pytest.raises(ValueError, match="max_position_embeddings"):
        ee._check_padded_length(sh, 76, 4, 77, "cpu")
    ee._check_padded_length(sh, 77, 2, 77, "cpu")


@pytest.mark.parametrize("k", [1, 3])
def test_native_vstar_reader_takes_k_row_files(tmp_path, k):
    """use_new_compute_z files of shape (k, hidden): the native batch reader serves them (k = 1: (1, hidden) and (hidden,)),
    flattened to the reference's "rq num" rows — the rows numpy's per-file path gives."""
    _need_host()
    reqs = syn.make_requests(70, ragged=True)
    hp = EMCIDHyperParams(**dict(syn.sd_hparams_dict(layers=(1, 2)), num_edit_tokens=k, use_new_compute_z=True))
    cache = str(tmp_path / "c") + "/"
    rng = np.random.default_rng(3)
    vs = []
    for i, r in enumerate(reqs):
        v = rng.standard_normal((k, 24)).astype(np.float32 if i % 3 else np.float64)
        if k == 1 and i % 2:
            v = v[0]
        path = syn.vstar_cache_path(cache, r)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez(path, v_star=v)
        vs.append(np.asarray(v, dtype=np.float32).reshape(k, 24))
    want = np.concatenate(vs, axis=0)
    names = [em.vstar_cache_name(cache, r, hp, i) for i, r in enumerate(reqs)]
    native = em._native_vstar_rows(names, 24, False, em._vstar_file_rows(hp))
    assert native is not None and not native[1].any()
    got = em.load_v_stars(reqs, hp, cache, width=24)
    np.testing.assert_array_equal(got.numpy(), want)
    np.testing.assert_array_equal(em.load_v_stars(reqs, hp, cache).numpy(), want)     # numpy's per-file path
    if k > 1:       # a file of another row count is not served natively and fails numpy's shape check like the reference's
        np.savez(syn.vstar_cache_path(cache, reqs[5]), v_star=np.zeros((k + 1, 24), np.float32))
        with pytest.raises(ValueError):
            em.load_v_stars(reqs, hp, cache, width=24)

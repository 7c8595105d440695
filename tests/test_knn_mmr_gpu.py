"""Diverse top-k by maximal marginal relevance on the GPU (K16, csrc/knn_mmr.hip)
against the exactly rounded oracle of tests/_mmr_ref.py.

A comparison with the oracle is made only where the oracle's minimum decision margin (the
winner's value minus the best value of a candidate with other bytes, over every query and step)
is at least ``margin_bound(D) = 64 (D + 16) 2^-53``: the test asserts that for every case and
leaves out no query. Positions must then be equal and values agree to 1e-12. Everything else
here is bit for bit: lam = 1 against ``search``, ``search_mmr`` against its three stages run
from the host, a compacted index against a fresh one, two threads against one.
"""
from __future__ import annotations

import threading

import numpy as np
import pytest

import _mmr_ref as ref
from _data import clustered_corpus, labels_for
from oracle.knn import cosine_scores

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def _compose(ix, q, k, fetch_k, lam, label=-1, row_offset=0):
    """search_mmr's stages from the host: the fetch search, K16 on its output, the gather."""
    s, r, s64 = ix.search(q, fetch_k, label=label, with_f64=True)
    pos = ix.mmr_select(r, s64, k, lam)
    gs, gs64, gr = ref.gather(pos, s, s64, r)
    return gs, np.where(gr >= 0, gr + row_offset, -1), gs64, pos


# ---------------------------------------------------------------- K16 alone
_K16_CORPUS = {}


def _k16_corpus(dim):
    """One corpus, index and cosine cache per width (shared by the cases; never changed)."""
    from app.vector_store import FlatIndex

    if dim not in _K16_CORPUS:
        x = clustered_corpus(3000, dim, 400 + dim, n_clusters=12, spread=0.3, dup_frac=0.05)
        ix = FlatIndex(dim)
        ix.add(x)
        _K16_CORPUS[dim] = (x, ix, ref.RowCosine(x))
    return _K16_CORPUS[dim]


def _k16_candidates(x, nq, m, empties, seed):
    """Per query the m best rows by the numpy f64 cosine in the search's order; ``empties[i]``
    slots at the tail of query i's list are empty (-1 / -inf)."""
    rng = np.random.default_rng(seed)
    q = x[rng.integers(0, len(x), nq)] + 0.05 * rng.standard_normal((nq, x.shape[1])).astype(np.float32)
    cos = cosine_scores(x, q)
    rows = np.empty((nq, m), np.int64)
    s = np.empty((nq, m), np.float64)
    for i in range(nq):
        order = np.lexsort((np.arange(len(x)), -cos[i]))[:m]
        rows[i], s[i] = order, cos[i, order]
        e = empties[i % len(empties)]
        if e:
            rows[i, m - e:] = -1
            s[i, m - e:] = NEG_INF
    return rows, s


# dim, m, k, lam, nq, empty tail slots per query (cycled), device pointers
K16_CASES = [
    (100, 1, 1, 0.5, 1, (0,), False),
    (100, 1, 1, 0.0, 3, (0, 1, 0), True),        # a list with no candidate at all
    (128, 15, 10, 0.3, 3, (0,), True),
    (128, 16, 16, 0.5, 3, (0, 3, 9), False),     # fewer valid candidates than k
    (128, 17, 10, 0.0, 3, (0, 8, 16), True),
    (128, 64, 10, 0.5, 257, (0, 0, 60), True),
    (512, 64, 64, 0.3, 3, (0, 1, 40), False),
    (512, 200, 10, 1.0, 3, (0,), True),
    (1536, 200, 10, 0.5, 3, (0, 195, 0), False),
    (100, 200, 200, 0.3, 1, (0,), True),
    (512, 1024, 10, 0.5, 3, (0, 0, 1000), True),
    (100, 1024, 1024, 0.5, 1, (640,), False),    # k = M at the limit; 384 candidates, the rest padding
    (1536, 17, 1, 0.3, 3, (0,), True),
]


@pytest.mark.parametrize("dim,m,k,lam,nq,empties,device", K16_CASES)
def test_k16_against_the_oracle(cuda, dim, m, k, lam, nq, empties, device):
    import torch

    x, ix, rc = _k16_corpus(dim)
    rows, s = _k16_candidates(x, nq, m, empties, 7 * m + k)
    opos, oval, margin = ref.mmr_oracle(rc, rows, s, k, lam)
    print(f"margin {margin:.3e} bound {ref.margin_bound(dim):.3e}")
    assert margin >= ref.margin_bound(dim)
    if device:
        pos, val = ix.mmr_select(torch.from_numpy(rows).to(cuda), torch.from_numpy(s).to(cuda), k, lam,
                                 with_values=True)
        pos, val = pos.cpu().numpy(), val.cpu().numpy()
    else:
        pos, val = ix.mmr_select(rows, s, k, lam, with_values=True)
    assert pos.dtype == np.int32 and val.dtype == np.float64
    np.testing.assert_array_equal(pos, opos)
    assert np.array_equal(val == NEG_INF, oval == NEG_INF)
    ok = oval > NEG_INF
    print(f"max |v - oracle| {np.abs(val[ok] - oval[ok]).max() if ok.any() else 0.0:.3e}")
    assert np.all(np.abs(val[ok] - oval[ok]) <= 1e-12)
    # without the values the positions are the same
    if not device:
        np.testing.assert_array_equal(ix.mmr_select(rows, s, k, lam), pos)


def test_k16_refuses_rows_past_the_index(cuda):
    import torch

    from app._native import NativeError

    x, ix, _ = _k16_corpus(128)
    rows, s = _k16_candidates(x, 2, 16, (0,), 5)
    rows[1, 3] = len(x)  # the first id the index has not handed out
    for dev in (False, True):
        a = (torch.from_numpy(rows).to(cuda), torch.from_numpy(s).to(cuda)) if dev else (rows, s)
        with pytest.raises(NativeError, match="cand_rows"):
            ix.mmr_select(*a, 4, 0.5)
    rows[1, 3] = len(x) - 1
    assert ix.mmr_select(rows, s, 4, 0.5).shape == (2, 4)  # the index still answers


# ---------------------------------------------------------------- the point of the feature
def _centres(n_clusters, d, seed):
    """clustered_corpus's centres: its generator's first draw."""
    return np.random.default_rng(seed).standard_normal((n_clusters, d)).astype(np.float32)


def test_mmr_covers_more_clusters_than_plain_search(cuda):
    from app.vector_store import FlatIndex

    d, n, nc, seed = 128, 600, 40, 79  # ~15 rows per cluster: the 64 best reach into other clusters
    x = clustered_corpus(n, d, seed, n_clusters=nc, spread=0.05, dup_frac=0.05)
    centres = _centres(nc, d, seed)
    cluster = np.argmax(cosine_scores(centres, x), axis=1)  # nearest centre of every row
    big = np.flatnonzero(np.bincount(cluster[np.abs(x).sum(1) > 0], minlength=nc) >= 10)
    assert len(big) >= 30
    q = centres[big]  # a query on the centre of every cluster that can fill a plain top-10
    ix = FlatIndex(d)
    ix.add(x)
    rc = ref.RowCosine(x)
    _, plain = ix.search(q, 10)
    s, r, s64 = ix.search(q, 64, with_f64=True)
    opos, _, margin = ref.mmr_oracle(rc, r, s64, 10, 0.5)
    assert margin >= ref.margin_bound(d)
    gs, gr = ix.search_mmr(q, 10, fetch_k=64, lam=0.5)
    es, er = ref.gather(opos, s, r)
    np.testing.assert_array_equal(gr, er)
    _bits_equal(gs, es)
    for i in range(len(q)):
        assert len(set(cluster[plain[i]])) == 1  # ten rows of the query's own cluster
        assert len(set(cluster[gr[i]])) > 1
    ix.close()


def test_duplicates_ties_and_zero_rows(cuda):
    """Forty random unit rows (pairwise cosines ~ +-0.1) and a query along their sum, tilted
    towards row 11, with two more copies of row 11 and two zero rows. Every distinct row keeps
    s - p above -0.3 while a copy of the selected row 11 has s - 1 ~ -0.57: the copies are
    chosen after every distinct candidate, and among themselves by position. A zero row scores
    0 against the query and against every row, so its value is exactly 0 at every step."""
    from app.vector_store import FlatIndex

    d, n = 100, 40
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = (x.sum(0) + 2.0 * x[11]).astype(np.float32)[None, :]
    x[23] = x[11]
    x[30] = x[11]
    x[5] = 0.0
    x[17] = 0.0
    ix = FlatIndex(d)
    ix.add(x)
    rc = ref.RowCosine(x)
    s, r, s64 = ix.search(q, n, with_f64=True)
    assert r[0, :3].tolist() == [11, 23, 30] and s64[0, 0] == s64[0, 1] == s64[0, 2]
    assert np.all(s64[0][np.isin(r[0], (5, 17))] == 0.0)
    opos, oval, margin = ref.mmr_oracle(rc, r, s64, n, 0.5)
    assert margin >= ref.margin_bound(d)
    pos, val = ix.mmr_select(r, s64, n, 0.5, with_values=True)
    np.testing.assert_array_equal(pos, opos)
    assert np.all(np.abs(val - oval) <= 1e-12)
    order = r[0][pos[0]].tolist()
    assert order[0] == 11 and sorted(order) == list(range(n))
    assert order[-2:] == [23, 30]  # the copies last; equal values: the smaller position first
    assert val[0, -2] == val[0, -1] < val[0, :-2].min()
    assert order.index(5) + 1 == order.index(17)  # the zero rows tie at exactly 0
    assert val[0, order.index(5)] == 0.0 and val[0, order.index(17)] == 0.0
    gs, gr = ix.search_mmr(q, n, fetch_k=n, lam=0.5)
    assert gr[0].tolist() == order
    ix.close()


# ---------------------------------------------------------------- lam = 1 and the composition
# path: dim, rows, queries, fetch_k (plan_search: K7s for nq <= 64, v3's 256-query groups for
# k <= 64, v1 for 64 < k <= 256, K7g above 512 dimensions)
PATHS = {
    "k7s": (512, 20_000, 33, 40),
    "v3": (128, 20_000, 300, 64),
    "v1": (100, 20_000, 40, 200),
    "k7g": (640, 5_000, 20, 40),
}
_PATH_INDEX = {}


def _path_index(name):
    from app.vector_store import FlatIndex

    if name not in _PATH_INDEX:
        dim, n, nq, fetch_k = PATHS[name]
        x = clustered_corpus(n, dim, 600 + dim, n_clusters=32, spread=0.05, dup_frac=0.05)
        lab = labels_for(n, 4, 601)
        lab[:5] = 7  # a user who owns fewer rows than fetch_k; nobody has label 9
        rng = np.random.default_rng(602)
        q = (x[rng.integers(0, n, nq)] + 0.02 * rng.standard_normal((nq, dim))).astype(np.float32)
        ix = FlatIndex(dim)
        ix.add(x, lab)
        _PATH_INDEX[name] = (ix, q, fetch_k)
    return _PATH_INDEX[name]


@pytest.mark.parametrize("path", list(PATHS))
def test_lambda_one_is_search(cuda, path):
    ix, q, fetch_k = _path_index(path)
    for label in (-1, 2):
        s, r, s64 = ix.search(q, 10, label=label, with_f64=True)
        ms, mr, ms64 = ix.search_mmr(q, 10, fetch_k=fetch_k, lam=1.0, label=label, with_f64=True)
        np.testing.assert_array_equal(mr, r)
        _bits_equal(ms, s)
        _bits_equal(ms64, s64)


@pytest.mark.parametrize("path", list(PATHS))
def test_search_mmr_is_the_composition_of_its_stages(cuda, path):
    import torch

    ix, q, fetch_k = _path_index(path)
    nq = len(q)
    per_query = np.array([(-1, 0, 1, 2, 3, 7, 9)[i % 7] for i in range(nq)], np.int32)
    for label, off, lam in ((-1, 0, 0.5), (2, 1_000_000, 0.3), (per_query, 12345, 0.5)):
        es, er, es64, pos = _compose(ix, q, 10, fetch_k, lam, label=label, row_offset=off)
        gs, gr, gs64 = ix.search_mmr(q, 10, fetch_k=fetch_k, lam=lam, label=label, row_offset=off, with_f64=True)
        np.testing.assert_array_equal(gr, er)
        _bits_equal(gs, es)
        _bits_equal(gs64, es64)
        assert np.any(pos != np.arange(10, dtype=np.int32))  # the selection is not the identity
        if isinstance(label, np.ndarray):
            few, none = np.flatnonzero(label == 7), np.flatnonzero(label == 9)
            assert np.all(gr[few, :5] >= off) and np.all(gr[few, 5:] == -1) and np.all(gs[few, 5:] == NEG_INF)
            assert np.all(gr[none] == -1) and np.all(gs64[none] == NEG_INF)
    # device pointers: the same bytes
    lab_t = torch.from_numpy(per_query).to(cuda)
    ts, tr, ts64 = ix.search_mmr(torch.from_numpy(q).to(cuda), 10, fetch_k=fetch_k, lam=0.5, label=lab_t,
                                 row_offset=12345, with_f64=True)
    np.testing.assert_array_equal(tr.cpu().numpy(), gr)
    _bits_equal(ts.cpu().numpy(), gs)
    _bits_equal(ts64.cpu().numpy(), gs64)
    # without the f64 scores, and with the default fetch_k = min(4 k, 1024)
    ds, dr = ix.search_mmr(q[:5], 10, lam=0.5)
    es, er, _, _ = _compose(ix, q[:5], 10, 40, 0.5)
    np.testing.assert_array_equal(dr, er)
    _bits_equal(ds, es)


def test_search_mmr_on_an_empty_index_and_argument_errors(cuda):
    from app._native import NativeError
    from app.vector_store import FlatIndex

    ix = FlatIndex(64)
    s, r = ix.search_mmr(np.ones((2, 64), np.float32), 3, fetch_k=8)
    assert np.all(r == -1) and np.all(s == NEG_INF)
    for kw in (dict(k=0), dict(k=9, fetch_k=8), dict(k=3, fetch_k=1025), dict(k=3, lam=1.5), dict(k=3, lam=float("nan"))):
        with pytest.raises(NativeError):
            ix.search_mmr(np.ones((2, 64), np.float32), **kw)
    ix.close()


# ---------------------------------------------------------------- compaction and threads
def test_compacted_index_answers_like_a_fresh_one(cuda):
    from app.vector_store import FlatIndex

    d, n = 128, 6000
    x = clustered_corpus(n, d, 90, n_clusters=24, spread=0.05)
    lab = labels_for(n, 3, 91)
    rng = np.random.default_rng(92)
    dead = rng.choice(n, n // 3, replace=False)
    live = np.setdiff1d(np.arange(n), dead)
    q = (x[rng.integers(0, n, 70)] + 0.02 * rng.standard_normal((70, d))).astype(np.float32)
    ix = FlatIndex(d)
    ix.add(x, lab)
    ix.delete(dead)
    before = ix.search_mmr(q, 10, fetch_k=64, lam=0.5, label=1, with_f64=True)
    remap = ix.compact()
    fresh = FlatIndex(d)
    fresh.add(x[live], lab[live])
    for label in (-1, 1):
        a = ix.search_mmr(q, 10, fetch_k=64, lam=0.5, label=label, with_f64=True)
        b = fresh.search_mmr(q, 10, fetch_k=64, lam=0.5, label=label, with_f64=True)
        np.testing.assert_array_equal(a[1], b[1])
        _bits_equal(a[0], b[0])
        _bits_equal(a[2], b[2])
    # and like itself before, through the remap
    np.testing.assert_array_equal(np.where(before[1] >= 0, remap[np.maximum(before[1], 0)], -1), a[1])
    _bits_equal(before[2], a[2])
    ix.close()
    fresh.close()


def test_two_threads_give_the_serial_results(cuda):
    ix, q, fetch_k = _path_index("v3")
    jobs = [(q[:150], 0.5, -1), (q[150:], 0.3, 2)]
    serial = [ix.search_mmr(a, 10, fetch_k=fetch_k, lam=lam, label=f, with_f64=True) for a, lam, f in jobs]
    got, errs = [[None] * 3, [None] * 3], []

    def work(i):
        try:
            a, lam, f = jobs[i]
            for rep in range(3):
                got[i][rep] = ix.search_mmr(a, 10, fetch_k=fetch_k, lam=lam, label=f, with_f64=True)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(2):
        for rep in range(3):
            for a, b in zip(got[i][rep], serial[i]):
                _bits_equal(a, b)


# ---------------------------------------------------------------- the drop-in surfaces
def _patch_stores(monkeypatch, tmp_path, name):
    from app.cache import clear_all_caches
    from app.ml import index_build, retrieve
    from app.storage.lancedb_store import LanceDBStore
    from app.storage.schema import MetadataStore

    store = LanceDBStore(str(tmp_path / name))
    meta = MetadataStore(str(tmp_path / name / "metadata.sqlite3"))
    monkeypatch.setattr(index_build, "_LANCEDB_STORE", store)
    monkeypatch.setattr(index_build, "_VERSION_FILE", tmp_path / "versions.json")
    monkeypatch.setattr(retrieve, "_LANCEDB_STORE", store)
    monkeypatch.setattr(retrieve, "_METADATA_STORE", meta)
    monkeypatch.setattr(retrieve, "get_index_version", index_build.get_index_version)
    clear_all_caches()
    return store, meta


def _store_unit(vec):
    from app.storage.lancedb_store import LanceDBStore

    return np.asarray(LanceDBStore._normalize(vec), np.float32)[None, :]


def _batch_unit(vec):
    q = np.asarray(vec, np.float32)[None, :]
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def _host_hits(table, user, q, k, fetch_k, lam):
    """What search_text / search_batch must return with mmr_lambda set, from their parts (q: the
    query as the surface normalises it)."""
    es, er, _, _ = _compose(table.index, q, k, fetch_k, lam, label=table.labels[user])
    return [{"chunk_id": table.chunk_ids[row], "score": 1.0 - float(np.float32(1.0) - np.float32(sc)),
             "meta": {"i": int(table.chunk_ids[row][1:])}} for sc, row in zip(es[0], er[0]) if row >= 0]


def test_store_and_search_batch_with_mmr(cuda, tmp_path, monkeypatch):
    from app.retrieval import search_batch
    from app.storage.lancedb_store import VectorRow

    store, _ = _patch_stores(monkeypatch, tmp_path, "db_mmr")
    users = ["ann", "ben"]
    x = clustered_corpus(600, 384, 11, n_clusters=30, spread=0.05)
    x = x[np.abs(x).sum(1) > 0]
    own = np.random.default_rng(12).integers(0, 2, len(x))
    store.upsert_text_vectors([VectorRow(chunk_id=f"t{i}", user_id=users[own[i]], document_id="d", modality="text",
                                         embedding=x[i], meta={"i": i}) for i in range(len(x))])
    table = store._text_table
    vecs = _centres(30, 384, 11)[:4]
    for i, u in enumerate(["ann", "ben", "ann", "ben"]):
        want = _host_hits(table, u, _store_unit(vecs[i]), 8, 40, 0.5)
        assert store.search_text(u, vecs[i].tolist(), 8, mmr_lambda=0.5, fetch_k=40) == want
        assert search_batch("text", u, vecs[i:i + 1], 8, mmr_lambda=0.5, fetch_k=40) == [
            _host_hits(table, u, _batch_unit(vecs[i]), 8, 40, 0.5)]
        plain = store.search_text(u, vecs[i].tolist(), 8)
        assert plain == store.search_text(u, vecs[i].tolist(), 8, mmr_lambda=None)
        assert [h["chunk_id"] for h in plain] != [h["chunk_id"] for h in want]
        # the default fetch_k is min(4 top_k, 1024)
        assert store.search_text(u, vecs[i].tolist(), 8, mmr_lambda=0.5) == _host_hits(table, u, _store_unit(vecs[i]),
                                                                                        8, 32, 0.5)
    who = ["ann", "ben", "nobody", "ann"]
    got = search_batch("text", who, vecs, 8, mmr_lambda=0.3, fetch_k=24)
    assert got[2] == []
    for i in (0, 1, 3):
        assert got[i] == _host_hits(table, who[i], _batch_unit(vecs[i]), 8, 24, 0.3)
    assert store.search_image("ann", vecs[0].tolist(), 3, mmr_lambda=0.5) == []


def test_retrieve_batch_with_mmr(cuda, tmp_path, monkeypatch):
    """retrieve_batch(mmr_lambda, mmr_fetch_k) is retrieve_batch over a search_batch that is
    always called with those two arguments: MMR sits in each modality's search, before rerank
    and fusion, and nowhere else."""
    import app.retrieval as retrieval
    from app.ml import index_build
    from app.storage.schema import Chunk

    _, meta = _patch_stores(monkeypatch, tmp_path, "db_mmr_retrieve")
    rng = np.random.default_rng(3)
    words = [f"w{i}" for i in range(60)]
    nodes = [{"id": f"doc{d}", "text": " ".join(" ".join(rng.choice(words, 10)) + "." for _ in range(3)),
              "metadata": {"source": "pdf", "page_no": d}} for d in range(40)]  # one short chunk per document
    chunks = index_build.index_text_nodes("ann", nodes)
    meta.upsert_chunks([Chunk(id=s["chunk_id"], document_id=s["metadata"]["doc_id"], modality="text", text=s["text"],
                              meta=s["metadata"]) for s in chunks])
    qs = ["w1 w2 w3 w4", "w50 w12 w7"]
    with_mmr = retrieval.retrieve_batch("ann", qs, top_k_text=6, rerank=False, mmr_lambda=0.1, mmr_fetch_k=24)
    plain = retrieval.retrieve_batch("ann", qs, top_k_text=6, rerank=False)
    calls = []
    real = retrieval.search_batch

    def forced(modality, user_id, vecs, top_k, mmr_lambda=None, fetch_k=None):
        calls.append((modality, mmr_lambda, fetch_k))
        return real(modality, user_id, vecs, top_k, mmr_lambda=0.1, fetch_k=24)

    monkeypatch.setattr(retrieval, "search_batch", forced)
    composed = retrieval.retrieve_batch("ann", qs, top_k_text=6, rerank=False)
    assert sorted(calls) == [("image", None, None), ("text", None, None)]
    assert with_mmr == composed
    assert all(with_mmr) and with_mmr != plain

"""kNN search with one label filter per query (mrag_knn_search_labels, FlatIndex.search with an
array for ``label``): a batch of different users' queries in one scan.

Two yardsticks for every case:
  * the oracle, called once per distinct filter value of the batch and scattered into place:
    rows bit-exact, f32 scores within 1e-6 of the f32 rounding of the oracle's f64;
  * the engine's own unchanged single-label search, run once per distinct filter: rows, f32
    scores and f64 scores must be EQUAL to it (both rescore the same rows with the same f64
    arithmetic, whatever scan found them).

Row labels: U users of skewed sizes (weights 0.8^u) and 2 % tombstones. Query filters are drawn
from 0 .. U + 1, so two users own nothing, and every 97th query carries ANY. Which kernels each
shape takes is pinned in tests/test_knn_labels_plan_cpu.py.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from _data import clustered_corpus, unit_rows
from oracle.knn import flat_cosine_topk

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-6
ANY = -1


def _skewed_labels(n, users, seed):
    rng = np.random.default_rng(seed)
    w = 0.8 ** np.arange(users)
    lab = rng.choice(users, n, p=w / w.sum()).astype(np.int32)
    lab[rng.choice(n, n // 50, replace=False)] = -2
    return lab


def _filters(nq, users, seed):
    f = np.random.default_rng(seed).integers(0, users + 2, nq).astype(np.int32)
    f[::97] = ANY
    return f


def _index(x, lab):
    """Rows with their labels; the rows labelled -2 are added under label 0 and deleted."""
    from app.vector_store import FlatIndex

    ix = FlatIndex(x.shape[1])
    ix.add(x, np.maximum(lab, 0))
    dead = np.nonzero(lab < 0)[0]
    if dead.size:
        ix.delete(dead)
    return ix


def _oracle(x, lab, q, k, f, row_offset=0):
    os_ = np.full((len(q), k), -np.inf)
    or_ = np.full((len(q), k), -1, np.int64)
    for L in np.unique(f):
        sel = np.nonzero(f == L)[0]
        os_[sel], or_[sel] = flat_cosine_topk(x, lab, q[sel], k, label_filter=int(L), row_offset=row_offset)
    return os_, or_


def _single_label(ix, q, k, f):
    """The unchanged path: one single-label search per distinct filter, scattered into place."""
    s = np.empty((len(q), k), np.float32)
    r = np.empty((len(q), k), np.int64)
    s64 = np.empty((len(q), k), np.float64)
    for L in np.unique(f):
        sel = np.nonzero(f == L)[0]
        s[sel], r[sel], s64[sel] = ix.search(q[sel], k, label=int(L), with_f64=True)
    return s, r, s64


def _labelled(ix, q, k, f):
    """The per-query entry point even where every filter is the same (FlatIndex.search sends such
    an array to the single-label search)."""
    return ix._search_labels(q, k, f, 0, True, group_equal=False)


def _check(got, os_, or_, ref=None):
    gs, gr = np.asarray(got[0]), np.asarray(got[1])
    assert gr.shape == or_.shape
    np.testing.assert_array_equal(gr, or_)
    valid = or_ >= 0
    assert np.all(np.isneginf(gs[~valid]))
    np.testing.assert_allclose(gs[valid], os_[valid].astype(np.float32), rtol=0, atol=SCORE_TOL)
    if ref is not None:
        np.testing.assert_array_equal(gr, ref[1])
        np.testing.assert_array_equal(gs, ref[0])
        np.testing.assert_array_equal(np.asarray(got[2]), ref[2])


def _run(ix, x, lab, q, k, f):
    got = ix.search(q, k, label=f, with_f64=True)
    os_, or_ = _oracle(x, lab, q, k, f)
    _check(got, os_, or_, _single_label(ix, q, k, f))
    return got, or_


@pytest.mark.parametrize("dim,k,nq", [(128, 10, 300), (384, 12, 65), (512, 16, 257), (256, 50, 130)])
def test_v3_groups_of_256(cuda, dim, k, nq):
    """v3 with 256-query groups (QB = 4, no sample pass at this size): partly filled last groups,
    every width, k at and above the per-lane list depth."""
    n, users = 20_000, 40
    x = unit_rows(n, dim, 300 + dim)
    lab = _skewed_labels(n, users, 301 + dim)
    q = unit_rows(nq, dim, 302 + dim)
    f = _filters(nq, users, 303 + dim)
    ix = _index(x, lab)
    _, or_ = _run(ix, x, lab, q, k, f)
    # the inputs exercise "no matches" and "fewer than k matches" (by the oracle alone)
    assert np.any(or_[:, 0] < 0) and np.any((or_[:, 0] >= 0) & (or_[:, -1] < 0))


@pytest.mark.parametrize("dim", [384, 512])
@pytest.mark.parametrize("k", [12, 50])
def test_k7s_small_batches(cuda, dim, k):
    """K7s (QB = 1): batches of 1, 7 and 64 queries; each row of the 64-query result also equals
    the corresponding one-query labelled search."""
    n, users = 20_000, 40
    x = unit_rows(n, dim, 310 + dim)
    lab = _skewed_labels(n, users, 311 + dim)
    q = unit_rows(64, dim, 312 + dim)
    f = _filters(64, users, 313 + dim + k)
    ix = _index(x, lab)
    os_, or_ = _oracle(x, lab, q, k, f)
    ref = _single_label(ix, q, k, f)
    for nq in (1, 7, 64):
        got = _labelled(ix, q[:nq], k, f[:nq])
        _check(got, os_[:nq], or_[:nq], tuple(a[:nq] for a in ref))
    for i in range(64):
        s1, r1, d1 = _labelled(ix, q[i], k, f[i:i + 1])
        np.testing.assert_array_equal(r1[0], got[1][i])
        np.testing.assert_array_equal(s1[0], got[0][i])
        np.testing.assert_array_equal(d1[0], got[2][i])


@pytest.fixture(scope="module")
def sampled_corpus():
    """The corpus of test_seeded_threshold_prepass with 12 skewed users, 1000 queries (half of
    them near rows), and its index; shared by the two sample-pass cases."""
    x = clustered_corpus(270_000, 128, 11, n_clusters=64, spread=0.05, dup_frac=0.05)
    lab = _skewed_labels(len(x), 12, 321)
    rng = np.random.default_rng(13)
    q = np.concatenate([x[rng.integers(0, len(x), 500)] + 0.01 * rng.standard_normal((500, 128)).astype(np.float32),
                        rng.standard_normal((500, 128)).astype(np.float32)])
    f = _filters(1000, 12, 323)
    return x, lab, q, f, {}


@pytest.mark.parametrize("k", [10, 32])
def test_sample_passes(cuda, sampled_corpus, k):
    """k = 10 takes the counting sample pass (MODE 2, the resolve kernel, a main scan that skips
    the sampled tiles); k = 32 the seed-only pass (MODE 1): the mask sits in the shared tile tail,
    so a row of another user must neither seed a query's threshold nor be listed for it."""
    x, lab, q, f, cache = sampled_corpus
    if "ix" not in cache:
        cache["ix"] = _index(x, lab)
    _run(cache["ix"], x, lab, q, k, f)


@pytest.mark.parametrize("n,dim,k,nq", [(30_000, 100, 100, 40), (5_000, 640, 10, 70), (5_000, 128, 300, 5),
                                        (5_000, 256, 100, 40), (5_000, 512, 100, 40)])
def test_deep_k_and_wide_rows(cuda, n, dim, k, nq):
    """k > 64 on v1 (per-lane masks; dims 100 and 256: its two labelled top-k instances), and K7g
    for rows wider than 512, k above 256 and deep k at 512 dims (where v1 has no such instance)."""
    users = 40
    x = unit_rows(n, dim, 330 + dim)
    lab = _skewed_labels(n, users, 331 + dim)
    q = unit_rows(nq, dim, 332 + dim)
    f = _filters(nq, users, 333 + dim)
    f[1] = 0  # the largest user: more than k rows at every size here
    _run(_index(x, lab), x, lab, q, k, f)


@pytest.mark.parametrize("nq", [48, 300])
def test_collect_pass_with_labels(cuda, nq):
    """Near-duplicate clusters defeat the fp16 certificate, so the failing queries are compacted
    through fail_list and K7c must look each one's filter up by its original query slot. The
    inputs are judged by the unchanged path first; nq = 300 fails more than 256 queries, so two
    collect groups run."""
    x = clustered_corpus(30_000, 512, 7, n_clusters=8, spread=0.01, dup_frac=0.2)
    lab = (np.arange(len(x)) % 3).astype(np.int32)
    q = x[np.random.default_rng(3).integers(0, len(x), nq)] + 0.001
    f = np.random.default_rng(4).integers(-1, 3, nq).astype(np.int32)  # the three users and ANY
    from app.vector_store import FlatIndex

    ix = FlatIndex(512)
    ix.add(x, lab)
    ix.search(q, 10, label=0)
    assert ix.last_stats()[0] > (256 if nq > 256 else 0), "the corpus must defeat the certificate on the unchanged path"
    got = ix.search(q, 10, label=f, with_f64=True)
    unc = ix.last_stats()[0]
    print(f"nq {nq}: uncertified {unc}")
    assert unc > (256 if nq > 256 else 0)
    os_, or_ = _oracle(x, lab, q, 10, f)
    _check(got, os_, or_, _single_label(ix, q, 10, f))


@pytest.mark.parametrize("dim", [100, 256, 384])
def test_small_tables_collect_at_every_width(cuda, dim):
    """Tables of a few tiles with k above what the split lists hold: K8 cannot certify, so K7c's
    labelled instance of this width runs with a -inf threshold, where only the mask keeps other
    users' rows and padding out (the 512-wide instance: test_collect_pass_with_labels)."""
    from app.vector_store import FlatIndex

    rng = np.random.default_rng(340 + dim)
    f = np.array([0, 1, 2, ANY, 5, 1, 0], np.int32)
    for n in (40, 130):
        x = rng.standard_normal((n, dim)).astype(np.float32)
        lab = rng.integers(0, 3, n).astype(np.int32)
        q = rng.standard_normal((len(f), dim)).astype(np.float32)
        ix = FlatIndex(dim)
        ix.add(x, lab)
        got = ix.search(q, 50, label=f, with_f64=True)
        assert ix.last_stats()[0] > 0
        _check(got, *_oracle(x, lab, q, 50, f), _single_label(ix, q, 50, f))
        ix.close()


def test_edges(cuda):
    import torch

    from app import _native
    from app.vector_store import FlatIndex

    n, dim, k = 3000, 128, 10
    x = unit_rows(n, dim, 350)
    lab = (np.arange(n) % 4).astype(np.int32)
    lab[:7] = 5  # a user with fewer than k rows
    lab[7] = 6   # ... and one with a single row
    ix = FlatIndex(dim)
    ix.add(x, lab)
    gone = np.arange(100, 400)  # tombstoned by set_labels after add
    ix.set_labels(gone, -2)
    lab[gone] = -2
    ix.set_labels([8, 9], 7)  # relabelled after add
    lab[[8, 9]] = 7
    q = unit_rows(9, dim, 351)
    f = np.array([0, 5, 6, 7, 9, ANY, 3, 5, 1], np.int32)  # user 9 owns nothing
    os_, or_ = _oracle(x, lab, q, k, f)
    assert (or_[1] >= 0).sum() == 7 and (or_[2] >= 0).sum() == 1 and (or_[4] >= 0).sum() == 0
    _check(ix.search(q, k, label=f, with_f64=True), os_, or_, _single_label(ix, q, k, f))
    # an all-ANY array equals label=-1, on the labelled kernels and as FlatIndex.search routes it
    b = ix.search(q, k, label=-1, with_f64=True)
    for a in (_labelled(ix, q, k, np.full(9, ANY, np.int32)), ix.search(q, k, label=np.full(9, ANY, np.int32),
                                                                        with_f64=True)):
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)
    s, r = ix.search(qt := torch.from_numpy(q).to(cuda), k, label=torch.full((9,), 3, dtype=torch.int32))
    np.testing.assert_array_equal(r.cpu().numpy(), ix.search(q, k, label=3)[1])  # equal entries, tensors
    # torch tensors for queries and filters, row offset, f64 scores
    s, r, s64 = ix.search(qt, k, label=torch.from_numpy(f).to(cuda), row_offset=1000, with_f64=True)
    oo_s, oo_r = _oracle(x, lab, q, k, f, row_offset=1000)
    _check((s.cpu().numpy(), r.cpu().numpy()), oo_s, oo_r)
    valid = oo_r >= 0
    np.testing.assert_allclose(s64.cpu().numpy()[valid], oo_s[valid], rtol=0, atol=1e-12)
    assert np.all(np.isneginf(s64.cpu().numpy()[~valid]))
    s2, r2 = ix.search(qt, k, label=f, row_offset=1000)  # tensor queries, array filters
    np.testing.assert_array_equal(r2.cpu().numpy(), oo_r)
    # wrong length, invalid entry
    with pytest.raises(ValueError):
        ix.search(q, k, label=f[:8])
    with pytest.raises(ValueError):
        ix.search(qt, k, label=torch.from_numpy(f[:8]).to(cuda))
    bad = f.copy()
    bad[4] = -3
    with pytest.raises(ValueError):
        ix.search(q, k, label=bad)
    with pytest.raises(ValueError):
        ix.search(qt, k, label=torch.from_numpy(bad).to(cuda))
    # the raw C call: a host array holding -3 is refused before any launch
    s = np.empty((9, k), np.float32)
    r = np.empty((9, k), np.int64)
    rc = _native.load().mrag_knn_search_labels(ix._h, q.ctypes.data, 9, k, bad.ctypes.data, 0, s.ctypes.data, None,
                                               r.ctypes.data, _native.MRAG_PTR_HOST, None)
    assert rc == 1  # MRAG_ERR_ARG
    # ... and a device array's entry below ANY matches nothing (mrag.h)
    st = torch.empty((9, k), dtype=torch.float32, device=cuda)
    rt = torch.empty((9, k), dtype=torch.int64, device=cuda)
    badt = torch.from_numpy(bad).to(cuda)
    torch.cuda.synchronize()
    rc = _native.load().mrag_knn_search_labels(ix._h, qt.data_ptr(), 9, k, badt.data_ptr(), 0, st.data_ptr(), None,
                                               rt.data_ptr(), _native.MRAG_PTR_DEVICE,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    want = or_.copy()
    want[4] = -1
    np.testing.assert_array_equal(rt.cpu().numpy(), want)
    # an empty index
    e = FlatIndex(dim)
    s, r = e.search(q, 3, label=f)
    assert np.all(r == -1) and np.all(np.isneginf(s))


def test_concurrent_labelled_searches_own_streams(cuda):
    """Two host threads, each running labelled searches on ONE index and its own stream: the
    per-search filter buffer lives in the search context, so the results equal the serial ones."""
    import threading

    import torch

    n, dim, users = 30_000, 256, 12
    x = clustered_corpus(n, dim, 21, n_clusters=40)
    lab = _skewed_labels(n, users, 361)
    ix = _index(x, lab)
    qs = [unit_rows(300, dim, 362), x[:200] + np.float32(1e-3)]
    fs = [_filters(300, users, 363), _filters(200, users, 364)]
    serial = []
    for q, f in zip(qs, fs):
        s, r = ix.search(torch.from_numpy(q).to(cuda), 10, label=torch.from_numpy(f).to(cuda))
        serial.append((s.cpu().numpy(), r.cpu().numpy()))
        _check(serial[-1], *_oracle(x, lab, q, 10, f))
    out = [None, None]
    errs = []

    def work(i):
        try:
            st = torch.cuda.Stream(device=cuda)
            with torch.cuda.stream(st):
                for _ in range(3):
                    s, r = ix.search(torch.from_numpy(qs[i]).to(cuda), 10, label=torch.from_numpy(fs[i]).to(cuda))
                    out[i] = (s.cpu().numpy(), r.cpu().numpy())
        except Exception as e:  # surfaced below
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    for i in range(2):
        np.testing.assert_array_equal(out[i][1], serial[i][1])
        np.testing.assert_array_equal(out[i][0], serial[i][0])


def test_sharded_index_passes_label_arrays(cuda):
    """ShardedFlatIndex.search / search_local forward an array for ``label`` (world of one)."""
    from app.vector_store.sharded import ShardedFlatIndex

    x = unit_rows(2000, 128, 370)
    lab = (np.arange(2000) % 3).astype(np.int32)
    ix = _index(x, lab)
    q = unit_rows(5, 128, 371)
    f = np.array([0, 1, 2, ANY, 7], np.int32)
    sh = ShardedFlatIndex(ix, row_offset=500)
    s, r = sh.search(q, 4, label=f)
    os_, or_ = _oracle(x, lab, q, 4, f, row_offset=500)
    _check((s, r), os_, or_)

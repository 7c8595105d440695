"""K15 (csrc/knn_compact.hip, mrag_knn_compact): the row remap against numpy's prefix sum, and a
compacted index against a fresh index that was given the live rows in order: every search must
agree bit for bit (f32 scores, f64 scores, rows), on every search path.

The paths that the shapes in SHAPES take at the compacted size are asserted on the CPU, through
the plan helper, in tests/test_knn_compact_plan_cpu.py."""
from __future__ import annotations

import ctypes
import threading

import numpy as np
import pytest

from _data import clustered_corpus, labels_for, unit_rows

pytestmark = pytest.mark.gpu

DELETED = -2
ANY = -1
SCAN_BLOCK = 4096  # labels per workgroup of K15a (knn_compact.h REMAP_BLOCK)

# ---------------------------------------------------------------------------------- remap (K15a)
REMAP_SIZES = [1, 63, 64, 65, 767, 768, 769, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1,
               SCAN_BLOCK ** 2 - 1, SCAN_BLOCK ** 2 + 1, (1 << 26) + 1]
assert SCAN_BLOCK ** 2 < 1 << 27
PATTERNS = ["none_dead", "all_dead", "first_only", "last_only", "alternating", "runs", "random", "all_but_one_dead"]


def _dead_mask(pattern: str, n: int) -> np.ndarray:
    i = np.arange(n, dtype=np.int64)
    if pattern == "none_dead":
        return np.zeros(n, bool)
    if pattern == "all_dead":
        return np.ones(n, bool)
    if pattern == "first_only":
        return i == 0
    if pattern == "last_only":
        return i == n - 1
    if pattern == "alternating":
        return (i & 1) == 1
    if pattern == "runs":  # dead runs of 3001 and live runs of 2003 rows: they straddle the 4096-label blocks
        return (i % 5004) < 3001
    if pattern == "random":
        return np.random.default_rng(n).integers(0, 2, n, dtype=np.int8) == 1
    if pattern == "all_but_one_dead":
        return i != (2 * n) // 3
    raise AssertionError(pattern)


@pytest.mark.parametrize("n", REMAP_SIZES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_row_remap_equals_numpy(cuda, n, pattern):
    import torch

    from app import _native

    dead = _dead_mask(pattern, n)
    labels = (np.arange(n, dtype=np.int64) % 7).astype(np.int32)
    labels[dead] = DELETED
    live = (~dead).astype(np.int64)
    want = np.where(dead, -1, np.cumsum(live) - live).astype(np.int32)
    lab = torch.from_numpy(labels).to(cuda)
    out = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    torch.cuda.synchronize()
    got_live = ctypes.c_int64(-1)
    _native.call("mrag_knn_row_remap", lab.data_ptr(), n, out.data_ptr(), ctypes.byref(got_live), None)
    assert got_live.value == int(live.sum())
    got = out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (n, pattern, bad[:5], got[bad[:5]], want[bad[:5]])


# ------------------------------------------------------- a compacted index equals a fresh one
N = 5000
# (dim, nq, k): the path each takes at the compacted size is pinned in test_knn_compact_plan_cpu.py
SHAPES = [
    (512, 300, 10),   # K7 v3, four query blocks per workgroup
    (512, 3, 10),     # K7s (small batches)
    (512, 300, 100),  # K7 v1 (deep lists)
    (384, 300, 50),
    (1, 300, 10),     # every cosine is +1, -1 or 0: the order is the tie rule alone
    (640, 40, 300),   # K7g (wide rows, deep k)
]
USERS = 3


def dead_rows(n: int = N) -> np.ndarray:
    """The deleted half of the n rows (the same for every dim)."""
    dead = np.random.default_rng(77).random(n) < 0.5
    dead[[11, 12, 13]] = True   # between the exact duplicates below
    dead[[10, 14, 15, n - 1]] = False
    return dead


def _corpus(dim: int):
    x = clustered_corpus(N, dim, 500 + dim, n_clusters=16)
    x[10] = unit_rows(1, dim, 499)[0]  # a direction no other row has (for dim > 1)
    x[14] = x[10]  # exact duplicates on both sides of deleted rows ...
    x[12] = x[10]  # ... and a deleted copy between them
    x[N - 1] = x[10]
    lab = labels_for(N, USERS, 600 + dim)
    lab[[10, 12, 14, N - 1]] = 1
    return x, lab


def _queries(x, live_rows, nq, dim, seed):
    q = unit_rows(nq, dim, seed)
    m = nq // 3
    q[:m] = x[live_rows[:: max(1, len(live_rows) // m)][:m]] + np.float32(1e-3)  # near the clusters: long tie runs
    q[0] = x[10]
    return q


@pytest.fixture(scope="module")
def pairs(cuda):
    """Per dim: A built by three adds and deletes, then compacted (its answers to every shape's
    searches taken first); B built from A's live rows in order."""
    from app.vector_store import FlatIndex

    built = {}

    def get(dim):
        if dim in built:
            return built[dim]
        x, lab = _corpus(dim)
        dead = dead_rows()
        a = FlatIndex(dim)
        for lo, hi in ((0, 2000), (2000, 3500), (3500, N)):
            assert a.add(x[lo:hi], lab[lo:hi]) == lo
            a.delete(lo + np.flatnonzero(dead[lo:hi]))
        live = np.flatnonzero(~dead)
        b = FlatIndex(dim)
        b.add(x[live], lab[live])
        assert len(a) == N and a.live_rows() == live.size == len(b)
        before = {}
        for d, nq, k in SHAPES:
            if d == dim:
                q = _queries(x, live, nq, dim, 800 + dim + k)
                for name, f in _label_kinds(nq, dim):
                    before[nq, k, name] = a.search(q, k, label=f, with_f64=True)
        remap = a.compact()
        built[dim] = {"x": x, "lab": lab, "dead": dead, "live": live, "a": a, "b": b, "before": before,
                      "remap": remap}
        return built[dim]

    yield get
    for p in built.values():
        p["a"].close()
        p["b"].close()


def _filters(nq, seed):
    f = np.random.default_rng(seed).integers(-1, USERS, nq).astype(np.int32)  # users and LABEL_ANY mixed
    f[0] = 1
    return f


def _label_kinds(nq, dim):
    return [("one", 1), ("any", ANY), ("per_query", _filters(nq, 700 + dim))]


@pytest.mark.parametrize("dim,nq,k", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_compacted_index_equals_fresh_index(pairs, dim, nq, k):
    p = pairs(dim)
    a, b = p["a"], p["b"]
    q = _queries(p["x"], p["live"], nq, dim, 800 + dim + k)
    want = np.where(p["dead"], -1, np.cumsum(~p["dead"]) - (~p["dead"])).astype(np.int64)
    np.testing.assert_array_equal(p["remap"], want)
    assert p["remap"].dtype == np.int64
    assert len(a) == len(b) == p["live"].size
    assert a.live_rows() == len(a)
    for name, f in _label_kinds(nq, dim):
        sa, ra, da = a.search(q, k, label=f, with_f64=True)
        sb, rb, db = b.search(q, k, label=f, with_f64=True)
        np.testing.assert_array_equal(ra, rb, err_msg=name)
        assert sa.tobytes() == sb.tobytes(), name
        assert da.tobytes() == db.tobytes(), name
        assert (ra >= 0).any()
        # and compaction changed no answer: the same rows under their new ids, the same scores
        s0, r0, d0 = p["before"][nq, k, name]
        np.testing.assert_array_equal(np.where(r0 >= 0, p["remap"][np.maximum(r0, 0)], -1), ra, err_msg=name)
        assert s0.tobytes() == sa.tobytes() and d0.tobytes() == da.tobytes(), name
    if dim > 1:  # the duplicates of row 10 come back in row order, the deleted copy (old row 12) never
        s, r = a.search(p["x"][10:11], 4, label=1)
        assert p["remap"][12] == -1
        assert r[0, :3].tolist() == [int(p["remap"][i]) for i in (10, 14, N - 1)]
        assert s[0, 0] == s[0, 1] == s[0, 2] > s[0, 3]


def test_torch_tensors_after_compaction(pairs, cuda):
    """Device-pointer searches (torch tensors, a caller's stream) on the compacted index."""
    import torch

    p = pairs(512)
    q = torch.from_numpy(_queries(p["x"], p["live"], 64, 512, 901)).to(cuda)
    f = torch.from_numpy(_filters(64, 902)).to(cuda)
    sa, ra = p["a"].search(q, 10, label=f)
    sb, rb = p["b"].search(q, 10, label=f)
    assert torch.equal(ra, rb) and torch.equal(sa, sb)


# ---------------------------------------------------------------------------------- lifecycle
def test_lifecycle_after_compaction(cuda):
    from app.vector_store import FlatIndex

    dim, n = 128, 3000
    x = unit_rows(n + 200, dim, 910)
    lab = labels_for(n + 200, USERS, 911)
    dead = np.random.default_rng(912).random(n) < 0.4
    ix = FlatIndex(dim)
    ix.add(x[:n], lab[:n])
    ix.delete(np.flatnonzero(dead))
    remap = ix.compact()
    live = int((~dead).sum())
    assert len(ix) == live == ix.live_rows()
    # add starts at the live count, and the new rows are found under their ids
    assert ix.add(x[n:], lab[n:]) == live
    assert len(ix) == live + 200
    s, r = ix.search(x[n:], 1)
    np.testing.assert_array_equal(r[:, 0], live + np.arange(200))
    # the old rows are found under their new ids
    keep = np.flatnonzero(~dead)[:100]
    s, r = ix.search(x[keep], 1)
    np.testing.assert_array_equal(r[:, 0], remap[keep])
    # delete by new ids
    ix.delete([int(remap[keep[0]]), live + 5])
    s, r = ix.search(np.stack([x[keep[0]], x[n + 5]]), 1)
    assert r[0, 0] != remap[keep[0]] and r[1, 0] != live + 5
    assert ix.live_rows() == live + 198
    remap2 = ix.compact()
    assert len(ix) == live + 198 and (remap2 < 0).sum() == 2
    # a second compaction with nothing deleted: the identity, the same size, the same answers
    q = unit_rows(50, dim, 913)
    want = ix.search(q, 10, with_f64=True)
    size = ctypes.c_int64(-1)
    from app import _native

    ident = np.full(len(ix), -5, np.int64)
    _native.call("mrag_knn_compact", ix._h, ident.ctypes.data, ctypes.byref(size))
    np.testing.assert_array_equal(ident, np.arange(live + 198))
    assert size.value == len(ix) == live + 198
    np.testing.assert_array_equal(ix.compact(), np.arange(live + 198))
    got = ix.search(q, 10, with_f64=True)
    for w, g in zip(want, got):
        assert w.tobytes() == g.tobytes()
    _native.call("mrag_knn_compact", ix._h, None, None)  # both outputs are optional
    ix.close()


def test_all_rows_dead_and_empty_index(cuda):
    from app.vector_store import FlatIndex

    dim = 256
    x = unit_rows(900, dim, 920)
    ix = FlatIndex(dim)
    assert ix.compact().shape == (0,) and len(ix) == 0 and ix.live_rows() == 0  # an empty index compacts
    ix.add(x, 0)
    ix.delete(np.arange(900))
    assert ix.live_rows() == 0
    remap = ix.compact()
    assert remap.shape == (900,) and np.all(remap == -1)
    assert len(ix) == 0
    s, r, d = ix.search(x[:5], 3, with_f64=True)  # the Empty plan path
    assert np.all(r == -1) and np.all(np.isneginf(s)) and np.all(np.isneginf(d))
    assert ix.add(x[:100], 2) == 0  # a later add starts at row 0
    s, r = ix.search(x[:100], 1, label=2)
    np.testing.assert_array_equal(r[:, 0], np.arange(100))
    assert ix.compact().tolist() == list(range(100))
    ix.close()


def test_wide_rows_every_gather_width(cuda):
    """K15b copies whole rows for every padded width: 128 (a half-wave per row), 256, 768 and 4096."""
    from app.vector_store import FlatIndex

    for dim in (100, 256, 768, 4096):
        n = 700 if dim < 4096 else 200
        x = unit_rows(n, dim, 930 + dim)
        dead = np.random.default_rng(dim).random(n) < 0.5
        dead[0], dead[n - 1] = True, False
        live = np.flatnonzero(~dead)
        a, b = FlatIndex(dim), FlatIndex(dim)
        a.add(x, (np.arange(n) % 2).astype(np.int32))
        a.delete(np.flatnonzero(dead))
        b.add(x[live], (live % 2).astype(np.int32))
        a.compact()
        q = np.concatenate([unit_rows(7, dim, 931), x[live[:5]]])
        for f in (ANY, 1):
            ga, gb = a.search(q, 20, label=f, with_f64=True), b.search(q, 20, label=f, with_f64=True)
            for u, v in zip(ga, gb):
                assert u.tobytes() == v.tobytes(), (dim, f)
        a.close()
        b.close()


# ------------------------------------------------------------------------- searches in flight
def test_searches_in_flight_during_compaction(cuda):
    """Four threads search (own streams) while a fifth compacts once: every answer is the answer
    of the index before (old row ids) or after (the same rows, remapped), with identical scores."""
    import torch

    from app.vector_store import FlatIndex

    dim, n, k = 512, 20_000, 10
    x = clustered_corpus(n, dim, 940, n_clusters=32)
    lab = labels_for(n, USERS, 941)
    dead = np.random.default_rng(942).random(n) < 0.5
    ix = FlatIndex(dim)
    ix.add(x, lab)
    ix.delete(np.flatnonzero(dead))
    qs = [torch.from_numpy(unit_rows(200, dim, 950 + i)).to(cuda) for i in range(4)]
    before = []
    for q in qs:
        s, r = ix.search(q, k, label=1)
        before.append((s.cpu().numpy(), r.cpu().numpy()))
    start = threading.Barrier(5)
    results = [[] for _ in range(4)]
    errs, remap = [], []

    def search(i):
        try:
            st = torch.cuda.Stream(device=cuda)
            start.wait(timeout=60)
            with torch.cuda.stream(st):
                for _ in range(12):
                    s, r = ix.search(qs[i], k, label=1)
                    results[i].append((s.cpu().numpy(), r.cpu().numpy()))
        except Exception as e:  # surfaced below
            errs.append(e)

    def compact():
        try:
            start.wait(timeout=60)
            remap.append(ix.compact())
        except Exception as e:  # surfaced below
            errs.append(e)

    th = [threading.Thread(target=search, args=(i,)) for i in range(4)] + [threading.Thread(target=compact)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    assert len(remap) == 1 and len(ix) == int((~dead).sum())
    for i in range(4):
        s0, r0 = before[i]
        r1 = np.where(r0 >= 0, remap[0][np.maximum(r0, 0)], -1)
        assert np.all(r1[r0 >= 0] >= 0)
        assert len(results[i]) == 12
        for s, r in results[i]:
            assert s.tobytes() == s0.tobytes()
            assert np.array_equal(r, r0) or np.array_equal(r, r1)
        s, r = ix.search(qs[i], k, label=1)  # and afterwards: the remapped rows
        assert np.array_equal(r.cpu().numpy(), r1) and s.cpu().numpy().tobytes() == s0.tobytes()
    ix.close()

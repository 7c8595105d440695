"""The kNN search at the edges between its paths (csrc/knn_plan.h) and at the edges of the number
formats, against the f64 oracle:

* v1's deep-list scan (64 < k <= 256) on tables of several tiles per split, at every list depth
  (KL 32, 16, 16, 8 for dim 100, 256, 384, 512), k = 65, 128 and MAX_K = 256, batches that fill a
  32-query wave partly, exactly and into a second workgroup, with and without a label filter;
* the two kernels on either side of a path switch (k = 64 | 65: v3 | v1, k = 256 | 257: v1 | K7g)
  return the same rows and bit-equal f32 and f64 scores, with exact duplicates across the cut;
* rows that are one axis plus 1e-5 noise (fp16 subnormals and zeros after normalisation), the
  same rows scaled to where an f32 sum of squares vanishes or overflows, and all-zero rows.
"""
from __future__ import annotations

import numpy as np
import pytest

from _data import clustered_corpus, labels_for
from oracle.knn import flat_cosine_topk
from test_knn_gpu import _check

pytestmark = pytest.mark.gpu


def _queries(x: np.ndarray, nq: int, seed) -> np.ndarray:
    """Even queries are near-duplicates of rows, odd ones random (so every prefix has both)."""
    rng = np.random.default_rng(seed)
    d = x.shape[1]
    near = x[rng.integers(0, len(x), nq)] + 0.01 * rng.standard_normal((nq, d)).astype(np.float32)
    rnd = rng.standard_normal((nq, d)).astype(np.float32)
    return np.where((np.arange(nq) % 2 == 0)[:, None], near, rnd).astype(np.float32)


@pytest.mark.parametrize("dim,n", [(100, 20_000), (256, 20_000), (384, 20_000), (512, 20_000), (256, 100_000)])
def test_v1_at_depth(cuda, dim, n):
    """The oracle's top-256 of 257 queries is computed once per filter; a search for k of the
    first nq queries must equal its first nq rows and k columns (the order is total)."""
    from app.vector_store import FlatIndex

    x = clustered_corpus(n, dim, 50 + dim, n_clusters=32, spread=0.05, dup_frac=0.05)
    lab = labels_for(n, 4, 51)
    q = _queries(x, 257, 52)
    ix = FlatIndex(dim)
    ix.add(x, lab)
    for f in (-1, 2):
        os_, or_ = flat_cosine_topk(x, lab, q, 256, label_filter=f)
        assert or_.min() >= 0
        for k in (65, 128, 256):
            for nq in (1, 33, 257):
                s, r = ix.search(q[:nq], k, label=f)
                _check(s, r, os_[:nq, :k], or_[:nq, :k])
    ix.close()


@pytest.mark.parametrize("dim", [128, 512])
def test_both_sides_of_a_switch_agree(cuda, dim):
    """k = 64 (v3) against the first 64 columns of k = 65 (v1), k = 256 (v1) against the first 256
    of k = 257 (K7g), on one index and one batch. Every path rescores through exact_cosine16, so
    rows, f32 scores and f64 scores are equal bit for bit. For the first four queries the rows
    ranked 64 to 66 and 256 to 258 are made copies of one another, so a tie crosses each cut."""
    from app.vector_store import FlatIndex

    n = 20_000
    x = clustered_corpus(n, dim, 60 + dim, n_clusters=32, spread=0.05, dup_frac=0.1)
    q = _queries(x, 40, 61)
    _, r0 = flat_cosine_topk(x, np.zeros(n), q[:4], 258)
    for j in range(4):
        for cut in (64, 256):
            x[r0[j, cut]] = x[r0[j, cut + 1]] = x[r0[j, cut - 1]]
    os_, or_ = flat_cosine_topk(x, np.zeros(n), q, 257)
    for j in range(4):
        assert os_[j, 63] == os_[j, 64] and os_[j, 255] == os_[j, 256], j  # ties across both cuts
    ix = FlatIndex(dim)
    ix.add(x)
    res = {k: ix.search(q, k, with_f64=True) for k in (64, 65, 256, 257)}
    for k, (s, r, s64) in res.items():
        _check(s, r, os_[:, :k], or_[:, :k])
    for k in (64, 256):
        (s, r, s64), (s1, r1, s641) = res[k], res[k + 1]
        np.testing.assert_array_equal(r, r1[:, :k])
        np.testing.assert_array_equal(s.view(np.uint32), np.ascontiguousarray(s1[:, :k]).view(np.uint32))
        np.testing.assert_array_equal(s64.view(np.uint64), np.ascontiguousarray(s641[:, :k]).view(np.uint64))
    ix.close()


def test_peaked_and_scaled_rows(cuda):
    """8,000 rows e_j + 1e-5 noise over 40 axes of 384 (after normalisation the noise is an fp16
    subnormal or zero), as many of the same form scaled by 1e-18 and by 1e+18 (and by 1e-20 and
    1e+20, where the f32 square of the peak itself is subnormal or infinite) and 50 all-zero rows,
    shuffled. The library's norms are f64, so a scaled row scores like the row. The scaled rows
    draw their own noise: scaled copies of one row differ by their f32 rounding alone and lie
    1e-16 to 1e-14 apart in cosine, where the oracle's own rounding would decide the order (the
    gaps are asserted below). Queries are Gaussian, or an axis plus 1e-2 noise, some scaled too."""
    from app.vector_store import FlatIndex

    d, m = 384, 8000
    rng = np.random.default_rng(70)
    axes = rng.choice(d, 40, replace=False)

    def peaked():
        p = (1e-5 * rng.standard_normal((m, d))).astype(np.float32)
        p[np.arange(m), axes[rng.integers(0, 40, m)]] += np.float32(1.0)
        return p

    x = np.concatenate([peaked() * np.float32(sc) for sc in (1.0, 1e-18, 1e18, 1e-20, 1e20)]
                       + [np.zeros((50, d), np.float32)])
    assert np.all(np.isfinite(x))
    with np.errstate(over="ignore"):
        ss = np.sum(x * x, axis=1, dtype=np.float32)
    assert np.isinf(ss).sum() == m and (ss == 0).sum() >= 50  # f32 norms would not do
    x = x[rng.permutation(len(x))]
    q = rng.standard_normal((16, d)).astype(np.float32)
    q[8:] *= np.float32(1e-2)
    q[np.arange(8, 16), axes[:8]] += np.float32(1.0)
    q[4:6] *= np.float32(1e-18)
    q[12:14] *= np.float32(1e18)
    ix = FlatIndex(d)
    ix.add(x)
    os_, or_ = flat_cosine_topk(x, np.zeros(len(x)), q, 101)
    assert np.all(np.diff(os_, axis=1) < -1e-13)  # the order is the scores', not their rounding's
    for k in (10, 100):
        s, r = ix.search(q, k)
        _check(s, r, os_[:, :k], or_[:, :k])
    ix.close()

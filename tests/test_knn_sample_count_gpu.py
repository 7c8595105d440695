"""The counting sample pass of the kNN scan: rows of the sampled tiles reach K8
only through the per-lane record and the resolve kernel, so the cases put the answer there, fill
one lane's record past its two groups, and overflow the extra lists.

Also the band cases written for a K8 that rescores only candidates with approx >= a_k - 2 EPS
(measured, not kept): many rows within 1e-4 of the k-th score, some bit-equal,
inside and outside sampled tiles, so the rows returned and their order depend on every one of
them being rescored; and a query with fewer than k matching rows.

Shapes: 1000 queries (4 query groups, 64 splits) over 270k rows, so that every split holds the
64 tiles the sample pass needs, at 128 dims and at 512 (the second instantiation);
tests/test_knn_plan_cpu.py asserts that these shapes take the counting pass. The oracle is
run on the planted queries and a few plain ones only (a query's result does not depend on the
rest of the batch), which keeps a case to a few seconds.
"""
from __future__ import annotations

import numpy as np
import pytest

from _data import unit_rows
from oracle.knn import flat_cosine_topk

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-6
NQ = 1000
NBAND = 30       # rows per planted query inside the band
BAND = 1e-4      # width of the band of exact scores
PLANTED = 6      # queries 0 .. PLANTED-1 carry a band
PLAIN = 20       # further queries checked against the oracle
FEW_LABEL = 5    # a label that only FEW_ROWS rows carry
FEW_ROWS = 7


def _check(gs, gr, os_, or_):
    gs = np.asarray(gs)
    gr = np.asarray(gr)
    assert gr.shape == or_.shape
    np.testing.assert_array_equal(gr, or_)
    valid = or_ >= 0
    assert np.all(np.isneginf(gs[~valid]))
    np.testing.assert_allclose(gs[valid], os_[valid].astype(np.float32), rtol=0, atol=SCORE_TOL)


def _corpus(n, dim, k, seed):
    """Random unit rows; for each planted query NBAND rows q/|q| + e with e orthogonal to q and
    |e| = t_j, so that the exact cosines 1 / sqrt(1 + t_j^2) step evenly down across BAND from
    0.958 (random rows stay below 0.5 at these dims): steps of 3.4e-6, far above the f32 rounding
    of the rows (1e-8) and far below EPS_F16 (1.05e-3), so the fp16 scan sees them in scrambled
    order while the oracle's order is unambiguous. Ranks k-2, k-1, k and k+1 are made two
    bit-equal pairs, so the k-th place is decided by (score, row asc) between duplicates. Half of
    a query's band lies in rows 0..4095 (the first tile of every split), half elsewhere, in
    random row order."""
    rng = np.random.default_rng(seed)
    x = unit_rows(n, dim, seed + 1)
    q = rng.standard_normal((NQ, dim)).astype(np.float32)
    lab = np.zeros(n, np.int32)
    inside = rng.permutation(4096)
    outside = 4096 + rng.permutation(n - 4096)
    c = 0.958 - BAND * np.arange(NBAND) / (NBAND - 1)
    t = np.sqrt(1.0 / c**2 - 1.0)
    for i in range(PLANTED):
        qh = q[i].astype(np.float64)
        qh /= np.linalg.norm(qh)
        e = rng.standard_normal((NBAND, dim))
        e -= np.outer(e @ qh, qh)
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        v = (qh[None, :] + t[:, None] * e).astype(np.float32)
        v[k - 1] = v[k - 2]
        v[k + 1] = v[k]
        half = NBAND // 2
        rows = np.concatenate([inside[i * half:(i + 1) * half], outside[i * half:(i + 1) * half]])
        x[rng.permutation(rows)] = v
    few = outside[PLANTED * NBAND:PLANTED * NBAND + FEW_ROWS]
    lab[few] = FEW_LABEL
    return x, lab, q


@pytest.fixture(scope="module", params=[(270_000, 128, 10), (270_000, 512, 12)], ids=["dp128_k10", "dp512_k12"])
def banded(request, cuda):
    from app.vector_store import FlatIndex

    n, dim, k = request.param
    x, lab, q = _corpus(n, dim, k, 700 + dim)
    ix = FlatIndex(dim)
    ix.add(x, lab)
    sel = np.arange(PLANTED + PLAIN)
    yield ix, x, lab, q, k, sel
    ix.close()


# ---- the counting sample pass: rows of the sampled tiles reach K8 through the
# resolve kernel only. Split s owns tiles s, s + 64, ... and its first tile is sampled, so rows
# 0..4095 are all sampled; a lane group owns the rows with the same (row % 16) / 4, a 4-row
# group is rows 16 rb + 4 g .. + 3 of a tile.
NBASE = 50       # query clusters; every query is a near-copy of one base
NNEAR = 20       # rows per base, cosines 0.98, 0.97, ... to the base (steps >> EPS_F16)
TILE_B = 60      # record overflow: four groups of one lane group of this tile
ROWS_B = [TILE_B * 64 + r for r in (0, 16, 32, 48)]
ROWS_C = [t * 64 + 60 + r for t in range(50) for r in range(4)]  # 50 whole groups, one per tile


def _near(v, cosines, rng):
    """Rows at the given cosines to v: v/|v| + t e with e a random unit vector orthogonal to v."""
    vh = v.astype(np.float64) / np.linalg.norm(v)
    e = rng.standard_normal((len(cosines), v.size))
    e -= np.outer(e @ vh, vh)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    t = np.sqrt(1.0 / np.asarray(cosines) ** 2 - 1.0)
    return (vh[None, :] + t[:, None] * e).astype(np.float32)


def _sampled_corpus(n, dim, seed):
    """Random unit rows with labels 0 / 1, and inside rows 0..4095:
    A. for each of NBASE bases NNEAR rows at cosines 0.98 - 0.01 j, each in another tile of
       0..59 (so no lane sees two of one base), label 1 except the best one (label 0);
    B. four rows within 3e-5 of cosine 0.99 to a vector vb at rows 0, 16, 32, 48 of tile 60;
    C. 200 rows within 2e-3 of cosine 0.99 to a vector vc, as 50 whole 4-row groups.
    Queries: 1000 near-copies of the bases (cosine ~0.999)."""
    rng = np.random.default_rng(seed)
    x = unit_rows(n, dim, seed + 1)
    lab = rng.integers(0, 2, n).astype(np.int32)
    bases = unit_rows(NBASE + 2, dim, seed + 2)
    used = np.zeros(64, np.int64)
    for b in range(NBASE):
        v = _near(bases[b], 0.98 - 0.01 * np.arange(NNEAR), rng)
        for j in range(NNEAR):
            t = (b + 3 * j) % 60
            row = t * 64 + used[t]
            used[t] += 1
            x[row] = v[j]
            lab[row] = 0 if j == 0 else 1
    assert used.max() <= 60
    vb, vc = bases[NBASE], bases[NBASE + 1]
    x[ROWS_B] = _near(vb, 0.99 - 1e-5 * np.arange(4), rng)
    x[ROWS_C] = _near(vc, 0.99 - 1e-5 * np.arange(len(ROWS_C)), rng)
    lab[ROWS_B] = 1
    lab[ROWS_C] = 1
    q = bases[np.arange(NQ) % NBASE] + (0.04 / np.sqrt(dim)) * rng.standard_normal((NQ, dim)).astype(np.float32)
    return x, lab, q.astype(np.float32), vb, vc


@pytest.fixture(scope="module")
def sampled128(cuda):
    from app.vector_store import FlatIndex

    x, lab, q, vb, vc = _sampled_corpus(270_000, 128, 900)
    ix = FlatIndex(128)
    ix.add(x, lab)
    yield ix, x, lab, q, vb, vc
    ix.close()


SEL_A = np.r_[0:NBASE + 10, NQ - 5:NQ]  # every base once, and a few repeats


@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("label", [-1, 1])
def test_resolved_rows_carry_the_answer(sampled128, k, label):
    """Every query's top-k lies in sampled tiles; with label 1 the best row of each query is
    masked. Exact, and every query certified by K8 (no collect pass)."""
    ix, x, lab, q, _, _ = sampled128
    s, r = ix.search(q, k, label=label)
    unc, _ = ix.last_stats()
    os_, or_ = flat_cosine_topk(x, lab, q[SEL_A], k, label_filter=label)
    assert np.all(or_ < 4096)
    _check(np.asarray(s)[SEL_A], np.asarray(r)[SEL_A], os_, or_)
    assert unc == 0


def test_resolved_rows_512(cuda):
    """The same at 512 dims, k = 12 (the second instantiation of the counting pass: 270k rows,
    the smallest corpus whose splits hold 64 tiles)."""
    from app.vector_store import FlatIndex

    x, lab, q, _, _ = _sampled_corpus(270_000, 512, 950)
    ix = FlatIndex(512)
    ix.add(x, lab)
    s, r = ix.search(q, 12, label=1)
    unc, _ = ix.last_stats()
    os_, or_ = flat_cosine_topk(x, lab, q[SEL_A], 12, label_filter=1)
    ix.close()
    assert np.all(or_ < 4096)
    _check(np.asarray(s)[SEL_A], np.asarray(r)[SEL_A], os_, or_)
    assert unc == 0


def test_record_overflow_goes_to_collect(sampled128):
    """Four near-tied groups in one lane's sample: the lane records two, the third is only bounded
    (m3), so the query cannot be certified and the collect pass finds the rows."""
    ix, x, lab, q, vb, _ = sampled128
    q2 = q.copy()
    q2[0] = vb
    s, r = ix.search(q2, 10)
    unc, _ = ix.last_stats()
    sel = np.arange(8)
    os_, or_ = flat_cosine_topk(x, lab, q2[sel], 10)
    assert sorted(or_[0, :4].tolist()) == ROWS_B
    _check(np.asarray(s)[sel], np.asarray(r)[sel], os_, or_)
    assert unc >= 1


def test_extra_list_overflow(sampled128):
    """200 sampled rows of one query above its seed, in 50 recorded groups: more than the extra
    lists hold; the best are kept, the best dropped score bounds the rest."""
    ix, x, lab, q, _, vc = sampled128
    q2 = q.copy()
    q2[1] = vc
    for k in (10, 16):
        s, r = ix.search(q2, k)
        sel = np.arange(8)
        os_, or_ = flat_cosine_topk(x, lab, q2[sel], k)
        assert set(or_[1].tolist()) <= set(ROWS_C)
        _check(np.asarray(s)[sel], np.asarray(r)[sel], os_, or_)


def test_band_of_near_ties_and_duplicates(banded):
    """k = 10 (12 at 512): 30 rows within 1e-4 of the k-th, two bit-equal pairs around it, inside
    and outside the sampled tiles: rows and order equal the oracle under (score desc, row asc);
    so do the plain queries of the same batch, whose band holds little more than the k best."""
    ix, x, lab, q, k, sel = banded
    s, r = ix.search(q, k)
    unc, _ = ix.last_stats()
    os_, or_ = flat_cosine_topk(x, lab, q[sel], k)
    band = os_[:PLANTED, 0] - os_[:PLANTED, -1]
    print(f"uncertified {unc}; planted queries' top-k span {band.max():.3g}")
    assert band.max() < BAND
    _check(np.asarray(s)[sel], np.asarray(r)[sel], os_, or_)


def test_band_below_and_above_k(banded):
    """The same band with k below it (k = 1: one winner out of 30 near-ties) and above it
    (k = 16 at 128: the band's 30 rows fill the top-16), where a_k sits elsewhere in the band."""
    ix, x, lab, q, k, sel = banded
    for kk in ((1, 16) if k == 10 else (1,)):
        s, r = ix.search(q, kk)
        os_, or_ = flat_cosine_topk(x, lab, q[sel], kk)
        _check(np.asarray(s)[sel], np.asarray(r)[sel], os_, or_)


def test_fewer_matches_than_k(banded):
    """A label only 7 rows carry: fewer than k candidates, every one is rescored and returned,
    the remaining slots are empty."""
    ix, x, lab, q, k, sel = banded
    s, r = ix.search(q, k, label=FEW_LABEL)
    os_, or_ = flat_cosine_topk(x, lab, q[sel], k, label_filter=FEW_LABEL)
    assert np.all((or_ >= 0).sum(axis=1) == FEW_ROWS)
    _check(np.asarray(s)[sel], np.asarray(r)[sel], os_, or_)

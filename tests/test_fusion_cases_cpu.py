"""What the K12 test inputs of tests/_fusion_cases.py reach on the host restatement
(``app.retrieval.fuse_scores``) alone, so that the GPU comparison in test_fusion_gpu.py provably
covers those outcomes; and the precondition the kernel relies on (valid hits form a prefix) for the
two kinds of list the pipeline produces."""
from __future__ import annotations

import numpy as np

import _fusion_cases as fc
from app.retrieval import fuse_scores


def _pairs():
    deg = fc.pad(fc.degenerate_lists())
    rnd = fc.pad(fc.random_lists(np.random.default_rng(3), len(deg), 300))
    return {"deg|random": (deg, rnd), "random|deg": (rnd, deg), "deg|rolled": (deg, np.roll(deg, 7, axis=0)),
            "deg|same": (deg, deg)}


def _all_combined():
    """name -> (pick, combined, kt) with every valid item kept (final_n = kt + ki)."""
    return {k: fuse_scores(a, b, a.shape[1] + b.shape[1]) + (a.shape[1],) for k, (a, b) in _pairs().items()}


def test_lists_stay_in_range_and_finite():
    for lists in (fc.degenerate_lists(), fc.score_range_lists(np.random.default_rng(0))):
        for v in lists:
            assert v.dtype == np.float32 and np.isfinite(v).all() and np.abs(v).max() <= 2
    for pick, comb, _ in _all_combined().values():
        assert np.isfinite(comb[pick >= 0]).all() and np.isnan(comb[pick < 0]).all()


def test_degenerate_family_has_zero_std_rows():
    """Rows whose text and image std are both exactly 0: every combined score is 0."""
    pick, comb, _ = _all_combined()["deg|rolled"]
    zero = np.all(np.where(pick >= 0, comb, 0.0) == 0.0, axis=1) & (pick >= 0).any(axis=1)
    assert zero.sum() >= 50


def test_degenerate_family_has_constant_lists_with_nonzero_std():
    """Constant lists whose f32 ``sum / n`` is not the constant: std is one ulp-sized step, not 0,
    and every item's z is exactly +1 or -1 (an f64 mean, or a different summation order, gives std 0
    and z 0 instead)."""
    one = np.float32(1)
    hit = 0
    for v in fc.degenerate_lists():
        if not np.all(v == v[0]):
            continue
        arr = (1.0 - (one - v).astype(np.float64)).astype(np.float32)
        if arr.std() != 0:
            pick, comb = fuse_scores(v[None, :], np.empty((1, 0), np.float32), len(v))
            assert np.all(np.abs(comb[0]) == 1.0) and np.all(comb[0] == comb[0, 0])
            hit += 1
    assert hit >= 8


def test_degenerate_family_has_text_image_ties():
    """An exact combined tie between a text and an image item (text must come first), both at 0
    (two zero-std lists) and at a non-zero z (the same list on both sides)."""
    zero_tie = nonzero_tie = 0
    for pick, comb, kt in _all_combined().values():
        for p, c in zip(pick, comb):
            v = p >= 0
            t, i = c[v & (p < kt)], c[v & (p >= kt)]
            both = np.intersect1d(t, i)
            zero_tie += bool(np.any(both == 0))
            nonzero_tie += bool(np.any(both != 0))
    assert zero_tie >= 50 and nonzero_tie >= 50


def test_degenerate_family_has_huge_combined():
    """Rows with ``|combined| > 1e3``. With lists of at most 300 items the family cannot reach them:
    the caller-visible score ``1 - f32(1 - s)`` is a multiple of 2^-24 and itself an f32, nothing
    underflows, and ``std^2 = sum((x_i - mean)^2) / n >= (x_j - mean)^2 / n`` gives ``|z_j| <= sqrt(n)``
    whatever the f32 mean is (largest value there: 17.3205 = sqrt(300); a constant list whose f32
    mean is one step off has z exactly +-1, see the test above). The outcome is reached by the
    family's two one-step-off lists of 2^20 + 1 items, which the GPU test runs as they are."""
    small = max(float(np.abs(comb[pick >= 0]).max()) for pick, comb, _ in _all_combined().values())
    assert small <= np.sqrt(300) * (1 + 1e-6)
    lists = fc.long_one_off_lists()
    ts, im = fc.pad(lists), fc.pad(lists[::-1])
    pick, comb = fuse_scores(ts, im, 8)
    assert np.isfinite(comb).all() and np.all(pick >= 0)
    print("largest |combined|: lists of <= 300 items", small, "; of 2^20 + 1 items", np.abs(comb).max(axis=1))
    assert np.all(np.abs(comb).max(axis=1) > 1e3)
    kt = ts.shape[1]
    assert np.all(comb[:, :2] > 1e3)  # the one-off item of either list: first of one, last of the other
    assert sorted(pick[0, :2].tolist()) == [0, 2 * kt - 1] and sorted(pick[1, :2].tolist()) == [kt - 1, kt]


def test_valid_hits_form_a_prefix():
    """K12 counts the finite scores of a list and reads that many leading items; ``fuse_scores``
    masks instead. Both kinds of list the pipeline passes keep the valid hits in front: a list
    sorted descending (``-inf`` sorts last), and the padding of ``FlatIndex.search`` (restated by
    ``oracle.knn.flat_cosine_topk``) when fewer rows match than k."""
    from oracle.knn import flat_cosine_topk

    def is_prefix(valid):
        return bool(np.all(valid[:, :-1] >= valid[:, 1:]))

    rng = np.random.default_rng(1)
    s = rng.uniform(-1, 1, (40, 17)).astype(np.float32)
    s[rng.uniform(size=s.shape) < 0.4] = -np.inf
    assert not is_prefix(np.isfinite(s))  # the check can fail
    assert is_prefix(np.isfinite(-np.sort(-s, axis=1)))
    x = rng.standard_normal((30, 16)).astype(np.float32)
    lab = (np.arange(30) % 5).astype(np.int32)  # 6 rows per label
    q = rng.standard_normal((9, 16)).astype(np.float32)
    for label, k in ((2, 10), (2, 6), (-1, 40), (7, 4)):
        sc, rows = flat_cosine_topk(x, lab, q, k, label_filter=label)
        valid = np.isfinite(sc)
        assert is_prefix(valid) and np.array_equal(valid, rows >= 0)
        assert np.all(sc[~valid] == -np.inf)
    assert is_prefix(np.isfinite(fc.prefix_counts(rng, 20)))
    assert is_prefix(np.isfinite(fc.pad(fc.degenerate_lists())))

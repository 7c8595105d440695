"""K12 (csrc/fusion.hip, mrag_fuse_scores): the reference's z-score fusion on the GPU,
bit-identical to the host restatement ``app.retrieval.fuse_scores`` (pinned against the
reference's ``_fuse_results`` by tests/test_compat_cpu.py) and to ``oracle.fusion`` on the
hit dicts: picks equal, combined f64 scores equal bit for bit. Cases: full lists, missing hits
(-inf padding), one-hit lists (std 0), empty lists, exact score ties, k up to 300."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _lists(rng, q, k, fill):
    s = -np.sort(-rng.uniform(-0.2, 0.9, (q, k)).astype(np.float32), axis=1)
    s[: q // 8] = np.round(s[: q // 8], 2)  # exact ties inside a list
    n = rng.integers(0, k + 1, q) if fill else np.full(q, k)
    n[:3] = [0, 1, min(2, k)]
    s[np.arange(k)[None, :] >= n[:, None]] = -np.inf
    return s


@pytest.mark.parametrize("kt,ki,final_n", [(50, 12, 4), (10, 10, 4), (300, 7, 9), (1, 1, 4), (130, 140, 20)])
def test_fusion_gpu_equals_host(cuda, kt, ki, final_n):
    import torch

    from app.retrieval import fuse_scores, fuse_scores_gpu
    from oracle.fusion import fuse_results

    rng = np.random.default_rng(kt * 1000 + ki)
    q = 700
    ts, im = _lists(rng, q, kt, True), _lists(rng, q, ki, True)
    ts[5], im[5] = ts[4], im[4]  # identical queries
    hp, hc = fuse_scores(ts, im, final_n)
    gp, gc = fuse_scores_gpu(torch.from_numpy(ts).to(cuda), torch.from_numpy(im).to(cuda), final_n)
    gp, gc = gp.cpu().numpy(), gc.cpu().numpy()
    np.testing.assert_array_equal(gp, hp)
    np.testing.assert_array_equal(gc, hc)  # NaN == NaN for empty slots
    one = np.float32(1.0)
    for i in range(0, q, 23):  # the reference's dict-based fusion on a sample
        th = [{"i": j, "score": float(1.0 - float(one - s))} for j, s in enumerate(ts[i]) if np.isfinite(s)]
        ih = [{"i": kt + j, "score": float(1.0 - float(one - s))} for j, s in enumerate(im[i]) if np.isfinite(s)]
        ref = fuse_results(th, ih, final_n)
        assert [r["i"] for r in ref] == [int(p) for p in gp[i] if p >= 0], i
        assert [r["combined_score"] for r in ref] == [float(c) for c, p in zip(gc[i], gp[i]) if p >= 0], i


# ---- direct calls of mrag_fuse_scores: guarded outputs, bit patterns, every edge of the inputs ----

PICK_GUARD = -(7 << 40) - 12345
COMB_GUARD = -2.5e300


def _fuse_guarded(cuda, ts, im, final_n):
    """mrag_fuse_scores on host arrays ts [q, kt], im [q, ki], writing into buffers with one guard
    row before and after; a modality without a list (k == 0) is passed as a NULL pointer."""
    import torch

    from app import _native

    q, kt, ki = ts.shape[0], ts.shape[1], im.shape[1]
    assert im.shape[0] == q and ts.dtype == im.dtype == np.float32
    tsd = torch.from_numpy(np.ascontiguousarray(ts)).to(cuda)
    imd = torch.from_numpy(np.ascontiguousarray(im)).to(cuda)
    pick = torch.full((q + 2, final_n), PICK_GUARD, dtype=torch.int64, device=cuda)
    comb = torch.full((q + 2, final_n), COMB_GUARD, dtype=torch.float64, device=cuda)
    _native.call("mrag_fuse_scores", tsd.data_ptr() if kt else 0, kt, imd.data_ptr() if ki else 0, ki, q, final_n,
                 pick.data_ptr() + final_n * 8, comb.data_ptr() + final_n * 8,
                 torch.cuda.current_stream().cuda_stream)
    pick, comb = pick.cpu().numpy(), comb.cpu().numpy()
    for g in (0, q + 1):
        assert np.all(pick[g] == PICK_GUARD) and np.all(comb[g] == COMB_GUARD), f"guard row {g} written"
    return pick[1:q + 1], comb[1:q + 1]


def _check(cuda, ts, im, final_n, oracle_step=1):
    """GPU == fuse_scores: picks exactly, combined by bit pattern, NaN exactly where pick == -1;
    and == the reference's dict-based fusion on every oracle_step-th query (0: none)."""
    from app.retrieval import fuse_scores
    from oracle.fusion import fuse_results

    ts, im = np.asarray(ts, np.float32), np.asarray(im, np.float32)
    finite = np.concatenate([ts[np.isfinite(ts)], im[np.isfinite(im)]])
    assert finite.size == 0 or np.abs(finite).max() <= 2
    hp, hc = fuse_scores(ts, im, final_n)
    assert hp.shape == hc.shape == (ts.shape[0], final_n)
    assert np.isfinite(hc[hp >= 0]).all() and np.isnan(hc[hp < 0]).all()  # the NaN check below means something
    gp, gc = _fuse_guarded(cuda, ts, im, final_n)
    np.testing.assert_array_equal(gp, hp)
    np.testing.assert_array_equal(np.isnan(gc), gp == -1)
    np.testing.assert_array_equal(np.where(gp >= 0, gc, 0.0).view(np.int64), np.where(hp >= 0, hc, 0.0).view(np.int64))
    one, kt = np.float32(1.0), ts.shape[1]
    for i in range(0, ts.shape[0], oracle_step) if oracle_step else ():
        th = [{"i": j, "score": float(1.0 - float(one - s))} for j, s in enumerate(ts[i]) if np.isfinite(s)]
        ih = [{"i": kt + j, "score": float(1.0 - float(one - s))} for j, s in enumerate(im[i]) if np.isfinite(s)]
        ref = fuse_results(th, ih, final_n)
        keep = gp[i] >= 0
        assert [r["i"] for r in ref] == gp[i][keep].tolist(), i
        rc = np.array([r["combined_score"] for r in ref], dtype=np.float64)
        np.testing.assert_array_equal(rc.view(np.int64), gc[i][keep].view(np.int64), err_msg=str(i))
    return gp, gc


@pytest.mark.parametrize("q", [1, 2, 3, 5, 257])
def test_fusion_query_tails(cuda, q):
    rng = np.random.default_rng(q)
    _check(cuda, _lists(rng, max(q, 8), 50, True)[:q], _lists(rng, max(q, 8), 12, True)[:q], 4)


@pytest.mark.parametrize("kt,ki,final_n", [(0, 12, 4), (50, 0, 4), (0, 0, 4), (0, 1, 1)])
def test_fusion_absent_modality(cuda, kt, ki, final_n):
    rng = np.random.default_rng(kt + ki)
    q = 37
    gp, _ = _check(cuda, _lists(rng, q, kt, True), _lists(rng, q, ki, True), final_n)
    if kt == 0 and ki == 0:
        assert np.all(gp == -1)


@pytest.mark.parametrize("kt,ki,final_n", [(5, 3, 8), (5, 3, 9), (70, 70, 64), (70, 70, 65), (70, 70, 130)])
def test_fusion_final_n_shapes(cuda, kt, ki, final_n):
    """final_n == nt + ni and one more (full lists), and final_n past one wave's 64 lanes with
    lists that are sometimes shorter than final_n."""
    import _fusion_cases as fc

    rng = np.random.default_rng(final_n)
    if kt == 5:
        ts, im = fc.pad(fc.random_lists(rng, 21, kt, full=True)), fc.pad(fc.random_lists(rng, 21, ki, full=True))
        gp, _ = _check(cuda, ts, im, final_n)
        assert np.all((gp >= 0).sum(axis=1) == kt + ki)
    else:
        ts, im = _lists(rng, 64, kt, True), _lists(rng, 64, ki, True)
        ts[7], im[7] = fc.random_lists(rng, 1, kt, full=True)[0], fc.random_lists(rng, 1, ki, full=True)[0]
        gp, _ = _check(cuda, ts, im, final_n, oracle_step=5)
        filled = (gp >= 0).sum(axis=1)
        assert filled.max() == final_n and filled.min() < final_n


@pytest.mark.parametrize("side", ["text", "image"])
def test_fusion_every_valid_count(cuda, side):
    """Query i has exactly i finite scores on one side, i = 0 .. 272: every leaf boundary of the
    pairwise sum (7/8/9, 127/128/129, 135/136, 255/256/257 ...) by construction."""
    import _fusion_cases as fc

    rng = np.random.default_rng(len(side))
    walk = fc.prefix_counts(rng, 272)
    assert np.array_equal(np.isfinite(walk).sum(axis=1), np.arange(273))
    other = _lists(rng, 273, 12, True)
    ts, im = (walk, other) if side == "text" else (other, walk)
    _check(cuda, ts, im, 6, oracle_step=7)


@pytest.mark.parametrize("pairing", ["deg|random", "random|deg", "deg|rolled", "deg|same"])
def test_fusion_degenerate_statistics(cuda, pairing):
    """Constant, one-step-off and adjacent-float lists (tests/_fusion_cases.py; what they reach is
    pinned on the host by test_fusion_cases_cpu.py): std == 0 against a one-step std, and the tie
    order between text and image items."""
    import _fusion_cases as fc

    deg = fc.pad(fc.degenerate_lists())
    rnd = fc.pad(fc.random_lists(np.random.default_rng(3), len(deg), 300))
    ts, im = {"deg|random": (deg, rnd), "random|deg": (rnd, deg), "deg|rolled": (deg, np.roll(deg, 7, axis=0)),
              "deg|same": (deg, deg)}[pairing]
    _check(cuda, ts, im, 24, oracle_step=9)


def test_fusion_score_range(cuda):
    """Scores at 1.0, one ulp above and below, negative down to -1, subnormal, and mixes of them."""
    import _fusion_cases as fc

    rng = np.random.default_rng(8)
    a = fc.score_range_lists(rng)
    b = fc.score_range_lists(rng)
    assert len(a) == len(b)
    ts, im = fc.pad(a), fc.pad(b[::-1])
    _check(cuda, ts, im, 12, oracle_step=3)
    _check(cuda, ts, fc.pad(fc.random_lists(rng, len(a), 40)), 5, oracle_step=5)


def test_fusion_long_lists_huge_z(cuda):
    """|z| <= sqrt(n): a combined score beyond 1e3 needs lists of more than 10^6 items. Two lists of
    2^20 + 1 equal scores but for one (tests/_fusion_cases.py), on both sides: z = +1024 and +1024.0005
    among a million near-zero ones, 14 levels of the pairwise sum."""
    import _fusion_cases as fc

    lists = fc.long_one_off_lists()
    _, gc = _check(cuda, fc.pad(lists), fc.pad(lists[::-1]), 8, oracle_step=0)
    assert np.all(np.abs(gc).max(axis=1) > 1e3)

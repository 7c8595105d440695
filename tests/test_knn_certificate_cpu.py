"""The conditions that make tests/test_knn_certificate_gpu.py mean something, checked without a
GPU on a numpy restatement of the row preparation (tests/_adversarial.py):

* the directed rows reach the error they are built for (down x down at least 0.55 eps below the
  cosine, up x up as far above, down x up on it), at every width and both magnitude profiles;
* no pair, planted or random, exceeds the bound of DESIGN.md §3.3 less its f32 accumulation term
  (the emulation sums in f64);
* in every case the GPU test searches, each query has at least k + 32 rows (SearchPlan::M's upper
  limit) whose fp16 score beats its weakest true neighbour's by more than D * 2^-23, twice the
  accumulation term: that row cannot be among the rescored candidates, the certificate cannot
  hold, and only the eps window of the collect stage brings the row back;
* the f64 oracle's top-k of each query is exactly its planted true rows;
* each case takes the path of the search plan that its name says.

eps is restated here from DESIGN.md §3.3 / §3.3a, not read from the library.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import _adversarial as adv
from oracle.knn import cosine_scores, flat_cosine_topk
from test_knn_plan_cpu import GENERIC, V1, V3, _plan, plan_lib  # noqa: F401  (plan_lib is a fixture)

WIDTHS = (100, 128, 256, 384, 512, 768)
PROFILES = ("gauss", "flat")


def eps_for_dim(D: int) -> float:
    """(2u + u^2) sum|q x| + D 2^-24 (f32 accumulation) + fp16 subnormals
    (2 sqrt(D) 2^-25) + f32 normalisation (4e-6), with 2 % to spare, never below 1.05e-3."""
    u = 2.0 ** -11
    e = (2 * u + u * u) + D * 2.0 ** -24 + 2.0 * math.sqrt(D) * 2.0 ** -25 + 4e-6
    return max(1.05e-3, 1.02 * e)


def test_eps_restated():
    for D in WIDTHS:
        assert eps_for_dim(D) == adv.EPS == 1.05e-3


@functools.lru_cache(maxsize=None)
def _planted_pairs(D, profile, nbase=4, per=50):
    """(query, rows) of each kind for nbase base vectors: rows at cosine 1 - 2e-4 to the query."""
    rng = np.random.default_rng(1000 + D)
    b = adv.profile_base(nbase, D, rng, profile)
    bb = np.repeat(b, per, 0)
    qd, qu = adv.directed_rows(b, adv.DOWN, rng), adv.directed_rows(b, adv.UP, rng)
    xd, xu = adv.directed_rows(bb, adv.DOWN, rng, 2e-4), adv.directed_rows(bb, adv.UP, rng, 2e-4)

    def err(q, x):
        out = [adv.emulated_scores(q[j:j + 1], x[j * per:(j + 1) * per])
               - cosine_scores(x[j * per:(j + 1) * per], q[j:j + 1]) for j in range(nbase)]
        return np.concatenate(out, axis=None)

    return err(qd, xd), err(qu, xu), err(qd, xu), (qd, qu, xd, xu)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("D", WIDTHS)
def test_directed_rows_round_one_way(D, profile):
    """After the library's preparation every component of a down row is the fp16 grid point at or
    below its magnitude, every component of an up row the one above."""
    _, _, _, (qd, qu, xd, xu) = _planted_pairs(D, profile)
    for rows, frac in ((qd, adv.DOWN), (xd, adv.DOWN), (qu, adv.UP), (xu, adv.UP)):
        v = rows.astype(np.float64)
        v = np.abs(v / np.linalg.norm(v, axis=1, keepdims=True))
        h = np.abs(adv.prepared_f16(rows).astype(np.float64))
        st = adv._step(v)
        pos = (v - np.floor(v / st) * st) / st  # fraction of a step above the grid point below
        assert np.all(np.abs(pos - frac) < 0.01), (D, profile, float(np.abs(pos - frac).max()))
        want = np.floor(v / st) * st + (st if frac > 0.5 else 0.0)
        np.testing.assert_array_equal(h, want)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("D", WIDTHS)
def test_error_reached(D, profile):
    eps = eps_for_dim(D)
    dd, uu, du, _ = _planted_pairs(D, profile)
    worst = max(np.abs(dd).max(), np.abs(uu).max(), np.abs(du).max()) / eps
    print(f"D {D} {profile}: mean down x down {dd.mean() / eps:+.3f} eps, up x up {uu.mean() / eps:+.3f} eps, "
          f"down x up {du.mean() / eps:+.3f} eps, largest |error| {worst:.3f} eps")
    assert dd.mean() <= -0.55 * eps
    assert uu.mean() >= 0.55 * eps
    assert abs(du.mean()) <= 0.05 * eps


@pytest.mark.parametrize("D", WIDTHS)
def test_bound_respected(D):
    eps = eps_for_dim(D)
    bound = eps - D * 2.0 ** -24
    worst = 0.0
    for profile in PROFILES:
        for e in _planted_pairs(D, profile)[:3]:
            worst = max(worst, float(np.abs(e).max()))
    rng = np.random.default_rng(2000 + D)
    q = rng.standard_normal((100, D)).astype(np.float32)
    x = rng.standard_normal((100, D)).astype(np.float32) * np.float32(3.0)
    x[:50] = q[:50] + 0.05 * rng.standard_normal((50, D)).astype(np.float32)  # half the pairs nearly parallel
    rnd = float(np.abs(adv.emulated_scores(q, x) - cosine_scores(x, q)).max())  # 100 x 100 pairs
    print(f"D {D}: largest |emulated - exact| / eps: planted {worst / eps:.3f}, 10000 random pairs {rnd / eps:.3f} "
          f"(bound {bound / eps:.3f})")
    assert worst <= bound and rnd <= bound


@pytest.mark.parametrize("name", sorted(adv.GPU_CASES))
def test_gpu_case_preconditions(name):
    D, k, n, nq, nbase, profile = adv.GPU_CASES[name]
    eps = eps_for_dim(D)
    c = adv.gpu_case(name)
    assert c.x.shape == (n, D) and c.q.shape == (nbase, D) and c.up_rows.shape[1] >= k + 48
    assert np.unique(c.planted).size == c.planted.size
    # spread over the whole corpus: many tiles, from the first twentieth to the last
    assert np.unique(c.planted // 64).size > 0.5 * min(c.planted.size, n // 64)
    assert c.planted.min() < 0.05 * n and c.planted.max() > 0.95 * n
    qn = c.q.astype(np.float64)
    qn /= np.linalg.norm(qn, axis=1, keepdims=True)
    assert (qn @ qn.T - np.eye(nbase)).max() < 0.5  # well-separated base vectors
    os_, or_ = flat_cosine_topk(c.x, np.zeros(n), c.q, k)
    ahead_min, win_min = n, np.inf
    for j in range(nbase):
        t, u = c.true_rows[j], c.up_rows[j]
        # the oracle sees the planted rows
        np.testing.assert_array_equal(np.sort(or_[j]), np.sort(t))
        ex_t, ex_u = cosine_scores(c.x[t], c.q[j:j + 1])[0], cosine_scores(c.x[u], c.q[j:j + 1])[0]
        gap = ex_t[:, None] - ex_u[None, :]
        assert 0.2 * eps <= gap.min() and gap.max() <= 0.4 * eps, (gap.min() / eps, gap.max() / eps)
        # the proof must fail
        em_t, em_u = adv.emulated_scores(c.q[j:j + 1], c.x[t])[0], adv.emulated_scores(c.q[j:j + 1], c.x[u])[0]
        ahead = int(np.sum(em_u > em_t.min() + D * 2.0 ** -23))
        assert ahead >= k + 32, (j, ahead)
        ahead_min = min(ahead_min, ahead)
        # how far below the k-th exact score of the rows ahead the weakest true row's fp16 score
        # lies: a collect window narrower than this loses the row
        first = np.argsort(-em_u)[: k + 32]
        win_min = min(win_min, (np.sort(ex_u[first])[::-1][k - 1] - em_t.min()) / eps)
    if profile == "flat":
        assert win_min > 0.5  # a window of eps / 2 would lose a true neighbour of every query
    print(f"{name}: at least {ahead_min} rows ahead of the weakest true neighbour (k + 32 = {k + 32}); "
          f"it lies {win_min:.3f} eps below the k-th exact score of the rows ahead")


def test_gpu_case_paths(plan_lib):  # noqa: F811
    """Each case takes the path it is named for, with several tiles in every split."""
    P = lambda name: _plan(plan_lib, *(adv.GPU_CASES[name][i] for i in (2, 3, 1, 0)))  # noqa: E731
    for name in ("k7s-512-k10", "k7s-512-k10-gauss"):
        p = P(name)
        assert (p["path"], p["qb"], p["qpg"], p["sampled"]) == (V3, 1, 64, 0) and p["ntiles"] >= 2 * p["S"], p
    for name in ("v3-128-k10", "v3-128-k50", "v3-384-k10", "v3-384-k50"):
        p = P(name)
        assert (p["path"], p["qb"], p["qpg"], p["sampled"]) == (V3, 4, 256, 0) and p["ntiles"] >= 3 * p["S"], p
    p = P("v3-counting-128-k10")
    assert (p["path"], p["qb"], p["sampled"], p["counting"], p["S"], p["ntiles"] // p["S"]) == (V3, 4, 1, 1, 64, 65), p
    p = P("v1-256-k100")
    assert (p["path"], p["KL"], p["M"]) == (V1, 16, 132) and p["ntiles"] >= 3 * p["S"], p
    assert P("k7g-768-k10")["path"] == GENERIC and P("k7g-512-k300")["path"] == GENERIC

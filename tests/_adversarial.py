"""Inputs that drive the fp16 score error of the kNN scan toward its bound.

Gaussian corpora round every component with a random sign, so the error of an fp16 dot product
cancels to a few 1e-5. The rows built here do not cancel: after the library's preparation
(f64 norm, ``x * (1/|x|)`` in f64, cast to f32, then to fp16) every component of a row sits a
chosen fraction of an fp16 step above the grid point below its magnitude, so a whole row rounds
toward zero ("down", fraction 0.47) or away from it ("up", 0.53). The fp16 dot product of two
nearly parallel down rows then comes out about 0.6 eps below their cosine, two up rows as far
above, and a down row against an up row lands on it.

Plain numpy, no GPU: ``emulated_scores`` restates the preparation kernel, so the fp16 values
are the ones the library stores.
"""
from __future__ import annotations

import numpy as np

DOWN, UP = 0.47, 0.53
EPS = 1.05e-3  # DESIGN.md §3.3 / §3.3a for every width up to 768 (restated in the CPU test)


def _step(a: np.ndarray) -> np.ndarray:
    """fp16 grid spacing at magnitude ``a`` (f64): 2^(e-10) in binade e, 2^-24 below 2^-14."""
    _, e = np.frexp(a)  # a = m * 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - 11, -24))


def _snap(a: np.ndarray, frac: float) -> np.ndarray:
    """Each magnitude moved to ``frac`` of a step above the fp16 grid point at or below it."""
    st = _step(a)
    return np.where(a > 0, (np.floor(a / st) + frac) * st, 0.0)


def _norms(y: np.ndarray) -> np.ndarray:
    y = y.astype(np.float32).astype(np.float64)  # the values the library will read
    return np.sqrt(np.einsum("ij,ij->i", y, y))


def _settle(y: np.ndarray, rounds: int = 4) -> np.ndarray:
    """Bring the snapped magnitudes' row norms closer to 1 by moving, per round, the one component
    of each row whose whole fp16 step best cancels what is left of 1 - |y|^2 (it stays the same
    fraction of a step above a grid point, within its binade)."""
    n, d = y.shape
    rows = np.arange(n)
    for _ in range(rounds):
        r = 1.0 - np.einsum("ij,ij->i", y, y)
        st = _step(y)
        _, e = np.frexp(y)
        edge = np.ldexp(0.5, e)  # lower edge of the component's binade
        up = np.where((y > 0) & (y + st < 2.0 * edge), 2.0 * y * st + st * st, np.inf)
        dn = np.where((y > 0) & (y - st >= edge), -(2.0 * y * st - st * st), np.inf)
        cand = np.concatenate([up, dn], axis=1)
        j = np.argmin(np.abs(cand - r[:, None]), axis=1)
        better = np.abs(cand[rows, j] - r) < np.abs(r)
        i = j % d
        y[rows, i] += np.where(better, np.where(j < d, 1.0, -1.0) * st[rows, i], 0.0)
    return y


def directed_rows(base: np.ndarray, frac: float, rng: np.random.Generator, noise=0.0) -> np.ndarray:
    """f32 rows near the f64 unit vectors ``base`` [n, D] whose every component, after the
    library's preparation, lies ``frac`` of an fp16 step above the grid point below its magnitude.

    ``noise`` (a scalar or [n]) is 1 - cosine of the row to its base vector, in a random direction
    (0: the base vector itself). The scale of a row is the one, found by bisection on the scale
    (the snapped norm is a rising staircase in it), that brings its norm closest to 1, settled by
    whole-step moves of single components, so the library's own normalisation moves nothing across
    a rounding midpoint."""
    base = np.asarray(base, np.float64)
    n, d = base.shape
    c = 1.0 - np.broadcast_to(np.asarray(noise, np.float64), (n,))
    w = rng.standard_normal((n, d))
    w -= np.einsum("ij,ij->i", w, base)[:, None] * base
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    t = c[:, None] * base + np.sqrt(np.maximum(0.0, 1.0 - c * c))[:, None] * w
    sign, a = np.sign(t), np.abs(t)
    lo = np.full(n, 1.0 - 1e-3)
    hi = np.full(n, 1.0 + 1e-3)
    for _ in range(20):
        mid = 0.5 * (lo + hi)
        below = _norms(_snap(mid[:, None] * a, frac)) < 1.0
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    ylo, yhi = _snap(lo[:, None] * a, frac), _snap(hi[:, None] * a, frac)
    y = np.where((np.abs(_norms(ylo) - 1.0) <= np.abs(_norms(yhi) - 1.0))[:, None], ylo, yhi)
    y = _settle(y)
    return (sign * y).astype(np.float32)


def prepared_f16(x: np.ndarray) -> np.ndarray:
    """``prep_rows_kernel`` in numpy: fp16(f32(x * (1/|x|))) with the norm and the product in f64."""
    xd = np.asarray(x, np.float32).astype(np.float64)
    nrm = np.sqrt(np.einsum("ij,ij->i", xd, xd))
    inv = np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)
    return (xd * inv[:, None]).astype(np.float32).astype(np.float16)


def emulated_scores(q: np.ndarray, x: np.ndarray) -> np.ndarray:
    """[nq, n] dot products of the fp16 operands the library stores, summed in f64."""
    return prepared_f16(q).astype(np.float64) @ prepared_f16(x).astype(np.float64).T


def profile_base(n: int, d: int, rng: np.random.Generator, profile: str = "gauss") -> np.ndarray:
    """f64 unit vectors: Gaussian components, or ``flat`` ones of random sign whose magnitudes
    sit low in two neighbouring fp16 binades (1.06 to 1.16 times a power of two, where a step is
    largest against the value), mixed so that the norm is 1."""
    if profile == "gauss":
        b = rng.standard_normal((n, d))
    else:
        e = np.floor(np.log2(1.0 / (1.11 * np.sqrt(d))))  # 1.11 * 2^e <= 1/sqrt(d) < 1.11 * 2^(e+1)
        p_hi = (1.0 / (1.11 ** 2 * d) - 4.0 ** e) / (3.0 * 4.0 ** e)  # share at 2^(e+1)
        hi = rng.random((n, d)) < p_hi
        b = np.ldexp(rng.uniform(1.06, 1.16, (n, d)), np.where(hi, int(e) + 1, int(e)))
        b *= rng.choice([-1.0, 1.0], (n, d))
    return b / np.linalg.norm(b, axis=1, keepdims=True)


class CertificateCase:
    """One corpus and one batch of down queries with their planted rows (``certificate_case``)."""

    def __init__(self, x, q, true_rows, up_rows, k):
        self.x, self.q, self.true_rows, self.up_rows, self.k = x, q, true_rows, up_rows, k

    @property
    def planted(self) -> np.ndarray:
        return np.concatenate([self.true_rows.ravel(), self.up_rows.ravel()])


TRUE_NOISE = 2e-4   # 1 - cosine of a true neighbour to its query
EXTRA_UP = 64       # up rows per query beyond k (k + 32 of them must come out ahead)
UP_GAP = (0.21, 0.24)  # an up row's cosine below the true rows', in eps


def certificate_case(D: int, k: int, n: int, seed, nbase: int = 8, profile: str = "flat") -> CertificateCase:
    """A corpus of ``n`` rows and ``nbase`` down queries whose fp16 certificate must fail.

    Per query, among Gaussian filler: k down rows at cosine about 1 - TRUE_NOISE (the true
    top-k) and k + EXTRA_UP up rows whose exact cosine is lower than every true row's by
    0.2 to 0.4 eps (drawn UP_GAP eps below, the snap adds under a hundredth) while their fp16
    score comes out higher than the true rows', which the scan sees 0.6 to 0.8 eps too low.
    With the flat profile and the gap at the low end of its range, the weakest true row's fp16
    score lies more than eps / 2 below the k-th exact score of the rows that outrank it, so a
    collect window of half the width loses it. Planted rows take shuffled positions over the
    whole corpus. Every query has its own base vector (pairwise cosine below 0.5), so one query's
    planted rows are filler for the others."""
    rng = np.random.default_rng(seed)
    base = profile_base(nbase, D, rng, profile)
    q = directed_rows(base, DOWN, rng)
    qd = q.astype(np.float64)
    qd /= np.linalg.norm(qd, axis=1, keepdims=True)
    nup = k + EXTRA_UP
    x = rng.standard_normal((n, D)).astype(np.float32)
    pos = rng.choice(n, nbase * (k + nup), replace=False)
    true_rows = pos[: nbase * k].reshape(nbase, k)
    up_rows = pos[nbase * k:].reshape(nbase, nup)
    for j in range(nbase):
        x[true_rows[j]] = directed_rows(np.repeat(qd[j:j + 1], k, 0), DOWN, rng, TRUE_NOISE)
        x[up_rows[j]] = directed_rows(np.repeat(qd[j:j + 1], nup, 0), UP, rng,
                                      TRUE_NOISE + rng.uniform(*UP_GAP, nup) * EPS)
    return CertificateCase(x, q, true_rows, up_rows, k)


# The shapes tests/test_knn_certificate_gpu.py searches, one per path of the plan (csrc/knn_plan.h;
# tests/test_knn_certificate_cpu.py checks each against plan_search): name -> D, k, rows, queries,
# base vectors (queries cycle over them), magnitude profile. Each is the smallest corpus that takes
# its path with several tiles in every split: a batch of up to 256 queries scans in 256 splits, so
# 50,000 rows give three tiles per split (20,000 give one); the counting sample pass needs 64 tiles
# per split, which 270,000 rows have once the batch fills four query groups (769 queries, 64
# splits of 65 tiles: with 65 queries the 256 splits hold 16 tiles each and nothing is sampled).
GPU_CASES = {
    "k7s-512-k10": (512, 10, 40_000, 8, 8, "flat"),
    "k7s-512-k10-gauss": (512, 10, 40_000, 8, 8, "gauss"),
    "v3-128-k10": (128, 10, 50_000, 65, 65, "flat"),
    "v3-128-k50": (128, 50, 50_000, 65, 65, "flat"),
    "v3-384-k10": (384, 10, 50_000, 65, 65, "flat"),
    "v3-384-k50": (384, 50, 50_000, 65, 65, "flat"),
    "v3-counting-128-k10": (128, 10, 270_000, 769, 8, "flat"),
    "v1-256-k100": (256, 100, 50_000, 8, 8, "flat"),
    "k7g-768-k10": (768, 10, 20_000, 8, 8, "flat"),
    "k7g-512-k300": (512, 300, 20_000, 8, 8, "flat"),
}
_BUILT = {}


def gpu_case(name: str) -> CertificateCase:
    """The named case of GPU_CASES, built once per process; ``qidx`` maps each of its queries to
    its base vector and ``labels`` admits (label 1) the true rows, every other up row and about
    half of the filler."""
    if name not in _BUILT:
        D, k, n, nq, nbase, profile = GPU_CASES[name]
        c = certificate_case(D, k, n, sorted(GPU_CASES).index(name) + 100, nbase=nbase, profile=profile)
        c.qidx = np.arange(nq) % nbase
        lab = np.random.default_rng(7).integers(0, 2, n).astype(np.int32)
        lab[c.true_rows.ravel()] = 1
        lab[c.up_rows[:, 0::2].ravel()] = 1
        lab[c.up_rows[:, 1::2].ravel()] = 0
        c.labels = lab
        _BUILT[name] = c
    return _BUILT[name]


def planted_first(c: CertificateCase, front: bool) -> np.ndarray:
    """Permutation of the corpus rows (new position -> old row) that moves the planted rows, in a
    shuffled order, to the front (or the back) and keeps the filler's order."""
    planted = np.random.default_rng(11).permutation(c.planted)
    rest = np.setdiff1d(np.arange(len(c.x)), planted)
    return np.concatenate([planted, rest] if front else [rest, planted])

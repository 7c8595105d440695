"""Hit-score lists for the K12 (z-score fusion) tests, shared by the GPU comparison in
test_fusion_gpu.py and the CPU check of what they reach in test_fusion_cases_cpu.py. Every list is
a 1-D f32 array of finite scores in [-2, 2]; ``pad`` lays lists out as ``FlatIndex.search`` returns
them: one row each, missing hits ``-inf`` at the end."""
from __future__ import annotations

import numpy as np

F = np.float32
DEGENERATE_N = (2, 3, 7, 8, 9, 10, 100, 128, 129, 300)
DEGENERATE_V = tuple(F(v) for v in (0.1, 0.7, 1.0 / 3.0, 1.0, 0.0, -0.25))
# the caller-visible score 1 - f32(1 - s) is a multiple of 2^-24 for |s| < 1: a one-ulp step of s
# below 0.5 can vanish there, so the families also step by 2^-24, which never does
STEP = F(2.0 ** -24)


def pad(lists, width=None) -> np.ndarray:
    width = max([len(v) for v in lists] + [0]) if width is None else width
    out = np.full((len(lists), width), -np.inf, dtype=np.float32)
    for i, v in enumerate(lists):
        out[i, :len(v)] = v
    return out


def random_lists(rng, q: int, k: int, full: bool = False):
    """Ordinary lists: uniform scores sorted descending, random valid counts."""
    out = []
    for _ in range(q):
        n = k if full else int(rng.integers(1, k + 1))
        out.append(-np.sort(-rng.uniform(-0.2, 0.9, n).astype(np.float32)))
    return out


def prefix_counts(rng, k: int):
    """Row i has exactly i finite scores (i = 0 .. k), sorted descending: every leaf boundary of
    numpy's pairwise sum."""
    s = -np.sort(-rng.uniform(-0.2, 0.9, (k + 1, k)).astype(np.float32), axis=1)
    s[np.arange(k)[None, :] >= np.arange(k + 1)[:, None]] = -np.inf
    return s


def degenerate_lists():
    """Lists whose f32 mean / std decide everything: constant; constant but for the first or last
    element one ulp (and one 2^-24 step) higher or lower; two adjacent floats."""
    out = []
    for n in DEGENERATE_N:
        for v in DEGENERATE_V:
            out.append(np.full(n, v, dtype=np.float32))
            for pos in (0, n - 1):
                for other in (np.nextafter(v, F(2)), np.nextafter(v, F(-2)), F(v + STEP), F(v - STEP)):
                    a = np.full(n, v, dtype=np.float32)
                    a[pos] = other
                    out.append(a)
    for v in DEGENERATE_V + (F(0.99999994), F(0.5), F(-1.0)):
        hi = np.nextafter(v, F(2))
        out.append(np.array([hi, v], dtype=np.float32))
        out.append(np.array([v, hi], dtype=np.float32))
    return out


LONG_N = (1 << 20) + 1


def long_one_off_lists():
    """|z| <= sqrt(n) for any list (std^2 >= (x_j - mean)^2 / n), so the lists above (n <= 300) stay
    below 17.4. A z beyond 1e3 needs more than 10^6 items: LONG_N equal scores but for one, one
    2^-24 step away, whose f32 sum and mean are exact. [step, 0, 0 ...] has z_0 = +1024;
    [1, 1 ... 1 + 2^-23] has the mean 1.0 exactly, z_last = +1024.0005 and every other z exactly 0.
    The size is the smallest that reaches the outcome; it also takes the pairwise sum 14 levels deep."""
    a = np.zeros(LONG_N, dtype=np.float32)
    a[0] = STEP
    b = np.ones(LONG_N, dtype=np.float32)
    b[-1] = np.nextafter(F(1), F(2))
    return [a, b]


def score_range_lists(rng):
    """Scores at and above 1.0 (the self-match through 1 - f32(1 - s)), just below it, negative
    down to -1, subnormal; alone, repeated, and mixed with ordinary scores; sorted descending."""
    special = np.array([np.nextafter(F(1), F(2)), 1.0, 0.99999994, 0.5, 1e-41, 0.0, -1e-41, -0.3, -1.0],
                       dtype=np.float32)
    assert special[4] != 0 and abs(special[4]) < np.finfo(np.float32).tiny
    out = [special.copy()]
    for v in special:
        out.append(np.array([v], dtype=np.float32))
        out.append(np.full(9, v, dtype=np.float32))
    for n in (2, 5, 8, 9, 17, 64, 129, 200):
        for _ in range(6):
            m = int(rng.integers(1, n + 1))
            a = np.concatenate([rng.choice(special, m), rng.uniform(-1, 1, n - m).astype(np.float32)])
            out.append(-np.sort(-a.astype(np.float32)))
    return out

"""Numpy / pure-Python restatement of the MMR selection, the oracle of
tests/test_knn_mmr_cpu.py and tests/test_knn_mmr_gpu.py.

Per query, with candidates in the search's order, scores ``s`` and pairwise cosines ``c``:
step 0 takes the first valid candidate (row >= 0 and score > -inf), step t >= 1 the unselected
valid candidate with the largest ``v = lam * s - (1 - lam) * p``, ``p`` the largest cosine to a
selected candidate; ties go to the smaller position; a list that runs out pads with -1 / -inf.
``v`` is evaluated in Python floats: two products and one subtraction, each rounded once.

Cosines between stored rows are exactly rounded: the products of two f32 values are exact in
f64, ``math.fsum`` sums them without error, so byte-identical rows give bit-identical cosines
and tie exactly, as they do in the kernel (whose sums are not exactly rounded but are the same
sums for the same bytes).

Besides positions and values the oracle returns the minimum decision margin: over every step
t >= 1, the winner's ``v`` minus the best ``v`` among the other candidates whose row bytes
differ from the winner's. A comparison with the GPU is valid only when that margin is at least
``margin_bound(D)``: the kernel's f64 accumulation differs from the exact sums by about
``D * 2**-53`` per cosine, two cosines enter a ``v``, 64 is headroom.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Tuple

import numpy as np

NEG_INF = float("-inf")


def margin_bound(d: int) -> float:
    return 64.0 * (d + 16) * 2.0 ** -53


def value(lam: float, s: float, p: float) -> float:
    rel = lam * s
    pen = (1.0 - lam) * p
    return rel - pen


def select_one(valid, s, cos: Callable[[int, int], float], k: int, lam: float,
               same: Optional[Callable[[int, int], bool]] = None) -> Tuple[list, list, float]:
    """One query. ``cos(i, j)``: pairwise score of candidate positions; ``same(i, j)``: whether
    their rows are byte-identical (excluded from the margin). Returns (pos[k], v[k], margin)."""
    m = len(s)
    lam = float(lam)
    p = [NEG_INF] * m
    taken = [False] * m
    cur = next((i for i in range(m) if valid[i]), None)
    curv = value(lam, float(s[cur]), 0.0) if cur is not None else NEG_INF
    pos, vals, margin = [], [], math.inf
    for t in range(k):
        pos.append(-1 if cur is None else cur)
        vals.append(NEG_INF if cur is None else curv)
        if cur is None or t + 1 == k:
            continue
        taken[cur] = True
        best, bv, vs = None, NEG_INF, {}
        for i in range(m):
            if taken[i] or not valid[i]:
                continue
            c = cos(i, cur)
            if c > p[i]:
                p[i] = c
            v = value(lam, float(s[i]), p[i])
            vs[i] = v
            if best is None or v > bv:  # ascending i: a tie keeps the smaller position
                best, bv = i, v
        if best is not None:
            others = [v for i, v in vs.items() if i != best and not (same is not None and same(i, best))]
            if others:
                margin = min(margin, bv - max(others))
        cur, curv = best, bv
    return pos, vals, margin


class RowCosine:
    """Exactly rounded cosines between rows of ``x`` (f32 [n, d]), cached per pair."""

    def __init__(self, x: np.ndarray):
        self.x = np.ascontiguousarray(x, dtype=np.float32)
        self.x64 = self.x.astype(np.float64)
        self._norm = {}
        self._cos = {}
        self._bytes = {}

    def norm(self, r: int) -> float:
        n = self._norm.get(r)
        if n is None:
            v = self.x64[r]
            n = self._norm[r] = math.sqrt(math.fsum((v * v).tolist()))
        return n

    def cos(self, a: int, b: int) -> float:
        key = (a, b) if a <= b else (b, a)
        c = self._cos.get(key)
        if c is None:
            na, nb = self.norm(a), self.norm(b)
            if na > 0.0 and nb > 0.0:
                c = math.fsum((self.x64[a] * self.x64[b]).tolist()) / (na * nb)
            else:
                c = 0.0
            self._cos[key] = c
        return c

    def query_cos(self, q: np.ndarray, r: int) -> float:
        """Exactly rounded cosine of an f32 query and row r (a relevance score)."""
        q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
        nq = math.sqrt(math.fsum((q64 * q64).tolist()))
        nr = self.norm(r)
        if not (nq > 0.0 and nr > 0.0):
            return 0.0
        return math.fsum((q64 * self.x64[r]).tolist()) / (nq * nr)

    def same(self, a: int, b: int) -> bool:
        if a == b:
            return True
        for r in (a, b):
            if r not in self._bytes:
                self._bytes[r] = self.x[r].tobytes()
        return self._bytes[a] == self._bytes[b]


def mmr_oracle(rc: RowCosine, rows: np.ndarray, scores64: np.ndarray, k: int, lam: float):
    """``rows`` int64 [nq, m] (local row ids, -1 empty), ``scores64`` f64 [nq, m]. Returns
    (pos int32 [nq, k], v f64 [nq, k], the minimum decision margin over all queries and steps)."""
    rows = np.asarray(rows, dtype=np.int64)
    s = np.asarray(scores64, dtype=np.float64)
    nq, m = rows.shape
    pos = np.full((nq, k), -1, np.int32)
    val = np.full((nq, k), NEG_INF, np.float64)
    margin = math.inf
    for qi in range(nq):
        r = rows[qi].tolist()
        sq = s[qi].tolist()
        valid = [ri >= 0 and si > NEG_INF for ri, si in zip(r, sq)]
        p, v, mg = select_one(valid, sq, lambda i, j: rc.cos(r[i], r[j]), k, lam,
                              lambda i, j: rc.same(r[i], r[j]))
        pos[qi] = p
        val[qi] = v
        margin = min(margin, mg)
    return pos, val, margin


def gather(pos: np.ndarray, *arrays, fill=(NEG_INF, -1)):
    """The host composition's last stage: ``arrays`` [nq, m] taken at ``pos`` [nq, k]; a slot
    with pos -1 gets -inf for a float array and -1 for an integer one."""
    safe = np.where(pos >= 0, pos, 0).astype(np.int64)
    out = []
    for a in arrays:
        g = np.take_along_axis(np.asarray(a), safe, axis=1)
        pad = fill[0] if np.issubdtype(g.dtype, np.floating) else fill[1]
        out.append(np.where(pos >= 0, g, np.asarray(pad, dtype=g.dtype)))
    return out

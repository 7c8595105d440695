"""K6 (csrc/l2norm.hip, mrag_l2norm_rows) against the reference's three numpy lines, bit for bit:
every width 1..1100 (each leaf shape of the wave kernel, the compile-time widths 384 / 512 / 768,
both sides of the 968 / 969 switch) plus 2048 and 4097, and 20000 and 100003 (past the 8192-element
blocks numpy sums in, where the kernel adds block sums in order), out of place and in place
(``y == x``, the form the encoders run), row counts around the 4- and 64-rows-per-block tails behind guard rows, and
rows of zeros, signed zeros, underflowing / subnormal / overflowing squares, subnormal quotients,
inf and NaN. Outputs are compared as uint32 patterns (so the sign of a zero counts), NaN positions
separately. The entry point is called through the C ABI with explicit pointers."""
from __future__ import annotations

import numpy as np
import pytest

SENTINEL = np.float32(-12345.678)
EDGE_DIMS = (5, 96, 300, 384, 512, 768, 1000)


def reference(x: np.ndarray) -> np.ndarray:
    """app/ml/embeddings.py:46-49 of the reference, on the same f32 array."""
    with np.errstate(all="ignore"):
        norms = np.linalg.norm(x, axis=1, keepdims=True)
        norms[norms == 0] = 1.0
        out = x / norms
    assert out.dtype == np.float32
    return out


def assert_same_bits(got: np.ndarray, ref: np.ndarray, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, what
    gn, rn = np.isnan(got), np.isnan(ref)
    np.testing.assert_array_equal(gn, rn, err_msg=f"NaN positions {what}")
    g = np.where(gn, np.float32(0), got).view(np.uint32)
    r = np.where(rn, np.float32(0), ref).view(np.uint32)
    np.testing.assert_array_equal(g, r, err_msg=f"bit patterns {what}")


def random_rows(rng, rows: int, dim: int) -> np.ndarray:
    scale = 10.0 ** rng.uniform(-3, 3, (rows, 1))
    return (rng.standard_normal((rows, dim)) * scale).astype(np.float32)


def edge_matrix(dim: int) -> np.ndarray:
    """One row per edge the kernel's arithmetic can get wrong (see the module docstring)."""
    rng = np.random.default_rng(1000 + dim)
    sign = np.where(rng.integers(0, 2, dim) == 1, 1.0, -1.0)
    mag = rng.uniform(0.5, 2.0, dim)
    f32 = np.float32
    rows = []
    rows.append(np.zeros(dim))                                   # 0: zeros
    rows.append(np.full(dim, -0.0))                              # 1: -0.0 everywhere
    r = np.zeros(dim); r[1 % dim] = -0.0; rows.append(r)         # 2: one -0.0 among zeros
    rows.append(sign * mag * 1e-30)                              # 3: squares underflow to 0, norm -> 1
    rows.append(sign * mag * 1e-20)                              # 4: subnormal squares (1e-40)
    rows.append(sign * mag * 3e-23)                              # 5: squares of a few subnormal ulps
    r = sign * mag * 3e-23; r[::2] = (sign * mag * 1e-20)[::2]; rows.append(r)  # 6: both, mixed
    r = np.full(dim, f32(1e-41), dtype=np.float64) * sign; r[dim // 2] = 1.0; rows.append(r)  # 7: norm 1
    r = sign * mag * 1e-41; r[dim // 3] = 3.0; rows.append(r)    # 8: subnormal / 3: rounded subnormal quotients
    r = sign * mag * 1e-38; r[0] = 7.0; rows.append(r)           # 9: normal inputs, subnormal quotients
    rows.append(sign * mag * 1e20)                               # 10: squares overflow, norm inf, outputs +-0
    r = sign * mag; r[dim - 1] = np.inf; rows.append(r)          # 11: inf / inf = NaN, finite / inf = +-0
    r = sign * mag; r[0] = -np.inf; r[dim - 1] = 1e30; rows.append(r)  # 12: -inf
    r = sign * mag; r[dim // 2] = np.nan; rows.append(r)         # 13: NaN norm
    r = sign * mag * 1e-10; r[dim // 2] = 1e18; rows.append(r)   # 14: one huge, many tiny
    r = np.zeros(dim); r[dim - 1] = np.finfo(f32).max; rows.append(r)  # 15: f32 max alone
    r = sign * mag * 1e-3; r[2 % dim] = -np.finfo(f32).max; rows.append(r)  # 16: -max among small
    with np.errstate(all="ignore"):
        return np.stack(rows).astype(np.float32)


def pairwise_leaves(n: int):
    """Leaf lengths of numpy's pairwise summation of n contiguous elements, in order."""
    if n <= 128:
        return [n]
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_leaves(n2) + pairwise_leaves(n - n2)


# ---- CPU: the inputs reach the branches they are meant to, and the dispatch claim holds ----------

def test_edge_matrix_reaches_every_branch():
    """The numpy reference of the edge matrix holds a subnormal output, a NaN, a -0.0 and an exact
    zero produced by an inf norm, at every tested width (a later change of the constants cannot
    quietly stop exercising them)."""
    tiny = np.finfo(np.float32).tiny
    for dim in EDGE_DIMS:
        x = edge_matrix(dim)
        ref = reference(x)
        with np.errstate(all="ignore"):
            norms = np.linalg.norm(x, axis=1)
            sq = x * x
        assert np.any((ref != 0) & (np.abs(ref) < tiny)), dim                 # subnormal quotient
        inexact = (np.abs(ref) < tiny) & (ref != 0) & (ref != x)
        assert np.any(inexact), dim                                           # ... that needed rounding
        assert np.any(np.isnan(ref)), dim
        assert np.any((ref == 0) & np.signbit(ref)), dim                      # -0.0
        inf_rows = np.isinf(norms)
        assert inf_rows.any() and np.any((ref[inf_rows] == 0) & (x[inf_rows] != 0)), dim
        assert np.any((sq != 0) & (sq < tiny)), dim                           # subnormal squares
        assert np.any((x != 0) & (sq == 0) & (norms[:, None] == 0)), dim      # underflow -> norm 1
        assert np.any(np.isinf(sq) & np.isfinite(x)), dim                     # overflowing squares


def test_pairwise_leaves_match_numpy_and_the_dispatch():
    """The wave kernel holds 8 leaves of at most 128 elements: true for every dim <= 968 and false
    at 969, where mrag_l2norm_rows switches to the thread-per-row kernel; the compile-time widths
    split into whole octets. The leaf restatement itself is checked against numpy's add.reduce, past
    8192 elements too, where numpy (and the kernels) sum block by block: that block size is numpy's
    default buffer size, and a numpy that changes it fails here without a GPU."""
    for n in range(1, 969):
        lv = pairwise_leaves(n)
        assert len(lv) <= 8 and max(lv) <= 128 and sum(lv) == n, n
        if n > 128:
            assert min(lv) >= 64, n
    assert len(pairwise_leaves(969)) == 9
    assert [len(pairwise_leaves(d)) for d in (384, 512, 768)] == [4, 4, 8]
    assert set(pairwise_leaves(768)) == {96}
    for d in (384, 512, 768):
        assert all(v % 8 == 0 for v in pairwise_leaves(d))

    def leaf_sum(v):
        f = np.float32
        if len(v) < 8:
            r = f(-0.0)
            for e in v:
                r = f(r + e)
            return r
        r = [f(e) for e in v[:8]]
        full = len(v) - len(v) % 8
        for i in range(8, full, 8):
            r = [f(r[j] + v[i + j]) for j in range(8)]
        res = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
        for e in v[full:]:
            res = f(res + e)
        return res

    def tree(v):
        if len(v) <= 128:
            return leaf_sum(v)
        n2 = len(v) // 2
        n2 -= n2 % 8
        return np.float32(tree(v[:n2]) + tree(v[n2:]))

    def blocks(v):  # add.reduce's inner loop gets at most np.getbufsize() == 8192 elements at a time
        tot = np.float32(-0.0)
        for o in range(0, len(v), 8192):
            tot = np.float32(tot + tree(v[o:o + 8192]))
        return tot

    assert np.getbufsize() == 8192
    rng = np.random.default_rng(5)
    for n in (1, 7, 8, 9, 127, 128, 129, 300, 768, 968, 969, 1100, 4097, 8192, 8193, 20000, 100003):
        whole_differs = 0
        for _ in range(1 if n <= 8192 else 6):
            v = (rng.standard_normal(n) ** 2).astype(np.float32)
            ref = np.add.reduce(v[None, :], axis=1)[0].view(np.uint32)
            assert blocks(v).view(np.uint32) == ref, n
            assert np.add.reduce(v).view(np.uint32) == ref, n  # 1-D and row reductions agree
            if n <= 8192:
                assert tree(v).view(np.uint32) == ref, n  # one block: the plain tree
            whole_differs += tree(v).view(np.uint32) != ref
        if n >= 20000:
            assert whole_differs, n  # these sizes tell the block loop from one tree over the row


# ---- GPU ------------------------------------------------------------------------------------------

def _launch(x_ptr, y_ptr, rows, dim):
    import torch

    from app import _native

    _native.call("mrag_l2norm_rows", x_ptr, y_ptr, rows, dim, torch.cuda.current_stream().cuda_stream)


def _run(cuda, x: np.ndarray, in_place: bool) -> np.ndarray:
    """The kernel on x [rows, dim] with one guard row before and after the output (the input too,
    when in place); asserts the guards are untouched."""
    import torch

    rows, dim = x.shape
    buf = np.full((rows + 2, dim), SENTINEL, dtype=np.float32)
    if in_place:
        buf[1:rows + 1] = x
        y = torch.from_numpy(buf).to(cuda)
        ptr = y.data_ptr() + dim * 4
        _launch(ptr, ptr, rows, dim)
    else:
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(cuda) if rows else torch.empty((1, dim), device=cuda)
        y = torch.from_numpy(buf).to(cuda)
        _launch(xd.data_ptr(), y.data_ptr() + dim * 4, rows, dim)
        if rows:
            assert_same_bits(xd.cpu().numpy(), x, "input modified")
    out = y.cpu().numpy()
    guard = np.full(dim, SENTINEL, dtype=np.float32).view(np.uint32)
    np.testing.assert_array_equal(out[0].view(np.uint32), guard, err_msg="row before the output written")
    np.testing.assert_array_equal(out[rows + 1].view(np.uint32), guard, err_msg="row after the output written")
    return out[1:rows + 1]


@pytest.mark.gpu
def test_every_width(cuda):
    import torch

    rng = np.random.default_rng(11)
    rows = 6
    dims = list(range(1, 1101)) + [2048, 4097, 20000, 100003]  # the last two: past numpy's 8192-element blocks
    xs = [random_rows(rng, rows, d) for d in dims]
    offs = np.concatenate([[0], np.cumsum([a.size for a in xs])])
    flat = np.concatenate([a.reshape(-1) for a in xs])
    xd = torch.from_numpy(flat).to(cuda)
    yd = torch.full_like(xd, float(SENTINEL))
    for d, o in zip(dims, offs[:-1]):
        _launch(xd.data_ptr() + int(o) * 4, yd.data_ptr() + int(o) * 4, rows, d)
    got = yd.cpu().numpy()
    bad = []
    for d, o, x in zip(dims, offs[:-1], xs):
        ref = reference(x)
        g = got[o:o + x.size].reshape(rows, d)
        if not np.array_equal(g.view(np.uint32), ref.view(np.uint32)):
            bad.append(d)
    assert not bad, f"widths that differ from numpy: {bad[:40]} ({len(bad)} in all)"


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [7, 128, 129, 384, 512, 768, 968, 969])
def test_in_place_equals_out_of_place(cuda, dim):
    x = random_rows(np.random.default_rng(dim), 67, dim)  # 16 blocks of 4 rows and a tail of 3
    ref = reference(x)
    assert_same_bits(_run(cuda, x, in_place=False), ref, f"out of place dim={dim}")
    assert_same_bits(_run(cuda, x.copy(), in_place=True), ref, f"in place dim={dim}")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [512, 300, 1000])
def test_row_tails_guarded(cuda, dim):
    rng = np.random.default_rng(dim + 1)
    for rows in (0, 1, 3, 4, 5, 63, 64, 65):
        x = random_rows(rng, rows, dim)
        ref = reference(x) if rows else x
        assert_same_bits(_run(cuda, x, in_place=False), ref, f"rows={rows} dim={dim}")
        assert_same_bits(_run(cuda, x.copy(), in_place=True), ref, f"in place rows={rows} dim={dim}")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", EDGE_DIMS)
def test_edge_values(cuda, dim):
    x = edge_matrix(dim)
    ref = reference(x)
    for in_place in (False, True):
        got = _run(cuda, x.copy(), in_place)
        for r in range(len(x)):  # row by row: the message names the edge
            assert_same_bits(got[r], ref[r], f"dim={dim} edge row {r} in_place={in_place}")

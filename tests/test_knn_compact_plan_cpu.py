"""The search paths that tests/test_knn_compact_gpu.py names for its shapes, checked on the CPU
with the plan helper of tests/test_knn_plan_cpu.py (csrc/knn_plan.h compiled for the host): the
compacted index and the fresh one hold the same number of rows, so they plan alike; what has to
hold is that the shapes between them take every path."""
from __future__ import annotations

from test_knn_compact_gpu import N, SHAPES, dead_rows
from test_knn_plan_cpu import EMPTY, GENERIC, V1, V3, _plan, plan_lib  # noqa: F401  (plan_lib: fixture)


def test_paths_of_test_knn_compact_gpu(plan_lib):  # noqa: F811
    live = int((~dead_rows()).sum())
    assert 0.45 * N < live < 0.55 * N  # "about half dead"
    want = {
        (512, 300, 10): (V3, 4),    # v3 with four query blocks
        (512, 3, 10): (V3, 1),      # K7s
        (512, 300, 100): (V1, None),
        (384, 300, 50): (V3, None),
        (1, 300, 10): (V3, None),
        (640, 40, 300): (GENERIC, None),
    }
    assert set(want) == set(SHAPES)
    for n in (live, N):  # after and before the compaction
        for (dim, nq, k), (path, qb) in want.items():
            p = _plan(plan_lib, n, nq, k, dim)
            assert p["path"] == path, (n, dim, nq, k, p)
            if qb is not None:
                assert p["qb"] == qb, (n, dim, nq, k, p)
    # between them: both fused kernels, both query blockings, the generic search
    assert _plan(plan_lib, 0, 5, 3, 256)["path"] == EMPTY  # test_all_rows_dead_and_empty_index

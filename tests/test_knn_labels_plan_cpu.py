"""The plan of a kNN search with per-query labels (csrc/knn_plan.h, plan_search's last argument),
compiled for the CPU (scripts/knn_plan_check.cpp): the paths the shapes of
tests/test_knn_labels_gpu.py take, the conditions the kernels rely on over the sweep's grid, and
that nothing about the plan of an unlabelled search depends on the new argument. No GPU."""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multimodal-rag-for-image-text-search_amd", "csrc")

EMPTY, GENERIC, V1, V3 = 0, 1, 2, 3  # SearchPath


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), shutil.which("hipcc"),
                            "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler available")
    so = str(tmp_path_factory.mktemp("knn_plan_labels") / "knn_plan_check.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", f"-I{CSRC}",
                    os.path.join(ROOT, "scripts", "knn_plan_check.cpp"), "-o", so],
                   check=True, capture_output=True, timeout=300)
    lib = ctypes.CDLL(so)
    lib.knn_plan_field_names.restype = ctypes.c_char_p
    lib.knn_plan_condition.restype = ctypes.c_char_p
    lib.knn_plan_fields.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.knn_plan_fields.restype = None
    lib.knn_plan_fields_labels.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p]
    lib.knn_plan_fields_labels.restype = None
    lib.knn_plan_sweep.argtypes = [ctypes.c_void_p]
    lib.knn_plan_sweep.restype = ctypes.c_int64
    lib.knn_plan_sweep_labels.argtypes = [ctypes.c_void_p]
    lib.knn_plan_sweep_labels.restype = ctypes.c_int64
    return lib


def _names(lib):
    return lib.knn_plan_field_names().decode().split(",")


def _plan(lib, n, nq, k, dim):
    """plan_search called without the new argument."""
    names = _names(lib)
    out = np.zeros(len(names), np.int64)
    lib.knn_plan_fields(n, nq, k, (dim + 127) // 128 * 128, out.ctypes.data)
    return dict(zip(names, out.tolist()))


def _plan_labels(lib, n, nq, k, dim, labelled=1):
    names = _names(lib) + ["pql"]
    assert len(names) == 23
    out = np.full(len(names), -7, np.int64)
    lib.knn_plan_fields_labels(n, nq, k, (dim + 127) // 128 * 128, labelled, out.ctypes.data)
    return dict(zip(names, out.tolist()))


# (n, nq, k, dim) of tests/test_knn_labels_gpu.py -> path, qb, sampled, counting (None: the path
# has no such field: v1 and K7g run without a sample pass and without v3's query blocks)
PATHS = [
    # 1. v3, 256-query groups; 313 tiles over 128 or 256 splits: no sample pass
    ((20_000, 300, 10, 128), (V3, 4, 0, 0)),
    ((20_000, 65, 12, 384), (V3, 4, 0, 0)),
    ((20_000, 257, 16, 512), (V3, 4, 0, 0)),
    ((20_000, 130, 50, 256), (V3, 4, 0, 0)),
    # 2. K7s
    *[((20_000, nq, k, dim), (V3, 1, 0, 0)) for dim in (384, 512) for k in (12, 50) for nq in (1, 7, 64)],
    # 3. the sample passes: counting for k = 10, seed-only for k = 32
    ((270_000, 1000, 10, 128), (V3, 4, 1, 1)),
    ((270_000, 1000, 32, 128), (V3, 4, 1, 0)),
    # 4. deep k (v1; K7g where v1's labelled instance does not exist) and wide rows / k above 256 (K7g)
    ((30_000, 40, 100, 100), (V1, None, 0, 0)),
    ((5_000, 40, 100, 256), (V1, None, 0, 0)),
    ((30_000, 40, 100, 384), (GENERIC, None, None, None)),
    ((5_000, 40, 100, 512), (GENERIC, None, None, None)),
    *[((n, 7, 50, dim), (V3, 1, 0, 0)) for n in (40, 130) for dim in (100, 256, 384)],
    ((5_000, 70, 10, 640), (GENERIC, None, None, None)),
    ((5_000, 5, 300, 128), (GENERIC, None, None, None)),
    # 5. the collect cases and 6./7. the edge and concurrency cases
    ((30_000, 48, 10, 512), (V3, 1, 0, 0)),
    ((30_000, 300, 10, 512), (V3, 4, 0, 0)),
    ((30_000, 300, 10, 256), (V3, 4, 0, 0)),
]


@pytest.mark.parametrize("shape,want", PATHS, ids=["-".join(map(str, s)) for s, _ in PATHS])
def test_paths_of_test_knn_labels_gpu(plan_lib, shape, want):
    p = _plan_labels(plan_lib, *shape)
    assert p["pql"] == 1
    for name, w in zip(("path", "qb", "sampled", "counting"), want):
        if w is not None:
            assert p[name] == w, (name, p)
    if want[0] == V1:  # the one v1 depth that has a per-query-label instance at this width
        assert p["KL"] == {128: 32, 256: 16, 384: 16, 512: 8}[(shape[3] + 127) // 128 * 128]


def test_sweep_conditions_hold_for_labelled_plans(plan_lib):
    """The existing sweep's grid and conditions (scripts/knn_plan_check.cpp) over the plans of
    labelled searches (with the K7g routing of deep k at wide rows as its own condition); the
    same number of points as the unlabelled sweep and no larger a K8 LDS figure, since a labelled
    search on the fused path keeps the unlabelled geometry."""
    out = np.zeros(7, np.int64)
    bad = plan_lib.knn_plan_sweep_labels(out.ctypes.data)
    first = (out[2:6].tolist(), plan_lib.knn_plan_condition(int(out[6])).decode()) if bad else None
    assert bad == 0, first
    ref = np.zeros(7, np.int64)
    assert plan_lib.knn_plan_sweep(ref.ctypes.data) == 0
    assert out[0] == ref[0] == 15015
    assert 0 < out[1] <= ref[1]


GRID_N = (0, 1, 63, 64, 65, 4096, 5000, 20_000, 262_144, 270_000, 1 << 20, 1 << 24, 1 << 26)
GRID_NQ = (1, 7, 64, 65, 256, 257, 1000, 4096)
GRID_K = (1, 6, 7, 10, 16, 17, 32, 64, 65, 100, 256, 257)
GRID_DIM = (1, 100, 128, 256, 384, 512, 640)


def test_unlabelled_plans_do_not_change(plan_lib):
    """plan_search without the new argument, with it false, and with it true: the first two agree
    in every field and carry pql = 0. The labelled plan differs from them in pql alone, except
    where the unlabelled search takes v1's top-k scan (k > 64) at a padded width above 256: that
    instance does not fit its registers with a per-lane filter, and the labelled search takes K7g
    (knn_plan.h, PQL_V1_MAX_DP)."""
    names = _names(plan_lib)
    points = rerouted = 0
    for n in GRID_N:
        for nq in GRID_NQ:
            for k in GRID_K:
                for dim in GRID_DIM:
                    base = _plan(plan_lib, n, nq, k, dim)
                    off = _plan_labels(plan_lib, n, nq, k, dim, 0)
                    on = _plan_labels(plan_lib, n, nq, k, dim, 1)
                    assert off["pql"] == 0 and on["pql"] == 1
                    for name in names:
                        assert off[name] == base[name], (name, (n, nq, k, dim))
                    if base["path"] == V1 and (dim + 127) // 128 * 128 > 256:
                        assert (on["path"], on["Qp"]) == (GENERIC, nq), (n, nq, k, dim)
                        rerouted += 1
                    else:
                        for name in names:
                            assert on[name] == base[name], (name, (n, nq, k, dim))
                    points += 1
    assert points == 13 * 8 * 12 * 7
    assert rerouted == 12 * 8 * 3 * 2  # n >= 1, k in (65, 100, 256), dim in (384, 512)


def test_existing_pinned_plan_still_holds(plan_lib):
    """One row of tests/test_knn_plan_cpu.py's table, read through the labelled export with the
    argument false: the flagship shape's plan, field for field."""
    p = _plan_labels(plan_lib, 1 << 20, 1000, 10, 512, 0)
    got = tuple(p[f] for f in ("path", "qb", "Qp", "S", "KL", "stride", "sampled", "sample_tiles", "idbits",
                               "counting", "M", "R", "Mp", "sel", "merge_lds"))
    assert got == (V3, 4, 1024, 64, 8, 16, 1, 16, 6, 1, 42, 1024, 64, 1, 11072)

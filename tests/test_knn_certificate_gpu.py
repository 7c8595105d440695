"""The kNN search on inputs that drive the fp16 score error toward eps, one case
per path of the search plan: K7s, v3 with 256-query groups with and without the counting sample
pass, v1's deep lists, and K7g for wide rows and for deep k (tests/_adversarial.py: GPU_CASES).

Every query is a "down" row. Its k true neighbours are down rows too, so the scan sees them 0.6 to
0.8 eps too low; at least k + 64 "up" rows that are really farther away come out ahead of them.
The weakest true neighbour is then not among the k + 32 rescored candidates, the certificate
cannot hold, and only the eps window of the collect stage (K7c/K10, or K7g's threshold) brings it
back. tests/test_knn_certificate_cpu.py checks those preconditions and the path of each case on a
numpy restatement; here the results must equal the f64 oracle.
"""
from __future__ import annotations

import numpy as np
import pytest

import _adversarial as adv
from oracle.knn import flat_cosine_topk
from test_knn_gpu import _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=sorted(adv.GPU_CASES))
def case(request):
    """The corpus, the query batch and the oracle's answers (computed once per base vector, then
    laid out per query), without and with the label filter."""
    c = adv.gpu_case(request.param)
    D, k, n, nq, nbase, _ = adv.GPU_CASES[request.param]
    q = np.ascontiguousarray(c.q[c.qidx])
    ref = flat_cosine_topk(c.x, np.zeros(n), c.q, k)
    ref_lab = flat_cosine_topk(c.x, c.labels, c.q, k, label_filter=1)
    yield {"name": request.param, "c": c, "q": q, "k": k, "D": D, "fused": not request.param.startswith("k7g"),
           "ref": tuple(a[c.qidx] for a in ref), "ref_lab": tuple(a[c.qidx] for a in ref_lab)}
    adv._BUILT.pop(request.param, None)  # the corpus is not kept for the rest of the run


def test_exact_and_uncertified(cuda, case):
    from app.vector_store import FlatIndex

    c, q, k = case["c"], case["q"], case["k"]
    ix = FlatIndex(case["D"])
    ix.add(c.x, c.labels)
    s, r = ix.search(q, k)
    unc, retries = ix.last_stats()
    bad = int(np.any(r != case["ref"][1], axis=1).sum())
    print(f"{case['name']}: {len(q)} queries, uncertified {unc}, retries {retries}, mismatching queries {bad}")
    _check(s, r, *case["ref"])
    if case["fused"]:
        assert unc >= len(q)  # the proof really failed for every adversarial query
    # a filter that admits the true rows and every other up row
    s, r = ix.search(q, k, label=1)
    _check(s, r, *case["ref_lab"])
    ix.close()


@pytest.mark.parametrize("front", [True, False], ids=["front", "back"])
def test_planted_rows_moved(cuda, case, front):
    """The planted rows at the front of the corpus, then at the back (other tiles, splits and lane
    groups; the first rows are a sampled tile of the counting pass): the same rows after remapping."""
    from app.vector_store import FlatIndex

    c = case["c"]
    perm = adv.planted_first(c, front)
    ix = FlatIndex(case["D"])
    ix.add(c.x[perm])
    s, r = ix.search(case["q"], case["k"])
    assert r.min() >= 0
    _check(s, perm[r], *case["ref"])
    ix.close()

"""A/B of the kNN search with per-query labels (FlatIndex.search with an array for ``label``)
against the two single-label forms it can be compared with. 1M x 512 rows, Q = 1000, k = 10,
queries, filters and outputs in HBM, one process, HIP events on one stream; the row label is
``row % U``.

Per U in --users:
  * ``labelled``: ONE search, query i carrying filter ``i % U``;
  * ``grouped``: the only alternative without per-query labels: one unchanged single-label search
    per distinct filter over its share of the queries (U searches); a step is their sum.
Per U in --mask-users (the cost of the per-query mask alone):
  * ``labelled0``: one labelled search, every query carrying filter 0, kept on the labelled kernels
    (FlatIndex.search itself sends an array of equal filters to the single-label search);
  * ``single0``: ``search(q, k, label=0)`` on the unchanged path.
The two forms of a comparison alternate in blocks of --steps steps over --pairs pairs in one
process; every step is timed by a pair of HIP events on the searches' stream (a search returns
when its device work is done, so the span is the step). The results of both forms are compared
once (rows and f32 scores equal).
One JSON line per (U, form) goes to --out (appended); nothing is printed but those lines.

    python scripts/knn_labels_bench.py --out profiles/knn_labels_ab.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-rag-for-image-text-search_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--users", type=int, nargs="*", default=[1, 4, 16, 64, 1000])
    ap.add_argument("--mask-users", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_labels_ab.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("knn_labels_bench.py needs a GPU")
    from app.vector_store import FlatIndex

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000)
    x = torch.randn((args.rows, args.dim), generator=g, device=dev)
    x = x / x.norm(dim=1, keepdim=True)
    q = torch.randn((args.queries, args.dim), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    rows = torch.arange(args.rows, device=dev, dtype=torch.int32)
    qi = torch.arange(args.queries, device=dev, dtype=torch.int32)
    box = {"gpu": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def ab(forms):
        """forms: {name: fn}; alternating blocks; returns {name: [ms per step]} and the last outputs."""
        ms = {n: [] for n in forms}
        last = {}
        for n, fn in forms.items():
            for _ in range(args.warmup):
                fn()
        for _ in range(args.pairs):
            for n, fn in forms.items():
                for _ in range(args.steps):
                    t, last[n] = timed(fn)
                    ms[n].append(t)
        return ms, last

    def emit(rec, ms):
        a = np.asarray(ms)
        rec.update({"rows": args.rows, "dim": args.dim, "queries": args.queries, "k": args.k, "steps": int(a.size),
                    "pairs": args.pairs, "median_ms": float(np.median(a)), "min_ms": float(a.min()),
                    "p90_ms": float(np.percentile(a, 90)), "mean_ms": float(a.mean()), **box})
        line = json.dumps(rec)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        print(line, flush=True)

    stream = torch.cuda.Stream(device=dev)  # the searches run on it (torch's current stream), the events too
    torch.cuda.synchronize()
    torch.cuda.set_stream(stream)
    for U in sorted(set(args.users) | set(args.mask_users)):
        ix = FlatIndex(args.dim)
        ix.add(x, rows % U)
        if U in args.users:
            filt = (qi % U).contiguous()
            groups = [(int(L), torch.nonzero(filt == L).reshape(-1)) for L in range(min(U, args.queries))]
            groups = [(L, sel, q[sel].contiguous()) for L, sel in groups]

            def labelled():  # FlatIndex.search as a caller sees it (U = 1: equal filters take the single-label search)
                return ix.search(q, args.k, label=filt)

            def grouped():  # the searches alone: putting the rows back in query order is not timed
                return [ix.search(qs, args.k, label=L) for L, _, qs in groups]

            ms, last = ab({"labelled": labelled, "grouped": grouped})
            s = torch.empty((args.queries, args.k), dtype=torch.float32, device=dev)
            r = torch.empty((args.queries, args.k), dtype=torch.int64, device=dev)
            for (_, sel, _), (gs, gr) in zip(groups, last["grouped"]):
                s[sel], r[sel] = gs, gr
            same = bool(torch.equal(last["labelled"][1], r) and torch.equal(last["labelled"][0], s))
            for n in ("labelled", "grouped"):
                emit({"case": "users", "U": U, "form": n, "searches_per_step": 1 if n == "labelled" else len(groups),
                      "results_equal": same}, ms[n])
        if U in args.mask_users:
            zeros = torch.zeros(args.queries, dtype=torch.int32, device=dev)
            ms, last = ab({"labelled0": lambda: ix._search_labels(q, args.k, zeros, 0, False, group_equal=False),
                           "single0": lambda: ix.search(q, args.k, label=0)})
            same = bool(torch.equal(last["labelled0"][1], last["single0"][1]) and
                        torch.equal(last["labelled0"][0], last["single0"][0]))
            for n in ("labelled0", "single0"):
                emit({"case": "mask", "U": U, "form": n, "searches_per_step": 1, "results_equal": same}, ms[n])
        ix.close()


if __name__ == "__main__":
    main()

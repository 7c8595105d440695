"""What diversity costs: ``FlatIndex.search_mmr`` against the fetch search it contains, K16 alone,
and K16 against the copy bandwidth of the rows it gathers. 1M x 512 rows, Q = 1000, k = 10,
fetch_k in --fetch, lam = 0.5; queries, candidates and outputs in HBM, one process, HIP events on
one stream (the protocol of scripts/knn_labels_bench.py).

Per fetch_k:
  * ``search`` (``search(q, fetch_k, with_f64=True)``) and ``search_mmr`` alternate in blocks of
    --steps steps over --pairs pairs; the cost of diversity is the difference of their medians;
  * ``k16``: ``mmr_select`` on the device output of that search;
  * ``copy``: one ``hipMemcpyAsync`` device to device of Q x fetch_k x DP x 4 bytes (what one
    gather of every candidate row once would move), timed the same way in the same process: the
    bandwidth K16's floor is computed with. K16 gathers every unselected candidate once per step,
    so it moves about (k - 1) times that from L2.
One JSON line per (fetch_k, form) goes to --out (appended) with the commit it ran on.

    python scripts/knn_mmr_bench.py --out profiles/knn_mmr.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-rag-for-image-text-search_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def _commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              timeout=10).stdout.strip() or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch", type=int, nargs="*", default=[40, 64, 200])
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit this runs on (default: git rev-parse of the tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_mmr.jsonl"))
    args = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("knn_mmr_bench.py needs a GPU")
    from app.vector_store import FlatIndex

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000)
    x = torch.randn((args.rows, args.dim), generator=g, device=dev)
    x = x / x.norm(dim=1, keepdim=True)
    q = torch.randn((args.queries, args.dim), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    box = {"gpu": torch.cuda.get_device_name(0), "host": platform.node(), "torch": torch.__version__,
           "commit": args.commit or _commit()}
    dp = (args.dim + 127) // 128 * 128

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def ab(forms):
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
        rec.update({"rows": args.rows, "dim": args.dim, "queries": args.queries, "k": args.k, "lam": args.lam,
                    "steps": int(a.size), "pairs": args.pairs, "median_ms": float(np.median(a)),
                    "min_ms": float(a.min()), "p90_ms": float(np.percentile(a, 90)), "mean_ms": float(a.mean()), **box})
        line = json.dumps(rec)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        print(line, flush=True)

    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_stream(stream)
    ix = FlatIndex(args.dim)
    ix.add(x)
    for m in args.fetch:
        ms, last = ab({"search": lambda: ix.search(q, m, with_f64=True),
                       "search_mmr": lambda: ix.search_mmr(q, args.k, fetch_k=m, lam=args.lam, with_f64=True)})
        s, r, s64 = last["search"]
        pos = ix.mmr_select(r, s64, args.k, args.lam).long()
        same = bool(torch.equal(torch.gather(r, 1, pos), last["search_mmr"][1]) and
                    torch.equal(torch.gather(s, 1, pos), last["search_mmr"][0]))
        med = {n: float(np.median(ms[n])) for n in ms}
        for n in ("search", "search_mmr"):
            emit({"case": "diversity", "fetch_k": m, "form": n, "composition_equal": same,
                  "mmr_minus_search_ms": med["search_mmr"] - med["search"]}, ms[n])
        gather_bytes = args.queries * m * dp * 4
        src = torch.empty(gather_bytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ms2, _ = ab({"k16": lambda: ix.mmr_select(r, s64, args.k, args.lam),
                     "copy": lambda: dst.copy_(src)})
        copy_med = float(np.median(ms2["copy"]))
        gbps = gather_bytes / (copy_med * 1e-3) / 1e9
        emit({"case": "k16", "fetch_k": m, "form": "k16", "gather_bytes_once": gather_bytes,
              "floor_ms_one_gather": copy_med, "floor_ms_k_minus_1_gathers": copy_med * (args.k - 1),
              "f64_fma": args.queries * (args.k - 1) * m * args.dim}, ms2["k16"])
        emit({"case": "k16", "fetch_k": m, "form": "copy", "bytes": gather_bytes, "copy_gb_per_s": gbps}, ms2["copy"])
        del src, dst
    ix.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What a compaction costs and what it buys (K15), at 1M x 512 with a random half
of the rows deleted. One JSON line per step into profiles/knn_compact.jsonl (or --out):

  cost    mrag_knn_compact in total (host clock; the call waits for its device work), K15a and
          K15b alone (the HIP events of mrag_knn_compact_profile, and K15a through
          mrag_knn_row_remap), each as bytes read plus written per second; beside them, in the same
          process, hipMemcpyAsync device-to-device of the bytes K15b writes: what grow() does,
          so the yardstick for the gather, with its own spread over the repeats.
  search  the plain search step (Q = 1000, k = 10, queries on the device) on the index before
          compaction, after it, and on a fresh index of the live rows, interleaved round by round;
          medians, and the fresh index's round-to-round spread to read the differences against.

Without --step this is the driver: each step runs in a process of its own under its own
`timeout`, one after the other, and the first failure stops the run.

    python scripts/knn_compact_bench.py [--rows 1048576] [--dim 512] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multimodal-rag-for-image-text-search_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = (("cost", 420), ("search", 420))  # step, its time limit in seconds


def _corpus(torch, rows, dim, dev):
    g = torch.Generator(device=dev).manual_seed(1000)
    x = torch.randn((rows, dim), generator=g, device=dev)
    x = x / x.norm(dim=1, keepdim=True)
    dead = torch.rand((rows,), generator=g, device=dev) < 0.5
    return x, dead


def _build(FlatIndex, x, dead_ids=None):
    ix = FlatIndex(x.shape[1])
    ix.add(x)
    if dead_ids is not None:
        ix.delete(dead_ids)
    return ix


def _hip_memcpy_async():
    """hipMemcpyAsync of the HIP runtime this process already has loaded (torch's), or None."""
    paths = []
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if "libamdhip64" in os.path.basename(path) and path not in paths:
                paths.append(path)
    for name in paths:
        try:
            fn = ctypes.CDLL(name).hipMemcpyAsync
        except (OSError, AttributeError):
            continue
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        return fn
    return None


def _spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def step_cost(args):
    import torch

    from app import _native
    from app.vector_store import FlatIndex

    dev = torch.device("cuda", 0)
    x, dead = _corpus(torch, args.rows, args.dim, dev)
    dead_ids = torch.nonzero(dead).flatten().cpu().numpy()
    live = args.rows - dead_ids.size
    total_ms, a_ms, b_ms = [], [], []
    a_bytes = b_bytes = 0
    for _ in range(args.repeats + 1):  # the first is the warm-up (code objects, first allocations)
        ix = _build(FlatIndex, x, dead_ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        remap = ix.compact()
        total_ms.append((time.perf_counter() - t0) * 1e3)
        ka, kb, a_bytes, b_bytes = ix.compact_profile()
        a_ms.append(ka)
        b_ms.append(kb)
        assert len(ix) == live and int((remap >= 0).sum()) == live
        ix.close()
    total_ms, a_ms, b_ms = total_ms[1:], a_ms[1:], b_ms[1:]

    # K15a alone through its entry point (the call allocates its block sums and waits: upper bound)
    lab = torch.zeros((args.rows,), dtype=torch.int32, device=dev)
    lab[dead] = -2
    out = torch.empty_like(lab)
    n_live = ctypes.c_int64(0)
    remap_ms = []
    for _ in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _native.call("mrag_knn_row_remap", lab.data_ptr(), args.rows, out.data_ptr(), ctypes.byref(n_live), None)
        remap_ms.append((time.perf_counter() - t0) * 1e3)
    remap_ms = remap_ms[1:]
    assert n_live.value == live

    # the yardstick: one device-to-device copy of the bytes K15b writes (its read + write = b_bytes)
    copy_bytes = live * (6 * ((args.dim + 127) // 128 * 128) + 12)  # x16 + x32 rows, norm and label of every live row
    src = torch.empty((copy_bytes,), dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    memcpy = _hip_memcpy_async()
    stream = torch.cuda.current_stream(dev)
    copy_ms = []
    for _ in range(args.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        if memcpy is not None:
            rc = memcpy(dst.data_ptr(), src.data_ptr(), copy_bytes, 3, stream.cuda_stream)  # 3: device to device
            if rc != 0:
                raise RuntimeError(f"hipMemcpyAsync returned {rc}")
        else:
            dst.copy_(src)
        e1.record(stream)
        e1.synchronize()
        copy_ms.append(e0.elapsed_time(e1))
    copy_ms = copy_ms[1:]
    assert torch.equal(dst[:4096], src[:4096])

    def rate(nbytes, ms):  # GB/s of every repeat
        return _spread([nbytes / (m * 1e-3) / 1e9 for m in ms])

    return {
        "step": "cost", "rows": args.rows, "dim": args.dim, "live": live, "repeats": args.repeats,
        "compact_total_ms": _spread(total_ms),
        "k15a_ms": _spread(a_ms), "k15a_bytes": a_bytes, "k15a_GBps": rate(a_bytes, a_ms),
        "k15a_entry_point_ms": _spread(remap_ms),
        "k15b_ms": _spread(b_ms), "k15b_bytes": b_bytes, "k15b_GBps": rate(b_bytes, b_ms),
        "copy_api": "hipMemcpyAsync" if memcpy is not None else "torch.Tensor.copy_",
        "copy_ms": _spread(copy_ms), "copy_bytes_read_plus_written": 2 * copy_bytes,
        "copy_GBps": rate(2 * copy_bytes, copy_ms),
        "note": "GBps: bytes read plus written over the time of each repeat",
    }


def step_search(args):
    import torch

    from app.vector_store import FlatIndex

    dev = torch.device("cuda", 0)
    x, dead = _corpus(torch, args.rows, args.dim, dev)
    dead_ids = torch.nonzero(dead).flatten().cpu().numpy()
    idx = {"before": _build(FlatIndex, x, dead_ids), "after": _build(FlatIndex, x, dead_ids),
           "fresh": _build(FlatIndex, x[~dead].contiguous())}
    remap = idx["after"].compact()
    del x
    torch.cuda.empty_cache()
    q = torch.randn((args.queries, args.dim), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    ref = {}
    for name, ix in idx.items():  # warm-up, and the answers
        for _ in range(3):
            ref[name] = ix.search(q, args.k)
    remap_t = torch.from_numpy(remap).to(dev)
    assert torch.equal(remap_t[ref["before"][1]], ref["after"][1]) and torch.equal(ref["before"][0], ref["after"][0])
    assert torch.equal(ref["after"][1], ref["fresh"][1]) and torch.equal(ref["after"][0], ref["fresh"][0])
    ms = {name: [] for name in idx}
    order = list(idx)
    for rnd in range(args.rounds):
        for name in order[rnd % 3:] + order[:rnd % 3]:  # interleaved, the order rotating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.searches):
                idx[name].search(q, args.k)  # returns once its device work is done
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.searches)
    med = {name: statistics.median(v) for name, v in ms.items()}
    fresh_spread = max(ms["fresh"]) - min(ms["fresh"])
    return {
        "step": "search", "rows": args.rows, "dim": args.dim, "live": int(len(idx["fresh"])), "queries": args.queries,
        "k": args.k, "rounds": args.rounds, "searches_per_round": args.searches,
        "ms_per_search": {name: _spread(v) for name, v in ms.items()}, "rounds_ms": ms,
        "fresh_round_to_round_spread_ms": fresh_spread,
        "after_minus_fresh_ms": med["after"] - med["fresh"],
        "before_minus_after_ms": med["before"] - med["after"],
        "before_minus_fresh_ms": med["before"] - med["fresh"],
        "after_within_fresh_spread": abs(med["after"] - med["fresh"]) <= fresh_spread,
        "after_and_fresh_faster_than_before_by_more_than_spread":
            min(med["before"] - med["after"], med["before"] - med["fresh"]) > fresh_spread,
        "answers": "before == after (through the remap) == fresh, rows and f32 scores",
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=[s for s, _ in STEPS], default=None)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7, help="cost step: timed repeats after one warm-up")
    ap.add_argument("--rounds", type=int, default=7, help="search step: interleaved rounds (at least five)")
    ap.add_argument("--searches", type=int, default=20, help="search step: searches per index and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_compact.jsonl"))
    args = ap.parse_args()
    if args.step is None:
        if os.path.exists(args.out):
            os.unlink(args.out)
        passed = [f"--{k}={getattr(args, k)}" for k in ("rows", "dim", "queries", "k", "repeats", "rounds", "searches")]
        for step, limit in STEPS:
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--out", args.out] + passed
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                print(f"step {step} failed with status {rc}: stopping", file=sys.stderr)
                sys.exit(rc)
        return
    if args.rounds < 5:
        ap.error("--rounds must be at least 5")
    rec = step_cost(args) if args.step == "cost" else step_search(args)
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()

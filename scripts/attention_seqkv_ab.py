#!/usr/bin/env python3
"""K4 A/B: attention alone, flash16 against seqkv forced through ``kernel=``, in one process,
timed with HIP events, interleaved flash16 / seqkv in pairs, at the towers' shapes:

    B 256  L 197  H 12  dh 64   ViT-B/16
    B 128  L 257  H 16  dh 64   ViT-L/14
    B 1000 L 77   H 8   dh 64   CLIP text (causal, ragged padding mask)
    B 256  L 256  H 12  dh 32   MiniLM (ragged padding mask; and without a mask)

One JSON line per (shape, pair) and a summary line per shape:
``win`` is true when seqkv is faster in every pair by more than the spread (max - min) of either
kernel's own times over the pairs. usage: attention_seqkv_ab.py [pairs=7] [launches=50] [out.jsonl]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multimodal-rag-for-image-text-search_amd"), ROOT]

import torch  # noqa: E402

from app.encoders import attention  # noqa: E402

SHAPES = [
    ("vit_b16", 256, 197, 12, 64, False, "none"),
    ("vit_l14", 128, 257, 16, 64, False, "none"),
    ("clip_text", 1000, 77, 8, 64, True, "ragged"),
    ("minilm", 256, 256, 12, 32, False, "ragged"),
    ("minilm_nomask", 256, 256, 12, 32, False, "none"),
]


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    for name, B, L, H, DH, causal, mk in SHAPES:
        g = torch.Generator(device=dev).manual_seed(L)
        qkv = (torch.randn((B * L, 3 * H * DH), generator=g, device=dev) * 0.5).half()
        mask = None
        if mk == "ragged":  # sequence lengths uniform in [L / 4, L]
            n = torch.randint(L // 4, L + 1, (B,), generator=g, device=dev)
            mask = (torch.arange(L, device=dev)[None, :] < n[:, None]).int().contiguous()
        outs = {k: torch.empty((B * L, H * DH), dtype=torch.float16, device=dev) for k in ("flash16", "seqkv")}

        def run(k, n):
            for _ in range(n):
                attention(qkv, outs[k], B, L, H, DH, mask=mask, causal=causal, kernel=k)

        for k in outs:
            run(k, 5)
        torch.cuda.synchronize()
        same = torch.equal(outs["flash16"].view(torch.int16), outs["seqkv"].view(torch.int16))
        t = {"flash16": [], "seqkv": []}
        for p in range(pairs):
            for k in ("flash16", "seqkv"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(k, launches)
                e1.record()
                e1.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / launches)
            emit({"shape": name, "B": B, "L": L, "H": H, "dh": DH, "causal": causal, "mask": mk, "pair": p,
                  "flash16_us": round(t["flash16"][-1], 2), "seqkv_us": round(t["seqkv"][-1], 2)})
        spread = max(max(v) - min(v) for v in t.values())
        win = all(f - s > spread for f, s in zip(t["flash16"], t["seqkv"]))
        emit({"shape": name, "summary": True, "same_bytes": same, "launches_per_time": launches,
              "flash16_us_min_max": [round(min(t["flash16"]), 2), round(max(t["flash16"]), 2)],
              "seqkv_us_min_max": [round(min(t["seqkv"]), 2), round(max(t["seqkv"]), 2)],
              "spread_us": round(spread, 2), "win": win,
              "ratio_flash16_over_seqkv": round(sum(t["flash16"]) / sum(t["seqkv"]), 3)})
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

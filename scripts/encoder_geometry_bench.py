#!/usr/bin/env python3
"""Image-tower throughput per CLIP geometry: batch-256 synthetic-weight images per second for
ViT-B/32, ViT-B/16 and ViT-L/14, one batch at a time and three in flight (bench_clip_images), with
the algorithmic FLOP per image (vit_flops_per_image) and the fraction of the 2.5 PFLOP/s fp16 MFMA
peak. One JSON line per geometry. usage: encoder_geometry_bench.py [steps=10] [out.jsonl]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multimodal-rag-for-image-text-search_amd"), ROOT]

from app.encoders import (CLIP_VISION_B16, CLIP_VISION_B32, CLIP_VISION_L14, bench_clip_images,  # noqa: E402
                          vit_flops_per_image)

PEAK_TFLOPS = 2500.0


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    lines = []
    for name, cfg in (("ViT-B/32", CLIP_VISION_B32), ("ViT-B/16", CLIP_VISION_B16), ("ViT-L/14", CLIP_VISION_L14)):
        flop = vit_flops_per_image(cfg)
        row = {"geometry": name, "tokens": (cfg.image_size // cfg.patch_size) ** 2 + 1, "batch": 256, "steps": steps,
               "gflop_per_image": round(flop / 1e9, 2)}
        for key, inflight in (("one_at_a_time", 1), ("three_in_flight", 3)):
            r = bench_clip_images(steps=steps, warmup=3, batch=256, inflight=inflight, cfg=cfg)
            row[key] = {"images_per_s": r["value"], "ms_per_batch": r["ms_per_batch"],
                        "tflops": round(flop * r["value"] / 1e12, 1),
                        "frac_of_peak": round(flop * r["value"] / 1e12 / PEAK_TFLOPS, 4)}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

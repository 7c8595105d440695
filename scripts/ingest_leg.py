"""The bench's embed_images_batch-from-files leg alone (bench.ingest_leg, part of bench.py --full):
prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "multimodal-rag-for-image-text-search_amd"), ROOT]
import bench  # noqa: E402

index_image, ingest = bench.ingest_leg()
print(json.dumps({"ingest_embed_images_batch": ingest, "index_image_nodes": index_image}), flush=True)

"""The batched retrieval layer with one user per query (app.retrieval.search_batch /
retrieve_batch with a sequence for ``user_id``): a multi-user batch is one flat-index launch per
modality, and result i equals the single-user call for (user_i, query_i)."""
from __future__ import annotations

import numpy as np
import pytest
from PIL import Image

from _data import unit_rows

pytestmark = pytest.mark.gpu


def _patch_stores(monkeypatch, tmp_path, name):
    from app.cache import clear_all_caches
    from app.ml import index_build, retrieve
    from app.storage.lancedb_store import LanceDBStore
    from app.storage.schema import MetadataStore

    store = LanceDBStore(str(tmp_path / name))
    meta = MetadataStore(str(tmp_path / name / "metadata.sqlite3"))
    monkeypatch.setattr(index_build, "_LANCEDB_STORE", store)
    monkeypatch.setattr(index_build, "_VERSION_FILE", tmp_path / "versions.json")
    monkeypatch.setattr(retrieve, "_LANCEDB_STORE", store)
    monkeypatch.setattr(retrieve, "_METADATA_STORE", meta)
    monkeypatch.setattr(retrieve, "get_index_version", index_build.get_index_version)
    clear_all_caches()
    return store, meta


def test_search_batch_one_user_per_query(cuda, tmp_path, monkeypatch):
    from app.retrieval import search_batch
    from app.storage.lancedb_store import VectorRow

    store, _ = _patch_stores(monkeypatch, tmp_path, "db_users")
    users = ["ann", "ben", "cy"]
    rng = np.random.default_rng(0)
    tx = unit_rows(900, 384, 1)
    ix = unit_rows(300, 512, 2)
    tu = rng.integers(0, 3, len(tx))
    iu = rng.integers(0, 3, len(ix))
    store.upsert_text_vectors([VectorRow(chunk_id=f"t{i}", user_id=users[tu[i]], document_id="d", modality="text",
                                         embedding=tx[i].tolist(), meta={"i": i}) for i in range(len(tx))])
    store.upsert_image_vectors([VectorRow(chunk_id=f"i{i}", user_id=users[iu[i]], document_id="d", modality="image",
                                          embedding=ix[i].tolist(), meta={"i": i}) for i in range(len(ix))])
    who = ["ann", "ben", "cy", "nobody", "ann"]
    for modality, dim in (("text", 384), ("image", 512)):
        vecs = unit_rows(5, dim, 3 + dim)
        got = search_batch(modality, who, vecs, 5)
        assert len(got) == 5
        for i, u in enumerate(who):
            assert got[i] == search_batch(modality, u, vecs[i:i + 1], 5)[0]  # dict for dict
        assert got[3] == [] and all(len(got[i]) == 5 for i in (0, 1, 2, 4))
        with pytest.raises(ValueError):
            search_batch(modality, who[:4], vecs, 5)
        assert search_batch(modality, "ann", vecs, 5) == [search_batch(modality, "ann", vecs[i:i + 1], 5)[0]
                                                          for i in range(5)]
    # a tuple of users is a sequence too; users nobody has seen alone give empty lists
    assert search_batch("text", ("nobody", "nobody2"), unit_rows(2, 384, 9), 3) == [[], []]


def test_retrieve_batch_one_user_per_query(cuda, tmp_path, monkeypatch):
    from app.ml import index_build
    from app.retrieval import retrieve_batch
    from app.storage.schema import Chunk

    _, meta = _patch_stores(monkeypatch, tmp_path, "db_retrieve")
    rng = np.random.default_rng(1)
    words = [f"w{i}" for i in range(200)]
    chunks = []
    for user, docs in (("ann", range(0, 3)), ("ben", range(3, 5))):
        nodes = [{"id": f"doc{d}", "text": " ".join(" ".join(rng.choice(words, 12)) + "." for _ in range(30)),
                  "metadata": {"source": "pdf", "page_no": d}} for d in docs]
        chunks += index_build.index_text_nodes(user, nodes)
    meta.upsert_chunks([Chunk(id=s["chunk_id"], document_id=s["metadata"]["doc_id"], modality="text", text=s["text"],
                              meta=s["metadata"]) for s in chunks])
    ipaths = []
    for i in range(4):
        p = tmp_path / f"im{i}.png"
        Image.fromarray(rng.integers(0, 256, (64 + 8 * i, 72, 3), dtype=np.uint8)).save(p)
        ipaths.append(p)
    for user, sel in (("ann", (0, 1, 2)), ("ben", (3,))):
        index_build.index_image_nodes(user, [{"id": f"img{i}", "metadata": {"file_path": str(ipaths[i]),
                                                                            "doc_id": "docimg"}} for i in sel])
    meta.upsert_chunks([Chunk(id=f"img{i}", document_id="docimg", modality="image", file_path=str(p))
                        for i, p in enumerate(ipaths)])
    qa, qb = "w1 w2 w3 w4", "w150 w12 w7"
    both = retrieve_batch(["ann", "ben"], [qa, qb], rerank=False)
    one_a = retrieve_batch("ann", [qa], rerank=False)[0]
    one_b = retrieve_batch("ben", [qb], rerank=False)[0]
    assert both == [one_a, one_b]
    assert one_a and one_b and {x["chunk_id"] for x in one_a}.isdisjoint(x["chunk_id"] for x in one_b)
    swapped = retrieve_batch(["ben", "ann"], [qa, qb], rerank=False)
    assert swapped[0] == retrieve_batch("ben", [qa], rerank=False)[0]
    with pytest.raises(ValueError):
        retrieve_batch(["ann"], [qa, qb], rerank=False)

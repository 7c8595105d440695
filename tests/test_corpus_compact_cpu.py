"""Compaction of the on-disk corpus format (app.storage.corpus_files): the live rows and payloads
rewritten in order as the next generation, the manifest replace as the commit point, crashes on
either side of it, and other CorpusFiles objects (other processes) on the same directory."""
from __future__ import annotations

import json
import os
import shutil

import numpy as np
import pytest


def _rows(ids, user="u1"):
    return [{"chunk_id": c, "user_id": user, "document_id": "d" + c, "modality": "text", "meta": json.dumps({"i": c})}
            for c in ids]


def _table(d, dim=8):
    """Three appends, 10 rows, rows 1, 4 and 7 deleted by the later ones: (files, vectors)."""
    from app.storage.corpus_files import CorpusFiles

    rng = np.random.default_rng(0)
    v = rng.standard_normal((10, dim)).astype(np.float32)
    f = CorpusFiles(d)
    with f.write_lock():
        f.append(v[:5], _rows(list("abcde")))
    with f.write_lock():
        f.append(v[5:8], _rows(["b", "f", "g"], user="u2"), dead=[1])
    with f.write_lock():
        f.append(v[8:], _rows(["e", "g"], user="u3"), dead=[4, 7])
    return f, v


LIVE = [0, 2, 3, 5, 6, 8, 9]
LIVE_IDS = ["a", "c", "d", "b", "f", "e", "g"]
LIVE_USERS = ["u1", "u1", "u1", "u2", "u2", "u3", "u3"]


def _read(files):
    segs = list(files.segments())
    vec = np.concatenate([np.asarray(s.vectors) for s in segs]) if segs else np.zeros((0, files.dim or 0), np.float32)
    cols = {c: sum((s.rows[c] for s in segs), []) for c in ("chunk_id", "user_id", "document_id", "meta")}
    return vec, cols


def _check_compacted(files, v, generation=1):
    assert files.generation == generation and files.manifest["generation"] == generation
    assert files.manifest["tombstones"] == 0 and files.tombstones().size == 0
    assert files.num_rows == len(LIVE) and files.dim == v.shape[1]
    vec, cols = _read(files)
    np.testing.assert_array_equal(vec, v[LIVE])
    assert cols["chunk_id"] == LIVE_IDS and cols["user_id"] == LIVE_USERS
    assert cols["document_id"] == ["d" + c for c in LIVE_IDS]
    assert cols["meta"] == [json.dumps({"i": c}) for c in LIVE_IDS]


@pytest.mark.parametrize("how", ["tombstones", "mask", "remap"])
def test_compact_and_reopen(tmp_path, how):
    from app.storage.corpus_files import CorpusFiles

    d = str(tmp_path / "t")
    f, v = _table(d)
    assert f.generation == 0 and f.tombstones().tolist() == [1, 4, 7]
    mask = np.zeros(10, bool)
    mask[LIVE] = True
    remap = np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int64)
    with f.write_lock():
        gen = f.compact({"tombstones": None, "mask": mask, "remap": remap}[how])
    assert gen == 1
    _check_compacted(f, v)
    _check_compacted(CorpusFiles(d), v)  # a new process's view
    names = sorted(n for n in os.listdir(d) if not n.startswith("."))
    assert names == ["gen000001_seg_000000.f32", "gen000001_seg_000000.parquet", "manifest.json"]
    with pytest.raises(ValueError):
        f.compact(np.ones(3, bool))


def test_compact_streams_into_several_segments(tmp_path):
    from app.storage.corpus_files import CorpusFiles

    d = str(tmp_path / "t")
    f, v = _table(d)
    f.SEGMENT_ROWS, f.COPY_ROWS = 3, 2  # 7 live rows -> segments of 3, 3 and 1, copied 2 rows at a time
    with f.write_lock():
        f.compact()
    assert [s["rows"] for s in f.manifest["segments"]] == [3, 3, 1]
    _check_compacted(CorpusFiles(d), v)


def test_directory_without_generation_key_is_generation_0(tmp_path):
    from app.storage.corpus_files import CorpusFiles

    d = str(tmp_path / "t")
    f, v = _table(d)
    m = json.load(open(f.manifest_path))
    assert "generation" not in m  # what every directory written before compaction existed holds
    assert sorted(s["name"] for s in m["segments"]) == ["seg_000000", "seg_000001", "seg_000002"]
    assert os.path.exists(os.path.join(d, "tombstones.i64"))
    g = CorpusFiles(d)
    assert g.generation == 0 and g.num_rows == 10 and g.tombstones().tolist() == [1, 4, 7]
    np.testing.assert_array_equal(_read(g)[0], v)


def test_append_after_compaction_has_generation_names(tmp_path):
    from app.storage.corpus_files import CorpusFiles

    d = str(tmp_path / "t")
    f, v = _table(d)
    with f.write_lock():
        f.compact()
    w = np.full((2, 8), 3, np.float32)
    with f.write_lock():
        f.append(w, _rows(["a", "z"], user="u4"), dead=[0])  # row 0 of the compacted order ("a")
    assert [s["name"] for s in f.manifest["segments"]] == ["gen000001_seg_000000", "gen000001_seg_000001"]
    assert os.path.exists(os.path.join(d, "gen000001_tombstones.i64"))
    assert not os.path.exists(os.path.join(d, "tombstones.i64"))
    g = CorpusFiles(d)
    assert g.generation == 1 and g.num_rows == 9 and g.tombstones().tolist() == [0]
    vec, cols = _read(g)
    np.testing.assert_array_equal(vec, np.concatenate([v[LIVE], w]))
    assert cols["chunk_id"] == LIVE_IDS + ["a", "z"]


def test_crash_before_the_commit_keeps_the_old_table(tmp_path):
    """New-generation files on disk, old manifest: the old table with its tombstones."""
    from app.storage.corpus_files import CorpusFiles

    d = str(tmp_path / "t")
    f, v = _table(d)
    old_manifest = open(f.manifest_path, "rb").read()
    keep = str(tmp_path / "old")
    shutil.copytree(d, keep)
    with f.write_lock():
        f.compact()
    # put back everything the compaction removed, and the old manifest over the new one
    for name in os.listdir(keep):
        if not os.path.exists(os.path.join(d, name)):
            shutil.copy(os.path.join(keep, name), os.path.join(d, name))
    with open(f.manifest_path, "wb") as h:
        h.write(old_manifest)
    assert os.path.exists(os.path.join(d, "gen000001_seg_000000.f32"))
    g = CorpusFiles(d)
    assert g.generation == 0 and g.num_rows == 10 and g.tombstones().tolist() == [1, 4, 7]
    np.testing.assert_array_equal(_read(g)[0], v)
    with g.write_lock():  # the next writer removes the strays, and its append is a generation-0 one
        assert not [n for n in os.listdir(d) if n.startswith("gen")]
        g.append(np.zeros((1, 8), np.float32), _rows(["q"]))
    assert g.manifest["segments"][-1]["name"] == "seg_000003"
    assert CorpusFiles(d).num_rows == 11


def test_crash_after_the_commit_keeps_the_new_table(tmp_path):
    """Old files left behind, new manifest: the new table; the next write_lock removes the strays."""
    from app.storage.corpus_files import CorpusFiles

    d = str(tmp_path / "t")
    f, v = _table(d)
    keep = str(tmp_path / "old")
    shutil.copytree(d, keep)
    with f.write_lock():
        f.compact()
    strays = [n for n in os.listdir(keep) if n.startswith("seg_") or n == "tombstones.i64"]
    assert len(strays) == 7
    for name in strays:
        assert not os.path.exists(os.path.join(d, name))  # the compaction removed them ...
        shutil.copy(os.path.join(keep, name), os.path.join(d, name))  # ... a crashed one would not have
    g = CorpusFiles(d)
    _check_compacted(g, v)
    with g.write_lock():
        pass
    assert not [n for n in strays if os.path.exists(os.path.join(d, n))]
    _check_compacted(CorpusFiles(d), v)


def test_second_compaction(tmp_path):
    from app.storage.corpus_files import CorpusFiles

    d = str(tmp_path / "t")
    f, v = _table(d)
    with f.write_lock():
        f.compact()
    w = np.full((2, 8), 3, np.float32)
    with f.write_lock():
        f.append(w, _rows(["c", "z"], user="u4"), dead=[1])  # "c" is row 1 now
    with f.write_lock():
        assert f.compact() == 2
    g = CorpusFiles(d)
    assert g.generation == 2 and g.manifest["tombstones"] == 0 and g.num_rows == 8
    vec, cols = _read(g)
    np.testing.assert_array_equal(vec, np.concatenate([v[[0, 3, 5, 6, 8, 9]], w]))
    assert cols["chunk_id"] == ["a", "d", "b", "f", "e", "g", "c", "z"]
    names = sorted(n for n in os.listdir(d) if not n.startswith("."))
    assert names == ["gen000002_seg_000000.f32", "gen000002_seg_000000.parquet", "manifest.json"]


def test_all_rows_dead(tmp_path):
    from app.storage.corpus_files import CorpusFiles

    d = str(tmp_path / "t")
    f, v = _table(d)
    with f.write_lock():
        f.compact(np.zeros(10, bool))
    g = CorpusFiles(d)
    assert g.generation == 1 and g.num_rows == 0 and g.dim == 8 and list(g.segments()) == []
    with g.write_lock():
        g.append(v[:2], _rows(["a", "b"]))
    assert CorpusFiles(d).num_rows == 2


def test_object_opened_before_sees_the_new_table_after_refresh(tmp_path):
    from app.storage.corpus_files import CorpusFiles

    d = str(tmp_path / "t")
    f, v = _table(d)
    other = CorpusFiles(d)  # another process, opened before the compaction
    assert other.generation == 0 and other.num_rows == 10
    with f.write_lock():
        f.compact()
    assert other.generation == 0  # still the manifest it read
    with pytest.raises(FileNotFoundError):
        list(other.segments())  # its files are gone: callers refresh and read again (_Table._sync)
    assert other.refresh() is True
    _check_compacted(other, v)
    assert other.refresh() is False

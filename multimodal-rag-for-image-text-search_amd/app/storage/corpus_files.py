"""On-disk corpus format: the persistence half of the Lance tables the reference keeps in
``LANCEDB_DIR`` (app/storage/lancedb_store.py:33-44 schema, :87-101 upsert = per-row
``delete(chunk_id == ...)`` then ``add``). SURVEY.md §8f row 2.

One directory per table (``<db>/mrag_tables/<table>/``), append-only between compactions:

* ``seg_<k>.f32``      — the segment's rows, fp32 ``[n][dim]`` little-endian, exactly the
                         (re-normalised) vectors the reference would write to Lance;
* ``seg_<k>.parquet``  — the row payloads: chunk_id, user_id, document_id, modality, meta
                         (JSON text), one Arrow row per vector row, same order;
* ``tombstones.i64``   — int64 global row ids deleted by later upserts (append-only);
* ``manifest.json``    — ``{"dim", "generation": g, "segments": [{"name", "rows"}],
                         "tombstones": n}``, replaced atomically (write + fsync +
                         ``os.replace``) after the segment / tombstone bytes are durable, so a
                         crash leaves either the old or the new table, never a torn one. A
                         manifest without ``generation`` is generation 0.

Compaction (``CorpusFiles.compact``, the on-disk half of ``LanceDBStore.optimize``) rewrites the
live rows, in order, as generation g + 1: it streams the old segments memmap by memmap into
``gen<g+1>_seg_<k>.f32`` / ``.parquet`` (at most ``SEGMENT_ROWS`` rows each), fsyncs them and
replaces the manifest with ``{"dim", "generation": g + 1, "segments": [...], "tombstones": 0}``;
that replace is the commit point. Files of a generation g > 0 carry it in their names
(``gen<g>_seg_<k>.*`` for the compacted segments and for later appends,
``gen<g>_tombstones.i64``); generation 0 keeps the plain names above. A leftover of another
generation can therefore never be taken for a listed file or overwritten by one: a crash before
the replace leaves the old table (tombstones included) and stray new files that nothing reads, a
crash after it the new table and stray old files; the next writer removes both kinds under the
lock. Row ids after a compaction are the compacted order, in every process: a process that
replayed generation g drops its copy and replays g + 1 from the start when it sees the new
manifest, and one that finds a listed file gone (it read the manifest a moment before the
compaction removed the file) refreshes and reads again.

Global row ids are the concatenation order of the segments, i.e. the GPU index's row ids,
so a reopened table returns the same rows in the same tie order (score desc, row asc).
Readers replay only the segments and tombstones the manifest lists.

Several processes share one directory (the reference's Celery worker indexes while the API
process searches, app/tasks.py:108,165 and api/routes.py:276, both on LANCEDB_DIR): writers
serialise on an exclusive ``fcntl`` lock of ``<dir>/.lock`` and re-read the manifest under
it before appending, so segment names and tombstone offsets never collide; readers need no
lock (the manifest is replaced atomically and lists only durable, immutable bytes) and pick
up other processes' commits with ``refresh()`` (a stat of the manifest per call).
"""
from __future__ import annotations

import contextlib
import fcntl
import json
import os
import re
from dataclasses import dataclass
from typing import Any, Dict, Iterator, List, Optional, Sequence

import numpy as np

COLUMNS = ("chunk_id", "user_id", "document_id", "modality", "meta")

# the table's own data files: (generation prefix)? seg_<k>.f32 / .parquet (+ .tmp) and tombstones.i64
_DATA_FILE = re.compile(r"^(?:gen(\d+)_)?(?:seg_\d+\.(?:f32|parquet)(?:\.tmp)?|tombstones\.i64)$")


def _prefix(generation: int) -> str:
    return f"gen{generation:06d}_" if generation > 0 else ""


def _fsync_write(path: str, data) -> None:
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(data)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


@dataclass
class Segment:
    vectors: np.ndarray          # f32 [n, dim] (memory-mapped)
    rows: Dict[str, List[Any]]   # column -> values


class CorpusFiles:
    """Append-only segment files of one table (rewritten by ``compact``)."""

    SEGMENT_ROWS = 1 << 20   # rows per segment that ``compact`` writes
    COPY_ROWS = 1 << 16      # rows it holds in memory at a time

    def __init__(self, directory: str):
        self.dir = directory
        self.manifest_path = os.path.join(directory, "manifest.json")
        self.manifest: Dict[str, Any] = {"dim": None, "segments": [], "tombstones": 0}
        self._stamp = None
        self._stages_checked = False
        self._strays_checked = None  # generation whose strays were last removed by this object
        self.refresh()

    def refresh(self) -> bool:
        """Re-read the manifest if another process committed since the last read (True if so)."""
        try:
            st = os.stat(self.manifest_path)
        except FileNotFoundError:
            return False
        stamp = (st.st_ino, st.st_mtime_ns, st.st_size)
        if stamp == self._stamp:
            return False
        with open(self.manifest_path) as f:
            self.manifest = json.load(f)
        self._stamp = stamp
        return True

    @contextlib.contextmanager
    def write_lock(self):
        """Exclusive inter-process writer lock; the manifest is fresh inside it."""
        os.makedirs(self.dir, exist_ok=True)
        fd = os.open(os.path.join(self.dir, ".lock"), os.O_RDWR | os.O_CREAT, 0o644)
        try:
            fcntl.flock(fd, fcntl.LOCK_EX)
            self.refresh()
            if not self._stages_checked:  # once per process and table: a listdir of the segments
                self._stages_checked = True
                self._drop_stale_stages()
            if self._strays_checked != self.generation:  # once per generation seen: another listdir
                self._drop_other_generations()
            yield self
        finally:
            fcntl.flock(fd, fcntl.LOCK_UN)
            os.close(fd)

    STALE_STAGE_S = 24 * 3600  # a staged Parquet this old belonged to a writer that died

    def _drop_stale_stages(self) -> None:
        """Remove ``stage_rows`` files a crashed writer left (never listed by a manifest); a live
        writer's staged file is younger than any index call (it is written while that call's
        images embed and renamed at its commit)."""
        import time

        now = time.time()
        with contextlib.suppress(OSError):
            for name in os.listdir(self.dir):
                if name.startswith(".stage_") and name.endswith(".parquet"):
                    path = os.path.join(self.dir, name)
                    with contextlib.suppress(OSError):
                        if now - os.stat(path).st_mtime > self.STALE_STAGE_S:
                            os.unlink(path)

    def _drop_other_generations(self) -> None:
        """Under the writer lock: remove the data files of any generation but the manifest's, i.e.
        what a compaction (finished, or crashed before its commit) left behind. No writer is
        active, so nothing lists or is about to list them."""
        g = self.generation
        with contextlib.suppress(OSError):
            for name in os.listdir(self.dir):
                m = _DATA_FILE.match(name)
                if m and int(m.group(1) or 0) != g:
                    with contextlib.suppress(OSError):
                        os.unlink(os.path.join(self.dir, name))
        self._strays_checked = g

    @property
    def dim(self) -> Optional[int]:
        return self.manifest["dim"]

    @property
    def generation(self) -> int:
        """Number of compactions the table has been through (0 for a manifest without the key)."""
        return int(self.manifest.get("generation", 0))

    def _tombstone_path(self, generation: Optional[int] = None) -> str:
        g = self.generation if generation is None else generation
        return os.path.join(self.dir, _prefix(g) + "tombstones.i64")

    @property
    def num_rows(self) -> int:
        return sum(s["rows"] for s in self.manifest["segments"])

    def stage_rows(self, rows: Sequence[Dict[str, Any]]) -> str:
        """The payload Parquet of an upcoming ``append``, written and fsynced ahead of it under a
        unique staging name in the table directory (index_image_nodes writes it while its images
        embed); ``append(..., staged=path)`` renames it into place. Not listed by any manifest
        until then; ``discard_staged`` removes it."""
        import tempfile

        import pyarrow as pa
        import pyarrow.parquet as pq

        os.makedirs(self.dir, exist_ok=True)
        fd, path = tempfile.mkstemp(prefix=".stage_", suffix=".parquet", dir=self.dir)
        os.close(fd)
        try:
            pq.write_table(pa.table({c: [str(r[c]) for r in rows] for c in COLUMNS}), path)
            with open(path, "rb") as f:
                os.fsync(f.fileno())
        except BaseException:
            self.discard_staged(path)
            raise
        return path

    @staticmethod
    def discard_staged(path: Optional[str]) -> None:
        if path:
            with contextlib.suppress(FileNotFoundError):
                os.unlink(path)

    def append(self, vectors: np.ndarray, rows: Sequence[Dict[str, Any]], dead: Sequence[int] = (),
               staged: Optional[str] = None) -> None:
        """Durably append one upsert: its tombstones (row ids it replaces) and its rows. Call
        it inside ``write_lock()`` when other processes may write the same table. ``staged``:
        the rows' Parquet from ``stage_rows`` (moved into place instead of written here)."""
        import pyarrow as pa
        import pyarrow.parquet as pq

        v = np.ascontiguousarray(vectors, dtype="<f4")
        if v.ndim != 2 or v.shape[0] != len(rows):
            raise ValueError("vectors must be [n, dim] with one payload row each")
        if staged is not None and pq.read_metadata(staged).num_rows != v.shape[0]:
            raise ValueError("staged payloads do not match the vectors")
        m = json.loads(json.dumps(self.manifest))  # committed to self.manifest only on success
        if m["dim"] is None:
            m["dim"] = int(v.shape[1])
        elif v.shape[1] != m["dim"]:
            raise ValueError(f"dim {v.shape[1]} != table dim {m['dim']}")
        os.makedirs(self.dir, exist_ok=True)
        if len(dead):
            path = self._tombstone_path(int(m.get("generation", 0)))
            with open(path, "ab"):
                pass
            with open(path, "r+b") as f:
                f.truncate(m["tombstones"] * 8)  # drop bytes of an uncommitted append
                f.seek(0, os.SEEK_END)
                f.write(np.asarray(dead, dtype="<i8").tobytes())
                f.flush()
                os.fsync(f.fileno())
            m["tombstones"] += len(dead)
        if v.shape[0]:
            name = f"{_prefix(int(m.get('generation', 0)))}seg_{len(m['segments']):06d}"
            _fsync_write(os.path.join(self.dir, name + ".f32"), v.data)  # the array's bytes, no copy
            if staged is not None:
                tmp = staged
            else:
                table = pa.table({c: [str(r[c]) for r in rows] for c in COLUMNS})
                tmp = os.path.join(self.dir, name + ".parquet.tmp")
                pq.write_table(table, tmp)
                with open(tmp, "rb") as f:
                    os.fsync(f.fileno())
            os.replace(tmp, os.path.join(self.dir, name + ".parquet"))
            m["segments"].append({"name": name, "rows": int(v.shape[0])})
        _fsync_write(self.manifest_path, json.dumps(m).encode())
        self.manifest = m
        st = os.stat(self.manifest_path)
        self._stamp = (st.st_ino, st.st_mtime_ns, st.st_size)

    def segments(self, start: int = 0) -> Iterator[Segment]:
        """The committed segments from index ``start`` on (all by default)."""
        import pyarrow.parquet as pq

        dim = self.manifest["dim"]
        for s in self.manifest["segments"][start:]:
            vec = np.memmap(os.path.join(self.dir, s["name"] + ".f32"), dtype="<f4", mode="r",
                            shape=(s["rows"], dim))
            t = pq.read_table(os.path.join(self.dir, s["name"] + ".parquet")).to_pydict()
            yield Segment(vectors=vec, rows=t)

    def tombstones(self, start: int = 0) -> np.ndarray:
        """Committed tombstones from position ``start`` on (all by default)."""
        n = self.manifest["tombstones"]
        if n <= start:
            return np.empty(0, dtype=np.int64)
        return np.fromfile(self._tombstone_path(), dtype="<i8", count=n - start,
                           offset=8 * start).astype(np.int64)

    def compact(self, live=None) -> int:
        """Rewrite the table without its deleted rows as the next generation; returns it. Call it
        inside ``write_lock()``. ``live``: bool mask [num_rows] of the rows to keep, or the int
        remap that ``FlatIndex.compact`` returns (kept where >= 0), or None for "every row no
        committed tombstone names". The old segments are streamed, ``COPY_ROWS`` rows at a time,
        into the new generation's segment files and fsynced; replacing the manifest commits; then
        the files that the new manifest does not list are removed."""
        import pyarrow as pa
        import pyarrow.parquet as pq

        old = self.manifest
        total = self.num_rows
        if live is None:
            mask = np.ones(total, dtype=bool)
            mask[self.tombstones()] = False
        else:
            a = np.asarray(live)
            mask = a if a.dtype == np.bool_ else a >= 0
            if mask.shape != (total,):
                raise ValueError(f"live must have one entry per committed row ({total}), got {mask.shape}")
        gen = self.generation + 1
        dim = old["dim"]
        os.makedirs(self.dir, exist_ok=True)
        new_segments: List[Dict[str, Any]] = []
        cur = None  # the open output segment: [name, f32 file, parquet writer, rows]

        def close_segment():
            nonlocal cur
            name, f, w, rows = cur
            w.close()
            f.flush()
            os.fsync(f.fileno())
            f.close()
            with open(os.path.join(self.dir, name + ".parquet"), "rb") as pf:
                os.fsync(pf.fileno())
            new_segments.append({"name": name, "rows": rows})
            cur = None

        try:
            row0 = 0
            for s in old["segments"]:
                keep = np.flatnonzero(mask[row0:row0 + s["rows"]])
                row0 += s["rows"]
                if keep.size == 0:
                    continue
                vec = np.memmap(os.path.join(self.dir, s["name"] + ".f32"), dtype="<f4", mode="r",
                                shape=(s["rows"], dim))
                table = pq.read_table(os.path.join(self.dir, s["name"] + ".parquet"))
                pos = 0
                while pos < keep.size:
                    if cur is None:
                        name = f"{_prefix(gen)}seg_{len(new_segments):06d}"
                        cur = [name, open(os.path.join(self.dir, name + ".f32"), "wb"),
                               pq.ParquetWriter(os.path.join(self.dir, name + ".parquet"), table.schema), 0]
                    take = keep[pos:pos + min(self.COPY_ROWS, self.SEGMENT_ROWS - cur[3])]
                    cur[1].write(np.ascontiguousarray(vec[take]).data)
                    cur[2].write_table(table.take(pa.array(take)).cast(cur[2].schema))
                    cur[3] += int(take.size)
                    pos += int(take.size)
                    if cur[3] >= self.SEGMENT_ROWS:
                        close_segment()
                del vec
            if cur is not None:
                close_segment()
        except BaseException:
            if cur is not None:  # the unlisted files stay for the next writer's sweep
                with contextlib.suppress(Exception):
                    cur[2].close()
                cur[1].close()
            raise
        m = {"dim": dim, "generation": gen, "segments": new_segments, "tombstones": 0}
        _fsync_write(self.manifest_path, json.dumps(m).encode())  # the commit point
        self.manifest = m
        st = os.stat(self.manifest_path)
        self._stamp = (st.st_ino, st.st_mtime_ns, st.st_size)
        self._drop_other_generations()
        return gen


__all__ = ["CorpusFiles", "Segment", "COLUMNS"]

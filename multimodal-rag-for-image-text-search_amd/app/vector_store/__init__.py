"""GPU flat cosine index — the engine behind ``app.storage.lancedb_store``.

Replaces the lancedb (Rust) flat scan the reference reaches through
``app/storage/lancedb_store.py:103-123`` and the per-row delete+append upsert at
``:87-101``. The arithmetic runs in ``libmrag.so`` (``csrc/knn.hip``): an fp16 MFMA
scan with per-lane top-k, exact f64 rescoring against the f32 master rows and a
certificate that proves the returned rows are the exact top-k.

``FlatIndex`` accepts numpy arrays (host pointers: the library copies in/out) or
torch CUDA tensors (device pointers, torch's current stream) — results come back
in the same kind.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple, Union

import numpy as np

from app import _native

ArrayLike = Union[np.ndarray, "torch.Tensor"]  # noqa: F821

MAX_DIM = 4096  # K7/K8 fused scan up to 512; K7g (knn_generic.hip) above
MAX_K = 65536
MMR_MAX_FETCH = 1024  # MRAG_KNN_MMR_MAX_FETCH: K16 keeps a query's candidates in LDS
LABEL_ANY = _native.MRAG_LABEL_ANY
LABEL_DELETED = _native.MRAG_LABEL_DELETED


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _stream_ptr(t) -> int:
    import torch

    return int(torch.cuda.current_stream(t.device).cuda_stream)


class FlatIndex:
    """Exact flat cosine index of fixed ``dim`` on one GPU (one Lance table or one shard).

    Row ids are assigned densely in insertion order; ``delete`` tombstones rows
    (their ids are not reused; ``compact`` removes them and renumbers the rest). Each row carries an int32 label (the host maps
    ``user_id`` strings to labels); ``search(..., label=L)`` is the reference's
    ``where("user_id == ...")`` prefilter.
    """

    def __init__(self, dim: int, device: int = 0) -> None:
        if not (1 <= int(dim) <= MAX_DIM):
            raise ValueError(f"dim must be in 1..{MAX_DIM}, got {dim}")
        self.dim = int(dim)
        self.device = int(device)
        h = ctypes.c_void_p()
        _native.call("mrag_knn_create", self.dim, self.device, ctypes.byref(h))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _native.load().mrag_knn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = ctypes.c_int64(0)
        _native.call("mrag_knn_size", self._h, ctypes.byref(n))
        return int(n.value)

    # ------------------------------------------------------------------ writes
    def add(self, rows: ArrayLike, labels: Union[ArrayLike, int, None] = 0) -> int:
        """Append rows ``[n, dim]`` (f32) with labels; returns the first new row id."""
        first = ctypes.c_int64(0)
        if _is_torch(rows):
            import torch

            r = rows.detach().to(dtype=torch.float32).contiguous()
            if r.ndim != 2 or r.shape[1] != self.dim:
                raise ValueError(f"rows must be [n, {self.dim}], got {tuple(r.shape)}")
            n = r.shape[0]
            if labels is None or isinstance(labels, int):
                lab = torch.full((n,), int(labels or 0), dtype=torch.int32, device=r.device)
            else:
                lab = torch.as_tensor(labels).to(device=r.device, dtype=torch.int32).contiguous()
                if tuple(lab.shape) != (n,):
                    raise ValueError(f"labels must be [{n}], got {tuple(lab.shape)}")
            if n and bool((lab < 0).any()):
                raise ValueError("labels must be >= 0")
            torch.cuda.current_stream(r.device).synchronize()
            _native.call("mrag_knn_add", self._h, r.data_ptr(), lab.data_ptr(), n,
                         _native.MRAG_PTR_DEVICE, ctypes.byref(first))
            return int(first.value)
        r = np.ascontiguousarray(rows, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}], got {r.shape}")
        n = r.shape[0]
        if labels is None or isinstance(labels, (int, np.integer)):
            lab = np.full((n,), int(labels or 0), dtype=np.int32)
        else:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.shape != (n,):
                raise ValueError("labels must be [n]")
        if np.any(lab < 0):
            raise ValueError("labels must be >= 0")
        _native.call("mrag_knn_add", self._h, r.ctypes.data, lab.ctypes.data, n,
                     _native.MRAG_PTR_HOST, ctypes.byref(first))
        return int(first.value)

    def set_labels(self, rows: Sequence[int], label: int) -> None:
        ids = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        if ids.size == 0:
            return
        _native.call("mrag_knn_set_labels", self._h, ids.ctypes.data, ids.size, int(label))

    def delete(self, rows: Sequence[int]) -> None:
        self.set_labels(rows, LABEL_DELETED)

    def live_rows(self) -> int:
        """Rows not deleted among the ``len(self)`` ids handed out."""
        n = ctypes.c_int64(0)
        _native.call("mrag_knn_live_rows", self._h, ctypes.byref(n))
        return int(n.value)

    def compact(self) -> np.ndarray:
        """Remove the deleted rows (K15, ``mrag_knn_compact``): the live rows keep their order and
        are renumbered densely, ``len(self)`` becomes the live count and the HBM buffers shrink to
        fit. Returns the int64 remap of the old size: ``remap[old_row]`` is the row's new id, -1
        for a deleted row. Afterwards the index answers every search as a fresh index that was
        given the live rows in order would. With nothing deleted it is the identity and nothing
        is reallocated. Searches may run beside it (they see the index before or after); an
        ``add`` from another thread may not (the remap is sized before the call)."""
        remap = np.empty(len(self), dtype=np.int64)
        size = ctypes.c_int64(0)
        _native.call("mrag_knn_compact", self._h, remap.ctypes.data, ctypes.byref(size))
        return remap

    def compact_profile(self) -> Tuple[float, float, int, int]:
        """(K15a ms, K15b ms, K15a bytes, K15b bytes) of the last ``compact`` (HIP events)."""
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        ba, bb = ctypes.c_int64(0), ctypes.c_int64(0)
        _native.call("mrag_knn_compact_profile", self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(ba),
                     ctypes.byref(bb))
        return float(a.value), float(b.value), int(ba.value), int(bb.value)

    # ------------------------------------------------------------------ search
    def search(self, queries: ArrayLike, k: int, label: Union[int, ArrayLike] = LABEL_ANY, row_offset: int = 0,
               with_f64: bool = False):
        """k best rows per query: ``(scores f32 [nq,k], rows int64 [nq,k][, scores f64])``.

        ``label`` is one filter for the whole batch (an int) or one per query (an array or
        tensor of ``nq`` int32 values, each a label >= 0 or ``LABEL_ANY``): query i then gets
        the k best rows among those its own filter admits, in the same single scan
        (``mrag_knn_search_labels``). An array whose entries are all equal takes the single-filter
        search (the same result by definition, without the per-query mask's cost: DESIGN.md §3.2).
        Empty slots (fewer matching rows than k) have score ``-inf`` and row ``-1``.
        """
        k = int(k)
        if not isinstance(label, (int, np.integer)):
            return self._search_labels(queries, k, label, int(row_offset), with_f64)
        if _is_torch(queries):
            import torch

            q = queries.detach().to(dtype=torch.float32).contiguous()
            if q.ndim == 1:
                q = q.unsqueeze(0)
            if q.shape[1] != self.dim:
                raise ValueError(f"queries must be [nq, {self.dim}]")
            nq = q.shape[0]
            s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            r = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            s64 = torch.empty((nq, k), dtype=torch.float64, device=q.device) if with_f64 else None
            _native.call("mrag_knn_search", self._h, q.data_ptr(), nq, k, int(label), int(row_offset),
                         s.data_ptr(), s64.data_ptr() if s64 is not None else None, r.data_ptr(),
                         _native.MRAG_PTR_DEVICE, _stream_ptr(q))
            return (s, r, s64) if with_f64 else (s, r)
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}], got {q.shape}")
        nq = q.shape[0]
        s = np.empty((nq, k), dtype=np.float32)
        r = np.empty((nq, k), dtype=np.int64)
        s64 = np.empty((nq, k), dtype=np.float64) if with_f64 else None
        _native.call("mrag_knn_search", self._h, q.ctypes.data, nq, k, int(label), int(row_offset),
                     s.ctypes.data, s64.ctypes.data if s64 is not None else None, r.ctypes.data,
                     _native.MRAG_PTR_HOST, None)
        return (s, r, s64) if with_f64 else (s, r)

    def _search_labels(self, queries: ArrayLike, k: int, labels: ArrayLike, row_offset: int, with_f64: bool,
                       group_equal: bool = True):
        """``search`` with one label filter per query. ``group_equal=False`` keeps an array of
        equal entries on the per-query entry point (measurements and kernel tests)."""
        if _is_torch(queries):
            import torch

            q = queries.detach().to(dtype=torch.float32).contiguous()
            if q.ndim == 1:
                q = q.unsqueeze(0)
            if q.shape[1] != self.dim:
                raise ValueError(f"queries must be [nq, {self.dim}]")
            nq = q.shape[0]
            lab = torch.as_tensor(np.asarray(labels) if not _is_torch(labels) else labels)
            lab = lab.detach().reshape(-1).to(device=q.device, dtype=torch.int32).contiguous()
            if lab.shape[0] != nq:
                raise ValueError(f"label must be an int or hold one filter per query ({nq}), got {lab.shape[0]}")
            if nq:
                lo, hi = (int(v) for v in torch.stack(torch.aminmax(lab)).tolist())  # one read-back for both checks
                if lo < LABEL_ANY:
                    raise ValueError("label filters must be labels >= 0 or LABEL_ANY")
                if lo == hi and group_equal:
                    return self.search(q, k, label=lo, row_offset=row_offset, with_f64=with_f64)
            s = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            r = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            s64 = torch.empty((nq, k), dtype=torch.float64, device=q.device) if with_f64 else None
            _native.call("mrag_knn_search_labels", self._h, q.data_ptr(), nq, k, lab.data_ptr(), row_offset,
                         s.data_ptr(), s64.data_ptr() if s64 is not None else None, r.data_ptr(),
                         _native.MRAG_PTR_DEVICE, _stream_ptr(q))
            return (s, r, s64) if with_f64 else (s, r)
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}], got {q.shape}")
        nq = q.shape[0]
        if _is_torch(labels):
            labels = labels.detach().cpu().numpy()
        lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)
        if lab.shape[0] != nq:
            raise ValueError(f"label must be an int or hold one filter per query ({nq}), got {lab.shape[0]}")
        if np.any(lab < LABEL_ANY):
            raise ValueError("label filters must be labels >= 0 or LABEL_ANY")
        if nq and group_equal and lab.min() == lab.max():
            return self.search(q, k, label=int(lab[0]), row_offset=row_offset, with_f64=with_f64)
        s = np.empty((nq, k), dtype=np.float32)
        r = np.empty((nq, k), dtype=np.int64)
        s64 = np.empty((nq, k), dtype=np.float64) if with_f64 else None
        _native.call("mrag_knn_search_labels", self._h, q.ctypes.data, nq, k, lab.ctypes.data, row_offset,
                     s.ctypes.data, s64.ctypes.data if s64 is not None else None, r.ctypes.data,
                     _native.MRAG_PTR_HOST, None)
        return (s, r, s64) if with_f64 else (s, r)

    # ------------------------------------------------------------------ diversity (K16)
    def search_mmr(self, queries: ArrayLike, k: int, fetch_k: Optional[int] = None, lam: float = 0.5,
                   label: Union[int, ArrayLike] = LABEL_ANY, row_offset: int = 0, with_f64: bool = False):
        """``search`` with diversity: k rows per query chosen by maximal marginal relevance among
        the ``fetch_k`` best (default ``min(4 k, 1024)``; at most ``MMR_MAX_FETCH``), in one
        native call (``mrag_knn_search_mmr``). Step 0 takes the best row; every
        later step the candidate with the largest ``lam * score - (1 - lam) * max cosine to a row
        already taken``. ``lam = 1`` is ``search(queries, k)``; smaller values trade relevance
        for spread. Returns what ``search`` returns, rows in selection order with their
        relevance scores. ``label`` as in ``search`` (one filter, or one per query)."""
        k = int(k)
        fetch_k = min(4 * k, MMR_MAX_FETCH) if fetch_k is None else int(fetch_k)
        row_offset = int(row_offset)
        per_query = not isinstance(label, (int, np.integer))
        if _is_torch(queries):
            import torch

            q = queries.detach().to(dtype=torch.float32).contiguous()
            if q.ndim == 1:
                q = q.unsqueeze(0)
            if q.shape[1] != self.dim:
                raise ValueError(f"queries must be [nq, {self.dim}]")
            nq = q.shape[0]
            lab = None
            if per_query:
                lab = torch.as_tensor(np.asarray(label) if not _is_torch(label) else label)
                lab = lab.detach().reshape(-1).to(device=q.device, dtype=torch.int32).contiguous()
                if lab.shape[0] != nq:
                    raise ValueError(f"label must be an int or hold one filter per query ({nq}), got {lab.shape[0]}")
                if nq and int(lab.min()) < LABEL_ANY:
                    raise ValueError("label filters must be labels >= 0 or LABEL_ANY")
            s = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=q.device)
            r = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=q.device)
            s64 = torch.empty((nq, max(k, 0)), dtype=torch.float64, device=q.device) if with_f64 else None
            _native.call("mrag_knn_search_mmr", self._h, q.data_ptr(), nq, k, fetch_k, float(lam),
                         LABEL_ANY if per_query else int(label), lab.data_ptr() if lab is not None else None,
                         row_offset, s.data_ptr(), s64.data_ptr() if s64 is not None else None, r.data_ptr(),
                         _native.MRAG_PTR_DEVICE, _stream_ptr(q))
            return (s, r, s64) if with_f64 else (s, r)
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"queries must be [nq, {self.dim}], got {q.shape}")
        nq = q.shape[0]
        lab = None
        if per_query:
            if _is_torch(label):
                label = label.detach().cpu().numpy()
            lab = np.ascontiguousarray(np.asarray(label).reshape(-1), dtype=np.int32)
            if lab.shape[0] != nq:
                raise ValueError(f"label must be an int or hold one filter per query ({nq}), got {lab.shape[0]}")
        s = np.empty((nq, max(k, 0)), dtype=np.float32)
        r = np.empty((nq, max(k, 0)), dtype=np.int64)
        s64 = np.empty((nq, max(k, 0)), dtype=np.float64) if with_f64 else None
        _native.call("mrag_knn_search_mmr", self._h, q.ctypes.data, nq, k, fetch_k, float(lam),
                     LABEL_ANY if per_query else int(label), lab.ctypes.data if lab is not None else None,
                     row_offset, s.ctypes.data, s64.ctypes.data if s64 is not None else None, r.ctypes.data,
                     _native.MRAG_PTR_HOST, None)
        return (s, r, s64) if with_f64 else (s, r)

    def mmr_select(self, rows: ArrayLike, scores64: ArrayLike, k: int, lam: float, with_values: bool = False):
        """K16 alone (``mrag_knn_mmr_select``): ``rows`` int64 ``[nq, m]`` (row ids of this index,
        -1 for an empty slot) and ``scores64`` f64 ``[nq, m]``, e.g. ``search(q, m, with_f64=True)``
        without a ``row_offset``. Returns the selected candidate positions int32 ``[nq, k]`` in
        selection order (-1 once the candidates run out) and, with ``with_values``, the f64 value
        each was selected with. numpy in, numpy out; torch CUDA in, torch out."""
        k = int(k)
        if _is_torch(rows):
            import torch

            r = rows.detach().to(dtype=torch.int64).contiguous()
            s64 = scores64.detach().to(device=r.device, dtype=torch.float64).contiguous()
            if r.ndim != 2 or s64.shape != r.shape:
                raise ValueError("rows and scores64 must both be [nq, m]")
            nq, m = r.shape
            pos = torch.empty((nq, max(k, 0)), dtype=torch.int32, device=r.device)
            val = torch.empty((nq, max(k, 0)), dtype=torch.float64, device=r.device) if with_values else None
            _native.call("mrag_knn_mmr_select", self._h, r.data_ptr(), s64.data_ptr(), nq, m, k, float(lam),
                         pos.data_ptr(), val.data_ptr() if val is not None else None, _native.MRAG_PTR_DEVICE,
                         _stream_ptr(r))
            return (pos, val) if with_values else pos
        r = np.ascontiguousarray(rows, dtype=np.int64)
        s64 = np.ascontiguousarray(scores64, dtype=np.float64)
        if r.ndim != 2 or s64.shape != r.shape:
            raise ValueError("rows and scores64 must both be [nq, m]")
        nq, m = r.shape
        pos = np.empty((nq, max(k, 0)), dtype=np.int32)
        val = np.empty((nq, max(k, 0)), dtype=np.float64) if with_values else None
        _native.call("mrag_knn_mmr_select", self._h, r.ctypes.data, s64.ctypes.data, nq, m, k, float(lam),
                     pos.ctypes.data, val.ctypes.data if val is not None else None, _native.MRAG_PTR_HOST, None)
        return (pos, val) if with_values else pos

    def profile(self, enable: int = -1) -> Tuple[float, int]:
        """Scan-kernel timing (HIP events on the search stream): enable=1 reset+on,
        0 off, -1 read. Returns (total scan ms, timed launches)."""
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        _native.call("mrag_knn_profile", self._h, int(enable), ctypes.byref(ms), ctypes.byref(n))
        return float(ms.value), int(n.value)

    def last_stats(self) -> Tuple[int, int]:
        """(uncertified queries, collect retries) of the last search."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        _native.call("mrag_knn_last_stats", self._h, ctypes.byref(a), ctypes.byref(b))
        return int(a.value), int(b.value)


def topk_merge(scores64, rows, k: int):
    """Merge per-shard lists ``[nlists, nq, k]`` (torch CUDA f64 / int64) into the
    global top-k under (score desc, row asc): K11 in ``csrc/knn.hip``."""
    import torch

    if scores64.ndim != 3 or rows.shape != scores64.shape:
        raise ValueError("expected [nlists, nq, k] scores and rows")
    nl, nq, kk = scores64.shape
    if kk != k:
        raise ValueError("k mismatch")
    s64 = scores64.contiguous()
    r = rows.contiguous()
    out_s = torch.empty((nq, k), dtype=torch.float32, device=s64.device)
    out_s64 = torch.empty((nq, k), dtype=torch.float64, device=s64.device)
    out_r = torch.empty((nq, k), dtype=torch.int64, device=s64.device)
    _native.call("mrag_topk_merge", s64.data_ptr(), r.data_ptr(), nl, nq, k, out_s.data_ptr(),
                 out_s64.data_ptr(), out_r.data_ptr(), _stream_ptr(s64))
    return out_s, out_r, out_s64


def l2norm_rows(x):
    """K6: the reference's numpy ``_normalize`` (app/ml/embeddings.py:46-49) on the GPU,
    bit-identical. ``x``: torch CUDA f32 [rows, dim]; returns a new tensor."""
    import torch

    t = x.detach().to(dtype=torch.float32).contiguous()
    if t.ndim != 2:
        raise ValueError("expected [rows, dim]")
    y = torch.empty_like(t)
    _native.call("mrag_l2norm_rows", t.data_ptr(), y.data_ptr(), t.shape[0], t.shape[1], _stream_ptr(t))
    return y


__all__ = ["FlatIndex", "topk_merge", "l2norm_rows", "LABEL_ANY", "LABEL_DELETED", "MMR_MAX_FETCH"]

"""Exact cosine top-k over the compressed-vector store, on the device: the retrieval side of
``diffusion_prefill`` (``FusionANN::search``, fusion_ann.rs:109-136, over the ``CompressedVector``
records ``KVCache`` keeps, prefill_kv.rs:69-140).  The scan reads the byte codes that
``compress_vectors`` wrote and folds the dequantization into the score; the rule is pinned in
include/dllm_quant.h (section 8g) and is bit-reproducible on the host.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch

from . import _lib
from ._lib import check
from .kvquant import compress_vectors, decompress_vectors
from .quantization import _dev, _ptr, _stream

MAX_K = 256


def search_table(codes: torch.Tensor, scales: torch.Tensor, zps: torch.Tensor) -> torch.Tensor:
    """dllm_search_table: the per-row (u, v) = (scale, zero point) / |row| pairs, f32 [rows, 2].
    One read of the codes; rebuild it only for rows that change."""
    q = _dev(codes, torch.uint8)
    rows, dim = q.shape
    table = torch.empty(rows, 2, dtype=torch.float32, device=q.device)
    check(_lib.load().dllm_search_table(_ptr(q), rows, dim, _ptr(_dev(scales, torch.float32)),
                                        _ptr(_dev(zps, torch.float32)), _ptr(table), _stream()))
    return table


def search_vectors(queries: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, zps: torch.Tensor, k: int,
                   table: torch.Tensor | None = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k rows of the store (codes u8 [rows, dim], scales / zps f32 [rows]) nearest to each query by
    cosine similarity -> (idx int32 [nq, k], scores f32 [nq, k]) in rank order (score descending, index
    ascending; index -1 / score -inf past the end of a store with fewer than k rows).  A 1-D query
    returns 1-D results.  ``table``: a prebuilt ``search_table`` of the same rows."""
    Q = _dev(queries, torch.float32)
    single = Q.dim() == 1
    if single:
        Q = Q.reshape(1, -1)
    q = _dev(codes, torch.uint8)
    rows, dim = q.shape
    if Q.shape[1] != dim:
        raise _lib.ShapeMismatch(f"queries have {Q.shape[1]} elements, the store's rows {dim}")
    if table is None:
        table = search_table(q, scales, zps)
    table = _dev(table, torch.float32)
    if table.numel() != 2 * rows:
        raise _lib.ShapeMismatch("table must be [rows, 2]")
    nq, k = Q.shape[0], int(k)
    if not 1 <= k <= MAX_K:
        raise _lib.InvalidParams("k must be between 1 and 256")
    L = _lib.load()
    idx = torch.empty(nq, k, dtype=torch.int32, device=Q.device)
    scores = torch.empty(nq, k, dtype=torch.float32, device=Q.device)
    wsb = L.dllm_search_workspace(nq, rows, k)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=Q.device)
    check(L.dllm_search_vectors(_ptr(Q), nq, _ptr(q), _ptr(table), rows, dim, k, _ptr(idx), _ptr(scores), _ptr(ws),
                                wsb, _stream()))
    return (idx[0], scores[0]) if single else (idx, scores)


class VectorIndex:
    """``KVCache`` (prefill_kv.rs:69-140) with ``FusionANN::search`` over it: vectors are compressed
    on insert (``compress_vector``, :104-121), kept as rows of one device store and searched on their
    byte codes.  Ids are the reference's u32 keys (``id.to_string()`` only fixes ``size_bytes``)."""

    def __init__(self, dim: int, bits: int):
        if not 1 <= int(dim) <= 65535:
            raise _lib.InvalidParams("dim must be between 1 and 65535")
        if not 1 <= int(bits) <= 8:
            raise _lib.InvalidParams("Bits must be between 1 and 8")
        self.dim, self.bits = int(dim), int(bits)
        self._slot: Dict[int, int] = {}     # id -> row of the store
        self._ids: List[int] = []           # row -> id
        self._codes = self._scales = self._zps = self._table = None   # device tensors, rows = capacity

    def __len__(self) -> int:
        return len(self._ids)

    # ---- bookkeeping (host only) ----------------------------------------------------------------
    def _assign(self, ids: Sequence[int]) -> Tuple[List[int], List[int]]:
        """Rows for a batch of ids: an id already present keeps its row (``DashMap::insert``
        replaces, :81), a new one appends.  An id repeated within the batch keeps its last vector,
        as successive inserts do.  -> (rows, positions in the batch that are written)."""
        last = {int(i): p for p, i in enumerate(ids)}
        rows, keep = [], []
        for p, i in enumerate(ids):
            i = int(i)
            if last[i] != p:
                continue
            if i not in self._slot:
                self._slot[i] = len(self._ids)
                self._ids.append(i)
            rows.append(self._slot[i])
            keep.append(p)
        return rows, keep

    def _lookup(self, ids: Sequence[int]) -> List[int]:
        """Row of each id, -1 where it is missing."""
        return [self._slot.get(int(i), -1) for i in ids]

    def size_bytes(self) -> int:
        """prefill_kv.rs:135-139: the codes' bytes plus each key string's."""
        return len(self._ids) * self.dim + sum(len(str(i)) for i in self._ids)

    # ---- device ------------------------------------------------------------------------------------
    def _reserve(self, n: int, device):
        cap = 0 if self._codes is None else self._codes.shape[0]
        if n <= cap:
            return
        new = max(n, 2 * cap, 64)
        grown = (torch.empty(new, self.dim, dtype=torch.uint8, device=device),
                 torch.empty(new, dtype=torch.float32, device=device),
                 torch.empty(new, dtype=torch.float32, device=device),
                 torch.empty(new, 2, dtype=torch.float32, device=device))
        if cap:
            for dst, src in zip(grown, (self._codes, self._scales, self._zps, self._table)):
                dst[:cap] = src
        self._codes, self._scales, self._zps, self._table = grown

    def insert_batch(self, ids: Sequence[int], x: torch.Tensor) -> None:
        """``insert_batch`` (:79-84) of ``compress_vector(id, x[i], bits)``: appends, and replaces the
        row of an id that is already stored.  The search table is built for the written rows only."""
        x = _dev(x, torch.float32)
        if x.dim() != 2 or x.shape[1] != self.dim or x.shape[0] != len(ids):
            raise _lib.ShapeMismatch(f"x must be [{len(ids)}, {self.dim}]")
        if not len(ids):
            return
        codes, scales, zps = compress_vectors(x, self.bits)
        table = search_table(codes, scales, zps)
        rows, keep = self._assign(ids)
        self._reserve(len(self._ids), x.device)
        at = torch.tensor(rows, dtype=torch.long, device=x.device)
        if len(keep) != len(ids):
            sel = torch.tensor(keep, dtype=torch.long, device=x.device)
            codes, scales, zps, table = codes[sel], scales[sel], zps[sel], table[sel]
        self._codes[at], self._scales[at], self._zps[at], self._table[at] = codes, scales, zps, table

    def get_batch(self, ids: Sequence[int]) -> torch.Tensor:
        """``get_batch`` (:87-101): the decompressed vectors, f32 [len(ids), dim]; a missing id gives
        a zero vector."""
        rows = self._lookup(ids)
        found = [p for p, r in enumerate(rows) if r >= 0]
        dev = self._codes.device if self._codes is not None else torch.device("cuda")
        out = torch.zeros(len(rows), self.dim, dtype=torch.float32, device=dev)
        if found:
            at = torch.tensor([rows[p] for p in found], dtype=torch.long, device=dev)
            out[torch.tensor(found, dtype=torch.long, device=dev)] = decompress_vectors(
                self._codes[at], self._scales[at], self._zps[at])
        return out

    def search_batch(self, Q: torch.Tensor, k: int) -> List[List[Tuple[int, float]]]:
        """``FusionANN::search`` for each row of Q: [(id, cosine)] in rank order, at most len(self)."""
        Q = _dev(Q, torch.float32).reshape(-1, self.dim)
        n = len(self._ids)
        if n == 0:
            if not 1 <= int(k) <= MAX_K:
                raise _lib.InvalidParams("k must be between 1 and 256")
            return [[] for _ in range(Q.shape[0])]
        idx, scores = search_vectors(Q, self._codes[:n], self._scales[:n], self._zps[:n], k, table=self._table[:n])
        idx, scores = idx.cpu().tolist(), scores.cpu().tolist()
        return [[(self._ids[i], s) for i, s in zip(ri, rs) if i >= 0] for ri, rs in zip(idx, scores)]

    def search(self, query: torch.Tensor, k: int) -> List[Tuple[int, float]]:
        return self.search_batch(_dev(query, torch.float32).reshape(1, -1), k)[0]

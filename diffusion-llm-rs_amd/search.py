"""Exact cosine top-k over the compressed-vector store, on the device: the retrieval side of
``diffusion_prefill`` (``FusionANN::search``, fusion_ann.rs:109-136, over the ``CompressedVector``
records ``KVCache`` keeps, prefill_kv.rs:69-140).  The scan reads the byte codes that
``compress_vectors`` wrote and folds the dequantization into the score; the rule is pinned in
include/dllm_quant.h (section 8g) and is bit-reproducible on the host.

Stored rows against stored rows (``neighbor_rows``, ``VectorIndex.neighbors`` / ``build_graph``) is the
navigation graph of ``ns-router-rs`` (``NsRouter::build_graph``, lib.rs:99-133): both operands are byte
codes, the dot product an exact integer off the int8 matrix cores; the rule is section 8l.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check
from .kvquant import compress_vectors, decompress_vectors
from .quantization import _dev, _ptr, _stream

MAX_K = 256
GRAPH_WORKSPACE_BUDGET = 256 << 20      # bytes of workspace build_graph's default block stays under


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


def neighbor_table(codes: torch.Tensor, scales: torch.Tensor, zps: torch.Tensor) -> torch.Tensor:
    """dllm_neighbor_table: the opaque per-row pair table (uint8 [rows, dllm_neighbor_table_bytes(1)]);
    a row's entry depends on that row alone, so ``table[a:b]`` is the table of rows a..b."""
    q = _dev(codes, torch.uint8)
    rows, dim = q.shape
    L = _lib.load()
    per = L.dllm_neighbor_table_bytes(1)
    table = torch.empty(rows, per, dtype=torch.uint8, device=q.device)
    check(L.dllm_neighbor_table(_ptr(q), rows, dim, _ptr(_dev(scales, torch.float32)), _ptr(_dev(zps, torch.float32)),
                                _ptr(table), _stream()))
    return table


def _as_table(table: torch.Tensor, rows: int) -> torch.Tensor:
    table = _dev(table, torch.uint8)
    if table.numel() != _lib.load().dllm_neighbor_table_bytes(rows):
        raise _lib.ShapeMismatch("table must be the neighbor_table of the same rows")
    return table


def neighbor_rows(qcodes: torch.Tensor, qscales: Optional[torch.Tensor], qzps: Optional[torch.Tensor],
                  codes: torch.Tensor, scales: Optional[torch.Tensor], zps: Optional[torch.Tensor], k: int,
                  threshold: float = -math.inf, self_base: int = -1, qtable: Optional[torch.Tensor] = None,
                  table: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k rows of the store nearest by cosine to each query row, the queries being compressed rows
    themselves (a block of the same store, or rows of another store of the same dim) -> (idx int32
    [nq, k], scores f32 [nq, k]) in rank order.  A pair is left out when it is the query's own row
    (``self_base`` >= 0: query j is row self_base + j of the store) or its score is below ``threshold``;
    such places and those past the end are index -1, score -inf.  ``qtable`` / ``table``: prebuilt
    ``neighbor_table`` of the queries / the store (then the scales and zero points may be None)."""
    qc, c = _dev(qcodes, torch.uint8), _dev(codes, torch.uint8)
    if qc.dim() != 2 or c.dim() != 2 or qc.shape[1] != c.shape[1]:
        raise _lib.ShapeMismatch(f"query rows have {tuple(qc.shape)[1:]} codes, the store's rows {tuple(c.shape)[1:]}")
    (nq, dim), rows, k = qc.shape, c.shape[0], int(k)
    if not 1 <= k <= MAX_K:
        raise _lib.InvalidParams("k must be between 1 and 256")
    qtable = neighbor_table(qc, qscales, qzps) if qtable is None else _as_table(qtable, nq)
    table = neighbor_table(c, scales, zps) if table is None else _as_table(table, rows)
    L = _lib.load()
    idx = torch.empty(nq, k, dtype=torch.int32, device=c.device)
    out = torch.empty(nq, k, dtype=torch.float32, device=c.device)
    wsb = L.dllm_neighbor_workspace(nq, rows, k)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=c.device)
    check(L.dllm_neighbor_rows(_ptr(qc), _ptr(qtable), nq, _ptr(c), _ptr(table), rows, dim, k, float(threshold),
                               int(self_base), _ptr(idx), _ptr(out), _ptr(ws), wsb, _stream()))
    return idx, out


class NavigationGraph:
    """``NsRouter::build_graph``'s ``DiGraph<String, f32>`` (ns-router-rs/src/lib.rs:99-133): one node per
    stored vector, up to k edges from each node to its nearest other nodes, weight = cosine.
    ``ids``: row -> id; ``idx`` / ``scores``: device tensors [n, k], -1 / -inf where a node has fewer edges."""

    def __init__(self, ids: Sequence[int], idx: torch.Tensor, scores: torch.Tensor):
        self.ids = [int(i) for i in ids]
        self.idx, self.scores = idx, scores
        self._row = {i: r for r, i in enumerate(self.ids)}
        self._host = None

    def __len__(self) -> int:
        return len(self.ids)

    def _lists(self):
        if self._host is None:
            self._host = (self.idx.cpu().tolist(), self.scores.cpu().tolist())
        return self._host

    def neighbors(self, id: int) -> List[Tuple[int, float]]:
        """One node's edges, [(id, cosine)] in rank order; [] for an id that is no node."""
        r = self._row.get(int(id), -1)
        if r < 0:
            return []
        idx, sc = self._lists()
        return [(self.ids[t], s) for t, s in zip(idx[r], sc[r]) if t >= 0]

    def edges(self) -> List[Tuple[int, int, float]]:
        """[(id_a, id_b, weight)], node by node in row order, each node's edges in rank order."""
        idx, sc = self._lists()
        return [(self.ids[r], self.ids[t], s) for r in range(len(self.ids)) for t, s in zip(idx[r], sc[r]) if t >= 0]


def graph_block(n: int, k: int, budget: int = GRAPH_WORKSPACE_BUDGET) -> int:
    """Query rows per call that keep dllm_neighbor_workspace(block, n, k) under ``budget`` bytes: the
    score matrix is 4 n bytes per query row and the select keys at most 8 k ceil(n / 2048) (1 + 1 / 8)."""
    per_row = 4 * n + 9 * k * (-(-n // 2048)) + 16
    return max(1, min(n, budget // per_row))


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
        self._pairs = None                  # the neighbor_table of rows [0, len), built on demand

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
        self._pairs = None
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

    # ---- rows against rows (ns-router-rs build_graph) ----------------------------------------------
    def _pair_table(self) -> torch.Tensor:
        """The pair table of the stored rows: built on the first use after an insert, then kept."""
        if self._pairs is None:
            n = len(self._ids)
            self._pairs = neighbor_table(self._codes[:n], self._scales[:n], self._zps[:n])
        return self._pairs

    def neighbors(self, ids: Sequence[int], k: int, threshold: float = -math.inf) -> List[List[Tuple[int, float]]]:
        """Per id the stored vectors nearest to that stored vector, [(id, cosine)] in rank order, the
        vector itself excluded and scores below ``threshold`` left out; [] for a missing id."""
        if not 1 <= int(k) <= MAX_K:
            raise _lib.InvalidParams("k must be between 1 and 256")
        rows = self._lookup(ids)
        found = [p for p, r in enumerate(rows) if r >= 0]
        out: List[List[Tuple[int, float]]] = [[] for _ in rows]
        if not found:
            return out
        n = len(self._ids)
        table = self._pair_table()
        for p in found:                     # one call per id: its own row is a different self_base each
            r = rows[p]
            idx, sc = neighbor_rows(self._codes[r:r + 1], None, None, self._codes[:n], None, None, k, threshold,
                                    self_base=r, qtable=table[r:r + 1], table=table)
            out[p] = [(self._ids[t], s) for t, s in zip(idx[0].cpu().tolist(), sc[0].cpu().tolist()) if t >= 0]
        return out

    def build_graph(self, k: int, threshold: float = 0.8, block: Optional[int] = None) -> NavigationGraph:
        """``NsRouter::build_graph``: every stored vector against every other, up to k edges per node with
        cosine >= ``threshold`` (``SystemConfig::similarity_threshold``).  The store is walked in blocks of
        ``block`` query rows (default: ``graph_block``, which keeps a call's workspace under
        GRAPH_WORKSPACE_BUDGET); a ragged last block is the normal case."""
        if not 1 <= int(k) <= MAX_K:
            raise _lib.InvalidParams("k must be between 1 and 256")
        n, k = len(self._ids), int(k)
        if block is not None and int(block) < 1:
            raise _lib.InvalidParams("block must be at least 1")
        dev = self._codes.device if self._codes is not None else torch.device("cuda")
        idx = torch.empty(n, k, dtype=torch.int32, device=dev)
        sc = torch.empty(n, k, dtype=torch.float32, device=dev)
        if n:
            step = graph_block(n, k) if block is None else int(block)
            table = self._pair_table()
            for r0 in range(0, n, step):
                r1 = min(n, r0 + step)
                idx[r0:r1], sc[r0:r1] = neighbor_rows(self._codes[r0:r1], None, None, self._codes[:n], None, None, k,
                                                      threshold, self_base=r0, qtable=table[r0:r1], table=table)
        return NavigationGraph(self._ids, idx, sc)

"""Deduplication of the compressed-vector store, on the device: ``IODedupEngine::store_vectors``
(io-dedup/src/lib.rs:119-135) between ``compress_vectors`` and the search -- ``compute_hash`` of each
row's code bytes (:161-166), ``deduplicate`` (:145-159: a row whose hash was seen before is dropped,
whatever its bytes) and ``merge_requests``' concatenation of the survivors (:181-212).  The three rules
are pinned in include/dllm_quant.h (section 8i); everything is integer arithmetic and bit-reproducible
on the host.

Hashes and sequence numbers are u64.  torch has no arithmetic on uint64, so they are returned as
int64 tensors holding the same 64 bits: ``t.cpu().numpy().view(numpy.uint64)`` is the value.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import _lib
from ._lib import check
from .quantization import _dev, _ptr, _stream


def _rows_of(codes) -> Tuple[torch.Tensor, int, int, int]:
    """codes as a device u8 matrix the kernels can read in place -> (tensor, rows, dim, ld).  A view
    with unit column stride and any row stride >= dim (a slice of wider rows, an offset into a larger
    buffer) is read where it lies; anything else is copied."""
    q = codes if isinstance(codes, torch.Tensor) and codes.is_cuda and codes.dtype == torch.uint8 else _dev(codes, torch.uint8)
    if q.dim() != 2:
        raise _lib.ShapeMismatch("codes must be [rows, dim]")
    rows, dim = q.shape
    if rows > 1 and dim and (q.stride(1) != 1 or q.stride(0) < dim):
        q = q.contiguous()
    if rows <= 1 and dim > 1 and q.stride(1) != 1:
        q = q.contiguous()
    return q, rows, dim, (q.stride(0) if rows > 1 else dim)


def hash_rows(codes: torch.Tensor) -> torch.Tensor:
    """dllm_hash_rows: ``compute_hash`` of every row of codes (u8 [rows, dim]) -> int64 [rows] holding
    the u64 hash bits (view as uint64 on the host).  One read of the codes; any alignment."""
    q, rows, dim, ld = _rows_of(codes)
    h = torch.empty(rows, dtype=torch.int64, device=q.device)
    check(_lib.load().dllm_hash_rows(_ptr(q), rows, dim, ld, _ptr(h), _stream()))
    return h


def _filter(hashes: torch.Tensor, base: int, table: torch.Tensor | None, slots: int):
    L = _lib.load()
    rows, dev = hashes.numel(), hashes.device
    keep = torch.zeros(rows, dtype=torch.uint8, device=dev)
    first = torch.empty(rows, dtype=torch.int64, device=dev)
    kept_rows = torch.empty(rows, dtype=torch.int32, device=dev)
    n_kept = torch.zeros(1, dtype=torch.int32, device=dev)     # rows == 0 writes nothing: the count stays 0
    wsb = L.dllm_dedup_workspace(rows)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(L.dllm_dedup_rows(_ptr(hashes), rows, base, _ptr(table), slots, _ptr(keep), _ptr(first), _ptr(kept_rows),
                            _ptr(n_kept), _ptr(ws), wsb, _stream()))
    return keep.view(torch.bool), first, kept_rows, n_kept[0]


def dedup_rows(codes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The one-shot filter, within this batch alone -> (keep bool [rows], first int64 [rows], kept_rows
    int32 [rows], n_kept int32 scalar), all on the device, nothing synchronised.  keep[r]: no earlier
    row has row r's hash.  first[r]: the index of the first row with that hash.  kept_rows: the kept
    indices ascending, then -1.  Equal hash means duplicate even where the bytes differ, as in the
    reference; compare rows r and first[r] to tell."""
    return _filter(hash_rows(codes), 0, None, 0)


def gather_rows(codes: torch.Tensor, kept_rows: torch.Tensor, n_kept: torch.Tensor, out: torch.Tensor | None = None
                ) -> torch.Tensor:
    """dllm_gather_rows: out[i] = codes[kept_rows[i]] for i < n_kept (read on the device; no sync) ->
    out u8 [rows, dim], rows from n_kept on untouched (uninitialised when out is not given)."""
    q, rows, dim, ld = _rows_of(codes)
    kept_rows, n_kept = _dev(kept_rows, torch.int32), _dev(n_kept, torch.int32).reshape(1)
    if out is None:
        out = torch.empty(rows, dim, dtype=torch.uint8, device=q.device)
    if out.dtype != torch.uint8 or out.dim() != 2 or out.shape != (rows, dim) or not out.is_contiguous() or \
            not out.is_cuda or kept_rows.numel() != rows:
        raise _lib.ShapeMismatch("out must be a contiguous device u8 [rows, dim], kept_rows int32 [rows]")
    if rows and dim:
        check(_lib.load().dllm_gather_rows(_ptr(q), dim, ld, _ptr(kept_rows), _ptr(n_kept), _ptr(out), dim, _stream()))
    return out


class DedupBuffer:
    """The reference's ``DedupBuffer`` (``seen_hashes``, io-dedup/src/lib.rs:102-106) as a device
    table: remembers every hash offered to ``filter`` until ``reset``.  ``max_rows`` is the number of
    rows that may be offered in all (duplicates included: a row's sequence number is its place among
    all rows ever offered, so the count never goes back); the table is kept at most half full."""

    def __init__(self, max_rows: int, device=None):
        max_rows = int(max_rows)
        if not 1 <= max_rows < 2 ** 40:
            raise _lib.InvalidParams("max_rows must be between 1 and 2^40")
        self.max_rows = max_rows
        self.slots = 2
        while self.slots < 2 * max_rows:
            self.slots *= 2
        L = _lib.load()
        self._table = torch.empty(L.dllm_dedup_table_bytes(self.slots) // 8, dtype=torch.int64,
                                  device=device if device is not None else "cuda")
        self.base = 0
        self.reset()

    def reset(self) -> None:
        """Forgets every hash; sequence numbers start again at 0."""
        check(_lib.load().dllm_dedup_table_init(_ptr(self._table), self.slots, _stream()))
        self.base = 0

    def filter_hashes(self, hashes: torch.Tensor):
        hashes = _dev(hashes, torch.int64)
        out = _filter(hashes, self.base, self._table, self.slots)
        self.base += hashes.numel()
        return out

    def filter(self, codes: torch.Tensor):
        """The stateful filter: as ``dedup_rows``, but a row is also dropped when an earlier call saw
        its hash, and ``first`` is a sequence number (the row's place among all rows offered since the
        last reset).  Raises InvalidParams, before anything runs, when the rows offered would exceed
        slots / 2."""
        return self.filter_hashes(hash_rows(codes))

    def seen(self) -> int:
        """The number of distinct hashes held (one small copy from the device)."""
        return int(self._table[1].item())

    def overflowed(self) -> bool:
        """The table's flag word: a row found no slot.  Cannot happen through ``filter``."""
        return bool(self._table[0].item())


def store_vectors(buf: DedupBuffer, ids: Sequence[int] | torch.Tensor, codes: torch.Tensor, scales: torch.Tensor,
                  zps: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """``IODedupEngine::store_vectors`` minus the file write: filter the batch against ``buf``, then
    gather -> (ids int64 [n], codes u8 [n, dim], scales f32 [n], zps f32 [n]) of the kept records, in
    order and contiguous, on the device, in buffers of the kept rows' size (a batch of duplicates
    hands back one row, not a view of a batch-sized allocation).  The one read of n_kept, between the
    filter and the gather, stands where the reference calls ``sync_all``."""
    q, rows, dim, _ = _rows_of(codes)
    ids = _dev(ids, torch.int64).reshape(-1)
    scales, zps = _dev(scales, torch.float32).reshape(-1), _dev(zps, torch.float32).reshape(-1)
    if ids.numel() != rows or scales.numel() != rows or zps.numel() != rows:
        raise _lib.ShapeMismatch(f"ids, scales and zps must have {rows} elements")
    _, _, kept_rows, n_kept = buf.filter(q)
    n = int(n_kept.item())
    if n > rows:
        raise _lib.QuantizationError(f"n_kept = {n} exceeds the batch's {rows} rows")
    out = torch.empty(n, dim, dtype=torch.uint8, device=q.device)   # n is the device's own count: n rows are written
    if n:
        check(_lib.load().dllm_gather_rows(_ptr(q), dim, q.stride(0) if rows > 1 else dim, _ptr(kept_rows),
                                           _ptr(n_kept.reshape(1)), _ptr(out), dim, _stream()))
    at = kept_rows[:n].long()
    return ids[at], out, scales[at], zps[at]

"""Two independent restatements of the dedup rules (include/dllm_quant.h, section 8i), for the tests.

* ``hash_fold`` / ``filter_loop``: the reference's loops literally, on Python ints (the fold with
  ``& (2**64 - 1)``, a dict of seen hashes).
* ``hash_rows`` / ``dedup``: numpy -- the power-weighted sum in wrapping uint64, and a first-occurrence
  filter built from a stable sort.
Everything is integer arithmetic: the tests compare with ``==``.
"""
import numpy as np

MASK = 2 ** 64 - 1
NOSEQ = MASK


def hash_fold(row) -> int:
    """compute_hash: fold(0u64, |acc, b| acc * 31 + b), wrapping."""
    acc = 0
    for b in bytes(bytearray(np.asarray(row, np.uint8))):
        acc = (acc * 31 + b) & MASK
    return acc


def hash_rows_loop(codes) -> np.ndarray:
    return np.array([hash_fold(r) for r in np.asarray(codes, np.uint8)], np.uint64)


def powers(dim: int) -> np.ndarray:
    """31^(dim - 1 - i) mod 2^64, i = 0 .. dim - 1 (a cumulative product that wraps in uint64)."""
    p = np.ones(dim, np.uint64)
    if dim > 1:
        with np.errstate(over="ignore"):
            p[1:] = np.cumprod(np.full(dim - 1, 31, np.uint64))
    return p[::-1].copy()


def hash_rows(codes) -> np.ndarray:
    """h = sum_i b_i 31^(dim - 1 - i) mod 2^64, row by row (uint64 arithmetic wraps)."""
    codes = np.asarray(codes, np.uint8)
    if codes.shape[0] == 0:
        return np.zeros(0, np.uint64)
    w = powers(codes.shape[1])
    with np.errstate(over="ignore"):
        return (codes.astype(np.uint64) * w[None, :]).sum(axis=1, dtype=np.uint64)


def filter_loop(hashes, base=0, seen=None):
    """deduplicate, literally: ``seen`` (a dict hash -> first sequence number) persists across calls.
    -> (keep u8, first u64, kept_rows i32 with the -1 tail, n_kept)."""
    seen = {} if seen is None else seen
    hashes = [int(h) for h in np.asarray(hashes, np.uint64)]
    keep, first, kept = [], [], []
    for r, h in enumerate(hashes):
        if h not in seen:
            seen[h] = base + r
            keep.append(1)
            kept.append(r)
        else:
            keep.append(0)
        first.append(seen[h])
    rows = len(hashes)
    return (np.array(keep, np.uint8), np.array(first, np.uint64),
            np.array(kept + [-1] * (rows - len(kept)), np.int32), len(kept))


class Seen:
    """The numpy filter's seen-set: parallel sorted arrays of hashes and first sequence numbers."""

    def __init__(self):
        self.h = np.zeros(0, np.uint64)
        self.s = np.zeros(0, np.uint64)


def dedup(hashes, base=0, seen=None):
    """The same contract from a stable sort: a row is kept iff it is the first of its hash in the
    batch and the hash is not in ``seen``."""
    seen = Seen() if seen is None else seen
    hashes = np.asarray(hashes, np.uint64)
    rows = hashes.size
    order = np.argsort(hashes, kind="stable")
    sh = hashes[order]
    head = np.ones(rows, bool)
    head[1:] = sh[1:] != sh[:-1]
    lead = order[np.maximum.accumulate(np.where(head, np.arange(rows), 0))] if rows else order   # first row of each run
    first_in_batch = np.empty(rows, np.int64)
    first_in_batch[order] = lead
    old = np.zeros(rows, bool)
    if seen.h.size:
        at = np.minimum(np.searchsorted(seen.h, hashes), seen.h.size - 1)
        old = seen.h[at] == hashes
    keep = (first_in_batch == np.arange(rows)) & ~old
    first = (first_in_batch + base).astype(np.uint64)
    if old.any():
        first[old] = seen.s[at[old]]
    kept = np.nonzero(keep)[0].astype(np.int32)
    allh = np.concatenate([seen.h, hashes[kept]])
    alls = np.concatenate([seen.s, first[kept]])
    o = np.argsort(allh, kind="stable")
    seen.h, seen.s = allh[o], alls[o]
    return (keep.astype(np.uint8), first, np.concatenate([kept, np.full(rows - kept.size, -1, np.int32)]),
            int(kept.size))


def row_with_hash(target: int, dim: int) -> np.ndarray:
    """A row of ``dim`` codes, all <= 30, whose hash is ``target`` < 31^dim: its base-31 digits (no wrap)."""
    digits = []
    t = int(target)
    for _ in range(dim):
        digits.append(t % 31)
        t //= 31
    assert t == 0, "target needs more digits than dim"
    return np.array(digits[::-1], np.uint8)


def batch(rows: int, dim: int, seed: int, dup: float = 0.0) -> np.ndarray:
    """Random codes; a fraction ``dup`` of the rows are copies of earlier rows."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (rows, dim), dtype=np.uint8)
    if dup > 0 and rows > 1:
        r = np.nonzero(rng.random(rows) < dup)[0]
        r = r[r > 0]
        src = (rng.random(r.size) * r).astype(np.int64)      # an earlier row each
        for a, b in zip(r, src):                               # in order: a copy of a copy stays a copy
            codes[a] = codes[b]
    return codes

"""GPU suite of the store deduplication: dllm_hash_rows / dllm_dedup_rows / dllm_gather_rows and the
Python layer over them, bit for bit against the restatements of tests/dedup_ref.py.  Everything is
integer arithmetic, so every comparison is ``==``.

Sizes the kernels turn on: a piece is 16 bytes cut at the 16-byte boundaries of memory; rows of up to
256 codes take 4 lanes each (64 bytes per trip), up to 2048 codes 16 lanes (256 bytes per trip), longer
ones a whole wave (1024 bytes per trip); a group of lanes has 4 rows in flight and a hash workgroup is
4 waves, i.e. 256, 64 or 16 rows; a buffer of under 31 bytes goes to a serial kernel; the filter's
scan blocks hold 1024 rows."""
import functools

import numpy as np
import pytest

from tests import dedup_ref as ref

pytestmark = pytest.mark.gpu

DIMS = [1, 3, 15, 16, 17, 31, 63, 64, 65, 255, 256, 257, 768, 769, 1023, 1025, 4097, 65535]
ROWS = [1, 2, 63, 64, 65, 1025]


def u64(t):
    """The u64 value of an int64 tensor of hash or sequence bits."""
    return t.cpu().numpy().view(np.uint64)


def dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def case(rows, dim):
    """(codes, hashes): computed once, never written to."""
    codes = ref.batch(rows, dim, seed=rows * 100003 + dim)
    out = codes, ref.hash_rows(codes)
    for a in out:
        a.setflags(write=False)
    return out


def check_filter(got, want):
    keep, first, kept_rows, n_kept = got
    wk, wf, wr, wn = want
    assert keep.cpu().numpy().astype(np.uint8).tolist() == wk.tolist()
    assert np.array_equal(u64(first), wf)
    assert kept_rows.dtype.itemsize == 4 and np.array_equal(kept_rows.cpu().numpy(), wr)
    assert int(n_kept.item()) == wn


# ---- rule 1: the hash -------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_hash_every_dim(dllm, cuda, dim):
    rows = 3 if dim == 65535 else 37          # ld = dim: an odd dim puts row starts on every residue mod 16
    codes, want = case(rows, dim)
    assert np.array_equal(u64(dllm.hash_rows(dev(codes))), want)
    assert int(want[rows - 1]) == ref.hash_fold(codes[rows - 1])       # the serial fold, on one row


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dim", [17, 769, 2100])                          # one dim per group width
def test_hash_every_row_count(dllm, cuda, rows, dim):
    codes, want = case(rows, dim)
    assert np.array_equal(u64(dllm.hash_rows(dev(codes))), want)


def test_hash_every_alignment(dllm, cuda):
    """ld = dim = 769 over 40 rows starts a row on every residue mod 16; the same rows inside wider
    rows (ld = 800); the same again from a base address 1, 7 and 13 bytes into a larger buffer."""
    import torch
    rows, dim = 40, 769
    codes, want = case(rows, dim)
    d = dev(codes)
    assert {(d.data_ptr() + r * dim) % 16 for r in range(rows)} == set(range(16))
    assert np.array_equal(u64(dllm.hash_rows(d)), want)
    wide = torch.full((rows, 800), 0xEE, dtype=torch.uint8, device="cuda")
    wide[:, :dim] = d
    view = wide[:, :dim]
    assert view.stride(0) == 800 and view.data_ptr() == wide.data_ptr()
    assert np.array_equal(u64(dllm.hash_rows(view)), want)
    for off in (1, 7, 13):
        for ld in (dim, 800):
            big = torch.full((rows * ld + 64,), 0xEE, dtype=torch.uint8, device="cuda")
            v = big[off:off + rows * ld].view(rows, ld)[:, :dim]
            v.copy_(d)
            assert v.data_ptr() == big.data_ptr() + off
            assert np.array_equal(u64(dllm.hash_rows(v)), want), (off, ld)
    for sdim in (5, 64, 200, 2100):           # the other group widths, from an odd address
        c, w = case(37, sdim)
        big = torch.zeros(37 * sdim + 32, dtype=torch.uint8, device="cuda")
        v = big[3:3 + 37 * sdim].view(37, sdim)
        v.copy_(dev(c))
        assert np.array_equal(u64(dllm.hash_rows(v)), w), sdim


@pytest.mark.parametrize("dim", [16, 64, 257, 769, 2100])
def test_hash_byte_patterns(dllm, cuda, dim):
    """All zero (hashes to 0), all 0xFF, one nonzero byte at each of the first and last 17 positions,
    random bytes."""
    pos = sorted(set(range(min(17, dim))) | set(range(max(dim - 17, 0), dim)))
    codes = np.zeros((3 + len(pos), dim), np.uint8)
    codes[1] = 0xFF
    codes[2] = ref.batch(1, dim, seed=dim)[0]
    for i, p in enumerate(pos):
        codes[3 + i, p] = 1 + (37 * p) % 255
    want = ref.hash_rows(codes)
    got = u64(dllm.hash_rows(dev(codes)))
    assert got[0] == 0 and int(got[1]) == ref.hash_fold(codes[1])
    assert np.array_equal(got, want)
    assert np.array_equal(got, ref.hash_rows_loop(codes))
    assert len(set(got[3:].tolist())) == len(pos)                         # every position has a weight of its own


# ---- rule 2: the filter -----------------------------------------------------------------------------

def test_reserved_key(dllm, cuda):
    """2^64 - 1 marks an empty slot, so a row hashing to it lives in a word of its own: built from its
    13 base-31 digits, offered twice beside the all-zero row (hash 0) offered twice; one-shot, on a
    table, and again on that table."""
    top, zero = ref.row_with_hash(2 ** 64 - 1, 13), np.zeros(13, np.uint8)
    codes = dev(np.stack([top, zero, top, zero]))
    assert u64(dllm.hash_rows(codes)).tolist() == [2 ** 64 - 1, 0, 2 ** 64 - 1, 0]
    buf = dllm.DedupBuffer(16)
    for got in (dllm.dedup_rows(codes), buf.filter(codes)):
        keep, first, kept, n = got
        assert keep.tolist() == [True, True, False, False] and u64(first).tolist() == [0, 1, 0, 1]
        assert kept.tolist() == [0, 1, -1, -1] and int(n) == 2
    keep, first, kept, n = buf.filter(codes)
    assert not keep.any() and u64(first).tolist() == [0, 1, 0, 1] and int(n) == 0 and kept.tolist() == [-1] * 4
    assert buf.seen() == 2 and not buf.overflowed()


def test_collision_follows_the_reference(dllm, cuda):
    """[1, 31] and [2, 0] differ and both hash to 62: the later one is dropped, first points at the earlier."""
    codes = dev(np.array([[1, 31], [2, 0], [2, 1]], np.uint8))
    assert u64(dllm.hash_rows(codes)).tolist() == [62, 62, 63]
    keep, first, kept, n = dllm.dedup_rows(codes)
    assert keep.tolist() == [True, False, True] and u64(first).tolist() == [0, 0, 2]
    assert kept.tolist() == [0, 2, -1] and int(n) == 2


def test_first_occurrence_order(dllm, cuda):
    """The same row at indices 0, 1000 and 2047 of 2048 keeps index 0 only; one row repeated 4096
    times (every thread on one slot) keeps row 0."""
    codes = ref.batch(2048, 24, seed=5).copy()
    codes[1000] = codes[2047] = codes[0]
    got = dllm.dedup_rows(dev(codes))
    check_filter(got, ref.filter_loop(ref.hash_rows(codes)))
    keep, first = got[0].cpu().numpy(), u64(got[1])
    assert keep[0] and not keep[1000] and not keep[2047] and first[1000] == 0 and first[2047] == 0
    assert int(got[3]) == 2046
    same = np.repeat(ref.batch(1, 24, seed=6), 4096, axis=0)
    keep, first, kept, n = dllm.dedup_rows(dev(same))
    assert int(n) == 1 and int(kept[0]) == 0 and (kept[1:] == -1).all()
    assert keep.sum().item() == 1 and bool(keep[0]) and (u64(first) == 0).all()


@pytest.mark.parametrize("rows", [1, 64, 65, 1024, 1025, 2049])
def test_filter_batch_shapes(dllm, cuda, rows):
    """Across the scan's block boundaries, with no duplicates, with half and with nearly all."""
    for dup in (0.0, 0.5, 0.97):
        codes = ref.batch(rows, 9, seed=rows, dup=dup)
        h = ref.hash_rows(codes)
        want = ref.filter_loop(h)
        got = dllm.dedup_rows(dev(codes))
        check_filter(got, want)
        if dup == 0.0:
            assert want[3] == rows and got[2].tolist() == list(range(rows))
        else:
            assert (got[2][want[3]:] == -1).all()                          # the -1 tail
    check_filter(dllm.dedup_rows(dev(codes)), ref.dedup(h))                # the second restatement, once


def test_filter_state(dllm, cuda):
    """Three calls on one table with overlapping content; then calls 2 and 3 in the other order: what
    is kept in all is the same set of hashes, `first` and which call keeps a shared row change."""
    pool = ref.batch(300, 12, seed=8)
    rng = np.random.default_rng(9)
    calls = [pool[rng.integers(0, 300, n)] for n in (700, 1100, 1500)]
    results = {}
    for order in ((0, 1, 2), (0, 2, 1)):
        buf, seen, base, kept_hashes = dllm.DedupBuffer(4096), {}, 0, []
        for c in order:
            h = ref.hash_rows(calls[c])
            want = ref.filter_loop(h, base, seen)
            got = buf.filter(dev(calls[c]))
            check_filter(got, want)
            kept_hashes.append(set(h[want[2][:want[3]]].tolist()))
            base += len(h)
        assert buf.base == base == 3300 and buf.seen() == len(seen) and not buf.overflowed()
        results[order] = kept_hashes
    a, b = results[(0, 1, 2)], results[(0, 2, 1)]
    assert a[0] == b[0] and a[0] | a[1] | a[2] == b[0] | b[1] | b[2]       # the union does not depend on the order
    assert a[1] != b[2] and a[1] | a[2] == b[1] | b[2]                     # who keeps a shared row does


def test_filter_table_half_full_and_reset(dllm, cuda):
    """max_rows = 512 -> 1024 slots: exactly 512 rows are accepted, one more is rejected before
    anything runs; reset() forgets."""
    codes = dev(ref.batch(512, 7, seed=10))
    buf = dllm.DedupBuffer(512)
    assert buf.slots == 1024
    want = ref.filter_loop(ref.hash_rows(codes.cpu().numpy()))
    check_filter(buf.filter(codes), want)
    assert buf.seen() == want[3] == 512
    with pytest.raises(dllm.InvalidParams):
        buf.filter(codes[:1])
    assert buf.base == 512 and buf.seen() == 512
    buf.reset()
    assert buf.base == 0 and buf.seen() == 0
    check_filter(buf.filter(codes), want)


def test_filter_is_deterministic(dllm, cuda):
    """The same call on two fresh tables: identical outputs (once; no loop)."""
    codes = dev(ref.batch(3000, 6, seed=11, dup=0.6))
    a = dllm.DedupBuffer(3000).filter(codes)
    b = dllm.DedupBuffer(3000).filter(codes)
    for x, y in zip(a, b):
        assert (x == y).all()


# ---- rule 3: the gather -----------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 17, 768, 769])
def test_gather(dllm, cuda, dim):
    import torch
    rows = 70
    codes = ref.batch(rows, dim, seed=dim, dup=0.5)
    d = dev(codes)
    keep, first, kept, n = dllm.dedup_rows(d)
    want = ref.filter_loop(ref.hash_rows(codes))
    out = torch.full((rows, dim), 0xA5, dtype=torch.uint8, device="cuda")
    dllm.gather_rows(d, kept, n, out=out)
    o = out.cpu().numpy()
    assert np.array_equal(o[:want[3]], codes[want[2][:want[3]]])
    assert (o[want[3]:] == 0xA5).all()                                     # rows past n_kept are untouched
    out.fill_(0xA5)                                                        # n_kept = 0 writes nothing
    dllm.gather_rows(d, kept, torch.zeros(1, dtype=torch.int32, device="cuda"), out=out)
    assert (out == 0xA5).all().item()


# ---- the Python layer -------------------------------------------------------------------------------

def test_store_vectors_on_a_prefill_batch(dllm, cuda):
    """An all-zero prefill batch (DiffusionPrefill::prefill hands the store zero embeddings): every
    record has the same codes and one is kept."""
    import torch
    x = torch.zeros(48, 64, device="cuda")
    codes, scales, zps = dllm.compress_vectors(x, 8)
    buf = dllm.DedupBuffer(256)
    ids, kc, ks, kz = dllm.store_vectors(buf, list(range(100, 148)), codes, scales, zps)
    assert ids.tolist() == [100] and kc.shape == (1, 64) and kc.is_contiguous()
    assert kc.untyped_storage().nbytes() == 64                            # one row's bytes, not a view of the batch's
    assert torch.equal(kc[0], codes[0])
    assert torch.equal(ks.view(torch.int32), scales[:1].view(torch.int32))
    assert torch.equal(kz.view(torch.int32), zps[:1].view(torch.int32))
    ids, kc, ks, kz = dllm.store_vectors(buf, list(range(200, 248)), codes, scales, zps)   # the next prefill: nothing new
    assert ids.numel() == 0 and kc.shape == (0, 64)
    assert buf.seen() == 1 and buf.base == 96


def test_vector_index_fed_through_the_filter(dllm, cuda):
    """Six distinct vectors, each stored five times: the unfiltered index answers a top-4 query with
    one vector four times over, the index fed through store_vectors with four different ones."""
    import torch
    dim, k = 32, 4
    base = torch.tensor(np.random.default_rng(12).standard_normal((6, dim)).astype(np.float32)).cuda()
    x = base.repeat(5, 1)                                                  # rows 0..29: vector r % 6
    ids = list(range(30))
    plain = dllm.VectorIndex(dim, 8)
    plain.insert_batch(ids, x)
    hits = plain.search(base[2], k)
    assert len({i % 6 for i, _ in hits}) == 1 and len({s for _, s in hits}) == 1   # the same vector k times
    codes, scales, zps = dllm.compress_vectors(x, 8)
    kept_ids, kc, ks, kz = dllm.store_vectors(dllm.DedupBuffer(64), ids, codes, scales, zps)
    assert kept_ids.tolist() == [0, 1, 2, 3, 4, 5]
    assert torch.equal(kc, codes[:6]) and torch.equal(ks, scales[:6]) and torch.equal(kz, zps[:6])
    filtered = dllm.VectorIndex(dim, 8)
    filtered.insert_batch(kept_ids.tolist(), x[kept_ids])                 # ids are the rows here
    hits = filtered.search(base[2], k)
    assert len(hits) == k and len({i for i, _ in hits}) == k and hits[0][0] == 2


def test_one_shot_entries_replay_from_a_graph(dllm, cuda):
    """hash, filter and gather captured once and replayed on new contents give the eager bits."""
    import torch
    rows, dim = 1500, 48
    a, b = ref.batch(rows, dim, seed=13, dup=0.5), ref.batch(rows, dim, seed=14, dup=0.9)
    static = dev(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                          # warm-up outside the capture
        dllm.gather_rows(static, *dllm.dedup_rows(static)[2:])
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        h = dllm.hash_rows(static)
        keep, first, kept, n = dllm.dedup_rows(static)
        out = dllm.gather_rows(static, kept, n)
    for codes in (b, a):
        static.copy_(dev(codes))
        g.replay()
        torch.cuda.synchronize()
        want = ref.filter_loop(ref.hash_rows(codes))
        assert np.array_equal(u64(h), ref.hash_rows(codes))
        check_filter((keep, first, kept, n), want)
        assert np.array_equal(out.cpu().numpy()[:want[3]], codes[want[2][:want[3]]])
        eager = dllm.dedup_rows(static)
        for x, y in zip((keep, first, kept, n), eager):
            assert (x == y).all()

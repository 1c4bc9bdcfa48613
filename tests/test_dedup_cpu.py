"""CPU suite of the store deduplication (include/dllm_quant.h, section 8i): the two restatements of
the rules (tests/dedup_ref.py) agree, the host entry points dllm_hash_rows_host / dllm_dedup_rows_host
/ dllm_gather_rows_host match them bit for bit (one-shot and across calls on one table, the reserved
key and the full-table flag included), the C entry points reject what the header says they reject
before any device work, and the Python surface is exported.  No GPU work here."""
import ctypes as C

import numpy as np
import pytest

from tests import dedup_ref as ref
from tests.host_check import run_host_check

# one byte; below, at and above a 16-byte piece; the 64- and 256-byte group edges; the default hidden
# size and its odd neighbour; a second trip of a 64-lane group (1025); many trips; the largest dim.
DIMS = [1, 3, 15, 16, 17, 31, 63, 64, 65, 255, 256, 257, 768, 769, 1023, 1025, 4097, 65535]


def host_hash(L, codes, dim=None, ld=None):
    codes = np.ascontiguousarray(codes, np.uint8)
    rows = codes.shape[0]
    ld = codes.shape[1] if ld is None else ld
    dim = codes.shape[1] if dim is None else dim
    h = np.full(rows, 77, np.uint64)
    assert L.dllm_hash_rows_host(codes.ctypes.data, rows, dim, ld, h.ctypes.data) == 0, L.dllm_last_error()
    return h


class HostTable:
    def __init__(self, L, slots):
        self.L, self.slots = L, slots
        assert L.dllm_dedup_table_bytes(slots) == (4 + 2 * slots) * 8
        self.words = np.zeros(4 + 2 * slots, np.uint64)
        assert L.dllm_dedup_table_init_host(self.words.ctypes.data, slots) == 0


def host_filter(L, hashes, base=0, table=None):
    hashes = np.ascontiguousarray(hashes, np.uint64)
    rows = hashes.size
    keep, first = np.full(rows, 7, np.uint8), np.full(rows, 7, np.uint64)
    kept, n = np.full(rows, 7, np.int32), np.full(1, 7, np.uint32)
    rc = L.dllm_dedup_rows_host(hashes.ctypes.data, rows, base, table.words.ctypes.data if table else None,
                                table.slots if table else 0, keep.ctypes.data, first.ctypes.data, kept.ctypes.data,
                                n.ctypes.data)
    assert rc == 0, L.dllm_last_error()
    return keep, first, kept, int(n[0])


def same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g), np.asarray(w)), (g, w)


# ---- the restatements -------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [d for d in DIMS if d <= 4097])
def test_hash_restatements_agree(dim):
    codes = ref.batch(3, dim, seed=dim)
    codes[1] = 0
    codes[2] = 255
    assert np.array_equal(ref.hash_rows(codes), ref.hash_rows_loop(codes))
    assert ref.hash_fold(codes[1]) == 0


def test_hash_known_values():
    assert ref.hash_fold([1, 31]) == 62 and ref.hash_fold([2, 0]) == 62        # the issue's collision
    assert ref.hash_fold([7]) == 7 and ref.hash_fold([1, 0, 0]) == 961
    top = ref.row_with_hash(2 ** 64 - 1, 13)
    assert top.max() <= 30 and ref.hash_fold(top) == 2 ** 64 - 1 and int(ref.hash_rows(top[None])[0]) == 2 ** 64 - 1
    # the fold wraps: 14 digits of 30 exceed 2^64
    assert ref.hash_fold([30] * 14) == (31 ** 14 - 1) % 2 ** 64 == int(ref.hash_rows(np.full((1, 14), 30))[0])


@pytest.mark.parametrize("rows,dup", [(1, 0.0), (40, 0.0), (40, 0.5), (300, 0.95)])
def test_filter_restatements_agree(rows, dup):
    h = ref.hash_rows(ref.batch(rows, 5, seed=rows, dup=dup))
    same(ref.dedup(h), ref.filter_loop(h))
    seen_a, seen_b, base = {}, ref.Seen(), 0
    for call in range(3):                                    # overlapping content across three calls
        hc = np.concatenate([h[call::2], ref.hash_rows(ref.batch(7, 5, seed=100 + call))])
        same(ref.dedup(hc, base, seen_b), ref.filter_loop(hc, base, seen_a))
        base += hc.size


# ---- the host entry points --------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_host_hash_matches_restatements(dllm, dim):
    L = dllm._lib.load()
    rows = 3 if dim == 65535 else 5
    codes = ref.batch(rows, dim, seed=dim + 1)
    codes[1], codes[2] = 0, 255
    want = ref.hash_rows(codes)
    assert np.array_equal(host_hash(L, codes), want)
    assert int(want[0]) == ref.hash_fold(codes[0]) and int(want[2]) == ref.hash_fold(codes[2])
    if dim > 1:       # a row stride wider than the row: the bytes between rows do not count
        assert np.array_equal(host_hash(L, codes, dim=dim - 1, ld=dim), ref.hash_rows(codes[:, :dim - 1]))


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 1025])
def test_host_hash_every_row_count(dllm, rows):
    codes = ref.batch(rows, 17, seed=rows)
    assert np.array_equal(host_hash(dllm._lib.load(), codes), ref.hash_rows(codes))


@pytest.mark.parametrize("rows,dup", [(1, 0.0), (64, 0.0), (65, 0.5), (1025, 0.5), (2049, 0.99)])
def test_host_filter_one_shot(dllm, rows, dup):
    L = dllm._lib.load()
    h = ref.hash_rows(ref.batch(rows, 4, seed=rows, dup=dup))
    want = ref.filter_loop(h)
    same(host_filter(L, h), want)
    same(host_filter(L, h, table=HostTable(L, 8192)), want)   # an empty table gives the one-shot answer
    if dup == 0.0:
        assert want[3] == rows


def test_host_filter_collision_follows_the_reference(dllm):
    """Rows [1, 31] and [2, 0] differ and both hash to 62: the later one is dropped, first points at
    the earlier."""
    L = dllm._lib.load()
    codes = np.array([[1, 31], [2, 0], [2, 1]], np.uint8)
    h = host_hash(L, codes)
    assert h.tolist() == [62, 62, 63]
    keep, first, kept, n = host_filter(L, h)
    assert keep.tolist() == [1, 0, 1] and first.tolist() == [0, 0, 2] and kept.tolist() == [0, 2, -1] and n == 2


def test_host_filter_reserved_key(dllm):
    """The row that hashes to 2^64 - 1 (the key that marks an empty slot) and the all-zero row, each
    offered twice, in one call and again in a second."""
    L = dllm._lib.load()
    top, zero = ref.row_with_hash(2 ** 64 - 1, 13), np.zeros(13, np.uint8)
    codes = np.stack([top, zero, top, zero])
    h = host_hash(L, codes)
    assert h.tolist() == [2 ** 64 - 1, 0, 2 ** 64 - 1, 0]
    t = HostTable(L, 16)
    for got in (host_filter(L, h), host_filter(L, h, table=t)):
        assert got[0].tolist() == [1, 1, 0, 0] and got[1].tolist() == [0, 1, 0, 1]
        assert got[2].tolist() == [0, 1, -1, -1] and got[3] == 2
    keep, first, kept, n = host_filter(L, h, base=4, table=t)
    assert keep.tolist() == [0, 0, 0, 0] and first.tolist() == [0, 1, 0, 1] and n == 0 and (kept == -1).all()
    assert int(t.words[0]) == 0 and int(t.words[1]) == 2


def test_host_filter_three_calls_on_one_table(dllm):
    L = dllm._lib.load()
    pool = ref.batch(60, 6, seed=3)
    rng = np.random.default_rng(4)
    calls = [ref.hash_rows(pool[rng.integers(0, 60, n)]) for n in (50, 33, 70)]
    t, seen, base = HostTable(L, 512), {}, 0
    for hc in calls:
        same(host_filter(L, hc, base, t), ref.filter_loop(hc, base, seen))
        base += hc.size
    assert int(t.words[1]) == len(seen) and int(t.words[0]) == 0
    # exactly half full is accepted; one row more is not
    t2 = HostTable(L, 64)
    h32 = np.arange(100, 132, dtype=np.uint64)
    assert host_filter(L, h32, 0, t2)[3] == 32
    k = np.zeros(1, np.uint8)
    f, kr, n = np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros(1, np.uint32)
    assert L.dllm_dedup_rows_host(h32.ctypes.data, 1, 32, t2.words.ctypes.data, 64, k.ctypes.data, f.ctypes.data,
                                  kr.ctypes.data, n.ctypes.data) == dllm._lib.ERR_INVALID_PARAMS
    assert b"slots / 2" in L.dllm_last_error()


def test_host_full_table_sets_the_flag(dllm):
    """A caller who understates `base` can fill the table: the flag word goes up, the rows without a
    slot come back keep = 0 with first = 2^64 - 1, and every earlier entry still answers."""
    L = dllm._lib.load()
    t = HostTable(L, 8)
    for c in range(2):
        assert host_filter(L, np.arange(10 + 4 * c, 14 + 4 * c, dtype=np.uint64), 0, t)[3] == 4
    assert int(t.words[0]) == 0 and int(t.words[1]) == 8
    keep, first, kept, n = host_filter(L, np.array([50, 10, 51, 17], np.uint64), 0, t)
    assert keep.tolist() == [0, 0, 0, 0] and n == 0
    assert first.tolist() == [ref.NOSEQ, 0, ref.NOSEQ, 3]
    assert int(t.words[0]) == 1 and int(t.words[1]) == 8


def test_host_gather(dllm):
    L = dllm._lib.load()
    for dim, ld in [(1, 1), (17, 17), (769, 800)]:
        wide = ref.batch(9, ld, seed=dim)
        kept = np.array([0, 3, 4, 8, -1, -1, -1, -1, -1], np.int32)
        for n in (0, 4):
            out = np.full((9, dim), 0xA5, np.uint8)
            cnt = np.array([n], np.uint32)
            assert L.dllm_gather_rows_host(wide.ctypes.data, dim, ld, kept.ctypes.data, cnt.ctypes.data,
                                           out.ctypes.data, dim) == 0
            assert np.array_equal(out[:n], wide[kept[:n], :dim]) and (out[n:] == 0xA5).all()


# ---- the error contract, through the C entry points, nothing launched -----------------------------------

def test_hash_and_gather_rejections(dllm):
    L = dllm._lib.load()
    INV, SHAPE = dllm._lib.ERR_INVALID_PARAMS, dllm._lib.ERR_SHAPE_MISMATCH
    p = C.c_void_p(4096)       # never dereferenced: every call below returns before a launch
    assert L.dllm_hash_rows(None, 4, 8, 8, p, None) == INV and b"NULL" in L.dllm_last_error()
    assert L.dllm_hash_rows(p, 4, 8, 8, None, None) == INV
    assert L.dllm_hash_rows(p, 4, 0, 8, p, None) == INV and b"between 1 and 65535" in L.dllm_last_error()
    assert L.dllm_hash_rows(p, 4, 65536, 65536, p, None) == INV
    assert L.dllm_hash_rows(p, 4, 8, 7, p, None) == INV and b"ld" in L.dllm_last_error()
    assert L.dllm_hash_rows(p, 2 ** 31, 8, 8, p, None) == SHAPE
    assert L.dllm_hash_rows(p, 4, 8, 8, C.c_void_p(4100), None) == INV       # hashes not 8-byte aligned
    assert L.dllm_hash_rows(None, 0, 8, 8, None, None) == 0
    assert L.dllm_hash_rows_host(None, 4, 8, 8, p) == INV
    assert L.dllm_hash_rows_host(p, 4, 0, 8, p) == INV and L.dllm_hash_rows_host(p, 4, 8, 7, p) == INV
    assert L.dllm_hash_rows_host(None, 0, 8, 8, None) == 0
    for bad in (dict(codes=None), dict(kept=None), dict(n=None), dict(out=None), dict(dim=0), dict(dim=65536, ld=65536),
                dict(ld=7), dict(out_ld=7)):
        a = dict(codes=p, dim=8, ld=8, kept=p, n=p, out=p, out_ld=8)
        a.update(bad)
        assert L.dllm_gather_rows(a["codes"], a["dim"], a["ld"], a["kept"], a["n"], a["out"], a["out_ld"], None) == INV, bad
        assert L.dllm_gather_rows_host(a["codes"], a["dim"], a["ld"], a["kept"], a["n"], a["out"], a["out_ld"]) == INV, bad


def test_filter_rejections(dllm):
    L = dllm._lib.load()
    INV, SHAPE = dllm._lib.ERR_INVALID_PARAMS, dllm._lib.ERR_SHAPE_MISMATCH
    p = C.c_void_p(4096)
    assert L.dllm_dedup_table_bytes(1024) == (4 + 2048) * 8
    assert L.dllm_dedup_table_bytes(0) == 0 and L.dllm_dedup_table_bytes(1000) == 0
    assert L.dllm_dedup_table_init(p, 1000, None) == INV and b"power of two" in L.dllm_last_error()
    assert L.dllm_dedup_table_init(None, 1024, None) == INV
    assert L.dllm_dedup_table_init_host(p, 1000) == INV and L.dllm_dedup_table_init_host(None, 1024) == INV
    ws = L.dllm_dedup_workspace(100)
    assert ws == 16 + (4 + 2 * 256) * 8 and ws % 16 == 0
    assert L.dllm_dedup_workspace(1025) == 16 + (4 + 2 * 4096) * 8          # two blocks of 1024 rows
    assert L.dllm_dedup_workspace(2 ** 31) == 0

    def call(h=p, rows=100, base=0, table=p, slots=1024, keep=p, first=p, kept=p, n=p, w=p, wb=ws):
        return L.dllm_dedup_rows(h, rows, base, table, slots, keep, first, kept, n, w, wb, None)

    for name in ("h", "keep", "first", "kept", "n", "w"):
        assert call(**{name: None}) == INV, name
        assert b"NULL" in L.dllm_last_error() or name == "w"
    assert call(slots=1000) == INV and b"power of two" in L.dllm_last_error()
    assert call(slots=128) == INV and b"slots / 2" in L.dllm_last_error()          # 100 > 64
    assert call(base=413) == INV and b"slots / 2" in L.dllm_last_error()           # 413 + 100 > 512
    assert call(base=2 ** 62) == INV
    assert call(wb=ws - 1) == INV and b"workspace" in L.dllm_last_error()
    assert call(table=None, slots=0, wb=ws - 1) == INV
    assert call(w=C.c_void_p(4100)) == INV
    assert call(rows=2 ** 31, wb=2 ** 62) == SHAPE
    assert call(rows=0) == 0                                                       # rows = 0: accepted, nothing launched
    assert call(rows=0, h=None, keep=None, first=None, kept=None, n=None, w=None, wb=0) == 0
    assert call(rows=0, table=None, slots=0) == 0
    assert call(rows=0, base=512) == 0 and call(rows=0, base=513) == INV           # the base contract holds with no rows too
    # the host mirror: the same checks, minus the workspace's
    def hcall(**k):
        a = dict(h=p, rows=100, base=0, table=p, slots=1024, keep=p, first=p, kept=p, n=p)
        a.update(k)
        return L.dllm_dedup_rows_host(*[a[x] for x in ("h", "rows", "base", "table", "slots", "keep", "first", "kept", "n")])

    assert hcall(slots=1000) == INV and hcall(slots=128) == INV and hcall(base=413) == INV and hcall(h=None) == INV
    assert hcall(rows=2 ** 31) == SHAPE and hcall(rows=0) == 0


# ---- the Python surface ---------------------------------------------------------------------------------

def test_wrappers_exported(dllm):
    for name in ("hash_rows", "dedup_rows", "gather_rows", "DedupBuffer", "store_vectors"):
        assert name in dllm.__all__ and callable(getattr(dllm, name))
    assert dllm.dedup.hash_rows is dllm.hash_rows
    assert "dedup" in dllm.__doc__
    with pytest.raises(dllm.InvalidParams):
        dllm.DedupBuffer(0)


# ---- the host entry points under the sanitizers -----------------------------------------------------------

def test_host_entry_points_under_sanitizers(tmp_path):
    """tests/cpp/dedup_host_check.cpp (its own main) with csrc/host_rules.cpp and error.cpp, compiled by
    g++ under the address and undefined-behaviour sanitizers (tests/host_check.py; no hipcc, no
    library) and run as a program of its own: exact-size heap buffers at every kind of dim, rows that end
    at the buffer's last byte, the reserved key, a table filled through a dishonest base."""
    run_host_check("dedup_host_check", tmp_path, timeout=120)



def test_cpp_mirror_dedup_buffer(dllm, tmp_path):
    """tests/cpp/dedup_mirror_check.cpp (its own main) drives include/dllm_quant.hpp's
    io_dedup::DedupBuffer: compute_hash, the collision pair, a second call on the same buffer, the
    capacity check, an all-zero prefill.  Host entry points only."""
    import os
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    lib = dllm._lib.LIB_PATH.parent
    exe = tmp_path / "dedup_mirror_check"
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", f"-I{root / 'include'}",
           str(root / "tests" / "cpp" / "dedup_mirror_check.cpp"), f"-L{lib}", "-ldllm_hip", f"-Wl,-rpath,{lib}",
           "-o", str(exe)]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout

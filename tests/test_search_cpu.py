"""CPU suite of the compressed-vector search: the two restatements of the score rule
(tests/search_ref.py) agree bit for bit, the host entry points dllm_search_table_host /
dllm_search_vectors_host match them bit for bit, the rule stays within the header's derived bound
of the f64 cosine of the decompressed rows, the C entry points reject what the header says they
reject before any device work, and VectorIndex's id bookkeeping.  No GPU work here."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import search_ref as ref
from tests.host_check import run_host_check

# dim: one element; one group; a quarter trip; the trip edge from both sides and a strand's second
# trip; a ragged second trip that is no multiple of 4 (rows then start at odd byte offsets); 768.
DIMS = [1, 4, 64, 252, 256, 260, 263, 768]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(dim, rows=5, nq=2):
    """(Q, codes, scales, zps, table, scores): computed once, never written to."""
    codes, scales, zps = ref.store(rows, dim, seed=dim)
    Q = np.random.default_rng(1000 + dim).standard_normal((nq, dim)).astype(np.float32)
    tab = ref.table(codes, scales, zps)
    out = Q, codes, scales, zps, tab, ref.scores(Q, codes, tab)
    for a in out:
        a.setflags(write=False)
    return out


def host_table(L, codes, scales, zps):
    codes, scales, zps = (np.ascontiguousarray(a) for a in (codes, scales, zps))
    rows, dim = codes.shape
    tab = np.zeros((rows, 2), np.float32)
    assert L.dllm_search_table_host(codes.ctypes.data, rows, dim, scales.ctypes.data, zps.ctypes.data,
                                    tab.ctypes.data) == 0
    return tab


def host_search(L, Q, codes, tab, k):
    Q, codes, tab = (np.ascontiguousarray(a) for a in (Q, codes, tab))
    nq, (rows, dim) = Q.shape[0], codes.shape
    idx = np.full((nq, k), 77, np.int32)
    sc = np.full((nq, k), 77, np.float32)
    rc = L.dllm_search_vectors_host(Q.ctypes.data, nq, codes.ctypes.data if rows else None,
                                    tab.ctypes.data if rows else None, rows, dim, k, idx.ctypes.data, sc.ctypes.data)
    assert rc == 0, L.dllm_last_error()
    return idx, sc


# ---- the restatements -------------------------------------------------------------------------------

def test_fma_emulation_is_one_rounding():
    """fma32 against the exact rational form, on operands that force every kind of alignment:
    addends far above, far below and level with the product, and sums that cancel."""
    rng = np.random.default_rng(5)
    n = 4000
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))).astype(np.float32)
    y = np.where(rng.random(n) < 0.5, rng.integers(0, 256, n), rng.standard_normal(n) * 1e3).astype(np.float32)
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-60, 60, n))).astype(np.float32)
    a[::7] = (-x[::7].astype(np.float64) * y[::7]).astype(np.float32)       # cancellation to the last bits
    a[::11] = (x[::11].astype(np.float64) * y[::11] * 2.0 ** 25).astype(np.float32)  # product near half an ulp of a
    got = ref.fma32(x, y, a)
    want = np.array([ref.fma_loop(*t) for t in zip(x, y, a)], np.float32)
    assert np.array_equal(bits(got), bits(want))
    # A case where rounding the f64 sum to f32 rounds twice: x y = 2^23 - 2^-23 and a = 2^47 + 2^24
    # (odd significand, ulp 2^24) sum to 2^-23 below the midpoint a + 2^23.  f64 rounds the sum onto
    # the midpoint, and ties-to-even then goes up; one rounding stays at a.
    x1, y1, a1 = np.float32(2.0 ** 12 + 2.0 ** -11), np.float32(2.0 ** 11 - 2.0 ** -12), np.float32(2.0 ** 47 + 2.0 ** 24)
    assert float(x1) * float(y1) == 2.0 ** 23 - 2.0 ** -23
    assert np.float32(float(x1) * float(y1) + float(a1)) != a1          # the naive emulation is wrong here
    assert bits(ref.fma32(x1, y1, a1)) == bits(a1) and bits(ref.fma_loop(x1, y1, a1)) == bits(a1)
    assert bits(ref.fma32(-x1, y1, -a1)) == bits(-a1)


@pytest.mark.parametrize("dim", [1, 4, 252, 260, 263])
def test_restatements_agree(dim):
    Q, codes, scales, zps, tab, sc = case(dim, rows=3)
    assert np.array_equal(bits(tab), bits(ref.table_loop(codes, scales, zps)))
    assert np.array_equal(bits(sc), bits(ref.scores_loop(Q, codes, tab)))
    for k in (1, 3, 5):
        a, b = ref.topk(sc, k), ref.topk_loop(sc, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("mask", ref.MASKS)
def test_restatements_agree_on_order_patterns(mask):
    """... and on the queries whose sums move with the order (so the GPU tests' reference is itself
    checked where it is most likely to be wrong)."""
    dim = 520
    codes, scales, zps = ref.store(2, dim, seed=3)
    Q = ref.order_pattern(2, dim, seed=1, mask=mask)
    tab = ref.table(codes, scales, zps)
    assert np.array_equal(bits(ref.scores(Q, codes, tab)), bits(ref.scores_loop(Q, codes, tab)))


def test_order_patterns_tell_orders_apart():
    """The patterns do what they are for: a plain left-to-right sum, and a tree with the levels in
    the opposite order, change the bits of their strand sums."""
    dim = 768
    Q = ref.order_pattern(8, dim, seed=0)
    ones = np.ones((1, dim), np.float32)
    pinned = ref.strand_sums(Q, ones)[:, 0]
    serial = np.array([np.cumsum(q, dtype=np.float32)[-1] for q in Q], np.float32)
    g = ref._groups(Q, np.float32)
    a = np.zeros((8, 64), np.float32)
    for t in range(g.shape[1]):
        for l in range(4):
            a = a + g[:, t, :, l]
    i, m = np.arange(64), 1
    while m < 64:                      # m = 1 .. 32 instead of 32 .. 1
        a = a + a[:, i ^ m]
        m *= 2
    assert (bits(pinned) != bits(serial)).any()
    assert (bits(pinned) != bits(a[:, 0])).any()


# ---- the host entry points --------------------------------------------------------------------------

@pytest.mark.parametrize("dim", DIMS)
def test_host_matches_restatement(dllm, dim):
    L = dllm._lib.load()
    Q, codes, scales, zps, tab, sc = case(dim)
    got_tab = host_table(L, codes, scales, zps)
    assert np.array_equal(bits(got_tab), bits(tab))
    for k in (1, 5, 8):
        idx, out = host_search(L, Q, codes, got_tab, k)
        want_idx, want = ref.topk(sc, k)
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(bits(out), bits(want))


def test_host_order_patterns(dllm):
    L = dllm._lib.load()
    dim = 775
    codes, scales, zps = ref.store(4, dim, seed=9)
    tab = ref.table(codes, scales, zps)
    for mask in ref.MASKS:
        Q = ref.order_pattern(3, dim, seed=2, mask=mask)
        idx, out = host_search(L, Q, codes, tab, 4)
        want_idx, want = ref.topk(ref.scores(Q, codes, tab), 4)
        assert np.array_equal(idx, want_idx) and np.array_equal(bits(out), bits(want)), mask


def test_host_slice_invariance(dllm):
    """A score depends on its query and row alone: rows [1, 4) searched on their own give the bits
    they have inside the whole store."""
    L = dllm._lib.load()
    Q, codes, scales, zps, tab, sc = case(260)
    idx, out = host_search(L, Q, codes[1:4], host_table(L, codes[1:4], scales[1:4], zps[1:4]), 3)
    for j in range(Q.shape[0]):
        assert np.array_equal(bits(out[j]), bits(sc[j, 1:4][idx[j]]))


# ---- the bound --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["normal", "offset"])
def test_rule_within_derived_bound(kind):
    """|score - f64 cosine of the decompressed row| <= (6 T + 20) 2^-24 kappa + 2^-51 kappa^3."""
    rows, dim, nq = 48, 768, 4
    rng = np.random.default_rng(11)
    if kind == "normal":
        codes, scales, zps = ref.store(rows, dim, seed=11)
    else:            # row values in [10, 10.1]: the zero point carries the row, v Qs the score
        x = (10.0 + 0.1 * rng.random((rows, dim))).astype(np.float32)
        zps = x.min(axis=1)
        scales = ((x.max(axis=1) - zps) / np.float32(255)).astype(np.float32)
        codes = np.clip((x - zps[:, None]) / scales[:, None], 0, 255).astype(np.uint8)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    sc = ref.scores(Q, codes, ref.table(codes, scales, zps))
    exact = ref.cosine_f64(Q, ref.decompress(codes, scales, zps))
    kap = ref.kappa(codes, scales, zps)
    err = np.abs(sc.astype(np.float64) - exact)
    lim = ref.bound(dim, kap)[None, :]
    print(kind, "max err", err.max(), "min bound", lim.min(), "kappa", kap.min(), kap.max())
    assert (kap >= 1.0 - 1e-12).all()
    assert (err <= lim).all()
    assert lim.max() < 1e-3      # the bound says something


# ---- ranking edge cases (host entry point and restatement) ----------------------------------------------

def test_duplicate_rows_tie_to_the_lower_index(dllm):
    L = dllm._lib.load()
    Q, codes, scales, zps, _, _ = case(64)
    codes, scales, zps = np.repeat(codes[:2], 3, axis=0), np.repeat(scales[:2], 3), np.repeat(zps[:2], 3)
    tab = host_table(L, codes, scales, zps)
    idx, out = host_search(L, Q, codes, tab, 6)
    for j in range(Q.shape[0]):
        first = idx[j, 0] // 3
        assert idx[j].tolist() == [3 * first, 3 * first + 1, 3 * first + 2, 3 * (1 - first), 3 * (1 - first) + 1,
                                   3 * (1 - first) + 2]
        assert len(set(bits(out[j, :3]).tolist())) == 1
    want_idx, want = ref.topk(ref.scores(Q, codes, ref.table(codes, scales, zps)), 6)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(out), bits(want))


def test_zero_query_scores_zero_in_index_order(dllm):
    L = dllm._lib.load()
    _, codes, scales, zps, tab, _ = case(64)
    idx, out = host_search(L, np.zeros((1, 64), np.float32), codes, tab, 4)
    assert idx[0].tolist() == [0, 1, 2, 3] and (out == 0).all() and not np.signbit(out).any()


def test_constant_and_zero_rows(dllm):
    """scale 0: a constant row is its zero point (cosine = sum q / (|q| sqrt(dim)) sign(z)); an
    all-zero row has no direction and scores 0."""
    L = dllm._lib.load()
    dim = 64
    Q = np.random.default_rng(2).standard_normal((2, dim)).astype(np.float32)
    codes = np.zeros((3, dim), np.uint8)
    codes[2] = 9
    scales = np.array([0.0, 0.0, 0.0], np.float32)
    zps = np.array([2.5, 0.0, -1.0], np.float32)
    tab = host_table(L, codes, scales, zps)
    assert np.array_equal(bits(tab), bits(ref.table(codes, scales, zps)))
    idx, out = host_search(L, Q, codes, tab, 3)
    want_idx, want = ref.topk(ref.scores(Q, codes, tab), 3)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(out), bits(want))
    for j in range(2):
        by_row = dict(zip(idx[j].tolist(), out[j].tolist()))
        c = Q[j].astype(np.float64).sum() / (np.linalg.norm(Q[j].astype(np.float64)) * np.sqrt(dim))
        assert by_row[1] == 0.0
        assert abs(by_row[0] - c) < 1e-5 and abs(by_row[2] + c) < 1e-5


def test_k_beyond_rows_fills_the_tail(dllm):
    L = dllm._lib.load()
    Q, codes, scales, zps, tab, sc = case(4)
    idx, out = host_search(L, Q, codes, tab, 9)
    assert (idx[:, 5:] == -1).all() and np.isneginf(out[:, 5:]).all()
    assert sorted(idx[0, :5].tolist()) == [0, 1, 2, 3, 4]
    want_idx, want = ref.topk(sc, 9)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(out), bits(want))
    # an empty store: every slot is the tail
    idx, out = host_search(L, Q, codes[:0], tab[:0], 3)
    assert (idx == -1).all() and np.isneginf(out).all()


def test_nan_scores_rank_last(dllm):
    """A NaN in a query makes every score of that query NaN: they rank below -inf, by index; a NaN
    scale does the same to one row, which then comes last."""
    L = dllm._lib.load()
    Q, codes, scales, zps, tab, _ = case(64)
    Q = Q.copy()
    Q[1, 17] = np.nan
    idx, out = host_search(L, Q, codes, tab, 5)
    assert np.isnan(out[1]).all() and idx[1].tolist() == [0, 1, 2, 3, 4]
    assert np.isfinite(out[0]).all()
    scales = scales.copy()
    scales[2] = np.nan
    tab2 = host_table(L, codes, scales, zps)
    idx, out = host_search(L, Q[:1], codes, tab2, 5)
    assert idx[0, 4] == 2 and np.isnan(out[0, 4]) and np.isfinite(out[0, :4]).all()
    want_idx, _ = ref.topk(ref.scores(Q[:1], codes, ref.table(codes, scales, zps)), 5)
    assert np.array_equal(idx, want_idx)


def test_signed_zero_and_infinities_rank():
    """The key order itself: -0 ties with +0 (index decides), NaN below -inf."""
    sc = np.array([[-0.0, 0.0, np.nan, -np.inf, np.inf, 1.0, -1.0, 0.0]], np.float32)
    idx, out = ref.topk(sc, 8)
    assert idx[0].tolist() == [4, 5, 0, 1, 7, 6, 3, 2]
    assert np.array_equal(idx, ref.topk_loop(sc, 8)[0])
    assert np.signbit(out[0, 2]) and not np.signbit(out[0, 3])     # the score bits come back as they are


# ---- the error contract, through the C entry points, nothing launched -----------------------------------

def test_search_vectors_rejections(dllm):
    L = dllm._lib.load()
    INV, SHAPE = dllm._lib.ERR_INVALID_PARAMS, dllm._lib.ERR_SHAPE_MISMATCH
    p = C.c_void_p(4096)       # never dereferenced: every call below returns before a launch
    ws = L.dllm_search_workspace(2, 10, 3)

    def call(Q=p, nq=2, codes=p, table=p, rows=10, dim=8, k=3, idx=p, scores=p, w=p, wb=ws):
        return L.dllm_search_vectors(Q, nq, codes, table, rows, dim, k, idx, scores, w, wb, None)

    for name in ("Q", "codes", "table", "idx", "scores", "w"):
        assert call(**{name: None}) == INV, name
        assert b"NULL" in L.dllm_last_error() or name == "w"
    assert call(k=0) == INV and call(k=257) == INV
    assert b"between 1 and 256" in L.dllm_last_error()
    assert call(dim=0) == INV and call(dim=65536) == INV
    assert call(wb=ws - 1) == INV and b"workspace" in L.dllm_last_error()
    assert call(rows=2 ** 31, wb=2 ** 62) == SHAPE
    assert call(nq=0) == 0
    assert call(nq=0, Q=None, idx=None, scores=None, w=None, wb=0) == 0
    # k is checked first, then dim, then rows
    assert call(k=0, dim=0, rows=2 ** 31) == INV and call(dim=0, rows=2 ** 31) == INV


def test_search_table_and_host_rejections(dllm):
    L = dllm._lib.load()
    INV, SHAPE = dllm._lib.ERR_INVALID_PARAMS, dllm._lib.ERR_SHAPE_MISMATCH
    p = C.c_void_p(4096)
    assert L.dllm_search_table(None, 4, 8, p, p, p, None) == INV
    assert L.dllm_search_table(p, 4, 8, None, p, p, None) == INV
    assert L.dllm_search_table(p, 4, 8, p, None, p, None) == INV
    assert L.dllm_search_table(p, 4, 8, p, p, None, None) == INV
    assert L.dllm_search_table(p, 4, 0, p, p, p, None) == INV
    assert L.dllm_search_table(p, 4, 65536, p, p, p, None) == INV
    assert L.dllm_search_table(p, 2 ** 31, 8, p, p, p, None) == SHAPE
    assert L.dllm_search_table(None, 0, 8, None, None, None, None) == 0
    assert L.dllm_search_table_host(None, 4, 8, p, p, p) == INV
    assert L.dllm_search_table_host(p, 4, 0, p, p, p) == INV
    assert L.dllm_search_table_host(p, 2 ** 31, 8, p, p, p) == SHAPE
    assert L.dllm_search_vectors_host(None, 1, p, p, 4, 8, 2, p, p) == INV
    assert L.dllm_search_vectors_host(p, 1, p, p, 4, 8, 0, p, p) == INV
    assert L.dllm_search_vectors_host(p, 1, p, p, 4, 8, 257, p, p) == INV
    assert L.dllm_search_vectors_host(p, 1, p, p, 4, 65536, 2, p, p) == INV
    assert L.dllm_search_vectors_host(p, 1, p, p, 2 ** 31, 8, 2, p, p) == SHAPE
    assert L.dllm_search_vectors_host(None, 0, None, None, 4, 8, 2, None, None) == 0


def test_workspace_query(dllm):
    """Scores f32 [nq][rows] + two floats per query, each rounded up to 16 bytes, + the candidate
    keys of the select passes (slices of 2048 keys, k u64 survivors each, until one slice is left)."""
    L = dllm._lib.load()
    up = lambda b: -(-b // 16) * 16
    assert L.dllm_search_workspace(1, 10, 3) == 16 + up(40)
    assert L.dllm_search_workspace(3, 2048, 256) == up(24) + up(3 * 2048 * 4)
    assert L.dllm_search_workspace(3, 2049, 256) == up(24) + up(3 * 2049 * 4) + 3 * 2 * 256 * 8
    n1 = 513 * 256                                  # 513 slices of 256 survivors -> 65 slices -> 9 -> 2 -> 1
    assert L.dllm_search_workspace(1, 2048 * 512 + 1, 256) == 16 + up((2048 * 512 + 1) * 4) + n1 * 8 + 65 * 256 * 8
    for nq, rows, k in [(1, 1, 1), (5, 4101, 256), (16, 1 << 20, 10)]:
        assert L.dllm_search_workspace(nq, rows, k) % 16 == 0
        assert L.dllm_search_workspace(nq, rows, k) >= nq * rows * 4


# ---- the Python surface ---------------------------------------------------------------------------------

def test_wrappers_exported(dllm):
    for name in ("search_vectors", "search_table", "VectorIndex"):
        assert name in dllm.__all__ and callable(getattr(dllm, name))
    assert dllm.search.search_vectors is dllm.search_vectors
    assert "search" in dllm.__doc__
    with pytest.raises(dllm.InvalidParams):
        dllm.VectorIndex(0, 8)
    with pytest.raises(dllm.InvalidParams):
        dllm.VectorIndex(16, 9)


def test_vector_index_bookkeeping(dllm):
    """Rows of ids without a device: new ids append, a stored id keeps its row (replacement), an id
    repeated in a batch keeps its last vector, a missing id looks up as -1."""
    ix = dllm.VectorIndex(16, 8)
    assert len(ix) == 0 and ix.size_bytes() == 0
    assert ix._assign([7, 3, 11]) == ([0, 1, 2], [0, 1, 2])
    assert ix._assign([3, 20]) == ([1, 3], [0, 1])
    assert len(ix) == 4
    assert ix._assign([5, 7, 5]) == ([0, 4], [1, 2])          # 7 replaces row 0; the second 5 is the one written
    assert len(ix) == 5
    assert ix._lookup([11, 99, 5, 7]) == [2, -1, 4, 0]
    # prefill_kv.rs:135-139: data.len() + the key string's bytes
    assert ix.size_bytes() == 5 * 16 + len("7") + len("3") + len("11") + len("20") + len("5")


# ---- the host entry points under the sanitizers -----------------------------------------------------------

def test_host_entry_points_under_sanitizers(tmp_path):
    """tests/cpp/search_host_check.cpp (its own main) with csrc/host_rules.cpp and error.cpp, compiled by
    g++ under the address and undefined-behaviour sanitizers (tests/host_check.py; no hipcc, no
    library): exact-size heap buffers at every kind of dim, k beyond rows, an empty store."""
    run_host_check("search_host_check", tmp_path, timeout=120)

"""Two independent restatements of the row-against-row cosine rule (include/dllm_quant.h, section 8l):
a vectorised numpy f64 one (the reference of the host and GPU tests) and a plain loop on Python ints
and floats (Python's float is IEEE f64 with one rounding per operation), plus the ranking with its
drops.  A helper module shared by the CPU and the GPU tests.

Rule: per row C1 = sum c, C2 = sum c^2 (integers); nb2 = ((s s) C2 + ((2 s) z) C1) + (z z) dim in f64;
w = 1 / sqrt(nb2) if s, z, nb2 finite and nb2 > 0 else 0; a = s w, b = z w.  Per pair D = sum c_r c_t
(integer); score = f32(((a_r a_t) D + ((a_r b_t) C1_r + (b_r a_t) C1_t)) + (b_r b_t) dim).  A pair is
dropped if it is the query's own row (self_base + j == t) or !(score >= threshold).  Rank: score
descending (-0 = +0), row index ascending; dropped pairs and places past the end are -1 / -inf."""
import math
from fractions import Fraction

import numpy as np

f32 = np.float32

# The opaque table as the library lays it out (24 bytes per row), for the tests that hand a numpy
# table to the host entry points or compare a device table with the reference.
ENTRY = np.dtype([("a", "<f8"), ("b", "<f8"), ("c1", "<u4"), ("pad", "<u4")])


# ---- vectorised ---------------------------------------------------------------------------------------

def table(codes, scales, zps):
    """-> (a f64 [rows], b f64 [rows], C1 int64 [rows])."""
    c = np.asarray(codes, np.uint8).astype(np.int64)
    dim = c.shape[1]
    c1, c2 = c.sum(axis=1), (c * c).sum(axis=1)
    s, z = np.asarray(scales, np.float32).astype(np.float64), np.asarray(zps, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        nb2 = ((s * s) * c2.astype(np.float64) + ((2.0 * s) * z) * c1.astype(np.float64)) + (z * z) * np.float64(dim)
        ok = np.isfinite(s) & np.isfinite(z) & np.isfinite(nb2) & (nb2 > 0)
        w = np.where(ok, 1.0 / np.sqrt(np.where(ok, nb2, 1.0)), 0.0)
        a = np.where(ok, s * w, 0.0)
        b = np.where(ok, z * w, 0.0)
    return a, b, c1


def table_bytes(tab):
    """The reference table in the library's layout."""
    a, b, c1 = tab
    out = np.zeros(len(a), ENTRY)
    out["a"], out["b"], out["c1"] = a, b, c1
    return out


def dots(qcodes, codes):
    """D [nq, rows] as f64, exact: every product and partial sum is an integer below 2^32 < 2^53, so the
    f64 matrix product has no rounding whatever order it sums in."""
    return np.asarray(qcodes, np.uint8).astype(np.float64) @ np.asarray(codes, np.uint8).astype(np.float64).T


def scores(qcodes, qtab, codes, tab):
    """-> [nq, rows] f32."""
    dim = np.float64(np.asarray(codes).shape[1])
    D = dots(qcodes, codes)
    (ar, br, c1r), (at, bt, c1t) = qtab, tab
    ar, br, c1r = ar[:, None], br[:, None], c1r.astype(np.float64)[:, None]
    at, bt, c1t = at[None, :], bt[None, :], c1t.astype(np.float64)[None, :]
    cross = (ar * bt) * c1r + (br * at) * c1t
    return (((ar * at) * D + cross) + (br * bt) * dim).astype(np.float32)


def keys(sc):
    sc = np.asarray(sc, np.float32)
    b = sc.view(np.uint32).copy()
    b[b == 0x80000000] = 0
    o = np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    idx = np.broadcast_to(np.arange(sc.shape[-1], dtype=np.uint32), sc.shape)
    return (o.astype(np.uint64) << np.uint64(32)) | (~idx).astype(np.uint64)


def rank(sc, k, threshold=-np.inf, self_base=-1):
    """sc [nq, rows] -> (idx int32 [nq, k], scores f32 [nq, k]) with the drops applied."""
    sc = np.asarray(sc, np.float32)
    nq, rows = sc.shape
    idx = np.full((nq, k), -1, np.int32)
    out = np.full((nq, k), -np.inf, np.float32)
    if not rows:
        return idx, out
    assert not np.isnan(sc).any()
    ky = keys(sc)
    drop = ~(sc >= f32(threshold))
    if self_base >= 0:
        j = np.arange(nq)
        drop[j, self_base + j] = True
    ky[drop] = 0
    order = np.argsort(ky, axis=1, kind="stable")[:, ::-1][:, :k]
    kept = np.take_along_axis(ky, order, axis=1) != 0
    n = order.shape[1]
    idx[:, :n] = np.where(kept, order, -1)
    out[:, :n] = np.where(kept, np.take_along_axis(sc, order, axis=1), -np.inf)
    return idx, out


def neighbors(qcodes, qscales, qzps, codes, scales, zps, k, threshold=-np.inf, self_base=-1):
    """The reference of dllm_neighbor_rows: -> (idx, scores, full score matrix)."""
    sc = scores(qcodes, table(qcodes, qscales, qzps), codes, table(codes, scales, zps))
    return rank(sc, k, threshold, self_base) + (sc,)


# ---- plain loop on Python ints and floats ---------------------------------------------------------------

def table_loop(codes, scales, zps):
    out = []
    for r, row in enumerate(codes):
        c1 = sum(int(c) for c in row)
        c2 = sum(int(c) * int(c) for c in row)
        s, z = float(f32(scales[r])), float(f32(zps[r]))
        a = b = 0.0
        if math.isfinite(s) and math.isfinite(z):
            try:
                nb2 = ((s * s) * float(c2) + ((2.0 * s) * z) * float(c1)) + (z * z) * float(len(row))
            except OverflowError:
                nb2 = math.inf
            if math.isfinite(nb2) and nb2 > 0.0:
                w = 1.0 / math.sqrt(nb2)
                a, b = s * w, z * w
        out.append((a, b, c1))
    return out


def scores_loop(qcodes, qtab, codes, tab):
    dim = len(codes[0])
    out = np.zeros((len(qcodes), len(codes)), np.float32)
    for j, q in enumerate(qcodes):
        ar, br, c1r = qtab[j]
        for t, row in enumerate(codes):
            at, bt, c1t = tab[t]
            D = sum(int(x) * int(y) for x, y in zip(q, row))
            cross = (ar * bt) * float(c1r) + (br * at) * float(c1t)
            out[j, t] = f32(((ar * at) * float(D) + cross) + (br * bt) * float(dim))
    return out


def rank_loop(sc, k, threshold=-np.inf, self_base=-1):
    idx = np.full((len(sc), k), -1, np.int32)
    out = np.full((len(sc), k), -np.inf, np.float32)
    for j, row in enumerate(sc):
        live = [t for t in range(len(row)) if not (self_base >= 0 and self_base + j == t) and row[t] >= f32(threshold)]
        for i, t in enumerate(sorted(live, key=lambda t: (-float(row[t]), t))[:k]):      # -0.0 == 0.0
            idx[j, i], out[j, i] = t, row[t]
    return idx, out


# ---- the exact cosine and the bound ---------------------------------------------------------------------

def _sqrt_fraction(v, digits=50):
    """sqrt of a Fraction to `digits` decimal digits, as a Fraction."""
    scale = 10 ** (2 * digits)
    return Fraction(math.isqrt(v.numerator * scale // v.denominator), 10 ** digits)


def cosine_exact(qrow, qs, qz, row, s, z):
    """The cosine of the algebraic vectors s c + z (s, z the f32 values, exact rationals)."""
    qs, qz, s, z = (Fraction(float(f32(x))) for x in (qs, qz, s, z))
    u = [qs * int(c) + qz for c in qrow]
    v = [s * int(c) + z for c in row]
    dot = sum(x * y for x, y in zip(u, v))
    n2 = sum(x * x for x in u) * sum(y * y for y in v)
    return float(dot / _sqrt_fraction(n2))


def kappa(codes, scales, zps):
    """(|s| |c|_2 + |z| sqrt(dim)) / |s c + z|_2 per row."""
    c = np.asarray(codes, np.float64)
    s, z = np.asarray(scales, np.float64), np.asarray(zps, np.float64)
    v = s[:, None] * c + z[:, None]
    return (np.abs(s) * np.linalg.norm(c, axis=1) + np.abs(z) * np.sqrt(c.shape[1])) / np.linalg.norm(v, axis=1)


def bound(kr, kt):
    """The header's first-order bound on |score - exact cosine|."""
    u = 2.0 ** -53
    return 2.0 ** -25 + 12 * u * kr * kt + 2.0 ** -51 * (kr ** 3 + kt ** 3) / 2


# ---- test data ------------------------------------------------------------------------------------------

def store(rows, dim, seed=0, bits=8, kind="normal"):
    """A store as compress_vector writes it, without a device: scale = (max - min) / (2^bits - 1), zero
    point = min, codes by truncation.  kind: N(0,1) rows, or rows in [10, 10.1]."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        x = rng.standard_normal((rows, dim)).astype(np.float32)
    else:
        x = (10.0 + 0.1 * rng.random((rows, dim))).astype(np.float32)
    lo, hi = x.min(axis=1), x.max(axis=1)
    scales = ((hi - lo) / f32((1 << bits) - 1)).astype(np.float32)
    with np.errstate(all="ignore"):
        codes = np.where(scales[:, None] > 0, (x - lo[:, None]) / scales[:, None], 0)
    codes = np.clip(np.nan_to_num(codes), 0, (1 << bits) - 1).astype(np.uint8)
    return codes, scales, lo.astype(np.float32)

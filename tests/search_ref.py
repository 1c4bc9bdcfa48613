"""Two independent restatements of the search score rule (include/dllm_quant.h, section 8g): a
vectorised numpy one (the reference of the host and GPU tests) and a plain loop over scalars that
walks strands and tree levels one by one in exact rational arithmetic.  A helper module shared by
the CPU and the GPU tests.

Rule: element d belongs to strand (d / 4) % 64; a strand's partial starts at +0 and takes its d
ascending with a = fma(x_d, y_d, a); the 64 partials combine by a[i] = a[i] + a[i ^ m], m = 32 .. 1.
A = strand sum of q_d float(c_d), Qs of q_d 1, Qn of q_d q_d.  Row table in f64: nb2 = ((s s) C2 +
((2 s) z) C1) + (z z) dim, w = nb2 > 0 ? f32(1 / sqrt(nb2)) : 0, (u, v) = (s w, z w) in f32.
wq = Qn > 0 ? 1 / sqrt(Qn) : 0 in f32.  score = fma(u, A, v Qs) wq.  Rank: score descending (-0 = +0,
NaN below -inf), then row index ascending.

The fused multiply-add.  Python 3.10 has no math.fma, so the vectorised form emulates it through f64
and is exact, not "nearly": every product formed here is exact in f64 (a 24-bit by a 24-bit
significand needs 48 bits; f64 has 53, and its exponent range holds every f32 product).  The sum
p + a is then taken with Knuth's branch-free TwoSum, whose error term e is exact, and the f64 sum is
replaced by its round-to-odd neighbour whenever e != 0 (truncate toward zero, then set the last
bit).  Rounding a round-to-odd value of precision >= 24 + 2 to f32 gives the correctly rounded f32
of the exact value (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums: proved
algorithms using rounding to odd", 2008), so no double rounding can occur.  The loop form does not
share this code: it rounds an exact Fraction to f32 with integer arithmetic."""
from fractions import Fraction

import numpy as np

STRANDS = 64
TRIP = 4 * STRANDS
f32 = np.float32


# ---- vectorised -----------------------------------------------------------------------------------

def fma32(x, y, a):
    """RN_f32(x y + a) for f32 arrays (one rounding)."""
    x, y, a = (np.asarray(t, np.float32).astype(np.float64) for t in (x, y, a))
    with np.errstate(over="ignore", invalid="ignore"):
        p = x * y                                   # exact
        s = p + a
        bb = s - p
        e = (p - (s - bb)) + (a - bb)               # exact: s + e == p + a
        odd = np.isfinite(s) & np.isfinite(e) & (e != 0)
        bits = np.ascontiguousarray(s).view(np.uint64).copy()
        toward_zero = odd & ((e > 0) != (s > 0))    # the exact sum is smaller in magnitude than s
        bits[toward_zero] -= np.uint64(1)
        bits[odd] |= np.uint64(1)
        return bits.view(np.float64).astype(np.float32)


def _tree(a):
    """[..., 64] -> [...]: a[i] = a[i] + a[i ^ m], m = 32 .. 1."""
    i = np.arange(STRANDS)
    m = STRANDS // 2
    while m:
        a = a + a[..., i ^ m]
        m //= 2
    return a[..., 0]


def _groups(x, dtype):
    """[n, dim] -> [n, trips, 64, 4] with zeros past dim (q = 0, c = 0 leave a partial unchanged)."""
    x = np.asarray(x)
    n, dim = x.shape
    trips = -(-dim // TRIP)
    pad = np.zeros((n, trips * TRIP), dtype)
    pad[:, :dim] = x
    return pad.reshape(n, trips, STRANDS, 4)


def strand_sums(X, Y):
    """X [n, dim] f32, Y [m, dim] f32 -> [n, m] f32: the strand sum of X[i, d] Y[j, d]."""
    gx, gy = _groups(X, np.float32), _groups(Y, np.float32)
    a = np.zeros((gx.shape[0], gy.shape[0], STRANDS), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(gx.shape[1]):
            for l in range(4):
                a = fma32(gx[:, None, t, :, l], gy[None, :, t, :, l], a)
        return _tree(a)


def query_stats(Q):
    """Q [nq, dim] -> (Qs [nq], wq [nq]) f32."""
    Q = np.asarray(Q, np.float32)
    ones = np.ones((1, Q.shape[1]), np.float32)
    qs = strand_sums(Q, ones)[:, 0]
    qn = np.array([strand_sums(Q[j:j + 1], Q[j:j + 1])[0, 0] for j in range(Q.shape[0])], np.float32)
    with np.errstate(all="ignore"):
        wq = np.where(qn > 0, f32(1.0) / np.sqrt(qn, dtype=np.float32), f32(0.0)).astype(np.float32)
    return qs, wq


def table(codes, scales, zps):
    """-> [rows, 2] f32 (u, v)."""
    c = np.asarray(codes, np.uint8).astype(np.uint64)
    dim = c.shape[1] if c.ndim == 2 else 0
    c1 = c.sum(axis=1).astype(np.float64)
    c2 = (c * c).sum(axis=1).astype(np.float64)
    sf, zf = np.asarray(scales, np.float32), np.asarray(zps, np.float32)
    s, z = sf.astype(np.float64), zf.astype(np.float64)
    with np.errstate(all="ignore"):
        nb2 = ((s * s) * c2 + ((2.0 * s) * z) * c1) + (z * z) * np.float64(dim)
        w = np.where(nb2 > 0, (1.0 / np.sqrt(nb2)).astype(np.float32), f32(0.0)).astype(np.float32)
        return np.stack([sf * w, zf * w], axis=1).astype(np.float32)


def scores(Q, codes, tab):
    """-> [nq, rows] f32."""
    Q = np.asarray(Q, np.float32)
    A = strand_sums(Q, np.asarray(codes, np.uint8).astype(np.float32))
    qs, wq = query_stats(Q)
    with np.errstate(all="ignore"):
        vq = (tab[None, :, 1] * qs[:, None]).astype(np.float32)
        return (fma32(np.broadcast_to(tab[None, :, 0], A.shape), A, vq) * wq[:, None]).astype(np.float32)


def keys(sc):
    """u64 keys whose descending order is the ranking: [..., rows]."""
    sc = np.asarray(sc, np.float32)
    b = sc.view(np.uint32).copy()
    b[b == 0x80000000] = 0
    o = np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    o[np.isnan(sc)] = 0
    idx = np.broadcast_to(np.arange(sc.shape[-1], dtype=np.uint32), sc.shape)
    return (o.astype(np.uint64) << np.uint64(32)) | (~idx).astype(np.uint64)


def topk(sc, k):
    """sc [nq, rows] -> (idx int32 [nq, k], scores f32 [nq, k]); tail -1 / -inf when k > rows."""
    sc = np.asarray(sc, np.float32)
    nq, rows = sc.shape
    idx = np.full((nq, k), -1, np.int32)
    out = np.full((nq, k), -np.inf, np.float32)
    if rows:
        order = np.argsort(keys(sc), axis=1, kind="stable")[:, ::-1][:, :k]
        idx[:, :order.shape[1]] = order
        out[:, :order.shape[1]] = np.take_along_axis(sc, order, axis=1)
    return idx, out


def search(Q, codes, scales, zps, k):
    """The reference of dllm_search_vectors: -> (idx, scores, full score matrix)."""
    sc = scores(Q, codes, table(codes, scales, zps))
    return topk(sc, k) + (sc,)


# ---- plain loop, exact rational arithmetic ------------------------------------------------------------

def _round_f32(v):
    """The f32 nearest to the Fraction v (ties to even), by integer arithmetic."""
    if v == 0:
        return f32(0.0)
    sign, v = (-1, -v) if v < 0 else (1, v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1                                        # 2^e <= v < 2^(e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(v, quantum)
    n = int(n)
    if 2 * rem > quantum or (2 * rem == quantum and n % 2):
        n += 1
    r = n * quantum
    if r >= Fraction(2) ** 128:
        return f32(sign * np.inf)
    return f32(sign * float(r))                       # exact: r is an f32 value


def fma_loop(x, y, a):
    x, y, a = float(x), float(y), float(a)
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(a)):
        with np.errstate(all="ignore"):
            return f32(np.float64(x) * np.float64(y) + np.float64(a))   # only its class matters
    v = Fraction(x) * Fraction(y) + Fraction(a)
    if v == 0:      # an exact zero is -0 only as (-0) + (-0)
        neg = (x == 0 or y == 0) and (np.signbit(x) != np.signbit(y)) and a == 0 and np.signbit(a)
        return f32(-0.0) if neg else f32(0.0)
    return _round_f32(v)


def strand_sum_loop(x, y):
    a = [f32(0.0)] * STRANDS
    for d in range(len(x)):
        s = (d // 4) % STRANDS
        a[s] = fma_loop(x[d], y[d], a[s])
    m = STRANDS // 2
    with np.errstate(all="ignore"):
        while m >= 1:
            a = [f32(a[i] + a[i ^ m]) for i in range(STRANDS)]
            m //= 2
    return a[0]


def table_loop(codes, scales, zps):
    out = np.zeros((len(codes), 2), np.float32)
    for r, row in enumerate(codes):
        c1 = sum(int(c) for c in row)
        c2 = sum(int(c) * int(c) for c in row)
        s, z = np.float64(scales[r]), np.float64(zps[r])
        with np.errstate(all="ignore"):
            nb2 = ((s * s) * np.float64(c2) + ((np.float64(2.0) * s) * z) * np.float64(c1)) + (z * z) * np.float64(len(row))
            w = f32(np.float64(1.0) / np.sqrt(nb2)) if nb2 > 0 else f32(0.0)
            out[r] = f32(scales[r]) * w, f32(zps[r]) * w
    return out


def scores_loop(Q, codes, tab):
    Q = np.asarray(Q, np.float32)
    out = np.zeros((len(Q), len(codes)), np.float32)
    for j, q in enumerate(Q):
        qs = strand_sum_loop(q, np.ones(len(q), np.float32))
        qn = strand_sum_loop(q, q)
        with np.errstate(all="ignore"):
            wq = f32(1.0) / np.sqrt(qn) if qn > 0 else f32(0.0)
            for r, row in enumerate(codes):
                A = strand_sum_loop(q, [f32(c) for c in row])
                out[j, r] = f32(fma_loop(tab[r, 0], A, f32(tab[r, 1] * qs)) * wq)
    return out


def topk_loop(sc, k):
    idx = np.full((len(sc), k), -1, np.int32)
    out = np.full((len(sc), k), -np.inf, np.float32)
    for j, row in enumerate(sc):
        def rank(r):
            s = row[r]
            return (2, 0.0, r) if np.isnan(s) else (1, -float(s), r)     # -0.0 == 0.0 compares equal
        for i, r in enumerate(sorted(range(len(row)), key=rank)[:k]):
            idx[j, i], out[j, i] = r, row[r]
    return idx, out


# ---- the exact cosine and the bound ---------------------------------------------------------------------

def cosine_f64(Q, rows_f32):
    """f64 cosine of each query with each decompressed row: [nq, rows]."""
    q, v = np.asarray(Q, np.float64), np.asarray(rows_f32, np.float64)
    return (q @ v.T) / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(v, axis=1)[None, :])


def kappa(codes, scales, zps):
    """The cancellation ratio of each row: (|s| |c|_2 + |z| sqrt(dim)) / |s c + z|_2."""
    c = np.asarray(codes, np.float64)
    s, z = np.asarray(scales, np.float64), np.asarray(zps, np.float64)
    v = s[:, None] * c + z[:, None]
    return (np.abs(s) * np.linalg.norm(c, axis=1) + np.abs(z) * np.sqrt(c.shape[1])) / np.linalg.norm(v, axis=1)


def bound(dim, kap):
    """The header's first-order bound on |score - exact cosine of the decompressed row|."""
    T = -(-dim // TRIP)
    return (6 * T + 20) * 2.0 ** -24 * kap + 2.0 ** -51 * kap ** 3


# ---- test data ------------------------------------------------------------------------------------------

MASKS = ("dense", "strands", "trips", "group")


def order_pattern(nq, dim, seed=0, mask="dense"):
    """Queries [nq, dim] f32 whose strand sums change bits under any reordering: random mantissas and
    signs with magnitudes 2^0 .. 2^20 on a geometric tail, so a few large terms carry each sum and
    the small ones survive only in the partials the pinned order forms before they meet a large one.
    The masks leave only the terms one stage of the order combines, which puts every rounding of that
    stage next to the total: "strands" one element per strand (the tree), "trips" strand 0's elements
    (a strand's chain over trips), "group" the first group of four (a strand's four components)."""
    rng = np.random.default_rng(seed)
    expo = np.minimum(rng.geometric(0.5, (nq, dim)) - 1, 20)
    x = (1.0 + rng.random((nq, dim))) * np.exp2(expo) * rng.choice([-1.0, 1.0], (nq, dim))
    d = np.arange(dim)
    strand, comp = (d // 4) % STRANDS, d % 4
    keep = {"dense": np.ones(dim, bool), "strands": (d < TRIP) & (comp == 0), "trips": strand == 0,
            "group": d < 4}[mask]
    return (x * keep).astype(np.float32)


def store(rows, dim, seed=0, bits=8):
    """A store as compress_vector (prefill_kv.rs:104-121) writes it, without a device: N(0,1) rows,
    scale = (max - min) / (2^bits - 1), zero point = min, codes by truncation.  Only its shape of
    data matters to these tests, not parity with the quantizer (tested elsewhere)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    lo, hi = x.min(axis=1), x.max(axis=1)
    scales = ((hi - lo) / f32((1 << bits) - 1)).astype(np.float32)
    with np.errstate(all="ignore"):
        codes = np.where(scales[:, None] > 0, (x - lo[:, None]) / scales[:, None], 0)
    codes = np.clip(np.nan_to_num(codes), 0, (1 << bits) - 1).astype(np.uint8)
    return codes, scales, lo.astype(np.float32)


def decompress(codes, scales, zps):
    """dequantize (prefill_kv.rs:62-66): x as f32 * scale + zero_point, two f32 roundings."""
    c = np.asarray(codes, np.uint8).astype(np.float32)
    return (c * np.asarray(scales, np.float32)[:, None] + np.asarray(zps, np.float32)[:, None]).astype(np.float32)

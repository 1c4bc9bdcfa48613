"""Two independent numpy restatements of the token sampling rule (include/dllm_quant.h, section 8j):
``sample`` is vectorised (``prepare`` a row once, ``pick`` any number of uniform triples from it),
``sample_loop`` is written as plain loops: its own Philox, a counting selection of the top-k
threshold, element-by-element folds and the literal first-j scan.  Both work on f32 arrays; an f16
input is widened exactly by the caller.  EXP and the halving tree are tests/token_ref.py's (the
readout's CPU suite checks EXP's two forms against each other); ``sample_loop(exact_exp=True)`` uses
that module's Fraction-based EXP, for small rows."""
import numpy as np

from tests import token_ref as ref
from tests.token_ref import CHUNK, LANES, QNAN, exp32, _tree

f32 = np.float32
TRIPS = CHUNK // (4 * LANES)
NINF = f32(-np.inf)
M32 = 0xFFFFFFFF
U_MAX = f32(1.0 - 2.0 ** -24)


def recip(temperature):
    """Rule 1's r = RN(1.0f / temperature)."""
    return f32(1.0) / f32(temperature)


# ---- vectorised -------------------------------------------------------------------------------------------

def philox(seed, idx):
    """Philox4x32-10, key (seed lo, seed hi), counters (i lo, i hi, 1, 0) for the u64 array idx -> u32 [n, 4]."""
    idx = np.asarray(idx, np.uint64)
    c = [idx & np.uint64(M32), idx >> np.uint64(32), np.full(idx.shape, 1, np.uint64), np.zeros(idx.shape, np.uint64)]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(M32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(M32)]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack(c, axis=-1).astype(np.uint32)


def uniforms(seed, offset, n):
    """Rule 4: f32 [n, 3], row b from the counter (offset + b) mod 2^64."""
    idx = np.array([(offset + b) % 2 ** 64 for b in range(n)], np.uint64)
    w = philox(seed, idx)[:, :3]
    return (w >> np.uint32(8)).astype(f32) * f32(2.0 ** -24)


def masked(x, temperature, top_k):
    """Rules 1 and 2: the tempered, masked row y (f32 [V]); NaNs stay where they are."""
    x = np.asarray(x, f32)
    r = recip(temperature)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (x * r).astype(f32)
    V = y.size
    if 0 < top_k < V and not np.isnan(y).any():
        tau = np.sort(y)[V - top_k]
        y = np.where(y >= tau, y, NINF).astype(f32)
    return y


class Row:
    """What rule 3 leaves of one row: m, Z, and the weights of the three levels."""

    def __init__(self, x, temperature=1.0, top_k=0):
        y = masked(x, temperature, top_k)
        self.V, self.y = y.size, y
        C = self.C = -(-self.V // CHUNK)
        pad = np.full(C * CHUNK, NINF, f32)
        pad[:self.V] = y
        pad = pad.reshape(C, CHUNK)
        self.ok = False
        self.m = self.Z = QNAN
        if np.isnan(y).any():
            return
        mc = pad.max(axis=1) + f32(0)
        m = mc.max()
        if np.isinf(m):
            return
        with np.errstate(invalid="ignore"):
            e = exp32(pad - mc[:, None])
        e[np.isneginf(mc)] = 0
        self.e = e.reshape(C, TRIPS, LANES, 4)                    # [chunk][trip][lane][component]
        s = np.zeros((C, LANES), f32)
        for k in range(TRIPS):
            for l in range(4):
                s = s + self.e[:, k, :, l]
        self.s = s                                               # the lane sums, before the tree
        Zc = _tree(s)
        with np.errstate(invalid="ignore"):
            self.w = np.where(np.isneginf(mc), f32(0), Zc * exp32(mc - m)).astype(f32)
        lanes = np.zeros(LANES, f32)
        for c in range(C):
            lanes[c % LANES] = lanes[c % LANES] + self.w[c]
        self.mc, self.m, self.Z, self.ok = mc, m, _tree(lanes), True


def _first(a, v):
    """Rule 5 for weights a [n, k] (one set per draw) and uniforms v [n]: the pick (-1 if none), per draw."""
    F = np.cumsum(a, axis=1, dtype=f32)
    with np.errstate(invalid="ignore"):
        t = (v * F[:, -1]).astype(f32)
        hit = t[:, None] < F
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1)


def pick(row, u):
    """Rules 5 to 7 on a prepared row for uniforms u [n, 3] -> tokens int32 [n], p_token f32 [n]."""
    u = np.asarray(u, f32).reshape(-1, 3)
    n = u.shape[0]
    tokens, p = np.full(n, -1, np.int32), np.full(n, QNAN, f32)
    if not row.ok:
        return tokens, p
    c = _first(np.broadcast_to(row.w, (n, row.C)), u[:, 0])
    live = c >= 0
    cs = np.where(live, c, 0)
    j = _first(row.s[cs], u[:, 1])
    live &= j >= 0
    js = np.where(live, j, 0)
    el = row.e[cs, :, js, :].reshape(n, 4 * TRIPS)                 # the lane's elements, q = 4 g' + comp
    q = _first(el, u[:, 2])
    live &= q >= 0
    qs = np.where(live, q, 0)
    idx = CHUNK * cs + 4 * (LANES * (qs // 4) + js) + qs % 4
    assert (idx[live] < row.V).all()
    tokens[live] = idx[live]
    p[live] = exp32(row.y[idx[live]] - row.m) / row.Z
    return tokens, p


def sample(x, temperature=1.0, top_k=0, seed=0, offset=0, u=None):
    """x f32 [M, V] -> tokens int32 [M], stats f32 [M, 3] = {m, Z, p_token}."""
    x = np.asarray(x, f32)
    M = x.shape[0]
    u = uniforms(seed, offset, M) if u is None else np.asarray(u, f32).reshape(M, 3)
    tokens, stats = np.zeros(M, np.int32), np.zeros((M, 3), f32)
    for b in range(M):
        row = Row(x[b], temperature, top_k)
        t, p = pick(row, u[b:b + 1])
        tokens[b], stats[b] = t[0], (row.m, row.Z, p[0])
    return tokens, stats


# ---- plain loops ------------------------------------------------------------------------------------------

def philox_loop(seed, i):
    c = [i & M32, (i >> 32) & M32, 1, 0]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def uniforms_loop(seed, i):
    return [f32(w >> 8) * f32(2.0 ** -24) for w in philox_loop(seed, i % 2 ** 64)[:3]]


def first_loop(a, v):
    """The literal scan: the first j with t < F_j, F the sequential fold from +0; -1 if none."""
    S = f32(0)
    for w in a:
        S = f32(S + w)
    with np.errstate(invalid="ignore"):
        t = f32(f32(v) * S)
    F = f32(0)
    for j, w in enumerate(a):
        F = f32(F + w)
        if t < F:
            return j
    return -1


def row_loop(x, temperature, top_k, u, exact_exp=False):
    """One row -> token, (m, Z, p_token)."""
    def EXP(d):
        return ref.exp_loop(d) if exact_exp else exp32(np.array([d], f32))[0]

    V = len(x)
    r = f32(f32(1.0) / f32(temperature))
    with np.errstate(over="ignore", invalid="ignore"):
        y = [f32(f32(v) * r) for v in x]
    bad = (-1, (QNAN, QNAN, QNAN))
    if any(v != v for v in y):
        return bad
    if 0 < top_k < V:
        tau = sorted(y, reverse=True)[top_k - 1]
        gt = ge = 0
        for v in y:                                                # the one value with #{>} < k <= #{>=}
            gt += v > tau
            ge += v >= tau
        assert gt < top_k <= ge
        y = [v if v >= tau else NINF for v in y]
    C = -(-V // CHUNK)
    mc, lane_sums = [], []
    ys = np.array(y, f32)
    for c in range(C):
        lo, hi = c * CHUNK, min(V, (c + 1) * CHUNK)
        mm = NINF
        for i in range(lo, hi):
            if y[i] > mm:
                mm = y[i]
        mm = f32(mm + f32(0))
        mc.append(mm)
        lane = [f32(0)] * LANES
        if not np.isinf(mm):
            ev = None if exact_exp else exp32(ys[lo:hi] - mm)
            for i in range(lo, hi):
                j = ((i - lo) // 4) % LANES
                lane[j] = f32(lane[j] + (EXP(f32(y[i] - mm)) if exact_exp else ev[i - lo]))
        lane_sums.append(lane)
    m = max(mc)
    if np.isinf(m):
        return bad
    w = [f32(0) if np.isneginf(mc[c]) else f32(ref._tree_loop(lane_sums[c]) * EXP(f32(mc[c] - m))) for c in range(C)]
    lane = [f32(0)] * LANES
    for c in range(C):
        lane[c % LANES] = f32(lane[c % LANES] + w[c])
    Z = ref._tree_loop(lane)
    none = (-1, (m, Z, QNAN))
    c = first_loop(w, u[0])
    if c < 0:
        return none
    j = first_loop(lane_sums[c], u[1])
    if j < 0:
        return none
    where = [CHUNK * c + 4 * (LANES * g + j) + comp for g in range(TRIPS) for comp in range(4)]
    q = first_loop([EXP(f32(y[i] - mc[c])) if i < V else f32(0) for i in where], u[2])
    if q < 0:
        return none
    tok = where[q]
    return tok, (m, Z, f32(EXP(f32(y[tok] - m)) / Z))


def sample_loop(x, temperature=1.0, top_k=0, seed=0, offset=0, u=None, exact_exp=False):
    x = np.asarray(x, f32)
    M = x.shape[0]
    tokens, stats = np.zeros(M, np.int32), np.zeros((M, 3), f32)
    for b in range(M):
        ub = uniforms_loop(seed, offset + b) if u is None else [f32(v) for v in np.asarray(u, f32).reshape(M, 3)[b]]
        tokens[b], stats[b] = row_loop([f32(v) for v in x[b]], temperature, top_k, ub, exact_exp)
    return tokens, stats


# ---- the distribution the rule samples --------------------------------------------------------------------

def softmax_masked_f64(x, temperature, top_k):
    """The f64 softmax of the masked y of one row."""
    y = masked(x, temperature, top_k).astype(np.float64)
    e = np.exp(y - y.max())
    return e / e.sum()


def chi2_z(counts, prob):
    """Pearson's statistic of counts [V] against prob [V]: bins with an expected count >= 5, the rest
    merged into one; returns (chi2, dof, z = (chi2 - dof) / sqrt(2 dof))."""
    n = counts.sum()
    exp = prob * n
    big = exp >= 5
    o = np.append(counts[big], counts[~big].sum()).astype(np.float64)
    e = np.append(exp[big], exp[~big].sum())
    keep = e > 0
    o, e = o[keep], e[keep]
    chi2 = float(((o - e) ** 2 / e).sum())
    dof = o.size - 1
    return chi2, dof, (chi2 - dof) / np.sqrt(2.0 * dof)

"""Two independent restatements of the top-p / min-p rule (include/dllm_quant.h, section 8k):
``tau`` is vectorised numpy (uint64 sums, a search on the cumulative masses, Python ints for the
96-bit comparison at the deciding places), ``tau_loop`` is a scalar loop that sorts the row and walks
it with Python ints.  Both give the combined threshold of 8k.5 of one row; ``sample`` / ``sample_loop``
then hand the masked row to tests/token_sample_ref.py, which owns EXP's use in {m, Z}, the uniforms and
the picks (a row that is already tempered and masked is sampled there at temperature 1 without a
mask: y * 1 is y to the bit)."""
import numpy as np

from tests import token_sample_ref as sr
from tests.token_ref import QNAN, exp32

f32 = np.float32
NINF = sr.NINF
ONE = 1 << 32


def pfix(top_p):
    """(u64) floor((double) top_p * 2^32); exact: an f32 times a power of two."""
    return int(np.floor(np.float64(f32(top_p)) * np.float64(2.0 ** 32)))


def mfix(min_p):
    """(u64) ceil((double) min_p * 2^32)."""
    return int(np.ceil(np.float64(f32(min_p)) * np.float64(2.0 ** 32)))


def tempered(x, temperature):
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(x, f32) * sr.recip(temperature)).astype(f32)


def degenerate(y):
    return bool(np.isnan(y).any() or np.isinf(y.max()))


# ---- vectorised -------------------------------------------------------------------------------------------

def weights(y, tau_k):
    """8k.2 for a row without a NaN and with a finite maximum: W u64 [V] and m."""
    m = f32(y.max() + f32(0))
    g = exp32(y - m)
    W = np.trunc(g.astype(np.float64) * 2.0 ** 32).astype(np.uint64)      # exact: 24 bits times 2^32
    W[~(y >= tau_k)] = 0
    return W, m


def tau_k_of(y, top_k):
    V = y.size
    return np.sort(y)[V - top_k] if 0 < top_k < V else NINF


class Prepared:
    """What does not depend on top_p and min_p of one row: y, tau_k, the weights, their cumulative sums
    down the sorted row.  ``tau(top_p, min_p)`` is the combined threshold (f32; NaN for a degenerate
    row, -inf when no mask is on)."""

    def __init__(self, x, temperature=1.0, top_k=0):
        y = self.y = tempered(x, temperature)
        self.bad = degenerate(y)
        if self.bad:
            return
        self.tk = tau_k_of(y, top_k)
        self.W, _ = weights(y, self.tk)
        self.T = int(self.W.sum(dtype=np.uint64))
        order = np.argsort(-y, kind="stable")
        ys, A = y[order], np.cumsum(self.W[order], dtype=np.uint64)
        last = np.flatnonzero(np.append(ys[1:] != ys[:-1], True))        # the last place of every distinct value
        self.values, self.Ag = ys[last], A[last]

    def tau(self, top_p=1.0, min_p=0.0):
        if self.bad:
            return QNAN
        out = [self.tk]
        if f32(top_p) != 1:
            Ag, target = self.Ag, pfix(top_p) * self.T
            j = int(np.searchsorted(Ag, np.uint64(-(-target // ONE)), side="left"))
            while j > 0 and (int(Ag[j - 1]) << 32) >= target:             # the 96-bit comparison decides
                j -= 1
            while (int(Ag[j]) << 32) < target:
                j += 1
            assert (int(Ag[j]) << 32) >= target and (j == 0 or (int(Ag[j - 1]) << 32) < target)
            out.append(self.values[j])
        if f32(min_p) != 0:
            out.append(self.y[self.W >= np.uint64(mfix(min_p))].min())
        return f32(max(out) + f32(0))


def tau(x, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    return Prepared(x, temperature, top_k).tau(top_p, min_p)


def mask(x, temperature, t):
    """The tempered row with everything below the threshold t turned into -inf."""
    y = tempered(x, temperature)
    if t != t or np.isneginf(t):
        return y
    return np.where(y >= t, y, NINF).astype(f32)


def row(x, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    """(token_sample_ref.Row of the masked row, tau)."""
    t = tau(x, temperature, top_k, top_p, min_p)
    return sr.Row(mask(x, temperature, t)), t


def sample(x, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=0, offset=0, u=None):
    """x f32 [M, V] -> tokens int32 [M], stats f32 [M, 4] = {m, Z, p_token, tau}."""
    x = np.asarray(x, f32)
    M = x.shape[0]
    u = sr.uniforms(seed, offset, M) if u is None else np.asarray(u, f32).reshape(M, 3)
    tokens, stats = np.zeros(M, np.int32), np.zeros((M, 4), f32)
    for b in range(M):
        r, t = row(x[b], temperature, top_k, top_p, min_p)
        tok, p = sr.pick(r, u[b:b + 1])
        tokens[b], stats[b] = tok[0], (r.m, r.Z, p[0], t)
    return tokens, stats


# ---- plain loops ------------------------------------------------------------------------------------------

class PreparedLoop:
    """The rule read aloud: the weights one by one, a walk down the sorted row, a minimum over a set."""

    def __init__(self, x, temperature=1.0, top_k=0):
        r = sr.recip(temperature)
        with np.errstate(over="ignore", invalid="ignore"):
            y = self.y = [f32(f32(v) * r) for v in x]
        V = self.V = len(y)
        self.bad = any(v != v for v in y) or bool(np.isinf(max(y)))
        if self.bad:
            return
        m = f32(max(y) + f32(0))
        self.tk = sorted(y, reverse=True)[top_k - 1] if 0 < top_k < V else NINF
        with np.errstate(invalid="ignore"):
            g = exp32(np.array(y, f32) - m)                               # EXP is token_ref's
        self.W = [int(float(gi) * 2.0 ** 32) if yi >= self.tk else 0 for gi, yi in zip(g, y)]
        self.T = sum(self.W)
        self.pairs = sorted(zip(y, self.W), key=lambda e: -e[0])

    def tau_p(self, top_p):
        P = int(float(f32(top_p)) * 2.0 ** 32)
        pairs, V = self.pairs, self.V
        A, i = 0, 0
        while True:
            j = i
            while j < V and pairs[j][0] == pairs[i][0]:
                A += pairs[j][1]
                j += 1
            if A * ONE >= P * self.T:
                return pairs[i][0]
            i = j

    def tau_m(self, min_p):
        q = float(f32(min_p)) * 2.0 ** 32
        Q = int(q) + (int(q) < q)
        return min(yi for yi, wi in zip(self.y, self.W) if wi >= Q)

    def tau(self, top_p=1.0, min_p=0.0):
        if self.bad:
            return QNAN
        best = self.tk
        if f32(top_p) != 1:
            best = max(best, self.tau_p(top_p))
        if f32(min_p) != 0:
            best = max(best, self.tau_m(min_p))
        return f32(best + f32(0))


def tau_loop(x, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    return PreparedLoop(x, temperature, top_k).tau(top_p, min_p)


def sample_loop(x, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=0, offset=0, u=None):
    x = np.asarray(x, f32)
    M = x.shape[0]
    tokens, stats = np.zeros(M, np.int32), np.zeros((M, 4), f32)
    for b in range(M):
        t = tau_loop(x[b], temperature, top_k, top_p, min_p)
        ub = sr.uniforms_loop(seed, offset + b) if u is None else [f32(v) for v in np.asarray(u, f32).reshape(M, 3)[b]]
        tokens[b], st = sr.row_loop([f32(v) for v in mask(x[b], temperature, t)], 1.0, 0, ub)
        stats[b] = (*st, t)
    return tokens, stats


def softmax_masked_f64(x, temperature, t):
    y = mask(x, temperature, t).astype(np.float64)
    e = np.exp(y - y.max())
    return e / e.sum()

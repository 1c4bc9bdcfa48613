"""Two independent restatements of dllm_noise_mse's summation order (include/dllm_quant.h): a
vectorised numpy one (the reference of the GPU tests) and a plain loop over np.float32 scalars that
walks lanes and tree levels one by one.  A helper module, shared by the CPU and the GPU tests.

Order, for one sample of n elements: d = RN(noise - pred), e = RN(d d); chunk c = elements
[16384 c, 16384 (c + 1)), elements past n are +0; groups of four go to 256 lanes round-robin; a
lane adds its groups in increasing order, components 0..3, from +0; the halving tree s[j] += s[j + h],
h = 128 .. 1, gives the chunk partial; the partials go to 256 lanes round-robin and through the same
tree; loss = RN(total / float32(n))."""
import numpy as np

CHUNK = 16384
LANES = 256
f32 = np.float32


def squared_errors(pred, noise):
    """e_i of every element: [B, n] f32.  pred f32 or f16 (widened exactly)."""
    p = np.asarray(pred).astype(np.float32)
    d = np.asarray(noise, np.float32) - p
    return d * d


# ---- vectorised ---------------------------------------------------------------------------------

def _tree(s):
    """[..., 256] -> [...]: the halving tree along the last axis."""
    h = LANES // 2
    while h:
        s = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def chunk_partials(e):
    """e [B, n] f32 -> P [B, C] f32."""
    e = np.asarray(e, np.float32)
    B, n = e.shape
    C = -(-n // CHUNK)
    pad = np.zeros((B, C * CHUNK), np.float32)
    pad[:, :n] = e
    g = pad.reshape(B, C, CHUNK // (4 * LANES), LANES, 4)      # [b, c, trip, lane, component]
    s = np.zeros((B, C, LANES), np.float32)
    for k in range(g.shape[2]):
        for l in range(4):
            s = s + g[:, :, k, :, l]
    return _tree(s)


def finish(P, n):
    """P [B, C] f32 -> loss [B] f32."""
    P = np.asarray(P, np.float32)
    B, C = P.shape
    trips = -(-C // LANES)
    pad = np.zeros((B, trips * LANES), np.float32)
    pad[:, :C] = P
    g = pad.reshape(B, trips, LANES)
    s = np.zeros((B, LANES), np.float32)
    for k in range(trips):
        s = s + g[:, k, :]
    return (_tree(s) / f32(n)).astype(np.float32)


def noise_mse(pred, noise):
    """The reference of dllm_noise_mse: pred, noise [B, n] -> loss [B] f32."""
    e = squared_errors(pred, noise)
    with np.errstate(over="ignore", invalid="ignore"):
        return finish(chunk_partials(e), e.shape[1])


# ---- plain loop -----------------------------------------------------------------------------------

def _tree_loop(s):
    s = list(s)
    h = LANES // 2
    while h >= 1:
        for j in range(h):
            s[j] = f32(s[j] + s[j + h])
        h //= 2
    return s[0]


def chunk_partial_loop(e, c):
    """Partial of chunk c of one sample's e [n]."""
    n = len(e)
    s = [f32(0.0)] * LANES
    for g in range(CHUNK // 4):
        for l in range(4):
            i = c * CHUNK + 4 * g + l
            if i < n:
                s[g % LANES] = f32(s[g % LANES] + e[i])
    return _tree_loop(s)


def finish_loop(P, n):
    """One sample's partials [C] -> loss."""
    s = [f32(0.0)] * LANES
    for c in range(len(P)):
        s[c % LANES] = f32(s[c % LANES] + P[c])
    return f32(_tree_loop(s) / f32(n))


def noise_mse_loop(pred, noise):
    e = squared_errors(pred, noise)
    out = np.zeros(e.shape[0], np.float32)
    for b in range(e.shape[0]):
        C = -(-e.shape[1] // CHUNK)
        P = [chunk_partial_loop(e[b], c) for c in range(C)]
        out[b] = finish_loop(P, e.shape[1])
    return out


# ---- test data ------------------------------------------------------------------------------------

MASKS = ("dense", "lanes", "trips", "comps", "chunks")


def lane_pattern(B, n, seed=0, mask="dense"):
    """noise [B, n] f32 for pred = 0: random mantissas and signs, magnitudes 2^0 .. 2^20 (squares
    up to 2^40) with a geometric tail, so that a few large terms carry each sum and the small ones
    survive only in the partial sums that the pinned order forms before they meet a large one.

    A reordered sum differs from the pinned one only in its roundings, and only roundings near the
    size of the total reach the result's bits, so one dense sample seldom tells two orders apart.
    The masks leave only the terms that one stage of the order combines, which puts every rounding
    of that stage next to the total: "lanes" one element per lane (the tree), "trips" lane 0's
    groups (a lane's sequential adds), "comps" the first group of each chunk (the four components),
    "chunks" one element per chunk (the pass over the partials)."""
    rng = np.random.default_rng(seed)
    expo = np.minimum(rng.geometric(0.5, (B, n)) - 1, 20)
    x = (1.0 + rng.random((B, n))) * np.exp2(expo) * rng.choice([-1.0, 1.0], (B, n))
    i = np.arange(n)
    g = (i % CHUNK) // 4
    lane, trip, comp = g % LANES, g // LANES, i % 4
    keep = {"dense": np.ones(n, bool), "lanes": (trip == 0) & (comp == 0), "trips": lane == 0, "comps": g == 0,
            "chunks": (g == 0) & (comp == 0)}[mask]
    return (x * keep).astype(np.float32)

"""The diffusion step's kernels (csrc/diffusion.hip: randn_kernel, p_sample_kernel, add_noise_kernel)
through their C-ABI entry points at the sizes, offsets, values and pointers where they can go wrong,
plus the noise stream's other two consumers (the fused GEMM epilogue and the p_losses stream kernel)
at the counter offsets, the f32 -> f16 hand-off cast past one trip, and the rows_per_sample clamp.

Reference: the C oracle (``orc.randn``, ``orc.p_sample``, ``orc.add_noise``); coefficients are
arbitrary distinct f32 triples / pairs per row (a row mix-up changes the bits), except the schedule
cases, which take ``orc.p_sample_coeffs`` / ``orc.add_noise_coeffs`` of ``DiffusionConfig()`` at
t = [0, 1, 999, 2000] under both scans (the exclusive scan's t = 0 row divides by zero).

Bar: every output bit-exact.  The one relaxation, written down here: where the reference output is
a NaN (inf - inf, 0 * inf, 0 / 0 coefficients, or a NaN input) only "is NaN" is compared, because
IEEE 754 leaves the sign and payload of such a NaN to the implementation (the rule of
tests/test_gpu_diffusion.same).  Special values are confined to one row of at most 16 elements per
case, the number of reference NaNs must equal the number the case planned (``SPECIAL3`` / ``SPECIAL2``
mark them one by one), and every other element is compared by bits.

``CASES`` is plain data and imports without a GPU (tests/test_diffusion_cases_cpu.py checks its
arithmetic, the planned NaN counts and the oracle stream's splice property on any machine).
``TRIP`` = elements one pass of a kernel's grid-stride loop covers at its capped grid; every
``big`` size is one trip plus a ragged remainder, the smallest at which the loop's stride runs.

Every output lives inside a larger device buffer pre-filled with a sentinel byte; after each call
the 64 bytes before and after the output's exact extent must still hold the sentinel, and after a
refused call the whole buffer must.

Counter offsets: 2^34 - 8 (the Philox block index passes 2^32 inside the call, so the counter's low
word carries into its high word) and 2^64 - 8 (the stream index wraps: include/dllm_quant.h takes it
modulo 2^64, as the oracle does), n = 19; for the fused epilogue 2^34 - 4096 and 2^64 - 4096 (the
carry lands mid-matrix); for the loss kernel 2^k - 2048 (inside a whole chunk's four-trip pass) and
2^k - 16640 (inside the first sample's ragged second chunk).
"""
from collections import namedtuple

import numpy as np
import pytest

from tests import p_losses_ref
from tests import test_gpu_linear_kernels as gk
from tests.test_gpu_quant_side_kernels import SENT, In, Out

SRC = "diffusion-llm-rs_amd/csrc/diffusion.hip"
TRIP = 4096 * 256 * 4        # diffusion.hip:124 elem_grid(): kCUs * 16 blocks x 256 threads x 4 elements
CAST_TRIP = 2048 * 256 * 4   # linear_wq.hip:1582 cast_f32_f16_kernel's grid: kCUs * 8 blocks x 256 threads x 4

ROW_EDGES = ((1, 1), (1, 3), (5, 1), (4, 6), (3, 8), (2, 1001))    # (B, D); (4, 6): quads straddle rows
CARRY, WRAP = 1 << 34, 1 << 64
COUNTER_OFFSETS = (CARRY - 8, WRAP - 8)
COUNTER_N = 19
SCHEDULE_T = (0, 1, 999, 2000)

# id, kernel, shapes (n for randn, (B, D) otherwise), path (the p_sample branch the id names, chosen
# by D % 4), big (elements, for a second-trip case).
Case = namedtuple("Case", "id kernel shapes path big")

CASES = [Case(*c) for c in [
    ("randn_small", "randn_kernel", (1, 2, 3, 4, 5, 7), None, None),
    ("randn_big", "randn_kernel", (TRIP + 7,), None, TRIP + 7),          # one whole quad and a 3-element tail
    ("p_sample_rows", "p_sample_kernel", ROW_EDGES, None, None),
    ("p_sample_big_vector", "p_sample_kernel", ((3, 1398104),), "vector", TRIP + 8),
    ("p_sample_big_scalar", "p_sample_kernel", ((3, 1398103),), "scalar", TRIP + 5),
    ("p_sample_specials_vector", "p_sample_kernel", ((3, 12),), "vector", None),
    ("p_sample_specials_scalar", "p_sample_kernel", ((3, 11),), "scalar", None),
    ("p_sample_schedule_vector", "p_sample_kernel", ((4, 8),), "vector", None),
    ("p_sample_schedule_scalar", "p_sample_kernel", ((4, 6),), "scalar", None),
    ("add_noise_rows", "add_noise_kernel", ROW_EDGES, None, None),
    ("add_noise_big", "add_noise_kernel", ((3, 1398103),), None, TRIP + 5),
    ("add_noise_specials", "add_noise_kernel", ((3, 11),), None, None),
    ("add_noise_schedule", "add_noise_kernel", ((4, 6),), None, None),
    ("counter", "randn_kernel, p_sample_kernel, add_noise_kernel", ((1, COUNTER_N),), None, None),
]]
BY_ID = {c.id: c for c in CASES}

# ---- values (shared with tests/test_diffusion_cases_cpu.py) ------------------------------------------

INF, NAN = float("inf"), float("nan")
SPECIAL_COEF3 = (0.75, -0.5, 1.25)
# (x_t, eps, noise, the reference is NaN) under SPECIAL_COEF3: (0.75 x - 0.5 eps) + 1.25 noise
SPECIAL3 = [
    (NAN, 1.0, 1.0, True),            # a NaN in each operand
    (1.0, NAN, 1.0, True),
    (1.0, 1.0, NAN, True),
    (INF, INF, -INF, True),           # inf - inf inside the mean
    (-INF, 1.0, INF, True),           # inf - inf between mean and noise term
    (INF, -INF, INF, False),          # +inf throughout
    (0.0, -0.0, 0.0, False),          # (+0 + +0) + +0 = +0
    (-0.0, 0.0, -0.0, False),         # (-0 + -0) + -0 = -0
    (1e-45, -1e-45, 1e-45, False),    # denormals: 0.75, 0.5 and 1.25 ulp of the smallest one
    (-3e38, 3e38, -3e38, False),      # overflow to -inf in the mean
    (3e38, -3e38, -3e38, True),       # overflow to +inf in the mean, to -inf in the noise term
    (-INF, 1.0, 1.0, False),
]
SPECIAL_COEF2 = (1.5, -1.25)
# (x0, noise, the reference is NaN) under SPECIAL_COEF2: 1.5 x0 - 1.25 noise
SPECIAL2 = [
    (NAN, 1.0, True),
    (1.0, NAN, True),
    (INF, INF, True),
    (INF, -INF, False),
    (0.0, -0.0, False),               # +0 + +0
    (-0.0, 0.0, False),               # -0 + -0
    (1e-45, -1e-45, False),           # 1.5 ulp (a tie) and 1.25 ulp of the smallest denormal
    (3e38, -3e38, False),             # both products overflow to +inf
    (3e38, 3e38, True),               # +inf - inf by overflow
    (-INF, 1.0, False),
    (1.0, -INF, False),
]


def coef3(B):
    """Distinct {c1, c2, std} per row."""
    r = np.arange(B, dtype=np.float32)
    return np.stack([0.625 + 0.125 * r, -0.375 - 0.0625 * r, 1.5 + 0.25 * r], axis=1).astype(np.float32)


def coef2(B):
    r = np.arange(B, dtype=np.float32)
    return np.stack([0.875 + 0.25 * r, -0.625 - 0.125 * r], axis=1).astype(np.float32)


def normal_inputs(B, D, k, seed):
    """k arrays [B, D] of N(0, 1) f32."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((B, D)).astype(np.float32) for _ in range(k)]


def p_sample_specials(B, D, row):
    """-> x_t, eps, noise [B, D], coef [B, 3], planned NaN count: SPECIAL3[:D] in row ``row``."""
    assert D <= len(SPECIAL3) and D <= 16
    x, e, z = normal_inputs(B, D, 3, seed=B * D)
    sp = np.array([s[:3] for s in SPECIAL3[:D]], np.float32)
    x[row], e[row], z[row] = sp[:, 0], sp[:, 1], sp[:, 2]
    c = coef3(B)
    c[row] = SPECIAL_COEF3
    return x, e, z, c, sum(s[3] for s in SPECIAL3[:D])


def add_noise_specials(B, D, row):
    """-> x0, noise [B, D], coef [B, 2], planned NaN count: SPECIAL2[:D] in row ``row``."""
    assert D <= len(SPECIAL2) and D <= 16
    x, z = normal_inputs(B, D, 2, seed=B * D + 1)
    sp = np.array([s[:2] for s in SPECIAL2[:D]], np.float32)
    x[row], z[row] = sp[:, 0], sp[:, 1]
    c = coef2(B)
    c[row] = SPECIAL_COEF2
    return x, z, c, sum(s[2] for s in SPECIAL2[:D])


def schedule_nans(D, inclusive):
    """Reference NaNs of a schedule case: the exclusive scan's t = 0 row has abar = abar_prev = 1,
    so c1 = beta / 0 = inf and c2 = std = 0 / 0: the whole first row."""
    return 0 if inclusive else D


def mse_offsets():
    """Loss-kernel stream offsets for samples of 16384 + 512 elements: the carry / wrap at element
    2048 of the first sample (its whole chunk, between trips 1 and 2 of a four-trip pass) and at
    element 16640 (its ragged chunk)."""
    return [w - d for w in (CARRY, WRAP) for d in (2048, 16384 + 256)]


MSE_B, MSE_N = 2, 16384 + 512


def same_f32(got, ref, planned_nans=0):
    """Bit-identical f32 except where the reference is NaN (module docstring); the reference holds
    exactly the planned number of NaNs."""
    got, ref = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(ref, np.float32).ravel()
    nan = np.isnan(ref)
    assert int(nan.sum()) == planned_nans, (int(nan.sum()), planned_nans)
    ok = (got.view(np.uint32) == ref.view(np.uint32)) | (nan & np.isnan(got))
    assert got.shape == ref.shape and ok.all(), (int((~ok).sum()), np.flatnonzero(~ok)[:8].tolist())


# ---- device side -----------------------------------------------------------------------------------

pytestmark = pytest.mark.gpu

SEED = 2**63 + 7          # both key words non-zero
BIG_OFFSET = 1 << 20


@pytest.fixture(scope="module")
def gpu(dllm, cuda):
    import torch

    class G:
        L = dllm._lib.load()
        check = staticmethod(dllm._lib.check)
        INVALID = dllm._lib.ERR_INVALID_PARAMS

        @staticmethod
        def stream():
            return torch.cuda.current_stream().cuda_stream
    G.torch = torch
    return G


@pytest.fixture(scope="module")
def big_stream(orc):
    """Stream elements BIG_OFFSET .. of SEED, TRIP + 8 of them: the reference of the second-trip
    randn case and the generated noise of the second-trip p_sample and add_noise cases."""
    z = orc.randn(SEED, BIG_OFFSET, TRIP + 8)
    z.setflags(write=False)
    return z


def untouched(out):
    return bool((out.t == SENT).all())


class Bufs:
    """Inputs and one or two guarded outputs for n elements."""

    def __init__(self, gpu, n, n_in=3, n_out=1):
        self.ins = [In(gpu.torch, 4 * (n + 1)) for _ in range(n_in)]
        self.outs = [Out(gpu.torch, 4 * n) for _ in range(n_out)]
        self.coef = In(gpu.torch, 4096)


# ---- randn -------------------------------------------------------------------------------------------

def _randn(gpu, orc, seed, offset, n, out, ref=None):
    gpu.check(gpu.L.dllm_randn(seed, offset, out.place(4 * n), n, gpu.stream()))
    same_f32(out.read(np.float32), orc.randn(seed, offset, n) if ref is None else ref)


def test_randn_small(gpu, orc):
    out = Out(gpu.torch, 4 * 8)
    for n in BY_ID["randn_small"].shapes:
        for offset in (0, 8):
            _randn(gpu, orc, SEED, offset, n, out)


def test_randn_second_trip(gpu, orc, big_stream):
    n = BY_ID["randn_big"].big
    _randn(gpu, orc, SEED, BIG_OFFSET, n, Out(gpu.torch, 4 * n), big_stream[:n])


@pytest.mark.parametrize("offset", COUNTER_OFFSETS, ids=["carry", "wrap"])
def test_randn_counter(gpu, orc, offset):
    _randn(gpu, orc, SEED, offset, COUNTER_N, Out(gpu.torch, 4 * COUNTER_N))


def test_randn_refusals(gpu):
    n = 8
    out = Out(gpu.torch, 4 * n + 16)
    assert gpu.L.dllm_randn(1, 0, out.place(4 * n, 4), n, gpu.stream()) == gpu.INVALID     # out 4 bytes off
    assert untouched(out)
    assert gpu.L.dllm_randn(1, 2, out.place(4 * n), n, gpu.stream()) == gpu.INVALID        # offset % 4
    assert untouched(out)
    assert gpu.L.dllm_randn(1, 0, out.place(4 * n), 0, gpu.stream()) == 0                  # n == 0
    gpu.torch.cuda.synchronize()
    assert untouched(out)


# ---- p_sample ----------------------------------------------------------------------------------------

def _p_sample(gpu, b, x, e, c, out_ref, *, noise=None, noise_shift=0, add=1, seed=0, offset=0, alias=None,
              planned_nans=0):
    """One dllm_p_sample call on [B, D] inputs; ``alias``: x_prev is x_t ("x") or eps ("eps")."""
    B, D = x.shape
    n = B * D
    out = b.outs[0]
    op = out.place(4 * n)
    xp, ep = b.ins[0].put(x), b.ins[1].put(e)
    if alias:
        out.view(gpu.torch.float32).copy_(gpu.torch.from_numpy((x if alias == "x" else e).ravel()))
        xp, ep = (op, ep) if alias == "x" else (xp, op)
    zp = None if noise is None else b.ins[2].put(noise, 4 * noise_shift)
    gpu.check(gpu.L.dllm_p_sample(xp, ep, zp, b.coef.put(c), B, D, add, seed, offset, op, gpu.stream()))
    same_f32(out.read(np.float32), out_ref, planned_nans)


def _p_sample_modes(gpu, orc, B, D, stream=None, full=True):
    """Generated noise, given noise (aligned and shifted by one element), add_noise = 0 beside a
    noise operand full of NaN, and both in-place forms, against the oracle."""
    n = B * D
    x, e, z = normal_inputs(B, D, 3, seed=n)
    c = coef3(B)
    b = Bufs(gpu, n)
    seed, offset = (SEED, BIG_OFFSET) if stream is not None else (77, 8)
    gen = (orc.randn(seed, offset, n) if stream is None else stream[:n]).reshape(B, D)
    ref_gen = orc.p_sample(x, e, gen, c, add_noise=True)
    _p_sample(gpu, b, x, e, c, ref_gen, seed=seed, offset=offset)
    ref_given = orc.p_sample(x, e, z, c, add_noise=True)
    _p_sample(gpu, b, x, e, c, ref_given, noise=z, noise_shift=1)
    if not full:
        return
    _p_sample(gpu, b, x, e, c, ref_given, noise=z)
    _p_sample(gpu, b, x, e, c, orc.p_sample(x, e, None, c, add_noise=False), noise=np.full((B, D), np.nan, np.float32),
              add=0)
    for alias in ("x", "eps"):
        _p_sample(gpu, b, x, e, c, ref_gen, seed=seed, offset=offset, alias=alias)
        _p_sample(gpu, b, x, e, c, ref_given, noise=z, noise_shift=1, alias=alias)


@pytest.mark.parametrize("B,D", BY_ID["p_sample_rows"].shapes)
def test_p_sample_row_edges(gpu, orc, B, D):
    _p_sample_modes(gpu, orc, B, D)


@pytest.mark.parametrize("case", ["p_sample_big_vector", "p_sample_big_scalar"])
def test_p_sample_second_trip(gpu, orc, big_stream, case):
    (B, D), = BY_ID[case].shapes
    assert B * D == BY_ID[case].big
    _p_sample_modes(gpu, orc, B, D, stream=big_stream, full=False)


@pytest.mark.parametrize("case,row", [("p_sample_specials_vector", 1), ("p_sample_specials_scalar", 2)])
def test_p_sample_specials(gpu, orc, case, row):
    """Vector path: the row is three whole quads.  Scalar path: the last row, which ends in the
    one-element tail quad (the overflow NaN)."""
    (B, D), = BY_ID[case].shapes
    x, e, z, c, planned = p_sample_specials(B, D, row)
    b = Bufs(gpu, B * D)
    ref = orc.p_sample(x, e, z, c, add_noise=True)
    for shift in (0, 1):
        _p_sample(gpu, b, x, e, c, ref, noise=z, noise_shift=shift, planned_nans=planned)
    _p_sample(gpu, b, x, e, c, ref, noise=z, alias="x", planned_nans=planned)


@pytest.mark.parametrize("inclusive", [False, True], ids=["exclusive", "inclusive"])
@pytest.mark.parametrize("case", ["p_sample_schedule_vector", "p_sample_schedule_scalar"])
def test_p_sample_schedule(gpu, dllm, orc, case, inclusive):
    (B, D), = BY_ID[case].shapes
    c = orc.p_sample_coeffs(dllm.DiffusionConfig().create_beta_schedule(), SCHEDULE_T, inclusive)
    x, e = normal_inputs(B, D, 2, seed=D)
    b = Bufs(gpu, B * D)
    planned = schedule_nans(D, inclusive)
    # the reference's own flag (t[0] == 0: no noise), then the same rows with noise added
    _p_sample(gpu, b, x, e, c, orc.p_sample(x, e, None, c, add_noise=False), add=0, planned_nans=planned)
    gen = orc.randn(5, 16, B * D).reshape(B, D)
    _p_sample(gpu, b, x, e, c, orc.p_sample(x, e, gen, c, add_noise=True), seed=5, offset=16, planned_nans=planned)


def test_p_sample_refusals(gpu):
    B, D = 2, 8
    n = B * D
    x, e = normal_inputs(B, D, 2, seed=0)
    b = Bufs(gpu, n)
    out = b.outs[0]
    cp = b.coef.put(coef3(B))
    for sx, se, so in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):            # x_t, eps, x_prev 4 bytes off
        rc = gpu.L.dllm_p_sample(b.ins[0].put(x, 4 * sx), b.ins[1].put(e, 4 * se), None, cp, B, D, 1, 3, 0,
                                 out.place(4 * n, 4 * so), gpu.stream())
        assert rc == gpu.INVALID and untouched(out), (sx, se, so)
    xp, ep = b.ins[0].put(x), b.ins[1].put(e)
    assert gpu.L.dllm_p_sample(xp, ep, None, cp, B, D, 1, 3, 6, out.place(4 * n), gpu.stream()) == gpu.INVALID
    assert untouched(out)
    for B0, D0 in ((0, D), (B, 0)):
        assert gpu.L.dllm_p_sample(xp, ep, None, cp, B0, D0, 1, 3, 0, out.place(4 * n), gpu.stream()) == 0
        gpu.torch.cuda.synchronize()
        assert untouched(out)


# ---- add_noise ---------------------------------------------------------------------------------------

def _add_noise(gpu, b, x, c, ref, *, noise=None, seed=0, offset=0, shifts=(0, 0, 0, 0), noise_out=None, alias=False,
               planned_nans=0):
    """One dllm_add_noise call; shifts = elements by which x0, noise, noisy and noise_out are moved;
    ``noise_out``: the expected noise (None: a NULL pointer)."""
    B, D = x.shape
    n = B * D
    out, nout = b.outs
    op = out.place(4 * n, 4 * shifts[2])
    xp = b.ins[0].put(x, 4 * shifts[0])
    if alias:
        out.view(gpu.torch.float32).copy_(gpu.torch.from_numpy(x.ravel()))
        xp = op
    zp = None if noise is None else b.ins[1].put(noise, 4 * shifts[1])
    np_ = nout.place(4 * n, 4 * shifts[3])
    gpu.check(gpu.L.dllm_add_noise(xp, zp, b.coef.put(c), B, D, seed, offset, op, None if noise_out is None else np_,
                                   gpu.stream()))
    same_f32(out.read(np.float32), ref, planned_nans)
    if noise_out is None:
        gpu.torch.cuda.synchronize()
        assert untouched(nout)
    else:
        same_f32(nout.read(np.float32), noise_out, int(np.isnan(noise_out).sum()))


def _add_noise_modes(gpu, orc, B, D, stream=None, full=True):
    n = B * D
    x, z = normal_inputs(B, D, 2, seed=n + 2)
    c = coef2(B)
    b = Bufs(gpu, n, n_in=2, n_out=2)
    seed, offset = (SEED, BIG_OFFSET) if stream is not None else (9, 4)
    gen = (orc.randn(seed, offset, n) if stream is None else stream[:n]).reshape(B, D)
    ref_gen, ref_given = orc.add_noise(x, gen, c), orc.add_noise(x, z, c)
    _add_noise(gpu, b, x, c, ref_gen, seed=seed, offset=offset, noise_out=gen)
    _add_noise(gpu, b, x, c, ref_given, noise=z, shifts=(1, 0, 1, 0))
    if not full:
        return
    _add_noise(gpu, b, x, c, ref_gen, seed=seed, offset=offset)                     # noise_out == NULL
    _add_noise(gpu, b, x, c, ref_given, noise=z)
    for k in range(4):                                                              # each pointer in turn
        sh = tuple(int(j == k) for j in range(4))
        if k == 3:
            _add_noise(gpu, b, x, c, ref_gen, seed=seed, offset=offset, shifts=sh, noise_out=gen)
        else:
            _add_noise(gpu, b, x, c, ref_given, noise=z, shifts=sh)
            _add_noise(gpu, b, x, c, ref_gen, seed=seed, offset=offset, shifts=(sh[0], 0, sh[2], 0), noise_out=gen)
    _add_noise(gpu, b, x, c, ref_gen, seed=seed, offset=offset, alias=True, noise_out=gen)   # noisy == x0
    _add_noise(gpu, b, x, c, ref_given, noise=z, alias=True, shifts=(0, 1, 0, 0))


@pytest.mark.parametrize("B,D", BY_ID["add_noise_rows"].shapes)
def test_add_noise_row_edges(gpu, orc, B, D):
    _add_noise_modes(gpu, orc, B, D)


def test_add_noise_second_trip(gpu, orc, big_stream):
    (B, D), = BY_ID["add_noise_big"].shapes
    assert B * D == BY_ID["add_noise_big"].big
    _add_noise_modes(gpu, orc, B, D, stream=big_stream, full=False)


def test_add_noise_specials(gpu, orc):
    (B, D), = BY_ID["add_noise_specials"].shapes
    x, z, c, planned = add_noise_specials(B, D, row=2)
    b = Bufs(gpu, B * D, n_in=2, n_out=2)
    ref = orc.add_noise(x, z, c)
    _add_noise(gpu, b, x, c, ref, noise=z, planned_nans=planned)
    _add_noise(gpu, b, x, c, ref, noise=z, shifts=(1, 1, 1, 0), planned_nans=planned)
    _add_noise(gpu, b, x, c, ref, noise=z, alias=True, planned_nans=planned)


@pytest.mark.parametrize("inclusive", [False, True], ids=["exclusive", "inclusive"])
def test_add_noise_schedule(gpu, dllm, orc, inclusive):
    (B, D), = BY_ID["add_noise_schedule"].shapes
    c = orc.add_noise_coeffs(dllm.DiffusionConfig().create_beta_schedule(), SCHEDULE_T, inclusive)
    x, = normal_inputs(B, D, 1, seed=3)
    gen = orc.randn(9, 4, B * D).reshape(B, D)
    _add_noise(gpu, Bufs(gpu, B * D, n_in=2, n_out=2), x, c, orc.add_noise(x, gen, c), seed=9, offset=4, noise_out=gen)


def test_add_noise_refusals(gpu):
    B, D = 2, 8
    n = B * D
    x, = normal_inputs(B, D, 1, seed=0)
    b = Bufs(gpu, n, n_in=2, n_out=2)
    out, nout = b.outs
    xp, cp = b.ins[0].put(x), b.coef.put(coef2(B))
    rc = gpu.L.dllm_add_noise(xp, None, cp, B, D, 3, 5, out.place(4 * n), nout.place(4 * n), gpu.stream())
    assert rc == gpu.INVALID and untouched(out) and untouched(nout)
    for B0, D0 in ((0, D), (B, 0)):
        assert gpu.L.dllm_add_noise(xp, None, cp, B0, D0, 3, 0, out.place(4 * n), nout.place(4 * n), gpu.stream()) == 0
        gpu.torch.cuda.synchronize()
        assert untouched(out) and untouched(nout)


# ---- the Philox counter inside a call -----------------------------------------------------------------

@pytest.mark.parametrize("offset", COUNTER_OFFSETS, ids=["carry", "wrap"])
def test_p_sample_add_noise_counter(gpu, orc, offset):
    (B, D), = BY_ID["counter"].shapes
    gen = orc.randn(SEED, offset, B * D).reshape(B, D)
    x, e = normal_inputs(B, D, 2, seed=19)
    _p_sample(gpu, Bufs(gpu, B * D), x, e, coef3(B), orc.p_sample(x, e, gen, coef3(B), add_noise=True), seed=SEED,
              offset=offset)
    _add_noise(gpu, Bufs(gpu, B * D, n_in=2, n_out=2), x, coef2(B), orc.add_noise(x, gen, coef2(B)), seed=SEED,
               offset=offset, noise_out=gen)


def smallest_fused_case():
    """The smallest MATRIX shape whose fused entry point runs a fused epilogue (M > 64)."""
    return min((c for c in gk.MATRIX if c.M > 64 and c.N % 4 == 0), key=lambda c: (c.M * c.N, c.K))


@pytest.fixture(scope="module")
def fused_layer(dllm, gpu, orc):
    case = smallest_fused_case()
    cache = {}
    lin, Xd, Y = gk.build(dllm, gpu.torch, orc, case, cache)
    yield case, lin, Xd, Y
    lin.close()


@pytest.mark.parametrize("offset", [CARRY - 4096, WRAP - 4096], ids=["carry", "wrap"])
def test_fused_epilogue_counter(gpu, dllm, orc, fused_layer, offset):
    """QuantLinear.forward_psample on exact_layer data (eps is exact, so the oracle's p_sample of it
    is the reference) with the carry / wrap at element 4096 of the M x N output."""
    case, lin, Xd, Y = fused_layer
    M, N, rps = case.M, case.N, gk.ROWS_PER_SAMPLE
    assert M * N > 2 * 4096 and not lin.plan(M, fused=True).flags & gk.PLAN_NOT_FUSED
    S = (M + rps - 1) // rps
    coef = orc.p_sample_coeffs(dllm.DiffusionConfig().create_beta_schedule(), [999 - 7 * i for i in range(S)],
                               inclusive=True)
    x_t, = normal_inputs(M, N, 1, seed=M + N)
    noise = orc.randn(SEED, offset, M * N).reshape(M, N)
    ref = orc.p_sample(x_t, Y.astype(np.float32), noise, np.repeat(coef, rps, axis=0)[:M], add_noise=True)
    out = Out(gpu.torch, 4 * M * N)
    out.place(4 * M * N)
    lin.forward_psample(Xd, gk.dev(gpu.torch, x_t), gk.dev(gpu.torch, coef), rps, True, SEED, offset,
                        out=out.view(gpu.torch.float32).view(M, N))
    same_f32(out.read(np.float32), ref)


@pytest.mark.parametrize("offset", mse_offsets(), ids=["carry_whole", "carry_ragged", "wrap_whole", "wrap_ragged"])
def test_noise_mse_counter(gpu, orc, offset):
    """dllm_noise_mse with noise == NULL: the loss of the oracle's stream elements, in the pinned
    summation order of tests/p_losses_ref.py."""
    B, n = MSE_B, MSE_N
    pred, = normal_inputs(B, n, 1, seed=7)
    ref = p_losses_ref.noise_mse(pred, orc.randn(SEED, offset, B * n).reshape(B, n))
    pin = In(gpu.torch, 4 * B * n)
    loss = Out(gpu.torch, 4 * B)
    wsb = max(gpu.L.dllm_noise_mse_workspace(B, n), 16)
    ws = Out(gpu.torch, wsb)
    gpu.check(gpu.L.dllm_noise_mse(pin.put(pred), 0, None, B, n, SEED, offset, loss.place(4 * B), ws.place(wsb), wsb,
                                   gpu.stream()))
    same_f32(loss.read(np.float32), ref)
    ws.read()


# ---- the f32 -> f16 hand-off of x at the first layer ----------------------------------------------------

HANDOFF_M, HANDOFF_K, HANDOFF_N = 8200, 256, 128       # M K = CAST_TRIP + 2048 elements
HANDOFF_SPECIAL_ROWS = (0, 4100, 8195, 8199)           # the last two lie in the cast's second trip


def handoff_specials(K):
    """RNE ties of the f16 grid (normal, at the overflow threshold, denormal), values past 65504,
    NaN, +-inf, +-0 and f16-denormal magnitudes, repeated along a row of K."""
    v = np.array([1 + 2.0**-11, 1 + 3 * 2.0**-11, -(1 + 2.0**-11), 2048 + 1, 2048 + 3, 65504, 65519.996, 65520, -65520,
                  1e5, -1e5, 3e38, np.nan, np.inf, -np.inf, 0.0, -0.0, 2.0**-24, 2.0**-25, -(2.0**-25), 1.5 * 2.0**-25,
                  3 * 2.0**-25, 5 * 2.0**-25, 2.0**-14, 2.0**-14 - 2.0**-25, 1e-7, -3e-6, 1e-45, 6.1e-5], np.float32)
    return np.resize(v, K)


def test_first_layer_f32_x_equals_f16_x(gpu, dllm):
    """lin(X f32) == lin(X.half()) by bits with M K past one trip of cast_f32_f16_kernel."""
    torch = gpu.torch
    M, K, N = HANDOFF_M, HANDOFF_K, HANDOFF_N
    assert CAST_TRIP < M * K <= CAST_TRIP + 4096 and max(HANDOFF_SPECIAL_ROWS) * K >= CAST_TRIP
    rng = np.random.default_rng(5)
    X = rng.standard_normal((M, K)).astype(np.float32)
    for i, r in enumerate(HANDOFF_SPECIAL_ROWS):
        X[r] = np.roll(handoff_specials(K), i)
    lin = dllm.QuantLinear.from_weight(torch.from_numpy((0.05 * rng.standard_normal((K, N))).astype(np.float32)).cuda(),
                                       None, 4, 128)
    Xd = torch.from_numpy(X).cuda()
    for dt, iv in ((torch.float32, torch.int32), (torch.float16, torch.int16)):
        a, b = lin(Xd, out_dtype=dt), lin(Xd.half(), out_dtype=dt)
        assert torch.equal(a.view(iv), b.view(iv)), dt
    finite = np.ones(M, bool)
    finite[list(HANDOFF_SPECIAL_ROWS)] = False
    assert bool(torch.isfinite(a[torch.from_numpy(finite).cuda()]).all())    # the special rows touch no other row
    lin.close()


# ---- rows_per_sample past the epilogue's int --------------------------------------------------------------

def test_rows_per_sample_clamp(gpu, dllm):
    """rows_per_sample = 2^32 ("one sample") gives the bits of rows_per_sample = M on a fused shape."""
    torch = gpu.torch
    M, d = 192, 256
    g = torch.Generator(device="cuda").manual_seed(2)
    lin = dllm.QuantLinear.from_weight(0.04 * torch.randn(d, d, device="cuda", generator=g), None, 4, 128)
    assert not lin.plan(M, fused=True).flags & gk.PLAN_NOT_FUSED
    X = torch.randn(M, d, device="cuda", generator=g).half()
    xt = torch.randn(M, d, device="cuda", generator=g)
    coef = torch.tensor([[0.75, -0.5, 1.25]], device="cuda")
    want = lin.forward_psample(X, xt, coef, M, True, 5, 16)
    out = Out(torch, 4 * M * d)
    for rps in (2**32, 2**32 + 1, M + 1):
        gpu.check(gpu.L.dllm_linear_forward_psample_ex(lin._h, X.data_ptr(), M, dllm._lib.F16, xt.data_ptr(),
                                                       coef.data_ptr(), rps, 1, 5, 16, None, out.place(4 * M * d), None,
                                                       gpu.stream()))
        assert np.array_equal(out.read(np.uint32), want.cpu().numpy().view(np.uint32).ravel()), rps
    lin.close()

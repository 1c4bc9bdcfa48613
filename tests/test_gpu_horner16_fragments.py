"""The 256 x 256 Horner kernel (HORNER16): where each weight lands in its A fragments, and that its
f16 stores rewrite every element.

The product schedule reads a wave's weight words from its LDS ring in fragment order: lane L takes
word 2h + (rho & 1) of source lane i + 32 (rho >> 1) (rho = L >> 4, i = L & 15) for column block 0
and the same word of the lane 16 above for column block 1, and dequantizes them with the zero points
of columns i and 16 + i (csrc/linear_horner.hip, MODE bit 14).

* Placement: X one-hot in k (row m has a single 1 at k = m mod K), so output row m is the dequantized
  weight row k plus the bias, exactly: a wrong source lane, word or zero-point column of the read
  shows as that (k, column), and the failure message names the first one.  (2816, 256, 3072), random
  codes, zero points and power-of-two scales per (group, column): a single term through the Horner
  chain is (q - zp) 2^e, exact in f32 and in f16.
* Tail: K = 128 (a kernel that is all tail), 256 and 384 (the two residues of the ring period) on
  whole tiles (2816, K, 3072: the f16 rows staged through the ring) and ragged ones (2689, K, 3068:
  the register stores), ``exact_layer`` data.  The f16 output goes into a NaN-filled buffer twice in
  a row; the second call must find every element rewritten with the f64 product's bits (rows stored
  from a slot that is not complete, or not stored, leave NaN or stale bits).
* Lab mark (lab build only): the parent schedule (variant 347: the skewed 4-slot ring with the lane
  swaps), the fragment-order schedule as a lab variant (350) and the product give identical bytes
  at (2816, 640, 3072) on N(0, 1) X and 0.02 N(0, 1) W -- non-integer data, where a changed summation
  order would show.  (Variant 349 drops the swaps without reordering the reads: timing only, its
  results are wrong, so it is only launched by scripts/horner_ab.py.)

Each case first asserts that the dispatch's own plan is HORNER16."""
import numpy as np
import pytest

from tests.test_gpu_linear_kernels import Case, bits_of, build, dev, exact_layer, host

pytestmark = pytest.mark.gpu

PLAN = ("HORNER16", 256, 256, 1, 1, 0)
PLACE = Case("frag_place_k256", 2816, 256, 3072, 4, 128, 0, 1, 0, PLAN)
TAIL = [Case(f"frag_tail_{name}_k{K}", M, K, N, 4, 128, 0, 1, 0, PLAN)
        for name, M, N in (("tiles", 2816, 3072), ("ragged", 2689, 3068)) for K in (128, 256, 384)]
LAB = (2816, 640, 3072)


@pytest.fixture(scope="module")
def torch(cuda):
    import torch as t
    return t


@pytest.fixture(scope="module")
def built():
    """The latest case's (handle, device X, f64 reference)."""
    cache = {}
    yield cache
    for old in cache.values():
        old[0].close()


@pytest.fixture(scope="module")
def placement(dllm, torch, orc):
    """(handle, one-hot device X, expected rows [M, N] f64) of the placement case, built once."""
    c = PLACE
    codes, scales, zps, bias, _, _ = exact_layer(c, seed=20)
    rows = np.arange(c.K) // c.group
    W = (codes.astype(np.float64) - zps[rows].astype(np.float64)) * scales[rows].astype(np.float64)
    k_of_m = np.arange(c.M) % c.K
    X = np.zeros((c.M, c.K), np.float16)
    X[np.arange(c.M), k_of_m] = 1
    lin = dllm.QuantLinear.from_quantized(dev(torch, orc.pack_bits(codes.ravel(), c.bits)), dev(torch, scales),
                                          dev(torch, zps), c.K, c.N, c.bits, c.group, bias=dev(torch, bias))
    yield lin, dev(torch, X), W[k_of_m] + bias
    lin.close()


@pytest.mark.parametrize("dt", ["float32", "float16"])
def test_fragment_placement(torch, placement, dt):
    """Every weight of every (k, column) comes out as (q - zp) * s of its own column and group."""
    lin, Xd, want = placement
    assert lin.plan(PLACE.M).astuple()[0] == "HORNER16", lin.plan(PLACE.M).astuple()
    ref = want.astype(np.dtype(dt))
    assert np.array_equal(ref.astype(np.float64), want)
    y = host(lin(Xd, out_dtype=getattr(torch, dt)))
    bad = np.argwhere(bits_of(y) != bits_of(ref))
    if bad.size:
        m, n = bad[0]
        pytest.fail(f"{dt}: {len(bad)} wrong; first at (k, column) = ({m % PLACE.K}, {n}) in row {m}: "
                    f"got {y[m, n]}, want {ref[m, n]}")


@pytest.mark.parametrize("case", TAIL, ids=[c.id for c in TAIL])
def test_tail_rewrites_every_element(dllm, torch, orc, built, case):
    """Two calls in a row into NaN-filled f16 outputs: each leaves the f64 product's RNE in every element."""
    lin, Xd, Y = build(dllm, torch, orc, case, built)
    assert lin.plan(case.M).astuple()[0] == "HORNER16", (case.id, lin.plan(case.M).astuple())
    ref16 = Y.astype(np.float32).astype(np.float16)
    out = torch.empty((case.M, case.N), device="cuda", dtype=torch.float16)
    for call in (1, 2):
        out.fill_(float("nan"))
        lin(Xd, out=out)
        y = host(out)
        left = np.argwhere(np.isnan(y))
        assert left.size == 0, (case.id, "call", call, "not rewritten", len(left), left[:4].tolist())
        bad = np.argwhere(bits_of(y) != bits_of(ref16))
        assert bad.size == 0, (case.id, "call", call, len(bad), bad[:4].tolist())


@pytest.mark.lab
def test_fragment_variants_identical_bytes(dllm, torch):
    """Parent schedule (347), fragment-order lab variant (350) and the product: the same bytes, f32 and f16."""
    M, K, N = LAB
    g = torch.Generator(device="cuda").manual_seed(5)
    W = 0.02 * torch.randn(K, N, device="cuda", generator=g)
    X = torch.randn(M, K, device="cuda", generator=g).half()
    lin = dllm.QuantLinear.from_weight(W, None, 4, 128)
    try:
        assert lin.plan(M).astuple()[0] == "HORNER16", lin.plan(M).astuple()
        outs = {}
        for v in (347, 350, -1):
            lin.set_kernel_variant(v)
            outs[v] = (host(lin(X, out_dtype=torch.float32)), host(lin(X, out_dtype=torch.float16)))
        assert np.isfinite(outs[347][0]).all() and np.abs(outs[347][0]).max() > 0
        for v in (350, -1):
            for i, what in enumerate(("f32", "f16")):
                bad = np.argwhere(bits_of(outs[v][i]) != bits_of(outs[347][i]))
                assert bad.size == 0, (v, what, len(bad), bad[:4].tolist())
    finally:
        lin.set_kernel_variant(-1)
        lin.close()

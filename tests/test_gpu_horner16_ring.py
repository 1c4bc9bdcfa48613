"""The 256 x 256 Horner kernel (HORNER16) over every length of its stage ring.

tests/test_gpu_linear_kernels.py reaches HORNER16 only at K = 256 (4 k-steps of 64).  The kernel's
ring schedule has a prologue (2 stages), a main loop unrolled over the group period (2 k-steps) on a
4-slot ring with a 3-slot ring of weight words per wave, and two peeled last k-steps, so here K runs
over {128, ..., 896}: 2 to 14 k-steps -- no main loop at all (K = 128), both residues of the ring
period (K / 64 mod 4 = 2 and 0), every slot of both rings holding the last stage.  Shapes: (2689, K,
3068) -- ragged M, N % 8 == 4, a padded last column block, the register stores -- and (2816, K, 3072)
-- whole tiles, the f16 rows staged through the drained ring.  int4 and int2, f32 and f16 outputs,
and a second call into a NaN-filled output (``run_plain`` of the kernel matrix), all bit-equal to
the f64 product on ``exact_layer`` data: at K = 896 the bound is 896 x 2 x 15 x 2^8 = 6.9e6 < 2^24,
so f32 is exact in every summation order and a stage read too early, too late or from the wrong
slot changes bits.  One fused p_sample case at K = 640 with rows_per_sample = 37.

Each case first asserts that the dispatch's own plan is HORNER16.

Lab build only (``lab`` mark): the three schedules of the 256-token kernel as lab variants 346 (4-slot
ring, waves in lockstep), 347 (4-slot ring, skew: the product) and 348 (3-slot ring, a barrier every
half k-step) each launch and give the same exact bits at K = 640."""
import numpy as np
import pytest

from tests.test_gpu_linear_kernels import Case, ROWS_PER_SAMPLE, build, run_fused, run_plain

pytestmark = pytest.mark.gpu

KS = (128, 256, 384, 512, 640, 768, 896)
SHAPES = (("ragged", 2689, 3068), ("tiles", 2816, 3072))
PLAN = ("HORNER16", 256, 256, 1, 1, 0)

CASES = [Case(f"ring_{name}_k{K}_int{bits}", M, K, N, bits, 128, 0, 1, 0, PLAN)
         for bits in (4, 2) for name, M, N in SHAPES for K in KS]
LAB = Case("ring_ragged_k640_int4_lab", 2689, 640, 3068, 4, 128, 0, 1, 0, PLAN)
FUSED = Case("ring_ragged_k640_int4_fused", 2689, 640, 3068, 4, 128, 0, 1, 0, PLAN)


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


def assert_horner16(dllm, torch, orc, case, built, fused):
    lin = build(dllm, torch, orc, case, built)[0]
    assert lin.plan(case.M, fused=fused).astuple()[0] == "HORNER16", (case.id, lin.plan(case.M, fused=fused).astuple())


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_horner16_ring_lengths(dllm, torch, orc, built, case):
    """f32 == the f64 product, f16 == its RNE, and the same bits again into NaN-filled outputs."""
    assert case.K // 64 in range(2, 15) and np.log2(case.K * 2 * 15 * 2 ** 8) < 24
    assert_horner16(dllm, torch, orc, case, built, fused=False)
    run_plain(dllm, torch, orc, case, built)


def test_horner16_ring_fused_psample(dllm, torch, orc, built):
    """The fused p_sample epilogue behind a 10-k-step ring: x_prev == the oracle's p_sample of the exact
    eps, samples of 37 rows straddling the 256-row tiles."""
    assert_horner16(dllm, torch, orc, FUSED, built, fused=True)
    run_fused(dllm, torch, orc, FUSED, built, ROWS_PER_SAMPLE)


@pytest.mark.lab
@pytest.mark.parametrize("variant", [346, 347, 348])
def test_horner16_schedule_variants(dllm, torch, orc, built, variant):
    """Every schedule arm of the A/B (profiles/horner16_ring4/) is reachable through
    dllm_linear_set_kernel_variant in the lab build and bit-exact."""
    lin = build(dllm, torch, orc, LAB, built)[0]
    lin.set_kernel_variant(variant)
    try:
        run_plain(dllm, torch, orc, LAB, built)
    finally:
        lin.set_kernel_variant(-1)

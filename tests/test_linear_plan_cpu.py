"""dllm_linear_plan_shape on the host: the linear layer's kernel selection (the routine the
dispatch itself switches on) obeys its invariants over a sweep of the policy's boundaries, gives the
documented plan at the anchor shapes, and every plan class the sweep reaches is run by the GPU
matrix of tests/test_gpu_linear_kernels.py.  No GPU, no handle."""
import itertools

import pytest

from tests import test_gpu_linear_kernels as gk

STAGGERED, DECODE_XL, SPLITK, NOT_FUSED = 1, 2, 4, 8
HORNER_FAMILY = {"HORNER16", "HORNER_PC", "HORNER_KG2", "HORNER_PC_KG2"}
EXACT, F16W = 0, 1

NS = [128, 200, 256, 512, 1020, 1024, 2048, 3000, 3968, 4092, 4096, 32768]   # 3968: Npad = 31 x 128
KS = [256, 384, 512, 768, 1024, 4096]


def sweep_ms():
    """M at every boundary of the policy +-1 up to 8200: the decode buckets, and the multiples of the
    tile heights (32 up to 512, 64 up to 2048, 128 beyond) at which a tile count can cross a round."""
    ms = set(range(1, 18)) | {31, 32, 33, 63, 64, 65, 66, 100, 300, 700, 3001, 4300}
    for b in itertools.chain(range(32, 513, 32), range(512, 2049, 64), range(2048, 8193, 128)):
        ms |= {b - 1, b, b + 1}
    return sorted(m for m in ms if 1 <= m <= 8200)


def sweep():
    """(K, N, bits, group, precision, horner_ok, prefill_only, M), thinned where a flag cannot matter:
    horner_ok = 0 only for the shapes whose handle computes ratios, prefill_only only at M <= 64."""
    ms = sweep_ms()
    for N, K, bits, group, precision in itertools.product(NS, KS, (2, 4, 8), (64, 128, 256), (EXACT, F16W)):
        ratios = precision == EXACT and bits in (2, 4) and group == 128
        for horner_ok in ((1, 0) if ratios else (1,)):
            for prefill_only in (0, 1):
                for M in ms:
                    if prefill_only and M > 64:
                        break
                    yield K, N, bits, group, precision, horner_ok, prefill_only, M


@pytest.fixture(scope="module")
def plan_shape(dllm):
    lib = dllm._lib

    def f(K, N, bits, group, M, precision=EXACT, horner_ok=1, prefill_only=0, fused=False):
        return lib.linear_plan_shape(K, N, bits, group, M, precision=precision, prefill_only=bool(prefill_only),
                                     horner_ok=bool(horner_ok), fused=fused).astuple()
    return f


@pytest.fixture(scope="module")
def swept(plan_shape):
    """[(shape, plan)] of the sweep's plain entry point, computed once."""
    return [(s, plan_shape(s[0], s[1], s[2], s[3], s[7], s[4], s[5], s[6])) for s in sweep()]


def test_plan_invariants(swept, plan_shape):
    assert len(swept) > 100_000
    for (K, N, bits, group, precision, horner_ok, prefill_only, M), plan in swept:
        kernel, tile_m, tile_n, kgroups, nsplit, flags = plan
        ctx = (K, N, bits, group, precision, horner_ok, prefill_only, M, plan)
        npad = (N + 127) // 128 * 128
        assert npad % tile_n == 0, ctx
        assert (kernel == "DECODE") == (M <= 64 and not prefill_only), ctx
        assert bool(flags & SPLITK) == (nsplit > 1) and not flags & NOT_FUSED, ctx
        if kernel == "DECODE":
            assert tile_m == (16 if M <= 16 else 32 if M <= 32 else 64) and kgroups == 1, ctx
            assert 1 <= nsplit <= (K + 127) // 128, ctx        # slices of whole 128-deep slabs
            if flags & DECODE_XL:
                assert 9 <= M <= 16 and nsplit == 1 and tile_n == 16, ctx
        elif kernel == "ROUNDED_RING":
            assert precision == F16W or K % group != 0, ctx
            assert 4 % kgroups == 0, ctx                       # k-groups share each 64-deep stage
            assert (K // 64) % nsplit == 0, ctx
        else:
            assert precision == EXACT and K % group == 0, ctx
            assert (K // group) % kgroups == 0, ctx            # each k-group streams whole groups
            assert (K // group) % nsplit == 0, ctx             # group-aligned K slices
        if kernel in HORNER_FAMILY:
            assert horner_ok and precision == EXACT and group == 128 and bits != 8 and npad % 256 == 0, ctx
            assert bits == 4 or kernel == "HORNER16", ctx
            assert nsplit == 1, ctx
        if flags & STAGGERED:
            assert kernel == "EXACT_FOLD" and (tile_m, tile_n) == (128, 256) and bits == 4 and group == 128, ctx
        assert flags & ~(STAGGERED | DECODE_XL | SPLITK) == 0, ctx


def test_plan_fused_entry(swept, plan_shape):
    """The fused entry point runs the same plan; at M <= 64 it reports the unfused pair."""
    for (K, N, bits, group, precision, horner_ok, prefill_only, M), plan in swept:
        if N % 4:
            continue
        fused = plan_shape(K, N, bits, group, M, precision, horner_ok, prefill_only, fused=True)
        assert fused[:5] == plan[:5] and fused[5] == plan[5] | (NOT_FUSED if M <= 64 else 0), (K, N, bits, group, M)


def test_plan_rejects_bad_arguments(dllm):
    import ctypes as C
    lib, L = dllm._lib.load(), dllm._lib
    out = L.LinearPlan()
    assert lib.dllm_linear_plan_shape(4096, 4096, 4, 128, 0, 1, 0, 0, C.byref(out)) == L.ERR_SHAPE_MISMATCH   # M = 0
    assert lib.dllm_linear_plan_shape(4096, 4096, 3, 128, 0, 1, 64, 0, C.byref(out)) == L.ERR_UNSUPPORTED
    assert lib.dllm_linear_plan_shape(4100, 4096, 4, 128, 0, 1, 64, 0, C.byref(out)) == L.ERR_SHAPE_MISMATCH
    assert lib.dllm_linear_plan_shape(4096, 4096, 4, 128, 0, 1, 64, 0, None) == L.ERR_INVALID_PARAMS
    assert lib.dllm_linear_plan_shape(4096, 4094, 4, 128, 0, 1, 128, 1, C.byref(out)) == L.ERR_UNSUPPORTED   # fused, N % 4
    assert lib.dllm_linear_plan(None, 64, 0, C.byref(out)) == L.ERR_INVALID_PARAMS


# (M, K, N, bits, horner_ok) -> (kernel, tile_m, tile_n, kgroups, nsplit, flags); int4 / int2 g128 EXACT.
ANCHORS = [
    ((4096, 4096, 4096, 4, 1), ("HORNER16", 256, 256, 1, 1, 0)),
    ((4096, 4096, 4096, 2, 1), ("HORNER16", 256, 256, 1, 1, 0)),
    ((8000, 4096, 4096, 4, 1), ("HORNER16", 256, 256, 1, 1, 0)),
    ((3001, 4096, 4096, 4, 1), ("HORNER16", 256, 256, 1, 1, 0)),
    ((2048, 4096, 4096, 4, 1), ("HORNER_PC", 128, 256, 1, 1, 0)),
    ((1800, 4096, 4096, 4, 1), ("HORNER_PC", 128, 256, 1, 1, 0)),
    ((4300, 4096, 4096, 4, 1), ("HORNER_PC", 128, 256, 1, 1, 0)),
    ((4096, 4096, 2048, 4, 1), ("HORNER_PC", 128, 256, 1, 1, 0)),
    ((4096, 4096, 1024, 4, 1), ("HORNER_PC_KG2", 128, 128, 2, 1, 0)),
    ((1024, 4096, 4096, 4, 1), ("HORNER_PC_KG2", 128, 128, 2, 1, 0)),
    ((700, 4096, 4096, 4, 1), ("HORNER_PC_KG2", 128, 128, 2, 1, 0)),
    ((512, 4096, 4096, 4, 1), ("HORNER_PC_KG2", 64, 128, 2, 1, 0)),
    ((384, 4096, 4096, 4, 1), ("HORNER_PC_KG2", 64, 128, 2, 1, 0)),
    ((4096, 4096, 512, 4, 1), ("HORNER_PC_KG2", 64, 128, 2, 1, 0)),
    ((256, 4096, 4096, 4, 1), ("EXACT_FOLD", 32, 128, 4, 1, 0)),
    ((65, 4096, 4096, 4, 1), ("EXACT_FOLD", 32, 128, 4, 1, 0)),
    ((2048, 4096, 4096, 2, 1), ("EXACT_FOLD", 128, 256, 1, 1, 0)),
    ((4096, 4096, 4096, 4, 0), ("EXACT_FOLD", 128, 256, 1, 1, STAGGERED)),
    ((384, 4096, 4096, 4, 0), ("EXACT_FOLD", 32, 128, 2, 1, 0)),
    ((100, 512, 32768, 4, 1), ("HORNER_KG2", 256, 128, 2, 1, 0)),
]


@pytest.mark.parametrize("shape,want", ANCHORS, ids=["M%d-K%d-N%d-int%d-horner%d" % s for s, _ in ANCHORS])
def test_plan_anchors(plan_shape, shape, want):
    M, K, N, bits, horner_ok = shape
    assert plan_shape(K, N, bits, 128, M, horner_ok=horner_ok) == want


def test_kg2_is_off_the_m1800_grid(plan_shape):
    """The 256 x 128 KG2 kernel is no longer reached at N 4096 (M 1793..1920 take the PC tiles); it
    stays reachable only where ceil(M / 128) == ceil(M / 256) on at least 256 column tiles."""
    for M in range(65, 8201):
        assert plan_shape(4096, 4096, 4, 128, M)[0] != "HORNER_KG2", M
    for M in (65, 100, 128):
        assert plan_shape(512, 32768, 4, 128, M)[0] == "HORNER_KG2", M
    assert plan_shape(512, 32768, 4, 128, 129)[0] != "HORNER_KG2"


def test_gpu_matrix_covers_every_reachable_class(swept, plan_shape):
    """Every (kernel, tile, kgroups, split, flags) class the sweep reaches is run by the GPU matrix, by
    the plain entry point and (N % 4 == 0) by the fused one; and each matrix entry's class is the
    library's answer for it.  A policy change that strands a kernel, or makes a new class reachable,
    fails here."""
    reached = {gk.plan_class(plan) for _, plan in swept}
    plain, fused = set(), set()
    for c in gk.MATRIX:
        got = plan_shape(c.K, c.N, c.bits, c.group, c.M, c.precision, c.horner_ok, c.prefill_only)
        assert got == c.plan, (c.id, got, c.plan)
        plain.add(gk.plan_class(got))
        if c.N % 4 == 0:
            gotf = plan_shape(c.K, c.N, c.bits, c.group, c.M, c.precision, c.horner_ok, c.prefill_only, fused=True)
            assert bool(gotf[5] & NOT_FUSED) == (c.M <= 64), (c.id, gotf)
            fused.add(gk.plan_class(gotf))
    assert reached - plain == set(), f"reachable but not in the GPU matrix: {sorted(reached - plain)}"
    assert reached - fused == set(), f"reachable but not run fused: {sorted(reached - fused)}"
    assert plain - reached == set(), f"in the GPU matrix but outside the sweep: {sorted(plain - reached)}"
    assert len({c.id for c in gk.MATRIX}) == len(gk.MATRIX)


def test_gpu_matrix_data_is_exact():
    """The matrix' data generator keeps its exactness condition at every case (checked on the two
    smallest cases in full; the assertion inside runs for each case on the GPU)."""
    for c in sorted(gk.MATRIX, key=lambda c: c.M * c.K * c.N)[:2]:
        codes, scales, zps, bias, X, Y = gk.exact_layer(c, seed=1)
        assert codes.shape == (c.K, c.N) and scales.shape == zps.shape and Y.shape == (c.M, c.N)

"""CPU checks behind tests/test_gpu_diffusion_edges.py: the case table's arithmetic (so a later edit
cannot shrink a case below the path it is there for), the planned NaN count of every specials and
schedule case against the oracle, and the splice property of the oracle's noise stream on which the
counter cases rest: elements from 4k on of a draw at ``off`` are the draw at ``off + 4k`` (taken
modulo 2^64), at the carry and at the wrap offsets."""
import numpy as np
import pytest

from tests import test_gpu_diffusion_edges as de


def test_case_table_arithmetic():
    assert len({c.id for c in de.CASES}) == len(de.CASES)
    assert de.TRIP == 4096 * 256 * 4 and de.CAST_TRIP == 2048 * 256 * 4
    kernels = " ".join(c.kernel for c in de.CASES)
    assert all(k in kernels for k in ("randn_kernel", "p_sample_kernel", "add_noise_kernel"))
    big = [c for c in de.CASES if c.big is not None]
    assert {c.kernel for c in big} == {"randn_kernel", "p_sample_kernel", "add_noise_kernel"}
    for c in big:
        assert de.TRIP < c.big <= de.TRIP + 16, (c.id, c.big)          # a second trip, and barely
        shape, = c.shapes
        assert int(np.prod(shape)) == c.big, c.id
        assert c.big * 4 <= 16 * 2**20 + 64, c.id                     # arrays of 16 MiB
    assert de.BY_ID["randn_big"].big - de.TRIP == 7                    # one whole quad and a 3-element tail
    for c in de.CASES:
        if c.path is None:
            continue
        assert c.path in c.id and c.path in ("vector", "scalar"), c.id
        for B, D in c.shapes:
            assert (D % 4 == 0) == (c.path == "vector"), c.id          # diffusion.hip: i0 + 4 <= n && D % 4 == 0
    rows = set(de.BY_ID["p_sample_rows"].shapes)
    assert rows >= {(1, 1), (1, 3), (5, 1), (4, 6), (3, 8), (2, 1001)} and rows == set(de.BY_ID["add_noise_rows"].shapes)
    assert any(D % 4 and (B * D) % 4 == 0 and B > 1 for B, D in rows)  # whole quads that straddle rows
    assert set(de.BY_ID["randn_small"].shapes) == {1, 2, 3, 4, 5, 7}
    (_, n), = de.BY_ID["counter"].shapes
    assert n == 19 and de.COUNTER_OFFSETS == (2**34 - 8, 2**64 - 8)
    assert all(o % 4 == 0 for o in de.COUNTER_OFFSETS + tuple(de.mse_offsets()))
    # the loss kernel's offsets: inside the first sample's whole chunk between two trips of one
    # four-trip pass (4 x 1024 elements), and inside its ragged chunk
    assert de.MSE_N % 4 == 0 and 16384 < de.MSE_N < 2 * 16384
    for w in (de.CARRY, de.WRAP):
        inside = sorted(w - o for o in de.mse_offsets() if 0 < w - o < de.MSE_N)
        assert len(inside) == 2 and inside[0] % 4096 in (1024, 2048, 3072) and 16384 < inside[1] < de.MSE_N
    assert de.HANDOFF_M * de.HANDOFF_K == de.CAST_TRIP + 2048
    assert sum(r * de.HANDOFF_K >= de.CAST_TRIP for r in de.HANDOFF_SPECIAL_ROWS) >= 1


def test_fused_counter_case_is_fused_and_straddles():
    c = de.smallest_fused_case()
    assert c.M > 64 and c.N % 4 == 0 and c.M * c.N > 2 * 4096          # the carry at element 4096 is mid-matrix
    assert all(c.M * c.N <= o.M * o.N for o in de.gk.MATRIX if o.M > 64 and o.N % 4 == 0)


def _nans(a):
    return int(np.isnan(a).sum())


@pytest.mark.parametrize("case,row", [("p_sample_specials_vector", 1), ("p_sample_specials_scalar", 2)])
def test_p_sample_specials_planned_nans(orc, case, row):
    (B, D), = de.BY_ID[case].shapes
    x, e, z, c, planned = de.p_sample_specials(B, D, row)
    ref = orc.p_sample(x, e, z, c, add_noise=True)
    assert _nans(ref) == planned == _nans(ref[row]) and 0 < planned < D
    for v in (x, e, z):                                                 # the row holds what it promises
        r = v[row]
        assert np.isnan(r).any() and np.isposinf(r).any() and np.isneginf(r).any()
        assert (r == 0).any() and np.signbit(r[r == 0]).any() and not np.signbit(r[r == 0]).all()
        assert (np.abs(r) == np.float32(1e-45)).any() and (np.abs(r) == np.float32(3e38)).any()
        assert np.isfinite(np.delete(v, row, axis=0)).all()
    assert np.isposinf(ref[row]).any() and np.isneginf(ref[row]).any()
    zeros = ref[row][ref[row] == 0]
    assert zeros.size >= 2 and np.signbit(zeros).any() and not np.signbit(zeros).all()
    if D % 4:                                                           # the tail quad holds a special element
        assert row == B - 1 and (B * D) % 4 and not np.isfinite(ref.ravel()[-1])


def test_add_noise_specials_planned_nans(orc):
    (B, D), = de.BY_ID["add_noise_specials"].shapes
    x, z, c, planned = de.add_noise_specials(B, D, row=2)
    ref = orc.add_noise(x, z, c)
    assert _nans(ref) == planned == _nans(ref[2]) and 0 < planned < D
    assert np.isposinf(ref[2]).any() and np.isneginf(ref[2]).any()
    zeros = ref[2][ref[2] == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    assert (B * D) % 4 and not np.isfinite(ref.ravel()[-1])


@pytest.mark.parametrize("inclusive", [False, True])
def test_schedule_planned_nans(orc, inclusive):
    betas = orc.beta_schedule(orc.BETA_LINEAR, 1000)
    for case in ("p_sample_schedule_vector", "p_sample_schedule_scalar"):
        (B, D), = de.BY_ID[case].shapes
        assert B == len(de.SCHEDULE_T) and D <= 16
        c = orc.p_sample_coeffs(betas, de.SCHEDULE_T, inclusive)
        assert np.isfinite(c[1:]).all() and np.isfinite(c[0]).all() == inclusive
        x, e = de.normal_inputs(B, D, 2, seed=D)
        for add in (False, True):
            assert _nans(orc.p_sample(x, e, np.ones_like(x), c, add_noise=add)) == de.schedule_nans(D, inclusive)
    assert np.isfinite(orc.add_noise_coeffs(betas, de.SCHEDULE_T, inclusive)).all()


@pytest.mark.parametrize("base", [de.CARRY, de.WRAP], ids=["carry", "wrap"])
def test_oracle_stream_splices(orc, base):
    """randn(s, off, n)[4k:] == randn(s, off + 4k, n - 4k) with off + 4k taken modulo 2^64, and the
    stream past the wrap is the stream from 0."""
    seed, n = 2**63 + 7, 19
    for back in (8, 4096):
        off = base - back
        m = max(n, back + n)
        whole = orc.randn(seed, off, m)
        for k in range(0, m // 4 + 1, max(1, m // 64)):
            part = orc.randn(seed, (off + 4 * k) % 2**64, m - 4 * k)
            assert np.array_equal(whole[4 * k:].view(np.uint32), part.view(np.uint32)), (back, k)
        at = orc.randn(seed, base % 2**64, n)                           # the elements from the carry / wrap on
        assert np.array_equal(whole[back:back + n].view(np.uint32), at.view(np.uint32))
    if base == de.WRAP:
        assert np.array_equal(orc.randn(3, 2**64 - 8, 16)[8:].view(np.uint32), orc.randn(3, 0, 8).view(np.uint32))
    # neighbouring blocks either side of the carry differ (a dropped high word would repeat them)
    lo, hi = orc.randn(seed, base % 2**64, 4), orc.randn(seed, (base + 2**34) % 2**64, 4)
    assert not np.array_equal(lo, hi)

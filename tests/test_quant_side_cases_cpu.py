"""CPU checks behind tests/test_gpu_quant_side_kernels.py: the case table's arithmetic (so a later
edit cannot shrink a case below the path it is there for), the two restatements of the reference
(C oracle and numpy) bit for bit on the value / parameter sets the GPU tests use, and
``onp.Calibration`` against a direct f32 scalar loop of calibrate.rs:42-69.

The library's host-slice entry points stage through device memory, so their three-way check
against both restatements is the GPU module's test_host_entry_points_agree_with_both_oracles."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import test_gpu_quant_side_kernels as sk

N = sk.HOST_N            # 5,003
SLACK = 1 << 20          # guard bytes, spare elements, params, workspace


def test_case_table_arithmetic():
    assert len({c.id for c in sk.CASES}) == len(sk.CASES)
    kernels = " ".join(c.kernel for c in sk.CASES)
    for k in ("default_quantize_kernel", "bit_quantize_kernel", "bit_dequantize_kernel", "dequantize_kernel",
              "adaptive_quantize_kernel", "decompress_rows_kernel", "compress_rows_kernel", "quantize_rows_cycle_kernel",
              "calib_hist_kernel", "pack_kernel", "unpack_kernel", "quantize_fused_kernel"):
        assert k in kernels, k
    for c in sk.CASES:
        assert c.src.startswith(sk.SRC + ":"), c.id
        assert c.id in sk.__doc__, c.id                       # every case is mapped to its table row
        if c.big is None:
            continue
        assert c.trip < c.big < 2 * c.trip, (c.id, c.trip, c.big)   # a second trip, and less than a whole one
        assert c.big * c.unit_bytes + SLACK < 80e6, (c.id, c.big * c.unit_bytes)
        assert all(s <= c.trip for s in c.sizes if c.id != "compress_rows"), c.id
    octet = [c for c in sk.CASES if c.trip == sk.OCTET_TRIP]
    assert len(octet) == 7
    for c in octet:                                            # one whole octet and a 5-element tail
        assert c.big - c.trip == 13 and c.sizes == (1, 7, 9, 257), c.id
    assert sk.BY_ID["adaptive_quantize"].big - sk.BY_ID["adaptive_quantize"].trip == 6
    assert sk.BY_ID["decompress_rows"].big % 257 == 0
    assert 65535 % 7 != 0 and sk.BY_ID["rows_cycle_rows"].big > 65535
    assert set(sk.CALIB_BINS) >= {1, 16384, 16385} and max(sk.CALIB_BINS) > 16385   # LDS limit on both sides
    sizes = [ch.size - 1 for ch in sk.calib_chunks()]
    assert sizes[:3] == [sk.BY_ID["calib_hist"].big, 1, 4099]


def test_mixed_input_holds_what_it_promises():
    for scale in (0.5, 0.37):
        x = sk.mixed_input(N, scale, 3, seed=0)
        assert x.size == N and x.dtype == np.float32
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        assert (x == 0).sum() >= 2 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
        tiny = np.abs(x[np.isfinite(x) & (x != 0)]).min()
        assert 0 < tiny < np.finfo(np.float32).tiny                 # a denormal
        assert np.abs(x[np.isfinite(x)]).max() == np.finfo(np.float32).max
    x = sk.mixed_input(N, 0.5, 0, seed=0)
    with np.errstate(all="ignore"):
        t = x[np.isfinite(x)] / np.float32(0.5)
        ties = (np.abs(np.fmod(t, np.float32(1.0))) == 0.5).sum()
    assert ties >= 40                                                # exact rounding ties at scale 0.5
    for n in (1, 7, 9):
        assert sk.mixed_input(n, 1.0, 0, seed=n).size == n


def test_default_quantizer_oracles_agree(orc, onp):
    codes = np.random.default_rng(0).integers(0, 256, N, dtype=np.uint8)
    for scale, zp in sk.DEFAULT_PARAMS:
        x = sk.mixed_input(N, scale, zp, seed=1)
        for qt in sk.QTYPES:
            assert np.array_equal(orc.default_quantize(x, qt, scale, zp), onp.default_quantize(x, qt, scale, zp)), (scale, zp, qt)
        assert sk.same_f32(orc.default_dequantize(codes, scale, zp), onp.default_dequantize(codes, scale, zp))


def test_bit_quantizer_oracles_agree(orc, onp):
    codes = np.random.default_rng(0).integers(0, 256, N, dtype=np.uint8)
    for scale, zp in sk.BIT_PARAMS:
        x = sk.mixed_input(N, scale, zp, seed=2)
        for bits in sk.BIT_WIDTHS:
            assert np.array_equal(orc.bit_quantize(x, bits, scale, zp), onp.bit_quantize(x, bits, scale, zp)), (scale, zp, bits)
        assert sk.same_f32(orc.bit_dequantize(codes, scale, zp), onp.bit_dequantize(codes, scale, zp))


def test_dequantize_pack_oracles_agree(orc, onp):
    rng = np.random.default_rng(3)
    for bits in range(1, 9):
        codes = rng.integers(0, 256, N, dtype=np.uint8)
        p = orc.pack_bits(codes, bits)
        assert np.array_equal(p, onp.pack_bits(codes, bits)) and p.size == orc.lib().orc_packed_bytes(N, bits)
        assert np.array_equal(orc.unpack_bits(p, N, bits), onp.unpack_bits(p, N, bits))
        assert np.array_equal(orc.unpack_bits(p, N, bits), codes & ((1 << bits) - 1))
        for s, z in sk.DEQ_PARAMS:
            assert sk.same_f32(orc.dequantize_tensor(codes, s, z), onp.dequantize_tensor(codes, np.float32(s), np.float32(z)))


def test_compress_vector_oracles_agree(orc, onp):
    for dim in sk.COMPRESS_DIMS + (N,):
        for row in sk.compress_rows_input(dim, seed=dim):
            for bits in sk.COMPRESS_BITS:
                (q, s, z), (nq, ns, nz) = orc.compress_vector(row, bits), onp.compress_vector(row, bits)
                assert np.array_equal(q, nq) and sk.same_f32(s, ns) and sk.same_f32(z, nz), (dim, bits)


def test_compress_rows_input_places_the_extremes():
    for dim in (257, 1000):
        rows = sk.compress_rows_input(dim, seed=dim)
        w3, late = rows[-2], rows[-1]
        assert 192 <= np.argmax(w3) < 256 and 192 <= np.argmin(w3) < 256
        assert np.argmax(late) >= 256 and (np.argmin(late) >= 256 or dim == 257)
        assert (rows[3] == rows[3][0]).all() and np.isnan(rows[4]).all()


def test_adaptive_quantizer_oracles_agree(orc, onp):
    for bits in sk.ADAPTIVE_BITS:
        a, b = orc.AdaptiveQuantizer(bits), onp.AdaptiveQuantizer(bits)
        g = np.random.default_rng(bits).standard_normal(4096).astype(np.float32) * 4
        a.update_stats(g)
        b.update_stats(g)
        (s, z), (ns, nz) = a.compute_params(), b.compute_params()
        assert sk.same_f32([s, z], [ns, nz]), bits
        x = sk.mixed_input(N, float(s) if np.isfinite(s) and s != 0 else 1.0, 0.0, seed=bits)
        assert np.array_equal(a.quantize(x)[0], b.quantize(x)[0]), bits


def test_quantize_vectors_oracles_agree(orc, onp):
    rng = np.random.default_rng(5)
    for req, shape in (([0, 1, 2, 3, 4, 6, 7], (75, 8)), (rng.integers(0, 8, 66).astype(np.uint8), (70, 41))):
        x = sk.log_uniform(rng, shape)
        (q, w), (nq, nw) = orc.quantize_vectors(x, sk.CFG_BITS, req), onp.quantize_vectors(x, sk.CFG_BITS, req)
        assert np.array_equal(q, nq) and np.array_equal(w, nw)
        top = ((1 << w.astype(np.int64)) - 1)[:, None]
        assert ((q > 0) & (q < top)).mean() > 0.1                  # the codes are not all 0 or at the clamp


# ---- calibrate.rs:42-69 as a scalar f32 loop --------------------------------------------------------

F32_MAX = float(np.finfo(np.float32).max)


def r32(v):
    """Rounds a double to f32 (overflow -> inf).  An f32 +, -, / computed exactly-rounded in double and
    rounded again is the correctly rounded f32 result (53 >= 2 * 24 + 2)."""
    return C.c_float(v).value


class ScalarCalibration:
    def __init__(self, num_bins):
        self.min, self.max = F32_MAX, -F32_MAX                          # :32-33
        self.num_bins, self.histogram, self.total_samples = num_bins, [0] * num_bins, 0

    def update(self, data):
        mn, mx = F32_MAX, -F32_MAX                                       # :43 fold; f32::min / max skip NaN
        for x in data:
            if x < mn:
                mn = x
            if x > mx:
                mx = x
        self.min = mn if mn < self.min else self.min                    # :47
        self.max = mx if mx > self.max else self.max                    # :48
        self.total_samples += len(data)                                  # :49
        if self.max > self.min:                                          # :59
            bw = r32(r32(self.max - self.min) / float(self.num_bins))    # :60
            for val in data:
                if val >= self.min and val <= self.max:                  # :62
                    q = r32(r32(val - self.min) / bw)                    # :63
                    if q != q or q <= 0.0:                               # `as usize`: NaN -> 0, negative -> 0
                        b = 0
                    elif q >= 18446744073709551616.0:                    # saturates at usize::MAX
                        b = (1 << 64) - 1
                    else:
                        b = int(math.floor(q))
                    self.histogram[min(b, self.num_bins - 1)] += 1       # :64-65


@pytest.mark.parametrize("bins", sk.CALIB_BINS)
def test_calibration_matches_scalar_loop(onp, bins):
    ref, cal = ScalarCalibration(bins), onp.Calibration(bins)
    for i, ch in enumerate(sk.calib_chunks()):
        ch = ch[1:] if i % 2 == 0 else ch[:-1]
        ref.update(ch.tolist())
        cal.update(ch)
        assert np.float32(ref.min) == cal.min and np.float32(ref.max) == cal.max, (bins, i)
        assert np.array_equal(np.array(ref.histogram, np.uint64), cal.histogram), (bins, i)
        assert ref.total_samples == cal.total_samples and int(cal.histogram.sum()) <= cal.total_samples
    assert np.isinf(cal.max) and np.isinf(cal.min)                       # the last chunk's +-inf were folded


def test_calibration_widening_and_special_chunks(onp):
    """The chunks do what the GPU test needs of them: the second and third widen the range, the
    fourth overflows max - min, the fifth holds +-inf, and the numpy restatement bins them (NaN index
    -> bin 0, as calibrate.rs:63's `as usize`) instead of raising."""
    cal = onp.Calibration(10)
    ch = sk.calib_chunks()
    cal.update(ch[0][1:])
    mn0, mx0 = cal.min, cal.max
    cal.update(ch[1][:-1])
    assert cal.max > mx0 and cal.min == mn0
    cal.update(ch[2][1:])
    assert cal.min < mn0
    before = cal.histogram.copy()
    cal.update(ch[3][:-1])
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(cal.max) - np.float32(cal.min)) and np.isfinite(cal.max)
    assert cal.histogram[0] - before[0] == 1000 and (cal.histogram[1:] == before[1:]).all()
    cal.update(ch[4][1:])
    assert cal.histogram[0] - before[0] == 1000 + 999                    # NaN is outside [min, max]

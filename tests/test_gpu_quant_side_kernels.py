"""The quantizer's side kernels (csrc/quant_kernels.hip, rows a4 / a8 / a10 / f4 of the coverage
table) through their C-ABI entry points, at the sizes where indexing can go wrong: a second trip
of every grid-stride loop at its capped grid, every wave of a block, unaligned bases, and the
bytes around every output.

Reference: the C oracle (``orc``); ``onp.Calibration`` for a10.  Bar: codes, packed bytes,
histograms, scales and zero points bit-exact; f32 outputs bit-exact; f16 outputs equal to the RNE
of the f32 reference.  The one relaxation, written down here: where the reference itself produces
a NaN (0/0 of a constant row, inf - inf of an all-NaN row) only "is NaN" is compared, because IEEE
754 leaves the sign and payload of an invalid operation's NaN to the implementation (x86 gives the
negative quiet NaN, the GPU the positive one) and the Rust source never inspects them.

``CASES`` is plain data and imports without a GPU (tests/test_quant_side_cases_cpu.py checks its
arithmetic and the two oracles on the same inputs on any machine).  "trip" = elements one pass of
the kernel's grid-stride loop covers at its capped grid, hard-coded with the source line it was
read from; every ``big`` size is one trip plus a ragged remainder (one whole octet and a 5-element
tail for the octet kernels), the smallest size at which the loop's stride is executed at all.

Every output lives inside a larger device buffer pre-filled with a sentinel byte; after each call
the 64 bytes before and after the output's exact extent (``dllm_packed_bytes`` for packed codes)
must still hold the sentinel.  Each kernel is called with every pointer aligned and again with the
input shifted by one element and the output by 1..7 bytes (codes), 4 bytes (f32) or 2 bytes (f16),
which selects the non-vector load/store paths of load_octet / store_codes / load_codes / store_f8.

Coverage table row -> case ids (previously unexecuted path):

* default_quantize_kernel -> ``default_quantize`` (second trip at 8,388,621; vec_in/vec_out = 0;
  rounding ties, +-0, denormals, both clamp sides, degenerate scales)
* bit_quantize_kernel, bit_dequantize_kernel -> ``bit_quantize``, ``bit_dequantize`` (second trip,
  partial tail octet after a full trip, f16 output, unaligned bases)
* dequantize_kernel -> ``dequantize`` (second trip at f16 output and at the odd width 3: no
  existing test dequantizes more than 1 << 20 elements against the oracle), ``default_dequantize``
* adaptive_quantize_kernel -> ``adaptive_quantize`` (second trip; byte-store fallback at an output
  offset by 1 byte beside the aligned word store)
* decompress_rows_kernel -> ``decompress_rows`` (second trip, i / dim with dim = 257)
* compress_rows_kernel -> ``compress_rows`` (extremes only in wave 3; only in the second column
  trip; dims 1, 63, 65, 257, 1000)
* quantize_rows_cycle_kernel -> ``rows_cycle_columns`` (gridDim.x = 64 and the column stride),
  ``rows_cycle_rows`` (second launch with the rotated table, cycle 7 does not divide 65,535)
* long-cycle branch of dllm_quantize_vectors -> ``long_cycle`` (rows at unaligned addresses,
  dim 41), ``long_cycle_columns`` (second trip at dim 131,085)
* calib_hist_kernel -> ``calib_hist`` (second trip; global-atomic path at 16,385 and 20,000 bins;
  16,384 bins = 64 KiB of LDS; one bin; min/max widening between chunks; +-inf and overflow)
* pack_kernel, unpack_kernel -> ``pack``, ``unpack`` (second trip against the oracle, unaligned
  bases; ``unpack`` at 4 bits is run past one trip by test_head_parallel_kv_cache_bitexact, but
  only against another unpack, so the case stays)
* main quantizer, no guard check before -> ``quantize_tensor_guard`` (fused and generic path,
  single, pair and with-params forms, packed widths 1..8 at n = 7, 9, 1003)
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

SRC = "diffusion-llm-rs_amd/csrc/quant_kernels.hip"
OCTET_TRIP = 4096 * 256 * 8      # octet_grid(): kCUs * 16 blocks x kBlock threads x 8 elements
SMALL = (1, 7, 9, 257)

# id, kernel, trip (elements per trip; None: no loop under test), src (where the grid was read),
# sizes (the small sizes / dims), big (one trip plus a ragged remainder, in the units of `trip`),
# unit_bytes (device bytes of inputs plus outputs per counted unit of `big`; pack and unpack share
# their three buffers).
Case = namedtuple("Case", "id kernel trip src sizes big unit_bytes")

CASES = [Case(*c) for c in [
    ("default_quantize", "default_quantize_kernel", OCTET_TRIP, SRC + ":858 (octet_grid), launch :1238",
     SMALL, OCTET_TRIP + 13, 4 + 1),
    ("bit_quantize", "bit_quantize_kernel", OCTET_TRIP, SRC + ":858, launch :1352", SMALL, OCTET_TRIP + 13, 4 + 1),
    ("bit_dequantize", "bit_dequantize_kernel", OCTET_TRIP, SRC + ":858, launch :1362", SMALL, OCTET_TRIP + 13, 1 + 4),
    ("dequantize", "dequantize_kernel", OCTET_TRIP, SRC + ":858, launch :1184", SMALL, OCTET_TRIP + 13, 1 + 4),
    ("default_dequantize", "dequantize_kernel", OCTET_TRIP, SRC + ":858, launch :1184 via :1247", SMALL,
     OCTET_TRIP + 13, 1 + 4),
    ("pack", "pack_kernel", OCTET_TRIP, SRC + ":858, launch :1212", SMALL, OCTET_TRIP + 13, 1 + 1 + 1),
    ("unpack", "unpack_kernel", OCTET_TRIP, SRC + ":858, launch :1221", SMALL, OCTET_TRIP + 13, 1 + 1 + 1),
    ("adaptive_quantize", "adaptive_quantize_kernel", 4096 * 256 * 4, SRC + ":1312 (kCUs * 16 blocks, 4 per thread)",
     SMALL, 4096 * 256 * 4 + 6, 4 + 1),
    ("decompress_rows", "decompress_rows_kernel", 4096 * 256, SRC + ":1436 (kCUs * 16 blocks, 1 per thread)",
     (1, 63, 65, 257, 1000), 4081 * 257, 1 + 4 + 4 + 1),      # big: 4081 rows of dim 257, through compress first
    ("compress_rows", "compress_rows_kernel", 256, SRC + ":732, :742 (one block per row, kBlock columns per trip)",
     (1, 63, 65, 257, 1000), 257, 4 + 1),
    ("rows_cycle_columns", "quantize_rows_cycle_kernel", 64 * 256, SRC + ":1384 (64 blocks along x), stride :718",
     (), 64 * 256 + 5, 3 * (4 + 1)),                           # 3 rows
    ("rows_cycle_rows", "quantize_rows_cycle_kernel", 65535, SRC + ":1393 (65,535 rows per launch)",
     (), 65535 + 70, 8 * (4 + 1)),                             # dim 8
    ("long_cycle", "bit_quantize_kernel", 64 * 256 * 8, SRC + ":1412 (64 blocks, 8 per thread)", (41,), None, 4 + 1),
    ("long_cycle_columns", "bit_quantize_kernel", 64 * 256 * 8, SRC + ":1412", (), 64 * 256 * 8 + 13, 66 * (4 + 1)),
    ("calib_hist", "calib_hist_kernel", 1024 * 256, SRC + ":1266 (kCUs * 4 blocks, 1 per thread)",
     (1, 4099), 1024 * 256 + 77, 4),
    ("quantize_tensor_guard", "quantize_fused_kernel, quantize_tensor_kernel, quantize_pair_kernel", None,
     SRC + ":1111-1176, :1457-1479", (7, 9, 1003), None, 4 + 2),
]]
BY_ID = {c.id: c for c in CASES}

# ---- values and parameters (shared with tests/test_quant_side_cases_cpu.py) ----------------------

FLT_MAX = float(np.finfo(np.float32).max)
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30, FLT_MAX, -FLT_MAX, 1e-40, -1e-40], np.float32)

DEFAULT_PARAMS = [(1.0, 0), (0.37, 3), (0.5, -5), (1e-30, 0), (-0.25, 100)]          # (scale, zero_point: i32)
QTYPES = (0, 1, 2, 3)                                                                  # Int8, Int4, Binary, Float8
BIT_PARAMS = [(0.05, -1.0), (float(np.float32(1.0) / np.float32(15.0)), 0.0), (1e-30, 0.0), (-0.5, 2.0)]
BIT_WIDTHS = (1, 2, 4, 8, 12, 16, 30)
ADAPTIVE_BITS = (0, 9, 12, 16, 25, 31)
COMPRESS_DIMS = (1, 63, 65, 257, 1000)
COMPRESS_BITS = (4, 8, 16)
CALIB_BINS = (1, 10, 16384, 16385, 20000)
CFG_BITS = (4, 6, 8, 16)                                                               # SystemConfig default


def mixed_input(n, scale, zp, seed):
    """n f32 values: NaN, +-inf, +-0, +-1e30, +-FLT_MAX, +-1e-40 (a denormal), every k/2 * scale for
    k = -40..40 (x / scale on an exact rounding tie at scale 0.5, beside one at 0.37), every
    zp + k * scale (a truncating quantizer's code boundaries), then N(0, 1) * 4.  Sizes below the
    173 listed values take a strided selection of them that depends on the seed."""
    k = np.arange(-40, 41, dtype=np.float32)
    with np.errstate(all="ignore"):
        ties = (k / np.float32(2.0)) * np.float32(scale)
        steps = np.float32(zp) + k * np.float32(scale)
    head = np.concatenate([SPECIALS, ties, steps]).astype(np.float32)
    if n <= head.size:
        return head[(np.arange(n) * 19 + seed) % head.size].copy()
    rng = np.random.default_rng(seed)
    return np.concatenate([head, (rng.standard_normal(n - head.size) * 4).astype(np.float32)])


def compress_rows_input(dim, seed):
    """Rows of one dim for compress_vector: Gaussian rows, a constant row (scale 0: the reference
    divides 0/0), an all-NaN row, a row starting with the special values, a row whose maximum and
    minimum sit only in columns 192..255 (wave 3 of the block), and one with them only in the
    second column trip (columns >= 256; at dim 257 only the maximum fits there).  dim 1 makes
    every row a one-element row."""
    rng = np.random.default_rng(seed)
    rows = [(rng.standard_normal(dim) * 3).astype(np.float32) for _ in range(3)]
    rows.append(np.full(dim, 2.5, np.float32))
    rows.append(np.full(dim, np.nan, np.float32))
    sp = (rng.standard_normal(dim) * 2).astype(np.float32)
    sp[:min(dim, SPECIALS.size)] = SPECIALS[:dim]
    rows.append(sp)
    sp2 = (rng.standard_normal(dim) * 2).astype(np.float32)          # finite extremes beside NaN and +-0
    sp2[:min(dim, 3)] = np.array([np.nan, 0.0, -0.0], np.float32)[:dim]
    rows.append(sp2)
    if dim >= 256:
        w3 = rng.uniform(-1, 1, dim).astype(np.float32)
        w3[200], w3[250] = 50.0, -60.0
        rows.append(w3)
    if dim > 256:
        late = rng.uniform(-1, 1, dim).astype(np.float32)
        late[256 + (dim - 257) // 2] = 70.0
        late[dim - 1 if dim > 257 else 199] = -80.0 if dim > 257 else -1.5
        rows.append(late)
    return np.stack(rows)


def calib_chunks(seed=3):
    """Three updates of 262,144 + 77, 1 and 4,099 elements with growing range (the second widens
    the maximum, the third the minimum, so later chunks bin with a new width while the counts
    accumulate), then a chunk whose range overflows f32 (max - min = inf) and one with +-inf and
    NaN.  Every chunk carries one spare element: the tests drop the first one of the even chunks
    (a base shifted by 4 bytes) and the last one of the odd chunks."""
    rng = np.random.default_rng(seed)
    c0 = rng.standard_normal(1024 * 256 + 77 + 1).astype(np.float32)
    c1 = np.array([7.5, 0.0], np.float32)
    c2 = (rng.standard_normal(4099 + 1) * 3 - 2).astype(np.float32)
    c2[17] = -20.0
    c3 = (rng.standard_normal(1000 + 1) * 5).astype(np.float32)
    c3[[5, 500]] = [-3e38, 3e38]
    c4 = (rng.standard_normal(1000 + 1) * 5).astype(np.float32)
    c4[[3, 77, 900]] = [np.inf, -np.inf, np.nan]
    return [c0, c1, c2, c3, c4]


def log_uniform(rng, shape):
    """|x| log-uniform in [1e-6, 2) with a few negatives and special values: with the prefill scales
    1 / (2^b - 1) every code from 0 to the clamp occurs, so a wrong (scale, max_val) slot shows."""
    x = (10.0 ** rng.uniform(-6, 0.3, shape)).astype(np.float32)
    flat = x.reshape(-1)
    flat[np.unique(rng.integers(0, flat.size, max(flat.size // 50, 1)))] *= -1
    flat[rng.integers(0, flat.size, SPECIALS.size)] = SPECIALS
    return x


def same_f32(a, b):
    """Bit-identical f32, or NaN in both (see the module docstring)."""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- device buffers with guard bytes ---------------------------------------------------------------

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 64
PAD = 128     # the output starts PAD + offset bytes into its buffer: a guard and room for the offsets
MAX_TEST_BYTES = 80e6
_allocated = []   # bytes of every In / Out buffer of the running test


@pytest.fixture(autouse=True)
def _device_bytes_per_test():
    """No test allocates 80 MB or more of inputs and outputs (the sizes are the smallest that reach
    each path, not workload sizes)."""
    _allocated.clear()
    yield
    assert sum(_allocated) < MAX_TEST_BYTES, sum(_allocated)


class Out:
    """An output of exactly ``nbytes`` at ``off`` bytes past a 128-byte aligned address, inside a
    larger device buffer filled with SENT before every call; ``read`` checks the guard bytes."""

    def __init__(self, torch, cap):
        self.t = torch.empty(PAD + cap + 16 + PAD, dtype=torch.uint8, device="cuda")
        _allocated.append(self.t.numel())
        assert self.t.data_ptr() % 128 == 0

    def place(self, nbytes, off=0, zero=False):
        assert 0 <= off < 16 and PAD + off + nbytes + GUARD <= self.t.numel()
        self.t.fill_(SENT)
        self.nbytes, self.off = nbytes, off
        if zero:
            self.t[PAD + off:PAD + off + nbytes].zero_()
        return self.t.data_ptr() + PAD + off

    def view(self, torch_dtype):
        return self.t[PAD + self.off:PAD + self.off + self.nbytes].view(torch_dtype)

    def read(self, dtype=np.uint8):
        h = self.t.cpu().numpy()
        a, b = PAD + self.off, PAD + self.off + self.nbytes
        assert (h[a - GUARD:a] == SENT).all(), "bytes before the output were overwritten"
        assert (h[b:b + GUARD] == SENT).all(), "bytes after the output were overwritten"
        return h[a:b].copy().view(dtype)


class In:
    """A device input placed ``off`` bytes past a 128-byte aligned address."""

    def __init__(self, torch, cap):
        self.torch = torch
        self.t = torch.zeros(cap + 32, dtype=torch.uint8, device="cuda")
        _allocated.append(self.t.numel())
        assert self.t.data_ptr() % 128 == 0

    def put(self, arr, off=0):
        b = np.ascontiguousarray(arr).view(np.uint8).ravel()
        assert off + b.size <= self.t.numel()
        self.t[off:off + b.size].copy_(self.torch.from_numpy(b))
        return self.t.data_ptr() + off


@pytest.fixture(scope="module")
def gpu(dllm, cuda):
    import torch

    class G:
        L = dllm._lib.load()
        check = staticmethod(dllm._lib.check)

        @staticmethod
        def stream():
            return torch.cuda.current_stream().cuda_stream
    G.torch = torch
    return G


CODE_VARIANTS = [(0, 0), (1, 0), (0, 4)] + [(1, o) for o in range(1, 8)]   # (input shift in elements, output offset)


def _codes_kernel(gpu, n, x1, call, ref, variants):
    """x1 holds n + 1 values; each variant runs the n values from x1[shift] at a base shifted by as
    many f32 elements into an output at its byte offset and compares the n code bytes."""
    xin, out = In(gpu.torch, 4 * (n + 1)), Out(gpu.torch, n)
    for shift, off in variants:
        xs = x1[shift:shift + n]
        xp = xin.put(xs, 4 * shift)
        gpu.check(call(xp, out.place(n, off)))
        assert np.array_equal(out.read(), ref(xs)), (n, shift, off)


# ---- a4: DefaultQuantizer ----------------------------------------------------------------------------

def _default_quantize(gpu, orc, n, combos, variants):
    for (scale, zp), qt in combos:
        x1 = mixed_input(n + 1, scale, zp, seed=n % 1000 + qt)
        _codes_kernel(gpu, n, x1,
                      lambda xp, op: gpu.L.dllm_default_quantize(xp, n, qt, scale, zp, op, gpu.stream()),
                      lambda xs: orc.default_quantize(xs, qt, scale, zp), variants)


def test_default_quantize_small(gpu, orc):
    for n in BY_ID["default_quantize"].sizes:
        _default_quantize(gpu, orc, n, [(p, qt) for p in DEFAULT_PARAMS for qt in QTYPES], CODE_VARIANTS)


@pytest.mark.parametrize("params,qt", [((0.5, -5), 0), ((0.37, 3), 1)])
def test_default_quantize_second_trip(gpu, orc, params, qt):
    _default_quantize(gpu, orc, BY_ID["default_quantize"].big, [(params, qt)], [(0, 0), (1, 3)])


def test_default_dequantize(gpu, orc):
    c = BY_ID["default_dequantize"]
    rng = np.random.default_rng(4)
    for n in c.sizes + (c.big,):
        q = rng.integers(0, 256, n, dtype=np.uint8)
        qin, out = In(gpu.torch, n + 1), Out(gpu.torch, 4 * n)
        for scale, zp in (DEFAULT_PARAMS if n < c.big else DEFAULT_PARAMS[1:2]):
            ref = orc.default_dequantize(q, scale, zp)
            for shift, off in ((0, 0), (1, 4)):
                gpu.check(gpu.L.dllm_default_dequantize(qin.put(q, shift), n, scale, zp, out.place(4 * n, off),
                                                        gpu.stream()))
                assert same_f32(out.read(np.float32), ref), (n, scale, zp, shift, off)


# ---- a8-ii: BitQuantizer ------------------------------------------------------------------------------

def _bit_quantize(gpu, orc, n, combos, variants):
    for (scale, zp), bits in combos:
        x1 = mixed_input(n + 1, scale, zp, seed=n % 1000 + bits)
        _codes_kernel(gpu, n, x1,
                      lambda xp, op: gpu.L.dllm_bit_quantize(xp, n, bits, scale, zp, op, gpu.stream()),
                      lambda xs: orc.bit_quantize(xs, bits, scale, zp), variants)


def test_bit_quantize_small(gpu, orc):
    for n in BY_ID["bit_quantize"].sizes:
        _bit_quantize(gpu, orc, n, [(p, b) for p in BIT_PARAMS for b in BIT_WIDTHS], CODE_VARIANTS)


@pytest.mark.parametrize("params,bits", [(BIT_PARAMS[0], 8), (BIT_PARAMS[3], 30)])
def test_bit_quantize_second_trip(gpu, orc, params, bits):
    _bit_quantize(gpu, orc, BY_ID["bit_quantize"].big, [(params, bits)], [(0, 0), (1, 3)])


def _f_out(gpu, call, n, f16, off, ref32):
    """Runs call(out_ptr, dtype) into a guarded f32 / f16 output and compares with the f32 reference
    (f16: its RNE)."""
    esz = 2 if f16 else 4
    out = Out(gpu.torch, esz * n)
    gpu.check(call(out.place(esz * n, off), 1 if f16 else 0))
    with np.errstate(over="ignore"):
        exp = ref32.astype(np.float16) if f16 else ref32
    got = out.read(np.float16 if f16 else np.float32)
    assert got.tobytes() == exp.tobytes()


def _bit_dequantize(gpu, orc, n, combos):
    rng = np.random.default_rng(n % 1000)
    q = rng.integers(0, 256, n, dtype=np.uint8)
    qin = In(gpu.torch, n + 1)
    for (scale, zp), f16, shift in combos:
        qp = qin.put(q, shift)
        _f_out(gpu, lambda op, dt: gpu.L.dllm_bit_dequantize(qp, n, scale, zp, op, dt, gpu.stream()), n, f16,
               (2 if f16 else 4) * shift, orc.bit_dequantize(q, scale, zp))


def test_bit_dequantize_small(gpu, orc):
    for n in BY_ID["bit_dequantize"].sizes:
        _bit_dequantize(gpu, orc, n, [(p, f16, s) for p in BIT_PARAMS for f16 in (0, 1) for s in (0, 1)])


@pytest.mark.parametrize("params,f16,shift", [(BIT_PARAMS[0], 1, 0), (BIT_PARAMS[1], 0, 1), (BIT_PARAMS[3], 1, 1)])
def test_bit_dequantize_second_trip(gpu, orc, params, f16, shift):
    _bit_dequantize(gpu, orc, BY_ID["bit_dequantize"].big, [(params, f16, shift)])


# ---- a2: dequantize_kernel, a6: pack / unpack -----------------------------------------------------------

DEQ_PARAMS = [(0.37, 3.0), (1e-30, 0.0), (-0.25, 100.0)]


def _dequantize(gpu, orc, n, bits, packed, f16, shift, scale, zp, by_tensor):
    rng = np.random.default_rng(n % 1000 + bits)
    codes = rng.integers(0, 1 << bits, n, dtype=np.uint8)
    stream = orc.pack_bits(codes, bits) if packed else codes
    assert stream.size == (gpu.L.dllm_packed_bytes(n, bits) if packed else n)
    qin = In(gpu.torch, stream.size + 1)          # stays alive until the call has been read back
    qp = qin.put(stream, shift)
    ref = orc.dequantize_tensor(codes, scale, zp)
    if by_tensor:
        pr = gpu.torch.tensor([scale, zp], dtype=gpu.torch.float32, device="cuda")
        call = lambda op, dt: gpu.L.dllm_dequantize_tensor(qp, n, bits, packed, pr.data_ptr(), op, dt, gpu.stream())  # noqa: E731
    else:
        call = lambda op, dt: gpu.L.dllm_dequantize_tensor_scalar(qp, n, bits, packed, scale, zp, op, dt, gpu.stream())  # noqa: E731
    _f_out(gpu, call, n, f16, (2 if f16 else 4) * shift, ref)


def test_dequantize_small(gpu, orc):
    for n in BY_ID["dequantize"].sizes:
        for bits in range(1, 9):
            for packed in (0, 1):
                for f16 in (0, 1):
                    for shift in (0, 1):
                        for i, (s, z) in enumerate(DEQ_PARAMS):
                            _dequantize(gpu, orc, n, bits, packed, f16, shift, s, z, by_tensor=(i == 0))


@pytest.mark.parametrize("bits,f16,shift,by_tensor", [(4, 1, 0, 1), (3, 0, 1, 0), (3, 1, 0, 0)])
def test_dequantize_second_trip(gpu, orc, bits, f16, shift, by_tensor):
    _dequantize(gpu, orc, BY_ID["dequantize"].big, bits, 1, f16, shift, *DEQ_PARAMS[0], by_tensor=by_tensor)


def _pack_unpack(gpu, orc, n, bits, variants):
    rng = np.random.default_rng(n % 1000 + bits)
    codes = rng.integers(0, 256, n, dtype=np.uint8)           # pack masks every code to its width
    packed = orc.pack_bits(codes, bits)
    nb = gpu.L.dllm_packed_bytes(n, bits)
    assert packed.size == nb
    cin, pin, out = In(gpu.torch, n + 1), In(gpu.torch, nb + 1), Out(gpu.torch, n)
    for shift, off in variants:
        gpu.check(gpu.L.dllm_pack(cin.put(codes, shift), n, bits, out.place(nb, off), gpu.stream()))
        assert np.array_equal(out.read(), packed), ("pack", n, bits, shift, off)
        gpu.check(gpu.L.dllm_unpack(pin.put(packed, shift), n, bits, out.place(n, off), gpu.stream()))
        assert np.array_equal(out.read(), codes & ((1 << bits) - 1)), ("unpack", n, bits, shift, off)


def test_pack_unpack_small(gpu, orc):
    for n in BY_ID["pack"].sizes:
        for bits in range(1, 9):
            _pack_unpack(gpu, orc, n, bits, [(0, 0), (1, 0), (0, 4)] + [(1, o) for o in range(1, 8)])


@pytest.mark.parametrize("bits", [4, 3])
def test_pack_unpack_second_trip(gpu, orc, bits):
    assert BY_ID["pack"].big == BY_ID["unpack"].big
    _pack_unpack(gpu, orc, BY_ID["pack"].big, bits, [(0, 0), (1, 3)])


# ---- f4: AdaptiveQuantizer at bits 0, 9..31 -----------------------------------------------------------

@pytest.mark.parametrize("bits", ADAPTIVE_BITS)
def test_adaptive_quantize(gpu, orc, bits):
    c = BY_ID["adaptive_quantize"]
    ref_q = orc.AdaptiveQuantizer(bits)
    ref_q.update_stats(np.random.default_rng(bits).standard_normal(4096).astype(np.float32) * 4)
    s, z = ref_q.compute_params()
    pr = gpu.torch.tensor([float(s), float(z)], dtype=gpu.torch.float32, device="cuda")
    assert same_f32(pr.cpu().numpy(), [s, z])

    def ref(xs):
        out = np.zeros(xs.size, np.uint8)
        assert orc.lib().orc_adaptive_quantize(xs.ctypes.data, xs.size, bits, float(s), float(z), out.ctypes.data) == 0
        return out
    for n in c.sizes + (c.big,):
        x1 = mixed_input(n + 1, float(s) if np.isfinite(s) and s != 0 else 1.0, 0.0, seed=bits + n % 1000)
        variants = [(0, 0), (1, 1)] if n == c.big else [(sh, o) for sh in (0, 1) for o in range(4)]
        _codes_kernel(gpu, n, x1,
                      lambda xp, op: gpu.L.dllm_adaptive_quantize(xp, n, bits, pr.data_ptr(), 0, op, gpu.stream()),
                      lambda xs: ref(np.ascontiguousarray(xs)), variants)


# ---- a8-iii: compress_vector / decompress over rows ---------------------------------------------------

def _compress_decompress(gpu, orc, x, bits, shift, off):
    rows, dim = x.shape
    refs = [orc.compress_vector(r, bits) for r in x]
    rq = np.stack([r[0] for r in refs])
    rs, rz = np.array([r[1] for r in refs], np.float32), np.array([r[2] for r in refs], np.float32)
    xin = In(gpu.torch, x.nbytes + 4)
    xp = xin.put(x, 4 * shift)
    oq, osc, ozp = Out(gpu.torch, rows * dim), Out(gpu.torch, 4 * rows), Out(gpu.torch, 4 * rows)
    gpu.check(gpu.L.dllm_compress_vectors(xp, rows, dim, bits, oq.place(rows * dim, off), osc.place(4 * rows, 4 * shift),
                                          ozp.place(4 * rows, 4 * shift), gpu.stream()))
    got_s, got_z = osc.read(np.float32), ozp.read(np.float32)
    bad = [i for i in range(rows) if not (same_f32(got_s[i], rs[i]) and same_f32(got_z[i], rz[i]))]
    assert not bad, ("scale / zero point of rows", bad[:8], dim, bits)
    got_q = oq.read().reshape(rows, dim)
    assert np.array_equal(got_q, rq), ("codes of rows", np.flatnonzero((got_q != rq).any(axis=1))[:8], dim, bits)
    # decompress the reference's codes with the reference's scales and zero points
    exp = np.stack([orc.bit_dequantize(rq[i], rs[i], rz[i]) for i in range(rows)])
    qin, sin, zin = In(gpu.torch, rows * dim + 1), In(gpu.torch, 4 * rows + 4), In(gpu.torch, 4 * rows + 4)
    qp, sp, zp = qin.put(rq, shift), sin.put(rs, 4 * shift), zin.put(rz, 4 * shift)
    oy = Out(gpu.torch, 4 * rows * dim)
    gpu.check(gpu.L.dllm_decompress_vectors(qp, rows, dim, sp, zp, oy.place(4 * rows * dim, 4 * shift), gpu.stream()))
    assert same_f32(oy.read(np.float32), exp), ("decompress", dim, bits)


@pytest.mark.parametrize("dim", COMPRESS_DIMS)
def test_compress_decompress_rows(gpu, orc, dim):
    x = compress_rows_input(dim, seed=dim)
    for bits in COMPRESS_BITS:
        for shift, off in ((0, 0), (1, 3)):
            _compress_decompress(gpu, orc, x, bits, shift, off)


def test_decompress_rows_second_trip(gpu, orc):
    c = BY_ID["decompress_rows"]
    dim = 257
    rows = c.big // dim
    assert rows * dim == c.big
    x = (np.random.default_rng(9).standard_normal((rows, dim)) * 2).astype(np.float32)
    x[::5] *= np.float32(7.0)
    special = compress_rows_input(dim, seed=1)
    x[-special.shape[0]:] = special                      # the rows of the second trip include the special ones
    _compress_decompress(gpu, orc, x, 8, 0, 0)


# ---- a8-ii: PrefillKVQuant::quantize_vectors ----------------------------------------------------------

def _quantize_vectors(gpu, orc, x, req, variants):
    rows, dim = x.shape
    cfg = np.array(CFG_BITS, np.uint8)
    req = np.ascontiguousarray(req, np.uint8)
    rq, rw = orc.quantize_vectors(x, cfg, req)
    xin, out = In(gpu.torch, x.nbytes + 4), Out(gpu.torch, rows * dim)
    for shift, off in variants:
        widths = np.full(rows + 2, SENT, np.uint8)
        gpu.check(gpu.L.dllm_quantize_vectors(xin.put(x, 4 * shift), rows, dim, cfg.ctypes.data, cfg.size,
                                              req.ctypes.data, req.size, out.place(rows * dim, off),
                                              widths.ctypes.data + 1, gpu.stream()))
        got = out.read().reshape(rows, dim)
        assert np.array_equal(got, rq), ("rows", np.flatnonzero((got != rq).any(axis=1))[:8], shift, off)
        assert np.array_equal(widths[1:-1], rw) and widths[0] == SENT and widths[-1] == SENT


def test_quantize_vectors_column_stride(gpu, orc):
    """Short cycle, dim = 16,384 + 5: gridDim.x = 64 and each thread's second column."""
    x = log_uniform(np.random.default_rng(1), (3, BY_ID["rows_cycle_columns"].big))
    _quantize_vectors(gpu, orc, x, [2, 4], [(0, 0), (1, 3)])


def test_quantize_vectors_second_launch(gpu, orc):
    """Short cycle, 65,535 + 70 rows of dim 8, cycle length 7: 65,535 % 7 = 1, so the second launch
    starts mid-cycle and needs the rotated table."""
    req = [0, 1, 2, 3, 4, 6, 7]
    assert 65535 % len(req) != 0
    x = log_uniform(np.random.default_rng(2), (BY_ID["rows_cycle_rows"].big, 8))
    _quantize_vectors(gpu, orc, x, req, [(0, 0), (1, 3)])


def test_quantize_vectors_long_cycle(gpu, orc):
    """66 request entries (> 64 slots: one launch per row), dim 41: rows start at every alignment."""
    rng = np.random.default_rng(3)
    req = rng.integers(0, 8, 66).astype(np.uint8)
    x = log_uniform(rng, (70, BY_ID["long_cycle"].sizes[0]))
    _quantize_vectors(gpu, orc, x, req, [(0, 0), (1, 3)])


def test_quantize_vectors_long_cycle_second_trip(gpu, orc):
    """The long-cycle branch past its 64-block grid: dim = 131,072 + 13, the 66 rows it needs."""
    rng = np.random.default_rng(4)
    req = rng.integers(0, 8, 66).astype(np.uint8)
    x = log_uniform(rng, (66, BY_ID["long_cycle_columns"].big))
    _quantize_vectors(gpu, orc, x, req, [(0, 0)])


# ---- a10: CalibrationData::update ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def calib_reference(onp):
    """Per bin count: the numpy restatement's (min, max, histogram, total_samples) after each chunk."""
    chunks = calib_chunks()
    states = {}
    for bins in CALIB_BINS:
        cal, st = onp.Calibration(bins), []
        for i, ch in enumerate(chunks):
            cal.update(ch[1:] if i % 2 == 0 else ch[:-1])
            st.append((np.array([cal.min, cal.max], np.float32), cal.histogram.astype(np.int64).copy(), cal.total_samples))
        states[bins] = st
    return chunks, states


@pytest.mark.parametrize("bins", CALIB_BINS)
def test_calibration_updates(gpu, dllm, calib_reference, bins):
    torch = gpu.torch
    chunks, states = calib_reference
    cal = dllm.CalibrationData.new(bins, False)
    ost, oh = Out(torch, 8), Out(torch, 8 * bins)
    ost.place(8)
    st = ost.view(torch.float32)
    st.copy_(cal._stats)
    oh.place(8 * bins, zero=True)
    cal._stats, cal._hist = st, oh.view(torch.int64)          # the wrapper's own state, inside guard bytes
    for i, ch in enumerate(chunks):
        t = torch.from_numpy(ch).cuda()
        cal.update(t[1:] if i % 2 == 0 else t[:-1])           # even chunks from a base shifted by 4 bytes
        rmm, rh, rn = states[bins][i]
        assert ost.read(np.float32).tobytes() == rmm.tobytes(), (bins, i)
        got = oh.read(np.int64)
        assert np.array_equal(got, rh), (bins, i, np.flatnonzero(got != rh)[:8])
        assert cal.total_samples == rn


# ---- the main quantizer: bytes around its outputs ------------------------------------------------------

def _ws(gpu, n):
    nb = max(gpu.L.dllm_quantize_tensor_workspace(n), 16)
    return gpu.torch.empty(nb, dtype=gpu.torch.uint8, device="cuda"), nb


@pytest.mark.parametrize("n", BY_ID["quantize_tensor_guard"].sizes)
def test_quantize_tensor_guard_bytes(gpu, orc, n):
    """dllm_quantize_tensor, _pair and _with_params (single and pair) at packed widths 1..8: with x
    16-byte and the outputs 8-byte aligned the fused kernel runs for widths 1, 2, 4, 8; shifted by
    one element / 1..7 bytes the generic kernels run."""
    L, torch = gpu.L, gpu.torch
    x1 = (np.random.default_rng(n).standard_normal(n + 1) * 3 + 0.5).astype(np.float32)
    x1[n // 2] = np.nan
    ws, wsb = _ws(gpu, n)
    xin = In(torch, 4 * (n + 1))
    oa, ob, pa, pb = Out(torch, n), Out(torch, n), Out(torch, 8), Out(torch, 8)
    ref = {}
    for shift in (0, 1):
        for bits in range(1, 9):
            rq, rs, rz = orc.quantize_tensor(x1[shift:shift + n], bits)
            ref[shift, bits] = (orc.pack_bits(rq, bits), np.array([rs, rz], np.float32))
    for shift, offs in ((0, (0,)), (1, range(1, 8))):
        xp = xin.put(x1[shift:shift + n], 4 * shift)
        for off in offs:
            for bits in range(1, 9):
                nb = L.dllm_packed_bytes(n, bits)
                exp, prm = ref[shift, bits]
                gpu.check(L.dllm_quantize_tensor(xp, n, bits, 1, oa.place(nb, off), pa.place(8, 4 * shift),
                                                 ws.data_ptr(), wsb, gpu.stream()))
                assert np.array_equal(oa.read(), exp), ("single", bits, shift, off)
                assert pa.read(np.float32).tobytes() == prm.tobytes(), ("single", bits, shift, off)
                prd = torch.from_numpy(prm).cuda()
                gpu.check(L.dllm_quantize_tensor_with_params(xp, n, bits, 1, prd.data_ptr(), oa.place(nb, off),
                                                             gpu.stream()))
                assert np.array_equal(oa.read(), exp), ("with_params", bits, shift, off)
            for ba, bb in ((8, 4), (4, 2), (2, 1), (1, 8), (3, 5), (6, 7)):
                na, nbb = L.dllm_packed_bytes(n, ba), L.dllm_packed_bytes(n, bb)
                (ea, ma), (eb, mb) = ref[shift, ba], ref[shift, bb]
                offb = (off * 3) % 8 if off else 0
                gpu.check(L.dllm_quantize_tensor_pair(xp, n, ba, bb, 1, oa.place(na, off), pa.place(8, 4 * shift),
                                                      ob.place(nbb, offb), pb.place(8, 0), ws.data_ptr(), wsb, gpu.stream()))
                assert np.array_equal(oa.read(), ea) and np.array_equal(ob.read(), eb), ("pair", ba, bb, shift, off)
                assert pa.read(np.float32).tobytes() == ma.tobytes() and pb.read(np.float32).tobytes() == mb.tobytes()
                da, db = torch.from_numpy(ma).cuda(), torch.from_numpy(mb).cuda()
                gpu.check(L.dllm_quantize_tensor_pair_with_params(xp, n, ba, bb, 1, da.data_ptr(), db.data_ptr(),
                                                                  oa.place(na, off), ob.place(nbb, offb), gpu.stream()))
                assert np.array_equal(oa.read(), ea) and np.array_equal(ob.read(), eb), ("pair_with_params", ba, bb)


# ---- host-slice entry points against both restatements --------------------------------------------------

HOST_N = 5003


def test_host_entry_points_agree_with_both_oracles(gpu, orc, onp):
    """dllm_default_quantize_host, dllm_default_dequantize_host, dllm_bit_quantize_host,
    dllm_bit_dequantize_host and dllm_compress_vector_host (they stage through the device, so they
    need one) on every value / parameter set above at n = 5,003: the C oracle, the numpy restatement
    and the library agree bit for bit."""
    L = gpu.L
    n = HOST_N
    q, y = np.zeros(n, np.uint8), np.zeros(n, np.float32)
    codes = np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8)
    for scale, zp in DEFAULT_PARAMS:
        x = mixed_input(n, scale, zp, seed=1)
        for qt in QTYPES:
            gpu.check(L.dllm_default_quantize_host(x.ctypes.data, n, qt, scale, zp, q.ctypes.data))
            assert np.array_equal(q, orc.default_quantize(x, qt, scale, zp)), (scale, zp, qt)
            assert np.array_equal(q, onp.default_quantize(x, qt, scale, zp)), (scale, zp, qt)
        gpu.check(L.dllm_default_dequantize_host(codes.ctypes.data, n, scale, zp, y.ctypes.data))
        assert same_f32(y, orc.default_dequantize(codes, scale, zp)) and same_f32(y, onp.default_dequantize(codes, scale, zp))
    for scale, zp in BIT_PARAMS:
        x = mixed_input(n, scale, zp, seed=2)
        for bits in BIT_WIDTHS:
            gpu.check(L.dllm_bit_quantize_host(x.ctypes.data, n, bits, scale, zp, q.ctypes.data))
            assert np.array_equal(q, orc.bit_quantize(x, bits, scale, zp)), (scale, zp, bits)
            assert np.array_equal(q, onp.bit_quantize(x, bits, scale, zp)), (scale, zp, bits)
        gpu.check(L.dllm_bit_dequantize_host(codes.ctypes.data, n, scale, zp, y.ctypes.data))
        assert same_f32(y, orc.bit_dequantize(codes, scale, zp)) and same_f32(y, onp.bit_dequantize(codes, scale, zp))
    s, z = C.c_float(), C.c_float()
    for dim in COMPRESS_DIMS + (HOST_N,):
        for row in compress_rows_input(dim, seed=dim):
            row = np.ascontiguousarray(row)
            for bits in COMPRESS_BITS:
                qd = np.zeros(dim, np.uint8)
                gpu.check(L.dllm_compress_vector_host(row.ctypes.data, dim, bits, qd.ctypes.data, C.byref(s), C.byref(z)))
                for rq, rs, rz in (orc.compress_vector(row, bits), onp.compress_vector(row, bits)):
                    assert np.array_equal(qd, rq) and same_f32(s.value, rs) and same_f32(z.value, rz), (dim, bits)

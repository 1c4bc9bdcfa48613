"""CPU suite of the token readout (include/dllm_quant.h, section 8h): the two restatements of the rule
(tests/token_ref.py) agree bit for bit, the host entry point dllm_token_readout_host matches them bit
for bit on tokens, stats and probabilities, the literal fold's token equals the closed form, EXP's
special values, Z and p stay within the header's derived bound of an f64 softmax, the C entry points
reject what the header says they reject, in its order, before any device work, and the host code and
the exhaustive EXP sweep run as stand-alone programs.  No GPU work here."""
import ctypes as C
import functools
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import token_ref as ref
from tests.host_check import run_host_check

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "diffusion-llm-rs_amd" / "csrc"
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.int32:
        return np.array_equal(a, b)
    return np.array_equal(ref.bits(a), ref.bits(b))


def host(L, x, dtype=0, ld=None, probs=True):
    """dllm_token_readout_host on rows of x placed at stride ld (padding NaN / +inf); the buffer ends
    with the last row's V elements."""
    M, V = x.shape
    ld = ld or V
    buf = np.empty((M, ld), np.float32)
    buf[:, 0::2], buf[:, 1::2] = NAN, INF
    buf[:, :V] = x
    buf = buf.reshape(-1)[:(M - 1) * ld + V]
    buf = np.ascontiguousarray(buf.astype(np.float16) if dtype == 1 else buf)
    tok = np.full(M, -7, np.int32)
    st = np.full((M, 2), 77, np.float32)
    p = np.full((M, V), 77, np.float32)
    rc = L.dllm_token_readout_host(buf.ctypes.data, dtype, M, V, ld, tok.ctypes.data, st.ctypes.data,
                                   p.ctypes.data if probs else None)
    assert rc == 0, L.dllm_last_error()
    return (tok, st, p) if probs else (tok, st)


VS = [1, 3, 4, 1023, 1025, 16385, 32773]


@functools.lru_cache(maxsize=None)
def case(V):
    """(names, x, tokens, stats, probs) of the adversarial rows at V: computed once, never written to."""
    names, rows = zip(*ref.adversarial(V))
    x = np.stack(rows)
    out = (x,) + ref.readout(x, probs=True)
    for a in out:
        a.setflags(write=False)
    return (names,) + out


# ---- the restatements -----------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 3, 4, 1025])
def test_restatements_agree(V):
    names, x, tok, st, p = case(V)
    ltok, lst, lp = ref.readout_loop(x, probs=True)
    for i, name in enumerate(names):
        assert tok[i] == ltok[i] and same(st[i], lst[i]) and same(p[i], lp[i]), name


def test_restatements_agree_across_chunks():
    """Two chunks (the second ragged), stats and token; the loop form takes seconds per row, so two
    rows: a random one and the one whose first chunk is all -inf."""
    names, x, tok, st, _ = case(16385)
    pick = [names.index("random"), names.index("a chunk of -inf beside a finite chunk")]
    ltok, lst = ref.readout_loop(x[pick])
    assert np.array_equal(tok[pick], ltok) and same(st[pick], lst)


@pytest.mark.parametrize("V", VS)
def test_fold_equals_closed_form(V):
    names, x, tok, _, _ = case(V)
    for i, name in enumerate(names):
        assert ref.fold_token(x[i]) == ref.closed_form_token(x[i]) == tok[i], name


def test_fold_examples():
    f = ref.fold_token
    assert f(np.array([9, NAN, 1, 2], np.float32)) == 3          # nothing before the last NaN wins
    assert f(np.array([9, 1, NAN], np.float32)) == 2             # the NaN itself, when it is last
    assert f(np.array([2, 2, 2], np.float32)) == 2               # constant logits: V - 1
    assert f(np.array([0.0, -0.0, -1], np.float32)) == 1         # -0 equals +0, the later wins
    assert f(np.array([-INF, -INF], np.float32)) == 1
    for row in ([9, NAN, 1, 2], [9, 1, NAN], [2, 2, 2], [0.0, -0.0, -1], [-INF, -INF], [NAN, 5, 5, 4]):
        r = np.array(row, np.float32)
        assert ref.closed_form_token(r) == f(r) == ref.readout(r[None])[0][0]


def test_special_rows():
    names, x, tok, st, p = case(16385)
    row = dict(zip(names, range(len(names))))
    i = row["constant"]
    assert tok[i] == 16384 and st[i, 0] == 1.5 and st[i, 1] == 16385.0
    i = row["all -inf"]
    assert tok[i] == 16384 and np.isneginf(st[i, 0]) and ref.bits(st[i, 1]) == 0 and same(p[i], np.full(16385, ref.QNAN))
    i = row["+inf"]
    assert tok[i] == 16385 // 3 and st[i, 0] == INF and ref.bits(st[i, 1]) == 0x7fc00000
    i = row["a chunk of -inf beside a finite chunk"]
    assert np.isfinite(st[i]).all() and st[i, 1] >= 1 and tok[i] >= ref.CHUNK
    i = row["NaN mid"]
    assert (ref.bits(st[i]) == 0x7fc00000).all() and tok[i] > 16385 // 2 and same(p[i], np.full(16385, ref.QNAN))
    i = row["zeros"]
    assert tok[i] == 16384 and ref.bits(st[i, 0]) == 0 and st[i, 1] == 16385.0    # a zero maximum is +0


# ---- EXP ---------------------------------------------------------------------------------------------------

def test_exp_special_values():
    e = ref.exp32
    assert ref.bits(e(np.float32(0.0))) == 0x3f800000 and ref.bits(e(np.float32(-0.0))) == 0x3f800000
    assert ref.bits(e(NAN)) == 0x7fc00000
    below = np.array([-INF, -1e30, -88.0, np.nextafter(np.float32(-87.0), np.float32(-100.0))], np.float32)
    assert (ref.bits(e(below)) == 0).all()
    d = np.concatenate([np.linspace(-87, 0, 20001), -np.exp2(np.linspace(-30, 6.44, 5000))]).astype(np.float32)
    d = d[d >= -87]
    got = e(d)
    assert (got >= np.float32(2.0 ** -126)).all() and (got <= 1).all()          # never denormal
    want = np.exp(d.astype(np.float64))
    ulp = np.exp2(np.floor(np.log2(want)) - 23)
    assert (np.abs(got.astype(np.float64) - want) / ulp).max() <= ref.EXP_ULPS
    assert same(got[::50], [ref.exp_loop(v) for v in d[::50]])


# ---- the host entry point -----------------------------------------------------------------------------------

@pytest.mark.parametrize("V", VS)
def test_host_matches_restatement(dllm, V):
    L = dllm._lib.load()
    names, x, tok, st, p = case(V)
    for dtype, ld in ((0, V), (0, V + 3), (1, V), (1, V + 5)):
        if dtype == 1 and not np.array_equal(x.astype(np.float16).astype(np.float32), x, equal_nan=True):
            pytest.fail("the test rows must be f16 values")
        htok, hst, hp = host(L, x, dtype, ld)
        for i, name in enumerate(names):
            assert htok[i] == tok[i] and same(hst[i], st[i]) and same(hp[i], p[i]), (name, dtype, ld)
        htok, hst = host(L, x, dtype, ld, probs=False)
        assert same(htok, tok) and same(hst, st)


def test_host_f32_values_beyond_f16(dllm):
    """f32 logits that are no f16 values: differences x - m that round."""
    L = dllm._lib.load()
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 20001)) * 2).astype(np.float32)
    tok, st, p = ref.readout(x, probs=True)
    htok, hst, hp = host(L, x, 0, 20004)
    assert same(htok, tok) and same(hst, st) and same(hp, p)


def test_host_row_independence(dllm):
    L = dllm._lib.load()
    names, x, tok, st, p = case(1025)
    for i in range(len(names)):
        t1, s1, p1 = host(L, x[i:i + 1])
        assert t1[0] == tok[i] and same(s1[0], st[i]) and same(p1[0], p[i]), names[i]


# ---- the bound --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["normal", "spread"])
def test_rule_within_derived_bound(kind):
    """Z against sum exp(x - m) and p against the softmax, both in f64, within the header's bound:
    (D + 4 e + 81 + ceil(C / 256)) u on Z, (d_i + D + 6 e + 82 + ceil(C / 256)) u softmax_i + 2^-125
    on p_i.  Rows ~ N(0, 4), and rows spread over about +-80 around... below the maximum."""
    rng = np.random.default_rng(17)
    V = 50257
    if kind == "normal":
        x = (2.0 * rng.standard_normal((4, V))).astype(np.float32)
    else:
        x = rng.uniform(-80.0, 80.0, (4, V)).astype(np.float32)
    tok, st, p = ref.readout(x, probs=True)
    m, S, sm = ref.softmax_f64(x)
    assert np.array_equal(st[:, 0].astype(np.float64), m) and np.array_equal(tok, np.argmax(x, axis=1))
    relZ = np.abs(st[:, 1].astype(np.float64) - S) / S
    limZ = ref.bound_Z(x)
    err = np.abs(p.astype(np.float64) - sm)
    lim = ref.bound_p(x) * sm + 2.0 ** -125
    print(kind, "Z rel err / u", (relZ / ref.U).max(), "bound / u", (limZ / ref.U).min(), "p err / bound", (err / lim).max())
    assert (relZ <= limZ).all()
    assert (err <= lim).all()
    assert limZ.max() < 2e-5 and (ref.bound_p(x) < 4e-5).all()      # the bound says something


# ---- the error contract, through the C entry points, nothing launched -------------------------------------------

def test_rejections_in_the_headers_order(dllm):
    L = dllm._lib.load()
    INV, UNS, SHAPE = dllm._lib.ERR_INVALID_PARAMS, dllm._lib.ERR_UNSUPPORTED, dllm._lib.ERR_SHAPE_MISMATCH
    p = C.c_void_p(4096)       # never dereferenced: every call below returns before a launch
    ws = L.dllm_token_readout_workspace(2, 40000)
    assert ws == 2 * 3 * 20 and L.dllm_token_readout_workspace(5, 16384) == 100
    assert L.dllm_token_readout_workspace(1, 16385) == 40 and L.dllm_token_readout_workspace(0, 9) == 0

    def call(logits=p, dtype=0, M=2, V=40000, ld=40000, tokens=p, stats=p, probs=None, w=p, wb=ws):
        return L.dllm_token_readout(logits, dtype, M, V, ld, tokens, stats, probs, w, wb, None)

    assert call(V=0, ld=0) == INV and call(ld=39999) == INV and b"ld" in L.dllm_last_error()
    assert call(V=2 ** 31, ld=2 ** 31, wb=2 ** 62) == SHAPE
    assert call(dtype=2) == UNS and call(dtype=-1) == UNS
    assert call(M=0) == 0 and call(M=0, logits=None, tokens=None, stats=None, w=None, wb=0) == 0
    for name in ("logits", "tokens", "stats", "w"):
        assert call(**{name: None}) == INV and b"NULL" in L.dllm_last_error(), name
    assert call(wb=ws - 1) == INV and b"workspace" in L.dllm_last_error()
    assert call(w=C.c_void_p(4098)) == INV
    # the order: V / ld, then V >= 2^31, then the dtype, then M == 0, then the pointers
    assert call(V=0, ld=0, dtype=9, logits=None) == INV
    assert call(V=2 ** 31, ld=2 ** 31 - 1) == INV
    assert call(V=2 ** 31, ld=2 ** 31, dtype=9, logits=None) == SHAPE
    assert call(dtype=9, M=0) == UNS and call(dtype=9, logits=None) == UNS
    assert call(M=0, wb=0) == 0
    # the host form: the same checks and codes
    h = lambda logits=p, dtype=0, M=2, V=8, ld=8, tokens=p, stats=p: L.dllm_token_readout_host(
        logits, dtype, M, V, ld, tokens, stats, None)
    assert h(V=0) == INV and h(ld=7) == INV and h(V=2 ** 31, ld=2 ** 31) == SHAPE and h(dtype=3) == UNS
    assert h(M=0, logits=None, tokens=None, stats=None) == 0
    assert h(logits=None) == INV and h(tokens=None) == INV and h(stats=None) == INV
    assert h(V=2 ** 31, ld=2 ** 31, dtype=3) == SHAPE and h(dtype=3, M=0) == UNS


def test_wrappers_exported(dllm):
    for name in ("token_readout", "TokenHead"):
        assert name in dllm.__all__ and callable(getattr(dllm, name))
    assert dllm.decode.token_readout is dllm.token_readout
    assert "decode" in dllm.__doc__
    assert "dllm_token_readout" in dllm._lib.HEADER.read_text()


# ---- the stand-alone programs -------------------------------------------------------------------------------------

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_host_entry_point_under_sanitizers(tmp_path):
    """tests/cpp/token_host_check.cpp (its own main) with csrc/host_rules.cpp and error.cpp, compiled by
    g++ under the address and undefined-behaviour sanitizers (tests/host_check.py; no hipcc, no
    library): exact-size heap buffers at every kind of V, both dtypes, padding that must not be read,
    the special rows, EXP's special points and a strided sample of its range."""
    run_host_check("token_host_check", tmp_path)



def test_exp_exhaustive_sweep(tmp_path):
    """EXP against the exact exponential over every f32 in [-87, 0] (1 118 699 521 values): the largest
    error is the figure the header states, no result is a denormal, zero, above 1 or NaN.  This sweep
    runs unsanitized at -O2 (host only, no library; about 15 s on 8 cores): under the sanitizers it
    would take minutes.  The sanitized program above runs the same EXP on a strided sample."""
    exe = tmp_path / "token_exp_sweep"
    cmd = [HIPCC, "-std=c++17", "-O2", "-ffp-contract=off", "-DTOKEN_CHECK_EXP_ONLY", f"-I{CSRC}",
           str(ROOT / "tests" / "cpp" / "token_host_check.cpp"), "-o", str(exe), "-lpthread"]
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(line.split(None, 1) for line in r.stdout.strip().splitlines())
    assert int(out["values"]) == 0xc2ae0000 - 0x80000000 + 1 and int(out["out_of_range"]) == 0
    worst = float(out["max_ulp_error"].split()[0])
    assert 0.5 < worst <= ref.EXP_ULPS
    header = (CSRC / "token_exp.hpp").read_text()
    assert f"{worst:.6f} ulp" in header and f"kExpUlps = {ref.EXP_ULPS}f" in header
    assert f"e = {ref.EXP_ULPS} ulp" in (ROOT / "include" / "dllm_quant.h").read_text()

"""dllm_kv_attention_hd on the host: the head-dim and width refusals and the empty calls return
before anything touches a device, so they run without a GPU (and with any pointers)."""
import pytest

D_REFUSED = (0, 32, 96, 256)


@pytest.fixture(scope="module")
def lib(dllm):
    return dllm._lib.load()


def hd(lib, sq, bits, skv, h, d, ptr=None):
    return lib.dllm_kv_attention_hd(ptr, sq, ptr, ptr, ptr, ptr, bits, skv, h, d, ptr, None)


def test_exported(dllm, lib):
    assert "dllm_kv_attention_hd" in dllm._lib.SIGNATURES
    assert dllm._lib.SIGNATURES["dllm_kv_attention_hd"] == dllm._lib.SIGNATURES["dllm_kv_attention_ex"]
    assert hasattr(lib, "dllm_kv_attention_hd")


@pytest.mark.parametrize("ptr", [None, 0x1000, 0x1002])
@pytest.mark.parametrize("D", D_REFUSED)
def test_other_head_dims_unsupported(dllm, lib, D, ptr):
    assert hd(lib, 33, 4, 33, 2, D, ptr) == dllm._lib.ERR_UNSUPPORTED
    assert hd(lib, 0, 4, 33, 2, D, ptr) == dllm._lib.ERR_UNSUPPORTED   # before the empty-call answer too
    assert b"64 or 128" in lib.dllm_last_error()


@pytest.mark.parametrize("D", [64, 128])
def test_bits_9_unsupported(dllm, lib, D):
    assert hd(lib, 33, 9, 33, 2, D) == dllm._lib.ERR_UNSUPPORTED
    assert hd(lib, 33, 255, 33, 2, D, 0x1000) == dllm._lib.ERR_UNSUPPORTED


@pytest.mark.parametrize("bits", [0, 1, 4, 8])
def test_d64_empty_calls_ok(dllm, lib, bits):
    assert hd(lib, 0, bits, 33, 2, 64) == dllm._lib.OK        # Sq = 0
    assert hd(lib, 33, bits, 33, 0, 64) == dllm._lib.OK       # H = 0
    assert hd(lib, 0, bits, 0, 0, 64, 0x1002) == dllm._lib.OK


def test_older_entry_points_still_refuse_d64(dllm, lib):
    E = dllm._lib
    assert lib.dllm_kv_attention_ex(None, 0, None, None, None, None, 4, 33, 2, 64, None, None) == E.ERR_UNSUPPORTED
    assert b"128" in lib.dllm_last_error()
    assert lib.dllm_kv_attention_ex(None, 33, None, None, None, None, 4, 33, 2, 64, None, None) == E.ERR_UNSUPPORTED
    assert lib.dllm_kv_attention(None, None, None, None, None, 4, 33, 2, 64, None, None) == E.ERR_UNSUPPORTED
    assert lib.dllm_kv_attention_ex(None, 0, None, None, None, None, 4, 33, 2, 128, None, None) == E.OK

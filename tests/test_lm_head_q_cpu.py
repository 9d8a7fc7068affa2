"""CPU: what the opt-in quantised lm_head (LlamaEngine(lm_head_dtype=...)) promises without a GPU: the option's values, the
quantisers as fixed points in values on head-shaped matrices (what lets a vocabulary change re-quantise the head from W_eff without
moving untouched rows), the op list, the class constants' range and the entry points' host-side validation."""
import pytest
import torch

from spider_amd.llm import resolve_lm_head_dtype

BF = torch.bfloat16


def test_resolve_lm_head_dtype():
    from spider_amd.llm import WEIGHT_DTYPES
    assert WEIGHT_DTYPES == ("bf16", "fp8", "mxfp4")
    for v in WEIGHT_DTYPES:
        assert resolve_lm_head_dtype(v) == v
    for bad in ("int4", "fp4", "FP8", None, 8, ""):
        with pytest.raises(ValueError, match="lm_head_dtype"):
            resolve_lm_head_dtype(bad)


def _head(seed):
    """a [331, 256] N(0, 0.08^2) head (the tests' tiny model) with an all-zero row, an all-zero block and, for MXFP4, a block whose
    largest element lies in (3, 3.5) * scale: amax = 3.25 * 2^-6 gives scale 2^-6 and rounds down to 3 * scale, which then
    requantises as (6, scale / 2) -- other bytes, the same values"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(331, 256, generator=g) * 0.08).to(BF)
    w[7] = 0
    w[11, 32:64] = 0
    w[13, 64:96] = (torch.rand(32, generator=g) * 2.0 ** -6).to(BF)
    w[13, 70] = 3.25 * 2.0 ** -6
    return w


@pytest.mark.parametrize("seed", [21, 25])
def test_quantisers_are_fixed_points_in_values(seed):
    from spider_amd.llm import dequantize_fp8_rows, dequantize_mxfp4, quantize_fp8_rows, quantize_mxfp4
    w = _head(seed)
    q8, s8 = quantize_fp8_rows(w)
    e8 = dequantize_fp8_rows(q8, s8)
    assert e8.dtype == BF and not torch.equal(e8, w) and torch.equal(e8[7], w[7])
    q8b, s8b = quantize_fp8_rows(e8)
    assert torch.equal(dequantize_fp8_rows(q8b, s8b), e8)
    q4, s4 = quantize_mxfp4(w)
    e4 = dequantize_mxfp4(q4, s4)
    assert e4.dtype == BF and not torch.equal(e4, w) and torch.equal(e4[7], w[7]) and torch.equal(e4[11, 32:64], w[11, 32:64])
    assert float(e4[13, 64:96].abs().max()) == 3 * 2.0 ** -6 and int(s4[13, 2]) == 127 - 6
    q4b, s4b = quantize_mxfp4(e4)
    assert torch.equal(dequantize_mxfp4(q4b, s4b), e4)
    assert int(s4b[13, 2]) == 127 - 7 and not torch.equal(q4b[13], q4[13])       # not a fixed point in bytes
    # rows written into W_eff and quantised again: the other rows keep their values
    for fmt, quant, deq, e in (("fp8", quantize_fp8_rows, dequantize_fp8_rows, e8), ("mxfp4", quantize_mxfp4, dequantize_mxfp4, e4)):
        assert resolve_lm_head_dtype(fmt) == fmt            # (the two head formats of the engine option)
        m = e.clone()
        m[100:105] = (torch.randn(5, 256, generator=torch.Generator().manual_seed(seed + 1)) * 0.08).to(BF)
        again = deq(*quant(m))
        keep = torch.ones(331, dtype=torch.bool)
        keep[100:105] = False
        assert torch.equal(again[keep], e[keep]) and not torch.equal(again[100:105], m[100:105])


def test_op_names_and_class_constants():
    import spider_amd.torch_ops as T
    from spider_amd import ops
    from spider_amd.llm import LlamaEngine
    assert T.LM_HEAD_Q_OP_NAMES == ("lm_head_argmax_w8", "lm_head_argmax_proc_w8", "lm_head_argmax_w4", "lm_head_argmax_proc_w4")
    assert not set(T.LM_HEAD_Q_OP_NAMES) & (set(T.OP_NAMES) | set(T.W8_OP_NAMES) | set(T.W4_OP_NAMES))
    assert len(T.OP_NAMES) == 14
    for name in T.LM_HEAD_Q_OP_NAMES:
        assert callable(getattr(ops, name)) and hasattr(torch.ops.spider_hip, name)
    assert ops.LM_HEAD_Q_MAX_ROWS == 4
    assert 0 <= LlamaEngine.LM_HEAD_FP8_MAX_ROWS <= 4 and 0 <= LlamaEngine.LM_HEAD_MXFP4_MAX_ROWS <= 4


def test_entry_points_validate_on_the_host():
    from spider_amd import lib as slib
    lib = slib.load()
    plain = lambda name, B, K: getattr(lib, name)(None, None, None, None, 0.0, None, None, None, None, B, 7, K, None)
    proc = lambda name, B, K: getattr(lib, name)(None, None, None, None, 0.0, *([None] * 11), B, 7, K, None)
    for fmt, mult in (("w8", 16), ("w4", 32)):
        for call, name in ((plain, "spider_lm_head_argmax_" + fmt), (proc, "spider_lm_head_argmax_proc_" + fmt)):
            assert call(name, 5, 64) == -1
            assert b"1..4" in lib.spider_last_error()
            assert call(name, 0, 64) == -1
            assert b"1..4" in lib.spider_last_error()
            assert call(name, 1, mult + 8) == -1
            assert f"multiple of {mult}".encode() in lib.spider_last_error()
            assert call(name, 1, 64) == -1
            assert b"null" in lib.spider_last_error()
    assert lib.spider_abi_version() == 4

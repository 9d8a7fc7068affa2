"""CPU: the per-row FP8 quantiser of the weight-only decode stream (spider_amd.llm.quantize_fp8_rows / dequantize_fp8_rows).

The contract the FP8 engine rests on: the scale is a power of two and the encoding is OCP e4m3fn, so W_eff = float(q) * scale is a
bf16 number and the quantised model is a bf16 model with weights W_eff."""
import math

import pytest
import torch

from spider_amd.llm import (dequantize, dequantize_fp8_rows, quantize_fp8_rows, resolve_weight_dtype)

K = 256


def _inputs():
    """N(0, sigma^2) rows for sigma in {0.02, 0.08, 1}, a zero row, a row scaled by 1e-30, a row with a 3e4 outlier, and rows whose
    largest element sits exactly on / next to a power of two times 448 (the edges of the scale rule)"""
    g = torch.Generator().manual_seed(7)
    rows = [torch.randn(K, generator=g) * s for s in (0.02, 0.08, 1.0) for _ in range(3)]
    rows.append(torch.zeros(K))
    rows.append(torch.randn(K, generator=g) * 1e-30)
    out = torch.randn(K, generator=g) * 0.05
    out[17] = 3e4
    rows.append(out)
    for top in (448.0, 448.0 * 2 ** -7, float(torch.nextafter(torch.tensor(448.0), torch.tensor(1e9))), 447.99, 224.0, 1.0):
        r = torch.randn(K, generator=g).clamp(-1, 1) * top * 0.5
        r[3] = -top
        rows.append(r)
    return torch.stack(rows)


@pytest.fixture(scope="module")
def case():
    W = _inputs()
    q, scale = quantize_fp8_rows(W)
    return W, q, scale


def test_scale_is_a_power_of_two_and_amax_lands_in_the_top_binade(case):
    W, q, scale = case
    assert q.dtype == torch.float8_e4m3fn and scale.dtype == torch.float32 and q.shape == W.shape and scale.shape == (W.shape[0],)
    m, _ = torch.frexp(scale)
    assert bool((m == 0.5).all()), "every scale is an exact power of two"
    amax = W.abs().amax(1).double()
    zero = amax == 0
    assert int(zero.sum()) == 1 and bool((scale[zero] == 1.0).all())
    ratio = amax[~zero] / scale[~zero].double()
    assert bool((ratio > 224).all()) and bool((ratio <= 448).all()), ratio
    # the rule itself: scale = 2^ceil(log2(amax / 448)), in exact integer / rational arithmetic
    for a, s in zip(amax[~zero].tolist(), scale[~zero].tolist()):
        e = round(math.log2(s))
        assert 2.0 ** e == s and a <= 448 * 2.0 ** e and a > 448 * 2.0 ** (e - 1)


def test_bytes_are_ocp_e4m3fn_and_hold_no_nan(case):
    W, q, scale = case
    b = q.view(torch.uint8)
    assert not bool(((b & 0x7f) == 0x7f).any()), "0x7f / 0xff are the NaN bytes of e4m3fn"
    assert bool((q.float().abs() <= 448).all())
    # 448 = 0x7e and 1.0 = 0x38 in OCP e4m3fn (bias 7); in MI300's e4m3fnuz (bias 8) 1.0 is 0x40 and 0x7e reads 224
    one = torch.zeros(2, 16)
    one[0, 0], one[0, 1], one[1, 0] = 448.0, 1.0, -448.0
    q1, s1 = quantize_fp8_rows(one)
    assert s1.tolist() == [1.0, 1.0]
    assert q1.view(torch.uint8)[0, :2].tolist() == [0x7e, 0x38] and int(q1.view(torch.uint8)[1, 0]) == 0xfe
    assert torch.tensor([0x7e, 0x38], dtype=torch.uint8).view(torch.float8_e4m3fn).float().tolist() == [448.0, 1.0]


def test_w_eff_is_a_bf16_number_and_requantises_to_itself(case):
    W, q, scale = case
    w_eff = q.float() * scale[:, None]
    assert torch.equal(w_eff.to(torch.bfloat16).float(), w_eff), "W_eff round-trips through bf16 exactly"
    assert torch.equal(dequantize_fp8_rows(q, scale).float(), w_eff) and dequantize is dequantize_fp8_rows
    assert dequantize_fp8_rows(q, scale).dtype == torch.bfloat16
    # quantising W_eff again returns the same (q, scale) and, always, the same model. The one exception the scale rule itself makes:
    # a row whose largest element lies in (224, 232) * scale rounds DOWN to 224 * scale, the bottom edge of the top binade, and
    # 2^ceil(log2(224 * scale / 448)) is scale / 2 -- the same W_eff then reads (2 q, scale / 2). _inputs() holds such a row.
    q2, s2 = quantize_fp8_rows(dequantize_fp8_rows(q, scale))
    assert torch.equal(q2.float() * s2[:, None], w_eff)
    edge = q.float().abs().amax(1) == 224
    assert int(edge.sum()) >= 1 and int((~edge).sum()) >= 12
    assert torch.equal(s2[~edge], scale[~edge]) and torch.equal(q2.view(torch.uint8)[~edge], q.view(torch.uint8)[~edge])
    assert torch.equal(s2[edge] * 2, scale[edge]) and torch.equal(q2.float()[edge], 2 * q.float()[edge])


def test_error_is_half_an_ulp_of_three_mantissa_bits_in_the_normal_range(case):
    W, q, scale = case
    w_eff = (q.float() * scale[:, None]).double()
    Wd = W.double()
    normal = (Wd / scale[:, None].double()).abs() >= 2.0 ** -6
    assert int(normal.sum()) > W.numel() // 2
    assert bool(((w_eff - Wd).abs()[normal] <= 2.0 ** -4 * Wd.abs()[normal]).all())
    # below the normal range the spacing is the subnormal one: 2^-9 in units of the scale
    assert bool(((w_eff - Wd).abs()[~normal] <= 2.0 ** -10 * scale[:, None].double().expand_as(Wd)[~normal]).all())


def test_weight_dtype_resolver():
    assert resolve_weight_dtype("bf16") == "bf16" and resolve_weight_dtype("fp8") == "fp8"
    for bad in ("int4", "fp8_e5m2", None, 8, "FP8"):
        with pytest.raises(ValueError, match="weight_dtype"):
            resolve_weight_dtype(bad)


def test_engine_constructor_refuses_an_unknown_weight_dtype_before_it_touches_a_device():
    from spider_amd.llm import LlamaEngine, LLMConfig
    cfg = LLMConfig(256, 2, 2, 1, 128, 512, 331, 10000.0, None, 1e-6, False, 256)
    with pytest.raises(ValueError, match="weight_dtype"):
        LlamaEngine(cfg, {}, "cuda:0", weight_dtype="int4")
    with pytest.raises(ValueError, match="weight_dtype"):
        LlamaEngine(cfg, {}, weight_dtype="e5m2")


def test_fp8_gemv_ops_are_registered_with_schema_and_fake_impl():
    import spider_amd.torch_ops as T
    assert T.W8_OP_NAMES == ("gemv_w8", "gemv_swiglu_w8")
    for n in T.W8_OP_NAMES:
        assert getattr(torch.ops.spider_hip, n).default._schema.name == f"spider_hip::{n}"
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *s, dt=torch.bfloat16: torch.empty(*s, dtype=dt, device="cuda")
        o = torch.ops.spider_hip
        q, s = e(18, 64, dt=torch.float8_e4m3fn), e(18, dt=torch.float32)
        assert o.gemv_w8(q, s, e(2, 64), e(18), e(2, 18), e(64), 1e-6).shape == (2, 18)
        assert o.gemv_w8(q, s, e(3, 64), None, None, None, 0.0).dtype == torch.bfloat16
        assert o.gemv_swiglu_w8(q, s, e(4, 64), e(64), 1e-6).shape == (4, 9)


def test_rejects_a_non_matrix():
    with pytest.raises(ValueError):
        quantize_fp8_rows(torch.zeros(4))

"""CPU: the MXFP4 quantiser of the weight-only decode stream (spider_amd.llm.quantize_mxfp4 / dequantize_mxfp4), the resolver, the
op registration and the host-side validation of the C entry points.

The contract the MXFP4 engine rests on: e2m1 has two significand bits and the E8M0 block scale is a power of two, so W_eff is a
bf16 matrix and the quantised model is a bf16 model with weights W_eff. The byte layout is the one of
transformers.integrations.mxfp4, whose dequantiser is the independent pin for the decode direction."""
import ctypes
import math

import pytest
import torch

from spider_amd.llm import FP4_VALUES, dequantize_mxfp4, quantize_mxfp4, resolve_weight_dtype

K = 256
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
NEXT = lambda v, to=1e9: float(torch.nextafter(torch.tensor(float(v)), torch.tensor(float(to))))


def _inputs():
    """The row recipe of test_fp8_quant_cpu._inputs, cut into blocks of 32: N(0, sigma^2) rows for sigma in {0.02, 0.08, 1}, a zero
    row, a row with 32 zeros inside it, a row scaled by 1e-30, a row with a 3e4 outlier, and rows in which every block's largest
    element sits exactly on / next to 6 * 2^e and 3 * 2^e (the edges of the scale rule)"""
    g = torch.Generator().manual_seed(7)
    rows = [torch.randn(K, generator=g) * s for s in (0.02, 0.08, 1.0) for _ in range(3)]
    rows.append(torch.zeros(K))
    hole = torch.randn(K, generator=g) * 0.02
    hole[64:96] = 0
    rows.append(hole)
    rows.append(torch.randn(K, generator=g) * 1e-30)
    out = torch.randn(K, generator=g) * 0.05
    out[17] = 3e4
    rows.append(out)
    for top in (6.0, 6.0 * 2 ** -7, NEXT(6.0), NEXT(6.0, 0), 3.0, NEXT(3.0), NEXT(3.0, 0), 3.0 * 2 ** 5, 3.4, 3.5, 1.0):
        r = torch.randn(K, generator=g).clamp(-1, 1) * top * 0.5
        r[3::32] = -top
        rows.append(r)
    return torch.stack(rows)


@pytest.fixture(scope="module")
def case():
    W = _inputs()
    blocks, scales = quantize_mxfp4(W)
    return W, blocks, scales


def _table_decode(blocks, scales):
    """the format as the contract states it, in fp64, element by element (no code shared with dequantize_mxfp4)"""
    N, K2 = blocks.shape
    out = torch.zeros(N, 2 * K2, dtype=torch.float64)
    bl, sl = blocks.tolist(), scales.tolist()
    for n in range(N):
        for j in range(K2):
            for h, c in enumerate((bl[n][j] & 15, bl[n][j] >> 4)):
                k = 2 * j + h
                out[n, k] = (-1.0 if c & 8 else 1.0) * GRID[c & 7] * 2.0 ** (sl[n][k // 32] - 127)
    return out


def test_layout_scale_rule_and_byte_range(case):
    W, blocks, scales = case
    N = W.shape[0]
    assert tuple(FP4_VALUES) == tuple(GRID)
    assert blocks.dtype == torch.uint8 and scales.dtype == torch.uint8 and blocks.shape == (N, K // 2) and scales.shape == (N, K // 32)
    assert int(scales.min()) >= 2 and int(scales.max()) <= 252
    amax = W.reshape(N, K // 32, 32).abs().amax(2).double()
    zero = amax == 0
    assert int(zero.sum()) == K // 32 + 1, "the zero row and the zero block"
    assert bool((scales[zero] == 127).all())
    scale = torch.ldexp(torch.ones(N, K // 32, dtype=torch.float64), scales.to(torch.int32) - 127)
    ratio = amax[~zero] / scale[~zero]
    assert bool((ratio > 3).all()) and bool((ratio <= 6).all()), ratio
    # the rule itself, scale = 2^ceil(log2(amax / 6)), in exact arithmetic
    for a, s in zip(amax[~zero].tolist(), scale[~zero].tolist()):
        e = round(math.log2(s))
        assert 2.0 ** e == s and a <= 6 * 2.0 ** e and a > 6 * 2.0 ** (e - 1)
    # low nibble first, sign in bit 3: 1.0 = code 2, -6 = code 15, 0.5 = code 1, -0 is a legal code
    v = torch.zeros(1, 32)
    v[0, :4] = torch.tensor([1.0, -6.0, 0.5, -0.0])
    b1, s1 = quantize_mxfp4(v)
    assert b1[0, :2].tolist() == [2 | (15 << 4), 1 | (8 << 4)] and s1.tolist() == [[127]]


def test_tie_table_both_signs():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    for e in (0, -9, 40):
        v = torch.zeros(2, 32)
        v[0, :7] = torch.tensor(ties)
        v[1, :7] = -torch.tensor(ties)
        v[0, 31], v[1, 31] = 6.0, -6.0            # pins the block scale to 2^e
        v = v * 2.0 ** e
        b, s = quantize_mxfp4(v)
        assert s.tolist() == [[127 + e], [127 + e]]
        w = dequantize_mxfp4(b, s, torch.float32) / 2.0 ** e
        assert w[0, :7].tolist() == want and w[1, :7].tolist() == [-x for x in want]
        assert torch.signbit(w[1, :7]).all(), "the sign is kept, -0 included"
        # next to a tie the nearer neighbour wins
        up = torch.zeros(1, 32)
        up[0, :7] = torch.tensor([NEXT(t) for t in ties])
        up[0, 7:14] = torch.tensor([NEXT(t, 0) for t in ties])
        up[0, 31] = 6.0
        w = dequantize_mxfp4(*quantize_mxfp4(up), torch.float32)
        assert w[0, :7].tolist() == [0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0] and w[0, 7:14].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0]


def test_dequantize_is_the_contract_and_equals_the_transformers_decode(case):
    W, blocks, scales = case
    N = W.shape[0]
    w_eff = dequantize_mxfp4(blocks, scales)
    assert w_eff.dtype == torch.bfloat16 and w_eff.shape == W.shape
    assert torch.equal(w_eff.double(), _table_decode(blocks, scales))
    from transformers.integrations.mxfp4 import convert_moe_packed_tensors
    ref = convert_moe_packed_tensors(blocks.reshape(1, N, K // 32, 16), scales.reshape(1, N, K // 32), dtype=torch.bfloat16)[0].T
    assert ref.shape == w_eff.shape and torch.equal(ref.view(torch.int16), w_eff.view(torch.int16)), "bit for bit"


def test_every_code_and_the_contract_scale_bytes_decode_exactly():
    blocks = torch.arange(256, dtype=torch.uint8).reshape(1, 256).repeat(5, 1)          # every pair of codes
    scales = torch.tensor([2, 64, 127, 190, 252], dtype=torch.uint8)[:, None].repeat(1, 16)
    w = dequantize_mxfp4(blocks, scales, torch.float32)
    assert torch.equal(w.double(), _table_decode(blocks, scales))
    assert torch.equal(w.to(torch.bfloat16).float(), w) and bool(torch.isfinite(w).all())
    nz = w != 0
    assert bool((w[nz].abs() >= 2.0 ** -126).all()), "every non-zero W_eff is a normal bf16 number"


def test_nearest_on_the_e2m1_grid(case):
    W, blocks, scales = case
    N = W.shape[0]
    scale = torch.ldexp(torch.ones(N, K // 32, dtype=torch.float64), scales.to(torch.int32) - 127).repeat_interleave(32, 1)
    a = W.double().abs() / scale
    err = (dequantize_mxfp4(blocks, scales, torch.float32).double() - W.double()).abs() / scale
    assert bool((a <= 6).all()), "no element saturates"
    # half the grid spacing: 0.5 up to 2, 1 up to 4, 2 up to 6
    half = torch.where(a <= 2, 0.25, torch.where(a <= 4, 0.5, 1.0))
    assert bool((err <= half).all())


def test_w_eff_is_a_bf16_number_and_requantises_to_itself(case):
    W, blocks, scales = case
    w_eff = dequantize_mxfp4(blocks, scales, torch.float32)
    assert torch.equal(w_eff.to(torch.bfloat16).float(), w_eff), "W_eff round-trips through bf16 exactly"
    b2, s2 = quantize_mxfp4(dequantize_mxfp4(blocks, scales))
    assert torch.equal(dequantize_mxfp4(b2, s2, torch.float32), w_eff), "the same model, always"
    # Not always the same bytes: a block whose largest element lies in (3, 3.5) * scale rounds DOWN to 3 * scale, and
    # 2^ceil(log2(3 * scale / 6)) is scale / 2 -- the same W_eff then reads (2 q, scale / 2), legal because no code above 3 exists in
    # such a block. _inputs() holds such blocks by construction (amax next above 3 * 2^e, 3.4 * 2^e) and among the random ones.
    N = W.shape[0]
    mag = torch.tensor(GRID)[(torch.stack([blocks & 7, (blocks >> 4) & 7], 2).reshape(N, K // 32, 32)).long()]
    top = mag.amax(2)
    nonzero = top > 0
    edge = top == 3
    assert bool((top[nonzero] >= 3).all())
    n_edge, n_rest = int(edge.sum()), int((nonzero & ~edge).sum())
    print(f"doubled-code blocks: {n_edge} of {int(nonzero.sum())} non-zero blocks")
    assert n_edge >= 16 + 8 and n_rest >= 64
    same = ~edge
    assert torch.equal(s2[same], scales[same])
    assert torch.equal(b2.reshape(N, K // 32, 16)[same], blocks.reshape(N, K // 32, 16)[same])
    assert torch.equal(s2[edge].int() + 1, scales[edge].int())
    mag2 = torch.tensor(GRID)[(torch.stack([b2 & 7, (b2 >> 4) & 7], 2).reshape(N, K // 32, 32)).long()]
    assert torch.equal(mag2[edge], 2 * mag[edge])
    # among random N(0, sigma^2) blocks a fair share does it (rows 0..8 of _inputs)
    rnd = edge[:9]
    print(f"doubled-code share of random blocks: {float(rnd.float().mean()):.3f}")
    assert 0 < int(rnd.sum()) < rnd.numel()


def test_rejects_what_the_format_cannot_hold():
    for bad in (torch.zeros(4), torch.zeros(2, 48), torch.zeros(2, 3, 32)):
        with pytest.raises(ValueError):
            quantize_mxfp4(bad)
    for v in (float("inf"), float("nan"), -float("inf"), NEXT(6.0 * 2.0 ** 125, float("inf"))):
        w = torch.zeros(2, 64)
        w[1, 40] = v
        with pytest.raises(ValueError):
            quantize_mxfp4(w)
    w = torch.zeros(1, 32)
    w[0, 0] = 6.0 * 2.0 ** 125
    b, s = quantize_mxfp4(w)
    assert s.tolist() == [[252]] and float(dequantize_mxfp4(b, s, torch.float32)[0, 0]) == 6.0 * 2.0 ** 125
    with pytest.raises(ValueError):
        dequantize_mxfp4(torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8))
    with pytest.raises(ValueError):
        dequantize_mxfp4(torch.zeros(2, 16, dtype=torch.int8), torch.zeros(2, 1, dtype=torch.uint8))


def test_weight_dtype_resolver():
    import spider_amd.llm as L
    assert L.WEIGHT_DTYPES == ("bf16", "fp8", "mxfp4")
    assert resolve_weight_dtype("mxfp4") == "mxfp4" and resolve_weight_dtype("bf16") == "bf16" and resolve_weight_dtype("fp8") == "fp8"
    for bad in ("int4", "fp8_e5m2", "e5m2", None, 8, "FP8", "MXFP4", "fp4", 4):
        with pytest.raises(ValueError, match="weight_dtype"):
            resolve_weight_dtype(bad)


def test_engine_constructor_refuses_a_hidden_size_off_the_block_before_it_touches_a_device():
    from spider_amd.llm import LlamaEngine, LLMConfig
    for hidden, n_q, hd, inter in ((240, 2, 128, 512), (256, 2, 128, 528), (256, 3, 80, 512)):
        cfg = LLMConfig(hidden, 2, n_q, 1, hd, inter, 331, 10000.0, None, 1e-6, False, 256)
        with pytest.raises(ValueError, match="multiples of 32"):
            LlamaEngine(cfg, {}, "cuda:0", weight_dtype="mxfp4")
    assert isinstance(LlamaEngine.MXFP4_MAX_ROWS, int) and 0 <= LlamaEngine.MXFP4_MAX_ROWS <= 4


def test_mxfp4_gemv_ops_are_registered_with_schema_and_fake_impl():
    import spider_amd.torch_ops as T
    assert T.W4_OP_NAMES == ("gemv_w4", "gemv_swiglu_w4") and T.W8_OP_NAMES == ("gemv_w8", "gemv_swiglu_w8")
    for n in T.W4_OP_NAMES:
        assert getattr(torch.ops.spider_hip, n).default._schema.name == f"spider_hip::{n}"
        assert n not in T.OP_NAMES
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *s, dt=torch.bfloat16: torch.empty(*s, dtype=dt, device="cuda")
        o = torch.ops.spider_hip
        q, s = e(18, 32, dt=torch.uint8), e(18, 2, dt=torch.uint8)
        assert o.gemv_w4(q, s, e(2, 64), e(18), e(2, 18), e(64), 1e-6).shape == (2, 18)
        assert o.gemv_w4(q, s, e(3, 64), None, None, None, 0.0).dtype == torch.bfloat16
        assert o.gemv_swiglu_w4(q, s, e(4, 64), e(64), 1e-6).shape == (4, 9)


def test_w4_norm_fits_mirrors_the_kernel_budget():
    from spider_amd import ops
    assert ops.W4_MAX_ROWS == 4
    # rows padded to whole 2048-element chunks, 4 KiB each, within 160 KiB less 256 bytes
    assert ops.w4_norm_fits(4, 3584) and ops.w4_norm_fits(1, 18944) and ops.w4_norm_fits(3, 18944)
    assert not ops.w4_norm_fits(4, 18944), "4 x 10 x 4 KiB = 160 KiB is 256 bytes too many"
    assert ops.w4_norm_fits(4, 18432) and not ops.w4_norm_fits(4, 18432 + 32)


def test_c_entry_points_validate_on_the_host_before_any_launch():
    """K % 32, the row count and null pointers are refused with -1 and a message, with no GPU in the machine"""
    from spider_amd import lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)           # never dereferenced: every call below is refused before a launch
    with pytest.raises(lib.SpiderHipError, match=r"rc=-1.*gemv_w4.*multiple of 32"):
        lib.call("spider_gemv_w4", p, p, p, p, None, None, None, 0.0, 1, 8, 48, None)
    with pytest.raises(lib.SpiderHipError, match=r"rc=-1.*gemv_w4.*1\.\.4"):
        lib.call("spider_gemv_w4", p, p, p, p, None, None, None, 0.0, 5, 8, 64, None)
    with pytest.raises(lib.SpiderHipError, match=r"rc=-1.*gemv_w4.*1\.\.4"):
        lib.call("spider_gemv_w4", p, p, p, p, None, None, None, 0.0, 0, 8, 64, None)
    with pytest.raises(lib.SpiderHipError, match=r"rc=-1.*gemv_w4.*null"):
        lib.call("spider_gemv_w4", p, None, p, p, None, None, None, 0.0, 1, 8, 64, None)
    with pytest.raises(lib.SpiderHipError, match=r"rc=-1.*gemv_swiglu_w4.*multiple of 32"):
        lib.call("spider_gemv_swiglu_w4", p, p, p, p, None, 0.0, 1, 8, 48, None)
    with pytest.raises(lib.SpiderHipError, match=r"rc=-1.*gemv_swiglu_w4.*1\.\.4"):
        lib.call("spider_gemv_swiglu_w4", p, p, p, p, None, 0.0, 5, 8, 64, None)
    with pytest.raises(lib.SpiderHipError, match=r"rc=-1.*gemv_swiglu_w4.*null"):
        lib.call("spider_gemv_swiglu_w4", None, p, p, p, None, 0.0, 2, 8, 64, None)
    assert lib.load().spider_abi_version() == 4

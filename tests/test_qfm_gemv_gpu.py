"""GPU: the fragment-major weight-only MFMA GEMVs (ops.gemv_fm_w4 / gemv_swiglu_fm_w4 / gemv_fm_w8 / gemv_swiglu_fm_w8,
csrc/gemv_qfm.hip) against the fp64 restatement and the derived bound of tests/test_mxfp4_gemv_gpu.py and tests/test_fp8_gemv_gpu.py,
whose case generators and helpers are imported: the reference is taken from the PUBLIC layouts (blocks / scales, q / scale), the
kernels read ops.repack_fm_w4 / repack_fm_w8 of them (tests/test_qfm_pack_cpu.py pins that the two decode to the same W_eff).

The bound: every product x[k] * W_eff[n, k] is exact in fp32, so the fp32 dot product differs from the exact one only by its K - 1
additions, in ANY order -- inside one MFMA, across k pieces, across the 8 waves whose partial tiles wave 0 sums from LDS:
E = 2 K u sum_k |x[k] W_eff[n, k]|, plus one bf16 ulp per rounding the epilogue makes (the contracts of gemv_w4 / gemv_w8). Every
element has to be inside; there is no outlier allowance and no fitted tolerance.

Shapes: B 1 = a single row of the B operand, 16 = a full tile, 13 = ragged, 5 / 8 = the engine's row counts. K (MXFP4, pieces of 128):
128 = one piece, 7 of 8 waves have an empty K range; 384 = three pieces, fewer than waves; 1152 = nine, an uneven split with odd counts
against the pieces in flight; 3584 = the workload's hidden size. K (FP8, pieces of 64): 64, 192, 576, 3584 for the same reasons.
N: 16 = one full group, 40 = a ragged last group, 257 = one row in the last group."""
import pytest
import torch

import test_fp8_gemv_gpu as m8
import test_mxfp4_gemv_gpu as m4

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ROWS = [1, 5, 8, 13, 16]
K4 = [128, 384, 1152, 3584]
K8 = [64, 192, 576, 3584]


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


def _plain(m, got, dot, bias, res, what):
    """the epilogue of gemv_w4 / gemv_w8, restated with the helpers of module m: (+bias) -> bf16 -> (+res -> bf16)"""
    v, e = dot
    if bias is not None:
        v = v + bias.double()
        e = e + m.U32 * v.abs()
    if res is not None:
        v, e = m._round(v, e)
        v = v + res.double()
        e = e + m.U32 * v.abs()
    v, e = m._round(v, e)
    m._check(got, v, e, what)


def _swiglu(m, got, dot, I, what):
    """bf16(bf16(silu(bf16(g))) * bf16(u)), the restatement of _check_swiglu in module m"""
    s, E = dot
    g, eg = m._round(s[:, :I], E[:, :I])
    u, eu = m._round(s[:, I:], E[:, I:])
    a = g * torch.sigmoid(g)
    a, ea = m._round(a, 1.1 * eg + 2.0 ** -16 * a.abs())
    v = a * u
    v, e = m._round(v, u.abs() * ea + a.abs() * eu + ea * eu + m.U32 * v.abs())
    m._check(got, v, e, what)


@pytest.mark.parametrize("K", K4)
@pytest.mark.parametrize("N", [16, 40, 257])
@pytest.mark.parametrize("B", ROWS)
def test_gemv_fm_w4(ops, dev, B, N, K):
    blocks, scales, x, bias, res, _ = m4._case(dev, B, N, K, seed=B + 7 * N + K)
    qfm, efm = ops.repack_fm_w4(blocks, scales)
    dot = m4._dot(x, blocks, scales)
    _plain(m4, ops.gemv_fm_w4(qfm, efm, x, N), dot, None, None, f"gemv_fm_w4 B{B} N{N} K{K}")
    _plain(m4, ops.gemv_fm_w4(qfm, efm, x, N, bias=bias, res=res), dot, bias, res, f"gemv_fm_w4 B{B} N{N} K{K} bias res")


@pytest.mark.parametrize("K", K4)
@pytest.mark.parametrize("I", [16, 48])
@pytest.mark.parametrize("B", ROWS)
def test_gemv_swiglu_fm_w4(ops, dev, B, I, K):
    blocks, scales, x, _, _, _ = m4._case(dev, B, I, K, seed=3 + B + 7 * I + K, rows=2 * I)
    qfm, efm = ops.repack_fm_w4(blocks, scales)
    _swiglu(m4, ops.gemv_swiglu_fm_w4(qfm, efm, x), m4._dot(x, blocks, scales), I, f"gemv_swiglu_fm_w4 B{B} I{I} K{K}")


@pytest.mark.parametrize("K", K8)
@pytest.mark.parametrize("N", [16, 40, 257])
@pytest.mark.parametrize("B", ROWS)
def test_gemv_fm_w8(ops, dev, B, N, K):
    q, scale, x, bias, res, _ = m8._case(dev, B, N, K, seed=B + 7 * N + K)
    qfm = ops.repack_fm_w8(q)
    dot = m8._dot(x, q, scale)
    _plain(m8, ops.gemv_fm_w8(qfm, scale, x, N), dot, None, None, f"gemv_fm_w8 B{B} N{N} K{K}")
    _plain(m8, ops.gemv_fm_w8(qfm, scale, x, N, bias=bias, res=res), dot, bias, res, f"gemv_fm_w8 B{B} N{N} K{K} bias res")


@pytest.mark.parametrize("K", K8)
@pytest.mark.parametrize("I", [16, 48])
@pytest.mark.parametrize("B", ROWS)
def test_gemv_swiglu_fm_w8(ops, dev, B, I, K):
    q, scale, x, _, _, _ = m8._case(dev, B, I, K, seed=3 + B + 7 * I + K, rows=2 * I)
    _swiglu(m8, ops.gemv_swiglu_fm_w8(ops.repack_fm_w8(q), scale, x), m8._dot(x, q, scale), I, f"gemv_swiglu_fm_w8 B{B} I{I} K{K}")


def test_two_calls_are_bit_identical(ops, dev):
    """a load that raced the LDS sum of the partial tiles would show as a difference between two launches"""
    B, N, K = 8, 257, 3584
    blocks, scales, x, bias, res, _ = m4._case(dev, B, N, K, seed=11)
    b2, s2, _, _, _, _ = m4._case(dev, B, 48, K, seed=12, rows=96)
    qfm, efm = ops.repack_fm_w4(blocks, scales)
    q2, e2 = ops.repack_fm_w4(b2, s2)
    q, scale, _, _, _, _ = m8._case(dev, B, N, K, seed=13)
    q8, s8, _, _, _, _ = m8._case(dev, B, 48, K, seed=14, rows=96)
    qf8, qf8gu = ops.repack_fm_w8(q), ops.repack_fm_w8(q8)
    for _ in range(3):
        assert torch.equal(ops.gemv_fm_w4(qfm, efm, x, N, bias=bias, res=res), ops.gemv_fm_w4(qfm, efm, x, N, bias=bias, res=res))
        assert torch.equal(ops.gemv_swiglu_fm_w4(q2, e2, x), ops.gemv_swiglu_fm_w4(q2, e2, x))
        assert torch.equal(ops.gemv_fm_w8(qf8, scale, x, N, bias=bias, res=res), ops.gemv_fm_w8(qf8, scale, x, N, bias=bias, res=res))
        assert torch.equal(ops.gemv_swiglu_fm_w8(qf8gu, s8, x), ops.gemv_swiglu_fm_w8(qf8gu, s8, x))


def test_shapes_outside_the_kernel_raise(ops, dev):
    from spider_amd.lib import SpiderHipError
    assert ops.QFM_MAX_ROWS == 16
    blocks, scales, x, bias, res, _ = m4._case(dev, 17, 16, 128, seed=1, rows=32)
    qfm, efm = ops.repack_fm_w4(blocks[:16], scales[:16])
    qgu, egu = ops.repack_fm_w4(blocks, scales)
    with pytest.raises(ValueError, match="rows"):
        ops.gemv_fm_w4(qfm, efm, x, 16)                                     # B = 17
    with pytest.raises(ValueError, match="rows"):
        ops.gemv_swiglu_fm_w4(qgu, egu, x)
    with pytest.raises(ValueError):
        ops.gemv_fm_w4(qfm, efm, x[:5], 17)                                 # 17 rows would be two groups
    with pytest.raises(ValueError):
        ops.gemv_fm_w4(qfm, efm[:, :, :8], x[:5], 16)                       # one scale dword per row and piece
    with pytest.raises(ValueError):
        ops.gemv_fm_w4(qfm, efm, x[:5, :64], 16)                            # x of another K
    with pytest.raises(ValueError):
        ops.gemv_fm_w4(qfm.view(torch.int8), efm, x[:5], 16)
    q, scale, x8, _, _, _ = m8._case(dev, 17, 16, 64, seed=2, rows=32)
    qf8 = ops.repack_fm_w8(q[:16])
    with pytest.raises(ValueError, match="rows"):
        ops.gemv_fm_w8(qf8, scale[:16], x8, 16)
    with pytest.raises(ValueError, match="rows"):
        ops.gemv_swiglu_fm_w8(ops.repack_fm_w8(q), scale, x8)
    with pytest.raises(ValueError):
        ops.gemv_fm_w8(qf8, scale[:15], x8[:5], 16)                         # one scale per weight row
    with pytest.raises(ValueError):
        ops.gemv_swiglu_fm_w8(ops.repack_fm_w8(q[:24]), scale[:24], x8[:5])  # 24 rows are no [gate | up] of I % 16 == 0
    # the same refusals from the entry points themselves
    from spider_amd import lib
    p = lambda t: t.data_ptr()
    with pytest.raises(SpiderHipError, match="multiple of 128"):
        lib.call("spider_gemv_fm_w4", p(qfm), p(efm), p(x), p(bias), None, None, 5, 16, 192, None)
    with pytest.raises(SpiderHipError, match=r"1\.\.16"):
        lib.call("spider_gemv_fm_w8", p(qf8), p(scale), p(x8), p(bias), None, None, 17, 16, 64, None)


def test_torch_ops_registration(ops, dev):
    import spider_amd.torch_ops as T
    assert T.QFM_OP_NAMES == ("gemv_fm_w4", "gemv_swiglu_fm_w4", "gemv_fm_w8", "gemv_swiglu_fm_w8")
    blocks, scales, x, bias, res, _ = m4._case(dev, 5, 40, 128, seed=5)
    qfm, efm = ops.repack_fm_w4(blocks, scales)
    assert torch.equal(torch.ops.spider_hip.gemv_fm_w4(qfm, efm, x, 40, bias, res), ops.gemv_fm_w4(qfm, efm, x, 40, bias=bias, res=res))
    b2, s2, _, _, _, _ = m4._case(dev, 5, 16, 128, seed=6, rows=32)
    q2, e2 = ops.repack_fm_w4(b2, s2)
    assert torch.equal(torch.ops.spider_hip.gemv_swiglu_fm_w4(q2, e2, x), ops.gemv_swiglu_fm_w4(q2, e2, x))
    torch.library.opcheck(torch.ops.spider_hip.gemv_fm_w4, (qfm, efm, x, 40, bias, res), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.spider_hip.gemv_swiglu_fm_w4, (q2, e2, x), test_utils=("test_schema", "test_faketensor"))
    q, scale, x8, bias8, res8, _ = m8._case(dev, 5, 40, 64, seed=7)
    qf8 = ops.repack_fm_w8(q)
    assert torch.equal(torch.ops.spider_hip.gemv_fm_w8(qf8, scale, x8, 40, bias8, res8), ops.gemv_fm_w8(qf8, scale, x8, 40, bias=bias8, res=res8))
    q8, s8, _, _, _, _ = m8._case(dev, 5, 16, 64, seed=8, rows=32)
    qf8gu = ops.repack_fm_w8(q8)
    assert torch.equal(torch.ops.spider_hip.gemv_swiglu_fm_w8(qf8gu, s8, x8), ops.gemv_swiglu_fm_w8(qf8gu, s8, x8))
    torch.library.opcheck(torch.ops.spider_hip.gemv_fm_w8, (qf8, scale, x8, 40, bias8, res8), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.spider_hip.gemv_swiglu_fm_w8, (qf8gu, s8, x8), test_utils=("test_schema", "test_faketensor"))

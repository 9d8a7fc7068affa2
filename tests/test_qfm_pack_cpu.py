"""CPU: the fragment-major layouts of the weight-only MFMA GEMVs (ops.repack_fm_w4 / repack_fm_w8, csrc/gemv_qfm.hip) against an
independent restatement of their index formula, element by element, and the inverses ops.unpack_fm_w4 / unpack_fm_w8.

The formula, as the kernel reads it (lane = 16 g + r, g = 0..3, r = 0..15, NG = ceil(N / 16)):
  MXFP4  qfm [NG, K / 128, 64, 16]: byte 4 sx + j of lane 16 g + r in piece (rg, kb) = blocks[16 rg + r, (128 kb + 32 sx + 8 g) / 2 + j]
         efm [NG, K / 128, 16, 4]:  byte (r, sx) of piece (rg, kb) = scales[16 rg + r, 4 kb + sx]
  FP8    qfm [NG, K / 64, 64, 16]:  byte 8 sx + e of lane 16 g + r in piece (rg, kb) = q[16 rg + r, 64 kb + 32 sx + 8 g + e]
Rows past N hold nibble code 0 and scale byte 127 (FP8: byte 0). The GPU tests take their reference from the public layouts, which
the last test licenses: dequantising the unpacked copy is dequantising the original."""
import pytest
import torch

from spider_amd import ops
from spider_amd.llm import dequantize_fp8_rows, dequantize_mxfp4

U8 = torch.uint8
W4_SHAPES = [(16, 128), (40, 384), (1, 128), (33, 256)]
W8_SHAPES = [(16, 64), (40, 192), (1, 64), (33, 192)]


def _w4(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    blocks = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32).to(U8)
    scales = torch.randint(1, 255, (N, K // 32), generator=g, dtype=torch.int32).to(U8)
    return blocks, scales


def _w8(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, (N, K), generator=g, dtype=torch.int32).to(U8)
    b[(b & 0x7f) == 0x7f] = 0x38          # no NaN byte
    return b.view(ops.FP8)


@pytest.mark.parametrize("N,K", W4_SHAPES)
def test_repack_fm_w4_is_the_index_formula(N, K):
    blocks, scales = _w4(N, K, 7 * N + K)
    qfm, efm = ops.repack_fm_w4(blocks, scales)
    NG = (N + 15) // 16
    assert qfm.dtype == U8 and efm.dtype == U8 and qfm.is_contiguous() and efm.is_contiguous()
    assert tuple(qfm.shape) == (NG, K // 128, 64, 16) and tuple(efm.shape) == (NG, K // 128, 16, 4)
    bl, sl, ql, el = blocks.tolist(), scales.tolist(), qfm.tolist(), efm.tolist()
    for rg in range(NG):
        for kb in range(K // 128):
            for r in range(16):
                n = 16 * rg + r
                for sx in range(4):
                    assert el[rg][kb][r][sx] == (sl[n][4 * kb + sx] if n < N else 127), (rg, kb, r, sx)
                    for g in range(4):
                        for j in range(4):
                            want = bl[n][(128 * kb + 32 * sx + 8 * g) // 2 + j] if n < N else 0
                            assert ql[rg][kb][16 * g + r][4 * sx + j] == want, (rg, kb, g, r, sx, j)
    b2, s2 = ops.unpack_fm_w4(qfm, efm, N)
    assert torch.equal(b2, blocks) and torch.equal(s2, scales) and b2.is_contiguous() and s2.is_contiguous()


@pytest.mark.parametrize("N,K", W8_SHAPES)
def test_repack_fm_w8_is_the_index_formula(N, K):
    q = _w8(N, K, 5 * N + K)
    qfm = ops.repack_fm_w8(q)
    NG = (N + 15) // 16
    assert qfm.dtype == U8 and qfm.is_contiguous() and tuple(qfm.shape) == (NG, K // 64, 64, 16)
    bl, ql = q.view(U8).tolist(), qfm.tolist()
    for rg in range(NG):
        for kb in range(K // 64):
            for r in range(16):
                n = 16 * rg + r
                for g in range(4):
                    for sx in range(2):
                        for e in range(8):
                            want = bl[n][64 * kb + 32 * sx + 8 * g + e] if n < N else 0
                            assert ql[rg][kb][16 * g + r][8 * sx + e] == want, (rg, kb, g, r, sx, e)
    q2 = ops.unpack_fm_w8(qfm, N, K)
    assert q2.dtype == ops.FP8 and torch.equal(q2.view(U8), q.view(U8)) and q2.is_contiguous()


def test_padding_rows_carry_code_0_and_scale_byte_127():
    blocks, scales = _w4(33, 256, 1)
    qfm, efm = ops.repack_fm_w4(blocks, scales)
    # the last group holds row 32 alone: lanes with r >= 1 are padding
    assert bool((qfm[2].view(2, 4, 16, 16)[:, :, 1:] == 0).all()) and bool((efm[2][:, 1:] == 127).all())
    assert torch.equal(efm[2][:, 0].reshape(-1), scales[32])
    q8 = ops.repack_fm_w8(_w8(33, 192, 2))
    assert bool((q8[2].view(3, 4, 16, 16)[:, :, 1:] == 0).all())


def test_shapes_outside_the_layout_raise():
    for K in (32, 64, 192, 320):                                   # multiples of 32 (the row-major rule), not of 128
        with pytest.raises(ValueError, match="128"):
            ops.repack_fm_w4(*_w4(16, K, 3))
    for K in (16, 32, 96):                                         # multiples of 16 (the row-major rule), not of 64
        with pytest.raises(ValueError, match="64"):
            ops.repack_fm_w8(_w8(16, K, 3))
    blocks, scales = _w4(16, 128, 3)
    with pytest.raises(ValueError):
        ops.repack_fm_w4(blocks, scales[:, :3])                    # one scale per block of 32
    with pytest.raises(ValueError):
        ops.repack_fm_w4(blocks.view(torch.int8), scales)
    with pytest.raises(ValueError):
        ops.repack_fm_w8(_w8(16, 64, 3).view(U8))                  # bytes have to come as float8_e4m3fn
    qfm, efm = ops.repack_fm_w4(blocks, scales)
    with pytest.raises(ValueError):
        ops.unpack_fm_w4(qfm, efm, 17)                             # 17 rows are two groups
    with pytest.raises(ValueError):
        ops.unpack_fm_w8(ops.repack_fm_w8(_w8(16, 64, 3)), 16, 128)


def test_dequantising_the_unpacked_copy_is_dequantising_the_original():
    """the whole op restated on the CPU in fp64: x @ W_eff^T from the fragment-major copy equals it from the public layout, exactly"""
    for N, K in W4_SHAPES:
        blocks, scales = _w4(N, K, N + K)
        scales = (scales % 29 + 107).to(U8)                        # (the GPU tests' range: every W_eff finite in bf16)
        a = dequantize_mxfp4(*ops.unpack_fm_w4(*ops.repack_fm_w4(blocks, scales), N))
        b = dequantize_mxfp4(blocks, scales)
        assert a.dtype == torch.bfloat16 and torch.equal(a, b)
        x = torch.randn(3, K, generator=torch.Generator().manual_seed(K)).bfloat16().double()
        assert torch.equal(x @ a.double().T, x @ b.double().T)
    for N, K in W8_SHAPES:
        q = _w8(N, K, N + K)
        sc = torch.ldexp(torch.ones(N), (torch.arange(N) % 16 - 12).to(torch.int32))
        a = dequantize_fp8_rows(ops.unpack_fm_w8(ops.repack_fm_w8(q), N, K), sc)
        b = dequantize_fp8_rows(q, sc)
        assert torch.equal(a, b)
        x = torch.randn(3, K, generator=torch.Generator().manual_seed(K)).bfloat16().double()
        assert torch.equal(x @ a.double().T, x @ b.double().T)


def test_constants_and_registration():
    import spider_amd.torch_ops as T
    from spider_amd import lib
    assert ops.QFM_MAX_ROWS == 16
    assert T.QFM_OP_NAMES == ("gemv_fm_w4", "gemv_swiglu_fm_w4", "gemv_fm_w8", "gemv_swiglu_fm_w8")
    for n in T.QFM_OP_NAMES:
        assert hasattr(torch.ops.spider_hip, n) and n not in T.OP_NAMES
        assert "spider_" + n in lib.SIGNATURES
    l = lib.load()
    # host-side refusals before any launch, no GPU needed
    assert l.spider_gemv_fm_w4(None, None, None, None, None, None, 5, 16, 192, None) == -1 and b"128" in l.spider_last_error()
    assert l.spider_gemv_fm_w8(None, None, None, None, None, None, 5, 16, 96, None) == -1 and b"64" in l.spider_last_error()
    assert l.spider_gemv_fm_w4(None, None, None, None, None, None, 17, 16, 128, None) == -1 and b"1..16" in l.spider_last_error()
    assert l.spider_gemv_swiglu_fm_w8(None, None, None, None, 5, 24, 64, None) == -1 and b"multiple of 16" in l.spider_last_error()
    assert l.spider_gemv_swiglu_fm_w4(None, None, None, None, 5, 16, 128, None) == -1 and b"null" in l.spider_last_error()

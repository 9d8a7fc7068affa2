"""The FP8 and the MXFP4 decode GEMVs (ops.gemv_w8 / ops.gemv_w4, csrc/gemv_wq.hip) stage the same activations, bit for bit.

Both formats go through one staging routine (csrc/wq_common.hpp: stage_rows_branchfree) that differs only in the LDS slot a vector
is stored to. One-hot weight rows W[n, k_n] = 1 read the staged copy back: every product but one is an exact zero, so out[b, n] is
exactly xin[b, k_n], the plain x or bf16(bf16(x * rs) * norm_w). The test asserts torch.equal between the two formats, and each
against the fp64 RMSNorm within the two bf16 roundings that form has (the bound of tests/test_fp8_gemv_gpu.py and
tests/test_mxfp4_gemv_gpu.py: one ulp of slack per rounding; the plain form must be x itself).

K reaches every form of the staging (NT = threads per block, CAP = stage_cap vectors of 8 elements per thread, CH = CAP / 2):
64 = a single partial batch of vectors; 1056 = not a whole chunk of either format; 4128 = 4 waves, the normalised row no longer fits
the registers (CH * NT * 8 = 4096); 8224 = 8 waves, one batch; 12320 = 8 waves, batched (CH * NT * 8 = 12288), and at four rows
104 KiB (FP8) / 112 KiB (MXFP4) of LDS, above the 64 KiB a launch gets without opting in.
Columns k_n: 0, 7, 8, K - 8, K - 1, both sides of every multiple of 1024 (so of 2048: the chunk of either format) below K, both
sides of CH * NT * 8 and CAP * NT * 8 where they lie inside the row, and 32 seeded others."""
import pytest
import torch

BF = torch.bfloat16
U8 = torch.uint8
ULP16 = 2.0 ** -7
EPS = 1e-5
KS = [64, 1056, 4128, 8224, 12320]


def _columns(K):
    nt = 512 if K >= 8192 else 256            # the dispatch rule: 8 waves per block from K = 8192
    cap = 6 if nt == 512 else 4
    cols = {0, 7, 8, K - 8, K - 1}
    for edge in list(range(1024, K, 1024)) + [cap // 2 * nt * 8, cap * nt * 8]:
        if 0 < edge < K:
            cols |= {edge - 1, edge}
    g = torch.Generator().manual_seed(K)
    cols |= set(torch.randint(0, K, (32,), generator=g).tolist())
    return sorted(cols)


def _one_hot(K):
    """(columns, FP8 bytes [N, K] + scales [N], MXFP4 blocks [N, K / 2] + scales [N, K / 32]) on the CPU, rows W[n, cols[n]] = 1:
    FP8 byte 0x38 with scale 1.0, MXFP4 code 2 with scale byte 127. Checked with the engine's own dequantisers."""
    from spider_amd.llm import dequantize_fp8_rows, dequantize_mxfp4
    cols = torch.tensor(_columns(K))
    N = cols.numel()
    n = torch.arange(N)
    q8 = torch.zeros(N, K, dtype=U8)
    q8[n, cols] = 0x38
    s8 = torch.ones(N, dtype=torch.float32)
    q4 = torch.zeros(N, K // 2, dtype=U8)
    q4[n, cols // 2] = torch.where(cols % 2 == 1, 0x20, 0x02).to(U8)
    s4 = torch.full((N, K // 32), 127, dtype=U8)
    want = torch.zeros(N, K, dtype=torch.float64)
    want[n, cols] = 1.0
    assert torch.equal(dequantize_fp8_rows(q8.view(torch.float8_e4m3fn), s8, torch.float64), want)
    assert torch.equal(dequantize_mxfp4(q4, s4, torch.float64), want)
    return cols, q8.view(torch.float8_e4m3fn), s8, q4, s4


@pytest.mark.parametrize("K", KS)
def test_one_hot_rows_dequantise_to_exact_ones_and_zeros(K):
    cols = _one_hot(K)[0]
    assert cols.numel() < 100 and int(cols.min()) == 0 and int(cols.max()) == K - 1


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("B", [1, 4])
def test_fp8_and_mxfp4_stage_the_same_activations(dev, B, K):
    from spider_amd import ops
    cols, q8, s8, q4, s4 = (t.to(dev) for t in _one_hot(K))
    assert ops.w8_norm_fits(B, K) and ops.w4_norm_fits(B, K)
    g = torch.Generator().manual_seed(B + K)
    x = torch.randn(B, K, generator=g).to(BF).to(dev)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF).to(dev)

    plain8, plain4 = ops.gemv_w8(q8, s8, x), ops.gemv_w4(q4, s4, x)
    assert torch.equal(plain8, plain4), f"plain B{B} K{K}: the formats differ"
    assert torch.equal(plain8, x[:, cols]), f"plain B{B} K{K}: not the staged x"

    norm8, norm4 = ops.gemv_w8(q8, s8, x, norm_w=nw, eps=EPS), ops.gemv_w4(q4, s4, x, norm_w=nw, eps=EPS)
    assert torch.equal(norm8, norm4), f"norm B{B} K{K}: the formats differ"
    xd = x.double()
    rs = torch.rsqrt((xd * xd).mean(-1, keepdim=True) + EPS)
    ref = (((xd * rs).to(BF).double() * nw.double()).to(BF).double())[:, cols]
    tol = ULP16 * ref.abs() * (1 + ULP16) + ULP16 * ref.abs() + 1e-30
    err = (norm8.double() - ref).abs()
    print(f"norm B{B} K{K}: max err / tol {float((err / tol).max()):.3g}")
    assert bool((err <= tol).all()), f"norm B{B} K{K}: max err / tol {float((err / tol).max()):.3g}"

"""Shared by tests/test_gptq_cpu.py, tests/test_gptq_ops_gpu.py and tests/test_llm_gptq_gpu.py: the cases of calibrated MXFP4
(`llm.quantize_mxfp4_gptq`), the near-tie rule under which an fp32 run is compared with the fp64 definition, and the figures."""
import functools

import torch

NEAR_TIE = 2e-5         # a row is a near-tie row when the fp64 run came this close to a rounding midpoint or to mantissa 0.75
NEAR_TIE_CAP = 0.10     # at most this share of a case's rows may be near-tie rows (a condition on the seeds, not on the code)


@functools.lru_cache(maxsize=None)
def correlated_case(N, K, T, seed):
    """(W [N, K] bf16-valued fp32, X [T, K] fp64, H = X^T X fp64): W ~ N(0, 0.02^2), inputs of rank 16 plus 0.3 isotropic noise"""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=g) * 0.02).bfloat16().float()
    X = (torch.randn(T, 16, generator=g) @ torch.randn(16, K, generator=g) + 0.3 * torch.randn(T, K, generator=g)).double()
    return W, X, X.t() @ X


@functools.lru_cache(maxsize=None)
def definition(N, K, T, seed):
    """the fp64 definition on `correlated_case`: (blocks, scales, near-tie mask [N])"""
    from spider_amd.llm import quantize_mxfp4_gptq
    W, X, H = correlated_case(N, K, T, seed)
    tr = {}
    b, s = quantize_mxfp4_gptq(W, H, trace=tr)
    return b, s, near_tie_rows(tr)


def near_tie_rows(trace):
    return (trace["mid_gap"] <= NEAR_TIE) | (trace["mant_gap"] <= NEAR_TIE)


def out_err(W, X, blocks, scales):
    """||X (W - Q)^T|| / ||X W^T|| in fp64"""
    from spider_amd.llm import dequantize_mxfp4
    Q = dequantize_mxfp4(blocks.cpu(), scales.cpu(), torch.float32).double()
    Wd = W.double().cpu()
    return float((X @ (Wd - Q).t()).norm() / (X @ Wd.t()).norm())


def codes_of(blocks):
    """[N, K] nibble codes from the packed bytes"""
    return torch.stack([blocks & 15, blocks >> 4], dim=2).reshape(blocks.shape[0], -1)


# (N, K, T, seed) of the device comparison: one row and one block; a second wave and a trailing update; a tail group narrower
# than the launch width; several launches. The seeds are checked against NEAR_TIE_CAP on the CPU (tests/test_gptq_cpu.py).
DEVICE_CASES = ((1, 32, 256, 11), (65, 64, 512, 12), (37, 96, 512, 13), (200, 256, 1024, 21))

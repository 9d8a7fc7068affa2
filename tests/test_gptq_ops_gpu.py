"""GPU: ops.gptq_mxfp4 (fp64 factor, fp32 sweep kernel of csrc/gptq.hip, fp32 trailing GEMMs) against the fp64 definition
`llm.quantize_mxfp4_gptq` on the same (W, H).

The device run rounds where the definition does not, so a decision that the definition took by a hair may fall the other way --
and, the rule being sequential, the rest of that ROW then differs legitimately. A row is a near-tie row when the fp64 run came
within 2e-5 (relative; absolute below 1) of a rounding midpoint with some |w_i| / s, or within 2e-5 of 0.75 with some block's
frexp mantissa (gptq_cases.near_tie_rows). Every other row must match byte for byte; near-tie rows are at most 10 % of a case's
rows (checked for these seeds on the CPU in tests/test_gptq_cpu.py); and on ALL rows the relative output error on the generating X
must be within 1 % of the definition's."""
import pytest
import torch

import gptq_cases as GC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,K,T,seed", GC.DEVICE_CASES)
def test_device_sweep_equals_the_definition(dev, N, K, T, seed):
    from spider_amd import ops
    W, X, H = GC.correlated_case(N, K, T, seed)
    b_ref, s_ref, tie = GC.definition(N, K, T, seed)
    assert int(tie.sum()) <= GC.NEAR_TIE_CAP * N
    b, s = ops.gptq_mxfp4(W.to(dev).bfloat16(), H.to(dev))
    assert b.is_cuda and b.dtype == torch.uint8 and s.dtype == torch.uint8 and b.shape == (N, K // 2) and s.shape == (N, K // 32)
    b, s = b.cpu(), s.cpu()
    row_ok = (b == b_ref).all(dim=1) & (s == s_ref).all(dim=1)
    e_ref, e_dev = GC.out_err(W, X, b_ref, s_ref), GC.out_err(W, X, b, s)
    print(f"({N}, {K}): {int((~row_ok).sum())} rows differ, {int(tie.sum())} near-tie rows; output error definition {e_ref:.6f} device {e_dev:.6f}")
    assert bool(row_ok[~tie].all()), f"rows {torch.nonzero(~row_ok & ~tie).flatten().tolist()} differ without a near tie"
    assert abs(e_dev - e_ref) <= 0.01 * e_ref
    # the group width changes the fp32 summation order of the compensation and nothing else
    for gb in (1, 2, 3):
        b2, s2 = ops.gptq_mxfp4(W.to(dev), H.to(dev), group_blocks=gb)
        ok2 = (b2.cpu() == b_ref).all(dim=1) & (s2.cpu() == s_ref).all(dim=1)
        assert bool(ok2[~tie].all()), gb
        assert abs(GC.out_err(W, X, b2, s2) - e_ref) <= 0.01 * e_ref


@pytest.mark.parametrize("N,K", [(1, 32), (65, 64), (37, 96), (200, 256)])
def test_diagonal_hessian_gives_round_to_nearest_bytes_on_every_row(dev, N, K):
    from spider_amd import ops
    from spider_amd.llm import quantize_mxfp4
    g = torch.Generator().manual_seed(N + K)
    W = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    W[0, :32] = 0.0                                     # an all-zero block
    if N > 1:
        W[1, :32] = 0.0
        W[1, 7], W[1, 9] = 0.5, -0.01                   # a negative entry that rounds to -0
    b0, s0 = quantize_mxfp4(W)
    for H in (torch.eye(K, dtype=torch.float64), torch.diag(torch.rand(K, generator=g).double() * 50.0 + 0.05)):
        b, s = ops.gptq_mxfp4(W.to(dev), H.to(dev))
        assert torch.equal(b.cpu(), b0) and torch.equal(s.cpu(), s0)


def test_custom_op_gives_the_same_bytes(dev):
    import spider_amd.torch_ops  # noqa: F401
    from spider_amd import ops
    W, X, H = GC.correlated_case(65, 64, 512, 12)
    Wd, Hd = W.to(dev).bfloat16(), H.to(dev)
    b, s = ops.gptq_mxfp4(Wd, Hd, 0.02)
    b2, s2 = torch.ops.spider_hip.gptq_mxfp4(Wd, Hd, 0.02)
    assert torch.equal(b, b2) and torch.equal(s, s2)
    b3, _ = torch.ops.spider_hip.gptq_mxfp4(Wd, Hd)    # (another damp is another result)
    assert not torch.equal(b, b3)


def test_driver_validation(dev):
    from spider_amd import ops
    W, H = torch.zeros(4, 64, device=dev), torch.eye(64, device=dev)
    with pytest.raises(ValueError, match="W has to be"):
        ops.gptq_mxfp4(W[:, :40], H[:40, :40])
    with pytest.raises(ValueError, match="H has to be"):
        ops.gptq_mxfp4(W, H[:32, :32])
    with pytest.raises(ValueError, match="damp"):
        ops.gptq_mxfp4(W, H, 0.0)
    with pytest.raises(ValueError, match="group_blocks"):
        ops.gptq_mxfp4(W, H, group_blocks=5)

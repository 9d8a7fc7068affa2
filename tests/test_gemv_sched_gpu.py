"""GPU: the two memory schedules of the decode GEMVs (spider_set_gemv_sched: 0 = one request at a time, 1 = one round trip per
block, the default) do the same arithmetic in the same order, so their outputs are bit-identical for every shape; the schedule-1
outputs are also checked against the fp32 product at the tolerances of tests/test_hip_ops.py::test_gemv / ::test_gemv_swiglu
(a switch that selected the same code twice would pass the equality and prove nothing -- hence also the setter's return value).

Shapes: K = 64 (fewer chunks than lanes), 1032 (a partly filled last chunk), 3584 (7 chunks, the model's), 4096 (8 chunks: the
whole-row cap), 4104 (one past it: the k loop with a tail); N not a multiple of the rows of a block; 2..4 sequences through the
fused RMSNorm; the long-K form (8 waves per block) with an even and an odd number of chunk sets and a tail chunk."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def close(got, ref, atol, rtol, what):
    """|got - ref| <= atol * std(ref) + rtol * |ref| elementwise (the measure of tests/test_hip_ops.py, rel_to_std form)"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs()
    tol = atol * float(ref.std()) + rtol * ref.abs()
    assert not bool((err > tol).any()), f"{what}: max err {float(err.max()):.4g}, {int((err > tol).sum())} / {err.numel()} out of tolerance"


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


def both(fn):
    """fn() under schedule 0 and under schedule 1 (previous setting restored); asserts the setter returns what was set"""
    from spider_amd import lib as slib
    lib = slib.load()
    prev = lib.spider_set_gemv_sched(0)
    try:
        y0 = fn().clone()
        assert lib.spider_set_gemv_sched(1) == 0
        y1 = fn().clone()
        assert lib.spider_set_gemv_sched(1) == 1
    finally:
        lib.spider_set_gemv_sched(prev)
    assert torch.equal(y0, y1), f"schedules differ in {int((y0 != y1).sum())} / {y0.numel()} elements"
    return y1


def check_gemv(ops, dev, B, N, K, forms):
    from oracle.llama import rmsnorm
    W, x = rnd(N, K, seed=1, scale=0.05), rnd(B, K, seed=2)
    bias, res, nw = rnd(N, seed=3), rnd(B, N, seed=4), (1 + 0.1 * rnd(K, seed=5).float()).to(BF)
    Wd, xd = W.to(dev), x.to(dev)
    ref = x.float() @ W.float().T
    if "plain" in forms:
        close(both(lambda: ops.gemv(Wd, xd)), ref, 1e-2, 1e-2, "gemv")
    if "bias_res" in forms:
        bd, rd = bias.to(dev), res.to(dev)
        close(both(lambda: ops.gemv(Wd, xd, bias=bd, res=rd)), ref + bias.float() + res.float(), 1.5e-2, 1e-2, "gemv+bias+res")
    if "norm" in forms:
        nd = nw.to(dev)
        xn = rmsnorm(x.float(), nw.float(), 1e-5).to(BF).float()
        close(both(lambda: ops.gemv(Wd, xd, norm_w=nd, eps=1e-5)), xn @ W.float().T, 2e-2, 1e-2, "gemv+norm")


@pytest.mark.parametrize("K", [64, 1032, 3584, 4096, 4104])
@pytest.mark.parametrize("N", [7, 24, 37])
def test_qkv_o_form(ops, dev, N, K):
    check_gemv(ops, dev, 1, N, K, ("plain", "bias_res", "norm"))


@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("N,K", [(24, 1032), (37, 4096)])
def test_batched_norm(ops, dev, B, N, K):
    check_gemv(ops, dev, B, N, K, ("norm",))


@pytest.mark.parametrize("K", [8192, 8704, 9224])
@pytest.mark.parametrize("N", [16, 37])
def test_long_k_form(ops, dev, N, K):
    check_gemv(ops, dev, 1, N, K, ("plain", "bias_res"))


@pytest.mark.parametrize("K", [1032, 3584])
@pytest.mark.parametrize("I", [20, 37])
@pytest.mark.parametrize("B", [1, 4])
def test_gemv_swiglu(ops, dev, B, I, K):
    W, x = rnd(2 * I, K, seed=1, scale=0.05), rnd(B, K, seed=2)
    Wd, xd = W.to(dev), x.to(dev)
    g, u = x.float() @ W[:I].float().T, x.float() @ W[I:].float().T
    close(both(lambda: ops.gemv_swiglu(Wd, xd)), F.silu(g) * u, 1.5e-2, 2e-2, "gemv_swiglu")
    # the form the model runs: fused RMSNorm in front (reference on the same bf16-rounded normalised activations)
    from oracle.llama import rmsnorm
    nw = (1 + 0.1 * rnd(K, seed=5).float()).to(BF)
    nd = nw.to(dev)
    xn = rmsnorm(x.float(), nw.float(), 1e-5).to(BF).float()
    gn, un = xn @ W[:I].float().T, xn @ W[I:].float().T
    close(both(lambda: ops.gemv_swiglu(Wd, xd, norm_w=nd, eps=1e-5)), F.silu(gn) * un, 1.5e-2, 2e-2, "gemv_swiglu+norm")

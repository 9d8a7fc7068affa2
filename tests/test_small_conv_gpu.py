"""fp64 parity of the small convolutions of csrc/unet_ops.hip (conv2d_small_cin / _f32in: Cin <= 8, one thread per pixel and 8 output
channels; conv2d_small_cout / _f32in: Cout <= 8, one wave per pixel) at the edges: 1-pixel and 1-wide maps, batches whose images differ
strongly, every lane-chunk count around the 64 lanes, the grid-stride loops past their block caps, and weights that stage just over
64 KiB of LDS. bf16 and f16, every element against the bound derived in tests/pointwise_checks.py; fp32 outputs are held to the
fp32 bound and the 16-bit output has to be the rounding of its fp32 twin."""
import pytest
import torch

import pointwise_checks as pc

pytestmark = pytest.mark.gpu

DT_IDS = [pc.name(d) for d in pc.DTYPES]
F32 = torch.float32


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


@pytest.fixture(scope="module")
def err():
    from spider_amd.lib import SpiderHipError
    return SpiderHipError


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    best, _ = pc.summary()
    for k in sorted(best):
        if k[0].startswith("conv2d"):
            print(f"[small conv summary] {k[0]} {k[1]} out={k[2]}: largest err / bound = {best[k]:.3f}")


def run_cin(ops, dev, case, dt, form):
    x, w, bias = pc.conv_inputs(case, dt)
    B, H, W, Cin, Cout, ks, use_bias = case
    bd = bias.to(dev) if use_bias else None
    if form == "h16":
        y = pc.into("conv2d_small_cin", (B, H, W, Cout), dt, dev, lambda o: ops.conv2d_small_cin(x.to(dt).to(dev), w.to(dev), bd, out=o))
        return pc.conv_verify("conv2d_small_cin", case, dt, False, y16=y)
    if form == "f32in":
        y = ops.conv2d_small_cin_f32in(x.to(dev), w.to(dev), bd)
        return pc.conv_verify("conv2d_small_cin_f32in", case, dt, True, y16=y.cpu())
    y, y32 = ops.conv2d_small_cin_f32in(x.to(dev), w.to(dev), bd, want32=True)
    return pc.conv_verify("conv2d_small_cin_f32in", case, dt, True, y16=y.cpu(), y32=y32.cpu())


def run_cout(ops, dev, case, dt, form):
    x, w, bias = pc.conv_inputs(case, dt)
    B, H, W, Cin, Cout, ks, use_bias = case
    bd = bias.to(dev) if use_bias else None
    if form == "f32in":
        return pc.conv_verify("conv2d_small_cout_f32in", case, dt, True, y32=ops.conv2d_small_cout_f32in(x.to(dev), w.to(dev), bd).cpu())
    xd = x.to(dt).to(dev)
    y32 = pc.into("conv2d_small_cout", (B, H, W, Cout), F32, dev, lambda o: ops.conv2d_small_cout(xd, w.to(dev), bd, out=o))
    y16 = pc.into("conv2d_small_cout", (B, H, W, Cout), dt, dev, lambda o: ops.conv2d_small_cout(xd, w.to(dev), bd, out_f32=False, out=o))
    return pc.conv_verify("conv2d_small_cout", case, dt, False, y16=y16, y32=y32)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ["h16", "f32in", "f32in_want32"])
def test_conv2d_small_cin(ops, dev, form, dt):
    for case in pc.cin_cases():
        if case != pc.CIN_LDS_CASE:
            run_cin(ops, dev, case, dt, form)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ["16_and_f32", "f32in"])
def test_conv2d_small_cout(ops, dev, form, dt):
    for case in pc.cout_cases():
        if case != pc.COUT_LDS_CASE:
            run_cout(ops, dev, case, dt, form)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ["h16", "f32in_want32"])
def test_conv2d_small_cin_above_64k_lds(ops, dev, form, dt):
    """Cout 232 x 3 x 3 x Cin 8 x 4 B = 66,816 B of staged weights"""
    run_cin(ops, dev, pc.CIN_LDS_CASE, dt, form)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ["16_and_f32", "f32in"])
def test_conv2d_small_cout_above_64k_lds(ops, dev, form, dt):
    """Cout 8 x 3 x 3 x Cin 456 x 2 B = 65,664 B of staged weights"""
    run_cout(ops, dev, pc.COUT_LDS_CASE, dt, form)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_small_conv_rejects(ops, dev, err, dt):
    def t(*shape, dtype=dt):
        return torch.ones(*shape, dtype=dtype, device=dev)

    for Cin, Cout, ks in ((9, 8, 3), (4, 12, 3), (4, 8, 5)):
        buf, out = pc.guarded((1, 4, 4, Cout), dt, dev)
        with pytest.raises(err):
            ops.conv2d_small_cin(t(1, 4, 4, Cin), t(Cout, ks, ks, Cin), out=out)
        with pytest.raises(err):
            ops.conv2d_small_cin_f32in(t(1, 4, 4, Cin, dtype=F32), t(Cout, ks, ks, Cin))
        assert pc.untouched(buf), "a rejected conv2d_small_cin wrote to its output"
    for Cin, Cout, ks in ((8, 9, 3), (12, 4, 3), (8, 4, 5)):
        buf, out = pc.guarded((1, 4, 4, Cout), F32, dev)
        with pytest.raises(err):
            ops.conv2d_small_cout(t(1, 4, 4, Cin), t(Cout, ks, ks, Cin), out=out)
        with pytest.raises(err):
            ops.conv2d_small_cout_f32in(t(1, 4, 4, Cin, dtype=F32), t(Cout, ks, ks, Cin))
        assert pc.untouched(buf), "a rejected conv2d_small_cout wrote to its output"
    # both outputs given, or neither: the wrapper cannot express it
    from spider_amd import lib
    x, w = t(1, 4, 4, 8), t(4, 3, 3, 8)
    y32, y16 = t(1, 4, 4, 4, dtype=F32), t(1, 4, 4, 4)
    sym = f"spider_conv2d_small_cout_{'f16' if dt == torch.float16 else 'bf16'}"
    for a, b in ((y32.data_ptr(), y16.data_ptr()), (None, None)):
        with pytest.raises(err):
            lib.call(sym, x.data_ptr(), w.data_ptr(), None, a, b, 1, 4, 4, 8, 4, 3, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((y32.cpu() == 1).all()) and bool((y16.cpu().float() == 1).all())

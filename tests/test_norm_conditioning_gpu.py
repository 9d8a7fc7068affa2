"""GPU parity of the normalisation kernels (csrc/unet_ops.hip, the GroupNorm producers / consumers of csrc/gemm.hip) against fp64,
on inputs whose mean is NOT small against their spread, at the shapes where the dispatch changes kernel, and in both 16-bit types.

Inputs are randn * sigma + mean (norm_checks.shifted_input): mean / sigma in {0, 4, 16, 64} (and 256 for fp32 inputs), its sign
alternating from group to group with one group at 0, so one tensor mixes conditionings and a wrong group lookup shows. The bounds are
the derived ones of tests/norm_checks.py; every element has to be inside, and the worst err / bound ratio of every check is printed
before its assertion (the measured table is in NOTEBOOK.md).

  routes that run their own statistics pass (ops.groupnorm, groupnorm_cat, groupnorm_f32in / _split without `partial`, layernorm,
  row_split with gamma)                                            -> the `centered` bound: independent of the mean
  routes that consume the public (sum, sum of squares) partials (groupnorm / groupnorm_f32in with `partial`, gemm_gn_in,
  gemm_gn_in_a32, the producing conv)                              -> the `onepass` bound, which grows with (mean / sigma)^2
  gemm_ln                                                          -> gemm_checks.pre_ln (mean-aware already)

The partials are built twice: by ops.groupnorm_stats, and by hand in fp64 rounded to fp32 (exact statistics: isolates the consumer).
The one bound that is not derived is test_precise_ops_gpu.py's relative L2 of the split form (3e-6 f16 / 3e-5 bf16), asserted here
for mean / sigma <= 16 only: beyond that the fp32 rounding of mean * a_c limits the value itself.
"""
import functools

import pytest
import torch

import gemm_checks as gc
import norm_checks as nc

pytestmark = pytest.mark.gpu

DTS = [torch.float16, torch.bfloat16]
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16"}
EPS = 1e-5
SPLIT_L2 = {torch.float16: 3e-6, torch.bfloat16: 3e-5}      # test_precise_ops_gpu.py::test_groupnorm_f32in_split, mean / sigma <= 16

# (B, HW, C, G): the smallest shapes that reach each branch of groupnorm_impl / gn_stats_kernel / gn_apply_kernel
SWEEP_SHAPES = [(1, 64, 320, 32),         # gn_small_kernel
                (1, 1024, 320, 32),       # gn_small_kernel at its boundary HW * C / G = 10240
                (1, 4096, 320, 32)]       # stats + apply, 128 chunks
OTHER_SHAPES = [(2, 32, 320, 32),         # gn_small_kernel, two images
                (1, 40, 8192, 32),        # gn_small_kernel, C / G = 256: pair index 127 in the packed offset
                (1, 1025, 320, 32),       # just outside: stats + apply, ragged last chunk
                (2, 64, 96, 32),          # odd C / G: stats + apply on a small map, an 8-channel vector spans three groups
                (1, 64, 64, 64),          # C / G = 1
                (2, 256, 64, 8), (2, 1056, 320, 16), (1, 256, 1280, 64),      # other G
                (1, 4099, 128, 32),       # per = 33: three empty trailing chunks, a ragged one before them
                (1, 33, 640, 32),         # one ragged chunk
                (1, 320, 2560, 32),       # blocks of 320 threads
                (1, 1, 320, 32)]          # one pixel
CASES16 = [(s, r) for s in SWEEP_SHAPES for r in (0, 4, 16, 64)] + [(s, r) for s in OTHER_SHAPES for r in (0, 16)]
CASES32 = [(s, r) for s in SWEEP_SHAPES for r in (0, 4, 16, 64, 256)] + [(s, r) for s in OTHER_SHAPES for r in (0, 16)]
GEMM_CASES = [(s, r) for s in SWEEP_SHAPES for r in (0, 4, 16, 64)] + [(s, r) for s in [(2, 256, 64, 8), (1, 256, 1280, 64)] for r in (0, 16)]


def case_id(c):
    (B, HW, C, G), r = c
    return f"{B}x{HW}x{C}g{G}-r{r}"


def sigma_of(shape):
    return 2.0 if shape[1] in (1024, 256, 33) else 1.0


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


@pytest.fixture(params=["a32_kernel", "split_once"])
def route(request, ops, monkeypatch):
    """the two routes of the fp32-operand GEMMs, as in test_precise_ops_gpu.py"""
    monkeypatch.setattr(ops, "A32_DUP_MIN_FLOP", float("inf") if request.param == "a32_kernel" else 0.0)
    monkeypatch.setattr(ops, "A32_SPLIT_MIN_FLOP", float("inf"))
    monkeypatch.setattr(ops, "A32_DUP_MIN_M", 0)
    return request.param


@functools.lru_cache(maxsize=2)
def problem(case, dt, fp32_in):
    """the input (as the kernel reads it), gamma, beta and the fp64 problem of one case, computed once"""
    (B, HW, C, G), r = case
    gen = torch.Generator().manual_seed(B * 7919 + HW * 31 + C + G + r)
    x = nc.shifted_input(gen, B, HW, C, G, sigma_of(case[0]), r)
    if not fp32_in:
        x = x.to(dt)
    gamma = (1 + 0.1 * torch.randn(C, generator=gen)).to(dt)
    beta = (0.1 * torch.randn(C, generator=gen)).to(dt)
    return x, gamma, beta, nc.gn64(x, gamma, beta, G, EPS)


def hand_partial(x, G, nchunk):
    """[B, nchunk, G, 2] (sum, sum of squares) per chunk of ceil(HW / nchunk) pixels and group, in fp64, rounded to fp32"""
    B, HW, C = x.shape
    per = -(-HW // nchunk)
    xp = torch.zeros(B, nchunk * per, C, dtype=torch.float64)
    xp[:, :HW] = x.double()
    xg = xp.view(B, nchunk, per, G, C // G)
    return torch.stack([xg.sum((2, 4)), (xg * xg).sum((2, 4))], -1).float().contiguous()


def partials(ops, dev, x16, xsrc, G):
    """{name: GnPartial}: by the statistics kernel (of the 16-bit tensor x16, when there is one) and by hand (of xsrc)"""
    HW = xsrc.shape[1]
    nchunk = ops.groupnorm_nchunk(HW)
    out = {"hand": ops.GnPartial(hand_partial(xsrc, G, nchunk).to(dev), nchunk, G)}
    if x16 is not None:
        out["stats"] = ops.groupnorm_stats(x16.to(dev), G, nchunk)
    return out


# =========================================================================================== routes 1 and 3: 16-bit input
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("case", CASES16, ids=case_id)
def test_groupnorm_16bit_input(ops, dev, case, dt):
    (B, HW, C, G), r = case
    x, gamma, beta, g = problem(case, dt, False)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    parts = partials(ops, dev, x, x, G)
    C1 = 8 * (C // 16) + 8                    # a seam inside a group wherever C / G is not a multiple of 8
    for silu in (False, True):
        tag = f"{case_id(case)} silu={int(silu)}"
        own = nc.norm_ref(g, "centered", dt, "16", silu)
        y = ops.groupnorm(xd, gd, bd, G, EPS, silu)
        nc.check(f"groupnorm {tag}", y, own, dt, fp32_out=False)
        yc, cat = ops.groupnorm_cat(xd[..., :C1].contiguous(), xd[..., C1:].contiguous(), gd, bd, G, EPS, silu)
        assert torch.equal(cat, xd), f"groupnorm_cat {tag}: the concatenated copy is not exact"
        assert torch.equal(yc, y), f"groupnorm_cat {tag}: differs from groupnorm of the materialised concat"
        pub = nc.norm_ref(g, "onepass", dt, "16", silu)
        for name, part in parts.items():
            nc.check(f"groupnorm partial={name} {tag}", ops.groupnorm(xd, gd, bd, G, EPS, silu, partial=part), pub, dt, fp32_out=False)
        # the fp32-input consumer on the same statistics: x32 = the 16-bit values, so the partials are those of what it reads
        pub32 = nc.norm_ref(g, "onepass", dt, "f32in", silu)
        y16, y32 = ops.groupnorm_f32in(xd.float(), gd, bd, G, EPS, silu, partial=parts["stats"], want16=True, want32=True)
        nc.check(f"groupnorm_f32in partial=stats y32 {tag}", y32, pub32, dt, fp32_out=True)
        nc.check(f"groupnorm_f32in partial=stats y {tag}", y16, pub32, dt, fp32_out=False)


# =========================================================================================== routes 2 and 3: fp32 input
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("case", CASES32, ids=case_id)
def test_groupnorm_f32_input(ops, dev, case, dt):
    (B, HW, C, G), r = case
    x, gamma, beta, g = problem(case, dt, True)
    xd, gd, bd = x.to(dev), gamma.to(dev), beta.to(dev)
    hand = partials(ops, dev, None, x, G)["hand"]
    for silu in (False, True):
        tag = f"{case_id(case)} silu={int(silu)}"
        own = nc.norm_ref(g, "centered", dt, "f32in", silu)
        y16, y32 = ops.groupnorm_f32in(xd, gd, bd, G, EPS, silu, want16=True, want32=True)
        nc.check(f"groupnorm_f32in y32 {tag}", y32, own, dt, fp32_out=True)
        nc.check(f"groupnorm_f32in y {tag}", y16, own, dt, fp32_out=False)
        y2 = ops.groupnorm_f32in_split(xd, gd, bd, G, EPS, silu).cpu()
        assert y2.shape == (B, HW, 2 * C)
        R = nc.norm_ref(g, "centered", dt, "split", silu)
        nc.check(f"groupnorm_f32in_split {tag}", y2[..., :C].double() + y2[..., C:].double(), R, dt, fp32_out=True)
        if r <= 16:
            l2 = nc.LOG[-1]["rel_l2"]
            assert l2 < SPLIT_L2[dt], f"groupnorm_f32in_split {tag}: rel L2 {l2:.3e}"
        pub = nc.norm_ref(g, "onepass", dt, "f32in", silu)
        p16, p32 = ops.groupnorm_f32in(xd, gd, bd, G, EPS, silu, partial=hand, want16=True, want32=True)
        nc.check(f"groupnorm_f32in partial=hand y32 {tag}", p32, pub, dt, fp32_out=True)
        nc.check(f"groupnorm_f32in partial=hand y {tag}", p16, pub, dt, fp32_out=False)
        s2 = ops.groupnorm_f32in_split(xd, gd, bd, G, EPS, silu, partial=hand).cpu()
        nc.check(f"groupnorm_f32in_split partial=hand {tag}", s2[..., :C].double() + s2[..., C:].double(),
                 nc.norm_ref(g, "onepass", dt, "split", silu), dt, fp32_out=True)


# =========================================================================================== route 3: GroupNorm inside the GEMM
def check_gemm(what, out, pre, dt):
    c16, c32 = out
    R = gc.finish(pre, dt)
    R.ref, R.tol32 = R.ref.reshape(c32.shape), R.tol32.reshape(c32.shape)
    nc.check(f"{what} c32", c32, R, dt, fp32_out=True)
    nc.check(f"{what} c16", c16, R, dt, fp32_out=False)


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("case", GEMM_CASES, ids=case_id)
def test_gemm_gn_in_on_shifted_groups(ops, dev, route, case, dt):
    (B, HW, C, G), r = case
    N = 320
    x, gamma, beta, _ = problem(case, dt, False)
    gen = torch.Generator().manual_seed(C + HW + r)
    W = (torch.randn(N, C, generator=gen) * C ** -0.5).to(dt)
    bias = (0.1 * torch.randn(N, generator=gen)).to(dt)
    Wd, bd_, gd, btd = ops.mark_weight(W.to(dev)), bias.to(dev), gamma.to(dev), beta.to(dev)
    eps = 1e-6
    tag = f"{case_id(case)} {route}"
    # 16-bit A: the normalised value is rounded into the kernel's image of A
    pre = nc.pre_gn_in(x, W, gamma, beta, G, HW, eps, dt, bias=bias)
    parts = partials(ops, dev, x, x, G)
    for name, part in parts.items():
        check_gemm(f"gemm_gn_in partial={name} {tag}", ops.gemm_gn_in(x.to(dev), Wd, part, gd, btd, HW, eps, bias=bd_, want32=True), pre, dt)
    # fp32 A that IS the 16-bit tensor (so the statistics kernel's partials are its own), normalised in fp32 and split hi / lo
    pre32 = nc.pre_gn_in(x, W, gamma, beta, G, HW, eps, dt, bias=bias, a32=True)
    for name, part in parts.items():
        check_gemm(f"gemm_gn_in_a32 partial={name} {tag}",
                   ops.gemm_gn_in_a32(x.float().to(dev), Wd, part, gd, btd, HW, eps, bias=bd_, want32=True), pre32, dt)
    # a true fp32 A with exact partials
    x32 = problem(case, dt, True)[0]
    pre32 = nc.pre_gn_in(x32, W, gamma, beta, G, HW, eps, dt, bias=bias, a32=True)
    hand = partials(ops, dev, None, x32, G)["hand"]
    check_gemm(f"gemm_gn_in_a32 fp32 A partial=hand {tag}",
               ops.gemm_gn_in_a32(x32.to(dev), Wd, hand, gd, btd, HW, eps, bias=bd_, want32=True), pre32, dt)


# =========================================================================================== route 4: the producing conv
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("shape", [
    (2, 64, 64, 320, 320),        # epilogue statistics, 64-row chunks
    (2, 32, 32, 640, 640),        # split-K: statistics from the reduce
    (2, 16, 16, 1280, 1280),      # 512 rows: 16-row chunks
], ids=lambda s: "x".join(map(str, s)))
def test_conv_producer_on_a_shifted_output(ops, dev, shape, dt):
    """the conv's bias is 16 x the output's sigma (sign alternating over the groups, group 1 at 0): the tensor whose statistics the
    epilogue takes is itself shifted. x ~ N(0, 1) and w ~ N(0, 1 / (9 Cin)) make the output's sigma 1."""
    B, H, Wd_, Cin, Cout = shape
    G = 32
    gen = torch.Generator(device=dev).manual_seed(H + Cin)
    x = torch.randn(B, H, Wd_, Cin, generator=gen, device=dev).to(dt)
    w = (torch.randn(Cout, 3, 3, Cin, generator=gen, device=dev) * (1.0 / (3 * Cin ** 0.5))).to(dt)
    sign = torch.tensor([0.0 if k == 1 else (1.0 if k % 2 == 0 else -1.0) for k in range(G)])
    bias = (16.0 * sign).repeat_interleave(Cout // G).to(dt).to(dev)
    out, part = ops.conv2d(x, w, bias=bias, stride=1, pad=1, gn_groups=G)
    assert torch.equal(out, ops.conv2d(x, w, bias=bias, stride=1, pad=1)), "the statistics-producing conv must write the same output"
    HW = H * Wd_
    cr = HW // part.nchunk
    assert cr in (16, 64) and part.nchunk * cr == HW and tuple(part.t.shape) == (B, part.nchunk, G, 2)
    o = out.cpu().reshape(B, HW, Cout)
    # partials against fp64 sums of the 16-bit output, PER CHUNK: an fp32 sum of n_k = cr C / G values in any order
    v = o.double().reshape(B, part.nchunk, cr, G, Cout // G)
    v2 = v * v
    S, Q, Q4 = v.sum((2, 4)), v2.sum((2, 4)), (v2 * v2).sum((2, 4))
    c = gc.acc_c(cr * Cout // G)
    got = part.t.double().cpu()
    rs = float(((got[..., 0] - S).abs() / (c * Q.sqrt())).max())
    rq = float(((got[..., 1] - Q).abs() / (c * Q4.sqrt() + 4 * nc.E32 * Q)).max())
    print(f"[norm_checks] conv partials {shape} {DT_ID[dt]} chunk rows {cr}: worst |dS| / (c sqrt(Q)) = {rs:.3f}, "
          f"worst |dQ| / (c sqrt(sum x^4) + 4 e Q) = {rq:.3f}")
    assert rs <= 1.0 and rq <= 1.0, (rs, rq)
    gen_c = torch.Generator().manual_seed(Cout)
    gamma, beta = (1 + 0.1 * torch.randn(Cout, generator=gen_c)).to(dt), (0.1 * torch.randn(Cout, generator=gen_c)).to(dt)
    g = nc.gn64(o, gamma, beta, G, EPS)
    assert float(g.mean.abs().max() / g.var.sqrt().min()) > 12, "the output is not shifted: the case does not test what it says"
    for silu in (False, True):
        y = ops.groupnorm(out, gamma.to(dev), beta.to(dev), G, EPS, silu, partial=part)
        nc.check(f"groupnorm on conv partials {shape} silu={int(silu)}", y, nc.norm_ref(g, "onepass", dt, "16", silu), dt, fp32_out=False)


# =========================================================================================== route 5: LayerNorm
LN_SHAPES = [(5, 8), (3, 520), (6, 2048), (3, 2056), (2, 8192)]      # the two ends of layernorm_wave_kernel and of layernorm_kernel


def ln_input(gen, rows, C, sigma, r):
    """randn * sigma + mean_row, mean_row / sigma = +-r alternating over the rows, row 1 at 0"""
    sign = torch.tensor([0.0 if m == 1 else (1.0 if m % 2 == 0 else -1.0) for m in range(rows)])
    return torch.randn(rows, C, generator=gen) * sigma + (sign * r * sigma)[:, None]


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("r", [0, 4, 16, 64, 256])
@pytest.mark.parametrize("rows,C", LN_SHAPES)
def test_layernorm_and_row_split_are_two_pass(ops, dev, rows, C, r, dt):
    """both LayerNorm kernels and row_split_kernel take the variance about the mean: they hold the `centered` bound whatever the mean
    is (a later one-pass "optimisation" would not)"""
    gen = torch.Generator().manual_seed(rows * 1000 + C + r)
    sigma = 2.0 if C == 520 else 1.0
    x32 = ln_input(gen, rows, C, sigma, r)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=gen)).to(dt), (0.1 * torch.randn(C, generator=gen)).to(dt)
    gd, bd = gamma.to(dev), beta.to(dev)
    tag = f"rows={rows} C={C} r={r}"
    if r <= 64:                                # 16-bit inputs go to 64, as for GroupNorm
        x = x32.to(dt)
        g = nc.ln64(x, gamma, beta, EPS)
        nc.check(f"layernorm {tag}", ops.layernorm(x.to(dev), gd, bd, EPS), nc.norm_ref(g, "centered", dt, "16"), dt, fp32_out=False)
    g = nc.ln64(x32, gamma, beta, EPS)
    y = ops.row_split(x32.to(dev), dt, gd, bd, EPS).cpu()
    nc.check(f"row_split LN {tag}", y[:, :C].double() + y[:, C:].double(), nc.norm_ref(g, "centered", dt, "split"), dt, fp32_out=True)


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("r", [0, 4, 16, 64])
@pytest.mark.parametrize("M,N,K", [(64, 320, 320), (40, 640, 1280)])
def test_gemm_ln_on_shifted_rows(ops, dev, M, N, K, r, dt):
    """the folded LayerNorm is one-pass by construction; gemm_checks.pre_ln models that, mean included"""
    gen = torch.Generator().manual_seed(M + N + K + r)
    A = ln_input(gen, M, K, 1.0, r).to(dt)
    W = (torch.randn(N, K, generator=gen) * K ** -0.5).to(dt)
    gamma, beta = (1 + 0.1 * torch.randn(K, generator=gen)).to(dt), (0.1 * torch.randn(K, generator=gen)).to(dt)
    bias = (0.1 * torch.randn(N, generator=gen)).to(dt)
    Wf, cs, cb = ops.fold_layernorm(W.to(dev), gamma.to(dev), beta.to(dev), bias.to(dev))
    out = ops.gemm_ln(A.to(dev), Wf, cs, cb, eps=EPS)
    pre = gc.pre_ln(A, Wf.cpu(), cs.cpu(), cb.cpu(), EPS)
    gc.check(f"gemm_ln M={M} N={N} K={K} r={r}", out, gc.finish(pre, dt), dt, fp32_out=False)

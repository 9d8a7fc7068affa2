"""The tile-major weight route (ops.mark_weight -> w_tiled = 1, csrc/gemm.hip: w_row_byte / w_tile_step / TapWalk::wtile) of the 16-bit
GEMM / conv entry points, in f16 and bf16.

Two checks, both sharp:
* ROUTE EQUALITY. launch() in gemm.hip looks at w_tiled only for == 2, so the same call with a marked and an unmarked weight takes the
  same kernel, tile, split-K and K order: same products, same summation order. The outputs must agree BIT FOR BIT; any difference is an
  addressing bug of the tiled route (or of ops.tile_weight64).
* ABSOLUTE PARITY against fp64 within the derived bound of tests/gemm_checks.py (fp32 outputs wherever the entry point has them,
  the 16-bit output tied to them by `out16 == out32.to(dtype)`), every element, no outlier allowance.

Operands are randn (zero mean: the bound needs it), weights scaled by K^-0.5, drawn from seeded CPU generators. The kernel named
beside a shape is the dispatcher's own line for it (SPIDER_GEMM_TRACE=1, recorded in NOTEBOOK.md); the tests do not read that variable.
3 x 3 stride-1 convs are kept off the streaming kernel (w_tiled = 2, tested elsewhere) by WS_ENABLE = False.
"""
import pytest
import torch

import gemm_checks as gc

pytestmark = pytest.mark.gpu

DTS = [torch.float16, torch.bfloat16]
DT_ID = {torch.float16: "f16", torch.bfloat16: "bf16"}


def rnd(g, *shape, scale=1.0, dt=torch.float16):
    return (torch.randn(*shape, generator=g) * scale).to(dt)


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    mp = pytest.MonkeyPatch()
    mp.setattr(o, "WS_ENABLE", False)
    yield o
    mp.undo()


def tup(x):
    return x if isinstance(x, tuple) else (x,)


def assert_tiled_route(wm):
    assert getattr(wm, "_spider_tiled", None) is not None, "the marked weight's tile-major copy was not built: wrong route"
    assert not hasattr(wm, "_spider_fm"), "the streaming kernel's copy was built: wrong route"


def assert_routes_equal(outs):
    """outs: {form: (outputs with the unmarked weight, outputs with the marked weight)}"""
    for form, (plain, tiled) in outs.items():
        assert len(plain) == len(tiled)
        for i, (a, b) in enumerate(zip(plain, tiled)):
            assert a.dtype == b.dtype and a.shape == b.shape
            n = int((a != b).sum())
            assert torch.equal(a, b), f"{form}[{i}]: {n} / {a.numel()} elements differ between the row-major and the tile-major route"


def check_pair(what, out, R, dt):
    """(C, C32) of a want32 call: the fp32 copy within tol32, the 16-bit output its rounding"""
    c16, c32 = out
    gc.check(what, c32, R, dt, fp32_out=True)
    assert torch.equal(c16, c32.to(dt)), f"{what}: the 16-bit output is not the rounded fp32 copy"


# =========================================================================================== 3a / 3c  gemm, M <= 512
GEMM_SHAPES = [
    (1, 1280, 320),       # single row                                             reg(64x64) splits=1
    (77, 320, 768),       # text-projection rows                                   reg(64x64) splits=1
    (200, 36, 72),        # ragged M, N < 64, K tail of 8                          reg(64x64) splits=1
    (130, 132, 1032),     # ragged N and K across tile borders                     reg(64x64) splits=1
    (64, 64, 8192),       # 64^2 tiles with split-K (t64 < 256 && nk >= 64)        reg(64x64) splits=16
    (512, 768, 2816),     # 128^2 tiles with split-K (nk >= 44 && t128 >= 24)      reg(128x128) splits=5
    (512, 320, 4096),     # LDS-DMA kernel reached at 512 rows by a long K         dma(128x160) splits=8
    (512, 10240, 320),    # 256 x 128 kernel reached at 512 rows                   p8h(256x128) splits=1
]
ACTS = ["silu", "gelu", "quick_gelu"]


@pytest.fixture(scope="module", params=[(s, dt) for s in GEMM_SHAPES for dt in DTS],
                ids=lambda p: "x".join(map(str, p[0])) + "-" + DT_ID[p[1]])
def gemm_case(request, ops, dev):
    (M, N, K), dt = request.param
    g = torch.Generator().manual_seed(1000 + M + N + K)
    rpg = max(1, (M + 3) // 4)
    t = dict(A=rnd(g, M, K, dt=dt), W=rnd(g, N, K, scale=K ** -0.5, dt=dt), bias=rnd(g, N, dt=dt), res=rnd(g, M, N, dt=dt),
             rowbias=rnd(g, (M + rpg - 1) // rpg, N, dt=dt), res32=torch.randn(M, N, generator=g))
    d = {k: v.to(dev) for k, v in t.items()}
    wm = ops.mark_weight(d["W"].clone())

    def forms(W):
        A = d["A"]
        o = {"plain": ops.gemm(A, W), "out_f32": ops.gemm(A, W, out_f32=True),
             "bias_res_scale": ops.gemm(A, W, bias=d["bias"], res=d["res"], out_scale=0.5),
             "rowbias": ops.gemm(A, W, rowbias=d["rowbias"], rows_per_group=rpg, want32=True),
             "res32": ops.gemm(A, W, bias=d["bias"], res32=d["res32"], want32=True)}
        for act in ACTS:
            o[act] = ops.gemm(A, W, bias=d["bias"], act=act, want32=True)
        return {k: tup(v) for k, v in o.items()}

    plain, tiled = forms(d["W"]), forms(wm)
    torch.cuda.synchronize()
    assert_tiled_route(wm)
    return dict(dt=dt, rpg=rpg, t=t, outs={k: (plain[k], tiled[k]) for k in plain})


def test_gemm_routes_agree_bit_for_bit(gemm_case):
    assert_routes_equal(gemm_case["outs"])


def test_gemm_tiled_route_within_derived_bound(gemm_case):
    c, dt, t = gemm_case, gemm_case["dt"], gemm_case["t"]
    out = {k: v[1] for k, v in c["outs"].items()}
    base = gc.matmul64(t["A"], t["W"])
    bare, biased = gc.pre_gemm(base), gc.pre_gemm(base, bias=t["bias"])
    gc.check("gemm plain", out["plain"][0], gc.finish(bare, dt), dt, fp32_out=False)
    gc.check("gemm out_f32", out["out_f32"][0], gc.finish(bare, dt), dt, fp32_out=True)
    gc.check("gemm bias+res+scale", out["bias_res_scale"][0], gc.finish(biased, dt, res=t["res"], out_scale=0.5), dt, fp32_out=False)
    check_pair("gemm rowbias", out["rowbias"], gc.finish(gc.pre_gemm(base, rowbias=t["rowbias"], rows_per_group=c["rpg"]), dt), dt)
    check_pair("gemm res32+want32", out["res32"], gc.finish(biased, dt, res32=t["res32"]), dt)
    for act in ACTS:
        check_pair(f"gemm {act}", out[act], gc.finish(biased, dt, act=act), dt)


# =========================================================================================== fused GLU epilogues (row remap into W)
GLU_SHAPES = [
    (100, 72, 64),        # inner < 64: value and gate rows inside one W tile      reg(64x64)
    (128, 5120, 1280),    # SD-1.5 8^2 ff1                                         reg(64x64)
    (512, 132, 1032),     # ragged inner and K: the gate rows start mid-tile       reg(64x64)
]
GLU = ["geglu", "swiglu", "geglu_exact"]


@pytest.fixture(scope="module", params=[(s, dt) for s in GLU_SHAPES for dt in DTS],
                ids=lambda p: "x".join(map(str, p[0])) + "-" + DT_ID[p[1]])
def glu_case(request, ops, dev):
    (M, inner, K), dt = request.param
    g = torch.Generator().manual_seed(2000 + M + inner + K)
    t = dict(A=rnd(g, M, K, dt=dt), W=rnd(g, 2 * inner, K, scale=K ** -0.5, dt=dt), bias=rnd(g, 2 * inner, dt=dt))
    d = {k: v.to(dev) for k, v in t.items()}
    wm = ops.mark_weight(d["W"].clone())
    forms = lambda W: {act: tup(ops.gemm(d["A"], W, bias=d["bias"], act=act)) for act in GLU}
    plain, tiled = forms(d["W"]), forms(wm)
    torch.cuda.synchronize()
    assert_tiled_route(wm)
    assert tuple(tiled["geglu"][0].shape) == (M, inner)
    return dict(dt=dt, t=t, outs={k: (plain[k], tiled[k]) for k in plain})


def test_glu_routes_agree_bit_for_bit(glu_case):
    assert_routes_equal(glu_case["outs"])


def test_glu_tiled_route_within_derived_bound(glu_case):
    dt, t = glu_case["dt"], glu_case["t"]
    pre = gc.pre_gemm(gc.matmul64(t["A"], t["W"]), bias=t["bias"])
    for act in GLU:
        gc.check(f"gemm {act}", glu_case["outs"][act][1][0], gc.finish_glu(pre, dt, act), dt, fp32_out=False)


# =========================================================================================== gemm_ln
LN_SHAPES = [
    (77, 72, 64),         # one K tile, N tail                                     reg(64x64)
    (512, 2560, 320),     # SD-1.5 16^2 ff1 (GEGLU form) / qkv widths              reg(64x64)
    (130, 1288, 328),     # ragged M, N, K                                         reg(64x64)
]
LN_EPS = 1e-5


@pytest.fixture(scope="module", params=[(s, dt) for s in LN_SHAPES for dt in DTS],
                ids=lambda p: "x".join(map(str, p[0])) + "-" + DT_ID[p[1]])
def ln_case(request, ops, dev):
    (M, N, K), dt = request.param
    g = torch.Generator().manual_seed(3000 + M + N + K)
    A, W, bias = rnd(g, M, K, dt=dt), rnd(g, N, K, scale=K ** -0.5, dt=dt), rnd(g, N, scale=0.2, dt=dt)
    gamma, beta = (1 + 0.2 * torch.randn(K, generator=g)).to(dt), rnd(g, K, scale=0.2, dt=dt)
    res = rnd(g, M, N, dt=dt)
    Wf, cs, cb = ops.fold_layernorm(W, gamma, beta, bias)            # host tensors: the fold is plain torch arithmetic
    t = dict(A=A, Wf=Wf, cs=cs, cb=cb, res=res)
    d = {k: v.to(dev) for k, v in t.items()}
    wm = ops.mark_weight(d["Wf"].clone())

    def forms(Wd):
        return {"plain": tup(ops.gemm_ln(d["A"], Wd, d["cs"], d["cb"], eps=LN_EPS)),
                "res": tup(ops.gemm_ln(d["A"], Wd, d["cs"], d["cb"], res=d["res"], eps=LN_EPS)),
                "geglu": tup(ops.gemm_ln(d["A"], Wd, d["cs"], d["cb"], act="geglu", eps=LN_EPS))}

    plain, tiled = forms(d["Wf"]), forms(wm)
    torch.cuda.synchronize()
    assert_tiled_route(wm)
    return dict(dt=dt, t=t, outs={k: (plain[k], tiled[k]) for k in plain})


def test_gemm_ln_routes_agree_bit_for_bit(ln_case):
    assert_routes_equal(ln_case["outs"])


def test_gemm_ln_tiled_route_within_derived_bound(ln_case):
    dt, t = ln_case["dt"], ln_case["t"]
    out = {k: v[1][0] for k, v in ln_case["outs"].items()}
    pre = gc.pre_ln(t["A"], t["Wf"], t["cs"], t["cb"], LN_EPS)
    gc.check("gemm_ln plain", out["plain"], gc.finish(pre, dt), dt, fp32_out=False)
    gc.check("gemm_ln res", out["res"], gc.finish(pre, dt, res=t["res"]), dt, fp32_out=False)
    gc.check("gemm_ln geglu", out["geglu"], gc.finish_glu(pre, dt, "geglu"), dt, fp32_out=False)


# =========================================================================================== gemm_gn_in
@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("B,HW,C,N", [(2, 64, 1280, 1280),       # SD-1.5 8^2 proj_in                   reg(64x64)
                                      (2, 256, 320, 320)])       # 16^2 map, 5 K tiles                   reg(64x64)
def test_gemm_gn_in_routes_agree_and_match_fp64(ops, dev, B, HW, C, N, dt):
    g = torch.Generator().manual_seed(4000 + HW + C)
    x, W, bias = rnd(g, B, HW, C, dt=dt), rnd(g, N, C, scale=C ** -0.5, dt=dt), rnd(g, N, scale=0.1, dt=dt)
    gam, bet = (1 + 0.1 * torch.randn(C, generator=g)).to(dt), rnd(g, C, scale=0.1, dt=dt)
    xd, Wd, bd, gd, btd = (v.to(dev) for v in (x, W, bias, gam, bet))
    wm = ops.mark_weight(Wd.clone())
    part = ops.groupnorm_stats(xd, 32, HW // 16)
    plain = ops.gemm_gn_in(xd, Wd, part, gd, btd, HW, 1e-6, bias=bd, want32=True)
    tiled = ops.gemm_gn_in(xd, wm, part, gd, btd, HW, 1e-6, bias=bd, want32=True)
    assert_tiled_route(wm)
    assert_routes_equal({"gemm_gn_in": (plain, tiled)})
    R = gc.ref64("gemm_gn_in", x, W, gam, bet, groups=32, HW=HW, eps=1e-6, bias=bias, dt=dt)
    R.ref, R.tol32 = R.ref.reshape(B, HW, N), R.tol32.reshape(B, HW, N)
    check_pair("gemm_gn_in", tiled, R, dt)


# =========================================================================================== convs, <= 512 output pixels
#  id, entry point, B, H, W, Cin, Cout, kh, kw, stride, pad, dil, up_size, act, act_param
CONVS = [
    ("1x1", "conv2d", 2, 16, 16, 192, 64, 1, 1, 1, (0, 0), 1, None, None, 0.0),            # reg(64x64)
    ("3x3", "conv2d", 2, 16, 16, 320, 320, 3, 3, 1, (1, 1), 1, None, None, 0.0),           # 512 rows, nk = 45: dma(128x160) splits=5, kcm + hbits
    ("3x3s2", "conv2d", 2, 32, 32, 64, 128, 3, 3, 2, (1, 1), 1, None, None, 0.0),          # reg(64x64), kcm
    ("3x3ups", "conv2d", 2, 8, 8, 128, 128, 3, 3, 1, (1, 1), 1, (16, 16), None, 0.0),      # fused 2x upsample (no hbits)
    ("up15x9", "conv_ex", 2, 8, 5, 128, 64, 3, 3, 1, (1, 1), 1, (15, 9), None, 0.0),       # upsample to 2 n - 1
    ("k11dil5", "conv1d", 1, 1, 257, 32, 32, 1, 11, 1, (0, 25), 5, None, None, 0.0),       # Cin % 64 != 0: per-lane taps
    ("k3dil3", "conv1d", 1, 1, 100, 8, 16, 1, 3, 1, (0, 3), 3, None, None, 0.0),           # Cin = 8: K = 24, one ragged K tile
    ("cin72", "conv_ex", 2, 9, 7, 72, 68, 3, 3, 1, (1, 1), 1, None, None, 0.0),            # taps straddle K tiles, ragged N
    ("3x1", "conv_ex", 2, 6, 35, 64, 64, 3, 1, 1, (1, 0), 1, None, None, 0.0),             # (3, 1) temporal kernel
    ("leaky", "conv1d", 1, 1, 90, 32, 32, 1, 3, 1, (0, 1), 1, None, "leaky_relu", 0.1),
    ("tanh", "conv1d", 1, 1, 90, 32, 32, 1, 3, 1, (0, 1), 1, None, "tanh", 0.0),
]


def conv_forms(ops, entry, d, w, stride, pad, dil, up, act, act_param):
    """form "16": bias + rowbias + 16-bit res through the case's own entry point (conv1d has no rowbias);
    form "32": bias + rowbias + res32 + want32 (conv2d, or conv_ex for the cases conv2d cannot express)"""
    x = d["x"]
    if entry == "conv2d":
        kw = dict(bias=d["bias"], rowbias=d["rowbias"], stride=stride, ups=up is not None)
        return {"16": tup(ops.conv2d(x, w, res=d["res"], **kw)), "32": ops.conv2d(x, w, res32=d["res32"], want32=True, **kw)}
    kw = dict(bias=d["bias"], stride=stride, pad=pad, dil=dil, up_size=up, act=act, act_param=act_param)
    o32 = ops.conv_ex(x, w, rowbias=d["rowbias"], res32=d["res32"], want32=True, **kw)
    if entry == "conv_ex":
        return {"16": tup(ops.conv_ex(x, w, rowbias=d["rowbias"], res=d["res"], **kw)), "32": o32}
    B, _, L, Cin = x.shape
    y = ops.conv1d(x.view(B, L, Cin), w.view(w.shape[0], w.shape[2], Cin), bias=d["bias"], res=d["res"].view(B, -1, w.shape[0]),
                   pad=pad[1], dil=dil, act=act, act_param=act_param)
    return {"16": (y.view(B, 1, y.shape[1], y.shape[2]),), "32": o32}


@pytest.fixture(scope="module", params=[(c, dt) for c in CONVS for dt in DTS], ids=lambda p: p[0][0] + "-" + DT_ID[p[1]])
def conv_case(request, ops, dev):
    (name, entry, B, H, W, Cin, Cout, kh, kw, stride, pad, dil, up, act, act_param), dt = request.param
    g = torch.Generator().manual_seed(5000 + sum(map(ord, name)))
    Hs, Ws = up if up is not None else (H, W)
    Ho = (Hs + 2 * pad[0] - dil * (kh - 1) - 1) // stride + 1
    Wo = (Ws + 2 * pad[1] - dil * (kw - 1) - 1) // stride + 1
    assert B * Ho * Wo <= 512
    t = dict(x=rnd(g, B, H, W, Cin, dt=dt), w=rnd(g, Cout, kh, kw, Cin, scale=(kh * kw * Cin) ** -0.5, dt=dt), bias=rnd(g, Cout, dt=dt),
             rowbias=rnd(g, B, Cout, dt=dt), res=rnd(g, B, Ho, Wo, Cout, dt=dt), res32=torch.randn(B, Ho, Wo, Cout, generator=g))
    d = {k: v.to(dev) for k, v in t.items()}
    wm = ops.mark_weight(d["w"].clone())
    geo = dict(stride=stride, pad=pad, dil=dil, up=up, act=act, act_param=act_param)
    plain, tiled = conv_forms(ops, entry, d, d["w"], **geo), conv_forms(ops, entry, d, wm, **geo)
    torch.cuda.synchronize()
    assert_tiled_route(wm)
    assert tuple(tiled["16"][0].shape) == (B, Ho, Wo, Cout)
    return dict(dt=dt, t=t, entry=entry, geo=geo, outs={k: (plain[k], tiled[k]) for k in plain})


def test_conv_routes_agree_bit_for_bit(conv_case):
    assert_routes_equal(conv_case["outs"])


def test_conv_tiled_route_within_derived_bound(conv_case):
    c, dt, t, geo = conv_case, conv_case["dt"], conv_case["t"], conv_case["geo"]
    base, (B, Ho, Wo) = gc.conv_base(t["x"], t["w"], geo["stride"], geo["pad"], geo["dil"], geo["up"])
    shape = (B, Ho, Wo, t["w"].shape[0])

    def ref(rowbias, **kw):
        pre = gc.pre_gemm(base, bias=t["bias"], rowbias=rowbias, rows_per_group=Ho * Wo)
        R = gc.finish(pre, dt, act=geo["act"], act_param=geo["act_param"], **kw)
        R.ref, R.tol32 = R.ref.reshape(shape), R.tol32.reshape(shape)
        return R

    rb16 = None if c["entry"] == "conv1d" else t["rowbias"]
    gc.check(f"{c['entry']} 16-bit res", c["outs"]["16"][1][0], ref(rb16, res=t["res"].reshape(-1, shape[3])), dt, fp32_out=False)
    entry32 = "conv2d" if c["entry"] == "conv2d" else "conv_ex"
    check_pair(f"{entry32} res32+want32", c["outs"]["32"][1], ref(t["rowbias"], res32=t["res32"].reshape(-1, shape[3])), dt)


# =========================================================================================== 3b  route equality on the large-M kernels
def dev_rnd(g, *shape, scale=1.0, dt=torch.float16):
    return (torch.randn(*shape, generator=g, device=g.device) * scale).to(dt)


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("M,N,K", [
    (4096, 320, 2560),      # dma(64x160) splits=2
    (2340, 312, 2568),      # dma(64x160) splits=3, ragged M / N / K   ((2100, 312, 2568) runs reg(64x64): 264 blocks miss the DMA rule)
    (4608, 3840, 1280),     # p8h(256x128) splits=1
    (1536, 3328, 3584),     # p8(256x256) splits=3                      ((1536, 3584, 3584) runs p8h(256x128), no split-K)
    (4000, 2500, 1096),     # p8(256x256) splits=1, ragged M / N / K
    (16384, 320, 320),      # cost-model dispatch: dma(128x160) splits=1
])
def test_large_gemm_routes_agree_bit_for_bit(ops, dev, monkeypatch, M, N, K, dt):
    """rows above WTILED_MAX_M take the row-major route in the engines; the knob's module mirror sends them down the tiled one, so
    the LDS-DMA / 256^2 / 256 x 128 kernels' reads through w_row_byte are compared at the sizes those kernels were built for"""
    monkeypatch.setattr(ops, "WTILED_MAX_M", 1 << 30)
    g = torch.Generator(device=dev).manual_seed(6000 + M + N + K)
    A, W = dev_rnd(g, M, K, dt=dt), dev_rnd(g, N, K, scale=K ** -0.5, dt=dt)
    bias, res32 = dev_rnd(g, N, dt=dt), torch.randn(M, N, generator=g, device=dev)
    wm = ops.mark_weight(W.clone())
    forms = lambda Wd: {"plain": tup(ops.gemm(A, Wd)), "silu": tup(ops.gemm(A, Wd, bias=bias, act="silu")),
                        "res32": ops.gemm(A, Wd, bias=bias, res32=res32, want32=True)}
    plain, tiled = forms(W), forms(wm)
    assert_tiled_route(wm)
    assert_routes_equal({k: (plain[k], tiled[k]) for k in plain})


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [
    (8, 48, 48, 64, 640, 1),        # p8(256x256) splits=1, halo taps
    (8, 47, 49, 128, 632, 1),       # p8(256x256) splits=1, ragged rows / columns
    (2, 64, 64, 320, 320, 2),       # dma(64x160) splits=4: stride 2 on the LDS-DMA kernel (M = 2048)
])
def test_large_conv_routes_agree_bit_for_bit(ops, dev, monkeypatch, B, H, W, Cin, Cout, stride, dt):
    monkeypatch.setattr(ops, "WTILED_MAX_M", 1 << 30)
    g = torch.Generator(device=dev).manual_seed(7000 + H + W + Cin)
    x, w = dev_rnd(g, B, H, W, Cin, dt=dt), dev_rnd(g, Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, dt=dt)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    bias, rb = dev_rnd(g, Cout, dt=dt), dev_rnd(g, B, Cout, dt=dt)
    res, res32 = dev_rnd(g, B, Ho, Wo, Cout, dt=dt), torch.randn(B, Ho, Wo, Cout, generator=g, device=dev)
    wm = ops.mark_weight(w.clone())
    forms = lambda wd: {"16": tup(ops.conv2d(x, wd, bias=bias, rowbias=rb, res=res, stride=stride)),
                        "32": ops.conv2d(x, wd, bias=bias, rowbias=rb, res32=res32, want32=True, stride=stride)}
    plain, tiled = forms(w), forms(wm)
    assert_tiled_route(wm)
    assert_routes_equal({k: (plain[k], tiled[k]) for k in plain})


# =========================================================================================== 3c  f16 on the large kernels against fp64
def sample_rows(M):
    """rows 0::8 plus the last 32: every 64- / 128- / 256-row tile and the M tail, at an eighth of the fp64 work"""
    return torch.unique(torch.cat([torch.arange(0, M, 8), torch.arange(M - 32, M)]))


@pytest.mark.parametrize("M,N,K", [
    (2048, 320, 2560),      # dma(64x160) splits=4
    (2048, 2560, 320),      # p8h(256x128) splits=1
    (4096, 4096, 512),      # p8(256x256) splits=1
])
def test_large_gemm_f16_within_derived_bound(ops, dev, monkeypatch, M, N, K):
    dt = torch.float16
    g = torch.Generator().manual_seed(8000 + M + N + K)
    A, W, bias = rnd(g, M, K, dt=dt), rnd(g, N, K, scale=K ** -0.5, dt=dt), rnd(g, N, dt=dt)
    res32 = torch.randn(M, N, generator=g)
    Ad, Wd, bd, rd = (v.to(dev) for v in (A, W, bias, res32))
    out = ops.gemm(Ad, Wd, bias=bd, res32=rd, want32=True)                   # the route the engines take at these sizes
    monkeypatch.setattr(ops, "WTILED_MAX_M", 1 << 30)
    wm = ops.mark_weight(Wd.clone())
    tiled = ops.gemm(Ad, wm, bias=bd, res32=rd, want32=True)
    assert_tiled_route(wm)
    assert_routes_equal({"res32": (out, tiled)})
    rows = sample_rows(M)
    R = gc.finish(gc.pre_gemm(gc.matmul64(A[rows], W), bias=bias), dt, res32=res32[rows])
    gc.check("large gemm res32+want32", out[1][rows.to(dev)], R, dt, fp32_out=True)
    assert torch.equal(out[0], out[1].to(dt))


def test_large_conv_f16_within_derived_bound(ops, dev, monkeypatch):
    dt = torch.float16
    B, H, W, Cin, Cout = 2, 32, 32, 320, 320                                 # 2048 rows, nk = 45: dma(64x160) splits=4
    g = torch.Generator().manual_seed(8100)
    x, w = rnd(g, B, H, W, Cin, dt=dt), rnd(g, Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5, dt=dt)
    bias, rb, res32 = rnd(g, Cout, dt=dt), rnd(g, B, Cout, dt=dt), torch.randn(B, H, W, Cout, generator=g)
    xd, wd, bd, rbd, rd = (v.to(dev) for v in (x, w, bias, rb, res32))
    out = ops.conv2d(xd, wd, bias=bd, rowbias=rbd, res32=rd, want32=True)
    monkeypatch.setattr(ops, "WTILED_MAX_M", 1 << 30)
    wm = ops.mark_weight(wd.clone())
    tiled = ops.conv2d(xd, wm, bias=bd, rowbias=rbd, res32=rd, want32=True)
    assert_tiled_route(wm)
    assert_routes_equal({"res32": (out, tiled)})
    rows = sample_rows(B * H * W)
    base, _ = gc.conv_base(x, w, 1, (1, 1), 1, None, rows=rows)
    pre = gc.pre_gemm(base, bias=bias, rowbias=rb, rows_per_group=H * W, row_ids=rows)
    R = gc.finish(pre, dt, res32=res32.reshape(-1, Cout)[rows])
    gc.check("large conv2d res32+want32", out[1].reshape(-1, Cout)[rows.to(dev)], R, dt, fp32_out=True)
    assert torch.equal(out[0], out[1].to(dt))


# =========================================================================================== 3d  eager vs captured
def test_tiled_gemm_graph_replay_is_bit_identical(ops, dev):
    dt = torch.float16
    g = torch.Generator(device=dev).manual_seed(9)
    A, W = dev_rnd(g, 77, 768, dt=dt), ops.mark_weight(dev_rnd(g, 320, 768, scale=768 ** -0.5, dt=dt))
    assert ops.prebuild_tiled([W]) == 5 * 12 * 8192
    copy = W._spider_tiled
    eager = ops.gemm(A, W)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out = ops.gemm(A, W)
    assert W._spider_tiled is copy, "the capture must use the prebuilt copy"
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert torch.equal(eager, ops.gemm(A, W.clone()))                        # and both equal the row-major route

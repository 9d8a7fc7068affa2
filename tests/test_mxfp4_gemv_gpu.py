"""GPU: the weight-only MXFP4 decode GEMVs (ops.gemv_w4 / ops.gemv_swiglu_w4, csrc/gemv_wq.hip) against an fp64 restatement on
W_eff[n, k] = e2m1(code) * 2^(scales[n, k / 32] - 127) that rounds where the kernel rounds.

The bound is the derived one of tests/test_fp8_gemv_gpu.py, restated for this format. With u = 2^-24 the unit roundoff of fp32:

  * a dequantised weight is a bf16 number (two significand bits times a power of two, applied inside the conversion), and every
    product x[k] * W_eff[n, k] is exact in fp32 (8 x 2 significand bits), so the fp32 dot product differs from the exact one only by
    its K - 1 additions; in ANY order that is at most (K - 1) u / (1 - (K - 1) u) * sum_k |x[k] W_eff[n, k]|. The test allows
    E = 2 K u * sum_k |x[k] W_eff[n, k]| (the factor 2 covers the two-term adder inside v_dot2c_f32_bf16).
  * a value the kernel rounds to bf16 (after the bias, after the residual, the three SwiGLU roundings) may land on the other side
    of a rounding boundary than the fp64 value whenever the two differ at all: the rounded values then differ by one bf16 ulp,
    <= 2^-7 |ref|. Every such rounding adds 2^-7 |ref| to the error carried so far; fp32 additions add u |ref|.
  * SwiGLU: |silu'| <= 1.1, and silu_f = x * rcp(1 + __expf(-x)) is within 2^-16 relative of silu.
  * fused RMSNorm: the test reads the kernel's OWN normalised activations through an identity weight matrix (one non-zero exact
    product per output: out = xin bit for bit), checks them against the fp64 RMSNorm within the two bf16 roundings that form has,
    and feeds them to the restatement. Every block recomputes the norm in the same order, so they are the values every launch of
    that (rows, K) uses: the waves per block, and with them the order of the sum, depend on nothing else.

The kernel reads the public scale layout [N, K / 32]; there is no private re-arrangement to pin."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U8 = torch.uint8
U32 = 2.0 ** -24
ULP16 = 2.0 ** -7
EPS = 1e-5
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
LDS_BUDGET = 160 * 1024 - 256


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


def _w_eff(blocks, scales):
    """the format as the C header states it, in fp64 (the test's own decode, on whichever device the bytes live)"""
    N, K = blocks.shape[0], blocks.shape[1] * 2
    table = torch.tensor(GRID + [-v for v in GRID], dtype=torch.float64, device=blocks.device)
    codes = torch.stack([blocks & 15, blocks >> 4], dim=2).reshape(N, K)
    sc = torch.ldexp(torch.ones(N, K // 32, dtype=torch.float64, device=blocks.device), scales.to(torch.int32) - 127)
    return table[codes.long()] * sc.repeat_interleave(32, dim=1)


def _case(dev, B, N, K, seed, rows=None):
    """random bytes (all 16 codes in both nibbles), scale bytes 107 .. 135 that differ between neighbouring blocks and rows, the
    last weight row alternating +-6 and +-0.5; x, bias, res, norm_w in bf16"""
    rows = rows or N
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, (rows, K // 2), generator=g, dtype=torch.int32).to(U8)
    if rows > 1 or B % 2 == 0:
        b[-1] = torch.tensor([7 | (15 << 4), 1 | (9 << 4)], dtype=U8).repeat(K // 4)      # +6, -6, +0.5, -0.5
    # steps 5 and 7 are coprime to 29: neighbours differ in both directions, all 29 bytes occur
    sc = (107 + (torch.arange(rows)[:, None] * 5 + torch.arange(K // 32)[None, :] * 7 + seed) % 29).to(U8)
    x = torch.randn(B, K, generator=g).to(BF)
    bias = (torch.randn(N, generator=g) * 4).to(BF)
    res = (torch.randn(B, N, generator=g) * 4).to(BF)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF)
    d = lambda t: t.to(dev)
    return d(b), d(sc), d(x), d(bias), d(res), d(nw)


_EYE = {}


def _kernel_xin(ops, dev, x, nw):
    """the kernel's own normalised activations [B, K] bf16, read through an identity matrix (see the module docstring), checked
    against the fp64 RMSNorm: bf16(bf16(x * rs) * w) with at most one ulp of slack per rounding"""
    K = x.shape[-1]
    if K not in _EYE:
        _EYE.clear()                                         # (the largest probe is K * K / 2 = 171 MiB: keep one at a time)
        eye = torch.zeros(K, K // 2, dtype=U8, device=dev)
        k = torch.arange(K, device=dev)
        eye[k, k // 2] = torch.where(k % 2 == 1, 0x20, 0x02).to(U8)     # code 2 = 1.0 in the nibble of weight k
        _EYE[K] = (eye, torch.full((K, K // 32), 127, dtype=U8, device=dev))
    eye, one = _EYE[K]
    xin = ops.gemv_w4(eye, one, x, norm_w=nw, eps=EPS)
    xd = x.double()
    rs = torch.rsqrt((xd * xd).mean(-1, keepdim=True) + EPS)
    a = (xd * rs).to(BF).double()
    ref = (a * nw.double()).to(BF).double()
    tol = ULP16 * ref.abs() * (1 + ULP16) + ULP16 * ref.abs() + 1e-30
    err = (xin.double() - ref).abs()
    assert bool((err <= tol).all()), f"fused RMSNorm: max err / tol {float((err / tol).max()):.3g}"
    return xin


def _dot(xin, blocks, scales):
    """(exact dot products, the summation bound E) in fp64"""
    xd, wd = xin.double(), _w_eff(blocks, scales)
    return xd @ wd.T, 2 * xin.shape[-1] * U32 * (xd.abs() @ wd.abs().T)


def _round(v, e):
    """a bf16 rounding of a value carried with error e"""
    r = v.to(BF).double()
    return r, e + ULP16 * r.abs()


def _check(got, ref, tol, what):
    err = (got.double() - ref).abs()
    ratio = float((err / tol.clamp_min(1e-300)).max())
    print(f"{what}: max err / derived bound = {ratio:.3g}")
    assert got.dtype == BF and got.shape == ref.shape
    assert bool((err <= tol).all()), f"{what}: max err / bound {ratio:.3g}, {int((err > tol).sum())} / {err.numel()} elements out"
    assert bool(torch.isfinite(got.float()).all())


def _check_gemv(ops, blocks, scales, x, xin, bias, res, norm_w, what):
    got = ops.gemv_w4(blocks, scales, x, bias=bias, res=res, norm_w=norm_w, eps=EPS)
    v, e = _dot(xin, blocks, scales)
    if bias is not None:
        v = v + bias.double()
        e = e + U32 * v.abs()
    if res is not None:
        v, e = _round(v, e)
        v = v + res.double()
        e = e + U32 * v.abs()
    v, e = _round(v, e)
    _check(got, v, e, what)
    return got


def _check_swiglu(ops, blocks, scales, x, xin, norm_w, what):
    I = blocks.shape[0] // 2
    got = ops.gemv_swiglu_w4(blocks, scales, x, norm_w=norm_w, eps=EPS)
    s, E = _dot(xin, blocks, scales)
    g, eg = _round(s[:, :I], E[:, :I])
    u, eu = _round(s[:, I:], E[:, I:])
    a = g * torch.sigmoid(g)
    a, ea = _round(a, 1.1 * eg + 2.0 ** -16 * a.abs())
    v = a * u
    v, e = _round(v, u.abs() * ea + a.abs() * eu + ea * eu + U32 * v.abs())
    _check(got, v, e, what)
    return got


# K: 32 = one MX block, one lane of one wave instruction; 2048 = exactly one wave instruction (64 lanes x 32 weights); 2080 = one
# ragged chunk (a single lane) behind a full one; 3584 = the workload's hidden size, 1.75 wave instructions.
# N: 1 = fewer rows than a block's waves own, 18 and 257 = not a multiple of the columns per block (4 or 8).
@pytest.mark.parametrize("K", [32, 2048, 2080, 3584])
@pytest.mark.parametrize("N", [1, 18, 257])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_gemv_w4(ops, dev, B, N, K):
    blocks, scales, x, bias, res, nw = _case(dev, B, N, K, seed=B + 7 * N + K)
    assert ops.w4_norm_fits(B, K)
    xin = _kernel_xin(ops, dev, x, nw)
    for has_bias in (False, True):
        for has_res in (False, True):
            for has_norm in (False, True):
                _check_gemv(ops, blocks, scales, x, xin if has_norm else x, bias if has_bias else None, res if has_res else None,
                            nw if has_norm else None, f"gemv_w4 B{B} N{N} K{K} bias{int(has_bias)} res{int(has_res)} norm{int(has_norm)}")


@pytest.mark.parametrize("K", [32, 2048, 2080, 3584])
@pytest.mark.parametrize("I", [9, 256])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_gemv_swiglu_w4(ops, dev, B, I, K):
    blocks, scales, x, _, _, nw = _case(dev, B, I, K, seed=3 + B + 7 * I + K, rows=2 * I)
    xin = _kernel_xin(ops, dev, x, nw)
    for has_norm in (False, True):
        _check_swiglu(ops, blocks, scales, x, xin if has_norm else x, nw if has_norm else None, f"gemv_swiglu_w4 B{B} I{I} K{K} norm{int(has_norm)}")


# The long row of the down projection: 8 waves per block (from K = 8192) and 10 chunks of 2048. One row stages 40 KiB; two rows
# 80 KiB, above the 64 KiB a launch gets without opting in; four rows would need 160 KiB, 256 bytes more than the budget, so the
# waves re-read x through L2 and the fused norm is refused.
@pytest.mark.parametrize("B,staged", [(1, True), (2, True), (4, False)])
def test_gemv_w4_long_rows_staged_and_through_l2(ops, dev, B, staged):
    from spider_amd.lib import SpiderHipError
    N, K = 24, 18944
    assert ops.w4_norm_fits(B, K) == (B * ((K + 2047) // 2048) * 4096 <= LDS_BUDGET) == staged
    blocks, scales, x, bias, res, nw = _case(dev, B, N, K, seed=B + N + K)
    _check_gemv(ops, blocks, scales, x, x, None, None, None, f"gemv_w4 B{B} N{N} K{K}")
    _check_gemv(ops, blocks, scales, x, x, bias, res, None, f"gemv_w4 B{B} N{N} K{K} bias res")
    _check_swiglu(ops, blocks, scales, x, x, None, f"gemv_swiglu_w4 B{B} I{N // 2} K{K}")
    if staged:
        xin = _kernel_xin(ops, dev, x, nw)
        _check_gemv(ops, blocks, scales, x, xin, bias, res, nw, f"gemv_w4 B{B} N{N} K{K} bias res norm")
        _check_swiglu(ops, blocks, scales, x, xin, nw, f"gemv_swiglu_w4 B{B} I{N // 2} K{K} norm")
    else:                 # no LDS copy, no fused norm: the entry point says so
        with pytest.raises(SpiderHipError, match="fused RMSNorm"):
            ops.gemv_w4(blocks, scales, x, norm_w=nw, eps=EPS)
        with pytest.raises(SpiderHipError, match="fused RMSNorm"):
            ops.gemv_swiglu_w4(blocks, scales, x, norm_w=nw, eps=EPS)
    _EYE.clear()


def test_gemv_w4_two_columns_per_wave_at_one_row(ops, dev):
    """N * K >= 24 Mi weights at one row: the plain form gives every wave two weight rows"""
    B, N, K = 1, 6144, 4096
    blocks, scales, x, bias, res, nw = _case(dev, B, N, K, seed=B + N + K)
    _check_gemv(ops, blocks, scales, x, x, bias, res, None, f"gemv_w4 B{B} N{N} K{K} bias res")


def test_one_hot_activations_return_w_eff_bit_for_bit(ops, dev):
    """x = 1.0 at one k: out[b, n] = W_eff[n, k_b] exactly, for every code in both nibbles and the scale bytes 2, 64, 127, 190, 252
    (2 and 252: the smallest and the largest the quantiser emits; 0.5 * 2^-125 is the smallest normal bf16 number, 6 * 2^125 is
    finite)"""
    K, SC = 64, [2, 64, 127, 190, 252]
    j = torch.arange(K // 2)
    row = (((j + 3) % 16) | (((20 - j) % 16) << 4)).to(U8)           # low nibbles and high nibbles each run through all 16 codes
    assert sorted((row[:16] & 15).tolist()) == list(range(16)) and sorted((row[:16] >> 4).tolist()) == list(range(16))
    blocks = row[None, :].repeat(len(SC), 1)
    scales = torch.tensor([[SC[n], SC[(n + 2) % len(SC)]] for n in range(len(SC))], dtype=U8)
    w = _w_eff(blocks, scales)                                       # on the host
    assert bool(torch.isfinite(w).all()) and torch.equal(w.float().to(BF).double(), w)
    assert float(w.abs()[w != 0].min()) == 2.0 ** -126 and float(w.abs().max()) == 6 * 2.0 ** 125
    blocks, scales = blocks.to(dev), scales.to(dev)
    for B in (1, 2, 3, 4):
        for k0 in range(0, K, 4):
            ks = [(k0 + b) % K for b in range(B)]
            x = torch.zeros(B, K, dtype=BF, device=dev)
            for b, k in enumerate(ks):
                x[b, k] = 1.0
            got = ops.gemv_w4(blocks, scales, x).double().cpu()
            want = w[:, ks].T
            bad = (got != want).nonzero().tolist()                     # (!= on values: a -0 weight may come back as +0)
            assert not bad, (B, ks, [(b, n, float(got[b, n]), float(want[b, n])) for b, n in bad[:8]])


def test_two_calls_and_a_captured_call_are_bit_identical(ops, dev):
    B, N, K = 3, 130, 3584
    blocks, scales, x, bias, res, nw = _case(dev, B, N, K, seed=11)
    b2, s2, _, _, _, _ = _case(dev, B, N, K, seed=12, rows=2 * N)
    a = ops.gemv_w4(blocks, scales, x, bias=bias, res=res, norm_w=nw, eps=EPS)
    b = ops.gemv_w4(blocks, scales, x, bias=bias, res=res, norm_w=nw, eps=EPS)
    sa = ops.gemv_swiglu_w4(b2, s2, x, norm_w=nw, eps=EPS)
    sb = ops.gemv_swiglu_w4(b2, s2, x, norm_w=nw, eps=EPS)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    out, sout = torch.zeros_like(a), torch.zeros_like(sa)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.gemv_w4(blocks, scales, x, bias=bias, res=res, norm_w=nw, eps=EPS, out=out)
            ops.gemv_swiglu_w4(b2, s2, x, norm_w=nw, eps=EPS, out=sout)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_(); sout.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a) and torch.equal(sout, sa)


def test_shapes_outside_the_kernel_raise(ops, dev):
    from spider_amd.lib import SpiderHipError
    blocks, scales, x, bias, res, nw = _case(dev, 1, 7, 64, seed=1)
    with pytest.raises(ValueError):
        ops.gemv_w4(blocks[:, :24], scales[:, :1], x[:, :48])               # K = 48 is a multiple of 16 (the FP8 rule), not of 32
    with pytest.raises(ValueError):
        ops.gemv_w4(blocks, scales[:3], x)                                   # one scale per block of every row
    with pytest.raises(ValueError):
        ops.gemv_w4(blocks, scales.view(torch.int8), x)                      # bytes have to come as uint8
    with pytest.raises(ValueError, match="rows"):
        ops.gemv_w4(blocks, scales, x.repeat(5, 1))
    with pytest.raises(ValueError, match="rows"):
        ops.gemv_swiglu_w4(blocks[:6], scales[:6], x.repeat(5, 1))
    # the same refusals from the entry point itself
    from spider_amd import lib
    p = lambda t: t.data_ptr()
    with pytest.raises(SpiderHipError, match="multiple of 32"):
        lib.call("spider_gemv_w4", p(blocks), p(scales), p(x), p(bias), None, None, None, 0.0, 1, 7, 48, None)
    with pytest.raises(SpiderHipError, match=r"1\.\.4"):
        lib.call("spider_gemv_swiglu_w4", p(blocks), p(scales), p(x), p(bias), None, 0.0, 5, 3, 64, None)


def test_torch_ops_registration(ops, dev):
    import spider_amd.torch_ops as T
    assert T.W4_OP_NAMES == ("gemv_w4", "gemv_swiglu_w4")
    blocks, scales, x, bias, res, nw = _case(dev, 2, 18, 64, seed=5)
    got = torch.ops.spider_hip.gemv_w4(blocks, scales, x, bias, res, nw, EPS)
    assert torch.equal(got, ops.gemv_w4(blocks, scales, x, bias=bias, res=res, norm_w=nw, eps=EPS))
    got = torch.ops.spider_hip.gemv_swiglu_w4(blocks, scales, x, nw, EPS)
    assert torch.equal(got, ops.gemv_swiglu_w4(blocks, scales, x, norm_w=nw, eps=EPS))
    torch.library.opcheck(torch.ops.spider_hip.gemv_w4, (blocks, scales, x, bias, res, nw, EPS), test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.spider_hip.gemv_swiglu_w4, (blocks, scales, x, nw, EPS), test_utils=("test_schema", "test_faketensor"))

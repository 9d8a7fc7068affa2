"""GPU: the weight-only FP8 decode GEMVs (ops.gemv_w8 / ops.gemv_swiglu_w8, csrc/gemv_wq.hip) against an fp64 restatement on
W_eff = float(q) * scale that rounds where the kernel rounds.

The bound is derived, not measured (the 1e-2 * std + 1e-2 * |ref| of tests/test_hip_ops.py for the bf16 GEMV is a measured one).
With u = 2^-24 the unit roundoff of fp32:

  * every product x[k] * f32(q[n, k]) is exact in fp32 (8 x 4 significand bits), so the fp32 dot product differs from the exact
    one only by its K - 1 additions; in ANY order that is at most (K - 1) u / (1 - (K - 1) u) * sum_k |x[k] q[n, k]|. The test allows
    E = 2 K u * sum_k |x[k] q[n, k]| (the factor 2 covers the two-term adder inside v_dot2c_f32_bf16). The power-of-two scale is exact.
  * a value the kernel rounds to bf16 (after the bias, after the residual, the three SwiGLU roundings) may land on the other side
    of a rounding boundary than the fp64 value whenever the two differ at all: the rounded values then differ by one bf16 ulp,
    <= 2^-7 |ref|. Every such rounding adds 2^-7 |ref| to the error carried so far; fp32 additions add u |ref|.
  * SwiGLU: |silu'| <= 1.1, and silu_f = x * rcp(1 + __expf(-x)) is within 2^-16 relative of silu (exp2 of a product rounded at
    |x| <= 88 and a 1 ulp reciprocal: < 6e-6).
  * fused RMSNorm: rsqrtf and the fp32 sum of squares may move the normalised activation across a bf16 boundary, which is no
    summation error. The test therefore reads the kernel's OWN normalised activations through an identity weight matrix (one
    non-zero exact product per output: out = xin bit for bit), checks them against the fp64 RMSNorm within the two bf16 roundings
    that form has, and feeds them to the restatement. Every block recomputes the norm in the same order, so they are the values
    every launch of that (rows, K) uses: the waves per block, and with them the order of the sum, depend on nothing else.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
U32 = 2.0 ** -24
ULP16 = 2.0 ** -7
EPS = 1e-5


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


def _case(dev, B, N, K, seed, rows=None):
    """random e4m3 bytes (no NaN byte), per-row scales 2^-12 .. 2^3 that differ from row to row, the last weight row = the bytes of
    +-448 and of the smallest subnormal; x, bias, res, norm_w in bf16"""
    rows = rows or N
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, (rows, K), generator=g, dtype=torch.int32).to(torch.uint8)
    b[(b & 0x7f) == 0x7f] = 0x38
    if rows > 1 or B % 2 == 0:
        b[-1] = torch.tensor([0x7e, 0xfe, 0x01, 0x81], dtype=torch.uint8).repeat(K // 4)
    e = (torch.arange(rows) * 5 + seed) % 16 - 12          # step 5 is coprime to 16: neighbours differ, all 16 exponents occur
    scale = torch.ldexp(torch.ones(rows), e.to(torch.int32)).float()
    x = torch.randn(B, K, generator=g).to(BF)
    bias = (torch.randn(N, generator=g) * 4).to(BF)
    res = (torch.randn(B, N, generator=g) * 4).to(BF)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF)
    d = lambda t: t.to(dev)
    return d(b).view(F8), d(scale), d(x), d(bias), d(res), d(nw)


_EYE = {}


def _kernel_xin(ops, dev, x, nw):
    """the kernel's own normalised activations [B, K] bf16, read through an identity matrix (see the module docstring), checked
    against the fp64 RMSNorm: bf16(bf16(x * rs) * w) with at most one ulp of slack per rounding"""
    K = x.shape[-1]
    if K not in _EYE:
        _EYE[K] = ((torch.eye(K, dtype=torch.uint8) * 0x38).to(dev).view(F8), torch.ones(K, device=dev))      # 0x38 = 1.0
    eye, one = _EYE[K]
    assert int(eye.view(torch.uint8)[0, 0]) == 0x38
    xin = ops.gemv_w8(eye, one, x, norm_w=nw, eps=EPS)
    xd = x.double()
    rs = torch.rsqrt((xd * xd).mean(-1, keepdim=True) + EPS)
    a = (xd * rs).to(BF).double()
    ref = (a * nw.double()).to(BF).double()
    tol = ULP16 * ref.abs() * (1 + ULP16) + ULP16 * ref.abs() + 1e-30
    err = (xin.double() - ref).abs()
    assert bool((err <= tol).all()), f"fused RMSNorm: max err / tol {float((err / tol).max()):.3g}"
    return xin


def _dot(xin, q, scale):
    """(exact scaled dot products, the summation bound E) in fp64"""
    xd, wd = xin.double(), q.float().double()
    s = xd @ wd.T * scale.double()
    E = 2 * xin.shape[-1] * U32 * (xd.abs() @ wd.abs().T) * scale.double()
    return s, E


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


def _check_gemv(ops, q, scale, x, xin, bias, res, norm_w, what):
    got = ops.gemv_w8(q, scale, x, bias=bias, res=res, norm_w=norm_w, eps=EPS)
    v, e = _dot(xin, q, scale)
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


def _check_swiglu(ops, q, scale, x, xin, norm_w, what):
    I = q.shape[0] // 2
    got = ops.gemv_swiglu_w8(q, scale, x, norm_w=norm_w, eps=EPS)
    s, E = _dot(xin, q, scale)
    g, eg = _round(s[:, :I], E[:, :I])
    u, eu = _round(s[:, I:], E[:, I:])
    a = g * torch.sigmoid(g)
    a, ea = _round(a, 1.1 * eg + 2.0 ** -16 * a.abs())
    v = a * u
    v, e = _round(v, u.abs() * ea + a.abs() * eu + ea * eu + U32 * v.abs())
    _check(got, v, e, what)
    return got


# K: 64 = shorter than one wave instruction (64 lanes x 16 weights), 1040 = one ragged chunk behind a full one, 4160 = a k loop
# (4 chunks per trip) with a ragged tail. N: 1 and 7 = fewer rows than a block's waves own, 130 = a ragged last block.
@pytest.mark.parametrize("K", [64, 1040, 4160])
@pytest.mark.parametrize("N", [1, 7, 130])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_gemv_w8_and_swiglu_w8(ops, dev, B, N, K):
    q, scale, x, bias, res, nw = _case(dev, B, N, K, seed=B + 7 * N + K)
    xin = _kernel_xin(ops, dev, x, nw)
    for has_bias in (False, True):
        for has_res in (False, True):
            for has_norm in (False, True):
                _check_gemv(ops, q, scale, x, xin if has_norm else x, bias if has_bias else None, res if has_res else None,
                            nw if has_norm else None, f"gemv_w8 B{B} N{N} K{K} bias{int(has_bias)} res{int(has_res)} norm{int(has_norm)}")
    q2, scale2, _, _, _, _ = _case(dev, B, N, K, seed=3 + B + 7 * N + K, rows=2 * N)
    for has_norm in (False, True):
        _check_swiglu(ops, q2, scale2, x, xin if has_norm else x, nw if has_norm else None, f"gemv_swiglu_w8 B{B} I{N} K{K} norm{int(has_norm)}")


# The other launch forms. K = 8208: 8 waves per block (from K = 8192), at 4 rows with a staged copy above the 64 KiB a launch gets
# without opting in (4 * 9 * 2 KiB). K = 19472: 2 rows stage 80 KiB; at 4 rows the copy (4 * 20 * 2 KiB, and B * K * 2 = 152 KiB
# of activations) exceeds the LDS budget of 160 KiB less 256 bytes, so the waves re-read x through L2 and the fused norm is refused.
# N * K >= 24 Mi weights at one row: two weight rows per wave.
@pytest.mark.parametrize("B,N,K", [(1, 130, 8208), (4, 7, 8208), (4, 130, 8208), (2, 7, 19472), (4, 18, 19472), (1, 6144, 4096)])
def test_gemv_w8_other_launch_forms(ops, dev, B, N, K):
    from spider_amd.lib import SpiderHipError
    q, scale, x, bias, res, nw = _case(dev, B, N, K, seed=B + N + K)
    _check_gemv(ops, q, scale, x, x, None, None, None, f"gemv_w8 B{B} N{N} K{K}")
    _check_gemv(ops, q, scale, x, x, bias, res, None, f"gemv_w8 B{B} N{N} K{K} bias res")
    if N % 2 == 0:
        _check_swiglu(ops, q, scale, x, x, None, f"gemv_swiglu_w8 B{B} I{N // 2} K{K}")
    assert ops.w8_norm_fits(B, K) == (B * ((K + 1023) // 1024) * 2048 <= 160 * 1024 - 256)
    if ops.w8_norm_fits(B, K):
        if K <= 8208:     # (the identity probe is K x K bytes)
            xin = _kernel_xin(ops, dev, x, nw)
            _check_gemv(ops, q, scale, x, xin, bias, res, nw, f"gemv_w8 B{B} N{N} K{K} bias res norm")
            if N % 2 == 0:
                _check_swiglu(ops, q, scale, x, xin, nw, f"gemv_swiglu_w8 B{B} I{N // 2} K{K} norm")
    else:                 # no LDS copy, no fused norm: the entry point says so
        assert (B, K) == (4, 19472)
        with pytest.raises(SpiderHipError, match="fused RMSNorm"):
            ops.gemv_w8(q, scale, x, norm_w=nw, eps=EPS)


def test_two_calls_and_a_captured_call_are_bit_identical(ops, dev):
    B, N, K = 3, 130, 4160
    q, scale, x, bias, res, nw = _case(dev, B, N, K, seed=11)
    q2, scale2, _, _, _, _ = _case(dev, B, N, K, seed=12, rows=2 * N)
    a = ops.gemv_w8(q, scale, x, bias=bias, res=res, norm_w=nw, eps=EPS)
    b = ops.gemv_w8(q, scale, x, bias=bias, res=res, norm_w=nw, eps=EPS)
    sa = ops.gemv_swiglu_w8(q2, scale2, x, norm_w=nw, eps=EPS)
    sb = ops.gemv_swiglu_w8(q2, scale2, x, norm_w=nw, eps=EPS)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    out, sout = torch.zeros_like(a), torch.zeros_like(sa)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            ops.gemv_w8(q, scale, x, bias=bias, res=res, norm_w=nw, eps=EPS, out=out)
            ops.gemv_swiglu_w8(q2, scale2, x, norm_w=nw, eps=EPS, out=sout)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_(); sout.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a) and torch.equal(sout, sa)


def test_shapes_outside_the_kernel_raise(ops, dev):
    from spider_amd.lib import SpiderHipError
    q, scale, x, bias, res, nw = _case(dev, 1, 7, 72, seed=1)          # 72 is a multiple of 8 (the bf16 GEMV's rule), not of 16
    with pytest.raises(SpiderHipError, match="multiple of 16"):
        ops.gemv_w8(q, scale, x)
    with pytest.raises(SpiderHipError, match="multiple of 16"):
        ops.gemv_swiglu_w8(q[:6], scale[:6], x)
    q, scale, x, bias, res, nw = _case(dev, 5, 7, 64, seed=2)
    with pytest.raises(SpiderHipError, match="batch"):
        ops.gemv_w8(q, scale, x)
    with pytest.raises(ValueError):
        ops.gemv_w8(q.view(torch.uint8), scale, x[:1])                   # bytes have to come as float8_e4m3fn
    with pytest.raises(ValueError):
        ops.gemv_w8(q, scale[:3], x[:1])                                 # one scale per weight row


def test_torch_ops_registration(ops, dev):
    import spider_amd.torch_ops as T
    assert T.W8_OP_NAMES == ("gemv_w8", "gemv_swiglu_w8")
    q, scale, x, bias, res, nw = _case(dev, 2, 18, 64, seed=5)
    got = torch.ops.spider_hip.gemv_w8(q, scale, x, bias, res, nw, EPS)
    assert torch.equal(got, ops.gemv_w8(q, scale, x, bias=bias, res=res, norm_w=nw, eps=EPS))
    got = torch.ops.spider_hip.gemv_swiglu_w8(q, scale, x, nw, EPS)
    assert torch.equal(got, ops.gemv_swiglu_w8(q, scale, x, norm_w=nw, eps=EPS))
    # (opcheck's test_schema clones its arguments through arithmetic that torch does not have for float8 tensors)
    torch.library.opcheck(torch.ops.spider_hip.gemv_w8, (q, scale, x, bias, res, nw, EPS), test_utils=("test_faketensor",))
    torch.library.opcheck(torch.ops.spider_hip.gemv_swiglu_w8, (q, scale, x, nw, EPS), test_utils=("test_faketensor",))

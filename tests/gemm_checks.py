"""fp64 restatements of the GEMM / conv entry points (ops.gemm, gemm_ln, gemm_gn_in, conv2d, conv_ex) with their epilogues, and a
DERIVED elementwise error bound for kernels that multiply 16-bit operands exactly and accumulate in fp32.

The bound (no fitted atol). With c = 8 sqrt(K) 2^-24 and q = sqrt(A^2 @ (W^2)^T + bias^2 + rowbias^2 + res^2):

    fp32 output (out_f32, the want32 copy):  tol32 = c q |out_scale|
    16-bit output:                           tol16 = max(u |ref|, eta) + tol32,   u = 2^-11 (f16) / 2^-8 (bf16)
                                             (eta = 2^-25 / 2^-134: half a subnormal step, the error of a correct rounding there)

8 sqrt(K) is a random-walk bound on fp32 accumulation of K products IN ANY ORDER (each partial sum carries a relative error of
2^-24; for zero-mean terms the partial sums grow like sqrt of the sum of squares, hence q and not sum |a w|). It holds for zero-mean
operands only: every test that uses it draws randn operands with the weights scaled by K^-0.5. tol16 is one correct rounding of an
fp32 value that is itself within tol32. Every element has to be inside; there is no outlier allowance.

Terms beyond the plain product, each from what the kernel's source documents:
* activation: the pre-activation bound is propagated with the Lipschitz constant 1.13 (gelu, silu, quick_gelu; tanh / relu / leaky
  are <= 1), plus ACT_TOL[kind] for the device function's own approximation error -- the one MEASURED term (NOTEBOOK.md);
* a 16-bit `res`: the kernels round act(...) to the 16-bit format BEFORE they add it ("as the reference's separate ops do",
  epilogue_store in csrc/gemm.hip), so u (|act(...)| + its bound) is added; an fp32 `res32` is added to the unrounded value;
* GEGLU / SwiGLU: the product rule over the roundings the ops.ACT comment documents (see finish_glu);
* gemm_ln: the fp32 row statistics (see pre_ln);  gemm_gn_in: the 16-bit rounding of the normalised A (see pre_gn_in).
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# half the spacing of the format's subnormals: below its smallest normal number (f16: 2^-14 = 6.1e-5, which GEGLU products of two
# small factors do reach) a correct rounding errs by up to this much, not by u |x|
ETA = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
LIP = 1.13                    # max |d act / dx| of gelu (1.129), silu (1.0998), quick_gelu (1.0998)
SMOOTH = ("silu", "gelu", "quick_gelu")
GLU_KIND = {"geglu": "gelu", "geglu_exact": "gelu", "swiglu": "silu"}
# The device activations' own error (absolute, at the activation's output), per kind: 4 x the largest excess of |got - ref64| over
# the derived bound, measured once on an MI355X with this table at zero (NOTEBOOK.md, "GEMM/conv route tests"). No case exceeded the
# derived bound (largest excess: silu -2.8e-6, gelu -2.7e-6, quick_gelu -2.8e-6, leaky_relu -3.5e-6, tanh -3.8e-6, i.e. inside),
# so every entry is 4 x 0.
ACT_TOL = {"silu": 0.0, "gelu": 0.0, "quick_gelu": 0.0, "tanh": 0.0, "relu": 0.0, "leaky_relu": 0.0}
LOG = []                      # one record per check(): the figures, appended before the assertion


def rnd_err(x, dt):
    """error bound of one correct rounding of |x| (fp64 tensor) to the 16-bit format"""
    return (U[dt] * x.abs()).clamp_min(ETA[dt])


def acc_c(K: int) -> float:
    return 8.0 * math.sqrt(K) * 2.0 ** -24


def act64(kind, x, param=0.0):
    if kind in (None, "none"):
        return x
    if kind == "silu":
        return x * torch.sigmoid(x)
    if kind == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if kind == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if kind == "leaky_relu":
        return torch.where(x > 0, x, x * param)
    if kind == "relu":
        return x.clamp_min(0)
    if kind == "tanh":
        return torch.tanh(x)
    raise ValueError(kind)


@dataclass
class Base:
    """A @ W^T and A^2 @ (W^2)^T in fp64 (K = reduction length): shared by every epilogue form of one problem"""
    p: torch.Tensor
    q2: torch.Tensor
    K: int


@dataclass
class Pre:
    """the value an epilogue starts from (after bias / rowbias / normalisation fix-up), in fp64, and the bound on the fp32 value the
    kernel holds for it"""
    p: torch.Tensor
    t: torch.Tensor
    K: int


@dataclass
class Ref:
    ref: torch.Tensor                 # fp64 result
    tol32: torch.Tensor               # derived bound on the kernel's fp32 value before its last rounding (without ACT_TOL)
    act: Optional[str] = None         # activation kind whose ACT_TOL applies
    gain: object = 1.0                # |d result / d activation output|: what ACT_TOL is multiplied by


def matmul64(A, W) -> Base:
    A, W = A.double(), W.double()
    return Base(A @ W.T, (A * A) @ (W * W).T, A.shape[-1])


def conv_cols(x, kh, kw, stride=1, pad=(0, 0), dil=1, up_size=None):
    """im2col of an NHWC tensor in fp64 -> ([B * Ho * Wo, Cin * kh * kw] in (channel, tap) order, Ho, Wo); `up_size`: through a
    nearest upsample to that size first (F.interpolate(size=...), what conv_ex documents)"""
    xi = x.double().permute(0, 3, 1, 2)
    if up_size is not None:
        xi = F.interpolate(xi, size=tuple(up_size), mode="nearest")
    B, _, Hs, Ws = xi.shape
    Ho = (Hs + 2 * pad[0] - dil * (kh - 1) - 1) // stride + 1
    Wo = (Ws + 2 * pad[1] - dil * (kw - 1) - 1) // stride + 1
    cols = F.unfold(xi, (kh, kw), dilation=dil, padding=tuple(pad), stride=stride)
    return cols.transpose(1, 2).reshape(B * Ho * Wo, -1), Ho, Wo


def conv_base(x, w, stride=1, pad=(0, 0), dil=1, up_size=None, rows=None):
    """the conv as a GEMM over [rows of] its im2col matrix; w [Cout, kh, kw, Cin] (OHWI). -> (Base [M, Cout], (B, Ho, Wo))"""
    Cout, kh, kw, Cin = w.shape
    cols, Ho, Wo = conv_cols(x, kh, kw, stride, pad, dil, up_size)
    if rows is not None:
        cols = cols[rows]
    return matmul64(cols, w.double().permute(0, 3, 1, 2).reshape(Cout, -1)), (x.shape[0], Ho, Wo)


def pre_gemm(base: Base, bias=None, rowbias=None, rows_per_group=0, row_ids=None) -> Pre:
    """A @ W^T + bias + rowbias[row // rows_per_group]; row_ids: the global row numbers when `base` holds a subset of the rows"""
    p, q2 = base.p.clone(), base.q2.clone()
    if bias is not None:
        b = bias.double()
        p += b
        q2 += b * b
    if rowbias is not None:
        m = torch.arange(p.shape[0]) if row_ids is None else row_ids
        rb = rowbias.double().reshape(-1, p.shape[1])[m // rows_per_group]
        p += rb
        q2 += rb * rb
    return Pre(p, acc_c(base.K) * q2.sqrt(), base.K)


def pre_ln(A, Wf, colsum, colbias, eps) -> Pre:
    """gemm_ln: rstd * (A @ Wf^T - mean * colsum) + colbias with (Wf, colsum, colbias) = ops.fold_layernorm(...) as operands.
    The kernels take mean = S1 / K and var = max(S2 / K - mean^2, 0) from fp32 sums S1, S2 of the row (ln_row_stats_kernel and the
    register-staged kernels: same formulas). With c = 8 sqrt(K) 2^-24 (random-walk bound of an fp32 sum, as for the product):
        |d mean| <= c sqrt(sum a^2) / K,   |d var| <= c sqrt(sum a^4) / K + 2 |mean| |d mean| + 4 * 2^-24 * S2 / K,
        |d rstd| / rstd <= |d var| / (2 (var + eps)) + 2^-22          (rsqrtf: 1 ulp, the add and the division before it)
    and the result inherits  rstd (c q + |d mean| |colsum|) + (|d rstd| / rstd) |rstd (acc - mean colsum)|  plus 4 fp32 roundings
    of the terms of the fix-up."""
    A64, W64 = A.double(), Wf.double()
    K = A64.shape[-1]
    A64 = A64.reshape(-1, K)
    c, e = acc_c(K), 2.0 ** -24
    acc, q = A64 @ W64.T, ((A64 * A64) @ (W64 * W64).T).sqrt()
    s2 = (A64 * A64).sum(1, keepdim=True)
    mean = A64.mean(1, keepdim=True)
    var = (s2 / K - mean * mean).clamp_min(0)
    rstd = (var + eps).rsqrt()
    cs, cb = colsum.double()[None, :], colbias.double()[None, :]
    core = rstd * (acc - mean * cs)
    d_mean = c * s2.sqrt() / K
    d_var = c * (A64 ** 4).sum(1, keepdim=True).sqrt() / K + 2 * mean.abs() * d_mean + 4 * e * s2 / K
    d_rstd_rel = d_var / (2 * (var + eps)) + 4 * e
    t = rstd * (c * q + d_mean * cs.abs()) + d_rstd_rel * core.abs() + 4 * e * ((rstd * acc).abs() + (rstd * mean * cs).abs() + cb.abs())
    return Pre(core + cb, t, K)


def pre_gn_in(A, W, gamma, beta, groups, HW, eps, dt, bias=None) -> Pre:
    """gemm_gn_in: GroupNorm(A) @ W^T + bias, A [B, HW, K]. The kernel stores round16(x * a_c + b_c) (a_c = rstd_g gamma_c, b_c =
    beta_c - mean_g a_c, fp32) into its image of A: every normalised element carries an independent 16-bit rounding error of at most
    u |a|, uniform in its interval (variance <= (u a)^2 / 3). Their weighted sum over K >= 320 terms is a zero-mean sum of independent
    bounded terms with standard deviation <= u / sqrt(3) * sqrt(a^2 @ (W^2)^T); 6 standard deviations (2e-9 per element, < 1e-3 over
    the elements of a test) bound it. The fp32 group statistics (sums of HW * K / G values) add a relative
    error e_s = 2 * 8 sqrt(HW K / G) 2^-24 on mean / rstd, i.e. at most e_s (|a - beta| + |gamma|) on an element of the normalised A
    (systematic: summed with |W|)."""
    B = A.shape[0]
    K = A.shape[-1]
    x = A.double().reshape(B, HW, groups, K // groups)
    mean = x.mean((1, 3), keepdim=True)
    var = (x * x).mean((1, 3), keepdim=True) - mean * mean
    g64, b64 = gamma.double(), beta.double()
    xn = ((x - mean) * (var + eps).rsqrt()).reshape(B * HW, K)
    a = xn * g64 + b64
    W64 = W.double()
    base = Base(a @ W64.T, (a * a) @ (W64 * W64).T, K)
    pre = pre_gemm(base, bias=bias)
    e_s = 2 * acc_c(HW * K // groups)
    syst = e_s * ((xn * g64).abs() + g64.abs()) @ W64.abs().T
    q_a = ((a * a) @ (W64 * W64).T).sqrt()
    pre.t = pre.t + 6.0 * U[dt] / math.sqrt(3.0) * q_a + syst
    return pre


def finish(pre: Pre, dt, act=None, act_param=0.0, res=None, res32=None, out_scale=1.0) -> Ref:
    """act(pre) (+ res) * out_scale, the order of every non-GLU epilogue"""
    act = None if act == "none" else act
    c = acc_c(pre.K)
    y = act64(act, pre.p, act_param)
    t = pre.t * (LIP if act in SMOOTH else 1.0)
    gain = 1.0
    r = None
    if res32 is not None:
        r = res32.double().reshape(y.shape)
    elif res is not None:
        r = res.double().reshape(y.shape)
        t = t + rnd_err(y.abs() + t, dt)          # act(...) is rounded to the 16-bit format before the 16-bit residual is added
        gain = 1.0 + U[dt]
    if r is not None:
        y = y + r
        t = (t * t + (c * r) ** 2).sqrt()         # the issue's q: res^2 under the root
    s = abs(float(out_scale))
    return Ref(y * float(out_scale), t * s, act if act in ACT_TOL else None, gain * s)


def finish_glu(pre: Pre, dt, act) -> Ref:
    """fused GLU epilogues over W = [first half | second half] rows (ops.ACT, geglu_out in csrc/gemm.hip); r() = one rounding to the
    16-bit format, relative error u; e_x = bound on the kernel's value of x:
      geglu (4):        out = r(v) * r(gelu(r(g))),        v = first half, g = second half
      swiglu (8):       out = r(silu(r(a))) * r(b),        a = first half (gate rows), b = second half (up rows)
      geglu_exact (9):  out = v * gelu(g), rounded once
    product rule: |x' y' - x y| <= e_x |y| + |x| e_y + e_x e_y; the final rounding of the product is tol16's u |ref|."""
    u = U[dt]
    inner = pre.p.shape[1] // 2
    a, b = pre.p[:, :inner], pre.p[:, inner:]
    ta, tb = pre.t[:, :inner], pre.t[:, inner:]
    rnd = lambda x, t: t + rnd_err(x.abs() + t, dt)      # bound after one more rounding of a value within t of x
    if act == "geglu":
        lin, e_lin = a, rnd(a, ta)
        fx = act64("gelu", b)
        e_f = rnd(fx, LIP * rnd(b, tb))
        gain = (lin.abs() + e_lin) * (1 + u)
    elif act == "swiglu":
        lin, e_lin = b, rnd(b, tb)
        fx = act64("silu", a)
        e_f = rnd(fx, LIP * rnd(a, ta))
        gain = (lin.abs() + e_lin) * (1 + u)
    elif act == "geglu_exact":
        lin, e_lin = a, ta
        fx = act64("gelu", b)
        e_f = LIP * tb
        gain = lin.abs() + e_lin
    else:
        raise ValueError(act)
    tol = e_lin * fx.abs() + lin.abs() * e_f + e_lin * e_f
    return Ref(lin * fx, tol, GLU_KIND[act], gain)


def ref64(op: str, *args, dt, **kw) -> Ref:
    """fp64 restatement of one call, operands = the 16-bit-rounded tensors the kernel gets:
      ref64("gemm", A, W, bias=, rowbias=, rows_per_group=, act=, res=, res32=, out_scale=, dt=)       (act may be a GLU kind)
      ref64("gemm_ln", A, Wf, colsum, colbias, eps=, res=, act=, dt=)
      ref64("gemm_gn_in", A, W, gamma, beta, groups=, HW=, eps=, bias=, dt=)
      ref64("conv2d", x, w, bias=, rowbias=, res=, res32=, stride=, pad=, ups=, out_scale=, dt=)         -> [B, Ho, Wo, Cout]
      ref64("conv_ex", x, w, bias=, rowbias=, res=, res32=, stride=, pad=(,), dil=, up_size=, act=, act_param=, out_scale=, dt=)
    Tests that check several epilogues of one problem build the Base once (matmul64 / conv_base) and call pre_gemm / finish."""
    if op == "gemm":
        A, W = args
        pre = pre_gemm(matmul64(A.reshape(-1, A.shape[-1]), W), kw.get("bias"), kw.get("rowbias"), kw.get("rows_per_group", 0))
        if kw.get("act") in GLU_KIND:
            return finish_glu(pre, dt, kw["act"])
        return finish(pre, dt, kw.get("act"), 0.1, kw.get("res"), kw.get("res32"), kw.get("out_scale", 1.0))
    if op == "gemm_ln":
        A, Wf, colsum, colbias = args
        pre = pre_ln(A, Wf, colsum, colbias, kw.get("eps", 1e-5))
        if kw.get("act") in GLU_KIND:
            return finish_glu(pre, dt, kw["act"])
        return finish(pre, dt, None, 0.0, kw.get("res"))
    if op == "gemm_gn_in":
        A, W, gamma, beta = args
        return finish(pre_gn_in(A, W, gamma, beta, kw["groups"], kw["HW"], kw["eps"], dt, kw.get("bias")), dt)
    if op in ("conv2d", "conv_ex"):
        x, w = args
        if op == "conv2d":
            ks = w.shape[1]
            pd = ks // 2 if kw.get("pad") is None else kw["pad"]
            pad, dil = (pd, pd), 1
            up = (2 * x.shape[1], 2 * x.shape[2]) if kw.get("ups") else None
        else:
            pad, dil, up = kw.get("pad", (0, 0)), kw.get("dil", 1), kw.get("up_size")
        base, (B, Ho, Wo) = conv_base(x, w, kw.get("stride", 1), pad, dil, up)
        pre = pre_gemm(base, kw.get("bias"), kw.get("rowbias"), Ho * Wo)
        R = finish(pre, dt, kw.get("act"), kw.get("act_param", 0.0), kw.get("res"), kw.get("res32"), kw.get("out_scale", 1.0))
        shape = (B, Ho, Wo, w.shape[0])
        R.ref, R.tol32 = R.ref.reshape(shape), R.tol32.reshape(shape)
        return R
    raise ValueError(op)


def bound(R: Ref, dt, fp32_out: bool, act_tol=None):
    """the elementwise tolerance of a result against R.ref: tol32 for an fp32 output, max(u |ref|, eta) + tol32 for a 16-bit one,
    plus the activation's measured term"""
    tol = R.tol32 if fp32_out else rnd_err(R.ref, dt) + R.tol32
    if R.act is not None:
        tol = tol + R.gain * (ACT_TOL if act_tol is None else act_tol)[R.act]
    return tol


def check(what: str, got, R: Ref, dt, fp32_out: bool):
    """every element of `got` within bound(); the figures go to LOG (and stdout) before the assertion"""
    got = got.detach().double().cpu().reshape(R.ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - R.ref).abs()
    derived = bound(R, dt, fp32_out, dict.fromkeys(ACT_TOL, 0.0))
    tol = bound(R, dt, fp32_out)
    ratio = float((err / derived.clamp_min(1e-300)).max())
    rec = {"what": what, "dtype": str(dt).replace("torch.", ""), "out": "f32" if fp32_out else "16", "ratio": ratio, "act": R.act}
    if R.act is not None:      # how far the activation's own error pushes past the derived bound, in units of the activation's output
        exc = (err - derived) / (R.gain if torch.is_tensor(R.gain) else torch.full_like(err, R.gain)).clamp_min(1e-300)
        i = int(exc.argmax())
        rec["act_excess"] = float(exc.reshape(-1)[i])
        rec["act_excess_at_ref"] = float(R.ref.reshape(-1)[i])
    LOG.append(rec)
    print(f"[gemm_checks] {what} {rec['dtype']} out={rec['out']}: max err / tol = {ratio:.3f}" +
          (f", act excess {rec['act_excess']:.3e}" if R.act is not None else ""))
    bad = ~(err <= tol)
    n_bad = int(bad.sum())
    assert n_bad == 0, (f"{what}: {n_bad} / {bad.numel()} elements outside the derived bound, worst err / tol = "
                        f"{float((err / tol.clamp_min(1e-300)).max()):.3f} (max err {float(err.max()):.4g})")

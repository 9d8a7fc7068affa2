"""fp64 restatements of the normalisation entry points (ops.groupnorm, groupnorm_cat, groupnorm_f32in, groupnorm_f32in_split,
layernorm, row_split with gamma, and the A side of gemm_gn_in / gemm_gn_in_a32) and a DERIVED elementwise error bound for kernels
that take their statistics in fp32. Companion of gemm_checks.py, whose rnd_err / acc_c / act64 / ACT_TOL / LIP it reuses.

The reference runs on exactly the values the kernel reads: 16-bit inputs after their rounding, fp32 inputs as they are, gamma and
beta in the 16-bit format. LayerNorm is GroupNorm with one group per row (B = rows, HW = 1, G = 1).

Two models of the kernel's fp32 statistics, each a pair (d_mean, d_var) per (batch, group), n = HW * C / G values per group,
c = acc_c(n) = 8 sqrt(n) 2^-24 (random-walk bound of an fp32 sum in any order, as in gemm_checks.pre_ln), e = 2^-24:

  onepass   the public (sum, sum of squares) format: mean = S / n, var = max(Q / n - mean^2, 0) from fp32 sums S, Q.
                d_mean = c sqrt(sum x^2) / n
                d_var  = c sqrt(sum x^4) / n + 2 |mean| d_mean + 4 e Q / n
            The last two terms grow with mean^2: Q / n = var + mean^2 carries the mean, and var is what is left after the
            subtraction. About 2 log2(|mean| / sigma) bits are lost.
  centered  statistics that no longer depend on the mean (two passes, a pivot, (mean, M2) merged by Chan's formula): the same
            formulas on z = x - mean, plus one fp32 rounding of the mean itself and the square of the mean's error (a second pass
            around a mean that is off by d_mean sees var + d_mean^2):
                d_mean = c sqrt(sum z^2) / n + e |mean|
                d_var  = c sqrt(sum z^4) / n + 4 e sum z^2 / n + d_mean^2

From those, the bound on the fp32 value x * a_c + b_c (a_c = rstd_g gamma_c, b_c = beta_c - mean_g a_c):

    t = rstd |gamma| d_mean                                              the mean's error, scaled like the output
      + (d_var / (2 (var + eps)) + 4 e) |xn gamma|                       rstd's relative error (rsqrtf: 1 ulp, the add, the division)
      + 4 e (|x a_c| + |mean a_c| + |beta|)                              the fp32 roundings of a_c, b_c and the fma

The last line covers gn_apply_kernel's fma form; (x - mu) * rs * gamma + beta (gn_small_kernel, the LayerNorm kernels) rounds
smaller intermediates and is inside it too.

Then the roundings each route performs (gc.rnd_err = one correct rounding to the 16-bit format):
  form "16"     16-bit routes: the affine value is rounded, SiLU (Lipschitz constant gc.LIP, gc.ACT_TOL) is taken of the rounded
                value, and the result is rounded again (the final rounding is added by check());
  form "f32in"  fp32-input routes: SiLU of the unrounded value; y32 carries no rounding, y one;
  form "split"  [hi | lo] compared as hi + lo. There is no first-order 16-bit term: hi + lo = v up to the rounding of the remainder
                lo = round16(v - hi), |v - hi| <= u |v|, i.e. max(u^2 |v|, eta) -- 2^-16 |v| in bf16, 2^-22 |v| in f16.
"""
import math
from dataclasses import dataclass

import torch

import gemm_checks as gc
from gemm_checks import ACT_TOL, LIP, Ref, U, acc_c, act64, rnd_err

E32 = 2.0 ** -24
LOG = []                      # one record per check(): the figures, appended before the assertion


@dataclass
class GN:
    """one GroupNorm problem in fp64; tensors are [B, HW, G, C / G] or broadcast over it"""
    x: torch.Tensor
    mean: torch.Tensor
    var: torch.Tensor
    rstd: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor
    xn: torch.Tensor
    eps: float
    shape: tuple

    @property
    def n(self):
        return self.x.shape[1] * self.x.shape[3]

    @property
    def aff(self):
        return self.xn * self.gamma + self.beta


def shifted_input(gen, B, HW, C, groups, sigma, ratio):
    """randn * sigma + mean_g (fp32) with mean_g / sigma = +-ratio: the sign alternates from group to group and group 1 has mean 0,
    so one tensor mixes conditionings and a wrong group lookup shows"""
    sign = torch.tensor([0.0 if g == 1 else (1.0 if g % 2 == 0 else -1.0) for g in range(groups)])
    mean = (sign * float(ratio) * float(sigma)).repeat_interleave(C // groups)
    return torch.randn(B, HW, C, generator=gen) * float(sigma) + mean


def gn64(x, gamma, beta, groups, eps) -> GN:
    """x [B, ..., C] (the values the kernel reads), gamma / beta [C] (16-bit tensors)"""
    B, C = x.shape[0], x.shape[-1]
    x64 = x.detach().double().cpu().reshape(B, -1, groups, C // groups)
    mean = x64.mean((1, 3), keepdim=True)
    var = ((x64 - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = (var + eps).rsqrt()
    g64 = gamma.detach().double().cpu().reshape(1, 1, groups, C // groups)
    b64 = beta.detach().double().cpu().reshape(1, 1, groups, C // groups)
    return GN(x64, mean, var, rstd, g64, b64, (x64 - mean) * rstd, float(eps), tuple(x.shape))


def ln64(x, gamma, beta, eps) -> GN:
    """LayerNorm over the last dim: one group per row"""
    K = x.shape[-1]
    g = gn64(x.reshape(-1, 1, K), gamma, beta if beta is not None else torch.zeros(K), 1, eps)
    g.shape = tuple(x.shape)
    return g


def stats_err(g: GN, model: str):
    """(d_mean, d_var) of the fp32 statistics, per (batch, group), by the named model (module docstring)"""
    n, c = g.n, acc_c(g.n)
    if model == "onepass":
        x2 = g.x * g.x
        Q = x2.sum((1, 3), keepdim=True)
        d_mean = c * Q.sqrt() / n
        d_var = c * (x2 * x2).sum((1, 3), keepdim=True).sqrt() / n + 2 * g.mean.abs() * d_mean + 4 * E32 * Q / n
        return d_mean, d_var
    if model == "centered":
        z2 = (g.x - g.mean) ** 2
        Q = z2.sum((1, 3), keepdim=True)
        d_mean = c * Q.sqrt() / n + E32 * g.mean.abs()
        d_var = c * (z2 * z2).sum((1, 3), keepdim=True).sqrt() / n + 4 * E32 * Q / n + d_mean * d_mean
        return d_mean, d_var
    raise ValueError(model)


def affine_tol(g: GN, d_mean, d_var):
    """bound on the kernel's fp32 value of x * a_c + b_c given the errors of its statistics"""
    a_c = g.rstd * g.gamma
    return (g.rstd * g.gamma.abs() * d_mean
            + (d_var / (2 * (g.var + g.eps)) + 4 * E32) * (g.xn * g.gamma).abs()
            + 4 * E32 * ((g.x * a_c).abs() + (g.mean * a_c).abs() + g.beta.abs()))


def blind_tol(g: GN):
    """the mean-blind model of gemm_checks.pre_gn_in: a relative error e_s = 2 acc_c(n) on mean / rstd, i.e. e_s (|xn gamma| +
    |gamma|) on an element. True for small means only -- kept here so that the CPU sweep can show where it stops holding."""
    return 2 * acc_c(g.n) * ((g.xn * g.gamma).abs() + g.gamma.abs())


def finish_norm(g: GN, t, dt, form: str, silu: bool = False) -> Ref:
    """the Ref of one route given the bound t on its fp32 affine value (forms: module docstring)"""
    v = g.aff
    if form == "16" and silu:
        t = t + rnd_err(v.abs() + t, dt)
    if silu:
        v, t = act64("silu", v), LIP * t
    if form == "split":
        t = t + rnd_err(U[dt] * (v.abs() + t), dt)
    elif form not in ("16", "f32in"):
        raise ValueError(form)
    return Ref(v.reshape(g.shape), t.reshape(g.shape), "silu" if silu else None, 1.0)


def norm_ref(g: GN, model: str, dt, form: str, silu: bool = False) -> Ref:
    return finish_norm(g, affine_tol(g, *stats_err(g, model)), dt, form, silu)


def pre_gn_in(A, W, gamma, beta, groups, HW, eps, dt, bias=None, a32=False) -> gc.Pre:
    """gemm_gn_in / gemm_gn_in_a32 with statistics in the public format: gemm_checks.pre_gn_in with its mean-blind e_s replaced by
    the `onepass` bound on every element of the normalised A (systematic: summed with |W|).
    a32 = False: the kernel stores round16(x a_c + b_c) -- independent roundings of at most u |a|, 6 standard deviations of their
    weighted sum as in gemm_checks.pre_gn_in. a32 = True: A32 is normalised in fp32 and split into hi + lo; what is lost is the
    rounding of lo, max(u^2 |a|, eta) per element, again independent; both routes accumulate 2 K products (two MFMAs per K step, or
    the doubled K of "split once"), hence acc_c(2 K)."""
    B, K = A.shape[0], A.shape[-1]
    g = gn64(A.reshape(B, HW, K), gamma, beta, groups, eps)
    a = g.aff.reshape(B * HW, K)
    t_a = affine_tol(g, *stats_err(g, "onepass")).reshape(B * HW, K)
    W64 = W.detach().double().cpu()
    W2 = W64 * W64
    base = gc.Base(a @ W64.T, (a * a) @ W2.T, 2 * K if a32 else K)
    pre = gc.pre_gemm(base, bias=None if bias is None else bias.detach().cpu())
    e_el = rnd_err(U[dt] * (a.abs() + t_a), dt) if a32 else rnd_err(a.abs() + t_a, dt)
    pre.t = pre.t + 6.0 / math.sqrt(3.0) * ((e_el * e_el) @ W2.T).sqrt() + t_a @ W64.abs().T
    return pre


def bound(R: Ref, dt, fp32_out: bool, act_tol=None):
    """tol32 for an fp32 result (or a hi + lo sum); plus one correct rounding of a value within tol32 of the reference for a 16-bit
    one; plus the activation's measured term"""
    tol = R.tol32 if fp32_out else R.tol32 + rnd_err(R.ref.abs() + R.tol32, dt)
    if R.act is not None:
        tol = tol + R.gain * (ACT_TOL if act_tol is None else act_tol)[R.act]
    return tol


def ratio(got, R: Ref, dt, fp32_out: bool):
    """(worst err / bound, relative L2 error) of `got` against R"""
    got = got.detach().double().cpu().reshape(R.ref.shape)
    err = (got - R.ref).abs()
    return float((err / bound(R, dt, fp32_out).clamp_min(1e-300)).max()), float(err.norm() / R.ref.norm().clamp_min(1e-300))


def check(what: str, got, R: Ref, dt, fp32_out: bool):
    """every element of `got` within bound(); the worst err / bound ratio is printed (and appended to LOG) before the assertion"""
    got = got.detach().double().cpu().reshape(R.ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    tol = bound(R, dt, fp32_out)
    err = (got - R.ref).abs()
    r, l2 = ratio(got, R, dt, fp32_out)
    LOG.append({"what": what, "dtype": str(dt).replace("torch.", ""), "out": "f32" if fp32_out else "16", "ratio": r, "rel_l2": l2})
    print(f"[norm_checks] {what} {LOG[-1]['dtype']} out={LOG[-1]['out']}: max err / tol = {r:.3f}, rel L2 = {l2:.3e}")
    bad = ~(err <= tol)
    n_bad = int(bad.sum())
    assert n_bad == 0, (f"{what}: {n_bad} / {bad.numel()} elements outside the derived bound, worst err / tol = {r:.3f} "
                        f"(max err {float(err.max()):.4g})")

"""Shared by the scoring tests: the fp64 reference of ops.logprob_rows (csrc/logprob.hip) on the SAME bf16 logits, and the tolerance of
every output, derived from the kernel's own summation.

The kernel gives a row T = 256 lanes. With u = 2^-24 (fp32 unit round-off), z_i = x_i - m (m = the row maximum, exact: a maximum of
bf16 values), e_i = exp(z_i), s = sum e_i, p_i = e_i / s:

  positive sums (s, s_ref)
    a lane adds its <= ceil(V / T) + 7 terms one after the other, the 256 lane sums merge in log2 T = 8 steps and the four wave sums
    in 3 more, every step one rounded add and one rounded product with a rescale factor that is exactly 1 when the maxima agree.
    That is the chain of n = ceil(V / T) + log2 T + 8 dependent fp32 operations the bound counts, each <= 2u relative (u for the
    add, u for what else touches the partial sum at that step):            |ds| / s <= EPS(V) = n * 2^-23.
    At V = 152064: n = 610, EPS = 7.3e-5. A kernel with fewer lanes per row (a more serial sum) would need a larger n: T >= 128 is
    what keeps the tolerance of lse at that size below 2e-4 (asserted in test_score_cpu.py).
  the exponential
    e_i = v_exp_f32(fl(z_i * log2 e)): the product's rounding (and the constant's) moves the exponent by <= 2u |z_i| log2 e, i.e. e_i by
    2u |z_i| relative, the instruction itself by 2u (1 ulp). A term that entered under an earlier, lower maximum is rescaled by
    exp(d_1) exp(d_2) ... with sum |d_k| <= |z_i|, the same form again. Weighted by p_i:   <= 2^-22 (1 + A),  A = sum p_i |z_i|.
  lse = m + log s      |d lse| <= EPS + 2^-22 (1 + A) + u (|log s| + |lse|)  [logf 1 ulp, one add]
                       TOL_LSE = EPS + 2^-22 (2 + A + |log s| + |lse|)
  logprob = x_t - lse  one more rounded subtraction:   TOL_LP = TOL_LSE + 2^-23 (|x_t| + |lse|)
  entropy = log s - t / s,  t = sum e_i z_i (all terms <= 0: a same-sign sum, the chain bound applies relative to |t|)
    t / s = -A carries 2 EPS (both sums), the exponential's error weighted by |z_i| (<= 2^-22 (A + A2), A2 = sum p_i z_i^2) and the
    rescale steps' fma(d, s, t), whose products d_k s_k sum to <= Z s with Z = max |z_i| (the d_k telescope):
                       TOL_ENT = EPS (1 + 2 A) + 2^-22 (2 + A + A2 + Z + |log s| + |entropy|)
  kl = w / s_ref - lse_ref + lse,  w = sum e_ref,i (y_i - x_i), a SIGNED sum: its error scales with Bd = sum p_ref,i |y_i - x_i|
    (the fp64 sum of absolute terms), chain + exponential (Z_ref = max |y_i - m_ref| bounds the exponent error of every term):
                       TOL_KL = TOL_LSE(x) + TOL_LSE(y) + Bd (2 EPS + 2^-22 (2 + Z_ref)) + 2^-22 (|lse| + |lse_ref| + Bd)
  argmax / argmax_ref: comparisons of exact values, no tolerance; the lowest id among the maxima.
The same rules with signed sums scaled by the fp64 sum of absolute terms are what gemm_checks.py / norm_checks.py use."""
import math

import torch

T_LANES = 256
U22, U23 = 2.0 ** -22, 2.0 ** -23


def eps_sum(V: int) -> float:
    return (math.ceil(V / T_LANES) + int(math.log2(T_LANES)) + 8) * U23


def reference(logits: torch.Tensor, targets: torch.Tensor, logits_ref=None) -> dict:
    """logits [rows, V] bf16 (CPU), targets [rows] -> fp64 / int64 [rows] values and tolerances. Computed once per case and shared."""
    x = logits.double()
    rows, V = x.shape
    eps = eps_sum(V)

    def stream(v):
        m = v.amax(-1, keepdim=True)
        z = v - m
        e = z.exp()
        s = e.sum(-1, keepdim=True)
        p = e / s
        ids = torch.arange(V)
        return dict(m=m[:, 0], s=s[:, 0], p=p, lse=(m + s.log())[:, 0], A=(p * z.abs()).sum(-1), A2=(p * z * z).sum(-1),
                    Z=z.abs().amax(-1), logp=z - s.log(),
                    argmax=torch.where(v == m, ids, torch.full_like(ids, V)).amin(-1))

    def tol_lse(a):
        return eps + U22 * (2 + a["A"] + a["s"].log().abs() + a["lse"].abs())
    a = stream(x)
    tg = targets.to(torch.int64)
    ok = (tg >= 0) & (tg < V)
    xt = x.gather(-1, tg.clamp(0, V - 1)[:, None])[:, 0]
    ent = -(a["p"] * a["logp"]).sum(-1)
    r = dict(lse=a["lse"], tol_lse=tol_lse(a), logprob=torch.where(ok, xt - a["lse"], torch.zeros(rows, dtype=torch.float64)),
             argmax=a["argmax"], entropy=ent)
    r["tol_logprob"] = torch.where(ok, r["tol_lse"] + U23 * (xt.abs() + a["lse"].abs()), torch.zeros(rows, dtype=torch.float64))
    r["tol_entropy"] = eps * (1 + 2 * a["A"]) + U22 * (2 + a["A"] + a["A2"] + a["Z"] + a["s"].log().abs() + ent.abs())
    if logits_ref is not None:
        y = logits_ref.double()
        b = stream(y)
        Bd = (b["p"] * (y - x).abs()).sum(-1)
        r["kl"] = (b["p"] * (b["logp"] - a["logp"])).sum(-1)
        r["argmax_ref"] = b["argmax"]
        r["tol_kl"] = r["tol_lse"] + tol_lse(b) + Bd * (2 * eps + U22 * (2 + b["Z"])) + U22 * (a["lse"].abs() + b["lse"].abs() + Bd)
    return r


def check(got: dict, ref: dict, what: str) -> None:
    """got: the tensors of ops.logprob_rows (any device); prints MEASURED worst err / tol per output, then asserts"""
    worst = {}
    for k in ("lse", "logprob", "entropy") + (("kl",) if "kl" in ref else ()):
        err = (got[k].detach().double().cpu() - ref[k]).abs()
        tol = ref["tol_" + k]
        assert bool(torch.isfinite(got[k]).all()), f"{what}: {k} is not finite"
        ratio = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        i = int(ratio.argmax())
        worst[k] = (float(err[i]), float(tol[i]), float(ratio[i]))
    print(f"MEASURED logprob_rows {what}: " + "  ".join(f"{k} err {e:.3g} / tol {t:.3g} = {q:.3f}" for k, (e, t, q) in worst.items()))
    for k, (e, t, q) in worst.items():
        assert q <= 1.0, f"{what}: {k} off by {e:.4g}, tolerance {t:.4g}"
    for k in ("argmax",) + (("argmax_ref",) if "kl" in ref else ()):
        assert torch.equal(got[k].detach().cpu().to(torch.int64), ref[k]), f"{what}: {k} differs"
    if "kl" in ref:
        assert bool((got["kl"].detach().double().cpu() >= -ref["tol_kl"]).all()), f"{what}: kl below -tol"

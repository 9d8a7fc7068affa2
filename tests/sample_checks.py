"""Shared by the sampling tests: the check of ONE sampling step of the device (spider_sample_partial_bf16 + spider_sample_select_f32,
or a decode step of LlamaEngine with do_sample=True) against the fp64 host restatement `spider_amd.llm.sample_token_host`."""
import torch

from spider_amd.llm import sample_token_host

DELTA = 2e-5


def delta():
    """Bound on the relative distance between the device's fp32 masses and the fp64 reference's, derived, not measured. The device
    forms p_j = expf(x_j / T - x_0 / T) for at most 64 candidates and sums them in rank order, all in fp32 (eps = 2^-24 = 6e-8):
      * y = x / T: one rounding each, |y| <= 64 for logits within +-64 at T >= 1 (bf16 logits of a language model stay well inside;
        beyond that the masses that matter have |y_j - y_0| small anyway): 64 * 6e-8 = 3.8e-6 absolute on each y, and the
        difference y_j - y_0 is exact or rounded once more, so <= 2 * 3.8e-6 + 6e-8 absolute in the exponent = the same RELATIVE
        error in p_j: 7.7e-6 at the very edge, about 4e-6 for |y| <= 32;
      * expf: about 2 ulp = 1.2e-7 relative;
      * one fp32 sum of at most 64 non-negative terms in order: <= 63 * 6e-8 = 3.8e-6 relative, typically sqrt(64) * 6e-8;
      * top_p held as fp32 (6e-8 relative), the products top_p * P and u * S: 6e-8 each.
    Sum: <= 1.2e-5 in the worst case; DELTA = 2e-5 leaves a factor below 2 and is 1/50 of the smallest probability step a
    24-bit uniform resolves against a mass of 1e-3."""
    return DELTA


def pack_bits(mask: torch.Tensor) -> torch.Tensor:
    """bool [R, V] -> int32 [R, ceil(V / 32)] holding the uint32 words of the kernels' bitmaps (bit n & 31 of word n >> 5)"""
    R, V = mask.shape
    W = (V + 31) // 32
    m = torch.zeros(R, W * 32, dtype=torch.int64)
    m[:, :V] = mask.long()
    w = (m.view(R, W, 32) << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def near_a_boundary(r: dict, top_p: float, u: float) -> bool:
    """Decided by the fp64 reference r = sample_token_host(...) alone: does a prefix mass lie within DELTA * P of the nucleus threshold
    top_p * P, or u * S within DELTA * S of an inner boundary of the CDF? Only there may the device differ from the reference."""
    d, cum, p = delta(), r["cum"], r["p"]
    P = float(cum[-1])
    if bool((((cum - p)[1:] - top_p * P).abs() <= d * P).any()):       # rank 0 is kept whatever the threshold
        return True
    return r["n_keep"] > 1 and bool(((cum[:r["n_keep"] - 1] - float(u) * r["S"]).abs() < d * r["S"]).any())


def _nucleus_range(r: dict, top_p: float):
    """the sizes of the nucleus that lie within DELTA * P of the reference's threshold"""
    d, cum, p = delta(), r["cum"], r["p"]
    P = float(cum[-1])
    before = cum - p
    return max(1, int((before < top_p * P - d * P).sum())), max(1, int((before < top_p * P + d * P).sum()))


def _token_in_interval(r: dict, n_keep: int, u: float, token: int) -> bool:
    """the token is a kept rank j of a nucleus of n_keep ranks, and u * S lies within DELTA * S of [cum[j - 1], cum[j])"""
    d, cum = delta(), r["cum"]
    cand = r["tokens"][:n_keep].tolist()
    if int(token) not in cand:
        return False
    j = cand.index(int(token))
    S = float(cum[n_keep - 1])
    t = float(u) * S
    left = float(cum[j - 1]) if j else 0.0
    return left - d * S <= t and (t < float(cum[j]) + d * S or j == n_keep - 1)


def check_sample_token(x, temperature, top_k, top_p, u_want, token) -> dict:
    """The check of `check_sample_step` where only the drawn token is known (a decode step of the engine, recomputed from the
    returned raw logits): some admissible nucleus size puts u * S within DELTA * S of the token's interval; away from every
    boundary the token is the reference's own. Returns the reference."""
    r = sample_token_host(x, temperature, top_k, top_p, u_want)
    lo, hi = _nucleus_range(r, top_p)
    assert any(_token_in_interval(r, n, u_want, token) for n in range(lo, hi + 1)), (int(token), r["token"], lo, hi, u_want)
    if not near_a_boundary(r, top_p, u_want):
        assert int(token) == r["token"], (int(token), r["token"])
    return r


def check_sample_step(x, temperature, top_k, top_p, u_want, cand_tok, cand_p, n_keep, u, token):
    """x [V]: the row's PROCESSED logits (fp32, process_logits_host); u_want = sample_uniform_host(seed, row, step); the rest is what
    the device wrote for the row (cand_tok / cand_p [64], n_keep, u, the token). Asserts
      * u is the definition's uniform, bit for bit;
      * the ranked candidates are the reference's, in order (a selection on fp32 values: exact), -1 / 0 behind them;
      * every p_j within DELTA (p_j <= p_0 = 1);
      * n_keep is the reference's; where some prefix mass lies within DELTA * P of top_p * P either neighbour is accepted;
      * the token is a kept rank j, and u * S lies within DELTA * S of [cum[j - 1], cum[j]) (S = the mass of the device's n_keep).
    Where `near_a_boundary` is False the device's n_keep and token must be the reference's own."""
    d = delta()
    r = sample_token_host(x, temperature, top_k, top_p, u_want)
    kk = r["tokens"].numel()
    assert float(u) == float(u_want), (float(u), u_want)
    assert cand_tok[:kk].tolist() == r["tokens"].tolist(), (cand_tok[:kk].tolist(), r["tokens"].tolist())
    assert (cand_tok[kk:] == -1).all() and (cand_p[kk:] == 0).all()
    assert (cand_p[:kk].double() - r["p"]).abs().max() <= d, (cand_p[:kk], r["p"])
    lo, hi = _nucleus_range(r, top_p)
    n_keep = int(n_keep)
    assert lo <= n_keep <= hi, (n_keep, lo, hi, r["n_keep"])
    assert _token_in_interval(r, n_keep, u_want, token), (int(token), r["token"], n_keep, u_want)
    if not near_a_boundary(r, top_p, u_want):
        assert n_keep == r["n_keep"] and int(token) == r["token"]

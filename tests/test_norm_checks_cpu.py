"""CPU tests of tests/norm_checks.py: the derived GroupNorm bounds get their teeth before any GPU is involved.

The GroupNorm statistics of csrc/unet_ops.hip are replayed in torch fp32 in the order the kernel comments document (gn_stats_kernel:
a thread owns an 8-channel vector and every KP-th pixel of its chunk, pixel lanes are summed through LDS, then the channels of a
group; gn_apply_kernel: nthr / G parts walk the chunks with stride `parts`, then the parts are summed; a_c = rstd gamma,
b_c = beta - mean a_c, y = fma(x, a_c, b_c)). Two formats are replayed: the public one-pass (sum, sum of squares) and the private
centred (mean, M2) format the own-pass entry points use (a thread sums about its own first value; lanes, channels and chunks are
merged by Chan's formula with the means kept as offsets from a pivot of the group).

* the `onepass` bound holds for the one-pass replay at every mean / sigma in {0, 4, 16, 64, 256}; the `centered` bound for the
  centred replay;
* the one-pass replay breaks the `centered` bound from 16 upwards and the mean-blind e_s of gemm_checks.pre_gn_in from 64 upwards --
  what makes the sweep worth having;
* statistics over one channel too few, over a group shifted by one channel across a seam, or with the last pixel chunk dropped land
  outside the bound at every sweep point.
"""
import pytest
import torch

import norm_checks as nc

SWEEP = [0, 4, 16, 64, 256]
C, G, EPS = 320, 32, 1e-5
DT = torch.float16                     # format of gamma / beta; the replayed value is the fp32 one before any 16-bit rounding


def f32(x):
    return x.to(torch.float32)


def fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in fp64"""
    return f32(a.double() * b.double() + c.double())


def gn_nchunk(HW):
    return min(max(HW // 32, 1), 128)


def replay_stats(x, groups, centered):
    """gn_stats_kernel on one image x [HW, C] fp32 -> partial [nchunk, G, 2] fp32"""
    HW, Cn = x.shape
    cpg, cv = Cn // groups, Cn // 8
    KP = max(256 // cv, 1)
    nchunk = gn_nchunk(HW)
    per = (HW + nchunk - 1) // nchunk
    out = torch.zeros(nchunk, groups, 2)
    for k in range(nchunk):
        p0, p1 = k * per, min(HW, k * per + per)
        if p0 >= p1:
            continue
        z, npix = x[p0:p1], p1 - p0
        if not centered:
            s, q = torch.zeros(KP, Cn), torch.zeros(KP, Cn)
            for i in range(0, npix, KP):                                # pixel p0 + i + lane belongs to `lane`
                rows = z[i:i + KP]
                s[:len(rows)] = s[:len(rows)] + rows
                q[:len(rows)] = fma(rows, rows, q[:len(rows)])
            ts, tq = torch.zeros(Cn), torch.zeros(Cn)
            for lane in range(KP):
                ts, tq = ts + s[lane], tq + q[lane]
            gs, gq = torch.zeros(groups), torch.zeros(groups)
            for c in range(cpg):
                gs, gq = gs + ts.view(groups, cpg)[:, c], gq + tq.view(groups, cpg)[:, c]
            out[k, :, 0], out[k, :, 1] = gs, gq
            continue
        # centred: a lane sums about its own first pixel, then (mean - group pivot, M2) merged by Chan's formula
        nl = min(KP, npix)                                              # lanes that own a pixel
        cnt = torch.tensor([(npix - l + KP - 1) // KP for l in range(nl)], dtype=torch.float32)
        first = z[:nl]
        pg = z[0, ::cpg].clone()                                        # the group's first channel at the chunk's first pixel
        s, q = torch.zeros(nl, Cn), torch.zeros(nl, Cn)
        for i in range(0, npix, KP):
            rows = z[i:i + KP]
            w = rows - first[:len(rows)]
            s[:len(rows)] = s[:len(rows)] + w
            q[:len(rows)] = fma(w, w, q[:len(rows)])
        dm = s * (1.0 / cnt)[:, None]
        m2 = fma(-s, dm, q).clamp_min(0)
        mu = (first - pg.repeat_interleave(cpg)) + dm
        ts, tq, na = torch.zeros(Cn), torch.zeros(Cn), 0.0
        for lane in range(nl):
            nb = float(cnt[lane])
            d, wgt = mu[lane] - ts, f32(torch.tensor(nb)) / f32(torch.tensor(na + nb))
            ts = fma(d, wgt.expand_as(d), ts)
            tq = tq + fma(d * d, (f32(torch.tensor(na)) * wgt).expand_as(d), m2[lane])
            na += nb
        # channels of a group hold npix values each: mean of the means (summed relative to the first one's), M2_c + npix (m_c - m)^2
        tsg, tqg = ts.view(groups, cpg), tq.view(groups, cpg)
        m0 = tsg[:, 0]
        gs, gq, dv = torch.zeros(groups), torch.zeros(groups), torch.zeros(groups)
        for i in range(cpg):
            gs, gq = gs + (tsg[:, i] - m0), gq + tqg[:, i]
        gs = gs * f32((1.0 / torch.tensor(float(cpg), dtype=torch.float64)))
        for i in range(cpg):
            d = (tsg[:, i] - m0) - gs
            dv = fma(d, d, dv)
        gq = fma(torch.full_like(dv, float(npix)), dv, gq)
        out[k, :, 0], out[k, :, 1] = pg + (gs + m0), gq
    return out


def replay_apply(x, part, gamma, beta, groups, eps, centered):
    """gn_apply_kernel's statistics prologue and fma on one image -> the fp32 value before any 16-bit rounding"""
    HW, Cn = x.shape
    cpg, cv = Cn // groups, Cn // 8
    nthr = cv * max(256 // cv, 1)
    parts = nthr // groups
    nchunk = part.shape[0]
    per = (HW + nchunk - 1) // nchunk
    P = part[0, :, 0]
    ps, pq = torch.zeros(parts, groups), torch.zeros(parts, groups)
    for p in range(parts):
        for c in range(p, nchunk, parts):
            if centered:
                nk = float(max(min(HW, (c + 1) * per) - c * per, 0) * cpg)
                d = part[c, :, 0] - P
                ps[p] = fma(torch.full_like(d, nk), d, ps[p])
                pq[p] = pq[p] + fma(nk * d, d, part[c, :, 1])
            else:
                ps[p], pq[p] = ps[p] + part[c, :, 0], pq[p] + part[c, :, 1]
    gs, gq = torch.zeros(groups), torch.zeros(groups)
    for p in range(parts):
        gs, gq = gs + ps[p], gq + pq[p]
    n = float(HW * cpg)
    if centered:
        dm = gs / n
        mu, var = P + dm, (fma(-gs, dm, gq) / n).clamp_min(0)
    else:
        mu = gs / n
        var = fma(-mu, mu, gq / n).clamp_min(0)
    rstd = f32((var + eps).double().rsqrt())
    ca = rstd.repeat_interleave(cpg) * f32(gamma)
    cb = fma(-mu.repeat_interleave(cpg), ca, f32(beta))
    return fma(x, ca, cb)


@pytest.fixture(scope="module", params=[64, 1024, 4096], ids=lambda hw: f"HW{hw}")
def sweep(request):
    """per sweep point: the input, the fp64 problem and both replays, computed once"""
    HW = request.param
    gen = torch.Generator().manual_seed(100 + HW)
    gamma = (1 + 0.1 * torch.randn(C, generator=gen)).to(DT)
    beta = (0.1 * torch.randn(C, generator=gen)).to(DT)
    out = {}
    for r in SWEEP:
        x = nc.shifted_input(gen, 1, HW, C, G, 1.0, r)
        g = nc.gn64(x, gamma, beta, G, EPS)
        y = {cen: replay_apply(x[0], replay_stats(x[0], G, cen), gamma, beta, G, EPS, cen)[None] for cen in (False, True)}
        out[r] = (x, g, y)
    return HW, gamma, beta, out


@pytest.mark.parametrize("r", SWEEP)
def test_onepass_bound_holds_for_the_onepass_replay(sweep, r):
    HW, _, _, out = sweep
    _, g, y = out[r]
    nc.check(f"one-pass replay HW={HW} mean/sigma={r}", y[False], nc.norm_ref(g, "onepass", DT, "f32in"), DT, fp32_out=True)


@pytest.mark.parametrize("r", SWEEP)
def test_centered_bound_holds_for_the_centered_replay(sweep, r):
    HW, _, _, out = sweep
    _, g, y = out[r]
    nc.check(f"centred replay HW={HW} mean/sigma={r}", y[True], nc.norm_ref(g, "centered", DT, "f32in"), DT, fp32_out=True)


@pytest.mark.parametrize("r", [16, 64, 256])
def test_onepass_replay_breaks_the_centered_bound(sweep, r):
    """what the own-pass routes were before they were centred: outside the bound they are held to now"""
    HW, _, _, out = sweep
    _, g, y = out[r]
    ratio, l2 = nc.ratio(y[False], nc.norm_ref(g, "centered", DT, "f32in"), DT, True)
    print(f"one-pass replay against the centred bound, HW={HW} mean/sigma={r}: err / tol = {ratio:.1f}, rel L2 = {l2:.2e}")
    assert ratio > 1.0


@pytest.mark.parametrize("r", [64, 256])
def test_mean_blind_e_s_fails_from_64(sweep, r):
    """gemm_checks.pre_gn_in's e_s (a relative error on mean / rstd, plus the same fp32 rounding terms the derived bound has) does not
    contain the one-pass statistics once the mean dominates"""
    HW, _, _, out = sweep
    _, g, y = out[r]
    a_c = g.rstd * g.gamma
    tol = nc.blind_tol(g) + 4 * nc.E32 * ((g.x * a_c).abs() + (g.mean * a_c).abs() + g.beta.abs())
    err = (y[False].double().reshape(g.x.shape) - g.aff).abs()
    ratio = float((err / tol).max())
    print(f"one-pass replay against the mean-blind e_s, HW={HW} mean/sigma={r}: err / tol = {ratio:.1f}")
    assert ratio > 1.0


def wrong_stats(g, kind):
    """fp64 GroupNorm of g.x with statistics over the wrong set of values -> [B, HW, G, C / G]"""
    x = g.x
    B, HW, Gn, cpg = x.shape
    if kind == "one_channel_short":
        sel = x[..., :cpg - 1]
    elif kind == "seam_shift":                     # channels [g cpg + 1, (g + 1) cpg + 1): one from the next group (the last wraps)
        flat = x.reshape(B, HW, Gn * cpg)
        sel = torch.roll(flat, -1, dims=2).reshape(B, HW, Gn, cpg)
    elif kind == "last_chunk_dropped":
        nchunk = gn_nchunk(HW)
        per = (HW + nchunk - 1) // nchunk
        sel = x[:, :(nchunk - 1) * per]
    else:
        raise ValueError(kind)
    mean = sel.mean((1, 3), keepdim=True)
    var = ((sel - mean) ** 2).mean((1, 3), keepdim=True)
    return (x - mean) * (var + g.eps).rsqrt() * g.gamma + g.beta


@pytest.mark.parametrize("kind", ["one_channel_short", "seam_shift", "last_chunk_dropped"])
@pytest.mark.parametrize("r", SWEEP)
def test_wrong_statistics_land_outside_the_bound(sweep, r, kind):
    """the looser of the two models (`onepass`) still rejects every wrong set of values, even where it is widest"""
    HW, _, _, out = sweep
    _, g, _ = out[r]
    for model in ("onepass", "centered"):
        R = nc.norm_ref(g, model, DT, "f32in")
        ratio, _ = nc.ratio(wrong_stats(g, kind), R, DT, True)
        print(f"{kind} HW={HW} mean/sigma={r} against {model}: err / tol = {ratio:.1f}")
        assert ratio > 1.0, (kind, model, ratio)
        with pytest.raises(AssertionError):
            nc.check(f"{kind} (must fail)", wrong_stats(g, kind), R, DT, fp32_out=True)


def test_forms_add_the_roundings_they_name():
    """16-bit form: one rounding of the result (two with SiLU); f32in: none before the output's own; split: second order only"""
    gen = torch.Generator().manual_seed(7)
    x = nc.shifted_input(gen, 1, 64, 64, 8, 2.0, 4).to(DT)
    gamma, beta = (1 + 0.1 * torch.randn(64, generator=gen)).to(DT), (0.1 * torch.randn(64, generator=gen)).to(DT)
    g = nc.gn64(x, gamma, beta, 8, EPS)
    for silu in (False, True):
        v = nc.act64("silu", g.aff) if silu else g.aff
        once = v.to(DT)                                          # the exact value rounded once: inside every 16-bit bound
        for form in ("16", "f32in"):
            nc.check(f"exact, rounded once ({form})", once, nc.norm_ref(g, "centered", DT, form, silu), DT, fp32_out=False)
        hi = v.to(DT)
        lo = (v - hi.double()).to(DT)
        R = nc.norm_ref(g, "centered", DT, "split", silu)
        nc.check("exact, split", hi.double() + lo.double(), R, DT, fp32_out=True)
        with pytest.raises(AssertionError):                      # the split form has no room for a first-order rounding
            nc.check("hi alone (must fail)", hi, R, DT, fp32_out=True)

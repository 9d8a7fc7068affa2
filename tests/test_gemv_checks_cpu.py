"""CPU tests of tests/gemv_checks.py: the derived bounds of the decode projections get their teeth before any GPU is involved.

THE REPLAY is fp32 with each product formed exactly (in fp64) and then rounded into the fp32 accumulator:
* GEMV (gemv_kernel, lmhead_partial_kernel): a lane sums its 8-element chunks at k = 8 lane + 512 u in order, then the 64 lanes are
  combined in the xor order of wave_sum (32, 16, 8, 4, 2, 1);
* MFMA kernels (skinny_gemm_kernel, skinny_fm_kernel): each wave's share [kb0, kb1) of K / 64 is summed in k order, then the 8
  partials are added in wave order. These kernels need K % 64 == 0, so their replay runs at K rounded down to a multiple of 64
  (64, 1024, 8192, 18944).
Followed by the epilogue's documented roundings, the replay is inside the bound of every form at K = 64, 1032, 8200 and 18944.

PLANTED FAULTS are formed in fp64 and rounded as the epilogue rounds, so that nothing but the fault separates them from the
reference. Each must land outside the bound at every K; where only a share of the elements is caught the share the run shows is
asserted (never zero). One exception is arithmetic, not a choice: `rs` over K - 8 elements changes the result by 4 / K of itself,
which is below one bf16 rounding (u = 2^-8) from K = 1032 on, so no bf16 output can show it there. It is caught at every K where
the format lets it be caught: on the fp32 value of the folded form ahead of its last rounding (bound c q rs + (c/2 + 2^-22) |ref|),
and on the bf16 outputs at K = 64; the shares on the bf16 outputs at larger K are printed.
"""
import pytest
import torch

import gemv_checks as gv
from gemm_checks import bound

BF = torch.bfloat16
KS = [64, 1032, 8200, 18944]
B, N, I = 2, 37, 20
EPS = gv.EPS


def f32(x):
    return x.to(torch.float32)


def bf(x):
    """one correct rounding to bf16, returned in fp64"""
    return x.to(torch.float32).to(BF).double()


def acc_step(acc, a, b):
    """fp32 accumulator += exact product"""
    return f32(acc.double() + a.double() * b.double())


def replay_gemv(x, W):
    """[B, K] x [N, K] -> [B, N] fp32 in the lane order of gemv_kernel"""
    Bn, K = x.shape
    Kp = (K + 511) // 512 * 512
    xp, Wp = torch.zeros(Bn, Kp, dtype=torch.float64), torch.zeros(W.shape[0], Kp, dtype=torch.float64)
    xp[:, :K], Wp[:, :K] = x.double(), W.double()                    # lanes past the end add nothing (the kernel skips them)
    xc, Wc = xp.view(Bn, 1, Kp // 512, 64, 8), Wp.view(1, -1, Kp // 512, 64, 8)
    acc = torch.zeros(Bn, W.shape[0], 64)
    for u in range(Kp // 512):
        for j in range(8):
            acc = acc_step(acc, xc[:, :, u, :, j], Wc[:, :, u, :, j])
    lanes = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def replay_mfma(x, W, drop_wave=None):
    """the K split of the skinny MFMA kernels: 8 waves, wave w sums k blocks [w nkb / 8, (w + 1) nkb / 8) in order"""
    Bn, K = x.shape
    assert K % 64 == 0
    nkb = K // 64
    xd, Wd = x.double(), W.double()
    tot = torch.zeros(Bn, W.shape[0])
    for w in range(8):
        part = torch.zeros(Bn, W.shape[0])
        for k in range(w * nkb // 8 * 64, (w + 1) * nkb // 8 * 64):
            part = acc_step(part, xd[:, k, None], Wd[None, :, k])
        if w != drop_wave:
            tot = tot + part
    return tot


def sumsq32(x):
    """fp32 sum of squares of each row, 256 strided partial sums then a tree (the bound covers any order)"""
    Bn, K = x.shape
    Kp = (K + 255) // 256 * 256
    xp = torch.zeros(Bn, Kp)
    xp[:, :K] = x.float()
    acc = torch.zeros(Bn, 256)
    for i in range(Kp // 256):
        acc = acc_step(acc, xp[:, i * 256:(i + 1) * 256], xp[:, i * 256:(i + 1) * 256])
    n = 256
    while n > 1:
        n //= 2
        acc = acc[:, :n] + acc[:, n:2 * n]
    return acc[:, 0:1]


def rs32(x, eps):
    K = x.shape[-1]
    return f32((f32(sumsq32(x) / K) + eps).double().rsqrt())


def stage_norm(x, nw, eps):
    """norm_vec: bf16(bf16(x * rs) * norm_w) with rs in fp32"""
    return (f32(x.float() * rs32(x, eps)).to(BF).float() * nw.float()).to(BF)


def epi_plain(acc, bias=None, res=None):
    """(+bias) -> bf16 -> (+res -> bf16), fp32 in between"""
    v = acc if bias is None else f32(acc + bias.float())
    if res is not None:
        v = f32(v.to(BF).float() + res.float())
    return v.to(BF)


def silu32(g):
    return f32(g.double() * torch.sigmoid(g.double()))


def epi_glu(acc):
    g, u = acc[:, :acc.shape[1] // 2].to(BF).float(), acc[:, acc.shape[1] // 2:].to(BF).float()
    return f32(silu32(g).to(BF).float() * u).to(BF)


@pytest.fixture(scope="module", params=KS, ids=lambda k: f"K{k}")
def prob(request):
    """one problem per K: operands, replays and references, computed once"""
    K = request.param
    Km = K // 64 * 64
    W, bias, nw = gv.weights(N, K)
    Wgu = gv.weights(2 * I, K, seed=21)[0]
    x, res = (t[:B] for t in gv.acts(K, N))
    x3 = gv.acts(K, N, 3.0)[0][:B]
    return dict(K=K, Km=Km, W=W, bias=bias, nw=nw, Wgu=Wgu, x=x, res=res, x3=x3,
                acc=replay_gemv(x, W), acc_gu=replay_gemv(x, Wgu))


def inside(what, got, R, fp32_out=False):
    gv.check(what, got, R, BF, fp32_out)


def test_replay_inside_plain_bias_res(prob):
    p = prob
    inside("replay plain", epi_plain(p["acc"]), gv.ref_gemv(p["x"], p["W"]))
    inside("replay bias", epi_plain(p["acc"], p["bias"]), gv.ref_gemv(p["x"], p["W"], bias=p["bias"]))
    inside("replay bias+res", epi_plain(p["acc"], p["bias"], p["res"]), gv.ref_gemv(p["x"], p["W"], bias=p["bias"], res=p["res"]))
    inside("replay plain fp32", p["acc"], gv.ref_gemv(p["x"], p["W"]), fp32_out=True)


def test_replay_inside_gate_up(prob):
    p = prob
    inside("replay gate/up", epi_glu(p["acc_gu"]), gv.ref_swiglu(p["x"], p["Wgu"]))


def test_replay_inside_fused_norm(prob):
    p = prob
    xs = stage_norm(p["x"], p["nw"], EPS)
    inside("replay norm", epi_plain(replay_gemv(xs, p["W"])), gv.ref_gemv(p["x"], p["W"], norm_w=p["nw"], eps=EPS))
    inside("replay norm gate/up", epi_glu(replay_gemv(xs, p["Wgu"])), gv.ref_swiglu(p["x"], p["Wgu"], norm_w=p["nw"], eps=EPS))


def test_replay_inside_mfma_and_folded_norm(prob):
    p = prob
    Km = p["Km"]
    x, x3, W, Wgu, nw = p["x"][:, :Km], p["x3"][:, :Km], p["W"][:, :Km], p["Wgu"][:, :Km], p["nw"][:Km]
    acc = replay_mfma(x, W)
    inside("replay mfma plain", epi_plain(acc), gv.ref_gemv(x, W))
    inside("replay mfma bias+res", epi_plain(acc, p["bias"], p["res"]), gv.ref_gemv(x, W, bias=p["bias"], res=p["res"]))
    inside("replay mfma gate/up", epi_glu(replay_mfma(x, Wgu)), gv.ref_swiglu(x, Wgu))
    rs = rs32(x3, EPS)
    accf = f32(replay_mfma(x3, gv.fold_weight(W, nw)) * rs)
    inside("replay folded norm fp32", accf, gv.ref_gemv(x3, W, norm_w=nw, eps=EPS, fold=True), fp32_out=True)
    inside("replay folded norm", epi_plain(accf, p["bias"], p["res"]),
           gv.ref_gemv(x3, W, bias=p["bias"], res=p["res"], norm_w=nw, eps=EPS, fold=True))
    accg = f32(replay_mfma(x3, gv.fold_weight(Wgu, nw)) * rs)
    inside("replay folded norm gate/up", epi_glu(accg), gv.ref_swiglu(x3, Wgu, norm_w=nw, eps=EPS, fold=True))


@pytest.mark.parametrize("scale", [1e-3, 1.0, 300.0])
@pytest.mark.parametrize("H", [8, 64, 2056, 8192])
def test_replay_inside_rmsnorm(H, scale):
    x, r = gv.draw(3, 3, H, scale=scale), gv.draw(4, 3, H, scale=scale)
    w = (1 + 0.1 * gv.draw(5, H).float()).to(BF)
    for h in (x, gv.add_bf16(x, r)):
        y = (f32(h.float() * rs32(h, EPS)).to(BF).float() * w.float()).to(BF)
        inside(f"replay rmsnorm H={H} scale={scale}", y, gv.ref_rmsnorm(h, w, EPS))
    # without the weight it is outside
    assert outside(bf(x.double() * gv.rs64(x, EPS)), gv.ref_rmsnorm(x, w, EPS)) > 0.5


# ------------------------------------------------------------------------------------------------ planted faults
def outside(got, R, fp32_out=False, sel=None):
    """share of the (selected) elements outside the bound"""
    err = (got.double().reshape(R.ref.shape) - R.ref).abs()
    bad = err > bound(R, BF, fp32_out)
    if sel is not None:
        bad = bad[sel]
    return float(bad.double().mean())


def test_fault_last_chunk_dropped(prob):
    p = prob
    x0 = p["x"].clone()
    x0[:, -8:] = 0
    s = outside(bf(x0.double() @ p["W"].double().T), gv.ref_gemv(p["x"], p["W"]))
    sb = outside(epi_plain(f32(x0.double() @ p["W"].double().T), p["bias"], p["res"]).double(),
                 gv.ref_gemv(p["x"], p["W"], bias=p["bias"], res=p["res"]))
    print(f"last chunk dropped K={p['K']}: outside plain {s:.2f}, bias+res {sb:.2f}")
    assert s >= 0.85 and sb >= 0.5


def test_fault_one_wave_share_dropped(prob):
    p = prob
    Km = p["Km"]
    x, W = p["x"][:, :Km], p["W"][:, :Km]
    nkb = Km // 64
    k0, k1 = 7 * nkb // 8 * 64, Km                       # wave 7 always owns a block
    x0 = x.clone()
    x0[:, k0:k1] = 0
    s = outside(bf(x0.double() @ W.double().T), gv.ref_gemv(x, W))
    print(f"wave 7's share dropped K={Km}: outside {s:.2f}")
    assert s >= 0.9


def test_fault_bias_of_previous_row_on_last_row(prob):
    p = prob
    b2 = p["bias"].clone()
    b2[-1] = p["bias"][-2]
    assert float((b2[-1] - p["bias"][-1]).abs()) > 0.1            # the operands make the fault a fault
    got = bf(p["x"].double() @ p["W"].double().T + b2.double())
    sel = torch.zeros(B, N, dtype=torch.bool)
    sel[:, -1] = True
    assert outside(got, gv.ref_gemv(p["x"], p["W"], bias=p["bias"]), sel=sel) == 1.0


def test_fault_residual_of_previous_sequence(prob):
    p = prob
    got = bf(bf(p["x"].double() @ p["W"].double().T + p["bias"].double()) + torch.roll(p["res"], 1, 0).double())
    s = outside(got, gv.ref_gemv(p["x"], p["W"], bias=p["bias"], res=p["res"]))
    print(f"residual of sequence b-1 K={p['K']}: outside {s:.2f}")
    assert s >= 0.95


def test_fault_up_row_read_from_gate_half(prob):
    p = prob
    g = bf(p["x"].double() @ p["Wgu"][:I].double().T)
    got = bf(bf(g * torch.sigmoid(g)) * g)
    s = outside(got, gv.ref_swiglu(p["x"], p["Wgu"]))
    print(f"up read from the gate half K={p['K']}: outside {s:.2f}")
    assert s >= 0.9


def test_fault_clamped_duplicate_written_into_row_N(prob):
    """the wave whose second row is clamped to N - 1 stores it at [b, N] = the flat position of [b + 1, 0]"""
    p = prob
    got = bf(p["x"].double() @ p["W"].double().T)
    got.view(-1)[N] = got[0, N - 1]
    sel = torch.zeros(B, N, dtype=torch.bool)
    sel[1, 0] = True
    assert outside(got, gv.ref_gemv(p["x"], p["W"]), sel=sel) == 1.0


def short_rs(x, eps):
    """rsqrt(sum over the first K - 8 elements / K + eps)"""
    x = x.double()
    return ((x[:, :-8] ** 2).sum(-1, keepdim=True) / x.shape[-1] + eps).rsqrt()


def test_fault_rs_over_K_minus_8(prob):
    p = prob
    K, Km = p["K"], p["Km"]
    x3, W, nw = p["x3"][:, :Km], p["W"][:, :Km], p["nw"][:Km]
    Wf = gv.fold_weight(W, nw)
    R = gv.ref_gemv(x3, W, norm_w=nw, eps=EPS, fold=True)
    v = (x3.double() @ Wf.double().T) * short_rs(x3, EPS)
    s32 = outside(v, R, fp32_out=True)
    s16 = outside(bf(v), R)
    srow = outside(bf(bf(bf(p["x"].double() * short_rs(p["x"], EPS)) * p["nw"].double()) @ p["W"].double().T),
                   gv.ref_gemv(p["x"], p["W"], norm_w=p["nw"], eps=EPS))
    print(f"rs over K-8 K={K}: outside folded fp32 {s32:.2f}, folded bf16 {s16:.2f}, row-major bf16 {srow:.2f}")
    assert s32 >= 0.75, "a 4 / K change of rs must show on the fp32 value of the folded form at every K"
    if 4.0 / K > gv.U[BF]:                                # the shift exceeds one bf16 rounding: K = 64 only (4 / 1032 < 2^-8)
        assert s16 >= 0.9 and srow >= 0.5


def test_fault_norm_weights_not_applied(prob):
    p = prob
    xn = bf(p["x"].double() * gv.rs64(p["x"], EPS))
    s = outside(bf(xn @ p["W"].double().T), gv.ref_gemv(p["x"], p["W"], norm_w=p["nw"], eps=EPS))
    Km = p["Km"]
    x3, W, nw = p["x3"][:, :Km], p["W"][:, :Km], p["nw"][:Km]
    sf = outside(bf((x3.double() @ W.double().T) * gv.rs64(x3, EPS)), gv.ref_gemv(x3, W, norm_w=nw, eps=EPS, fold=True))
    print(f"norm weights not applied K={p['K']}: outside row-major {s:.2f}, folded {sf:.2f}")
    assert s >= 0.5 and sf >= 0.85


# ------------------------------------------------------------------------------------------------ the case table
def test_table_routes_are_the_expected_ones():
    for c in gv.TABLE:
        assert gv.route(c.entry, c.B, c.N, c.K, c.norm) == c.route, c


def test_table_covers_every_required_instantiation():
    reached = {c.route for c in gv.TABLE}
    missing = [r for r in gv.REQUIRED if r not in reached]
    assert not missing, missing
    # both schedules of every gemv_kernel case exist as instantiations of their own (SCHED 0 through spider_set_gemv_sched(0))
    for c in gv.TABLE:
        if c.route[0] == "gemv_kernel":
            assert gv.route(c.entry, c.B, c.N, c.K, c.norm, sched=0) == c.route[:6] + (0,)
    stage = {(c.B, c.route[5], c.K, c.norm): gv.staging(c.B, c.route[5], c.K, c.norm) for c in gv.TABLE if c.route[0] == "gemv_kernel"}
    for key, form in gv.REQUIRED_STAGING.items():
        assert stage.get(key) == form, (key, stage.get(key), form)


def test_r2_threshold():
    assert gv.route("gemv", 1, 6144, 4096, False) == ("gemv_kernel", 1, 2, False, True, 4, 1)
    assert gv.route("gemv", 1, 6143, 4096, False) == ("gemv_kernel", 1, 1, False, True, 4, 1)
    assert gv.route("gemv", 1, 1329, 18944, False)[2] == 2 and gv.route("gemv", 1, 1328, 18944, False)[2] == 1


def test_route_edges():
    assert gv.route("gemv", 8, 64, 18944, False) == ("skinny_gemm_kernel", False, 8)      # test_hip_ops.py::test_gemv's (8, 64, 18944)
    assert gv.route("gemv", 4, 37, 8192, True)[4] is True
    with pytest.raises(ValueError, match="fused RMSNorm needs"):
        gv.route("gemv", 4, 37, 8200, True)
    with pytest.raises(ValueError):
        gv.route("gemv", 9, 37, 1032, False)
    with pytest.raises(ValueError):
        gv.route("gemv_swiglu_fm", 2, 24, 64, False)
    assert gv.staging(1, 4, 8192, False) == "plain-1" and gv.staging(1, 4, 4096, True) == "norm-regs"
    assert gv.staging(1, 8, 24576, False) == "plain-1"
    nparts, per = gv.lm_rows_per_block(131073)
    assert (nparts, per) == (2048, 65) and nparts - (131073 + per - 1) // per == 31


@pytest.mark.parametrize("c", gv.cases("lm") + gv.cases("lm_fm"), ids=lambda c: f"{c.entry}-B{c.B}-V{c.N}-K{c.K}-{'norm' if c.norm else 'plain'}")
def test_planted_winners_pass_the_margin(c):
    fm = c.entry.endswith("_fm")
    W, x, nw, rows, R = gv.lm_case(c.N, c.K, c.B, c.norm, fm, 3.0 if fm and c.norm else 1.0)      # asserts the margins
    assert len(set(rows)) == c.B and R.ref.shape == (c.B, c.N)
    if c.B >= 5:
        per = 16 if fm else gv.lm_rows_per_block(c.N)[1]
        nblk = (c.N + per - 1) // per
        assert rows[:4] == [0, c.N - 1, per - 1, (nblk - 1) * per] and (rows[4] % per) % 2 == 1

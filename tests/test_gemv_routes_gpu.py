"""GPU: the bf16 decode projections of csrc/llm_decode.hip (gemv, gemv_swiglu, gemv_fm, gemv_swiglu_fm, lm_head_argmax, lm_head_argmax_fm,
rmsnorm) against fp64 within the derived bounds of tests/gemv_checks.py, over every route of their dispatch that shapes alone reach:
gemv_kernel at 5..8 rows, with the activations read through L2, with two rows per wave (the 48 MiB threshold, odd N), with every
batch loop of the staging; skinny_gemm_kernel and skinny_fm_kernel at every row count class, with uneven K shares, ragged N and the
folded RMSNorm; the lm_head kernels with planted winners at the block edges and with ties inside a wave, a block and across blocks.

The cases and the route each is expected to take come from gemv_checks.TABLE (tests/test_gemv_checks_cpu.py asserts that the table
reaches every instantiation through gemv_checks.route, a restatement of the dispatch). Every gemv_kernel case runs under both
settings of spider_set_gemv_sched: the outputs must be bit-identical and the schedule-1 output is held to the bound. Outputs are
written into the front of a sentinel-filled buffer whose tail must survive. Every element must be inside its bound.
"""
import pytest
import torch

import gemv_checks as gv

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EPS = gv.EPS
SENT = -77.0


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


def both(fn):
    """fn() under schedule 0 and under schedule 1 (previous setting restored); asserts the setter returns what was set"""
    from spider_amd import lib as slib
    lib = slib.load()
    prev = lib.spider_set_gemv_sched(0)
    try:
        y0 = fn().clone()
        assert lib.spider_set_gemv_sched(1) == 0
        y1 = fn().clone()
        assert lib.spider_set_gemv_sched(1) == 1
    finally:
        lib.spider_set_gemv_sched(prev)
    assert torch.equal(y0, y1), f"schedules differ in {int((y0 != y1).sum())} / {y0.numel()} elements"
    return y1


def once(fn):
    return fn().clone()


def guarded(dev, B, N, call):
    """call(out) with out = the first B * N elements of a sentinel-filled buffer; the 64 elements behind it must survive"""
    buf = torch.full((B * N + 64,), SENT, dtype=BF, device=dev)
    y = call(buf[:B * N].view(B, N))
    assert bool((buf[B * N:] == SENT).all()), "the kernel wrote behind its output"
    return y


def tag(route, form):
    return "/".join(str(int(v)) if isinstance(v, bool) else str(v) for v in route) + " | " + form


def run_gemv_case(ops, dev, c, run=both, cols=None, W=None, bias=None, nw=None):
    """one `gemv` row of the table: plain and + bias + res (c.norm False) or the fused norm (c.norm True); cols: check that subset"""
    if W is None:
        W, bias, nw = gv.weights(c.N, c.K)
    x, res = (t[:c.B] for t in gv.acts(c.K, c.N))
    Wd, xd = W.to(dev), x.to(dev)
    sub = (lambda t: t) if cols is None else (lambda t: t[..., cols])
    Ws, bs, rs_ = (W, bias, res) if cols is None else (W[cols], bias[cols], res[:, cols])

    def fin(y):
        assert bool(torch.isfinite(y.float()).all())
        return sub(y)
    if c.norm:
        nd = nw.to(dev)
        y = run(lambda: guarded(dev, c.B, c.N, lambda o: ops.gemv(Wd, xd, norm_w=nd, eps=EPS, out=o)))
        gv.check(tag(c.route, "norm"), fin(y), gv.ref_gemv(x, Ws, norm_w=nw, eps=EPS), BF, False)
        return
    y = run(lambda: guarded(dev, c.B, c.N, lambda o: ops.gemv(Wd, xd, out=o)))
    gv.check(tag(c.route, "plain"), fin(y), gv.ref_gemv(x, Ws), BF, False)
    bd, rd = bias.to(dev), res.contiguous().to(dev)
    y = run(lambda: guarded(dev, c.B, c.N, lambda o: ops.gemv(Wd, xd, bias=bd, res=rd, out=o)))
    gv.check(tag(c.route, "bias+res"), fin(y), gv.ref_gemv(x, Ws, bias=bs, res=rs_), BF, False)


def run_swiglu_case(ops, dev, c, run=both):
    Wgu, _, nw = gv.weights(2 * c.N, c.K, seed=21)
    x = gv.acts(c.K, c.N)[0][:c.B]
    Wd, xd = Wgu.to(dev), x.to(dev)
    if c.norm:
        nd = nw.to(dev)
        y = run(lambda: guarded(dev, c.B, c.N, lambda o: ops.gemv_swiglu(Wd, xd, norm_w=nd, eps=EPS, out=o)))
        gv.check(tag(c.route, "gate/up norm"), y, gv.ref_swiglu(x, Wgu, norm_w=nw, eps=EPS), BF, False)
    else:
        y = run(lambda: guarded(dev, c.B, c.N, lambda o: ops.gemv_swiglu(Wd, xd, out=o)))
        gv.check(tag(c.route, "gate/up"), y, gv.ref_swiglu(x, Wgu), BF, False)


def run_case(ops, dev, c, run=both):
    (run_gemv_case if c.entry == "gemv" else run_swiglu_case)(ops, dev, c, run)


def cid(c):
    return f"{c.entry}-B{c.B}-N{c.N}-K{c.K}-{'norm' if c.norm else 'plain'}"


# ================================================================================================ gemv_kernel
@pytest.mark.parametrize("c", gv.cases("rows"), ids=cid)
def test_rows_5_to_8_on_the_fma_kernel(ops, dev, c):
    run_case(ops, dev, c)


@pytest.mark.parametrize("c", gv.cases("xl2"), ids=cid)
def test_activations_through_l2(ops, dev, c):
    run_case(ops, dev, c)


def test_fused_norm_refused_above_64k(ops, dev):
    """(4, 8200): one step above 64 KiB the library refuses the fused norm and launches nothing"""
    from spider_amd.lib import SpiderHipError
    W, _, nw = gv.weights(37, 8200)
    x = gv.acts(8200, 37)[0][:4]
    out = torch.full((4, 37), SENT, dtype=BF, device=dev)
    with pytest.raises(SpiderHipError, match="fused RMSNorm needs batch\\*K\\*2 <= 64 KiB"):
        ops.gemv(W.to(dev), x.to(dev), norm_w=nw.to(dev), eps=EPS, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()), "the refused call wrote its output"


@pytest.mark.parametrize("c", gv.cases("stage"), ids=cid)
def test_staging_batches(ops, dev, c):
    run_case(ops, dev, c)


def subset_rows(N):
    """the first 64 rows, the last 64, 256 seeded ones, the last row and the last even row"""
    g = torch.Generator().manual_seed(N)
    pick = torch.cat([torch.arange(64), torch.arange(N - 64, N), torch.randperm(N, generator=g)[:256],
                      torch.tensor([N - 1, (N - 1) // 2 * 2])])
    return torch.unique(pick)


@pytest.fixture(scope="module")
def w_6145():
    return gv.weights(6145, 4096, seed=31)


@pytest.fixture(scope="module")
def w_1329():
    return gv.weights(1329, 18944, seed=41)


@pytest.mark.parametrize("c", gv.cases("r2", K=4096), ids=cid)
def test_two_rows_per_wave_at_the_threshold(ops, dev, c, w_6145):
    W, bias, nw = w_6145
    run_gemv_case(ops, dev, c, cols=subset_rows(c.N), W=W[:c.N], bias=bias[:c.N], nw=nw)


@pytest.mark.parametrize("c", gv.cases("r2", K=18944), ids=cid)
def test_two_rows_per_wave_long_k_odd_n(ops, dev, c, w_1329):
    W, bias, nw = w_1329
    run_gemv_case(ops, dev, c, cols=subset_rows(c.N), W=W, bias=bias, nw=nw)


# ================================================================================================ the MFMA kernels
@pytest.mark.parametrize("K", [64, 576, 832, 3648])
@pytest.mark.parametrize("B", [5, 9, 13, 16])
def test_skinny_gemm_kernel(ops, dev, B, K):
    cs = gv.cases("mfma", B=B, K=K)
    assert len(cs) == 4
    for c in cs:
        run_case(ops, dev, c, run=once)


def run_fm_case(ops, dev, c):
    fold = c.norm
    ne = EPS if fold else None
    if c.entry == "gemv_fm":
        W, bias, nw = gv.weights(c.N, c.K)
        x, res = (t[:c.B] for t in gv.acts(c.K, c.N, 3.0))
        Wfm = ops.repack_fm16(W.to(dev), nw.to(dev) if fold else None)
        xd, bd, rd = x.to(dev), bias.to(dev), res.contiguous().to(dev)
        kw = dict(norm_w=nw, eps=EPS, fold=True) if fold else {}
        y = guarded(dev, c.B, c.N, lambda o: ops.gemv_fm(Wfm, xd, c.N, out=o, norm_eps=ne))
        gv.check(tag(c.route, "plain"), y, gv.ref_gemv(x, W, **kw), BF, False)
        y = guarded(dev, c.B, c.N, lambda o: ops.gemv_fm(Wfm, xd, c.N, bias=bd, res=rd, out=o, norm_eps=ne))
        gv.check(tag(c.route, "bias+res"), y, gv.ref_gemv(x, W, bias=bias, res=res, **kw), BF, False)
    else:
        Wgu, _, nw = gv.weights(2 * c.N, c.K, seed=21)
        x = gv.acts(c.K, c.N, 3.0)[0][:c.B]
        Wfm = ops.repack_fm16(Wgu.to(dev), nw.to(dev) if fold else None)
        xd = x.to(dev)
        kw = dict(norm_w=nw, eps=EPS, fold=True) if fold else {}
        y = guarded(dev, c.B, c.N, lambda o: ops.gemv_swiglu_fm(Wfm, xd, out=o, norm_eps=ne))
        gv.check(tag(c.route, "gate/up"), y, gv.ref_swiglu(x, Wgu, **kw), BF, False)


@pytest.mark.parametrize("K", [64, 576, 832, 3648])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 7, 8, 9, 15, 16])
def test_skinny_fm_kernel(ops, dev, B, K):
    cs = gv.cases("fm", B=B, K=K)
    assert len(cs) == 8
    for c in cs:
        run_fm_case(ops, dev, c)


def x_in_16_rows(dev, x, fill):
    buf = torch.full((16, x.shape[1]), fill, dtype=BF, device=dev)
    buf[:x.shape[0]] = x.to(dev)
    return buf[:x.shape[0]]


@pytest.mark.parametrize("B", [5, 9, 13])
def test_skinny_gemm_kernel_ignores_rows_past_B(ops, dev, B):
    N, K, I = 37, 576, 23
    W, bias, _ = gv.weights(N, K)
    Wgu = gv.weights(2 * I, K, seed=21)[0]
    x, res = (t[:B] for t in gv.acts(K, N))
    Wd, Wgd, bd, rd = W.to(dev), Wgu.to(dev), bias.to(dev), res.contiguous().to(dev)
    y = [(ops.gemv(Wd, xb, bias=bd, res=rd), ops.gemv_swiglu(Wgd, xb)) for xb in (x_in_16_rows(dev, x, 0.0), x_in_16_rows(dev, x, 1e4))]
    assert torch.equal(y[0][0], y[1][0]) and torch.equal(y[0][1], y[1][1])


@pytest.mark.parametrize("B", [1, 2, 7, 15])
def test_skinny_fm_kernel_ignores_rows_past_B(ops, dev, B):
    N, K, I = 37, 576, 16
    W, bias, nw = gv.weights(N, K)
    Wgu = gv.weights(2 * I, K, seed=21)[0]
    x, res = (t[:B] for t in gv.acts(K, N, 3.0))
    bd, rd = bias.to(dev), res.contiguous().to(dev)
    for fold in (False, True):
        ne = EPS if fold else None
        Wfm = ops.repack_fm16(W.to(dev), nw.to(dev) if fold else None)
        Wgfm = ops.repack_fm16(Wgu.to(dev), nw.to(dev) if fold else None)
        y = [(ops.gemv_fm(Wfm, xb, N, bias=bd, res=rd, norm_eps=ne), ops.gemv_swiglu_fm(Wgfm, xb, norm_eps=ne))
             for xb in (x_in_16_rows(dev, x, 0.0), x_in_16_rows(dev, x, 1e4))]
        assert torch.equal(y[0][0], y[1][0]) and torch.equal(y[0][1], y[1][1])
        assert bool(torch.isfinite(y[1][0].float()).all()) and bool(torch.isfinite(y[1][1].float()).all())


# ================================================================================================ lm_head
def neutral_proc(ops, dev, B, V):
    """nothing seen, nothing banned, penalty 1, no minimum length"""
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    return dict(seen=z(B, ops.bitmap_words(V)), ban=z(B, ops.bitmap_words(V)), penalty=torch.ones(1, dtype=torch.float32, device=dev),
                min_new=z(1), eos_ids=z(8), n_eos=z(1), n_hist=z(B))


def run_lm_case(ops, dev, c):
    fm = c.entry.endswith("_fm")
    W, x, nw, rows, R = gv.lm_case(c.N, c.K, c.B, c.norm, fm, 3.0 if fm and c.norm else 1.0)
    xd = x.to(dev)
    logits = torch.full((c.B * c.N + 64,), SENT, dtype=BF, device=dev)
    lg = logits[:c.B * c.N].view(c.B, c.N)
    if fm:
        Wfm = ops.repack_fm16(W.to(dev), nw.to(dev) if c.norm else None)
        ne = EPS if c.norm else None
        ids = ops.lm_head_argmax_fm(Wfm, xd, c.N, logits=lg, norm_eps=ne)
        ids2 = ops.lm_head_argmax_fm(Wfm, xd, c.N, norm_eps=ne)
    else:
        Wd, nd = W.to(dev), (nw.to(dev) if c.norm else None)
        ids = ops.lm_head_argmax(Wd, xd, norm_w=nd, eps=EPS, logits=lg)
        ids2 = ops.lm_head_argmax(Wd, xd, norm_w=nd, eps=EPS)
    # the *_proc entry points (their own instantiations) with processors that change nothing: the same logits, the same id
    lg_p = torch.full_like(lg, SENT)
    proc = neutral_proc(ops, dev, c.B, c.N)
    if fm:
        ids_p = ops.lm_head_argmax_fm_proc(Wfm, xd, c.N, proc, logits=lg_p, norm_eps=ne)
    else:
        ids_p = ops.lm_head_argmax_proc(Wd, xd, proc, norm_w=nd, eps=EPS, logits=lg_p)
    assert torch.equal(lg_p, lg) and torch.equal(ids_p, ids), "the processed form with neutral processors differs"
    assert bool((logits[c.B * c.N:] == SENT).all()), "the kernel wrote behind its logits"
    gv.check(tag(c.route, "logits norm" if c.norm else "logits"), lg, R, BF, False)
    own = lg.float().cpu().argmax(-1)                       # torch returns the first maximum: the lowest index
    assert ids.cpu().long().tolist() == own.tolist(), "not the lowest-index arg-max of the kernel's own logits"
    assert ids.cpu().tolist() == rows, "not the fp64 arg-max (the planted winner)"
    assert ids2.cpu().tolist() == rows, "the id changes when no logits are asked for"


@pytest.mark.parametrize("c", gv.cases("lm"), ids=cid)
def test_lm_head_row_major(ops, dev, c):
    run_lm_case(ops, dev, c)


@pytest.mark.parametrize("c", gv.cases("lm_fm"), ids=cid)
def test_lm_head_fragment_major(ops, dev, c):
    run_lm_case(ops, dev, c)


def tie_weight(V, K, rows):
    W = torch.zeros(V, K, dtype=BF)
    W[rows, 0] = 1.0
    return W


@pytest.mark.parametrize("rows", [(2, 3), (0, 2), (17, 250)], ids=["one_wave", "two_waves", "two_blocks"])
@pytest.mark.parametrize("B", [1, 5])
def test_lm_head_row_major_ties(ops, dev, B, rows):
    """identical rows -> identical logits -> the lowest id wins (R = 2: rows 2, 3 are one wave's pair; 0 and 2 two waves of block 0;
    V = 300 gives 5 blocks of 60 rows)"""
    x = torch.zeros(B, 64, dtype=BF)
    x[:, 0] = 1.0
    W = tie_weight(300, 64, list(rows))
    assert ops.lm_head_argmax(W.to(dev), x.to(dev)).cpu().tolist() == [rows[0]] * B
    W[rows[0], 0] = 0.5                                     # and the other one when it alone is the maximum
    assert ops.lm_head_argmax(W.to(dev), x.to(dev)).cpu().tolist() == [rows[1]] * B


@pytest.mark.parametrize("rows", [(1, 2), (2, 9), (49, 8305)], ids=["one_lane", "lane_groups", "two_row_groups"])
@pytest.mark.parametrize("B", [1, 7, 16])
def test_lm_head_fragment_major_ties(ops, dev, B, rows):
    """V = 33000: 2063 row groups over 516 blocks, so block 3 owns groups 3 and 519 (rows 49 and 8305)"""
    V, K = 33000, 128
    assert ops.lm_head_nparts(V) == 516 and 8305 // 16 - 49 // 16 == 516
    x = torch.zeros(B, K, dtype=BF)
    x[:, 0] = 1.0
    W = tie_weight(V, K, list(rows))
    assert ops.lm_head_argmax_fm(ops.repack_fm16(W.to(dev)), x.to(dev), V).cpu().tolist() == [rows[0]] * B
    W[rows[0], 0] = 0.5
    assert ops.lm_head_argmax_fm(ops.repack_fm16(W.to(dev)), x.to(dev), V).cpu().tolist() == [rows[1]] * B


# ================================================================================================ rmsnorm
@pytest.mark.parametrize("H", [8, 64, 2056, 8184, 8192])
def test_rmsnorm(ops, dev, H):
    w = (1 + 0.1 * gv.draw(5, H).float()).to(BF)
    wd = w.to(dev)
    for rows in (1, 3):
        for scale in (1e-3, 1.0, 300.0):
            x, r = gv.draw(3, rows, H, scale=scale), gv.draw(4, rows, H, scale=scale)
            what = f"rmsnorm H={H} rows={rows} scale={scale}"
            y = guarded(dev, rows, H, lambda o: ops.rmsnorm(x.to(dev), wd, EPS, out=o))
            gv.check("rmsnorm | " + what, y, gv.ref_rmsnorm(x, w, EPS), BF, False)
            h = gv.add_bf16(x, r)
            ro = torch.full((rows * H + 64,), SENT, dtype=BF, device=dev)
            y = guarded(dev, rows, H, lambda o: ops.rmsnorm(x.to(dev), wd, EPS, res=r.to(dev), res_out=ro[:rows * H].view(rows, H), out=o))
            assert torch.equal(ro[:rows * H].view(rows, H).cpu(), h), "res_out is not bf16(x + res)"
            assert bool((ro[rows * H:] == SENT).all())
            gv.check("rmsnorm | " + what + " +res", y, gv.ref_rmsnorm(h, w, EPS), BF, False)
            y = ops.rmsnorm(x.to(dev), wd, EPS, res=r.to(dev))                  # res without res_out
            gv.check("rmsnorm | " + what + " +res, no res_out", y, gv.ref_rmsnorm(h, w, EPS), BF, False)

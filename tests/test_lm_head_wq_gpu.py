"""GPU: the weight-only FP8 / MXFP4 lm_head kernels (ops.lm_head_argmax[_proc]_w8 / _w4, csrc/lm_head_wq.hip).

Raw logits are held to an fp64 restatement on W_eff that rounds where the kernel rounds, with the derived bound of
tests/test_fp8_gemv_gpu.py / tests/test_mxfp4_gemv_gpu.py restated here. With u = 2^-24 the unit roundoff of fp32:

  * a dequantised weight is a bf16 number (FP8: three significand bits, the row's power-of-two scale multiplies the fp32 sum
    exactly; MXFP4: two significand bits times a power of two applied inside the conversion), so every product x[k] * W[n, k] is
    exact in fp32 and the fp32 dot product differs from the exact one only by its K - 1 additions, in ANY order at most
    (K - 1) u / (1 - (K - 1) u) * sum_k |x[k] W_eff[n, k]|. The test allows E = 2 K u sum_k |x[k] W_eff[n, k]| (the factor 2 covers
    the two-term adder inside v_dot2c_f32_bf16);
  * the logit is rounded to bf16 once: it may land on the other side of a rounding boundary than the fp64 value, one bf16 ulp
    <= 2^-7 |ref|.   |err| <= E + 2^-7 |ref|.
  * fused RMSNorm: the test reads the kernel's OWN normalised activations through an identity head (V = K one-hot rows of 1.0: the
    logits output is xin bit for bit), checks them against the fp64 RMSNorm within its two bf16 roundings, and feeds them to the
    restatement.

Chosen ids have no tolerance: out_ids[b] is the lowest-index arg-max of llm.process_logits_host applied to the kernel's own raw
logits output (no processors in the plain form), with and without the logits output."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
U8 = torch.uint8
F8 = torch.float8_e4m3fn
U32 = 2.0 ** -24
ULP16 = 2.0 ** -7
EPS = 1e-5
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
LDS_BUDGET = 160 * 1024 - 256
PENALTY = 1.3
FMTS = ("w8", "w4")


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------ the formats, restated in fp64
def _w_eff4(blocks, scales):
    N, K = blocks.shape[0], blocks.shape[1] * 2
    table = torch.tensor(GRID + [-v for v in GRID], dtype=torch.float64, device=blocks.device)
    codes = torch.stack([blocks & 15, blocks >> 4], dim=2).reshape(N, K)
    sc = torch.ldexp(torch.ones(N, K // 32, dtype=torch.float64, device=blocks.device), scales.to(torch.int32) - 127)
    return table[codes.long()] * sc.repeat_interleave(32, dim=1)


def _e4m3_table():
    """value of every e4m3fn byte (bias 7, subnormals at exponent 0, 0x7f / 0xff = NaN), from the format's definition"""
    t = []
    for b in range(256):
        s, e, m = -1.0 if b & 128 else 1.0, (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            t.append(float("nan"))
        elif e == 0:
            t.append(s * m / 8 * 2.0 ** -6)
        else:
            t.append(s * (1 + m / 8) * 2.0 ** (e - 7))
    return torch.tensor(t, dtype=torch.float64)


def _w_eff8(q, scale):
    return _e4m3_table().to(q.device)[q.view(U8).long()] * scale.double()[:, None]


def _w_eff(fmt, q, s):
    return _w_eff8(q, s) if fmt == "w8" else _w_eff4(q, s)


def _case(fmt, dev, B, V, K, seed):
    """random weight bytes over all codes with scales that differ between neighbours; x, norm_w in bf16.
    w4: all 16 codes in both nibbles, scale bytes 107 .. 135 that differ between neighbouring blocks and rows (the recipe of
    tests/test_mxfp4_gemv_gpu.py: _case). w8: bytes over all finite e4m3 codes, power-of-two scales 2^-12 .. 2^-5 that differ by row."""
    g = torch.Generator().manual_seed(seed)
    if fmt == "w4":
        q = torch.randint(0, 256, (V, K // 2), generator=g, dtype=torch.int32).to(U8)
        s = (107 + (torch.arange(V)[:, None] * 5 + torch.arange(K // 32)[None, :] * 7 + seed) % 29).to(U8)
    else:
        q = torch.randint(0, 256, (V, K), generator=g, dtype=torch.int32).to(U8)
        q[(q & 127) == 127] = 0x7e                                    # NaN codes -> +-448 stays out: 0x7e = 448
        q = q.view(F8)
        s = torch.ldexp(torch.ones(V), -12 + (torch.arange(V) * 3 + seed) % 8).float()
    x = torch.randn(B, K, generator=g).to(BF)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF)
    return q.to(dev), s.to(dev), x.to(dev), nw.to(dev)


def _fits(ops, fmt, B, K):
    return ops.w8_norm_fits(B, K) if fmt == "w8" else ops.w4_norm_fits(B, K)


def _call(ops, fmt, q, s, x, proc=None, **kw):
    if proc is None:
        return (ops.lm_head_argmax_w8 if fmt == "w8" else ops.lm_head_argmax_w4)(q, s, x, **kw)
    return (ops.lm_head_argmax_proc_w8 if fmt == "w8" else ops.lm_head_argmax_proc_w4)(q, s, x, proc, **kw)


def _logits(ops, fmt, q, s, x, proc=None, norm_w=None):
    lg = torch.full((x.shape[0], q.shape[0]), float("nan"), dtype=BF, device=x.device)
    ids = _call(ops, fmt, q, s, x, proc, norm_w=norm_w, eps=EPS, logits=lg)
    return ids, lg


_EYE = {}


def _kernel_xin(ops, fmt, dev, x, nw):
    """the kernel's own normalised activations [B, K] bf16, read through an identity head (see the module docstring), checked
    against the fp64 RMSNorm: bf16(bf16(x * rs) * w) with at most one ulp of slack per rounding"""
    K = x.shape[-1]
    if (fmt, K) not in _EYE:
        _EYE.clear()
        k = torch.arange(K, device=dev)
        if fmt == "w4":
            eye = torch.zeros(K, K // 2, dtype=U8, device=dev)
            eye[k, k // 2] = torch.where(k % 2 == 1, 0x20, 0x02).to(U8)     # code 2 = 1.0 in the nibble of weight k
            _EYE[(fmt, K)] = (eye, torch.full((K, K // 32), 127, dtype=U8, device=dev))
        else:
            eye = torch.zeros(K, K, dtype=U8, device=dev)
            eye[k, k] = 0x38                                                # 1.0
            _EYE[(fmt, K)] = (eye.view(F8), torch.ones(K, dtype=torch.float32, device=dev))
    eye, one = _EYE[(fmt, K)]
    _, xin = _logits(ops, fmt, eye, one, x, norm_w=nw)
    xd = x.double()
    rs = torch.rsqrt((xd * xd).mean(-1, keepdim=True) + EPS)
    a = (xd * rs).to(BF).double()
    ref = (a * nw.double()).to(BF).double()
    tol = ULP16 * ref.abs() * (1 + ULP16) + ULP16 * ref.abs() + 1e-30
    err = (xin.double() - ref).abs()
    assert bool((err <= tol).all()), f"fused RMSNorm: max err / tol {float((err / tol).max()):.3g}"
    return xin


def _check_logits(got, xin, w, what):
    """|got - bf16(exact)| <= 2 K u sum |x W_eff| + 2^-7 |ref|"""
    xd = xin.double()
    ref = (xd @ w.T).to(BF).double()
    tol = 2 * xin.shape[-1] * U32 * (xd.abs() @ w.abs().T) + ULP16 * ref.abs()
    err = (got.double() - ref).abs()
    ratio = float((err / tol.clamp_min(1e-300)).max())
    print(f"{what}: max err / derived bound = {ratio:.3g}")
    assert got.dtype == BF and got.shape == ref.shape and bool(torch.isfinite(got.float()).all())
    assert bool((err <= tol).all()), f"{what}: max err / bound {ratio:.3g}, {int((err > tol).sum())} / {err.numel()} elements out"


# ------------------------------------------------------------------------------------------ processors
def _bitmap(mask, dev):
    """bool [B, V] -> the kernels' bitmap: uint32 words kept as int32 [B, ceil(V / 32)], bit n & 31 of word n >> 5"""
    B, V = mask.shape
    W = (V + 31) // 32
    m = torch.zeros(B, W * 32, dtype=torch.int64)
    m[:, :V] = mask.long()
    v = (m.view(B, W, 32) << torch.arange(32)).sum(-1)
    v = torch.where(v >= 2 ** 31, v - 2 ** 32, v)
    return v.to(torch.int32).contiguous().to(dev)


def _proc(dev, seen, ban, n_hist, min_new, eos):
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    return dict(seen=_bitmap(seen, dev), ban=_bitmap(ban, dev), penalty=torch.tensor([PENALTY], dtype=torch.float32, device=dev),
                min_new=i32([min_new]), eos_ids=i32((list(eos) + [0] * 8)[:8]), n_eos=i32([len(eos)]), n_hist=i32(list(n_hist)))


def _host_ids(lg, seen=None, ban=None, n_hist=None, min_new=0, eos=()):
    """lowest-index arg-max of process_logits_host on the raw logits, row by row (the rows differ in their sets and counters)"""
    from spider_amd.llm import process_logits_host
    lg = lg.cpu()
    B, V = lg.shape
    out = []
    for b in range(B):
        if seen is None:
            lv = process_logits_host(lg[b:b + 1], torch.zeros(1, V, dtype=torch.bool), 1.0, [], None, 0, 0)
        else:
            lv = process_logits_host(lg[b:b + 1], seen[b:b + 1], PENALTY, ban[b].nonzero().flatten().tolist(), list(eos), n_hist[b],
                                     min_new)
        out.append(int((lv[0] == lv[0].max()).nonzero()[0]))
    return out


def _proc_case(B, V, seed):
    """a random seen set (a third of the ids), a ban set (a tenth), two EOS ids banned on the even rows only (n_hist < min_new)"""
    g = torch.Generator().manual_seed(1000 + seed)
    seen = torch.rand(B, V, generator=g) < 0.33
    ban = torch.rand(B, V, generator=g) < 0.1
    ban[:, 0] = False
    n_hist = [1 if b % 2 == 0 else 5 for b in range(B)]
    eos = sorted({V // 2, V - 1})
    return seen, ban, n_hist, 3, eos


# K: one load of one lane (16 / 32), one full wave instruction (1024 / 2048), one full + one ragged lane (1040 / 2080), 3584 = the
# workload's hidden size. V: 1 and 97 = fewer rows than the blocks' waves own, 331 = ragged within a block (6 blocks of 56 rows),
# 4100 = 65 blocks of 64 rows with the last range of 4 rows. B: every row count the kernels exist for.
KS = {"w8": (16, 1024, 1040, 3584), "w4": (32, 2048, 2080, 3584)}


@pytest.mark.parametrize("V", [1, 97, 331, 4100])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("fmt,ki", [(f, i) for f in FMTS for i in range(4)])
def test_logits_and_ids(ops, dev, fmt, ki, B, V):
    K = KS[fmt][ki]
    q, s, x, nw = _case(fmt, dev, B, V, K, seed=B + 7 * V + K)
    w = _w_eff(fmt, q, s)
    assert _fits(ops, fmt, B, K) and ops.lm_head_nparts(V) == (V + 63) // 64
    xin = _kernel_xin(ops, fmt, dev, x, nw)
    seen, ban0, n_hist, min_new, eos = _proc_case(B, V, B + V + K)
    for norm in (None, nw):
        what = f"lm_head_{fmt} B{B} V{V} K{K} norm{int(norm is not None)}"
        ids, lg = _logits(ops, fmt, q, s, x, norm_w=norm)
        _check_logits(lg, x if norm is None else xin, w, what)
        assert ids.dtype == torch.int32 and ids.tolist() == _host_ids(lg), what
        assert torch.equal(_call(ops, fmt, q, s, x, norm_w=norm, eps=EPS), ids), what + ": ids without the logits output"
        ban = ban0.clone()
        ban[0, int(ids[0])] = True          # the first row's unprocessed choice is banned: the processors change something in every case
        proc = _proc(dev, seen, ban, n_hist, min_new, eos)
        pids, plg = _logits(ops, fmt, q, s, x, proc, norm_w=norm)
        assert V == 1 or int(pids[0]) != int(ids[0]), what + " proc: a banned id was chosen"
        assert torch.equal(plg, lg), what + ": the logits output stays raw"
        assert pids.tolist() == _host_ids(plg, seen, ban, n_hist, min_new, eos), what + " proc"
        assert torch.equal(_call(ops, fmt, q, s, x, proc, norm_w=norm, eps=EPS), pids), what + " proc: ids without the logits output"
    if V > 8:      # the processors change at least one choice somewhere in the sweep's larger cases; say which
        print(f"lm_head_{fmt} B{B} V{V} K{K}: plain ids {ids.tolist()} processed ids {pids.tolist()}")


# The long row: 10 chunks of 2048 (w4) / 20 of 1024 (w8). Two rows stage 80 KiB, above the 64 KiB a launch gets without opting in;
# four rows would need 160 KiB, 256 bytes more than the budget: the waves read x through L2 and the fused norm is refused.
@pytest.mark.parametrize("fmt,K", [("w8", 19472), ("w4", 18464)])
@pytest.mark.parametrize("B,staged", [(2, True), (4, False)])
def test_long_rows_staged_and_through_l2(ops, dev, fmt, K, B, staged):
    from spider_amd.lib import SpiderHipError
    V = 9
    chunk, per = (1024, 2048) if fmt == "w8" else (2048, 4096)
    assert _fits(ops, fmt, B, K) == (B * ((K + chunk - 1) // chunk) * per <= LDS_BUDGET) == staged
    q, s, x, nw = _case(fmt, dev, B, V, K, seed=B + K)
    ids, lg = _logits(ops, fmt, q, s, x)
    _check_logits(lg, x, _w_eff(fmt, q, s), f"lm_head_{fmt} B{B} V{V} K{K}")
    assert ids.tolist() == _host_ids(lg)
    seen, ban, n_hist, min_new, eos = _proc_case(B, V, K)
    pids, plg = _logits(ops, fmt, q, s, x, _proc(dev, seen, ban, n_hist, min_new, eos))
    assert torch.equal(plg, lg) and pids.tolist() == _host_ids(plg, seen, ban, n_hist, min_new, eos)
    if not staged:
        with pytest.raises(SpiderHipError, match="fused RMSNorm"):
            _call(ops, fmt, q, s, x, norm_w=nw, eps=EPS)
        with pytest.raises(SpiderHipError, match="fused RMSNorm"):
            _call(ops, fmt, q, s, x, _proc(dev, seen, ban, n_hist, min_new, eos), norm_w=nw, eps=EPS)
        from spider_amd import lib
        p = lambda t: t.data_ptr()
        ws = (torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        with pytest.raises(SpiderHipError, match="fused RMSNorm"):
            lib.call("spider_lm_head_argmax_" + fmt, p(q), p(s), p(x), p(nw), EPS, p(ids), None, p(ws[0]), p(ws[1]), B, V, K, None)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B", [1, 4])
def test_engineered_ties_go_to_the_lowest_id(ops, dev, fmt, B):
    """the best row of the batch, with its scales, duplicated at ids of another wave of the same block (5 -> 9 with up to 4 rows per
    wave iteration, 5 -> 21 with 8), of other blocks (100, 200) and of the last partial group (330): equal logits bit for bit, and
    the lowest of the duplicates' ids wins; every row of the batch is a power-of-two multiple of row 0, so all rows agree"""
    V, K = 331, 3584
    q, s, x, _ = _case(fmt, dev, 1, V, K, seed=77 + B)
    x = torch.cat([x * 2.0 ** b for b in range(B)], 0).contiguous()
    ids0, _ = _logits(ops, fmt, q, s, x)
    m = int(ids0[0])
    assert ids0.tolist() == [m] * B
    for dup in ([330], [200, 330], [100, 200, 330], [21, 100, 330], [9, 21, 100], [5, 9, 21, 100, 200, 330]):
        q2, s2 = q.clone(), s.clone()
        for n in dup:
            q2.view(U8)[n] = q.view(U8)[m]
            s2[n] = s[m]
        ids, lg = _logits(ops, fmt, q2, s2, x)
        want = min(dup + [m])
        assert all(torch.equal(lg[:, n], lg[:, m]) for n in dup), dup
        assert ids.tolist() == [want] * B == _host_ids(lg), (dup, m, ids.tolist())
        assert _call(ops, fmt, q2, s2, x).tolist() == [want] * B


@pytest.mark.parametrize("fmt", FMTS)
def test_all_banned_rows_return_id_0(ops, dev, fmt):
    V, K = 331, 256
    for B in (1, 2, 4):
        q, s, x, nw = _case(fmt, dev, B, V, K, seed=5 + B)
        seen = torch.zeros(B, V, dtype=torch.bool)
        ban = torch.zeros(B, V, dtype=torch.bool)
        ban[0::2] = True                                   # even rows: every id banned; odd rows: free
        proc = _proc(dev, seen, ban, [0] * B, 0, [])
        ids, lg = _logits(ops, fmt, q, s, x, proc, norm_w=nw)
        free, _ = _logits(ops, fmt, q, s, x, norm_w=nw)
        want = [0 if b % 2 == 0 else int(free[b]) for b in range(B)]
        assert ids.tolist() == want == _host_ids(lg, seen, ban, [0] * B, 0, []), (B, ids.tolist(), want)
        # every id an EOS-before-min_new or banned id: the same through the EOS rule for the ids 0 and 1 of a two-row vocabulary
        ids2 = _call(ops, fmt, q[:2].contiguous(), s[:2].contiguous(), x, _proc(dev, seen[:, :2], seen[:, :2], [0] * B, 1, [0, 1]))
        assert ids2.tolist() == [0] * B


def test_one_hot_activations_return_w_eff_bit_for_bit_w4(ops, dev):
    """x = 1.0 at one k: logit[b, n] = W_eff[n, k_b] exactly, for every code in both nibbles and the scale bytes 2, 64, 127, 190, 252"""
    K, SC = 64, [2, 64, 127, 190, 252]
    j = torch.arange(K // 2)
    row = (((j + 3) % 16) | (((20 - j) % 16) << 4)).to(U8)
    assert sorted((row[:16] & 15).tolist()) == list(range(16)) and sorted((row[:16] >> 4).tolist()) == list(range(16))
    blocks = row[None, :].repeat(len(SC), 1)
    scales = torch.tensor([[SC[n], SC[(n + 2) % len(SC)]] for n in range(len(SC))], dtype=U8)
    w = _w_eff4(blocks, scales)
    assert bool(torch.isfinite(w).all()) and torch.equal(w.float().to(BF).double(), w)
    _one_hot(ops, "w4", dev, blocks.to(dev), scales.to(dev), w, K)


def test_one_hot_activations_return_w_eff_bit_for_bit_w8(ops, dev):
    """the same for every finite e4m3 byte under the row scales 2^-20, 2^-3, 1 and 2^10"""
    K = 256
    row = torch.arange(256, dtype=torch.int32).to(U8)
    row[(row & 127) == 127] = 0
    q = row[None, :].repeat(4, 1)
    scale = torch.tensor([2.0 ** -20, 2.0 ** -3, 1.0, 2.0 ** 10])
    w = _w_eff8(q, scale)
    assert bool(torch.isfinite(w).all()) and torch.equal(w.float().to(BF).double(), w) and float(w.abs().max()) == 448 * 2.0 ** 10
    assert torch.equal(w[2].float(), q[2].view(F8).float())      # (scale 1: the table above is torch's e4m3fn)
    _one_hot(ops, "w8", dev, q.view(F8).to(dev), scale.to(dev), w, K)


def _one_hot(ops, fmt, dev, q, s, w, K):
    for B in (1, 2, 3, 4):
        for k0 in range(0, K, 4):
            ks = [(k0 + b) % K for b in range(B)]
            x = torch.zeros(B, K, dtype=BF, device=dev)
            for b, k in enumerate(ks):
                x[b, k] = 1.0
            ids, lg = _logits(ops, fmt, q, s, x)
            got, want = lg.double().cpu(), w[:, ks].T
            bad = (got != want).nonzero().tolist()                     # (!= on values: a -0 weight may come back as +0)
            assert not bad, (B, ks, [(b, n, float(got[b, n]), float(want[b, n])) for b, n in bad[:8]])
            assert ids.tolist() == _host_ids(lg)


@pytest.mark.parametrize("fmt", FMTS)
def test_two_calls_and_a_captured_call_are_bit_identical(ops, dev, fmt):
    B, V, K = 3, 4100, 3584
    q, s, x, nw = _case(fmt, dev, B, V, K, seed=11)
    seen, ban, n_hist, min_new, eos = _proc_case(B, V, 11)
    proc = _proc(dev, seen, ban, n_hist, min_new, eos)
    npart = ops.lm_head_nparts(V)
    mk = lambda: dict(ids=torch.zeros(B, dtype=torch.int32, device=dev), lg=torch.zeros(B, V, dtype=BF, device=dev),
                      ws=(torch.zeros(B * npart, dtype=torch.float32, device=dev), torch.zeros(B * npart, dtype=torch.int32, device=dev)))

    def run(o, pr):
        _call(ops, fmt, q, s, x, pr, norm_w=nw, eps=EPS, out_ids=o["ids"], logits=o["lg"], ws=o["ws"])
    same = lambda a, b: torch.equal(a["ids"], b["ids"]) and torch.equal(a["lg"], b["lg"]) and torch.equal(a["ws"][0], b["ws"][0]) \
        and torch.equal(a["ws"][1], b["ws"][1])
    a, b, pa, pb, c, pc = mk(), mk(), mk(), mk(), mk(), mk()
    run(a, None); run(b, None); run(pa, proc); run(pb, proc)
    assert same(a, b) and same(pa, pb)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run(c, None)
            run(pc, proc)
    torch.cuda.current_stream().wait_stream(side)
    for o in (c, pc):
        o["ids"].zero_(); o["lg"].zero_(); o["ws"][0].zero_(); o["ws"][1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same(c, a) and same(pc, pa)


def test_shapes_outside_the_kernels_raise(ops, dev):
    from spider_amd import lib
    from spider_amd.lib import SpiderHipError
    p = lambda t: t.data_ptr()
    seen, ban, n_hist, min_new, eos = _proc_case(1, 7, 1)
    for fmt, bad_k in (("w8", 24), ("w4", 48)):
        q, s, x, nw = _case(fmt, dev, 1, 7, 64, seed=1)
        proc = _proc(dev, seen, ban, n_hist, min_new, eos)
        proc5 = _proc(dev, seen.repeat(5, 1), ban.repeat(5, 1), n_hist * 5, min_new, eos)
        cols = bad_k if fmt == "w8" else bad_k // 2
        with pytest.raises(ValueError):                                         # K not a multiple of 16 / 32
            _call(ops, fmt, q[:, :cols].contiguous(), s if fmt == "w8" else s[:, :1].contiguous(), x[:, :bad_k].contiguous())
        with pytest.raises(ValueError):                                         # one scale per row / per block of every row
            _call(ops, fmt, q, s[:3].contiguous(), x)
        with pytest.raises(ValueError):                                         # scales of the wrong dtype
            _call(ops, fmt, q, s.double() if fmt == "w8" else s.view(torch.int8), x)
        with pytest.raises(ValueError):                                         # weights of the wrong dtype
            _call(ops, fmt, q.view(torch.int8), s, x)
        with pytest.raises(ValueError, match="rows"):
            _call(ops, fmt, q, s, x.repeat(5, 1))
        with pytest.raises(ValueError, match="rows"):
            _call(ops, fmt, q, s, x.repeat(5, 1), proc5)
        # the same refusals from the entry points themselves, before any launch
        ids = torch.zeros(5, dtype=torch.int32, device=dev)
        ws = (torch.zeros(5, dtype=torch.float32, device=dev), torch.zeros(5, dtype=torch.int32, device=dev))
        pa = [p(proc[k]) for k in ("seen", "ban", "penalty", "min_new", "eos_ids", "n_eos", "n_hist")]
        with pytest.raises(SpiderHipError, match="multiple of 16" if fmt == "w8" else "multiple of 32"):
            lib.call("spider_lm_head_argmax_" + fmt, p(q), p(s), p(x), None, 0.0, p(ids), None, p(ws[0]), p(ws[1]), 1, 7, bad_k, None)
        with pytest.raises(SpiderHipError, match=r"1\.\.4"):
            lib.call("spider_lm_head_argmax_" + fmt, p(q), p(s), p(x), None, 0.0, p(ids), None, p(ws[0]), p(ws[1]), 5, 7, 64, None)
        with pytest.raises(SpiderHipError, match=r"1\.\.4"):
            lib.call("spider_lm_head_argmax_proc_" + fmt, p(q), p(s), p(x), None, 0.0, p(ids), None, p(ws[0]), p(ws[1]), *pa, 5, 7, 64, None)
        with pytest.raises(SpiderHipError, match="null"):
            lib.call("spider_lm_head_argmax_" + fmt, p(q), None, p(x), None, 0.0, p(ids), None, p(ws[0]), p(ws[1]), 1, 7, 64, None)
        with pytest.raises(SpiderHipError, match="required"):
            lib.call("spider_lm_head_argmax_proc_" + fmt, p(q), p(s), p(x), None, 0.0, p(ids), None, p(ws[0]), p(ws[1]),
                     *([None] + pa[1:]), 1, 7, 64, None)


def test_torch_ops_registration(ops, dev):
    import spider_amd.torch_ops as T
    assert T.LM_HEAD_Q_OP_NAMES == ("lm_head_argmax_w8", "lm_head_argmax_proc_w8", "lm_head_argmax_w4", "lm_head_argmax_proc_w4")
    seen, ban, n_hist, min_new, eos = _proc_case(2, 97, 3)
    for fmt in FMTS:
        q, s, x, nw = _case(fmt, dev, 2, 97, 64, seed=5)
        proc = _proc(dev, seen, ban, n_hist, min_new, eos)
        pa = tuple(proc[k] for k in ("seen", "ban", "penalty", "min_new", "eos_ids", "n_eos", "n_hist"))
        plain, procd = getattr(torch.ops.spider_hip, "lm_head_argmax_" + fmt), getattr(torch.ops.spider_hip, "lm_head_argmax_proc_" + fmt)
        assert torch.equal(plain(x, q, s, nw, EPS), _call(ops, fmt, q, s, x, norm_w=nw, eps=EPS))
        assert torch.equal(procd(x, q, s, *pa, nw, EPS), _call(ops, fmt, q, s, x, proc, norm_w=nw, eps=EPS))
        if fmt == "w8":
            # opcheck's test_schema clones its arguments through arithmetic that torch does not have for float8 tensors: the FP8
            # ops also take the same bytes as uint8, and the schema is checked on that form
            torch.library.opcheck(plain, (x, q, s, nw, EPS), test_utils=("test_faketensor",))
            torch.library.opcheck(procd, (x, q, s, *pa, nw, EPS), test_utils=("test_faketensor",))
            q = q.view(U8)
            assert torch.equal(plain(x, q, s, nw, EPS), _call(ops, fmt, q.view(F8), s, x, norm_w=nw, eps=EPS))
        torch.library.opcheck(plain, (x, q, s, nw, EPS), test_utils=("test_schema", "test_faketensor"))
        torch.library.opcheck(procd, (x, q, s, *pa, nw, EPS), test_utils=("test_schema", "test_faketensor"))

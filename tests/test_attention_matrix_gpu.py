"""Attention kernels against tests/attn_checks.py: every head dim of the ABI, the mask edges of prefill, kv_off != 0, packed
segments, split-KV decode with empty splits, and an exact "count" variant. test_attention_checks_cpu.py proves on the host that the
fp64 reference fits each tolerance with half of it to spare and that a mask one key off cannot pass any of these cases.

Which instantiation of attn_flash.hip's launch<DP>() (and of llm_decode.hip's decode attention) each group is meant to reach.
DP = padded head width (64 for d <= 64, 96 for d <= 96, 128 for d <= 128, else 160); ONES = the ones column, taken when d < DP.

  group 1, head-dim sweep through spider_attn_{bf16,f16}, d = 8, 16, ..., 160, both dtypes:
    ragged (Lq 70, Lk 150)    attn_flash_kernel<DP, ONES, PLAIN=true> for every DP, ONES on for d not in {64, 96, 128, 160}; the last
                              key tile is partial (150 = 2 * 64 + 22)
    tiles  (Lq 200, Lk 192)   d <= 48: attn_flash_pipe_kernel<64, true, KQ=3>; d = 56: <64, true>; d = 64: <64, false>;
                              d = 72 .. 88: <96, true>; d = 96: <96, false>; d >= 104: attn_flash_kernel<128 / 160, ONES, PLAIN=true>
                              over whole tiles; the second query tile is ragged (200 = 128 + 72)
    masked (causal + kv_beg)  attn_flash_kernel<DP, ONES, PLAIN=false> for every DP, ONES on / off as above; batch row 1 starts at
                              kv_beg 70: t_begin = 1 (odd first tile), first visible tile partial
    fused buffer, d = 64      attn_flash_pipe_kernel<64, false> with q / k / v as column slices (row stride != Hq * d)
  group 2, prefill (attention_cache as LlamaEngine._prefill calls it, cache strides, S 300, T_max 320):
    d 128 bf16, d 128 f16     attn_flash_kernel<128, false, false>;  d 64 bf16: <64, false, false>
    kv_beg 0 / 1 / 63 / 64 / 65 / 127 / 128 / 129 / 255 / 299: t_begin 0 .. 4, even and odd, whole leading tiles skipped,
    kv_beg on, one below and one above a tile edge, rows i < kv_beg exactly 0
  group 3, kv_off (spider_attn_bf16, causal, Lq != Lk): d 128 -> <128, false, false>, d 80 -> <96, true, false>;
    kv_off = Lk - Lq, 64, 63, 37 (keys below Lk never seen), -5 (rows with no key), and kv_off 64 with kv_beg [0, 66]
  group 4, packed segments (spider_attn_varlen_{bf16,f16}, tile records, strided column slices):
    d 64 -> <64, false, false>, d 80 -> <96, true, false>, d 128 (GQA 4 / 2) -> <128, false, false>, each in bf16 and f16;
    segments of 1, 63, 64, 65, 127, 128, 129, 300, 2 rows: seg_kbeg on and off tile edges, 1 .. 3 query tiles per segment;
    rope_rows_kernel at d 64 / 128 on strided views
  group 5, decode (bf16, d 128): attn_decode_kernel<128, G> + attn_combine_kernel and attn_decode_fused_kernel<128, G, 4, 4> /
    <128, G, 8, 8> (the 8-wave form where T_max / nsplit >= 96: len300, nearempty) with the combine forms 0 / 1 / 2, for
    G = 7, 4, 1, 2, 7 (n_q, n_kv = (28, 4), (32, 8), (8, 8), (4, 2), (7, 1)); splits left empty (1, 7, 9 keys over 8 splits,
    kv_beg = kv_end - 3), 64 splits, and kv_beg / kv_end differing per row
  group 6, count variant of groups 2 .. 5: the same instantiations with q = 0 and one-hot v, compared with the exact rational
    answer to 2 ulp of the output type; exactly 0 where the exact answer is 0"""
import pytest
import torch

import attn_checks as ac

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [ac.BF, ac.F16], ids=["bf16", "f16"])
COUNT = pytest.mark.parametrize("count", [False, True], ids=["random", "count"])
N_FLASH = ac.N_CASES - len(ac.DECODE)        # ac.cases(): prefill, kv_off and varlen cases first, the decode cases last


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


def _i32(vals, dev):
    return None if vals is None else torch.tensor(list(vals), dtype=torch.int32, device=dev)


def _cache(t, dev):
    """logical [B, N, Hkv, d] -> the KV cache layout [B, Hkv, N, d]"""
    return t.permute(0, 2, 1, 3).contiguous().to(dev)


def run_case(ops, dev, case, one_buffer=False):
    """the case through the op its kind names -> [B, Lq, Hq, d] on the CPU"""
    B, Lq, Hq, d = case.q.shape
    N, Hkv = case.k.shape[1:3]
    p = case.par
    if case.kind == "flash":
        if one_buffer:      # q / k / v = column slices of one [B, max(Lq, Lk), (Hq + 2 Hkv) * d] buffer; rows past Lk of k / v hold junk
            R = max(Lq, N)
            buf = ac.junk(B, R, (Hq + 2 * Hkv) * d, seed=5, dtype=case.dtype)
            buf[:, :Lq, :Hq * d] = case.q.reshape(B, Lq, -1)
            buf[:, :N, Hq * d:(Hq + Hkv) * d] = case.k.reshape(B, N, -1)
            buf[:, :N, (Hq + Hkv) * d:] = case.v.reshape(B, N, -1)
            buf = buf.to(dev)
            q, k, v = buf[:, :Lq, :Hq * d], buf[:, :N, Hq * d:(Hq + Hkv) * d], buf[:, :N, (Hq + Hkv) * d:]
        else:
            q, k, v = case.q.reshape(B, Lq, -1).to(dev), case.k.reshape(B, N, -1).to(dev), case.v.reshape(B, N, -1).to(dev)
        out = ops.attention(q, k, v, Hq, Hkv, causal=p["causal"], kv_off=p["kv_off"], kv_beg=_i32(p["kv_beg"], dev))
    elif case.kind == "cache":
        out = ops.attention_cache(case.q.to(dev), _cache(case.k, dev), _cache(case.v, dev), Lk=p["Lk"], causal=True, kv_off=0,
                                  kv_beg=_i32(p["kv_beg"], dev))
    elif case.kind == "varlen":
        x = torch.cat([case.q.reshape(Lq, -1), case.k.reshape(N, -1), case.v.reshape(N, -1)], 1).to(dev)
        out = ops.attention_varlen(x[:, :Hq * d], x[:, Hq * d:(Hq + Hkv) * d], x[:, (Hq + Hkv) * d:], Hq, ops.varlen_tiles(p["cu"], dev),
                                   n_kv_heads=Hkv)
    else:
        out = ops.attn_decode(case.q[:, 0].to(dev), _cache(case.k, dev), _cache(case.v, dev), _i32(p["end"], dev),
                              kv_beg=_i32(p["beg"], dev), nsplit=p["nsplit"])
    torch.cuda.synchronize()
    return out.cpu().view(B, Lq, Hq, d)


# ---------------------------------------------------------------------------------------------- exp(0) == 1 on the device
def test_exp_of_zero_is_exactly_one(ops, dev):
    """The count variant's 2-ulp bound needs every visible probability to be exactly 1: __expf(0) of the decode kernels, read
    from the fp32 split partials (m = 0, l = 1, O = the key's v row), and v_exp_f32(0) of the flash kernels, through a row whose
    single key must come back bit for bit."""
    d, T = 128, 8
    k, v = ac.rnd(1, 2, T, d, seed=1).to(dev), ac.rnd(1, 2, T, d, seed=2).to(dev)
    ws = (torch.full((4 * 2 * d,), 7.0, device=dev), torch.full((4 * 2 * 2,), 7.0, device=dev))
    out = ops.attn_decode(torch.zeros(1, 4, d, dtype=BF, device=dev), k, v, _i32([2], dev), kv_beg=_i32([0], dev), nsplit=2, ws=ws)
    ml = ws[1].view(4, 2, 2).cpu()
    assert torch.equal(ml, torch.tensor([0.0, 1.0]).expand(4, 2, 2)), ml             # every split holds one key: m = 0, l = expf(0)
    assert torch.equal(ws[0].view(4, 2, d).cpu(), v[0, :, :2].float().cpu().repeat_interleave(2, 0))
    assert torch.equal(out.view(4, d).float().cpu(), (v[0, :, :2].float().sum(1) / 2).to(BF).float().cpu().repeat_interleave(2, 0))
    for dh in (64, 40):                                                                # without and with the ones column
        kk, vv = ac.rnd(1, 5, dh, seed=3).to(dev), ac.rnd(1, 5, dh, seed=4).to(dev)
        o = ops.attention(torch.zeros(1, 5, dh, dtype=BF, device=dev), kk, vv, 1, causal=True)
        assert torch.equal(o[0, 0], vv[0, 0])                                          # row 0 sees key 0 only: 1 * v / 1


# ---------------------------------------------------------------------------------------------- group 1
@DTYPES
@pytest.mark.parametrize("mode", ac.SWEEP_MODES)
@pytest.mark.parametrize("d", ac.SWEEP_D)
def test_head_dim_sweep(ops, dev, d, mode, dtype):
    case = ac.sweep_case(d, dtype, mode)
    ac.check(run_case(ops, dev, case), case)


def test_pipelined_d64_from_one_fused_buffer(ops, dev):
    case = ac.sweep_case(64, ac.BF, "tiles")
    ac.check(run_case(ops, dev, case, one_buffer=True), case, "one buffer")


# ---------------------------------------------------------------------------------------------- groups 2, 3, 4 (+ their count variants)
@COUNT
@pytest.mark.parametrize("idx", range(N_FLASH))
def test_mask_edges(ops, dev, idx, count):
    case = ac.cases(count)[idx]
    ac.check(run_case(ops, dev, case), case)


@pytest.mark.parametrize("d", [64, 128])
def test_rope_rows_strided_views_exact(ops, dev, d):
    """rope_rows_ on the q and k column slices of a fused [T, 3 * nh * d + 8] buffer: one fp32 rotation (separately rounded
    products, one add) and one bf16 rounding, so the match is exact; every column outside the two views stays untouched."""
    from oracle import qwen_towers as oq
    g = torch.Generator().manual_seed(d)
    T, nh = 333, 3
    W = nh * d
    x0 = torch.randn(T, 3 * W + 8, generator=g).bfloat16()
    ang = torch.randn(T, d // 2, generator=g)
    cs = torch.cat([ang.cos(), ang.sin()], 1).contiguous()
    cos, sin = ang.cos().repeat(1, 2)[:, None], ang.sin().repeat(1, 2)[:, None]
    x = x0.to(dev)
    ops.rope_rows_(x[:, :W], cs.to(dev), nh)
    ops.rope_rows_(x[:, W:2 * W], cs.to(dev), nh)
    got = x.cpu()
    for c0 in (0, W):
        f = x0[:, c0:c0 + W].float().reshape(T, nh, d)
        assert torch.equal(got[:, c0:c0 + W].float().reshape(T, nh, d), (f * cos + oq._rot_half(f) * sin).bfloat16().float())
    assert torch.equal(got[:, 2 * W:], x0[:, 2 * W:])


# ---------------------------------------------------------------------------------------------- group 5 (+ its count variant)
@COUNT
@pytest.mark.parametrize("name", [c[0] for c in ac.DECODE])
def test_decode_split_kv(ops, dev, name, count):
    case = ac.cases(count)[N_FLASH + [c[0] for c in ac.DECODE].index(name)]
    ac.check(run_case(ops, dev, case), case, "attn_decode")


@COUNT
@pytest.mark.parametrize("inline", [0, 1, 2])
@pytest.mark.parametrize("name", [c[0] for c in ac.DECODE])
def test_decode_fused(ops, dev, name, inline, count):
    """attn_decode_fused: kv_end counts the appended token, whose k / v come from qkv (the cache slot holds junk before the call).
    Random variant: pre-rotation q / k / v in qkv; the reference is attn_ref64 on the rotated q that rope_kv_append returns and on
    the caches the fused launch leaves (bit-identical to rope_kv_append's), and the fused output is also held to the unfused one.
    Count variant: q = 0 (rotates to 0), the v part of qkv carries the class pattern of slot kv_end - 1."""
    from oracle.llama import LlamaCfg, rope_table
    from spider_amd import lib as slib
    case = ac.cases(count)[N_FLASH + [c[0] for c in ac.DECODE].index(name)]
    B, _, n_q, d = case.q.shape
    T_max, n_kv = case.k.shape[1:3]
    beg, end, nsplit = case.par["beg"], case.par["end"], case.par["nsplit"]
    new = [e - 1 for e in end]
    prev = slib.load().spider_set_attn_inline(inline)
    try:
        cs = rope_table(LlamaCfg(head_dim=d, rope_theta=1e6), T_max + 8).to(dev)
        qkv = ac.rnd(B, n_q + 2 * n_kv, d, seed=77 + n_q)
        kc0, vc0 = case.k.clone(), case.v.clone()
        for b in range(B):
            if count:
                qkv[b, :n_q] = 0
                qkv[b, n_q + n_kv:] = case.v[b, new[b]]
            kc0[b, new[b]], vc0[b, new[b]] = ac.JUNK, -ac.JUNK
        qkv = qkv.view(B, -1).to(dev)
        kv_end, kv_beg = _i32(end, dev), _i32(beg, dev)
        pos, slot = (kv_end - 1 - kv_beg).to(torch.int32), (kv_end - 1).to(torch.int32)
        k1, v1 = _cache(kc0, dev), _cache(vc0, dev)
        q = torch.empty(B, 1, n_q, d, dtype=BF, device=dev)
        ops.rope_kv_append(qkv, pos, slot, cs, q, k1, v1, B, 1, n_q, n_kv, d)
        unfused = ops.attn_decode(q.view(B, n_q, d), k1, v1, kv_end, kv_beg=kv_beg, nsplit=nsplit)
        k2, v2 = _cache(kc0, dev), _cache(vc0, dev)
        cnt = torch.zeros(B * n_kv, dtype=torch.int32, device=dev)
        ws = (torch.empty(B * n_q * nsplit * d, dtype=torch.float32, device=dev), torch.empty(B * n_q * nsplit * 2, dtype=torch.float32, device=dev))
        out = torch.empty(B, n_q * d, dtype=BF, device=dev)
        ops.attn_decode_fused(qkv, pos, cs, k2, v2, kv_end, kv_beg, cnt, n_q, nsplit, ws, out)
        torch.cuda.synchronize()
        assert torch.equal(k1, k2) and torch.equal(v1, v2), "KV append must be bit-identical"
        assert int(cnt.abs().sum()) == 0, "ticket counters must be back to zero"
        got, unf = out.cpu().view(B, 1, n_q, d), unfused.cpu().view(B, 1, n_q, d)
        if count:
            seen = torch.stack(case.vis)[:, 0]                                       # [B, T_max]: the appended slot included
            assert torch.equal(v2.cpu().permute(0, 2, 1, 3)[seen], case.v[seen])
            ac.check(got, case, f"fused inline={inline}")
            ac.check(unf, case, "unfused after rope_kv_append")
        else:
            kh, vh = k2.cpu().permute(0, 2, 1, 3), v2.cpu().permute(0, 2, 1, 3)
            ref = torch.stack([ac.attn_ref64(q[b].cpu(), kh[b], vh[b], case.vis[b], case.scale) for b in range(B)])
            ac.check(got, case, f"fused inline={inline}", ref=ref)
            ac.check(got, case, f"fused inline={inline} vs unfused", ref=unf.double(), tol=ac.TOL_FUSED_VS_UNFUSED)
    finally:
        slib.load().spider_set_attn_inline(0 if prev < 0 else prev)

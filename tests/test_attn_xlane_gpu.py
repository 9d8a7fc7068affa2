"""GPU: the two forms of the fused decode attention kernel (spider_set_attn_xlane: 0 = q RoPE in every wave, ds_bpermute exchanges,
4-byte tail stores; 1 = q RoPE once per block through LDS, DPP / v_permlane*_swap exchanges, 16-byte tail stores, the default) do
the same arithmetic in the same order: output, appended K / V cache rows and both partial workspaces are compared with
torch.equal. The same holds for the decode GEMVs, whose VALU cross-lane reductions run under the default GEMV schedule and
whose shuffle form under spider_set_gemv_sched(0) (lm_head keeps the shuffle form under both).

Attention cases (each through both forms): G = 1, 4, 7, 8; n_kv = 1, 2; B = 1 and 3 (a different kv_beg in every row); old-context
lengths 0, 1, 2, 15, 16, 17, 63, 64, 65, 200 (0: only the appended token; 15 / 16 / 17: one 16-row pass of the 4-wave block
partly filled, full, one over; 63 / 64 / 65: the same for its 64-row chunk; 200: a second chunk, and more than one row per lane
group of the 8-wave block); nsplit = 1, 4, 64 (64 splits of at most 200 rows: most splits own no row); T_max / nsplit below 96
(4 waves x 4 rows) and at least 96 (8 waves x 8 rows); combine forms 0, 1, 2; a cos / sin table of random angles (every row
distinct) read at pos = slot - kv_beg + 3 (pos != slot in every row)."""
import pytest
import torch

import attn_checks as ac

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
D = 128
LENS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 200]
ROWS3 = [(0, 1, 2), (15, 16, 17), (63, 64, 65), (200, 0, 17)]        # B = 3: every length once more, mixed within a launch
BEG3 = [0, 3, 5]
# (nsplit, T_max): T_max / nsplit = 95 -> the 4-wave block, >= 96 -> the 8-wave block
SHAPES = [(1, 95), (1, 210), (4, 380), (4, 384), (64, 6080), (64, 6144)]


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from spider_amd import lib as slib
    return slib.load()


def _rand(shape, seed, dev, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(dev)


@pytest.fixture(scope="module")
def table(dev):
    """[512, D] = [cos | sin] of random angles: no two rows alike, so a read of the wrong row shows"""
    g = torch.Generator().manual_seed(7)
    ang = torch.rand(512, D // 2, generator=g) * 6.28
    return torch.cat([ang.cos(), ang.sin()], 1).contiguous().to(dev)


_POOL = {}


def _pool(n_kv, T_max, dev):
    """K / V caches [3, n_kv, T_max, D], made once per shape and never written (every launch runs on a clone)"""
    key = (n_kv, T_max)
    if key not in _POOL:
        _POOL[key] = (_rand((3, n_kv, T_max, D), 100 + n_kv + T_max, dev), _rand((3, n_kv, T_max, D), 200 + n_kv + T_max, dev))
    return _POOL[key]


def fused_once(ops, dev, table, G, n_kv, lens, nsplit, T_max, seed):
    """one attn_decode_fused launch on fresh clones -> (out, k cache, v cache, partial o, partial (m, l), counters)"""
    B, n_q = len(lens), G * n_kv
    k0, v0 = _pool(n_kv, T_max, dev)
    k, v = k0[:B].clone(), v0[:B].clone()
    beg = BEG3[:B]
    kv_beg = torch.tensor(beg, dtype=torch.int32, device=dev)
    kv_end = torch.tensor([b + n + 1 for b, n in zip(beg, lens)], dtype=torch.int32, device=dev)
    pos = (kv_end - 1 - kv_beg + 3).to(torch.int32)
    qkv = _rand((B, (n_q + 2 * n_kv) * D), seed, dev)
    cnt = torch.zeros(B * n_kv, dtype=torch.int32, device=dev)
    ws = (torch.full((B * n_q * nsplit * D,), 7.0, device=dev), torch.full((B * n_q * nsplit * 2,), 7.0, device=dev))
    out = torch.full((B, n_q * D), 5.0, dtype=BF, device=dev)
    ops.attn_decode_fused(qkv, pos, table, k, v, kv_end, kv_beg, cnt, n_q, nsplit, ws, out)
    return out, k, v, ws[0], ws[1], cnt


def both_forms(lib, fn):
    """fn() under the old form and under the new one (previous setting restored); the setter must return what was set"""
    prev = lib.spider_set_attn_xlane(0)
    try:
        r0 = fn()
        assert lib.spider_set_attn_xlane(1) == 0
        r1 = fn()
        assert lib.spider_set_attn_xlane(1) == 1
    finally:
        lib.spider_set_attn_xlane(prev)
    torch.cuda.synchronize()
    return r0, r1


NAMES = ("out", "k cache", "v cache", "partial o", "partial m / l", "counters")


def assert_same(r0, r1, what):
    for name, a, b in zip(NAMES, r0, r1):
        assert torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} / {a.numel()} elements"


@pytest.mark.parametrize("inline", [0, 1, 2])
@pytest.mark.parametrize("G", [1, 4, 7, 8])
def test_forms_bit_identical(ops, lib, dev, table, G, inline):
    prev = lib.spider_set_attn_inline(inline)
    try:
        n = 0
        for n_kv in (1, 2):
            for nsplit, T_max in SHAPES:
                if inline and nsplit == 1:
                    continue                                   # one split has no combine: covered under inline = 0
                for lens in [(x,) for x in LENS] + ROWS3:
                    if BEG3[len(lens) - 1] + max(lens) + 1 > T_max:
                        continue                               # 200 old rows do not fit the 95-slot cache of the one-split 4-wave case
                    r0, r1 = both_forms(lib, lambda: fused_once(ops, dev, table, G, n_kv, lens, nsplit, T_max, 300 + n))
                    assert_same(r0, r1, f"G {G} n_kv {n_kv} lens {lens} nsplit {nsplit} T_max {T_max}")
                    assert int(r1[5].abs().sum()) == 0, "ticket counters must be back to zero"
                    n += 1
        assert n == 2 * (14 * (4 if inline else 5) + (0 if inline else 12))
    finally:
        lib.spider_set_attn_inline(0 if prev < 0 else prev)


def test_graph_replay(ops, lib, dev, table):
    """the new form captured in a graph and replayed three times (the ticket counters reset themselves) == the old form run eagerly"""
    G, n_kv, nsplit, T_max, lens = 7, 2, 4, 384, (200, 0, 17)
    prev_inline = lib.spider_set_attn_inline(2)
    try:
        prev = lib.spider_set_attn_xlane(0)
        try:
            old = fused_once(ops, dev, table, G, n_kv, lens, nsplit, T_max, 901)
            lib.spider_set_attn_xlane(1)
            B, n_q = len(lens), G * n_kv
            k0, v0 = _pool(n_kv, T_max, dev)
            k, v = k0[:B].clone(), v0[:B].clone()
            kv_beg = torch.tensor(BEG3, dtype=torch.int32, device=dev)
            kv_end = torch.tensor([b + n + 1 for b, n in zip(BEG3, lens)], dtype=torch.int32, device=dev)
            pos = (kv_end - 1 - kv_beg + 3).to(torch.int32)
            qkv = _rand((B, (n_q + 2 * n_kv) * D), 901, dev)
            cnt = torch.zeros(B * n_kv, dtype=torch.int32, device=dev)
            ws = (torch.full((B * n_q * nsplit * D,), 7.0, device=dev), torch.full((B * n_q * nsplit * 2,), 7.0, device=dev))
            out = torch.full((B, n_q * D), 5.0, dtype=BF, device=dev)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                ops.attn_decode_fused(qkv, pos, table, k, v, kv_end, kv_beg, cnt, n_q, nsplit, ws, out)     # warm-up outside the capture
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ops.attn_decode_fused(qkv, pos, table, k, v, kv_end, kv_beg, cnt, n_q, nsplit, ws, out)
            for rep in range(3):
                out.fill_(5.0)
                graph.replay()
                torch.cuda.synchronize()
                assert_same(old, (out, k, v, ws[0], ws[1], cnt), f"replay {rep}")
        finally:
            lib.spider_set_attn_xlane(prev)
    finally:
        lib.spider_set_attn_inline(0 if prev_inline < 0 else prev_inline)


def test_new_form_against_fp64_reference(ops, lib, dev):
    """the new form on the 64-split, 1537-key case of tests/attn_checks.py against attn_ref64 at the tolerance
    tests/test_attention_matrix_gpu.py::test_decode_fused holds split-KV decode to (the case's own: TOL_DECODE)"""
    from oracle.llama import LlamaCfg, rope_table
    case = ac.decode_case("len1537")
    B, _, n_q, d = case.q.shape
    T_max, n_kv = case.k.shape[1:3]
    beg, end, nsplit = case.par["beg"], case.par["end"], case.par["nsplit"]
    prev = lib.spider_set_attn_xlane(1)
    try:
        cs = rope_table(LlamaCfg(head_dim=d, rope_theta=1e6), T_max + 8).to(dev)
        qkv = ac.rnd(B, n_q + 2 * n_kv, d, seed=77 + n_q).view(B, -1).to(dev)
        kc0, vc0 = case.k.clone(), case.v.clone()
        for b in range(B):
            kc0[b, end[b] - 1], vc0[b, end[b] - 1] = ac.JUNK, -ac.JUNK
        kv_end = torch.tensor(end, dtype=torch.int32, device=dev)
        kv_beg = torch.tensor(beg, dtype=torch.int32, device=dev)
        pos, slot = (kv_end - 1 - kv_beg).to(torch.int32), (kv_end - 1).to(torch.int32)
        k1, v1 = kc0.permute(0, 2, 1, 3).contiguous().to(dev), vc0.permute(0, 2, 1, 3).contiguous().to(dev)
        q = torch.empty(B, 1, n_q, d, dtype=BF, device=dev)
        ops.rope_kv_append(qkv, pos, slot, cs, q, k1, v1, B, 1, n_q, n_kv, d)        # the rotated q and the caches the reference reads
        k2, v2 = kc0.permute(0, 2, 1, 3).contiguous().to(dev), vc0.permute(0, 2, 1, 3).contiguous().to(dev)
        cnt = torch.zeros(B * n_kv, dtype=torch.int32, device=dev)
        ws = (torch.empty(B * n_q * nsplit * d, dtype=torch.float32, device=dev), torch.empty(B * n_q * nsplit * 2, dtype=torch.float32, device=dev))
        out = torch.empty(B, n_q * d, dtype=BF, device=dev)
        ops.attn_decode_fused(qkv, pos, cs, k2, v2, kv_end, kv_beg, cnt, n_q, nsplit, ws, out)
        torch.cuda.synchronize()
        assert torch.equal(k1, k2) and torch.equal(v1, v2), "KV append must be bit-identical to rope_kv_append's"
        kh, vh = k2.cpu().permute(0, 2, 1, 3), v2.cpu().permute(0, 2, 1, 3)
        ref = torch.stack([ac.attn_ref64(q[b].cpu(), kh[b], vh[b], case.vis[b], case.scale) for b in range(B)])
        ac.check(out.cpu().view(B, 1, n_q, d), case, "fused, VALU cross-lane form", ref=ref)
    finally:
        lib.spider_set_attn_xlane(prev)


# ---------------------------------------------------------------------------------------------- GEMVs and lm_head
def both_scheds(lib, fn):
    """fn() under GEMV schedule 0 (__shfl_xor reductions) and under the default (VALU reductions in gemv_kernel); previous setting restored"""
    prev = lib.spider_set_gemv_sched(0)
    try:
        y0 = [t.clone() for t in fn()]
        assert lib.spider_set_gemv_sched(1) == 0
        y1 = [t.clone() for t in fn()]
    finally:
        lib.spider_set_gemv_sched(prev)
    for a, b in zip(y0, y1):
        assert torch.equal(a, b), f"schedules differ in {int((a != b).sum())} / {a.numel()} elements"
    return y1


# the smallest K of tests/test_gemv_sched_gpu.py's table that reaches each staging path of the SCHED 1 / 2 instantiations:
#   gemv_kernel<B, 1, false, true, 4, 1>  K 64: plain staging and the normalised row held in registers (block_sum), B = 1 and 2
#   gemv_kernel<1, 1, false, true, 4, 2>  K 4104: plain staging with a k loop, and the normalised row re-read in batches
#   gemv_kernel<1, 1, false, true, 8, 2>  K 8192: the 8-wave long-K form (plain staging; the fused norm caps K below it)
#   gemv_kernel<B, 1, true, true, 4, 2>   K 1032: gate / up, plain and normalised, B = 1 and 4
@pytest.mark.parametrize("B,N,K,norm", [(1, 7, 64, False), (1, 7, 64, True), (2, 24, 64, True), (1, 37, 4104, False), (1, 37, 4104, True),
                                        (1, 16, 8192, False)])
def test_gemv_valu_reductions(ops, lib, dev, B, N, K, norm):
    W, x = _rand((N, K), 1, dev, 0.05), _rand((B, K), 2, dev)
    nw = (1 + 0.1 * _rand((K,), 5, dev).float()).to(BF) if norm else None
    y, = both_scheds(lib, lambda: [ops.gemv(W, x, norm_w=nw, eps=1e-5)])
    assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("norm", [False, True])
def test_gemv_swiglu_valu_reductions(ops, lib, dev, B, norm):
    I, K = 20, 1032
    W, x = _rand((2 * I, K), 1, dev, 0.05), _rand((B, K), 2, dev)
    nw = (1 + 0.1 * _rand((K,), 5, dev).float()).to(BF) if norm else None
    y, = both_scheds(lib, lambda: [ops.gemv_swiglu(W, x, norm_w=nw, eps=1e-5)])
    assert bool(torch.isfinite(y.float()).all()) and float(y.float().abs().max()) > 0


@pytest.mark.parametrize("norm", [False, True])
def test_lm_head_same_under_both_schedules(ops, lib, dev, norm):
    """lmhead_partial_kernel<1, 2>: its VALU form measured no better than the shuffle form and is not in the code, so the GEMV
    schedule must not change its ids or logits. V = 333 (6 blocks, the last one partly filled, an odd row left over), K = 1032"""
    V, K = 333, 1032
    W, x = _rand((V, K), 11, dev, 0.05), _rand((1, K), 12, dev)
    nw = (1 + 0.1 * _rand((K,), 5, dev).float()).to(BF) if norm else None

    def run():
        logits = torch.zeros(1, V, dtype=BF, device=dev)
        return [ops.lm_head_argmax(W, x, norm_w=nw, eps=1e-5, logits=logits), logits]
    ids, logits = both_scheds(lib, run)
    assert int(ids[0]) == int(logits.float().argmax()) and float(logits.float().abs().max()) > 0

"""GPU: the processed lm_head + arg-max entry points (repetition penalty / ban set / EOS-before-min_new in the epilogue), the token
bitmap writer and the bitmap-updating decode_advance.

The processed ops must choose EXACTLY the lowest-index arg-max of the processors applied on the CPU, in fp32, to the op's own raw
bf16 logits output: the kernel's arithmetic (one fp32 multiply or one IEEE fp32 division per seen id, -inf for banned ids) is the
same as the CPU's, so there is no tolerance.

Weights: rows J1 < J2 are identical and aligned with every activation row, so they are the raw winners, exactly tied, in every
sequence; the scenarios then decide between them and the rest through the bitmaps and parameters alone."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 256
J1, J2 = 5, 37          # the tied raw winners (two different bitmap words)


def _pack(mask: torch.Tensor) -> torch.Tensor:
    """bool [B, V] -> bitmap words [B, ceil(V/32)] (uint32 bit patterns in an int32 tensor)"""
    B, V = mask.shape
    W = (V + 31) // 32
    m = np.zeros((B, W * 32), dtype=np.uint64)
    m[:, :V] = mask.cpu().numpy()
    words = (m.reshape(B, W, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


def _unpack(words: torch.Tensor, V: int) -> torch.Tensor:
    w = words.cpu().numpy().view(np.uint32).astype(np.uint64)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint64)) & 1
    return torch.from_numpy(bits.reshape(w.shape[0], -1)[:, :V].astype(bool))


def _reference(raw, seen, ban, p, eos, n_hist, min_new):
    """the processors on the CPU in fp32, as transformers applies them (RepetitionPenalty: score < 0 ? score * p : score / p)"""
    lv = raw.float().clone()
    lv = torch.where(seen, torch.where(lv < 0, lv * p, lv / p), lv)
    lv[ban] = -math.inf
    for b in range(lv.shape[0]):
        if int(n_hist[b]) < min_new:
            for t in eos:
                lv[b, t] = -math.inf
    return lv.argmax(-1)        # first (lowest) index among equal maxima; 0 when everything is -inf


class _Case:
    """one (V, B, layout): weights, activations, the raw logits of the unprocessed op, and a runner for the processed op"""

    def __init__(self, dev, V, B, fm):
        from spider_amd import ops
        self.ops, self.dev, self.V, self.B, self.fm = ops, dev, V, B, fm
        g = torch.Generator().manual_seed(1000 * V + 16 * B + fm)
        base = torch.randn(K, generator=g)
        W = torch.randn(V, K, generator=g) * 0.5
        W[J1] = base
        W[J2] = base
        x = base[None] + 0.5 * torch.randn(B, K, generator=g)
        self.W = W.bfloat16().to(dev)
        self.x = x.bfloat16().to(dev)
        self.Wfm = ops.repack_fm16(self.W) if fm else None
        lg = torch.empty(B, V, dtype=torch.bfloat16, device=dev)
        self.raw_ids = self._run(None, lg).cpu().long()
        self.raw = lg.float().cpu()
        # what the scenarios build on: J1 / J2 tie exactly and win raw in every row, with a positive logit
        assert torch.equal(self.raw[:, J1], self.raw[:, J2]) and bool((self.raw[:, J1] > 0).all())
        assert torch.equal(self.raw_ids, torch.full((B,), J1)) and torch.equal(self.raw.argmax(-1), self.raw_ids)

    def _run(self, proc, logits=None):
        o = self.ops
        if proc is None:
            return o.lm_head_argmax_fm(self.Wfm, self.x, self.V, logits=logits) if self.fm else o.lm_head_argmax(self.W, self.x, logits=logits)
        if self.fm:
            return o.lm_head_argmax_fm_proc(self.Wfm, self.x, self.V, proc, logits=logits)
        return o.lm_head_argmax_proc(self.W, self.x, proc, logits=logits)

    def check(self, name, seen=None, ban=None, p=1.0, eos=(), n_hist=None, min_new=0):
        B, V, dev = self.B, self.V, self.dev
        z = torch.zeros(B, V, dtype=torch.bool)
        seen = z if seen is None else seen
        ban = z if ban is None else ban
        n_hist = torch.zeros(B, dtype=torch.int32) if n_hist is None else n_hist
        proc = dict(seen=_pack(seen).to(dev), ban=_pack(ban).to(dev), penalty=torch.tensor([p], dtype=torch.float32, device=dev),
                    min_new=torch.tensor([min_new], dtype=torch.int32, device=dev),
                    eos_ids=torch.tensor(list(eos) + [-1] * (8 - len(eos)), dtype=torch.int32, device=dev),
                    n_eos=torch.tensor([len(eos)], dtype=torch.int32, device=dev), n_hist=n_hist.to(dev))
        lg = torch.empty(B, V, dtype=torch.bfloat16, device=dev)
        got = self._run(proc, lg).cpu().long()
        assert torch.equal(lg.float().cpu(), self.raw), f"{name}: the logits output must stay the raw logits"
        want = _reference(self.raw, seen, ban, p, list(eos), n_hist, min_new)
        assert torch.equal(got, want), (name, got.tolist(), want.tolist())
        return got


def _mask(B, V, per_row):
    m = torch.zeros(B, V, dtype=torch.bool)
    for b, ids in per_row.items():
        if b < B:
            m[b, list(ids)] = True
    return m


@pytest.mark.parametrize("V", [97, 331, 4100])
@pytest.mark.parametrize("B,fm", [(1, False), (3, False), (8, False), (2, True), (8, True), (16, True)])
def test_processed_lm_head_equals_cpu_processors_on_raw_logits(dev, V, B, fm):
    c = _Case(dev, V, B, fm)
    raw = c.raw
    rows = range(B)
    allrows = lambda ids: _mask(B, V, {b: ids for b in rows})
    J = torch.full((B,), J1)
    third = raw.clone()
    third[:, [J1, J2]] = -math.inf
    third_id, third_v = third.argmax(-1), third.max(-1).values
    assert bool((third_v > 0).all())
    p_big = float((raw[:, J1] / third_v).max()) * 1.25        # pushes a seen J1 / J2 below the third-best logit in every row

    # neutral parameters, empty bitmaps: the unprocessed op's ids
    assert torch.equal(c.check("neutral"), c.raw_ids)
    # bits that do not matter to the winner: ids 0 and V-1, two ids of one word in one row, an id seen in one row only
    per = {0: [0, V - 1, 64, 70]}
    if B > 1:
        per[1] = [0, 70]
        per[B - 1] = per.get(B - 1, []) + [V - 1, 66]
    assert torch.equal(c.check("edges", seen=_mask(B, V, per), p=1.3), J)
    # the exact tie: unpenalised the lower id wins; the lower one seen -> division by p > 1 puts it below its twin
    assert torch.equal(c.check("tie, lower seen", seen=allrows([J1]), p=1.05), torch.full((B,), J2))
    assert torch.equal(c.check("tie, higher seen", seen=allrows([J2]), p=1.05), J)
    assert torch.equal(c.check("tie, both seen", seen=allrows([J1, J2]), p=1.05), J)
    # the raw winners seen with a positive logit and a penalty large enough: division decides, the third-best id wins
    assert torch.equal(c.check("division decides", seen=allrows([J1, J2]), p=p_big), third_id)
    # ... in one row and not in another
    if B > 1:
        got = c.check("per-row seen", seen=_mask(B, V, {0: [J1, J2]}), p=p_big)
        assert int(got[0]) == int(third_id[0]) and torch.equal(got[1:], J[1:])
    # a seen id with a NEGATIVE logit: everything but two negative-logit ids banned, the better one seen -> multiplication by p
    # makes it more negative than the other, which wins
    neg = raw.clone()
    neg[neg >= 0] = -math.inf
    a_id = neg.argmax(-1)                                       # the negative logit closest to zero, per row
    neg[neg >= neg.max(-1, keepdim=True).values] = -math.inf   # (and anything equal to it)
    b_id = neg.argmax(-1)                                       # the next one strictly below
    va, vb = raw[torch.arange(B), a_id], raw[torch.arange(B), b_id]
    assert bool((va < 0).all() and (vb < va).all())
    ban2 = torch.ones(B, V, dtype=torch.bool)
    ban2[torch.arange(B), a_id] = False
    ban2[torch.arange(B), b_id] = False
    assert torch.equal(c.check("two negatives", ban=ban2), a_id)
    p_neg = float((vb / va).max()) * 1.25
    seen_a = torch.zeros(B, V, dtype=torch.bool)
    seen_a[torch.arange(B), a_id] = True
    assert torch.equal(c.check("multiplication decides", seen=seen_a, ban=ban2, p=p_neg), b_id)
    # raw winner banned -> its twin; both banned -> the third; everything banned -> id 0
    assert torch.equal(c.check("winner banned", ban=allrows([J1])), torch.full((B,), J2))
    assert torch.equal(c.check("winners banned", ban=allrows([J1, J2])), third_id)
    assert torch.equal(c.check("all banned", ban=torch.ones(B, V, dtype=torch.bool)), torch.zeros(B, dtype=torch.long))
    # EOS = the raw winners: banned at n_hist = min_new - 1, allowed at n_hist = min_new (alternating rows)
    nh = torch.tensor([3 if b % 2 == 0 else 4 for b in rows], dtype=torch.int32)
    extra = next(t for t in range(V - 1, 0, -1) if t not in third_id.tolist())      # a third EOS id that is nobody's runner-up
    got = c.check("eos before min_new", eos=[J2, extra, J1], n_hist=nh, min_new=4)
    assert all(int(got[b]) == (int(third_id[b]) if b % 2 == 0 else J1) for b in rows)
    assert torch.equal(c.check("min_new 0", eos=[J1, J2], n_hist=torch.zeros(B, dtype=torch.int32), min_new=0), J)
    # everything at once on random bitmaps (a third of the ids seen, a tenth banned)
    g = torch.Generator().manual_seed(V + B)
    for p in (1.05, 1.3, 0.7):
        c.check(f"random p={p}", seen=torch.rand(B, V, generator=g) < 0.33, ban=torch.rand(B, V, generator=g) < 0.1, p=p,
                eos=[J1, 1, V - 1], n_hist=torch.randint(0, 6, (B,), generator=g, dtype=torch.int32), min_new=3)


@pytest.mark.parametrize("V", [97, 331])
def test_token_bitmap_set_against_numpy(dev, V):
    from spider_amd import ops
    B, n = 3, 50
    g = torch.Generator().manual_seed(V)
    ids = torch.randint(0, V, (B, n), generator=g, dtype=torch.int32)
    ids[:, 10] = ids[:, 3]                                      # duplicates
    ids[0, :4] = torch.tensor([0, V - 1, 31, 32], dtype=torch.int32)
    ids[1, :5] = torch.tensor([-1, V, V + 5, 2**31 - 1, -2**31], dtype=torch.int32)     # outside [0, V): ignored
    W = (V + 31) // 32
    before = torch.randint(-2**31, 2**31 - 1, (B, W), generator=g, dtype=torch.int64).to(torch.int32)
    before[:, -1] &= (1 << (V % 32)) - 1                        # no bit at or past V is set, and none may become set
    bm = before.clone().to(dev)
    ops.token_bitmap_set(ids.to(dev), bm, V)
    want = _unpack(before, V)
    for b in range(B):
        for t in ids[b].tolist():
            if 0 <= t < V:
                want[b, t] = True
    assert torch.equal(bm.cpu(), _pack(want))
    # a second bitmap from zeros, one id per row (the first generated token)
    bm2 = torch.zeros(B, W, dtype=torch.int32, device=dev)
    one = torch.tensor([[0], [V - 1], [40]], dtype=torch.int32)
    ops.token_bitmap_set(one.to(dev), bm2, V)
    assert torch.equal(_unpack(bm2, V), _mask(B, V, {0: [0], 1: [V - 1], 2: [40]}))


def test_decode_advance_seen_sets_one_bit_and_equals_decode_advance(dev):
    from spider_amd import ops
    B, V, cap = 5, 331, 16
    W = (V + 31) // 32
    g = torch.Generator().manual_seed(4)
    nxt = torch.tensor([0, V - 1, 64, 95, 200], dtype=torch.int32)
    mk = lambda: dict(next_ids=nxt.clone().to(dev), cur_ids=torch.arange(B, dtype=torch.int32).to(dev),
                      pos=torch.tensor([3, 9, 4, 4, 0], dtype=torch.int32).to(dev), slot=torch.full((B,), 9, dtype=torch.int32).to(dev),
                      kv_end=torch.full((B,), 10, dtype=torch.int32).to(dev),
                      hist=torch.full((B, cap), -7, dtype=torch.int32).to(dev), n_hist=torch.tensor([1, 2, 3, 15, 16], dtype=torch.int32).to(dev))
    a, b = mk(), mk()
    seen0 = torch.rand(B, V, generator=g) < 0.3
    seen0[torch.arange(B), nxt.long()] = False
    seen = _pack(seen0).to(dev)
    ops.decode_advance(a["next_ids"], a["cur_ids"], a["pos"], a["slot"], a["kv_end"], a["hist"], a["n_hist"])
    ops.decode_advance_seen(b["next_ids"], b["cur_ids"], b["pos"], b["slot"], b["kv_end"], seen, V, b["hist"], b["n_hist"])
    for k in a:
        assert torch.equal(a[k], b[k]), k
    after = _unpack(seen, V)
    flipped = after ^ seen0
    assert torch.equal(flipped.sum(1), torch.ones(B, dtype=torch.long))
    assert bool(flipped[torch.arange(B), nxt.long()].all())
    # a bit that is already set stays set, nothing else moves
    b["next_ids"].copy_(nxt.to(dev))
    ops.decode_advance_seen(b["next_ids"], b["cur_ids"], b["pos"], b["slot"], b["kv_end"], seen, V, b["hist"], b["n_hist"])
    assert torch.equal(_unpack(seen, V), after)

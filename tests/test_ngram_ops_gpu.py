"""GPU: ops.ngram_ban and ops.decode_advance_seen_ngram against the host definition (spider_amd.llm.ngram_banned_host), exact
equality of the bitmap words. Sequences are drawn over a handful of token ids so that n-grams repeat; the slack of prompt_ids behind
n_prompt and of hist behind n_hist[b] is filled with one of those ids, so a scan that read past the sequence would ban it."""
import random

import pytest
import torch

from spider_amd.llm import ngram_banned_host

pytestmark = pytest.mark.gpu

PCAP, CAP = 24, 48


def _alphabet(V):
    return [0, 31, 32, V - 1, V // 2] + ([4095, 4096] if V > 4096 else [63, 64])


def _words(V, rows_of_ids):
    """int32 [B, ceil(V/32)] with the bits of the ids in [0, V) of every row set"""
    W = (V + 31) // 32
    out = torch.zeros(len(rows_of_ids), W, dtype=torch.int64)
    for b, ids in enumerate(rows_of_ids):
        for t in ids:
            if 0 <= t < V:
                out[b, t >> 5] |= 1 << (t & 31)
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)


def _noisy_periodic(rng, al, L, noise=0.125):
    """a motif of 2..5 ids repeated, one position in eight replaced: n-grams of every tested size repeat, and not everywhere"""
    motif = [rng.choice(al) for _ in range(rng.randint(2, 5))]
    return [rng.choice(al) if rng.random() < noise else motif[i % len(motif)] for i in range(L)]


def _buffers(dev, V, n, P, prompts, hists, static, fill):
    B = len(hists)
    prompt_ids = torch.full((B, PCAP), fill, dtype=torch.int32)
    hist = torch.full((B, CAP), fill, dtype=torch.int32)
    for b in range(B):
        prompt_ids[b, :P] = torch.tensor(prompts[b][:P], dtype=torch.int32)
        hist[b, :len(hists[b])] = torch.tensor(hists[b], dtype=torch.int32)
    W = (V + 31) // 32
    ng = dict(prompt_ids=prompt_ids.to(dev), n_prompt=torch.tensor([P], dtype=torch.int32, device=dev),
              ngram=torch.tensor([n], dtype=torch.int32, device=dev), ban=_words(V, static).to(dev),
              ban_step=torch.full((B, W), 0x5a5a5a5a, dtype=torch.int32, device=dev))
    return ng, hist.to(dev), torch.tensor([len(h) for h in hists], dtype=torch.int32, device=dev)


def _want(V, n, P, prompts, hists, static):
    return _words(V, [set(static[b]) | ngram_banned_host(list(prompts[b][:P]) + list(hists[b]), n) for b in range(len(hists))])


def _check(dev, V, n, P, prompts, hists, static=None, fill=None):
    from spider_amd import ops
    B = len(hists)
    static = static if static is not None else [[] for _ in range(B)]
    fill = _alphabet(V)[0] if fill is None else fill
    ng, hist, n_hist = _buffers(dev, V, n, P, prompts, hists, static, fill)
    ban0, hist0 = ng["ban"].clone(), hist.clone()
    ops.ngram_ban(ng, hist, n_hist, V)
    want = _want(V, n, P, prompts, hists, static)
    assert torch.equal(ng["ban_step"].cpu(), want), (V, n, P, prompts, hists)
    assert torch.equal(ng["ban"], ban0) and torch.equal(hist, hist0)        # inputs untouched
    return want


@pytest.mark.parametrize("n", [1, 2, 3, 7])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", [331, 4099])
def test_random_rows_against_host(dev, V, B, n):
    """rows of different n_hist in one launch, a shared prompt length, static ban bits that must survive, ids outside [0, V)"""
    rng = random.Random(V * 100 + B * 10 + n)
    al = _alphabet(V)
    added = 0
    for P in (0, 5, PCAP):
        lens = [rng.choice([0, 1, n - 1, n, 17, CAP]) for _ in range(B)]
        lens[0] = CAP
        seqs = [_noisy_periodic(rng, al, P + l, 0.125 if b else 0.0) for b, l in enumerate(lens)]   # row 0: exactly periodic
        prompts, hists = [s[:P] for s in seqs], [s[P:] for s in seqs]
        if P >= 5:
            prompts[0][1], prompts[0][3] = -3, V + 7       # ids outside [0, V) inside the prompt: they compare, they set nothing
            prompts[B - 1][P - 1] = V
        static = [[rng.randrange(V) for _ in range(9)] + [V - 1] for _ in range(B)]
        want = _check(dev, V, n, P, prompts, hists, static, fill=al[0])
        added += int((want != _words(V, static)).sum())
    assert added > 0        # the scan added bits of its own


@pytest.mark.parametrize("V", [331, 4099])
def test_boundaries(dev, V):
    a, b, c, d, x = _alphabet(V)[:5]
    # n_prompt = 0 (inputs_embeds): generated tokens alone; and n_hist = 0: the prompt alone
    _check(dev, V, 2, 0, [[], []], [[a, b, c, a], [a, a]])
    _check(dev, V, 2, 4, [[a, b, c, a], [d, d, d, d]], [[], []])
    _check(dev, V, 1, 3, [[a, b, c]], [[]])
    # the matching n-gram straddles the prompt / generated boundary: (a b) -> c with a the last prompt id
    w = _check(dev, V, 3, 2, [[x, a]], [[b, c, d, a, b]], fill=d)
    assert torch.equal(w, _words(V, [[c]]))
    # ... and the tail itself straddles it
    w = _check(dev, V, 3, 4, [[a, b, c, a]], [[b]], fill=d)
    assert torch.equal(w, _words(V, [[c]]))
    # the match that ends at the last admissible start i = L - n bans the sequence's last token; the start one past it would
    # compare the tail with itself and ban the slack token behind the sequence
    w = _check(dev, V, 3, 1, [[x]], [[a, a, a]], fill=d)
    assert torch.equal(w, _words(V, [[a]]))
    w = _check(dev, V, 2, 0, [[]], [[b, a]], fill=d)        # one past the last start: (a) -> slack; must ban nothing
    assert int(w.ne(0).sum()) == 0
    # L + 1 == n (the tail is the whole sequence: no start position) and L + 1 == n - 1 (tail longer than the sequence)
    for L in (2, 1, 0):
        w = _check(dev, V, 3, 1 if L else 0, [[a]], [[a] * (L - 1) if L else []], fill=a)
        assert int(w.ne(0).sum()) == 0
    w = _check(dev, V, 7, 3, [[a, a, a]], [[a, a]], static=[[5]], fill=a)     # L + 1 == n - 1; the static bit survives
    assert torch.equal(w, _words(V, [[5]]))
    # an id outside [0, V) as the token behind a match sets nothing; as part of the (n-1)-gram it matches itself
    w = _check(dev, V, 2, 3, [[a, V + 9, a]], [[]])
    assert int(w.ne(0).sum()) == 0
    w = _check(dev, V, 2, 3, [[-4, c, b]], [[-4]])
    assert torch.equal(w, _words(V, [[c]]))
    # size 0 or below: ban_step = ban; a size far beyond any sequence bans nothing
    for n in (0, -2, 2 ** 31 - 1):
        w = _check(dev, V, n, 2, [[a, a]], [[a, a, a]], static=[[0, V - 1]])
        assert torch.equal(w, _words(V, [[0, V - 1]]))


@pytest.mark.parametrize("n", [1, 2, 3, 7])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", [331, 4099])
def test_advance_form_equals_advance_seen_then_ngram_ban(dev, V, B, n):
    from spider_amd import ops
    rng = random.Random(V + 31 * B + n)
    small = _alphabet(V)
    P = 6
    lens = [CAP - 1, 0, CAP, 5, n, 20, 1, 9][:B]        # n_hist = CAP: the token is not stored, the counter still moves
    seqs = [_noisy_periodic(rng, small, P + l + 1, 0.125 if b else 0.0) for b, l in enumerate(lens)]    # row 0: exactly periodic
    prompts, hists, nxt = [s[:P] for s in seqs], [s[P:-1] for s in seqs], [s[-1] for s in seqs]
    static = [[rng.randrange(V) for _ in range(5)] for _ in range(B)]
    if B > 1:
        nxt[1] = V + 3                                   # outside the vocabulary: no seen bit, no ban bit
    W = (V + 31) // 32

    def mk():
        ng, hist, n_hist = _buffers(dev, V, n, P, prompts, hists, static, small[0])
        cur = dict(next_ids=torch.tensor(nxt, dtype=torch.int32, device=dev), cur_ids=torch.arange(B, dtype=torch.int32, device=dev),
                   pos=torch.arange(3, 3 + B, dtype=torch.int32, device=dev), slot=torch.full((B,), 9, dtype=torch.int32, device=dev),
                   kv_end=torch.full((B,), 10, dtype=torch.int32, device=dev), hist=hist, n_hist=n_hist,
                   seen=_words(V, [h[:3] for h in hists]).to(dev))
        return ng, cur

    nga, ca = mk()
    ngb, cb = mk()
    ops.decode_advance_seen(ca["next_ids"], ca["cur_ids"], ca["pos"], ca["slot"], ca["kv_end"], ca["seen"], V, ca["hist"], ca["n_hist"])
    ops.ngram_ban(nga, ca["hist"], ca["n_hist"], V)
    ops.decode_advance_seen_ngram(cb["next_ids"], cb["cur_ids"], cb["pos"], cb["slot"], cb["kv_end"], cb["seen"], V, cb["hist"],
                                  cb["n_hist"], ngb)
    for k in ca:
        assert torch.equal(ca[k], cb[k]), k
    assert cb["n_hist"].tolist() == [l + 1 for l in lens]
    for k in ("prompt_ids", "n_prompt", "ngram", "ban"):
        assert torch.equal(nga[k], ngb[k]), k
    # every row of the fused form equals the host definition on the advanced sequence (it carries the new token itself), and the
    # stand-alone op on the advanced state -- but for a row whose history was full: that token is in no buffer for the latter
    want = _want(V, n, P, prompts, [h + [t] for h, t in zip(hists, nxt)], static)
    got = ngb["ban_step"].cpu()
    assert got.shape == (B, W) and torch.equal(got, want), (hists, nxt)
    for b in range(B):
        if lens[b] < CAP:
            assert torch.equal(nga["ban_step"][b].cpu(), got[b]), b
    assert bool((want != _words(V, static)).any())      # the scan added bits of its own

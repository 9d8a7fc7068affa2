"""GPU: the two sampling launches (spider_sample_partial_bf16 + spider_sample_select_f32, csrc/sample.hip) on synthetic bf16 logits
against the fp64 host restatement (tests/sample_checks.py: exact candidate lists, derived bound DELTA on the masses), over
  V     70 (one short slice, 64 < V), 331 (odd: rows not 16-byte aligned), 4096 (one slice exactly full), 8200 (three slices, 8-token tail)
  rows  1, 3, 8     top_k 1, 5, 50, 64     top_p 1.0, 0.9, 0.3, 1e-6     T 0.7, 1.0, 1.5     with / without the processors' bitmaps
with planted duplicate values (the id tie rule, inside the list and at the top-k cut), and one chi-square check of 4096 draws."""
import pytest
import torch

from sample_checks import check_sample_step, near_a_boundary, pack_bits
from spider_amd.llm import process_logits_host, sample_token_host, sample_uniform_host

pytestmark = pytest.mark.gpu

VS, ROWS = (70, 331, 4096, 8200), (1, 3, 8)
TOP_K, TOP_P, TEMP = (1, 5, 50, 64), (1.0, 0.9, 0.3, 1e-6), (0.7, 1.0, 1.5)
PEN, MIN_NEW, ROW0 = 1.3, 3, 5


def make_case(V, rows, bitmaps):
    """raw bf16 logits [rows, V] with planted duplicates, the processors' state (or None), the processed logits [rows, V] fp32, the
    steps n_hist [rows] and the seed -- all on the host, from fixed seeds"""
    g = torch.Generator().manual_seed(7 * V + 3 * rows + bitmaps)
    # unit spread: the smallest of 64 candidates keeps a mass well above DELTA * P even at T = 0.7 and V = 70, so a top_p of 1.0
    # does not sit within DELTA of every tail rank's prefix mass (logits spread like a language model's make that the rule)
    raw = torch.randn(rows, V, generator=g).to(torch.bfloat16)
    for r in range(rows):       # the row's best value three times (first / middle / last token: every slice, the tail) ...
        top = raw[r].float().max() + 0.5
        raw[r, [r, V // 2, V - 1]] = top.to(torch.bfloat16)
        order = raw[r].float().sort(descending=True, stable=True)[1]
        for k in (5, 50):       # ... and a tie across the cut of top_k = 5 and 50: rank k takes the value of rank k - 1
            raw[r, order[k]] = raw[r, order[k - 1]]
    n_hist = torch.tensor([(2 * r + 1) % 7 for r in range(rows)], dtype=torch.int32)      # steps below and above MIN_NEW
    seed = (0x9E3779B97F4A7C15 * (V + rows)) % 2 ** 64
    if not bitmaps:
        return dict(raw=raw, x=raw.float(), n_hist=n_hist, seed=seed, proc=None)
    seen = torch.rand(rows, V, generator=g) < 0.15
    seen[:, V // 2] = True                              # one of the planted maxima is penalised
    ban = sorted({3, V - 1, int(torch.randint(0, V, (1,), generator=g))})       # ... one is banned
    eos = [0, V - 2, V // 3]                            # row 0's third maximum (token 0) is an EOS id: gone while n_hist < MIN_NEW
    banm = torch.zeros(rows, V, dtype=torch.bool)
    banm[:, ban] = True
    x = torch.stack([process_logits_host(raw[r:r + 1], seen[r:r + 1], PEN, ban, eos, int(n_hist[r]), MIN_NEW)[0] for r in range(rows)])
    proc = dict(seen=pack_bits(seen), ban=pack_bits(banm), penalty=torch.tensor([PEN]), min_new=torch.tensor([MIN_NEW], dtype=torch.int32),
                eos_ids=torch.tensor(eos + [-1] * 5, dtype=torch.int32), n_eos=torch.tensor([len(eos)], dtype=torch.int32), n_hist=n_hist)
    return dict(raw=raw, x=x, n_hist=n_hist, seed=seed, proc=proc)


@pytest.mark.parametrize("bitmaps", [False, True])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("V", VS)
def test_sample_step_matches_host(dev, V, rows, bitmaps):
    from spider_amd import ops
    c = make_case(V, rows, bitmaps)
    raw = c["raw"].to(dev)
    proc = None if c["proc"] is None else {k: v.to(dev) for k, v in c["proc"].items()}
    n_hist = c["n_hist"].to(dev)
    sm = ops.sample_state(rows, V, dev)
    next_ids = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    us = [sample_uniform_host(c["seed"], ROW0 + r, int(c["n_hist"][r])) for r in range(rows)]
    for top_k in TOP_K:
        for top_p in TOP_P:
            for T in TEMP:
                ops.sample_set_params(sm, T, top_k, top_p, c["seed"], ROW0)
                ops.sample_partial(raw, sm, proc)
                ops.sample_select(sm, n_hist, next_ids, V)
                tok, ct, cp, nk, u = (t.cpu() for t in (next_ids, sm["cand_tok"], sm["cand_p"], sm["n_keep"], sm["u"]))
                for r in range(rows):
                    check_sample_step(c["x"][r], T, top_k, top_p, us[r], ct[r], cp[r], nk[r], u[r], tok[r])
                    if top_k == 1 or top_p == 1e-6:      # greedy: the lowest id among the row's maxima
                        assert int(tok[r]) == int(c["x"][r].argmax()) and (top_k > 1 or int(nk[r]) == 1)


def test_ties_are_exercised_and_widening_is_rare():
    """On the host, over the cases of the test above (the fp64 reference alone decides both): the id tie rule is hit inside the
    candidate lists and at the top-k cut, and the cases in which either neighbour is accepted are at most 2 %."""
    st = {"cases": 0, "widened": 0, "ties": 0, "cut_ties": 0}
    for V in VS:
        for rows in ROWS:
            for bitmaps in (False, True):
                c = make_case(V, rows, bitmaps)
                for r in range(rows):
                    u = sample_uniform_host(c["seed"], ROW0 + r, int(c["n_hist"][r]))
                    full = c["x"][r].sort(descending=True, stable=True)[0]
                    for top_k in TOP_K:
                        for top_p in TOP_P:
                            for T in TEMP:
                                ref = sample_token_host(c["x"][r], T, top_k, top_p, u)
                                st["cases"] += 1
                                st["widened"] += near_a_boundary(ref, top_p, u)
                                st["ties"] += bool((ref["x"][1:] == ref["x"][:-1]).any())
                                st["cut_ties"] += bool(full[top_k - 1] == full[top_k])
    assert st["cases"] == sum(ROWS) * len(VS) * 2 * len(TOP_K) * len(TOP_P) * len(TEMP)
    assert st["ties"] > st["cases"] // 4 and st["cut_ties"] > st["cases"] // 8, st
    assert st["widened"] <= 0.02 * st["cases"], st


def test_null_bitmaps_equal_neutral_processors(dev):
    """seen = ban = NULL is the processors' neutral state: empty bitmaps, penalty 1, no EOS rule give the same outputs"""
    from spider_amd import ops
    V, rows = 8200, 3
    c = make_case(V, rows, False)
    raw, n_hist = c["raw"].to(dev), c["n_hist"].to(dev)
    W = ops.bitmap_words(V)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    proc = dict(seen=i32(rows, W), ban=i32(rows, W), penalty=torch.ones(1, device=dev), min_new=i32(1), eos_ids=i32(8), n_eos=i32(1),
                n_hist=n_hist)
    outs = []
    for pr in (None, proc):
        sm = ops.sample_state(rows, V, dev)
        ids = torch.zeros(rows, dtype=torch.int32, device=dev)
        ops.sample_set_params(sm, 0.8, 50, 0.9, c["seed"], 0)
        ops.sample_partial(raw, sm, pr)
        ops.sample_select(sm, n_hist, ids, V)
        outs.append([t.cpu() for t in (ids, sm["cand_tok"], sm["cand_p"], sm["n_keep"], sm["u"])])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_draws_follow_the_distribution(dev):
    """4096 draws of ONE row (64 launches of 64 rows: distinct (row, step) counters) against the fp64 probabilities of its nucleus by
    chi-square, threshold = the 1 - 1e-6 quantile (the draws are deterministic: this cannot flake). A biased uniform or an
    off-by-one in the CDF moves the statistic by hundreds."""
    from spider_amd import ops
    V, R, L = 331, 64, 64
    g = torch.Generator().manual_seed(3)
    row = -torch.rand(V, generator=g) * 4
    top = torch.randperm(V, generator=g)[:8]
    row[top] = torch.tensor([5.0, 4.75, 4.5, 4.5, 4.25, 4.0, 3.75, 3.5])
    raw = row.to(torch.bfloat16)[None].expand(R, V).contiguous()
    T, top_k, top_p, seed = 1.0, 50, 0.9, 0x1234567890ABCDEF
    ref = sample_token_host(raw[0].float(), T, top_k, top_p, 0.5)
    nk = ref["n_keep"]
    assert 6 <= nk <= 10
    prob = ref["p"][:nk] / ref["S"]
    sm = ops.sample_state(R, V, dev)
    ops.sample_set_params(sm, T, top_k, top_p, seed, 0)
    raw_d = raw.to(dev)
    ids = torch.zeros(R, dtype=torch.int32, device=dev)
    draws = []
    for step in range(L):
        ops.sample_partial(raw_d, sm)
        ops.sample_select(sm, torch.full((R,), step, dtype=torch.int32, device=dev), ids, V)
        draws.append(ids.cpu().clone())
        if step == 0:
            assert sm["u"].cpu().tolist() == [sample_uniform_host(seed, r, 0) for r in range(R)]
    draws = torch.cat(draws).long()
    kept = ref["tokens"][:nk]
    assert torch.isin(draws, kept).all()
    counts = torch.stack([(draws == t).sum() for t in kept]).double()
    expect = prob * draws.numel()
    stat = float(((counts - expect) ** 2 / expect).sum())
    tail = float(torch.special.gammaincc(torch.tensor((nk - 1) / 2.0, dtype=torch.float64), torch.tensor(stat / 2.0, dtype=torch.float64)))
    assert tail > 1e-6, (stat, counts.tolist(), expect.tolist())       # P(chi2_{nk-1} >= stat) > 1e-6  <=>  stat below the quantile

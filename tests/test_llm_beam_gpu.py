"""GPU: LlamaEngine.generate(num_beams=K) end to end: the beam step inside the decode graph, the KV reorder and the host replay.

  * every step of the trace passes the property check of tests/beam_checks.py, computed from the engine's own raw logits
    (return_logits) and the running scores the trace implies;
  * sequences_scores is the fp64 sum of log-probabilities along the returned ancestry / length^penalty, within n * delta;
  * KV / ancestry: for every running beam of the last step, the raw logits along its back-pointer chain match the fp32 oracle's
    teacher-forced logits of the same tokens: relative L2 < 2.5e-2 (the bound of tests/test_llm_engine.py) over the chain [N, V].
    A reorder that mixes histories up cannot pass: with two final beams' histories swapped the same figure is at least ten times
    that bound on these models (tests/test_beam_seeds_cpu.py, on the oracle), and one step on a foreign history alone moves it by
    about that step's own distance / sqrt(N);
  * graph and eager write identical traces, sync_every 1 and 5 return identical output, num_beams=1 is untouched by a beam call."""
import pytest
import torch

from beam_checks import check_beam_step, delta

pytestmark = pytest.mark.gpu

V, N, S = 331, 16, 9
BOUND = 2.5e-2


def _engine(dev, layers, max_batch, seed, row_major=False):       # the recipe of tests/test_llm_processors_gpu.py
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd.llm import LlamaEngine, LLMConfig
    ocfg = LlamaCfg(256, layers, 2, 1, 128, 512, V, 10000.0, None, 1e-6, False, 256)
    w = LlamaOracle.random_weights(ocfg, seed=seed, std=0.08)
    eng = LlamaEngine(LLMConfig(**ocfg.__dict__), w, dev, max_batch=max_batch, max_len=128)
    if row_major:
        eng.FM_MIN_BATCH = 99
    return eng, LlamaOracle(ocfg, w)


def _inputs(eng, B, seed, mode):
    ids = torch.randint(3, V, (B, S), generator=torch.Generator().manual_seed(100 + seed))
    am = torch.ones(B, S, dtype=torch.long)
    if mode == "embeds":
        return dict(inputs_embeds=eng.embed_tokens(ids)), ids, am
    for b in range(B):
        ids[b, :2 + b] = 0
        am[b, :2 + b] = 0
    return dict(input_ids=ids, attention_mask=am), ids, am


def _trace(eng, B, K, C, n):
    st = eng._graphs[(B, False, True, 0, "beam", K, C)][0]
    return tuple(t[:n].cpu().clone() for t in st["beam"]["trace"]), st


def _running(score, beam, tok, K, eos):
    """the running beams a trace entry implies: the first K continuations whose token is no EOS id"""
    B, C = score.shape
    keep = [[c for c in range(C) if int(tok[b, c]) not in (eos or ())][:K] for b in range(B)]
    idx = torch.tensor(keep)
    return score.gather(1, idx), beam.gather(1, idx), tok.gather(1, idx)


def _check_steps(trace, logits, B, K, eos):
    """property check of every step; returns the running (scores, beams, tokens) of every step"""
    run = torch.zeros(B, K)
    run[:, 1:] = -1e9
    hist = []
    for t in range(trace[0].shape[0]):
        sc, bm, tk = (x[t] for x in trace)
        nr, ns, nt = _running(sc, bm, tk, K, eos)
        check_beam_step(logits[:, t].float(), run, eos, sc, bm, tk, nr, ns, nt)
        hist.append((nr, ns, nt))
        run = nr
    return hist


def _chains(hist, b, K):
    """for every running beam of the last step of batch row b: (tokens [n], beam whose logits chose each token [n])"""
    n = len(hist)
    out = []
    for k in range(K):
        toks, rows, cur = [], [], k
        for t in range(n - 1, -1, -1):
            toks.append(int(hist[t][2][b, cur]))
            cur = int(hist[t][1][b, cur])
            rows.append(cur)
        out.append((toks[::-1], rows[::-1]))
    return out


def _teacher(oracle, ids_row, am_row, toks):
    """fp32 oracle logits [n, V] that chose toks[0..n-1]: one forward over prompt + toks[:-1]"""
    n = len(toks)
    ids = torch.cat([ids_row, torch.tensor(toks[:-1], dtype=torch.long)])[None]
    am = torch.cat([am_row, torch.ones(n - 1, dtype=torch.long)])[None]
    pos = (am.cumsum(-1) - 1).clamp(min=0)
    lg, _, _ = oracle.forward(ids, pos, None, am)
    return lg[0, S - 1:]


# (B, K, weight seed, layers): seeds kept where swapping two final beams' histories moves the chain figure to >= 10 * BOUND on the oracle
# (tests/test_beam_seeds_cpu.py)
CONFIGS = [(1, 2, 21, 2), (1, 4, 23, 2), (2, 4, 25, 3), (1, 8, 28, 2)]


@pytest.mark.parametrize("mode", ["ids", "embeds"])
@pytest.mark.parametrize("row_major", [False, True])
@pytest.mark.parametrize("B,K,seed,layers", CONFIGS)
def test_beam_generate(dev, B, K, seed, layers, row_major, mode):
    eng, oracle = _engine(dev, layers, 8, seed, row_major)
    inp, ids, am = _inputs(eng, B, seed, mode)
    kw = dict(num_beams=K, max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
    # --- no EOS: N steps, the K best returned; graph against eager
    free = eng.generate(**inp, **kw, num_return_sequences=K)
    C = 2 * K
    tr_g, st = _trace(eng, B, K, C, N)
    assert free.logits.shape == (B * K, N, V) and free.sequences.shape == (B * K, N + (S if mode == "ids" else 0))
    last = (st["beam"]["run"].cpu().clone(), st["beam"]["src_beam"].cpu().clone(), st["next_ids"].cpu().view(B, K).clone())
    eager = eng.generate(**inp, **kw, num_return_sequences=K, use_graph=False)
    tr_e, _ = _trace(eng, B, K, C, N)
    for a, b in zip(tr_g, tr_e):
        assert torch.equal(a, b)
    assert torch.equal(free.sequences, eager.sequences) and torch.equal(free.logits, eager.logits)
    assert torch.equal(free.sequences_scores, eager.sequences_scores)
    logits = free.logits.cpu()
    hist = _check_steps(tr_g, logits, B, K, None)
    # the device's own running beams after the last step are the ones the trace implies
    assert torch.equal(last[0], hist[-1][0]) and torch.equal(last[1].long(), hist[-1][1]) and torch.equal(last[2].long(), hist[-1][2])
    # --- KV / ancestry against teacher forcing
    for b in range(B):
        chains = _chains(hist, b, K)
        ref = [_teacher(oracle, ids[b], am[b], toks) for toks, _ in chains]
        for (toks, rows), r in zip(chains, ref):
            got = torch.stack([logits[b * K + rows[t], t].float() for t in range(N)])      # [N, V] along the back-pointer chain
            rel = float((got - r).norm() / r.norm())
            assert rel < BOUND, (b, rel)
    # the returned sequences are these chains (no EOS: every hypothesis has N tokens), best first
    gen = free.sequences[:, -N:].cpu()
    for b in range(B):
        assert gen[b * K].tolist() == _chains(hist, b, K)[0][0]
    # --- an EOS id from the stream: hypotheses finish mid-way
    eos = [int(gen[0, 5])]
    for lp in (1.0, 0.0):
        kwe = dict(kw, eos_token_id=eos, pad_token_id=1, length_penalty=lp, num_return_sequences=K)
        o = eng.generate(**inp, **kwe)
        n = o.logits.shape[1]
        tr, _ = _trace(eng, B, K, C, n)
        lg = o.logits.cpu()
        _check_steps(tr, lg, B, K, eos)
        o5 = eng.generate(**inp, **kwe, sync_every=5)
        oe = eng.generate(**inp, **kwe, use_graph=False)
        for x in (o5, oe):
            assert torch.equal(o.sequences, x.sequences) and torch.equal(o.sequences_scores, x.sequences_scores)
            assert torch.equal(o.beam_indices, x.beam_indices) and torch.equal(o.logits, x.logits)
        # sequences_scores = sum of log-probs along the returned ancestry / length^lp
        seq, bi, ss = o.sequences[:, (S if mode == "ids" else 0):].cpu(), o.beam_indices.cpu(), o.sequences_scores.cpu()
        lsm = torch.log_softmax(lg.double(), -1)
        for j in range(seq.shape[0]):
            ln = int((bi[j] >= 0).sum())
            tot = sum(float(lsm[int(bi[j, t]), t, int(seq[j, t])]) for t in range(ln))
            assert abs(float(ss[j]) - tot / ln ** lp) <= n * delta(tot), (j, float(ss[j]), tot, ln)
            assert (seq[j, ln:] == 1).all()
        # the case counts: a hypothesis finished mid-way (the EOS id is a token of the free run's best beam, so it is among the
        # top K continuations of some step <= 5, whatever is returned in the end)
        assert any(int(tr[2][t, b, c]) in eos for t in range(min(n, 6)) for b in range(B) for c in range(K))


def test_greedy_is_untouched_by_a_beam_call(dev):
    eng, _ = _engine(dev, 2, 8, 21)
    fresh, _ = _engine(dev, 2, 8, 21)
    inp, ids, am = _inputs(eng, 2, 21, "ids")
    before = eng.generate(**inp, max_new_tokens=N)
    keys = set(eng._graphs)
    assert eng.would_capture(2, False, False, 0, num_beams=4) and not eng.would_capture(2, False, False, 0)
    eng.generate(**inp, max_new_tokens=N, num_beams=4)
    assert not eng.would_capture(2, False, False, 0, num_beams=4)
    assert set(eng._graphs) - keys == {(2, False, False, 0, "beam", 4, 8)}
    after = eng.generate(**inp, max_new_tokens=N)
    want = fresh.generate(**inp, max_new_tokens=N)
    assert torch.equal(before, want) and torch.equal(after, want)
    assert set(eng._graphs) - keys == {(2, False, False, 0, "beam", 4, 8)}      # num_beams=1: the same state key and graph as before


def test_beam_requests_outside_the_implemented_ground_raise(dev):
    eng, _ = _engine(dev, 2, 4, 21)
    inp, ids, am = _inputs(eng, 1, 21, "ids")
    with pytest.raises(ValueError, match="max_batch"):
        eng.generate(**inp, max_new_tokens=4, num_beams=8)
    with pytest.raises(NotImplementedError, match="generate only"):      # the split prefill / decode path is greedy
        eng.prefill_begin(**inp, max_new_tokens=4, num_beams=2)
    for kw in (dict(do_sample=True), dict(output_hidden_states=True), dict(repetition_penalty=1.3), dict(num_beam_groups=2),
               dict(stopping_criteria=[lambda i, s: False]), dict(suppress_tokens=[5])):
        with pytest.raises(NotImplementedError):
            eng.generate(**inp, max_new_tokens=4, num_beams=2, **kw)

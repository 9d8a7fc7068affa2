"""GPU: LlamaEngine.generate(no_repeat_ngram_size=n) on the processed decode path, greedy and sampled.

Replay check (as tests/test_llm_processors_gpu.py): with return_logits=True the engine returns the RAW logits of every step.
transformers' NoRepeatNGramLogitsProcessor and the other processors of the call, applied in fp32 on the CPU to the raw logits of
step t with the engine's own history up to t, must make the lowest-index arg-max the engine's token at every step of every row --
exact. Which ids the processor sees per input mode is pinned against HF's generate in tests/test_ngram_cpu.py.

The weight / prompt seeds of the replay test are ones for which the plain greedy stream of these prompts repeats a 3-gram (and so a
2-gram and a token) within N tokens in both input modes and both weight layouts, so the ban has work to do without any other
processor (few seeds do: a random tiny model rarely loops; candidates came from oracle.llama's greedy stream on the CPU, the choice
among them from the engines' own streams); every case asserts that it did (`touched`)."""
import dataclasses

import pytest
import torch

from sample_checks import check_sample_step
from spider_amd.llm import (ngram_banned_host, process_logits_host, resolve_logits_processors, sample_token_host,
                            sample_uniform_host)

pytestmark = pytest.mark.gpu

V, N, S = 331, 40, 9
SEED_B1, SEED_B3 = 45, 45
SEED_REPLAY_B3 = 39


def _engine(dev, layers, max_batch, seed, row_major=False, mrope=False):     # the recipe of tests/test_llm_processors_gpu.py
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd.llm import LlamaEngine, LLMConfig
    ocfg = LlamaCfg(256, layers, 2, 1, 128, 512, V, 10000.0, None, 1e-6, False, 256)
    w = LlamaOracle.random_weights(ocfg, seed=seed, std=0.08)
    cfg = LLMConfig(**ocfg.__dict__)
    if mrope:
        cfg = dataclasses.replace(cfg, mrope_section=(16, 24, 24))
    eng = LlamaEngine(cfg, w, dev, max_batch=max_batch, max_len=128)
    if row_major:
        eng.FM_MIN_BATCH = 99
    return eng


def _inputs(eng, B, seed, mode):
    """ids [B, S]; 'ids': left-padded input_ids (+ attention_mask), the pads are ids of the prompt; 'embeds': inputs_embeds only"""
    ids = torch.randint(3, V, (B, S), generator=torch.Generator().manual_seed(100 + seed))
    if mode == "embeds":
        return dict(inputs_embeds=eng.embed_tokens(ids)), None
    am = torch.ones(B, S, dtype=torch.long)
    for b in range(B):
        npad = 2 + b
        ids[b, :npad] = 0
        am[b, :npad] = 0
    return dict(input_ids=ids, attention_mask=am), ids


def _replay(gen, logits, prompt, n, eos=None, p=1.0, min_new=0, ban=()):
    """HF's processors on the raw logits, step by step. Returns (first mismatch or None, number of (row, step) pairs whose raw
    arg-max was n-gram-banned). Rows are compared up to their first EOS (afterwards the engine pads)."""
    from transformers import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                              SuppressTokensLogitsProcessor)
    gen, logits = gen.cpu().long(), logits.float().cpu()
    B, steps = gen.shape
    procs = []
    if p != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=p))
    procs.append(NoRepeatNGramLogitsProcessor(n))
    if eos and min_new > 0:
        procs.append(MinNewTokensLengthLogitsProcessor(0 if prompt is None else prompt.shape[1], min_new, eos))
    if ban:
        procs.append(SuppressTokensLogitsProcessor(list(ban)))
    alive = torch.ones(B, dtype=torch.bool)
    touched = 0
    for t in range(steps):
        hist = gen[:, :t] if prompt is None else torch.cat([prompt.long(), gen[:, :t]], 1)
        raw = logits[:, t]
        sc = raw.clone()
        for pr in procs:
            sc = pr(hist, sc)
        want = sc.argmax(-1)
        for b in range(B):
            if not alive[b]:
                continue
            if int(want[b]) != int(gen[b, t]):
                return (b, t, int(want[b]), int(gen[b, t])), touched
            touched += int(raw[b].argmax()) in ngram_banned_host(hist[b].tolist(), n)
        if eos:
            alive &= ~torch.isin(gen[:, t], torch.tensor(eos))
    return None, touched


# (name, layers, B, row_major, weight seed): B = 1 row-major with the folded norm; B = 3 fragment-major; B = 3 forced row-major
ENGINES = [("b1", 2, 1, False, SEED_B1), ("b3fm", 3, 3, False, SEED_REPLAY_B3), ("b3rm", 3, 3, True, SEED_REPLAY_B3)]


@pytest.mark.parametrize("case", ["alone", "together"])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("mode", ["ids", "embeds"])
@pytest.mark.parametrize("ename,layers,B,row_major,seed", ENGINES)
def test_ngram_generate_replays_under_hf_processors(dev, ename, layers, B, row_major, seed, mode, n, case):
    eng = _engine(dev, layers, B, seed, row_major)
    inp, prompt = _inputs(eng, B, seed, mode)
    plain_gen = eng.generate(**inp, max_new_tokens=N)[:, -N:].cpu()
    if case == "alone":
        kw, eos, pen, min_new, ban = {}, None, 1.0, 0, []
    else:
        # a penalty below 1 (it rewards repeats: more for the n-gram ban to refuse), an EOS id that the unprocessed row 0 emits
        # among its first 6 tokens, and a ban set: ids 0, V - 1
        eos = [int(plain_gen[0, 2])]
        ban = sorted({0, V - 1} - set(eos))
        pen, min_new = 0.4, 6
        kw = dict(repetition_penalty=pen, min_new_tokens=min_new, suppress_tokens=ban, eos_token_id=eos, pad_token_id=1)
    outs = {}
    for use_graph in (True, False):
        o = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True, use_graph=use_graph,
                         no_repeat_ngram_size=n, **kw)
        steps = o.logits.shape[1]
        gen = o.sequences[:, -steps:]
        bad, touched = _replay(gen, o.logits, prompt, n, eos, pen, min_new, ban)
        assert bad is None, f"graph={use_graph}: (row, step, HF replay, engine) = {bad}"
        assert touched > 0      # the case counts only if some raw winner was n-gram-banned
        outs[use_graph] = (gen, o.logits)
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])     # graph == eager, bit for bit
    assert set(eng._graphs) == {(B, False, False, 0), (B, False, True, 0, True, "ngram")}


def test_one_graph_serves_every_size_and_the_other_states_stay(dev):
    """a plain call and a processed call with no_repeat_ngram_size=0 create no "ngram" state and return, after n-gram requests on
    the same engine, what they returned before; the n-gram requests of sizes 2 and 3 share one captured graph"""
    B = 3
    eng = _engine(dev, 3, B, SEED_B3)
    inp, prompt = _inputs(eng, B, SEED_B3, "ids")
    plain = eng.generate(**inp, max_new_tokens=N)
    proc = eng.generate(**inp, max_new_tokens=N, repetition_penalty=1.3, no_repeat_ngram_size=0)
    assert torch.equal(plain, eng.generate(**inp, max_new_tokens=N, no_repeat_ngram_size=None))
    keys = set(eng._graphs)
    assert keys == {(B, False, False, 0), (B, False, False, 0, True)}
    graphs = {k: eng._graphs[k][1] for k in keys}
    assert eng.would_capture(B, no_repeat_ngram=True) and not eng.would_capture(B) and not eng.would_capture(B, processed=True)
    res = {}
    for n in (2, 3):
        o = eng.generate(**inp, max_new_tokens=N, no_repeat_ngram_size=n, return_dict_in_generate=True)
        res[n] = o.sequences[:, S:].cpu()
        if n == 2:
            assert not eng.would_capture(B, no_repeat_ngram=True)
            graph = eng._graphs[(B, False, False, 0, True, "ngram")][1]
        for b in range(B):      # no n-gram of the row's whole sequence occurs twice
            s = prompt[b].tolist() + res[n][b].tolist()
            grams = [tuple(s[i:i + n]) for i in range(len(s) - n + 1) if i + n > S]
            assert len(set(grams)) == len(grams) and not (set(grams) & {tuple(s[i:i + n]) for i in range(S - n + 1)})
    assert eng._graphs[(B, False, False, 0, True, "ngram")][1] is graph
    assert set(eng._graphs) - keys == {(B, False, False, 0, True, "ngram")}
    assert not torch.equal(res[2], res[3]) and not torch.equal(res[3], plain[:, S:].cpu())
    assert torch.equal(eng.generate(**inp, max_new_tokens=N), plain)
    assert torch.equal(eng.generate(**inp, max_new_tokens=N, repetition_penalty=1.3, no_repeat_ngram_size=0), proc)
    assert all(eng._graphs[k][1] is graphs[k] for k in keys)        # the same captured graphs as before
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            eng.generate(**inp, max_new_tokens=4, no_repeat_ngram_size=bad)
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        eng.generate(input_ids=inp["input_ids"][:1], max_new_tokens=4, num_beams=2, no_repeat_ngram_size=2)


def test_routes_return_the_same_tokens(dev):
    """sync_every 1 / 5, the split path on cache set 0 and on cache set 1, a request adopted from a staging set, hidden states"""
    B = 3
    eng = _engine(dev, 3, B, SEED_B3)
    inp, prompt = _inputs(eng, B, SEED_B3, "ids")
    kw = dict(max_new_tokens=N, no_repeat_ngram_size=2, repetition_penalty=0.8, suppress_tokens=[0, 5])
    want = eng.generate(**inp, **kw)
    assert not torch.equal(want, eng.generate(**inp, **dict(kw, no_repeat_ngram_size=0)))
    assert torch.equal(eng.generate(**inp, **kw, sync_every=5), want)
    assert torch.equal(eng.decode_finish(eng.prefill_begin(**inp, **kw)), want)
    # another request's values (size, prompt, bans) are left in the buffers of sets 0 and 1; every request must bring its own
    other, _ = _inputs(eng, B, SEED_B3 + 1, "ids")
    eng.generate(**other, max_new_tokens=6, no_repeat_ngram_size=1, suppress_tokens=[9, 11, 200])
    eng.generate(**other, max_new_tokens=6, no_repeat_ngram_size=1, suppress_tokens=[9, 11, 200], cache_set=1)
    h = eng.prefill_begin(**inp, cache_set=1, **kw)
    assert h.skey == (B, False, False, 1, True, "ngram")
    assert torch.equal(eng.decode_finish(h), want)
    h0 = eng.adopt(eng.prefill_begin(**inp, cache_set=1, **kw), 0)
    assert h0.skey == (B, False, False, 0, True, "ngram")
    assert torch.equal(eng.decode_finish(h0), want)
    o = eng.generate(**inp, **kw, sync_every=4, output_hidden_states=True, return_dict_in_generate=True)
    assert torch.equal(o.sequences, want) and len(o.hidden_states) == N


def test_mrope_prompt_pass(dev):
    eng = _engine(dev, 2, 2, SEED_B3, mrope=True)
    inp, prompt = _inputs(eng, 2, SEED_B3, "ids")
    kw = dict(max_new_tokens=N, no_repeat_ngram_size=2, repetition_penalty=0.8)
    a = eng.generate(**inp, **kw)
    # text-only (t, h, w) positions are the 1-D positions: the same tokens through the mRoPE prompt pass
    pos = (inp["attention_mask"].cumsum(-1) - 1).clamp(min=0)
    c = eng.generate(**inp, **kw, position_ids=pos[None].expand(3, -1, -1).contiguous())
    assert torch.equal(a, c) and not torch.equal(a, eng.generate(**inp, **dict(kw, no_repeat_ngram_size=None)))


def test_eleven_rows_equal_the_groups_run_by_hand(dev):
    eng = _engine(dev, 2, 8, 23)
    ids = torch.randint(3, V, (11, S), generator=torch.Generator().manual_seed(8))
    kw = dict(max_new_tokens=16, no_repeat_ngram_size=2, repetition_penalty=0.8)
    allr = eng.generate(input_ids=ids, **kw)
    assert allr.shape == (11, S + 16)
    assert torch.equal(allr[:8], eng.generate(input_ids=ids[:8], **kw)) and torch.equal(allr[8:], eng.generate(input_ids=ids[8:], **kw))
    assert not torch.equal(allr, eng.generate(input_ids=ids, **dict(kw, no_repeat_ngram_size=0)))
    for b in range(11):
        s = allr[b].tolist()
        grams = [tuple(s[i:i + 2]) for i in range(len(s) - 1) if i + 2 > S]
        assert len(set(grams)) == len(grams) and not (set(grams) & {tuple(s[i:i + 2]) for i in range(S - 1)})


@pytest.mark.parametrize("mode", ["ids", "embeds"])
def test_sampling_respects_the_ngram_ban(dev, mode):
    B, n, seed = 3, 2, 0xBADC0FFEE
    samp = dict(temperature=0.8, top_k=20, top_p=0.9)
    pen = 0.5       # rewards repeats: the draws return to tokens they have been at, and the ban set fills
    eng = _engine(dev, 3, B, SEED_B3)
    inp, prompt = _inputs(eng, B, SEED_B3, mode)
    kw = dict(do_sample=True, seed=seed, no_repeat_ngram_size=n, repetition_penalty=pen, return_dict_in_generate=True,
              return_logits=True, **samp)
    o = eng.generate(**inp, max_new_tokens=N, **kw)
    gen, logits = o.sequences[:, -N:].cpu(), o.logits.float().cpu()
    assert (B, False, True, 0, True, "sample", "ngram") in eng._graphs
    p, min_new, ban = resolve_logits_processors(S, None, pen)

    def step(t):
        """per row: (banned set, processed logits) of step t under the engine's own history"""
        seen = torch.zeros(B, V, dtype=torch.bool)
        seqs = [[] if prompt is None else prompt[b].tolist() for b in range(B)]
        if prompt is not None:
            seen.scatter_(1, prompt, True)
        if t:
            seen.scatter_(1, gen[:, :t], True)
        banned = [ngram_banned_host(seqs[b] + gen[b, :t].tolist(), n) for b in range(B)]
        return banned, process_logits_host(logits[:, t], seen, p, ban, None, t, min_new, banned)

    last = None     # the last step at which the ban removed a token from some row's candidates
    for t in range(N):
        banned, x = step(t)
        x_free = process_logits_host(logits[:, t], torch.zeros(B, V, dtype=torch.bool), 1.0, [], None, t, 0)
        for b in range(B):
            assert int(gen[b, t]) not in banned[b], (b, t)
            if banned[b] & set(sample_token_host(x_free[b], samp["temperature"], samp["top_k"], samp["top_p"], 0.5)["tokens"].tolist()):
                last = t
    assert last is not None and last >= 1
    # the same request cut behind that step: the same tokens, and the state holds that step's candidates
    o2 = eng.generate(**inp, max_new_tokens=last + 1, **kw)
    assert torch.equal(o2.sequences[:, -(last + 1):].cpu(), gen[:, :last + 1])
    sm = eng._graphs[(B, False, True, 0, True, "sample", "ngram")][0]["sample"]
    banned, x = step(last)
    for b in range(B):
        check_sample_step(x[b], samp["temperature"], samp["top_k"], samp["top_p"], sample_uniform_host(seed, b, last),
                          sm["cand_tok"][b].cpu(), sm["cand_p"][b].cpu(), sm["n_keep"][b].cpu(), sm["u"][b].cpu(), gen[b, last])
        assert not (banned[b] & set(sm["cand_tok"][b].cpu().tolist()) - {-1}) or all(
            float(sm["cand_p"][b, j]) == 0.0 for j, tk in enumerate(sm["cand_tok"][b].cpu().tolist()) if tk in banned[b])

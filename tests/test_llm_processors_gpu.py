"""GPU: LlamaEngine.generate with logits processors (repetition_penalty, min_new_tokens / min_length, suppress_tokens,
single-token bad_words_ids) on the processed decode path.

Replay check: with return_logits=True the engine returns the RAW logits of every step. transformers' own processor classes,
applied in fp32 on the CPU to the raw logits of step t with the engine's own history up to t, must make the lowest-index arg-max
the engine's token at every step of every row -- exact, the kernels apply the same fp32 arithmetic to the same bf16 logits. Which
ids the penalty sees per input mode and how min_length resolves are pinned against HF's generate in
tests/test_logits_processors_cpu.py."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

V, N, S = 331, 24, 9


def _engine(dev, layers, max_batch, seed, row_major=False, mrope=False):
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd.llm import LlamaEngine, LLMConfig
    ocfg = LlamaCfg(256, layers, 2, 1, 128, 512, V, 10000.0, None, 1e-6, False, 256)
    w = LlamaOracle.random_weights(ocfg, seed=seed, std=0.08)
    cfg = LLMConfig(**ocfg.__dict__)
    if mrope:
        cfg = dataclasses.replace(cfg, mrope_section=(16, 24, 24))
    eng = LlamaEngine(cfg, w, dev, max_batch=max_batch, max_len=128)
    if row_major:       # what SPIDER_DECODE_FM_MIN above the batch size selects: the row-major GEMVs and lm_head for every batch size
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


def _replay(gen, logits, prompt, eos, p, min_new, ban):
    """HF's processors on the raw logits, step by step. Returns (first mismatch or None, number of (row, step) pairs whose raw
    arg-max was an id the processors act on). Rows are compared up to their first EOS (afterwards the engine pads)."""
    from transformers import (MinNewTokensLengthLogitsProcessor, RepetitionPenaltyLogitsProcessor, SuppressTokensLogitsProcessor)
    gen, logits = gen.cpu().long(), logits.float().cpu()
    B, n = gen.shape
    procs = []
    if p != 1.0:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=p))
    if eos and min_new > 0:
        procs.append(MinNewTokensLengthLogitsProcessor(0 if prompt is None else prompt.shape[1], min_new, eos))
    if ban:
        procs.append(SuppressTokensLogitsProcessor(ban))
    alive = torch.ones(B, dtype=torch.bool)
    touched = 0
    for t in range(n):
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
            r = int(raw[b].argmax())
            if (p != 1.0 and r in hist[b].tolist()) or r in ban or (eos and t < min_new and r in eos):
                touched += 1
        if eos:
            alive &= ~torch.isin(gen[:, t], torch.tensor(eos))
    return None, touched


# (name, layers, B, row_major, weight seed): B = 1 row-major with the folded norm; B = 3 fragment-major; B = 3 forced row-major
ENGINES = [("b1", 2, 1, False, 21), ("b3fm", 3, 3, False, 25), ("b3rm", 3, 3, True, 25)]


@pytest.mark.parametrize("case", ["penalty", "all"])
@pytest.mark.parametrize("mode", ["ids", "embeds"])
@pytest.mark.parametrize("ename,layers,B,row_major,seed", ENGINES)
def test_processed_generate_replays_under_hf_processors(dev, ename, layers, B, row_major, seed, mode, case):
    eng = _engine(dev, layers, B, seed, row_major)
    inp, prompt = _inputs(eng, B, seed, mode)
    plain = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
    plain_gen = plain.sequences[:, -N:].cpu()
    if case == "penalty":
        kw, eos, pen, min_new, ban = dict(repetition_penalty=1.3), None, 1.3, 0, []
    else:
        # EOS: a token the unprocessed row 0 emits among its first 6 tokens; ban set: ids 0, V - 1 and a token of the stream
        eos = [int(plain_gen[0, 2])]
        ban = sorted({0, V - 1, int(plain_gen[B - 1, 4])} - set(eos))
        pen, min_new = 1.05, 6
        kw = dict(repetition_penalty=pen, min_new_tokens=min_new, suppress_tokens=ban[:2], bad_words_ids=[[t] for t in ban[2:]],
                  eos_token_id=eos, pad_token_id=1)
    outs = {}
    for use_graph in (True, False):
        o = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True, use_graph=use_graph, **kw)
        n = o.logits.shape[1]
        gen = o.sequences[:, -n:]
        bad, touched = _replay(gen, o.logits, prompt, eos, pen, min_new, ban)
        assert bad is None, f"graph={use_graph}: (row, step, HF replay, engine) = {bad}"
        # the case counts only if the processors decided something: a raw winner they act on, and tokens unlike the plain run's
        assert touched > 0
        assert not torch.equal(gen.cpu(), plain_gen[:, :n])
        outs[use_graph] = (gen, o.logits)
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])     # graph == eager, bit for bit
    skeys = set(eng._graphs)
    assert (B, False, True, 0) in skeys and (B, False, True, 0, True) in skeys and len(skeys) == 2


def test_parameters_are_read_at_replay_time(dev):
    """two requests with different penalties and min_new on ONE captured graph, each matching its own replay"""
    eng = _engine(dev, 3, 3, 25)
    inp, prompt = _inputs(eng, 3, 25, "ids")
    plain = eng.generate(**inp, max_new_tokens=N)[:, -N:].cpu()
    eos = [int(plain[0, 2]), int(plain[1, 3])]
    assert eng.would_capture(3, False, True, 0, processed=True)
    res = []
    for i, (pen, mn) in enumerate(((1.3, 4), (1.05, 9))):
        if i == 1:
            assert not eng.would_capture(3, False, True, 0, processed=True)
            graph = eng._graphs[(3, False, True, 0, True)][1]
        o = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True, repetition_penalty=pen,
                         min_new_tokens=mn, eos_token_id=eos, pad_token_id=1)
        n = o.logits.shape[1]
        gen = o.sequences[:, -n:]
        bad, touched = _replay(gen, o.logits, prompt, eos, pen, mn, [])
        assert bad is None and touched > 0, (pen, mn, bad, touched)
        assert not torch.isin(gen[:, :mn].cpu(), torch.tensor(eos)).any()
        res.append(gen.cpu())
    assert eng._graphs[(3, False, True, 0, True)][1] is graph
    assert res[0].shape != res[1].shape or not torch.equal(res[0], res[1])


def test_adopt_mid_request_keeps_the_tokens(dev):
    eng = _engine(dev, 2, 1, 21)
    inp, prompt = _inputs(eng, 1, 21, "ids")
    kw = dict(max_new_tokens=N, repetition_penalty=1.3, suppress_tokens=[0, 5], min_new_tokens=3, eos_token_id=[7])
    want = eng.generate(**inp, **kw)
    # another request's values are left in set 0's buffers; the adopted request must bring its own
    eng.generate(**inp, max_new_tokens=4, repetition_penalty=1.05, suppress_tokens=[9, 11, 200])
    h = eng.prefill_begin(**inp, cache_set=1, **kw)
    assert h.skey == (1, False, False, 1, True)
    h0 = eng.adopt(h, 0)
    assert h0.skey == (1, False, False, 0, True)
    assert torch.equal(eng.decode_finish(h0), want)


def test_eleven_rows_equal_the_groups_run_by_hand(dev):
    eng = _engine(dev, 2, 8, 23)
    ids = torch.randint(3, V, (11, S), generator=torch.Generator().manual_seed(8))
    kw = dict(max_new_tokens=12, repetition_penalty=1.3, suppress_tokens=[0, 4], bad_words_ids=[[17]])
    allr = eng.generate(input_ids=ids, **kw)
    assert allr.shape == (11, S + 12)
    assert torch.equal(allr[:8], eng.generate(input_ids=ids[:8], **kw)) and torch.equal(allr[8:], eng.generate(input_ids=ids[8:], **kw))
    assert not torch.equal(allr, eng.generate(input_ids=ids, max_new_tokens=12))
    assert not torch.isin(allr[:, S:].cpu(), torch.tensor([0, 4, 17])).any()


def test_neutral_arguments_use_the_unprocessed_state(dev):
    eng = _engine(dev, 2, 1, 21)
    inp, _ = _inputs(eng, 1, 21, "embeds")
    a = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
    # explicit neutral values, and the reference's own defaults (spider.py:1471: min_length=1, repetition_penalty=1) with an EOS id
    b = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True, repetition_penalty=1.0, min_length=0)
    c = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True, repetition_penalty=1, min_length=1,
                     suppress_tokens=[], eos_token_id=[V + 5])
    for o in (b, c):
        assert torch.equal(a.sequences, o.sequences) and torch.equal(a.logits, o.logits)
    assert set(eng._graphs) == {(1, False, True, 0)}
    with pytest.raises(NotImplementedError, match=r"\[3, 4\]"):
        eng.generate(**inp, max_new_tokens=4, bad_words_ids=[[3, 4]])
    with pytest.raises(ValueError):
        eng.generate(**inp, max_new_tokens=4, repetition_penalty=2)


def test_sync_every_hidden_states_and_mrope_on_the_processed_path(dev):
    eng = _engine(dev, 2, 2, 25, mrope=True)
    inp, prompt = _inputs(eng, 2, 25, "ids")
    plain = eng.generate(**inp, max_new_tokens=N)[:, -N:].cpu()
    kw = dict(max_new_tokens=N, repetition_penalty=1.3, min_new_tokens=5, eos_token_id=[int(plain[0, 1])], pad_token_id=1,
              return_dict_in_generate=True)
    a = eng.generate(**inp, **kw)
    b = eng.generate(**inp, **kw, sync_every=4, output_hidden_states=True)
    assert torch.equal(a.sequences, b.sequences) and len(b.hidden_states) == a.sequences.shape[1] - S
    # text-only (t, h, w) positions are the 1-D positions: the same tokens through the mRoPE prompt pass
    am = inp["attention_mask"]
    pos = (am.cumsum(-1) - 1).clamp(min=0)
    c = eng.generate(**inp, **kw, position_ids=pos[None].expand(3, -1, -1).contiguous())
    assert torch.equal(a.sequences, c.sequences)


class _IdTok:
    """the signal-token stand-in of tests/test_trained_spider.py, with a decode that shows the ids"""
    pad_token_id, bos_token_id = 0, 1

    def __call__(self, text, return_tensors="pt", add_special_tokens=False):
        from test_trained_spider import _Tok
        return _Tok()(text)

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(int(t)) for t in ids)


def test_trained_spider_passes_the_penalty_through(dev):
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd import routing
    from spider_amd.llm import LlamaEngine, LLMConfig
    from spider_amd.spider_trained import TrainedSpider
    ocfg = LlamaCfg(64, 2, 2, 1, 128, 128, 128, 10000.0, None, 1e-6, False, 256)
    llm = LlamaEngine(LLMConfig(**ocfg.__dict__), LlamaOracle.random_weights(ocfg, seed=31, std=0.08), dev, max_batch=1, max_len=256)
    mods = {"IMAGE": dict(alignment_output_tokens=77, alignment_output_dim=64, alignment_layer=[-1])}
    ts = TrainedSpider(llm, _IdTok(), [], mods, {"IMAGE": 1}, max_context_len=24)
    samples = {"TaskPrompt": ["[IMAGE]"], "Question": ["draw a red car"]}
    a1 = ts.generate(samples, *routing.new_outputs(), repetition_penalty=1)[0]
    a0 = ts.generate(samples, *routing.new_outputs())[0]
    a2 = ts.generate(samples, *routing.new_outputs(), repetition_penalty=1.3)[0]
    assert a0 == a1 and a1 != a2
    assert any(len(k) == 5 for k in llm._graphs) and any(len(k) == 4 for k in llm._graphs)

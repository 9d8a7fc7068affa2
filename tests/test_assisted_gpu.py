"""GPU: assisted decoding (assistant_model / num_assistant_tokens) -- the two hand-off kernels of csrc/spec_assist.hip against
`assisted_round_host` on every buffer of both launches, and the engine with a draft engine beside it: on the successor models of
tests/assisted_cases.py (greedy output and exact counters), with the target's own weights as draft, on the reference-pinned d128
fixture of tests/test_llm_engine.py, with quantised targets, a left-padded prompt, the tightest caches, and the refusals."""
import json
import os

import numpy as np
import pytest
import torch

import assisted_cases as ac
import prompt_lookup_cases as pc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- the hand-off kernels
def _run_assist_case(case, dev, via_torch_op=False):
    from spider_amd import ops
    t = {k: getattr(case, k).clone().to(dev) for k in case.BUFFERS}
    tgt = dict(ids=t["ids"], pos=t["pos"], slot=t["slot"])
    src2 = dict(out=t["d2_out"], pos=t["d2_pos"], slot=t["d2_slot"])
    src1 = dict(out=t["d1_out"], pos=t["d1_pos"], slot=t["d1_slot"])
    dst = dict(ids=t["d1_ids"], pos=t["d1_pos"], slot=t["d1_slot"], kv_end=t["d1_kv_end"])
    if via_torch_op:
        import spider_amd.torch_ops  # noqa: F401
    B, R = case.B, case.R
    for j in range(1, case.nd + 1):
        # the draft step that ran in front of push j: its arg-max is draft j (row 1 of the two-row step, then the single row)
        src, row = (src2, 1) if j == 1 else (src1, 0)
        src["out"].view(B, -1)[:, row] = torch.tensor([s["drafts"][j - 1] for s in case.seqs], dtype=torch.int32, device=dev)
        if via_torch_op:
            torch.ops.spider_hip.spec_assist_push_(src["out"], src["pos"], src["slot"], row, t["ids"], t["pos"], t["slot"], j,
                                                   t["d1_ids"], t["d1_pos"], t["d1_slot"], t["d1_kv_end"], case.vd)
        else:
            ops.spec_assist_push(src, row, tgt, j, dst, case.vd)
        want = case.expected_after_push(j)
        for k in ("ids", "pos", "slot"):
            assert t[k].view(B, R)[:, j].tolist() == want[k], (case.name, j, k)
        for k in ("d1_ids", "d1_pos", "d1_slot", "d1_kv_end"):
            assert t[k].tolist() == want[k], (case.name, j, k, t[k].tolist(), want[k])
    if via_torch_op:
        torch.ops.spider_hip.spec_assist_advance_(t["lm_out"], t["ids"], t["pos"], t["slot"], t["kv_end"], t["n_draft"], t["hist"],
                                                  t["n_hist"], t["counters"], t["d2_ids"], t["d2_pos"], t["d2_slot"], t["d2_kv_end"],
                                                  case.vd)
    else:
        ops.spec_assist_advance(dict(lm_out=t["lm_out"], ids=t["ids"], pos=t["pos"], slot=t["slot"], kv_end=t["kv_end"],
                                     n_draft=t["n_draft"], counters=t["counters"]), t["hist"], t["n_hist"],
                                dict(ids=t["d2_ids"], pos=t["d2_pos"], slot=t["d2_slot"], kv_end=t["d2_kv_end"]), case.vd)
    want = case.expected()
    for k in case.BUFFERS:      # outputs bit for bit; inputs (lm_out, n_draft, the draft steps' arg-max) as they were
        assert torch.equal(t[k].cpu(), want[k]), (case.name, k, t[k].cpu().tolist(), want[k].tolist())


@pytest.mark.parametrize("K", [1, 3, 7])
def test_assist_kernels_equal_host_restatement_random(dev, K):
    for case in ac.random_assist_cases(K):
        _run_assist_case(case, dev)


@pytest.mark.parametrize("case", ac.named_assist_cases(), ids=repr)
def test_assist_kernels_equal_host_restatement_named(dev, case):
    _run_assist_case(case, dev)
    _run_assist_case(case, dev, via_torch_op=True)


def test_assist_ops_refuse_other_shapes(dev):
    from spider_amd import ops
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    rows = lambda n: dict(ids=i32(n), pos=i32(n), slot=i32(n))
    src, dst = dict(out=i32(2), pos=i32(2), slot=i32(2)), dict(rows(1), kv_end=i32(1))
    with pytest.raises(ValueError, match="draft row"):
        ops.spec_assist_push(src, 1, rows(4), 4, dst, 296)
    with pytest.raises(ValueError, match="source row"):
        ops.spec_assist_push(src, 2, rows(4), 1, dst, 296)
    with pytest.raises(ValueError, match="rows"):
        ops.spec_assist_push(src, 1, rows(9), 1, dst, 296)
    sp = dict(rows(4), lm_out=i32(4), kv_end=i32(1), n_draft=i32(1), counters=torch.zeros(1, 3, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="catch-up"):
        ops.spec_assist_advance(sp, torch.zeros(1, 8, dtype=torch.int32, device=dev), i32(1), dict(rows(1), kv_end=i32(1)), 296)


# ---------------------------------------------------------------------------------------------- engine, successor models
def _engine(dev, model, **kw):
    from spider_amd.llm import LlamaEngine, LLMConfig
    cfg, w = model
    return LlamaEngine(LLMConfig(**cfg.__dict__), w, dev, **dict(dict(max_len=128), **kw))


def _counts(rec):
    return {k: rec[k] for k in ("steps", "drafted", "accepted")}


def _chain(tokens):
    """the engine's own greedy successor along a generated sequence whose tokens depend on their predecessor alone (succ elsewhere:
    the rows behind a rejected draft are never looked at)"""
    t = [int(x) for x in tokens]
    nxt = dict(zip(t[:-1], t[1:]))
    return lambda v: nxt.get(v, pc.succ(v))


IDS = torch.tensor([pc.PROMPT])
S, T = len(pc.PROMPT), pc.T_NEW


@pytest.mark.parametrize("max_batch", [1, 8], ids=["row-major", "fragment-major"])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_engine_draft_successor_model(dev, K, max_batch):
    eng, draft = _engine(dev, pc.successor_model(), max_batch=max_batch), _engine(dev, ac.draft_model(), max_batch=2)
    assert eng.fm_batch == (max_batch == 8)     # both have a route for K + 1 rows: row-major GEMVs serve up to 8 rows
    greedy, _ = pc.successor_greedy()
    sim_tok, sim = ac.simulate_tokens(greedy[0], T, K)
    if K == 3:
        assert sim == ac.K3
    assert eng.would_capture(1, num_assistant_tokens=K) and eng.last_assisted is None
    out = eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=draft, num_assistant_tokens=K, return_dict_in_generate=True)
    assert not eng.would_capture(1, num_assistant_tokens=K) and eng.would_capture(1) and eng.would_capture(1, prompt_lookup_num_tokens=K)
    assert out.sequences[0, :S].tolist() == pc.PROMPT
    assert out.sequences[0, S:].tolist() == list(greedy[:T]) == sim_tok
    # without the feature the keyword is ignored and `assisted` does not exist
    assert out.assisted == _counts(sim) == eng.last_assisted, (out.assisted, sim)
    assert out.prompt_lookup is None and eng.last_prompt_lookup is None
    # the same tokens and counters without the graph; with fewer host checks the rounds that ran past the end are counted too
    eager = eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=draft, num_assistant_tokens=K, use_graph=False,
                         num_assistant_tokens_schedule="constant", assistant_confidence_threshold=0)
    assert torch.equal(eager, out.sequences) and eng.last_assisted == out.assisted
    for use_graph in (True, False):
        every3 = eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=draft, num_assistant_tokens=K, sync_every=3,
                              use_graph=use_graph)
        assert torch.equal(every3, out.sequences)
        assert out.assisted["steps"] <= eng.last_assisted["steps"] <= out.assisted["steps"] + 2
    # the plain greedy output of the same engine is the same sequence, and leaves no record behind
    assert torch.equal(eng.generate(input_ids=IDS, max_new_tokens=T), out.sequences) and eng.last_assisted is None
    # an EOS that arrives inside an accepted draft ends the row there, as on the plain path
    eos = pc.C[5]
    want = eng.generate(input_ids=IDS, max_new_tokens=T, eos_token_id=eos)
    for se in (1, 3):
        got = eng.generate(input_ids=IDS, max_new_tokens=T, eos_token_id=eos, assistant_model=draft, num_assistant_tokens=K, sync_every=se)
        assert torch.equal(got, want) and int(got[0, -1]) == eos and got.shape[1] < S + T


@pytest.mark.parametrize("K", [1, 3, 7])
def test_engine_own_weights_as_draft_accept_everything(dev, K):
    eng, draft = _engine(dev, pc.successor_model(), max_batch=1), _engine(dev, pc.successor_model(), max_batch=2)
    greedy, _ = pc.successor_greedy()
    sim_tok, sim = ac.simulate_tokens(greedy[0], T, K, draft_next=pc.succ, draft_vocab=300)
    assert sim["accepted"] == sim["drafted"] == K * sim["steps"]
    out = eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=draft, num_assistant_tokens=K, return_dict_in_generate=True)
    assert out.sequences[0, S:].tolist() == sim_tok
    assert out.assisted == _counts(sim), (out.assisted, sim)        # steps = ceil((T - 1) / (K + 1)), by the simulation


def test_engine_num_assistant_tokens_defaults_to_five(dev):
    eng, draft = _engine(dev, pc.successor_model(), max_batch=1), _engine(dev, ac.draft_model(), max_batch=2)
    out = eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=draft, return_dict_in_generate=True)
    greedy, _ = pc.successor_greedy()
    assert out.sequences[0, S:].tolist() == list(greedy[:T]) and out.assisted == _counts(ac.simulate_tokens(greedy[0], T, 5)[1])
    assert not eng.would_capture(1, num_assistant_tokens=5)


@pytest.mark.parametrize("weight_dtype", ["fp8", "mxfp4"])
def test_engine_quantised_targets(dev, weight_dtype):
    """K = 5: six rows, the fragment-major quantised stream of a batched_weight_stream engine"""
    K = 5
    eng = _engine(dev, pc.successor_model(), max_batch=8, weight_dtype=weight_dtype, batched_weight_stream=True)
    draft = _engine(dev, ac.draft_model(), max_batch=2)
    plain = eng.generate(input_ids=IDS, max_new_tokens=T)
    out = eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=draft, num_assistant_tokens=K, return_dict_in_generate=True)
    assert torch.equal(out.sequences, plain)
    assert out.assisted == _counts(ac.simulate_tokens(int(plain[0, S]), T, K, target_next=_chain(plain[0, S:]))[1])
    assert out.assisted["accepted"] > 0
    assert torch.equal(eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=draft, num_assistant_tokens=K, use_graph=False), plain)


def test_engine_left_padded_prompt_and_ids_the_draft_model_does_not_have(dev):
    eng, draft = _engine(dev, pc.successor_model(), max_batch=1), _engine(dev, ac.draft_model(), max_batch=2)
    prompt = list(pc.PROMPT)
    prompt[4], prompt[9] = 298, 297         # >= the draft model's 296 rows
    ids = torch.tensor([[0, 0] + prompt])
    mask = torch.tensor([[0, 0] + [1] * len(prompt)])
    plain = eng.generate(input_ids=ids, attention_mask=mask, max_new_tokens=T)
    for K in (3, 7):
        out = eng.generate(input_ids=ids, attention_mask=mask, max_new_tokens=T, assistant_model=draft, num_assistant_tokens=K,
                           return_dict_in_generate=True)
        assert torch.equal(out.sequences, plain)
        assert out.assisted == _counts(ac.simulate_tokens(int(plain[0, ids.shape[1]]), T, K, target_next=_chain(plain[0, ids.shape[1]:]))[1])
        assert 0 < out.assisted["accepted"] < out.assisted["drafted"]


@pytest.mark.parametrize("K, sync_every, T_", [(3, 3, 42), (7, 2, 42), (1, 4, 18)])
def test_engine_last_round_ends_exactly_at_max_len_on_both_engines(dev, K, sync_every, T_):
    """max_len == S + max_new_tokens + K on both engines, the tightest caches resolve_assisted admits, with the draft that is always
    right and T - 2 a multiple of K + 1, so that the last round starts one token short of T and appends K + 1: a round advances by
    K + 1 slots, so the rounds replayed before the host reads n_hist are bounded by the caches. A K / V
    row appended past slot max_len - 1 of the last kv head lands in batch row 1 of the layer's cache."""
    max_len = S + T_ + K
    eng = _engine(dev, pc.successor_model(), max_batch=2, max_len=max_len)
    draft = _engine(dev, pc.successor_model(), max_batch=2, max_len=max_len)
    want = eng.generate(input_ids=IDS, max_new_tokens=T_)
    SENT = 777.0
    for e in (eng, draft):
        for t in e._kv(0):
            t[:, 1].fill_(SENT)
    out = eng.generate(input_ids=IDS, max_new_tokens=T_, assistant_model=draft, num_assistant_tokens=K, sync_every=sync_every,
                       return_dict_in_generate=True)
    assert torch.equal(out.sequences, want)
    assert out.assisted["accepted"] == out.assisted["drafted"] > 0
    for who, e in (("engine", eng), ("draft engine", draft)):
        for name, t in zip("kv", e._kv(0)):
            assert bool((t[:, 1] == SENT).all()), f"{who} {name} cache: rows of the neighbouring batch row were written"
    with pytest.raises(ValueError, match="engine's max_len"):
        eng.generate(input_ids=IDS, max_new_tokens=T_ + 1, assistant_model=_engine(dev, ac.draft_model(), max_batch=2), num_assistant_tokens=K)
    short = _engine(dev, ac.draft_model(), max_batch=2, max_len=max_len - 1)
    with pytest.raises(ValueError, match="assistant_model's max_len"):
        eng.generate(input_ids=IDS, max_new_tokens=T_, assistant_model=short, num_assistant_tokens=K)


def test_engine_other_requests_and_the_draft_engine_are_left_as_they_were(dev):
    eng, draft = _engine(dev, pc.successor_model(), max_batch=1), _engine(dev, ac.draft_model(), max_batch=2)
    greedy0 = eng.generate(input_ids=IDS, max_new_tokens=T)
    lookup0 = eng.generate(input_ids=IDS, max_new_tokens=T, prompt_lookup_num_tokens=3, return_dict_in_generate=True)
    draft0 = draft.generate(input_ids=IDS, max_new_tokens=T)
    keys0, dkeys0 = set(eng._graphs), set(draft._graphs)
    out = eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=draft, num_assistant_tokens=3)
    assert torch.equal(out, greedy0)
    assert set(eng._graphs) - keys0 == {eng._state_key(1, False, False, 0, assist=3)} and set(draft._graphs) == dkeys0
    assert torch.equal(eng.generate(input_ids=IDS, max_new_tokens=T), greedy0)
    again = eng.generate(input_ids=IDS, max_new_tokens=T, prompt_lookup_num_tokens=3, return_dict_in_generate=True)
    assert torch.equal(again.sequences, lookup0.sequences) and again.prompt_lookup == lookup0.prompt_lookup and again.assisted is None
    assert torch.equal(draft.generate(input_ids=IDS, max_new_tokens=T), draft0)
    # the draft engine's own request in between does not disturb the next assisted call, and another draft engine captures anew
    assert torch.equal(eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=draft, num_assistant_tokens=3), greedy0)
    other = _engine(dev, pc.successor_model(), max_batch=2)
    res = eng.generate(input_ids=IDS, max_new_tokens=T, assistant_model=other, num_assistant_tokens=3, return_dict_in_generate=True)
    assert torch.equal(res.sequences, greedy0) and res.assisted["accepted"] == res.assisted["drafted"]
    assert set(eng._graphs) - keys0 == {eng._state_key(1, False, False, 0, assist=3)}


def test_engine_refuses_what_the_round_does_not_serve(dev):
    eng, draft = _engine(dev, pc.successor_model(), max_batch=2), _engine(dev, ac.draft_model(), max_batch=2)
    from spider_amd.llm import LlamaEngine, LLMConfig
    from oracle.llama import LlamaCfg, LlamaOracle
    c64 = LlamaCfg(128, 1, 2, 2, 64, 256, 296, 10000.0, None, 1e-6, False, 256)
    d64 = LlamaEngine(LLMConfig(**c64.__dict__), LlamaOracle.random_weights(c64, seed=1), dev, max_batch=2, max_len=128)
    cbig = LlamaCfg(128, 1, 2, 1, 128, 256, 304, 10000.0, None, 1e-6, False, 256)
    dbig = LlamaEngine(LLMConfig(**cbig.__dict__), LlamaOracle.random_weights(cbig, seed=1), dev, max_batch=2, max_len=128)
    for kw, exc, word in ((dict(num_assistant_tokens=8), ValueError, "num_assistant_tokens"),
                          (dict(num_assistant_tokens=0), ValueError, "num_assistant_tokens"),
                          (dict(num_assistant_tokens_schedule="heuristic"), NotImplementedError, "num_assistant_tokens_schedule"),
                          (dict(assistant_confidence_threshold=0.4), NotImplementedError, "assistant_confidence_threshold"),
                          (dict(assistant_model=None), ValueError, "num_assistant_tokens"),
                          (dict(do_sample=True), NotImplementedError, "do_sample"),
                          (dict(num_beams=2), NotImplementedError, "num_beams"),
                          (dict(repetition_penalty=1.3), NotImplementedError, "repetition_penalty"),
                          (dict(no_repeat_ngram_size=2), NotImplementedError, "no_repeat_ngram_size"),
                          (dict(output_hidden_states=True), NotImplementedError, "output_hidden_states"),
                          (dict(return_logits=True), NotImplementedError, "return_logits"),
                          (dict(prompt_lookup_num_tokens=3), NotImplementedError, "prompt_lookup_num_tokens"),
                          (dict(assistant_model=eng), ValueError, "assistant_model"),
                          (dict(assistant_model=d64), NotImplementedError, "head_dim"),
                          (dict(assistant_model=dbig), ValueError, "vocabulary"),
                          (dict(assistant_model=_engine(dev, ac.draft_model(), max_batch=1)), NotImplementedError, "max_batch"),
                          (dict(max_new_tokens=114), ValueError, "max_len")):       # 12 + 114 + 3 = 129 > 128
        with pytest.raises(exc, match=word):
            eng.generate(input_ids=IDS, **dict(dict(max_new_tokens=8, assistant_model=draft, num_assistant_tokens=3), **kw))
    with pytest.raises(NotImplementedError, match="head_dim"):      # the target's own head_dim
        d64.generate(input_ids=IDS, max_new_tokens=8, assistant_model=draft, num_assistant_tokens=3)
    with pytest.raises(NotImplementedError, match="batch"):
        eng.generate(input_ids=torch.tensor([pc.PROMPT, pc.PROMPT]), max_new_tokens=8, assistant_model=draft, num_assistant_tokens=3)
    with pytest.raises(NotImplementedError, match="inputs_embeds"):
        eng.generate(inputs_embeds=eng.embed_tokens(IDS), max_new_tokens=8, assistant_model=draft, num_assistant_tokens=3)
    with pytest.raises(NotImplementedError, match="prefill_begin"):
        eng.prefill_begin(input_ids=IDS, max_new_tokens=8, assistant_model=draft, num_assistant_tokens=3)
    far = _engine(dev, ac.draft_model(), max_batch=2)
    far.device = torch.device("cuda", dev.index + 1)        # (what an engine built there would say; nothing is run on it)
    with pytest.raises(NotImplementedError, match="device"):
        eng.generate(input_ids=IDS, max_new_tokens=8, assistant_model=far, num_assistant_tokens=3)
    assert eng.generate(input_ids=IDS, max_new_tokens=113, assistant_model=draft, num_assistant_tokens=3).shape[1] == 12 + 113


# ---------------------------------------------------------------------------------------------- engine, reference-pinned model
def test_engine_reference_pinned_fixture_with_a_random_draft(dev, golden_dir):
    """The d128 fixture of tests/test_llm_engine.py (tokens of the reference's own LlamaForCausalLM, margins >= 0.1) with a draft
    engine of random weights: the drafts are mostly rejected, and the tokens are the fixture's under the rule of
    test_batched_fold_path_tokens_match_single_row_path: a first divergence only where the oracle margin is < 0.1."""
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd.llm import LlamaEngine, LLMConfig
    z = np.load(os.path.join(golden_dir, "llama_ref_d128_0.npz"))
    ocfg = LlamaCfg(**json.loads(str(z["cfg"])))
    w = LlamaOracle.random_weights(ocfg, seed=int(z["seed"]), std=float(z["std"]))
    wsum = sum(float(v.double().abs().sum()) for v in w.values())
    assert abs(wsum - float(z["wsum"])) <= 1e-9 * float(z["wsum"]), "random_weights no longer reproduces the fixture's weights"
    ids, ref_tok, margins = torch.from_numpy(z["ids"]), torch.from_numpy(z["tokens"]), torch.from_numpy(z["margins"])
    S_, T_ = ids.shape[1], ref_tok.shape[1]
    eng = LlamaEngine(LLMConfig(**ocfg.__dict__), w, dev, max_batch=1, max_len=64)
    dcfg = LlamaCfg(128, 1, 2, 1, 128, 256, ocfg.vocab - 11, 10000.0, None, 1e-6, False, 128)
    draft = LlamaEngine(LLMConfig(**dcfg.__dict__), LlamaOracle.random_weights(dcfg, seed=9, std=0.08), dev, max_batch=2, max_len=64)
    drafted = accepted = 0
    for b in range(ids.shape[0]):
        out = eng.generate(input_ids=ids[b:b + 1], max_new_tokens=T_, assistant_model=draft, num_assistant_tokens=3,
                           return_dict_in_generate=True)
        gen = out.sequences[0, S_:].cpu()
        assert gen.numel() == T_
        for t in range(T_):
            if int(gen[t]) != int(ref_tok[b, t]):
                assert float(margins[b, t]) < 0.1, f"row {b} step {t}: diverges from the reference at a healthy margin"
                break
        rec = out.assisted
        assert rec["steps"] + rec["accepted"] >= T_ - 1 and rec["accepted"] <= rec["drafted"] == 3 * rec["steps"]
        drafted, accepted = drafted + rec["drafted"], accepted + rec["accepted"]
    print(f"MEASURED assisted decoding on the d128 fixture, random draft: {drafted} tokens drafted, {accepted} accepted")
    assert accepted < drafted / 2, "a random draft engine is mostly wrong"

"""CPU: the host restatement of assisted decoding (spider_amd.llm.assisted_round_host) replayed over the two fp32 oracles, the
request validation (resolve_assisted), and the surfaces the hand-off kernels are reachable through. No GPU."""
import inspect
import types

import pytest
import torch

import assisted_cases as ac
import prompt_lookup_cases as pc
from spider_amd import llm as L


def test_both_models_follow_their_successor_maps_by_a_wide_margin():
    greedy, margin = pc.successor_greedy()
    follows, dmargin = ac.draft_margin()
    print(f"MEASURED top-2 margins: target {margin:.2f}, draft model along the target's sequence {dmargin:.2f}")
    assert margin >= 0.1 and dmargin >= 0.1
    assert follows, "the draft oracle has to follow draft_succ wherever assisted decoding asks it"
    assert all(ac.draft_succ(v) != pc.succ(v) for v in ac.DRAFT_WRONG) and set(ac.DRAFT_WRONG) <= set(pc.C)
    assert len(ac.DRAFT_WRONG) == 2 and ac.draft_model()[0].vocab == ac.DRAFT_VOCAB < pc.successor_model()[0].vocab


def test_inputs_give_rounds_of_every_kind():
    """a condition on the inputs: PROMPT, K = 3 and 40 new tokens contain full, partial and zero acceptance"""
    greedy, _ = pc.successor_greedy()
    tok, rec = ac.simulate_tokens(greedy[0], pc.T_NEW, 3)
    assert tok == list(greedy[:pc.T_NEW])
    assert rec == ac.K3, rec
    assert min(rec["full"], rec["partial"], rec["rejected"]) >= 1


@pytest.mark.parametrize("K", [1, 3, 7])
def test_round_host_replayed_over_the_two_oracles_reproduces_greedy_and_the_counters(K):
    tcfg, tw = pc.successor_model()
    dcfg, dw = ac.draft_model()
    greedy, _ = pc.successor_greedy()
    tok, rec = ac.simulate_oracles(tcfg, tw, dcfg, dw, pc.PROMPT, pc.T_NEW, K)
    assert tok == list(greedy[:pc.T_NEW])
    tok2, rec2 = ac.simulate_tokens(greedy[0], pc.T_NEW, K)
    assert tok2 == tok and rec2 == rec, (rec, rec2)
    assert rec["drafted"] == K * rec["steps"] and rec["steps"] + rec["accepted"] >= pc.T_NEW - 1


def test_the_targets_own_weights_as_draft_accept_everything():
    greedy, _ = pc.successor_greedy()
    for K in (1, 3, 7):
        tok, rec = ac.simulate_tokens(greedy[0], pc.T_NEW, K, draft_next=pc.succ, draft_vocab=300)
        assert tok == list(greedy[:pc.T_NEW]) and rec["accepted"] == rec["drafted"] and rec["steps"] == -(-(pc.T_NEW - 1) // (K + 1))


def test_round_host():
    r = L.assisted_round_host(6, 15, 20, [7, 8, 9], [7, 8, 3, 10], 296)
    assert r["rows"] == [(6, 15, 20), (7, 16, 21), (8, 17, 22), (9, 18, 23)]
    assert r["feed"] == [(7, 16, 21, 22), (8, 17, 22, 23), (9, 18, 23, 24)]
    assert r["a"] == 2 and r["append"] == [7, 8, 3] and r["row0"] == (3, 18, 23)
    assert r["catch_up"] == dict(ids=[8, 3], pos=[17, 18], slot=[22, 23], kv_end=23)
    r = L.assisted_round_host(298, 4, 4, [297], [5, 6], 296)        # nothing accepted, ids the draft model does not have
    assert r["a"] == 0 and r["append"] == [5] and r["feed"] == [(0, 5, 5, 6)] and r["rows"][1] == (297, 5, 5)
    assert r["catch_up"] == dict(ids=[0, 5], pos=[4, 5], slot=[4, 5], kv_end=5)
    r = L.assisted_round_host(1, 0, 0, [2, 3], [2, 3, 299], 296)    # everything accepted: the rows are d_K and the model's token
    assert r["a"] == 2 and r["catch_up"]["ids"] == [3, 0] and r["row0"] == (299, 3, 3)
    assert L.assisted_round_host(1, 0, 0, [2, 3], [2, 3, 4], 296, n_draft=1)["a"] == 1


def test_kernel_cases_cover_the_named_situations():
    by = {c.name: c for c in ac.named_assist_cases()}
    assert [by["none-accepted"].round(b)["a"] for b in (0, 1)] == [0, 0]
    assert [by["all-accepted"].round(b)["a"] for b in (0, 1)] == [3, 3] and by["K7-all-accepted"].round(0)["a"] == 7
    assert [by["partial"].round(b)["a"] for b in (0, 1)] == [2, 1]
    e = by["ids-past-the-draft-vocabulary"].expected()
    assert e["d2_ids"].tolist() == [0, 3, 3, 0] and 298 in e["hist"][0].tolist() and e["ids"][4] == 299 and e["ids"][2] == 298
    e = by["kv_beg-pos-differs-from-slot"].expected()
    assert (e["slot"] - e["pos"]).tolist() == [5] * 8 and (e["d2_slot"] - e["d2_pos"]).tolist() == [5] * 4
    e = by["hist-one-short-of-cap"].expected()
    assert e["n_hist"].tolist() == [19, 17] and e["hist"][0, 15] == 7
    c = by["stale-ids-past-the-drafts"]
    assert [c.round(b)["a"] for b in (0, 1)] == [2, 2] and c.expected()["ids"][7] == 9 and c.expected()["counters"][0].tolist() == [6, 11, 6]
    for K in (1, 3, 7):
        cases = ac.random_assist_cases(K)
        kinds = {("none" if c.round(b)["a"] == 0 else "all" if c.round(b)["a"] == K else "some") for c in cases for b in (0, 1)}
        assert kinds >= ({"none", "all"} if K == 1 else {"none", "all", "some"})


def _engine(vocab=300, head_dim=128, max_batch=2, max_len=64, device="cuda:0"):
    return types.SimpleNamespace(cfg=types.SimpleNamespace(vocab=vocab, head_dim=head_dim), max_batch=max_batch, max_len=max_len,
                                 device=torch.device(device), _prefill=None, _decode_step=None)


OK = dict(B=1, S=12, max_new_tokens=40, decode_rows=8)


def test_resolve_assisted_accepts():
    tgt, d = _engine(max_batch=1), _engine(vocab=296)
    assert L.resolve_assisted(None, target=tgt, **OK) is None
    assert L.resolve_assisted(None, target=tgt, B=4, S=100, max_new_tokens=100, do_sample=True) is None     # off: nothing is looked at
    assert L.resolve_assisted(d, target=tgt, **OK) == 5 and L.resolve_assisted(d, None, "constant", 0, target=tgt, **OK) == 5
    assert L.resolve_assisted(d, 1, target=tgt, **OK) == 1 and L.resolve_assisted(d, 7, None, 0.0, target=tgt, **OK) == 7
    assert L.resolve_assisted(d, 7, target=_engine(max_len=59), **OK) == 7      # 12 + 40 + 7
    assert L.resolve_assisted(_engine(vocab=300), 3, target=tgt, prompt_lookup_num_tokens=0, **OK) == 3


@pytest.mark.parametrize("kw, exc, word", [
    (dict(num_assistant_tokens=8), ValueError, "num_assistant_tokens"),
    (dict(num_assistant_tokens=0), ValueError, "num_assistant_tokens"),
    (dict(num_assistant_tokens=True), ValueError, "num_assistant_tokens"),
    (dict(num_assistant_tokens=2.0), ValueError, "num_assistant_tokens"),
    (dict(num_assistant_tokens=4, decode_rows=4), ValueError, "num_assistant_tokens"),
    (dict(num_assistant_tokens_schedule="heuristic"), NotImplementedError, "num_assistant_tokens_schedule"),
    (dict(assistant_confidence_threshold=0.4), NotImplementedError, "assistant_confidence_threshold"),
    (dict(assistant_model=None, num_assistant_tokens=3), ValueError, "num_assistant_tokens"),
    (dict(assistant_model=None, num_assistant_tokens=None, num_assistant_tokens_schedule="constant"), ValueError, "num_assistant_tokens_schedule"),
    (dict(assistant_model=None, num_assistant_tokens=None, assistant_confidence_threshold=0), ValueError, "assistant_confidence_threshold"),
    (dict(assistant_model="gpt2"), TypeError, "assistant_model"),
    (dict(B=2), NotImplementedError, "batch"),
    (dict(do_sample=True), NotImplementedError, "do_sample"),
    (dict(num_beams=2), NotImplementedError, "num_beams"),
    (dict(processed=True), NotImplementedError, "repetition_penalty"),
    (dict(no_repeat_ngram_size=3), NotImplementedError, "no_repeat_ngram_size"),
    (dict(output_hidden_states=True), NotImplementedError, "output_hidden_states"),
    (dict(return_logits=True), NotImplementedError, "return_logits"),
    (dict(prompt_lookup_num_tokens=3), NotImplementedError, "prompt_lookup_num_tokens"),
    (dict(embeds_only=True), NotImplementedError, "inputs_embeds"),
    (dict(whole_generate=False), NotImplementedError, "prefill_begin"),
    (dict(target=_engine(head_dim=64)), NotImplementedError, "head_dim"),
    (dict(assistant_model=_engine(head_dim=64)), NotImplementedError, "head_dim"),
    (dict(assistant_model=_engine(max_batch=1)), NotImplementedError, "max_batch"),
    (dict(assistant_model=_engine(device="cuda:1")), NotImplementedError, "device"),
    (dict(assistant_model=_engine(vocab=301)), ValueError, "vocabulary"),
    (dict(target=_engine(max_len=54)), ValueError, "max_len"),              # 12 + 40 + 3 = 55
    (dict(assistant_model=_engine(max_len=54)), ValueError, "max_len"),
])
def test_resolve_assisted_refuses(kw, exc, word):
    args = dict(OK, assistant_model=_engine(vocab=296), num_assistant_tokens=3, target=_engine())
    args.update(kw)
    with pytest.raises(exc, match=word):
        L.resolve_assisted(**args)


def test_resolve_assisted_refuses_the_engine_itself():
    tgt = _engine()
    with pytest.raises(ValueError, match="assistant_model"):
        L.resolve_assisted(tgt, 3, target=tgt, **OK)


def test_keywords_are_named_arguments_and_state_keys_are_apart():
    """the keywords no longer vanish into **unused; an assisted request has a state key of its own per K"""
    sig = inspect.signature(L.LlamaEngine.prefill_begin).parameters
    for name in ("assistant_model", "num_assistant_tokens", "num_assistant_tokens_schedule", "assistant_confidence_threshold"):
        assert sig[name].default is None and sig[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD, name
    key = L.LlamaEngine._state_key
    assert key(1, False, False, 0, assist=0) == (1, False, False, 0)
    a3, a7 = key(1, False, False, 0, assist=3), key(1, False, False, 0, assist=7)
    others = {key(b, False, False, 0) for b in range(1, 9)} | {key(1, False, False, 0, True), key(1, False, False, 0, ngram=True),
                                                              key(1, False, False, 0, sample=True), key(1, False, False, 0, beam=(4, 8)),
                                                              key(1, False, False, 0, lookup=3), key(1, False, False, 0, lookup=7)}
    assert a3 != a7 and a3 not in others and a7 not in others and key(1, False, False, 1, assist=3) != a3
    assert "num_assistant_tokens" in inspect.signature(L.LlamaEngine.would_capture).parameters
    out = L.GenerateOutput(None)
    assert out.assisted is None and out.prompt_lookup is None


def test_ops_are_registered_and_mirrored():
    import spider_amd.torch_ops as T
    from spider_amd import lib, ops
    assert T.ASSIST_OP_NAMES == ("spec_assist_push_", "spec_assist_advance_")
    for n in T.ASSIST_OP_NAMES:
        assert hasattr(torch.ops.spider_hip, n) and n not in T.OP_NAMES + T.DECODE_OP_NAMES + T.SPEC_OP_NAMES
    for n, nargs in (("spider_spec_assist_push_i32", 17), ("spider_spec_assist_advance_i32", 18)):
        assert len(lib.SIGNATURES[n][1]) == nargs
    for n in ("spec_assist_push", "spec_assist_advance"):
        assert callable(getattr(ops, n))
    l = lib.load()      # validation happens on the host before any launch
    assert l.spider_spec_assist_push_i32(None, None, None, 2, 1, None, None, None, 4, 1, None, None, None, None, 296, 1, None) == -1
    assert b"required" in l.spider_last_error()
    assert l.spider_spec_assist_advance_i32(*([None] * 8), 4, None, 4, None, None, None, None, 296, 1, None) == -1
    assert b"required" in l.spider_last_error()

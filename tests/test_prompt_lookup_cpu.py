"""CPU: the host restatements of prompt-lookup decoding (spider_amd.llm.prompt_lookup_draft_host / spec_accept_host) against
transformers' PromptLookupCandidateGenerator and the fp32 oracle, the request validation (resolve_prompt_lookup), and the
surfaces the kernels are reachable through. No GPU."""
import inspect
import random

import pytest
import torch

import prompt_lookup_cases as pc
from spider_amd import llm as L


def test_draft_host_equals_transformers_candidate_generator():
    """a few hundred random sequences over 5 symbols, lengths 2 .. 60, K in {1, 3, 7}, N in {1, 2, 3}, max_length far away"""
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    rng = random.Random(0)
    n_with_draft = 0
    for _ in range(40):
        for K in (1, 3, 7):
            for N in (1, 2, 3):
                seq = [rng.randrange(5) for _ in range(rng.randrange(2, 61))]
                gen = PromptLookupCandidateGenerator(num_output_tokens=K, max_matching_ngram_size=N, max_length=10 ** 6)
                cand, _ = gen.get_candidates(torch.tensor([seq]))
                want = cand[0, len(seq):].tolist()
                got = L.prompt_lookup_draft_host(seq, K, N)
                assert got == want, (seq, K, N, got, want)
                n_with_draft += bool(got)
    assert n_with_draft > 200
    # the edges: one token, no repetition, K = 0
    assert L.prompt_lookup_draft_host([4], 3, 2) == [] and L.prompt_lookup_draft_host([1, 2, 3, 4], 3, 2) == []
    assert L.prompt_lookup_draft_host([1, 2, 1], 0, 2) == []
    assert L.prompt_lookup_draft_host([1, 2, 7, 1, 2, 8, 1, 2], 3, 2) == [7, 1, 2]      # the earliest of several matches
    assert L.prompt_lookup_draft_host([1, 2, 3, 9, 8, 3, 7, 1, 2, 3], 2, 3) == [9, 8]   # the longest n-gram first


def test_accept_host():
    assert L.spec_accept_host([5, 6, 7, 8], 3, [6, 7, 8, 9]) == 3
    assert L.spec_accept_host([5, 6, 7, 8], 3, [6, 7, 0, 8]) == 2
    assert L.spec_accept_host([5, 6, 7, 8], 3, [0, 7, 8, 9]) == 0
    assert L.spec_accept_host([5, 6, 7, 8], 1, [6, 7, 8, 9]) == 1       # rows past n_draft are filler
    assert L.spec_accept_host([5, 5, 5, 5], 0, [5, 5, 5, 5]) == 0


def test_host_simulation_on_the_successor_model_reproduces_greedy_and_the_counts():
    cfg, w = pc.successor_model()
    greedy, margin = pc.successor_greedy()
    v, want = pc.PROMPT[-1], []
    for _ in range(len(greedy)):
        v = pc.succ(v)
        want.append(v)
    assert list(greedy) == want, "the oracle's greedy output has to follow succ"
    print(f"MEASURED successor model: minimum top-2 margin {margin:.2f}")
    assert margin > 10.0        # measured 14.2: bf16 and the quantised engines cannot flip a token
    for K in (1, 3, 7):
        tok, rec = pc.simulate_oracle(cfg, w, pc.PROMPT, pc.T_NEW, K, 2)
        assert tok == list(greedy[:pc.T_NEW]), K
        tok2, rec2 = pc.simulate_tokens(pc.PROMPT, greedy, pc.T_NEW, K, 2)
        assert tok2 == tok and rec2 == rec, (K, rec, rec2)
        assert rec["steps"] + rec["accepted"] >= pc.T_NEW - 1 and rec["accepted"] > 0
        if K == 3:
            assert {k: rec[k] for k in pc.K3N2} == pc.K3N2, rec


def test_kernel_cases_cover_the_named_situations():
    by = {c.name: c.expected() for c in pc.named_spec_cases()}
    assert by["no-match-draft"]["n_draft"].tolist() == [0, 0] and by["tail-matches-only-itself-adv"]["n_draft"].tolist() == [0, 0]
    assert by["continuation-shorter-than-K-draft"]["n_draft"][0] == 2
    assert by["earliest-of-several-adv"]["ids"][:4].tolist() == [2, 7, 1, 2]
    e = by["no-draft-after-leftover-drafts"]
    assert e["n_draft"].tolist() == [0, 0] and e["ids"].tolist() == [25] * 4 + [26] * 4
    e = by["append-across-cap"]
    assert e["n_hist"].tolist() == [19, 17] and -1 in e["ids"].tolist()
    assert by["all-accepted"]["counters"][0].tolist() == [6, 12, 7]


OK = dict(B=1, S=12, max_new_tokens=40, max_len=64, decode_rows=8, head_dim=128)


def test_resolve_prompt_lookup_accepts():
    assert L.resolve_prompt_lookup(None, 5, **OK) is None and L.resolve_prompt_lookup(0, 99, **OK) is None
    assert L.resolve_prompt_lookup(None, B=4, S=100, max_new_tokens=100, max_len=10, do_sample=True) is None    # off: nothing is looked at
    assert L.resolve_prompt_lookup(3, **OK) == (3, 2) and L.resolve_prompt_lookup(3, None, **OK) == (3, 2)
    assert L.resolve_prompt_lookup(1, 1, **OK) == (1, 1) and L.resolve_prompt_lookup(7, 8, **OK) == (7, 8)
    assert L.resolve_prompt_lookup(7, 2, **dict(OK, max_len=59)) == (7, 2)      # 12 + 40 + 7


@pytest.mark.parametrize("kw, exc, word", [
    (dict(prompt_lookup_num_tokens=8), ValueError, "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=-1), ValueError, "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=True), ValueError, "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=2.0), ValueError, "prompt_lookup_num_tokens"),
    (dict(prompt_lookup_num_tokens=4, decode_rows=4), ValueError, "prompt_lookup_num_tokens"),
    (dict(max_matching_ngram_size=0), ValueError, "max_matching_ngram_size"),
    (dict(max_matching_ngram_size=9), ValueError, "max_matching_ngram_size"),
    (dict(max_matching_ngram_size=2.0), ValueError, "max_matching_ngram_size"),
    (dict(B=2), NotImplementedError, "batch"),
    (dict(do_sample=True), NotImplementedError, "do_sample"),
    (dict(num_beams=2), NotImplementedError, "num_beams"),
    (dict(processed=True), NotImplementedError, "repetition_penalty"),
    (dict(no_repeat_ngram_size=3), NotImplementedError, "no_repeat_ngram_size"),
    (dict(output_hidden_states=True), NotImplementedError, "output_hidden_states"),
    (dict(return_logits=True), NotImplementedError, "return_logits"),
    (dict(head_dim=64), NotImplementedError, "head_dim"),
    (dict(max_len=54), ValueError, "max_len"),          # 12 + 40 + 3 = 55
])
def test_resolve_prompt_lookup_refuses(kw, exc, word):
    args = dict(OK, prompt_lookup_num_tokens=3, max_matching_ngram_size=2)
    args.update(kw)
    with pytest.raises(exc, match=word):
        L.resolve_prompt_lookup(**args)


def test_keywords_are_named_arguments_and_state_keys_are_apart():
    """the two keywords no longer vanish into **unused; a prompt-lookup request has a state key of its own per K"""
    sig = inspect.signature(L.LlamaEngine.prefill_begin).parameters
    assert sig["prompt_lookup_num_tokens"].default is None and sig["max_matching_ngram_size"].default is None
    key = L.LlamaEngine._state_key
    assert key(1, False, False, 0) == (1, False, False, 0) and key(1, False, False, 0, lookup=0) == (1, False, False, 0)
    k3, k7 = key(1, False, False, 0, lookup=3), key(1, False, False, 0, lookup=7)
    others = {key(b, False, False, 0) for b in range(1, 9)} | {key(1, False, False, 0, True), key(1, False, False, 0, ngram=True),
                                                              key(1, False, False, 0, sample=True), key(1, False, False, 0, beam=(4, 8))}
    assert k3 != k7 and k3 not in others and k7 not in others and key(1, False, False, 1, lookup=3) != k3
    assert "prompt_lookup_num_tokens" in inspect.signature(L.LlamaEngine.would_capture).parameters
    assert L.GenerateOutput(None).prompt_lookup is None


def test_ops_are_registered_and_mirrored():
    import spider_amd.torch_ops as T
    from spider_amd import lib, ops
    assert T.SPEC_OP_NAMES == ("attn_verify", "prompt_lookup_draft_", "spec_advance_draft_")
    for n in T.SPEC_OP_NAMES:
        assert hasattr(torch.ops.spider_hip, n) and n not in T.OP_NAMES + T.DECODE_OP_NAMES
    for n, nargs in (("spider_attn_verify_bf16", 17), ("spider_prompt_lookup_draft_i32", 15), ("spider_spec_advance_draft_i32", 18)):
        assert len(lib.SIGNATURES[n][1]) == nargs
    for n in ("attn_verify", "spec_advance_draft", "prompt_lookup_draft"):
        assert callable(getattr(ops, n))
    l = lib.load()      # validation happens on the host before any launch
    assert l.spider_attn_verify_bf16(None, None, None, None, None, None, None, None, 1, 2, 4, 2, 64, 16, 1.0, 1, None) == -1
    assert b"head_dim" in l.spider_last_error()
    assert l.spider_attn_verify_bf16(None, None, None, None, None, None, None, None, 1, 9, 4, 2, 128, 16, 1.0, 1, None) == -1
    assert b"rows per sequence" in l.spider_last_error()
    assert l.spider_attn_verify_bf16(None, None, None, None, None, None, None, None, 1, 2, 18, 2, 128, 16, 1.0, 1, None) == -1
    assert l.spider_spec_advance_draft_i32(*([None] * 8), 4, None, None, 4, None, None, None, 4, 1, None) == -1

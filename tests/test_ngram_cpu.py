"""CPU: the host statement of no_repeat_ngram_size (spider_amd.llm.ngram_banned_host, resolve_no_repeat_ngram and the per-row
banned sets of process_logits_host) against transformers: the processor class on random sequences, and HF's own greedy `generate`
replayed from its raw logits. Pins which ids the n-gram scan sees in each input mode (input_ids: the row's prompt ids, pads
included, + the generated ids; inputs_embeds: the generated ids alone), the validation errors and the state keys."""
import random

import pytest
import torch

from spider_amd.llm import (LlamaEngine, ngram_banned_host, process_logits_host, resolve_beam_search, resolve_logits_processors,
                            resolve_no_repeat_ngram)

V, B, S, N = 97, 3, 7, 24


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_ngram_banned_host_equals_hf_processor(n):
    from transformers import NoRepeatNGramLogitsProcessor
    rng = random.Random(1000 + n)
    proc = NoRepeatNGramLogitsProcessor(n)
    nonempty = 0
    for L in range(0, 41):
        for alphabet in (4, 4, 5, 5, 6, 6):
            seq = [rng.randrange(alphabet) for _ in range(L)]
            sc = proc(torch.tensor([seq], dtype=torch.long).view(1, L), torch.zeros(1, 9))
            want = set(torch.isinf(sc[0]).nonzero().view(-1).tolist())
            got = ngram_banned_host(seq, n)
            assert got == want, (n, seq, got, want)
            nonempty += bool(want)
            if L + 1 < n:
                assert got == set()
    assert nonempty > 0         # repeats abound over such alphabets: the comparison is not one of empty sets


def test_size_longer_than_the_sequence_bans_nothing():
    assert ngram_banned_host([1, 2, 1, 2], 6) == set() and ngram_banned_host([1, 2, 1, 2], 5) == set()
    assert ngram_banned_host([1, 2, 1], 2) == {2} and ngram_banned_host([], 1) == set() and ngram_banned_host([4, 4, 9], 1) == {4, 9}


def _tiny_hf(seed=0):       # the recipe of tests/test_logits_processors_cpu.py
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=128)
    m = LlamaForCausalLM(cfg).eval()
    for p in m.parameters():
        p.data.mul_(4.0)
    return m


_MODEL = {}


def _model():
    if 0 not in _MODEL:
        _MODEL[0] = _tiny_hf(0)
    return _MODEL[0]


@pytest.mark.parametrize("mode", ["ids", "embeds"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_host_replay_equals_hf_generate(n, mode):
    """HF greedy with no_repeat_ngram_size (and repetition_penalty = 0.5, which rewards repeats, so that the tiny model loops at
    once and the n-gram ban has work to do): the host processors on HF's raw logits reproduce its tokens at every step."""
    m = _model()
    ids = torch.randint(3, V, (B, S), generator=torch.Generator().manual_seed(0))
    am = torch.ones(B, S, dtype=torch.long)
    for b, npad in ((1, 2), (2, 4)):        # left padding: the pad id 0 sits in input_ids, where HF's processor sees it
        ids[b, :npad] = 0
        am[b, :npad] = 0
    pen = 0.5
    args = dict(max_new_tokens=N, do_sample=False, eos_token_id=None, pad_token_id=0, output_logits=True, return_dict_in_generate=True,
                attention_mask=am, no_repeat_ngram_size=n, repetition_penalty=pen)
    if mode == "ids":
        out = m.generate(ids, **args)
        ref, prompt = out.sequences[:, S:], ids
    else:
        out = m.generate(inputs_embeds=m.get_input_embeddings()(ids), **args)
        ref, prompt = out.sequences, None
    raw = torch.stack(out.logits, 1).float()
    assert ref.shape == (B, N) and raw.shape == (B, N, V)
    p, min_new, ban = resolve_logits_processors(S, None, pen)
    assert resolve_no_repeat_ngram(n) == n
    seen = torch.zeros(B, V, dtype=torch.bool)
    seqs = [[] for _ in range(B)]
    if prompt is not None:
        seen.scatter_(1, prompt, True)
        seqs = [prompt[b].tolist() for b in range(B)]
    touched = 0
    for t in range(N):
        banned = [ngram_banned_host(seqs[b], n) for b in range(B)]
        lv = process_logits_host(raw[:, t], seen, p, ban, None, t, min_new, banned)
        nxt = lv.argmax(-1)
        assert torch.equal(nxt, ref[:, t]), (t, nxt, ref[:, t])
        for b in range(B):
            assert int(nxt[b]) not in banned[b]
            touched += int(raw[b, t].argmax()) in banned[b]
            seqs[b].append(int(nxt[b]))
        seen.scatter_(1, nxt[:, None], True)
    assert touched > 0, "no raw arg-max was n-gram-banned: the case decided nothing"


def test_resolution_and_validation():
    r = resolve_no_repeat_ngram
    assert r(None) == 0 and r(0) == 0 and r(1) == 1 and r(3) == 3 and r(10 ** 6) == 10 ** 6
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            r(bad)
    from transformers import NoRepeatNGramLogitsProcessor
    for bad in (-1, 2.5, 0):
        with pytest.raises(ValueError):
            NoRepeatNGramLogitsProcessor(bad)
    # beam search refuses it the way it refuses the other processors, and says so
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        resolve_beam_search(1, 2, 8, V, None, processed=r(3) > 0)
    assert resolve_beam_search(1, 2, 8, V, None, processed=r(0) > 0) == 4
    # process_logits_host: neutral by default
    lg = torch.randn(2, V)
    z = torch.zeros(2, V, dtype=torch.bool)
    assert torch.equal(process_logits_host(lg, z, 1.0, [], None, 0, 0), lg)
    got = process_logits_host(lg, z, 1.0, [], None, 0, 0, [{3, V + 4}, set()])
    assert got[0, 3] == -float("inf") and torch.equal(got[1], lg[1]) and int(torch.isinf(got).sum()) == 1


def test_state_keys():
    k = LlamaEngine._state_key
    assert k(3, False, True, 0) == (3, False, True, 0)
    assert k(3, False, True, 0, True) == (3, False, True, 0, True)
    assert k(3, False, True, 1, False, None, True) == (3, False, True, 1, "sample")
    assert k(3, False, True, 1, True, None, True) == (3, False, True, 1, True, "sample")
    assert k(2, False, False, 0, False, (4, 8)) == (2, False, False, 0, "beam", 4, 8)
    today = {k(3, False, True, 0), k(3, False, True, 0, True), k(3, False, True, 0, False, None, True), k(3, False, True, 0, True, None, True)}
    ng = k(3, False, True, 0, True, None, False, True)
    ngs = k(3, False, True, 0, True, None, True, True)
    assert ng == (3, False, True, 0, True, "ngram") and ngs == (3, False, True, 0, True, "sample", "ngram")
    assert ng not in today and ngs not in today and ng != ngs


def test_custom_ops_have_schema_and_fake_impl():
    import spider_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert T.DECODE_OP_NAMES == ("ngram_ban_", "decode_advance_seen_ngram_")
    for name in T.DECODE_OP_NAMES:
        assert getattr(torch.ops.spider_hip, name).default._schema.name == f"spider_hip::{name}"
    with FakeTensorMode():
        e = lambda *s: torch.empty(*s, dtype=torch.int32, device="cuda")
        o = torch.ops.spider_hip
        Bq, W = 2, (V + 31) // 32
        assert o.ngram_ban_(e(Bq, 16), e(1), e(Bq, 32), e(Bq), e(1), e(Bq, W), e(Bq, W), V) is None
        assert o.decode_advance_seen_ngram_(e(Bq), e(Bq), e(Bq), e(Bq), e(Bq), e(Bq, 32), e(Bq), e(Bq, W), e(Bq, 16), e(1), e(1),
                                            e(Bq, W), e(Bq, W), V) is None


def test_engine_signature_names_the_keyword():
    import inspect
    sig = inspect.signature(LlamaEngine.prefill_begin).parameters
    assert "no_repeat_ngram_size" in sig and sig["no_repeat_ngram_size"].default is None
    wc = inspect.signature(LlamaEngine.would_capture).parameters
    assert "no_repeat_ngram" in wc and wc["no_repeat_ngram"].default is False

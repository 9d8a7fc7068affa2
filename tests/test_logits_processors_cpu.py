"""CPU: the host statement of the greedy logits processors (spider_amd.llm.resolve_logits_processors + process_logits_host, which
the engine uses to resolve its keywords and the GPU tests assume) against transformers' own `generate`: a replay of greedy decode
with the processors applied to HF's RAW logits (`output_logits`) and the history so far must give HF's tokens, one by one.
Pins: which ids the repetition penalty sees in each input mode (input_ids: every prompt id, pads included, + generated ids;
inputs_embeds only: the generated ids), how min_length / min_new_tokens turn into ONE count of EOS-free tokens in each input mode,
that suppress_tokens and single-token bad_words_ids are one ban set, and the validation errors."""
import pytest
import torch

from spider_amd.llm import process_logits_host, resolve_logits_processors

V, B, S, N = 97, 3, 7, 24


def _tiny_hf(seed=0):       # the recipe of tests/test_generate_semantics_cpu.py
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=128)
    m = LlamaForCausalLM(cfg).eval()
    for p in m.parameters():
        p.data.mul_(4.0)
    return m


_CACHE = {}


def _setup(seed):
    """model, prompt ids, a left-padded mask, and EOS candidates taken from the free-running stream (shared, never modified)"""
    if seed not in _CACHE:
        m = _tiny_hf(seed)
        ids = torch.randint(3, V, (B, S), generator=torch.Generator().manual_seed(seed))
        free = m.generate(ids, max_new_tokens=N, do_sample=False, eos_token_id=None, pad_token_id=0)[:, S:]
        _CACHE[seed] = (m, ids, free)
    return _CACHE[seed]


def _replay(hf_out, prompt, eos, pad, kw):
    """Greedy decode restated on the host from HF's raw logits: returns the tokens [B, n] with HF's pad-after-EOS bookkeeping."""
    raw = torch.stack(hf_out.logits, 1).float()                     # [B, n, V] raw (unprocessed) logits of every step
    n = raw.shape[1]
    S_in = prompt.shape[1] if prompt is not None else kw["_embeds_len"]
    p, min_new, ban = resolve_logits_processors(S_in, eos, kw.get("repetition_penalty", 1.0), kw.get("min_length", 0),
                                                kw.get("min_new_tokens", 0), kw.get("suppress_tokens"), kw.get("bad_words_ids"))
    seen = torch.zeros(B, V, dtype=torch.bool)
    if prompt is not None:
        seen.scatter_(1, prompt, True)
    unfinished = torch.ones(B, dtype=torch.bool)
    toks = []
    for t in range(n):
        lv = process_logits_host(raw[:, t], seen, p, ban, eos, t, min_new)
        nxt = lv.argmax(-1)                                         # torch CPU argmax: first (lowest) index among equals
        if eos:
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
        toks.append(nxt)
        seen.scatter_(1, nxt[:, None], True)
        if eos:
            unfinished &= ~torch.isin(nxt, torch.tensor(eos))
    return torch.stack(toks, 1), (p, min_new, ban)


def _hf(m, ids, mode, am, eos, pad, kw):
    args = dict(max_new_tokens=N, do_sample=False, eos_token_id=eos, pad_token_id=pad, output_logits=True, return_dict_in_generate=True)
    args.update({k: v for k, v in kw.items() if not k.startswith("_")})
    if am is not None:
        args["attention_mask"] = am
    if mode == "ids":
        out = m.generate(ids, **args)
        return out, out.sequences[:, S:]
    out = m.generate(inputs_embeds=m.get_input_embeddings()(ids), **args)
    return out, out.sequences


CASES = [
    dict(repetition_penalty=1.05),
    dict(repetition_penalty=1.3),
    dict(repetition_penalty=1.3, min_new_tokens=6),
    dict(min_length=S + 5),             # input_ids: 5 EOS-free tokens; inputs_embeds: HF subtracts the prompt length -> also 5
    dict(min_length=4),                 # shorter than the prompt: a no-op in both modes
    dict(min_length=1),                 # the reference's default (spider.py:1471): a no-op
    dict(repetition_penalty=1.05, min_new_tokens=6, suppress_tokens=[5, 11, 96]),
    dict(repetition_penalty=1.3, bad_words_ids=[[7]], suppress_tokens=[0]),
]


@pytest.mark.parametrize("mode", ["ids", "embeds"])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("seed", [0, 1])
def test_host_replay_equals_hf_generate(seed, case, padded, mode):
    m, ids, free = _setup(seed)
    kw = dict(CASES[case])
    am = None
    if padded:      # left padding: row 1 has 2 pads, row 2 has 4 (pad id 0 sits in input_ids and is penalised there, as in HF)
        ids = ids.clone()
        am = torch.ones(B, S, dtype=torch.long)
        for b, npad in ((1, 2), (2, 4)):
            ids[b, :npad] = 0
            am[b, :npad] = 0
    # EOS ids that the free-running stream emits early (so that min_new / min_length have something to forbid) and late
    eos = sorted({int(free[0, 2]), int(free[1, 11])})
    for name in ("suppress_tokens",):                # keep the EOS ids out of the ban set: the cases are about the EOS rule
        if name in kw:
            kw[name] = [t for t in kw[name] if t not in eos]
    if "bad_words_ids" in kw:                        # ... and one bad word that IS an EOS id, which HF drops from the list
        kw["bad_words_ids"] = kw["bad_words_ids"] + [[eos[0]]]
    pad = 1
    out, ref = _hf(m, ids, mode, am, eos, pad, kw)
    kw["_embeds_len"] = S
    got, (p, min_new, ban) = _replay(out, ids if mode == "ids" else None, eos, pad, kw)
    assert got.shape == ref.shape and torch.equal(got, ref), (kw, got, ref)
    # the resolved count is what the case says
    want_min_new = kw.get("min_new_tokens") or max(0, kw.get("min_length", 0) - S)
    assert min_new == want_min_new
    if min_new:
        assert not torch.isin(ref[:, :min_new], torch.tensor(eos)).any()
    if "bad_words_ids" in kw:
        assert eos[0] not in ban and 7 in ban


def test_processors_change_the_stream():
    """the cases above are not vacuous: a penalty of 1.3 and a min_new_tokens count change HF's own tokens"""
    m, ids, free = _setup(0)
    pen = m.generate(ids, max_new_tokens=N, do_sample=False, eos_token_id=None, pad_token_id=0, repetition_penalty=1.3)[:, S:]
    assert not torch.equal(pen, free)
    eos = [int(free[0, 2])]
    a = m.generate(ids, max_new_tokens=N, do_sample=False, eos_token_id=eos, pad_token_id=1)[:, S:]
    b = m.generate(ids, max_new_tokens=N, do_sample=False, eos_token_id=eos, pad_token_id=1, min_new_tokens=6)[:, S:]
    assert int(a[0, 2]) == eos[0] and int(b[0, 2]) != eos[0]


def test_resolution_and_validation():
    r = resolve_logits_processors
    assert r(7, [2]) == (1.0, 0, [])
    assert r(7, [2], repetition_penalty=1) == (1.0, 0, [])                  # the reference's integer default
    assert r(7, [2], min_length=1) == (1.0, 0, [])                          # the reference's min_length=1
    assert r(7, None, min_length=50, min_new_tokens=9) == (1.0, 0, [])      # no EOS id: nothing to ban
    assert r(7, [2], min_length=10) == (1.0, 3, [])
    assert r(7, [2], min_length=10, min_new_tokens=2) == (1.0, 2, [])       # min_new_tokens takes precedence (HF)
    assert r(7, [2, 3], suppress_tokens=[9, 4, 9], bad_words_ids=[[4], [2], [6]]) == (1.0, 0, [4, 6, 9])
    with pytest.raises(NotImplementedError, match=r"\[5, 6\]"):
        r(7, [2], bad_words_ids=[[4], [5, 6]])
    for bad in (0.0, -1.5, 2, "1.3"):
        with pytest.raises(ValueError, match="strictly positive float"):
            r(7, [2], repetition_penalty=bad)
    from transformers import RepetitionPenaltyLogitsProcessor
    for bad in (0.0, -1.5, 2):
        with pytest.raises(ValueError):
            RepetitionPenaltyLogitsProcessor(penalty=bad)
    with pytest.raises(ValueError):
        r(7, [2], min_new_tokens=-1)
    with pytest.raises(ValueError):
        r(7, list(range(9)), min_new_tokens=3)


def test_engine_signature_names_the_keywords():
    """the keywords are named parameters of prefill_begin (no longer swallowed by **unused) with neutral defaults"""
    import inspect
    from spider_amd.llm import LlamaEngine
    sig = inspect.signature(LlamaEngine.prefill_begin).parameters
    for name, default in (("repetition_penalty", 1.0), ("min_length", 0), ("min_new_tokens", 0), ("suppress_tokens", None),
                          ("bad_words_ids", None)):
        assert name in sig and sig[name].default == default
    assert "processed" in inspect.signature(LlamaEngine.would_capture).parameters

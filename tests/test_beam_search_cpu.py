"""CPU: the host half of beam search (spider_amd.llm.beam_finalize_host, resolve_beam_search) against transformers'
own `generate(num_beams=K)`. The trace the device would write -- per step the C = max(2, 1 + n_eos) * K best continuations of every
batch row -- is built here from HF's RAW logits (`output_logits`) with the torch ops HF uses (log_softmax, topk), so the replay of
the finished-hypotheses bookkeeping (length penalty, early_stopping False / True / "never", the early-stop heuristic, max length,
num_return_sequences, the fill value) has to give HF's sequences and scores exactly, and has to end at the step HF's loop ended."""
import itertools

import pytest
import torch

from beam_checks import beam_step_host
from spider_amd.llm import beam_finalize_host, resolve_beam_search

V, S, N = 97, 7, 12


def _tiny_hf(seed=0):       # the recipe of tests/test_logits_processors_cpu.py
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=128)
    m = LlamaForCausalLM(cfg).eval()
    for p in m.parameters():
        p.data.mul_(4.0)
    return m


_CACHE = {}


def _model():
    if "m" not in _CACHE:
        _CACHE["m"] = _tiny_hf(0)
    return _CACHE["m"]


def _inputs(B, mode):
    """'ids': left-padded input_ids + attention_mask (row b has b pads); 'embeds': inputs_embeds of the same ids, no padding"""
    m = _model()
    ids = torch.randint(3, V, (B, S), generator=torch.Generator().manual_seed(5 + B))
    if mode == "embeds":
        return dict(inputs_embeds=m.get_input_embeddings()(ids).detach()), None
    am = torch.ones(B, S, dtype=torch.long)
    for b in range(B):
        ids[b, :b] = 0
        am[b, :b] = 0
    return dict(input_ids=ids, attention_mask=am), ids


def _hf(K, B, mode, eos, pad, **kw):
    inp, prompt = _inputs(B, mode)
    out = _model().generate(**inp, num_beams=K, max_new_tokens=N, do_sample=False, eos_token_id=eos, pad_token_id=pad,
                            output_logits=True, output_scores=True, return_dict_in_generate=True, **kw)
    return out, prompt


def _free_stream(K, B, mode):
    """the best beam's tokens of row 0 without any EOS id (shared, never modified): where the EOS ids of the cases come from"""
    key = (K, B, mode)
    if key not in _CACHE:
        out, prompt = _hf(K, B, mode, None, 0)
        _CACHE[key] = out.sequences[0, (0 if prompt is None else S):].clone()
    return _CACHE[key]


def _trace_from_hf(out, B, K, C, eos):
    """the device's trace, restated with torch ops on HF's raw logits of its running beams"""
    run = torch.zeros(B, K)
    run[:, 1:] = -1e9
    sc, bm, tk = [], [], []
    for lg in out.logits:
        (s, b, t), (run, _, _) = beam_step_host(lg, run, C, eos)
        sc.append(s); bm.append(b); tk.append(t)
    return torch.stack(sc), torch.stack(bm), torch.stack(tk)


def _eos_ids(K, B, mode, n_eos):
    free = _free_stream(K, B, mode)
    return [None, [int(free[3])], sorted({int(free[3]), int(free[7])})][n_eos]


@pytest.mark.parametrize("n_eos", [0, 1, 2])
@pytest.mark.parametrize("mode", ["ids", "embeds"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [2, 4])
def test_finalize_equals_hf_beam_search(K, B, mode, n_eos):
    eos = _eos_ids(K, B, mode, n_eos)
    C = resolve_beam_search(B, K, 16, V, eos, decode_rows=16)
    assert C == max(2, 1 + n_eos) * K
    pad = 1
    ended_early = finished_midway = 0
    for lp, es, nrs in itertools.product((0.0, 1.0, 2.0), (False, True, "never"), (1, K)):
        out, prompt = _hf(K, B, mode, eos, pad, length_penalty=lp, early_stopping=es, num_return_sequences=nrs)
        n_hf = len(out.logits)
        trace = _trace_from_hf(out, B, K, C, eos)
        res, st = beam_finalize_host(trace, K, N, eos, pad, lp, es, nrs, prompt)
        what = (lp, es, nrs)
        assert res is not None and res["n_steps"] == n_hf, what
        assert res["sequences"].shape == out.sequences.shape and torch.equal(res["sequences"], out.sequences), what
        assert torch.equal(res["sequences_scores"], out.sequences_scores), what
        assert torch.equal(res["beam_indices"].long(), out.beam_indices.long()), what
        # in blocks of 5 steps, as `sync_every=5` hands them over: nothing before the last block, then the same result
        st2, got = None, None
        for t0 in range(0, n_hf, 5):
            assert got is None
            got, st2 = beam_finalize_host(tuple(x[t0:t0 + 5] for x in trace), K, N, eos, pad, lp, es, nrs, prompt, st2, t0)
        assert torch.equal(got["sequences"], out.sequences) and torch.equal(got["sequences_scores"], out.sequences_scores)
        # over-decoded steps behind HF's last one are ignored
        if n_hf < N:
            junk = tuple(torch.cat([x, x[-1:].clone()]) for x in trace)
            r3, _ = beam_finalize_host(junk, K, N, eos, pad, lp, es, nrs, prompt)
            assert r3["n_steps"] == n_hf and torch.equal(r3["sequences"], out.sequences)
        ended_early += n_hf < N
        gen = out.sequences if prompt is None else out.sequences[:, S:]
        finished_midway += bool(eos) and bool(torch.isin(gen[:, :-1], torch.tensor(eos or [-5])).any())
    if eos:     # the cases count: hypotheses finished before the last step (loops that end early: test_knobs_change_hf_output)
        assert finished_midway > 0


def test_knobs_change_hf_output():
    """the cases above are not vacuous: the length penalty and early_stopping change what HF returns"""
    K, B, mode = 2, 1, "ids"
    eos = _eos_ids(K, B, mode, 2)
    outs = {(lp, es): _hf(K, B, mode, eos, 1, length_penalty=lp, early_stopping=es)[0] for lp in (0.0, 2.0) for es in (True, "never")}
    seqs = {k: (tuple(v.sequences.shape), v.sequences.flatten().tolist()) for k, v in outs.items()}
    assert seqs[(0.0, True)] != seqs[(2.0, "never")]
    assert len(outs[(0.0, True)].logits) < len(outs[(2.0, "never")].logits)


def test_beam_step_host_orders_and_picks():
    lg = torch.full((2, 6), -10.0)
    lg[0, 4], lg[0, 2], lg[1, 5] = 3.0, 2.0, 2.5
    run = torch.tensor([[0.0, -0.5]])
    (s, b, t), (rs, rb, rt) = beam_step_host(lg, run, 4, [4])
    assert (b[0, :3].tolist(), t[0, :3].tolist()) == ([0, 1, 0], [4, 5, 2])
    assert torch.all(s[0, :-1] >= s[0, 1:])
    assert (rb[0].tolist(), rt[0].tolist()) == ([1, 0], [5, 2]) and torch.equal(rs[0], s[0, 1:3])     # token 4 is EOS: not running


def test_validation_errors():
    r = lambda **kw: resolve_beam_search(kw.pop("B", 1), kw.pop("num_beams", 4), kw.pop("max_batch", 8), kw.pop("vocab", V),
                                         kw.pop("eos", [2]), **kw)
    assert r() == 8 and r(eos=None) == 8 and r(eos=[2, 3]) == 12 and r(num_beams=8, eos=[2, 3, 4]) == 32
    assert r(B=2, num_beams=4) == 8 and r(num_return_sequences=4, early_stopping="never", length_penalty=0) == 8
    for bad in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="num_beams"):
            r(num_beams=bad)
    with pytest.raises(ValueError, match="rows"):
        r(B=3, num_beams=4)                 # 12 rows > DECODE_ROWS
    with pytest.raises(ValueError, match="max_batch"):
        r(B=1, num_beams=4, max_batch=2)
    with pytest.raises(ValueError, match="continuations"):
        r(num_beams=8, eos=[2, 3, 4, 5])    # 5 * 8 = 40 > 32
    with pytest.raises(ValueError, match="continuations"):
        r(num_beams=4, vocab=7)
    with pytest.raises(ValueError, match="num_return_sequences"):
        r(num_return_sequences=5)
    with pytest.raises(ValueError, match="early_stopping"):
        r(early_stopping="always")
    for kw in (dict(do_sample=True), dict(stopping_criteria=[lambda i, s: False]), dict(output_hidden_states=True),
               dict(processed=True), dict(num_beam_groups=2), dict(constraints=[object()]), dict(force_words_ids=[[3]])):
        with pytest.raises(NotImplementedError):
            r(**kw)


def test_engine_signature_names_the_keywords():
    import inspect
    from spider_amd.llm import GenerateOutput, LlamaEngine
    sig = inspect.signature(LlamaEngine.prefill_begin).parameters
    for name, default in (("num_beams", 1), ("length_penalty", 1.0), ("early_stopping", False), ("num_return_sequences", 1),
                          ("num_beam_groups", 1), ("constraints", None)):
        assert name in sig and sig[name].default == default
    assert "num_beams" in inspect.signature(LlamaEngine.would_capture).parameters
    # num_beams = 1 keeps the keys the greedy states have always had
    assert LlamaEngine._state_key(3, False, True, 0) == (3, False, True, 0)
    assert LlamaEngine._state_key(3, False, True, 0, True) == (3, False, True, 0, True)
    assert LlamaEngine._state_key(2, False, True, 0, False, (4, 8)) == (2, False, True, 0, "beam", 4, 8)
    o = GenerateOutput(torch.zeros(1, 2))
    assert o.sequences_scores is None and o.beam_indices is None

"""GPU: LlamaEngine.generate(do_sample=True) end to end: the two sampling launches behind the raw-logits lm_head inside the decode graph.

  * every step of every row passes the token check of tests/sample_checks.py, recomputed on the host from the engine's own raw
    logits (return_logits), the prompt and the generated history (the processors' `seen` set) and
    sample_uniform_host(seed, absolute row, step) -- processors off, on (repetition_penalty=1.05, min_new_tokens=5) and with an EOS
    id taken from the stream; both weight layouts, both input modes;
  * top_k=1 and top_p=1e-6 return the sequences of do_sample=False with the same processors;
  * one seed gives one output, whatever the execution: graph / eager, sync_every 1 / 5, generate / prefill_begin + decode_finish, an
    11-row call (groups of 8 + 3) against the 8-row call; two seeds differ; torch.manual_seed makes seed=None reproducible;
  * a sampling call adds exactly one state key and leaves the greedy and beam requests' keys, graphs and outputs alone."""
import pytest
import torch

from sample_checks import check_sample_token
from spider_amd.llm import process_logits_host, resolve_logits_processors, sample_uniform_host
from test_llm_beam_gpu import N, S, V, _engine, _inputs

pytestmark = pytest.mark.gpu

SAMPLING = dict(temperature=0.8, top_k=20, top_p=0.9)
PROC = dict(repetition_penalty=1.05, min_new_tokens=5)


def _gen(out, mode):
    return (out.sequences[:, S:] if mode == "ids" else out.sequences).cpu()


def _check_steps(out, ids, mode, seed, eos=None, row0=0, proc=None, sampling=SAMPLING):
    """every step of every row, up to the row's first EOS; returns the number of steps checked"""
    proc = proc or {}
    logits, gen = out.logits.float().cpu(), _gen(out, mode)
    B, n = gen.shape
    assert logits.shape == (B, n, V)
    pen, min_new, ban = resolve_logits_processors(S, eos, proc.get("repetition_penalty", 1.0), 0, proc.get("min_new_tokens", 0))
    seen = torch.zeros(B, V, dtype=torch.bool)
    if mode == "ids":
        seen.scatter_(1, ids, True)
    done = 0
    for b in range(B):
        for t in range(n):
            x = process_logits_host(logits[b:b + 1, t], seen[b:b + 1], pen, ban, eos, t, min_new)[0]
            r = check_sample_token(x, sampling["temperature"], sampling["top_k"], sampling["top_p"],
                                   sample_uniform_host(seed, row0 + b, t), gen[b, t])
            assert t >= min_new or not eos or int(gen[b, t]) not in eos
            seen[b, gen[b, t]] = True
            done += 1
            if eos and int(gen[b, t]) in eos:
                break
    return done


@pytest.mark.parametrize("mode", ["ids", "embeds"])
@pytest.mark.parametrize("row_major", [False, True])
@pytest.mark.parametrize("processors", [False, True])
def test_sampled_steps_match_host(dev, processors, row_major, mode):
    B, seed = 3, 0xC0FFEE123456789
    eng, _ = _engine(dev, 2 + processors, 8, 31 + processors, row_major)
    inp, ids, am = _inputs(eng, B, 31, mode)
    proc = PROC if processors else {}
    kw = dict(max_new_tokens=N, do_sample=True, seed=seed, return_dict_in_generate=True, return_logits=True, **SAMPLING, **proc)
    free = eng.generate(**inp, **kw)
    assert _gen(free, mode).shape == (B, N)
    assert _check_steps(free, ids, mode, seed, proc=proc) == B * N
    assert (B, False, True, 0) + ((True,) if processors else ()) + ("sample",) in eng._graphs
    # an EOS id from the stream (past min_new_tokens): EOS-free before, rows end at it, pads behind it
    eos = [int(_gen(free, mode)[0, 7])]
    out = eng.generate(**inp, **kw, eos_token_id=eos, pad_token_id=1)
    gen = _gen(out, mode)
    assert _check_steps(out, ids, mode, seed, eos=eos, proc=proc) >= gen.shape[1]
    hit = (gen == eos[0]).long().cumsum(1)
    assert (gen[(hit - (gen == eos[0]).long()) > 0] == 1).all() and bool((gen == eos[0]).any())


@pytest.mark.parametrize("processors", [False, True])
def test_top_k_1_and_tiny_top_p_are_greedy(dev, processors):
    eng, _ = _engine(dev, 2, 8, 33)
    inp, ids, am = _inputs(eng, 3, 33, "ids")
    proc = dict(PROC, eos_token_id=[7]) if processors else {}
    want = eng.generate(**inp, max_new_tokens=N, **proc)
    a = eng.generate(**inp, max_new_tokens=N, do_sample=True, top_k=1, temperature=1.7, seed=5, **proc)
    b = eng.generate(**inp, max_new_tokens=N, do_sample=True, top_p=1e-6, temperature=0.6, seed=6, **proc)
    assert torch.equal(a, want) and torch.equal(b, want)


def test_one_seed_one_output(dev):
    eng, _ = _engine(dev, 2, 8, 35)
    seed = 2 ** 63 + 12345
    inp11, ids11, _ = _inputs(eng, 11, 35, "embeds")
    emb = inp11["inputs_embeds"]
    kw = dict(max_new_tokens=N, do_sample=True, seed=seed, **SAMPLING, **PROC)
    inp = dict(inputs_embeds=emb[:8])
    ref = eng.generate(**inp, **kw)
    assert torch.equal(eng.generate(**inp, **kw), ref)                                  # replay of the captured graph
    assert torch.equal(eng.generate(**inp, **kw, use_graph=False), ref)
    assert torch.equal(eng.generate(**inp, **kw, sync_every=5), ref)
    assert torch.equal(eng.decode_finish(eng.prefill_begin(**inp, **kw)), ref)
    assert torch.equal(eng.generate(**inp, **kw, cache_set=1), ref)                     # another cache set ...
    staged = eng.prefill_begin(**inp, **kw, cache_set=2)                                # ... and a request adopted into set 0
    assert torch.equal(eng.decode_finish(eng.adopt(staged, 0)), ref)
    # 11 rows = groups of 8 and 3: the first 8 rows are the 8-row call, rows 8..10 draw with their absolute indices
    big = eng.generate(inputs_embeds=emb, **kw, return_dict_in_generate=True, return_logits=True)
    assert torch.equal(big.sequences[:8], ref)
    tail = type(big)(big.sequences[8:])
    tail.logits = big.logits[8:]
    assert _check_steps(tail, ids11[8:], "embeds", seed, row0=8, proc=PROC) == 3 * N
    alone = eng.generate(inputs_embeds=emb[8:], **kw)           # the same rows as rows 0..2 of their own call: other uniforms
    assert not torch.equal(alone, big.sequences[8:])
    # seeds
    assert not torch.equal(eng.generate(**inp, **dict(kw, seed=seed + 1)), ref)
    kw.pop("seed")
    torch.manual_seed(77)
    a = eng.generate(**inp, **kw)
    torch.manual_seed(77)
    b = eng.generate(**inp, **kw)
    c = eng.generate(**inp, **kw)
    assert torch.equal(a, b) and not torch.equal(b, c)


def test_greedy_and_beam_are_untouched_by_a_sampling_call(dev):
    eng, _ = _engine(dev, 2, 8, 21)
    fresh, _ = _engine(dev, 2, 8, 21)
    inp, ids, am = _inputs(eng, 2, 21, "ids")
    before = eng.generate(**inp, max_new_tokens=N)
    before_p = eng.generate(**inp, max_new_tokens=N, **PROC, eos_token_id=[7])
    before_b = eng.generate(**inp, max_new_tokens=N, num_beams=4)
    keys = set(eng._graphs)
    assert keys == {(2, False, False, 0), (2, False, False, 0, True), (2, False, False, 0, "beam", 4, 8)}
    graphs = {k: eng._graphs[k][1] for k in keys}
    assert eng.would_capture(2, False, False, 0, do_sample=True) and not eng.would_capture(2, False, False, 0)
    eng.generate(**inp, max_new_tokens=N, do_sample=True, seed=3, **SAMPLING)
    assert set(eng._graphs) - keys == {(2, False, False, 0, "sample")}
    assert not eng.would_capture(2, False, False, 0, do_sample=True)
    eng.generate(**inp, max_new_tokens=N, do_sample=True, seed=4, temperature=1.3, top_k=64, top_p=0.5)      # other values: same graph
    assert set(eng._graphs) - keys == {(2, False, False, 0, "sample")}
    eng.generate(**inp, max_new_tokens=N, do_sample=True, seed=3, **SAMPLING, **PROC, eos_token_id=[7])
    assert set(eng._graphs) - keys == {(2, False, False, 0, "sample"), (2, False, False, 0, True, "sample")}
    assert torch.equal(eng.generate(**inp, max_new_tokens=N), before)
    assert torch.equal(eng.generate(**inp, max_new_tokens=N, **PROC, eos_token_id=[7]), before_p)
    assert torch.equal(eng.generate(**inp, max_new_tokens=N, num_beams=4), before_b)
    assert torch.equal(fresh.generate(**inp, max_new_tokens=N), before)
    assert torch.equal(fresh.generate(**inp, max_new_tokens=N, **PROC, eos_token_id=[7]), before_p)
    assert torch.equal(fresh.generate(**inp, max_new_tokens=N, num_beams=4), before_b)
    assert all(eng._graphs[k][1] is graphs[k] for k in keys)        # the same captured graphs as before
    # do_sample=False ignores the warper arguments
    assert torch.equal(eng.generate(**inp, max_new_tokens=N, temperature=-1.0, top_k=0, top_p=3.0), before)


def test_sampling_requests_outside_the_implemented_ground_raise(dev):
    eng, _ = _engine(dev, 2, 4, 21)
    inp, ids, am = _inputs(eng, 1, 21, "ids")
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=2), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1),
               dict(top_k=2.5), dict(seed=1.5)):
        with pytest.raises(ValueError):
            eng.generate(**inp, max_new_tokens=4, do_sample=True, **kw)
    for kw in (dict(top_k=0), dict(top_k=65), dict(num_return_sequences=2)):
        with pytest.raises(NotImplementedError):
            eng.generate(**inp, max_new_tokens=4, do_sample=True, **kw)
    with pytest.raises(NotImplementedError, match="64"):
        eng.generate(**inp, max_new_tokens=4, do_sample=True, top_k=65)
    with pytest.raises(NotImplementedError, match="beam-search multinomial sampling"):       # as before this feature
        eng.generate(**inp, max_new_tokens=4, do_sample=True, num_beams=2)
    assert not eng._graphs or all("sample" not in k for k in eng._graphs)
    # the defaults: top_k = HF's 50, temperature 1, top_p 1
    out = eng.generate(**inp, max_new_tokens=4, do_sample=True, seed=1)
    assert out.shape == (1, S + 4)

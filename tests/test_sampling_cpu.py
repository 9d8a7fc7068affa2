"""CPU: the host statement of the sampling step (spider_amd.llm.sample_uniform_host / sample_token_host / resolve_sampling, which the
engine resolves its keywords with and the GPU tests check the kernels against).
  * the uniform: Philox4x32-10 against an independent implementation written here from the published constants, the Random123
    known-answer vector, and u strictly inside (0, 1);
  * the distribution: transformers' own `generate(do_sample=True)` on the tiny Llama of tests/test_logits_processors_cpu.py. HF draws
    with torch.multinomial from its global generator, so its TOKENS cannot be compared; its processed `scores` can: at every step
    `sample_token_host` on HF's RAW logits and the history so far must keep exactly the tokens whose score HF left finite, with the
    same renormalised probabilities. That pins the order processors -> temperature -> top-k -> top-p and the ids the penalty sees;
  * the validation errors, including the ValueErrors of HF's warper classes for the same values."""
import pytest
import torch

from spider_amd.llm import (SAMPLE_MAX_K, process_logits_host, resolve_logits_processors, resolve_sampling, resolve_seed,
                            sample_token_host, sample_uniform_host)
from test_logits_processors_cpu import B, N, S, V, _setup

M32 = 0xFFFFFFFF


def _philox4x32_10(ctr, key):
    """Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw 2011): ten rounds of two 32x32 -> 64 bit multiplications by
    0xD2511F53 / 0xCD9E8D57, the key bumped by the Weyl constants 0x9E3779B9 / 0xBB67AE85 before every round but the first."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for rnd in range(10):
        if rnd:
            k0 = (k0 + 0x9E3779B9) % 2 ** 32
            k1 = (k1 + 0xBB67AE85) % 2 ** 32
        hi0, lo0 = divmod(0xD2511F53 * c0, 2 ** 32)
        hi1, lo1 = divmod(0xCD9E8D57 * c2, 2 ** 32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def test_philox_known_answer_and_uniform():
    assert _philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert sample_uniform_host(0, 0, 0) == ((0x6627E8D5 >> 9) + 0.5) * 2.0 ** -23
    g = torch.Generator().manual_seed(5)
    seeds = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, 2 ** 64 - 1] + [int(x) for x in torch.randint(0, 2 ** 62, (6,), generator=g)]
    n = 0
    for seed in seeds:
        for row in (0, 1, 7, 8, 10, 63, 2 ** 31 - 1):
            for step in list(range(120)) + [4095, 2 ** 31 - 1]:
                u = sample_uniform_host(seed, row, step)
                x = _philox4x32_10((step, row, 0, 0), (seed & M32, seed >> 32))[0]
                assert u == ((x >> 9) + 0.5) * 2.0 ** -23
                assert 0.0 < u < 1.0 and float(torch.tensor(u, dtype=torch.float32)) == u       # exact in fp32
                n += 1
    assert n >= 10 ** 4
    # distinct (row, step) and distinct seeds give distinct streams
    assert len({sample_uniform_host(3, r, s) for r in range(8) for s in range(64)}) > 500
    assert sample_uniform_host(3, 0, 1) != sample_uniform_host(3, 1, 0) != sample_uniform_host(4, 1, 0)


def test_resolve_seed():
    torch.manual_seed(11)
    a = resolve_seed(None)
    torch.manual_seed(11)
    assert resolve_seed(None) == a and 0 <= a < 2 ** 63 and resolve_seed(None) != a
    assert resolve_seed(5) == 5 and resolve_seed(2 ** 64 - 1) == 2 ** 64 - 1 and resolve_seed(-1) == 2 ** 64 - 1
    with pytest.raises(ValueError):
        resolve_seed(1.5)


# the reference's own call first (conversation.py:151-173; top_k unset = HF's default), then the other paths of the definition
CASES = [
    dict(temperature=1.0, top_p=0.9, repetition_penalty=1.05, min_length=1),
    dict(temperature=0.7, top_p=0.9, repetition_penalty=1.05, min_length=1, top_k=50),
    dict(temperature=1.5, top_k=5, top_p=1.0),
    dict(temperature=0.7, top_k=20, top_p=0.3, repetition_penalty=1.3, min_new_tokens=6),
    dict(temperature=1.3, top_k=64, top_p=0.9, suppress_tokens=[5, 11, 96], min_length=S + 5),
    dict(temperature=2.0, top_k=1, top_p=0.9, repetition_penalty=1.3),
    dict(temperature=1.0, top_k=40, top_p=1e-6),
]


def _run_case(seed, case, padded, mode):
    """-> (steps checked, steps exempt for a tie at the top-k cut)"""
    m, ids, free = _setup(seed)
    kw = dict(CASES[case])
    am = None
    if padded:      # left padding as in tests/test_logits_processors_cpu.py: pad id 0 sits in input_ids and is penalised there
        ids = ids.clone()
        am = torch.ones(B, S, dtype=torch.long)
        for b, npad in ((1, 2), (2, 4)):
            ids[b, :npad] = 0
            am[b, :npad] = 0
    eos = sorted({int(free[0, 2]), int(free[1, 11])})
    if "suppress_tokens" in kw:
        kw["suppress_tokens"] = [t for t in kw["suppress_tokens"] if t not in eos]
    pad = 1
    args = dict(max_new_tokens=N, do_sample=True, eos_token_id=eos, pad_token_id=pad, output_logits=True, output_scores=True,
                return_dict_in_generate=True, **kw)
    if am is not None:
        args["attention_mask"] = am
    torch.manual_seed(1000 * seed + 10 * case + padded)
    if mode == "ids":
        out = m.generate(ids, **args)
        gen = out.sequences[:, S:]
    else:
        out = m.generate(inputs_embeds=m.get_input_embeddings()(ids), **args)
        gen = out.sequences
    T, k, top_p = resolve_sampling(True, kw["temperature"], kw.get("top_k"), kw["top_p"])
    if "top_k" not in kw:
        assert k == 50      # what transformers' generate resolves an unset top_k to
    pen, min_new, ban = resolve_logits_processors(S, eos, kw.get("repetition_penalty", 1.0), kw.get("min_length", 0),
                                                  kw.get("min_new_tokens", 0), kw.get("suppress_tokens"), None)
    seen = torch.zeros(B, V, dtype=torch.bool)
    if mode == "ids":
        seen.scatter_(1, ids, True)
    n_steps, n_tie = 0, 0
    for t in range(len(out.logits)):
        x = process_logits_host(out.logits[t].float(), seen, pen, ban, eos, t, min_new)
        for b in range(B):
            xs = torch.sort(x[b], descending=True, stable=True)[0]
            n_steps += 1
            if k < V and xs[k - 1] == xs[k]:        # the documented deviation: HF keeps every token tied with the k-th value
                n_tie += 1
                continue
            r = sample_token_host(x[b], T, k, top_p, 0.5)
            sc = out.scores[t][b].double()
            kept_hf = torch.isfinite(sc).nonzero().view(-1)
            kept = r["tokens"][:r["n_keep"]]
            assert sorted(kept.tolist()) == kept_hf.tolist(), (case, t, b)
            p_hf = torch.softmax(sc, -1)[kept]
            assert (p_hf - r["p"][:r["n_keep"]] / r["S"]).abs().max() < 1e-6, (case, t, b)
            assert r["token"] in kept.tolist() and r["n_keep"] <= k
        seen.scatter_(1, gen[:, t:t + 1], True)     # HF's penalty sees the row's sequence so far, pads after EOS included
    return n_steps, n_tie


@pytest.mark.parametrize("mode", ["ids", "embeds"])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_step_equals_hf_warped_scores(case, padded, mode):
    n_steps, n_tie = _run_case(0, case, padded, mode)
    assert n_steps >= B * 8
    assert n_tie == 0       # an fp32 model has no ties at the cut (they would be exempt, at most 1 step in 20)


def test_sample_token_host_definition():
    """the corners of the definition on hand-made rows"""
    x = torch.tensor([1.0, 3.0, 3.0, -float("inf"), 2.0, 3.0])
    r = sample_token_host(x, 1.0, 4, 1.0, 0.5)
    assert r["tokens"].tolist() == [1, 2, 5, 4] and r["n_keep"] == 4       # ties -> ascending id; exactly k
    assert sample_token_host(x, 1.0, 2, 1.0, 0.999)["tokens"].tolist() == [1, 2]       # the tie at the cut goes to the lower ids
    # the CDF: three equal masses and e^-1
    assert [sample_token_host(x, 1.0, 4, 1.0, u)["token"] for u in (0.01, 0.3, 0.6, 0.95)] == [1, 2, 5, 4]
    # nucleus: rank j kept iff the mass before it < top_p * P; one token always stays
    P = 3 + torch.exp(torch.tensor(-1.0)).item()
    assert sample_token_host(x, 1.0, 4, 2.5 / P, 0.5)["n_keep"] == 3 and sample_token_host(x, 1.0, 4, 2.0 / P - 1e-9, 0.5)["n_keep"] == 2
    assert sample_token_host(x, 1.0, 4, 1e-6, 0.999)["token"] == 1 and sample_token_host(x, 1.0, 1, 1.0, 0.999)["token"] == 1
    # -inf candidates carry no mass; a row that is all -inf yields the lowest id
    r = sample_token_host(x, 0.5, 6, 1.0, 0.9999999)
    assert r["tokens"].tolist() == [1, 2, 5, 4, 0, 3] and r["p"][5] == 0 and r["token"] != 3
    assert abs(float(r["p"][3]) - torch.exp(torch.tensor(-2.0, dtype=torch.float64)).item()) < 1e-12      # (2 - 3) / 0.5
    assert sample_token_host(torch.full((5,), -float("inf")), 1.0, 3, 0.9, 0.7)["token"] == 0
    assert sample_token_host(x, 1.0, 50, 1.0, 0.5)["tokens"].numel() == 6      # top_k beyond the vocabulary


def test_resolve_sampling():
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    assert resolve_sampling(False, temperature=-3, top_k=0, top_p=7) is None        # greedy ignores the warper arguments, as HF does
    assert resolve_sampling(True) == (1.0, 50, 1.0)
    assert resolve_sampling(True, 0.7, 20, 0.9) == (0.7, 20, 0.9)
    assert resolve_sampling(True, 1, 64, 1) == (1.0, 64, 1.0)                       # the reference's integer defaults
    for bad in (0.0, -1.0, 2, "1"):
        with pytest.raises(ValueError):
            TemperatureLogitsWarper(bad)
        with pytest.raises(ValueError):
            resolve_sampling(True, temperature=bad)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            TopPLogitsWarper(bad)
        with pytest.raises(ValueError):
            resolve_sampling(True, top_p=bad)
    with pytest.raises(ValueError):
        resolve_sampling(True, top_p=0.0)           # nothing would be kept but the forced token: not a nucleus
    for bad in (-3, 2.5):
        with pytest.raises(ValueError):
            TopKLogitsWarper(bad)
        with pytest.raises(ValueError):
            resolve_sampling(True, top_k=bad)
    for off in (0, SAMPLE_MAX_K + 1, 152064):       # 0 switches HF's filter off: a full-vocabulary nucleus
        with pytest.raises(NotImplementedError, match=str(SAMPLE_MAX_K)):
            resolve_sampling(True, top_k=off)
    with pytest.raises(NotImplementedError):
        resolve_sampling(True, num_return_sequences=2)

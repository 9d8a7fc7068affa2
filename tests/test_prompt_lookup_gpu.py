"""GPU: prompt-lookup decoding (prompt_lookup_num_tokens) -- the verify attention against the fp64 reference of tests/attn_checks.py
under the per-row visibility rule, the accept / draft kernels against the host restatements on every output buffer, and the engine
on the successor model of tests/prompt_lookup_cases.py (greedy output, counters, K / V rows) and on the reference-pinned d128
fixture of tests/test_llm_engine.py."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_checks as ac
import prompt_lookup_cases as pc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
T_MAX = 256
LENS = (1, 5, 200)      # keys row 0 sees: one, fewer than the splits, several strides of every wave


# ---------------------------------------------------------------------------------------------- attn_verify
@functools.lru_cache(maxsize=None)
def _verify_case(n_q, n_kv, R, B, beg, li):
    """q [B * R, n_q, d], caches [B, n_kv, T_MAX, d] with JUNK in every slot no row of the sequence may see, kv_beg / kv_end [B],
    and the fp64 reference [B * R, n_q * d] (computed once, shared by the nsplit values; nobody writes into it)"""
    d, seed = 128, 1000 * n_q + 100 * R + 10 * B + beg + li
    q = ac.rnd(B * R, n_q, d, seed=seed)
    k, v = ac.junk(B, n_kv, T_MAX, d, seed=seed + 1), ac.junk(B, n_kv, T_MAX, d, seed=seed + 2)
    kv_beg, kv_end, ref = [], [], []
    for b in range(B):
        length = LENS[(li + b) % len(LENS)]       # the sequences of a batch differ in length
        lo, hi = beg + b, beg + b + length        # ... and in their first slot
        k[b, :, lo:hi + R - 1] = ac.rnd(n_kv, length + R - 1, d, seed=seed + 3 + b)
        v[b, :, lo:hi + R - 1] = ac.rnd(n_kv, length + R - 1, d, seed=seed + 5 + b)
        j = torch.arange(T_MAX)[None]
        vis = (j >= lo) & (j < hi + torch.arange(R)[:, None])        # row r: kv_beg <= j < kv_end + r
        ref.append(ac.attn_ref64(q[b * R:(b + 1) * R], k[b].transpose(0, 1), v[b].transpose(0, 1), vis, 1.0 / math.sqrt(d)))
        kv_beg.append(lo)
        kv_end.append(hi)
    return q, k, v, torch.tensor(kv_beg, dtype=torch.int32), torch.tensor(kv_end, dtype=torch.int32), torch.cat(ref).reshape(B * R, n_q * d)


@pytest.mark.parametrize("R", [1, 2, 5, 8])
@pytest.mark.parametrize("n_q, n_kv", [(28, 4), (4, 2), (8, 1)])
def test_attn_verify_matches_fp64_reference(dev, n_q, n_kv, R):
    from spider_amd import ops
    atol, rtol = ac.TOL_DECODE
    worst = 0.0
    for B in (1, 2):
        for beg in (0, 3):
            for li in range(len(LENS)):
                q, k, v, kv_beg, kv_end, ref = _verify_case(n_q, n_kv, R, B, beg, li)
                qd, kd, vd, bd, ed = (t.to(dev) for t in (q, k, v, kv_beg, kv_end))
                for nsplit in (1, 8, 64):
                    got = ops.attn_verify(qd, kd, vd, ed, R, kv_beg=bd, nsplit=nsplit).float().cpu()
                    assert bool(torch.isfinite(got).all()), (B, beg, li, nsplit)
                    w = ac.err_over_tol(got, ref, atol + rtol * ref.abs())
                    worst = max(worst, w)
                    assert w <= 1.0, f"heads {n_q}/{n_kv} R={R} B={B} kv_beg={beg} lens[{li}] nsplit={nsplit}: err / tol = {w:.4g}"
                if beg == 0 and B == 1:     # kv_beg = None means slot 0
                    assert torch.equal(ops.attn_verify(qd, kd, vd, ed, R, nsplit=8), ops.attn_verify(qd, kd, vd, ed, R, kv_beg=bd, nsplit=8))
    print(f"MEASURED attn_verify heads {n_q}/{n_kv} R={R}: worst err / tol {worst:.4f}")


@pytest.mark.parametrize("nsplit", [1, 8])
def test_attn_verify_edge_moves_by_one_slot_per_row(dev, nsplit):
    """changing K / V at slot kv_end + r leaves the rows <= r bit-identical and changes row r + 1"""
    from spider_amd import ops
    n_q, n_kv, R, d, beg, length = 28, 4, 5, 128, 3, 5
    q = ac.rnd(R, n_q, d, seed=1).to(dev)
    k, v = ac.rnd(1, n_kv, T_MAX, d, seed=2).to(dev), ac.rnd(1, n_kv, T_MAX, d, seed=3).to(dev)
    kv_beg, kv_end = torch.tensor([beg], dtype=torch.int32, device=dev), torch.tensor([beg + length], dtype=torch.int32, device=dev)
    base = ops.attn_verify(q, k, v, kv_end, R, kv_beg=kv_beg, nsplit=nsplit).clone()
    for r in range(R):
        k2, v2 = k.clone(), v.clone()
        k2[0, :, beg + length + r] = ac.rnd(n_kv, d, seed=10 + r).to(dev)
        v2[0, :, beg + length + r] = ac.rnd(n_kv, d, seed=20 + r).to(dev)
        got = ops.attn_verify(q, k2, v2, kv_end, R, kv_beg=kv_beg, nsplit=nsplit)
        assert torch.equal(got[:r + 1], base[:r + 1]), f"row <= {r} reads slot kv_end + {r}"
        if r + 1 < R:
            assert not torch.equal(got[r + 1], base[r + 1]), f"row {r + 1} does not read slot kv_end + {r}"
    # the slot in front of kv_beg is nobody's
    k2 = k.clone()
    k2[0, :, beg - 1] = ac.JUNK
    assert torch.equal(ops.attn_verify(q, k2, v, kv_end, R, kv_beg=kv_beg, nsplit=nsplit), base)


def test_attn_verify_one_row_is_attn_decode_and_refuses_other_shapes(dev):
    from spider_amd import ops
    from spider_amd.lib import SpiderHipError
    q, k, v, kv_beg, kv_end, _ = _verify_case(28, 4, 1, 2, 3, 2)
    qd, kd, vd, bd, ed = (t.to(dev) for t in (q, k, v, kv_beg, kv_end))
    assert torch.equal(ops.attn_verify(qd, kd, vd, ed, 1, kv_beg=bd, nsplit=8), ops.attn_decode(qd, kd, vd, ed, kv_beg=bd, nsplit=8))
    with pytest.raises(ValueError, match="R has to be"):
        ops.attn_verify(qd, kd, vd, ed, 9, kv_beg=bd)
    with pytest.raises(SpiderHipError, match="head_dim"):
        ops.attn_verify(torch.zeros(2, 4, 64, dtype=BF, device=dev), torch.zeros(1, 2, 16, 64, dtype=BF, device=dev),
                        torch.zeros(1, 2, 16, 64, dtype=BF, device=dev), torch.ones(1, dtype=torch.int32, device=dev), 2)
    with pytest.raises(SpiderHipError, match="group size"):
        ops.attn_verify(torch.zeros(2, 18, 128, dtype=BF, device=dev), torch.zeros(1, 2, 16, 128, dtype=BF, device=dev),
                        torch.zeros(1, 2, 16, 128, dtype=BF, device=dev), torch.ones(1, dtype=torch.int32, device=dev), 2)


# ---------------------------------------------------------------------------------------------- accept / draft kernels
def _run_spec_case(case, dev, via_torch_op=False):
    from spider_amd import ops
    names = ("prompt_ids", "n_prompt", "hist", "n_hist", "ids", "pos", "slot", "lm_out", "kv_end", "n_draft", "counters", "ngram", "k_draft")
    t = {k: getattr(case, k).clone().to(dev) for k in names}
    guard = {k: v.clone() for k, v in t.items() if k in ("prompt_ids", "n_prompt", "lm_out", "ngram", "k_draft")}
    sp = {k: t[k] for k in names if k not in ("hist", "n_hist")}
    if via_torch_op:
        import spider_amd.torch_ops  # noqa: F401
        if case.advance:
            torch.ops.spider_hip.spec_advance_draft_(t["lm_out"], t["ids"], t["pos"], t["slot"], t["kv_end"], t["n_draft"], t["hist"],
                                                     t["n_hist"], t["prompt_ids"], t["n_prompt"], t["ngram"], t["k_draft"], t["counters"])
        else:
            torch.ops.spider_hip.prompt_lookup_draft_(t["prompt_ids"], t["n_prompt"], t["hist"], t["n_hist"], t["ngram"], t["k_draft"],
                                                      t["ids"], t["pos"], t["slot"], t["n_draft"])
    elif case.advance:
        ops.spec_advance_draft(sp, t["hist"], t["n_hist"])
    else:
        ops.prompt_lookup_draft(sp, t["hist"], t["n_hist"])
    want = case.expected()
    for k in case.OUTPUTS:
        assert torch.equal(t[k].cpu(), want[k]), (case.name, k, t[k].cpu().tolist(), want[k].tolist())
    for k, v in guard.items():      # inputs stay as they were
        assert torch.equal(t[k], v), (case.name, k)


@pytest.mark.parametrize("K", [1, 3, 7])
def test_spec_kernels_equal_host_restatements_random(dev, K):
    cases = pc.random_spec_cases(K)
    assert sum(int(c.expected()["n_draft"].sum()) > 0 for c in cases) >= 10
    for case in cases:
        _run_spec_case(case, dev)


@pytest.mark.parametrize("case", pc.named_spec_cases(), ids=repr)
def test_spec_kernels_equal_host_restatements_named(dev, case):
    _run_spec_case(case, dev)
    _run_spec_case(case, dev, via_torch_op=True)


def test_spec_kernels_long_sequence_more_than_one_stride(dev):
    """a sequence longer than the block (1024 threads): the only match sits behind the first stride"""
    hist = list(range(100, 100 + 1500)) + [7, 8, 9, 10] + list(range(2000, 2600)) + [7, 8]
    case = pc.SpecCase("long", [[1, 2, 3]], [hist], 3, 2, cap=4096, advance=False)
    assert case.expected()["ids"].tolist() == [8, 9, 10, 2000]
    _run_spec_case(case, dev)


# ---------------------------------------------------------------------------------------------- engine, successor model
def _successor_engine(dev, **kw):
    from spider_amd.llm import LlamaEngine, LLMConfig
    cfg, w = pc.successor_model()
    return LlamaEngine(LLMConfig(**cfg.__dict__), w, dev, max_len=128, **kw)


def _counts(rec):
    return {k: rec[k] for k in ("steps", "drafted", "accepted")}


@pytest.mark.parametrize("max_batch", [1, 8], ids=["row-major", "fragment-major"])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_engine_successor_model(dev, K, max_batch):
    eng = _successor_engine(dev, max_batch=max_batch)
    assert eng.fm_batch == (max_batch == 8)
    ids = torch.tensor([pc.PROMPT])
    S, T = ids.shape[1], pc.T_NEW
    plain = eng.generate(input_ids=ids, max_new_tokens=T + K)        # K more: what the model says behind the last drafts
    k_plain = [t[:, 0, :, :S + T - 1].clone() for t in eng._kv(0)]
    assert eng.last_prompt_lookup is None
    sim_tok, sim = pc.simulate_tokens(pc.PROMPT, plain[0, S:].tolist(), T, K, 2)
    if K == 3:
        assert {k: sim[k] for k in pc.K3N2} == pc.K3N2, sim
    assert eng.would_capture(1, prompt_lookup_num_tokens=K) and not eng.would_capture(1)
    out = eng.generate(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=K, return_dict_in_generate=True)
    assert not eng.would_capture(1, prompt_lookup_num_tokens=K)
    assert torch.equal(out.sequences, plain[:, :S + T]), (out.sequences[0, S:].tolist(), plain[0, S:S + T].tolist())
    assert out.sequences[0, S:].tolist() == sim_tok
    assert out.prompt_lookup == _counts(sim) == eng.last_prompt_lookup, (out.prompt_lookup, sim)
    assert out.prompt_lookup["accepted"] > 0        # without the feature the keyword is ignored and nothing is ever drafted
    # the K / V rows of every token that was fed, accepted drafts included, are the plain run's inside the bf16 bound of step logits
    for name, a, b in zip("kv", eng._kv(0), k_plain):
        for l in range(eng.cfg.layers):
            got, ref = a[l, 0, :, :S + T - 1].float(), b[l].float()
            rel = float((got - ref).norm() / ref.norm())
            assert rel < 2.5e-2, (name, l, rel)
    # the same tokens and counters without the graph, with fewer host checks, with max_matching_ngram_size spelled out
    eager = eng.generate(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=K, use_graph=False, max_matching_ngram_size=2)
    assert torch.equal(eager, out.sequences) and eng.last_prompt_lookup == out.prompt_lookup
    every4 = eng.generate(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=K, sync_every=4)
    assert torch.equal(every4, out.sequences) and eng.last_prompt_lookup["steps"] >= out.prompt_lookup["steps"]
    # the split path, and a handle adopted into another cache set
    hd = eng.prefill_begin(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=K)
    assert torch.equal(eng.decode_finish(hd), out.sequences) and eng.last_prompt_lookup == out.prompt_lookup
    hd = eng.adopt(eng.prefill_begin(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=K, cache_set=1), 0)
    assert torch.equal(eng.decode_finish(hd), out.sequences) and eng.last_prompt_lookup == out.prompt_lookup
    # an EOS that arrives inside an accepted draft ends the row there, as on the plain path
    eos = pc.C[5]
    want = eng.generate(input_ids=ids, max_new_tokens=T, eos_token_id=eos)
    for se in (1, 4):
        got = eng.generate(input_ids=ids, max_new_tokens=T, eos_token_id=eos, prompt_lookup_num_tokens=K, sync_every=se)
        assert torch.equal(got, want) and int(got[0, -1]) == eos and got.shape[1] < S + T
    # a stopping criterion is checked at every length, not only where a step ended
    from spider_amd.llm import StoppingCriteriaSub
    sc = [StoppingCriteriaSub([[pc.C[4], pc.C[5]]])]
    want = eng.generate(input_ids=ids, max_new_tokens=T, stopping_criteria=sc)
    got = eng.generate(input_ids=ids, max_new_tokens=T, stopping_criteria=sc, prompt_lookup_num_tokens=K, sync_every=2)
    assert torch.equal(got, want) and got.shape[1] < S + T
    # inputs_embeds only: the lookup runs over the generated tokens alone
    emb = eng.embed_tokens(ids)
    want = eng.generate(inputs_embeds=emb, max_new_tokens=T + K)
    got = eng.generate(inputs_embeds=emb, max_new_tokens=T, prompt_lookup_num_tokens=K, return_dict_in_generate=True)
    assert torch.equal(got.sequences, want[:, :T])
    assert got.prompt_lookup == _counts(pc.simulate_tokens([], want[0].tolist(), T, K, 2)[1]) and got.prompt_lookup["accepted"] > 0
    # N is a value the one graph reads
    got = eng.generate(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=K, max_matching_ngram_size=1, return_dict_in_generate=True)
    assert torch.equal(got.sequences, out.sequences)
    assert got.prompt_lookup == _counts(pc.simulate_tokens(pc.PROMPT, plain[0, S:].tolist(), T, K, 1)[1])
    # off is off, and a plain call leaves no record behind
    assert eng.last_prompt_lookup is not None
    assert torch.equal(eng.generate(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=0), plain[:, :S + T])
    assert eng.last_prompt_lookup is None


@pytest.mark.parametrize("K, sync_every, T", [(7, 8, 40), (3, 4, 113), (7, 3, 41)])
def test_engine_steps_between_host_checks_stay_inside_the_cache(dev, K, sync_every, T):
    """max_len == S + max_new_tokens + K, the tightest cache resolve_prompt_lookup admits, with sync_every > 1 on the model that
    accepts every draft: a step advances by up to K + 1 slots, so the steps replayed before the host reads n_hist have to be
    bounded by the cache as well as by the tokens still wanted. A K / V row appended past slot max_len - 1 of the last kv head
    lands in batch row 1 of the layer's cache (one of a lower head in the next head's first slots, which the sequence reads)."""
    from spider_amd.llm import LlamaEngine, LLMConfig
    cfg, w = pc.successor_model()
    S = len(pc.PROMPT)
    eng = LlamaEngine(LLMConfig(**cfg.__dict__), w, dev, max_batch=2, max_len=S + T + K)
    ids = torch.tensor([pc.PROMPT])
    want = eng.generate(input_ids=ids, max_new_tokens=T)
    kv_plain = [t[:, 0, :, :S + T - 1].clone() for t in eng._kv(0)]
    SENT = 777.0
    for t in eng._kv(0):
        t[:, 1].fill_(SENT)
    out = eng.generate(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=K, sync_every=sync_every, return_dict_in_generate=True)
    assert torch.equal(out.sequences, want)
    rec = out.prompt_lookup
    assert rec["accepted"] > rec["steps"], rec       # most steps accept several drafts: the cursors do move by more than one
    for name, t, ref in zip("kv", eng._kv(0), kv_plain):
        assert bool((t[:, 1] == SENT).all()), f"{name} cache: rows of the neighbouring batch row were written"
        for l in range(cfg.layers):
            got, r = t[l, 0, :, :S + T - 1].float(), ref[l].float()
            assert float((got - r).norm() / r.norm()) < 2.5e-2, (name, l)
    with pytest.raises(ValueError, match="max_len"):
        eng.generate(input_ids=ids, max_new_tokens=T + 1, prompt_lookup_num_tokens=K, sync_every=sync_every)


@pytest.mark.parametrize("weight_dtype", ["fp8", "mxfp4"])
def test_engine_successor_model_quantised_streams(dev, weight_dtype):
    K = 3
    eng = _successor_engine(dev, max_batch=1, weight_dtype=weight_dtype)
    ids = torch.tensor([pc.PROMPT])
    S, T = ids.shape[1], pc.T_NEW
    plain = eng.generate(input_ids=ids, max_new_tokens=T + K)
    out = eng.generate(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=K, return_dict_in_generate=True)
    assert torch.equal(out.sequences, plain[:, :S + T])
    assert out.prompt_lookup == _counts(pc.simulate_tokens(pc.PROMPT, plain[0, S:].tolist(), T, K, 2)[1])
    assert out.prompt_lookup["accepted"] > 0
    assert torch.equal(eng.generate(input_ids=ids, max_new_tokens=T, prompt_lookup_num_tokens=K, use_graph=False), out.sequences)


def test_engine_refuses_what_the_verify_step_does_not_serve(dev):
    eng = _successor_engine(dev, max_batch=2)
    ids = torch.tensor([pc.PROMPT])
    for kw, exc, word in ((dict(prompt_lookup_num_tokens=8), ValueError, "prompt_lookup_num_tokens"),
                          (dict(max_matching_ngram_size=9), ValueError, "max_matching_ngram_size"),
                          (dict(do_sample=True), NotImplementedError, "do_sample"),
                          (dict(num_beams=2), NotImplementedError, "num_beams"),
                          (dict(repetition_penalty=1.3), NotImplementedError, "repetition_penalty"),
                          (dict(no_repeat_ngram_size=2), NotImplementedError, "no_repeat_ngram_size"),
                          (dict(output_hidden_states=True), NotImplementedError, "output_hidden_states"),
                          (dict(return_logits=True), NotImplementedError, "return_logits"),
                          (dict(max_new_tokens=114), ValueError, "max_len")):       # 12 + 114 + 3 = 129 > 128
        with pytest.raises(exc, match=word):
            eng.generate(input_ids=ids, **dict(dict(max_new_tokens=8, prompt_lookup_num_tokens=3), **kw))
    with pytest.raises(NotImplementedError, match="batch"):
        eng.generate(input_ids=torch.tensor([pc.PROMPT, pc.PROMPT]), max_new_tokens=8, prompt_lookup_num_tokens=3)
    assert eng.generate(input_ids=ids, max_new_tokens=113, prompt_lookup_num_tokens=3).shape[1] == 12 + 113


# ---------------------------------------------------------------------------------------------- engine, reference-pinned model
def test_engine_reference_pinned_fixture(dev, golden_dir):
    """The d128 fixture of tests/test_llm_engine.py (tokens of the reference's own LlamaForCausalLM, margins >= 0.1): real attention
    dependence and mostly rejected drafts. K = 3 reproduces the fixture's tokens under the rule of
    test_batched_fold_path_tokens_match_single_row_path: a first divergence only where the oracle margin is < 0.1."""
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd.llm import LlamaEngine, LLMConfig
    z = np.load(os.path.join(golden_dir, "llama_ref_d128_0.npz"))
    ocfg = LlamaCfg(**json.loads(str(z["cfg"])))
    w = LlamaOracle.random_weights(ocfg, seed=int(z["seed"]), std=float(z["std"]))
    wsum = sum(float(v.double().abs().sum()) for v in w.values())
    assert abs(wsum - float(z["wsum"])) <= 1e-9 * float(z["wsum"]), "random_weights no longer reproduces the fixture's weights"
    ids, ref_tok, margins = torch.from_numpy(z["ids"]), torch.from_numpy(z["tokens"]), torch.from_numpy(z["margins"])
    S, T = ids.shape[1], ref_tok.shape[1]
    eng = LlamaEngine(LLMConfig(**ocfg.__dict__), w, dev, max_batch=1, max_len=64)
    drafted = accepted = 0
    for b in range(ids.shape[0]):
        for N in (2, 1):        # (transformers' default; single tokens repeat more often, so N = 1 drafts more)
            out = eng.generate(input_ids=ids[b:b + 1], max_new_tokens=T, prompt_lookup_num_tokens=3, max_matching_ngram_size=N,
                               return_dict_in_generate=True)
            gen = out.sequences[0, S:].cpu()
            assert gen.numel() == T
            for t in range(T):
                if int(gen[t]) != int(ref_tok[b, t]):
                    assert float(margins[b, t]) < 0.1, f"row {b} N={N} step {t}: diverges from the reference at a healthy margin"
                    break
            rec = out.prompt_lookup
            assert rec["steps"] + rec["accepted"] >= T - 1 and rec["accepted"] <= rec["drafted"]
            drafted, accepted = drafted + rec["drafted"], accepted + rec["accepted"]
    print(f"MEASURED prompt lookup on the d128 fixture: {drafted} tokens drafted, {accepted} accepted")
    assert drafted > 0, "the fixture's sequences have to exercise the verify step with drafts"


# ---------------------------------------------------------------------------------------------- thinker / SpiderFreeInfer pass-through
def _successor_thinker(dev):
    import dataclasses
    from spider_amd.llm import LlamaEngine, LLMConfig
    from spider_amd.qwen_omni import OmniTokenIds, QwenOmniThinker
    cfg, w = pc.successor_model()
    # text tokens carry three equal rotary components, for which the multimodal RoPE is the plain one
    lcfg = dataclasses.replace(LLMConfig(**cfg.__dict__), mrope_section=(16, 24, 24))
    tok = OmniTokenIds(image=290, video=291, audio=292, vision_start=293, audio_start=294)
    return QwenOmniThinker(LlamaEngine(lcfg, w, dev, max_batch=1, max_len=128), None, None, tok)


def test_thinker_and_spider_free_infer_pass_the_keywords_through(dev):
    from benchkit.synthetic import SyntheticOmniProcessor
    from spider_amd import SpiderFreeInfer
    th = _successor_thinker(dev)
    ids = torch.tensor([pc.PROMPT])
    S, T = ids.shape[1], pc.T_NEW
    plain = th.generate(ids, None, max_new_tokens=T + 3, eos_token_id=[])
    # (sync_every=1: the thinker's default of 8 lets steps run past the last token, and the counters count them)
    out = th.generate(ids, None, max_new_tokens=T, eos_token_id=[], prompt_lookup_num_tokens=3, return_dict_in_generate=True, sync_every=1)
    assert torch.equal(out.sequences, plain[:, :S + T])
    rec = out.prompt_lookup
    assert rec and rec["steps"] > 0 and rec["accepted"] > 0 and rec == th.llm.last_prompt_lookup
    # the thinker hands inputs_embeds over: the lookup sees the generated tokens alone
    assert rec == _counts(pc.simulate_tokens([], plain[0, S:].tolist(), T, 3, 2)[1])
    assert not th.would_capture(ids, prompt_lookup_num_tokens=3) and th.would_capture(ids, prompt_lookup_num_tokens=5)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        th.generate(ids, None, max_new_tokens=T, prompt_lookup_num_tokens=3, max_matching_ngram_size=0)
    lazy = th.generate(ids, None, max_new_tokens=T, eos_token_id=[], prompt_lookup_num_tokens=3, return_dict_in_generate=True)
    assert torch.equal(lazy.sequences, out.sequences) and lazy.prompt_lookup["steps"] >= rec["steps"]
    gk = dict(max_new_tokens=T, eos_token_id=[], spk="Chelsie", use_audio_in_video=True, sync_every=1)
    inputs = {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
    mk = lambda **kw: SpiderFreeInfer(th, SyntheticOmniProcessor(vocab=300), False, device=dev, mode="spider_story_free_qwen",
                                      generate_kwargs=dict(gk, **kw))
    off, on = mk(), mk(prompt_lookup_num_tokens=3, max_matching_ngram_size=2)
    want = off.llm_pass(inputs)[0]
    th.llm.last_prompt_lookup = None
    assert torch.equal(on.llm_pass(inputs)[0], want) and th.llm.last_prompt_lookup == rec
    th.llm.last_prompt_lookup = None
    handle, images = on.prefill_pass(inputs, 1)         # depth 3: prompt pass into the staging set, adopted into set 0, decoded there
    assert torch.equal(on.decode_pass(*on._adopt((handle, images)))[0], want) and th.llm.last_prompt_lookup == rec

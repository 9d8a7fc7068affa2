"""GPU: LlamaEngine.score (teacher-forced log-probabilities, loss, KL between engines) against the fp32 CPU oracle, against its own
definition `score_host`, against the decode path, on quantised engines and through the thinker.

Model: the d128 recipe of tests/test_llm_engine.py::test_engine_matches_oracle_d128 (seed 0), B = 2, S = 21, row 1 left-padded by 5.
Bounds:
  (a) prompt logits against LlamaOracle.forward at every real (attention_mask == 1) row inside that test's bounds: rel-L2 < 2.5e-2,
      max abs < 5 % of the logit range. (Pad rows are not compared: the oracle lets a row that masks everything see itself, the
      engine's attention gives such a row zeros.)
  (b) per scored position |token_logprobs - oracle fp64 logprob| <= 2 max_j |x_engine - x_oracle| + kernel tolerance: lse and x_t are
      1-Lipschitz in the sup norm, so this is a theorem about shift, gather, mask and chunking (it holds at the first real token
      of the padded row too, whose logits row is a pad row).
  (c) token_logprobs, argmax, entropy, loss against score_host on the engine's own bf16 logits within the kernel tolerance of
      logprob_checks.py.
Quantised engines: on the CPU oracle with dequantised layer weights, same ids, mean KL against the original weights is 0.0134 (fp8)
and 0.185 (mxfp4), with the head quantised too 0.0142 and 0.196: a factor 13.8, so mean_kl(mxfp4) > mean_kl(fp8) is asserted."""
import json
import os

import numpy as np
import pytest
import torch

import logprob_checks as lc

pytestmark = pytest.mark.gpu
B, S, PAD = 2, 21, 5


def _ocfg():
    from oracle.llama import LlamaCfg
    return LlamaCfg(256, 3, 4, 2, 128, 512, 331, 500000.0,
                    dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=64),
                    1e-5, False, 512)


def _engine(dev, w, **kw):
    from spider_amd.llm import LlamaEngine, LLMConfig
    return LlamaEngine(LLMConfig(**_ocfg().__dict__), w, dev, max_batch=2, max_len=128, **kw)


@pytest.fixture(scope="module")
def ctx(dev):
    from oracle.llama import LlamaOracle
    ocfg = _ocfg()
    w = LlamaOracle.random_weights(ocfg, seed=0, std=0.08)
    ids = torch.randint(3, ocfg.vocab, (B, S), generator=torch.Generator().manual_seed(0))
    am = torch.ones_like(ids)
    am[1, :PAD] = 0
    ids[1, :PAD] = 0
    pos = (am.cumsum(-1) - 1).clamp(min=0)
    oracle = LlamaOracle(ocfg, w)
    with torch.no_grad():
        ref = oracle.forward(ids, pos, None, am)[0]
    eng = _engine(dev, w)
    out = eng.score(input_ids=ids, attention_mask=am, return_logits=True)
    return dict(w=w, ids=ids, am=am, oracle=oracle, ref=ref, eng=eng, out=out)


def _aligned_tolerances(logits, tg, logits_ref=None):
    """kernel tolerances of logprob_checks for logits [B, S, V] (bf16, CPU) -> label-aligned [B, S] (row t - 1 -> index t)"""
    from spider_amd.llm import IGNORE_INDEX
    Bq, Sq, V = logits.shape
    nxt = torch.full_like(tg, IGNORE_INDEX)
    nxt[:, :-1] = tg[:, 1:]
    r = lc.reference(logits.reshape(Bq * Sq, V), nxt.reshape(-1), None if logits_ref is None else logits_ref.reshape(Bq * Sq, V))
    out = {}
    for k in ("tol_logprob", "tol_entropy") + (("tol_kl",) if logits_ref is not None else ()):
        t = torch.zeros(Bq, Sq, dtype=torch.float64)
        t[:, 1:] = r[k].view(Bq, Sq)[:, :-1]
        out[k] = t
    return out


def _check_against_host(out, labels, am, what, other_logits=None):
    """(c): every field of the engine's ScoreOutput against score_host on the engine's own logits"""
    from spider_amd.llm import score_host, score_targets
    lg = out.logits.cpu()
    host = score_host(lg, labels, am, logits_ref=other_logits)
    tol = _aligned_tolerances(lg, score_targets(labels, am), other_logits)
    m = host.mask
    assert torch.equal(out.mask.cpu(), m) and out.n_tokens == host.n_tokens == int(m.sum())
    assert torch.equal(out.argmax.cpu(), host.argmax)
    e_lp = (out.token_logprobs.double().cpu() - host.token_logprobs).abs()
    e_en = (out.entropy.double().cpu() - host.entropy).abs()
    print(f"MEASURED score vs score_host {what}: logprob err {float(e_lp.max()):.3g} (tol {float(tol['tol_logprob'][m].min()):.3g}+), "
          f"entropy err {float(e_en.max()):.3g} (tol {float(tol['tol_entropy'][m].min()):.3g}+), loss {out.loss:.6f} vs {host.loss:.6f}")
    assert bool((e_lp <= tol["tol_logprob"])[m].all()) and float(e_lp[~m].max()) == 0.0
    assert bool((e_en <= tol["tol_entropy"])[m].all()) and float(e_en[~m].max()) == 0.0
    assert abs(out.loss - host.loss) <= float(tol["tol_logprob"][m].mean()) + 1e-6 * abs(host.loss)
    assert abs(out.perplexity - float(np.exp(out.loss))) <= 1e-9 * out.perplexity
    if other_logits is not None:
        e_kl = (out.kl.double().cpu() - host.kl).abs()
        print(f"MEASURED score vs score_host {what}: kl err {float(e_kl.max()):.3g}, mean_kl {out.mean_kl:.6f} vs {host.mean_kl:.6f}, "
              f"top1_agree {out.top1_agree:.4f}")
        assert bool((e_kl <= tol["tol_kl"])[m].all()) and bool((out.kl.double().cpu() >= -tol["tol_kl"]).all())
        assert abs(out.mean_kl - host.mean_kl) <= float(tol["tol_kl"][m].mean()) + 1e-6 * abs(host.mean_kl)
        assert abs(out.top1_agree - host.top1_agree) <= 1e-12
    return host


def test_prompt_logits_match_the_oracle_at_every_real_position(ctx):
    got, ref, real = ctx["out"].logits.float().cpu(), ctx["ref"], ctx["am"].bool()
    assert got.shape == (B, S, 331) and ctx["out"].logits.dtype == torch.bfloat16
    g, r = got[real], ref[real]
    rel, mx = float((g - r).norm() / r.norm()), float((g - r).abs().max())
    print(f"MEASURED score prompt logits vs oracle: rel-L2 {rel:.5f}, max abs {mx:.4f} of range {float(r.abs().max()):.3f}")
    assert rel < 2.5e-2 and mx < 0.05 * float(r.abs().max())
    assert bool(torch.isfinite(got).all()), "pad rows must stay finite: the row kernel takes finite logits"


def test_token_logprobs_within_the_lipschitz_bound_of_the_oracle(ctx):
    from spider_amd.llm import score_host, score_targets
    out, ids, am = ctx["out"], ctx["ids"], ctx["am"]
    want = score_host(ctx["ref"], ids, am)
    tol = _aligned_tolerances(out.logits.cpu(), score_targets(ids, am))["tol_logprob"]
    sup = torch.zeros(B, S, dtype=torch.float64)
    sup[:, 1:] = (out.logits.double().cpu() - ctx["ref"].double()).abs().amax(-1)[:, :-1]
    err = (out.token_logprobs.double().cpu() - want.token_logprobs).abs()
    m = want.mask
    assert torch.equal(out.mask.cpu(), m) and int(m.sum()) == (S - 1) + (S - PAD)
    print(f"MEASURED score token_logprobs vs oracle: worst err / (2 sup + tol) {float((err / (2 * sup + tol).clamp(min=1e-30))[m].max()):.3f}, "
          f"loss {out.loss:.5f} vs {want.loss:.5f}")
    assert bool((err <= 2 * sup + tol)[m].all())


def test_fields_equal_score_host_on_the_engines_own_logits(ctx):
    _check_against_host(ctx["out"], ctx["ids"], ctx["am"], "V=331")
    # labels with ignored positions, passed explicitly
    labels = ctx["ids"].clone()
    labels[0, 4:9] = -100
    out = ctx["eng"].score(input_ids=ctx["ids"], attention_mask=ctx["am"], labels=labels, return_logits=True)
    assert out.n_tokens == ctx["out"].n_tokens - 5 and torch.equal(out.logits, ctx["out"].logits)
    _check_against_host(out, labels, ctx["am"], "V=331, -100 labels")


def test_resized_vocabulary(ctx, dev):
    """336 rows: a multiple of 8, the head itself is the GEMM operand; 331 runs on the zero-padded copy of the same width, so the
    shared columns are the same bits"""
    eng = _engine(dev, ctx["w"])
    eng.resize_token_embeddings(336, seed=1)
    ids = ctx["ids"].clone()
    ids[0, 3], ids[1, 9] = 335, 333
    out = eng.score(input_ids=ids, attention_mask=ctx["am"], return_logits=True)
    assert out.logits.shape == (B, S, 336)
    _check_against_host(out, ids, ctx["am"], "V=336")
    same = eng.score(input_ids=ctx["ids"], attention_mask=ctx["am"], return_logits=True)
    assert torch.equal(same.logits[..., :331], ctx["out"].logits)
    with pytest.raises(ValueError, match="other"):
        ctx["eng"].score(input_ids=ctx["ids"], other=eng)


def test_chunks_self_reference_and_side_effects(ctx):
    eng, ids, am, out = ctx["eng"], ctx["ids"], ctx["am"], ctx["out"]
    before = eng.generate(input_ids=ids, attention_mask=am, max_new_tokens=6)
    graphs = {k: (id(v[0]), id(v[1])) for k, v in eng._graphs.items()}
    try:
        eng.SCORE_CHUNK_ROWS = 8                    # 42 rows: five chunks of 8 and a tail of 2
        small = eng.score(input_ids=ids, attention_mask=am, return_logits=True)
    finally:
        eng.SCORE_CHUNK_ROWS = None
    for k in ("token_logprobs", "argmax", "entropy", "mask", "logits"):
        assert torch.equal(getattr(small, k), getattr(out, k)), k
    assert small.loss == out.loss and small.n_tokens == out.n_tokens
    me = eng.score(input_ids=ids, attention_mask=am, other=eng)
    assert float(me.kl.abs().max()) == 0.0 and me.mean_kl == 0.0 and me.top1_agree == 1.0
    assert torch.equal(me.token_logprobs, out.token_logprobs)
    assert {k: (id(v[0]), id(v[1])) for k, v in eng._graphs.items()} == graphs, "score must not touch the decode states / graphs"
    assert torch.equal(eng.generate(input_ids=ids, attention_mask=am, max_new_tokens=6), before)
    # inputs_embeds need labels; with them the result is the input_ids one
    emb = eng.embed_tokens(ids)
    with pytest.raises(ValueError, match="labels"):
        eng.score(inputs_embeds=emb, attention_mask=am)
    via = eng.score(inputs_embeds=emb, attention_mask=am, labels=ids)
    assert torch.equal(via.token_logprobs, out.token_logprobs) and via.loss == out.loss


@pytest.mark.parametrize("k", [0, 1, 2])
def test_reference_pinned_fixture_first_token(dev, golden_dir, k):
    """tests/golden/llama_ref_d128_{k}.npz (the reference's own LlamaForCausalLM): scoring prompt ++ first generated token, the
    prediction behind the last prompt position is that token"""
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd.llm import LlamaEngine, LLMConfig
    z = np.load(os.path.join(golden_dir, f"llama_ref_d128_{k}.npz"))
    ocfg = LlamaCfg(**json.loads(str(z["cfg"])))
    w = LlamaOracle.random_weights(ocfg, seed=int(z["seed"]), std=float(z["std"]))
    eng = LlamaEngine(LLMConfig(**ocfg.__dict__), w, dev, max_batch=2, max_len=64)
    ids, first = torch.from_numpy(z["ids"]), torch.from_numpy(z["tokens"])[:, :1]
    Sp = ids.shape[1]
    out = eng.score(input_ids=torch.cat([ids, first.to(ids.dtype)], 1))
    assert torch.equal(out.argmax[:, Sp].cpu(), first[:, 0].to(torch.int64))
    ref0 = torch.log_softmax(torch.from_numpy(z["step_logits"])[:, 0].double(), -1).gather(-1, first.to(torch.int64))[:, 0]
    err = (out.token_logprobs[:, Sp].double().cpu() - ref0).abs()
    print(f"MEASURED score d128 fixture {k}: first-token logprob {out.token_logprobs[:, Sp].tolist()} vs reference {ref0.tolist()}")
    assert float(err.max()) <= 2 * 0.05 * float(torch.from_numpy(z["step_logits"])[:, 0].abs().max())


def test_decode_consistency(ctx):
    """score(prompt ++ generated) against generate(..., return_logits=True): the prompt route (MFMA GEMMs over all rows) and the
    decode route (weight streams, one row per step) are each held to 5 % of the logit range per logit against the oracle
    (test_engine_matches_oracle_d128), and a log-probability moves by at most twice the sup distance of its logits row"""
    eng, oracle, ids = ctx["eng"], ctx["oracle"], ctx["ids"].clone()
    ids[1, :PAD] = torch.randint(3, 331, (PAD,), generator=torch.Generator().manual_seed(5))       # no padding here
    T = 16
    gen = eng.generate(input_ids=ids, max_new_tokens=T, return_dict_in_generate=True, return_logits=True)
    seq = gen.sequences.cpu()
    out = eng.score(input_ids=seq)
    with torch.no_grad():
        ref = oracle.forward(seq, torch.arange(S + T)[None].expand(B, -1), None, None)[0]
    steps = torch.log_softmax(gen.logits.float().cpu().double(), -1)                              # [B, T, V]
    want = steps.gather(-1, seq[:, S:, None])[..., 0]
    got = out.token_logprobs[:, S:].double().cpu()
    bound = 2 * 0.05 * float(ref[:, S - 1:-1].abs().max())
    print(f"MEASURED score vs decode steps: max |logprob difference| {float((got - want).abs().max()):.4f}, bound {bound:.4f}")
    assert float((got - want).abs().max()) <= bound
    top2 = ref[:, S - 1:-1].topk(2, -1).values
    wide = (top2[..., 0] - top2[..., 1]) >= 0.1
    assert int(wide.sum()) > 0 and torch.equal(out.argmax[:, S:].cpu()[wide], seq[:, S:][wide])


@pytest.mark.parametrize("head", [False, True])
def test_quantised_engines_against_the_bf16_engine(ctx, dev, head):
    eng, ids, am = ctx["eng"], ctx["ids"], ctx["am"]
    base_logits = ctx["out"].logits.cpu()
    kls = {}
    for fmt in ("fp8", "mxfp4"):
        q = _engine(dev, ctx["w"], weight_dtype=fmt, lm_head_dtype=fmt if head else "bf16")
        out = q.score(input_ids=ids, attention_mask=am, other=eng, return_logits=True)
        _check_against_host(out, ids, am, f"weight_dtype={fmt} lm_head quantised={head}", other_logits=base_logits)
        assert out.mean_kl > 0.0 and 0.0 <= out.top1_agree <= 1.0
        kls[fmt] = out.mean_kl
        print(f"MEASURED score {fmt} (head {head}) vs bf16 engine: mean KL {out.mean_kl:.5f}, loss {out.loss:.5f} vs {ctx['out'].loss:.5f}, "
              f"top-1 agreement {out.top1_agree:.3f}")
    assert kls["mxfp4"] > kls["fp8"]        # CPU oracle on the dequantised weights, same ids: a factor 13.8 (module docstring)


def test_thinker_pass_through(dev):
    from test_prompt_lookup_gpu import _successor_thinker
    import prompt_lookup_cases as pc
    th = _successor_thinker(dev)
    row = [0, 0] + list(pc.PROMPT)
    row[6], row[7] = 290, 292                      # an image and an audio placeholder (no towers: their rows stay token embeddings)
    ids = torch.tensor([row])
    am = torch.ones_like(ids)
    am[0, :2] = 0
    out = th.score(ids, am)
    want_mask = am.bool() & (ids != 290) & (ids != 292)
    want_mask[:, 0] = False
    assert torch.equal(out.mask.cpu(), want_mask)
    emb, pos = th.prepare_inputs(ids, am)
    labels = torch.where(want_mask, ids, torch.full_like(ids, -100))
    ref = th.llm.score(inputs_embeds=emb, position_ids=pos, attention_mask=am, labels=labels)
    assert torch.equal(out.token_logprobs, ref.token_logprobs) and out.loss == ref.loss and out.n_tokens == int(want_mask.sum())
    # the successor model predicts succ(v) behind v: scored behind C[0] -> C[1]
    t = row.index(pc.C[1])
    assert row[t - 1] == pc.C[0] and int(out.argmax[0, t]) == pc.C[1]
    explicit = th.score(ids, am, labels=ids.clone())
    assert explicit.n_tokens == int(am.sum())           # every real position (index 0 is a pad here)

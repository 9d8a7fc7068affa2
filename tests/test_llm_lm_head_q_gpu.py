"""GPU: LlamaEngine(lm_head_dtype="fp8" | "mxfp4") end to end -- one model, two encodings of its lm_head. Mirrors
tests/test_llm_mxfp4_gpu.py (same tiny model: hidden 256, inter 512, head_dim 128, V 331, std 0.08, layers 2 / 3, seeds 21 / 25).

The engine with a quantised head IS a bf16 model whose lm_head is W_eff = dequantize(quantize(head)) (spider_amd/llm.py), so it is
held to the bound every bf16 engine is held to against the fp32 oracle (relative L2 < 2.5e-2), with the oracle built with the W_eff
head: the raw logits along each row's own greedy chain against the oracle teacher-forced on the same tokens.

What that bound can tell apart. MXFP4: round-to-nearest e2m1 moves the head by about a tenth, and the oracle with the ORIGINAL head
sits 4.7 to 4.9 bounds from the oracle with the W_eff head on the same tokens (computed on the CPU on the W_eff oracle's own greedy
chains for rows 1 / 3 / 4 / 5 and both input modes, which covers every MXFP4 case below: 2 layers / seed 21 0.1181 - 0.1189,
3 layers / seed 25 0.1180 - 0.1222; every case has >= 4 bounds there, none was dropped); the test asserts >= 3 bounds on the
engine's chains, so an engine that silently streamed the original head would fail. FP8: the same distance is 0.0260 - 0.0271,
1.04 - 1.08 bounds, and this engine-level bound CANNOT tell the two heads apart; it is not asserted. The FP8 head is discriminated by the
derived kernel-level bound of tests/test_lm_head_wq_gpu.py (2 K u sum |x W| + 2^-7 |ref|, against W_eff in fp64) and by the
bit-identity test below (constant forced to 0: the bf16 kernels on W_eff, bit for bit the bf16 engine built from W_eff).

LlamaEngine.LM_HEAD_FP8_MAX_ROWS / LM_HEAD_MXFP4_MAX_ROWS are measured crossovers; the tests force the row counts they mean to run
on the quantised head (the kernels exist for 1..4 rows) and on the fallback (the bf16 lm_head route on W_eff, as 5 rows always take).
No text-quality claim is made for either format: on random N(0, 0.08^2) heads of [331, 256] MXFP4 moves the logits by 11.8 %
relative L2 and changes the arg-max of 11 - 13 of 64 random activation rows, FP8 2.7 % and 3 - 4 of 64 (computed on the CPU)."""
import functools

import pytest
import torch

from beam_checks import check_beam_step  # noqa: F401  (the beam property check behind test_llm_beam_gpu._check_steps)
from test_llm_beam_gpu import BOUND, N, S, V, _inputs, _teacher

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
FMTS = ("fp8", "mxfp4")
BASE_KEYS = {"w_qkv", "b_qkv", "w_o", "w_gu", "w_down", "ln1", "ln2"}
FM_KEYS = {"w_qkv_fm", "w_gu_fm", "w_o_fm", "w_down_fm"}
Q4_KEYS = {k + s for k in ("w_qkv", "w_o", "w_gu", "w_down") for s in ("_q4", "_e4")}
HEAD_ATTRS = ("lm_head_q8", "lm_head_s8", "lm_head_q4", "lm_head_e4")
NEW_OPS = ("lm_head_argmax_w8", "lm_head_argmax_proc_w8", "lm_head_argmax_w4", "lm_head_argmax_proc_w4")


def _quant(fmt, t):
    from spider_amd.llm import quantize_fp8_rows, quantize_mxfp4
    return (quantize_fp8_rows if fmt == "fp8" else quantize_mxfp4)(t)


def _dequant(fmt, q, s):
    from spider_amd.llm import dequantize_fp8_rows, dequantize_mxfp4
    return (dequantize_fp8_rows if fmt == "fp8" else dequantize_mxfp4)(q, s)


def _bytes(eng, fmt):
    return (eng.lm_head_q8, eng.lm_head_s8) if fmt == "fp8" else (eng.lm_head_q4, eng.lm_head_e4)


@functools.lru_cache(maxsize=None)
def _model(layers, seed, fmt, tied=False):
    """(oracle config, original weights, weights with the W_eff head, oracle on the originals, oracle with the W_eff head)"""
    from oracle.llama import LlamaCfg, LlamaOracle
    ocfg = LlamaCfg(256, layers, 2, 1, 128, 512, V, 10000.0, None, 1e-6, False, 256, tied)
    w = LlamaOracle.random_weights(ocfg, seed=seed, std=0.08)
    w_eff = dict(w)
    w_eff["lm_head.weight"] = _dequant(fmt, *_quant(fmt, w["lm_head.weight"].to(BF))).float()
    return ocfg, w, w_eff, LlamaOracle(ocfg, w), LlamaOracle(ocfg, w_eff)


def _engine(dev, layers, seed, fmt, max_batch=8, lm_head_dtype=None, weight_dtype="bf16", weights=None, max_rows=None, tied=False):
    from spider_amd.llm import LlamaEngine, LLMConfig
    ocfg, w, _, _, _ = _model(layers, seed, fmt, tied)
    eng = LlamaEngine(LLMConfig(**ocfg.__dict__), w if weights is None else weights, dev, max_batch=max_batch, max_len=128,
                      weight_dtype=weight_dtype, lm_head_dtype=fmt if lm_head_dtype is None else lm_head_dtype)
    if max_rows is not None:
        eng.LM_HEAD_FP8_MAX_ROWS = eng.LM_HEAD_MXFP4_MAX_ROWS = max_rows
    return eng


def _count(monkeypatch):
    """counts the calls of the four quantised lm_head ops (eager steps and the steps a graph capture records), by name"""
    from spider_amd import ops
    calls = {"n": 0}
    for name in NEW_OPS:
        real = getattr(ops, name)
        calls[name] = 0

        def wrapped(*a, _real=real, _name=name, **kw):
            calls["n"] += 1
            calls[_name] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("fmt", FMTS)
def test_engine_state_is_the_head_in_two_encodings(dev, fmt):
    from spider_amd import ops
    from spider_amd.llm import LlamaEngine
    ocfg, w, w_eff, _, _ = _model(2, 21, fmt)
    eng = _engine(dev, 2, 21, fmt)
    assert eng.lm_head_dtype == fmt and eng.weight_dtype == "bf16"
    assert 0 <= LlamaEngine.LM_HEAD_FP8_MAX_ROWS <= 4 and 0 <= LlamaEngine.LM_HEAD_MXFP4_MAX_ROWS <= ops.LM_HEAD_Q_MAX_ROWS == 4
    eq = lambda t, ref: t.dtype == BF and torch.equal(t.float().cpu(), ref.float())
    assert eq(eng.lm_head, w_eff["lm_head.weight"]) and not torch.equal(eng.lm_head.float().cpu(), w["lm_head.weight"])
    q, sc = _quant(fmt, w["lm_head.weight"].to(BF))
    gq, gs = _bytes(eng, fmt)
    assert gq.is_contiguous() and gs.is_contiguous() and torch.equal(gq.cpu().view(torch.uint8), q.view(torch.uint8)) and torch.equal(gs.cpu(), sc)
    if fmt == "fp8":
        assert gq.dtype == torch.float8_e4m3fn and gq.shape == (V, 256) and gs.dtype == torch.float32 and gs.shape == (V,)
        assert not hasattr(eng, "lm_head_q4") and not hasattr(eng, "lm_head_e4")
    else:
        assert gq.dtype == torch.uint8 and gq.shape == (V, 128) and gs.dtype == torch.uint8 and gs.shape == (V, 8)
        assert not hasattr(eng, "lm_head_q8") and not hasattr(eng, "lm_head_s8")
    # the rest of the model is the checkpoint's
    assert eq(eng.embed_w, w["model.embed_tokens.weight"]) and eq(eng.norm, w["model.norm.weight"])
    for l, lw in enumerate(eng.layers):
        assert set(lw) == BASE_KEYS | (FM_KEYS if eng.fm_batch else set())
        assert eq(lw["w_o"], w[f"model.layers.{l}.self_attn.o_proj.weight"]) and eq(lw["w_down"], w[f"model.layers.{l}.mlp.down_proj.weight"])
    assert eng.fm_batch and torch.equal(eng.lm_head_fm, ops.repack_fm16(eng.lm_head, eng.norm))
    # a tied configuration: the embedding keeps the checkpoint's values, the head is a matrix of its own
    _, wt, wt_eff, _, _ = _model(2, 21, fmt, True)
    tied = _engine(dev, 2, 21, fmt, tied=True)
    assert tied.cfg.tie_embeddings and tied.lm_head is not tied.embed_w
    assert eq(tied.embed_w, wt["model.embed_tokens.weight"]) and eq(tied.lm_head, wt_eff["lm_head.weight"])
    assert torch.equal(_bytes(tied, fmt)[0].cpu().view(torch.uint8), _quant(fmt, wt["model.embed_tokens.weight"].to(BF))[0].view(torch.uint8))
    # quantised layers and a quantised head together: both sets of bytes
    both = _engine(dev, 2, 21, "mxfp4", weight_dtype="mxfp4")
    assert both.weight_dtype == "mxfp4" and both.lm_head_dtype == "mxfp4" and hasattr(both, "lm_head_q4")
    assert all(set(lw) == BASE_KEYS | Q4_KEYS | (FM_KEYS if both.fm_batch else set()) for lw in both.layers)


# rows 1, 3 and 4 with the constant forced to 4 (every row count the kernels exist for): the quantised head; 5 rows, and 3 rows of an
# engine told to stop at 2: the fallback route (the bf16 lm_head on W_eff). Both input modes, 2 and 3 layers.
CASES = [(1, 2, 21, "ids", 4), (1, 3, 25, "embeds", 4), (3, 3, 25, "ids", 4), (3, 2, 21, "embeds", 4), (4, 2, 21, "ids", 4),
         (4, 3, 25, "embeds", 4), (3, 3, 25, "ids", 2), (5, 3, 25, "ids", 4), (5, 2, 21, "embeds", 4)]


@pytest.mark.parametrize("B,layers,seed,mode,max_rows", CASES)
@pytest.mark.parametrize("fmt", FMTS)
def test_logits_match_the_oracle_with_the_w_eff_head(dev, monkeypatch, fmt, B, layers, seed, mode, max_rows):
    _, _, _, oracle_orig, oracle_eff = _model(layers, seed, fmt)
    eng = _engine(dev, layers, seed, fmt, max_rows=max_rows)
    calls = _count(monkeypatch)
    inp, ids, am = _inputs(eng, B, seed, mode)
    out = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
    assert (calls["n"] > 0) == (B <= max_rows), "rows up to the constant stream the quantised head, more rows do not"
    assert calls["n"] == calls["lm_head_argmax_w8" if fmt == "fp8" else "lm_head_argmax_w4"]
    logits, gen = out.logits.float().cpu(), out.sequences[:, -N:].cpu()
    assert logits.shape == (B, N, V) and set(eng._graphs) == {(B, False, True, 0)}
    ref_eff = [_teacher(oracle_eff, ids[b], am[b], gen[b].tolist()) for b in range(B)]
    for b in range(B):
        rel = _rel(logits[b], ref_eff[b])
        print(f"{fmt} B={B} layers={layers} {mode} row {b}: rel L2 to the oracle with the W_eff head {rel:.4f}")
        assert rel < BOUND, (b, rel)
    ref_orig = torch.cat([_teacher(oracle_orig, ids[b], am[b], gen[b].tolist()) for b in range(B)])
    sens = _rel(ref_orig, torch.cat(ref_eff))
    print(f"{fmt} B={B} layers={layers} {mode}: oracle(original head) to oracle(W_eff head) {sens:.4f} = {sens / BOUND:.1f} bounds")
    if fmt == "mxfp4":      # (FP8: about one bound, not asserted -- see the module docstring)
        assert sens >= 3 * BOUND, sens
        assert _rel(logits.reshape(-1, V), ref_orig) > BOUND


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("fmt", FMTS)
def test_quantised_head_engine_and_bf16_engine_on_w_eff_are_one_model(dev, monkeypatch, fmt, B):
    ocfg, w, w_eff, _, _ = _model(2, 21, fmt)
    qe = _engine(dev, 2, 21, fmt, max_rows=4)          # the quantised head at both row counts, whatever the measured default
    bf = _engine(dev, 2, 21, fmt, lm_head_dtype="bf16", weights=w_eff)
    assert torch.equal(qe.lm_head, bf.lm_head) and not any(hasattr(bf, a) for a in HEAD_ATTRS)
    inp, ids, am = _inputs(qe, B, 21, "ids")
    kw = dict(max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
    calls = _count(monkeypatch)
    a = qe.generate(**inp, **kw)
    assert calls["n"] > 0
    n0 = calls["n"]
    b = bf.generate(**inp, **kw)
    assert calls["n"] == n0
    la, lb = a.logits.float().cpu(), b.logits.float().cpu()
    ga, gb = a.sequences[:, -N:].cpu(), b.sequences[:, -N:].cpu()
    for r in range(B):
        # the two engines see the same history up to and including the first step at which their tokens differ (a near-tie)
        same = (ga[r] == gb[r]).long().cumprod(0)
        n = min(N, int(same.sum()) + 1)
        rel = _rel(la[r, :n], lb[r, :n])
        print(f"{fmt} B={B} row {r}: {n} common steps, rel L2 between the encodings {rel:.4f}")
        assert rel < BOUND, (r, n, rel)
    # with the quantised kernels switched off the engine runs the bf16 engine's kernels on the bf16 engine's head: bit for bit
    off = _engine(dev, 2, 21, fmt, max_rows=0)
    c = off.generate(**inp, **kw)
    assert calls["n"] == n0
    assert torch.equal(c.sequences, b.sequences) and torch.equal(c.logits, b.logits)


@pytest.mark.parametrize("fmt", FMTS)
def test_sampling_processors_and_beams_run_behind_the_quantised_head(dev, monkeypatch, fmt):
    from test_llm_beam_gpu import _check_steps as beam_check_steps, _trace
    from test_llm_ngram_gpu import _replay as ngram_replay
    from test_llm_processors_gpu import _replay
    from test_llm_sampling_gpu import SAMPLING, _check_steps as sample_check_steps
    eng = _engine(dev, 2, 21, fmt, max_rows=4)
    plain_op, proc_op = ("lm_head_argmax_w8", "lm_head_argmax_proc_w8") if fmt == "fp8" else ("lm_head_argmax_w4", "lm_head_argmax_proc_w4")
    calls = _count(monkeypatch)
    B = 3
    inp, ids, am = _inputs(eng, B, 21, "ids")
    # --- do_sample: one seed, one output; every step passes the host token check; graph == eager
    kw = dict(max_new_tokens=N, do_sample=True, seed=1234567, return_dict_in_generate=True, return_logits=True, **SAMPLING)
    s1, s2, s3 = eng.generate(**inp, **kw), eng.generate(**inp, **kw), eng.generate(**inp, **kw, use_graph=False)
    assert torch.equal(s1.sequences, s2.sequences) and torch.equal(s1.sequences, s3.sequences) and torch.equal(s1.logits, s3.logits)
    assert sample_check_steps(s1, ids, "ids", 1234567) == B * N
    assert not torch.equal(eng.generate(**inp, **dict(kw, seed=7654321)).sequences, s1.sequences)
    assert calls[plain_op] > 0 and calls[proc_op] == 0, "the sampling step reads the raw logits of the plain quantised launch"
    # --- repetition_penalty: the tokens replay under transformers' processor on the engine's raw logits; graph == eager
    kw = dict(max_new_tokens=N, repetition_penalty=1.3, return_dict_in_generate=True, return_logits=True)
    p1, p2 = eng.generate(**inp, **kw), eng.generate(**inp, **kw, use_graph=False)
    assert torch.equal(p1.sequences, p2.sequences) and torch.equal(p1.logits, p2.logits)
    bad, touched = _replay(p1.sequences[:, -N:], p1.logits, ids, None, 1.3, 0, [])
    assert bad is None and touched > 0, (bad, touched)
    assert calls[proc_op] > 0, "processed requests take the PROC form of the quantised launch"
    # --- no_repeat_ngram_size=2: the same replay with the n-gram bans
    kw = dict(max_new_tokens=N, no_repeat_ngram_size=2, return_dict_in_generate=True, return_logits=True)
    g1, g2 = eng.generate(**inp, **kw), eng.generate(**inp, **kw, use_graph=False)
    assert torch.equal(g1.sequences, g2.sequences) and torch.equal(g1.logits, g2.logits)
    bad, _ = ngram_replay(g1.sequences[:, -N:], g1.logits, ids, 2)
    assert bad is None, bad
    # --- num_beams=2 (2 rows): every step of the trace passes check_beam_step; graph and eager write the same trace
    inp1, _, _ = _inputs(eng, 1, 21, "ids")
    kw = dict(max_new_tokens=N, num_beams=2, num_return_sequences=2, return_dict_in_generate=True, return_logits=True)
    n0 = calls[plain_op]
    b1 = eng.generate(**inp1, **kw)
    assert calls[plain_op] > n0, "the beam rows stream the quantised head too"
    tr_g, _ = _trace(eng, 1, 2, 4, N)
    b2 = eng.generate(**inp1, **kw, use_graph=False)
    tr_e, _ = _trace(eng, 1, 2, 4, N)
    assert all(torch.equal(x, y) for x, y in zip(tr_g, tr_e))
    assert torch.equal(b1.sequences, b2.sequences) and torch.equal(b1.sequences_scores, b2.sequences_scores)
    assert len(beam_check_steps(tr_g, b1.logits.cpu(), 1, 2, None)) == N
    keys = {(B, False, True, 0, "sample"), (B, False, True, 0, True), (B, False, True, 0, True, "ngram"), (1, False, True, 0, "beam", 2, 4)}
    assert set(eng._graphs) == keys
    # exactly the keys a bf16 engine produces for the same requests
    bf = _engine(dev, 2, 21, fmt, lm_head_dtype="bf16")
    n0 = calls["n"]
    bf.generate(**inp, max_new_tokens=4, do_sample=True, seed=1, return_dict_in_generate=True, return_logits=True, **SAMPLING)
    bf.generate(**inp, max_new_tokens=4, repetition_penalty=1.3, return_dict_in_generate=True, return_logits=True)
    bf.generate(**inp, max_new_tokens=4, no_repeat_ngram_size=2, return_dict_in_generate=True, return_logits=True)
    bf.generate(**inp1, max_new_tokens=4, num_beams=2, return_dict_in_generate=True, return_logits=True)
    assert set(bf._graphs) == keys and calls["n"] == n0


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
def test_vocabulary_changes_keep_the_two_encodings_in_step(dev, monkeypatch, fmt, tied):
    ocfg, w, _, _, _ = _model(2, 21, fmt, tied)
    eng = _engine(dev, 2, 21, fmt, max_rows=4, tied=tied)
    calls = _count(monkeypatch)
    inp, ids, am = _inputs(eng, 2, 21, "ids")
    eng.generate(**inp, max_new_tokens=4)
    assert eng._graphs
    u8 = lambda t: t.cpu().view(torch.uint8)

    def in_step(src):
        """bytes == quantize(source), lm_head == its W_eff, the fragment-major copy is built from it"""
        from spider_amd import ops
        q, sc = _quant(fmt, src.cpu())
        gq, gs = _bytes(eng, fmt)
        assert torch.equal(u8(gq), q.view(torch.uint8)) and torch.equal(gs.cpu(), sc) and gq.is_contiguous() and gs.is_contiguous()
        assert eng.lm_head.dtype == BF and torch.equal(eng.lm_head.cpu(), _dequant(fmt, q, sc))
        assert torch.equal(eng.lm_head_fm, ops.repack_fm16(eng.lm_head, eng.norm))
        assert eng.lm_head is not eng.embed_w
    before, emb_before = eng.lm_head.clone(), eng.embed_w.clone()
    # --- resize: old rows keep their W_eff values, the new rows are quantised too
    ret = eng.resize_token_embeddings(V + 5, seed=3)
    assert ret is eng.embed_w and eng.cfg.vocab == V + 5 and eng.lm_head.shape == (V + 5, 256) == eng.embed_w.shape and eng._graphs == {}
    assert torch.equal(eng.lm_head[:V], before) and torch.equal(eng.embed_w[:V], emb_before)
    assert float(eng.lm_head[V:].float().abs().max()) > 0
    if tied:
        in_step(eng.embed_w)
    else:       # the source was the grown head itself; both quantisers are fixed points on it in values
        assert torch.equal(_dequant(fmt, *_quant(fmt, eng.lm_head.cpu())), eng.lm_head.cpu())
        assert torch.equal(_dequant(fmt, *(t.cpu() for t in _bytes(eng, fmt))), eng.lm_head.cpu())
    eng.generate(**inp, max_new_tokens=4)
    assert eng._graphs
    # --- trained rows for the new tokens
    g = torch.Generator().manual_seed(9)
    head_rows = (torch.randn(5, 256, generator=g) * 0.08).to(BF)
    emb_rows = (torch.randn(5, 256, generator=g) * 0.08).to(BF)
    if tied:    # embed_rows reach the head; lm_head_rows land in the embedding matrix, as they do on a tied bf16 engine
        eng.load_token_rows(V, embed_rows=emb_rows)
        assert eng._graphs == {} and torch.equal(eng.embed_w[V:].cpu(), emb_rows) and torch.equal(eng.embed_w[:V], emb_before)
        in_step(eng.embed_w)
        assert torch.equal(eng.lm_head[V:].cpu(), _dequant(fmt, *_quant(fmt, emb_rows)))
        eng.load_token_rows(V + 1, lm_head_rows=head_rows[:2])
        assert torch.equal(eng.embed_w[V + 1:V + 3].cpu(), head_rows[:2])
        in_step(eng.embed_w)
    else:
        eng.load_token_rows(V, embed_rows=emb_rows, lm_head_rows=head_rows)
        assert eng._graphs == {} and torch.equal(eng.embed_w[V:].cpu(), emb_rows)
        in_step(torch.cat([before.cpu(), head_rows]))
    assert torch.equal(eng.lm_head[:V], before), "rows nobody touched keep their values"
    n0 = calls["n"]
    out = eng.generate(**inp, max_new_tokens=N)
    assert calls["n"] > n0 and int(out.max()) < V + 5 and eng._graphs
    # --- the default engine in the same calls: unchanged
    dflt = _engine(dev, 2, 21, fmt, lm_head_dtype="bf16", tied=tied)
    dflt.resize_token_embeddings(V + 5, seed=3)
    dflt.load_token_rows(V, embed_rows=emb_rows, lm_head_rows=head_rows)
    assert (dflt.lm_head is dflt.embed_w) == tied and not any(hasattr(dflt, a) for a in HEAD_ATTRS)
    assert torch.equal(dflt.lm_head[V:].cpu(), head_rows)
    assert torch.equal(dflt.embed_w[V:].cpu(), head_rows if tied else emb_rows)


def test_defaults_are_untouched(dev, monkeypatch):
    from spider_amd.llm import LlamaEngine
    ocfg, w, _, _, _ = _model(2, 21, "mxfp4")
    eng = _engine(dev, 2, 21, "mxfp4", lm_head_dtype="bf16")
    positional = LlamaEngine(eng.cfg, w, dev, 8, 128)                     # the constructor's positional arguments mean what they meant
    fp8 = LlamaEngine(eng.cfg, w, dev, 8, 128, "fp8")
    mx = LlamaEngine(eng.cfg, w, dev, 8, 128, weight_dtype="mxfp4")
    calls = _count(monkeypatch)
    for e, wd in ((eng, "bf16"), (positional, "bf16"), (fp8, "fp8"), (mx, "mxfp4")):
        assert e.weight_dtype == wd and e.lm_head_dtype == "bf16" and not any(hasattr(e, a) for a in HEAD_ATTRS)
        assert torch.equal(e.lm_head.float().cpu(), w["lm_head.weight"])
    inp, ids, am = _inputs(eng, 3, 21, "ids")
    inp1, _, _ = _inputs(eng, 1, 21, "ids")
    a = eng.generate(**inp, max_new_tokens=N)
    for e in (eng, fp8, mx):
        e.generate(**inp, max_new_tokens=N)
        e.generate(**inp1, max_new_tokens=N)
        assert set(e._graphs) == {(3, False, False, 0), (1, False, False, 0)}
    assert torch.equal(positional.generate(**inp, max_new_tokens=N), a) and calls["n"] == 0
    # an engine with a quantised head keys its states the same way
    q = _engine(dev, 2, 21, "mxfp4", max_rows=4)
    q.generate(**inp, max_new_tokens=N)
    assert set(q._graphs) == {(3, False, False, 0)} and calls["n"] > 0
    with pytest.raises(ValueError, match="lm_head_dtype"):
        _engine(dev, 2, 21, "mxfp4", lm_head_dtype="int4")
    with pytest.raises(ValueError, match="lm_head_dtype"):
        LlamaEngine.random_init(eng.cfg, dev, lm_head_dtype="int4")

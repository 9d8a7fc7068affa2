"""GPU: LlamaEngine(weight_dtype="mxfp4") end to end -- one model, two encodings. Mirrors tests/test_llm_fp8_gpu.py.

The MXFP4 engine IS a bf16 model with weights W_eff = dequantize_mxfp4(quantize_mxfp4(W)) (spider_amd/llm.py), so it is held to the
bound a bf16 engine is held to against the fp32 oracle (tests/test_llm_engine.py: relative L2 < 2.5e-2), with the oracle built
from W_eff: the raw logits along each row's own greedy chain against the oracle teacher-forced on the same tokens. That bound can
tell the two models apart: round-to-nearest MXFP4 moves the weights by about a tenth, and the oracle on the ORIGINAL weights sits
19 to 24 bounds from the oracle on W_eff on the same tokens (on the W_eff oracle's own greedy chains, computed on the CPU for the
seeds, row counts and input modes below: 2 layers / seed 21 0.478 - 0.502, 3 layers / seed 25 0.534 - 0.603; the FP8 engine has
about 5 bounds). The test asserts >= 3 bounds on the engine's chains -- an engine that silently
streamed the originals would fail. LlamaEngine.MXFP4_MAX_ROWS is a measured crossover; the tests force the row counts they mean
to run on the MXFP4 GEMVs (the kernels exist for 1..4 rows) and on the fallback (the bf16 route on W_eff, as 5 rows always take)."""
import functools

import pytest
import torch

from beam_checks import check_beam_step  # noqa: F401  (the beam property check behind test_llm_beam_gpu._check_steps)
from test_llm_beam_gpu import BOUND, N, S, V, _inputs, _teacher

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
BASE_KEYS = {"w_qkv", "b_qkv", "w_o", "w_gu", "w_down", "ln1", "ln2"}
FM_KEYS = {"w_qkv_fm", "w_gu_fm", "w_o_fm", "w_down_fm"}
Q8_KEYS = {k + s for k in ("w_qkv", "w_o", "w_gu", "w_down") for s in ("_q8", "_s8")}
Q4_KEYS = {k + s for k in ("w_qkv", "w_o", "w_gu", "w_down") for s in ("_q4", "_e4")}


@functools.lru_cache(maxsize=None)
def _model(layers, seed):
    """(oracle config, original weights, W_eff weights, oracle on the originals, oracle on W_eff): hidden 256, inter 512,
    head_dim 128, V 331, std 0.08 -- the engine recipe of tests/test_llm_beam_gpu.py. Blocks of 32 run along a weight row, so
    quantising q / k / v (gate / up) apart equals quantising the engine's concatenation."""
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd.llm import dequantize_mxfp4, quantize_mxfp4
    ocfg = LlamaCfg(256, layers, 2, 1, 128, 512, V, 10000.0, None, 1e-6, False, 256)
    w = LlamaOracle.random_weights(ocfg, seed=seed, std=0.08)
    w_eff = {k: (dequantize_mxfp4(*quantize_mxfp4(v.to(BF))).float() if k.split(".")[-2] in PROJ else v) for k, v in w.items()}
    return ocfg, w, w_eff, LlamaOracle(ocfg, w), LlamaOracle(ocfg, w_eff)


def _engine(dev, layers, seed, max_batch=8, weight_dtype="mxfp4", weights=None, max_rows=None):
    from spider_amd.llm import LlamaEngine, LLMConfig
    ocfg, w, w_eff, _, _ = _model(layers, seed)
    eng = LlamaEngine(LLMConfig(**ocfg.__dict__), w if weights is None else weights, dev, max_batch=max_batch, max_len=128,
                      weight_dtype=weight_dtype)
    if max_rows is not None:
        eng.MXFP4_MAX_ROWS = max_rows
    return eng


def _count(monkeypatch, names=("gemv_w4", "gemv_swiglu_w4")):
    """counts the calls of the two MXFP4 ops (eager steps and the steps a graph capture records)"""
    from spider_amd import ops
    calls = {"n": 0}
    for name in names:
        real = getattr(ops, name)

        def wrapped(*a, _real=real, **kw):
            calls["n"] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_engine_state_is_w_eff_in_two_encodings(dev):
    from spider_amd import ops
    from spider_amd.llm import LlamaEngine, quantize_mxfp4
    ocfg, w, w_eff, _, _ = _model(2, 21)
    eng = _engine(dev, 2, 21)
    assert eng.weight_dtype == "mxfp4" and 0 <= LlamaEngine.MXFP4_MAX_ROWS <= ops.W4_MAX_ROWS == 4
    eq = lambda t, ref: t.dtype == BF and torch.equal(t.float().cpu(), ref.float())
    for l, lw in enumerate(eng.layers):
        assert set(lw) == BASE_KEYS | Q4_KEYS | (FM_KEYS if eng.fm_batch else set())
        p = f"model.layers.{l}."
        cat = lambda d, names: torch.cat([d[p + n + ".weight"] for n in names], 0)
        for key, names in (("w_qkv", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")), ("w_o", ("self_attn.o_proj",)),
                           ("w_gu", ("mlp.gate_proj", "mlp.up_proj")), ("w_down", ("mlp.down_proj",))):
            assert eq(lw[key], cat(w_eff, names)), key                       # = dequantize_mxfp4(quantize_mxfp4(original)), exactly
            assert not torch.equal(lw[key].float().cpu(), cat(w, names))     # (and the originals are no fixed point of it)
            q, sc = quantize_mxfp4(cat(w, names).to(BF))
            n, k = lw[key].shape
            assert lw[key + "_q4"].dtype == torch.uint8 and lw[key + "_e4"].dtype == torch.uint8
            assert lw[key + "_q4"].shape == (n, k // 2) and lw[key + "_e4"].shape == (n, k // 32)
            assert lw[key + "_q4"].is_contiguous() and lw[key + "_e4"].is_contiguous()
            assert torch.equal(lw[key + "_q4"].cpu(), q) and torch.equal(lw[key + "_e4"].cpu(), sc)
        assert eq(lw["ln1"], w[p + "input_layernorm.weight"]) and eq(lw["ln2"], w[p + "post_attention_layernorm.weight"])
        if eng.fm_batch:     # the fragment-major copies are built from W_eff too
            assert torch.equal(lw["w_o_fm"], ops.repack_fm16(lw["w_o"])) and torch.equal(lw["w_gu_fm"], ops.repack_fm16(lw["w_gu"], lw["ln2"]))
    assert eq(eng.lm_head, w["lm_head.weight"]) and eq(eng.embed_w, w["model.embed_tokens.weight"]) and eq(eng.norm, w["model.norm.weight"])


# rows 1, 3 and 4 with MXFP4_MAX_ROWS = 4 (every row count the kernels exist for): the MXFP4 GEMVs; 5 rows, and 3 rows of an engine
# told to stop at 2: the fallback route (fragment-major bf16 on W_eff). Both input modes, 2 and 3 layers.
@pytest.mark.parametrize("B,layers,seed,mode,max_rows", [
    (1, 2, 21, "ids", 4), (1, 3, 25, "embeds", 4), (3, 3, 25, "ids", 4), (3, 2, 21, "embeds", 4), (4, 2, 21, "ids", 4),
    (4, 3, 25, "embeds", 4), (3, 3, 25, "ids", 2), (5, 3, 25, "ids", 4), (5, 2, 21, "embeds", 4)])
def test_logits_match_the_oracle_on_w_eff(dev, monkeypatch, B, layers, seed, mode, max_rows):
    _, _, _, oracle_orig, oracle_eff = _model(layers, seed)
    eng = _engine(dev, layers, seed, max_rows=max_rows)
    calls = _count(monkeypatch)
    inp, ids, am = _inputs(eng, B, seed, mode)
    out = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
    assert (calls["n"] > 0) == (B <= max_rows), "rows up to MXFP4_MAX_ROWS stream the MXFP4 bytes, more rows do not"
    logits, gen = out.logits.float().cpu(), out.sequences[:, -N:].cpu()
    assert logits.shape == (B, N, V) and set(eng._graphs) == {(B, False, True, 0)}
    ref_eff = [_teacher(oracle_eff, ids[b], am[b], gen[b].tolist()) for b in range(B)]
    for b in range(B):
        rel = _rel(logits[b], ref_eff[b])
        print(f"B={B} layers={layers} {mode} row {b}: rel L2 to the oracle on W_eff {rel:.4f}")
        assert rel < BOUND, (b, rel)
    # sensitivity of that bound, on the same tokens: the oracle on the original weights is not within it, by a factor
    ref_orig = torch.cat([_teacher(oracle_orig, ids[b], am[b], gen[b].tolist()) for b in range(B)])
    sens = _rel(ref_orig, torch.cat(ref_eff))
    print(f"B={B} layers={layers} {mode}: oracle(original) to oracle(W_eff) {sens:.4f} = {sens / BOUND:.1f} bounds")
    assert sens >= 3 * BOUND, sens
    assert _rel(logits.reshape(-1, V), ref_orig) > BOUND


@pytest.mark.parametrize("B", [1, 4])
def test_mxfp4_engine_and_bf16_engine_on_w_eff_are_one_model(dev, monkeypatch, B):
    ocfg, w, w_eff, _, _ = _model(2, 21)
    mx = _engine(dev, 2, 21, max_rows=4)        # the MXFP4 kernels at both row counts, whatever the measured default
    bf = _engine(dev, 2, 21, weight_dtype="bf16", weights=w_eff)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(mx.layers, bf.layers) for k in ("w_qkv", "w_o", "w_gu", "w_down"))
    inp, ids, am = _inputs(mx, B, 21, "ids")
    kw = dict(max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
    calls = _count(monkeypatch)
    a = mx.generate(**inp, **kw)
    assert calls["n"] > 0
    b = bf.generate(**inp, **kw)
    la, lb = a.logits.float().cpu(), b.logits.float().cpu()
    ga, gb = a.sequences[:, -N:].cpu(), b.sequences[:, -N:].cpu()
    for r in range(B):
        # the two engines see the same history up to and including the first step at which their tokens differ (a near-tie)
        same = (ga[r] == gb[r]).long().cumprod(0)
        n = min(N, int(same.sum()) + 1)
        rel = _rel(la[r, :n], lb[r, :n])
        print(f"B={B} row {r}: {n} common steps, rel L2 between the encodings {rel:.4f}")
        assert rel < BOUND, (r, n, rel)
    # with the MXFP4 kernels switched off the MXFP4 engine runs the bf16 engine's kernels on the bf16 engine's weights: bit for bit
    off = _engine(dev, 2, 21, max_rows=0)
    before = calls["n"]
    c = off.generate(**inp, **kw)
    assert calls["n"] == before
    assert torch.equal(c.sequences, b.sequences) and torch.equal(c.logits, b.logits)


def test_sampling_penalty_and_beams_run_behind_the_mxfp4_layers(dev, monkeypatch):
    from test_llm_beam_gpu import _check_steps as beam_check_steps, _trace
    from test_llm_processors_gpu import _replay
    from test_llm_sampling_gpu import SAMPLING, _check_steps as sample_check_steps
    eng = _engine(dev, 2, 21, max_rows=4)
    calls = _count(monkeypatch)
    B = 3
    inp, ids, am = _inputs(eng, B, 21, "ids")
    # --- do_sample: one seed, one output; every step passes the host token check; graph == eager
    kw = dict(max_new_tokens=N, do_sample=True, seed=1234567, return_dict_in_generate=True, return_logits=True, **SAMPLING)
    s1, s2, s3 = eng.generate(**inp, **kw), eng.generate(**inp, **kw), eng.generate(**inp, **kw, use_graph=False)
    assert torch.equal(s1.sequences, s2.sequences) and torch.equal(s1.sequences, s3.sequences) and torch.equal(s1.logits, s3.logits)
    assert sample_check_steps(s1, ids, "ids", 1234567) == B * N
    assert not torch.equal(eng.generate(**inp, **dict(kw, seed=7654321)).sequences, s1.sequences)
    # --- repetition_penalty: the tokens replay under transformers' processor on the engine's raw logits; graph == eager
    kw = dict(max_new_tokens=N, repetition_penalty=1.3, return_dict_in_generate=True, return_logits=True)
    p1, p2 = eng.generate(**inp, **kw), eng.generate(**inp, **kw, use_graph=False)
    assert torch.equal(p1.sequences, p2.sequences) and torch.equal(p1.logits, p2.logits)
    bad, touched = _replay(p1.sequences[:, -N:], p1.logits, ids, None, 1.3, 0, [])
    assert bad is None and touched > 0, (bad, touched)
    # --- num_beams=2 (2 rows): every step of the trace passes check_beam_step; graph and eager write the same trace
    inp1, _, _ = _inputs(eng, 1, 21, "ids")
    kw = dict(max_new_tokens=N, num_beams=2, num_return_sequences=2, return_dict_in_generate=True, return_logits=True)
    n0 = calls["n"]
    b1 = eng.generate(**inp1, **kw)
    assert calls["n"] > n0, "the beam rows stream the MXFP4 bytes too"
    tr_g, _ = _trace(eng, 1, 2, 4, N)
    b2 = eng.generate(**inp1, **kw, use_graph=False)
    tr_e, _ = _trace(eng, 1, 2, 4, N)
    assert all(torch.equal(x, y) for x, y in zip(tr_g, tr_e))
    assert torch.equal(b1.sequences, b2.sequences) and torch.equal(b1.sequences_scores, b2.sequences_scores)
    assert len(beam_check_steps(tr_g, b1.logits.cpu(), 1, 2, None)) == N
    assert set(eng._graphs) == {(B, False, True, 0, "sample"), (B, False, True, 0, True), (1, False, True, 0, "beam", 2, 4)}


def test_default_and_fp8_engines_are_untouched(dev, monkeypatch):
    from spider_amd.llm import LlamaEngine
    ocfg, w, w_eff, _, _ = _model(2, 21)
    eng = _engine(dev, 2, 21, weight_dtype="bf16")
    positional = LlamaEngine(eng.cfg, w, dev, 8, 128)                     # the constructor's positional arguments mean what they meant
    fp8 = _engine(dev, 2, 21, weight_dtype="fp8")
    assert eng.weight_dtype == "bf16" and positional.weight_dtype == "bf16" and fp8.weight_dtype == "fp8" and LlamaEngine.FP8_MAX_ROWS == 3
    calls = _count(monkeypatch)
    for l, (lw, lp, l8) in enumerate(zip(eng.layers, positional.layers, fp8.layers)):
        assert set(lw) == BASE_KEYS | (FM_KEYS if eng.fm_batch else set()) == set(lp)
        assert set(l8) == BASE_KEYS | Q8_KEYS | (FM_KEYS if fp8.fm_batch else set())
        assert not any(k.endswith(("_q4", "_e4")) for k in list(lw) + list(l8))
        assert torch.equal(lw["w_o"].float().cpu(), w[f"model.layers.{l}.self_attn.o_proj.weight"])
    inp, ids, am = _inputs(eng, 3, 21, "ids")
    a = eng.generate(**inp, max_new_tokens=N)
    inp1, _, _ = _inputs(eng, 1, 21, "ids")
    eng.generate(**inp1, max_new_tokens=N)
    fp8.generate(**inp, max_new_tokens=N)
    fp8.generate(**inp1, max_new_tokens=N)
    assert set(eng._graphs) == {(3, False, False, 0), (1, False, False, 0)} == set(fp8._graphs) and calls["n"] == 0
    assert torch.equal(positional.generate(**inp, max_new_tokens=N), a)
    # an MXFP4 engine keys its states the same way (a state belongs to an engine)
    mx = _engine(dev, 2, 21, max_rows=4)
    mx.generate(**inp, max_new_tokens=N)
    assert set(mx._graphs) == {(3, False, False, 0)} and calls["n"] > 0
    with pytest.raises(ValueError, match="weight_dtype"):
        _engine(dev, 2, 21, weight_dtype="int4")

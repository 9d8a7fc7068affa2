"""GPU: LlamaEngine(weight_dtype="fp8" | "mxfp4", batched_weight_stream=True) end to end -- W_eff in a third encoding.

With the keyword every layer holds its quantised bytes once more, in the fragment-major order of csrc/gemv_qfm.hip, and decode steps
of more rows than the row-major kernels serve (up to FP8_FM_MAX_ROWS / MXFP4_FM_MAX_ROWS) stream them through the MFMA kernels. The
engine stays a bf16 model on W_eff, so it is held to the bound of tests/test_llm_mxfp4_gpu.py / tests/test_llm_fp8_gpu.py, whose model
recipes and helpers are imported: raw logits along each row's own greedy chain within BOUND (relative L2 < 2.5e-2) of the fp32 oracle
on W_eff, teacher-forced on the same tokens, while the oracle on the ORIGINAL weights is >= 3 bounds away on those tokens. That
distance is a property of the two oracles; on the W_eff oracle's own greedy chains, computed on the CPU for the seeds, row counts and
input modes below, it is 18.9 - 24.1 bounds for MXFP4 (2 layers / seed 21: 0.473 - 0.494, 3 layers / seed 25: 0.562 - 0.603) and
4.5 - 5.8 bounds for FP8 (0.112 - 0.120, 0.139 - 0.146) at 5 and 8 rows.
The imported `_inputs` left-pads row b of an "ids" request with 2 + b ids: from row 7 on that is the whole prompt of 9, a row with
nothing to attend to, which no engine and no oracle defines. `_inputs` below restarts the run of pads there (row 7: 2 pads).
*_FM_MAX_ROWS are measured crossovers (scripts/exp/qfm_decode_cost.py); the tests force the row counts they mean to run on the new
kernels, as the existing tests force MXFP4_MAX_ROWS."""
import pytest
import torch

import test_llm_fp8_gpu as t8
import test_llm_mxfp4_gpu as t4
from test_llm_beam_gpu import BOUND, N, S, V, _teacher
from test_llm_beam_gpu import _inputs as _inputs_upto_7_rows

pytestmark = pytest.mark.gpu

W = ("w_qkv", "w_o", "w_gu", "w_down")
Q4FM_KEYS = {k + s for k in W for s in ("_q4fm", "_e4fm")}
Q8FM_KEYS = {k + "_q8fm" for k in W}
NEW_OPS = ("gemv_fm_w4", "gemv_swiglu_fm_w4", "gemv_fm_w8", "gemv_swiglu_fm_w8")
OLD_OPS = ("gemv_w4", "gemv_swiglu_w4", "gemv_w8", "gemv_swiglu_w8")


def _model(fmt, layers, seed):
    return (t4 if fmt == "mxfp4" else t8)._model(layers, seed)


def _engine(dev, fmt, layers, seed, stream=True, fm_rows=8, max_batch=8):
    """fm_rows: the forced *_FM_MAX_ROWS (None: the class's measured value); the row-major range is forced to 4 for both formats"""
    from spider_amd.llm import LlamaEngine, LLMConfig
    ocfg, w, _, _, _ = _model(fmt if fmt != "bf16" else "mxfp4", layers, seed)
    kw = dict(batched_weight_stream=True) if stream else {}
    eng = LlamaEngine(LLMConfig(**ocfg.__dict__), w, dev, max_batch=max_batch, max_len=128, weight_dtype=fmt, **kw)
    eng.MXFP4_MAX_ROWS = eng.FP8_MAX_ROWS = 4
    if fm_rows is not None:
        eng.MXFP4_FM_MAX_ROWS = eng.FP8_FM_MAX_ROWS = fm_rows
    return eng


def _inputs(eng, B, seed, mode):
    """test_llm_beam_gpu._inputs with a real prompt in every row (module docstring); rows 0..6 are that helper's"""
    inp, ids, am = _inputs_upto_7_rows(eng, B, seed, mode)
    if mode == "ids":
        fresh = torch.randint(3, V, (B, S), generator=torch.Generator().manual_seed(100 + seed))
        for b in range(S - 2, B):
            pad = 2 + b - (S - 2)
            ids[b], am[b] = fresh[b], 1
            ids[b, :pad] = 0
            am[b, :pad] = 0
        assert inp["input_ids"] is ids and inp["attention_mask"] is am and int(am.sum(1).min()) >= 1
    return inp, ids, am


def _counts(monkeypatch):
    """calls of the fragment-major and of the row-major weight-only ops (eager steps and the steps a graph capture records)"""
    return t4._count(monkeypatch, NEW_OPS), t4._count(monkeypatch, OLD_OPS)


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_engine_state_holds_the_bytes_in_fragment_major_order(dev):
    from spider_amd import ops
    from spider_amd.llm import LlamaEngine, LLMConfig
    assert 0 <= LlamaEngine.MXFP4_FM_MAX_ROWS <= LlamaEngine.DECODE_ROWS and 0 <= LlamaEngine.FP8_FM_MAX_ROWS <= LlamaEngine.DECODE_ROWS
    assert LlamaEngine.MXFP4_FM_MAX_ROWS in (0, *range(LlamaEngine.MXFP4_MAX_ROWS + 1, 9)) and LlamaEngine.FP8_FM_MAX_ROWS in (0, *range(LlamaEngine.FP8_MAX_ROWS + 1, 9))
    mx, f8 = _engine(dev, "mxfp4", 2, 21, fm_rows=None), _engine(dev, "fp8", 2, 21, fm_rows=None)
    assert mx.batched_weight_stream and f8.batched_weight_stream and mx.MXFP4_FM_MAX_ROWS == LlamaEngine.MXFP4_FM_MAX_ROWS
    for lw in mx.layers:
        assert set(lw) == t4.BASE_KEYS | t4.Q4_KEYS | t4.FM_KEYS | Q4FM_KEYS
        for k in W:
            qfm, efm = ops.repack_fm_w4(lw[k + "_q4"], lw[k + "_e4"])
            assert torch.equal(lw[k + "_q4fm"], qfm) and torch.equal(lw[k + "_e4fm"], efm) and lw[k + "_q4fm"].is_contiguous()
    for lw in f8.layers:
        assert set(lw) == t8.BASE_KEYS | t8.Q8_KEYS | t8.FM_KEYS | Q8FM_KEYS
        for k in W:
            assert torch.equal(lw[k + "_q8fm"], ops.repack_fm_w8(lw[k + "_q8"])) and lw[k + "_q8fm"].dtype == torch.uint8
    # without the keyword: today's key sets
    for lw in _engine(dev, "mxfp4", 2, 21, stream=False).layers:
        assert set(lw) == t4.BASE_KEYS | t4.Q4_KEYS | t4.FM_KEYS
    for lw in _engine(dev, "fp8", 2, 21, stream=False).layers:
        assert set(lw) == t8.BASE_KEYS | t8.Q8_KEYS | t8.FM_KEYS
    # what the keyword refuses
    ocfg, w, _, _, _ = _model("mxfp4", 2, 21)
    mk = lambda cfg=None, **kw: LlamaEngine(LLMConfig(**(cfg or ocfg).__dict__), w, dev, max_len=128, batched_weight_stream=True, **kw)
    with pytest.raises(ValueError, match="weight_dtype"):
        mk(max_batch=8)
    with pytest.raises(ValueError, match="weight_dtype"):
        mk(max_batch=8, weight_dtype="bf16")
    for fmt in ("mxfp4", "fp8"):
        with pytest.raises(ValueError, match="max_batch"):
            mk(max_batch=4, weight_dtype=fmt)
    from oracle.llama import LlamaCfg
    for fmt, bad in (("mxfp4", 192), ("mxfp4", 320), ("fp8", 96), ("fp8", 160)):     # multiples of the row-major rule (32 / 16), not of 128 / 64
        for field in ("inter", "hidden"):
            c = LlamaCfg(bad if field == "hidden" else 256, 2, 2, 1, 128, bad if field == "inter" else 512, V, 10000.0, None, 1e-6, False, 256)
            with pytest.raises(ValueError, match="multiples of"):
                mk(cfg=c, max_batch=8, weight_dtype=fmt)
    import inspect
    for fn in (LlamaEngine.__init__, LlamaEngine.random_init, LlamaEngine.from_pretrained):      # the keyword sits behind lm_head_dtype
        names = list(inspect.signature(fn).parameters)
        assert names[-2:] == ["lm_head_dtype", "batched_weight_stream"] and inspect.signature(fn).parameters["batched_weight_stream"].default is False


# 5 and 8 rows on the fragment-major quantised kernels; both formats, both input modes, 2 and 3 layers
@pytest.mark.parametrize("fmt,B,layers,seed,mode", [
    ("mxfp4", 5, 2, 21, "ids"), ("mxfp4", 5, 3, 25, "embeds"), ("mxfp4", 8, 3, 25, "ids"), ("mxfp4", 8, 2, 21, "embeds"),
    ("fp8", 5, 3, 25, "ids"), ("fp8", 5, 2, 21, "embeds"), ("fp8", 8, 2, 21, "ids"), ("fp8", 8, 3, 25, "embeds")])
def test_logits_match_the_oracle_on_w_eff(dev, monkeypatch, fmt, B, layers, seed, mode):
    _, _, _, oracle_orig, oracle_eff = _model(fmt, layers, seed)
    eng = _engine(dev, fmt, layers, seed)
    new, old = _counts(monkeypatch)
    inp, ids, am = _inputs(eng, B, seed, mode)
    out = eng.generate(**inp, max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
    assert new["n"] > 0 and old["n"] == 0, "5..8 rows stream the fragment-major bytes and nothing else"
    logits, gen = out.logits.float().cpu(), out.sequences[:, -N:].cpu()
    assert logits.shape == (B, N, V) and set(eng._graphs) == {(B, False, True, 0)}
    ref_eff = [_teacher(oracle_eff, ids[b], am[b], gen[b].tolist()) for b in range(B)]
    for b in range(B):
        rel = _rel(logits[b], ref_eff[b])
        print(f"{fmt} B={B} layers={layers} {mode} row {b}: rel L2 to the oracle on W_eff {rel:.4f}")
        assert rel < BOUND, (b, rel)
    ref_orig = torch.cat([_teacher(oracle_orig, ids[b], am[b], gen[b].tolist()) for b in range(B)])
    sens = _rel(ref_orig, torch.cat(ref_eff))
    print(f"{fmt} B={B} layers={layers} {mode}: oracle(original) to oracle(W_eff) {sens:.4f} = {sens / BOUND:.1f} bounds")
    assert sens >= 3 * BOUND, sens
    assert _rel(logits.reshape(-1, V), ref_orig) > BOUND


@pytest.mark.parametrize("fmt", ["mxfp4", "fp8"])
def test_rows_3_and_4_stay_on_the_row_major_kernels(dev, monkeypatch, fmt):
    eng = _engine(dev, fmt, 2, 21)
    new, old = _counts(monkeypatch)
    for B in (3, 4):
        inp, _, _ = _inputs(eng, B, 21, "ids")
        eng.generate(**inp, max_new_tokens=N)
    assert old["n"] > 0 and new["n"] == 0


@pytest.mark.parametrize("fmt", ["mxfp4", "fp8"])
def test_fm_max_rows_0_is_an_engine_without_the_keyword(dev, monkeypatch, fmt):
    off, plain = _engine(dev, fmt, 2, 21, fm_rows=0), _engine(dev, fmt, 2, 21, stream=False, fm_rows=None)
    new, _ = _counts(monkeypatch)
    kw = dict(max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
    for B in (5, 8):
        inp, _, _ = _inputs(off, B, 21, "ids")
        a, b = off.generate(**inp, **kw), plain.generate(**inp, **kw)
        assert torch.equal(a.sequences, b.sequences) and torch.equal(a.logits, b.logits)
    assert new["n"] == 0


def test_other_request_kinds_run_behind_the_fragment_major_layers(dev, monkeypatch):
    from test_llm_beam_gpu import _check_steps as beam_check_steps, _trace
    from test_llm_sampling_gpu import SAMPLING
    for fmt in ("mxfp4", "fp8"):
        eng = _engine(dev, fmt, 2, 21)
        new, old = _counts(monkeypatch)
        B = 5
        inp, ids, am = _inputs(eng, B, 21, "ids")
        base = dict(max_new_tokens=N, return_dict_in_generate=True, return_logits=True)
        for kw in (dict(base), dict(base, repetition_penalty=1.3), dict(base, do_sample=True, seed=1234567, **SAMPLING)):
            g, e = eng.generate(**inp, **kw), eng.generate(**inp, **kw, use_graph=False)
            assert torch.equal(g.sequences, e.sequences) and torch.equal(g.logits, e.logits), (fmt, sorted(kw))
        # num_beams=4 on 2 prompts (8 rows): every step of the trace passes check_beam_step; graph and eager write the same trace
        inp2, _, _ = _inputs(eng, 2, 21, "ids")
        kw = dict(base, num_beams=4, num_return_sequences=4)
        n0 = new["n"]
        b1 = eng.generate(**inp2, **kw)
        assert new["n"] > n0, "the beam rows stream the fragment-major bytes too"
        tr_g, _ = _trace(eng, 2, 4, 8, N)
        b2 = eng.generate(**inp2, **kw, use_graph=False)
        tr_e, _ = _trace(eng, 2, 4, 8, N)
        assert all(torch.equal(x, y) for x, y in zip(tr_g, tr_e))
        assert torch.equal(b1.sequences, b2.sequences) and torch.equal(b1.sequences_scores, b2.sequences_scores)
        assert len(beam_check_steps(tr_g, b1.logits.cpu(), 2, 4, None)) == N
        assert old["n"] == 0
        assert set(eng._graphs) == {(B, False, True, 0), (B, False, True, 0, True), (B, False, True, 0, "sample"), (2, False, True, 0, "beam", 4, 8)}


def test_old_engines_beside_a_keyword_engine_are_untouched(dev, monkeypatch):
    new_eng = _engine(dev, "mxfp4", 2, 21)
    inp, _, _ = _inputs(new_eng, 5, 21, "ids")
    new_eng.generate(**inp, max_new_tokens=N)                      # the keyword engine has run its kernels before the others are built
    olds = {name: [_engine(dev, name, 2, 21, stream=False, fm_rows=None) for _ in range(2)] for name in ("bf16", "mxfp4")}
    new, _ = _counts(monkeypatch)
    for name, (a, b) in olds.items():
        for lw in a.layers:
            assert set(lw) == t4.BASE_KEYS | t4.FM_KEYS | (t4.Q4_KEYS if name == "mxfp4" else set())
        assert not a.batched_weight_stream
        n0 = new["n"]
        ta = a.generate(**inp, max_new_tokens=N)
        assert new["n"] == n0, name
        new_eng.generate(**inp, max_new_tokens=N)                  # ... and runs them (its captured graph) between the two
        tb = b.generate(**inp, max_new_tokens=N)
        assert new["n"] == n0 and torch.equal(ta, tb), name

"""GPU: LlamaEngine(..., calibration=dict(input_ids=...)) -- MXFP4 codes chosen by GPTQ on the engine's own activations.

The model is tiny (hidden 256, inter 512, 2 layers, 2 q heads, 1 kv head, head_dim 128, vocab 512; LlamaOracle.random_weights seed
31, std 0.02), calibrated on 8 x 128 ids drawn with seed 1031. Storage does not change, so the calibrated engine is held to what
tests/test_llm_mxfp4_gpu.py holds the round-to-nearest engine to: it IS a bf16 model on W_eff.

Mean KL to the unquantised model on the calibration tokens, calibrated / round to nearest: the definition applied to these weights
through transformers' LlamaForCausalLM on the CPU (scripts/exp/gptq_reference_kl.py --seed 31 --std 0.02) gives 0.00383 -> 0.00122,
ratio 0.318. The device ratio has to lie below the midpoint between that and 1, 0.659: it only has to show that the engine applied
what the definition prescribes, so half the reference's gain is the margin."""
import functools
import json
import os

import pytest
import torch

import gptq_cases as GC

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
BOUND = 2.5e-2                  # relative L2 between two encodings of one bf16 model (tests/test_llm_mxfp4_gpu.py)
REF_KL_RATIO = 0.318            # see the module docstring
V, SEED, STD = 512, 31, 0.02
MATS = ("w_qkv", "w_o", "w_gu", "w_down")


@functools.lru_cache(maxsize=None)
def _model():
    from oracle.llama import LlamaCfg, LlamaOracle
    ocfg = LlamaCfg(256, 2, 2, 1, 128, 512, V, 10000.0, None, 1e-6, False, 256)
    w = LlamaOracle.random_weights(ocfg, seed=SEED, std=STD)
    ids = torch.randint(0, V, (8, 128), generator=torch.Generator().manual_seed(1000 + SEED))
    return ocfg, w, ids


def _engine(dev, weight_dtype="mxfp4", lm_head_dtype="mxfp4", calibration=None, weights=None, bws=True, **kw):
    from spider_amd.llm import LlamaEngine, LLMConfig
    ocfg, w, _ = _model()
    return LlamaEngine(LLMConfig(**ocfg.__dict__), w if weights is None else weights, dev, max_batch=8, max_len=160,
                       weight_dtype=weight_dtype, lm_head_dtype=lm_head_dtype,
                       batched_weight_stream=bws and weight_dtype != "bf16", calibration=calibration, **kw)


@functools.lru_cache(maxsize=None)
def _calibrated(dev):
    return _engine(dev, calibration=dict(input_ids=_model()[2]))


def _w_eff_dict(eng):
    """the checkpoint a bf16 engine needs to hold exactly this engine's W_eff"""
    ocfg, w, _ = _model()
    out = {k: v for k, v in w.items()}
    qd, kd = ocfg.n_q * ocfg.head_dim, ocfg.n_kv * ocfg.head_dim
    for l, lw in enumerate(eng.layers):
        p = f"model.layers.{l}."
        q, k, v = lw["w_qkv"].split([qd, kd, kd], 0)
        g, u = lw["w_gu"].split([ocfg.inter, ocfg.inter], 0)
        for name, t in (("self_attn.q_proj", q), ("self_attn.k_proj", k), ("self_attn.v_proj", v), ("self_attn.o_proj", lw["w_o"]),
                        ("mlp.gate_proj", g), ("mlp.up_proj", u), ("mlp.down_proj", lw["w_down"])):
            out[p + name + ".weight"] = t.float().cpu()
    out["lm_head.weight"] = eng.lm_head.float().cpu()
    return out


def _orig(l, key):
    ocfg, w, _ = _model()
    p = f"model.layers.{l}."
    names = {"w_qkv": ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "w_o": ("self_attn.o_proj",),
             "w_gu": ("mlp.gate_proj", "mlp.up_proj"), "w_down": ("mlp.down_proj",)}[key]
    return torch.cat([w[p + n + ".weight"] for n in names], 0)


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _layer0_qkv_reference(eng, ids, am=None):
    """the definition on layer 0's w_qkv with H recomputed here from rmsnorm(embed(ids)), real rows only"""
    from spider_amd import ops
    from spider_amd.llm import quantize_mxfp4_gptq
    x = ops.rmsnorm(eng.embed_tokens(ids).view(-1, eng.cfg.hidden), eng.layers[0]["ln1"], eng.cfg.eps).double().cpu()
    if am is not None:
        x = x[am.reshape(-1) != 0]
    tr = {}
    b, s = quantize_mxfp4_gptq(_orig(0, "w_qkv"), x.t() @ x, trace=tr)
    return b, s, GC.near_tie_rows(tr)


def _check_layer0(eng, ids, am=None):
    b_ref, s_ref, tie = _layer0_qkv_reference(eng, ids, am)
    lw = eng.layers[0]
    ok = (lw["w_qkv_q4"].cpu() == b_ref).all(dim=1) & (lw["w_qkv_e4"].cpu() == s_ref).all(dim=1)
    print(f"layer 0 w_qkv: {int((~ok).sum())} of {ok.numel()} rows differ from the definition, {int(tie.sum())} near-tie rows")
    assert int(tie.sum()) <= GC.NEAR_TIE_CAP * tie.numel()
    assert bool(ok[~tie].all()), torch.nonzero(~ok & ~tie).flatten().tolist()
    return b_ref


def test_calibrated_engine_is_a_bf16_model_on_w_eff(dev):
    from spider_amd import ops
    from spider_amd.llm import dequantize_mxfp4, quantize_mxfp4
    eng = _calibrated(dev)
    assert eng.weight_dtype == "mxfp4" and eng.lm_head_dtype == "mxfp4" and eng.batched_weight_stream
    for l, lw in enumerate(eng.layers):
        for k in MATS:
            n, kk = lw[k].shape
            assert lw[k].dtype == BF and lw[k].is_contiguous() and lw[k + "_q4"].shape == (n, kk // 2) and lw[k + "_e4"].shape == (n, kk // 32)
            assert torch.equal(dequantize_mxfp4(lw[k + "_q4"], lw[k + "_e4"]), lw[k]), (l, k)     # bit for bit
            assert not torch.equal(lw[k + "_q4"].cpu(), quantize_mxfp4(_orig(l, k))[0]), (l, k)  # and not the round-to-nearest codes
            q4fm, e4fm = ops.repack_fm_w4(lw[k + "_q4"], lw[k + "_e4"])                            # the third encoding: built afterwards
            assert torch.equal(lw[k + "_q4fm"], q4fm) and torch.equal(lw[k + "_e4fm"], e4fm)
        if eng.fm_batch:
            assert torch.equal(lw["w_o_fm"], ops.repack_fm16(lw["w_o"])) and torch.equal(lw["w_qkv_fm"], ops.repack_fm16(lw["w_qkv"], lw["ln1"]))
    assert torch.equal(dequantize_mxfp4(eng.lm_head_q4, eng.lm_head_e4), eng.lm_head)
    assert not torch.equal(eng.lm_head_q4.cpu(), quantize_mxfp4(_model()[1]["lm_head.weight"])[0])
    if eng.fm_batch:
        assert torch.equal(eng.lm_head_fm, ops.repack_fm16(eng.lm_head, eng.norm))
    assert float(eng.k_cache.abs().max()) == 0.0 and eng._graphs == {}          # the scratch use left nothing behind
    # the same construction twice gives the same bytes
    again = _engine(dev, calibration=dict(input_ids=_model()[2], damp=0.01))
    assert all(torch.equal(a[k + "_q4"], b[k + "_q4"]) and torch.equal(a[k + "_e4"], b[k + "_e4"]) for a, b in zip(eng.layers, again.layers) for k in MATS)
    assert torch.equal(eng.lm_head_q4, again.lm_head_q4)


@pytest.mark.parametrize("B", [1, 5])
def test_streamed_bytes_decode_like_a_bf16_engine_on_w_eff(dev, monkeypatch, B):
    """1 row: the row-major MXFP4 GEMVs and the MXFP4 lm_head stream the calibrated bytes; 5 rows: the fragment-major MXFP4 kernels"""
    from spider_amd.llm import LlamaEngine
    for name, rows in (("MXFP4_MAX_ROWS", 4), ("LM_HEAD_MXFP4_MAX_ROWS", 3), ("MXFP4_FM_MAX_ROWS", 8)):
        monkeypatch.setattr(LlamaEngine, name, rows)        # the kernels meant, whatever the measured defaults
    from spider_amd import ops
    calls = {"n": 0}
    for name in (("gemv_w4", "gemv_swiglu_w4", "lm_head_argmax_w4") if B == 1 else ("gemv_fm_w4", "gemv_swiglu_fm_w4")):
        def wrapped(*a, _real=getattr(ops, name), **kw):
            calls["n"] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    eng = _calibrated(dev)
    bf = _engine(dev, "bf16", "bf16", weights=_w_eff_dict(eng))
    assert all(torch.equal(a[k], b[k]) for a, b in zip(eng.layers, bf.layers) for k in MATS) and torch.equal(eng.lm_head, bf.lm_head)
    ids = torch.randint(3, V, (B, 9), generator=torch.Generator().manual_seed(7))
    kw = dict(input_ids=ids, max_new_tokens=16, return_dict_in_generate=True, return_logits=True)
    a = eng.generate(**kw)
    assert calls["n"] > 0, "the step streams the calibrated bytes"
    n_streamed = calls["n"]
    b = bf.generate(**kw)
    assert calls["n"] == n_streamed
    la, lb, ga, gb = a.logits.float().cpu(), b.logits.float().cpu(), a.sequences[:, -16:].cpu(), b.sequences[:, -16:].cpu()
    for r in range(B):
        same = (ga[r] == gb[r]).long().cumprod(0)       # the same history up to and including the first differing token (a near-tie)
        n = min(16, int(same.sum()) + 1)
        rel = _rel(la[r, :n], lb[r, :n])
        print(f"B={B} row {r}: {n} common steps, rel L2 between the encodings {rel:.4f}")
        assert rel < BOUND, (r, n, rel)
    # with the byte streams switched off the calibrated engine runs the bf16 engine's kernels on the bf16 engine's weights: bit for bit
    off = _engine(dev, calibration=dict(input_ids=_model()[2]), bws=False)
    off.MXFP4_MAX_ROWS = off.LM_HEAD_MXFP4_MAX_ROWS = 0
    c = off.generate(**kw)
    assert torch.equal(c.sequences, b.sequences) and torch.equal(c.logits, b.logits)


def test_every_matrix_is_recorded_with_a_smaller_proxy_loss(dev):
    eng = _calibrated(dev)
    cal = eng.calibration
    assert cal["method"] == "gptq" and cal["n_tokens"] == 8 * 128 and cal["damp"] == 0.01
    assert [(l, k) for l, k, _, _ in cal["matrices"]] == [(l, k) for l in range(2) for k in MATS] + [(None, "lm_head")]
    for l, k, p_rtn, p_gptq in cal["matrices"]:
        print(f"layer {l} {k}: proxy loss round to nearest {p_rtn:.5f}, calibrated {p_gptq:.5f}")
        assert 0 < p_gptq < p_rtn, (l, k)


def test_layer0_qkv_bytes_are_the_definitions(dev):
    _check_layer0(_calibrated(dev), _model()[2])


def test_mean_kl_on_the_calibration_tokens(dev):
    ids = _model()[2]
    bf, rtn, cal = _engine(dev, "bf16", "bf16"), _engine(dev), _calibrated(dev)
    kl_rtn = float(rtn.score(input_ids=ids, other=bf).mean_kl)
    kl_cal = float(cal.score(input_ids=ids, other=bf).mean_kl)
    print(f"mean KL to the bf16 engine on the calibration tokens: round to nearest {kl_rtn:.5f}, calibrated {kl_cal:.5f}, ratio "
          f"{kl_cal / kl_rtn:.3f} (CPU reference {REF_KL_RATIO}, bound {(REF_KL_RATIO + 1) / 2:.3f})")
    assert kl_cal / kl_rtn < (REF_KL_RATIO + 1) / 2


def test_left_padding_keeps_padded_rows_out_of_the_hessians(dev):
    ids = _model()[2].clone()
    am = torch.ones_like(ids)
    am[1, :37] = 0
    am[6, :5] = 0
    ids[am == 0] = 0
    masked = _engine(dev, lm_head_dtype="bf16", calibration=dict(input_ids=ids, attention_mask=am), bws=False)
    plain = _engine(dev, lm_head_dtype="bf16", calibration=dict(input_ids=ids), bws=False)
    assert masked.calibration["n_tokens"] == 8 * 128 - 42 and plain.calibration["n_tokens"] == 8 * 128
    assert not torch.equal(masked.layers[0]["w_qkv_q4"], plain.layers[0]["w_qkv_q4"])
    b_ref = _check_layer0(masked, ids, am)
    assert not torch.equal(plain.layers[0]["w_qkv_q4"].cpu(), b_ref)
    assert [(l, k) for l, k, _, _ in masked.calibration["matrices"]] == [(l, k) for l in range(2) for k in MATS]      # (bf16 head: not listed)


def test_default_is_unchanged(dev):
    from spider_amd.llm import quantize_mxfp4
    a, b = _engine(dev), _engine(dev, calibration=None)
    cal = _calibrated(dev)
    assert a.calibration is None and b.calibration is None
    assert set(vars(a)) == set(vars(b)) == set(vars(cal))           # no attribute comes or goes with the keyword
    for l, (la, lc) in enumerate(zip(a.layers, cal.layers)):
        assert set(la) == set(lc)
        for k in MATS:
            q, sc = quantize_mxfp4(_orig(l, k))
            assert torch.equal(la[k + "_q4"].cpu(), q) and torch.equal(la[k + "_e4"].cpu(), sc)
    q, sc = quantize_mxfp4(_model()[1]["lm_head.weight"])
    assert torch.equal(a.lm_head_q4.cpu(), q) and torch.equal(a.lm_head_e4.cpu(), sc)
    ids = torch.randint(3, V, (1, 9), generator=torch.Generator().manual_seed(7))
    assert torch.equal(a.generate(input_ids=ids, max_new_tokens=8), b.generate(input_ids=ids, max_new_tokens=8))
    assert set(a._graphs) == {(1, False, False, 0)} == set(b._graphs)


def test_keyword_is_on_the_three_constructors():
    import inspect
    from spider_amd.llm import LlamaEngine
    for fn in (LlamaEngine.__init__, LlamaEngine.random_init, LlamaEngine.from_pretrained):
        p = inspect.signature(fn).parameters
        assert p["calibration"].default is None and list(p)[-2:] == ["lm_head_dtype", "batched_weight_stream"]


def test_calibration_needs_an_mxfp4_part(dev):
    cal = dict(input_ids=_model()[2])
    for wd, hd in (("bf16", "bf16"), ("fp8", "bf16"), ("fp8", "fp8"), ("bf16", "fp8")):
        with pytest.raises(ValueError, match="mxfp4"):
            _engine(dev, wd, hd, calibration=cal)
    with pytest.raises(ValueError, match="max_len"):
        _engine(dev, calibration=dict(input_ids=torch.zeros(1, 161, dtype=torch.long)))
    with pytest.raises(ValueError, match="input_ids"):
        _engine(dev, calibration=dict(input_ids=_model()[2] + V))
    # FP8 layers keep quantize_fp8_rows; only the MXFP4 head is calibrated, on the Hessian behind those layers
    from spider_amd.llm import quantize_fp8_rows
    mixed = _engine(dev, "fp8", "mxfp4", calibration=cal)
    assert torch.equal(mixed.layers[1]["w_down_q8"].cpu().view(torch.uint8), quantize_fp8_rows(_orig(1, "w_down").to(BF))[0].view(torch.uint8))
    assert [(l, k) for l, k, _, _ in mixed.calibration["matrices"]] == [(None, "lm_head")]
    assert mixed.calibration["matrices"][0][3] < mixed.calibration["matrices"][0][2]
    with pytest.raises(ValueError, match="calibrated"):
        mixed.resize_token_embeddings(V + 8)


def test_from_pretrained_passes_the_keyword_through(dev, tmp_path):
    from safetensors.torch import save_file
    from spider_amd.llm import LlamaEngine
    ocfg, w, ids = _model()
    d = str(tmp_path / "llm")
    os.makedirs(d)
    json.dump({"architectures": ["LlamaForCausalLM"], "model_type": "llama", "hidden_size": 256, "num_hidden_layers": 2,
               "num_attention_heads": 2, "num_key_value_heads": 1, "head_dim": 128, "intermediate_size": 512, "vocab_size": V,
               "rope_theta": 10000.0, "rms_norm_eps": 1e-6, "max_position_embeddings": 256, "tie_word_embeddings": False,
               "attention_bias": False, "torch_dtype": "bfloat16"}, open(os.path.join(d, "config.json"), "w"))
    save_file({k: v.bfloat16().contiguous() for k, v in w.items()}, os.path.join(d, "model.safetensors"))
    eng = LlamaEngine.from_pretrained(d, dev, max_batch=8, max_len=160, weight_dtype="mxfp4", lm_head_dtype="mxfp4",
                                      batched_weight_stream=True, calibration=dict(input_ids=ids))
    ref = _calibrated(dev)
    assert eng.calibration["n_tokens"] == 1024 and eng.calibration["matrices"] == ref.calibration["matrices"]
    assert all(torch.equal(a[k + "_q4"], b[k + "_q4"]) for a, b in zip(eng.layers, ref.layers) for k in MATS)
    assert torch.equal(eng.lm_head_q4, ref.lm_head_q4)
    assert LlamaEngine.from_pretrained(d, dev, max_batch=1, max_len=64, weight_dtype="mxfp4").calibration is None

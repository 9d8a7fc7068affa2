"""Native LLM engine: greedy autoregressive decode on the HIP kernels (no transformers / torch math).

Drop-in for the reference's LLM seam B3:
    llama_model.generate(inputs_embeds | input_ids, attention_mask, max_new_tokens, num_beams=1,
                         do_sample=False, use_cache=True, stopping_criteria, output_hidden_states,
                         return_dict_in_generate, output_attentions)      spider/models/spider.py:1492-1508
    -> .sequences  [B, T_new] (generated tokens only for an inputs_embeds call, prompt + generated for
                   input_ids -- HF semantics the reference relies on, spider.py:1428-1449)
    -> .hidden_states[step][layer]  [B, S|1, H]
    embed_tokens(ids)                                                     spider/models/base_model.py:253-258
Arithmetic follows spider/models/modeling_llama3.py:68-313 (Llama-3 GQA + rope scaling) and the Qwen2.5
text decoder (qkv bias) that qwen2.5omni_spider_web.py:468 drives.

Data layout in HBM (per engine):
    embed  [V, H] bf16 | per layer: w_qkv [(n_q+2n_kv)d, H], b_qkv?, w_o [H, n_q d], w_gate_up [2I, H],
    w_down [H, I], ln1 [H], ln2 [H] | norm [H] | lm_head [V, H]
    KV cache: 2 x [L, B_max, n_kv, T_max, d] bf16, preallocated once; rope table [max_pos, d] fp32.
Decode = 5 weight-streaming launches per layer (+1 tiny split-KV combine), captured in a hipGraph.

Logits processors (opt-in keywords of generate: repetition_penalty, min_length / min_new_tokens, suppress_tokens, single-token
bad_words_ids -- what spider.py:1471-1508 and conversation.py:151-172 forward to HF's generate) run in the arg-max epilogue of the
lm_head kernels on per-sequence token bitmaps kept in the decode state; neutral values use the unprocessed kernels and graph.

Beam search (num_beams 2..8, with length_penalty / early_stopping / num_return_sequences): the beam step of transformers'
`_beam_search` -- log-softmax of the raw logits, the best continuations of a batch row's K beams, the KV-cache reorder -- is three
launches behind the lm_head inside the captured decode graph (csrc/beam_search.hip); `beam_finalize_host` replays HF's
finished-hypotheses bookkeeping on the trace the device wrote. num_beams=1 is the greedy path, unchanged.

Sampling (do_sample=True with temperature / top_k 1..64 / top_p / seed, as conversation.py:151-173 calls generate): behind the
raw-logits lm_head two launches (csrc/sample.hip) apply the processors, keep the top_k best, cut the nucleus and draw with a
counter-based generator, inside the captured decode graph; `sample_token_host` / `sample_uniform_host` are the definition.

Prompt-lookup decoding (prompt_lookup_num_tokens=K, max_matching_ngram_size=N; one greedy sequence): the decode step runs at K + 1
rows -- the last accepted token and K tokens drafted from an earlier occurrence of the sequence's last n-gram -- with the R-row
weight streams, rope_kv_append(S = R) and a verify attention in which row r sees r more cache rows; one launch accepts the agreed
prefix, appends it and drafts the next step (csrc/spec_decode.hip). `prompt_lookup_draft_host` / `spec_accept_host` are the definition.

Assisted decoding (assistant_model=draft_engine, num_assistant_tokens=K; one greedy sequence): the drafts come from a second, smaller
LlamaEngine instead. A round is one two-row step of the draft engine (catch-up + first draft), K - 1 single-row steps, the target's
verify step on K + 1 rows and two kinds of small launches that carry tokens and cursors between the engines (csrc/spec_assist.hip);
it has no host sync and is captured as one graph. `assisted_round_host` is the definition.
"""
from __future__ import annotations

import os
import math
from collections import namedtuple
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import torch

from . import ops
from .graphs import capture as capture_graph

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn       # OCP e4m3fn: max 448 (byte 0x7e), 1.0 = 0x38 -- the FP8 of gfx950, not MI300's e4m3fnuz
FP8_MAX = 448.0
WEIGHT_DTYPES = ("bf16", "fp8", "mxfp4")
MX_BLOCK = 32                   # weights per E8M0 scale of the OCP Microscaling formats
FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # e2m1 magnitudes by code & 7; bit 3 of the code is the sign


def resolve_weight_dtype(weight_dtype) -> str:
    """`weight_dtype` of LlamaEngine: "bf16" (default), "fp8" (weight-only e4m3 stream for the decode GEMVs) or "mxfp4"
    (weight-only e2m1 stream with one E8M0 scale per block of 32)"""
    if weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype has to be one of {WEIGHT_DTYPES}, but is {weight_dtype!r}")
    return weight_dtype


def resolve_lm_head_dtype(lm_head_dtype) -> str:
    """`lm_head_dtype` of LlamaEngine: "bf16" (default), "fp8" or "mxfp4" (weight-only stream of the lm_head at decode, in the
    formats of `weight_dtype` and independent of it)"""
    if lm_head_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"lm_head_dtype has to be one of {WEIGHT_DTYPES}, but is {lm_head_dtype!r}")
    return lm_head_dtype


def quantize_fp8_rows(W: torch.Tensor):
    """Per-row weight-only FP8: W [N, K] -> (q [N, K] float8_e4m3fn, scale [N] float32) with
        scale[n] = 2^ceil(log2(max|W[n, :]| / 448))   (1.0 for an all-zero row),   q[n, :] = fp8(W[n, :] / scale[n]).
    The scale is a power of two on purpose: e4m3 has 3 mantissa bits, so W_eff = float(q) * scale is a bf16 number, and a
    power-of-two factor commutes with every fp32 rounding. A model quantised this way IS a bf16 model with weights W_eff:
    kernels that stream q and scale the fp32 dot product by scale[n] compute, up to summation order, what the bf16 kernels
    compute on W_eff. The relative precision of e4m3 does not depend on the scale, so the restriction costs no accuracy.
    Pure torch; runs wherever W lives."""
    if W.dim() != 2:
        raise ValueError(f"quantize_fp8_rows: expected a [N, K] matrix, got {tuple(W.shape)}")
    Wf = W.detach().float()
    amax = Wf.abs().amax(dim=1)
    # no rounded logarithm or division: amax = m * 2^e with m in [0.5, 1) and 448 = 0.875 * 2^9, so amax / 448 = (m / 0.875) * 2^(e - 9)
    # lies in (0.5, 1] * 2^(e - 9) when m <= 0.875 and in (1, 1.15) * 2^(e - 9) otherwise
    m, e = torch.frexp(amax)
    e = (e - 9 + (m > 0.875).to(e.dtype)).clamp(-126, 127)    # a normal fp32 power of two (rows below 448 * 2^-126 lose range)
    scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax))
    q = (Wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return q, scale


def dequantize_fp8_rows(q: torch.Tensor, scale: torch.Tensor, dtype=BF16) -> torch.Tensor:
    """W_eff = float(q) * scale[:, None] in `dtype` (exact in bf16 for the scales of quantize_fp8_rows)"""
    return (q.float() * scale.float()[:, None]).to(dtype)


dequantize = dequantize_fp8_rows


def quantize_mxfp4(W: torch.Tensor):
    """Weight-only OCP MXFP4: W [N, K], K % 32 == 0 -> (blocks uint8 [N, K / 2], scales uint8 [N, K / 32]).
    Byte j of row n holds weight 2 j in its low nibble and weight 2 j + 1 in its high nibble; a nibble code c has sign bit 3 and
    magnitude FP4_VALUES[c & 7]. Block g of row n (weights 32 g .. 32 g + 31) is multiplied by 2^(scales[n, g] - 127) (E8M0).
    This is the layout of transformers.integrations.mxfp4 (FP4_VALUES, low nibble first, scales - 127, ldexp).
        scale = 2^ceil(log2(amax / 6))  per block (byte 127 for an all-zero block; the exponent is clamped to [-125, 125], bytes
        2 .. 252, so that every non-zero W_eff is a normal, finite bf16 number), which is quantize_fp8_rows' rule with e2m1's largest
        value: no element saturates, and amax / scale lies in (3, 6] for every non-zero block.
        Elements are rounded to nearest on the e2m1 grid, ties to the even significand: |v| / scale = 0.25, 0.75, 1.25, 1.75, 2.5,
        3.5, 5 round to 0, 1, 1, 2, 2, 4, 4. The sign is kept (-0 is a legal code).
    e2m1 has two significand bits and the scale is a power of two, so W_eff = dequantize_mxfp4(blocks, scales) is a bf16 matrix and
    a model quantised this way IS a bf16 model with weights W_eff, as with quantize_fp8_rows. Quantising W_eff again returns W_eff,
    but not always the same bytes: a block whose largest element lies in (3, 3.5) * scale rounds down to 3 * scale and then
    requantises as (2 q, scale / 2). Round-to-nearest MXFP4 is coarse: ||W_eff - W|| / ||W|| = 11.8 % on N(0, 0.02^2) rows, where
    quantize_fp8_rows has 2.6 %. Pure torch; runs wherever W lives."""
    if W.dim() != 2 or W.shape[1] % MX_BLOCK:
        raise ValueError(f"quantize_mxfp4: expected a [N, K] matrix with K % {MX_BLOCK} == 0, got {tuple(W.shape)}")
    N, K = W.shape
    Wf = W.detach().float().reshape(N, K // MX_BLOCK, MX_BLOCK)
    amax = Wf.abs().amax(dim=2)
    if not bool(torch.isfinite(amax).all()) or bool((amax > 6.0 * 2.0 ** 125).any()):
        raise ValueError("quantize_mxfp4: entries have to be finite and at most 6 * 2^125 in magnitude")
    # no rounded logarithm or division: amax = m * 2^e with m in [0.5, 1) and 6 = 0.75 * 2^3, so amax / 6 = (m / 0.75) * 2^(e - 3)
    # lies in (2/3, 1] * 2^(e - 3) when m <= 0.75 and in (1, 4/3) * 2^(e - 3) otherwise
    m, e = torch.frexp(amax)
    e = (e - 3 + (m > 0.75).to(e.dtype)).clamp(-125, 125)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    a = Wf.abs() / torch.ldexp(torch.ones_like(amax), e)[:, :, None]     # exact: a power of two (a result below 2^-126 rounds to code 0 either way)
    # code = number of midpoints passed; a tie goes up exactly when the upper neighbour has the even code
    code = torch.zeros_like(a, dtype=torch.uint8)
    for i, mid in enumerate((0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)):
        code += ((a >= mid) if i & 1 else (a > mid)).to(torch.uint8)
    code = (code | (torch.signbit(Wf).to(torch.uint8) << 3)).reshape(N, K // 2, 2)
    blocks = code[:, :, 0] | (code[:, :, 1] << 4)
    return blocks.contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4(blocks: torch.Tensor, scales: torch.Tensor, dtype=BF16) -> torch.Tensor:
    """W_eff [N, K] in `dtype` from blocks uint8 [N, K / 2] and scales uint8 [N, K / 32] (layout: quantize_mxfp4); exact in bf16
    for scale bytes 2 .. 252"""
    if blocks.dim() != 2 or scales.dim() != 2 or blocks.dtype != torch.uint8 or scales.dtype != torch.uint8 \
            or blocks.shape[1] % (MX_BLOCK // 2) or tuple(scales.shape) != (blocks.shape[0], blocks.shape[1] // (MX_BLOCK // 2)):
        raise ValueError(f"dequantize_mxfp4: expected uint8 blocks [N, K / 2] and scales [N, K / 32], got {tuple(blocks.shape)} "
                         f"{blocks.dtype} and {tuple(scales.shape)} {scales.dtype}")
    N, K = blocks.shape[0], blocks.shape[1] * 2
    table = torch.tensor(FP4_VALUES + tuple(-v for v in FP4_VALUES), dtype=torch.float32, device=blocks.device)
    codes = torch.stack([blocks & 15, blocks >> 4], dim=2).reshape(N, K // MX_BLOCK, MX_BLOCK)
    vals = table[codes.long()]
    return torch.ldexp(vals, (scales.to(torch.int32) - 127)[:, :, None]).reshape(N, K).to(dtype)


FP4_MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)     # between neighbouring FP4_VALUES; odd positions round up on a tie


def gptq_prepare(W: torch.Tensor, H: torch.Tensor, damp: float = 0.01, who: str = "quantize_mxfp4_gptq"):
    """Steps 1 - 3 of `quantize_mxfp4_gptq`: validate, clear dead inputs, damp. Returns fp64 copies (W [N, K], H [K, K]) on W's
    device; a violation raises ValueError naming the argument."""
    if not isinstance(W, torch.Tensor) or W.dim() != 2 or W.shape[1] % MX_BLOCK or W.numel() == 0 or not W.is_floating_point():
        raise ValueError(f"{who}: W has to be a floating-point [N, K] matrix with K % {MX_BLOCK} == 0, got "
                         f"{tuple(W.shape) if isinstance(W, torch.Tensor) else type(W)}")
    N, K = W.shape
    if not isinstance(H, torch.Tensor) or tuple(H.shape) != (K, K) or not H.is_floating_point():
        raise ValueError(f"{who}: H has to be a floating-point [{K}, {K}] matrix (sum of x x^T over the layer's inputs), got "
                         f"{tuple(H.shape) if isinstance(H, torch.Tensor) else type(H)}")
    if isinstance(damp, bool) or not isinstance(damp, (int, float)) or not math.isfinite(damp) or damp <= 0:
        raise ValueError(f"{who}: damp has to be a finite number > 0, but is {damp!r}")
    Wd = W.detach().to(torch.float64).clone()
    Hd = H.detach().to(device=W.device, dtype=torch.float64).clone()
    if not bool(torch.isfinite(Wd).all()) or bool((Wd.abs() > 6.0 * 2.0 ** 125).any()):
        raise ValueError(f"{who}: W: entries have to be finite and at most 6 * 2^125 in magnitude")
    if not bool(torch.isfinite(Hd).all()):
        raise ValueError(f"{who}: H: entries have to be finite")
    if float((Hd - Hd.t()).abs().max()) > 1e-5 * float(Hd.abs().max()):
        raise ValueError(f"{who}: H has to be symmetric")
    d = torch.diagonal(Hd)
    if bool((d < 0).any()):
        raise ValueError(f"{who}: H: the diagonal of a sum of x x^T cannot be negative")
    dead = d == 0
    d[dead] = 1.0                      # (a view: writes H's diagonal)
    Wd[:, dead] = 0.0
    d += float(damp) * float(d.mean())
    return Wd, Hd


def gptq_factor(Hd: torch.Tensor, who: str = "quantize_mxfp4_gptq") -> torch.Tensor:
    """U [K, K] fp64, upper triangular with H^-1 = U^T U (step 4), by cholesky -> cholesky_inverse -> cholesky(upper), on Hd's device"""
    L, info = torch.linalg.cholesky_ex(Hd)
    if int(info) != 0:
        raise ValueError(f"{who}: H is not positive definite after damping (it has to be a sum of x x^T)")
    U, info = torch.linalg.cholesky_ex(torch.cholesky_inverse(L), upper=True)
    if int(info) != 0:
        raise ValueError(f"{who}: H is too ill-conditioned to factor its inverse; raise damp")
    return U


def quantize_mxfp4_gptq(W: torch.Tensor, H: torch.Tensor, damp: float = 0.01, trace: Optional[dict] = None):
    """Calibrated MXFP4 (GPTQ: Frantar et al. 2022, on MX blocks): W [N, K], H [K, K] = sum x x^T over the inputs the matrix sees
    -> (blocks uint8 [N, K / 2], scales uint8 [N, K / 32]) in `quantize_mxfp4`'s layout. The codes are chosen column by column
    along K; each column's rounding error is pushed into the columns not yet quantised, weighted by the inverse Hessian, so that
    ||X (W - Q)^T|| shrinks where plain rounding minimises ||W - Q||. In fp64, every row independently:
      1. W [N, K] with K % 32 == 0, H [K, K] finite and symmetric, damp > 0 (else ValueError naming the argument).
      2. dead inputs: where H[k, k] == 0, H[k, k] = 1 and W[:, k] = 0.       3. H += damp * mean(diag H) * I.
      4. U = the upper Cholesky factor of H^-1 (H^-1 = U^T U).
      5. per block g (columns j = 32 g .. 32 g + 31), in order:
         scale: `quantize_mxfp4`'s exponent rule on the amax of the block's CURRENT (already compensated) weights;
         for i = 0 .. 31 in order: a = |w_i| / s, code by `quantize_mxfp4`'s midpoint rule (a > 6 can occur now and saturates at
         code 7), sign bit from w_i, q = +-value * s;  e_i = (w_i - q) / U[j+i, j+i];  w_i' -= e_i U[j+i, j+i'] for i < i' <= 31;
         then W[:, j+32:] -= E U[j:j+32, j+32:] with E = [e_0 .. e_31].
    A diagonal H leaves nothing to compensate and returns `quantize_mxfp4(W)`'s bytes (a weight that is exactly -0.0 may come out
    as +0.0); `dequantize_mxfp4` of the result is a bf16 matrix as before. What it costs: the plain weight error ||W - Q|| / ||W||
    goes UP (11.4 % -> 13.5 % on N(0, 0.02^2) rows under correlated inputs), and on inputs unlike the calibration set the output
    error can exceed round-to-nearest's. Pure torch; runs wherever W lives (`ops.gptq_mxfp4` is the device form in fp32).
    trace: a dict that receives, per row, how close this fp64 run came to a decision another precision could take differently:
    `mid_gap` [N] = min over the row's weights of |a - midpoint| / max(1, midpoint), and `mant_gap` [N] = min over the row's
    non-zero blocks of |m - 0.75| (m the frexp mantissa of the block's amax)."""
    Wd, Hd = gptq_prepare(W, H, damp)
    U = gptq_factor(Hd)
    N, K = Wd.shape
    mids = torch.tensor(FP4_MIDPOINTS, dtype=torch.float64, device=Wd.device)
    up = torch.tensor([i & 1 for i in range(7)], dtype=torch.bool, device=Wd.device)
    table = torch.tensor(FP4_VALUES, dtype=torch.float64, device=Wd.device)
    codes = torch.empty(N, K, dtype=torch.uint8, device=Wd.device)
    scales = torch.empty(N, K // MX_BLOCK, dtype=torch.uint8, device=Wd.device)
    E = torch.empty(N, MX_BLOCK, dtype=torch.float64, device=Wd.device)
    mid_gap = torch.full((N,), float("inf"), dtype=torch.float64, device=Wd.device)
    mant_gap = mid_gap.clone()
    for g in range(K // MX_BLOCK):
        j = g * MX_BLOCK
        Wb = Wd[:, j:j + MX_BLOCK]
        amax = Wb.abs().amax(dim=1)
        m, e = torch.frexp(amax)
        e = (e - 3 + (m > 0.75).to(e.dtype)).clamp(-125, 125)
        e = torch.where(amax > 0, e, torch.zeros_like(e))
        s = torch.ldexp(torch.ones_like(amax), e)
        scales[:, g] = (e + 127).to(torch.uint8)
        mant_gap = torch.minimum(mant_gap, torch.where(amax > 0, (m - 0.75).abs(), mant_gap))
        for i in range(MX_BLOCK):
            w = Wb[:, i].clone()
            a = (w.abs() / s)[:, None]
            c = (torch.where(up, a >= mids, a > mids)).sum(dim=1)
            mid_gap = torch.minimum(mid_gap, ((a - mids).abs() / mids.clamp(min=1.0)).amin(dim=1))
            q = torch.copysign(table[c] * s, w)
            codes[:, j + i] = c.to(torch.uint8) | (torch.signbit(w).to(torch.uint8) << 3)
            E[:, i] = (w - q) / U[j + i, j + i]
            if i + 1 < MX_BLOCK:
                Wb[:, i + 1:] -= E[:, i:i + 1] * U[j + i, j + i + 1:j + MX_BLOCK][None]
        if j + MX_BLOCK < K:
            Wd[:, j + MX_BLOCK:] -= E @ U[j:j + MX_BLOCK, j + MX_BLOCK:]
    if trace is not None:
        trace["mid_gap"], trace["mant_gap"] = mid_gap, mant_gap
    codes = codes.reshape(N, K // 2, 2)
    return (codes[:, :, 0] | (codes[:, :, 1] << 4)).contiguous(), scales.contiguous()


def gptq_proxy_loss(W: torch.Tensor, Q: torch.Tensor, H: torch.Tensor) -> float:
    """tr((W - Q) H (W - Q)^T) / tr(W H W^T) in fp64: the squared relative output error ||X (W - Q)^T||^2 / ||X W^T||^2 over the
    inputs X that H = X^T X sums (the layer-wise objective GPTQ minimises)"""
    Hd = H.detach().to(device=W.device, dtype=torch.float64)
    Wd = W.detach().to(torch.float64)
    D = Wd - Q.detach().to(device=W.device, dtype=torch.float64)
    den = float(((Wd @ Hd) * Wd).sum())
    return float(((D @ Hd) * D).sum()) / den if den > 0 else 0.0


def resolve_calibration(calibration, vocab: int, max_len: int, weight_dtype: str = "bf16", lm_head_dtype: str = "bf16"):
    """`calibration` of LlamaEngine, checked on the host: None (no calibration; returns None), or a dict with `input_ids` [n, S]
    (integer, ids in [0, vocab), S <= max_len), optionally `attention_mask` [n, S] (LEFT padding, as in prefill_begin) and `damp`
    (default 0.01). At least one of weight_dtype / lm_head_dtype has to be "mxfp4". A violation raises ValueError naming the
    field. Returns dict(input_ids int64 [n, S], attention_mask int64 [n, S] or None, damp float, n_tokens int) on the host."""
    if calibration is None:
        return None
    if not isinstance(calibration, dict):
        raise ValueError(f"calibration has to be None or a dict with input_ids (and attention_mask, damp), but is {type(calibration).__name__}")
    if "mxfp4" not in (weight_dtype, lm_head_dtype):
        raise ValueError("calibration needs weight_dtype='mxfp4' or lm_head_dtype='mxfp4' (it chooses MXFP4 codes; FP8 and bf16 parts "
                         "have nothing to calibrate)")
    extra = sorted(set(calibration) - {"input_ids", "attention_mask", "damp"})
    if extra:
        raise ValueError(f"calibration: unknown field(s) {extra}; the fields are input_ids, attention_mask, damp")
    ids = calibration.get("input_ids")
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64) or ids.numel() == 0:
        raise ValueError("calibration: input_ids is required: a non-empty integer tensor [n, S]")
    ids = ids.detach().cpu().to(torch.int64)
    n, S = ids.shape
    if int(ids.min()) < 0 or int(ids.max()) >= vocab:
        raise ValueError(f"calibration: input_ids must be in [0, {vocab})")
    if S > max_len:
        raise ValueError(f"calibration: input_ids: length {S} exceeds max_len {max_len}")
    am = calibration.get("attention_mask")
    if am is not None:
        if not isinstance(am, torch.Tensor) or tuple(am.shape) != (n, S):
            raise ValueError(f"calibration: attention_mask must be [{n}, {S}]")
        am = (am.detach().cpu() != 0).to(torch.int64)
        if bool((am[:, 1:] < am[:, :-1]).any()) or bool((am[:, -1] == 0).any()):
            raise ValueError("calibration: attention_mask must describe LEFT padding: zeros, then ones up to the last position of every row")
    damp = calibration.get("damp", 0.01)
    if isinstance(damp, bool) or not isinstance(damp, (int, float)) or not math.isfinite(damp) or damp <= 0:
        raise ValueError(f"calibration: damp has to be a finite number > 0, but is {damp!r}")
    return dict(input_ids=ids, attention_mask=am, damp=float(damp), n_tokens=int(am.sum()) if am is not None else n * S)


@dataclass
class LLMConfig:
    hidden: int
    layers: int
    n_q: int
    n_kv: int
    head_dim: int
    inter: int
    vocab: int
    rope_theta: float = 10000.0
    rope_scaling: Optional[dict] = None
    eps: float = 1e-6
    qkv_bias: bool = False
    max_pos: int = 8192
    tie_embeddings: bool = False
    mrope_section: Optional[tuple] = None   # Qwen2.5-Omni thinker: (16, 24, 24) rotary pairs follow (t, h, w) positions

    @staticmethod
    def llama3_8b():   # DeepSeek-R1-Distill-Llama-8B (r1_llama3_8B_infer.py:4, demo/inference_api.py:92-95)
        return LLMConfig(4096, 32, 32, 8, 128, 14336, 128256, 500000.0,
                         dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                              original_max_position_embeddings=8192), 1e-5, False, 8192)

    @staticmethod
    def qwen25_7b():   # Qwen2.5-Omni-7B thinker text decoder (qwen2.5omni_spider_web.py:368-384)
        return LLMConfig(3584, 28, 28, 4, 128, 18944, 152064, 1000000.0, None, 1e-6, True, 8192, False, (16, 24, 24))

    @staticmethod
    def from_hf_dict(c: dict) -> "LLMConfig":
        if "thinker_config" in c:  # Qwen2.5-Omni nests the text decoder config
            c = c["thinker_config"].get("text_config", c["thinker_config"])
        hd = c.get("head_dim") or c["hidden_size"] // c["num_attention_heads"]
        return LLMConfig(c["hidden_size"], c["num_hidden_layers"], c["num_attention_heads"],
                         c.get("num_key_value_heads", c["num_attention_heads"]), hd, c["intermediate_size"],
                         c["vocab_size"], float(c.get("rope_theta", 10000.0)), c.get("rope_scaling"),
                         float(c.get("rms_norm_eps", 1e-6)),
                         bool(c.get("attention_bias", c.get("model_type", "").startswith("qwen"))),
                         int(c.get("max_position_embeddings", 8192)), bool(c.get("tie_word_embeddings", False)),
                         tuple((c.get("rope_scaling") or {}).get("mrope_section") or ()) or None)


def rope_inv_freq(cfg: LLMConfig) -> torch.Tensor:
    """fp32 inverse frequencies incl. llama3 scaling (modeling_llama3.py:91-113 -> ROPE_INIT_FUNCTIONS)."""
    d = cfg.head_dim
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, d, 2, dtype=torch.int64).float() / d))
    rs = cfg.rope_scaling
    if rs and rs.get("rope_type", rs.get("type")) == "llama3":
        factor, lo, hi = rs["factor"], rs["low_freq_factor"], rs["high_freq_factor"]
        old = rs["original_max_position_embeddings"]
        wl = 2 * math.pi / inv
        inv_l = torch.where(wl > old / lo, inv / factor, inv)
        smooth = (old / wl - lo) / (hi - lo)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        mid = ~(wl < old / hi) * ~(wl > old / lo)
        inv = torch.where(mid, smoothed, inv_l)
    return inv


def rope_table(cfg: LLMConfig, n_pos: int) -> torch.Tensor:
    fr = torch.outer(torch.arange(n_pos, dtype=torch.float32), rope_inv_freq(cfg))
    return torch.cat([fr.cos(), fr.sin()], dim=-1).contiguous()


def read_generation_config(path: str) -> dict:
    """The defaults HF `generate` takes from the checkpoint when the caller passes none (the reference's
    `model.generate(**inputs, spk=..., use_audio_in_video=True)`, qwen2.5omni_spider_web.py:468, and
    `r1_llama3_8B_chat.py:14` rely on them): eos_token_id (int or list), pad_token_id, max_new_tokens / max_length,
    and Qwen2.5-Omni's thinker_max_new_tokens. generation_config.json wins over config.json, as in transformers."""
    import json
    gc: dict = {}
    for name in ("config.json", "generation_config.json"):
        f = os.path.join(path, name)
        if not os.path.exists(f):
            continue
        d = json.load(open(f))
        srcs = [d]
        if name == "config.json" and "thinker_config" in d:
            srcs += [d["thinker_config"], d["thinker_config"].get("text_config", {})]
        for src in srcs:
            for k in ("eos_token_id", "pad_token_id", "bos_token_id", "max_new_tokens", "max_length",
                      "thinker_max_new_tokens", "thinker_eos_token_id"):
                if src.get(k) is not None:
                    gc[k] = src[k]
    return gc


def _id_list(v) -> Optional[List[int]]:
    if v is None:
        return None
    return [int(v)] if isinstance(v, int) else [int(x) for x in v]


MAX_EOS_IDS = 8     # EOS ids the min-length processor of the lm_head kernels compares against


def resolve_logits_processors(prompt_len: int, eos: Optional[List[int]], repetition_penalty=1.0, min_length=0, min_new_tokens=0,
                              suppress_tokens=None, bad_words_ids=None):
    """The deterministic logits processors of transformers' `generate` (GenerationMixin._get_logits_processor), resolved on the
    host to what the lm_head kernels take: (penalty p, min_new, sorted ban list).
      * repetition_penalty: RepetitionPenaltyLogitsProcessor is built for any value other than 1 and insists on a float > 0.
      * min_new = number of generated tokens before which EOS is banned. min_new_tokens > 0 wins (HF sets min_length from it);
        otherwise min_length counts the prompt: max(0, min_length - prompt_len), in both input modes (with inputs_embeds only
        HF reduces min_length by the prompt length, _prepare_generated_length). No EOS id: both are no-ops.
      * suppress_tokens and single-token bad_words_ids are one ban set; NoBadWordsLogitsProcessor drops entries equal to [eos].
        A multi-token bad word depends on the previous tokens and is not implemented."""
    p = 1.0
    if repetition_penalty is not None and repetition_penalty != 1.0:
        if not isinstance(repetition_penalty, float) or not (repetition_penalty > 0):
            raise ValueError(f"`repetition_penalty` has to be a strictly positive float, but is {repetition_penalty}")
        p = repetition_penalty
    for name, v in (("min_length", min_length), ("min_new_tokens", min_new_tokens)):
        if v is not None and (not isinstance(v, int) or v < 0):
            raise ValueError(f"`{name}` has to be a non-negative integer, but is {v}")
    min_new = 0
    if eos:
        if len(eos) > MAX_EOS_IDS:
            raise ValueError(f"at most {MAX_EOS_IDS} eos_token_id values are supported with min_length / min_new_tokens")
        min_new = int(min_new_tokens) if min_new_tokens else max(0, int(min_length or 0) - int(prompt_len))
    ban = set(int(t) for t in (suppress_tokens if suppress_tokens is not None else ()))
    for w in (bad_words_ids or ()):
        w = [int(t) for t in w]
        if len(w) != 1:
            raise NotImplementedError(f"bad_words_ids entry {w}: only single-token bad words are supported "
                                      "(a multi-token entry bans its last token only after its prefix)")
        if not (eos and w[0] in eos):
            ban.add(w[0])
    return p, min_new, sorted(ban)


def resolve_no_repeat_ngram(no_repeat_ngram_size) -> int:
    """`no_repeat_ngram_size` of transformers' `generate`: None and 0 build no processor (returns 0); anything else has to be what
    NoRepeatNGramLogitsProcessor insists on, a strictly positive integer. No upper limit: a size longer than the sequence bans
    nothing."""
    if no_repeat_ngram_size is None or (no_repeat_ngram_size == 0 and not isinstance(no_repeat_ngram_size, (bool, float))):
        return 0
    if isinstance(no_repeat_ngram_size, bool) or not isinstance(no_repeat_ngram_size, int) or no_repeat_ngram_size < 1:
        raise ValueError(f"`no_repeat_ngram_size` has to be a strictly positive integer, but is {no_repeat_ngram_size}")
    if no_repeat_ngram_size > 2 ** 31 - 1:
        raise ValueError(f"`no_repeat_ngram_size` has to fit 32 bits, but is {no_repeat_ngram_size}")
    return int(no_repeat_ngram_size)


def ngram_banned_host(seq: Sequence[int], n: int) -> set:
    """The tokens transformers' NoRepeatNGramLogitsProcessor(n) bans behind the sequence seq = s[0..L): x is banned iff some i in
    [0, L - n + 1) has s[i .. i+n-1) == s[L-n+1 .. L) and s[i+n-1] == x; nothing while L + 1 < n; n = 1 bans every token of s.
    seq is the row's input_ids (pads included) followed by its generated tokens; the generated tokens alone for an inputs_embeds
    call -- the conventions of the penalty's `seen` set (`resolve_logits_processors`)."""
    s = [int(t) for t in seq]
    L, n = len(s), int(n)
    if n < 1 or L + 1 < n:
        return set()
    tail = s[L - n + 1:L]
    return {s[i + n - 1] for i in range(L - n + 1) if s[i:i + n - 1] == tail}


def process_logits_host(logits: torch.Tensor, seen: torch.Tensor, p: float, ban: Sequence[int], eos: Optional[List[int]],
                        n_new: int, min_new: int, ngram_banned: Optional[Sequence[Sequence[int]]] = None) -> torch.Tensor:
    """Host restatement of the lm_head kernels' epilogue, in fp32, on raw logits [B, V]: `seen` [B, V] bool marks the ids the
    repetition penalty applies to (every id of the row's input_ids, pads included, plus the generated ids; the generated ids alone
    for an inputs_embeds call), `n_new` = tokens generated so far. `ngram_banned`: per row, the ids no_repeat_ngram_size bans at
    this step (`ngram_banned_host`); None = none. The greedy token is the lowest-index arg-max of the result."""
    lv = logits.float().clone()
    if p != 1.0:
        lv = torch.where(seen, torch.where(lv < 0, lv * p, lv / p), lv)
    V = lv.shape[-1]
    for b, row in enumerate(ngram_banned or ()):
        for t in row:
            if 0 <= t < V:
                lv[b, t] = -math.inf
    for t in ban:
        if 0 <= t < V:
            lv[:, t] = -math.inf
    if eos and n_new < min_new:
        for t in eos:
            if 0 <= t < V:
                lv[:, t] = -math.inf
    return lv


def prompt_lookup_off(prompt_lookup_num_tokens) -> bool:
    """None and 0 switch prompt-lookup decoding off, as in transformers; every other value is validated by `resolve_prompt_lookup`"""
    K = prompt_lookup_num_tokens
    return K is None or (K == 0 and not isinstance(K, (bool, float)))


def resolve_prompt_lookup(prompt_lookup_num_tokens, max_matching_ngram_size=None, B: int = 1, S: int = 0, max_new_tokens: int = 0,
                          max_len: int = 0, decode_rows: int = 8, head_dim: int = 128, do_sample: bool = False, num_beams=1,
                          processed: bool = False, no_repeat_ngram_size=None, output_hidden_states: bool = False,
                          return_logits: bool = False):
    """Validate `generate(prompt_lookup_num_tokens=K, max_matching_ngram_size=N)` (transformers' prompt-lookup decoding) against what
    the verify step implements and return (K, N), or None when the keyword is off (None or 0: everything stays as without it, and
    max_matching_ngram_size is not looked at, as in transformers). K drafts ride as K more rows of the decode step, so K is an int
    in 1 .. min(decode_rows, ops.SPEC_MAX_ROWS) - 1; N defaults to transformers' 2 and has to lie in 1 .. ops.SPEC_MAX_NGRAM. The served ground is one
    greedy sequence (batch 1, num_beams 1, do_sample False) without logits processors, no_repeat_ngram_size, output_hidden_states or
    return_logits, at head_dim 128, with S + max_new_tokens + K <= max_len (a rejected draft still writes its K / V row). Everything
    else raises and names the argument; nothing is ignored."""
    K = prompt_lookup_num_tokens
    if prompt_lookup_off(K):
        return None
    rows = min(decode_rows, ops.SPEC_MAX_ROWS)      # of the decode graph, and of the verify kernels
    if isinstance(K, bool) or not isinstance(K, int) or not (1 <= K <= rows - 1):
        raise ValueError(f"`prompt_lookup_num_tokens` has to be an integer in [1, {rows - 1}] (the drafts are rows of the "
                         f"decode graph's {rows}) or None / 0, but is {K}")
    N = 2 if max_matching_ngram_size is None else max_matching_ngram_size
    if isinstance(N, bool) or not isinstance(N, int) or not (1 <= N <= ops.SPEC_MAX_NGRAM):
        raise ValueError(f"`max_matching_ngram_size` has to be an integer in [1, {ops.SPEC_MAX_NGRAM}], but is {N}")
    if B != 1:
        raise NotImplementedError(f"prompt_lookup_num_tokens serves one sequence per call (transformers' assisted decoding is batch 1 too), "
                                  f"but the batch has {B} rows")
    if do_sample:
        raise NotImplementedError("prompt_lookup_num_tokens with do_sample=True is not implemented (speculative sampling needs the rejection rule)")
    if num_beams != 1:
        raise NotImplementedError("prompt_lookup_num_tokens with num_beams > 1 is not implemented")
    if no_repeat_ngram_size:
        raise NotImplementedError("prompt_lookup_num_tokens with no_repeat_ngram_size is not implemented: pass None or 0")
    if processed:
        raise NotImplementedError("prompt_lookup_num_tokens with repetition_penalty / min_length / min_new_tokens / suppress_tokens / "
                                  "bad_words_ids is not implemented: pass their neutral values")
    if output_hidden_states:
        raise NotImplementedError("prompt_lookup_num_tokens with output_hidden_states is not implemented")
    if return_logits:
        raise NotImplementedError("prompt_lookup_num_tokens with return_logits is not implemented")
    if head_dim != 128:
        raise NotImplementedError(f"prompt_lookup_num_tokens needs head_dim 128 (the verify attention), but head_dim is {head_dim}")
    if S + max_new_tokens + K > max_len:
        raise ValueError(f"prompt_lookup_num_tokens={K}: prompt {S} + max_new_tokens {max_new_tokens} + {K} draft rows exceed the "
                         f"engine's max_len={max_len} (a rejected draft still writes its K / V row)")
    return K, N


def prompt_lookup_draft_host(seq: Sequence[int], K: int, N: int) -> List[int]:
    """The draft of transformers' PromptLookupCandidateGenerator(num_output_tokens=K, max_matching_ngram_size=N) behind the sequence
    seq = s[0..L), with logits_processor=None, no EOS cut and max_length far away: for n = min(N, L - 1) .. 1 the EARLIEST i with
    s[i : i + n] == s[L - n :] and i + n < L gives s[i + n : min(i + n + K, L)]; the first n that has one wins, else []. seq is the
    row's input_ids (pads included) followed by its generated tokens; the generated tokens alone for an inputs_embeds call."""
    s = [int(t) for t in seq]
    L, K, N = len(s), int(K), int(N)
    if K < 1:
        return []
    for n in range(min(N, L - 1), 0, -1):
        tail = s[L - n:]
        for i in range(L - n):
            if s[i:i + n] == tail:
                return s[i + n:min(i + n + K, L)]
    return []


def spec_accept_host(ids: Sequence[int], n_draft: int, lm_out: Sequence[int]) -> int:
    """The number of drafts a verify step accepts: ids[0] is the last accepted token, ids[1 .. n_draft] its drafted successors and
    lm_out[r] the model's greedy token behind row r; a = the largest j <= n_draft with lm_out[i - 1] == ids[i] for all 1 <= i <= j.
    The sequence then grows by lm_out[0 .. a]: the a agreed drafts and the model's own token behind the last of them."""
    a = 0
    while a < int(n_draft) and int(lm_out[a]) == int(ids[a + 1]):
        a += 1
    return a


def resolve_assisted(assistant_model, num_assistant_tokens=None, num_assistant_tokens_schedule=None,
                     assistant_confidence_threshold=None, target=None, B: int = 1, S: int = 0, max_new_tokens: int = 0,
                     decode_rows: int = 8, do_sample: bool = False, num_beams=1, processed: bool = False, no_repeat_ngram_size=None,
                     output_hidden_states: bool = False, return_logits: bool = False, prompt_lookup_num_tokens=None,
                     embeds_only: bool = False, whole_generate: bool = True):
    """Validate `generate(assistant_model=draft, num_assistant_tokens=K)` (transformers' assisted decoding) against what the round
    implements and return K, or None when assistant_model is None (everything stays as without it; the three companion keywords
    then have to be None too -- they would mean nothing). `target` and `assistant_model` are read as engines: cfg.head_dim,
    cfg.vocab, max_batch, max_len, device. K defaults to 5 and is an int in 1 .. min(decode_rows, ops.SPEC_MAX_ROWS) - 1 (the
    drafts are rows of the target's decode graph); num_assistant_tokens_schedule may be None / "constant" and
    assistant_confidence_threshold None / 0 (K is fixed; no heuristic and no early stop of the draft loop). The served ground is one
    greedy sequence given as input_ids through `generate` (batch 1, num_beams 1, do_sample False), without logits processors,
    no_repeat_ngram_size, output_hidden_states, return_logits or prompt_lookup_num_tokens, both engines at head_dim 128 on one
    device, the draft engine distinct from the target, with max_batch >= 2 (its catch-up step has two rows) and a vocabulary no
    larger than the target's, and S + max_new_tokens + K <= max_len of both engines (a rejected draft still writes its K / V row).
    Everything else raises and names the argument; nothing is ignored."""
    K = num_assistant_tokens
    if assistant_model is None:
        for name, v in (("num_assistant_tokens", K), ("num_assistant_tokens_schedule", num_assistant_tokens_schedule),
                        ("assistant_confidence_threshold", assistant_confidence_threshold)):
            if v is not None:
                raise ValueError(f"`{name}` was given without `assistant_model`: it configures assisted decoding and means nothing alone")
        return None
    rows = min(decode_rows, ops.SPEC_MAX_ROWS)
    K = 5 if K is None else K
    if isinstance(K, bool) or not isinstance(K, int) or not (1 <= K <= rows - 1):
        raise ValueError(f"`num_assistant_tokens` has to be an integer in [1, {rows - 1}] (the drafts are rows of the decode "
                         f"graph's {rows}) or None, but is {K}")
    if num_assistant_tokens_schedule not in (None, "constant"):
        raise NotImplementedError(f"num_assistant_tokens_schedule={num_assistant_tokens_schedule!r} is not implemented: the number of "
                                  f"drafts is fixed, pass None or 'constant'")
    th = assistant_confidence_threshold
    if th is not None and (isinstance(th, bool) or not isinstance(th, (int, float)) or th != 0):
        raise NotImplementedError(f"assistant_confidence_threshold={th!r} is not implemented: every round drafts num_assistant_tokens "
                                  f"tokens, pass None or 0")
    if assistant_model is target:
        raise ValueError("`assistant_model` is the engine itself: a draft engine of its own (weights, KV cache, decode states) is needed")
    for attr in ("cfg", "max_batch", "max_len", "device", "_prefill", "_decode_step"):
        if not hasattr(assistant_model, attr):
            raise TypeError(f"`assistant_model` has to be a LlamaEngine, but is {type(assistant_model).__name__}")
    if not whole_generate:
        raise NotImplementedError("assistant_model runs through LlamaEngine.generate only: the split prefill_begin / adopt / decode_finish "
                                  "path has no draft engine's cache to carry along")
    if embeds_only:
        raise NotImplementedError("assistant_model with inputs_embeds and no input_ids is not implemented: the draft engine cannot embed them")
    if not prompt_lookup_off(prompt_lookup_num_tokens):
        raise NotImplementedError("assistant_model together with prompt_lookup_num_tokens is not implemented: one source of drafts per call")
    if B != 1:
        raise NotImplementedError(f"assistant_model serves one sequence per call (transformers' assisted decoding is batch 1 too), "
                                  f"but the batch has {B} rows")
    if do_sample:
        raise NotImplementedError("assistant_model with do_sample=True is not implemented (speculative sampling needs the rejection rule)")
    if num_beams != 1:
        raise NotImplementedError("assistant_model with num_beams > 1 is not implemented")
    if no_repeat_ngram_size:
        raise NotImplementedError("assistant_model with no_repeat_ngram_size is not implemented: pass None or 0")
    if processed:
        raise NotImplementedError("assistant_model with repetition_penalty / min_length / min_new_tokens / suppress_tokens / "
                                  "bad_words_ids is not implemented: pass their neutral values")
    if output_hidden_states:
        raise NotImplementedError("assistant_model with output_hidden_states is not implemented")
    if return_logits:
        raise NotImplementedError("assistant_model with return_logits is not implemented")
    d = assistant_model
    for who, eng in (("the engine's", target), ("the assistant_model's", d)):
        if eng.cfg.head_dim != 128:
            raise NotImplementedError(f"assistant_model needs head_dim 128 on both engines (the verify attention), but {who} head_dim "
                                      f"is {eng.cfg.head_dim}")
    if d.max_batch < 2:
        raise NotImplementedError(f"assistant_model needs a draft engine with max_batch >= 2 (its catch-up step carries two rows), "
                                  f"but its max_batch is {d.max_batch}")
    if torch.device(d.device) != torch.device(target.device):
        raise NotImplementedError(f"assistant_model lives on another device ({d.device}) than the engine ({target.device})")
    if d.cfg.vocab > target.cfg.vocab:
        raise ValueError(f"assistant_model has a larger vocabulary ({d.cfg.vocab}) than the engine ({target.cfg.vocab}): its drafts "
                         f"could name ids the engine does not have")
    for who, eng in (("the engine's", target), ("the assistant_model's", d)):
        if S + max_new_tokens + K > eng.max_len:
            raise ValueError(f"num_assistant_tokens={K}: prompt {S} + max_new_tokens {max_new_tokens} + {K} draft rows exceed {who} "
                             f"max_len={eng.max_len} (a rejected draft still writes its K / V row)")
    return K


def assisted_round_host(ids0: int, pos0: int, slot0: int, drafts: Sequence[int], lm_out: Sequence[int], draft_vocab: int,
                        n_draft: Optional[int] = None) -> dict:
    """One round of assisted decoding behind the draft steps and the verify step, on the host: what the launches of
    csrc/spec_assist.hip leave in the two engines' cursors. The sequence ends with the token ids0 at position pos0 and cache slot
    slot0 (they differ by kv_beg for a left-padded prompt); drafts = d_1 .. d_K as the draft engine proposed them one by one;
    lm_out[r] = the target's greedy token behind row r of the verify step [ids0, d_1 .. d_K]; n_draft (default K) of the rows count
    as drafts. Returns
      rows      [(id, pos, slot)] of the K + 1 verify rows as the pushes left them (row 0 is the caller's)
      feed      [(id, pos, slot, kv_end)] of the draft engine's single row behind every push: ids >= draft_vocab read as 0 THERE only
      a         drafts accepted (`spec_accept_host`);  append = lm_out[: a + 1], the tokens that join the sequence
      row0      (id, pos, slot) of the next round's row 0: (lm_out[a], pos0 + a + 1, slot0 + a + 1);  the target's kv_end and n_hist
                grow by a + 1, the counters by (1, n_draft, a)
      catch_up  dict(ids, pos, slot: two each, kv_end) of the draft engine's next two-row step: the sequence's last two tokens
                (row a of this round and lm_out[a]; ids >= draft_vocab as 0) at (pos0 + a, pos0 + a + 1) / (slot0 + a, slot0 + a + 1),
                kv_end = slot0 + a + 1 -- row 0 rewrites a K / V row the draft engine may hold already, which makes the round's shape
                independent of a: after a fully accepted round the draft engine never consumed d_K, and this row supplies it."""
    K = len(drafts)
    nd = K if n_draft is None else max(0, min(int(n_draft), K))
    dv = lambda t: int(t) if 0 <= int(t) < draft_vocab else 0
    rows = [(int(ids0), int(pos0), int(slot0))] + [(int(d), pos0 + j, slot0 + j) for j, d in enumerate(drafts, 1)]
    feed = [(dv(d), pos0 + j, slot0 + j, slot0 + j + 1) for j, d in enumerate(drafts, 1)]
    a = spec_accept_host([r[0] for r in rows], nd, lm_out)
    prev, last = rows[a][0], int(lm_out[a])
    return dict(rows=rows, feed=feed, a=a, n_draft=nd, append=[int(t) for t in lm_out[:a + 1]],
                row0=(last, pos0 + a + 1, slot0 + a + 1),
                catch_up=dict(ids=[dv(prev), dv(last)], pos=[pos0 + a, pos0 + a + 1], slot=[slot0 + a, slot0 + a + 1],
                              kv_end=slot0 + a + 1))


SAMPLE_MAX_K = 64       # top_k limit of the sampling kernels (csrc/sample.hip)


def resolve_sampling(do_sample, temperature=1.0, top_k=None, top_p=1.0, num_return_sequences=1):
    """Validate the sampling keywords of `generate` against what the sampling kernels implement and return (temperature, top_k,
    top_p), or None for do_sample=False (which ignores the three warper arguments, as HF does). The ValueErrors are the ones
    transformers' TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper raise for the same values; a top_k that switches
    the filter off (0) or exceeds the kernels' candidate list raises NotImplementedError: the nucleus is taken among at most
    SAMPLE_MAX_K tokens, a full-vocabulary top-p is not implemented. top_k=None is what transformers' `generate` resolves it to."""
    if not do_sample:
        return None
    if num_return_sequences not in (None, 1):
        raise NotImplementedError("do_sample=True with num_return_sequences > 1 is not implemented")
    if temperature is None or (temperature == 1 and not isinstance(temperature, bool)):
        temperature = 1.0       # HF builds no warper for 1 (the reference's integer default, spider.py:1471-1477)
    if not isinstance(temperature, float) or not (temperature > 0):
        raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float")
    try:
        top_p = float(top_p)
    except (TypeError, ValueError):
        raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}") from None
    if not (0 < top_p <= 1.0):
        raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}")
    if top_k is None:
        top_k = 50
        try:
            from transformers import GenerationConfig
            top_k = GenerationConfig._get_default_generation_params().get("top_k", top_k)
        except (ImportError, AttributeError):
            pass
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"`top_k` has to be a strictly positive integer, but is {top_k}")
    if top_k == 0 or top_k > SAMPLE_MAX_K:
        raise NotImplementedError(f"top_k={top_k}: sampling keeps between 1 and {SAMPLE_MAX_K} candidates per step (top_k = 0 switches "
                                  "HF's filter off; a full-vocabulary nucleus is not implemented)")
    return temperature, top_k, top_p


def resolve_seed(seed) -> int:
    """The 64-bit seed of a sampling request: an int as given; None draws 63 bits from torch's default CPU generator, so
    torch.manual_seed makes a run reproducible."""
    if seed is None:
        return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f"`seed` has to be an integer or None, but is {seed}")
    return seed & (2 ** 64 - 1)


def sample_uniform_host(seed: int, row: int, step: int) -> float:
    """The uniform of the sampling kernels for (seed, absolute row of the call, number of tokens the row has generated so far):
    Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) at counter (step, row, 0, 0); u = ((out[0] >> 9) + 0.5) * 2^-23: 24
    significant bits, so exact in fp32 and strictly inside (0, 1)."""
    M = 0xFFFFFFFF
    c = [step & M, row & M, 0, 0]
    k0, k1 = seed & M, (seed >> 32) & M
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M, (p0 >> 32) ^ c[3] ^ k1, p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return ((c[0] >> 9) + 0.5) * 2.0 ** -23


def sample_token_host(x: torch.Tensor, temperature: float, top_k: int, top_p: float, u: float) -> dict:
    """Host restatement in fp64 of the sampling step (csrc/sample.hip) for ONE row of processed logits x [V] (fp32, the result of
    `process_logits_host`):
      candidates  the top_k tokens by (x descending, token id ascending) = rank 0 .. top_k - 1. EXACTLY top_k: HF's TopKLogitsWarper
                  keeps every token that ties with the k-th value, here the lower ids win
      p           p_j = exp(x_j / T - x_0 / T), 0 where x_j = -inf; P = their sum
      n_keep      rank j is kept iff the mass before it < top_p * P (HF's TopPLogitsWarper on the survivors of top-k); at least 1
      token       the first kept rank j with u * S < p_0 + ... + p_j, S = the kept mass; rank n_keep - 1 if rounding leaves none
    Returns dict(tokens [k] int64, x [k] fp32, p [k] fp64, cum [k] fp64 (cum[j] = p_0 + ... + p_j), n_keep, S, rank, token)."""
    x = x.detach().float().cpu().view(-1)
    k = min(int(top_k), x.numel())
    xs, idx = torch.sort(x, descending=True, stable=True)        # stable: equal values keep the ascending ids
    xs, idx = xs[:k], idx[:k]
    y = xs.double() / float(temperature)
    p = torch.where(torch.isinf(xs) & (xs < 0), torch.zeros_like(y), torch.exp(y - y[0]))
    p = torch.nan_to_num(p, nan=0.0)        # a row that is all -inf
    cum = p.cumsum(0)
    P = float(cum[-1])
    before = cum - p
    n_keep = max(1, int((before < float(top_p) * P).sum()))
    S = float(cum[n_keep - 1])
    hit = (float(u) * S < cum[:n_keep]).nonzero()
    rank = int(hit[0]) if hit.numel() else n_keep - 1
    return dict(tokens=idx, x=xs, p=p, cum=cum, n_keep=n_keep, S=S, rank=rank, token=int(idx[rank]))


IGNORE_INDEX = -100     # HF's ignore_index: a label that is not scored


class ScoreOutput:
    """Result of `LlamaEngine.score` / `score_host`. Every per-position field is [B, S] and aligned to the LABEL it scores: index t
    comes from the logits row t - 1 (HF's shift); index 0 and ignored positions hold 0 (argmax: -1) and `mask` is False there.
      token_logprobs  log p(labels[b, t] | tokens before t)      mask      the scored positions
      argmax          the model's own prediction for index t     entropy   of that predictive distribution (nats)
      loss = -sum(token_logprobs) / n_tokens over the mask (what LlamaForCausalLM(...).loss returns; NaN when n_tokens == 0),
      n_tokens, perplexity = exp(loss)
    with a reference distribution (`other` / `logits_ref`): kl = KL(reference || this) per position, mean_kl over the mask and
    top1_agree = the share of scored positions where both arg-maxima agree; with return_logits the bf16 logits [B, S, V]."""

    def __init__(self, token_logprobs, mask, argmax, entropy, loss, n_tokens, kl=None, mean_kl=None, top1_agree=None, logits=None):
        self.token_logprobs, self.mask, self.argmax, self.entropy = token_logprobs, mask, argmax, entropy
        self.loss, self.n_tokens = float(loss), int(n_tokens)
        self.perplexity = math.exp(min(self.loss, 709.0))       # (NaN stays NaN)
        self.kl, self.mean_kl, self.top1_agree, self.logits = kl, mean_kl, top1_agree, logits

    def __getitem__(self, k):
        return getattr(self, k)


def score_targets(labels: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The label each position is scored against, int64 [B, S] on the CPU: labels[b, t] where t >= 1, attention_mask[b, t] != 0 and
    the label is not -100; IGNORE_INDEX elsewhere. This is the mask of `score` and `score_host`. A left-padded row's first real
    token is scored from the logits of a pad position, as transformers does: give it label -100 to leave it out."""
    tg = labels.detach().to("cpu", torch.int64).clone()
    tg[:, 0] = IGNORE_INDEX
    if attention_mask is not None:
        tg[attention_mask.detach().cpu() == 0] = IGNORE_INDEX
    return tg


def _score_assemble(tg, lp, am, ent, kl=None, am_ref=None, logits=None) -> ScoreOutput:
    """per-row results (row (b, s) of the logits: [B, S]) -> the label-aligned, masked fields of a ScoreOutput"""
    mask = tg != IGNORE_INDEX
    mask = mask.to(lp.device)

    def shift(v, fill):
        out = torch.full_like(v, fill)
        out[:, 1:] = v[:, :-1]
        return torch.where(mask, out, torch.full_like(out, fill))
    tlp, amx, en = shift(lp, 0), shift(am, -1), shift(ent, 0)
    n = int(mask.sum())
    loss = float(-tlp.double().sum() / n) if n else float("nan")
    o = ScoreOutput(tlp, mask, amx, en, loss, n, logits=logits)
    if kl is not None:
        o.kl = shift(kl, 0)
        o.mean_kl = float(o.kl.double().sum() / n) if n else float("nan")
        o.top1_agree = float((shift(am_ref, -1) == amx)[mask].double().mean()) if n else float("nan")
    return o


def score_host(logits: torch.Tensor, labels: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
               logits_ref: Optional[torch.Tensor] = None) -> ScoreOutput:
    """Host restatement in fp64 of `LlamaEngine.score` on given logits [B, S, V] (any float dtype; the values are taken as they are):
    the definition of every ScoreOutput field. Row t - 1 scores labels[b, t] (`score_targets` is the mask): x = logits[b, t - 1],
    lse = log sum exp x, token_logprobs = x[label] - lse, argmax = the lowest id among the maxima, entropy = -sum p log p,
    loss = the mean negative log-probability over the mask = F.cross_entropy(logits[:, :-1], labels[:, 1:], ignore_index=-100) of
    LlamaForCausalLM.forward(labels=). With logits_ref (the reference distribution): kl = sum p_ref (log p_ref - log p)."""
    x = logits.detach().double().cpu()
    B, S, V = x.shape
    tg = score_targets(labels, attention_mask)
    if tuple(tg.shape) != (B, S):
        raise ValueError(f"labels must be [{B}, {S}], got {tuple(tg.shape)}")
    if int(tg.max()) >= V or bool(((tg < 0) & (tg != IGNORE_INDEX)).any()):
        raise ValueError(f"labels must be in [0, {V}) or {IGNORE_INDEX}")
    nxt = torch.full_like(tg, IGNORE_INDEX)
    nxt[:, :-1] = tg[:, 1:]                     # the label row (b, s) is scored against
    lsm = torch.log_softmax(x, -1)
    lp = torch.where(nxt >= 0, lsm.gather(-1, nxt.clamp(min=0)[..., None])[..., 0], torch.zeros(B, S, dtype=torch.float64))
    ids = torch.arange(V)

    def first_max(v):
        return torch.where(v == v.amax(-1, keepdim=True), ids, torch.full_like(ids, V)).amin(-1)
    ent = -(lsm.exp() * lsm).sum(-1)
    kl = am_ref = None
    if logits_ref is not None:
        y = logits_ref.detach().double().cpu()
        if y.shape != x.shape:
            raise ValueError(f"logits_ref must be {tuple(x.shape)}, got {tuple(y.shape)}")
        lsr = torch.log_softmax(y, -1)
        kl = (lsr.exp() * (lsr - lsm)).sum(-1)
        am_ref = first_max(y)
    return _score_assemble(tg, lp, first_max(x), ent, kl, am_ref)


def resolve_score(vocab: int, hidden: int, max_batch: int, max_len: int, mrope: bool, input_ids=None, inputs_embeds=None,
                  attention_mask=None, position_ids=None, labels=None):
    """The served ground of `LlamaEngine.score`, checked on the host before anything is enqueued (the input rules of prefill_begin);
    a violation raises ValueError naming the argument. Returns (B, S, targets) with targets = `score_targets` of the labels
    (default: input_ids)."""
    if (input_ids is None) == (inputs_embeds is None):
        raise ValueError("score: exactly one of input_ids and inputs_embeds must be given")
    if input_ids is not None:
        if input_ids.dim() != 2 or input_ids.dtype not in (torch.int32, torch.int64) or input_ids.numel() == 0:
            raise ValueError(f"input_ids must be a non-empty integer tensor [B, S], got {tuple(input_ids.shape)} {input_ids.dtype}")
        B, S = input_ids.shape
        ic = input_ids.detach().cpu()
        if int(ic.min()) < 0 or int(ic.max()) >= vocab:
            raise ValueError(f"input_ids must be in [0, {vocab})")
        name = "input_ids"
    else:
        if inputs_embeds.dim() != 3 or inputs_embeds.shape[-1] != hidden or inputs_embeds.numel() == 0:
            raise ValueError(f"inputs_embeds must be [B, S, {hidden}], got {tuple(inputs_embeds.shape)}")
        B, S = inputs_embeds.shape[:2]
        name = "inputs_embeds"
        if labels is None:
            raise ValueError("labels are required with inputs_embeds alone (there are no ids to default to)")
    if B > max_batch or S > max_len:
        raise ValueError(f"{name}: batch {B} / length {S} exceed the preallocated KV cache ({max_batch} x {max_len})")
    if attention_mask is not None:
        if tuple(attention_mask.shape) != (B, S):
            raise ValueError(f"attention_mask must be [{B}, {S}], got {tuple(attention_mask.shape)}")
        am = (attention_mask.detach().cpu() != 0).to(torch.int64)
        if bool((am[:, 1:] < am[:, :-1]).any()) or bool((am[:, -1] == 0).any()):
            raise ValueError("attention_mask must describe LEFT padding: zeros, then ones up to the last position of every row")
    if position_ids is not None:
        if not mrope:
            raise ValueError("position_ids with 3 components need a model with mrope_section (Qwen2.5-Omni thinker)")
        if tuple(position_ids.shape) != (3, B, S):
            raise ValueError(f"position_ids must be [3, {B}, {S}], got {tuple(position_ids.shape)}")
    if labels is None:
        labels = input_ids
    if tuple(labels.shape) != (B, S) or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"labels must be an integer tensor [{B}, {S}], got {tuple(labels.shape)} {labels.dtype}")
    tg = score_targets(labels, attention_mask)
    if int(tg.max()) >= vocab or bool(((tg < 0) & (tg != IGNORE_INDEX)).any()):
        raise ValueError(f"labels must be in [0, {vocab}) or {IGNORE_INDEX} (ignored)")
    return B, S, tg


def finalize_greedy(tokens: torch.Tensor, eos: Optional[List[int]], pad: Optional[int], stopping_criteria,
                    prompt: Optional[torch.Tensor], checked: int = 0):
    """HF greedy-search bookkeeping (`_sample` with do_sample=False, as driven by spider.py:1492-1508), applied to a
    block of already generated tokens [B, n] (CPU int64):
      * a row is finished after its first EOS token; every later token of that row is pad_token_id
        (`next_tokens * unfinished + pad * (1 - unfinished)`);
      * the loop ends at the first length k where every row is finished, or where a stopping criterion returns True
        (StoppingCriteriaSub, spider.py:55-73, looks at sequence 0 and ends the whole batch);
    Returns (tokens with pads applied, k, stopped). `checked` = lengths < checked were already examined (the criteria
    are re-run only on the new prefixes, so `sync_every` > 1 finds the exact stop step after the fact)."""
    B, n = tokens.shape
    tk = tokens.clone()
    if eos:
        is_eos = torch.isin(tk, torch.tensor(eos))
        seen = is_eos.long().cumsum(1)
        after = (seen - is_eos.long()) > 0          # strictly after the row's first EOS
        if pad is None:
            pad = eos[0]                            # HF: "Setting pad_token_id to eos_token_id"
        tk[after] = pad
        done_at = torch.where(is_eos.any(1), is_eos.long().argmax(1) + 1, torch.full((B,), n + 1))
        k_eos = int(done_at.max())                  # all rows finished once the slowest has emitted its EOS
    else:
        k_eos = n + 1
    k_sc = n + 1
    if stopping_criteria:
        for k in range(max(1, checked), min(n, k_eos) + 1):
            seq = tk[:, :k] if prompt is None else torch.cat([prompt, tk[:, :k]], 1)
            if any(bool(torch.as_tensor(sc(seq, None)).all()) for sc in stopping_criteria):
                k_sc = k
                break
    k = min(k_eos, k_sc)
    if k <= n:
        return tk[:, :k], k, True
    return tk, n, False


BEAM_MAX_K = 8          # beams per batch row (the decode graph holds DECODE_ROWS = 8 rows)
BEAM_MAX_C = 32         # continuations kept per batch row and step by the selection kernel


def resolve_beam_search(B: int, num_beams, max_batch: int, vocab: int, eos: Optional[List[int]], decode_rows: int = 8,
                        do_sample: bool = False, stopping_criteria=None, output_hidden_states: bool = False, processed: bool = False,
                        num_beam_groups=1, constraints=None, force_words_ids=None, num_return_sequences=1, length_penalty=1.0,
                        early_stopping=False) -> int:
    """Validate a `generate(num_beams > 1, ...)` request against what the beam path implements and return C, the number of
    continuations kept per batch row and step: transformers' `beams_to_keep = max(2, 1 + n_eos) * num_beams` (sized so that
    num_beams unfinished ones always exist). Everything outside the implemented ground raises; nothing is ignored."""
    if not isinstance(num_beams, int) or isinstance(num_beams, bool) or not (2 <= num_beams <= BEAM_MAX_K):
        raise ValueError(f"num_beams has to be an integer in [1, {BEAM_MAX_K}], but is {num_beams}")
    if do_sample:
        raise NotImplementedError("beam-search multinomial sampling (num_beams > 1 with do_sample=True) is not implemented")
    if num_beam_groups not in (None, 1):
        raise NotImplementedError("group beam search (num_beam_groups > 1) is not implemented")
    if constraints or force_words_ids:
        raise NotImplementedError("constrained beam search (constraints / force_words_ids) is not implemented")
    if stopping_criteria:
        raise NotImplementedError("user stopping_criteria with num_beams > 1 are not implemented (EOS ids and max_new_tokens end a beam)")
    if output_hidden_states:
        raise NotImplementedError("output_hidden_states with num_beams > 1 is not implemented")
    if processed:
        raise NotImplementedError("repetition_penalty / min_length / min_new_tokens / suppress_tokens / bad_words_ids / "
                                  "no_repeat_ngram_size with num_beams > 1 are not implemented: pass their neutral values")
    if B * num_beams > decode_rows or B * num_beams > max_batch:
        raise ValueError(f"batch {B} x num_beams {num_beams} = {B * num_beams} rows exceed the decode graph's {decode_rows} rows "
                         f"or the engine's max_batch={max_batch}")
    if not isinstance(num_return_sequences, int) or not (1 <= num_return_sequences <= num_beams):
        raise ValueError(f"`num_return_sequences` ({num_return_sequences}) has to be in [1, num_beams={num_beams}]")
    if not (early_stopping is True or early_stopping is False or early_stopping == "never"):
        raise ValueError(f"`early_stopping` must be a boolean or 'never', but is {early_stopping}")
    if not isinstance(length_penalty, (int, float)) or isinstance(length_penalty, bool):
        raise ValueError(f"`length_penalty` has to be a number, but is {length_penalty}")
    n_eos = len(eos) if eos else 0
    if n_eos > MAX_EOS_IDS:
        raise ValueError(f"at most {MAX_EOS_IDS} eos_token_id values are supported with num_beams > 1")
    C = max(2, 1 + n_eos) * num_beams
    if C > BEAM_MAX_C or C > vocab:
        raise ValueError(f"max(2, 1 + n_eos) * num_beams = {C} continuations per step exceed the selection kernel's {BEAM_MAX_C} "
                         f"(or the vocabulary, {vocab})")
    return C


class _BeamHostState:
    """The finished-hypotheses state of transformers' `_beam_search`, in generated-token coordinates (prompt length 0)."""

    def __init__(self, B, K, max_new, fill):
        self.B, self.K, self.t, self.done = B, K, 0, False
        self.running_seq = torch.full((B, K, max_new), fill, dtype=torch.int64)
        self.seq = self.running_seq.clone()
        self.running_idx = torch.full((B, K, max_new), -1, dtype=torch.int32)
        self.idx = self.running_idx.clone()
        self.running_scores = torch.zeros(B, K, dtype=torch.float32)
        self.running_scores[:, 1:] = -1e9
        self.scores = torch.full((B, K), -1e9, dtype=torch.float32)
        self.finished = torch.zeros(B, K, dtype=torch.bool)
        self.unsat = torch.ones(B, 1, dtype=torch.bool)      # is_early_stop_heuristic_unsatisfied


def beam_finalize_host(trace, num_beams: int, max_new_tokens: int, eos: Optional[List[int]], pad: Optional[int],
                       length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1,
                       prompt: Optional[torch.Tensor] = None, state: Optional[_BeamHostState] = None, first_step: int = 0):
    """HF beam-search bookkeeping (transformers 5.x `GenerationMixin._beam_search` with `_update_finished_beams`,
    `_check_early_stop_heuristic`, `_beam_search_has_unfinished_sequences`; num_beams / length_penalty arrive from spider.py:1471-1508
    and conversation.py:151-173), replayed on the CPU over the trace the device wrote: trace = (score f32, beam, token), each
    [n, B, C], the C best continuations of steps first_step .. first_step + n - 1 in score order (beam = source beam within the batch
    row). The running beams of the next step are the first K continuations that neither are an EOS id nor reach max_new_tokens --
    what the device chose without asking. Same fp32 torch expressions as HF, so scores are equal, not close.
    Returns (result, state): result is None while HF's loop would still run (call again with the later steps and `state`); else a
    dict: sequences [B * num_return_sequences, S + n] (prompt [B, S] prepended when given; short ones filled as HF fills them:
    pad_token_id, or eos[0] when that is None or 0), sequences_scores, beam_indices (row b * K + beam per generated token, -1 past
    the end) and n_steps, the number of steps HF's loop ran (later steps of the trace are over-decode and ignored)."""
    score, beam, tok = (t.cpu() for t in trace)
    n, B, C = score.shape
    K = int(num_beams)
    eos_t = torch.tensor(eos) if eos else None
    if state is None:
        fill = (pad if pad else eos[0]) if eos else -1        # HF: `pad_token_id or eos_token_id[0] if eos_token_id is not None else -1`
        state = _BeamHostState(B, K, max_new_tokens, fill)
    st = state
    assert first_step <= st.t, "beam_finalize_host: the trace block starts after the first step not yet replayed"
    top_mask = torch.cat([torch.ones(K, dtype=torch.bool), torch.zeros(C - K, dtype=torch.bool)])
    take = lambda x, i: torch.take_along_dim(x, i.reshape(i.shape + (1,) * (x.dim() - i.dim())), dim=1)
    while not st.done and st.t - first_step < n:
        t = st.t
        lp, bi, tk = score[t - first_step].float(), beam[t - first_step].long(), tok[t - first_step].long()
        # _get_top_k_continuations: the candidates' sequences and back-pointers
        topk_seq = take(st.running_seq, bi)
        topk_idx = take(st.running_idx, bi)
        topk_seq[:, :, t] = tk
        topk_idx[:, :, t] = (bi + torch.arange(B)[:, None] * K).to(torch.int32)
        # stopping criteria of a candidate: EosTokenCriteria | MaxLengthCriteria
        hits = torch.isin(tk, eos_t) if eos_t is not None else torch.zeros_like(tk, dtype=torch.bool)
        if t + 1 >= max_new_tokens:
            hits = torch.ones_like(hits)
        # _get_running_beams_for_next_iteration
        run_lp = lp + hits.to(torch.float32) * -1.0e9
        sel = torch.argsort(hits.long() * C + torch.arange(C)[None], dim=1)[:, :K]
        st.running_seq, st.running_scores, st.running_idx = take(topk_seq, sel), take(run_lp, sel), take(topk_idx, sel)
        # _update_finished_beams
        did = hits & top_mask[None, :]
        flp = lp / ((t + 1) ** length_penalty)
        full = torch.all(st.finished, dim=-1, keepdim=True) & (early_stopping is True)
        flp = flp + full.to(torch.float32) * -1.0e9
        flp = flp + (~st.unsat).to(torch.float32) * -1.0e9
        flp = flp + (~did) * -1.0e9
        m_scores = torch.cat((st.scores, flp), dim=1)
        pick = torch.topk(m_scores, k=K)[1]
        st.seq = take(torch.cat((st.seq, topk_seq), dim=1), pick)
        st.scores = take(m_scores, pick)
        st.idx = take(torch.cat((st.idx, topk_idx), dim=1), pick)
        st.finished = take(torch.cat((st.finished, did), dim=1), pick)
        st.t = t + 1
        # _check_early_stop_heuristic at the new length, _beam_search_has_unfinished_sequences
        best_len = max_new_tokens if (early_stopping == "never" and length_penalty > 0.0) else st.t
        best_running = st.running_scores[:, :1] / (best_len ** length_penalty)
        worst_fin = torch.where(st.finished, torch.min(st.scores, dim=1, keepdim=True)[0], -1.0e9)
        st.unsat = st.unsat & torch.any(best_running > worst_fin, dim=-1, keepdim=True)
        go_on = torch.any(st.unsat) & ~(torch.all(st.finished) & (early_stopping is True)) & ~torch.all(hits)
        st.done = not bool(go_on)
    if not st.done:
        return None, st
    R = int(num_return_sequences)
    seqs = st.seq[:, :R].reshape(B * R, -1)
    idx = st.idx[:, :R].reshape(B * R, -1)
    n_gen = int(((idx + 1).bool()).sum(dim=1).max())
    seqs = seqs[:, :n_gen]
    if prompt is not None:
        seqs = torch.cat([prompt.cpu().long().repeat_interleave(R, dim=0), seqs], 1)
    return dict(sequences=seqs, sequences_scores=st.scores[:, :R].reshape(B * R), beam_indices=idx[:, :n_gen], n_steps=st.t), st


_FUSE_SWIGLU = os.environ.get("SPIDER_PREFILL_SWIGLU_FUSE", "1") != "0"     # tuning aid: 0 = separate SwiGLU launch after the gate/up GEMM


class _PrefillHandle:
    """what LlamaEngine.prefill_begin hands to decode_finish (the locals of `generate` at its half-way point)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class GenerateOutput:
    def __init__(self, sequences, hidden_states=None, sequences_scores=None, beam_indices=None, prompt_lookup=None, assisted=None):
        self.sequences = sequences
        self.hidden_states = hidden_states
        self.sequences_scores = sequences_scores     # beam search only (num_beams > 1)
        self.beam_indices = beam_indices
        self.prompt_lookup = prompt_lookup           # prompt_lookup_num_tokens only: dict(steps=, drafted=, accepted=)
        self.assisted = assisted                     # assistant_model only: dict(steps=, drafted=, accepted=), steps = rounds

    def __getitem__(self, k):
        return getattr(self, k)


class StoppingCriteriaSub:
    """spider/models/spider.py:55-73: stop when the tail of sequence 0 equals any stop-id list."""

    def __init__(self, stops: Sequence[Sequence[int]] = ()):
        self.stops = [list(s) for s in stops]

    def __call__(self, input_ids: torch.Tensor, scores=None) -> bool:
        row = input_ids[0].tolist()
        for s in self.stops:
            if len(row) >= len(s) and row[len(row) - len(s):] == s:
                return True
        return False


# The weight routes of a decode step. A route is one encoding of the weights and the ops that stream it: the layer GEMV, the gate-up
# GEMV with SwiGLU, the lm_head arg-max and its form with logits processors (the fragment-major quantised copies exist for the layers
# only). `suffixes` name where the encoding lives: layer key "w_qkv" / "w_o" / "w_gu" / "w_down" + suffix, engine attribute "lm_head" +
# suffix. The ops are named, not bound: a step looks them up in `ops` when it runs. fm: the fragment-major op families, which take the
# output rows N (the lm_head: V) behind x and no norm_w= (the bf16 copies carry the norm's weight and take norm_eps=).
_Route = namedtuple("_Route", "gemv swiglu head head_proc suffixes fm")
ROUTES = {
    "bf16":     _Route("gemv", "gemv_swiglu", "lm_head_argmax", "lm_head_argmax_proc", ("",), False),
    "bf16_fm":  _Route("gemv_fm", "gemv_swiglu_fm", "lm_head_argmax_fm", "lm_head_argmax_fm_proc", ("_fm",), True),
    "fp8":      _Route("gemv_w8", "gemv_swiglu_w8", "lm_head_argmax_w8", "lm_head_argmax_proc_w8", ("_q8", "_s8"), False),
    "mxfp4":    _Route("gemv_w4", "gemv_swiglu_w4", "lm_head_argmax_w4", "lm_head_argmax_proc_w4", ("_q4", "_e4"), False),
    "fp8_fm":   _Route("gemv_fm_w8", "gemv_swiglu_fm_w8", None, None, ("_q8fm", "_s8"), True),
    "mxfp4_fm": _Route("gemv_fm_w4", "gemv_swiglu_fm_w4", None, None, ("_q4fm", "_e4fm"), True),
}
# How the RMSNorm in front of qkv, gate-up and the lm_head is served: norm_w= / eps= of the GEMV, folded into the weights (norm_eps=),
# or ops.rmsnorm into st["xn"] as a launch of its own
NORM_ARG, NORM_FOLDED, NORM_LAUNCH = "arg", "folded", "launch"
# What a quantised weight format brings: its quantiser pair, and where `LlamaEngine._decode_route` reads its row ranges (attributes of
# the engine: measured crossovers; of `ops`: what the kernels exist for) and the LDS test of its fused norm
_Quant = namedtuple("_Quant", "quantize dequantize rows fm_rows head_rows op_rows norm_fits")
QUANT = {
    "fp8":   _Quant(quantize_fp8_rows, dequantize_fp8_rows, "FP8_MAX_ROWS", "FP8_FM_MAX_ROWS", "LM_HEAD_FP8_MAX_ROWS", "W8_MAX_ROWS", "w8_norm_fits"),
    "mxfp4": _Quant(quantize_mxfp4, dequantize_mxfp4, "MXFP4_MAX_ROWS", "MXFP4_FM_MAX_ROWS", "LM_HEAD_MXFP4_MAX_ROWS", "W4_MAX_ROWS", "w4_norm_fits"),
}


def quantize_weight(W: torch.Tensor, fmt: str):
    """W -> (W_eff, q, scales) in weight format fmt ("fp8" / "mxfp4"): the bytes and what they decode to, the bf16 matrix every bf16
    kernel of a quantised engine reads"""
    q, sc = QUANT[fmt].quantize(W)
    return QUANT[fmt].dequantize(q, sc).contiguous(), q.contiguous(), sc.contiguous()


class LlamaEngine:
    DECODE_ROWS = 8     # sequences per decode graph (lm_head / split-KV workspaces are sized for 8)
    # From this many sequences on the decode GEMVs run as skinny MFMA GEMMs on fragment-major weight copies (SPIDER_DECODE_FM_MIN).
    # Measured on MI355X, Qwen2.5-7B shapes at context 1536 (scripts/exp/decode_vs_batch.py), ms per decode step by rows 1 / 2 / 3 / 4 / 5 / 8:
    # row-major GEMVs 2.84 / 3.28 / 3.75 / 4.36 (then fragment-major 3.21 / 3.43); fragment-major from 2 rows: 2.99 / 3.09 / 3.16 / 3.23 / 3.43.
    FM_MIN_BATCH = int(os.environ.get("SPIDER_DECODE_FM_MIN", "2"))
    # weight_dtype="fp8" engines: decode graphs of up to this many rows stream the e4m3 bytes (csrc/gemv_wq.hip, which exists for 1..4
    # rows), larger ones take the bf16 route above on the dequantised weights. Measured on MI355X, Qwen2.5-7B shapes at context 1536
    # (scripts/exp/fp8_decode_cost.py: both engines alternated in one process, 3 rounds of 96 replays, medians; rounds within 1 us),
    # us per captured decode step by rows 1 / 2 / 3 / 4: bf16 on the route above (row-major at 1, fragment-major from 2)
    # 2638 / 2911 / 2996 / 3063, fp8 1823 / 2162 / 2536 / 3003 = 0.69 / 0.74 / 0.85 / 0.98 of it. 2 % at 4 rows is below the 3 % that
    # counts as a difference, so the range stops at 3.
    FP8_MAX_ROWS = 3
    # weight_dtype="mxfp4" engines: decode graphs of up to this many rows stream the e2m1 bytes and E8M0 scales (csrc/gemv_wq.hip, which
    # exists for 1..4 rows). Set by the same rule as FP8_MAX_ROWS from scripts/exp/mxfp4_decode_cost.py: the largest row count at which
    # the MXFP4 step beats the bf16 route of the same row count by >= 3 %. Measured on MI355X, Qwen2.5-7B shapes at context 1536 (the
    # three engines alternated in one process, 3 rounds of 96 replays, medians; rounds within 2 us), us per captured decode step by
    # rows 1 / 2 / 3 / 4: bf16 2635 / 2910 / 2987 / 3067, fp8 1826 / 2156 / 2531 / 2986, mxfp4 1551 / 1876 / 2277 / 2872 =
    # 0.59 / 0.65 / 0.76 / 0.94 of the bf16 step: 6.4 % at 4 rows counts, so the range is every row count the kernels exist for.
    MXFP4_MAX_ROWS = 4
    # lm_head_dtype="fp8" / "mxfp4" engines: decode graphs of up to this many rows stream the quantised head (csrc/lm_head_wq.hip, which
    # exists for 1..4 rows), larger ones take the bf16 lm_head route on the dequantised head. The rule of FP8_MAX_ROWS: the largest row
    # count at which the captured step with the quantised head beats the step with the bf16 head (same weight_dtype, same rows, same
    # process) by >= 3 %, measured under weight_dtype="mxfp4", where the head's share of the step is largest; 0 when no row count does.
    # Measured on MI355X, Qwen2.5-7B shapes at context 1536 (scripts/exp/lm_head_q_cost.py, profiles/lm_head_q_cost.txt: one engine per
    # weight_dtype with its head switched, the configurations alternated in one process, 3 rounds of 96 replays, medians; rounds
    # within 2 us), us per captured decode step by rows 1 / 2 / 3 / 4, head bf16 | fp8 | mxfp4 (ratios to the bf16 head):
    #   weight_dtype mxfp4: 1536 / 1880 / 2274 / 2881 | 1447 / 1783 / 2201 / 2835 (0.942 / 0.948 / 0.968 / 0.984)
    #                       | 1432 / 1769 / 2174 / 2810 (0.932 / 0.941 / 0.956 / 0.975)
    #   weight_dtype fp8:   1830 / 2167 / 2541 / 3020 | 1744 / 2087 / 2467 / 2975 (0.953 / 0.963 / 0.971 / 0.985)
    #                       | 1710 / 2055 / 2446 / 2951 (0.935 / 0.948 / 0.962 / 0.977)
    #   weight_dtype bf16:  2646 / 2926 / 3006 / 3093 | 2564 / 2849 / 2938 / 3065 (0.969 / 0.974 / 0.977 / 0.991)
    #                       | 2528 / 2817 / 2918 / 3043 (0.955 / 0.963 / 0.971 / 0.984)
    # Under weight_dtype="mxfp4" both heads save >= 3 % up to 3 rows; 1.6 % (fp8) and 2.5 % (mxfp4) at 4 rows do not count.
    LM_HEAD_FP8_MAX_ROWS = 3
    LM_HEAD_MXFP4_MAX_ROWS = 3
    # batched_weight_stream=True engines: decode graphs of more rows than FP8_MAX_ROWS / MXFP4_MAX_ROWS, up to this many, stream the
    # quantised bytes in fragment-major order through the MFMA kernels of csrc/gemv_qfm.hip (which exist for 1..16 rows); larger ones take
    # the bf16 fragment-major route on W_eff. The rule of FP8_MAX_ROWS: the largest row count <= DECODE_ROWS up to which EVERY row count
    # above the row-major range beats the bf16 fragment-major step of the same row count, in the same process, by >= 3 %; 0 when none does.
    # Measured on MI355X, Qwen2.5-7B shapes at context 1536, max_batch 8 (scripts/exp/qfm_decode_cost.py, profiles/qfm_decode_cost.txt:
    # the three engines alternated in one process, 3 rounds of 96 replays, medians; rounds within 2 us), us per captured decode step by
    # rows 4 / 5 / 6 / 8: bf16 3090 / 3145 / 3210 / 3340, fp8 2515 / 2571 / 2622 / 2758 = 0.814 / 0.817 / 0.817 / 0.826 of it, mxfp4
    # (2878 row-major at 4 rows) 2325 / 2387 / 2543 = 0.739 / 0.743 / 0.762 of it at 5 / 6 / 8. 7 rows were not measured.
    FP8_FM_MAX_ROWS = 8
    MXFP4_FM_MAX_ROWS = 8

    def __init__(self, cfg: LLMConfig, weights: dict, device="cuda:0", max_batch: int = 1, max_len: int = 4096,
                 weight_dtype: str = "bf16", calibration=None, lm_head_dtype: str = "bf16", batched_weight_stream: bool = False):
        """weight_dtype="fp8": weight-only FP8 for the decode weight stream. w_qkv, w_o, w_gu and w_down of every layer are
        quantised per output row (`quantize_fp8_rows`: OCP e4m3 with a power-of-two scale; embeddings, lm_head, norms and biases
        stay bf16) and the layer's bf16 matrices are REPLACED by the dequantised W_eff, which bf16 holds exactly. The engine then
        is a bf16 model with weights W_eff in two encodings: prefill, the fragment-major copies and decode graphs of more than
        FP8_MAX_ROWS rows run on W_eff as before, and decode steps of up to FP8_MAX_ROWS rows stream the bytes q (`*_q8`) and
        multiply the fp32 dot product by the row's scale (`*_s8`) -- the same function up to summation order, half the bytes per
        token. Memory: q is kept beside W_eff, about 1.5x the layer weights of a bf16 engine without fragment-major copies.
        weight_dtype="mxfp4": the same construction on OCP MXFP4 (`quantize_mxfp4`: e2m1 nibbles, one E8M0 power-of-two scale per
        block of 32 weights, 4.25 bits per weight). W_eff is again exactly a bf16 matrix and replaces the layer's matrices; decode
        steps of up to MXFP4_MAX_ROWS rows stream the nibbles (`*_q4`) and the scale bytes (`*_e4`), which the kernel applies inside
        the conversion. The format is coarse (11.8 % relative RMS weight error on N(0, 0.02^2) rows, FP8 2.6 %) and no text-quality
        claim is made for it.
        The default "bf16" changes nothing: no tensor, no kernel, no graph key.
        lm_head_dtype="fp8" / "mxfp4" (independent of weight_dtype, which leaves the head alone): the same construction on the
        lm_head. `lm_head` becomes W_eff = dequantize(quantize(head)), a bf16 matrix of its own even when the configuration ties
        the embeddings (`embed_w` keeps the checkpoint's values: the engine is a model with an untied, quantised head), and the
        bytes live beside it: `lm_head_q8` / `lm_head_s8` (float8_e4m3fn [V, H], fp32 [V]) or `lm_head_q4` / `lm_head_e4` (uint8
        [V, H / 2], [V, H / 32]). The fragment-major copy, the prefill's first-token lm_head and decode graphs of more than
        LM_HEAD_FP8_MAX_ROWS / LM_HEAD_MXFP4_MAX_ROWS rows run on W_eff; decode steps of up to that many rows stream the bytes in the
        lm_head launch (greedy, processed, sampling and beam branches alike). Graph keys do not change. The formats are as coarse
        on the head as on the layers (module docstring of tests/test_llm_lm_head_q_gpu.py has the figures) and no text-quality claim
        is made; the default "bf16" adds no tensor, no kernel and no graph key.
        batched_weight_stream=True (needs weight_dtype "fp8" / "mxfp4" and max_batch >= 5): decode steps of more rows than the
        row-major kernels serve, up to FP8_FM_MAX_ROWS / MXFP4_FM_MAX_ROWS, stream the quantised bytes too, through the fragment-major
        MFMA kernels of csrc/gemv_qfm.hip. Every layer gets one more quantised copy of its four matrices, repacked from the bytes the
        engine already holds (`*_q8fm`, or `*_q4fm` / `*_e4fm`; ops.repack_fm_w8 / repack_fm_w4), and those steps run rmsnorm ->
        gemv_fm_w* (qkv, bias) -> attention -> gemv_fm_w* (o, res) -> rmsnorm -> gemv_swiglu_fm_w* -> gemv_fm_w* (down, res): the same
        function of W_eff as the bf16 fragment-major route, in another summation order and with the RMSNorm in a launch of its own
        instead of folded into the weights. The lm_head is not touched. Graph keys do not change; the default False adds no tensor
        and changes no step.
        calibration=dict(input_ids=[n, S], attention_mask=None, damp=0.01) (pass it by name: it sits behind weight_dtype, in front of
        lm_head_dtype and batched_weight_stream, which stay the last two parameters; needs weight_dtype or lm_head_dtype "mxfp4";
        `resolve_calibration` has the rules): the MXFP4 codes are chosen by `quantize_mxfp4_gptq` instead of round to nearest, on
        the Hessians of what each matrix really sees when the engine runs these tokens (`_calibrate`: one sequential pass, every
        layer calibrated behind the already quantised layers before it; ops.gptq_mxfp4, csrc/gptq.hip). Storage, kernels, graphs
        and the "bf16 model on W_eff" property are unchanged -- only the bytes differ. `self.calibration` records method, n_tokens,
        damp and, per quantised matrix, (layer, name, proxy_rtn, proxy_gptq) by `gptq_proxy_loss` (layer None: the lm_head). The
        gain holds on inputs like the calibration set: the plain weight error goes up, inputs unlike the set can fare worse than
        round to nearest (with fewer calibration tokens than a matrix has inputs the Hessians are rank-deficient and held-out
        tokens DO fare worse: profiles/quant_quality_gptq_synthetic.txt), and no text-quality claim is made. FP8 parts keep `quantize_fp8_rows`. A calibrated head cannot be
        quantised again (resize_token_embeddings / load_token_rows raise): build a new engine. The default None changes nothing:
        no tensor, no kernel, no graph key."""
        self.weight_dtype = resolve_weight_dtype(weight_dtype)
        self.lm_head_dtype = resolve_lm_head_dtype(lm_head_dtype)
        self.batched_weight_stream = bool(batched_weight_stream)
        if self.batched_weight_stream:
            if self.weight_dtype == "bf16":
                raise ValueError("batched_weight_stream=True needs weight_dtype 'fp8' or 'mxfp4' (a bf16 engine has no quantised bytes to stream)")
            if max_batch < 5:
                raise ValueError("batched_weight_stream=True needs max_batch >= 5 (up to 4 rows the row-major kernels stream the bytes)")
            m = 128 if self.weight_dtype == "mxfp4" else 64
            if cfg.hidden % m or cfg.inter % m or (cfg.n_q * cfg.head_dim) % m:
                raise ValueError(f"batched_weight_stream=True with weight_dtype={self.weight_dtype!r} needs hidden, inter and n_q * head_dim "
                                 f"to be multiples of {m} (one fragment-major piece is 16 rows x {m} weights)")
        if self.lm_head_dtype == "mxfp4" and cfg.hidden % 32:
            raise ValueError("lm_head_dtype='mxfp4' needs hidden to be a multiple of 32 (one E8M0 scale per block of 32 weights)")
        if self.lm_head_dtype == "fp8" and cfg.hidden % 16:
            raise ValueError("lm_head_dtype='fp8' needs hidden to be a multiple of 16 (16 weights per 16-byte load)")
        if self.weight_dtype == "mxfp4" and (cfg.hidden % 32 or cfg.inter % 32 or (cfg.n_q * cfg.head_dim) % 32):
            raise ValueError("weight_dtype='mxfp4' needs hidden, inter and n_q * head_dim to be multiples of 32 (one E8M0 scale per block of 32 weights)")
        if self.weight_dtype == "fp8" and (cfg.hidden % 16 or cfg.inter % 16 or (cfg.n_q * cfg.head_dim) % 16):
            raise ValueError("weight_dtype='fp8' needs hidden, inter and n_q * head_dim to be multiples of 16 (16 weights per 16-byte load)")
        cal = resolve_calibration(calibration, cfg.vocab, max_len, self.weight_dtype, self.lm_head_dtype)
        self.calibration = None
        cal_layers = cal is not None and self.weight_dtype == "mxfp4"       # (their codes come from _calibrate, below)
        self._cal_head = cal is not None and self.lm_head_dtype == "mxfp4"
        self.cfg, self.device = cfg, torch.device(device)
        self.max_batch, self.max_len = max_batch, max_len
        dv = self.device
        g = lambda k: weights[k].to(device=dv, dtype=BF16).contiguous()
        self.embed_w = g("model.embed_tokens.weight")
        self._head_tied = bool(cfg.tie_embeddings or "lm_head.weight" not in weights)
        self.lm_head = self.embed_w if self._head_tied else g("lm_head.weight")
        if not self._cal_head:
            self._quantize_head()
        self.norm = g("model.norm.weight")
        self.layers = []
        for l in range(cfg.layers):
            p = f"model.layers.{l}."
            lw = dict(
                w_qkv=torch.cat([g(p + "self_attn.q_proj.weight"), g(p + "self_attn.k_proj.weight"),
                                 g(p + "self_attn.v_proj.weight")], 0).contiguous(),
                b_qkv=(torch.cat([g(p + "self_attn.q_proj.bias"), g(p + "self_attn.k_proj.bias"),
                                  g(p + "self_attn.v_proj.bias")], 0).contiguous() if cfg.qkv_bias else None),
                w_o=g(p + "self_attn.o_proj.weight"),
                w_gu=torch.cat([g(p + "mlp.gate_proj.weight"), g(p + "mlp.up_proj.weight")], 0).contiguous(),
                w_down=g(p + "mlp.down_proj.weight"),
                ln1=g(p + "input_layernorm.weight"), ln2=g(p + "post_attention_layernorm.weight"))
            if self.weight_dtype != "bf16" and not cal_layers:
                sq, ss = ROUTES[self.weight_dtype].suffixes
                for k in ("w_qkv", "w_o", "w_gu", "w_down"):     # lw[k] becomes W_eff: what every bf16 kernel of this engine reads
                    lw[k], lw[k + sq], lw[k + ss] = quantize_weight(lw[k], self.weight_dtype)
            self.layers.append(lw)
        if cal is not None:
            self._alloc()       # (the pass needs the rope table and cache set 0 as scratch)
            self._calibrate(cal, cal_layers)
        # Batched decode (5..8 sequences per graph) streams a second, fragment-major copy of every decode weight (ops.repack_fm16:
        # 1 KiB contiguous per wave instruction of the skinny MFMA kernels). Memory is laid out for 288 GB of HBM: the copy
        # costs one more model size (15 GB for the 7B / 8B decoders) and buys 1.4 - 1.6x on the batched weight streams.
        self.fm_batch = max_batch >= self.FM_MIN_BATCH and cfg.hidden % 64 == 0 and cfg.inter % 64 == 0 \
            and (cfg.n_q * cfg.head_dim) % 64 == 0 and os.environ.get("SPIDER_DECODE_FM", "1") != "0"
        if self.fm_batch:
            for lw in self.layers:     # the projections behind a LlamaRMSNorm carry its weight (fold_rmsnorm form of the kernels)
                lw["w_qkv_fm"] = ops.repack_fm16(lw["w_qkv"], lw["ln1"])
                lw["w_gu_fm"] = ops.repack_fm16(lw["w_gu"], lw["ln2"])
                lw["w_o_fm"] = ops.repack_fm16(lw["w_o"])
                lw["w_down_fm"] = ops.repack_fm16(lw["w_down"])
            self.lm_head_fm = ops.repack_fm16(self.lm_head, self.norm)
        if self.batched_weight_stream:      # the third encoding of W_eff: the engine's own bytes in fragment-major order
            for lw in self.layers:
                for k in ("w_qkv", "w_o", "w_gu", "w_down"):
                    if self.weight_dtype == "fp8":
                        lw[k + "_q8fm"] = ops.repack_fm_w8(lw[k + "_q8"])
                    else:
                        lw[k + "_q4fm"], lw[k + "_e4fm"] = ops.repack_fm_w4(lw[k + "_q4"], lw[k + "_e4"])
        if cal is None:
            self._alloc()

    def _quantize_head(self):
        """lm_head_dtype="fp8" / "mxfp4": quantise the head's source -- the embedding matrix of a tied configuration, else the head
        matrix itself, where both quantisers are fixed points in values -- and make `lm_head` its W_eff beside the bytes"""
        if self.lm_head_dtype == "bf16":
            return
        if self._cal_head:
            raise ValueError("the lm_head of this engine was calibrated (calibration=...): its codes depend on the calibration pass and "
                             "cannot be derived again after the vocabulary changed; build a new engine")
        src = self.embed_w if self._head_tied else self.lm_head
        self.lm_head, q, sc = quantize_weight(src, self.lm_head_dtype)
        for suffix, t in zip(ROUTES[self.lm_head_dtype].suffixes, (q, sc)):
            setattr(self, "lm_head" + suffix, t)

    # ------------------------------------------------------------------ construction helpers
    @classmethod
    def random_init(cls, cfg: LLMConfig, device="cuda:0", max_batch=1, max_len=4096, seed=0, std=0.02, weight_dtype="bf16",
                    calibration=None, lm_head_dtype="bf16", batched_weight_stream=False):
        """Random N(0, std^2) weights of the architecture's true shapes, created directly in HBM
        (init scheme of modeling_llama3.py:405-414). Used by bench.py: timing is weight-value independent."""
        gen = torch.Generator(device=device).manual_seed(seed)
        r = lambda *s: (torch.randn(*s, generator=gen, device=device, dtype=torch.float32) * std).to(BF16)
        one = lambda n: torch.ones(n, device=device, dtype=BF16)
        w = {"model.embed_tokens.weight": r(cfg.vocab, cfg.hidden), "model.norm.weight": one(cfg.hidden)}
        if not cfg.tie_embeddings:
            w["lm_head.weight"] = r(cfg.vocab, cfg.hidden)
        qd, kd = cfg.n_q * cfg.head_dim, cfg.n_kv * cfg.head_dim
        for l in range(cfg.layers):
            p = f"model.layers.{l}."
            w[p + "self_attn.q_proj.weight"] = r(qd, cfg.hidden)
            w[p + "self_attn.k_proj.weight"] = r(kd, cfg.hidden)
            w[p + "self_attn.v_proj.weight"] = r(kd, cfg.hidden)
            w[p + "self_attn.o_proj.weight"] = r(cfg.hidden, qd)
            if cfg.qkv_bias:
                w[p + "self_attn.q_proj.bias"] = r(qd)
                w[p + "self_attn.k_proj.bias"] = r(kd)
                w[p + "self_attn.v_proj.bias"] = r(kd)
            w[p + "mlp.gate_proj.weight"] = r(cfg.inter, cfg.hidden)
            w[p + "mlp.up_proj.weight"] = r(cfg.inter, cfg.hidden)
            w[p + "mlp.down_proj.weight"] = r(cfg.hidden, cfg.inter)
            w[p + "input_layernorm.weight"] = one(cfg.hidden)
            w[p + "post_attention_layernorm.weight"] = one(cfg.hidden)
        return cls(cfg, w, device, max_batch, max_len, weight_dtype=weight_dtype, lm_head_dtype=lm_head_dtype,
                   batched_weight_stream=batched_weight_stream, calibration=calibration)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", max_batch=1, max_len=4096, weight_dtype="bf16", calibration=None,
                        lm_head_dtype="bf16", batched_weight_stream=False):
        """Load an HF checkpoint directory: config.json + model.safetensors(.index.json + shards) or pytorch_model.bin
        (spider_amd/checkpoint.py). From a Qwen2.5-Omni directory only `thinker.model.*` / `thinker.lm_head.*` are read.
        weight_dtype="fp8" / "mxfp4" quantise the layer matrices at load, lm_head_dtype="fp8" / "mxfp4" the lm_head (see the
        constructor); batched_weight_stream=True adds the fragment-major quantised copies for decode graphs of 5..8 rows;
        calibration=dict(input_ids=...) chooses the MXFP4 codes by GPTQ on those tokens (see the constructor)."""
        from .checkpoint import load_state_dict, read_config

        def keep(k: str):
            kk = k.replace("thinker.model.", "model.").replace("thinker.lm_head.", "lm_head.")
            return kk if kk.startswith(("model.", "lm_head.")) else None
        cfg = LLMConfig.from_hf_dict(read_config(path))
        eng = cls(cfg, load_state_dict(path, keep=keep), device, max_batch, max_len, weight_dtype=weight_dtype,
                  lm_head_dtype=lm_head_dtype, batched_weight_stream=batched_weight_stream, calibration=calibration)
        eng.generation_config = read_generation_config(path)
        return eng

    @torch.no_grad()
    def _calibrate(self, cal: dict, cal_layers: bool):
        """The sequential calibration pass behind `calibration=`: `_prefill`'s layer loop over ALL calibration rows, in chunks of at
        most max_batch sequences with cache set 0 as scratch; the residual stream of every row is kept between layers. In front of
        each matrix the Hessian H = sum x x^T of its input rows (fp64 sums on the device; rows that attention_mask pads do not
        enter) is summed, the matrix is quantised by ops.gptq_mxfp4 and REPLACED by its W_eff with the bytes beside it, and the
        stream moves on through the quantised matrix: later matrices are calibrated on what the earlier ones really produce.
        cal_layers False (weight_dtype is not "mxfp4"): the layers run as they are and only the head is calibrated, on the
        Hessian of rmsnorm(h_final, norm)."""
        c, dv, B = self.cfg, self.device, self.max_batch
        ids = cal["input_ids"].to(dv)
        n, S = ids.shape
        am = cal["attention_mask"]
        am_d = am.to(dv).to(torch.int32) if am is not None else torch.ones(n, S, dtype=torch.int32, device=dv)
        pos2d = (am_d.cumsum(-1) - 1).clamp(min=0).to(torch.int32).contiguous()
        slot = torch.arange(S, dtype=torch.int32, device=dv)[None].expand(B, S).contiguous().view(-1)
        kv_beg = (S - am_d.sum(-1)).to(torch.int32).contiguous()
        has_pad = am is not None and bool((am == 0).any())
        real = am_d.view(-1).bool() if has_pad else None
        chunks = [(a, min(a + B, n)) for a in range(0, n, B)]
        record = []

        def hessian(x):
            H = torch.zeros(x.shape[1], x.shape[1], dtype=torch.float64, device=dv)
            xs = x[real] if real is not None else x
            for a in range(0, xs.shape[0], 4096):
                x64 = xs[a:a + 4096].double()
                H.addmm_(x64.t(), x64)
            return (H + H.t()) * 0.5

        def quantise(W, x, layer, name):
            H = hessian(x)
            q, sc = ops.gptq_mxfp4(W, H, cal["damp"])
            W_eff = dequantize_mxfp4(q, sc).contiguous()
            rtn = dequantize_mxfp4(*quantize_mxfp4(W))
            record.append((layer, name, gptq_proxy_loss(W, rtn, H), gptq_proxy_loss(W, W_eff, H)))
            return W_eff, q, sc

        def rows(fn, width):        # a row-wise stage over all sequences, chunk by chunk
            out = torch.empty(n * S, width, dtype=BF16, device=dv)
            for a, b in chunks:
                out[a * S:b * S] = fn(a * S, b * S)
            return out
        h = self.embed_tokens(ids).view(n * S, -1)
        k_cache, v_cache = self._kv(0)
        for l, lw in enumerate(self.layers):
            def put(k, x):
                if cal_layers:
                    lw[k], lw[k + "_q4"], lw[k + "_e4"] = quantise(lw[k], x, l, k)
            x = rows(lambda a, b: ops.rmsnorm(h[a:b], lw["ln1"], c.eps), c.hidden)
            put("w_qkv", x)
            att = torch.empty(n * S, c.n_q * c.head_dim, dtype=BF16, device=dv)
            for a, b in chunks:
                nb = b - a
                qkv = ops.gemm(x[a * S:b * S], lw["w_qkv"], bias=lw["b_qkv"])
                q = torch.empty(nb, S, c.n_q, c.head_dim, dtype=BF16, device=dv)
                ops.rope_kv_append(qkv, pos2d[a:b].contiguous().view(-1), slot[:nb * S], self.cos_sin, q, k_cache[l], v_cache[l], nb, S,
                                   c.n_q, c.n_kv, c.head_dim)
                att[a * S:b * S] = ops.attention_cache(q, k_cache[l], v_cache[l], Lk=S, causal=True, kv_off=0,
                                                       kv_beg=kv_beg[a:b].contiguous() if has_pad else None).view(nb * S, -1)
            put("w_o", att)
            h = rows(lambda a, b: ops.gemm(att[a:b], lw["w_o"], res=h[a:b]), c.hidden)
            x = rows(lambda a, b: ops.rmsnorm(h[a:b], lw["ln2"], c.eps), c.hidden)
            put("w_gu", x)
            if _FUSE_SWIGLU:
                act = rows(lambda a, b: ops.gemm(x[a:b], lw["w_gu"], act="swiglu"), c.inter)
            else:
                act = rows(lambda a, b: ops.swiglu(ops.gemm(x[a:b], lw["w_gu"])), c.inter)
            put("w_down", act)
            h = rows(lambda a, b: ops.gemm(act[a:b], lw["w_down"], res=h[a:b]), c.hidden)
        if self._cal_head:
            x = rows(lambda a, b: ops.rmsnorm(h[a:b], self.norm, c.eps), c.hidden)
            src = self.embed_w if self._head_tied else self.lm_head
            W_eff, q, sc = quantise(src, x, None, "lm_head")
            self.lm_head, self.lm_head_q4, self.lm_head_e4 = W_eff, q, sc
        k_cache.zero_(); v_cache.zero_()        # (scratch use over: the cache a new engine hands out is zero)
        self.calibration = dict(method="gptq", n_tokens=cal["n_tokens"], damp=cal["damp"], matrices=record)

    def _alloc(self):
        c, dv, B, T = self.cfg, self.device, self.max_batch, self.max_len
        self.k_cache = torch.zeros(c.layers, B, c.n_kv, T, c.head_dim, dtype=BF16, device=dv)
        self.v_cache = torch.zeros_like(self.k_cache)
        # KV cache sets: set 0 is the engine's cache; further sets (allocated on first use) let TWO requests be in flight at once --
        # the prefill of one on one stream while another decodes on a second stream (SpiderFreeInfer's three-stage pipelining)
        self._kv_sets = [(self.k_cache, self.v_cache)]
        self.cos_sin = rope_table(c, max(c.max_pos, T)).to(dv)
        self._graphs = {}
        self._beam_kv_tmp = {}      # cache set -> second K / V buffer of the beam-search reorder (allocated by the first beam request)
        self.last_prompt_lookup = None      # dict(steps=, drafted=, accepted=) of the last decode_finish when it was a prompt-lookup request, else None
        self.last_assisted = None           # the same record of the last decode_finish when it was an assistant_model request, else None

    def _kv(self, cache_set: int):
        while len(self._kv_sets) <= cache_set:
            self._kv_sets.append((torch.zeros_like(self.k_cache), torch.zeros_like(self.v_cache)))
        return self._kv_sets[cache_set]

    # ------------------------------------------------------------------ embeddings
    def embed_tokens(self, ids: torch.Tensor) -> torch.Tensor:
        return ops.embed(self.embed_w, ids.to(device=self.device, dtype=torch.int32).contiguous())

    def resize_token_embeddings(self, new_num_tokens: Optional[int] = None, std: float = 0.02, seed: Optional[int] = None):
        """`PreTrainedModel.resize_token_embeddings` as the reference calls it after adding its signal tokens to the tokenizer
        (spider.py:177: `self.llama_model.resize_token_embeddings(len(self.llama_tokenizer))`): the input embedding and -- unless
        tied -- the lm_head grow (or shrink) to `new_num_tokens` rows. Old rows keep their values; new rows are N(0, std^2), the
        `_init_weights` rule of the pinned transformers 4.43 (modeling_llama3.py:405-414) -- a trained Spider checkpoint then
        overwrites them (`load_token_rows`). Captured decode graphs and the vocabulary-sized buffers are rebuilt on the next call.
        Returns the embedding matrix, like the HF method returns the embedding module."""
        c = self.cfg
        old = self.embed_w.shape[0]
        if new_num_tokens is None or new_num_tokens == old:
            return self.embed_w
        if new_num_tokens <= 0:
            raise ValueError(f"resize_token_embeddings: new_num_tokens={new_num_tokens}")
        gen = None
        if seed is not None:
            gen = torch.Generator(device=self.device).manual_seed(seed)

        def grow(w):
            out = torch.empty(new_num_tokens, w.shape[1], dtype=w.dtype, device=w.device)
            n = min(old, new_num_tokens)
            out[:n] = w[:n]
            if new_num_tokens > old:
                out[old:] = (torch.randn(new_num_tokens - old, w.shape[1], generator=gen, device=w.device, dtype=torch.float32) * std).to(w.dtype)
            return out.contiguous()
        quant = self.lm_head_dtype != "bf16"    # a quantised head is a matrix of its own: the configuration says whether it is tied
        tied = self._head_tied if quant else self.lm_head is self.embed_w
        self.embed_w = grow(self.embed_w)
        if not tied:
            self.lm_head = grow(self.lm_head)
        elif not quant:
            self.lm_head = self.embed_w     # (a tied quantised head is re-derived from embed_w by _vocab_changed)
        import dataclasses
        self.cfg = dataclasses.replace(c, vocab=new_num_tokens)     # (the config object may be shared with other engines)
        self._vocab_changed()
        return self.embed_w

    def load_token_rows(self, first_row: int, embed_rows: Optional[torch.Tensor] = None, lm_head_rows: Optional[torch.Tensor] = None):
        """Overwrite rows [first_row, first_row + n) of the input embedding and / or the lm_head: the trained rows a Spider
        checkpoint stores for its signal tokens (the reference keeps `old_embed_tokens` / `old_lm_head` copies for exactly
        this split, spider.py:165-173). With a quantised head (lm_head_dtype) the rows land in the matrix a bf16 engine would
        write -- the embedding matrix of a tied configuration, else the head -- and the head is quantised again from it."""
        head = self.embed_w if (self.lm_head_dtype != "bf16" and self._head_tied) else self.lm_head
        for w, rows, name in ((self.embed_w, embed_rows, "embed_rows"), (head, lm_head_rows, "lm_head_rows")):
            if rows is None:
                continue
            if rows.ndim != 2 or rows.shape[1] != w.shape[1] or first_row < 0 or first_row + rows.shape[0] > w.shape[0]:
                raise ValueError(f"load_token_rows: {name} {tuple(rows.shape)} does not fit rows [{first_row}, ...) of {tuple(w.shape)}")
            w[first_row:first_row + rows.shape[0]] = rows.to(device=w.device, dtype=w.dtype)
        self._vocab_changed()

    @staticmethod
    def _state_key(B: int, output_hidden_states: bool, return_logits: bool, cache_set: int, processed: bool = False,
                   beam: Optional[tuple] = None, sample: bool = False, ngram: bool = False, lookup: int = 0, assist: int = 0) -> tuple:
        """key of a decode state + captured graph; requests with logits processors have their own (one more element), and so have
        beam-search requests (B = batch rows; beam = (num_beams, continuations kept per step): three more elements), sampling
        requests ("sample", behind the processors' element), requests with no_repeat_ngram_size ("ngram" as the last element;
        they are processed requests), prompt-lookup requests (lookup = K > 0 drafts: "lookup" and the K + 1 rows of the step;
        one graph serves every max_matching_ngram_size) and assistant_model requests (assist = K > 0 drafts: "assist" and the K + 1
        rows of the verify step; the state remembers its draft engine)"""
        key = (int(B), bool(output_hidden_states), bool(return_logits), int(cache_set))
        if assist:
            return key + ("assist", int(assist) + 1)
        if lookup:
            return key + ("lookup", int(lookup) + 1)
        if beam is not None:
            return key + ("beam", int(beam[0]), int(beam[1]))
        key = key + (True,) if (processed or ngram) else key
        key = key + ("sample",) if sample else key
        return key + ("ngram",) if ngram else key

    def would_capture(self, B: int, output_hidden_states: bool = False, return_logits: bool = False, cache_set: int = 0,
                      processed: bool = False, num_beams: int = 1, n_eos: int = 0, do_sample: bool = False,
                      no_repeat_ngram: bool = False, prompt_lookup_num_tokens: Optional[int] = None,
                      num_assistant_tokens: Optional[int] = None) -> bool:
        """True when the decode loop of such a request would capture its hipGraph (state missing or not captured yet).
        processed: a request with non-neutral logits processors (repetition_penalty != 1, a ban set, or EOS banned at first)
        num_beams > 1: a beam-search request of B batch rows with n_eos EOS ids (they size the continuations kept per step)
        do_sample: a sampling request (one graph serves every temperature / top_k / top_p / seed)
        no_repeat_ngram: a request with no_repeat_ngram_size > 0 (one graph serves every size)
        prompt_lookup_num_tokens: a prompt-lookup request of that many drafts (one graph per K serves every max_matching_ngram_size)
        num_assistant_tokens: an assistant_model request of that many drafts (one graph per K holds the whole round of both engines;
        a call with another draft engine captures again)"""
        beam = (num_beams, max(2, 1 + n_eos) * num_beams) if num_beams > 1 else None
        ent = self._graphs.get(self._state_key(B, output_hidden_states, return_logits, cache_set, processed, beam, bool(do_sample),
                                               bool(no_repeat_ngram), int(prompt_lookup_num_tokens or 0), int(num_assistant_tokens or 0)))
        return ent is None or ent[1] is None

    def _vocab_changed(self):
        """the lm_head moved or changed: drop what was derived from it (fragment-major copy, captured decode graphs, lm_head
        workspaces and logits buffers, all keyed in self._graphs); a quantised head is quantised again from its source first
        (rows nobody touched keep their W_eff values: both quantisers are fixed points in values)"""
        self._quantize_head()
        if self.fm_batch:
            self.lm_head_fm = ops.repack_fm16(self.lm_head, self.norm)
        self._graphs = {}
        self._beam_kv_tmp = {}      # held by the beam states just dropped

    # ------------------------------------------------------------------ prefill
    def _prefill(self, h: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor, kv_beg: Optional[torch.Tensor],
                 B: int, S: int, hidden_out: Optional[list], mrope: bool = False, cache_set: int = 0):
        """h [B*S, H] bf16; pos [B*S] (or [3, B*S] with mrope); writes KV slots, returns the final residual stream [B*S, H]."""
        c = self.cfg
        k_cache, v_cache = self._kv(cache_set)
        sec = c.mrope_section if mrope else None
        if hidden_out is not None:
            hidden_out.append(h.view(B, S, -1).clone())
        for l, lw in enumerate(self.layers):
            x = ops.rmsnorm(h, lw["ln1"], c.eps)
            qkv = ops.gemm(x, lw["w_qkv"], bias=lw["b_qkv"])
            q = torch.empty(B, S, c.n_q, c.head_dim, dtype=BF16, device=self.device)
            ops.rope_kv_append(qkv, pos, slot, self.cos_sin, q, k_cache[l], v_cache[l], B, S, c.n_q, c.n_kv, c.head_dim,
                               mrope_section=sec)
            a = ops.attention_cache(q, k_cache[l], v_cache[l], Lk=S, causal=True, kv_off=0, kv_beg=kv_beg)
            h = ops.gemm(a.view(B * S, -1), lw["w_o"], res=h)
            x = ops.rmsnorm(h, lw["ln2"], c.eps)
            if _FUSE_SWIGLU:
                act = ops.gemm(x, lw["w_gu"], act="swiglu")  # gate / up projection with SwiGLU in the epilogue (no [S, 2I] round trip)
            else:
                act = ops.swiglu(ops.gemm(x, lw["w_gu"]))
            h = ops.gemm(act, lw["w_down"], res=h)
            if hidden_out is not None:
                hidden_out.append(h.view(B, S, -1).clone())
        return h

    # ------------------------------------------------------------------ one decode step (graph-capturable)
    def _decode_step(self, st: dict):
        c, B = self.cfg, st["B"]
        k_cache, v_cache = st["kv"]
        h = ops.embed(self.embed_w, st["cur_ids"]) if st["embeds_in"] is None else st["embeds_in"]
        hs = st.get("hidden_buf")
        if hs is not None:
            hs[0].copy_(h)
        layer, norm, *head = self._decode_route(B)
        route = ROUTES[layer]

        def proj(op, lw, k, x, N=None, norm_key=None, **kw):
            """one layer GEMV on this step's route: ops.<op> on the route's encoding of lw[k]; norm_key: behind that RMSNorm"""
            if norm_key is not None and norm == NORM_ARG:
                kw.update(norm_w=lw[norm_key], eps=c.eps)
            elif norm_key is not None and norm == NORM_FOLDED:
                kw["norm_eps"] = c.eps
            elif norm_key is not None:
                x = ops.rmsnorm(x, lw[norm_key], c.eps, out=st["xn"])
            rows = (N,) if route.fm and N is not None else ()
            return getattr(ops, op)(*(lw[k + s] for s in route.suffixes), x, *rows, **kw)
        lookup = st.get("lookup")     # prompt-lookup verify step: the layer loop below at B = R rows, attention under the causal rule
        # a step of an assisted round (`_assist_round`: the target's verify step, the draft engine's two-row and single-row steps): it
        # ends behind the lm_head, the round's own launches move the cursors; more than one row are rows of ONE sequence, as above
        assist = st.get("assist")
        one_seq = lookup is not None or (assist is not None and B > 1)
        for l, lw in enumerate(self.layers):
            proj(route.gemv, lw, "w_qkv", h, lw["w_qkv"].shape[0], norm_key="ln1", bias=lw["b_qkv"], out=st["qkv"])
            if one_seq:     # the B rows are ONE sequence's token and its drafts: R appended K / V rows, row r sees r more of them
                ops.rope_kv_append(st["qkv"], st["pos"], st["slot"], self.cos_sin, st["q"], k_cache[l], v_cache[l],
                                   1, B, c.n_q, c.n_kv, c.head_dim)
                ops.attn_verify(st["q"], k_cache[l], v_cache[l], st["kv_end"], B, kv_beg=st["kv_beg"], nsplit=st["nsplit"],
                                ws=st["attn_ws"], out=st["attn"])
            elif c.head_dim == 128:   # RoPE + KV append + split-KV attention + combine: one launch
                ops.attn_decode_fused(st["qkv"], st["pos"], self.cos_sin, k_cache[l], v_cache[l], st["kv_end"],
                                      st["kv_beg"], st["attn_cnt"], c.n_q, st["nsplit"], st["attn_ws"], st["attn"])
            else:
                ops.rope_kv_append(st["qkv"], st["pos"], st["slot"], self.cos_sin, st["q"], k_cache[l], v_cache[l],
                                   B, 1, c.n_q, c.n_kv, c.head_dim)
                ops.attn_decode(st["q"], k_cache[l], v_cache[l], st["kv_end"], kv_beg=st["kv_beg"],
                                nsplit=st["nsplit"], ws=st["attn_ws"], out=st["attn"])
            h1 = proj(route.gemv, lw, "w_o", st["attn"], c.hidden, res=h, out=st["h1"])
            proj(route.swiglu, lw, "w_gu", h1, norm_key="ln2", out=st["act"])
            h = proj(route.gemv, lw, "w_down", st["act"], c.hidden, res=h1, out=st["h2"][l & 1])
            if hs is not None:
                hs[l + 1].copy_(h)
        if assist is not None:      # the model's token behind every row; pushes / advance follow in `_assist_round`
            self._lm_head_step(st, h, st["next_ids"], None, None, head)
            return
        if lookup is not None:      # the model's token behind every row, then accept / append / advance / draft in one launch
            self._lm_head_step(st, h, st["next_ids"], None, None, head)
            ops.spec_advance_draft(lookup, st["hist"], st["n_hist"])
            return
        if st.get("beam") is not None:      # beam search: the raw logits of the B * K rows go to the beam step instead of an arg-max
            self._lm_head_step(st, h, st["beam"]["lm_ids"], st["logits"], None, head)
            self._beam_step(st)
            return
        proc = st.get("proc")      # logits processors in the arg-max epilogue (their parameters are read from the state's buffers)
        if st.get("sample") is not None:    # sampling: the raw logits go to the sampling step, which applies the processors itself
            self._lm_head_step(st, h, st["sample"]["lm_ids"], st["logits"], None, head)
            self._sample_step(st)
        else:
            self._lm_head_step(st, h, st["next_ids"], st.get("logits"), proc, head)
        if hs is not None:  # HF reports the normed state as the last hidden state (modeling_llama3.py:619-623)
            ops.rmsnorm(h, self.norm, c.eps, out=hs[c.layers])
        # advance the device-side cursors and append the token to the on-device history (index math only, one launch)
        if st.get("ngram_bufs") is not None:    # ... and the same launch scans the sequence for the next step's n-gram bans
            ops.decode_advance_seen_ngram(st["next_ids"], st["cur_ids"], st["pos"], st["slot"], st["kv_end"], st["seen"], c.vocab,
                                          st["hist"], st["n_hist"], st["ngram_bufs"])
        elif proc is not None:    # ... and the token joins the sequence's `seen` set before the next step's lm_head
            ops.decode_advance_seen(st["next_ids"], st["cur_ids"], st["pos"], st["slot"], st["kv_end"], st["seen"], c.vocab,
                                    st["hist"], st["n_hist"])
        else:
            ops.decode_advance(st["next_ids"], st["cur_ids"], st["pos"], st["slot"], st["kv_end"], st["hist"], st["n_hist"])

    def _decode_route(self, B: int) -> tuple:
        """(layer route, its norm mode, head route, its norm mode) of a B-row decode step: keys of ROUTES and NORM_* values. Read at
        the top of every step from the engine's settings and the row ranges as they are at that moment.
        Layers: weight_dtype "fp8" / "mxfp4" engines stream the bytes row-major up to FP8_MAX_ROWS / MXFP4_MAX_ROWS rows (the norm fused
        while the rows fit the kernel's LDS budget, else in a launch of its own); batched_weight_stream engines above that, up to
        *_FM_MAX_ROWS rows, the same bytes in fragment-major order (csrc/gemv_qfm.hip; a quantised matrix cannot carry the norm);
        everything else is bf16 -- fragment-major from FM_MIN_BATCH rows of an engine with the copies, which carry the norm's
        weight, else row-major, whose GEMV fuses the norm for up to 4 rows.
        Head: lm_head_dtype "fp8" / "mxfp4" engines stream its bytes up to LM_HEAD_*_MAX_ROWS rows (csrc/lm_head_wq.hip), everything
        else is the bf16 route of that row count -- whatever the layers take."""
        H = self.cfg.hidden
        fm = self.fm_batch and B >= self.FM_MIN_BATCH
        q = QUANT.get(self.weight_dtype)
        if q and B <= min(getattr(self, q.rows), getattr(ops, q.op_rows)):
            layer = (self.weight_dtype, NORM_ARG if getattr(ops, q.norm_fits)(B, H) else NORM_LAUNCH)
        elif q and self.batched_weight_stream and B <= min(getattr(self, q.fm_rows), ops.QFM_MAX_ROWS):
            layer = (self.weight_dtype + "_fm", NORM_LAUNCH)
        elif fm:
            layer = ("bf16_fm", NORM_FOLDED)
        else:
            layer = ("bf16", NORM_ARG if B < 5 else NORM_LAUNCH)
        q = QUANT.get(self.lm_head_dtype)
        if q and B <= min(getattr(self, q.head_rows), ops.LM_HEAD_Q_MAX_ROWS):
            head = (self.lm_head_dtype, NORM_ARG if getattr(ops, q.norm_fits)(B, H) else NORM_LAUNCH)
        else:
            head = ("bf16_fm", NORM_FOLDED) if fm else ("bf16", NORM_ARG)
        return layer + head

    def _lm_head_step(self, st: dict, h: torch.Tensor, out_ids: torch.Tensor, logits: Optional[torch.Tensor], proc: Optional[dict],
                      head: Sequence[str]):
        """The lm_head launch of a decode step: final norm + lm_head + arg-max (through `proc` when given) of the residual stream h
        into out_ids, raw logits into `logits` when given, on head = (route, norm mode) of `_decode_route`."""
        c, (name, norm) = self.cfg, head
        route = ROUTES[name]
        if route.fm:
            args, kw = (h, c.vocab), dict(norm_eps=c.eps)
        elif norm == NORM_LAUNCH:   # (a hidden size beyond the kernel's LDS budget)
            args, kw = (ops.rmsnorm(h, self.norm, c.eps, out=st["xn"]),), dict(eps=c.eps)
        else:
            args, kw = (h,), dict(norm_w=self.norm, eps=c.eps)
        if proc is not None:
            args += (proc,)
        getattr(ops, route.head if proc is None else route.head_proc)(
            *(getattr(self, "lm_head" + s) for s in route.suffixes), *args, out_ids=out_ids, ws=st["lm_ws"], logits=logits, **kw)

    def _sample_step(self, st: dict):
        """Behind the raw-logits lm_head of a sampling step (graph-capturable, no host sync): st["next_ids"] = one draw per row from
        the processed, temperature / top-k / top-p warped distribution, at step n_hist[row] (`sample_token_host`)."""
        ops.sample_partial(st["logits"], st["sample"], st.get("proc"))
        ops.sample_select(st["sample"], st["n_hist"], st["next_ids"], self.cfg.vocab)

    def _beam_step(self, st: dict, reorder: bool = True):
        """Behind the lm_head of a beam-search step (graph-capturable, no host sync): the C best continuations of every batch row go
        to the trace, the first K non-EOS ones become the running beams (scores, tokens), the KV rows follow their source beams and
        the cursors advance. reorder=False: selection only (step 0, whose rows are still the un-expanded prompt rows)."""
        bm, c = st["beam"], self.cfg
        ops.beam_partial(st["logits"], bm["C"], bm["ws"])
        ops.beam_select(bm["ws"], bm["run"], bm["eos_ids"], bm["n_eos"], st["n_hist"], bm["trace"], bm["src_beam"], st["next_ids"],
                        c.vocab, bm["C"])
        if reorder:
            ops.kv_row_gather(st["kv"][0], st["kv"][1], bm["kv_tmp"][0], bm["kv_tmp"][1], bm["src_beam"], st["kv_beg"], st["kv_end"],
                              bm["K"])
            ops.decode_advance(st["next_ids"], st["cur_ids"], st["pos"], st["slot"], st["kv_end"], st["hist"], st["n_hist"])

    _PROC_BUFS = ("seen", "ban", "penalty", "min_new", "eos_ids", "n_eos")
    _NGRAM_BUFS = ("prompt_ids", "n_prompt", "ngram", "ban_step")

    def _make_state(self, B: int, want_hidden: bool, want_logits: bool, cache_set: int = 0, processed: bool = False,
                    beam: Optional[tuple] = None, sample: bool = False, ngram: bool = False) -> dict:
        c, dv = self.cfg, self.device
        nq_d = c.n_q * c.head_dim
        # one split-KV block per CU (256): measured on Qwen-7B shapes at T~1.6k: 2.93 / 2.90 / 3.14 ms per token at 32 / 64 / 96 splits
        nsplit = max(1, min(64, 256 // max(1, B * c.n_kv)))
        if os.environ.get("SPIDER_ATTN_NSPLIT"):       # tuning aid
            nsplit = int(os.environ["SPIDER_ATTN_NSPLIT"])
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dv)
        bf = lambda *s: torch.empty(*s, dtype=BF16, device=dv)
        npart = ops.lm_head_nparts(c.vocab)
        st = dict(B=B, nsplit=nsplit, cur_ids=i32(B), next_ids=i32(B), pos=i32(B), slot=i32(B), kv_end=i32(B), kv_beg=i32(B),
                  qkv=bf(B, (c.n_q + 2 * c.n_kv) * c.head_dim), q=bf(B, c.n_q, c.head_dim), attn=bf(B, nq_d),
                  h1=bf(B, c.hidden), h2=[bf(B, c.hidden), bf(B, c.hidden)], act=bf(B, c.inter), xn=bf(B, c.hidden),
                  attn_ws=(torch.empty(B * c.n_q * nsplit * c.head_dim, dtype=torch.float32, device=dv),
                           torch.empty(B * c.n_q * nsplit * 2, dtype=torch.float32, device=dv)),
                  lm_ws=(torch.empty(B * npart, dtype=torch.float32, device=dv), i32(B * npart)),
                  attn_cnt=i32(B * c.n_kv), embeds_in=None, hist=i32(B, self.max_len), n_hist=i32(B), kv=self._kv(cache_set))
        if want_hidden:
            st["hidden_buf"] = bf(c.layers + 1, B, c.hidden)
        if want_logits:
            st["logits"] = bf(B, c.vocab)
        if processed:   # token bitmaps (uint32 words kept as int32) and the processors' parameters, all read by the kernels at run time
            W = ops.bitmap_words(c.vocab)
            st.update(seen=i32(B, W), ban=i32(B, W), penalty=torch.ones(1, dtype=torch.float32, device=dv), min_new=i32(1),
                      eos_ids=i32(MAX_EOS_IDS), n_eos=i32(1))
            st["proc"] = {k: st[k] for k in self._PROC_BUFS + ("n_hist",)}
        if ngram:       # no_repeat_ngram_size: the row's prompt ids, the size, and the per-step ban bitmap (static bans | n-gram bans)
            st.update(prompt_ids=i32(B, self.max_len), n_prompt=i32(1), ngram=i32(1), ban_step=i32(B, W))
            st["proc"]["ban"] = st["ban_step"]      # what the lm_head and sampling kernels read as the ban set
            st["ngram_bufs"] = {k: st[k] for k in self._NGRAM_BUFS + ("ban",)}
        if sample:     # the parameters, workspace and outputs of the two sampling launches (the logits buffer is always there)
            st["sample"] = dict(ops.sample_state(B, c.vocab, dv), lm_ids=i32(B))
        if beam is not None:    # B = batch rows * K here. The trace holds max_len steps; the second KV buffer belongs to the cache set
            K, C = beam
            nb = B // K
            if cache_set not in self._beam_kv_tmp:
                self._beam_kv_tmp[cache_set] = (torch.zeros_like(self.k_cache), torch.zeros_like(self.v_cache))
            st["beam"] = dict(K=K, C=C, run=torch.zeros(nb, K, dtype=torch.float32, device=dv), src_beam=i32(nb, K), lm_ids=i32(B),
                              eos_ids=i32(MAX_EOS_IDS), n_eos=i32(1), ws=ops.beam_workspace(B, c.vocab, C, dv),
                              trace=(torch.zeros(self.max_len, nb, C, dtype=torch.float32, device=dv), i32(self.max_len, nb, C),
                                     i32(self.max_len, nb, C)),
                              kv_tmp=self._beam_kv_tmp[cache_set])
        return st

    def _make_lookup_state(self, R: int, cache_set: int = 0) -> dict:
        """decode state of a prompt-lookup request: the activations and step cursors (cur_ids = the rows' input ids, next_ids = the
        model's token behind every row, pos, slot) of R = K + 1 rows, the cache cursors and token history of ONE sequence, and under
        "lookup" the buffers of ops.spec_advance_draft / ops.prompt_lookup_draft"""
        st = self._make_state(R, False, False, cache_set)
        dv = self.device
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dv)
        st.update(kv_end=i32(1), kv_beg=i32(1), hist=i32(1, self.max_len), n_hist=i32(1), first=i32(1))
        st["lookup"] = dict(prompt_ids=i32(1, self.max_len), n_prompt=i32(1), ngram=i32(1), k_draft=i32(1), n_draft=i32(1),
                            counters=torch.zeros(1, 3, dtype=torch.int64, device=dv), ids=st["cur_ids"], pos=st["pos"],
                            slot=st["slot"], lm_out=st["next_ids"], kv_end=st["kv_end"])
        return st

    _LOOKUP_BUFS = ("prompt_ids", "n_prompt", "ngram", "k_draft", "n_draft", "counters")

    # ------------------------------------------------------------------ public generate
    @torch.no_grad()
    def generate(self, input_ids: Optional[torch.Tensor] = None, inputs_embeds: Optional[torch.Tensor] = None, **kw):
        """Greedy decode = `prefill_begin` + `decode_finish` back to back (arguments: see prefill_begin)."""
        h = self.prefill_begin(input_ids, inputs_embeds, _whole_generate=True, **kw)
        return self.decode_finish(h) if isinstance(h, _PrefillHandle) else h

    @torch.no_grad()
    def prefill_begin(self, input_ids: Optional[torch.Tensor] = None, inputs_embeds: Optional[torch.Tensor] = None,
                      attention_mask: Optional[torch.Tensor] = None, max_new_tokens: Optional[int] = None,
                      stopping_criteria: Optional[Sequence[Callable]] = None, eos_token_id=None, pad_token_id=None,
                      output_hidden_states: bool = False, return_dict_in_generate: bool = False,
                      num_beams: int = 1, do_sample: bool = False, use_cache: bool = True, output_attentions: bool = False,
                      use_graph: bool = True, sync_every: int = 1, return_logits: bool = False,
                      position_ids: Optional[torch.Tensor] = None, cache_set: int = 0, repetition_penalty=1.0, min_length=0,
                      min_new_tokens=0, suppress_tokens=None, bad_words_ids=None, length_penalty=1.0, early_stopping=False,
                      num_return_sequences=1, num_beam_groups=1, constraints=None, force_words_ids=None, temperature=1.0,
                      top_k=None, top_p=1.0, seed=None, no_repeat_ngram_size=None, prompt_lookup_num_tokens=None,
                      max_matching_ngram_size=None, assistant_model=None, num_assistant_tokens=None,
                      num_assistant_tokens_schedule=None, assistant_confidence_threshold=None, _whole_generate=False, _row0=0,
                      **unused):
        """First half of `generate`: the prompt pass (KV cache of `cache_set` filled, first token chosen, decode cursors set), all
        ENQUEUED on the current stream without a host sync; returns a handle for `decode_finish`. Two requests can be in flight on
        two streams when they use different cache sets (prefill of one beside the decode loop of the other: SpiderFreeInfer's
        three-stage pipelining); the caller orders `decode_finish(h)` after this call's stream work. More than DECODE_ROWS rows: the
        whole grouped generate runs here and its result is returned instead of a handle.

        Greedy decode. Left-padded batches are described by attention_mask (0 = pad), as
        prepare_generation_embedding does (spider.py:1658-1661). `sync_every` > 1 checks the stop
        conditions only every N tokens (one device->host copy per check instead of per token).
        position_ids [3, B, S]: multimodal (t, h, w) rotary positions of the prompt (Qwen2.5-Omni thinker with image / audio
        embeddings spliced into inputs_embeds; cfg.mrope_section required). Generated tokens continue at
        max(position_ids) + 1 on all three components, as transformers' rope_deltas bookkeeping does.
        eos_token_id / pad_token_id / max_new_tokens default to the checkpoint's generation config (HF behaviour):
        a row is finished at its first EOS and padded with pad_token_id afterwards; the call returns when every row is
        finished. More than DECODE_ROWS (8) rows are processed in groups of 8 (rows are independent).
        repetition_penalty / min_length / min_new_tokens / suppress_tokens / bad_words_ids (single-token entries): transformers'
        logits processors of the same names (`resolve_logits_processors`), applied on the device before the arg-max. Keyword
        arguments only -- they are not read from the checkpoint's generation config. Neutral values (1.0, no EOS ban, empty ban
        set) run the unprocessed kernels and decode graph.
        no_repeat_ngram_size=n (an int >= 1; None / 0 = off): transformers' NoRepeatNGramLogitsProcessor -- a token that would complete
        an n-gram already in the row's sequence gets -inf (`ngram_banned_host` is the definition; the sequence is the one the penalty
        sees: input_ids row, pads included, + generated tokens; the generated tokens alone for inputs_embeds). Greedy and
        do_sample=True; num_beams > 1 raises. Such a request is a processed one with a state and graph of its own (one for every n):
        the launch that closes a decode step also scans the row's history into the next step's ban bitmap. Measured on an MI355X,
        Qwen2.5-7B shapes, context 1536, against the same processed request without the keyword (scripts/exp/ngram_cost.py, medians
        of 3 alternated rounds of 96 replays, rounds within 1.3 us of each other): 1 row 2722.7 -> 2726.9 us per step (+4.1 us),
        8 rows 3471.9 -> 3479.4 us (+7.6 us).
        num_beams > 1 (2..8, batch * num_beams <= DECODE_ROWS and <= max_batch): transformers' beam search with length_penalty,
        early_stopping (False / True / "never") and num_return_sequences. The beam step runs on the device inside the decode graph
        and `beam_finalize_host` replays HF's finished-hypotheses bookkeeping at the `sync_every` points. Only `generate` accepts it
        (its decode loop syncs with the host, so there is no handle to return): a direct prefill_begin(num_beams > 1) raises.
        `generate` returns sequences [B * num_return_sequences, ...], with return_dict_in_generate also
        sequences_scores and beam_indices, with return_logits the running beams' raw logits [B * num_beams, n, V]. Sampling, user
        stopping_criteria, output_hidden_states, non-neutral logits processors, beam groups and constraints raise.
        do_sample=True (num_beams = 1; conversation.py:151-173 always asks for it): one seeded draw per row and step from the
        distribution HF's processors and its temperature / top_k / top_p warpers leave, chosen on the device inside the decode graph
        (`sample_token_host` is the definition; `resolve_sampling` the accepted ground: top_k 1..64, None = HF's default). Keyword
        arguments only. The token of row r at step n depends on (seed, r, n) and the logits alone -- not on graph / eager,
        sync_every, the split path, the cache set or the grouping of more than 8 rows. seed=None draws the seed from torch's default
        CPU generator (torch.manual_seed makes the call reproducible). do_sample=False ignores the three warper arguments.
        prompt_lookup_num_tokens=K (an int 1..7; None / 0 = off) with max_matching_ngram_size=N (1..8, default 2): transformers'
        prompt-lookup decoding for one greedy sequence (`resolve_prompt_lookup` is the served ground). Every decode step carries the
        last accepted token and up to K tokens drafted from an earlier occurrence of the sequence's last n-gram
        (`prompt_lookup_draft_host`; the sequence is the input_ids row + generated tokens, the generated tokens alone for
        inputs_embeds) as K + 1 rows of the weight streams, verifies them in one pass (csrc/spec_decode.hip) and keeps the prefix the
        model agrees with plus the model's own next token (`spec_accept_host`): 1 .. K + 1 tokens per step, and the sequence is the
        greedy one. A state and graph of its own per K. The counters dict(steps=, drafted=, accepted=) of the call are
        `GenerateOutput.prompt_lookup` and `last_prompt_lookup`; with sync_every > 1 they include the steps that ran past the stop.
        assistant_model=draft_engine (a second LlamaEngine of the same tokenizer family; None = off) with num_assistant_tokens=K (an
        int 1..7, default 5): transformers' assisted decoding for one greedy sequence through `generate` (`resolve_assisted` is the
        served ground; num_assistant_tokens_schedule takes None / "constant", assistant_confidence_threshold None / 0). The draft
        engine prefills the same input_ids and attention_mask into its own cache set 0; every round it proposes K tokens -- one
        two-row step on the sequence's last two tokens, which also catches its cache up whatever the last round accepted, then K - 1
        single-row steps -- the engine verifies them as K + 1 rows exactly as for prompt lookup, and one launch accepts, appends,
        advances and hands the draft engine its next two rows (csrc/spec_assist.hip, `assisted_round_host`). The whole round is one
        captured graph, keyed by K and bound to its draft engine. The sequence is the engine's greedy one whatever the draft engine
        proposes. Its vocabulary may be smaller than the engine's: an id it does not have is fed to it as id 0, to it alone. The
        counters dict(steps=, drafted=, accepted=) of the call (steps = rounds) are `GenerateOutput.assisted` and `last_assisted`;
        with sync_every > 1 they include the rounds that ran past the stop. `GenerateOutput.prompt_lookup` stays None."""
        sampling = resolve_sampling(do_sample, temperature, top_k, top_p, num_return_sequences) if num_beams == 1 else None
        ngram = resolve_no_repeat_ngram(no_repeat_ngram_size)
        if sampling is not None:
            seed = resolve_seed(seed)
        c, dv = self.cfg, self.device
        gc = getattr(self, "generation_config", None) or {}
        if eos_token_id is None:
            eos_token_id = gc.get("eos_token_id")
        if pad_token_id is None:
            pad_token_id = gc.get("pad_token_id")
        embeds_only = input_ids is None
        S_in = inputs_embeds.shape[1] if embeds_only else input_ids.shape[1]
        if max_new_tokens is None:   # HF: generation_config.max_new_tokens, else max_length (default 20) counts the prompt
            max_new_tokens = gc.get("max_new_tokens") or max(1, int(gc.get("max_length", 20)) - (0 if embeds_only else S_in))
        B_all = inputs_embeds.shape[0] if embeds_only else input_ids.shape[0]
        lookup = None       # (K, N) of a prompt-lookup request
        if not prompt_lookup_off(prompt_lookup_num_tokens):
            pen, min_new, ban = resolve_logits_processors(S_in, _id_list(eos_token_id), repetition_penalty, min_length, min_new_tokens,
                                                          suppress_tokens, bad_words_ids)
            lookup = resolve_prompt_lookup(prompt_lookup_num_tokens, max_matching_ngram_size, B_all, S_in, max_new_tokens, self.max_len,
                                           self.DECODE_ROWS, c.head_dim, bool(do_sample), num_beams,
                                           pen != 1.0 or min_new > 0 or bool(ban), ngram, output_hidden_states, return_logits)
        assist = None       # K of an assistant_model request
        if (assistant_model is not None or num_assistant_tokens is not None or num_assistant_tokens_schedule is not None
                or assistant_confidence_threshold is not None):
            if assistant_model is not None and position_ids is not None:
                raise NotImplementedError("assistant_model with position_ids is not implemented: the draft engine has no multimodal prompt")
            pen, min_new, ban = resolve_logits_processors(S_in, _id_list(eos_token_id), repetition_penalty, min_length, min_new_tokens,
                                                          suppress_tokens, bad_words_ids)
            assist = resolve_assisted(assistant_model, num_assistant_tokens, num_assistant_tokens_schedule, assistant_confidence_threshold,
                                      self, B_all, S_in, max_new_tokens, self.DECODE_ROWS, bool(do_sample), num_beams,
                                      pen != 1.0 or min_new > 0 or bool(ban), ngram, output_hidden_states, return_logits,
                                      prompt_lookup_num_tokens, embeds_only, _whole_generate)
        beam = None
        if num_beams != 1 and not _whole_generate:
            raise NotImplementedError("num_beams > 1 runs through LlamaEngine.generate only: the split prefill_begin / adopt / decode_finish "
                                      "path (SpiderFreeInfer's pipelining, QwenOmniThinker) is greedy")
        if num_beams != 1:
            pen, min_new, ban = resolve_logits_processors(S_in, _id_list(eos_token_id), repetition_penalty, min_length, min_new_tokens,
                                                          suppress_tokens, bad_words_ids)
            C_keep = resolve_beam_search(B_all, num_beams, self.max_batch, c.vocab, _id_list(eos_token_id), self.DECODE_ROWS, do_sample,
                                         stopping_criteria, output_hidden_states, pen != 1.0 or min_new > 0 or bool(ban) or ngram > 0,
                                         num_beam_groups, constraints, force_words_ids, num_return_sequences, length_penalty,
                                         early_stopping)
            beam = (num_beams, C_keep)
        if B_all > self.DECODE_ROWS:
            return self._generate_grouped(input_ids, inputs_embeds, attention_mask, position_ids, B_all, dict(
                max_new_tokens=max_new_tokens, stopping_criteria=stopping_criteria, eos_token_id=eos_token_id,
                pad_token_id=pad_token_id, output_hidden_states=output_hidden_states, use_graph=use_graph,
                sync_every=sync_every, return_logits=return_logits, cache_set=cache_set, repetition_penalty=repetition_penalty,
                min_length=min_length, min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens,
                bad_words_ids=bad_words_ids, no_repeat_ngram_size=ngram,
                **(dict(do_sample=True, temperature=sampling[0], top_k=sampling[1], top_p=sampling[2], seed=seed)
                   if sampling is not None else {})), return_dict_in_generate)
        if embeds_only:
            h0 = inputs_embeds.to(device=dv, dtype=BF16).contiguous()
            B, S = h0.shape[0], h0.shape[1]
        else:
            input_ids = input_ids.to(dv)
            B, S = input_ids.shape
            h0 = self.embed_tokens(input_ids)
        if B > self.max_batch or S + max_new_tokens > self.max_len:
            raise ValueError(f"batch {B} / length {S}+{max_new_tokens} exceed the preallocated KV cache "
                             f"({self.max_batch} x {self.max_len})")
        eos_l = _id_list(eos_token_id)
        pen, min_new, ban = resolve_logits_processors(S, eos_l, repetition_penalty, min_length, min_new_tokens, suppress_tokens,
                                                      bad_words_ids)
        processed = pen != 1.0 or min_new > 0 or bool(ban) or ngram > 0
        am = (attention_mask.to(dv).to(torch.int32) if attention_mask is not None
              else torch.ones(B, S, dtype=torch.int32, device=dv))
        pos2d = (am.cumsum(-1) - 1).clamp(min=0).to(torch.int32).contiguous()
        slot2d = torch.arange(S, dtype=torch.int32, device=dv)[None].expand(B, S).contiguous()
        kv_beg = (S - am.sum(-1)).to(torch.int32).contiguous()     # first valid slot (left padding)
        has_pad = attention_mask is not None and bool((am == 0).any())

        hidden_steps: Optional[List] = [] if output_hidden_states else None
        step0: Optional[list] = [] if output_hidden_states else None
        if position_ids is not None:
            if c.mrope_section is None:
                raise ValueError("position_ids with 3 components need a model with mrope_section (Qwen2.5-Omni thinker)")
            if tuple(position_ids.shape) != (3, B, S):
                raise ValueError(f"position_ids must be [3, {B}, {S}], got {tuple(position_ids.shape)}")
            pos3 = position_ids.to(device=dv, dtype=torch.int32).contiguous()
            h = self._prefill(h0.view(B * S, -1), pos3.view(3, -1), slot2d.view(-1), kv_beg if has_pad else None, B, S, step0, mrope=True,
                              cache_set=cache_set)
            # left-padded rows: the pad slots carry a dummy position (get_rope_index writes 1 there) and are masked by kv_beg
            next_pos = torch.where(am.bool()[None], pos3, torch.zeros_like(pos3)).amax(dim=(0, 2)) + 1
        else:
            h = self._prefill(h0.view(B * S, -1), pos2d.view(-1), slot2d.view(-1), kv_beg if has_pad else None, B, S, step0,
                              cache_set=cache_set)
            next_pos = pos2d[:, -1] + 1
        if beam is not None:
            return self._beam_decode(beam, h.view(B, S, -1)[:, -1], next_pos, kv_beg, B, S, None if embeds_only else input_ids,
                                     max_new_tokens, eos_l, pad_token_id, float(length_penalty), early_stopping, num_return_sequences,
                                     return_dict_in_generate, use_graph, max(1, int(sync_every)), return_logits, cache_set)

        if lookup is not None:
            return self._lookup_begin(lookup, h.view(B, S, -1)[:, -1].contiguous(), next_pos, kv_beg, S, embeds_only, input_ids,
                                      max_new_tokens, stopping_criteria, eos_token_id, pad_token_id, return_dict_in_generate,
                                      use_graph, sync_every, cache_set)

        if assist is not None:
            # the draft engine's prompt pass: the same slots, positions and padding, ids it does not have as id 0
            d = assistant_model
            d_ids = torch.where(input_ids < d.cfg.vocab, input_ids, torch.zeros_like(input_ids))
            d._prefill(d.embed_tokens(d_ids).view(B * S, -1), pos2d.view(-1), slot2d.view(-1), kv_beg if has_pad else None, B, S, None)
            return self._assist_begin(assist, d, d_ids, h.view(B, S, -1)[:, -1].contiguous(), next_pos, kv_beg, S, input_ids,
                                      max_new_tokens, stopping_criteria, eos_token_id, pad_token_id, return_dict_in_generate,
                                      use_graph, sync_every, cache_set)

        # decode state (static buffers + captured hipGraph) is cached per (batch, outputs): repeated generate() calls
        # replay the same graph instead of re-capturing ~200 launches
        sample = sampling is not None
        skey = self._state_key(B, output_hidden_states, return_logits, cache_set, processed, None, sample, ngram > 0)
        if skey not in self._graphs:
            self._graphs[skey] = [self._make_state(B, output_hidden_states, return_logits or sample, cache_set, processed, None,
                                                   sample, ngram > 0), None]
        st = self._graphs[skey][0]
        st["kv_beg"].copy_(kv_beg)
        last = h.view(B, S, -1)[:, -1].contiguous()
        if sample:      # this request's values; rows of a grouped call keep their absolute index in the call
            ops.sample_set_params(st["sample"], *sampling, seed, int(_row0))
            st["n_hist"].zero_()        # step 0: no token generated yet
        if processed:
            # this request's processor parameters and token sets go into the state's buffers (the captured graph reads them there);
            # the penalised set starts as every id of the row's input_ids, pads included -- empty for an inputs_embeds call (HF)
            st["penalty"].fill_(pen)
            st["min_new"].fill_(min_new)
            st["n_eos"].fill_(len(eos_l) if (eos_l and min_new > 0) else 0)
            if eos_l and min_new > 0:
                st["eos_ids"].copy_(torch.tensor(eos_l + [-1] * (MAX_EOS_IDS - len(eos_l)), dtype=torch.int32))
            st["seen"].zero_()
            st["ban"].zero_()
            st["n_hist"].zero_()        # step 0: no token generated yet
            if not embeds_only:
                ops.token_bitmap_set(input_ids.to(torch.int32).contiguous(), st["seen"], c.vocab)
            if ban:
                ops.token_bitmap_set(torch.tensor(ban, dtype=torch.int32, device=dv)[None].expand(B, -1).contiguous(), st["ban"], c.vocab)
            if ngram > 0:
                # the n-gram scan reads the row's input_ids (pads included, as HF's processor does; none for inputs_embeds) in front
                # of the generated tokens; the bans of the first token come from the prompt alone (n_hist = 0)
                st["ngram"].fill_(ngram)
                st["n_prompt"].fill_(0 if embeds_only else S)
                if not embeds_only:
                    st["prompt_ids"][:, :S].copy_(input_ids)
                ops.ngram_ban(st["ngram_bufs"], st["hist"], st["n_hist"], c.vocab)
            if not sample:
                ops.lm_head_argmax_proc(self.lm_head, last, st["proc"], norm_w=self.norm, eps=c.eps, out_ids=st["next_ids"],
                                        ws=st["lm_ws"], logits=st.get("logits"))
        elif not sample:
            ops.lm_head_argmax(self.lm_head, last, norm_w=self.norm, eps=c.eps, out_ids=st["next_ids"], ws=st["lm_ws"],
                               logits=st.get("logits"))
        if sample:      # the first token is drawn by the same two launches as every later one, at step 0
            ops.lm_head_argmax(self.lm_head, last, norm_w=self.norm, eps=c.eps, out_ids=st["sample"]["lm_ids"], ws=st["lm_ws"],
                               logits=st["logits"])
            self._sample_step(st)
        if processed:
            ops.token_bitmap_set(st["next_ids"].view(B, 1), st["seen"], c.vocab)
        if output_hidden_states:
            step0[-1] = ops.rmsnorm(h, self.norm, c.eps).view(B, S, -1)
            hidden_steps.append(tuple(step0))
        st["cur_ids"].copy_(st["next_ids"])
        st["pos"].copy_(next_pos)
        st["slot"].fill_(S)
        st["kv_end"].fill_(S + 1)

        # generated ids live in the decode state's history buffer: every decode step appends its token there itself
        # (decode_advance), so the loop below issues nothing but the graph replay
        if max_new_tokens > st["hist"].shape[1]:
            raise ValueError(f"max_new_tokens={max_new_tokens} exceeds the engine's max_len={st['hist'].shape[1]}")
        tokens = st["hist"][:, :max_new_tokens]
        tokens[:, 0].copy_(st["next_ids"])
        st["n_hist"].fill_(1)
        if ngram > 0:   # the bans of the first decode step; every later step's come from its predecessor's advance launch
            ops.ngram_ban(st["ngram_bufs"], st["hist"], st["n_hist"], c.vocab)
        logits_steps = [st["logits"].clone()] if return_logits else None
        return _PrefillHandle(B=B, S=S, st=st, skey=skey, embeds_only=embeds_only, input_ids=input_ids, max_new_tokens=max_new_tokens,
                              stopping_criteria=stopping_criteria, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
                              output_hidden_states=output_hidden_states, return_dict_in_generate=return_dict_in_generate,
                              use_graph=use_graph, sync_every=sync_every, return_logits=return_logits, hidden_steps=hidden_steps,
                              logits_steps=logits_steps, tokens=tokens)

    # ------------------------------------------------------------------ teacher-forced scoring
    SCORE_SCRATCH_BYTES = 320 << 20     # bf16 logits scratch of one chunk (1024 rows at V = 152064)
    SCORE_CHUNK_ROWS = None             # rows per chunk; None = sized from the scratch and the GEMM's 2 GiB output limit

    def _score_head(self):
        """the lm_head as `score` multiplies it: [ld, H] with ld = V rounded up to 8, so that the logits rows are 16-byte groups and
        the GEMM runs its usual N % 8 == 0 forms whatever the vocabulary. A vocabulary that is a multiple of 8 uses `lm_head`
        itself; any other gets a copy with zero rows appended (their logits are 0 and never read), rebuilt when the head changes."""
        W = self.lm_head
        V, H = W.shape
        ld = (V + 7) // 8 * 8
        if ld == V:
            return W, ld
        tag = (W.data_ptr(), W._version, V)
        cached = getattr(self, "_score_head_pad", None)
        if cached is None or cached[0] != tag:
            Wp = torch.zeros(ld, H, dtype=BF16, device=self.device)
            Wp[:V].copy_(W)
            self._score_head_pad = cached = (tag, Wp)
        return cached[1], ld

    def _score_logits(self, input_ids, inputs_embeds, attention_mask, position_ids, B, S, cache_set):
        """the prompt pass of `prefill_begin` on these inputs: the final residual stream [B * S, H]"""
        dv = self.device
        h0 = (inputs_embeds.to(device=dv, dtype=BF16).contiguous() if input_ids is None else self.embed_tokens(input_ids.to(dv)))
        am = (attention_mask.to(dv).to(torch.int32) if attention_mask is not None else torch.ones(B, S, dtype=torch.int32, device=dv))
        pos2d = (am.cumsum(-1) - 1).clamp(min=0).to(torch.int32).contiguous()
        slot2d = torch.arange(S, dtype=torch.int32, device=dv)[None].expand(B, S).contiguous()
        kv_beg = (S - am.sum(-1)).to(torch.int32).contiguous()
        has_pad = attention_mask is not None and bool((am == 0).any())
        if position_ids is not None:
            pos3 = position_ids.to(device=dv, dtype=torch.int32).contiguous()
            return self._prefill(h0.view(B * S, -1), pos3.view(3, -1), slot2d.view(-1), kv_beg if has_pad else None, B, S, None, mrope=True,
                                 cache_set=cache_set)
        return self._prefill(h0.view(B * S, -1), pos2d.view(-1), slot2d.view(-1), kv_beg if has_pad else None, B, S, None,
                             cache_set=cache_set)

    @torch.no_grad()
    def score(self, input_ids: Optional[torch.Tensor] = None, inputs_embeds: Optional[torch.Tensor] = None,
              attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None,
              labels: Optional[torch.Tensor] = None, other: Optional["LlamaEngine"] = None, cache_set: int = 0,
              return_logits: bool = False) -> ScoreOutput:
        """Teacher-forced pass: the `logits` / `loss` half of LlamaForCausalLM.forward(input_ids, labels=...), and the divergence
        from a second engine. The inputs follow the rules of `prefill_begin` (left padding by attention_mask, position_ids
        [3, B, S] with mrope_section, B <= max_batch, S <= max_len; `resolve_score` raises ValueError naming the argument).
        labels [B, S] default to input_ids and are required with inputs_embeds alone; positions with attention_mask == 0 or label
        -100 are ignored, labels >= vocab raise (`score_targets`).
        The prompt pass runs as in `prefill_begin` (it fills the KV cache of `cache_set`); the rows of the final residual stream
        then go in chunks through the final RMSNorm, the lm_head GEMM into a bf16 scratch [chunk, ld] and `ops.logprob_rows`
        (csrc/logprob.hip): bf16 logits, then an fp32 log-softmax -- HF's arithmetic. A quantised engine (weight_dtype /
        lm_head_dtype) is exactly a bf16 model on W_eff, which is what this pass multiplies: it measures that model exactly.
        other: a second LlamaEngine of the same vocabulary on the same device (else ValueError) runs the same inputs through its own
        prompt pass (its cache set 0) and is the REFERENCE distribution: kl = KL(other || self) per position, mean_kl, top1_agree.
        return_logits=True (tests and small cases: B * S * V bf16) also returns the logits [B, S, V].
        `score_host` is the definition of every field of the result. No decode state or captured graph is made or touched."""
        c, dv = self.cfg, self.device
        B, S, tg = resolve_score(c.vocab, c.hidden, self.max_batch, self.max_len, c.mrope_section is not None, input_ids, inputs_embeds,
                                 attention_mask, position_ids, labels)
        if other is not None:
            if not isinstance(other, LlamaEngine) or other.cfg.vocab != c.vocab or other.device != dv:
                raise ValueError("other must be a LlamaEngine of the same vocabulary on the same device")
            if input_ids is None and other.cfg.hidden != c.hidden:
                raise ValueError("other: scoring inputs_embeds against a second engine needs the same hidden size")
            if B > other.max_batch or S > other.max_len:
                raise ValueError(f"other: batch {B} / length {S} exceed its preallocated KV cache ({other.max_batch} x {other.max_len})")
        if int(cache_set) < 0:
            raise ValueError(f"cache_set={cache_set}")
        V = c.vocab
        R = B * S
        nxt = torch.full_like(tg, IGNORE_INDEX)
        nxt[:, :-1] = tg[:, 1:]                     # the label row (b, s) of the logits is scored against
        targets = nxt.to(device=dv, dtype=torch.int32).view(-1).contiguous()
        engines = [self] if other is None or other is self else [self, other]
        hs = [e._score_logits(input_ids, inputs_embeds, attention_mask, position_ids, B, S, cache_set if e is self else 0) for e in engines]
        heads = [e._score_head() for e in engines]
        ld = heads[0][1]
        chunk = self.SCORE_CHUNK_ROWS or max(1, min(1024, self.SCORE_SCRATCH_BYTES // (2 * ld), ((1 << 31) - 1) // (2 * ld)))
        chunk = min(int(chunk), R)
        scratch = [torch.empty(chunk, ld, dtype=BF16, device=dv) for _ in engines]
        f32 = lambda: torch.empty(R, dtype=torch.float32, device=dv)
        i32 = lambda: torch.empty(R, dtype=torch.int32, device=dv)
        res = dict(logprob=f32(), argmax=i32(), entropy=f32())
        if other is not None:
            res["kl"], res["argmax_ref"] = f32(), i32()
        full = torch.empty(R, V, dtype=BF16, device=dv) if return_logits else None
        for a in range(0, R, chunk):
            n = min(chunk, R - a)
            for e, h, (W, _), sc in zip(engines, hs, heads, scratch):
                ops.gemm(ops.rmsnorm(h[a:a + n], e.norm, e.cfg.eps), W, out=sc[:n])
            ref = None if other is None else scratch[-1][:n]        # (other is self: the same rows are their own reference)
            o = ops.logprob_rows(scratch[0][:n], targets[a:a + n], V, logits_ref=ref)
            for k in res:
                res[k][a:a + n].copy_(o[k])
            if full is not None:
                full[a:a + n].copy_(scratch[0][:n, :V])
        v = lambda k: res[k].view(B, S)
        return _score_assemble(tg, v("logprob"), v("argmax").to(torch.int64), v("entropy"), v("kl") if other is not None else None,
                               v("argmax_ref").to(torch.int64) if other is not None else None,
                               full.view(B, S, V) if full is not None else None)

    def _lookup_begin(self, lookup, last, next_pos, kv_beg, S, embeds_only, input_ids, max_new_tokens, stopping_criteria,
                      eos_token_id, pad_token_id, return_dict_in_generate, use_graph, sync_every, cache_set) -> "_PrefillHandle":
        """Behind the prompt pass of a prompt-lookup request (one sequence; `last` [1, H] is its final residual at the last position):
        the first token, the cursors of row 0, this request's K / N and prompt ids in the state's buffers, and the draft of the first
        verify step -- all enqueued, no host sync."""
        c = self.cfg
        K, N = lookup
        skey = self._state_key(1, False, False, cache_set, lookup=K)
        if skey not in self._graphs:
            self._graphs[skey] = [self._make_lookup_state(K + 1, cache_set), None]
        st = self._graphs[skey][0]
        lk = st["lookup"]
        st["kv_beg"].copy_(kv_beg)
        ops.lm_head_argmax(self.lm_head, last, norm_w=self.norm, eps=c.eps, out_ids=st["first"], ws=st["lm_ws"])
        st["cur_ids"][:1].copy_(st["first"])
        st["pos"][:1].copy_(next_pos)
        st["slot"][:1].fill_(S)
        st["kv_end"].fill_(S + 1)
        st["hist"][:, :1].copy_(st["first"].view(1, 1))
        st["n_hist"].fill_(1)
        lk["ngram"].fill_(N)
        lk["k_draft"].fill_(K)
        lk["counters"].zero_()
        lk["n_prompt"].fill_(0 if embeds_only else S)       # with inputs_embeds only, the lookup runs over the generated tokens alone
        if not embeds_only:
            lk["prompt_ids"][:, :S].copy_(input_ids)
        ops.prompt_lookup_draft(lk, st["hist"], st["n_hist"])
        return _PrefillHandle(B=1, S=S, st=st, skey=skey, embeds_only=embeds_only, input_ids=input_ids, max_new_tokens=max_new_tokens,
                              stopping_criteria=stopping_criteria, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
                              output_hidden_states=False, return_dict_in_generate=return_dict_in_generate, use_graph=use_graph,
                              sync_every=sync_every, return_logits=False, hidden_steps=None, logits_steps=None,
                              tokens=st["hist"][:, :max_new_tokens], lookup=lookup)

    def _make_assist_state(self, K: int, draft: "LlamaEngine", cache_set: int = 0) -> dict:
        """decode state of an assistant_model request: the activations and step cursors of the K + 1 verify rows and the cache
        cursors and token history of ONE sequence (as `_make_lookup_state`), and under "assist" the draft engine with its two
        decode states -- `d2`, the two-row catch-up step, and `d1`, the single-row step -- and the buffers of the hand-off launches"""
        st = self._make_state(K + 1, False, False, cache_set)
        dv = self.device
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dv)
        st.update(kv_end=i32(1), kv_beg=i32(1), hist=i32(1, self.max_len), n_hist=i32(1), first=i32(1))
        d2, d1 = draft._make_state(2, False, False, 0), draft._make_state(1, False, False, 0)
        d2.update(kv_end=i32(1), kv_beg=i32(1), assist=True)
        d1.update(assist=True)
        st["assist"] = dict(K=K, draft=draft, draft_graphs=draft._graphs, d2=d2, d1=d1, n_draft=i32(1),
                            counters=torch.zeros(1, 3, dtype=torch.int64, device=dv),
                            sp=None, tgt=dict(ids=st["cur_ids"], pos=st["pos"], slot=st["slot"]),
                            src2=dict(out=d2["next_ids"], pos=d2["pos"], slot=d2["slot"]),
                            src1=dict(out=d1["next_ids"], pos=d1["pos"], slot=d1["slot"]),
                            dst=dict(ids=d1["cur_ids"], pos=d1["pos"], slot=d1["slot"], kv_end=d1["kv_end"]),
                            catch_up=dict(ids=d2["cur_ids"], pos=d2["pos"], slot=d2["slot"], kv_end=d2["kv_end"]))
        a = st["assist"]
        a["sp"] = dict(lm_out=st["next_ids"], ids=st["cur_ids"], pos=st["pos"], slot=st["slot"], kv_end=st["kv_end"],
                       n_draft=a["n_draft"], counters=a["counters"])
        return st

    def _assist_round(self, st: dict):
        """One round of assisted decoding (graph-capturable, no host sync): the draft engine's two-row step on the sequence's last
        two tokens, whose second arg-max is draft 1, K - 1 single-row steps for the other drafts -- every draft pushed into its row
        of the verify step and into the draft engine's next row --, the verify step on K + 1 rows, and the closing launch."""
        a = st["assist"]
        d, K, vd = a["draft"], a["K"], a["draft"].cfg.vocab
        d._decode_step(a["d2"])
        ops.spec_assist_push(a["src2"], 1, a["tgt"], 1, a["dst"], vd)
        for j in range(2, K + 1):
            d._decode_step(a["d1"])
            ops.spec_assist_push(a["src1"], 0, a["tgt"], j, a["dst"], vd)
        self._decode_step(st)
        ops.spec_assist_advance(a["sp"], st["hist"], st["n_hist"], a["catch_up"], vd)

    def _assist_begin(self, K, draft, d_ids, last, next_pos, kv_beg, S, input_ids, max_new_tokens, stopping_criteria, eos_token_id,
                      pad_token_id, return_dict_in_generate, use_graph, sync_every, cache_set) -> "_PrefillHandle":
        """Behind the two prompt passes of an assistant_model request (one sequence; `last` [1, H] is the engine's final residual at
        the last position, d_ids the prompt as the draft engine read it): the first token, the cursors of row 0, and the draft
        engine's first catch-up rows [input_ids[-1], first token] -- all enqueued, no host sync."""
        c = self.cfg
        skey = self._state_key(1, False, False, cache_set, assist=K)
        ent = self._graphs.get(skey)
        if ent is None or ent[0]["assist"]["draft"] is not draft or ent[0]["assist"]["draft_graphs"] is not draft._graphs:
            # (another draft engine, or one whose head moved -- `_vocab_changed` starts a new `_graphs`: the captured round holds the
            # old launches)
            self._graphs[skey] = ent = [self._make_assist_state(K, draft, cache_set), None]
        st = ent[0]
        a = st["assist"]
        d2 = a["d2"]
        st["kv_beg"].copy_(kv_beg)
        d2["kv_beg"].copy_(kv_beg)
        a["d1"]["kv_beg"].copy_(kv_beg)
        ops.lm_head_argmax(self.lm_head, last, norm_w=self.norm, eps=c.eps, out_ids=st["first"], ws=st["lm_ws"])
        st["cur_ids"][:1].copy_(st["first"])
        st["pos"][:1].copy_(next_pos)
        st["slot"][:1].fill_(S)
        st["kv_end"].fill_(S + 1)
        st["hist"][:, :1].copy_(st["first"].view(1, 1))
        st["n_hist"].fill_(1)
        a["n_draft"].fill_(K)
        a["counters"].zero_()
        d2["cur_ids"][:1].copy_(d_ids[0, -1:])
        d2["cur_ids"][1:].copy_(torch.where(st["first"] < draft.cfg.vocab, st["first"], torch.zeros_like(st["first"])))
        d2["pos"][:1].copy_(next_pos - 1)
        d2["pos"][1:].copy_(next_pos)
        d2["slot"].copy_(torch.tensor([S - 1, S], dtype=torch.int32))
        d2["kv_end"].fill_(S)
        return _PrefillHandle(B=1, S=S, st=st, skey=skey, embeds_only=False, input_ids=input_ids, max_new_tokens=max_new_tokens,
                              stopping_criteria=stopping_criteria, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
                              output_hidden_states=False, return_dict_in_generate=return_dict_in_generate, use_graph=use_graph,
                              sync_every=sync_every, return_logits=False, hidden_steps=None, logits_steps=None,
                              tokens=st["hist"][:, :max_new_tokens], assist=K)

    @torch.no_grad()
    def adopt(self, hd: "_PrefillHandle", cache_set: int = 0) -> "_PrefillHandle":
        """Move a prefilled request into KV cache set `cache_set` (device copies of the prompt's K / V rows and of the decode cursors,
        enqueued on the current stream) and return the handle bound to that set. Used by SpiderFreeInfer's three-stage pipelining: the
        prompt pass of request k+2 fills a STAGING set while request k+1 decodes from set 0; before its own decode loop the request is
        adopted into set 0, so every decode loop replays the ONE decode graph of set 0 (a second graph executable alive in the
        process was measured to put the two-stream schedule into a time-slicing regime: every kernel + 10-25 us, step 513 -> 920 ms)."""
        src = hd.skey[3]
        if src == cache_set:
            return hd
        B, S = hd.B, hd.S
        if getattr(hd, "lookup", None) is not None:     # a prompt-lookup request: its row-0 cursors, drafted rows and lookup buffers
            skey = self._state_key(1, False, False, cache_set, lookup=hd.lookup[0])
            if skey not in self._graphs:
                self._graphs[skey] = [self._make_lookup_state(hd.lookup[0] + 1, cache_set), None]
            dst, st = self._graphs[skey][0], hd.st
            (ks, vs), (kd, vd) = self._kv(src), self._kv(cache_set)
            kd[:, :1, :, :S + 1].copy_(ks[:, :1, :, :S + 1])
            vd[:, :1, :, :S + 1].copy_(vs[:, :1, :, :S + 1])
            for k in ("cur_ids", "next_ids", "pos", "slot", "kv_end", "kv_beg", "n_hist", "first"):
                dst[k].copy_(st[k])
            for k in self._LOOKUP_BUFS:
                dst["lookup"][k].copy_(st["lookup"][k])
            dst["hist"][:, :1].copy_(st["hist"][:, :1])
            nd = _PrefillHandle(**hd.__dict__)
            nd.st, nd.skey, nd.tokens = dst, skey, dst["hist"][:, :hd.max_new_tokens]
            return nd
        processed, sample, ngram = hd.skey[4:5] == (True,), "sample" in hd.skey[4:], "ngram" in hd.skey[4:]
        skey = self._state_key(B, hd.output_hidden_states, hd.return_logits, cache_set, processed, None, sample, ngram)
        if skey not in self._graphs:
            self._graphs[skey] = [self._make_state(B, hd.output_hidden_states, hd.return_logits or sample, cache_set, processed, None,
                                                   sample, ngram), None]
        dst, st = self._graphs[skey][0], hd.st
        (ks, vs), (kd, vd) = self._kv(src), self._kv(cache_set)
        kd[:, :B, :, :S + 1].copy_(ks[:, :B, :, :S + 1])
        vd[:, :B, :, :S + 1].copy_(vs[:, :B, :, :S + 1])
        for k in (("cur_ids", "next_ids", "pos", "slot", "kv_end", "kv_beg", "n_hist") + (self._PROC_BUFS if processed else ())
                  + (self._NGRAM_BUFS if ngram else ())):
            dst[k].copy_(st[k])
        dst["hist"][:, :1].copy_(st["hist"][:, :1])
        for k in ("logits", "hidden_buf"):
            if k in st:
                dst[k].copy_(st[k])
        if sample:
            for k in ("temperature", "top_p", "top_k", "seed", "row0"):
                dst["sample"][k].copy_(st["sample"][k])
        nd = _PrefillHandle(**hd.__dict__)
        nd.st, nd.skey, nd.tokens = dst, skey, dst["hist"][:, :hd.max_new_tokens]
        return nd

    @torch.no_grad()
    def decode_finish(self, hd: "_PrefillHandle"):
        """Second half of `generate`: the decode loop (one hipGraph replay per token), the stop checks and the HF bookkeeping."""
        c, dv = self.cfg, self.device
        B, S, st, skey, embeds_only, input_ids = hd.B, hd.S, hd.st, hd.skey, hd.embeds_only, hd.input_ids
        max_new_tokens, stopping_criteria, eos_token_id, pad_token_id = hd.max_new_tokens, hd.stopping_criteria, hd.eos_token_id, hd.pad_token_id
        output_hidden_states, return_dict_in_generate, use_graph = hd.output_hidden_states, hd.return_dict_in_generate, hd.use_graph
        sync_every, return_logits, hidden_steps, logits_steps, tokens = hd.sync_every, hd.return_logits, hd.hidden_steps, hd.logits_steps, hd.tokens
        eos = _id_list(eos_token_id)
        prompt_cpu = None if embeds_only else input_ids.cpu().long()
        need_check = bool(eos) or bool(stopping_criteria)
        final = None      # (padded tokens [B, k] on the host, k) once a stop condition has been met
        lookup = getattr(hd, "lookup", None)    # (K, N) of a prompt-lookup request
        assist = getattr(hd, "assist", None)    # K of an assistant_model request: a "step" is a whole round of both engines
        step = (lambda: self._assist_round(st)) if assist is not None else (lambda: self._decode_step(st))

        def check(n_done: int, already: int):
            if not need_check:
                return None
            tk, k, hit = finalize_greedy(tokens[:, :n_done].cpu().long(), eos, pad_token_id, stopping_criteria,
                                         prompt_cpu, already + 1)
            return (tk, k) if hit else None

        graph = self._graphs[skey][1] if use_graph else None
        n = 1
        checked = 1
        final = check(1, 0)
        if use_graph and graph is None and final is None and max_new_tokens > 2:
            # warm the kernels outside capture, then capture one decode step; cursors live on device
            snap = {k: st[k].clone() for k in ("cur_ids", "next_ids", "pos", "slot", "kv_end", "n_hist", "seen", "ban_step") if k in st}
            snap_lk = []    # (buffer, copy) pairs outside the state's top level
            if lookup is not None:      # (the warm-up step's history entries and K / V rows lie past the cursors and are written again)
                snap_lk = [(st["lookup"][k], st["lookup"][k].clone()) for k in ("n_draft", "counters")]
            if assist is not None:      # (likewise in both engines' caches; the round's last launch rewrites the draft's catch-up rows)
                snap_lk = [(t, t.clone()) for t in [st["assist"]["counters"]] + [st["assist"]["d2"][k] for k in ("cur_ids", "pos", "slot", "kv_end")]]
            s = torch.cuda.Stream(device=dv)
            s.wait_stream(torch.cuda.current_stream(dv))
            with torch.cuda.stream(s):
                step()
            torch.cuda.current_stream(dv).wait_stream(s)
            for k, v in snap.items():
                st[k].copy_(v)
            for t, v in snap_lk:
                t.copy_(v)
            graph = torch.cuda.CUDAGraph()
            with capture_graph(graph):
                step()
            for k, v in snap.items():   # capture does not execute; restore is a no-op safety net
                st[k].copy_(v)
            for t, v in snap_lk:
                t.copy_(v)
            self._graphs[skey][1] = graph
        while (lookup is not None or assist is not None) and n < max_new_tokens and final is None:
            # prompt lookup: every verify step yields 1 .. K + 1 tokens, so `sync_every` steps (at most one per token still wanted) run
            # before the host reads how many there are; the stop checks then look at every new length, as on the path below.
            # The cache bounds them too: the host knows n tokens, step j of the block may start from n + j (K + 1) and writes K / V
            # rows up to slot S + n + j (K + 1) + K - 1, which has to stay below max_len (resolve_prompt_lookup admits j = 0).
            # An assisted round is such a step: K + 1 verify rows in the engine's cache, fewer in the draft engine's (its last
            # row is draft K - 1), so the shorter of the two caches bounds the rounds.
            K = lookup[0] if lookup is not None else assist
            cache_len = self.max_len if assist is None else min(self.max_len, st["assist"]["draft"].max_len)
            fit = (cache_len - S - n - K) // (K + 1) + 1
            for _ in range(max(1, min(int(sync_every), max_new_tokens - n, fit))):
                if graph is not None:
                    graph.replay()
                else:
                    step()
            n = min(int(st["n_hist"].item()), max_new_tokens)
            final = check(n, checked)
            checked = n
        while n < max_new_tokens and final is None:
            if graph is not None:
                graph.replay()
            else:
                self._decode_step(st)
            if output_hidden_states:
                hidden_steps.append(tuple(t.clone().unsqueeze(1) for t in st["hidden_buf"]))
            if return_logits:
                logits_steps.append(st["logits"].clone())
            n += 1
            if n % sync_every == 0 or n == max_new_tokens:
                final = check(n, checked)
                checked = n
        if final is not None:   # rows padded after their first EOS; steps that ran past the stop (sync_every > 1) dropped
            gen, n = final[0].to(dv), final[1]
            if output_hidden_states:
                del hidden_steps[n:]
            if return_logits:
                del logits_steps[n:]
        elif need_check:        # no stop met within max_new_tokens: finished rows are still padded
            gen = finalize_greedy(tokens[:, :n].cpu().long(), eos, pad_token_id, None, None)[0].to(dv)
        else:
            gen = tokens[:, :n].long()
        seqs = gen if embeds_only else torch.cat([input_ids.long(), gen], 1)
        out = GenerateOutput(seqs, tuple(hidden_steps) if output_hidden_states else None)
        if return_logits:
            out.logits = torch.stack(logits_steps, 1)
        self.last_prompt_lookup = None      # the record of the LAST call: a plain request has none
        if lookup is not None:      # the device's counters of this call (steps that ran past a stop included)
            steps, drafted, accepted = (int(x) for x in st["lookup"]["counters"][0].tolist())
            out.prompt_lookup = self.last_prompt_lookup = dict(steps=steps, drafted=drafted, accepted=accepted)
        self.last_assisted = None
        if assist is not None:      # likewise; a step is a round
            steps, drafted, accepted = (int(x) for x in st["assist"]["counters"][0].tolist())
            out.assisted = self.last_assisted = dict(steps=steps, drafted=drafted, accepted=accepted)
        return out if return_dict_in_generate else seqs

    def _beam_decode(self, beam, last, next_pos, kv_beg, B, S, input_ids, max_new_tokens, eos, pad, length_penalty, early_stopping,
                     num_return_sequences, as_dict, use_graph, sync_every, return_logits, cache_set):
        """Beam search behind the prompt pass (which ran once per batch row: `last` [B, H] is its final residual at the last
        position). Step 0 scores K copies of that row (HF's score vector [0, -1e9, ...] keeps beam 0 only), the prompt's KV rows are
        expanded to row b * K + k <- row b with the reorder kernel, then every decode step is one graph replay; the host reads the
        trace every `sync_every` steps and stops at the step HF's loop ends (`beam_finalize_host`)."""
        c, dv = self.cfg, self.device
        K, C = beam
        R = B * K
        if max_new_tokens > self.max_len:
            raise ValueError(f"max_new_tokens={max_new_tokens} exceeds the engine's max_len={self.max_len}")
        skey = self._state_key(B, False, return_logits, cache_set, False, beam)
        if skey not in self._graphs:
            self._graphs[skey] = [self._make_state(R, False, True, cache_set, False, beam), None]
        st = self._graphs[skey][0]
        bm = st["beam"]
        rep = lambda t: t.repeat_interleave(K, 0).contiguous()
        bm["run"].copy_(torch.tensor([0.0] + [-1e9] * (K - 1), dtype=torch.float32)[None].expand(B, K))
        bm["n_eos"].fill_(len(eos) if eos else 0)
        bm["eos_ids"].copy_(torch.tensor((eos or []) + [-1] * (MAX_EOS_IDS - len(eos or [])), dtype=torch.int32))
        st["n_hist"].zero_()
        ops.lm_head_argmax(self.lm_head, rep(last), norm_w=self.norm, eps=c.eps, out_ids=bm["lm_ids"], ws=st["lm_ws"], logits=st["logits"])
        self._beam_step(st, reorder=False)
        st["kv_beg"].copy_(rep(kv_beg))
        st["kv_end"].fill_(S)
        row_map = rep(torch.arange(B, dtype=torch.int32, device=dv))
        ops.kv_row_gather(st["kv"][0], st["kv"][1], bm["kv_tmp"][0], bm["kv_tmp"][1], row_map, st["kv_beg"], st["kv_end"], R)
        st["cur_ids"].copy_(st["next_ids"])
        st["pos"].copy_(rep(next_pos.to(torch.int32)))
        st["slot"].fill_(S)
        st["kv_end"].fill_(S + 1)
        st["n_hist"].fill_(1)
        logits_steps = [st["logits"].clone()] if return_logits else None
        prompt_cpu = None if input_ids is None else input_ids.cpu().long()
        host = [None, None, 0]      # (result, bookkeeping state, steps already handed to the host)

        def check(n_done: int):
            blk = tuple(t[host[2]:n_done].cpu() for t in bm["trace"])
            host[0], host[1] = beam_finalize_host(blk, K, max_new_tokens, eos, pad, length_penalty, early_stopping,
                                                  num_return_sequences, prompt_cpu, host[1], host[2])
            host[2] = n_done

        graph = self._graphs[skey][1] if use_graph else None
        n = 1
        check(1)
        while n < max_new_tokens and host[0] is None:
            if graph is not None:
                graph.replay()
            else:
                self._decode_step(st)
                if use_graph and max_new_tokens - n > 2:
                    # That eager step was a real one and loaded the kernels; the following ones replay its capture. (A warm-up step
                    # that is rolled back, as on the greedy path, would have to undo the reorder of the KV rows as well.)
                    graph = torch.cuda.CUDAGraph()
                    with capture_graph(graph):
                        self._decode_step(st)
                    self._graphs[skey][1] = graph
            if return_logits:
                logits_steps.append(st["logits"].clone())
            n += 1
            if n % sync_every == 0 or n == max_new_tokens:
                check(n)
        res = host[0]
        seqs = res["sequences"].to(dv)
        out = GenerateOutput(seqs, None, res["sequences_scores"].to(dv), res["beam_indices"].to(dv))
        if return_logits:
            out.logits = torch.stack(logits_steps[:res["n_steps"]], 1)
        return out if as_dict else seqs

    def _generate_grouped(self, input_ids, inputs_embeds, attention_mask, position_ids, B_all: int, kw: dict, as_dict: bool):
        """More rows than one decode graph holds: groups of DECODE_ROWS, results joined the way one HF call would return
        them (every row padded to the longest group with pad_token_id; a group that ended early repeats the LAST POSITION of its
        last state, [rows, 1, H], for the steps it did not run -- its first entry is the prompt state [rows, S, H])."""
        if kw.get("stopping_criteria"):
            raise NotImplementedError("stopping_criteria look at sequence 0 and end the whole batch (spider.py:55-73); "
                                      f"use them with at most {self.DECODE_ROWS} rows per call")
        outs = []
        R = self.DECODE_ROWS
        for b0 in range(0, B_all, R):
            sl = slice(b0, min(B_all, b0 + R))
            outs.append(self.generate(
                input_ids=None if input_ids is None else input_ids[sl],
                inputs_embeds=None if inputs_embeds is None else inputs_embeds[sl],
                attention_mask=None if attention_mask is None else attention_mask[sl],
                position_ids=None if position_ids is None else position_ids[:, sl], return_dict_in_generate=True, _row0=b0, **kw))
        eos = _id_list(kw.get("eos_token_id"))
        pad = kw.get("pad_token_id")
        pad = pad if pad is not None else (eos[0] if eos else 0)
        T = max(o.sequences.shape[1] for o in outs)
        seqs = torch.cat([torch.nn.functional.pad(o.sequences, (0, T - o.sequences.shape[1]), value=pad) for o in outs], 0)
        out = GenerateOutput(seqs, None)
        if kw.get("output_hidden_states"):
            n_steps = max(len(o.hidden_states) for o in outs)
            hs = []
            for stp in range(n_steps):
                per = [o.hidden_states[stp] if stp < len(o.hidden_states) else tuple(h[:, -1:, :] for h in o.hidden_states[-1])
                       for o in outs]
                hs.append(tuple(torch.cat([p[l] for p in per], 0) for l in range(len(per[0]))))
            out.hidden_states = tuple(hs)
        if kw.get("return_logits"):
            n_steps = max(o.logits.shape[1] for o in outs)
            out.logits = torch.cat([torch.cat([o.logits, o.logits[:, -1:].expand(-1, n_steps - o.logits.shape[1], -1)], 1)
                                    for o in outs], 0)
        return out if as_dict else seqs

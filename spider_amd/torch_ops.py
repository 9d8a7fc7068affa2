"""PyTorch-ROCm custom-op surface of the HIP kernels: `torch.ops.spider_hip.*` (north_star: "hand-written CDNA4 HIP kernels
surfaced as PyTorch-ROCm custom ops"; SURVEY.md section 8b export list).

Each op is a `torch.library.custom_op` whose implementation is the C-ABI call of spider_amd.ops (ctypes -> libspider_hip.so,
launched on torch's current stream) and whose fake (meta) implementation gives output shapes / dtypes, so the kernels are
visible to the dispatcher, to FakeTensor tracing and to `torch.compile` graphs as opaque nodes. They are what a maintainer
binds in place of the reference's module forwards:
    LlamaRMSNorm.forward / LlamaMLP.forward / LlamaAttention.forward      spider/models/modeling_llama3.py:77-82,197-199,214-313
    UNet2DConditionModel blocks called from the denoising loop             spider/models/custom_sd.py:629-647
There is no CPU implementation: the ops raise on non-HIP tensors like the rest of the product path.

    import spider_amd.torch_ops            # registers the library
    y = torch.ops.spider_hip.rmsnorm(x, w, 1e-6, None)
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

BF16 = torch.bfloat16
_lib = "spider_hip"


def _op(name, mutates=()):
    return torch.library.custom_op(f"{_lib}::{name}", mutates_args=mutates, device_types="cuda")


# ------------------------------------------------------------------------------------------ LLM path (a1 - a6)
@_op("rmsnorm")
def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = w * bf16((x + residual) * rsqrt(mean((x + residual)^2) + eps))     modeling_llama3.py:77-82"""
    return ops.rmsnorm(x.contiguous(), w, eps, res=residual)


@rmsnorm.register_fake
def _(x, w, eps, residual=None):
    return torch.empty_like(x)


@_op("rope_qk_", mutates=("q_out", "k_cache", "v_cache"))
def rope_qk_(qkv: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor, cos_sin: torch.Tensor, q_out: torch.Tensor,
             k_cache: torch.Tensor, v_cache: torch.Tensor, n_q: int, n_kv: int, head_dim: int) -> None:
    """RoPE on q / k of the fused projection rows + append of k, v at `slot` (apply_rotary_pos_emb + cache update,
    modeling_llama3.py:128-183,240-313). qkv [B, S, (n_q + 2 n_kv) d]; q_out [B, S, n_q, d]; caches [B, n_kv, T, d]."""
    B, S = qkv.shape[0], qkv.shape[1]
    ops.rope_kv_append(qkv.contiguous(), pos, slot, cos_sin, q_out, k_cache, v_cache, B, S, n_q, n_kv, head_dim)


@_op("attn_decode")
def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_end: torch.Tensor,
                kv_beg: Optional[torch.Tensor] = None) -> torch.Tensor:
    """one query token per sequence against the KV cache (GQA, fp32 softmax); q [B, n_q, d] -> [B, n_q * d]"""
    return ops.attn_decode(q.contiguous(), k_cache, v_cache, kv_end, kv_beg=kv_beg)


@attn_decode.register_fake
def _(q, k_cache, v_cache, kv_end, kv_beg=None):
    return q.new_empty(q.shape[0], q.shape[1] * q.shape[2])


@_op("attn_prefill_causal")
def attn_prefill_causal(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n_heads: int, n_kv_heads: int) -> torch.Tensor:
    """causal GQA attention over a prompt; q [B, S, n_heads d], k / v [B, S, n_kv_heads d] -> [B, S, n_heads d]"""
    return ops.attention(q, k, v, n_heads, n_kv_heads=n_kv_heads, causal=True)


@attn_prefill_causal.register_fake
def _(q, k, v, n_heads, n_kv_heads):
    return q.new_empty(q.shape)


@_op("swiglu")
def swiglu(gate_up: torch.Tensor) -> torch.Tensor:
    """silu(gate) * up on a fused [gate | up] projection (LlamaMLP, modeling_llama3.py:197-199)"""
    return ops.swiglu(gate_up.contiguous())


@swiglu.register_fake
def _(gate_up):
    return gate_up.new_empty(*gate_up.shape[:-1], gate_up.shape[-1] // 2)


@_op("linear_bf16")
def linear_bf16(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x @ w^T + b on the MFMA GEMM (nn.Linear layout w [N, K])"""
    return ops.gemm(x.contiguous(), w, bias=b)


@linear_bf16.register_fake
def _(x, w, b=None):
    return x.new_empty(*x.shape[:-1], w.shape[0])


@_op("lm_head_argmax")
def lm_head_argmax(h: torch.Tensor, w: torch.Tensor, norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """final RMSNorm (optional) + lm_head + greedy argmax, ties -> lowest id; h [B <= 8, H] -> int32 [B]"""
    return ops.lm_head_argmax(w, h.contiguous(), norm_w=norm_w, eps=eps)


@lm_head_argmax.register_fake
def _(h, w, norm_w=None, eps=1e-6):
    return h.new_empty(h.shape[0], dtype=torch.int32)


# ------------------------------------------------------------------------------------------ UNet path (a9 - a12)
@_op("groupnorm_silu")
def groupnorm_silu(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, groups: int, eps: float, act: bool) -> torch.Tensor:
    """GroupNorm (+ SiLU when act) on NHWC [B, H, W, C] (ResnetBlock2D.norm1/2, Transformer2DModel.norm)"""
    return ops.groupnorm(x.contiguous(), w, b, groups, eps, act)


@groupnorm_silu.register_fake
def _(x, w, b, groups, eps, act):
    return torch.empty_like(x)


@_op("conv2d_nhwc")
def conv2d_nhwc(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], stride: int, pad: int) -> torch.Tensor:
    """implicit-GEMM conv: x [B, H, W, Cin], w [Cout, k, k, Cin] (OHWI) -> [B, Ho, Wo, Cout]"""
    return ops.conv2d(x.contiguous(), w, bias=b, stride=stride, pad=pad)


@conv2d_nhwc.register_fake
def _(x, w, b, stride, pad):
    B, H, W, _ = x.shape
    k = w.shape[1]
    return x.new_empty(B, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, w.shape[0])


@_op("attn_self")
def attn_self(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n_heads: int) -> torch.Tensor:
    """UNet self-attention (q, k, v may be column slices of one fused projection); [B, N, C] -> [B, N, C]"""
    return ops.attention(q, k, v, n_heads)


@attn_self.register_fake
def _(q, k, v, n_heads):
    return q.new_empty(q.shape)


@_op("attn_cross_kv77")
def attn_cross_kv77(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, n_heads: int) -> torch.Tensor:
    """cross-attention against the 77 projected text tokens (K / V computed once per prompt)"""
    return ops.attention(q, kc, vc, n_heads)


@attn_cross_kv77.register_fake
def _(q, kc, vc, n_heads):
    return q.new_empty(q.shape)


@_op("attn_consistent")
def attn_consistent(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n_heads: int, keep_bits: torch.Tensor, blk: int,
                    q_off: int) -> torch.Tensor:
    """StoryDiffusion consistent self-attention: a key is visible if its keep bit is set or it lies in the query's own image
    block of `blk` tokens (SpatialAttnProcessor2_0 + cal_attn_mask_xl, Comic_Generation.py:129-196, gradio_utils.py:241-287)"""
    return ops.attention(q, k, v, n_heads, keep_bits=keep_bits, blk=blk, q_off=q_off)


@attn_consistent.register_fake
def _(q, k, v, n_heads, keep_bits, blk, q_off):
    return q.new_empty(q.shape)


@_op("geglu")
def geglu(x: torch.Tensor) -> torch.Tensor:
    """value * gelu(gate) on a fused [value | gate] projection (diffusers FeedForward GEGLU)"""
    return ops.geglu(x.contiguous())


@geglu.register_fake
def _(x):
    return x.new_empty(*x.shape[:-1], x.shape[-1] // 2)


@_op("cfg_step")
def cfg_step(eps2: torch.Tensor, latents: torch.Tensor, guidance: float, c_sample: float, c_eps: float) -> torch.Tensor:
    """classifier-free-guidance combine + a linear scheduler update (custom_sd.py:642-647):
    eps = e_u + g (e_c - e_u) from the UNet output eps2 [2B, h, w, C] fp32 NHWC, result = c_sample * latents + c_eps * eps
    (fp32 NCHW; DDIM's step is exactly this form, PNDM adds stored history terms through spider_lincomb)."""
    eps = ops.cfg_combine(eps2.contiguous(), guidance)
    return ops.lincomb([latents.contiguous(), eps], [c_sample, c_eps])


@cfg_step.register_fake
def _(eps2, latents, guidance, c_sample, c_eps):
    return torch.empty_like(latents)


# ------------------------------------------------------------------------------------------ decode bookkeeping (in place)
@_op("ngram_ban_", mutates=("ban_step",))
def ngram_ban_(prompt_ids: torch.Tensor, n_prompt: torch.Tensor, hist: torch.Tensor, n_hist: torch.Tensor, ngram: torch.Tensor,
               ban: torch.Tensor, ban_step: torch.Tensor, vocab: int) -> None:
    """no_repeat_ngram_size: ban_step = ban | the tokens that would complete an n-gram (n = ngram[0]) already in the row's sequence
    prompt_ids[b, :n_prompt[0]] ++ hist[b, :n_hist[b]] (transformers NoRepeatNGramLogitsProcessor); bitmaps int32 [B, ceil(V/32)]"""
    ops.ngram_ban(dict(prompt_ids=prompt_ids, n_prompt=n_prompt, ngram=ngram, ban=ban, ban_step=ban_step), hist, n_hist, vocab)


@ngram_ban_.register_fake
def _(prompt_ids, n_prompt, hist, n_hist, ngram, ban, ban_step, vocab):
    return None


@_op("decode_advance_seen_ngram_", mutates=("cur_ids", "pos", "slot", "kv_end", "hist", "n_hist", "seen", "ban_step"))
def decode_advance_seen_ngram_(next_ids: torch.Tensor, cur_ids: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor,
                               kv_end: torch.Tensor, hist: torch.Tensor, n_hist: torch.Tensor, seen: torch.Tensor,
                               prompt_ids: torch.Tensor, n_prompt: torch.Tensor, ngram: torch.Tensor, ban: torch.Tensor,
                               ban_step: torch.Tensor, vocab: int) -> None:
    """end of a processed decode step: the chosen token becomes the next input, joins the history and the `seen` set, the cursors
    advance, and ban_step becomes ngram_ban_ of the advanced sequence -- one launch"""
    ops.decode_advance_seen_ngram(next_ids, cur_ids, pos, slot, kv_end, seen, vocab, hist, n_hist,
                                  dict(prompt_ids=prompt_ids, n_prompt=n_prompt, ngram=ngram, ban=ban, ban_step=ban_step))


@decode_advance_seen_ngram_.register_fake
def _(next_ids, cur_ids, pos, slot, kv_end, hist, n_hist, seen, prompt_ids, n_prompt, ngram, ban, ban_step, vocab):
    return None


# ------------------------------------------------------------------------------------------ prompt-lookup decoding
@_op("attn_verify")
def attn_verify(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, kv_end: torch.Tensor, rows_per_seq: int,
                kv_beg: Optional[torch.Tensor] = None, nsplit: int = 1) -> torch.Tensor:
    """R = rows_per_seq consecutive query rows per sequence against the sequence's KV cache; row r sees the slots
    kv_beg[b] <= j < kv_end[b] + r. q [B * R, n_q, d] -> [B * R, n_q * d]"""
    return ops.attn_verify(q.contiguous(), k_cache, v_cache, kv_end, rows_per_seq, kv_beg=kv_beg, nsplit=nsplit)


@attn_verify.register_fake
def _(q, k_cache, v_cache, kv_end, rows_per_seq, kv_beg=None, nsplit=1):
    return q.new_empty(q.shape[0], q.shape[1] * q.shape[2])


@_op("prompt_lookup_draft_", mutates=("ids", "pos", "slot", "n_draft"))
def prompt_lookup_draft_(prompt_ids: torch.Tensor, n_prompt: torch.Tensor, hist: torch.Tensor, n_hist: torch.Tensor,
                         ngram: torch.Tensor, k_draft: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor,
                         n_draft: torch.Tensor) -> None:
    """prompt-lookup draft (transformers PromptLookupCandidateGenerator) of rows 1 ... R - 1 of a verify step from
    prompt_ids[b, :n_prompt[b]] ++ hist[b, :n_hist[b]]; ids / pos / slot int32 [B * R], row 0 is the caller's"""
    ops.prompt_lookup_draft(dict(prompt_ids=prompt_ids, n_prompt=n_prompt, ngram=ngram, k_draft=k_draft, ids=ids, pos=pos, slot=slot,
                                 n_draft=n_draft), hist, n_hist)


@prompt_lookup_draft_.register_fake
def _(prompt_ids, n_prompt, hist, n_hist, ngram, k_draft, ids, pos, slot, n_draft):
    return None


@_op("spec_advance_draft_", mutates=("ids", "pos", "slot", "kv_end", "n_draft", "hist", "n_hist", "counters"))
def spec_advance_draft_(lm_out: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor, kv_end: torch.Tensor,
                        n_draft: torch.Tensor, hist: torch.Tensor, n_hist: torch.Tensor, prompt_ids: torch.Tensor,
                        n_prompt: torch.Tensor, ngram: torch.Tensor, k_draft: torch.Tensor, counters: torch.Tensor) -> None:
    """end of a verify step: the drafts lm_out agrees with are accepted and appended to hist, the cursors advance, counters
    int64 [B, 3] += (1, drafted, accepted), and the next step's rows are drafted -- one launch"""
    ops.spec_advance_draft(dict(prompt_ids=prompt_ids, n_prompt=n_prompt, ngram=ngram, k_draft=k_draft, ids=ids, pos=pos, slot=slot,
                                n_draft=n_draft, lm_out=lm_out, kv_end=kv_end, counters=counters), hist, n_hist)


@spec_advance_draft_.register_fake
def _(lm_out, ids, pos, slot, kv_end, n_draft, hist, n_hist, prompt_ids, n_prompt, ngram, k_draft, counters):
    return None


# ------------------------------------------------------------------------------------------ assisted decoding
@_op("spec_assist_push_", mutates=("t_ids", "t_pos", "t_slot", "d_ids", "d_pos", "d_slot", "d_kv_end"))
def spec_assist_push_(src_out: torch.Tensor, src_pos: torch.Tensor, src_slot: torch.Tensor, src_row: int, t_ids: torch.Tensor,
                      t_pos: torch.Tensor, t_slot: torch.Tensor, j: int, d_ids: torch.Tensor, d_pos: torch.Tensor,
                      d_slot: torch.Tensor, d_kv_end: torch.Tensor, draft_vocab: int) -> None:
    """behind a draft step: the arg-max of source row src_row becomes row j of the target's verify step (one position and slot
    behind its source) and the draft engine's next single row (ids at or above draft_vocab read as 0 there)"""
    ops.spec_assist_push(dict(out=src_out, pos=src_pos, slot=src_slot), src_row, dict(ids=t_ids, pos=t_pos, slot=t_slot), j,
                         dict(ids=d_ids, pos=d_pos, slot=d_slot, kv_end=d_kv_end), draft_vocab)


@spec_assist_push_.register_fake
def _(src_out, src_pos, src_slot, src_row, t_ids, t_pos, t_slot, j, d_ids, d_pos, d_slot, d_kv_end, draft_vocab):
    return None


@_op("spec_assist_advance_", mutates=("ids", "pos", "slot", "kv_end", "hist", "n_hist", "counters", "d_ids", "d_pos", "d_slot", "d_kv_end"))
def spec_assist_advance_(lm_out: torch.Tensor, ids: torch.Tensor, pos: torch.Tensor, slot: torch.Tensor, kv_end: torch.Tensor,
                         n_draft: torch.Tensor, hist: torch.Tensor, n_hist: torch.Tensor, counters: torch.Tensor,
                         d_ids: torch.Tensor, d_pos: torch.Tensor, d_slot: torch.Tensor, d_kv_end: torch.Tensor,
                         draft_vocab: int) -> None:
    """end of an assisted round: the drafts lm_out agrees with are accepted and appended to hist, row 0 and kv_end advance,
    counters int64 [B, 3] += (1, drafted, accepted), and the draft engine's two catch-up rows are written -- one launch"""
    ops.spec_assist_advance(dict(lm_out=lm_out, ids=ids, pos=pos, slot=slot, kv_end=kv_end, n_draft=n_draft, counters=counters),
                            hist, n_hist, dict(ids=d_ids, pos=d_pos, slot=d_slot, kv_end=d_kv_end), draft_vocab)


@spec_assist_advance_.register_fake
def _(lm_out, ids, pos, slot, kv_end, n_draft, hist, n_hist, counters, d_ids, d_pos, d_slot, d_kv_end, draft_vocab):
    return None


# ------------------------------------------------------------------------------------------ weight-only FP8 decode GEMVs
@_op("gemv_w8")
def gemv_w8(wq: torch.Tensor, scale: torch.Tensor, x: torch.Tensor, bias: Optional[torch.Tensor] = None,
            res: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """nn.Linear at decode on weight-only FP8: wq [N, K] float8_e4m3fn, scale [N] fp32 per weight row; x [B <= 4, K] bf16 ->
    [B, N] bf16 = scale[n] * (xin @ f32(wq)^T) (+bias) (+res), xin = RMSNorm(x) * norm_w when norm_w is given"""
    return ops.gemv_w8(wq, scale, x.contiguous(), bias=bias, res=res, norm_w=norm_w, eps=eps)


@gemv_w8.register_fake
def _(wq, scale, x, bias=None, res=None, norm_w=None, eps=1e-6):
    return x.new_empty(x.numel() // wq.shape[1], wq.shape[0])


@_op("gemv_swiglu_w8")
def gemv_swiglu_w8(wq_gate_up: torch.Tensor, scale: torch.Tensor, x: torch.Tensor, norm_w: Optional[torch.Tensor] = None,
                   eps: float = 1e-6) -> torch.Tensor:
    """LlamaMLP gate / up + SiLU * mul on weight-only FP8: wq_gate_up [2 I, K] = [gate rows | up rows], scale [2 I]; -> [B <= 4, I]"""
    return ops.gemv_swiglu_w8(wq_gate_up, scale, x.contiguous(), norm_w=norm_w, eps=eps)


@gemv_swiglu_w8.register_fake
def _(wq_gate_up, scale, x, norm_w=None, eps=1e-6):
    return x.new_empty(x.numel() // wq_gate_up.shape[1], wq_gate_up.shape[0] // 2)


# ------------------------------------------------------------------------------------------ weight-only MXFP4 decode GEMVs
@_op("gemv_w4")
def gemv_w4(blocks: torch.Tensor, scales: torch.Tensor, x: torch.Tensor, bias: Optional[torch.Tensor] = None,
            res: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """nn.Linear at decode on weight-only MXFP4: blocks [N, K / 2] uint8 (two e2m1 codes per byte, low nibble first), scales
    [N, K / 32] uint8 (E8M0); x [B <= 4, K] bf16 -> [B, N] bf16 = xin @ W_eff^T (+bias) (+res), xin = RMSNorm(x) * norm_w when
    norm_w is given"""
    return ops.gemv_w4(blocks, scales, x.contiguous(), bias=bias, res=res, norm_w=norm_w, eps=eps)


@gemv_w4.register_fake
def _(blocks, scales, x, bias=None, res=None, norm_w=None, eps=1e-6):
    return x.new_empty(x.numel() // (2 * blocks.shape[1]), blocks.shape[0])


@_op("gemv_swiglu_w4")
def gemv_swiglu_w4(blocks_gate_up: torch.Tensor, scales: torch.Tensor, x: torch.Tensor, norm_w: Optional[torch.Tensor] = None,
                   eps: float = 1e-6) -> torch.Tensor:
    """LlamaMLP gate / up + SiLU * mul on weight-only MXFP4: blocks_gate_up [2 I, K / 2] = [gate rows | up rows], scales
    [2 I, K / 32]; -> [B <= 4, I]"""
    return ops.gemv_swiglu_w4(blocks_gate_up, scales, x.contiguous(), norm_w=norm_w, eps=eps)


@gemv_swiglu_w4.register_fake
def _(blocks_gate_up, scales, x, norm_w=None, eps=1e-6):
    return x.new_empty(x.numel() // (2 * blocks_gate_up.shape[1]), blocks_gate_up.shape[0] // 2)


# ------------------------------------------------------------------------------------------ fragment-major weight-only GEMVs
@_op("gemv_fm_w4")
def gemv_fm_w4(qfm: torch.Tensor, efm: torch.Tensor, x: torch.Tensor, n: int, bias: Optional[torch.Tensor] = None,
               res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gemv_w4 for up to 16 rows on (qfm, efm) = ops.repack_fm_w4(blocks, scales): x [B <= 16, K] bf16 -> [B, n] bf16 =
    x @ W_eff^T (+bias) (+res) on the matrix cores; no fused RMSNorm"""
    return ops.gemv_fm_w4(qfm, efm, x.contiguous(), n, bias=bias, res=res)


@gemv_fm_w4.register_fake
def _(qfm, efm, x, n, bias=None, res=None):
    return x.new_empty(x.numel() // (128 * qfm.shape[1]), n)


@_op("gemv_swiglu_fm_w4")
def gemv_swiglu_fm_w4(qfm: torch.Tensor, efm: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """gemv_swiglu_w4 for up to 16 rows on ops.repack_fm_w4 of [gate rows | up rows] (I % 16 == 0); -> [B <= 16, I]"""
    return ops.gemv_swiglu_fm_w4(qfm, efm, x.contiguous())


@gemv_swiglu_fm_w4.register_fake
def _(qfm, efm, x):
    return x.new_empty(x.numel() // (128 * qfm.shape[1]), qfm.shape[0] * 8)


@_op("gemv_fm_w8")
def gemv_fm_w8(qfm: torch.Tensor, scale: torch.Tensor, x: torch.Tensor, n: int, bias: Optional[torch.Tensor] = None,
               res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gemv_w8 for up to 16 rows on qfm = ops.repack_fm_w8(wq), scale [n] fp32: x [B <= 16, K] bf16 -> [B, n] bf16 =
    scale[n] * (x @ f32(wq)^T) (+bias) (+res) on the matrix cores; no fused RMSNorm"""
    return ops.gemv_fm_w8(qfm, scale, x.contiguous(), n, bias=bias, res=res)


@gemv_fm_w8.register_fake
def _(qfm, scale, x, n, bias=None, res=None):
    return x.new_empty(x.numel() // (64 * qfm.shape[1]), n)


@_op("gemv_swiglu_fm_w8")
def gemv_swiglu_fm_w8(qfm: torch.Tensor, scale: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """gemv_swiglu_w8 for up to 16 rows on ops.repack_fm_w8 of [gate rows | up rows] (I % 16 == 0), scale [2 I]; -> [B <= 16, I]"""
    return ops.gemv_swiglu_fm_w8(qfm, scale, x.contiguous())


@gemv_swiglu_fm_w8.register_fake
def _(qfm, scale, x):
    return x.new_empty(x.numel() // (64 * qfm.shape[1]), qfm.shape[0] * 8)


# ------------------------------------------------------------------------------------------ weight-only FP8 / MXFP4 lm_head
def _as_fp8(q: torch.Tensor) -> torch.Tensor:
    return q.view(ops.FP8) if q.dtype == torch.uint8 else q


@_op("lm_head_argmax_w8")
def lm_head_argmax_w8(h: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, norm_w: Optional[torch.Tensor] = None,
                      eps: float = 1e-6) -> torch.Tensor:
    """final RMSNorm (optional) + lm_head + greedy argmax on a weight-only FP8 head: q [V, K] float8_e4m3fn (or the same bytes as
    uint8), scale [V] fp32; ties -> lowest id; h [B <= 4, K] -> int32 [B]"""
    return ops.lm_head_argmax_w8(_as_fp8(q), scale, h.contiguous(), norm_w=norm_w, eps=eps)


@lm_head_argmax_w8.register_fake
def _(h, q, scale, norm_w=None, eps=1e-6):
    return h.new_empty(h.numel() // q.shape[1], dtype=torch.int32)


@_op("lm_head_argmax_proc_w8")
def lm_head_argmax_proc_w8(h: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, seen: torch.Tensor, ban: torch.Tensor,
                           penalty: torch.Tensor, min_new: torch.Tensor, eos_ids: torch.Tensor, n_eos: torch.Tensor,
                           n_hist: torch.Tensor, norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """lm_head_argmax_w8 with the logits processors in the arg-max epilogue: repetition penalty on the ids of `seen`, -inf on the
    ids of `ban` and on the EOS ids while n_hist < min_new (buffers of ops.lm_head_argmax_proc)"""
    proc = dict(seen=seen, ban=ban, penalty=penalty, min_new=min_new, eos_ids=eos_ids, n_eos=n_eos, n_hist=n_hist)
    return ops.lm_head_argmax_proc_w8(_as_fp8(q), scale, h.contiguous(), proc, norm_w=norm_w, eps=eps)


@lm_head_argmax_proc_w8.register_fake
def _(h, q, scale, seen, ban, penalty, min_new, eos_ids, n_eos, n_hist, norm_w=None, eps=1e-6):
    return h.new_empty(h.numel() // q.shape[1], dtype=torch.int32)


@_op("lm_head_argmax_w4")
def lm_head_argmax_w4(h: torch.Tensor, blocks: torch.Tensor, scales: torch.Tensor, norm_w: Optional[torch.Tensor] = None,
                      eps: float = 1e-6) -> torch.Tensor:
    """final RMSNorm (optional) + lm_head + greedy argmax on a weight-only MXFP4 head: blocks [V, K / 2] uint8, scales [V, K / 32]
    uint8 (E8M0); ties -> lowest id; h [B <= 4, K] -> int32 [B]"""
    return ops.lm_head_argmax_w4(blocks, scales, h.contiguous(), norm_w=norm_w, eps=eps)


@lm_head_argmax_w4.register_fake
def _(h, blocks, scales, norm_w=None, eps=1e-6):
    return h.new_empty(h.numel() // (2 * blocks.shape[1]), dtype=torch.int32)


@_op("lm_head_argmax_proc_w4")
def lm_head_argmax_proc_w4(h: torch.Tensor, blocks: torch.Tensor, scales: torch.Tensor, seen: torch.Tensor, ban: torch.Tensor,
                           penalty: torch.Tensor, min_new: torch.Tensor, eos_ids: torch.Tensor, n_eos: torch.Tensor,
                           n_hist: torch.Tensor, norm_w: Optional[torch.Tensor] = None, eps: float = 1e-6) -> torch.Tensor:
    """lm_head_argmax_w4 with the logits processors of lm_head_argmax_proc_w8"""
    proc = dict(seen=seen, ban=ban, penalty=penalty, min_new=min_new, eos_ids=eos_ids, n_eos=n_eos, n_hist=n_hist)
    return ops.lm_head_argmax_proc_w4(blocks, scales, h.contiguous(), proc, norm_w=norm_w, eps=eps)


@lm_head_argmax_proc_w4.register_fake
def _(h, blocks, scales, seen, ban, penalty, min_new, eos_ids, n_eos, n_hist, norm_w=None, eps=1e-6):
    return h.new_empty(h.numel() // (2 * blocks.shape[1]), dtype=torch.int32)


# ------------------------------------------------------------------------------------------ safety checker around the CLIP ViT
@_op("clip_preprocess")
def clip_preprocess(images: torch.Tensor, xbounds: torch.Tensor, xtaps: torch.Tensor, ybounds: torch.Tensor, ytaps: torch.Tensor,
                    norm: torch.Tensor, patch: int, f16: bool) -> torch.Tensor:
    """numpy_to_pil + CLIPImageProcessor on the device (run_safety_checker's feature extractor, custom_sd.py:376-384): images
    [B,3,H,W] fp32 in [0,1] -> patch rows [B * (crop / patch)^2, Kp] bf16 / f16 for the ViT's patch-embedding GEMM. The int32 tap
    tables (ops.clip_preprocess_tables: bounds [crop, 2], taps [crop, ks]) and norm [6] = mean, std live on the device."""
    tables = dict(xb=xbounds, xt=xtaps, yb=ybounds, yt=ytaps, norm=norm, H=images.shape[2], W=images.shape[3], crop=xbounds.shape[0],
                  ks_x=xtaps.shape[1], ks_y=ytaps.shape[1])
    return ops.clip_preprocess(images.contiguous(), tables, patch, dtype=torch.float16 if f16 else BF16)


@clip_preprocess.register_fake
def _(images, xbounds, xtaps, ybounds, ytaps, norm, patch, f16):
    crop = xbounds.shape[0]
    return images.new_empty(images.shape[0] * (crop // patch) ** 2, (3 * patch * patch + 7) // 8 * 8, dtype=torch.float16 if f16 else BF16)


@_op("safety_decide")
def safety_decide(image_embeds: torch.Tensor, concept_embeds: torch.Tensor, special_care_embeds: torch.Tensor, thr_concept: torch.Tensor,
                  thr_special: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """StableDiffusionSafetyChecker.forward after the ViT: -> (scores fp32 [B, n_special + n_concept], flags int32 [B])"""
    return ops.safety_decide(image_embeds.contiguous(), concept_embeds, special_care_embeds, thr_concept, thr_special)


@safety_decide.register_fake
def _(image_embeds, concept_embeds, special_care_embeds, thr_concept, thr_special):
    B = image_embeds.shape[0]
    return (image_embeds.new_empty(B, concept_embeds.shape[0] + special_care_embeds.shape[0], dtype=torch.float32),
            image_embeds.new_empty(B, dtype=torch.int32))


@_op("image_blackout_", mutates=("images",))
def image_blackout_(images: torch.Tensor, flags: torch.Tensor) -> None:
    """every image of [B,3,H,W] fp32 whose flag is set becomes zeros, in place (custom_sd.py:376-384: flagged images come back black)"""
    ops.image_blackout_(images, flags)


@image_blackout_.register_fake
def _(images, flags):
    return None


# ------------------------------------------------------------------------------------------ Whisper log-mel features (audio input)
@_op("logmel")
def logmel(waves: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, max_length: int, table: torch.Tensor, fb: torch.Tensor,
           n_samples: int, hop: int) -> tuple[torch.Tensor, torch.Tensor]:
    """WhisperFeatureExtractor(padding="max_length") on the device: packed fp32 waveforms + int32 offsets / lengths [B] ->
    (input_features [B, mel, n_samples // hop] fp32, attention_mask [B, n_samples // hop] int32). max_length: the longest clip's
    sample count, known on the host (it sizes the grid); table / fb: audio_features.logmel_tables."""
    tables = dict(table=table, fb=fb, n_fft=table.shape[0], hop=hop, mel=fb.shape[1], n_samples=n_samples, cap=n_samples // hop)
    B = offsets.shape[0]
    return ops.logmel(waves.contiguous(), [max_length] * B, tables, offsets=offsets, lengths_dev=lengths)


@logmel.register_fake
def _(waves, offsets, lengths, max_length, table, fb, n_samples, hop):
    B, cap = offsets.shape[0], n_samples // hop
    return waves.new_empty(B, fb.shape[1], cap, dtype=torch.float32), waves.new_empty(B, cap, dtype=torch.int32)


# ------------------------------------------------------------------------------------------ Qwen2-VL image patch rows (image input)
@_op("qwen_image_patches")
def qwen_image_patches(packed_u8: torch.Tensor, desc: torch.Tensor, tabs: torch.Tensor, lut: torch.Tensor, rows: int, patch: int,
                       merge: int, temporal: int, tmp_bytes: int, max_h_items: int, max_tiles: int, f32: bool) -> torch.Tensor:
    """Qwen2VLImageProcessorPil on the device: packed uint8 HWC images -> pixel_values [rows, 3 temporal patch^2], bf16 or (f32) fp32.
    desc / tabs / lut and the five integers are the entries of ops.qwen_image_tables for the images' sizes (lut: the one of the
    output format)."""
    dtype = torch.float32 if f32 else BF16
    tables = dict(desc=desc, tabs=tabs, lut={dtype: lut}, sizes=(None,) * desc.shape[0], rows=rows, cols=3 * temporal * patch * patch,
                  in_bytes=packed_u8.numel(), tmp_bytes=tmp_bytes, max_h_items=max_h_items, max_tiles=max_tiles, patch=patch, merge=merge,
                  temporal=temporal)
    return ops.qwen_image_patches(packed_u8.contiguous(), tables, dtype)


@qwen_image_patches.register_fake
def _(packed_u8, desc, tabs, lut, rows, patch, merge, temporal, tmp_bytes, max_h_items, max_tiles, f32):
    return packed_u8.new_empty(rows, 3 * temporal * patch * patch, dtype=torch.float32 if f32 else BF16)


# ------------------------------------------------------------------------------------------ teacher-forced scoring of logits rows
@_op("logprob_rows")
def logprob_rows(logits: torch.Tensor, targets: torch.Tensor, V: int, logits_ref: Optional[torch.Tensor] = None
                 ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`logits.float()` -> `log_softmax` -> `gather(targets)` (ForCausalLMLoss) per row of bf16 logits [rows, ld] with V valid
    columns, in one pass: (logprob, lse, argmax, entropy, kl, argmax_ref), fp32 / int32 [rows]; kl = KL(softmax(logits_ref) ||
    softmax(logits)); without logits_ref the last two are empty. Targets outside [0, V) (ignore_index -100) score 0."""
    o = ops.logprob_rows(logits, targets, V, logits_ref)
    kl = o["kl"] if logits_ref is not None else logits.new_empty(0, dtype=torch.float32)
    ar = o["argmax_ref"] if logits_ref is not None else logits.new_empty(0, dtype=torch.int32)
    return o["logprob"], o["lse"], o["argmax"], o["entropy"], kl, ar


@logprob_rows.register_fake
def _(logits, targets, V, logits_ref=None):
    rows, n = logits.shape[0], (logits.shape[0] if logits_ref is not None else 0)
    f32 = lambda k: logits.new_empty(k, dtype=torch.float32)
    i32 = lambda k: logits.new_empty(k, dtype=torch.int32)
    return f32(rows), f32(rows), i32(rows), f32(rows), f32(n), i32(n)


# ------------------------------------------------------------------------------------------ calibrated MXFP4 (GPTQ on MX blocks)
@_op("gptq_mxfp4")
def gptq_mxfp4(W: torch.Tensor, H: torch.Tensor, damp: float = 0.01) -> tuple[torch.Tensor, torch.Tensor]:
    """`llm.quantize_mxfp4_gptq(W, H, damp)` on the device (ops.gptq_mxfp4: fp64 factor, fp32 sweep kernel of csrc/gptq.hip):
    W [N, K], H [K, K] -> (blocks uint8 [N, K / 2], scales uint8 [N, K / 32]) in `quantize_mxfp4`'s layout"""
    return ops.gptq_mxfp4(W, H, damp)


@gptq_mxfp4.register_fake
def _(W, H, damp=0.01):
    N, K = W.shape
    return W.new_empty(N, K // 2, dtype=torch.uint8), W.new_empty(N, K // 32, dtype=torch.uint8)


# the export list of SURVEY.md section 8b; the in-place decode-bookkeeping ops, the FP8 and MXFP4 GEMVs (row-major and fragment-major) and lm_heads, the safety-checker
# ops, the audio and image feature ops, the scoring op and the calibration op above are listed apart
SAFETY_OP_NAMES = ("clip_preprocess", "safety_decide", "image_blackout_")
AUDIO_OP_NAMES = ("logmel",)
IMAGE_OP_NAMES = ("qwen_image_patches",)
W8_OP_NAMES = ("gemv_w8", "gemv_swiglu_w8")
W4_OP_NAMES = ("gemv_w4", "gemv_swiglu_w4")
QFM_OP_NAMES = ("gemv_fm_w4", "gemv_swiglu_fm_w4", "gemv_fm_w8", "gemv_swiglu_fm_w8")
LM_HEAD_Q_OP_NAMES = ("lm_head_argmax_w8", "lm_head_argmax_proc_w8", "lm_head_argmax_w4", "lm_head_argmax_proc_w4")
DECODE_OP_NAMES = ("ngram_ban_", "decode_advance_seen_ngram_")
SPEC_OP_NAMES = ("attn_verify", "prompt_lookup_draft_", "spec_advance_draft_")
ASSIST_OP_NAMES = ("spec_assist_push_", "spec_assist_advance_")
SCORE_OP_NAMES = ("logprob_rows",)
GPTQ_OP_NAMES = ("gptq_mxfp4",)
OP_NAMES = ("rmsnorm", "rope_qk_", "attn_decode", "attn_prefill_causal", "swiglu", "linear_bf16", "lm_head_argmax", "groupnorm_silu",
            "conv2d_nhwc", "attn_self", "attn_cross_kv77", "attn_consistent", "geglu", "cfg_step")

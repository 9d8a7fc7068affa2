"""Native UNet2DConditionModel step on the HIP kernels (NHWC bf16), for SD-v1.5 (SpiderFree IMAGE decoder,
spider/models/spider_decoder.py:100-120 -> custom_sd.py:634-639) and SDXL (StoryDiffusion,
StoryDiffusion/Comic_Generation.py:313,440). The layer graph restates diffusers==0.25.0 (external to the
reference tree; see oracle/unet.py for the algorithm statement and the 'parity unpinned' note).

MI355X-first choices (vs. the reference's per-op PyTorch calls):
  * activations stay NHWC bf16 in HBM: conv = implicit GEMM on MFMA, 1x1 conv / proj_in / proj_out = plain GEMM
  * self-attention q,k,v come from ONE fused [3C,C] GEMM and are consumed in place (strided views, no transposes)
  * cross-attention K/V of the 77 text tokens are projected ONCE per prompt and reused by all steps
  * the whole time-embedding path (sinusoid -> MLP -> every resnet's time_emb_proj) is computed once per call
    for all timesteps with 3 GEMMs; each step only copies its slice into a static buffer
  * bias / time-embedding / residual adds, 1/rescale and the nearest-2x upsample are fused into GEMM epilogues
    or the conv's input addressing; one UNet step is one hipGraph replay (about 420 kernel launches for SD-v1.5)
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import ops
from .graphs import capture as capture_graph

BF16 = torch.bfloat16


@dataclass
class UNetConfig:
    in_ch: int = 4
    out_ch: int = 4
    block_out: Tuple[int, ...] = (320, 640, 1280, 1280)
    down_attn: Tuple[bool, ...] = (True, True, True, False)
    up_attn: Tuple[bool, ...] = (False, True, True, True)
    depth: Tuple[int, ...] = (1, 1, 1, 1)
    heads: Tuple[int, ...] = (8, 8, 8, 8)
    layers_per_block: int = 2
    cross_dim: int = 768
    groups: int = 32
    linear_proj: bool = False
    addition_time_dim: int = 0
    addition_in: int = 0
    mid_depth: Optional[int] = None
    # AudioLDM form (custom_ad.py:575-581: encoder_hidden_states=None, class_labels=prompt_embeds)
    class_in: int = 0              # class_embed_type="simple_projection": Linear(class_in, temb_dim)
    class_concat: bool = False     # class_embeddings_concat: resnets see cat([temb, class_emb])
    cross_dims: Optional[Tuple[int, ...]] = None   # per-down-block cross_attention_dim

    @staticmethod
    def sd15():
        return UNetConfig()

    @staticmethod
    def audioldm():   # cvssp/audioldm-s-full-v2 unet/config.json (checkpoint-side values; re-read by from_pretrained)
        return UNetConfig(8, 8, (128, 256, 384, 640), (False, True, True, True), (True, True, True, False), (1, 1, 1, 1),
                          (8, 8, 8, 8), 2, 0, 32, False, 0, 0, None, 512, True, (128, 256, 384, 640))

    @staticmethod
    def audioldm_l():   # cvssp/audioldm-l-full unet/config.json: the decoder the reference configures (train_configs/spider_decoder_cfg.py:37)
        return UNetConfig(8, 8, (256, 512, 768, 1280), (False, True, True, True), (True, True, True, False), (1, 1, 1, 1),
                     (8, 8, 8, 8), 2, 0, 32, False, 0, 0, None, 512, True, (256, 512, 768, 1280))

    def cross_dim_of(self, down_idx: int) -> int:
        return self.cross_dims[down_idx] if self.cross_dims is not None else self.cross_dim

    @property
    def temb_in(self):
        return self.temb_dim * (2 if (self.class_in and self.class_concat) else 1)

    @staticmethod
    def sdxl():
        return UNetConfig(4, 4, (320, 640, 1280), (False, True, True), (True, True, False), (1, 2, 10), (5, 10, 20), 2,
                          2048, 32, True, 256, 2816, 10)

    @staticmethod
    def from_diffusers_dict(c: dict) -> "UNetConfig":
        bo = tuple(c["block_out_channels"])
        nb = len(bo)
        ahd = c.get("num_attention_heads") or c["attention_head_dim"]
        heads = tuple(ahd) if isinstance(ahd, (list, tuple)) else (ahd,) * nb
        tl = c.get("transformer_layers_per_block", 1)
        depth = tuple(tl) if isinstance(tl, (list, tuple)) else (tl,) * nb
        xd = c.get("cross_attention_dim")
        xds = tuple(xd) if isinstance(xd, (list, tuple)) else None
        text_time = c.get("addition_embed_type") == "text_time"
        simple_proj = c.get("class_embed_type") == "simple_projection"
        if c.get("class_embed_type") not in (None, "simple_projection"):
            raise NotImplementedError(f"class_embed_type={c['class_embed_type']!r}")
        pdim = c.get("projection_class_embeddings_input_dim") or 0
        return UNetConfig(c["in_channels"], c["out_channels"], bo,
                          tuple(t.startswith("CrossAttn") for t in c["down_block_types"]),
                          tuple(t.startswith("CrossAttn") for t in c["up_block_types"]), depth, heads,
                          c.get("layers_per_block", 2), 0 if xds is not None else (xd or 0), c.get("norm_num_groups", 32),
                          bool(c.get("use_linear_projection", False)), c.get("addition_time_embed_dim") or 0,
                          pdim if text_time else 0, depth[-1] if text_time else None,
                          pdim if simple_proj else 0, bool(c.get("class_embeddings_concat", False)), xds)

    @property
    def temb_dim(self):
        return self.block_out[0] * 4


def timestep_embedding(t: torch.Tensor, dim: int, flip_sin_to_cos=True, shift=0.0) -> torch.Tensor:
    """diffusers Timesteps (fp32 on the host; [n, dim])."""
    half = dim // 2
    exponent = -math.log(10000.0) * torch.arange(half, dtype=torch.float32) / (half - shift)
    emb = t.float()[:, None] * torch.exp(exponent)[None]
    emb = torch.cat([emb.sin(), emb.cos()], -1)
    if flip_sin_to_cos:
        emb = torch.cat([emb[:, half:], emb[:, :half]], -1)
    return emb


class UNetEngine:
    def __init__(self, cfg: UNetConfig, weights: Dict[str, torch.Tensor], device="cuda:0", dtype=BF16, stream32: bool = False,
                 precise: bool = False):
        """dtype: torch.bfloat16 or torch.float16 -- the 16-bit storage / MFMA operand format of the whole engine (the reference
        loads its diffusion decoders with torch_dtype=torch.float16, spider_decoder.py:109; both instantiations of every kernel
        exist, see csrc/common.hpp).
        stream32: carry the residual stream (resnet outputs, the token stream of the transformer blocks) as an fp32 master beside
        its 16-bit shadow: every `x + f(x)` adds in fp32 (GEMM / conv epilogue operands res32 / c32d), every consumer (GroupNorm,
        folded LayerNorm, MFMA operands) reads the shadow. Removes the accumulating rounding of ~70 residual adds per evaluation
        (the second precision lever next to dtype).
        precise (implies stream32): the third lever, for north_star's 1e-3. Every kernel that consumes the residual stream reads its
        fp32 MASTER instead of the 16-bit shadow -- the GroupNorms (ops.groupnorm_f32in), conv_shortcut, the down- / upsamplers and
        proj_out through an fp32 A operand split into hi + lo halves inside the kernel (two MFMAs per K step: ops.conv_a32 /
        gemm_a32), Transformer2DModel.norm -> proj_in the same way on the fp32 GroupNorm output, conv_in / conv_out on fp32 inputs;
        conv1's output stays fp32 for norm2, and the GEGLU product is rounded once. These are the sites the per-site attribution
        (scripts/exp/precision_sites.py) charges with ~75 % of the error variance of one evaluation; their cost is on small / latency-
        bound launches (DESIGN.md section 4 for the measured ms and rel-L2)."""
        assert dtype in (torch.bfloat16, torch.float16), "UNetEngine: dtype must be bfloat16 or float16"
        # precise = 2: additionally the three LayerNorm-consuming projections of every BasicTransformerBlock (q/k/v, to_q, GEGLU) read
        # the fp32 token stream with gamma applied on the A side and the EXACT weight (ops.gemm_ln_a32) -- the re-rounded W * gamma of
        # the folded form is the largest error site of the transformer-heavy models (SDXL: 24 % of the variance)
        self.precise_ln = int(precise) >= 2
        self.precise = bool(precise)
        stream32 = bool(stream32) or self.precise
        self.cfg, self.device, self.dtype, self.stream32 = cfg, torch.device(device), dtype, bool(stream32)
        BF16 = dtype      # every 16-bit tensor this engine creates is of the engine dtype
        self.w: Dict[str, torch.Tensor] = {}
        dv = self.device
        for n, t in weights.items():
            t = t.to(dv)
            if t.ndim == 4:      # conv OIHW -> OHWI (K-contiguous rows for the implicit GEMM)
                t = t.permute(0, 2, 3, 1)
            self.w[n] = t.to(BF16).contiguous()
        # fused projections
        for n in [k[:-len(".attn1.to_q.weight")] for k in list(self.w) if k.endswith(".attn1.to_q.weight")]:
            self.w[n + ".attn1.qkv"] = torch.cat([self.w[n + ".attn1.to_q.weight"], self.w[n + ".attn1.to_k.weight"],
                                                  self.w[n + ".attn1.to_v.weight"]], 0).contiguous()
            self.w[n + ".attn2.kv"] = torch.cat([self.w[n + ".attn2.to_k.weight"], self.w[n + ".attn2.to_v.weight"]], 0).contiguous()
            if self.w[n + ".attn2.to_k.weight"].shape[1] == self.w[n + ".attn2.to_q.weight"].shape[1]:
                # encoder_hidden_states=None (AudioLDM): attn2 attends to its own input, one fused [3C,C] projection
                self.w[n + ".attn2.qkv"] = torch.cat([self.w[n + ".attn2.to_q.weight"], self.w[n + ".attn2.kv"]], 0).contiguous()
        # LayerNorm folded into the projection that consumes it (ops.fold_layernorm / spider_gemm_ln_bf16): norm1 -> attn1 q/k/v,
        # norm2 -> attn2 to_q (or q/k/v when attn2 is a second self-attention), norm3 -> the GEGLU projection. One-time
        # parameter folding at load; the un-folded weights stay for the paths that need the normalised tokens themselves
        # (StoryDiffusion's id bank stores them, story.py).
        self.ln: Dict[str, tuple] = {}
        self.fuse_ln = os.environ.get("SPIDER_LN_FUSE", "1") != "0"
        for b in [k[:-len(".norm1.weight")] for k in list(self.w) if k.endswith(".norm1.weight") and ".transformer_blocks." in k]:
            W = self.w
            if b + ".attn1.qkv" not in W:
                continue
            self.ln[b + ".attn1"] = ops.fold_layernorm(W[b + ".attn1.qkv"], W[b + ".norm1.weight"], W[b + ".norm1.bias"])
            w2 = W[b + ".attn2.qkv"] if b + ".attn2.qkv" in W else W[b + ".attn2.to_q.weight"]
            self.ln[b + ".attn2"] = ops.fold_layernorm(w2, W[b + ".norm2.weight"], W[b + ".norm2.bias"])
            self.ln[b + ".ff"] = ops.fold_layernorm(W[b + ".ff.net.0.proj.weight"], W[b + ".norm3.weight"], W[b + ".norm3.bias"],
                                                    W[b + ".ff.net.0.proj.bias"])
        self.lnx: Dict[str, tuple] = {}
        if self.precise_ln:
            for b in [k[:-len(".attn1")] for k in self.ln if k.endswith(".attn1")]:
                W = self.w
                self.lnx[b + ".attn1"] = ops.fold_layernorm_exact(W[b + ".attn1.qkv"], W[b + ".norm1.weight"], W[b + ".norm1.bias"])
                w2 = W[b + ".attn2.qkv"] if b + ".attn2.qkv" in W else W[b + ".attn2.to_q.weight"]
                self.lnx[b + ".attn2"] = ops.fold_layernorm_exact(w2, W[b + ".norm2.weight"], W[b + ".norm2.bias"])
                self.lnx[b + ".ff"] = ops.fold_layernorm_exact(W[b + ".ff.net.0.proj.weight"], W[b + ".norm3.weight"], W[b + ".norm3.bias"],
                                                               W[b + ".ff.net.0.proj.bias"])
        # Fused cross-attention sub-block (ops.xattn_fused): weight-only halves of the per-prompt fold (prepare() finishes it
        # with the prompt's K / V): WqT_g[c, j] = gamma2[c] * Wq[j, c] and wqb[j] = sum_c Wq[j, c] * beta2[c].
        self.fuse_xattn = os.environ.get("SPIDER_XATTN_FUSE", "1") != "0"
        self.gn_cat = os.environ.get("SPIDER_GN_CAT", "1") != "0"     # up-block norm1 reads (hidden, skip) in place (tuning aid)
        # GroupNorm statistics from the producing conv's epilogue / split-K reduce, and Transformer2DModel.norm folded into proj_in's
        # A operand (round 4; tuning aids: SPIDER_GN_PRODUCER=0 / SPIDER_GN_FUSE_IN=0 restore the stand-alone GroupNorm passes)
        self.gn_producer = ops.GN_PRODUCER
        self.gn_fuse_in = os.environ.get("SPIDER_GN_FUSE_IN", "1") != "0"
        self.xattn_min_rows = int(os.environ.get("SPIDER_XATTN_MIN_ROWS", "1024"))
        self.xw: Dict[str, dict] = {}
        for b in list(self.ln):
            if not b.endswith(".attn2"):
                continue
            l = b[:-len(".attn2")]
            W = self.w
            Wq = W[l + ".attn2.to_q.weight"]
            C = Wq.shape[0]
            if C % 64 != 0 or C > 1280 or self._heads_of(l) != 8 or ".temp_attentions." in l or l.startswith("transformer_in"):
                continue
            g2, b2 = W[l + ".norm2.weight"].float(), W[l + ".norm2.bias"].float()
            wqb4 = torch.zeros(4, C, dtype=BF16, device=dv)
            wqb4[0] = (Wq.float() @ b2).to(BF16)
            self.xw[l] = dict(wqt_g=(Wq.float() * g2[None, :]).t().contiguous().to(BF16), wqb4=wqb4)
        self._ones4 = {}
        # 1x1-conv proj_in / proj_out weights are used as plain [C, C] linears: keep the 2-D form (one tensor object per weight,
        # so that ops.mark_weight's tile-major copy is found again on every call)
        for n in [k for k in self.w if (k.endswith(".proj_in.weight") or k.endswith(".proj_out.weight")) and self.w[k].ndim == 4]:
            self.w[n] = self.w[n].reshape(self.w[n].shape[0], -1).contiguous()
        # weight-streaming problems (16^2 / 8^2 maps: M <= 512 rows) run on tile-major weight copies built on first use
        for t in self.w.values():
            if t.ndim >= 2:
                ops.mark_weight(t)
        for tup in self.ln.values():
            ops.mark_weight(tup[0])
        self.xf: Dict[str, dict] = {}
        # resnet table: order of time_emb_proj consumers
        self.resnets = [k[:-len(".time_emb_proj.weight")] for k in self.w if k.endswith(".time_emb_proj.weight")]
        self.tproj_w = torch.cat([self.w[r + ".time_emb_proj.weight"] for r in self.resnets], 0).contiguous()
        self.tproj_b = torch.cat([self.w[r + ".time_emb_proj.bias"] for r in self.resnets], 0).contiguous()
        self.tproj_off, off = {}, 0
        for r in self.resnets:
            c = self.w[r + ".time_emb_proj.weight"].shape[0]
            self.tproj_off[r] = (off, c)
            off += c
        self.tproj_total = off
        self.cross_layers = [k[:-len(".attn2.kv")] for k in self.w if k.endswith(".attn2.kv")]
        self.self_attn_hook: Optional[Callable] = None   # StoryDiffusion consistent self-attention
        self.freeu: Optional[Tuple[float, float, float, float]] = None
        self._graph = None
        self._graph_key = None
        self.kv: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ diffusers-style processor registry (attn_processors.py)
    @property
    def attn_processors(self):
        """names -> installed processor (None = native kernels), as `UNet2DConditionModel.attn_processors` (Comic_Generation.py:353)"""
        from . import attn_processors as ap
        return ap.attn_processors(self)

    def set_attn_processor(self, processor) -> None:
        """`UNet2DConditionModel.set_attn_processor(dict | processor)` (Comic_Generation.py:371); see attn_processors.py for the scope"""
        from . import attn_processors as ap
        ap.set_attn_processor(self, processor)

    def _heads_of(self, layer: str) -> int:
        """attention heads of the transformer block `layer` (diffusers: attention_head_dim per block of the config)"""
        cfg = self.cfg
        parts = layer.split(".")
        if parts[0] == "down_blocks":
            return cfg.heads[int(parts[1])]
        if parts[0] == "up_blocks":
            return list(reversed(cfg.heads))[int(parts[1])]
        return cfg.heads[-1]

    # ------------------------------------------------------------------ construction
    @classmethod
    def random_init(cls, cfg: UNetConfig, device="cuda:0", seed=0, dtype=BF16, stream32: bool = False, precise: bool = False):
        from_shapes = _param_shapes(cfg)
        gen = torch.Generator(device=device).manual_seed(seed)
        w = {}
        for n, shp in from_shapes.items():
            if n.endswith(".bias"):
                t = torch.randn(shp, generator=gen, device=device) * 0.02
            elif "norm" in n.split(".")[-2]:
                t = torch.ones(shp, device=device)
            else:
                t = torch.randn(shp, generator=gen, device=device) * (1.0 / math.sqrt(math.prod(shp[1:])))
            w[n] = t.to(torch.bfloat16)     # same values for either engine dtype (bf16-representable, exact in f16 too)
        if precise:
            return cls(cfg, w, device, dtype=dtype, precise=precise)
        return cls(cfg, w, device, dtype=dtype, stream32=stream32) if stream32 else cls(cfg, w, device, dtype=dtype)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", dtype=BF16, stream32: bool = False, precise: bool = False):
        """diffusers layout: <path>/config.json + diffusion_pytorch_model.safetensors / .bin (spider_amd/checkpoint.py)."""
        from .checkpoint import load_state_dict, read_config
        cfg = UNetConfig.from_diffusers_dict(read_config(path))
        if precise:
            return cls(cfg, load_state_dict(path), device, dtype=dtype, precise=precise)
        return cls(cfg, load_state_dict(path), device, dtype=dtype, stream32=stream32)

    # ------------------------------------------------------------------ per-call preparation
    def prepare(self, timesteps: torch.Tensor, enc: Optional[torch.Tensor], added: Optional[dict] = None,
                class_labels: Optional[torch.Tensor] = None):
        """timesteps [n] (host), enc [B2, 77, cross] bf16 on device, added: SDXL {'text_embeds','time_ids'}.
        Computes every step's per-resnet time projection and every cross-attention layer's K/V once.
        AudioLDM form: enc=None (attn2 attends to its own input) and class_labels [B2, class_in]."""
        cfg, dv, BF16 = self.cfg, self.device, self.dtype
        B2 = enc.shape[0] if enc is not None else class_labels.shape[0]
        frames = getattr(self, "frames", 1)      # UNet3D: every sample of the CFG batch is `frames` images
        rows = B2 * frames
        n = len(timesteps)
        te = timestep_embedding(torch.as_tensor(timesteps), cfg.block_out[0]).to(dv).to(BF16)          # [n, c0]
        h = ops.gemm(te, self.w["time_embedding.linear_1.weight"], bias=self.w["time_embedding.linear_1.bias"], act="silu")
        emb = ops.gemm(h, self.w["time_embedding.linear_2.weight"], bias=self.w["time_embedding.linear_2.bias"])  # [n, T]
        if cfg.addition_in:
            tid = timestep_embedding(added["time_ids"].flatten().cpu(), cfg.addition_time_dim).reshape(B2, -1)
            add = torch.cat([added["text_embeds"].to(dv).float(), tid.to(dv)], -1).to(BF16).contiguous()
            a = ops.gemm(add, self.w["add_embedding.linear_1.weight"], bias=self.w["add_embedding.linear_1.bias"], act="silu")
            aug = ops.gemm(a, self.w["add_embedding.linear_2.weight"], bias=self.w["add_embedding.linear_2.bias"])  # [B2, T]
            emb = (emb[:, None, :].float() + aug[None].float()).to(BF16).reshape(n * B2, -1).contiguous()
            per = B2
        elif cfg.class_in:
            ce = ops.gemm(class_labels.to(device=dv, dtype=BF16).contiguous(), self.w["class_embedding.weight"],
                          bias=self.w["class_embedding.bias"])                                       # [B2, T]
            if cfg.class_concat:
                emb = torch.cat([emb[:, None, :].expand(n, B2, -1), ce[None].expand(n, B2, -1)], -1)
            else:
                emb = (emb[:, None, :].float() + ce[None].float()).to(BF16)
            emb = emb.reshape(n * B2, -1).contiguous()
            per = B2
        else:
            per = 1
        se = ops.act(emb.contiguous(), "silu")
        tp = ops.gemm(se, self.tproj_w, bias=self.tproj_b)                     # [n*per, total]
        tp = tp.view(n, per, self.tproj_total)
        if per == 1:
            tp = tp.expand(n, rows, self.tproj_total)
        elif frames > 1:
            tp = tp[:, :, None, :].expand(n, B2, frames, self.tproj_total).reshape(n, rows, self.tproj_total)
        # regroup to [n, concat_r(rows * C_r)] so each resnet's rowbias block [rows, C_r] is contiguous
        self.tproj_steps = torch.cat([tp[:, :, o:o + c].reshape(n, rows * c) for (o, c) in (self.tproj_off[r] for r in self.resnets)], 1).contiguous()
        self.self_cross = enc is None
        enc = enc.to(BF16).contiguous() if enc is not None else torch.empty(B2, 0, 0, dtype=BF16, device=dv)
        # Static buffers (the per-step time projections and the cross-attention K/V) persist across calls with the same
        # CFG batch, so the captured hipGraph of one UNet evaluation stays valid from one prompt to the next.
        if getattr(self, "B2", None) != B2 or getattr(self, "_enc_len", None) != enc.shape[1] or getattr(self, "_rows", None) != rows:
            self.tproj_cur = torch.empty_like(self.tproj_steps[0])
            self.tproj_view, off = {}, 0
            for r in self.resnets:
                c = self.tproj_off[r][1]
                self.tproj_view[r] = self.tproj_cur[off:off + rows * c].view(rows, c)
                off += rows * c
            self._rows = rows
            self.kv = {} if self.self_cross else {
                l: torch.empty(B2, enc.shape[1], self.w[l + ".attn2.kv"].shape[0], dtype=BF16, device=dv) for l in self.cross_layers}
            self.xf = {}
            if not self.self_cross and self.fuse_xattn and frames == 1 and enc.shape[1] <= ops.XATTN_LP:
                HL = 8 * ops.XATTN_LP
                for l in self.cross_layers:
                    if l in self.xw:
                        C = self.xw[l]["wqt_g"].shape[0]
                        self.xf[l] = dict(kexp=torch.zeros(B2, 8, ops.XATTN_LP, 8, C // 8, dtype=BF16, device=dv),
                                          vexp=torch.zeros(B2, 8, ops.XATTN_LP, 8, C // 8, dtype=BF16, device=dv),
                                          mq=torch.empty(B2 * HL, C, dtype=BF16, device=dv), mo=torch.empty(B2 * C, HL, dtype=BF16, device=dv),
                                          mq_fm=torch.empty(B2 * HL // 16, C // 64, 2, 64, 8, dtype=BF16, device=dv),
                                          mo_fm=torch.empty(B2 * C // 16, HL // 64, 2, 64, 8, dtype=BF16, device=dv),
                                          cs=torch.empty(B2 * HL, dtype=torch.float32, device=dv),
                                          cb=torch.empty(B2 * HL, dtype=torch.float32, device=dv))
            self._graph = None
            self.B2, self._enc_len = B2, enc.shape[1]
        if not self.self_cross:
            for l in self.cross_layers:
                ops.gemm(enc, self.w[l + ".attn2.kv"], out=self.kv[l])           # [B2, 77, 2C]
            for l, f in self.xf.items():
                self._fold_cross(l, f, B2, enc.shape[1])

    def _fold_cross(self, l: str, f: dict, B2: int, n_keys: int):
        """Once per prompt: fold the text K / V of cross-attention layer `l` into its q / out projections (operands of
        ops.xattn_fused, written in place so that a captured step graph stays valid). Data movement in torch, arithmetic on the
        MFMA GEMM: Mq = scale * Kexp . (Wq diag(gamma2)), Mo = Wo . Vexp^T with Kexp / Vexp the block-diagonal head expansion."""
        w, xw = self.w, self.xw[l]
        C = xw["wqt_g"].shape[0]
        H, LP, d = 8, ops.XATTN_LP, C // 8
        HL = H * LP
        kv = self.kv[l]
        ar = torch.arange(H, device=kv.device)
        f["kexp"][:, ar, :n_keys, ar, :] = kv[..., :C].reshape(B2, n_keys, H, d).permute(2, 0, 1, 3)
        f["vexp"][:, ar, :n_keys, ar, :] = kv[..., C:].reshape(B2, n_keys, H, d).permute(2, 0, 1, 3)
        kexp, vexp = f["kexp"].view(B2 * HL, C), f["vexp"].view(B2, HL, C)
        scale = 1.0 / math.sqrt(d)
        ops.gemm(kexp, xw["wqt_g"], out_scale=scale, out=f["mq"])                                 # [B2*HL, C]
        if C not in self._ones4:
            o4 = torch.zeros(4, C, dtype=self.dtype, device=kv.device); o4[0] = 1.0
            self._ones4[C] = o4
        f["cs"].copy_(ops.gemm(f["mq"], self._ones4[C], out_f32=True)[:, 0])
        f["cb"].copy_(ops.gemm(kexp, xw["wqb4"], out_scale=scale, out_f32=True)[:, 0])
        for b in range(B2):
            ops.gemm(w[l + ".attn2.to_out.0.weight"], vexp[b], out=f["mo"][b * C:(b + 1) * C])  # [C, HL]
        f["mq_fm"].copy_(ops.repack_fm16(f["mq"]))
        f["mo_fm"].copy_(ops.repack_fm16(f["mo"]))

    # ------------------------------------------------------------------ blocks
    def _gn(self, n, x, silu, eps=1e-5, partial=None):
        """GroupNorm `n` of x; `partial` (or x._gnp): statistics its producing conv left behind (ops.conv_ex(gn_groups=...))"""
        if partial is None:
            partial = getattr(x, "_gnp", None)
        x32 = getattr(x, "_s32", None) if self.precise else None
        if x32 is not None:       # precise: the fp32 master, one rounding on the way out
            return ops.groupnorm_f32in(x32, self.w[n + ".weight"], self.w[n + ".bias"], self.cfg.groups, eps, silu, partial=partial)
        return ops.groupnorm(x, self.w[n + ".weight"], self.w[n + ".bias"], self.cfg.groups, eps, silu, partial=partial)

    def _resnet(self, n, x, out_gn: bool = False):
        """x: the block input, or a (hidden, skip) pair of an up block: norm1 then reads the two tensors in place and hands back
        their concatenation for the shortcut (no concat launch). GroupNorm statistics come from the PRODUCER of each normalised
        tensor where one exists (SPIDER_GN_PRODUCER, default on): conv1 leaves those of norm2's input, the block's input may carry
        its own (x._gnp), and with out_gn conv2 leaves those of the block's output for the GroupNorm that consumes it next."""
        w = self.w
        G = self.cfg.groups if self.gn_producer else None
        if self.precise:
            return self._resnet_precise(n, x, G, out_gn)
        if isinstance(x, tuple) and not self.gn_cat:
            x = ops.concat_channels(x[0], x[1])
        if isinstance(x, tuple):
            a, x = ops.groupnorm_cat(x[0], x[1], w[n + ".norm1.weight"], w[n + ".norm1.bias"], self.cfg.groups, 1e-5, True)
        else:
            a = self._gn(n + ".norm1", x, True)
        if G:
            h, hp = ops.conv2d(a, w[n + ".conv1.weight"], bias=w[n + ".conv1.bias"], rowbias=self.tproj_view[n], gn_groups=G)
        else:
            h, hp = ops.conv2d(a, w[n + ".conv1.weight"], bias=w[n + ".conv1.bias"], rowbias=self.tproj_view[n]), None
        a = self._gn(n + ".norm2", h, True, partial=hp)
        sc = x
        og = G if out_gn else None
        if not self.stream32:
            if n + ".conv_shortcut.weight" in w:
                sc = ops.conv2d(x, w[n + ".conv_shortcut.weight"], bias=w[n + ".conv_shortcut.bias"], pad=0)
            out = ops.conv2d(a, w[n + ".conv2.weight"], bias=w[n + ".conv2.bias"], res=sc, gn_groups=og)
            if og:
                out, op_ = out
                out._gnp = op_
            return out
        # fp32 residual stream: the shortcut (identity: the block input's master; 1x1 conv: its unrounded output) is added in fp32
        sc32 = getattr(x, "_s32", None)
        if n + ".conv_shortcut.weight" in w:
            sc, sc32 = ops.conv2d(x, w[n + ".conv_shortcut.weight"], bias=w[n + ".conv_shortcut.bias"], pad=0, want32=True)
        r = ops.conv2d(a, w[n + ".conv2.weight"], bias=w[n + ".conv2.bias"], res=None if sc32 is not None else sc,
                       res32=sc32, want32=True, gn_groups=og)
        out, out32 = r[0], r[1]
        out._s32 = out32
        if og:
            out._gnp = r[2]
        return out

    def _resnet_precise(self, n, x, G, out_gn):
        """ResnetBlock2D with every read of the stream on its fp32 master (UNetEngine(precise=True)): norm1 and the 1x1 shortcut read
        x32 (the skip concat as an fp32 concat), conv1's output stays fp32 for norm2, the adds are fp32 as with stream32."""
        w = self.w
        if isinstance(x, tuple):
            x32 = ops.concat_channels_f32(x[0]._s32, x[1]._s32)
            xp = None
        else:
            x32, xp = x._s32, getattr(x, "_gnp", None)
        a = ops.groupnorm_f32in(x32, w[n + ".norm1.weight"], w[n + ".norm1.bias"], self.cfg.groups, 1e-5, True, partial=xp)
        r = ops.conv2d(a, w[n + ".conv1.weight"], bias=w[n + ".conv1.bias"], rowbias=self.tproj_view[n], want32=True, gn_groups=G)
        h32, hp = r[1], (r[2] if G else None)
        a = ops.groupnorm_f32in(h32, w[n + ".norm2.weight"], w[n + ".norm2.bias"], self.cfg.groups, 1e-5, True, partial=hp)
        sc32 = x32
        if n + ".conv_shortcut.weight" in w:
            sc32 = ops.conv_a32(x32, w[n + ".conv_shortcut.weight"], bias=w[n + ".conv_shortcut.bias"], want32=True)[1]
        og = G if out_gn else None
        r = ops.conv2d(a, w[n + ".conv2.weight"], bias=w[n + ".conv2.bias"], res32=sc32, want32=True, gn_groups=og)
        out = r[0]
        out._s32 = r[1]
        if og:
            out._gnp = r[2]
        return out

    def _self_attn(self, b, y, heads):
        """y [B, N, C] (LayerNorm output) -> attention output before the to_out projection's residual."""
        C = y.shape[-1]
        qkv = ops.gemm(y, self.w[b + ".attn1.qkv"])
        return ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads)

    def _proj2(self, b, y, ln_input: bool, y32=None):
        """attn2's projection of the block input: y is the norm2 output (ln_input=False) or the un-normalised residual stream
        (ln_input=True: norm2 folded into the GEMM). y32 (precise = 2): the stream's fp32 master, exact-weight form."""
        if ln_input and y32 is not None and (b + ".attn2") in self.lnx:
            W_, g_, cs, cb, be_, bi_ = self.lnx[b + ".attn2"]
            C = y.shape[-1]
            if not self.self_cross and W_.shape[0] != C:
                W_, cs, cb, bi_ = W_[:C], cs[:C], cb[:C], (None if bi_ is None else bi_[:C])
            return ops.gemm_ln_a32(y32, W_, g_, cs, cb, be_, bi_)
        if ln_input:
            Wf, cs, cb = self.ln[b + ".attn2"]
            C = y.shape[-1]
            if not self.self_cross and Wf.shape[0] != C:   # folded from a fused [q | k | v] weight, text K/V in use: q rows only
                Wf, cs, cb = Wf[:C], cs[:C], cb[:C]
            return ops.gemm_ln(y, Wf, cs, cb)
        return ops.gemm(y, self.w[b + (".attn2.qkv" if self.self_cross else ".attn2.to_q.weight")])

    def _cross_attn(self, b, y, heads, ln_input: bool = False, y32=None):
        """attn2 of a BasicTransformerBlock: K/V of the text tokens were projected in prepare(); with
        encoder_hidden_states=None (AudioLDM) it is a second self-attention."""
        C = y.shape[-1]
        if self.self_cross:
            qkv = self._proj2(b, y, ln_input, y32)
            return ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads)
        q = self._proj2(b, y, ln_input, y32)
        kv = self.kv[b]
        return ops.attention(q, kv[..., :C], kv[..., C:], heads)

    def _transformer(self, n, x, heads, depth):
        w = self.w
        B, H, W_, C = x.shape
        s32 = self.stream32
        h32 = None
        # stream32: every residual GEMM below takes the stream's fp32 master (res32) and returns the new master beside the shadow
        rg = (lambda A_, W_w, bias, h_, h32_: ops.gemm(A_, W_w, bias=bias, res32=h32_, want32=True)) if s32 else \
             (lambda A_, W_w, bias, h_, h32_: (ops.gemm(A_, W_w, bias=bias, res=h_), None))
        xp = getattr(x, "_gnp", None)
        geglu = "geglu_exact" if self.precise else "geglu"
        if self.precise:
            # norm on the fp32 master, its fp32 output split hi / lo inside proj_in
            x32 = x._s32
            if xp is not None and self.gn_fuse_in and (H * W_) % 64 == 0 and C % 64 == 0 and w[n + ".proj_in.weight"].shape[0] % 4 == 0:
                h, h32 = ops.gemm_gn_in_a32(x32.view(B, H * W_, C), w[n + ".proj_in.weight"], xp, w[n + ".norm.weight"], w[n + ".norm.bias"],
                                            H * W_, 1e-6, bias=w[n + ".proj_in.bias"], want32=True)
            else:
                a32 = ops.groupnorm_f32in(x32, w[n + ".norm.weight"], w[n + ".norm.bias"], self.cfg.groups, 1e-6, False, partial=xp,
                                          want16=False, want32=True)
                h, h32 = ops.gemm_a32(a32.view(B, H * W_, C), w[n + ".proj_in.weight"], bias=w[n + ".proj_in.bias"], want32=True)
        elif xp is not None and self.gn_fuse_in and (H * W_) % 64 == 0 and C % 64 == 0 and B * H * W_ < 16384 and w[n + ".proj_in.weight"].shape[0] % 4 == 0:
            # norm + proj_in in ONE launch: the statistics came with x (its producing conv), the normalisation is applied to the GEMM's
            # A operand on its way into LDS -- no statistics pass, no apply pass, no normalised copy of x
            r = ops.gemm_gn_in(x.view(B, H * W_, C), w[n + ".proj_in.weight"], xp, w[n + ".norm.weight"], w[n + ".norm.bias"], H * W_, 1e-6,
                               bias=w[n + ".proj_in.bias"], want32=s32)
            h, h32 = r if s32 else (r, None)
        else:
            a = self._gn(n + ".norm", x, False, eps=1e-6)
            if s32:
                h, h32 = ops.gemm(a.view(B, H * W_, C), w[n + ".proj_in.weight"], bias=w[n + ".proj_in.bias"], want32=True)
            else:
                h = ops.gemm(a.view(B, H * W_, C), w[n + ".proj_in.weight"], bias=w[n + ".proj_in.bias"])
        for d in range(depth):
            b = f"{n}.transformer_blocks.{d}"
            fuse = self.fuse_ln
            if self.self_attn_hook is not None and self.self_attn_hook.wants(b + ".attn1"):
                if self.precise_ln:     # [hi | lo] of the fp32 LayerNorm of the stream's master: the hook projects it against [W | W]
                    y = ops.row_split(h32, self.dtype, w[b + ".norm1.weight"], w[b + ".norm1.bias"], 1e-5)
                else:
                    y = ops.layernorm(h, w[b + ".norm1.weight"], w[b + ".norm1.bias"])
                o = self.self_attn_hook(self, b + ".attn1", y, heads)
            elif fuse and self.precise_ln:      # the fp32 token stream, exact weight
                qkv = ops.gemm_ln_a32(h32, *self.lnx[b + ".attn1"])
                o = ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads)
            elif fuse:     # norm1 + q/k/v projection: one launch
                qkv = ops.gemm_ln(h, *self.ln[b + ".attn1"])
                o = ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads)
            else:
                o = self._self_attn(b, ops.layernorm(h, w[b + ".norm1.weight"], w[b + ".norm1.bias"]), heads)
            h, h32 = rg(o, w[b + ".attn1.to_out.0.weight"], w[b + ".attn1.to_out.0.bias"], h, h32)
            xf = self.xf.get(b) if (fuse and not self.precise_ln) else None     # (precise = 2: to_q reads the fp32 stream instead)
            # Fused where it wins (measured, scripts/bench_xattn.py: 17 vs 31 us at 2 x 4096 tokens / C = 320, 22 vs 29 us at
            # 2 x 1024 / 640): with fewer than ~64 row tiles (the 16^2 / 8^2 maps at C = 1280: 46 vs 34 us, 36 vs 29 us) one block's
            # serial chain of 20 + 20 dependent operand loads is longer than the three launches it replaces, which spread over the chip.
            if xf is not None and (H * W_) % 16 == 0 and B * H * W_ >= self.xattn_min_rows:   # norm2 + to_q + attention + to_out + residual
                if s32:
                    h, h32 = ops.xattn_fused(h, xf["mq_fm"], xf["mo_fm"], xf["cs"], xf["cb"], w[b + ".attn2.to_out.0.bias"], B, heads,
                                             self._enc_len, x32=h32, want32=True)
                else:
                    h = ops.xattn_fused(h, xf["mq_fm"], xf["mo_fm"], xf["cs"], xf["cb"], w[b + ".attn2.to_out.0.bias"], B, heads, self._enc_len)
            else:
                if fuse:
                    o = self._cross_attn(b, h, heads, ln_input=True, y32=h32 if self.precise_ln else None)
                else:
                    o = self._cross_attn(b, ops.layernorm(h, w[b + ".norm2.weight"], w[b + ".norm2.bias"]), heads)
                h, h32 = rg(o, w[b + ".attn2.to_out.0.weight"], w[b + ".attn2.to_out.0.bias"], h, h32)
            if fuse and self.precise_ln:
                g = ops.gemm_ln_a32(h32, *self.lnx[b + ".ff"], act=geglu)
            elif fuse:       # norm3 + GEGLU projection: one launch
                g = ops.gemm_ln(h, *self.ln[b + ".ff"], act=geglu)
            else:
                y = ops.layernorm(h, w[b + ".norm3.weight"], w[b + ".norm3.bias"])
                g = ops.gemm(y, w[b + ".ff.net.0.proj.weight"], bias=w[b + ".ff.net.0.proj.bias"], act=geglu)  # fused GEGLU
            h, h32 = rg(g, w[b + ".ff.net.2.weight"], w[b + ".ff.net.2.bias"], h, h32)
        if self.precise:     # proj_out reads the stream's master
            out, out32 = ops.gemm_a32(h32, w[n + ".proj_out.weight"], bias=w[n + ".proj_out.bias"], res32=x._s32.view(B, H * W_, C), want32=True)
            outv = out.view(B, H, W_, C)
            outv._s32 = out32.view(B, H, W_, C)
            return outv
        if s32:
            x32 = getattr(x, "_s32", None)
            out, out32 = ops.gemm(h, w[n + ".proj_out.weight"], bias=w[n + ".proj_out.bias"], want32=True,
                                  res=None if x32 is not None else x.view(B, H * W_, C),
                                  res32=None if x32 is None else x32.view(B, H * W_, C))
            outv = out.view(B, H, W_, C)
            outv._s32 = out32.view(B, H, W_, C)
            return outv
        out = ops.gemm(h, w[n + ".proj_out.weight"], bias=w[n + ".proj_out.bias"], res=x.view(B, H * W_, C))
        return out.view(B, H, W_, C)

    def _forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [B2, h, w, in_ch] bf16 NHWC -> eps [B2, h, w, out_ch] fp32 NHWC (time step = current tproj_cur)."""
        cfg, w = self.cfg, self.w
        P = self.precise
        if P:                  # x: fp32 NHWC (ops.latent_to_nhwc_f32); conv_in leaves the master of the stream
            if x.dtype != torch.float32:
                x = x.float()
            h, h32 = ops.conv2d_small_cin_f32in(x, w["conv_in.weight"], w["conv_in.bias"], want32=True)
            h._s32 = h32
        else:
            h = ops.conv2d_small_cin(x, w["conv_in.weight"], w["conv_in.bias"])
        skips = [h]
        nb = len(cfg.block_out)
        for i in range(nb):
            for j in range(cfg.layers_per_block):
                # the block's output is normalised next by its transformer, or (no transformer) by the following resnet's norm1
                h = self._resnet(f"down_blocks.{i}.resnets.{j}", h, out_gn=cfg.down_attn[i] or j + 1 < cfg.layers_per_block or i == nb - 1)
                if cfg.down_attn[i]:
                    h = self._transformer(f"down_blocks.{i}.attentions.{j}", h, cfg.heads[i], cfg.depth[i])
                skips.append(h)
            if i != nb - 1 and P:        # Downsample2D reads the stream's master; its output is stream too
                dw = w[f"down_blocks.{i}.downsamplers.0.conv.weight"]
                h32 = h._s32
                h, o32 = ops.conv_a32(h32, dw, bias=w[f"down_blocks.{i}.downsamplers.0.conv.bias"], stride=2, pad=(1, 1), want32=True)
                h._s32 = o32
                skips.append(h)
            elif i != nb - 1:
                if self.gn_producer:     # the next block's first norm1 normalises this conv's output
                    h, hp = ops.conv2d(h, w[f"down_blocks.{i}.downsamplers.0.conv.weight"], bias=w[f"down_blocks.{i}.downsamplers.0.conv.bias"],
                                       stride=2, pad=1, gn_groups=cfg.groups)
                    h._gnp = hp
                else:
                    h = ops.conv2d(h, w[f"down_blocks.{i}.downsamplers.0.conv.weight"], bias=w[f"down_blocks.{i}.downsamplers.0.conv.bias"],
                                   stride=2, pad=1)
                skips.append(h)
        h = self._resnet("mid_block.resnets.0", h, out_gn=True)
        h = self._transformer("mid_block.attentions.0", h, cfg.heads[-1], cfg.mid_depth if cfg.mid_depth is not None else cfg.depth[-1])
        h = self._resnet("mid_block.resnets.1", h)
        rheads, rdepth = list(reversed(cfg.heads)), list(reversed(cfg.depth))
        for i in range(nb):
            for j in range(cfg.layers_per_block + 1):
                skip = skips.pop()
                hh = h
                if self.freeu is not None and i < 2:
                    if self.precise:      # on the fp32 masters: the scaled half and the filtered skip are never rounded to 16 bits
                        hh, skip = _apply_freeu32(i, hh, skip, *self.freeu)
                    else:
                        hh, skip = _apply_freeu(i, hh, skip, *self.freeu)
                h = self._resnet(f"up_blocks.{i}.resnets.{j}", (hh, skip), out_gn=cfg.up_attn[i])
                if cfg.up_attn[i]:
                    h = self._transformer(f"up_blocks.{i}.attentions.{j}", h, rheads[i], rdepth[i])
            if i != nb - 1:
                # Upsample2D to the size of the next skip connection (diffusers' forward_upsample_size rule; = exact 2x
                # on latents that are multiples of 2^(levels-1), 2x-1 on e.g. the 125-row AudioLDM latent)
                th, tw = skips[-1].shape[1], skips[-1].shape[2]
                if P:
                    h32 = h._s32
                    h, o32 = ops.conv_a32(h32, w[f"up_blocks.{i}.upsamplers.0.conv.weight"], bias=w[f"up_blocks.{i}.upsamplers.0.conv.bias"],
                                          pad=(1, 1), up_size=(th, tw), want32=True)
                    h._s32 = o32
                else:
                    h = ops.conv_ex(h, w[f"up_blocks.{i}.upsamplers.0.conv.weight"], bias=w[f"up_blocks.{i}.upsamplers.0.conv.bias"],
                                    pad=(1, 1), up_size=(th, tw))
        if P:
            a32 = ops.groupnorm_f32in(h._s32, w["conv_norm_out.weight"], w["conv_norm_out.bias"], cfg.groups, 1e-5, True, want16=False, want32=True)
            return ops.conv2d_small_cout_f32in(a32, w["conv_out.weight"], w["conv_out.bias"])
        a = self._gn("conv_norm_out", h, True)
        return ops.conv2d_small_cout(a, w["conv_out.weight"], w["conv_out.bias"], out_f32=True)

    # ------------------------------------------------------------------ public step
    def step(self, x: torch.Tensor, step_idx: int, use_graph: bool = True) -> torch.Tensor:
        """One UNet evaluation at timestep index `step_idx` of the prepared schedule. x bf16 NHWC [B2,h,w,C]."""
        self.tproj_cur.copy_(self.tproj_steps[step_idx])
        if not use_graph or self.self_attn_hook is not None:
            return self._forward(x)
        key = tuple(x.shape)
        if self._graph is None or self._graph_key != key:
            self._x_static = torch.empty_like(x)
            self._x_static.copy_(x)
            s = torch.cuda.Stream(device=self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                self._forward(self._x_static)       # warm-up outside capture
            torch.cuda.current_stream(self.device).wait_stream(s)
            self._graph = torch.cuda.CUDAGraph()
            with capture_graph(self._graph):
                self._out_static = self._forward(self._x_static)
            self._graph_key = key
        self._x_static.copy_(x)
        self._graph.replay()
        return self._out_static


def _fourier_filter(x_nhwc: torch.Tensor, threshold: int, scale: float) -> torch.Tensor:
    """FreeU low-pass on the skip features (hipFFT through torch.fft is glue, not a north_star kernel)."""
    x = x_nhwc.float().permute(0, 3, 1, 2)
    B, C, H, W = x.shape
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), device=x.device)
    cr, cc = H // 2, W // 2
    mask[..., cr - threshold:cr + threshold, cc - threshold:cc + threshold] = scale
    xf = torch.fft.ifftshift(xf * mask, dim=(-2, -1))
    return torch.fft.ifftn(xf, dim=(-2, -1)).real.permute(0, 2, 3, 1).to(x_nhwc.dtype).contiguous()


def _apply_freeu(res_idx, hidden, skip, s1, s2, b1, b2):
    n = hidden.shape[-1] // 2
    b, s = (b1, s1) if res_idx == 0 else (b2, s2)
    hidden = torch.cat([(hidden[..., :n].float() * b).to(hidden.dtype), hidden[..., n:]], -1).contiguous()
    return hidden, _fourier_filter(skip, 1, s)


def _apply_freeu32(res_idx, hidden, skip, s1, s2, b1, b2):
    """FreeU in the precise modes: the same two edits on the fp32 masters (`_s32`) of the up-block input and of the skip feature;
    the 16-bit tensors returned are their shadows (the precise resnet reads the masters only)."""
    h32, k32 = hidden._s32, skip._s32
    n = h32.shape[-1] // 2
    b, s = (b1, s1) if res_idx == 0 else (b2, s2)
    h32 = torch.cat([h32[..., :n] * b, h32[..., n:]], -1).contiguous()
    k32 = _fourier_filter(k32, 1, s)
    hs, ks = h32.to(hidden.dtype), k32.to(skip.dtype)
    hs._s32, ks._s32 = h32, k32
    return hs, ks


def _param_shapes(cfg: UNetConfig) -> dict:
    """name -> shape in diffusers naming (conv OIHW); mirrors UNet2DConditionModel's module tree."""
    S = {}
    T, c0 = cfg.temb_dim, cfg.block_out[0]

    def conv(n, co, ci, k): S[n + ".weight"] = (co, ci, k, k); S[n + ".bias"] = (co,)
    def lin(n, co, ci, bias=True):
        S[n + ".weight"] = (co, ci)
        if bias: S[n + ".bias"] = (co,)
    def norm(n, c): S[n + ".weight"] = (c,); S[n + ".bias"] = (c,)
    def resnet(n, ci, co):
        norm(n + ".norm1", ci); conv(n + ".conv1", co, ci, 3); lin(n + ".time_emb_proj", co, cfg.temb_in)
        norm(n + ".norm2", co); conv(n + ".conv2", co, co, 3)
        if ci != co: conv(n + ".conv_shortcut", co, ci, 1)
    def transformer(n, c, depth, xd):
        norm(n + ".norm", c)
        if cfg.linear_proj: lin(n + ".proj_in", c, c); lin(n + ".proj_out", c, c)
        else: conv(n + ".proj_in", c, c, 1); conv(n + ".proj_out", c, c, 1)
        for d in range(depth):
            b = f"{n}.transformer_blocks.{d}"
            norm(b + ".norm1", c); norm(b + ".norm2", c); norm(b + ".norm3", c)
            for a, kd in (("attn1", c), ("attn2", xd)):
                lin(f"{b}.{a}.to_q", c, c, False); lin(f"{b}.{a}.to_k", c, kd, False); lin(f"{b}.{a}.to_v", c, kd, False)
                lin(f"{b}.{a}.to_out.0", c, c)
            lin(b + ".ff.net.0.proj", 8 * c, c); lin(b + ".ff.net.2", c, 4 * c)

    conv("conv_in", c0, cfg.in_ch, 3)
    lin("time_embedding.linear_1", T, c0); lin("time_embedding.linear_2", T, T)
    if cfg.addition_in:
        lin("add_embedding.linear_1", T, cfg.addition_in); lin("add_embedding.linear_2", T, T)
    if cfg.class_in:
        lin("class_embedding", T, cfg.class_in)
    nb, ch = len(cfg.block_out), c0
    for i, co in enumerate(cfg.block_out):
        for j in range(cfg.layers_per_block):
            resnet(f"down_blocks.{i}.resnets.{j}", ch if j == 0 else co, co)
            if cfg.down_attn[i]: transformer(f"down_blocks.{i}.attentions.{j}", co, cfg.depth[i], cfg.cross_dim_of(i))
        ch = co
        if i != nb - 1: conv(f"down_blocks.{i}.downsamplers.0.conv", co, co, 3)
    cm = cfg.block_out[-1]
    resnet("mid_block.resnets.0", cm, cm)
    transformer("mid_block.attentions.0", cm, cfg.mid_depth if cfg.mid_depth is not None else cfg.depth[-1], cfg.cross_dim_of(nb - 1))
    resnet("mid_block.resnets.1", cm, cm)
    rev, rdepth, prev = list(reversed(cfg.block_out)), list(reversed(cfg.depth)), cm
    for i, co in enumerate(rev):
        cin_skip = rev[min(i + 1, nb - 1)]
        for j in range(cfg.layers_per_block + 1):
            skip = cin_skip if j == cfg.layers_per_block else co
            resnet(f"up_blocks.{i}.resnets.{j}", (prev if j == 0 else co) + skip, co)
            if cfg.up_attn[i]: transformer(f"up_blocks.{i}.attentions.{j}", co, rdepth[i], cfg.cross_dim_of(nb - 1 - i))
        prev = co
        if i != nb - 1: conv(f"up_blocks.{i}.upsamplers.0.conv", co, co, 3)
    norm("conv_norm_out", c0); conv("conv_out", cfg.out_ch, c0, 3)
    return S


def unet_flops(cfg: UNetConfig, h: int, w: int, text_len: int = 77, self_cross: bool = False) -> dict:
    """Exact multiply-add count (x2) of one UNet evaluation per sample at latent h x w, by category
    (convs 2*Cin*Cout*k^2*h*w, linears 2*N*Cin*Cout, attention cores 4*N*Lk*C) -- the layer-table sum that
    SURVEY.md section 8d asks for instead of the literature figure."""
    S = _param_shapes(cfg)
    res = {}   # module prefix -> (h, w) at which it runs
    fl = dict(conv=0.0, linear=0.0, attn_self=0.0, attn_cross=0.0)
    nb = len(cfg.block_out)
    hh, ww = h, w
    sizes, level = {}, []
    for i in range(nb):
        sizes[f"down_blocks.{i}."] = (hh, ww)
        level.append((hh, ww))
        if i != nb - 1:
            hh, ww = (hh + 1) // 2, (ww + 1) // 2          # stride-2, pad-1, 3x3
            sizes[f"down_blocks.{i}.downsamplers"] = (hh, ww)
    sizes["mid_block."] = (hh, ww)
    for i in range(nb):
        sizes[f"up_blocks.{i}."] = level[nb - 1 - i]
        if i != nb - 1:
            sizes[f"up_blocks.{i}.upsamplers"] = level[nb - 2 - i]
    sizes["conv_in"] = sizes["conv_out"] = (h, w)

    def size_of(name):
        best = None
        for p, s in sizes.items():
            if name.startswith(p) and (best is None or len(p) > len(best[0])):
                best = (p, s)
        return best[1] if best else (1, 1)

    for n, shp in S.items():
        if not n.endswith(".weight") or len(shp) == 1:
            continue
        sh, sw = size_of(n)
        if len(shp) == 4:
            fl["conv"] += 2.0 * shp[0] * shp[1] * shp[2] * shp[3] * sh * sw
        elif "time_emb" in n or "add_embedding" in n:
            continue  # hoisted out of the step
        elif (".attn2.to_k" in n or ".attn2.to_v" in n) and not self_cross:
            continue  # hoisted: projected once per prompt
        else:
            fl["linear"] += 2.0 * shp[0] * shp[1] * sh * sw
            if n.endswith(".attn1.to_q.weight"):
                fl["attn_self"] += 4.0 * (sh * sw) ** 2 * shp[0]
            if n.endswith(".attn2.to_q.weight"):
                fl["attn_cross"] += 4.0 * (sh * sw) * (sh * sw if self_cross else text_len) * shp[0]
    fl["total"] = sum(fl.values())
    return fl


def denoise(unet: "UNetEngine", scheduler, latents: torch.Tensor, enc: Optional[torch.Tensor], guidance: float, steps: int,
            added: Optional[dict] = None, use_graph: bool = True, class_labels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's denoising loop (custom_sd.py:627-652) on device: latents fp32 NCHW [B,4,h,w] in HBM,
    enc [2B,77,C] (uncond first, as _encode_prompt concatenates them, custom_sd.py:372). Per step:
    cat([latents]*2)+scale (1 launch) -> UNet graph replay -> CFG combine (1) -> scheduler update (1).
    AudioLDM (custom_ad.py:568-594): enc=None, class_labels [2B, class_in] (uncond first)."""
    ts = scheduler.set_timesteps(steps)
    unet.prepare(ts, enc, added, class_labels)
    latents = (latents * scheduler.init_noise_sigma).contiguous()
    do_cfg = guidance > 1.0
    for i, t in enumerate(ts):
        if getattr(unet, "precise", False):
            x2 = ops.latent_to_nhwc_f32(latents, reps=2 if do_cfg else 1)
        else:
            x2 = ops.latent_to_nhwc(latents, reps=2 if do_cfg else 1, dtype=unet.dtype)
        e = unet.step(x2, i, use_graph=use_graph)
        eps = ops.cfg_combine(e, guidance) if do_cfg else ops.nhwc_to_nchw(e)
        latents = scheduler.step(eps, t, latents)
    return latents


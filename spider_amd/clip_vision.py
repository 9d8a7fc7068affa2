"""CLIP vision tower on the HIP kernels: `CLIPVisionModelWithProjection` of transformers, the image encoder of the Stable Diffusion
safety checker (spider/models/custom_sd.py:376-384). Patch embedding (conv patch x patch, stride patch, no bias) as ONE GEMM over patch
rows, class + position embeddings, `pre_layrnorm` (the HF key is spelled like that), N pre-LN layers of the CLIPTextEngine form without
the causal mask (fused [3H,H] QKV GEMM, flash attention, out-proj with residual, quick-GELU / GELU MLP), `post_layernorm` of the class
token as the pooled output, `visual_projection` (no bias) -> image_embeds [B, D].

The patch rows are [B * P, Kp] with column (c, dy, dx) -- the flattening of the conv weight -- and Kp = 3 patch^2 rounded up to a
multiple of 8 (588 -> 592 for ViT-L/14: ops.gemm needs K % 8 == 0); the weight's pad columns are zero, and ops.clip_preprocess writes
zeros in the rows' pad columns."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import ops

BF16 = torch.bfloat16


@dataclass
class CLIPVisionConfig:
    hidden: int = 1024
    layers: int = 24
    heads: int = 16
    inter: int = 4096
    image: int = 224
    patch: int = 14
    proj: int = 768
    eps: float = 1e-5
    act: str = "quick_gelu"

    @staticmethod
    def vit_l14():      # openai/clip-vit-large-patch14, the tower of the published SD safety checker
        return CLIPVisionConfig()

    @staticmethod
    def from_hf_dict(c: dict, projection_dim: Optional[int] = None):
        """`c` is a CLIPVisionConfig dict (the `vision_config` of a CLIP config.json); absent keys take transformers' defaults."""
        return CLIPVisionConfig(c.get("hidden_size", 768), c.get("num_hidden_layers", 12), c.get("num_attention_heads", 12),
                                c.get("intermediate_size", 3072), c.get("image_size", 224), c.get("patch_size", 32),
                                projection_dim if projection_dim is not None else c.get("projection_dim", 512),
                                c.get("layer_norm_eps", 1e-5), c.get("hidden_act", "quick_gelu"))

    @property
    def n_patches(self) -> int:
        return (self.image // self.patch) ** 2

    @property
    def k_patch(self) -> int:
        return 3 * self.patch * self.patch

    @property
    def k_padded(self) -> int:
        return (self.k_patch + 7) // 8 * 8


def _shapes(c: CLIPVisionConfig) -> dict:
    S = {"vision_model.embeddings.class_embedding": (c.hidden,),
         "vision_model.embeddings.patch_embedding.weight": (c.hidden, 3, c.patch, c.patch),
         "vision_model.embeddings.position_embedding.weight": (c.n_patches + 1, c.hidden),
         "vision_model.pre_layrnorm.weight": (c.hidden,), "vision_model.pre_layrnorm.bias": (c.hidden,)}
    for l in range(c.layers):
        p = f"vision_model.encoder.layers.{l}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            S[p + f"self_attn.{n}.weight"] = (c.hidden, c.hidden); S[p + f"self_attn.{n}.bias"] = (c.hidden,)
        for n in ("layer_norm1", "layer_norm2"):
            S[p + n + ".weight"] = (c.hidden,); S[p + n + ".bias"] = (c.hidden,)
        S[p + "mlp.fc1.weight"] = (c.inter, c.hidden); S[p + "mlp.fc1.bias"] = (c.inter,)
        S[p + "mlp.fc2.weight"] = (c.hidden, c.inter); S[p + "mlp.fc2.bias"] = (c.hidden,)
    S["vision_model.post_layernorm.weight"] = (c.hidden,); S["vision_model.post_layernorm.bias"] = (c.hidden,)
    S["visual_projection.weight"] = (c.proj, c.hidden)
    return S


def random_vision_weights(cfg: CLIPVisionConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    """fp32 CPU tensors under the CLIPVisionModelWithProjection names, scaled so that activations stay O(1) through any depth
    (norm weights 1 + 0.1 n, biases 0.05 n, embeddings 0.3 n, matrices n / sqrt(fan_in)) and rounded to bf16 values, which both
    engine formats hold exactly."""
    import math
    gen = torch.Generator().manual_seed(seed)
    w = {}
    for n, shp in _shapes(cfg).items():
        t = torch.randn(shp, generator=gen)
        if n.endswith(".bias"):
            t = t * 0.05
        elif ("norm" in n or "layrnorm" in n) and n.endswith(".weight"):
            t = 1.0 + t * 0.1
        elif "class_embedding" in n or "position_embedding" in n:
            t = t * 0.3
        else:
            t = t / math.sqrt(math.prod(shp[1:]))
        w[n] = t.bfloat16().float()
    return w


def vision_key(name: str, prefix: str = "") -> Optional[str]:
    """Checkpoint key -> the engine's name (CLIPVisionModelWithProjection layout), or None for a tensor the tower does not own.
    `prefix` is what stands in front of `vision_model.` in the file: "" for a CLIPVisionModelWithProjection directory,
    "vision_model." for the safety checker, whose tower is a CLIPVisionModel (`vision_model.vision_model.*`). `visual_projection.weight`
    carries no prefix in either."""
    if name == "visual_projection.weight":
        return name
    head = prefix + "vision_model."
    if name.startswith(head):
        name = "vision_model." + name[len(head):]
        return None if name.endswith("embeddings.position_ids") else name      # a buffer old exports carry
    return None


class CLIPVisionEngine:
    def __init__(self, cfg: CLIPVisionConfig, weights: Dict[str, torch.Tensor], device="cuda:0", dtype=BF16):
        assert dtype in (torch.bfloat16, torch.float16), "CLIPVisionEngine: dtype must be bfloat16 or float16"
        assert cfg.hidden % cfg.heads == 0 and cfg.hidden % 8 == 0 and cfg.proj % 8 == 0 and cfg.image % cfg.patch == 0
        if cfg.act not in ("quick_gelu", "gelu"):
            raise NotImplementedError(f"CLIPVisionEngine: hidden_act {cfg.act!r} (only quick_gelu and gelu)")
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        missing = [k for k in _shapes(cfg) if k not in weights]
        if missing:
            raise KeyError(f"CLIPVisionEngine: the weights lack {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        g = lambda k: weights[k].to(device=self.device, dtype=dtype).contiguous()
        wp = weights["vision_model.embeddings.patch_embedding.weight"].to(device=self.device, dtype=dtype).reshape(cfg.hidden, cfg.k_patch)
        self.w_patch = torch.zeros(cfg.hidden, cfg.k_padded, dtype=dtype, device=self.device)      # pad columns stay zero
        self.w_patch[:, :cfg.k_patch] = wp
        pos = weights["vision_model.embeddings.position_embedding.weight"].float()
        cls = weights["vision_model.embeddings.class_embedding"].float()
        self.pos_patches = pos[1:].to(device=self.device, dtype=dtype).contiguous()                  # residual of the patch GEMM
        self.cls_pos = (cls + pos[0]).to(device=self.device, dtype=dtype).contiguous()               # token 0 of every image
        self.pre_ln = (g("vision_model.pre_layrnorm.weight"), g("vision_model.pre_layrnorm.bias"))
        self.layers = []
        for l in range(cfg.layers):
            p = f"vision_model.encoder.layers.{l}."
            self.layers.append(dict(
                w_qkv=torch.cat([g(p + "self_attn.q_proj.weight"), g(p + "self_attn.k_proj.weight"), g(p + "self_attn.v_proj.weight")], 0).contiguous(),
                b_qkv=torch.cat([g(p + "self_attn.q_proj.bias"), g(p + "self_attn.k_proj.bias"), g(p + "self_attn.v_proj.bias")], 0).contiguous(),
                w_o=g(p + "self_attn.out_proj.weight"), b_o=g(p + "self_attn.out_proj.bias"),
                ln1=(g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias")), ln2=(g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias")),
                w1=g(p + "mlp.fc1.weight"), b1=g(p + "mlp.fc1.bias"), w2=g(p + "mlp.fc2.weight"), b2=g(p + "mlp.fc2.bias")))
        self.post_ln = (g("vision_model.post_layernorm.weight"), g("vision_model.post_layernorm.bias"))
        self.visual_projection = g("visual_projection.weight")

    @classmethod
    def random_init(cls, cfg: CLIPVisionConfig, device="cuda:0", seed=0, dtype=BF16):
        return cls(cfg, random_vision_weights(cfg, seed), device, dtype=dtype)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", dtype=BF16, prefix: str = ""):
        """A CLIPVisionModelWithProjection directory (prefix "") or a tower nested under `prefix` in a larger state dict."""
        from .checkpoint import load_state_dict, read_config
        c = read_config(path)
        cfg = CLIPVisionConfig.from_hf_dict(c.get("vision_config", c), c.get("projection_dim"))
        return cls(cfg, load_state_dict(path, keep=lambda k: vision_key(k, prefix)), device, dtype=dtype)

    @torch.no_grad()
    def encode(self, patch_rows: torch.Tensor, use_graph: bool = True) -> torch.Tensor:
        """patch_rows [B * P, Kp] 16-bit (ops.clip_preprocess) -> image_embeds [B, D]. One hipGraph per batch size."""
        if use_graph:
            if not hasattr(self, "_graph"):
                from .graphs import GraphRunner
                self._graph = GraphRunner(self._encode)
            return self._graph(patch_rows)
        return self._encode(patch_rows)

    def _encode(self, rows: torch.Tensor) -> torch.Tensor:
        c = self.cfg
        P, H = c.n_patches, c.hidden
        if rows.ndim != 2 or rows.shape[1] != c.k_padded or rows.shape[0] % P or rows.dtype != self.dtype:
            raise ValueError(f"CLIPVisionEngine: patch rows must be [B * {P}, {c.k_padded}] {self.dtype}, got {tuple(rows.shape)} {rows.dtype}")
        B = rows.shape[0] // P
        h = torch.empty(B, P + 1, H, dtype=self.dtype, device=rows.device)
        h[:, 0] = self.cls_pos                                         # class token + its position: constant rows
        for b in range(B):                                             # patch embedding + position embedding, written behind token 0
            ops.gemm(rows[b * P:(b + 1) * P], self.w_patch, res=self.pos_patches, out=h[b, 1:])
        h = ops.layernorm(h, *self.pre_ln, c.eps)
        d = H // c.heads
        for lw in self.layers:
            x = ops.layernorm(h, *lw["ln1"], c.eps)
            qkv = ops.gemm(x, lw["w_qkv"], bias=lw["b_qkv"])
            a = ops.attention(qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:], c.heads, scale=d ** -0.5, causal=False)
            h = ops.gemm(a, lw["w_o"], bias=lw["b_o"], res=h)
            x = ops.layernorm(h, *lw["ln2"], c.eps)
            m = ops.gemm(x, lw["w1"], bias=lw["b1"], act=c.act)
            h = ops.gemm(m, lw["w2"], bias=lw["b2"], res=h)
        pooled = ops.layernorm(h[:, 0].contiguous(), *self.post_ln, c.eps)
        return ops.gemm(pooled, self.visual_projection)

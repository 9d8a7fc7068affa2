"""Stable Diffusion safety checker on the device: what `run_safety_checker` does to every generated image before it is returned
(spider/models/custom_sd.py:376-384, called at :658; the reference's decoder loads the pipeline without `safety_checker=None`,
spider_decoder.py:109,114, so a published SD-v1.5 directory brings `safety_checker/` and `feature_extractor/` along).

    feature extractor (numpy_to_pil + CLIPImageProcessor)   ops.clip_preprocess        on the VAE's fp32 image where it lies
    CLIPVisionModel + visual_projection                     CLIPVisionEngine           the CLIPTextEngine kernels, no causal mask
    cosine distances, special-care cascade, flags           ops.safety_decide
    flagged images -> black                                 ops.image_blackout_

replayed as one hipGraph per image shape; the image then makes its one device -> host trip already filtered.

diffusers is absent here and in the reference tree (the reference imports it from site-packages), so the decision rule is restated
from the published algorithm -- `StableDiffusionSafetyChecker.forward` of diffusers 0.25 -- and anchored on the reference's call sites
custom_sd.py:376-384,658; like the UNet and the VAE it is unpinned upstream. The rule: cosine similarities of the projected image
embedding against `special_care_embeds` and `concept_embeds`; special-care concepts first, in index order, each scored
round(cos - threshold + adjustment, 3) with adjustment 0 until one scores > 0 and 0.01 from then on (the special-care concepts that
follow included); then every concept scored the same way; an image is flagged iff any concept score is > 0. Flagged images are
returned as zeros and `nsfw_content_detected` says which.

`safety_preprocess_host` and `safety_decide_host` restate the two new device stages in torch on the host, for the tests (in the
style of llm.process_logits_host); nothing on the product path calls them."""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence

import torch

from . import ops
from .clip_vision import CLIPVisionConfig, CLIPVisionEngine, random_vision_weights, vision_key

BF16 = torch.bfloat16
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
N_CONCEPTS, N_SPECIAL = 17, 3       # the published checker
CHECKER_BUFFERS = ("concept_embeds", "special_care_embeds", "concept_embeds_weights", "special_care_embeds_weights")


# ------------------------------------------------------------------------------------------ feature_extractor/preprocessor_config.json
def preprocess_config(cfg: Optional[dict] = None) -> dict:
    """A CLIPImageProcessor / CLIPFeatureExtractor config dict -> dict(size, crop, mean, std). The device feature extractor is
    resize-shortest-edge BICUBIC + centre crop + rescale 1/255 + normalise; any other setting raises NotImplementedError naming the key.
    None gives CLIP's defaults (224 / 224)."""
    c = dict(cfg or {})
    for k in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
        if not c.get(k, True):
            raise NotImplementedError(f"preprocessor_config: {k}=false is not implemented by the device feature extractor")
    if c.get("resample", 3) != 3:
        raise NotImplementedError(f"preprocessor_config: resample={c['resample']} is not implemented (only 3 = BICUBIC)")
    if abs(c.get("rescale_factor", 1 / 255) - 1 / 255) > 1e-9:
        raise NotImplementedError(f"preprocessor_config: rescale_factor={c['rescale_factor']} is not implemented (only 1/255)")
    if c.get("do_pad", False):
        raise NotImplementedError("preprocessor_config: do_pad=true is not implemented")
    size = c.get("size", 224)
    if isinstance(size, dict):
        if set(size) != {"shortest_edge"}:
            raise NotImplementedError(f"preprocessor_config: size={size} is not implemented (only shortest_edge)")
        size = size["shortest_edge"]
    crop = c.get("crop_size", 224)
    if isinstance(crop, dict):
        if set(crop) != {"height", "width"} or crop["height"] != crop["width"]:
            raise NotImplementedError(f"preprocessor_config: crop_size={crop} is not implemented (only square height / width)")
        crop = crop["height"]
    mean, std = c.get("image_mean", CLIP_MEAN), c.get("image_std", CLIP_STD)
    if len(mean) != 3 or len(std) != 3:
        raise NotImplementedError("preprocessor_config: image_mean / image_std must have 3 entries")
    return dict(size=int(size), crop=int(crop), mean=tuple(float(m) for m in mean), std=tuple(float(s) for s in std))


def read_preprocess_config(path: str) -> dict:
    """`<path>/preprocessor_config.json` when present, else CLIP's defaults."""
    p = os.path.join(path, "preprocessor_config.json")
    return preprocess_config(json.load(open(p)) if os.path.exists(p) else None)


# ------------------------------------------------------------------------------------------ host restatements (tests)
def safety_preprocess_host(images: torch.Tensor, size: int = 224, crop: int = 224, mean: Sequence[float] = CLIP_MEAN,
                           std: Sequence[float] = CLIP_STD) -> torch.Tensor:
    """images [B,3,H,W] in [0,1] -> pixel_values [B,3,crop,crop] fp32, the stages the reference runs on the host in their order:
    numpy_to_pil ((x * 255).round(), half-even), Pillow's antialiased BICUBIC to shortest edge `size` (horizontal pass, then vertical,
    each rounded to 8 bits and clipped), centre crop, (v / 255 - mean) / std in fp32. The two passes are matrix products in float64
    over the integer taps of ops.bicubic_taps: every product and sum is an integer below 2^53, so they are Pillow's int32
    accumulations exactly."""
    x = images.detach().float().cpu()
    B, C, H, W = x.shape
    Hr, Wr, top, left = ops.clip_resize_geometry(H, W, size, crop)
    q = (x * 255.0).round().clamp_(0, 255).double()

    def dense(in_size, out_size, first):
        bounds, taps = ops.bicubic_taps(in_size, out_size, first, crop)
        M = torch.zeros(crop, in_size, dtype=torch.float64)
        for j in range(crop):
            x0, n = int(bounds[j, 0]), int(bounds[j, 1])
            M[j, x0:x0 + n] = torch.as_tensor(taps[j, :n]).double()
        return M

    one, half = float(1 << ops.RESIZE_PRECISION_BITS), float(1 << (ops.RESIZE_PRECISION_BITS - 1))
    clip8 = lambda acc: torch.floor((acc + half) / one).clamp_(0, 255)
    t = clip8(q @ dense(W, Wr, left).T)                                     # [B,3,H,crop]
    v = clip8(dense(H, Hr, top) @ t)                                        # [B,3,crop,crop]
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return (v.float() / 255.0 - m) / s


def patchify_host(pixel_values: torch.Tensor, patch: int) -> torch.Tensor:
    """[B,3,S,S] -> patch rows [B * (S/patch)^2, Kp] with column (c, dy, dx) and zero pad columns: the layout ops.clip_preprocess writes."""
    B, C, S, _ = pixel_values.shape
    g = S // patch
    r = pixel_values.reshape(B, C, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, C * patch * patch)
    Kp = (r.shape[1] + 7) // 8 * 8
    return torch.nn.functional.pad(r, (0, Kp - r.shape[1]))


def safety_decide_host(image_embeds: torch.Tensor, concepts: torch.Tensor, special: torch.Tensor, thr_c: torch.Tensor,
                       thr_s: torch.Tensor):
    """-> (scores fp32 [B, n_special + n_concept], special-care first; flags bool [B]): the rule of the module docstring in fp32."""
    norm = lambda t: torch.nn.functional.normalize(t.detach().float().cpu(), dim=-1)
    e = norm(image_embeds)
    cos_s, cos_c = e @ norm(special).T, e @ norm(concepts).T
    thr_c, thr_s = thr_c.detach().float().cpu(), thr_s.detach().float().cpu()
    B, n_s, n_c = e.shape[0], special.shape[0], concepts.shape[0]
    scores = torch.zeros(B, n_s + n_c, dtype=torch.float32)
    flags = torch.zeros(B, dtype=torch.bool)
    k1000 = torch.tensor(1000.0, dtype=torch.float32)
    for b in range(B):
        adj = torch.tensor(0.0, dtype=torch.float32)
        for j in range(n_s + n_c):
            cos, thr = (cos_s[b, j], thr_s[j]) if j < n_s else (cos_c[b, j - n_s], thr_c[j - n_s])
            s = torch.round((cos - thr + adj) * k1000) / k1000        # round(x, 3) of a numpy float32: half-even on x * 1000
            scores[b, j] = s
            if s > 0:
                if j < n_s:
                    adj = torch.tensor(0.01, dtype=torch.float32)
                else:
                    flags[b] = True
    return scores, flags


# ------------------------------------------------------------------------------------------ engine
def checker_key(name: str) -> Optional[str]:
    """Key of a StableDiffusionSafetyChecker state dict -> the engine's name, or None for a tensor the checker does not read
    (`vision_model.vision_model.*` is the tower, a CLIPVisionModel; `visual_projection.weight`; the four concept buffers)."""
    if name in CHECKER_BUFFERS:
        return name
    return vision_key(name, prefix="vision_model.")


def random_checker_weights(cfg: CLIPVisionConfig, seed: int = 0, n_concepts: int = N_CONCEPTS, n_special: int = N_SPECIAL):
    """fp32 CPU tensors under the engine's names: a random tower, random concepts, thresholds nothing reaches (cos <= 1 < 2)."""
    w = random_vision_weights(cfg, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    w["concept_embeds"] = torch.randn(n_concepts, cfg.proj, generator=gen)
    w["special_care_embeds"] = torch.randn(n_special, cfg.proj, generator=gen)
    w["concept_embeds_weights"] = torch.full((n_concepts,), 2.0)
    w["special_care_embeds_weights"] = torch.full((n_special,), 2.0)
    return w


class SafetyCheckerEngine:
    def __init__(self, cfg: CLIPVisionConfig, weights: Dict[str, torch.Tensor], device="cuda:0", dtype=BF16, preprocess: Optional[dict] = None):
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        self.vision = CLIPVisionEngine(cfg, weights, device, dtype=dtype)
        self.pre = dict(preprocess) if preprocess is not None else preprocess_config({"size": cfg.image, "crop_size": cfg.image})
        if self.pre["crop"] != cfg.image:
            raise ValueError(f"SafetyCheckerEngine: crop_size {self.pre['crop']} does not match the tower's image_size {cfg.image}")
        e16 = lambda k: weights[k].to(device=self.device, dtype=dtype).contiguous()
        f32 = lambda k: weights[k].to(device=self.device, dtype=torch.float32).contiguous()
        self.concept_embeds, self.special_care_embeds = e16("concept_embeds"), e16("special_care_embeds")
        self.concept_thr, self.special_thr = f32("concept_embeds_weights"), f32("special_care_embeds_weights")
        assert self.concept_embeds.shape[1] == cfg.proj and self.special_care_embeds.shape[1] == cfg.proj
        self.unread: List[str] = []

    @classmethod
    def random_init(cls, cfg: CLIPVisionConfig, device="cuda:0", seed=0, dtype=BF16, preprocess: Optional[dict] = None):
        return cls(cfg, random_checker_weights(cfg, seed), device, dtype=dtype, preprocess=preprocess)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", dtype=BF16, preprocess: Optional[dict] = None):
        """`safety_checker/` of a diffusers pipeline directory: config.json is a CLIP config (vision_config, projection_dim)."""
        from .checkpoint import load_state_dict, read_config
        c = read_config(path)
        cfg = CLIPVisionConfig.from_hf_dict(c.get("vision_config", {}), c.get("projection_dim", 512))
        sd = load_state_dict(path)
        w, unread = {}, []
        for k, v in sd.items():
            kk = checker_key(k)
            if kk is not None:
                w[kk] = v
            elif not k.endswith("position_ids"):
                unread.append(k)
        if unread:
            import warnings
            warnings.warn(f"{path}: {len(unread)} tensors of the safety checker are not read: {unread[:4]}")
        eng = cls(cfg, w, device, dtype=dtype, preprocess=preprocess)
        eng.unread = unread
        return eng

    # ---------------------------------------------------------------- the stages (each usable on its own; all stream-ordered, no sync)
    def preprocess(self, images: torch.Tensor) -> torch.Tensor:
        p = self.pre
        tables = ops.clip_preprocess_tables(images.shape[2], images.shape[3], p["size"], p["crop"], p["mean"], p["std"], images.device)
        return ops.clip_preprocess(images, tables, self.cfg.patch, dtype=self.dtype)

    def decide(self, image_embeds: torch.Tensor):
        return ops.safety_decide(image_embeds, self.concept_embeds, self.special_care_embeds, self.concept_thr, self.special_thr)

    def _run(self, images: torch.Tensor):
        embeds = self.vision._encode(self.preprocess(images))
        scores, flags = self.decide(embeds)
        return ops.image_blackout_(images, flags), flags, scores, embeds

    @torch.no_grad()
    def run(self, images: torch.Tensor, use_graph: bool = True):
        """images [B,3,H,W] fp32 in [0,1] on the device -> (images with the flagged ones zeroed, flags int32 [B], scores fp32
        [B, n_special + n_concept], image_embeds [B, D]). With the graph the input is left as it was (the replay works on a copy);
        without it the black-out is in place."""
        images = images.contiguous()
        if use_graph:
            if not hasattr(self, "_graph"):
                from .graphs import GraphRunner
                self._graph = GraphRunner(self._run)
            return self._graph(images)
        return self._run(images)

    def __call__(self, images_dev: torch.Tensor, use_graph: bool = True):
        out = self.run(images_dev, use_graph)
        return out[0], out[1]

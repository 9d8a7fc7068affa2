"""Shared inputs, references and bounds of the safety-checker tests (test_safety_cpu.py, test_safety_gpu.py).

Feature extractor: the reference is transformers' CLIPImageProcessor (its Pillow backend) fed `numpy_to_pil` of the same images --
the two host stages of run_safety_checker (custom_sd.py:376-384). The bound is derived, not measured: at most 2 of 8-bit's 256 levels
per pixel, 2 / (255 std_c) after normalisation. Pillow's resampler uses 22-bit fixed-point taps, so a pass can differ from another
evaluation of the same filter by one level only where the exact value lies at a rounding boundary; the second pass spreads a one-level
input error over sum |w| <= 1.26 and may flip its own rounding once."""
import functools

import torch

from spider_amd.safety import CLIP_MEAN, CLIP_STD

# name -> (H, W, shortest edge = crop)
PREPROCESS_CASES = {
    "down64": (64, 64, 56),            # a mild downscale
    "up40": (40, 40, 56),              # an upscale: support exactly 2
    "rect96x128": (96, 128, 56),       # non-square: the crop bites
    "real512": (512, 512, 224),        # the real ratio 16/7
    "checker512": (512, 512, 224),     # 8 x 8-block checkerboard: the worst case for the negative lobes and the clip
}


@functools.lru_cache(maxsize=None)
def case_images(name: str, B: int = 1) -> torch.Tensor:
    """[B,3,H,W] fp32 in [0,1]; treat as read-only (cached)."""
    H, W, _ = PREPROCESS_CASES[name]
    if name == "checker512":
        y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        board = (((y // 8) + (x // 8)) % 2).float()
        # image b, channel c: the board, its inverse, or the board shifted by half a block
        return torch.stack([torch.stack([board if (b + c) % 3 == 0 else (1 - board if (b + c) % 3 == 1 else board.roll(4, 1))
                                         for c in range(3)]) for b in range(B)]).contiguous()
    g = torch.Generator().manual_seed(100 + sorted(PREPROCESS_CASES).index(name))
    return torch.rand(B, 3, H, W, generator=g)


@functools.lru_cache(maxsize=None)
def reference_pixel_values(name: str, B: int = 1) -> torch.Tensor:
    """CLIPImageProcessor(numpy_to_pil(images)).pixel_values, [B,3,crop,crop] fp32; computed once per case, read-only."""
    from transformers import CLIPImageProcessor
    from spider_amd.pipelines import numpy_to_pil
    _, _, size = PREPROCESS_CASES[name]
    proc = CLIPImageProcessor(size={"shortest_edge": size}, crop_size={"height": size, "width": size}, resample=3,
                              image_mean=list(CLIP_MEAN), image_std=list(CLIP_STD))
    pil = numpy_to_pil(case_images(name, B).permute(0, 2, 3, 1).numpy())
    return torch.as_tensor(proc(pil, return_tensors="pt")["pixel_values"]).float()


def level_bound(levels: float = 2.0) -> torch.Tensor:
    """`levels` 8-bit levels after normalisation, per channel: [1,3,1,1]"""
    return (levels / (255.0 * torch.tensor(CLIP_STD))).view(1, 3, 1, 1)


def half_ulp(mag: torch.Tensor, dtype) -> torch.Tensor:
    """half a unit in the last place of `dtype` (bf16: 8 significand bits, f16: 11, subnormals below 2^-14) at magnitude `mag`"""
    _, e = torch.frexp(mag.float().clamp_min(1e-30))              # mag = m * 2^e, m in [0.5, 1): the binade starts at 2^(e - 1)
    bits, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    return torch.ldexp(torch.ones_like(mag, dtype=torch.float32), (e - 1).clamp_min(emin) - (bits - 1) - 1)


def unpatchify(rows: torch.Tensor, B: int, crop: int, patch: int) -> torch.Tensor:
    """patch rows [B * g^2, Kp] -> ([B,3,crop,crop], the pad columns [B * g^2, Kp - 3 patch^2])"""
    g, K = crop // patch, 3 * patch * patch
    img = rows[:, :K].reshape(B, g, g, 3, patch, patch).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, crop, crop)
    return img, rows[:, K:]


def decide_cases(D: int = 64):
    """Constructed embeddings for the decision rule: dict name -> (image_embeds [B,D], concepts [17,D], special [3,D], thr_c [17],
    thr_s [3], expected flags). Concepts and special-care concepts are orthonormal axes, so cos against axis i is the i-th coordinate
    of the normalised embedding, and every score is set by construction. Values are exact in bf16 and f16 where the case needs it."""
    n_c, n_s = 17, 3
    eye = torch.eye(D)
    concepts, special = eye[:n_c].clone(), eye[n_c:n_c + n_s].clone()
    free = eye[n_c + n_s]                                      # an axis orthogonal to every concept
    big = torch.full((n_c,), 2.0), torch.full((n_s,), 2.0)     # thresholds nothing reaches

    def emb(a_c, a_s, a_free):
        """a_c on concept 0, a_s on special-care concept 0, a_free on the free axis: small integers with an integer norm, so the
        embedding is exact in fp32, bf16 and f16 and its cosines are a_c / norm and a_s / norm to one fp32 rounding"""
        return a_c * concepts[0] + a_s * special[0] + a_free * free

    cases = {}
    thr_c = big[0].clone(); thr_c[0] = 0.5
    cases["cos1_flags"] = (emb(1, 0, 0)[None], concepts, special, thr_c, big[1], [True])
    cases["orthogonal_clean"] = (emb(0, 0, 1)[None], concepts, special, thr_c, big[1], [False])
    # concept 0 at cos - thr = 0.6 - 0.605 = -0.005: unflagged alone; flagged once special-care concept 0 fires (cos 0.8 > 0.25):
    # -0.005 + 0.01 = +0.005. The +0.01 also reaches the special-care concepts that follow: special 1 (cos 0, thr 0.005) scores
    # -0.005 before and +0.005 after (visible in the scores; a special-care hit does not flag by itself)
    thr_c2 = big[0].clone(); thr_c2[0] = 0.605
    thr_s2 = big[1].clone(); thr_s2[0] = 0.25; thr_s2[1] = 0.005
    cases["adjust_alone"] = (emb(3, 0, 4)[None], concepts, special, thr_c2, big[1], [False])
    cases["adjust_cascade"] = (emb(3, 4, 0)[None], concepts, special, thr_c2, thr_s2, [True])
    # raw scores 0.0004 / 0.0006 on either side of the rounding step: round(.., 3) gives 0.0 (no flag) / 0.001 (flag)
    thr_lo = big[0].clone(); thr_lo[0] = 0.6 - 0.0004
    thr_hi = big[0].clone(); thr_hi[0] = 0.6 - 0.0006
    cases["round_down_0004"] = (emb(3, 0, 4)[None], concepts, special, thr_lo, big[1], [False])
    cases["round_up_0006"] = (emb(3, 0, 4)[None], concepts, special, thr_hi, big[1], [True])
    # a special-care hit alone does not flag
    cases["special_only"] = (emb(0, 3, 4)[None], concepts, special, big[0], thr_s2, [False])
    # B = 3 with mixed flags, the cascade in the middle row
    cases["batch3_mixed"] = (torch.stack([emb(3, 0, 4), emb(3, 4, 0), emb(0, 0, 1)]), concepts, special, thr_c2, thr_s2,
                             [False, True, False])
    return cases


def rounding_margin(image_embeds, concepts, special, thr_c, thr_s) -> float:
    """smallest distance of any pre-rounding score x = cos - thr + adjustment (host, fp32) from a rounding step of round(x, 3),
    i.e. from (k + 0.5) / 1000, over both possible adjustments"""
    import torch.nn.functional as F
    e = F.normalize(image_embeds.float(), dim=-1)
    cos = torch.cat([e @ F.normalize(special.float(), dim=-1).T, e @ F.normalize(concepts.float(), dim=-1).T], 1)
    thr = torch.cat([thr_s.float(), thr_c.float()])
    m = 1.0
    for adj in (0.0, 0.01):
        x = (cos - thr + adj) * 1000.0
        m = min(m, float(((x - torch.floor(x)) - 0.5).abs().min()) / 1000.0)
    return m

"""Shared images, case table and references of the Qwen2-VL image patch tests (test_qwen_image_cpu.py, test_qwen_image_gpu.py).

The reference is transformers' Qwen2VLImageProcessorPil(min_pixels=, max_pixels=)(images=..., return_tensors="pt"), built directly (no
checkpoint). The checks are bit equality: Pillow resizes 8-bit images in integers, and normalisation maps 256 values per channel.
`restate` is the same computation in numpy from the host planning code the kernel reads (ops.qwen_image_tables: smart_resize,
bicubic_taps, descriptors, lookup table) and the row / column index of the patch layout."""
import functools

import numpy as np
import torch

from spider_amd import ops
from spider_amd.image_features import ImagePatchConfig

LO, HI = 56 * 56, 28 * 28 * 1280          # Qwen2VLImageProcessor's own bounds: 3136 / 1003520

# (name, H, W, kind, min_pixels, max_pixels, grid (t, h, w)): the smallest shapes at which each thing can go wrong
CASES = (
    ("min_pixels_ceil_upscale", 37, 53, "random", LO, HI, (1, 4, 6)),
    ("upscale_2x_taps_clipped", 28, 28, "random", LO, HI, (1, 4, 4)),
    ("one_axis_identity", 100, 140, "random", LO, HI, (1, 8, 10)),
    ("both_axes_identity", 56, 84, "random", LO, HI, (1, 4, 6)),
    ("max_pixels_floor_downscale", 300, 500, "random", LO, 12544, (1, 6, 10)),
    ("downscale_87_taps", 600, 600, "random", LO, 3136, (1, 2, 2)),
    ("single_merge_column", 900, 31, "random", LO, 31360, (1, 64, 2)),
    ("overshoot_clipped", 61, 500, "binary", LO, HI, (1, 4, 36)),
    ("constant_0", 56, 56, 0, LO, HI, (1, 4, 4)),
    ("constant_128", 56, 56, 128, LO, HI, (1, 4, 4)),
    ("constant_255", 56, 56, 255, LO, HI, (1, 4, 4)),
)
NAMES = tuple(c[0] for c in CASES)
BY_NAME = {c[0]: c for c in CASES}


def config(min_pixels=LO, max_pixels=HI, **kw) -> ImagePatchConfig:
    return ImagePatchConfig(min_pixels=min_pixels, max_pixels=max_pixels, **kw)


def case_config(name: str) -> ImagePatchConfig:
    return config(BY_NAME[name][4], BY_NAME[name][5])


def groups():
    """{(min_pixels, max_pixels): [case names]}: the rows that share one configuration go in as one packed batch of mixed sizes"""
    out = {}
    for c in CASES:
        out.setdefault((c[4], c[5]), []).append(c[0])
    return out


@functools.lru_cache(maxsize=None)
def image(name: str) -> np.ndarray:
    """uint8 [H, W, 3], fixed seed per case; treat as read-only (cached)."""
    _, H, W, kind, _, _, _ = BY_NAME[name]
    g = np.random.default_rng(100 + NAMES.index(name))
    if kind == "random":
        a = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "binary":
        a = (g.integers(0, 2, (H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)
    else:
        a = np.full((H, W, 3), kind, dtype=np.uint8)
    a.setflags(write=False)
    return a


def hf_processor(cfg: ImagePatchConfig):
    """a fresh host processor: its constructor writes the bounds into a dict the class shares, so both are always given"""
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil
    return Qwen2VLImageProcessorPil(min_pixels=cfg.min_pixels, max_pixels=cfg.max_pixels, patch_size=cfg.patch_size,
                                    temporal_patch_size=cfg.temporal_patch_size, merge_size=cfg.merge_size)


def reference(images, cfg: ImagePatchConfig):
    """the host processor on a list of images -> (pixel_values fp32 [T, 3 Tp P^2], image_grid_thw int64 [n, 3])"""
    out = hf_processor(cfg)(images=[np.asarray(a) if isinstance(a, np.ndarray) else a for a in images], return_tensors="pt")
    return out["pixel_values"], out["image_grid_thw"]


@functools.lru_cache(maxsize=None)
def case_reference(name: str):
    """computed once per case, read-only"""
    return reference([image(name)], case_config(name))


def _pass(src, bounds, taps):
    """one 8-bit resampling pass along axis 0 of src [n_in, ...] uint8 -> [n_out, ...] uint8: clip8((sum v tap + 2^21) >> 22)"""
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    s = src.astype(np.int64)
    for j, (x0, n) in enumerate(bounds):
        acc = np.tensordot(taps[j, :n].astype(np.int64), s[x0:x0 + n], axes=(0, 0)) + (1 << (ops.RESIZE_PRECISION_BITS - 1))
        out[j] = np.clip(acc >> ops.RESIZE_PRECISION_BITS, 0, 255)
    return out


def restate(images, cfg: ImagePatchConfig, dtype=torch.float32):
    """numpy restatement from the tables the kernel reads -> (pixel_values [T, 3 Tp P^2] of `dtype`, image_grid_thw int64 [n, 3])"""
    imgs = [np.asarray(a) for a in images]
    t = ops.qwen_image_tables([a.shape[:2] for a in imgs], cfg, "cpu")
    desc, tabs = t["desc"].numpy(), t["tabs"].numpy()
    lut = t["lut"][dtype].reshape(-1)
    lut = lut.view(torch.float32) if dtype == torch.float32 else lut.to(torch.int16).view(torch.bfloat16)      # [3 * 256] output elements
    P, m, Tp = cfg.patch_size, cfg.merge_size, cfg.temporal_patch_size
    out = torch.full((t["rows"], t["cols"]), float("nan"), dtype=dtype)
    packed = np.concatenate([a.reshape(-1) for a in imgs])
    for d in desc:
        in_off, H, W, Ho, Wo, xb, xt, ksx, yb, yt, ksy, row0, _, y_first, y_count, _ = (int(v) for v in d)
        img = packed[in_off:in_off + H * W * 3].reshape(H, W, 3)
        xbounds, xtaps = tabs[xb:xb + 2 * Wo].reshape(Wo, 2), tabs[xt:xt + Wo * ksx].reshape(Wo, ksx)
        ybounds, ytaps = tabs[yb:yb + 2 * Ho].reshape(Ho, 2), tabs[yt:yt + Ho * ksy].reshape(Ho, ksy)
        assert y_first == ybounds[:, 0].min() and y_first + y_count == (ybounds[:, 0] + ybounds[:, 1]).max()
        h = _pass(img.transpose(1, 0, 2), xbounds, xtaps).transpose(1, 0, 2)                  # horizontal first: [H, Wo, 3]
        v = _pass(h, ybounds, ytaps)                                                         # [Ho, Wo, 3]
        y, x = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
        gh, dy, gw, dx = y // P, y % P, x // P, x % P
        row = ((gh // m * (Wo // P // m) + gw // m) * m + gh % m) * m + gw % m + row0
        for c in range(3):
            val = lut[torch.from_numpy(c * 256 + v[:, :, c].astype(np.int64))]
            for tt in range(Tp):
                out[torch.from_numpy(row), torch.from_numpy(((c * Tp + tt) * P + dy) * P + dx)] = val
    return out, torch.tensor(t["grid"], dtype=torch.int64)

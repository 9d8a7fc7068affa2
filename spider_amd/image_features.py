"""Image input of Qwen2.5-Omni on the device: what `Qwen2_5OmniProcessor.image_processor` (transformers' Qwen2-VL image processor, PIL
backend) computes on the host -- `smart_resize` with Pillow's antialiased BICUBIC, `(v / 255 - mean) / std`, the merge-block patch order
with the frame written `temporal_patch_size` times -- from the images' uint8 pixels in two launches (csrc/image_features.hip through
ops.qwen_image_patches). The result carries the host processor's bits: Pillow's 22-bit integer taps (ops.bicubic_taps) with both passes
rounded to 8 bits, and a [3, 256] lookup table that numpy fills the way transformers' `rescale` and `normalize` do, cast once to the
output format. `pixel_values` is bf16 by default (the vision tower's first step is that cast); `dtype=torch.float32` gives the host's
fp32 tensor.

    ImagePatchConfig              the keys of preprocessor_config.json the path implements; anything else raises, naming the key
    ImagePatchEngine              images -> (pixel_values on the device, image_grid_thw on the host)
    DeviceQwen2VLImageProcessor   stands where `processor.image_processor` stands (SpiderFreeInfer(device_image_features=True))

Video frames (`pixel_values_videos`) are not covered: transformers' video processor runs on torchvision, which gives no host
result to hold a device path to; `videos=` stays with the host processor."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, replace
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
BICUBIC = 3          # PIL.Image.Resampling.BICUBIC


@dataclass(frozen=True)
class ImagePatchConfig:
    """Qwen2VLImageProcessor's own defaults; Qwen2.5-Omni's preprocessor_config.json sets max_pixels = 12845056."""
    min_pixels: int = 56 * 56
    max_pixels: int = 28 * 28 * 1280
    patch_size: int = 14
    temporal_patch_size: int = 2
    merge_size: int = 2
    image_mean: Tuple[float, ...] = OPENAI_CLIP_MEAN
    image_std: Tuple[float, ...] = OPENAI_CLIP_STD
    rescale_factor: float = 1 / 255
    resample: int = BICUBIC

    def __post_init__(self):
        for key in ("image_mean", "image_std"):
            v = getattr(self, key)
            if isinstance(v, (int, float)) or len(v) != 3:
                raise NotImplementedError(f"{key}={v!r} is not implemented (three values, one per RGB channel)")
            object.__setattr__(self, key, tuple(float(x) for x in v))
        if int(self.resample) != BICUBIC:
            raise NotImplementedError(f"resample={self.resample!r} is not implemented (only 3, PIL's BICUBIC)")
        if float(self.rescale_factor) != 1 / 255:
            raise NotImplementedError(f"rescale_factor={self.rescale_factor!r} is not implemented (only 1 / 255)")
        for key in ("min_pixels", "max_pixels", "patch_size", "temporal_patch_size", "merge_size"):
            if int(getattr(self, key)) < 1:
                raise ValueError(f"{key} must be positive, got {getattr(self, key)!r}")
            object.__setattr__(self, key, int(getattr(self, key)))
        object.__setattr__(self, "resample", BICUBIC)
        object.__setattr__(self, "rescale_factor", 1 / 255)

    @property
    def factor(self) -> int:
        return self.patch_size * self.merge_size

    @property
    def patch_dim(self) -> int:
        return 3 * self.temporal_patch_size * self.patch_size ** 2

    @property
    def size(self) -> dict:
        return {"shortest_edge": self.min_pixels, "longest_edge": self.max_pixels}

    @classmethod
    def from_preprocessor_config(cls, src) -> "ImagePatchConfig":
        """src: a dict, a preprocessor_config.json or a checkpoint directory. Both spellings of the pixel bounds are read
        (`min_pixels` / `max_pixels`, which win as in transformers, and `size` {shortest_edge, longest_edge}); keys of the audio side
        and names the processor keeps for itself are ignored; a switch the device path does not implement raises, naming the key."""
        if not isinstance(src, dict):
            path = os.path.join(src, "preprocessor_config.json") if os.path.isdir(src) else src
            with open(path) as f:
                src = json.load(f)
        for key in ("do_resize", "do_rescale", "do_normalize"):
            if src.get(key) is False:
                raise NotImplementedError(f"{key}=False is not implemented: the device path always resizes, rescales and normalises")
        for key in ("do_center_crop", "do_pad"):
            if src.get(key):
                raise NotImplementedError(f"{key}={src[key]!r} is not implemented")
        if src.get("do_convert_rgb") is False:
            raise NotImplementedError("do_convert_rgb=False is not implemented: PIL images are converted to RGB")
        kw = {}
        size = src.get("size")
        if size is not None:
            size = dict(size)
            if "shortest_edge" not in size or "longest_edge" not in size:
                raise NotImplementedError(f"size={size!r} is not implemented (shortest_edge and longest_edge, the pixel bounds)")
            kw.update(min_pixels=size["shortest_edge"], max_pixels=size["longest_edge"])
        for key in ("min_pixels", "max_pixels", "patch_size", "temporal_patch_size", "merge_size", "image_mean", "image_std",
                    "rescale_factor", "resample"):
            if src.get(key) is not None:
                kw[key] = src[key]
        if "resample" in kw:
            kw["resample"] = int(getattr(kw["resample"], "value", kw["resample"]))
        return cls(**kw)

    from_pretrained = from_preprocessor_config


def _to_hwc_u8(img):
    """one image -> uint8 [H, W, 3], a numpy array on the host or a torch tensor where the image already lies on a device.
    PIL images of any mode go through .convert("RGB"), as the host processor does; arrays and tensors must be uint8 with three
    channels, first ([3, H, W]) or last ([H, W, 3]; a 3 x H x 3 array counts as channels-first, as in transformers)."""
    if hasattr(img, "convert") and hasattr(img, "mode"):                       # PIL.Image.Image
        return np.asarray(img if img.mode == "RGB" else img.convert("RGB"), dtype=np.uint8)
    if isinstance(img, np.ndarray):
        a = img
    elif isinstance(img, torch.Tensor):
        a = img.detach()
    else:
        raise TypeError(f"an image must be a PIL image, a uint8 numpy array or a uint8 torch tensor, got {type(img).__name__}")
    if a.dtype not in (np.uint8, torch.uint8):
        raise TypeError(f"images must be uint8 (0 ... 255), got {a.dtype}: float images are not rescaled on this path")
    if a.ndim != 3:
        raise ValueError(f"an image must have three dimensions (HWC or CHW), got shape {tuple(a.shape)}: pass a batch as a list of images")
    if a.shape[0] == 3:
        a = a.transpose(1, 2, 0) if isinstance(a, np.ndarray) else a.permute(1, 2, 0)
    elif a.shape[2] != 3:
        raise ValueError(f"an image must have three channels, first or last, got shape {tuple(a.shape)}")
    if isinstance(a, torch.Tensor) and not a.is_cuda:
        a = a.numpy()
    return a


def image_sizes(images) -> Tuple[Tuple[int, int], ...]:
    """(H, W) per image without touching the pixels: all `grid_thw` and `would_capture` need"""
    out = []
    for img in images:
        if hasattr(img, "convert") and hasattr(img, "mode"):
            out.append((img.height, img.width))
        else:
            a = _to_hwc_u8(img)
            out.append((int(a.shape[0]), int(a.shape[1])))
    return tuple(out)


def _as_list(images) -> list:
    if isinstance(images, (list, tuple)):
        flat = []
        for x in images:
            flat.extend(x if isinstance(x, (list, tuple)) else [x])
        return flat
    return [images]


def _host_tensor(a: np.ndarray) -> torch.Tensor:
    """a tensor over the array's memory, read only to be copied to the device: PIL hands out read-only arrays, and a copy made just to
    quiet torch's warning about them would cost a pass over the image"""
    import warnings
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
        return torch.from_numpy(a)


class ImagePatchEngine:
    def __init__(self, cfg: ImagePatchConfig = ImagePatchConfig(), device="cuda:0", dtype=torch.bfloat16):
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", dtype=torch.bfloat16):
        """a checkpoint directory: reads its preprocessor_config.json"""
        return cls(ImagePatchConfig.from_preprocessor_config(path), device, dtype)

    def grid_thw(self, sizes: Sequence[Tuple[int, int]]) -> torch.Tensor:
        """image_grid_thw int64 [n, 3] for images of these (H, W): host arithmetic only (placeholder expansion, would_capture)"""
        c = self.cfg
        rows = []
        for H, W in sizes:
            Ho, Wo = ops.qwen_smart_resize(int(H), int(W), c.factor, c.min_pixels, c.max_pixels)
            rows.append([1, Ho // c.patch_size, Wo // c.patch_size])
        return torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)

    def tables(self, sizes) -> dict:
        return ops.qwen_image_tables(sizes, self.cfg, self.device)

    def pack(self, images):
        """images -> (packed uint8 HWC pixels on the device, sizes). Images on the host are joined and copied in ONE upload; images
        already on the device are joined there."""
        imgs = [_to_hwc_u8(x) for x in _as_list(images)]
        if not imgs:
            raise ValueError("ImagePatchEngine: no images")
        sizes = tuple((int(a.shape[0]), int(a.shape[1])) for a in imgs)
        if all(isinstance(a, np.ndarray) for a in imgs):
            flat = [np.ascontiguousarray(a).reshape(-1) for a in imgs]
            packed = _host_tensor(flat[0] if len(flat) == 1 else np.concatenate(flat)).to(self.device)
        else:
            flat = [(_host_tensor(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(self.device).contiguous().reshape(-1)
                    for a in imgs]
            packed = flat[0] if len(flat) == 1 else torch.cat(flat)
        return packed, sizes

    @torch.no_grad()
    def __call__(self, images, dtype=None, out=None):
        """images: one image or a list (PIL of any mode, uint8 numpy HWC, uint8 torch CHW / HWC on the host or on the device), each
        its own size. -> (pixel_values [sum t h w, 3 Tp P^2] on the device, bf16 unless `dtype` / the engine's dtype says fp32;
        image_grid_thw int64 [n, 3] on the host). One upload and one pair of launches per call."""
        with torch.cuda.device(self.device):
            packed, sizes = self.pack(images)
            t = self.tables(sizes)
            px = ops.qwen_image_patches(packed, t, self.dtype if dtype is None else dtype, out)
        return px, torch.tensor(t["grid"], dtype=torch.int64)


# ------------------------------------------------------------------------------------------ drop-in for processor.image_processor
class DeviceQwen2VLImageProcessor:
    """Stands where `Qwen2_5OmniProcessor.image_processor` stands: `__call__(images=..., return_tensors="pt")` returns a BatchFeature
    with `pixel_values` on the device (bf16 unless built or called with dtype=torch.float32, which gives the host processor's fp32
    bits) and `image_grid_thw` int64 on the host. Per call `min_pixels` + `max_pixels` (both, as the host class asks) or `size`
    replace the bounds; any other keyword that differs from the configuration raises NotImplementedError. `videos=` is not served."""
    model_input_names = ["pixel_values", "image_grid_thw"]

    def __init__(self, cfg: ImagePatchConfig = ImagePatchConfig(), device="cuda:0", dtype=torch.bfloat16):
        self.cfg, self.device, self.dtype = cfg, torch.device(device), dtype
        self.engine = ImagePatchEngine(cfg, device, dtype)
        self.merge_size, self.patch_size, self.temporal_patch_size = cfg.merge_size, cfg.patch_size, cfg.temporal_patch_size
        self.min_pixels, self.max_pixels, self.size = cfg.min_pixels, cfg.max_pixels, cfg.size
        self.image_mean, self.image_std, self.rescale_factor, self.resample = list(cfg.image_mean), list(cfg.image_std), cfg.rescale_factor, cfg.resample
        self.do_resize = self.do_rescale = self.do_normalize = self.do_convert_rgb = True

    @classmethod
    def from_image_processor(cls, ip, device="cuda:0", dtype=torch.bfloat16):
        """from a transformers Qwen2-VL image processor (its own attributes are the configuration)"""
        keys = ("size", "patch_size", "temporal_patch_size", "merge_size", "image_mean", "image_std", "rescale_factor", "resample",
                "do_resize", "do_rescale", "do_normalize", "do_convert_rgb", "do_center_crop", "do_pad")
        src = {k: getattr(ip, k) for k in keys if getattr(ip, k, None) is not None}
        if "size" in src:
            src["size"] = {k: src["size"][k] for k in ("shortest_edge", "longest_edge") if src["size"].get(k) is not None}
        else:                                                            # older classes keep the bounds as attributes of their own
            src.update({k: getattr(ip, k) for k in ("min_pixels", "max_pixels") if getattr(ip, k, None) is not None})
        return cls(ImagePatchConfig.from_preprocessor_config(src), device, dtype)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0", dtype=torch.bfloat16):
        return cls(ImagePatchConfig.from_preprocessor_config(path), device, dtype)

    def _call_config(self, kw: dict) -> ImagePatchConfig:
        cfg = self.cfg
        size, lo, hi = kw.pop("size", None), kw.pop("min_pixels", None), kw.pop("max_pixels", None)
        if size is not None:
            size = dict(size)
            if not size.get("shortest_edge") or not size.get("longest_edge"):
                raise ValueError(f"`size` dict must contain 'shortest_edge' and 'longest_edge' keys but got {size}.")
            cfg = replace(cfg, min_pixels=size["shortest_edge"], max_pixels=size["longest_edge"])
        if (lo is None) != (hi is None):
            raise ValueError("pass min_pixels and max_pixels together (or size=): the host processor ignores one given alone")
        if lo is not None:
            cfg = replace(cfg, min_pixels=lo, max_pixels=hi)
        same = dict(do_resize=True, do_rescale=True, do_normalize=True, do_convert_rgb=True, resample=cfg.resample,
                    rescale_factor=cfg.rescale_factor, image_mean=cfg.image_mean, image_std=cfg.image_std, patch_size=cfg.patch_size,
                    temporal_patch_size=cfg.temporal_patch_size, merge_size=cfg.merge_size, do_center_crop=False, do_pad=False,
                    input_data_format=None, data_format=None, device=None, disable_grouping=None, crop_size=None, pad_size=None,
                    default_to_square=None)
        for k, v in kw.items():
            if v is None:
                continue
            if k not in same:
                raise NotImplementedError(f"DeviceQwen2VLImageProcessor: {k}={v!r} is not implemented")
            want = same[k]
            v = int(getattr(v, "value", v)) if k == "resample" else (tuple(float(x) for x in v) if k in ("image_mean", "image_std") else v)
            if k == "device":
                if torch.device(v) != self.device:
                    raise NotImplementedError(f"DeviceQwen2VLImageProcessor: device={v!r} differs from the engine's {self.device}")
            elif k in ("do_center_crop", "do_pad"):
                if v:
                    raise NotImplementedError(f"DeviceQwen2VLImageProcessor: {k}={v!r} is not implemented")
            elif want is None or v != want:
                raise NotImplementedError(f"DeviceQwen2VLImageProcessor: {k}={v!r} is not implemented (configured: {want!r})")
        return cfg

    def __call__(self, images=None, videos=None, return_tensors="pt", dtype=None, **kw):
        if videos is not None:
            raise NotImplementedError("DeviceQwen2VLImageProcessor: videos= is not implemented (frames stay with the host video processor)")
        if images is None:
            raise ValueError("DeviceQwen2VLImageProcessor: images is required")
        if getattr(return_tensors, "value", return_tensors) != "pt":
            raise NotImplementedError(f"DeviceQwen2VLImageProcessor: return_tensors={return_tensors!r} is not implemented (only 'pt')")
        cfg = self._call_config(kw)
        eng = self.engine if cfg == self.cfg else ImagePatchEngine(cfg, self.device, self.dtype)
        px, grid = eng(images, dtype=dtype)
        from transformers.image_processing_utils import BatchFeature       # the image processors' own subclass
        return BatchFeature({"pixel_values": px, "image_grid_thw": grid})

    preprocess = __call__

    def get_number_of_image_patches(self, height: int, width: int, images_kwargs: Optional[dict] = None) -> int:
        cfg = self._call_config(dict(images_kwargs or {}))
        _, h, w = ImagePatchEngine(cfg, self.device).grid_thw([(height, width)])[0].tolist()
        return h * w


def is_qwen2vl_image_processor(ip) -> bool:
    """by class name along the MRO: no import of transformers for a processor that has none"""
    return any(c.__name__.startswith("Qwen2VLImageProcessor") for c in type(ip).__mro__)

"""Cost of the image preprocessing of a request that carries a picture, both sides of the change in ONE process on the same images:
  (a) transformers' Qwen2VLImageProcessorPil on the host CPU under Qwen2.5-Omni's bounds (min_pixels 3136, max_pixels 12845056): wall
      time, warm, median of `--hf-iters` calls, and the host -> device copy of the fp32 tensor it leaves;
  (b) ops.qwen_image_patches: the two launches between two HIP events, uint8 pixels already on the device, tables warm, median of
      `--iters` calls (bf16 and fp32 output); and ImagePatchEngine end to end (packing, upload of the uint8 pixels, launches, a final
      synchronise) as wall time;
for one 448 x 448 image, one 1092 x 1456 image and a 3000 x 4000 photo. Bytes written per output pixel: 3 channels x temporal 2 x
2 (bf16). `--device-only` runs (b) alone: the form to put under `rocprofv3 --kernel-trace --stats -- python
scripts/exp/image_patches_cost.py --device-only` for the two kernels' own times (the store bandwidth of the second launch).

    PYTHONPATH=. python scripts/exp/image_patches_cost.py [--iters 30] [--hf-iters 5] [--device-only]"""
import argparse
import statistics
import time

import numpy as np
import torch

from spider_amd import ops
from spider_amd.image_features import ImagePatchConfig, ImagePatchEngine

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--hf-iters", type=int, default=5)
ap.add_argument("--device-only", action="store_true")
args = ap.parse_args()

cfg = ImagePatchConfig(max_pixels=12845056)
rng = np.random.default_rng(0)
IMAGES = {"448 x 448": (448, 448), "1092 x 1456": (1092, 1456), "3000 x 4000": (3000, 4000)}


def wall_ms(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def event_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t), min(t), max(t)


eng = ImagePatchEngine(cfg, "cuda:0")
print(f"torch threads {torch.get_num_threads()}; device {torch.cuda.get_device_name(0)}; iters {args.iters}, hf-iters {args.hf_iters}")
for name, (H, W) in IMAGES.items():
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    packed, sizes = eng.pack([img])
    t = eng.tables(sizes)
    _, gh, gw = t["grid"][0]
    print(f"{name}: grid (1, {gh}, {gw}) = {t['rows']} rows, resized {gh * 14} x {gw * 14}, taps {int(t['desc'][0, 7])} / {int(t['desc'][0, 10])}; "
          f"uint8 in {packed.numel() / 1e6:.1f} MB, intermediate {t['tmp_bytes'] / 1e6:.1f} MB")
    for dt, nm in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        out = torch.empty(t["rows"], t["cols"], dtype=dt, device="cuda:0")
        d = event_ms(lambda: ops.qwen_image_patches(packed, t, dt, out), max(args.iters, 20))
        mb = out.numel() * out.element_size() / 1e6
        print(f"{name}: (b) both launches, {nm} out {mb:.1f} MB: median {d[0] * 1e3:.1f} us (min {d[1] * 1e3:.1f}, max {d[2] * 1e3:.1f}) "
              f"= {mb / d[0] / 1e3:.2f} TB/s of output over both launches")

    def device():
        eng([img])
        torch.cuda.synchronize()
    w = wall_ms(device, max(args.iters, 20))
    print(f"{name}: (b) engine end to end (pack, upload {packed.numel() / 1e6:.1f} MB, launches, synchronise): median {w[0]:.3f} ms "
          f"(min {w[1]:.3f}, max {w[2]:.3f})")
    if args.device_only:
        continue
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import Qwen2VLImageProcessorPil
    ip = Qwen2VLImageProcessorPil(min_pixels=cfg.min_pixels, max_pixels=cfg.max_pixels)
    host = lambda: ip(images=[img], return_tensors="pt")
    h = wall_ms(host, args.hf_iters, warm=1)
    ref = host()["pixel_values"]

    def upload():
        ref.to("cuda:0")
        torch.cuda.synchronize()
    u = wall_ms(upload, max(args.hf_iters, 5), warm=1)
    print(f"{name}: (a) host processor median {h[0]:.1f} ms (min {h[1]:.1f}, max {h[2]:.1f}; {args.hf_iters} calls) + upload of "
          f"{ref.numel() * 4 / 1e6:.1f} MB fp32 {u[0]:.2f} ms; (a) / (b end to end) = {(h[0] + u[0]) / w[0]:.0f}x")
    got16, got32 = eng([img])[0].cpu(), eng([img], dtype=torch.float32)[0].cpu()
    print(f"{name}: bf16 rows equal the host's: {bool(torch.equal(got16, ref.to(torch.bfloat16)))}; fp32 rows equal: {bool(torch.equal(got32, ref))}")

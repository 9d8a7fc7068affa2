"""Cost of the audio feature extraction of a spoken request, both sides of the change in ONE process on the same clips:
  (a) transformers.WhisperFeatureExtractor on the host CPU, called the way Qwen2_5OmniProcessor calls it (padding="max_length":
      every clip padded to 300 s, 30,000 STFT frames, a [B, 128, 30000] fp32 result), warm, median of `--hf-iters` calls;
  (b) LogMelEngine: host packing + host -> device copy of the waveforms + the two launches, torch.cuda.synchronize at the end, wall
      time, median of `--iters` calls after warm-up;
for one 30 s clip and for three clips (30 s, 12 s, 5 s). `--device-only` runs (b) alone: the form to put under
`rocprofv3 --kernel-trace --stats -- python scripts/exp/logmel_cost.py --device-only` for the two kernels' own times.

    PYTHONPATH=. python scripts/exp/logmel_cost.py [--iters 30] [--hf-iters 10] [--device-only]"""
import argparse
import statistics
import time

import numpy as np
import torch

from spider_amd.audio_features import LogMelConfig, LogMelEngine

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--hf-iters", type=int, default=10)
ap.add_argument("--device-only", action="store_true")
args = ap.parse_args()

cfg = LogMelConfig()
rng = np.random.default_rng(0)
clip = lambda seconds: (0.1 * rng.standard_normal(int(seconds * cfg.sampling_rate))).astype(np.float32)
BATCHES = {"one 30 s clip": [clip(30)], "three clips (30 s, 12 s, 5 s)": [clip(30), clip(12), clip(5)]}


def median_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


eng = LogMelEngine(cfg, "cuda:0")
print(f"torch threads {torch.get_num_threads()}; device {torch.cuda.get_device_name(0)}")
for name, clips in BATCHES.items():
    def device():
        eng(clips, cfg.sampling_rate)
        torch.cuda.synchronize()
    d = median_ms(device, args.iters)
    print(f"{name}: (b) device path  median {d[0]:.3f} ms  (min {d[1]:.3f}, max {d[2]:.3f}; {args.iters} calls)")
    if args.device_only:
        continue
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=cfg.feature_size, n_fft=cfg.n_fft, hop_length=cfg.hop_length, chunk_length=cfg.chunk_length)
    host = lambda: fe(clips, sampling_rate=cfg.sampling_rate, padding="max_length", return_attention_mask=True, return_tensors="pt")
    t0 = time.perf_counter()
    ref = host()
    first = (time.perf_counter() - t0) * 1e3
    h = median_ms(host, args.hf_iters, warm=1)
    print(f"{name}: (a) HF extractor on the host CPU  median {h[0]:.1f} ms  (min {h[1]:.1f}, max {h[2]:.1f}; {args.hf_iters} calls; "
          f"first call {first:.1f} ms)")
    print(f"{name}: (a) / (b) = {h[0] / d[0]:.0f}x")
    f, m, _ = eng(clips, cfg.sampling_rate)
    print(f"{name}: max |device - HF| = {float((f.cpu() - ref['input_features']).abs().max()):.3e}; masks equal: "
          f"{bool(torch.equal(m.cpu(), ref['attention_mask'].to(torch.int32)))}")

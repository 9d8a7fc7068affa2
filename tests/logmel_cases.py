"""Shared clips, references and bounds of the log-mel feature tests (test_logmel_cpu.py, test_logmel_gpu.py).

Two references: `spider_amd.audio_features.logmel_host`, the fp64 definition, and transformers' WhisperFeatureExtractor, built
directly with Qwen2.5-Omni's 128 / 400 / 160 and a short chunk_length (no checkpoint), called the way Qwen2_5OmniProcessor calls it.

Bounds (stated, not measured on the kernel): the audio tower reads the features as bf16 (qwen_omni.py, AudioTowerEngine.forward);
values lie in [-1.5, 2), so a bf16 half-ulp in [0.5, 1) is 2^-9 and 2^-13 is 1/16 of it. definition <-> HF's own fp32 path gets the
same 2^-13, and device <-> HF the two distances added, 2^-12."""
import functools
import math

import numpy as np
import torch

from spider_amd.audio_features import LogMelConfig, logmel_host, valid_frames

TOL_HOST = 2.0 ** -13          # device <-> fp64 definition, and definition <-> HF
TOL_HF = 2.0 ** -12            # device <-> HF

SMALL = LogMelConfig(chunk_length=2)          # n_samples 32000, cap 200
SR = SMALL.sampling_rate

# fewer samples than the reflect pad / than one window, hop and window boundaries, a non-multiple of the hop, the clip that ends
# exactly at n_samples (tail reflect) and its neighbours, truncation
LENGTHS = (1, 159, 160, 161, 199, 200, 201, 399, 400, 401, 1000, 31999, 32000, 32001, 40000)
SIGNALS = ("noise", "tone440", "tone1k", "chirp", "bursts", "zeros", "clipped")


@functools.lru_cache(maxsize=None)
def clip(signal: str, L: int) -> np.ndarray:
    """fp32 [L], fixed seed per (signal, L); treat as read-only (cached)."""
    g = np.random.default_rng(1000 * SIGNALS.index(signal) + L % 997)
    t = np.arange(L, dtype=np.float64) / SR
    if signal == "noise":
        x = 0.1 * g.standard_normal(L)
    elif signal == "tone440":                  # most of [mel, cap] lies on the clip_max - 8 clamp
        x = 0.5 * np.sin(2 * math.pi * 440.0 * t) + 1e-4 * g.standard_normal(L)
    elif signal == "tone1k":
        x = 0.5 * np.sin(2 * math.pi * 1000.0 * t)
    elif signal == "chirp":                    # 100 -> 7300 Hz, linear over the clip
        T = max(L, 2) / SR
        x = 0.5 * np.sin(2 * math.pi * (100.0 * t + (7300.0 - 100.0) * t * t / (2 * T)))
    elif signal == "bursts":                   # 50 ms of noise, 50 ms of exact zeros
        x = 0.2 * g.standard_normal(L) * ((np.arange(L) // 800) % 2 == 0)
    elif signal == "zeros":
        x = np.zeros(L)
    elif signal == "clipped":
        x = np.clip(1.5 * g.standard_normal(L), -1.0, 1.0)
    else:
        raise KeyError(signal)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def hf_extractor(chunk_length: int = 2):
    from transformers import WhisperFeatureExtractor
    return WhisperFeatureExtractor(feature_size=128, n_fft=400, hop_length=160, chunk_length=chunk_length)


def hf_call(clips, chunk_length: int = 2):
    """the processor's call -> (input_features fp32 [B, 128, cap], attention_mask int32 [B, cap])"""
    out = hf_extractor(chunk_length)([np.asarray(c) for c in clips], sampling_rate=SR, padding="max_length", return_attention_mask=True,
                                     return_tensors="pt")
    return out["input_features"], out["attention_mask"]


@functools.lru_cache(maxsize=None)
def reference(signal: str, L: int):
    """(definition fp64 [128, 200], HF features fp32 [128, 200], HF mask int32 [200], nv); computed once per case, read-only."""
    x = clip(signal, L)
    f, m = hf_call([x])
    return logmel_host(x[:SMALL.n_samples], SMALL), f[0], m[0], valid_frames(L, SMALL)

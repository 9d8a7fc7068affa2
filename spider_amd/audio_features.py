"""Whisper log-mel features on the device: the audio input side of Qwen2.5-Omni. `Qwen2_5OmniProcessor` hands every clip to
`transformers.WhisperFeatureExtractor` with padding="max_length": the clip is padded to 300 s, run through a host STFT of 30,000
frames and copied to the device as a 15 MB tensor of which the thinker keeps the valid frames. Here the waveform goes to the device
as it is and `ops.logmel` (csrc/audio_features.hip) computes the frames that hold signal.

The feature, for one clip zero-padded to n_samples (`logmel_host` states it in fp64; it is
WhisperFeatureExtractor._torch_extract_fbank_features):
    1. reflect-pad n_fft // 2 on both sides             5. mel projection, Slaney scale + Slaney norm, 0 ... 8000 Hz
    2. frames of n_fft at hop_length, periodic Hann     6. log10(max(., 1e-10))
    3. power |X_k|^2, k = 0 ... n_fft / 2               7. max(., clip_max - 8), clip_max over the clip's whole [mel, cap] array
    4. drop the last frame                              8. (. + 4) / 4
nv = ceil(L / hop_length) frames are valid (the attention mask HF returns). The frames behind them whose window still reaches the
clip hold real values and count in clip_max; every frame whose window holds only padding holds the floor value
(max(clip_max - 8, -10) + 4) / 4. An all-zero clip is -1.5 everywhere.

    LogMelEngine                        clips -> (input_features [B, mel, cap] fp32, attention_mask [B, cap] int32, frame counts)
    DeviceWhisperFeatureExtractor       drop-in for `processor.feature_extractor` (SpiderFreeInfer(device_audio_features=True))
    QwenOmniThinker(audio_waveforms=)   the same features without the processor; frame counts come from the host-known lengths
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import ops

MAX_N_FFT, MAX_MEL = 512, 128          # what spider_logmel_f32 covers (csrc/audio_features.hip)


# ------------------------------------------------------------------------------------------ preprocessor_config.json
@dataclass(frozen=True)
class LogMelConfig:
    """Qwen2.5-Omni's values are the defaults (preprocessor_config.json of the checkpoint: 128 mel bins, 400 / 160, 16 kHz, 300 s)."""
    feature_size: int = 128
    n_fft: int = 400
    hop_length: int = 160
    sampling_rate: int = 16000
    chunk_length: int = 300
    n_samples: Optional[int] = None          # chunk_length * sampling_rate unless the config names it
    max_frequency: float = 8000.0            # WhisperFeatureExtractor's constant

    def __post_init__(self):
        if self.n_samples is None:
            object.__setattr__(self, "n_samples", int(self.chunk_length) * int(self.sampling_rate))
        if self.n_fft % 2 or not 2 <= self.n_fft <= MAX_N_FFT:
            raise NotImplementedError(f"preprocessor_config: n_fft={self.n_fft} is not implemented (even, at most {MAX_N_FFT})")
        if not 1 <= self.feature_size <= MAX_MEL:
            raise NotImplementedError(f"preprocessor_config: feature_size={self.feature_size} is not implemented (at most {MAX_MEL})")
        if not 1 <= self.hop_length <= self.n_fft:
            raise NotImplementedError(f"preprocessor_config: hop_length={self.hop_length} is not implemented (1 ... n_fft)")
        if self.n_samples < max(self.hop_length, self.n_fft // 2 + 1):
            raise NotImplementedError(f"preprocessor_config: n_samples={self.n_samples} is shorter than one hop / the reflect pad")

    @property
    def nb_max_frames(self) -> int:          # cap: frames of a full clip after the last one is dropped
        return self.n_samples // self.hop_length

    @property
    def n_bins(self) -> int:
        return self.n_fft // 2 + 1

    @classmethod
    def from_preprocessor_config(cls, cfg: Union[dict, str, None] = None) -> "LogMelConfig":
        """A WhisperFeatureExtractor config dict, or the path of a preprocessor_config.json / of the directory that holds it.
        Settings the device extractor does not implement raise NotImplementedError naming the key."""
        if isinstance(cfg, (str, os.PathLike)):
            p = os.fspath(cfg)
            if os.path.isdir(p):
                p = os.path.join(p, "preprocessor_config.json")
            cfg = json.load(open(p))
        c = dict(cfg or {})
        if c.get("dither", 0.0) != 0.0:
            raise NotImplementedError(f"preprocessor_config: dither={c['dither']} is not implemented (only 0.0)")
        if c.get("do_normalize", False):
            raise NotImplementedError("preprocessor_config: do_normalize=true is not implemented")
        if c.get("padding_value", 0.0) != 0.0:
            raise NotImplementedError(f"preprocessor_config: padding_value={c['padding_value']} is not implemented (only 0.0)")
        d = cls()
        sr = int(c.get("sampling_rate", d.sampling_rate))
        chunk = int(c.get("chunk_length", d.chunk_length))
        n_samples = int(c["n_samples"]) if c.get("n_samples") is not None else chunk * sr
        out = cls(feature_size=int(c.get("feature_size", d.feature_size)), n_fft=int(c.get("n_fft", d.n_fft)),
                  hop_length=int(c.get("hop_length", d.hop_length)), sampling_rate=sr, chunk_length=chunk, n_samples=n_samples)
        if c.get("nb_max_frames") is not None and int(c["nb_max_frames"]) != out.nb_max_frames:
            raise NotImplementedError(f"preprocessor_config: nb_max_frames={c['nb_max_frames']} is not n_samples // hop_length "
                                      f"= {out.nb_max_frames}")
        return out


# ------------------------------------------------------------------------------------------ the definition (host, fp64)
def _hz_to_mel_slaney(f):
    f = np.asarray(f, dtype=np.float64)
    mel = 3.0 * f / 200.0
    logstep = 27.0 / np.log(6.4)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * logstep, mel)


def _mel_to_hz_slaney(m):
    m = np.asarray(m, dtype=np.float64)
    logstep = np.log(6.4) / 27.0
    return np.where(m >= 15.0, 1000.0 * np.exp(logstep * (m - 15.0)), 200.0 * m / 3.0)


def mel_filter_bank_slaney(n_bins: int = 201, n_mel: int = 128, min_frequency: float = 0.0, max_frequency: float = 8000.0,
                           sampling_rate: int = 16000) -> np.ndarray:
    """Triangular filters on the Slaney mel scale (linear below 1 kHz, logarithmic above), each scaled by 2 / (its band's width in
    Hz) -> fp64 [n_bins, n_mel]. n_mel + 2 edge frequencies are spaced evenly in mel between the two limits; bin k lies at
    k (sampling_rate // 2) / (n_bins - 1) Hz; filter m rises from edge m to edge m + 1 and falls to edge m + 2."""
    edges = _mel_to_hz_slaney(np.linspace(_hz_to_mel_slaney(min_frequency), _hz_to_mel_slaney(max_frequency), n_mel + 2))
    bins = np.linspace(0, sampling_rate // 2, n_bins)
    width = np.diff(edges)
    slopes = edges[None, :] - bins[:, None]
    down = -slopes[:, :-2] / width[:-1]
    up = slopes[:, 2:] / width[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    return fb * (2.0 / (edges[2:n_mel + 2] - edges[:n_mel]))[None, :]


def valid_frames(length: int, cfg: LogMelConfig) -> int:
    """nv: the ones of HF's attention mask for a clip of `length` samples (truncated to n_samples)"""
    return -(-min(int(length), cfg.n_samples) // cfg.hop_length)


def logmel_host(wave, cfg: LogMelConfig = LogMelConfig()) -> torch.Tensor:
    """The definition: one clip (1-D, at most n_samples; shorter clips are zero-padded) -> fp64 [feature_size, nb_max_frames]."""
    x = torch.as_tensor(np.asarray(wave, dtype=np.float64)).flatten()
    if x.numel() > cfg.n_samples:
        raise ValueError(f"logmel_host: the clip has {x.numel()} samples, more than n_samples = {cfg.n_samples}")
    x = torch.nn.functional.pad(x, (0, cfg.n_samples - x.numel()))
    half = cfg.n_fft // 2
    y = torch.cat([x[1:half + 1].flip(0), x, x[-half - 1:-1].flip(0)])                       # 1. reflect pad
    n = torch.arange(cfg.n_fft, dtype=torch.float64)
    window = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / cfg.n_fft)                           # periodic Hann
    frames = y.unfold(0, cfg.n_fft, cfg.hop_length)[:cfg.nb_max_frames]                      # 2. + 4. the last frame is dropped
    k = torch.arange(cfg.n_bins, dtype=torch.float64)
    ang = 2.0 * math.pi * torch.outer(n, k) / cfg.n_fft
    out = torch.empty(cfg.feature_size, cfg.nb_max_frames, dtype=torch.float64)
    fb = torch.from_numpy(mel_filter_bank_slaney(cfg.n_bins, cfg.feature_size, 0.0, cfg.max_frequency, cfg.sampling_rate))
    wc, ws = window[:, None] * ang.cos(), window[:, None] * ang.sin()
    for s in range(0, cfg.nb_max_frames, 4096):
        f = frames[s:s + 4096]
        power = (f @ wc) ** 2 + (f @ ws) ** 2                                               # 3.
        out[:, s:s + 4096] = (power @ fb).T                                                 # 5.
    out = out.clamp_min(1e-10).log10()                                                       # 6.
    out = torch.maximum(out, out.max() - 8.0)                                                # 7.
    return (out + 4.0) / 4.0                                                                 # 8.


# ------------------------------------------------------------------------------------------ device tables
_TABLES = {}


def logmel_tables(cfg: LogMelConfig, device) -> dict:
    """What ops.logmel reads, built once per (config, device) on the host in fp64 and rounded to fp32:
    `table` [n_fft, 64 G], G = ceil(n_bins / 32): for bin group g, columns [64 g, 64 g + 32) hold w[n] cos(2 pi n k / n_fft) and
    [64 g + 32, 64 g + 64) hold w[n] sin(2 pi n k / n_fft) of the bins k = 32 g ... 32 g + 31 (w = periodic Hann; zero columns beyond
    n_fft / 2), so that one lane of the kernel holds a bin's real and imaginary part; `fb` [n_bins, feature_size]."""
    device = torch.device(device)
    key = (cfg, device.type, device.index)
    t = _TABLES.get(key)
    if t is None:
        n = np.arange(cfg.n_fft, dtype=np.float64)
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / cfg.n_fft)
        G = (cfg.n_bins + 31) // 32
        k = np.arange(32 * G)
        # the angle is reduced exactly in integers before it is scaled: n k mod n_fft
        ang = 2.0 * np.pi * ((n[:, None].astype(np.int64) * k[None, :]) % cfg.n_fft) / cfg.n_fft
        live = (k < cfg.n_bins)[None, :]
        cos = np.where(live, w[:, None] * np.cos(ang), 0.0).reshape(cfg.n_fft, G, 32)
        sin = np.where(live, w[:, None] * np.sin(ang), 0.0).reshape(cfg.n_fft, G, 32)
        table = np.concatenate([cos, sin], axis=2).reshape(cfg.n_fft, 64 * G).astype(np.float32)
        fb = mel_filter_bank_slaney(cfg.n_bins, cfg.feature_size, 0.0, cfg.max_frequency, cfg.sampling_rate).astype(np.float32)
        t = dict(table=torch.from_numpy(table).contiguous().to(device), fb=torch.from_numpy(fb).contiguous().to(device),
                 n_fft=cfg.n_fft, hop=cfg.hop_length, mel=cfg.feature_size, n_samples=cfg.n_samples, cap=cfg.nb_max_frames)
        _TABLES[key] = t
    return t


# ------------------------------------------------------------------------------------------ engine
def _clip_to_f32(a) -> np.ndarray:
    """one clip as HF takes it: a 1-D array / tensor / list of floats, float64 cast to fp32"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 2 and 1 in a.shape:
        a = a.reshape(-1)
    if a.ndim != 1:
        raise ValueError("Only mono-channel audio is supported: every clip must be one-dimensional")
    return a


class LogMelEngine:
    def __init__(self, cfg: LogMelConfig = LogMelConfig(), device="cuda:0"):
        self.cfg, self.device = cfg, torch.device(device)
        self.tables = logmel_tables(cfg, self.device)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0"):
        """a checkpoint directory: reads its preprocessor_config.json"""
        return cls(LogMelConfig.from_preprocessor_config(path), device)

    def check_sampling_rate(self, sampling_rate: Optional[int], who: str = "LogMelEngine") -> None:
        if sampling_rate is not None and sampling_rate != self.cfg.sampling_rate:
            raise ValueError(
                f"The model corresponding to this feature extractor: {who} was trained using a sampling rate of "
                f"{self.cfg.sampling_rate}. Please make sure that the provided `raw_speech` input was sampled with "
                f"{self.cfg.sampling_rate} and not {sampling_rate}.")

    def pack(self, audios: Sequence):
        """clips -> (packed fp32 waveform on the device, meta int32 [2, B] = offsets, lengths on the device, lengths on the host).
        Clips longer than n_samples are truncated as HF truncates. Two host -> device copies, no device -> host read."""
        clips = [_clip_to_f32(a)[:self.cfg.n_samples] for a in audios]
        if not clips:
            raise ValueError("LogMelEngine: no clips")
        lens = [int(c.shape[0]) for c in clips]
        offs = [0]
        for n in lens[:-1]:
            offs.append(offs[-1] + n)
        if offs[-1] + lens[-1] >= 2 ** 31:
            raise ValueError("LogMelEngine: more than 2^31 samples in one batch")
        packed = torch.from_numpy(np.concatenate(clips) if sum(lens) else np.zeros(1, dtype=np.float32))
        meta = torch.tensor([offs, lens], dtype=torch.int32)
        return packed.to(self.device), meta.to(self.device), lens

    @torch.no_grad()
    def __call__(self, audios: Sequence, sampling_rate: Optional[int] = None):
        """audios: list of 1-D float arrays / tensors. -> (input_features [B, mel, cap] fp32 on the device, attention_mask [B, cap]
        int32 on the device, valid frames per clip ceil(L / hop_length): list[int] on the host)."""
        self.check_sampling_rate(sampling_rate)
        with torch.cuda.device(self.device):
            waves, meta, lens = self.pack(audios)
            feats, mask = ops.logmel(waves, lens, self.tables, offsets=meta[0], lengths_dev=meta[1])
        return feats, mask, [valid_frames(n, self.cfg) for n in lens]


# ------------------------------------------------------------------------------------------ drop-in for processor.feature_extractor
class DeviceWhisperFeatureExtractor:
    """Stands where `Qwen2_5OmniProcessor.feature_extractor` stands and answers the call the processor makes,
    `(audio, sampling_rate=16000, padding="max_length", return_attention_mask=True, return_tensors="pt")`, with a BatchFeature whose
    `input_features` [B, mel, cap] fp32 and `attention_mask` [B, cap] int32 lie on the device. Requests HF would serve another way
    (another padding, no truncation, a max_length, normalisation, numpy output) raise NotImplementedError."""
    model_input_names = ["input_features"]

    def __init__(self, cfg: LogMelConfig = LogMelConfig(), device="cuda:0"):
        self.engine = LogMelEngine(cfg, device)
        self.cfg = cfg
        self.feature_size, self.sampling_rate, self.hop_length = cfg.feature_size, cfg.sampling_rate, cfg.hop_length
        self.chunk_length, self.n_fft, self.n_samples, self.nb_max_frames = cfg.chunk_length, cfg.n_fft, cfg.n_samples, cfg.nb_max_frames
        self.padding_value, self.dither, self.return_attention_mask = 0.0, 0.0, False

    @classmethod
    def from_feature_extractor(cls, fe, device="cuda:0"):
        """from a transformers.WhisperFeatureExtractor (its own attributes are the config)"""
        keys = ("feature_size", "n_fft", "hop_length", "sampling_rate", "chunk_length", "n_samples", "nb_max_frames", "dither",
                "do_normalize", "padding_value")
        return cls(LogMelConfig.from_preprocessor_config({k: getattr(fe, k) for k in keys if getattr(fe, k, None) is not None}), device)

    @classmethod
    def from_pretrained(cls, path: str, device="cuda:0"):
        return cls(LogMelConfig.from_preprocessor_config(path), device)

    def __call__(self, raw_speech, truncation: bool = True, pad_to_multiple_of=None, return_tensors=None, return_attention_mask=None,
                 padding="max_length", max_length=None, sampling_rate=None, do_normalize=None, device=None, **kwargs):
        self.engine.check_sampling_rate(sampling_rate, "DeviceWhisperFeatureExtractor")
        if getattr(padding, "value", padding) != "max_length":
            raise NotImplementedError(f"DeviceWhisperFeatureExtractor: padding={padding!r} is not implemented (only 'max_length')")
        if truncation is not True:
            raise NotImplementedError(f"DeviceWhisperFeatureExtractor: truncation={truncation!r} is not implemented (only True)")
        if max_length not in (None, self.n_samples):
            raise NotImplementedError(f"DeviceWhisperFeatureExtractor: max_length={max_length} is not implemented (only n_samples)")
        if pad_to_multiple_of is not None:
            raise NotImplementedError("DeviceWhisperFeatureExtractor: pad_to_multiple_of is not implemented")
        if do_normalize:
            raise NotImplementedError("DeviceWhisperFeatureExtractor: do_normalize is not implemented")
        if getattr(return_tensors, "value", return_tensors) != "pt":
            raise NotImplementedError(f"DeviceWhisperFeatureExtractor: return_tensors={return_tensors!r} is not implemented (only 'pt')")
        batched = (isinstance(raw_speech, np.ndarray) and raw_speech.ndim > 1) or (isinstance(raw_speech, torch.Tensor) and raw_speech.dim() > 1) \
            or (isinstance(raw_speech, (list, tuple)) and len(raw_speech) > 0 and isinstance(raw_speech[0], (np.ndarray, torch.Tensor, tuple, list)))
        clips = list(raw_speech) if batched else [raw_speech]
        feats, mask, _ = self.engine(clips)
        from transformers.feature_extraction_utils import BatchFeature
        out = {"input_features": feats}
        if return_attention_mask:
            out["attention_mask"] = mask
        return BatchFeature(out)


def is_whisper_feature_extractor(fe) -> bool:
    """by class name along the MRO: no import of transformers for a processor that has none"""
    return any(c.__name__ == "WhisperFeatureExtractor" for c in type(fe).__mro__)

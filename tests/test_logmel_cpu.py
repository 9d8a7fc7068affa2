"""CPU: the stated definition of the Whisper log-mel feature (spider_amd/audio_features.py) against transformers -- the filter
bank against transformers.audio_utils.mel_filter_bank, `logmel_host` against WhisperFeatureExtractor on the clips of
logmel_cases.py -- and the config / argument checks of the device extractor that need no device."""
import json
import math

import numpy as np
import pytest
import torch

import logmel_cases as LC
from spider_amd import audio_features as AF


def test_filter_bank_equals_transformers():
    from transformers.audio_utils import mel_filter_bank
    ref = mel_filter_bank(201, 128, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney")
    got = AF.mel_filter_bank_slaney(201, 128, 0.0, 8000.0, 16000)
    assert got.dtype == np.float64 and got.shape == ref.shape == (201, 128)
    assert float(np.abs(got - ref).max()) <= 1e-12
    small = AF.mel_filter_bank_slaney(33, 16, 0.0, 8000.0, 16000)       # another geometry: the tiny audio tower's 16 bins
    assert float(np.abs(small - mel_filter_bank(33, 16, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney")).max()) <= 1e-12


@pytest.mark.parametrize("signal", LC.SIGNALS)
def test_definition_matches_whisper_feature_extractor(signal):
    worst = 0.0
    for L in LC.LENGTHS:
        host, hf, mask, nv = LC.reference(signal, L)
        assert tuple(host.shape) == tuple(hf.shape) == (128, 200) and hf.dtype == torch.float32
        err = float((host - hf.double()).abs().max())
        worst = max(worst, err)
        assert err <= LC.TOL_HOST, f"{signal} L={L}: {err:.3e}"
        assert nv == math.ceil(min(L, 32000) / 160) == int(mask.sum())
        assert torch.equal(mask, (torch.arange(200) < nv).to(mask.dtype))
    print(f"{signal}: max |definition - HF| = {worst:.3e}")


def test_floor_frames_and_all_zero_clip():
    host, _, _, nv = LC.reference("noise", 1000)
    floor = host[:, nv + 2:]
    assert floor.numel() > 0 and bool((floor == floor[0, 0]).all())
    cmax = float(host.max()) * 4.0 - 4.0                          # undo (. + 4) / 4 on the maximum
    assert abs(float(floor[0, 0]) - (max(cmax - 8.0, -10.0) + 4.0) / 4.0) < 1e-12
    assert bool((host[:, nv] != floor[0, 0]).any())                # the frame behind the valid ones still sees signal
    zero = LC.reference("zeros", 400)[0]
    assert bool((zero == -1.5).all())


def test_config_reads_omni_preprocessor_config(tmp_path):
    omni = {"chunk_length": 300, "dither": 0.0, "feature_extractor_type": "WhisperFeatureExtractor", "feature_size": 128,
            "hop_length": 160, "n_fft": 400, "n_samples": 4800000, "nb_max_frames": 30000, "padding_side": "right",
            "padding_value": 0.0, "processor_class": "Qwen2_5OmniProcessor", "return_attention_mask": True, "sampling_rate": 16000,
            "image_mean": [0.48145466, 0.4578275, 0.40821073], "patch_size": 14}
    cfg = AF.LogMelConfig.from_preprocessor_config(omni)
    assert cfg == AF.LogMelConfig() and cfg.n_samples == 4800000 and cfg.nb_max_frames == 30000 and cfg.n_bins == 201
    json.dump(omni, open(tmp_path / "preprocessor_config.json", "w"))
    assert AF.LogMelConfig.from_preprocessor_config(str(tmp_path)) == cfg
    assert AF.LogMelConfig.from_preprocessor_config(str(tmp_path / "preprocessor_config.json")) == cfg
    assert AF.LogMelConfig.from_preprocessor_config({"chunk_length": 2}).nb_max_frames == 200
    for bad, key in (({"dither": 1e-4}, "dither"), ({"do_normalize": True}, "do_normalize"), ({"n_fft": 1024}, "n_fft"),
                     ({"n_fft": 399}, "n_fft"), ({"feature_size": 256}, "feature_size")):
        with pytest.raises(NotImplementedError, match=key):
            AF.LogMelConfig.from_preprocessor_config(dict(omni, **bad))


def test_config_from_a_whisper_feature_extractor_object():
    fe = LC.hf_extractor(2)
    assert AF.is_whisper_feature_extractor(fe) and not AF.is_whisper_feature_extractor(object())
    keys = ("feature_size", "n_fft", "hop_length", "sampling_rate", "chunk_length", "n_samples", "nb_max_frames", "dither")
    assert AF.LogMelConfig.from_preprocessor_config({k: getattr(fe, k) for k in keys}) == LC.SMALL


def test_wrong_sampling_rate_raises_value_error():
    eng = AF.LogMelEngine.__new__(AF.LogMelEngine)               # the check reads the config alone: no device
    eng.cfg = LC.SMALL
    eng.check_sampling_rate(16000)
    eng.check_sampling_rate(None)
    with pytest.raises(ValueError, match="sampling rate of 16000"):
        eng.check_sampling_rate(44100)
    with pytest.raises(ValueError):                               # HF raises the same type for the same call
        LC.hf_extractor(2)([LC.clip("noise", 400)], sampling_rate=44100)


def test_device_tables_layout():
    """the windowed DFT table the kernel streams: cos | sin per group of 32 bins, zero columns beyond n_fft / 2"""
    t = AF.logmel_tables(LC.SMALL, "cpu")
    tab = t["table"].double()
    assert tuple(tab.shape) == (400, 448) and tuple(t["fb"].shape) == (201, 128) and t["cap"] == 200
    n = torch.arange(400, dtype=torch.float64)
    w = 0.5 - 0.5 * torch.cos(2 * math.pi * n / 400)
    for k in (0, 1, 31, 32, 100, 200):
        g, j = divmod(k, 32)
        assert float((tab[:, 64 * g + j] - w * torch.cos(2 * math.pi * n * k / 400)).abs().max()) < 1e-6
        assert float((tab[:, 64 * g + 32 + j] - w * torch.sin(2 * math.pi * n * k / 400)).abs().max()) < 1e-6
    assert bool((tab[:, 64 * 6 + 9:64 * 6 + 32] == 0).all()) and bool((tab[:, 64 * 6 + 32 + 9:] == 0).all())      # bins 201 ... 223


def test_custom_op_registered_with_schema_and_fake_impl():
    import spider_amd.torch_ops as T
    assert T.AUDIO_OP_NAMES == ("logmel",)
    assert torch.ops.spider_hip.logmel.default._schema.name == "spider_hip::logmel"
    assert len(torch.ops.spider_hip.logmel.default._schema.returns) == 2
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        f, m = torch.ops.spider_hip.logmel(e(5000), e(3, dt=torch.int32), e(3, dt=torch.int32), 3000, e(400, 448), e(201, 128), 32000, 160)
        assert tuple(f.shape) == (3, 128, 200) and f.dtype == torch.float32 and tuple(m.shape) == (3, 200) and m.dtype == torch.int32


def test_argument_validation_on_the_host():
    from spider_amd import lib as slib
    lib = slib.load()
    assert lib.spider_logmel_tile_frames() == 32
    one = 16                                                    # any non-null value: validation fails before a launch
    args = lambda **k: [one] * 8 + [k.get(n, d) for n, d in (("B", 1), ("n_samples", 32000), ("n_fft", 400), ("hop", 160), ("mel", 128),
                                                               ("cap", 200), ("ldt", 448), ("max_tiles", 1))] + [None]
    for bad, word in ((dict(n_fft=1024, ldt=64 * 17), b"n_fft"), (dict(n_fft=399), b"n_fft"), (dict(mel=129), b"mel"),
                      (dict(hop=401), b"hop_length"), (dict(cap=201), b"cap"), (dict(ldt=416), b"leading dimension"),
                      (dict(max_tiles=8), b"max_tiles"), (dict(n_fft=512, hop=512, ldt=64 * 9, cap=50), b"LDS")):
        assert lib.spider_logmel_f32(*args(**bad)) == -1, bad
        assert word in lib.spider_last_error(), (bad, lib.spider_last_error())
    assert lib.spider_logmel_f32(None, *args()[1:]) == -1 and b"null" in lib.spider_last_error()

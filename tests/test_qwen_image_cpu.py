"""CPU: the host side of the device image path (spider_amd/image_features.py, ops.qwen_smart_resize / qwen_image_tables) against
transformers' Qwen2-VL image processor -- the resize rule over a seeded sweep, the numpy restatement from the tables the kernel reads
against Qwen2VLImageProcessorPil bit for bit on the cases of qwen_image_cases.py -- and the config / input / plumbing checks that
need no device."""
import json
import math

import numpy as np
import pytest
import torch

import qwen_image_cases as QC
from spider_amd import image_features as IF
from spider_amd import ops


def test_smart_resize_equals_transformers_over_a_seeded_sweep():
    from transformers.models.qwen2_vl.image_processing_pil_qwen2_vl import smart_resize
    g = np.random.default_rng(0)
    n_err = 0
    cases = [(int(g.integers(1, 4200)), int(g.integers(1, 4200)), int(g.choice([28, 8, 32])), int(g.choice([3136, 784, 200704, 64])),
              int(g.choice([3136, 12544, 1003520, 12845056]))) for _ in range(1900)]
    cases += [(h, w, 28, 3136, 1003520) for h in (1, 13, 14, 15, 41, 42, 43, 70, 98) for w in (1, 14, 42, 70, 2800, 2814, 8401)]   # .5 ties, ratio 200
    cases += [(1, 200, 28, 3136, 1003520), (1, 201, 28, 3136, 1003520), (5, 1000, 28, 3136, 1003520), (5, 1001, 28, 3136, 1003520)]
    for H, W, f, lo, hi in cases:
        try:
            ref = smart_resize(H, W, f, lo, hi)
        except ValueError as e:
            n_err += 1
            with pytest.raises(ValueError, match="absolute aspect ratio must be smaller than 200") as got:
                ops.qwen_smart_resize(H, W, f, lo, hi)
            assert str(got.value) == str(e)
            continue
        assert ops.qwen_smart_resize(H, W, f, lo, hi) == ref, (H, W, f, lo, hi)
    assert len(cases) >= 1950 and n_err >= 5


@pytest.mark.parametrize("name", QC.NAMES)
def test_restatement_from_the_kernels_tables_equals_the_host_processor(name):
    ref, grid = QC.case_reference(name)
    cfg = QC.case_config(name)
    assert tuple(grid[0].tolist()) == QC.BY_NAME[name][6] and grid.dtype == torch.int64
    assert ref.dtype == torch.float32 and tuple(ref.shape) == (int(grid.prod()), 1176)
    got, g = QC.restate([QC.image(name)], cfg, torch.float32)
    assert torch.equal(g, grid) and torch.equal(got, ref)
    got16, _ = QC.restate([QC.image(name)], cfg, torch.bfloat16)
    assert got16.dtype == torch.bfloat16 and torch.equal(got16, ref.to(torch.bfloat16))
    assert torch.equal(IF.ImagePatchEngine(cfg, "cpu").grid_thw([QC.image(name).shape[:2]]), grid)


def test_lookup_table_ends_and_mixed_batch_descriptors():
    names = QC.groups()[(QC.LO, QC.HI)]
    cfg = QC.config()
    t = ops.qwen_image_tables([QC.image(n).shape[:2] for n in names], cfg, "cpu")
    lut = t["lut"][torch.float32].view(torch.float32)
    assert tuple(lut.shape) == (3, 256) and float(lut.min()) == float(lut[0, 0]) and float(lut.max()) == float(lut[2, 255])
    assert abs(float(lut[0, 0]) + 1.7922626) < 1e-6 and abs(float(lut[2, 255]) - 2.1458969) < 1e-6
    desc = t["desc"]
    assert tuple(desc.shape) == (len(names), ops.QWEN_DESC_WORDS) and desc.dtype == torch.int64
    rows = [int(np.prod(QC.BY_NAME[n][6])) for n in names]
    assert desc[:, 11].tolist() == [sum(rows[:i]) for i in range(len(names))] and t["rows"] == sum(rows)     # row offsets follow grid_thw
    assert desc[:, 0].tolist() == [sum(QC.image(n).size for n in names[:i]) for i in range(len(names))]
    assert all(int(v) % 4 == 0 for v in desc[:, 12]) and t["grid"] == [QC.BY_NAME[n][6] for n in names]
    assert ops.qwen_image_tables([QC.image(n).shape[:2] for n in names], cfg, "cpu") is t                 # cached per (sizes, cfg, device)
    # identity passes are one tap of 2^22; 600 -> 28 (21.4x: beta = 10.7 floors to one merge block) has 2 ceil(2 * 21.4) + 1 = 87 taps
    d = ops.qwen_image_tables([(56, 84)], cfg, "cpu")["desc"][0]
    assert int(d[7]) == 1 and int(d[10]) == 1
    d = ops.qwen_image_tables([(600, 600)], QC.case_config("downscale_87_taps"), "cpu")["desc"][0]
    assert int(d[7]) == 87 and int(d[10]) == 87 and int(d[13]) == 0 and int(d[14]) == 600


OMNI = {"chunk_length": 300, "feature_extractor_type": "WhisperFeatureExtractor", "feature_size": 128, "hop_length": 160,
        "image_mean": [0.48145466, 0.4578275, 0.40821073], "image_processor_type": "Qwen2VLImageProcessor",
        "image_std": [0.26862954, 0.26130258, 0.27577711], "max_pixels": 12845056, "merge_size": 2, "min_pixels": 3136, "n_fft": 400,
        "patch_size": 14, "processor_class": "Qwen2_5OmniProcessor", "temporal_patch_size": 2, "do_resize": True, "do_rescale": True,
        "do_normalize": True, "do_convert_rgb": True, "resample": 3, "rescale_factor": 0.00392156862745098, "sampling_rate": 16000}


def test_config_reads_both_spellings_and_names_what_it_does_not_do(tmp_path):
    cfg = IF.ImagePatchConfig.from_preprocessor_config(OMNI)
    assert cfg == IF.ImagePatchConfig(max_pixels=12845056) and cfg.factor == 28 and cfg.patch_dim == 1176
    assert cfg.size == {"shortest_edge": 3136, "longest_edge": 12845056}
    sized = {k: v for k, v in OMNI.items() if k not in ("min_pixels", "max_pixels")}
    sized["size"] = {"shortest_edge": 3136, "longest_edge": 12845056}
    assert IF.ImagePatchConfig.from_preprocessor_config(sized) == cfg
    assert IF.ImagePatchConfig.from_preprocessor_config(dict(sized, max_pixels=12544)).max_pixels == 12544      # the pixel keys win
    json.dump(OMNI, open(tmp_path / "preprocessor_config.json", "w"))
    assert IF.ImagePatchConfig.from_pretrained(str(tmp_path)) == cfg
    assert IF.ImagePatchConfig.from_pretrained(str(tmp_path / "preprocessor_config.json")) == cfg
    assert IF.ImagePatchEngine.from_pretrained(str(tmp_path), "cpu").cfg == cfg
    for bad, key in (({"resample": 2}, "resample"), ({"do_resize": False}, "do_resize"), ({"do_rescale": False}, "do_rescale"),
                     ({"do_normalize": False}, "do_normalize"), ({"rescale_factor": 1 / 256}, "rescale_factor"),
                     ({"image_mean": [0.5]}, "image_mean"), ({"image_std": 0.5}, "image_std"), ({"image_std": [0.5] * 4}, "image_std"),
                     ({"size": {"height": 224, "width": 224}, "min_pixels": None, "max_pixels": None}, "size"),
                     ({"do_convert_rgb": False}, "do_convert_rgb"), ({"do_pad": True}, "do_pad")):
        with pytest.raises(NotImplementedError, match=key):
            IF.ImagePatchConfig.from_preprocessor_config(dict(OMNI, **bad))


def test_config_from_a_host_image_processor_object():
    ip = QC.hf_processor(QC.config(3136, 12544))
    assert IF.is_qwen2vl_image_processor(ip) and not IF.is_qwen2vl_image_processor(object())
    d = IF.DeviceQwen2VLImageProcessor.from_image_processor(ip, "cpu")          # the constructor touches no device
    assert d.cfg == QC.config(3136, 12544)
    assert d.model_input_names == ["pixel_values", "image_grid_thw"] == list(ip.model_input_names)
    assert (d.merge_size, d.patch_size, d.temporal_patch_size, d.min_pixels, d.max_pixels) == (2, 14, 2, 3136, 12544)
    assert d.size == {"shortest_edge": 3136, "longest_edge": 12544} == {k: ip.size[k] for k in ("shortest_edge", "longest_edge")}
    assert d.get_number_of_image_patches(300, 500) == ip.get_number_of_image_patches(300, 500) == 60
    kw = {"min_pixels": 3136, "max_pixels": 1003520}
    assert d.get_number_of_image_patches(300, 500, kw) == ip.get_number_of_image_patches(300, 500, kw)
    # requests the device path does not serve are refused before any device work
    img = QC.image("both_axes_identity")
    for bad in (dict(do_resize=False), dict(resample=2), dict(do_normalize=False), dict(image_mean=[0.5, 0.5, 0.5]), dict(patch_size=16),
                dict(return_tensors="np"), dict(videos=[img]), dict(data_format="channels_last"), dict(do_center_crop=True)):
        with pytest.raises(NotImplementedError):
            d(images=[img], **dict(dict(return_tensors="pt"), **bad))
    with pytest.raises(ValueError, match="together"):
        d(images=[img], max_pixels=12544)


def test_symbol_is_exported_and_listed():
    import ctypes
    from spider_amd import lib as slib
    assert "spider_qwen_image_patches" in slib.SIGNATURES and len(slib.SIGNATURES["spider_qwen_image_patches"][1]) == 14
    assert hasattr(ctypes.CDLL(slib.LIB_PATH), "spider_qwen_image_patches")
    lib = slib.load()
    assert lib.spider_abi_version() == 4
    one = 16                                                     # any non-null value: validation fails before a launch
    args = lambda **k: [one] * 6 + [k.get(n, d) for n, d in (("n", 1), ("patch", 14), ("merge", 2), ("temporal", 2), ("h_items", 64),
                                                               ("tiles", 4), ("f32", 0))] + [None]
    for bad, word in ((dict(n=0), b"images"), (dict(patch=15), b"multiples of 4"), (dict(patch=6, temporal=1, merge=2), b"16 bytes"),
                      (dict(f32=2), b"format"), (dict(tiles=0), b"empty grid"), (dict(patch=64, merge=8), b"LDS")):
        assert lib.spider_qwen_image_patches(*args(**bad)) == -1, bad
        assert word in lib.spider_last_error(), (bad, lib.spider_last_error())
    assert lib.spider_qwen_image_patches(None, *args()[1:]) == -1 and b"null" in lib.spider_last_error()


def test_custom_op_registered_with_schema_and_fake_impl():
    import spider_amd.torch_ops as T
    assert T.IMAGE_OP_NAMES == ("qwen_image_patches",)
    assert torch.ops.spider_hip.qwen_image_patches.default._schema.name == "spider_hip::qwen_image_patches"
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *s, dt: torch.empty(*s, dtype=dt, device="cuda")
        a = (e(56 * 84 * 3, dt=torch.uint8), e(1, 16, dt=torch.int64), e(500, dt=torch.int32), e(3, 256, dt=torch.int32), 24, 14, 2, 2,
             3 * 56 * 84, 56 * 21, 6)
        y = torch.ops.spider_hip.qwen_image_patches(*a, False)
        assert tuple(y.shape) == (24, 1176) and y.dtype == torch.bfloat16
        y = torch.ops.spider_hip.qwen_image_patches(*a, True)
        assert tuple(y.shape) == (24, 1176) and y.dtype == torch.float32


def test_input_kinds_are_accepted_or_refused():
    from PIL import Image
    a = QC.image("min_pixels_ceil_upscale")                       # [37, 53, 3]
    rgb = Image.fromarray(a)
    assert np.array_equal(IF._to_hwc_u8(rgb), a)
    for mode in ("L", "RGBA", "P", "CMYK"):
        im = rgb.convert(mode)
        got = IF._to_hwc_u8(im)
        assert got.dtype == np.uint8 and np.array_equal(got, np.asarray(im.convert("RGB"))), mode      # what the host processor does
    assert np.array_equal(IF._to_hwc_u8(torch.from_numpy(a.copy()).permute(2, 0, 1)), a)              # torch CHW
    assert np.array_equal(IF._to_hwc_u8(torch.from_numpy(a.copy())), a)                               # torch HWC
    assert np.array_equal(IF._to_hwc_u8(np.ascontiguousarray(a.transpose(2, 0, 1))), a)               # numpy CHW
    assert IF.image_sizes([rgb, a, torch.from_numpy(a.copy()).permute(2, 0, 1)]) == ((37, 53),) * 3
    with pytest.raises(TypeError, match="uint8"):
        IF._to_hwc_u8(a.astype(np.float32) / 255)
    with pytest.raises(TypeError, match="uint8"):
        IF._to_hwc_u8(torch.from_numpy(a.copy()).float())
    with pytest.raises(ValueError, match="three dimensions"):
        IF._to_hwc_u8(a[None])                                    # a 4-D batch
    with pytest.raises(ValueError, match="three dimensions"):
        IF._to_hwc_u8(a[:, :, 0])
    with pytest.raises(ValueError, match="three channels"):
        IF._to_hwc_u8(np.zeros((8, 8, 4), dtype=np.uint8))
    with pytest.raises(TypeError, match="PIL image"):
        IF._to_hwc_u8("photo.png")
    with pytest.raises(ValueError, match="aspect ratio"):
        IF.ImagePatchEngine(QC.config(), "cpu").grid_thw([(1, 300)])


def test_thinker_and_spider_free_keywords_exist():
    import inspect
    from spider_amd.qwen_omni import QwenOmniThinker
    from spider_amd.spider_free import SpiderFreeInfer
    assert inspect.signature(QwenOmniThinker.prepare_inputs).parameters["images"].default is None
    assert inspect.signature(QwenOmniThinker.would_capture).parameters["images"].default is None
    assert inspect.signature(SpiderFreeInfer.__init__).parameters["device_image_features"].default is False

"""GPU: Qwen2-VL image patch rows on the device (csrc/image_features.hip through ops.qwen_image_patches, ImagePatchEngine, the
image-processor drop-in, QwenOmniThinker(images=), SpiderFreeInfer(device_image_features=True)) against transformers'
Qwen2VLImageProcessorPil. Images, case table and references: qwen_image_cases.py.

Every comparison is torch.equal: Pillow's 8-bit resampling is integer arithmetic and the normalised value comes from a 256-entry table
per channel that numpy fills as the host processor computes it, so there is no tolerance to state."""
import numpy as np
import pytest
import torch

import qwen_image_cases as QC
from oracle import qwen_towers as oq

pytestmark = pytest.mark.gpu


def _engine(dev, cfg=None, **kw):
    from spider_amd.image_features import ImagePatchEngine
    return ImagePatchEngine(cfg or QC.config(), dev, **kw)


@pytest.mark.parametrize("name", QC.NAMES)
def test_each_case_equals_the_host_processor_bit_for_bit(dev, name):
    ref, grid = QC.case_reference(name)
    eng = _engine(dev, QC.case_config(name))
    px, g = eng([QC.image(name)])
    assert px.is_cuda and px.dtype == torch.bfloat16 and tuple(px.shape) == tuple(ref.shape)
    assert g.dtype == torch.int64 and not g.is_cuda and torch.equal(g, grid) and tuple(g[0].tolist()) == QC.BY_NAME[name][6]
    assert torch.equal(px.cpu(), ref.to(torch.bfloat16)), f"{name}: bf16 rows differ from the host processor's"
    px32, g32 = eng([QC.image(name)], dtype=torch.float32)
    assert px32.dtype == torch.float32 and torch.equal(g32, grid)
    assert torch.equal(px32.cpu(), ref), f"{name}: fp32 rows differ from the host processor's"


@pytest.mark.parametrize("bounds", sorted(QC.groups()))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_mixed_sizes_in_one_packed_batch(dev, bounds, dtype):
    """the rows of the table that share one configuration as ONE call: each image's rows are the bits it gives alone (and the host's),
    the row offsets follow image_grid_thw; an `out=` buffer filled with NaN holds none afterwards"""
    names = QC.groups()[bounds]
    cfg = QC.config(*bounds)
    eng = _engine(dev, cfg)
    imgs = [QC.image(n) for n in names]
    t = eng.tables([a.shape[:2] for a in imgs])
    out = torch.full((t["rows"], t["cols"]), float("nan"), dtype=dtype, device=dev)
    px, grid = eng(imgs, dtype=dtype, out=out)
    assert px.data_ptr() == out.data_ptr() and not bool(torch.isnan(out).any()), "an element of out was not written"
    ref_all, grid_all = QC.reference(imgs, cfg)
    assert torch.equal(grid, grid_all) and torch.equal(px.cpu(), ref_all.to(dtype))
    row = 0
    for i, n in enumerate(names):
        rows = int(grid[i].prod())
        assert tuple(grid[i].tolist()) == QC.BY_NAME[n][6]
        alone, _ = eng([imgs[i]], dtype=dtype)
        assert torch.equal(px[row:row + rows], alone), f"{n}: rows in the batch differ from the rows it gives alone"
        assert torch.equal(alone.cpu(), QC.case_reference(n)[0].to(dtype))
        row += rows
    assert row == px.shape[0]


def test_more_tiles_than_blocks_and_a_tile_count_no_multiple_of_the_grid(dev):
    """1403 x 1703 -> 1400 x 1708: 50 x 61 = 3050 merge blocks and a horizontal pass of 1403 x 427 = 599,081 items, both beyond the 2048
    blocks either launch is capped at, so both grid-stride loops take a second trip that is not a full one; against the host
    processor (about 0.2 s there) under Qwen2.5-Omni's max_pixels"""
    g = np.random.default_rng(7)
    img = g.integers(0, 256, (1403, 1703, 3), dtype=np.uint8)
    cfg = QC.config(QC.LO, 12845056)
    ref, grid = QC.reference([img], cfg)
    assert grid.tolist() == [[1, 100, 122]]
    px, g2 = _engine(dev, cfg)([img])
    assert torch.equal(g2, grid) and torch.equal(px.cpu(), ref.to(torch.bfloat16))


def test_input_kinds_give_identical_bits(dev):
    from PIL import Image
    a = QC.image("min_pixels_ceil_upscale")
    eng = _engine(dev)
    base, grid = eng([a])
    ref = QC.case_reference("min_pixels_ceil_upscale")[0].to(torch.bfloat16)
    assert torch.equal(base.cpu(), ref)
    chw = torch.from_numpy(a.copy()).permute(2, 0, 1)
    kinds = {"PIL": Image.fromarray(a), "numpy HWC": a, "torch CHW host": chw, "torch CHW host contiguous": chw.contiguous(),
             "torch HWC host": torch.from_numpy(a.copy()), "torch CHW device": chw.to(dev), "torch HWC device": torch.from_numpy(a.copy()).to(dev)}
    for what, img in kinds.items():
        px, g = eng([img])
        assert torch.equal(px, base) and torch.equal(g, grid), what
    assert torch.equal(eng(a)[0], base)                                        # one image, not a list
    px, g = eng([kinds["torch CHW device"], a])                                # device and host images in one call
    assert torch.equal(px[:24], base) and torch.equal(px[24:], base)
    for mode in ("L", "RGBA", "P"):                                            # converted with .convert("RGB") on the host, as the host does
        im = Image.fromarray(a).convert(mode)
        got = eng([im])[0].cpu()
        assert torch.equal(got, QC.reference([im], QC.config())[0].to(torch.bfloat16)), mode
    with pytest.raises(TypeError, match="uint8"):
        eng([a.astype(np.float32)])
    with pytest.raises(ValueError, match="three dimensions"):
        eng([a[None]])


def test_graph_replay_equals_eager_and_a_second_call_builds_no_table(dev):
    from spider_amd import ops
    eng = _engine(dev)
    imgs = [QC.image("one_axis_identity"), QC.image("overshoot_clipped")]
    packed, sizes = eng.pack(imgs)
    t = eng.tables(sizes)
    eager = ops.qwen_image_patches(packed, t)
    n_tables = len(ops._QWEN_TABLES)
    out = torch.full_like(eager, float("nan"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            t2 = eng.tables(sizes)                                             # same sizes: the cached tables, nothing is built or copied
            ops.qwen_image_patches(packed, t2, out=out)
    torch.cuda.current_stream().wait_stream(s)
    assert t2 is t and len(ops._QWEN_TABLES) == n_tables
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert torch.equal(eng(imgs)[0], eager) and len(ops._QWEN_TABLES) == n_tables
    ref, _ = QC.reference(imgs, QC.config())
    assert torch.equal(eager.cpu(), ref.to(torch.bfloat16))


def test_torch_op_equals_ops(dev):
    import spider_amd.torch_ops as T
    from spider_amd import ops
    assert T.IMAGE_OP_NAMES == ("qwen_image_patches",) and hasattr(torch.ops.spider_hip, "qwen_image_patches")
    eng = _engine(dev)
    packed, sizes = eng.pack([QC.image("min_pixels_ceil_upscale"), QC.image("both_axes_identity")])
    t = eng.tables(sizes)
    for dt in (torch.bfloat16, torch.float32):
        y = torch.ops.spider_hip.qwen_image_patches(packed, t["desc"], t["tabs"], t["lut"][dt], t["rows"], t["patch"], t["merge"], t["temporal"],
                                                    t["tmp_bytes"], t["max_h_items"], t["max_tiles"], dt == torch.float32)
        assert y.dtype == dt and torch.equal(y, ops.qwen_image_patches(packed, t, dt))


# ---------------------------------------------------------------------------------------------- plumbing
def test_drop_in_answers_the_processors_call_like_the_host_class(dev):
    from spider_amd.image_features import DeviceQwen2VLImageProcessor
    cfg = QC.config()
    ip = QC.hf_processor(cfg)
    dip = DeviceQwen2VLImageProcessor.from_image_processor(ip, dev)
    imgs = [QC.image("max_pixels_floor_downscale"), QC.image("min_pixels_ceil_upscale")]
    got, ref = dip(images=imgs, return_tensors="pt"), ip(images=imgs, return_tensors="pt")
    assert type(got) is type(ref) and set(got.keys()) == set(ref.keys()) == {"pixel_values", "image_grid_thw"}
    assert got["pixel_values"].is_cuda and got["pixel_values"].dtype == torch.bfloat16
    assert not got["image_grid_thw"].is_cuda and got["image_grid_thw"].dtype == torch.int64 == ref["image_grid_thw"].dtype
    assert torch.equal(got["image_grid_thw"], ref["image_grid_thw"])
    assert torch.equal(got["pixel_values"].cpu(), ref["pixel_values"].to(torch.bfloat16))
    f32 = dip(images=imgs, return_tensors="pt", dtype=torch.float32)
    assert torch.equal(f32["pixel_values"].cpu(), ref["pixel_values"])
    # per-call bounds, as the host class honours them: both pixel bounds, or size
    kw = dict(min_pixels=3136, max_pixels=12544)
    got, ref = dip(images=imgs, return_tensors="pt", **kw), ip(images=imgs, return_tensors="pt", **kw)
    assert ref["image_grid_thw"].tolist() == [[1, 6, 10], [1, 4, 6]] and torch.equal(got["image_grid_thw"], ref["image_grid_thw"])
    assert torch.equal(got["pixel_values"].cpu(), ref["pixel_values"].to(torch.bfloat16))
    size = {"shortest_edge": 3136, "longest_edge": 12544}
    got2 = dip(images=imgs, return_tensors="pt", size=size)
    assert torch.equal(got2["pixel_values"], got["pixel_values"])
    assert torch.equal(ip(images=imgs, return_tensors="pt", size=size)["pixel_values"], ref["pixel_values"])
    single = dip(images=imgs[1], return_tensors="pt")                           # one image, not a list
    assert torch.equal(single["pixel_values"].cpu(), QC.case_reference("min_pixels_ceil_upscale")[0].to(torch.bfloat16))
    for bad in (dict(do_resize=False), dict(resample=2), dict(return_tensors="np"), dict(videos=imgs)):
        with pytest.raises(NotImplementedError):
            dip(images=imgs, **dict(dict(return_tensors="pt"), **bad))


TOWER_CFG = dict(min_pixels=64, max_pixels=640, patch_size=4)                   # 37 x 53 -> 16 x 24 pixels = grid (1, 4, 6) at patch 4


def _tower_cfg():
    return oq.VisionCfg(depth=2, hidden=64, heads=2, inter=88, in_channels=3, patch=4, temporal_patch=2, merge=2, window=16,
                        out_hidden=256, fullatt=(1,), eps=1e-6)


def test_vision_tower_gives_equal_output_from_device_rows_and_host_pixel_values(dev):
    from spider_amd.image_features import ImagePatchConfig, ImagePatchEngine
    from spider_amd.qwen_omni import VisionTowerConfig, VisionTowerEngine
    cfg = ImagePatchConfig(**TOWER_CFG)
    img = QC.image("min_pixels_ceil_upscale")
    ref_px, ref_grid = QC.reference([img], cfg)
    assert ref_grid.tolist() == [[1, 4, 6]] and tuple(ref_px.shape) == (24, 96)
    px, grid = ImagePatchEngine(cfg, dev)([img])
    assert torch.equal(grid, ref_grid) and torch.equal(px.cpu(), ref_px.to(torch.bfloat16))
    vc = _tower_cfg()
    tower = VisionTowerEngine(VisionTowerConfig(**vc.__dict__), oq.random_weights(oq.vision_param_shapes(vc), seed=18), dev)
    assert torch.equal(tower(px, grid), tower(ref_px, ref_grid))


def _tiny_thinker(dev, seed=17):
    from oracle.llama import LlamaCfg, LlamaOracle
    from spider_amd.image_features import ImagePatchConfig, ImagePatchEngine
    from spider_amd.llm import LlamaEngine, LLMConfig
    from spider_amd.qwen_omni import OmniTokenIds, QwenOmniThinker, VisionTowerConfig, VisionTowerEngine
    lcfg = LlamaCfg(256, 2, 4, 2, 128, 512, 400, 1000000.0, None, 1e-6, True, 512, False, (16, 24, 24))
    lw = LlamaOracle.random_weights(lcfg, seed=seed, std=0.08)
    vc = _tower_cfg()
    tok = OmniTokenIds(image=390, video=391, audio=392, vision_start=393, audio_start=394)
    return QwenOmniThinker(LlamaEngine(LLMConfig(**lcfg.__dict__), lw, dev, max_batch=1, max_len=128),
                           VisionTowerEngine(VisionTowerConfig(**vc.__dict__), oq.random_weights(oq.vision_param_shapes(vc), seed=seed + 1), dev),
                           None, tok, image_patches=ImagePatchEngine(ImagePatchConfig(**TOWER_CFG), dev))


IDS = [5, 6, 393] + [390] * 6 + [396, 8, 9]                                     # 24 patches / merge^2 = 6 image tokens


def test_thinker_images_equal_the_pixel_values_path_bit_for_bit(dev):
    th = _tiny_thinker(dev)
    img = QC.image("min_pixels_ceil_upscale")
    px, grid = QC.reference([img], th.image_patches.cfg)
    ids = torch.tensor([IDS])
    assert th.would_capture(ids, images=[img]) is True and th.would_capture(ids, pixel_values=px, image_grid_thw=grid) is True
    e_ref, p_ref = th.prepare_inputs(ids, torch.ones_like(ids), pixel_values=px, image_grid_thw=grid)
    e, p = th.prepare_inputs(ids, torch.ones_like(ids), images=[img])
    assert torch.equal(e, e_ref) and torch.equal(p, p_ref)
    kw = dict(max_new_tokens=4, eos_token_id=[])
    assert torch.equal(th.generate(ids, None, images=[img], **kw), th.generate(ids, None, pixel_values=px, image_grid_thw=grid, **kw))
    # the tower graph of this grid exists now: the answer comes from the image's size alone and is the pixel_values path's
    assert th.would_capture(ids, images=[img]) == th.would_capture(ids, pixel_values=px, image_grid_thw=grid)
    assert th.would_capture(ids, images=[QC.image("upscale_2x_taps_clipped")]) is True                      # another grid would capture
    with pytest.raises(ValueError, match="not both"):
        th.prepare_inputs(ids, None, images=[img], pixel_values=px, image_grid_thw=grid)
    with pytest.raises(ValueError, match="not both"):
        th.would_capture(ids, images=[img], pixel_values=px, image_grid_thw=grid)
    # built on first use from the tower's geometry and Qwen2.5-Omni's pixel bounds when none is handed in
    th.image_patches = None
    c = th._image_engine().cfg
    assert (c.patch_size, c.merge_size, c.temporal_patch_size, c.min_pixels, c.max_pixels) == (4, 2, 2, 3136, 12845056)


def test_spider_free_infer_with_an_image_in_the_request(dev):
    """SpiderFreeInfer(device_image_features=True): the processor's Qwen2-VL image processor is swapped for the drop-in once, a request
    that carries an image gets the inputs and the tokens of the flag-off instance; with the flag off nothing is swapped."""
    from benchkit.synthetic import SyntheticOmniProcessor
    from spider_amd import SpiderDecoderInfer, SpiderFreeInfer
    from spider_amd.image_features import DeviceQwen2VLImageProcessor, ImagePatchConfig
    th = _tiny_thinker(dev, seed=27)
    img = QC.image("min_pixels_ceil_upscale")
    ids = torch.tensor([IDS])

    class Proc(SyntheticOmniProcessor):          # what Qwen2_5OmniProcessor does with one image: placeholders + its image processor's output
        def __init__(self, **kw):
            super().__init__(**kw)
            self.image_processor = QC.hf_processor(ImagePatchConfig(**TOWER_CFG))

        def __call__(self, text=None, audios=None, images=None, videos=None, return_tensors="pt", padding=True):
            self.prompt_len = ids.shape[1]
            out = {"input_ids": ids, "attention_mask": torch.ones_like(ids)}
            if images is not None:
                out.update(self.image_processor(images=images, return_tensors="pt"))
            return out

    class Pipe:
        def __call__(self, prompt=None, **kw):
            class O:
                images = [f"img:{p}" for p in prompt]
            return O()

    mk = lambda: SpiderDecoderInfer({"model": dict(type="spider_decoder", pipelines={"IMAGE": Pipe()}, device=str(dev))})
    gk = dict(max_new_tokens=6, eos_token_id=[], spk="Chelsie", use_audio_in_video=True)
    mm = lambda messages, use_audio_in_video: (None, [img], None)
    off_proc = Proc(vocab=400)
    host_ip = off_proc.image_processor
    off = SpiderFreeInfer(th, off_proc, mk(), device=dev, generate_kwargs=gk, process_mm_info=mm)
    assert off_proc.image_processor is host_ip
    on_proc = Proc(vocab=400)
    on = SpiderFreeInfer(th, on_proc, mk(), device=dev, generate_kwargs=gk, process_mm_info=mm, device_image_features=True)
    assert isinstance(on_proc.image_processor, DeviceQwen2VLImageProcessor) and on_proc.image_processor.cfg == ImagePatchConfig(**TOWER_CFG)
    msgs = [{"role": "user", "content": [{"type": "image", "image": "x.png"}, {"type": "text", "text": "what do you see?"}]}]
    a, b = on.build_inputs(msgs), off.build_inputs(msgs)
    assert a["pixel_values"].is_cuda and not b["pixel_values"].is_cuda and not a["image_grid_thw"].is_cuda
    assert torch.equal(a["pixel_values"].cpu(), b["pixel_values"].to(torch.bfloat16)) and torch.equal(a["image_grid_thw"], b["image_grid_thw"])
    assert torch.equal(a["input_ids"], b["input_ids"])
    r_on, r_off = on(msgs), off(msgs)
    assert torch.equal(r_on.text_ids, r_off.text_ids), "the request is answered as with the host image processor"
    assert torch.equal(r_on.text_ids, th.generate(ids, None, max_new_tokens=6, eos_token_id=[], images=[img])[0].cpu())
    assert r_on.predictions["IMAGE"] == [f"img:{r_on.predictions_text['IMAGE'][0]}"]
    with pytest.raises(ValueError, match="Qwen2-VL image processor"):
        SpiderFreeInfer(th, SyntheticOmniProcessor(vocab=400), mk(), device=dev, device_image_features=True)

"""CPU: the host restatements of the safety checker's two new device stages and its loader (spider_amd/safety.py).

  * safety_preprocess_host against transformers' CLIPImageProcessor (Pillow backend) fed numpy_to_pil of the same images -- the
    reference's host stages (custom_sd.py:376-384). Bound derived in safety_cases.py: 2 of 8-bit's 256 levels per pixel.
  * safety_decide_host on constructed embeddings: the published rule's flag, adjustment cascade and three-decimal rounding.
  * SafetyCheckerEngine.from_pretrained on a directory in the checker's key layout: every key mapped, no tensor unread."""
import json
import os

import pytest
import torch

import safety_cases as sc


@pytest.mark.parametrize("name", list(sc.PREPROCESS_CASES))
def test_preprocess_host_matches_clip_image_processor(name):
    from spider_amd.safety import safety_preprocess_host
    H, W, size = sc.PREPROCESS_CASES[name]
    ref = sc.reference_pixel_values(name, 2)
    got = safety_preprocess_host(sc.case_images(name, 2), size, size)
    assert got.shape == ref.shape == (2, 3, size, size) and got.dtype == torch.float32
    err = (got - ref).abs()
    levels = err * 255.0 * torch.tensor(sc.CLIP_STD).view(1, 3, 1, 1)
    print(f"MEASURED safety_preprocess_host case={name} differing_share={float((levels > 0.5).float().mean()):.6f} "
          f"max_levels={float(levels.max()):.3f}")
    assert bool((err <= sc.level_bound(2.0) + 1e-6).all()), float(levels.max())      # 1e-6: fp32 rounding of (v/255 - mean)/std


def test_preprocess_geometry_and_taps():
    from spider_amd import ops
    assert ops.clip_resize_geometry(96, 128, 56, 56) == (56, 74, 0, 9)          # long edge int(56 * 128 / 96), left (74 - 56) // 2
    assert ops.clip_resize_geometry(128, 96, 56, 56) == (74, 56, 9, 0)
    assert ops.clip_resize_geometry(512, 512, 224, 224) == (224, 224, 0, 0)
    with pytest.raises(NotImplementedError):
        ops.clip_resize_geometry(64, 64, 56, 60)
    b, t = ops.bicubic_taps(512, 224)
    assert t.shape == (224, 11) and int(b[:, 1].max()) <= 11                     # support 2 * 16/7 = 4.57 -> ksize 2 * 5 + 1
    assert abs(int(t[100].sum()) - (1 << 22)) <= 11                              # taps sum to 1 up to their own rounding
    b, t = ops.bicubic_taps(40, 56)
    assert t.shape[1] == 5 and int(b[:, 1].max()) <= 4                           # an upscale: support exactly 2
    b, t = ops.bicubic_taps(56, 56)                                              # Pillow skips a pass that keeps the size
    assert t.shape == (56, 1) and (t == 1 << 22).all() and (b[:, 0] == torch.arange(56).numpy()).all()
    bw, tw = ops.bicubic_taps(128, 74, 9, 56)                                    # the crop window is a slice of the full table
    bf, tf = ops.bicubic_taps(128, 74)
    assert (bw == bf[9:65]).all() and (tw == tf[9:65]).all()


def test_preprocess_config_rejects_what_the_device_does_not_do():
    from spider_amd.safety import preprocess_config
    d = preprocess_config(None)
    assert d["size"] == 224 and d["crop"] == 224 and d["mean"] == sc.CLIP_MEAN and d["std"] == sc.CLIP_STD
    sd15 = {"crop_size": 224, "do_center_crop": True, "do_convert_rgb": True, "do_normalize": True, "do_resize": True,
            "feature_extractor_type": "CLIPFeatureExtractor", "image_mean": list(sc.CLIP_MEAN), "image_std": list(sc.CLIP_STD),
            "resample": 3, "size": 224}
    assert preprocess_config(sd15) == d
    assert preprocess_config({"size": {"shortest_edge": 56}, "crop_size": {"height": 56, "width": 56}})["crop"] == 56
    for key, val in (("do_resize", False), ("do_center_crop", False), ("do_normalize", False), ("do_rescale", False), ("resample", 2),
                     ("rescale_factor", 1.0), ("size", {"height": 224, "width": 224}), ("crop_size", {"height": 224, "width": 200})):
        with pytest.raises(NotImplementedError, match=key):
            preprocess_config({key: val})


def test_decide_host_rule():
    from spider_amd.safety import safety_decide_host
    cases = sc.decide_cases()
    for name, (emb, concepts, special, thr_c, thr_s, want) in cases.items():
        scores, flags = safety_decide_host(emb, concepts, special, thr_c, thr_s)
        assert flags.tolist() == want, (name, scores)
        assert scores.shape == (emb.shape[0], 3 + 17)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    s = lambda name: safety_decide_host(*cases[name][:5])[0]
    assert float(s("cos1_flags")[0, 3]) == f32(0.5)
    assert float(s("adjust_alone")[0, 3]) == f32(-0.005) and float(s("adjust_cascade")[0, 3]) == f32(0.005)
    # the adjustment starts AFTER the special-care concept that fired and reaches the special-care concepts that follow
    assert float(s("adjust_cascade")[0, 0]) == f32(0.55) and float(s("adjust_cascade")[0, 1]) == f32(0.005)
    assert float(s("special_only")[0, 1]) == f32(0.005) and float(s("special_only")[0, 3]) == f32(-1.99)
    assert float(s("round_down_0004")[0, 3]) == 0.0 and float(s("round_up_0006")[0, 3]) == f32(0.001)
    # half-even on x * 1000: 0.0005 -> 0.000, 0.0015 -> 0.002 (cos 0.5 is exact; the thresholds are fp32 values a hair off the tie,
    # so only the direction that the fp32 value takes is checked against the same arithmetic written out)
    for thr in (0.4995, 0.4985):
        t = cases["cos1_flags"][3].clone(); t[0] = thr
        e = torch.zeros(1, 64); e[0, 0] = 1.0; e[0, 40] = 3.0 ** 0.5          # cos = 0.5 against concept 0
        x = (torch.nn.functional.normalize(e)[0, 0] - t[0]) * torch.tensor(1000.0)
        assert float(safety_decide_host(e, cases["cos1_flags"][1], cases["cos1_flags"][2], t, cases["cos1_flags"][4])[0][0, 3]) == \
            float(torch.round(x) / 1000.0)


def _write_checker_dir(root, cfg, weights, extra=None):
    """`safety_checker/` as diffusers publishes it: the tower under vision_model.vision_model.*, visual_projection, the four buffers,
    the position_ids buffer old exports carry, config.json as a CLIP config"""
    from safetensors.torch import save_file
    os.makedirs(root, exist_ok=True)
    sd = {}
    for k, v in weights.items():
        sd[("vision_model." + k) if k.startswith("vision_model.") else k] = v.to(torch.float16).contiguous()
    sd["vision_model.vision_model.embeddings.position_ids"] = torch.arange(cfg.n_patches + 1)[None]
    sd.update(extra or {})
    save_file(sd, os.path.join(root, "model.safetensors"))
    json.dump({"architectures": ["StableDiffusionSafetyChecker"], "projection_dim": cfg.proj,
               "vision_config": {"hidden_size": cfg.hidden, "intermediate_size": cfg.inter, "num_hidden_layers": cfg.layers,
                                 "num_attention_heads": cfg.heads, "image_size": cfg.image, "patch_size": cfg.patch,
                                 "hidden_act": cfg.act, "layer_norm_eps": cfg.eps},
               "text_config": {"hidden_size": 32}}, open(os.path.join(root, "config.json"), "w"))
    return sd


def test_checker_loader_maps_every_key(tmp_path):
    from transformers import CLIPVisionConfig as HFVisionConfig, CLIPVisionModelWithProjection
    from spider_amd.clip_vision import CLIPVisionConfig, vision_key
    from spider_amd.safety import SafetyCheckerEngine, checker_key, random_checker_weights
    cfg = CLIPVisionConfig(hidden=32, layers=2, heads=2, inter=64, image=28, patch=14, proj=16)
    # the names come from transformers' own module, not from the engine's table
    hf = CLIPVisionModelWithProjection(HFVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                                                      image_size=28, patch_size=14, projection_dim=16))
    w = {k: v.detach().clone() for k, v in hf.state_dict().items() if not k.endswith("position_ids")}
    rw = random_checker_weights(cfg, seed=3)
    assert set(w) == {k for k in rw if k not in ("concept_embeds", "special_care_embeds", "concept_embeds_weights", "special_care_embeds_weights")}
    for k in ("concept_embeds", "special_care_embeds", "concept_embeds_weights", "special_care_embeds_weights"):
        w[k] = rw[k]
    sd = _write_checker_dir(str(tmp_path / "safety_checker"), cfg, w)
    mapped = {k: checker_key(k) for k in sd}
    assert [k for k, v in mapped.items() if v is None] == ["vision_model.vision_model.embeddings.position_ids"]
    assert len(set(v for v in mapped.values() if v)) == len(sd) - 1                       # one engine name per tensor
    assert vision_key("vision_model.embeddings.class_embedding") == "vision_model.embeddings.class_embedding"
    assert vision_key("text_model.embeddings.token_embedding.weight") is None
    eng = SafetyCheckerEngine.from_pretrained(str(tmp_path / "safety_checker"), device="cpu", dtype=torch.float16)
    assert eng.unread == [] and eng.cfg == cfg
    assert eng.pre["size"] == 28 and eng.pre["crop"] == 28
    h = lambda t: t.to(torch.float16)
    assert torch.equal(eng.concept_embeds, h(w["concept_embeds"])) and torch.equal(eng.special_care_embeds, h(w["special_care_embeds"]))
    assert eng.concept_thr.dtype == torch.float32 and torch.equal(eng.concept_thr, h(w["concept_embeds_weights"]).float())
    assert torch.equal(eng.special_thr, h(w["special_care_embeds_weights"]).float())
    v = eng.vision
    assert torch.equal(v.visual_projection, h(w["visual_projection.weight"]))
    assert v.w_patch.shape == (32, 592) and bool((v.w_patch[:, 588:] == 0).all())         # K = 588 padded to 592 with zero columns
    assert torch.equal(v.w_patch[:, :588], h(w["vision_model.embeddings.patch_embedding.weight"]).reshape(32, 588))
    assert torch.equal(v.layers[1]["w_qkv"][32:64], h(w["vision_model.encoder.layers.1.self_attn.k_proj.weight"]))
    assert torch.equal(v.pre_ln[0], h(w["vision_model.pre_layrnorm.weight"]))
    # a tensor the checker does not know is reported, not dropped in silence
    _write_checker_dir(str(tmp_path / "odd"), cfg, w, extra={"text_model.stray": torch.zeros(2)})
    with pytest.warns(UserWarning, match="not read"):
        odd = SafetyCheckerEngine.from_pretrained(str(tmp_path / "odd"), device="cpu", dtype=torch.float16)
    assert odd.unread == ["text_model.stray"]


def test_custom_op_schemas_registered():
    import spider_amd.torch_ops as T
    assert T.SAFETY_OP_NAMES == ("clip_preprocess", "safety_decide", "image_blackout_")
    for n in T.SAFETY_OP_NAMES:
        assert hasattr(torch.ops.spider_hip, n)
    schema = torch.ops.spider_hip.image_blackout_.default._schema
    assert [(a.name, a.is_write) for a in schema.arguments] == [("images", True), ("flags", False)]      # in place on the images only
    assert len(torch.ops.spider_hip.safety_decide.default._schema.returns) == 2


def test_argument_validation_on_the_host():
    from spider_amd import lib as slib
    lib = slib.load()
    assert lib.spider_abi_version() == 4
    one = 16                                                    # any non-null, 16-byte-aligned value: validation fails before a launch
    assert lib.spider_safety_decide(one, one, one, one, one, one, one, 1, 12, 17, 3, 0, None) == -1
    assert b"D % 8" in lib.spider_last_error()
    assert lib.spider_safety_decide(one, one, one, one, one, one, one, 1, 64, 62, 3, 0, None) == -1
    assert b"at most 64" in lib.spider_last_error()
    assert lib.spider_safety_decide(None, one, one, one, one, one, one, 1, 64, 17, 3, 0, None) == -1
    assert b"null" in lib.spider_last_error()
    assert lib.spider_safety_decide(8, one, one, one, one, one, one, 1, 64, 17, 3, 0, None) == -1
    assert b"aligned" in lib.spider_last_error()
    assert lib.spider_clip_preprocess(one, one, one, one, one, 11, one, one, 11, one, 1, 512, 512, 224, 14, 588, 0, None) == -1
    assert b"Kp % 8" in lib.spider_last_error()
    assert lib.spider_clip_preprocess(one, one, one, one, one, 11, one, one, 11, one, 1, 512, 512, 220, 14, 592, 0, None) == -1
    assert b"multiple of patch" in lib.spider_last_error()
    assert lib.spider_clip_preprocess(one, one, 8, one, one, 11, one, one, 11, one, 1, 512, 512, 224, 14, 592, 0, None) == -1
    assert b"aligned" in lib.spider_last_error()
    assert lib.spider_image_blackout_f32(one, one, 1, 6, None) == -1
    assert b"multiple of 4" in lib.spider_last_error()
    assert lib.spider_image_blackout_f32(None, one, 1, 8, None) == -1

"""GPU: the safety checker on the device (spider_amd/safety.py, csrc/safety.hip) -- the feature-extractor kernel against
transformers' CLIPImageProcessor, the CLIP vision engine against transformers' CLIPVisionModelWithProjection in fp32, the decision
kernel against its host restatement, the black-out, and the checker inside StableDiffusionPipeline. Shapes are the smallest at which
each piece can still go wrong; bounds are derived (safety_cases.py) or the ones the same kernels are held to elsewhere."""
import json
import os

import numpy as np
import pytest
import torch

import safety_cases as sc

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


# ------------------------------------------------------------------------------------------ feature extractor
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", list(sc.PREPROCESS_CASES))
def test_preprocess_kernel_matches_clip_image_processor(dev, name, B, dtype):
    from spider_amd import ops
    H, W, size = sc.PREPROCESS_CASES[name]
    patch = 14
    ref = sc.reference_pixel_values(name, B)
    tables = ops.clip_preprocess_tables(H, W, size, size, sc.CLIP_MEAN, sc.CLIP_STD, dev)
    rows = ops.clip_preprocess(sc.case_images(name, B).to(dev), tables, patch, dtype=DT[dtype])
    assert rows.shape == (B * (size // patch) ** 2, 592) and rows.dtype == DT[dtype]
    got, pad = sc.unpatchify(rows.float().cpu(), B, size, patch)
    assert pad.shape[1] == 4 and bool((pad == 0).all())                     # K = 588 -> 592: the pad columns are exactly zero
    err = (got - ref).abs()
    bound = sc.level_bound(2.0)
    bound = bound + sc.half_ulp(ref.abs() + bound, DT[dtype])               # + half an ulp of the output format at the value
    levels = (got - ref).abs() * 255.0 * torch.tensor(sc.CLIP_STD).view(1, 3, 1, 1)
    print(f"MEASURED clip_preprocess case={name} B={B} dtype={dtype} max_levels={float(levels.max()):.3f} (includes the {dtype} rounding)")
    assert bool((err <= bound).all()), float(levels.max())


def test_preprocess_kernel_equals_host_restatement(dev):
    """the integer passes are Pillow's: on the non-square case the kernel's f16 rows are the host restatement's values rounded once"""
    from spider_amd import ops
    from spider_amd.safety import patchify_host, safety_preprocess_host
    H, W, size = sc.PREPROCESS_CASES["rect96x128"]
    img = sc.case_images("rect96x128", 3)
    tables = ops.clip_preprocess_tables(H, W, size, size, sc.CLIP_MEAN, sc.CLIP_STD, dev)
    rows = ops.clip_preprocess(img.to(dev), tables, 14, dtype=torch.float16).cpu()
    want = patchify_host(safety_preprocess_host(img, size, size), 14)
    assert bool(((rows.float() - want).abs() <= sc.half_ulp(want.abs(), torch.float16) + 1e-7).all())      # 1e-7: fp32 division order


# ------------------------------------------------------------------------------------------ vision engine
def _hf_vision(cfg, weights):
    from transformers import CLIPVisionConfig as HFVisionConfig, CLIPVisionModelWithProjection
    hf = CLIPVisionModelWithProjection(HFVisionConfig(hidden_size=cfg.hidden, intermediate_size=cfg.inter, num_hidden_layers=cfg.layers,
                                                      num_attention_heads=cfg.heads, image_size=cfg.image, patch_size=cfg.patch,
                                                      projection_dim=cfg.proj, hidden_act=cfg.act, layer_norm_eps=cfg.eps)).eval()
    res = hf.load_state_dict(weights, strict=False)
    assert not res.unexpected_keys and all(k.endswith("position_ids") for k in res.missing_keys), res
    return hf


def _rel(a, b):
    return float((a.float().cpu() - b).norm() / b.norm())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("config", ["A", "B"])
def test_clip_vision_engine_matches_transformers(dev, config, dtype):
    """A: 2 layers, 17 tokens. B: 1 layer at image 224 -- 257 tokens, an odd count that ends an attention tile mid-way. K = 588 -> 592
    in both. Bound: the one tests/test_clip_vae_engine.py holds CLIPTextEngine to for the same dtype (same kernels, same layer form,
    same depth). Measured on MI355X: see NOTEBOOK.md (safety checker entry)."""
    from spider_amd.clip_vision import CLIPVisionConfig, CLIPVisionEngine, random_vision_weights
    from spider_amd.safety import patchify_host
    cfg = {"A": CLIPVisionConfig(hidden=128, layers=2, heads=2, inter=256, image=56, patch=14, proj=64),
           "B": CLIPVisionConfig(hidden=128, layers=1, heads=2, inter=256, image=224, patch=14, proj=64)}[config]
    w = random_vision_weights(cfg, seed=11)
    B = 3 if config == "A" else 2
    px = torch.randn(B, 3, cfg.image, cfg.image, generator=torch.Generator().manual_seed(4)) * 1.2       # normalised pixels: about [-1.8, 2.2]
    with torch.no_grad():
        ref = _hf_vision(cfg, w)(pixel_values=px).image_embeds
    eng = CLIPVisionEngine(cfg, w, dev, dtype=DT[dtype])
    rows = patchify_host(px, cfg.patch).to(device=dev, dtype=DT[dtype])
    assert rows.shape == (B * cfg.n_patches, 592)
    got = eng.encode(rows)
    assert got.shape == (B, cfg.proj) and got.dtype == DT[dtype]
    assert torch.equal(got, eng.encode(rows, use_graph=False))                # graph and eager: the same launches
    r = _rel(got, ref)
    print(f"MEASURED clip_vision config={config} dtype={dtype} rel={r:.5f}")
    assert r < {"bf16": 1.5e-2, "f16": 1e-3}[dtype]       # measured A: 7.4e-3 / 8.3e-4, B: 4.5e-3 / 5.7e-4


# ------------------------------------------------------------------------------------------ decision + black-out
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_decide_kernel_matches_host(dev, dtype):
    from spider_amd import ops
    from spider_amd.safety import safety_decide_host
    tol = 1e-5                                  # + 2^-20 |s|: fp32 dots of D <= 768 unit-norm terms, tree-reduced
    checked = 0
    cases = dict(sc.decide_cases(64))
    # random 16-bit embeddings at the published width: the dots are real reductions here (D = 768, 17 + 3 rows over 4 waves).
    # Image 0 lies close to concept 0 (flagged), image 1 close to special-care concept 1 (adjustment, no flag), image 2 to nothing.
    # Each threshold is moved by less than one step so that cos - thr sits a quarter step above a multiple of 0.001 (the +0.01
    # adjustment is ten whole steps), which keeps every score clear of a rounding step.
    g = torch.Generator().manual_seed(9)
    e, c, s = torch.randn(3, 768, generator=g), torch.randn(17, 768, generator=g), torch.randn(3, 768, generator=g)
    c[0] = e[0] + 0.3 * torch.randn(768, generator=g)
    s[1] = e[1] + 0.3 * torch.randn(768, generator=g)
    norm = lambda t: torch.nn.functional.normalize(t.to(DT[dtype]).float(), dim=-1)
    for b, want in enumerate([True, False, False]):
        cos_c, cos_s = norm(e[b:b + 1]) @ norm(c).T, norm(e[b:b + 1]) @ norm(s).T
        centre = lambda cos, thr: (cos[0] - (torch.round((cos[0] - thr) * 1000.0) + 0.25) / 1000.0).float()
        cases[f"random768_{b}"] = (e[b:b + 1], c, s, centre(cos_c, 0.2037), centre(cos_s, 0.1913), [want])
    for name, (emb, concepts, special, thr_c, thr_s, want) in cases.items():
        emb, concepts, special = (t.to(DT[dtype]) for t in (emb, concepts, special))       # the SAME 16-bit values on both sides
        h_scores, h_flags = safety_decide_host(emb, concepts, special, thr_c, thr_s)
        margin = sc.rounding_margin(emb, concepts, special, thr_c, thr_s)
        assert margin > 2 * tol, (name, margin)                               # every case sits clear of a rounding step: none is skipped
        scores, flags = ops.safety_decide(emb.to(dev), concepts.to(dev), special.to(dev), thr_c.to(dev), thr_s.to(dev))
        assert scores.dtype == torch.float32 and flags.dtype == torch.int32
        d = (scores.cpu() - h_scores).abs()
        assert bool((d <= tol + 2.0 ** -20 * h_scores.abs()).all()), (name, float(d.max()))
        assert flags.cpu().bool().tolist() == h_flags.tolist() == want, (name, scores)
        checked += 1
    assert checked == len(cases) == 11
    assert float(safety_decide_host(*[t.to(DT[dtype]) if i < 3 else t for i, t in enumerate(cases["random768_1"][:5])])[0][0, 1]) > 0   # special 1 fired


def test_blackout(dev):
    from spider_amd import ops
    img = torch.rand(3, 3, 20, 36, generator=torch.Generator().manual_seed(1))          # 2160 floats per image: not a multiple of 1024
    img[1, 0, 0, 0] = float("nan")                                                       # a flagged image is zeros whatever it held
    flags = torch.tensor([0, 1, 0], dtype=torch.int32)
    out = ops.image_blackout_(img.to(dev), flags.to(dev)).cpu()
    assert torch.equal(out[0], img[0]) and torch.equal(out[2], img[2]) and bool((out[1] == 0).all())
    big = torch.rand(2, 3, 512, 512, generator=torch.Generator().manual_seed(2))         # more than one grid-stride step per block
    out = ops.image_blackout_(big.to(dev), torch.tensor([1, 0], dtype=torch.int32, device=dev)).cpu()
    assert bool((out[0] == 0).all()) and torch.equal(out[1], big[1])


# ------------------------------------------------------------------------------------------ pipeline
CHECKER_CFG = dict(hidden=128, layers=2, heads=2, inter=256, image=56, patch=14, proj=64)


def _image_sensitive_checker_weights(cfg, seed):
    """random_init's weights with sharp attention and strong residual branches. Under the plain random init the pooled state is
    dominated by the class token's own constant path: the class token attends almost uniformly, so what it gathers is the mean over
    the patches, and two generated images embed at cos 0.63 - 0.96 (measured on MI355X over 6 seeds x 6 latent choices) -- no
    threshold of 0.5 can tell them apart, which a trained tower does. q / k x 8 makes the class token read a few patches instead of
    their mean; out_proj / fc2 x 4 lets what it reads outweigh the constant residual. Measured with the latents of the test below:
    cos 0.25 - 0.30 over seeds 5 - 8. Every kernel runs as it does for any other weights."""
    from spider_amd.safety import random_checker_weights
    w = random_checker_weights(cfg, seed=seed)
    for k in w:
        if k.endswith(("q_proj.weight", "k_proj.weight")):
            w[k] = w[k] * 8.0
        if k.endswith(("out_proj.weight", "fc2.weight")):
            w[k] = w[k] * 4.0
    return w


@pytest.fixture(scope="module")
def sd_dir(tmp_path_factory):
    """the tiny SD directory of test_from_pretrained_gpu.py plus safety_checker/ and feature_extractor/"""
    from test_from_pretrained_gpu import _write_sd_directory
    from test_safety_cpu import _write_checker_dir
    from spider_amd.clip_vision import CLIPVisionConfig
    root = str(tmp_path_factory.mktemp("sd_checker") / "sd")
    _write_sd_directory(root)
    cfg = CLIPVisionConfig(**CHECKER_CFG)
    _write_checker_dir(os.path.join(root, "safety_checker"), cfg, _image_sensitive_checker_weights(cfg, seed=5))
    os.makedirs(os.path.join(root, "feature_extractor"))
    json.dump({"crop_size": 56, "do_center_crop": True, "do_convert_rgb": True, "do_normalize": True, "do_resize": True,
               "feature_extractor_type": "CLIPFeatureExtractor", "image_mean": list(sc.CLIP_MEAN), "image_std": list(sc.CLIP_STD),
               "resample": 3, "size": 56}, open(os.path.join(root, "feature_extractor", "preprocessor_config.json"), "w"))
    return root


def test_pipeline_with_checker(dev, sd_dir):
    from spider_amd.pipelines import StableDiffusionPipeline
    from spider_amd.safety import SafetyCheckerEngine
    pipe = StableDiffusionPipeline.from_pretrained(sd_dir, torch_dtype=torch.float16, device=dev)
    plain = StableDiffusionPipeline.from_pretrained(sd_dir, torch_dtype=torch.float16, device=dev, safety_checker=None)
    ck = pipe.safety_checker
    assert isinstance(ck, SafetyCheckerEngine) and ck.unread == [] and ck.dtype == torch.float16 and plain.safety_checker is None
    assert ck.pre["size"] == 56 and ck.pre["crop"] == 56 and ck.cfg.hidden == 128
    # image 0 from noise, image 1 from constant latents: two images that differ in more than their noise
    lat = torch.cat([torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(5)), torch.full((1, 4, 16, 16), 2.0)])
    kw = dict(prompt=["a red door", "a blue boat"], num_inference_steps=4, latents=lat, output_type="np")
    base = plain(**kw)
    assert base.nsfw_content_detected is None and base.images.shape == (2, 64, 64, 3) and base.images.std() > 1e-3
    assert plain(**kw, return_dict=False)[1] is None
    # nothing reaches the loaded thresholds (2.0): the checker runs, flags nothing and leaves every pixel as it was
    clean = pipe(**kw)
    assert clean.nsfw_content_detected == [False, False] and np.array_equal(clean.images, base.images)
    # concept 0 := the normalised embedding the checker itself produces for image 0, threshold 0.5; every other threshold stays 2
    img_dev = torch.from_numpy(base.images).permute(0, 3, 1, 2).contiguous().to(dev)
    _, flags0, scores0, embeds = ck.run(img_dev.clone(), use_graph=False)
    assert flags0.tolist() == [0, 0]
    ck.concept_embeds[0] = torch.nn.functional.normalize(embeds[0].float(), dim=-1).to(ck.dtype)
    ck.concept_thr[0] = 0.5
    cos1 = float(torch.nn.functional.cosine_similarity(embeds[0].float(), embeds[1].float(), dim=0))
    print(f"MEASURED safety_pipeline cos(image0, image1)={cos1:.4f}")
    assert cos1 < 0.4, cos1           # the fixture's precondition: image 1 sits clear of the 0.5 threshold (0.304 on MI355X)
    out = pipe(**kw)
    assert out.nsfw_content_detected == [True, False]
    assert bool((out.images[0] == 0).all()) and np.array_equal(out.images[1], base.images[1])        # black / bit for bit
    # graph and eager agree, on every output
    g = ck.run(img_dev.clone(), use_graph=True)
    e = ck.run(img_dev.clone(), use_graph=False)
    assert all(torch.equal(a, b) for a, b in zip(g, e)) and g[1].tolist() == [1, 0]
    assert bool((g[0][0] == 0).all()) and torch.equal(g[0][1], img_dev[1])
    # the other output forms
    im, has = pipe(**kw, return_dict=False)
    assert has == [True, False] and np.array_equal(im, out.images)
    pil = pipe(**{**kw, "output_type": "pil"})
    assert pil.nsfw_content_detected == [True, False] and pil.images[0].getextrema() == ((0, 0), (0, 0), (0, 0))
    latent = pipe(**{**kw, "output_type": "latent"})
    assert latent.nsfw_content_detected is None and latent.images.shape == (2, 4, 16, 16)


def test_feature_extractor_settings_the_device_lacks_raise(dev, sd_dir, tmp_path):
    import shutil
    from spider_amd.pipelines import StableDiffusionPipeline
    root = str(tmp_path / "sd")
    shutil.copytree(sd_dir, root)
    p = os.path.join(root, "feature_extractor", "preprocessor_config.json")
    c = json.load(open(p))
    c["resample"] = 2
    json.dump(c, open(p, "w"))
    with pytest.raises(NotImplementedError, match="resample"):
        StableDiffusionPipeline.from_pretrained(root, torch_dtype=torch.float16, device=dev)

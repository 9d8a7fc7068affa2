"""Long fp32 ORACLE loops, run once in the build container, so that the GPU suite can compare full denoising loops without spending
its time budget on CPU work:

    python tests/golden/make_oracle_loops.py [sd15] [audioldm] [sdxl] [zeroscope] [zeroscope8]    # 8 cores: ~2, ~2, ~5, ~45, ~3 minutes

  oracle_loop_sd15_pndm40.npz      SD-v1.5 UNet (UNetCfg.sd15(), weights seed 0), [1, 4, 64, 64] latent, 40 PNDM steps = 41 evaluations,
                           guidance 7.5 (configs[1]; custom_sd.py:627-652): latents in / out.
  oracle_loop_audioldm_l_ddim40.npz  AudioLDM-L UNet (UNetCfg.audioldm_l(), weights seed 2), class-label conditioning, [1, 8, 125, 16]
                           latent of 5 s of audio, 40 DDIM steps, guidance 2.5 (custom_ad.py:568-594): latents in / out.

  oracle_loop_sdxl50.npz   SDXL UNet (oracle.unet.UNetCfg.sdxl(), weights random_unet_weights(seed=4)), CFG batch 2 on a
                           [1, 4, 64, 64] latent (512^2), 50 DDIM steps, guidance 5.0 -- the scheduler / step count / guidance
                           of the story decoder (Comic_Generation.py:316-317, 440) without the
                           consistent-self-attention coins: inputs (latent, prompt states, pooled states, time ids) and the
                           fp32 latents after the loop, plus the latents after steps 1, 10 and 25.

  oracle_loop_zeroscope40_f16*.npz zeroscope UNet3D (oracle.unet3d.UNet3DCfg.zeroscope(), weights random_unet3d_weights(seed=6)),
                           CFG batch 2 on the [1, 4, 16, 40, 72] latent of configs[3] / [4], 40 DDIM steps, guidance 9.0
                           (spider_decoder.py:122-143, custom_vd.py:664-697): checksums of the seeded inputs and the fp32 latents after 1, 20, 40 steps.

  oracle_step_zeroscope_8frames.npz  ONE evaluation of the same UNet3D at 8 frames ([2, 4, 8, 40, 72], timestep 701): the fp32 output
                           (target `zeroscope8`, not part of the default list).

These vectors are produced by the CPU RESTATEMENT (oracle/unet.py), not by the reference: diffusers is absent from the image
(SURVEY.md section 8c), so they pin the HIP engine to the oracle over a whole loop -- the quantity north_star names -- and leave the
oracle itself "parity unpinned upstream" as DESIGN.md section 4 records. Nothing under /root/reference is read.
"""
import os
import sys
import time

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from oracle.unet import DDIMOracle, UNetCfg, UNetOracle, random_unet_weights  # noqa: E402


def sdxl_inputs():
    """the seeded inputs of the SDXL loop fixture (also used by the GPU test to rebuild the engine side)"""
    g = torch.Generator().manual_seed(21)
    lat = torch.randn(1, 4, 64, 64, generator=g)
    enc = torch.randn(2, 77, 2048, generator=g).bfloat16().float()
    added = dict(text_embeds=torch.randn(2, 1280, generator=g).bfloat16().float(),
                 time_ids=torch.tensor([[512, 512, 0, 0, 512, 512]] * 2, dtype=torch.float32))
    return lat, enc, added


@torch.no_grad()
def sdxl_loop(steps=50, guidance=5.0, keep=(1, 10, 25)):
    ocfg = UNetCfg.sdxl()
    w = random_unet_weights(ocfg, seed=4)
    unet, sched = UNetOracle(ocfg, w), DDIMOracle()
    lat, enc, added = sdxl_inputs()
    ts = sched.set_timesteps(steps)
    x = lat * sched.init_noise_sigma
    kept = {}
    t0 = time.time()
    for i, t in enumerate(ts):
        e = unet.forward(torch.cat([x] * 2), t, enc, added)
        eu, ec = e.chunk(2)
        x = sched.step(eu + guidance * (ec - eu), t, x)
        if i + 1 in keep:
            kept[f"after_{i + 1}"] = x.numpy().copy()
        print(f"step {i + 1}/{steps} t={int(t)} |x|={float(x.norm()):.4f} ({time.time() - t0:.0f} s)", flush=True)
    np.savez_compressed(os.path.join(OUT, "oracle_loop_sdxl50.npz"), latents_in=lat.numpy(), enc=enc.numpy(),
                        text_embeds=added["text_embeds"].numpy(), time_ids=added["time_ids"].numpy(),
                        latents_out=x.numpy(), steps=steps, guidance=guidance, weights_seed=4, **kept)


def sd15_inputs():
    """the seeded case of tests/test_fullsize_parity.py::sd15_case (prompt states) + the loop's starting latent"""
    g = torch.Generator().manual_seed(1)
    torch.randn(2, 4, 64, 64, generator=g)                       # (the single-evaluation test's sample: same generator stream)
    enc = torch.randn(2, 77, 768, generator=g).bfloat16().float()
    lat = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(11))
    return lat, enc


@torch.no_grad()
def sd15_loop(steps=40, guidance=7.5):
    """configs[1]'s image decoder: SD-v1.5 UNet, 40 PNDM steps = 41 evaluations, guidance 7.5 (custom_sd.py:627-652)."""
    from oracle.unet import PNDMOracle, denoise_loop
    ocfg = UNetCfg.sd15()
    lat, enc = sd15_inputs()
    t0 = time.time()
    ref = denoise_loop(UNetOracle(ocfg, random_unet_weights(ocfg, seed=0)), PNDMOracle(), lat, enc, guidance, steps)
    print(f"sd15 loop: {time.time() - t0:.0f} s", flush=True)
    np.savez_compressed(os.path.join(OUT, "oracle_loop_sd15_pndm40.npz"), latents_in=lat.numpy(), enc_sum=float(enc.double().sum()),
                        latents_out=ref.numpy(), steps=steps, guidance=guidance, weights_seed=0)


def audioldm_inputs():
    g = torch.Generator().manual_seed(13)
    lat = torch.randn(1, 8, 125, 16, generator=g)
    cl = torch.nn.functional.normalize(torch.randn(2, UNetCfg.audioldm_l().class_in, generator=g), dim=-1).bfloat16().float()
    return lat, cl


@torch.no_grad()
def audioldm_loop(steps=40, guidance=2.5):
    """configs[3] / [4]'s audio decoder: AudioLDM-L UNet, class-label conditioning, 40 DDIM steps, guidance 2.5 on the
    [1, 8, 125, 16] latent of 5 s of audio (custom_ad.py:568-594)."""
    from oracle.unet import denoise_loop
    ocfg = UNetCfg.audioldm_l()
    lat, cl = audioldm_inputs()
    t0 = time.time()
    ref = denoise_loop(UNetOracle(ocfg, random_unet_weights(ocfg, seed=2)), DDIMOracle(), lat, None, guidance, steps, class_labels=cl)
    print(f"audioldm loop: {time.time() - t0:.0f} s", flush=True)
    np.savez_compressed(os.path.join(OUT, "oracle_loop_audioldm_l_ddim40.npz"), latents_in=lat.numpy(), class_labels=cl.numpy(),
                        latents_out=ref.numpy(), steps=steps, guidance=guidance, weights_seed=2)


def zeroscope_inputs(frames=16):
    g = torch.Generator().manual_seed(23)
    lat = torch.randn(1, 4, frames, 40, 72, generator=g)
    enc = torch.randn(2, 77, 1024, generator=g).bfloat16().float()
    return lat, enc


@torch.no_grad()
def zeroscope_loop(frames=16, steps=40, guidance=9.0, keep=(1, 20)):
    """configs[3] / [4]'s video decoder: zeroscope UNet3D, [1, 4, 16, 40, 72] latents, 40 DDIM steps, guidance 9.0
    (spider_decoder.py:122-143 -> custom_vd.py:664-697; the scheduler sees the frames as batch, :684-692)."""
    from oracle.unet3d import UNet3DCfg, UNet3DOracle, random_unet3d_weights
    ocfg = UNet3DCfg.zeroscope()
    unet, sched = UNet3DOracle(ocfg, random_unet3d_weights(ocfg, seed=6)), DDIMOracle()
    lat, enc = zeroscope_inputs(frames)
    ts = sched.set_timesteps(steps)
    x = lat * sched.init_noise_sigma
    kept = {}
    t0 = time.time()
    for i, t in enumerate(ts):
        e = unet.forward(torch.cat([x] * 2), t, enc)
        eu, ec = e.chunk(2)
        eps = eu + guidance * (ec - eu)
        B, C, Fr, H, W = x.shape
        flat = lambda v: v.permute(0, 2, 1, 3, 4).reshape(B * Fr, C, H, W)
        x = sched.step(flat(eps), t, flat(x))[None, :].reshape(B, Fr, C, H, W).permute(0, 2, 1, 3, 4)
        if i + 1 in keep:
            kept[f"after_{i + 1}"] = x.numpy().copy()
        print(f"step {i + 1}/{steps} t={int(t)} |x|={float(x.norm()):.4f} ({time.time() - t0:.0f} s)", flush=True)
    # (0.7 MB per latent tensor: the seeded inputs are not stored, only their checksums -- the test regenerates them; the latents after
    # step 1 go with the scalars, every later tensor into a file of its own, so that no fixture exceeds 1 MiB)
    stem = os.path.join(OUT, f"oracle_loop_zeroscope{steps}_f{frames}")
    later = {**{k: v for k, v in kept.items() if k != "after_1"}, "latents_out": x.contiguous().numpy()}
    np.savez_compressed(f"{stem}.npz", latents_in_sum=float(lat.double().sum()), enc_sum=float(enc.double().sum()), steps=steps,
                        guidance=guidance, frames=frames, weights_seed=6, after_1=kept["after_1"])
    for k, v in later.items():
        np.savez_compressed(f"{stem}_{k}.npz", **{k: v})


def zeroscope8_inputs(frames=8):
    """the seeded inputs of the single-evaluation fixture at 8 frames (the GPU test rebuilds them and checks the checksums)"""
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, 4, frames, 40, 72, generator=g).bfloat16().float()
    enc = torch.randn(2, 77, 1024, generator=g).bfloat16().float()
    return x, enc


@torch.no_grad()
def zeroscope8_step(frames=8, t=701):
    """ONE fp32 oracle evaluation of the zeroscope UNet3D at 8 frames of 40 x 72 (weights seed 6, timestep 701, CFG batch 2): the live
    oracle took 50-65 s of the GPU suite's time budget per run (round 6: the suite was at 704 of the driver's 900 s)."""
    from oracle.unet3d import UNet3DCfg, UNet3DOracle, random_unet3d_weights
    ocfg = UNet3DCfg.zeroscope()
    w = random_unet3d_weights(ocfg, seed=6)
    x, enc = zeroscope8_inputs(frames)
    assert enc.shape[-1] == ocfg.cross_dim
    t0 = time.time()
    ref = UNet3DOracle(ocfg, w).forward(x, torch.tensor(t), enc)
    print(f"zeroscope8: one evaluation in {time.time() - t0:.0f} s", flush=True)
    np.savez(os.path.join(OUT, "oracle_step_zeroscope_8frames.npz"), ref=ref.numpy().astype(np.float32), weights_seed=6, t=t, frames=frames,
             x_sum=float(x.double().sum()), enc_sum=float(enc.double().sum()))


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("ORACLE_THREADS", os.cpu_count() or 8)))
    which = sys.argv[1:] or ["sd15", "audioldm", "sdxl", "zeroscope"]
    if "sd15" in which:
        sd15_loop()
    if "audioldm" in which:
        audioldm_loop()
    if "sdxl" in which:
        sdxl_loop()
    if "zeroscope" in which:
        zeroscope_loop()
    if "zeroscope8" in which:
        zeroscope8_step()

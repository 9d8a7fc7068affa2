"""What calibrated MXFP4 (ops.gptq_mxfp4, csrc/gptq.hip) costs at Qwen2.5-7B shapes: one layer's four matrices, each timed in its
parts -- the Hessian sum over T input rows (fp64 addmm), validation / damping (prepare), the factor U (fp64 cholesky ->
cholesky_inverse -> cholesky, on the device or the host: reported), the sweep (kernel launches + fp32 trailing updates) and, apart,
the kernel launches alone (the same launches without the updates: the kernel's time does not depend on the values) -- and the
projection for 28 layers. Also the sweep of the qkv matrix by group width 1..4 (ops.GPTQ_GROUP_BLOCKS is chosen from it).
Inputs are random (rank 64 plus isotropic noise): the cost does not depend on them. The first matrix (w_qkv) also pays the first
call of the solver and the GEMMs at its size; the group-width line repeats its sweep warm. Records what it is; there is no threshold.

    python scripts/exp/gptq_cost.py [--rows 2048] [--out profiles/gptq_cost.txt]
"""
import argparse
import time

import torch

from spider_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=2048, help="calibration rows T behind every Hessian")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t


def kernel_only(N, K, gb):
    """the launches of one sweep without the trailing updates, on a matrix of ones and U = I"""
    Wt = torch.full((K, N), 0.01, dtype=torch.float32, device=dev)
    U = torch.eye(K, dtype=torch.float32, device=dev)
    blocks = torch.empty(N, K // 2, dtype=torch.uint8, device=dev)
    scales = torch.empty(N, K // 32, dtype=torch.uint8, device=dev)
    Et = torch.empty(32 * gb, N, dtype=torch.float32, device=dev)

    def go():
        for j0 in range(0, K, 32 * gb):
            ops.gptq_mxfp4_sweep(Wt, U, blocks, scales, Et, j0, min(gb, (K - j0) // 32))
    go()
    return timed(go)[1]


g = torch.Generator(device=dev).manual_seed(0)
H_, I_, QKV = 3584, 18944, (28 + 2 * 4) * 128
say(f"Qwen2.5-7B layer shapes, {args.rows} calibration rows, damp 0.01; seconds, one run each behind a warm-up of the small pieces; "
    f"factor U on the {ops.gptq_factor_where(dev)}")
ops.gptq_mxfp4(torch.randn(64, 64, device=dev), torch.eye(64, device=dev, dtype=torch.float64))      # warm-up: library load, handles
say("| matrix | N | K | hessian | prepare | factor | sweep (group 4) | of it kernel launches | launches |")
say("|---|---|---|---|---|---|---|---|---|")
total = 0.0
for name, N, K in (("w_qkv", QKV, H_), ("w_o", H_, H_), ("w_gu", 2 * I_, H_), ("w_down", H_, I_)):
    W = (torch.randn(N, K, generator=g, device=dev) * 0.02).bfloat16()
    X = (torch.randn(args.rows, 64, generator=g, device=dev) @ torch.randn(64, K, generator=g, device=dev)
         + 0.3 * torch.randn(args.rows, K, generator=g, device=dev)).bfloat16()

    def hessian():
        x64 = X.double()
        return torch.zeros(K, K, dtype=torch.float64, device=dev).addmm_(x64.t(), x64)
    H, t_h = timed(hessian)
    tm = {}
    ops.gptq_mxfp4(W, H, 0.01, timing=tm)
    t_k = kernel_only(N, K, ops.GPTQ_GROUP_BLOCKS)
    n_launch = -(-K // (32 * ops.GPTQ_GROUP_BLOCKS))
    say(f"| {name} | {N} | {K} | {t_h:.3f} | {tm['prepare']:.3f} | {tm['factor']:.3f} ({tm['factor_where']}) | {tm['sweep']:.3f} | {t_k:.3f} | {n_launch} |")
    total += t_h + tm["prepare"] + tm["factor"] + tm["sweep"]
    if name == "w_qkv":
        widths = []
        for gb in (1, 2, 3, 4):
            t2 = {}
            ops.gptq_mxfp4(W, H, 0.01, group_blocks=gb, timing=t2)
            widths.append(f"{gb}: {t2['sweep']:.3f} (kernel {kernel_only(N, K, gb):.3f})")
    del W, X, H
    torch.cuda.empty_cache()
say("")
say("w_qkv sweep by group width (MX blocks per launch): " + ", ".join(widths))
say(f"one layer {total:.2f} s; 28 layers {28 * total:.1f} s (the engine's pass adds the proxy losses -- two fp64 products W H per matrix -- and "
    f"the forward of the calibration rows)")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")

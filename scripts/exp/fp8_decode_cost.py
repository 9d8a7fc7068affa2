"""What weight_dtype="fp8" buys per decode step (Qwen2.5-7B shapes, context 1536, rows 1 / 2 / 3 / 4): the captured decode step of
an FP8 engine (e4m3 bytes through gemv_w8 / gemv_swiglu_w8 in all four layer projections) against the captured step of a bf16 engine
on the route it takes for that row count -- row-major GEMVs at 1 row, fragment-major MFMA from 2 rows (LlamaEngine.FM_MIN_BATCH). Both
engines live in one process and are alternated, ROUNDS rounds; every round times T single graph replays with device events and
reports their median and quartiles; the figure per row count is the median of the round medians. By the keep / reject rule of
DESIGN.md section 5 a difference below 3 % is no difference: FP8_MAX_ROWS is the largest row count at which FP8 wins by >= 3 %.

Second part (alone with --ops-only): the four projections by themselves, captured launches cycling through the 28 layers'
weights (233 MB of e4m3 or 466 MB of bf16 per layer, so no launch finds its weights in the 256 MB Infinity Cache), FP8 against
the bf16 kernel of the same route -- which projection pays. The dispatch of csrc/gemv_wq.hip can be varied from the environment
(SPIDER_W8_NWB, SPIDER_W8_R, SPIDER_W8_GU_R, SPIDER_W8_LDS_MAX), one process per setting.

    python scripts/exp/fp8_decode_cost.py [--out FILE] [--rows 1,2,3,4] [--ops-only]"""
import argparse
import statistics
import sys

import torch

from spider_amd import ops
from spider_amd.llm import LlamaEngine, LLMConfig

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--rows", default="1,2,3,4")
ap.add_argument("--ops-only", action="store_true", help="skip the decode steps, time the projections alone")
args = ap.parse_args()

dev = torch.device("cuda:0")
cfg = LLMConfig.qwen25_7b()
CTX, T, ROUNDS = 1536, 96, 3
ROWS = [int(r) for r in args.rows.split(",")]
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


ENG = {"bf16": LlamaEngine.random_init(cfg, dev, max_batch=4, max_len=CTX + 160, seed=0),
       "fp8": LlamaEngine.random_init(cfg, dev, max_batch=4, max_len=CTX + 160, seed=0, weight_dtype="fp8")}
ENG["fp8"].FP8_MAX_ROWS = ops.W8_MAX_ROWS      # measure every row count the kernels exist for, whatever the class default is
say(f"engines: bf16 fm_batch={ENG['bf16'].fm_batch} FM_MIN_BATCH={ENG['bf16'].FM_MIN_BATCH}; fp8 rows <= {ENG['fp8'].FP8_MAX_ROWS}; "
    f"context {CTX}, {T} replays per round, {ROUNDS} rounds")


def replays(eng, B, ids):
    """prompt pass + a few steps (state set, graph captured on the first call), then T timed replays of the decode graph"""
    eng.generate(input_ids=ids, max_new_tokens=8, eos_token_id=[])
    graph = eng._graphs[(B, False, False, 0)][1]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(T + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(T):
        graph.replay()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(T)]      # us


def quart(xs):
    q = statistics.quantiles(xs, n=4)
    return q[1], q[0], q[2]


table = []
for B in ([] if args.ops_only else ROWS):
    ids = torch.randint(3, cfg.vocab, (B, CTX), generator=torch.Generator().manual_seed(B))
    for name in ENG:     # warm-up: kernels loaded, graphs captured
        replays(ENG[name], B, ids)
    med = {name: [] for name in ENG}
    for r in range(ROUNDS):
        for name in ENG:
            m, lo, hi = quart(replays(ENG[name], B, ids))
            med[name].append(m)
            say(f"rows {B} round {r} {name:4s} step median {m:8.1f} us  quartiles [{lo:.1f}, {hi:.1f}]")
    mb, mf = statistics.median(med["bf16"]), statistics.median(med["fp8"])
    route = "row-major" if not (ENG["bf16"].fm_batch and B >= ENG["bf16"].FM_MIN_BATCH) else "fragment-major"
    say(f"rows {B}: bf16 ({route}) {mb:.1f} us (rounds {min(med['bf16']):.1f} .. {max(med['bf16']):.1f}), fp8 {mf:.1f} us "
        f"(rounds {min(med['fp8']):.1f} .. {max(med['fp8']):.1f}), fp8 / bf16 = {mf / mb:.3f} ({(1 - mf / mb) * 100:+.1f} % saved)")
    table.append((B, route, mb, mf))

if table:
    say("")
    say("| rows | bf16 route | bf16 us / step | fp8 us / step | fp8 / bf16 |")
    say("|---|---|---|---|---|")
    for B, route, mb, mf in table:
        say(f"| {B} | {route} | {mb:.0f} | {mf:.0f} | {mf / mb:.3f} |")
    wins = [B for B, _, mb, mf in table if mf <= 0.97 * mb]
    say(f"FP8 wins by >= 3 % at rows {wins}")

# ---- the projections alone, weights cold (a different layer per launch)
say("")
L = cfg.layers
fp8, bf = ENG["fp8"], ENG["bf16"]
bfl = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)


def timed(fn, reps=10):
    """us per launch: one pass through the layers captured in a graph (the host cannot launch a 5 us kernel every 5 us), `reps` replays"""
    fn(0)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for l in range(L):
                fn(l)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * L)


for B in ROWS:
    fm = bf.fm_batch and B >= bf.FM_MIN_BATCH
    h, a, act = bfl(B, cfg.hidden), bfl(B, cfg.n_q * cfg.head_dim), bfl(B, cfg.inter)
    nq = fp8.layers[0]["w_qkv"].shape[0]
    pairs = {
        "qkv": (lambda l: ops.gemv_w8(fp8.layers[l]["w_qkv_q8"], fp8.layers[l]["w_qkv_s8"], h, bias=fp8.layers[l]["b_qkv"],
                                      norm_w=fp8.layers[l]["ln1"], eps=cfg.eps),
                (lambda l: ops.gemv_fm(bf.layers[l]["w_qkv_fm"], h, nq, bias=bf.layers[l]["b_qkv"], norm_eps=cfg.eps)) if fm else
                (lambda l: ops.gemv(bf.layers[l]["w_qkv"], h, bias=bf.layers[l]["b_qkv"], norm_w=bf.layers[l]["ln1"], eps=cfg.eps))),
        "o": (lambda l: ops.gemv_w8(fp8.layers[l]["w_o_q8"], fp8.layers[l]["w_o_s8"], a, res=h),
              (lambda l: ops.gemv_fm(bf.layers[l]["w_o_fm"], a, cfg.hidden, res=h)) if fm else
              (lambda l: ops.gemv(bf.layers[l]["w_o"], a, res=h))),
        "gate_up": (lambda l: ops.gemv_swiglu_w8(fp8.layers[l]["w_gu_q8"], fp8.layers[l]["w_gu_s8"], h, norm_w=fp8.layers[l]["ln2"], eps=cfg.eps),
                    (lambda l: ops.gemv_swiglu_fm(bf.layers[l]["w_gu_fm"], h, norm_eps=cfg.eps)) if fm else
                    (lambda l: ops.gemv_swiglu(bf.layers[l]["w_gu"], h, norm_w=bf.layers[l]["ln2"], eps=cfg.eps))),
        "down": (lambda l: ops.gemv_w8(fp8.layers[l]["w_down_q8"], fp8.layers[l]["w_down_s8"], act, res=h),
                 (lambda l: ops.gemv_fm(bf.layers[l]["w_down_fm"], act, cfg.hidden, res=h)) if fm else
                 (lambda l: ops.gemv(bf.layers[l]["w_down"], act, res=h))),
    }
    for name, (f8, f16) in pairs.items():
        t16a, t8a, t16b, t8b = timed(f16), timed(f8), timed(f16), timed(f8)
        t16, t8 = (t16a + t16b) / 2, (t8a + t8b) / 2
        nbytes = fp8.layers[0][{"qkv": "w_qkv_q8", "o": "w_o_q8", "gate_up": "w_gu_q8", "down": "w_down_q8"}[name]].numel()
        say(f"rows {B} {name:8s} bf16 {'fm' if fm else 'rm'} {t16:7.1f} us ({2 * nbytes / t16 / 1e6:5.2f} TB/s)   fp8 {t8:7.1f} us "
            f"({nbytes / t8 / 1e6:5.2f} TB/s)   fp8 / bf16 = {t8 / t16:.3f}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
sys.exit(0)

"""What weight_dtype="mxfp4" buys per decode step (Qwen2.5-7B shapes, context 1536, rows 1 / 2 / 3 / 4), on the method of
scripts/exp/fp8_decode_cost.py: the captured decode step of an MXFP4 engine (e2m1 nibbles and E8M0 block scales through gemv_w4 /
gemv_swiglu_w4 in all four layer projections) against the captured step of a bf16 engine on the route it takes for that row count
-- row-major GEMVs at 1 row, fragment-major MFMA from 2 rows (LlamaEngine.FM_MIN_BATCH) -- with the FP8 engine beside it for
comparison. The three engines live in one process and are alternated, ROUNDS rounds; every round times T single graph replays with
device events and reports their median and quartiles; the figure per row count is the median of the round medians. By the keep /
reject rule of DESIGN.md section 5 a difference below 3 % is no difference: MXFP4_MAX_ROWS is the largest row count at which MXFP4
beats the bf16 route of the same row count by >= 3 %.

Second part (alone with --ops-only): the four projections by themselves, captured launches cycling through the 28 layers'
weights (124 MB of MXFP4, 233 MB of e4m3 or 466 MB of bf16 per layer; a cycle through the 28 layers is 3.5 GB of MXFP4 against
the 256 MB of the Infinity Cache, so no launch finds its weights there).

    python scripts/exp/mxfp4_decode_cost.py [--out FILE] [--rows 1,2,3,4] [--ops-only]"""
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


ENG = {name: LlamaEngine.random_init(cfg, dev, max_batch=4, max_len=CTX + 160, seed=0, weight_dtype=name) for name in ("bf16", "fp8", "mxfp4")}
ENG["fp8"].FP8_MAX_ROWS = ops.W8_MAX_ROWS      # measure every row count the kernels exist for, whatever the class defaults are
ENG["mxfp4"].MXFP4_MAX_ROWS = ops.W4_MAX_ROWS
say(f"engines: bf16 fm_batch={ENG['bf16'].fm_batch} FM_MIN_BATCH={ENG['bf16'].FM_MIN_BATCH}; fp8 rows <= {ENG['fp8'].FP8_MAX_ROWS}; "
    f"mxfp4 rows <= {ENG['mxfp4'].MXFP4_MAX_ROWS}; context {CTX}, {T} replays per round, {ROUNDS} rounds")


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
            say(f"rows {B} round {r} {name:5s} step median {m:8.1f} us  quartiles [{lo:.1f}, {hi:.1f}]")
    m = {name: statistics.median(med[name]) for name in ENG}
    route = "row-major" if not (ENG["bf16"].fm_batch and B >= ENG["bf16"].FM_MIN_BATCH) else "fragment-major"
    say(f"rows {B}: bf16 ({route}) {m['bf16']:.1f} us (rounds {min(med['bf16']):.1f} .. {max(med['bf16']):.1f}), "
        f"fp8 {m['fp8']:.1f} us (rounds {min(med['fp8']):.1f} .. {max(med['fp8']):.1f}), "
        f"mxfp4 {m['mxfp4']:.1f} us (rounds {min(med['mxfp4']):.1f} .. {max(med['mxfp4']):.1f}); fp8 / bf16 = {m['fp8'] / m['bf16']:.3f}, "
        f"mxfp4 / bf16 = {m['mxfp4'] / m['bf16']:.3f} ({(1 - m['mxfp4'] / m['bf16']) * 100:+.1f} % saved)")
    table.append((B, route, m["bf16"], m["fp8"], m["mxfp4"]))

if table:
    say("")
    say("| rows | bf16 route | bf16 us / step | fp8 us / step | mxfp4 us / step | fp8 / bf16 | mxfp4 / bf16 |")
    say("|---|---|---|---|---|---|---|")
    for B, route, mb, m8, m4 in table:
        say(f"| {B} | {route} | {mb:.0f} | {m8:.0f} | {m4:.0f} | {m8 / mb:.3f} | {m4 / mb:.3f} |")
    wins = [B for B, _, mb, _, m4 in table if m4 <= 0.97 * mb]
    say(f"MXFP4 beats the bf16 route of the same row count by >= 3 % at rows {wins}")

# ---- the projections alone, weights cold (a different layer per launch)
say("")
L = cfg.layers
mx, fp8, bf = ENG["mxfp4"], ENG["fp8"], ENG["bf16"]
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
    nq = bf.layers[0]["w_qkv"].shape[0]
    fuse4 = ops.w4_norm_fits(B, cfg.hidden)
    assert fuse4 and ops.w8_norm_fits(B, cfg.hidden)
    forms = {
        "qkv": ((lambda l: ops.gemv_w4(mx.layers[l]["w_qkv_q4"], mx.layers[l]["w_qkv_e4"], h, bias=mx.layers[l]["b_qkv"],
                                       norm_w=mx.layers[l]["ln1"], eps=cfg.eps)),
                (lambda l: ops.gemv_w8(fp8.layers[l]["w_qkv_q8"], fp8.layers[l]["w_qkv_s8"], h, bias=fp8.layers[l]["b_qkv"],
                                       norm_w=fp8.layers[l]["ln1"], eps=cfg.eps)),
                (lambda l: ops.gemv_fm(bf.layers[l]["w_qkv_fm"], h, nq, bias=bf.layers[l]["b_qkv"], norm_eps=cfg.eps)) if fm else
                (lambda l: ops.gemv(bf.layers[l]["w_qkv"], h, bias=bf.layers[l]["b_qkv"], norm_w=bf.layers[l]["ln1"], eps=cfg.eps))),
        "o": ((lambda l: ops.gemv_w4(mx.layers[l]["w_o_q4"], mx.layers[l]["w_o_e4"], a, res=h)),
              (lambda l: ops.gemv_w8(fp8.layers[l]["w_o_q8"], fp8.layers[l]["w_o_s8"], a, res=h)),
              (lambda l: ops.gemv_fm(bf.layers[l]["w_o_fm"], a, cfg.hidden, res=h)) if fm else
              (lambda l: ops.gemv(bf.layers[l]["w_o"], a, res=h))),
        "gate_up": ((lambda l: ops.gemv_swiglu_w4(mx.layers[l]["w_gu_q4"], mx.layers[l]["w_gu_e4"], h, norm_w=mx.layers[l]["ln2"], eps=cfg.eps)),
                    (lambda l: ops.gemv_swiglu_w8(fp8.layers[l]["w_gu_q8"], fp8.layers[l]["w_gu_s8"], h, norm_w=fp8.layers[l]["ln2"], eps=cfg.eps)),
                    (lambda l: ops.gemv_swiglu_fm(bf.layers[l]["w_gu_fm"], h, norm_eps=cfg.eps)) if fm else
                    (lambda l: ops.gemv_swiglu(bf.layers[l]["w_gu"], h, norm_w=bf.layers[l]["ln2"], eps=cfg.eps))),
        "down": ((lambda l: ops.gemv_w4(mx.layers[l]["w_down_q4"], mx.layers[l]["w_down_e4"], act, res=h)),
                 (lambda l: ops.gemv_w8(fp8.layers[l]["w_down_q8"], fp8.layers[l]["w_down_s8"], act, res=h)),
                 (lambda l: ops.gemv_fm(bf.layers[l]["w_down_fm"], act, cfg.hidden, res=h)) if fm else
                 (lambda l: ops.gemv(bf.layers[l]["w_down"], act, res=h))),
    }
    for name, (f4, f8, f16) in forms.items():
        ts = [[timed(f) for f in (f16, f8, f4)] for _ in range(2)]
        t16, t8, t4 = ((ts[0][i] + ts[1][i]) / 2 for i in range(3))
        key = {"qkv": "w_qkv", "o": "w_o", "gate_up": "w_gu", "down": "w_down"}[name]
        nw = fp8.layers[0][key + "_q8"].numel()                                                  # weights = e4m3 bytes
        n4 = mx.layers[0][key + "_q4"].numel() + mx.layers[0][key + "_e4"].numel()              # nibbles + scale bytes
        say(f"rows {B} {name:8s} bf16 {'fm' if fm else 'rm'} {t16:7.1f} us ({2 * nw / t16 / 1e6:5.2f} TB/s)   fp8 {t8:7.1f} us "
            f"({nw / t8 / 1e6:5.2f} TB/s)   mxfp4 {t4:7.1f} us ({n4 / t4 / 1e6:5.2f} TB/s)   fp8 / bf16 = {t8 / t16:.3f}   "
            f"mxfp4 / bf16 = {t4 / t16:.3f}   mxfp4 / fp8 = {t4 / t8:.3f}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
sys.exit(0)

"""What batched_weight_stream=True buys per decode step at 4 / 5 / 6 / 8 rows (Qwen2.5-7B shapes, context 1536, max_batch 8), on the
method of scripts/exp/mxfp4_decode_cost.py: the captured decode step of an FP8 and of an MXFP4 engine built with the keyword -- the
quantised bytes through the fragment-major MFMA kernels of csrc/gemv_qfm.hip (rmsnorm -> gemv_fm_w* -> attention -> gemv_fm_w* ->
rmsnorm -> gemv_swiglu_fm_w* -> gemv_fm_w*) -- against the captured step of a bf16 engine on the fragment-major bf16 route of the same
row count. The three engines live in one process and are alternated, ROUNDS rounds; every round times T single graph replays with
device events and reports their median and quartiles; the figure per row count is the median of the round medians. By the keep /
reject rule of DESIGN.md section 5 a difference below 3 % is no difference: FP8_FM_MAX_ROWS / MXFP4_FM_MAX_ROWS is the largest row
count <= DECODE_ROWS up to which EVERY measured row count above the row-major range (FP8_MAX_ROWS / MXFP4_MAX_ROWS) beats the bf16
step by >= 3 %, 0 when the first one does not. Row counts inside the row-major range run the row-major kernels here too (MXFP4 at 4
rows) and are printed for reference.

Second part (alone with --ops-only): the four projections by themselves at the same row counts, captured launches cycling through
the 28 layers' weights, so no launch finds its weights in the Infinity Cache; microseconds and weight bytes per second.

    timeout -k 10 900 python scripts/exp/qfm_decode_cost.py --out profiles/qfm_decode_cost.txt
    timeout -k 10 600 python scripts/exp/qfm_decode_cost.py --ops-only --out profiles/qfm_decode_cost_ops.txt
(each GPU step under a time limit of its own; profiles/qfm_decode_cost.txt holds both reports)"""
import argparse
import os
import statistics
import sys

import torch

from spider_amd import ops
from spider_amd.llm import LlamaEngine, LLMConfig

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--rows", default="4,5,6,8")
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


ENG = {"bf16": LlamaEngine.random_init(cfg, dev, max_batch=8, max_len=CTX + 160, seed=0)}
for name in ("fp8", "mxfp4"):
    ENG[name] = LlamaEngine.random_init(cfg, dev, max_batch=8, max_len=CTX + 160, seed=0, weight_dtype=name, batched_weight_stream=True)
ENG["fp8"].FP8_FM_MAX_ROWS = ENG["mxfp4"].MXFP4_FM_MAX_ROWS = LlamaEngine.DECODE_ROWS     # measure every row count, whatever the class defaults are
say(f"engines: bf16 fm_batch={ENG['bf16'].fm_batch} FM_MIN_BATCH={ENG['bf16'].FM_MIN_BATCH}; fp8 row-major <= {ENG['fp8'].FP8_MAX_ROWS} rows, "
    f"mxfp4 row-major <= {ENG['mxfp4'].MXFP4_MAX_ROWS} rows, fragment-major above; SPIDER_QFM_D={os.environ.get('SPIDER_QFM_D', 'default')}; "
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


def route(name, B):
    rm = ENG[name].FP8_MAX_ROWS if name == "fp8" else ENG[name].MXFP4_MAX_ROWS
    return "row-major" if B <= rm else "fragment-major"


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
    say(f"rows {B}: bf16 (fragment-major) {m['bf16']:.1f} us (rounds {min(med['bf16']):.1f} .. {max(med['bf16']):.1f}), "
        f"fp8 ({route('fp8', B)}) {m['fp8']:.1f} us (rounds {min(med['fp8']):.1f} .. {max(med['fp8']):.1f}), "
        f"mxfp4 ({route('mxfp4', B)}) {m['mxfp4']:.1f} us (rounds {min(med['mxfp4']):.1f} .. {max(med['mxfp4']):.1f}); "
        f"fp8 / bf16 = {m['fp8'] / m['bf16']:.3f}, mxfp4 / bf16 = {m['mxfp4'] / m['bf16']:.3f}")
    table.append((B, m["bf16"], m["fp8"], m["mxfp4"]))

if table:
    say("")
    say("| rows | bf16 us / step | fp8 us / step (route) | mxfp4 us / step (route) | fp8 / bf16 | mxfp4 / bf16 |")
    say("|---|---|---|---|---|---|")
    for B, mb, m8, m4 in table:
        say(f"| {B} | {mb:.0f} | {m8:.0f} ({route('fp8', B)}) | {m4:.0f} ({route('mxfp4', B)}) | {m8 / mb:.3f} | {m4 / mb:.3f} |")
    for name, col in (("fp8", 2), ("mxfp4", 3)):
        best = 0
        for row in table:
            if route(name, row[0]) == "row-major":
                continue
            if row[col] > 0.97 * row[1]:
                break
            best = row[0]
        say(f"{name}: every measured fragment-major row count up to {best} beats the bf16 step of the same row count by >= 3 % "
            f"-> {name.upper()}_FM_MAX_ROWS = {best}")

# ---- the projections alone, weights cold (a different layer per launch)
if args.ops_only:
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
        h, a, act = bfl(B, cfg.hidden), bfl(B, cfg.n_q * cfg.head_dim), bfl(B, cfg.inter)
        nq = bf.layers[0]["w_qkv"].shape[0]
        # the bf16 forms fold the RMSNorm (their weights carry it); the quantised forms read normalised rows, as in the engine's step
        forms = {
            "qkv": ((lambda l: ops.gemv_fm_w4(mx.layers[l]["w_qkv_q4fm"], mx.layers[l]["w_qkv_e4fm"], h, nq, bias=mx.layers[l]["b_qkv"])),
                    (lambda l: ops.gemv_fm_w8(fp8.layers[l]["w_qkv_q8fm"], fp8.layers[l]["w_qkv_s8"], h, nq, bias=fp8.layers[l]["b_qkv"])),
                    (lambda l: ops.gemv_fm(bf.layers[l]["w_qkv_fm"], h, nq, bias=bf.layers[l]["b_qkv"], norm_eps=cfg.eps))),
            "o": ((lambda l: ops.gemv_fm_w4(mx.layers[l]["w_o_q4fm"], mx.layers[l]["w_o_e4fm"], a, cfg.hidden, res=h)),
                  (lambda l: ops.gemv_fm_w8(fp8.layers[l]["w_o_q8fm"], fp8.layers[l]["w_o_s8"], a, cfg.hidden, res=h)),
                  (lambda l: ops.gemv_fm(bf.layers[l]["w_o_fm"], a, cfg.hidden, res=h))),
            "gate_up": ((lambda l: ops.gemv_swiglu_fm_w4(mx.layers[l]["w_gu_q4fm"], mx.layers[l]["w_gu_e4fm"], h)),
                        (lambda l: ops.gemv_swiglu_fm_w8(fp8.layers[l]["w_gu_q8fm"], fp8.layers[l]["w_gu_s8"], h)),
                        (lambda l: ops.gemv_swiglu_fm(bf.layers[l]["w_gu_fm"], h, norm_eps=cfg.eps))),
            "down": ((lambda l: ops.gemv_fm_w4(mx.layers[l]["w_down_q4fm"], mx.layers[l]["w_down_e4fm"], act, cfg.hidden, res=h)),
                     (lambda l: ops.gemv_fm_w8(fp8.layers[l]["w_down_q8fm"], fp8.layers[l]["w_down_s8"], act, cfg.hidden, res=h)),
                     (lambda l: ops.gemv_fm(bf.layers[l]["w_down_fm"], act, cfg.hidden, res=h))),
            "rmsnorm": ((lambda l: ops.rmsnorm(h, mx.layers[l]["ln1"], cfg.eps)),) * 3,
        }
        for name, (f4, f8, f16) in forms.items():
            ts = [[timed(f) for f in (f16, f8, f4)] for _ in range(2)]
            t16, t8, t4 = ((ts[0][i] + ts[1][i]) / 2 for i in range(3))
            if name == "rmsnorm":
                say(f"rows {B} rmsnorm  {t16:7.1f} us per launch (two per layer in the quantised step, none in the bf16 step)")
                continue
            key = {"qkv": "w_qkv", "o": "w_o", "gate_up": "w_gu", "down": "w_down"}[name]
            nw = fp8.layers[0][key + "_q8fm"].numel()                                                  # e4m3 bytes (padded rows included)
            n4 = mx.layers[0][key + "_q4fm"].numel() + mx.layers[0][key + "_e4fm"].numel()            # nibbles + scale bytes
            say(f"rows {B} {name:8s} bf16 fm {t16:7.1f} us ({2 * nw / t16 / 1e6:5.2f} TB/s)   fp8 fm {t8:7.1f} us "
                f"({nw / t8 / 1e6:5.2f} TB/s)   mxfp4 fm {t4:7.1f} us ({n4 / t4 / 1e6:5.2f} TB/s)   fp8 / bf16 = {t8 / t16:.3f}   "
                f"mxfp4 / bf16 = {t4 / t16:.3f}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
sys.exit(0)

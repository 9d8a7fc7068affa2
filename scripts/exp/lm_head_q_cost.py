"""What lm_head_dtype="fp8" / "mxfp4" buys per decode step (Qwen2.5-7B shapes, context 1536, rows 1 / 2 / 3 / 4), on the method of
scripts/exp/mxfp4_decode_cost.py.

First part (alone with --ops-only; needs no engine): the lm_head launch by itself -- final RMSNorm + [152064, 3584] head + arg-max --
for the heads bf16 / fp8 / mxfp4. The bf16 route of the same row count is the comparison: row-major (lm_head_argmax) at 1 row,
fragment-major (lm_head_argmax_fm) from 2 rows. Captured launches cycle through COPIES copies of the head (1.09 GB of bf16, 0.55 GB
of e4m3, 0.31 GB of MXFP4 each, against the 256 MB of the Infinity Cache), so no launch finds its weights there. SPIDER_LMQ_R
(2 / 4 / 8 vocabulary rows per wave iteration of csrc/lm_head_wq.hip) is read by the library once per process: run this part once
per value to compare the forms.

Second part: the whole captured decode step under weight_dtype bf16 / fp8 / mxfp4. One engine per weight_dtype carries all three
encodings of its head (W_eff of the MXFP4 head as the bf16 matrix -- timing does not depend on values); the head is switched with
lm_head_dtype and each (weight_dtype, head) pair keeps its own states and graphs. The nine configurations are alternated in one
process, ROUNDS rounds; every round times T single graph replays with device events and reports their median and quartiles; the
figure per row count is the median of the round medians. By the keep / reject rule of DESIGN.md section 5 a difference below 3 % is
no difference: LM_HEAD_FP8_MAX_ROWS / LM_HEAD_MXFP4_MAX_ROWS are the largest row counts at which the step with the quantised head
beats the step with the bf16 head (same weight_dtype, same rows) by >= 3 % under weight_dtype="mxfp4", where the head's share is
largest.

    python scripts/exp/lm_head_q_cost.py [--out FILE] [--rows 1,2,3,4] [--ops-only] [--weights bf16,fp8,mxfp4]"""
import argparse
import os
import statistics
import sys

import torch

from spider_amd import ops
from spider_amd.llm import LlamaEngine, LLMConfig, dequantize_mxfp4, quantize_fp8_rows

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--rows", default="1,2,3,4")
ap.add_argument("--ops-only", action="store_true", help="skip the decode steps, time the lm_head launch alone")
ap.add_argument("--weights", default="bf16,fp8,mxfp4", help="weight_dtype values of the decode-step part")
args = ap.parse_args()

dev = torch.device("cuda:0")
cfg = LLMConfig.qwen25_7b()
CTX, T, ROUNDS, COPIES = 1536, 96, 3, 4
ROWS = [int(r) for r in args.rows.split(",")]
HEADS = ("bf16", "fp8", "mxfp4")
LINES = []
BF = torch.bfloat16


def say(s):
    print(s, flush=True)
    LINES.append(s)


def quart(xs):
    q = statistics.quantiles(xs, n=4)
    return q[1], q[0], q[2]


say(f"lm_head [{cfg.vocab}, {cfg.hidden}]; SPIDER_LMQ_R={os.environ.get('SPIDER_LMQ_R', '(default)')}; {T} replays per round, {ROUNDS} rounds")

# ---- the lm_head launch alone, weights cold (a different copy of the head per launch). Random bytes: every byte pattern is a finite
# weight in both formats but e4m3's two NaN codes, which are cleared; scale bytes 117 .. 127 keep the logits finite.
V, H = cfg.vocab, cfg.hidden
g = torch.Generator(device=dev).manual_seed(0)
rnd = lambda *s: torch.randint(0, 256, s, generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
q4 = [rnd(V, H // 2) for _ in range(COPIES)]
e4 = [(117 + rnd(V, H // 32) % 11).to(torch.uint8) for _ in range(COPIES)]
q8, s8, w16, wfm = [], [], [], []
norm = (1 + 0.1 * torch.randn(H, device=dev, generator=g)).to(BF)
for c in range(COPIES):
    w = dequantize_mxfp4(q4[c], e4[c])
    w16.append(w)
    wfm.append(ops.repack_fm16(w, norm))
    q, s = quantize_fp8_rows(w)
    q8.append(q.contiguous())
    s8.append(s.contiguous())
    del w, q, s


def timed(fn, reps):
    """us per launch: one pass through the copies captured in a graph, `reps` timed replays; median and quartiles over the replays"""
    fn(0)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for c in range(COPIES):
                fn(c)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(reps):
        graph.replay()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return quart([ev[i].elapsed_time(ev[i + 1]) * 1e3 / COPIES for i in range(reps)])


for B in ROWS:
    x = torch.randn(B, H, device=dev, generator=g).to(BF)
    npart = ops.lm_head_nparts(V)
    ws = (torch.empty(B * npart, dtype=torch.float32, device=dev), torch.empty(B * npart, dtype=torch.int32, device=dev))
    ids = torch.empty(B, dtype=torch.int32, device=dev)
    lg = torch.empty(B, V, dtype=BF, device=dev)
    fm = B >= LlamaEngine.FM_MIN_BATCH
    assert ops.w8_norm_fits(B, H) and ops.w4_norm_fits(B, H)
    for logits in (None, lg):
        f16 = (lambda c: ops.lm_head_argmax_fm(wfm[c], x, V, out_ids=ids, ws=ws, logits=logits, norm_eps=cfg.eps)) if fm else \
            (lambda c: ops.lm_head_argmax(w16[c], x, norm_w=norm, eps=cfg.eps, out_ids=ids, ws=ws, logits=logits))
        f8 = lambda c: ops.lm_head_argmax_w8(q8[c], s8[c], x, norm_w=norm, eps=cfg.eps, out_ids=ids, ws=ws, logits=logits)
        f4 = lambda c: ops.lm_head_argmax_w4(q4[c], e4[c], x, norm_w=norm, eps=cfg.eps, out_ids=ids, ws=ws, logits=logits)
        res = {}
        for name, f in (("bf16", f16), ("fp8", f8), ("mxfp4", f4)):
            meds = [timed(f, 24) for _ in range(ROUNDS)]
            res[name] = (statistics.median(m[0] for m in meds), min(m[1] for m in meds), max(m[2] for m in meds))
        nb = {"bf16": 2 * V * H, "fp8": V * H + 4 * V, "mxfp4": V * H // 2 + V * H // 32}
        say(f"rows {B} lm_head launch{' + logits' if logits is not None else '         '}: " + "   ".join(
            f"{n} {'fm' if (fm and n == 'bf16') else 'rm'} {res[n][0]:6.1f} us [{res[n][1]:.1f}, {res[n][2]:.1f}] ({nb[n] / res[n][0] / 1e6:4.2f} TB/s)"
            for n in HEADS) + f"   fp8 / bf16 = {res['fp8'][0] / res['bf16'][0]:.3f}   mxfp4 / bf16 = {res['mxfp4'][0] / res['bf16'][0]:.3f}")
del q4, e4, q8, s8, w16, wfm
torch.cuda.empty_cache()


# ---- the captured decode step
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


table = {}
for wd in ([] if args.ops_only else args.weights.split(",")):
    eng = LlamaEngine.random_init(cfg, dev, max_batch=4, max_len=CTX + 160, seed=0, weight_dtype=wd, lm_head_dtype="mxfp4")
    eng.lm_head_q8, eng.lm_head_s8 = (t.contiguous() for t in quantize_fp8_rows(eng.lm_head))      # the third encoding, beside the two
    eng.FP8_MAX_ROWS, eng.MXFP4_MAX_ROWS = ops.W8_MAX_ROWS, ops.W4_MAX_ROWS     # every row count the kernels exist for
    eng.LM_HEAD_FP8_MAX_ROWS = eng.LM_HEAD_MXFP4_MAX_ROWS = ops.LM_HEAD_Q_MAX_ROWS
    graphs = {hd: {} for hd in HEADS}

    def use(hd):
        eng.lm_head_dtype, eng._graphs = hd, graphs[hd]
    for B in ROWS:
        ids = torch.randint(3, cfg.vocab, (B, CTX), generator=torch.Generator().manual_seed(B))
        for hd in HEADS:     # warm-up: kernels loaded, graphs captured
            use(hd)
            replays(eng, B, ids)
        med = {hd: [] for hd in HEADS}
        for r in range(ROUNDS):
            for hd in HEADS:
                use(hd)
                m, lo, hi = quart(replays(eng, B, ids))
                med[hd].append(m)
                say(f"weights {wd:5s} rows {B} round {r} head {hd:5s} step median {m:8.1f} us  quartiles [{lo:.1f}, {hi:.1f}]")
        m = {hd: statistics.median(med[hd]) for hd in HEADS}
        route = "fragment-major" if (eng.fm_batch and B >= eng.FM_MIN_BATCH) else "row-major"
        say(f"weights {wd} rows {B}: head bf16 ({route}) {m['bf16']:.1f} us (rounds {min(med['bf16']):.1f} .. {max(med['bf16']):.1f}), "
            f"fp8 {m['fp8']:.1f} us (rounds {min(med['fp8']):.1f} .. {max(med['fp8']):.1f}), "
            f"mxfp4 {m['mxfp4']:.1f} us (rounds {min(med['mxfp4']):.1f} .. {max(med['mxfp4']):.1f}); "
            f"fp8 / bf16 = {m['fp8'] / m['bf16']:.3f}, mxfp4 / bf16 = {m['mxfp4'] / m['bf16']:.3f}")
        table[(wd, B)] = (route, m["bf16"], m["fp8"], m["mxfp4"])
    del eng, graphs
    torch.cuda.empty_cache()

if table:
    say("")
    say("| weight_dtype | rows | bf16 head route | bf16 head us / step | fp8 head us / step | mxfp4 head us / step | fp8 / bf16 | mxfp4 / bf16 |")
    say("|---|---|---|---|---|---|---|---|")
    for (wd, B), (route, mb, m8, m4) in table.items():
        say(f"| {wd} | {B} | {route} | {mb:.0f} | {m8:.0f} | {m4:.0f} | {m8 / mb:.3f} | {m4 / mb:.3f} |")
    for wd in sorted({k[0] for k in table}):
        w8 = [B for (w, B), (_, mb, m8, _) in table.items() if w == wd and m8 <= 0.97 * mb]
        w4 = [B for (w, B), (_, mb, _, m4) in table.items() if w == wd and m4 <= 0.97 * mb]
        say(f"weights {wd}: the fp8 head beats the bf16 head of the same row count by >= 3 % at rows {w8}, the mxfp4 head at rows {w4}")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
sys.exit(0)

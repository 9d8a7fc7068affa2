"""What LlamaEngine.score costs beyond the prompt pass, and what the row kernel of csrc/logprob.hip reaches (Qwen2.5-7B shapes).

First part (alone with --ops-only; needs no engine): ops.logprob_rows on bf16 logits [1024, 152064] (311 MB, above the 256 MB of the
Infinity Cache), without and with logits_ref (622 MB read). The two configurations are alternated in one process, ROUNDS rounds of
T launches timed with device events; the figure is the median of the round medians, as achieved bytes per second
(2 or 4 bytes per logit; the outputs are 24 bytes per row).

Second part: one engine, B = 1, S = 1536: `score` (prompt pass + chunks of final RMSNorm, lm_head GEMM into the bf16 scratch, row
kernel) against the prompt pass alone (`_score_logits`), alternated, ROUNDS rounds of T calls each, every call timed with device
events around it; and the same for the chunk loop's two launches by themselves on one 1024-row chunk, which is the write + re-read
of the logits that a log-sum-exp fused into the GEMM epilogue would save.

    python scripts/exp/score_cost.py [--out FILE] [--ops-only]"""
import argparse
import statistics
import sys

import torch

from spider_amd import ops
from spider_amd.llm import LlamaEngine, LLMConfig

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--ops-only", action="store_true", help="time the row kernel alone")
args = ap.parse_args()

dev = torch.device("cuda:0")
cfg = LLMConfig.qwen25_7b()
BF = torch.bfloat16
ROUNDS = 3
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps):
    """ms per call, median and quartiles over `reps` calls, each between two device events"""
    fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    torch.cuda.synchronize()
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    q = statistics.quantiles([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)], n=4)
    return q[1], q[0], q[2]


def alternate(configs, reps):
    """configs: name -> fn; ROUNDS rounds, the configurations in turn; -> name -> (median of round medians, min, max of them)"""
    for fn in configs.values():
        fn()
    meds = {n: [] for n in configs}
    for r in range(ROUNDS):
        for n, fn in configs.items():
            m, lo, hi = timed(fn, reps)
            meds[n].append(m)
            say(f"  round {r} {n:28s} median {m * 1e3:10.1f} us  quartiles [{lo * 1e3:.1f}, {hi * 1e3:.1f}]")
    return {n: (statistics.median(v), min(v), max(v)) for n, v in meds.items()}


# ---- the row kernel alone
ROWS, V = 1024, cfg.vocab
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(ROWS, V, device=dev, generator=g).to(BF)
y = (x.float() + 0.5 * torch.randn(ROWS, V, device=dev, generator=g)).to(BF)
tg = torch.randint(0, V, (ROWS,), device=dev, generator=g, dtype=torch.int32)
say(f"logprob_rows on [{ROWS}, {V}] bf16, N(0, 1) logits; {ROUNDS} rounds of 40 launches")
res = alternate({"logprob_rows": lambda: ops.logprob_rows(x, tg), "logprob_rows + logits_ref": lambda: ops.logprob_rows(x, tg, logits_ref=y)}, 40)
for n, nbytes in (("logprob_rows", 2 * ROWS * V), ("logprob_rows + logits_ref", 4 * ROWS * V)):
    m, lo, hi = res[n]
    say(f"{n}: {m * 1e3:.1f} us (rounds {lo * 1e3:.1f} .. {hi * 1e3:.1f}) = {nbytes / m / 1e9:.2f} TB/s of logits read")
del y

# ---- one chunk of the score loop, and score against the prompt pass
if not args.ops_only:
    S = 1536
    eng = LlamaEngine.random_init(cfg, dev, max_batch=1, max_len=S + 32, seed=0)
    ids = torch.randint(3, V, (1, S), generator=torch.Generator().manual_seed(1))
    h = torch.randn(ROWS, cfg.hidden, device=dev, generator=g).to(BF)
    out = torch.empty(ROWS, V, dtype=BF, device=dev)
    W, _ = eng._score_head()
    say(f"one chunk of {ROWS} rows: final RMSNorm + lm_head GEMM [{ROWS}, {cfg.hidden}] x [{V}, {cfg.hidden}]^T "
        f"({2 * ROWS * V * cfg.hidden / 1e12:.2f} TFLOP) into the bf16 scratch, then the row kernel; 10 calls per round")
    res = alternate({"rmsnorm + gemm": lambda: ops.gemm(ops.rmsnorm(h, eng.norm, cfg.eps), W, out=out),
                     "rmsnorm + gemm + logprob_rows": lambda: ops.logprob_rows(ops.gemm(ops.rmsnorm(h, eng.norm, cfg.eps), W, out=out), tg)}, 10)
    a, b = res["rmsnorm + gemm"][0], res["rmsnorm + gemm + logprob_rows"][0]
    say(f"chunk: GEMM {a * 1e3:.0f} us ({2 * ROWS * V * cfg.hidden / a / 1e9:.0f} TFLOP/s), with the row kernel {b * 1e3:.0f} us: the kernel and "
        f"its re-read of the logits are {100 * (b - a) / b:.1f} % of the chunk (the write is inside the GEMM time)")
    say(f"score at B = 1, S = {S} against the prompt pass alone; 4 calls per round")
    res = alternate({"prompt pass": lambda: eng._score_logits(ids, None, None, None, 1, S, 0),
                     "score": lambda: eng.score(input_ids=ids)}, 4)
    p, s = res["prompt pass"][0], res["score"][0]
    say(f"prompt pass {p:.2f} ms (rounds {res['prompt pass'][1]:.2f} .. {res['prompt pass'][2]:.2f}), score {s:.2f} ms "
        f"(rounds {res['score'][1]:.2f} .. {res['score'][2]:.2f}): + {s - p:.2f} ms = {100 * (s - p) / p:.1f} % for the head, the row kernel "
        f"and the host-side assembly of the result (one device -> host read of the token count)")

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
sys.exit(0)

"""What a prompt-lookup verify step costs and what it can buy (Qwen2.5-7B shapes, context 1536, one sequence): the captured plain
decode step (1 row) against the captured verify step of prompt_lookup_num_tokens = R - 1 at R = 2, 3, 4, 6, 8 rows -- the engine's
R-row weight streams, rope_kv_append(S = R), attn_verify, the R-row lm_head and spec_advance_draft -- on a bf16 engine and, with
--engines, on the opt-in FP8 / MXFP4 engines (batched_weight_stream=True, so that every row count streams the quantised bytes). The
method is that of scripts/exp/fp8_decode_cost.py: all configurations live in one process and are alternated, ROUNDS rounds; every round
times T single graph replays with device events and reports their median and quartiles; the figure per configuration is the median
of the round medians. The time of a verify step does not depend on how many drafts are accepted (the cursors move, the work does
not), so random weights serve.

From those: the break-even acceptance per step, t_R / t_1 - 1 -- a verify step yields 1 + a tokens where the plain step yields 1,
so it pays when the mean number of accepted drafts per step exceeds that.

Second part, the ceiling: the embeddings and the lm_head of the same full-size engine are rewritten into a successor model (the
greedy token behind v is the next id of v's block of 7, tests/prompt_lookup_cases.py at full size), on which greedy decoding cycles
and, once the cycle is in the history, every draft is accepted. Tokens per second of the decode loop (prompt pass excluded, host
checks every 8 steps) with and without the keyword, and the counters the device kept. This is the most the step can give, NOT a
figure for real text: the speed-up there is (1 + mean accepted per step) * t_1 / t_R at an acceptance rate that depends on the
model and the prompt, and no checkpoint here can provide one.

    PYTHONPATH=. python scripts/exp/prompt_lookup_cost.py [--out FILE] [--rows 2,3,4,6,8] [--engines bf16,fp8,mxfp4] [--new 448]"""
import argparse
import statistics
import sys
import time

import torch

from spider_amd.llm import LlamaEngine, LLMConfig

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--rows", default="2,3,4,6,8")
ap.add_argument("--engines", default="bf16")
ap.add_argument("--new", type=int, default=448, help="tokens generated per run of the ceiling part")
args = ap.parse_args()

dev = torch.device("cuda:0")
cfg = LLMConfig.qwen25_7b()
CTX, T, ROUNDS = 1536, 96, 3
ROWS = [int(r) for r in args.rows.split(",")]
MAX_LEN = CTX + 1024        # the timed replays move the cursors by up to 8 slots each: 8 + 100 * 8 + 7 < 1024
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def make(name):
    kw = {} if name == "bf16" else dict(weight_dtype=name, batched_weight_stream=True)
    return LlamaEngine.random_init(cfg, dev, max_batch=8, max_len=MAX_LEN, seed=0, **kw)


ENG = {name: make(name) for name in args.engines.split(",")}
say(f"engines {list(ENG)} (max_batch 8: bf16 rows >= {LlamaEngine.FM_MIN_BATCH} fragment-major; fp8 / mxfp4 with batched_weight_stream); "
    f"context {CTX}, {T} replays per round, {ROUNDS} rounds")
ids = torch.randint(3, cfg.vocab, (1, CTX), generator=torch.Generator().manual_seed(1))


def replays(eng, R):
    """prompt pass + a few steps (state set, graph captured on the first call), then T timed replays of the step's graph"""
    if R == 1:
        eng.generate(input_ids=ids, max_new_tokens=8, eos_token_id=[])
        graph = eng._graphs[eng._state_key(1, False, False, 0)][1]
    else:
        eng.generate(input_ids=ids, max_new_tokens=8, eos_token_id=[], prompt_lookup_num_tokens=R - 1)
        graph = eng._graphs[eng._state_key(1, False, False, 0, lookup=R - 1)][1]
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


CONF = [(name, R) for name in ENG for R in [1] + ROWS]
for name, R in CONF:        # warm-up: kernels loaded, graphs captured
    replays(ENG[name], R)
med = {c: [] for c in CONF}
for r in range(ROUNDS):
    for c in CONF:
        m, lo, hi = quart(replays(ENG[c[0]], c[1]))
        med[c].append(m)
        say(f"round {r} {c[0]:5s} rows {c[1]} step median {m:8.1f} us  quartiles [{lo:.1f}, {hi:.1f}]")
step = {c: statistics.median(med[c]) for c in CONF}
say("")
say("| engine | rows R | us / step | rounds | t_R / t_1 | break-even accepted drafts / step | ceiling tokens / step-time = R * t_1 / t_R |")
say("|---|---|---|---|---|---|---|")
for name, R in CONF:
    t1, tR = step[(name, 1)], step[(name, R)]
    kind = "plain" if R == 1 else f"verify K={R - 1}"
    say(f"| {name} | {R} ({kind}) | {tR:.0f} | {min(med[(name, R)]):.0f} .. {max(med[(name, R)]):.0f} | {tR / t1:.3f} | "
        f"{'-' if R == 1 else f'{tR / t1 - 1:.3f}'} | {'-' if R == 1 else f'{R * t1 / tR:.2f}'} |")
for name in ENG:
    never = [R for R in ROWS if R * step[(name, 1)] / step[(name, R)] <= 1.0]
    say(f"{name}: verify steps that cannot beat the plain step even at full acceptance: {never or 'none'}")

# ---- the ceiling: a successor model at full size, every draft accepted once the cycle is in the history
say("")
V, H = cfg.vocab, cfg.hidden
v = torch.arange(V, device=dev)
b0 = 3 + (v - 3).div(7, rounding_mode="floor") * 7
pred = b0 + (v - b0 - 1) % 7                       # succ(pred[u]) = u inside complete blocks of 7 that start at id 3
valid = (v >= 3) & (b0 + 6 < V)
E = (torch.randn(V, H, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * 2.0).to(torch.bfloat16)
prompt = torch.cat([ids[:, :CTX - 1], torch.tensor([[17]])], 1)
for name, eng in ENG.items():
    eng.embed_w.copy_(E)
    head = eng.lm_head.float()
    head[valid] += 0.25 * E[pred[valid]].float()
    eng.lm_head = head.to(torch.bfloat16).contiguous()
    del head
    eng._vocab_changed()        # fragment-major head rebuilt, graphs dropped
    rate = {}
    for R in [1] + ROWS:
        kw = dict(prompt_lookup_num_tokens=R - 1) if R > 1 else {}
        best = None
        for rep in range(3):        # the first run captures the graph
            hd = eng.prefill_begin(input_ids=prompt, max_new_tokens=args.new, eos_token_id=[], sync_every=8,
                                   return_dict_in_generate=True, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eng.decode_finish(hd)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                best = dt if best is None else min(best, dt)
        gen = out.sequences[0, CTX:].tolist()
        follows = sum(int(gen[i + 1] == 17 + (gen[i] - 17 + 1) % 7) for i in range(len(gen) - 1)) / max(1, len(gen) - 1)
        rate[R] = (len(gen) - 1) / best
        rec = out.prompt_lookup
        say(f"ceiling {name:5s} rows {R}: {len(gen) - 1} tokens in {best * 1e3:7.1f} ms = {rate[R]:7.1f} tokens/s "
            f"({rate[R] / rate[1]:.2f} x plain), {follows * 100:.0f} % of the tokens follow succ"
            + (f", steps {rec['steps']} drafted {rec['drafted']} accepted {rec['accepted']} "
               f"({rec['accepted'] / max(1, rec['steps']):.2f} per step)" if rec else ""))

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
sys.exit(0)

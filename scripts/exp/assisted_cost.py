"""What a round of assisted decoding costs and what it can buy (target: Qwen2.5-7B shapes; draft engine: Qwen2.5-1.5B shapes --
hidden 1536, 28 layers, 12 / 2 heads of 128, intermediate 8960, vocab 151936; context 1536, one sequence): the captured plain decode
step of the target (1 row) against the captured round of num_assistant_tokens = K at K = 1, 3, 5, 7 -- the draft engine's two-row
step, its K - 1 single-row steps, the K pushes, the target's verify step on K + 1 rows and the advance -- and, to split the round,
the captured prompt-lookup verify step of the same K + 1 rows (the round without its draft steps). The method is that of
scripts/exp/prompt_lookup_cost.py: all configurations live in one process and are alternated, ROUNDS rounds; every round times T
single graph replays with device events and reports their median and quartiles; the figure per configuration is the median of the
round medians. The time of a round does not depend on how many drafts are accepted, so random weights serve.

From those: the break-even acceptance per round, t_round / t_1 - 1 -- a round yields 1 + a tokens where the plain step yields 1.

Second part, the ceiling: both full-size engines are rewritten into successor models (tests/prompt_lookup_cases.py at full size), so
that the draft engine is always right and every draft is accepted. Tokens per second of the decode loop (both prompt passes
excluded, host checks every 8 rounds) with and without the keyword, and the counters the device kept. This is the most a round can
give, NOT a figure for real text: there the speed-up is (1 + mean accepted per round) * t_1 / t_round at an acceptance rate that
depends on the pair of models and the prompt, and no checkpoint here can provide one.

    PYTHONPATH=. python scripts/exp/assisted_cost.py [--out FILE] [--drafts 1,3,5,7] [--new 448]"""
import argparse
import statistics
import sys
import time

import torch

from spider_amd.llm import LlamaEngine, LLMConfig

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--drafts", default="1,3,5,7")
ap.add_argument("--new", type=int, default=448, help="tokens generated per run of the ceiling part")
args = ap.parse_args()

dev = torch.device("cuda:0")
cfg = LLMConfig.qwen25_7b()
# (the head is kept apart from the embeddings, unlike the checkpoint's: the ceiling part rewrites it; a step reads the same bytes)
dcfg = LLMConfig(1536, 28, 12, 2, 128, 8960, 151936, 1000000.0, None, 1e-6, True, 8192, False, None)
CTX, T, ROUNDS = 1536, 96, 3
KS = [int(k) for k in args.drafts.split(",")]
MAX_LEN = CTX + 1024        # the timed replays move the cursors by up to 8 slots each: 8 + 100 * 8 + 7 < 1024
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


eng = LlamaEngine.random_init(cfg, dev, max_batch=8, max_len=MAX_LEN, seed=0)
draft = LlamaEngine.random_init(dcfg, dev, max_batch=2, max_len=MAX_LEN, seed=1)
say(f"target Qwen2.5-7B shapes (max_batch 8: rows >= {LlamaEngine.FM_MIN_BATCH} fragment-major), draft engine Qwen2.5-1.5B shapes (max_batch 2); "
    f"bf16; context {CTX}, {T} replays per round, {ROUNDS} rounds")
ids = torch.randint(3, dcfg.vocab, (1, CTX), generator=torch.Generator().manual_seed(1))


def replays(kind, K):
    """prompt pass + a few steps (state set, graph captured on the first call), then T timed replays of the captured graph"""
    if kind == "plain":
        eng.generate(input_ids=ids, max_new_tokens=8, eos_token_id=[])
        graph = eng._graphs[eng._state_key(1, False, False, 0)][1]
    elif kind == "lookup":
        eng.generate(input_ids=ids, max_new_tokens=8, eos_token_id=[], prompt_lookup_num_tokens=K)
        graph = eng._graphs[eng._state_key(1, False, False, 0, lookup=K)][1]
    elif kind == "draft1":      # the draft engine's own plain step: what one more draft costs
        draft.generate(input_ids=ids, max_new_tokens=8, eos_token_id=[])
        graph = draft._graphs[draft._state_key(1, False, False, 0)][1]
    else:
        eng.generate(input_ids=ids, max_new_tokens=8, eos_token_id=[], assistant_model=draft, num_assistant_tokens=K)
        graph = eng._graphs[eng._state_key(1, False, False, 0, assist=K)][1]
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


CONF = [("plain", 0), ("draft1", 0)] + [(kind, K) for K in KS for kind in ("assist", "lookup")]
for c in CONF:        # warm-up: kernels loaded, graphs captured
    replays(*c)
med = {c: [] for c in CONF}
for r in range(ROUNDS):
    for c in CONF:
        m, lo, hi = quart(replays(*c))
        med[c].append(m)
        say(f"round {r} {c[0]:6s} K {c[1]} median {m:8.1f} us  quartiles [{lo:.1f}, {hi:.1f}]")
step = {c: statistics.median(med[c]) for c in CONF}
t1 = step[("plain", 0)]
say("")
say(f"plain step of the target t_1 = {t1:.0f} us (rounds {min(med[('plain', 0)]):.0f} .. {max(med[('plain', 0)]):.0f}); "
    f"plain step of the draft engine {step[('draft1', 0)]:.0f} us = {step[('draft1', 0)] / t1:.3f} t_1")
say("")
say("| K | rows of the verify step | us / round | rounds | verify step alone (prompt-lookup graph) | draft side = round - verify | t_round / t_1 "
    "| break-even accepted drafts / round | ceiling tokens / step-time = (K + 1) * t_1 / t_round |")
say("|---|---|---|---|---|---|---|---|---|")
for K in KS:
    tr, tv = step[("assist", K)], step[("lookup", K)]
    say(f"| {K} | {K + 1} | {tr:.0f} | {min(med[('assist', K)]):.0f} .. {max(med[('assist', K)]):.0f} | {tv:.0f} | {tr - tv:.0f} | {tr / t1:.3f} | "
        f"{tr / t1 - 1:.3f} | {(K + 1) * t1 / tr:.2f} |")
never = [K for K in KS if (K + 1) * t1 / step[("assist", K)] <= 1.03]
say(f"rounds that do not beat the plain step by 3 % even at full acceptance: K = {never or 'none'}")

# ---- the ceiling: two successor models at full size, the draft engine always right
say("")


def successor(e, scale=2.0):
    V, H = e.cfg.vocab, e.cfg.hidden
    v = torch.arange(V, device=dev)
    b0 = 3 + (v - 3).div(7, rounding_mode="floor") * 7
    pred = b0 + (v - b0 - 1) % 7                       # succ(pred[u]) = u inside complete blocks of 7 that start at id 3
    valid = (v >= 3) & (b0 + 6 < V)
    E = (torch.randn(V, H, device=dev, generator=torch.Generator(device=dev).manual_seed(3)) * scale).to(torch.bfloat16)
    e.embed_w.copy_(E)
    head = e.lm_head.float()
    head[valid] += 0.25 * E[pred[valid]].float()
    e.lm_head = head.to(torch.bfloat16).contiguous()
    del head
    e._vocab_changed()        # fragment-major head rebuilt, graphs dropped


successor(eng)
successor(draft)
prompt = torch.cat([ids[:, :CTX - 1], torch.tensor([[17]])], 1)
rate = {}
for K in [0] + KS:
    kw = dict(assistant_model=draft, num_assistant_tokens=K) if K else {}
    best = None
    for rep in range(3):        # the first run captures the graph
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.generate(input_ids=prompt, max_new_tokens=args.new, eos_token_id=[], sync_every=8, return_dict_in_generate=True, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep:
            best = dt if best is None else min(best, dt)
    # generate is one call for an assisted request, so the prompt passes are timed apart and taken off
    pre = None
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate(input_ids=prompt, max_new_tokens=1, eos_token_id=[])
        if K:
            draft.generate(input_ids=prompt, max_new_tokens=1, eos_token_id=[])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rep:
            pre = dt if pre is None else min(pre, dt)
    gen = out.sequences[0, CTX:].tolist()
    follows = sum(int(gen[i + 1] == 17 + (gen[i] - 17 + 1) % 7) for i in range(len(gen) - 1)) / max(1, len(gen) - 1)
    rate[K] = (len(gen) - 1) / (best - pre)
    rec = out.assisted
    say(f"ceiling K {K}: {len(gen) - 1} tokens in {(best - pre) * 1e3:7.1f} ms (call {best * 1e3:.1f} ms - prompt passes {pre * 1e3:.1f} ms) = "
        f"{rate[K]:7.1f} tokens/s ({rate[K] / rate[0]:.2f} x plain), {follows * 100:.0f} % of the tokens follow succ"
        + (f", rounds {rec['steps']} drafted {rec['drafted']} accepted {rec['accepted']} "
           f"({rec['accepted'] / max(1, rec['steps']):.2f} per round)" if rec else ""))

if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
sys.exit(0)

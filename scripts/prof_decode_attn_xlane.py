"""A/B of the two forms of the fused decode attention kernel (spider_set_attn_xlane 0 / 1) in ONE process: Qwen2.5-7B shapes,
1536-token prompt, N greedy tokens, ROUNDS alternating rounds; the captured decode graphs are dropped at each switch (a graph
replays the kernels it was captured with). Prints tok/s per round, the medians and the spread of each form's rounds.
SPIDER_GEMV_SCHED=0 in the environment takes the VALU reductions out of the GEMVs and lm_head as well (both columns then run
the shuffle GEMVs).   python scripts/prof_decode_attn_xlane.py [N] [ROUNDS]"""
import statistics
import sys
import time

import torch

from spider_amd import lib as slib
from spider_amd.llm import LlamaEngine, LLMConfig

dev = torch.device("cuda:0")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
lib = slib.load()
eng = LlamaEngine.random_init(LLMConfig.qwen25_7b(), dev, max_batch=1, max_len=2048)
ids = torch.randint(3, 150000, (1, 1536), device=dev)


def timed(k, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.generate(input_ids=ids, max_new_tokens=k, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def decode_tok_s(form):
    lib.spider_set_attn_xlane(form)
    for ent in eng._graphs.values():     # [state, captured graph]: keep the state, capture again under this form
        ent[1] = None
    eng.generate(input_ids=ids, max_new_tokens=4)          # captures
    tp = min(timed(2, use_graph=False) for _ in range(2))  # prompt pass + 2 tokens
    tg = timed(n, sync_every=n)
    return (n - 2) / (tg - tp)


prev = lib.spider_set_attn_xlane(1)
try:
    res = {0: [], 1: []}
    for r in range(rounds):
        for form in (0, 1):
            res[form].append(decode_tok_s(form))
        print(f"round {r}: xlane 0 {res[0][-1]:.1f} tok/s, xlane 1 {res[1][-1]:.1f} tok/s", flush=True)
    m0, m1 = statistics.median(res[0]), statistics.median(res[1])
    print(f"median of {rounds}: xlane 0 {m0:.1f} tok/s ({1e3 / m0:.3f} ms/token), xlane 1 {m1:.1f} tok/s ({1e3 / m1:.3f} ms/token), "
          f"ratio {m1 / m0:.4f}; spread (max - min) xlane 0 {max(res[0]) - min(res[0]):.1f}, xlane 1 {max(res[1]) - min(res[1]):.1f} tok/s")
finally:
    lib.spider_set_attn_xlane(prev)

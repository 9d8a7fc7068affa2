"""Cost of do_sample=True in the decode graph: ms per decode step of the greedy and of the sampling decode graph (Qwen2.5-7B shapes,
V = 152064, context 1536, 1 and 8 rows), both in ONE process, alternating, medians over the rounds (the rule of DESIGN section 5),
and each of the two sampling launches alone (on the state's own logits buffer, 200 launches back to back).
The sampling step runs the raw-logits lm_head instead of the arg-max one (one more [B, V] bf16 store), then reads those B * V * 2
bytes once and selects top_k candidates per 4096-token slice, one per round.

    PYTHONPATH=. python scripts/sampling_decode_cost.py [rounds] [steps per block]
    PYTHONPATH=<tree> python scripts/sampling_decode_cost.py --greedy-only [rounds] [steps]     one JSON line: greedy ms per step,
        for comparing two trees (run the processes alternately and take the median per tree)"""
import json
import statistics
import sys

import torch

from spider_amd import ops
from spider_amd.llm import LlamaEngine, LLMConfig

args = [a for a in sys.argv[1:] if not a.startswith("--")]
GREEDY_ONLY = "--greedy-only" in sys.argv
ROUNDS = int(args[0]) if len(args) > 0 else 7
STEPS = int(args[1]) if len(args) > 1 else 48
CTX = 1536
dev = torch.device("cuda:0")
cfg = LLMConfig.qwen25_7b()
eng = LlamaEngine.random_init(cfg, dev, max_batch=8, max_len=CTX + STEPS + 32, seed=0)
CURSORS = ("cur_ids", "next_ids", "pos", "slot", "kv_end", "n_hist")
SAMPLE = dict(do_sample=True, top_k=50, top_p=0.9, temperature=1.0, seed=1)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


result = {}
if not GREEDY_ONLY:
    print(f"rows  greedy ms/step (median, min..max)   sampling ms/step (median, min..max)   delta us   delta %   "
          f"partial + select alone us   [{ROUNDS} rounds x {STEPS} steps]")
for B in (1, 8):
    ids = torch.randint(3, cfg.vocab, (B, CTX), generator=torch.Generator().manual_seed(B))
    paths = {}
    for name, kw in (("greedy", {}),) + (() if GREEDY_ONLY else (("sample", SAMPLE),)):
        eng.generate(input_ids=ids, max_new_tokens=4, sync_every=4, **kw)          # prompt pass + graph capture
        h = eng.prefill_begin(input_ids=ids, max_new_tokens=4, **kw)               # cursors at the end of the prompt
        st, graph = h.st, eng._graphs[h.skey][1]
        assert graph is not None and (("sample" in st) == (name == "sample"))
        paths[name] = (st, graph, {k: st[k].clone() for k in CURSORS})
    times = {n: [] for n in paths}
    for r in range(ROUNDS + 1):                                                    # round 0 warms both
        for name in (tuple(paths) if r % 2 == 0 else tuple(paths)[::-1]):
            st, graph, snap = paths[name]
            for k, v in snap.items():
                st[k].copy_(v)
            t = timed(graph.replay, STEPS)
            if r:
                times[name].append(t)
    med = {n: statistics.median(v) for n, v in times.items()}
    result[f"greedy_ms_b{B}"] = round(med["greedy"], 5)
    if GREEDY_ONLY:
        continue
    st = paths["sample"][0]
    med_us = lambda fn: statistics.median(timed(fn, 200) for _ in range(ROUNDS)) * 1e3
    alone = (med_us(lambda: ops.sample_partial(st["logits"], st["sample"], st.get("proc"))),
             med_us(lambda: ops.sample_select(st["sample"], st["n_hist"], st["next_ids"], cfg.vocab)))
    fmt = lambda n: f"{med[n]:.4f} ({min(times[n]):.4f}..{max(times[n]):.4f})"
    d = med["sample"] - med["greedy"]
    print(f"{B:4d}  {fmt('greedy'):>35}   {fmt('sample'):>37}   {1e3 * d:8.1f}   {100 * d / med['greedy']:+7.2f}   {alone[0]:14.1f} + {alone[1]:.1f}", flush=True)
if GREEDY_ONLY:
    print(json.dumps(result), flush=True)

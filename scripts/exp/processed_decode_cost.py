"""Cost of the logits processors in the lm_head epilogue: ms per decode step of the processed and the unprocessed decode graph
(Qwen2.5-7B shapes, context 1536, 1 and 8 rows), both in ONE process, alternating, medians over the rounds (the rule of DESIGN
section 5). The processed step reads one bitmap word per vocabulary row and sequence (19 KB per sequence, L2 resident) beside the
1.09 GB lm_head stream, and its decode_advance sets one bit.

    PYTHONPATH=. python scripts/exp/processed_decode_cost.py [rounds] [steps per block]"""
import statistics
import sys

import torch

from spider_amd.llm import LlamaEngine, LLMConfig

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 48
CTX = 1536
dev = torch.device("cuda:0")
cfg = LLMConfig.qwen25_7b()
eng = LlamaEngine.random_init(cfg, dev, max_batch=8, max_len=CTX + STEPS + 32, seed=0)
CURSORS = ("cur_ids", "next_ids", "pos", "slot", "kv_end", "n_hist")

print(f"rows  unprocessed ms/step (median, min..max)   processed ms/step (median, min..max)   delta %   [{ROUNDS} rounds x {STEPS} steps]")
for B in (1, 8):
    ids = torch.randint(3, cfg.vocab, (B, CTX), generator=torch.Generator().manual_seed(B))
    paths = {}
    for name, kw in (("plain", {}), ("proc", dict(repetition_penalty=1.05, min_new_tokens=16, eos_token_id=[7, 9], suppress_tokens=[0, 1, 2]))):
        eng.generate(input_ids=ids, max_new_tokens=4, sync_every=4, **kw)          # prompt pass + graph capture
        h = eng.prefill_begin(input_ids=ids, max_new_tokens=4, **kw)               # cursors at the end of the prompt
        st, graph = h.st, eng._graphs[h.skey][1]
        assert graph is not None and (("proc" in st) == (name == "proc"))
        paths[name] = (st, graph, {k: st[k].clone() for k in CURSORS})
    times = {n: [] for n in paths}
    for r in range(ROUNDS + 1):                                                    # round 0 warms both
        for name in (("plain", "proc") if r % 2 == 0 else ("proc", "plain")):
            st, graph, snap = paths[name]
            for k, v in snap.items():
                st[k].copy_(v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(STEPS):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1) / STEPS)
    med = {n: statistics.median(v) for n, v in times.items()}
    fmt = lambda n: f"{med[n]:.4f} ({min(times[n]):.4f}..{max(times[n]):.4f})"
    print(f"{B:4d}  {fmt('plain'):>38}   {fmt('proc'):>36}   {100 * (med['proc'] / med['plain'] - 1):+.2f}", flush=True)

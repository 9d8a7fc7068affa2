"""Cost of a beam-search decode step: ms per step of the beam graph (unchanged layer stack and lm_head + partial reduction, select,
KV row reorder) against the plain batched greedy graph at the SAME row count (Qwen2.5-7B shapes, context 1536, one batch row with
K = 2 / 4 / 8 beams against K greedy rows), both in ONE process, alternating, medians over the rounds (the rule of DESIGN section 5).
Also prints how many of the K rows changed their source beam per step on this (random-weight) model: only those rows are moved.

    PYTHONPATH=. python scripts/exp/beam_decode_cost.py [rounds] [steps per block]"""
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

print(f"rows  greedy ms/step (median, min..max)   beam ms/step (median, min..max)   delta %   rows moved/step   [{ROUNDS} rounds x {STEPS} steps]")
for K in (2, 4, 8):
    ids = torch.randint(3, cfg.vocab, (K, CTX), generator=torch.Generator().manual_seed(K))
    eng.generate(input_ids=ids, max_new_tokens=4, sync_every=4)                    # prompt pass + graph capture, K greedy rows
    h = eng.prefill_begin(input_ids=ids, max_new_tokens=4)
    paths = {"greedy": (h.st, eng._graphs[h.skey][1], {k: h.st[k].clone() for k in CURSORS})}
    eng.generate(input_ids=ids[:1], max_new_tokens=8, num_beams=K, sync_every=8)   # one batch row, K beams: prompt pass + capture
    skey = eng._state_key(1, False, False, 0, False, (K, 2 * K))
    st, graph = eng._graphs[skey]
    assert graph is not None
    snap = {k: st[k].clone() for k in CURSORS}
    snap_run = st["beam"]["run"].clone()
    paths["beam"] = (st, graph, snap)
    times = {n: [] for n in paths}
    for r in range(ROUNDS + 1):                                                    # round 0 warms both
        for name in (("greedy", "beam") if r % 2 == 0 else ("beam", "greedy")):
            s, g, sn = paths[name]
            for k, v in sn.items():
                s[k].copy_(v)
            if name == "beam":
                s["beam"]["run"].copy_(snap_run)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(STEPS):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[name].append(e0.elapsed_time(e1) / STEPS)
    # rows that changed their source beam, from the last block's trace entries (no EOS id: the first K continuations run on)
    n0 = int(snap["n_hist"][0])
    src = st["beam"]["trace"][1][n0:n0 + STEPS, 0, :K].cpu()
    moved = float((src != torch.arange(K)[None]).sum()) / STEPS
    med = {n: statistics.median(v) for n, v in times.items()}
    fmt = lambda n: f"{med[n]:.4f} ({min(times[n]):.4f}..{max(times[n]):.4f})"
    print(f"{K:4d}  {fmt('greedy'):>34}   {fmt('beam'):>30}   {100 * (med['beam'] / med['greedy'] - 1):+.2f}   {moved:.2f} of {K}", flush=True)

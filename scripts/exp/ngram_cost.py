"""What no_repeat_ngram_size adds to a processed decode step (Qwen2.5-7B shapes, context 1536, 1 and 8 rows): the step of a
processed request (repetition_penalty=1.05) against the same request with no_repeat_ngram_size=3, whose closing launch also scans
the row's history (ngram_ban_kernel<ADVANCE> in place of decode_advance_seen_kernel). The request without the keyword runs the
kernels, state and graph it ran before the keyword existed, so it is the baseline. The two are alternated, three rounds; every
round times T single graph replays with device events and reports their median and quartiles. The two closing launches are also
timed alone, back to back on one stream, as the direct cost of the scan at this history length."""
import statistics
import sys

import torch

from spider_amd import ops
from spider_amd.llm import LlamaEngine, LLMConfig

dev = torch.device("cuda:0")
cfg = LLMConfig.qwen25_7b()
CTX, T, ROUNDS = 1536, 96, 3
eng = LlamaEngine.random_init(cfg, dev, max_batch=8, max_len=CTX + 160, seed=0)
KW = {"base": dict(repetition_penalty=1.05), "ngram": dict(repetition_penalty=1.05, no_repeat_ngram_size=3)}


def replays(B, ids, kw, key):
    """prompt pass + a few steps (state set, graph captured on the first call), then T timed replays of the decode graph"""
    eng.generate(input_ids=ids, max_new_tokens=8, eos_token_id=[], **kw)
    graph = eng._graphs[key][1]
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


for B in (1, 8):
    ids = torch.randint(3, cfg.vocab, (B, CTX), generator=torch.Generator().manual_seed(B))
    keys = {"base": (B, False, False, 0, True), "ngram": (B, False, False, 0, True, "ngram")}
    for name in KW:     # warm-up: kernels loaded, graphs captured
        replays(B, ids, KW[name], keys[name])
    med = {"base": [], "ngram": []}
    for r in range(ROUNDS):
        for name in ("base", "ngram"):
            m, lo, hi = quart(replays(B, ids, KW[name], keys[name]))
            med[name].append(m)
            print(f"rows {B} round {r} {name:5s} step median {m:8.1f} us  quartiles [{lo:.1f}, {hi:.1f}]", flush=True)
    mb, mn = statistics.median(med["base"]), statistics.median(med["ngram"])
    print(f"rows {B}: processed {mb:.1f} us (rounds {min(med['base']):.1f} .. {max(med['base']):.1f}), with n = 3 {mn:.1f} us "
          f"(rounds {min(med['ngram']):.1f} .. {max(med['ngram']):.1f}), difference {mn - mb:+.1f} us", flush=True)
    # the two closing launches alone, on the n-gram state as the replays left it (history ~ 8 + T tokens behind a 1536 prompt)
    st = eng._graphs[keys["ngram"]][0]
    snap = {k: st[k].clone() for k in ("cur_ids", "pos", "slot", "kv_end", "n_hist", "seen", "ban_step")}
    for name, fn in (("decode_advance_seen", lambda: ops.decode_advance_seen(st["next_ids"], st["cur_ids"], st["pos"], st["slot"], st["kv_end"],
                                                                           st["seen"], cfg.vocab, st["hist"], st["n_hist"])),
                     ("decode_advance_seen_ngram", lambda: ops.decode_advance_seen_ngram(st["next_ids"], st["cur_ids"], st["pos"], st["slot"],
                                                                                       st["kv_end"], st["seen"], cfg.vocab, st["hist"],
                                                                                       st["n_hist"], st["ngram_bufs"]))):
        K = 20      # the history has room for them (max_len = CTX + 160)
        for _ in range(3):
            fn()
        for k, v in snap.items():
            st[k].copy_(v)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(K):
            fn()
        e1.record()
        torch.cuda.synchronize()
        for k, v in snap.items():
            st[k].copy_(v)
        print(f"rows {B}: {name} alone, {K} launches back to back: {e0.elapsed_time(e1) * 1e3 / K:.2f} us per launch (launch-bound)", flush=True)
sys.exit(0)

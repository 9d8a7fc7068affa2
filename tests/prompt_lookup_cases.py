"""Shared by the prompt-lookup tests (test_prompt_lookup_cpu.py on the host, test_prompt_lookup_gpu.py on the device): the
successor model on which greedy decoding copies, host simulations of a whole prompt-lookup generation, and the cases and host
reference of the accept / draft kernels. Everything here is host code on CPU tensors."""
import functools
import random

import torch

from oracle.llama import LlamaCfg, LlamaOracle
from spider_amd.llm import prompt_lookup_draft_host, spec_accept_host

# ---------------------------------------------------------------------------------------------- the successor model
SUCC_BLOCK, SUCC_FIRST = 7, 3
C = list(range(17, 24))                                         # one block of 7: succ walks 17 -> 18 -> ... -> 23 -> 17
PROMPT = [250, 251, C[0], C[1], 260, 261, C[3], C[4], C[5], 262, 270, C[0]]
T_NEW = 40
# prompt lookup with K = 3, N = 2 on PROMPT: 14 verify steps, 26 drafts accepted; by step: 7 with every draft accepted, 4 with
# some, 1 with none, 2 that had no draft (recomputed and asserted by test_prompt_lookup_cpu.py)
K3N2 = dict(steps=14, accepted=26, full=7, partial=4, rejected=1, undrafted=2)


def succ(v: int, vocab: int = 300):
    """next id inside the block of 7 that holds v (blocks start at id 3); None outside the complete blocks"""
    if v < SUCC_FIRST or (v - SUCC_FIRST) // SUCC_BLOCK >= (vocab - SUCC_FIRST) // SUCC_BLOCK:
        return None
    b0 = SUCC_FIRST + (v - SUCC_FIRST) // SUCC_BLOCK * SUCC_BLOCK
    return b0 + (v - b0 + 1) % SUCC_BLOCK


@functools.lru_cache(maxsize=None)
def successor_model():
    """(LlamaCfg, weights): a random 2-layer GQA model at head_dim 128 whose lm_head row succ(v) carries 0.25 * the embedding of v,
    so that the greedy token behind v is succ(v) by a wide margin whatever the context adds"""
    cfg = LlamaCfg(256, 2, 4, 2, 128, 512, 300, 10000.0, None, 1e-6, False, 256)
    w = dict(LlamaOracle.random_weights(cfg, seed=31, std=0.04))
    E = (torch.randn(300, 256, generator=torch.Generator().manual_seed(3)) * 0.5).bfloat16().float()
    head = w["lm_head.weight"].clone()
    for v in range(cfg.vocab):
        if succ(v) is not None:
            head[succ(v)] += 0.25 * E[v]
    w["model.embed_tokens.weight"] = E
    w["lm_head.weight"] = head.bfloat16().float()
    return cfg, w


@functools.lru_cache(maxsize=None)
def successor_greedy(n_new: int = T_NEW + 7):
    """(tokens [n_new], minimum top-2 margin) of the fp32 oracle behind PROMPT"""
    cfg, w = successor_model()
    tok, logits = LlamaOracle(cfg, w).greedy(torch.tensor([PROMPT]), n_new, return_logits=True)
    top2 = logits[0].topk(2, -1).values
    return tuple(tok[0].tolist()), float((top2[:, 0] - top2[:, 1]).min())


def _tally(kinds, n_draft, a):
    kinds.append("undrafted" if n_draft == 0 else "rejected" if a == 0 else "full" if a == n_draft else "partial")


def _record(steps, drafted, accepted, kinds):
    return dict(steps=steps, drafted=drafted, accepted=accepted, **{k: kinds.count(k) for k in ("full", "partial", "rejected", "undrafted")})


def simulate_tokens(prompt, greedy, T, K, N):
    """Prompt-lookup generation of T tokens replayed on the host from the model's greedy continuation `greedy` (>= T + K tokens
    behind `prompt`): the model's token behind a row whose drafts so far were right is the greedy one; behind a wrong draft it is
    never looked at (-1 here). -> (tokens [T], record)"""
    hist, kinds, drafted, accepted = [greedy[0]], [], 0, 0
    while len(hist) < T:
        d = prompt_lookup_draft_host(list(prompt) + hist, K, N)
        n, ids = len(hist), [hist[-1]] + d
        lm_out, ok = [], True
        for r in range(len(ids)):
            ok = ok and (r == 0 or ids[r] == greedy[n + r - 1])
            lm_out.append(greedy[n + r] if ok else -1)
        a = spec_accept_host(ids, len(d), lm_out)
        hist += lm_out[:a + 1]
        drafted, accepted = drafted + len(d), accepted + a
        _tally(kinds, len(d), a)
    return hist[:T], _record(len(kinds), drafted, accepted, kinds)


def simulate_oracle(cfg, w, prompt, T, K, N):
    """The same generation with every verify step RUN on the fp32 oracle: the K + 1 rows go through one forward pass behind the
    KV cache of the accepted tokens, the arg-max behind every row is the model's token, and the cache is cut back to the accepted
    length. -> (tokens [T], record)"""
    oracle = LlamaOracle(cfg, w)
    S = len(prompt)
    logits, kv, _ = oracle.forward(torch.tensor([prompt]), torch.arange(S)[None], None, None)
    hist, n_ctx, kinds, drafted, accepted = [int(logits[0, -1].argmax())], S, [], 0, 0
    while len(hist) < T:
        d = prompt_lookup_draft_host(list(prompt) + hist, K, N)
        ids = [hist[-1]] + d
        logits, kv2, _ = oracle.forward(torch.tensor([ids]), n_ctx + torch.arange(len(ids))[None], kv, None)
        lm_out = logits[0].argmax(-1).tolist()
        a = spec_accept_host(ids, len(d), lm_out)
        hist += lm_out[:a + 1]
        n_ctx += a + 1
        kv = [(k[:, :, :n_ctx], v[:, :, :n_ctx]) for k, v in kv2]
        drafted, accepted = drafted + len(d), accepted + a
        _tally(kinds, len(d), a)
    return hist[:T], _record(len(kinds), drafted, accepted, kinds)


# ---------------------------------------------------------------------------------------------- accept / draft kernel cases
class SpecCase:
    """One launch of spec_advance_draft (advance=True) or prompt_lookup_draft: B sequences of R = K + 1 rows. Tensors are what the
    ops take (int32; counters int64)."""

    def __init__(self, name, prompts, hists, K, N, cap=64, pcap=40, drafts=None, lm_outs=None, advance=True, stale_ids=None):
        B, R = len(prompts), K + 1
        self.name, self.B, self.R, self.K, self.N, self.cap, self.pcap, self.advance = name, B, R, K, N, cap, pcap, advance
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
        self.prompt_ids, self.n_prompt, self.hist, self.n_hist = i32(B, pcap), i32(B), i32(B, cap), i32(B)
        self.ids, self.pos, self.slot, self.lm_out = i32(B * R), i32(B * R), i32(B * R), i32(B * R)
        self.kv_end, self.n_draft = i32(B), i32(B)
        self.counters = torch.tensor([[5, 9, 4]] * B, dtype=torch.int64)
        self.ngram, self.k_draft = torch.tensor([N], dtype=torch.int32), torch.tensor([K], dtype=torch.int32)
        for b in range(B):
            P, nh = len(prompts[b]), len(hists[b])
            self.prompt_ids[b, :P] = torch.tensor(prompts[b], dtype=torch.int32)
            self.n_prompt[b], self.n_hist[b] = P, nh
            stored = hists[b][:cap]
            self.hist[b, :len(stored)] = torch.tensor(stored, dtype=torch.int32)
            d = list(drafts[b]) if drafts else []
            row = [hists[b][-1]] + d
            row += (list(stale_ids[b]) if stale_ids else [hists[b][-1]] * R)[len(row):R]
            self.ids[b * R:(b + 1) * R] = torch.tensor(row, dtype=torch.int32)
            self.n_draft[b] = len(d)
            self.pos[b * R:(b + 1) * R] = 100 * b + 7 + P + nh - 1 + torch.arange(R)
            self.slot[b * R:(b + 1) * R] = P + nh - 1 + torch.arange(R)
            self.kv_end[b] = P + nh
            if lm_outs:
                self.lm_out[b * R:(b + 1) * R] = torch.tensor(list(lm_outs[b]), dtype=torch.int32)

    def __repr__(self):
        return self.name

    OUTPUTS = ("hist", "n_hist", "ids", "pos", "slot", "kv_end", "n_draft", "counters")

    def expected(self) -> dict:
        """every output buffer after the launch, by the host restatements"""
        B, R, K, cap = self.B, self.R, self.K, self.cap
        o = {k: getattr(self, k).clone() for k in self.OUTPUTS}
        for b in range(B):
            P, nh = int(self.n_prompt[b]), int(self.n_hist[b])
            row, lm = self.ids[b * R:(b + 1) * R].tolist(), self.lm_out[b * R:(b + 1) * R].tolist()
            last, adv = row[0], 0
            if self.advance:
                nd = min(max(int(self.n_draft[b]), 0), K)
                a = spec_accept_host(row, nd, lm)
                for j, t in enumerate(lm[:a + 1]):
                    if nh + j < cap:
                        o["hist"][b, nh + j] = t
                last, adv = lm[a], a + 1
                o["n_hist"][b] = nh + adv
                o["kv_end"][b] += adv
                o["counters"][b] += torch.tensor([1, nd, a])
            nh += adv
            seq = self.prompt_ids[b, :P].tolist() + [int(o["hist"][b, j]) if j < cap else -1 for j in range(nh)]
            d = prompt_lookup_draft_host(seq, K, self.N)
            o["n_draft"][b] = len(d)
            o["ids"][b * R:(b + 1) * R] = torch.tensor([last] + d + [last] * (R - 1 - len(d)), dtype=torch.int32)
            o["pos"][b * R:(b + 1) * R] = int(self.pos[b * R]) + adv + torch.arange(R)
            o["slot"][b * R:(b + 1) * R] = int(self.slot[b * R]) + adv + torch.arange(R)
        return o


def random_spec_cases(K, seed=0):
    """alphabet of 5, B = 2, P in {0, 1, 37}, n_hist in {1, 2, 50}, N in {1, 2, 3}; drafts and model tokens agree 70 % of the time"""
    rng = random.Random(1000 * seed + K)
    A = lambda n: [rng.randrange(5) for _ in range(n)]
    out = []
    for P in (0, 1, 37):
        for nh in (1, 2, 50):
            for N in (1, 2, 3):
                for advance in (True, False):
                    prompts, hists = [A(P), A(P)], [A(nh), A(nh)]
                    drafts = [A(rng.randrange(K + 1)) for _ in range(2)]
                    lm_outs = []
                    for b in range(2):
                        row = [hists[b][-1]] + drafts[b] + [hists[b][-1]] * (K + 1)
                        lm_outs.append([row[r + 1] if rng.random() < 0.7 else rng.randrange(5) for r in range(K + 1)])
                    out.append(SpecCase(f"rand-K{K}-P{P}-h{nh}-N{N}-{'adv' if advance else 'draft'}", prompts, hists, K, N,
                                        drafts=drafts if advance else None, lm_outs=lm_outs if advance else None, advance=advance))
    return out


def named_spec_cases():
    c = []
    for adv in (False, True):
        t = "adv" if adv else "draft"
        # the advance forms reach the same sequence by appending its last token: a step without drafts whose model token it is
        mk = lambda name, prompt, hist, K, N: c.append(SpecCase(
            f"{name}-{t}", [prompt, prompt[::-1]], [hist[:-1] if adv else hist] * 2, K, N,
            drafts=[[], []] if adv else None, lm_outs=[[hist[-1]] + [0] * K] * 2 if adv else None, advance=adv))
        mk("no-match", [10, 11, 12], [13, 14, 15, 16], 3, 2)
        mk("tail-matches-only-itself", [1, 2, 1, 2], [1, 2, 3], 3, 3)
        mk("continuation-shorter-than-K", [5, 1, 2], [1, 2], 3, 2)
        mk("earliest-of-several", [1, 2, 7, 1, 2, 8], [9, 1, 2], 3, 2)
        mk("longest-ngram-wins", [1, 2, 3, 9, 8, 3, 7], [1, 2, 3], 2, 3)
        mk("ngram-capped-by-length", [], [4, 4], 7, 3)
    # a step whose two drafts are rejected and whose successor has no draft: rows 1 .. R - 1 fall back to the last token
    c.append(SpecCase("no-draft-after-leftover-drafts", [[20, 21, 22]] * 2, [[23, 24]] * 2, 3, 2, drafts=[[30, 31], [30]],
                      lm_outs=[[25, 0, 0, 0], [26, 0, 0, 0]], stale_ids=[[0, 0, 0, 77], [0, 0, 78, 79]]))
    # every draft accepted: a + 1 = K + 1 tokens appended, the next draft continues the copy
    c.append(SpecCase("all-accepted", [[1, 2, 3, 4, 5, 6, 7, 8]] * 2, [[1, 2], [9, 1]], 3, 2, drafts=[[3, 4, 5], [2, 3, 4]],
                      lm_outs=[[3, 4, 5, 6], [2, 3, 4, 0]]))
    # the append crosses the history's capacity: slots at or past cap are dropped and read as -1 by the draft
    h = [(7 * i) % 5 for i in range(15)]
    c.append(SpecCase("append-across-cap", [[1, 2, 3]] * 2, [h, h[:14]], 3, 2, cap=16, drafts=[[1, 2, 3], [1, 2]],
                      lm_outs=[[1, 2, 3, 4], [1, 2, 4, 0]]))
    c.append(SpecCase("history-past-cap", [[1, 2, 3]] * 2, [h + [1, 2, 3], h + [4]], 3, 2, cap=16, drafts=[[1], []],
                      lm_outs=[[1, 2, 0, 0], [3, 0, 0, 0]]))
    return c

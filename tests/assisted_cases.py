"""Shared by the assisted-decoding tests (test_assisted_cpu.py on the host, test_assisted_gpu.py on the device): the draft successor
model beside the successor model of tests/prompt_lookup_cases.py, host simulations of a whole assisted generation, and the cases
and host reference of the two hand-off kernels. Everything here is host code on CPU tensors; prompt_lookup_cases is imported and
left as it is."""
import functools
import random

import torch

import prompt_lookup_cases as pc
from oracle.llama import LlamaCfg, LlamaOracle
from spider_amd.llm import assisted_round_host

# ---------------------------------------------------------------------------------------------- the draft successor model
DRAFT_VOCAB = 296       # < 300: the target has four ids the draft model does not know
# where the draft model disagrees with succ: two ids of the block C the greedy walk of PROMPT cycles through. With K = 3 and 40 new
# tokens the rounds then come in all three kinds (asserted by test_assisted_cpu.py)
DRAFT_WRONG = {pc.C[2]: 101, pc.C[3]: 205}
# assisted decoding with K = 3 on PROMPT: rounds by kind (recomputed and asserted by test_assisted_cpu.py)
K3 = dict(steps=18, drafted=54, accepted=24, full=6, partial=6, rejected=6)


def draft_succ(v: int):
    """the draft model's successor map: succ on its own vocabulary, except at the two ids of DRAFT_WRONG"""
    return DRAFT_WRONG.get(v, pc.succ(v, DRAFT_VOCAB))


@functools.lru_cache(maxsize=None)
def draft_model():
    """(LlamaCfg, weights): successor_model()'s recipe at a smaller width -- 1 layer, hidden 128, 2 / 1 heads of 128, vocab 296 --
    whose lm_head row draft_succ(v) carries 0.25 * the embedding of v"""
    cfg = LlamaCfg(128, 1, 2, 1, 128, 256, DRAFT_VOCAB, 10000.0, None, 1e-6, False, 256)
    w = dict(LlamaOracle.random_weights(cfg, seed=47, std=0.04))
    E = (torch.randn(DRAFT_VOCAB, 128, generator=torch.Generator().manual_seed(5)) * 0.5).bfloat16().float()
    head = w["lm_head.weight"].clone()
    for v in range(cfg.vocab):
        if draft_succ(v) is not None:
            head[draft_succ(v)] += 0.25 * E[v]
    w["model.embed_tokens.weight"] = E
    w["lm_head.weight"] = head.bfloat16().float()
    return cfg, w


def draft_id(t: int, vocab: int = DRAFT_VOCAB) -> int:
    return t if 0 <= t < vocab else 0


@functools.lru_cache(maxsize=None)
def draft_margin(n_new: int = pc.T_NEW + 7):
    """(every arg-max equals draft_succ of the token in front of it, minimum top-2 margin) of the fp32 draft oracle read along the
    TARGET's greedy sequence behind PROMPT, from the last prompt token on: the contexts the draft engine meets in assisted decoding"""
    cfg, w = draft_model()
    seq = list(pc.PROMPT) + list(pc.successor_greedy()[0][:n_new])
    S = len(pc.PROMPT)
    logits, _, _ = LlamaOracle(cfg, w).forward(torch.tensor([[draft_id(t) for t in seq]]), torch.arange(len(seq))[None], None, None)
    lg = logits[0, S - 1:]
    top2 = lg.topk(2, -1).values
    follows = lg.argmax(-1).tolist() == [draft_succ(draft_id(t)) for t in seq[S - 1:]]
    return follows, float((top2[:, 0] - top2[:, 1]).min())


def _tally(kinds, K, a):
    kinds.append("rejected" if a == 0 else "full" if a == K else "partial")


def _record(kinds, drafted, accepted):
    return dict(steps=len(kinds), drafted=drafted, accepted=accepted, **{k: kinds.count(k) for k in ("full", "partial", "rejected")})


def simulate_tokens(first: int, T: int, K: int, target_next=pc.succ, draft_next=draft_succ, draft_vocab: int = DRAFT_VOCAB):
    """Assisted generation of T tokens replayed on the host for two models whose greedy token depends on the last token alone:
    `first` is the token behind the prompt. -> (tokens [T], record)"""
    hist, kinds, drafted, accepted = [first], [], 0, 0
    while len(hist) < T:
        drafts, t = [], hist[-1]
        for _ in range(K):
            t = draft_next(draft_id(t, draft_vocab))
            drafts.append(t)
        lm_out = [target_next(t) for t in [hist[-1]] + drafts]
        r = assisted_round_host(hist[-1], 0, 0, drafts, lm_out, draft_vocab)
        hist += r["append"]
        drafted, accepted = drafted + K, accepted + r["a"]
        _tally(kinds, K, r["a"])
    return hist[:T], _record(kinds, drafted, accepted)


def simulate_oracles(tcfg, tw, dcfg, dw, prompt, T, K):
    """The same generation with every step RUN on the two fp32 oracles and every hand-off taken from `assisted_round_host`: the
    draft oracle reads the sequence as the kernels feed it (slot by slot, ids it does not have as 0), the K + 1 verify rows go
    through one forward pass of the target behind the KV cache of the accepted tokens. -> (tokens [T], record)"""
    target, draft = LlamaOracle(tcfg, tw), LlamaOracle(dcfg, dw)
    S = len(prompt)
    logits, kv, _ = target.forward(torch.tensor([prompt]), torch.arange(S)[None], None, None)
    hist, n_ctx, kinds, drafted, accepted = [int(logits[0, -1].argmax())], S, [], 0, 0
    dview = {s: draft_id(t, dcfg.vocab) for s, t in enumerate(prompt)}      # what the draft engine's cache rows were computed from

    def draft_behind(kv_end):
        ids = [dview[s] for s in range(kv_end)]
        return int(draft.forward(torch.tensor([ids]), torch.arange(kv_end)[None], None, None)[0][0, -1].argmax())
    catch = dict(ids=[dview[S - 1], draft_id(hist[0], dcfg.vocab)], slot=[S - 1, S], kv_end=S)
    while len(hist) < T:
        for s, t in zip(catch["slot"], catch["ids"]):
            dview[s] = t
        drafts = [draft_behind(catch["kv_end"] + 1)]        # row 1 of the two-row step sees one slot more than row 0
        for j in range(1, K):
            dview[n_ctx + j] = draft_id(drafts[-1], dcfg.vocab)
            drafts.append(draft_behind(n_ctx + j + 1))
        ids = [hist[-1]] + drafts
        logits, kv2, _ = target.forward(torch.tensor([ids]), n_ctx + torch.arange(K + 1)[None], kv, None)
        r = assisted_round_host(hist[-1], n_ctx, n_ctx, drafts, logits[0].argmax(-1).tolist(), dcfg.vocab)
        assert [f[0] for f in r["feed"][:K - 1]] == [dview[n_ctx + j] for j in range(1, K)]
        hist += r["append"]
        n_ctx += r["a"] + 1
        assert r["row0"] == (hist[-1], n_ctx, n_ctx)
        kv = [(k[:, :, :n_ctx], v[:, :, :n_ctx]) for k, v in kv2]
        catch = r["catch_up"]
        drafted, accepted = drafted + K, accepted + r["a"]
        _tally(kinds, K, r["a"])
    return hist[:T], _record(kinds, drafted, accepted)


# ---------------------------------------------------------------------------------------------- hand-off kernel cases
class AssistCase:
    """One round's hand-off launches for B sequences of R = K + 1 verify rows: n_draft pushes, then the advance. Per sequence b:
    seqs[b] = dict(ids0, pos0, slot0, drafts [K], lm_out [K + 1], hist [tokens so far], n_draft (default K), stale (ids the rows
    past the drafts hold, default none)). Tensors are what the ops take (int32; counters int64)."""

    def __init__(self, name, K, seqs, cap=64, draft_vocab=DRAFT_VOCAB):
        B, R = len(seqs), K + 1
        self.name, self.B, self.R, self.K, self.cap, self.vd, self.seqs = name, B, R, K, cap, draft_vocab, seqs
        nds = {s.get("n_draft", K) for s in seqs}
        assert len(nds) == 1, "the pushes are launches for the whole batch: one n_draft per case"
        self.nd = nds.pop()
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
        self.ids, self.pos, self.slot, self.lm_out = i32(B * R), i32(B * R), i32(B * R), i32(B * R)
        self.kv_end, self.n_draft, self.hist, self.n_hist = i32(B), i32(B), i32(B, cap), i32(B)
        self.counters = torch.tensor([[5, 9, 4]] * B, dtype=torch.int64)
        # the draft engine's states: d2 = its two-row step (the catch-up rows of this round), d1 = its single-row step
        self.d2_ids, self.d2_pos, self.d2_slot, self.d2_out, self.d2_kv_end = i32(B * 2), i32(B * 2), i32(B * 2), i32(B * 2), i32(B)
        self.d1_ids, self.d1_pos, self.d1_slot, self.d1_out, self.d1_kv_end = i32(B), i32(B), i32(B), i32(B), i32(B)
        for b, s in enumerate(seqs):
            assert len(s["drafts"]) == K and len(s["lm_out"]) == R
            self.ids[b * R] = s["ids0"]
            self.ids[b * R + 1:(b + 1) * R] = torch.tensor(list(s.get("stale", [-7] * K)), dtype=torch.int32)
            self.pos[b * R], self.slot[b * R] = s["pos0"], s["slot0"]
            self.pos[b * R + 1:(b + 1) * R] = -7
            self.slot[b * R + 1:(b + 1) * R] = -7
            self.lm_out[b * R:(b + 1) * R] = torch.tensor(list(s["lm_out"]), dtype=torch.int32)
            self.kv_end[b], self.n_draft[b] = s["slot0"] + 1, self.nd
            stored = s["hist"][:cap]
            self.hist[b, :len(stored)] = torch.tensor(stored, dtype=torch.int32)
            self.n_hist[b] = len(s["hist"])
            self.d2_ids[b * 2:b * 2 + 2] = torch.tensor([3, draft_id(s["ids0"], draft_vocab)], dtype=torch.int32)
            self.d2_pos[b * 2:b * 2 + 2] = torch.tensor([s["pos0"] - 1, s["pos0"]], dtype=torch.int32)
            self.d2_slot[b * 2:b * 2 + 2] = torch.tensor([s["slot0"] - 1, s["slot0"]], dtype=torch.int32)
            self.d2_kv_end[b] = s["slot0"]
            self.d2_out[b * 2:b * 2 + 2] = torch.tensor([-3, -3], dtype=torch.int32)

    def __repr__(self):
        return self.name

    BUFFERS = ("ids", "pos", "slot", "lm_out", "kv_end", "n_draft", "hist", "n_hist", "counters", "d2_ids", "d2_pos", "d2_slot",
               "d2_out", "d2_kv_end", "d1_ids", "d1_pos", "d1_slot", "d1_out", "d1_kv_end")

    def round(self, b):
        s = self.seqs[b]
        return assisted_round_host(s["ids0"], s["pos0"], s["slot0"], s["drafts"], s["lm_out"], self.vd, self.nd)

    def expected_after_push(self, j) -> dict:
        """the pushed row of the target and the draft engine's single row behind push j (1-based)"""
        o = dict(ids=[], pos=[], slot=[], d1_ids=[], d1_pos=[], d1_slot=[], d1_kv_end=[])
        for b in range(self.B):
            r = self.round(b)
            for k, v in zip(("ids", "pos", "slot"), r["rows"][j]):
                o[k].append(v)
            for k, v in zip(("d1_ids", "d1_pos", "d1_slot", "d1_kv_end"), r["feed"][j - 1]):
                o[k].append(v)
        return o

    def expected(self) -> dict:
        """every buffer behind the round's last launch, by the host restatement"""
        B, R, cap = self.B, self.R, self.cap
        o = {k: getattr(self, k).clone() for k in self.BUFFERS}
        for b in range(B):
            r, s = self.round(b), self.seqs[b]
            for j in range(1, self.nd + 1):
                o["ids"][b * R + j], o["pos"][b * R + j], o["slot"][b * R + j] = r["rows"][j]
            if self.nd:
                o["d1_ids"][b], o["d1_pos"][b], o["d1_slot"][b], o["d1_kv_end"][b] = r["feed"][self.nd - 1]
                o["d2_out"][b * 2 + 1] = s["drafts"][0]
                if self.nd > 1:
                    o["d1_out"][b] = s["drafts"][self.nd - 1]
            nh = len(s["hist"])
            for i, t in enumerate(r["append"]):
                if nh + i < cap:
                    o["hist"][b, nh + i] = t
            o["n_hist"][b] = nh + r["a"] + 1
            o["kv_end"][b] += r["a"] + 1
            o["counters"][b] += torch.tensor([1, r["n_draft"], r["a"]])
            o["ids"][b * R], o["pos"][b * R], o["slot"][b * R] = r["row0"]
            cu = r["catch_up"]
            for k in ("ids", "pos", "slot"):
                o["d2_" + k][b * 2:b * 2 + 2] = torch.tensor(cu[k], dtype=torch.int32)
            o["d2_kv_end"][b] = cu["kv_end"]
        return o


def _seq(ids0, pos0, slot0, drafts, lm_out, hist, **kw):
    return dict(ids0=ids0, pos0=pos0, slot0=slot0, drafts=list(drafts), lm_out=list(lm_out), hist=list(hist), **kw)


def random_assist_cases(K, seed=0):
    """alphabet of 5 (+ now and then an id the draft model does not have), B = 2, drafts and model tokens agree 70 % of the time"""
    rng = random.Random(2000 * seed + K)
    out = []
    for n in range(12):
        seqs = []
        for b in range(2):
            tok = lambda: rng.randrange(5) if rng.random() < 0.9 else DRAFT_VOCAB + rng.randrange(4)
            nh, beg = rng.choice((1, 2, 50)), rng.choice((0, 0, 3))
            slot0 = rng.randrange(1, 40) + nh + beg
            hist = [tok() for _ in range(nh)]
            drafts = [rng.randrange(5) for _ in range(K)]
            row = [hist[-1]] + drafts + [0]
            lm_out = [row[r + 1] if rng.random() < 0.7 else tok() for r in range(K + 1)]
            seqs.append(_seq(hist[-1], slot0 - beg, slot0, drafts, lm_out, hist))
        out.append(AssistCase(f"rand-K{K}-{n}", K, seqs))
    return out


def named_assist_cases():
    c = []
    h = [4, 5, 6]
    # a = 0: the first draft is wrong; the catch-up rows are row 0's token and the model's
    c.append(AssistCase("none-accepted", 3, [_seq(6, 20, 20, [7, 8, 9], [1, 8, 9, 2], h), _seq(6, 9, 9, [1, 1, 1], [2, 1, 1, 1], h)]))
    # a = K: K + 1 tokens appended; the draft engine never consumed d_K, its catch-up row 0 supplies it
    c.append(AssistCase("all-accepted", 3, [_seq(6, 20, 20, [7, 8, 9], [7, 8, 9, 10], h), _seq(6, 9, 9, [1, 1, 1], [1, 1, 1, 1], h)]))
    c.append(AssistCase("partial", 3, [_seq(6, 20, 20, [7, 8, 9], [7, 8, 3, 10], h), _seq(6, 9, 9, [1, 2, 3], [1, 0, 3, 4], h)]))
    c.append(AssistCase("K1", 1, [_seq(6, 20, 20, [7], [7, 8], h), _seq(6, 9, 9, [7], [8, 9], h)]))
    c.append(AssistCase("K7-all-accepted", 7, [_seq(1, 30, 30, range(2, 9), range(2, 10), h), _seq(1, 30, 30, range(2, 9), [2, 3, 4, 5, 0, 7, 8, 9], h)]))
    # ids the draft model does not have: an accepted target id as the draft (row a) and as the model's own token -- the draft side
    # reads 0, hist and the target's row 0 the true id
    big = DRAFT_VOCAB + 2
    c.append(AssistCase("ids-past-the-draft-vocabulary", 3, [_seq(6, 20, 20, [7, big, 9], [7, big, 3, 10], h),
                                                             _seq(big, 9, 9, [1, 2, 3], [1, 2, 3, big + 1], h + [big])]))
    c.append(AssistCase("row0-past-the-draft-vocabulary-none-accepted", 3, [_seq(big, 20, 20, [7, 8, 9], [1, 8, 9, 2], h + [big])] * 2))
    # a left-padded prompt: kv_beg = 5 pads, positions run 5 behind the slots
    c.append(AssistCase("kv_beg-pos-differs-from-slot", 3, [_seq(6, 15, 20, [7, 8, 9], [7, 8, 3, 10], h), _seq(6, 4, 9, [7, 8, 9], [7, 8, 9, 1], h)]))
    # the history is one short of its capacity: the first appended token is stored, the others are dropped, n_hist counts all
    h15 = [(7 * i) % 5 for i in range(15)]
    c.append(AssistCase("hist-one-short-of-cap", 3, [_seq(h15[-1], 20, 20, [7, 8, 9], [7, 8, 9, 10], h15), _seq(h15[-1], 9, 9, [7, 8, 9], [7, 1, 9, 9], h15)],
                        cap=16))
    # two of three rows are drafts; row 3 holds a stale id that equals the model's token behind row 2 and must not be accepted
    c.append(AssistCase("stale-ids-past-the-drafts", 3, [_seq(6, 20, 20, [7, 8, 9], [7, 8, 9, 10], h, n_draft=2, stale=[0, 0, 9]),
                                                         _seq(6, 9, 9, [7, 8, 9], [7, 8, 9, 10], h, n_draft=2, stale=[55, 66, 9])]))
    return c

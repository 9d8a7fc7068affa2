"""Shared by the beam-search GPU tests: the property check of one device beam step against an fp64 host restatement."""
import torch


def delta(s):
    """Bound on |device score - fp64 score|: 1e-4 + |s| * 2^-20. Derived, not measured: each thread of the partial reduction adds
    16 exponentials serially and the rest is a tree, so the sum-exp error stays below the 4e-5 that a few hundred serial fp32 adds
    would give; expf / logf and the three fp32 roundings of a score s (lse, logit - lse, run + ...) add about 3e-5 + |s| * 2^-22."""
    return 1e-4 + abs(float(s)) * 2.0 ** -20


def check_beam_step(logits, run, eos, score, beam, tok, new_run, src, nxt):
    """logits [B*K, V] (raw bf16 values), run [B, K] fp32 before the step; the step's outputs: score / beam / tok [B, C] (trace
    entry), new_run / src / nxt [B, K]. All CPU tensors. Asserts the four properties of the step; returns the number of adjacent
    reported pairs with EQUAL scores (so that callers can tell whether the tie rule was exercised)."""
    B, K = run.shape
    V = logits.shape[-1]
    C = score.shape[1]
    host = torch.log_softmax(logits.double(), -1).view(B, K, V) + run.double()[:, :, None]
    ties = 0
    for b in range(B):
        flat = beam[b].long() * V + tok[b].long()
        assert int(beam[b].min()) >= 0 and int(beam[b].max()) < K and int(tok[b].min()) >= 0 and int(tok[b].max()) < V
        assert flat.unique().numel() == C, "a continuation is reported twice"
        hs = host[b].reshape(-1)
        # 1. every reported score is the host score of its (beam, token)
        for c in range(C):
            d = abs(float(score[b, c]) - float(hs[flat[c]]))
            assert d <= delta(hs[flat[c]]), (b, c, float(score[b, c]), float(hs[flat[c]]))
        # 2. no unreported continuation beats the C-th reported one
        rest = hs.clone()
        rest[flat] = -float("inf")
        assert float(rest.max()) <= float(score[b, C - 1]) + delta(score[b, C - 1]), (b, float(rest.max()), float(score[b, C - 1]))
        # 3. the order rule: score descending, then beam * V + token ascending
        for c in range(C - 1):
            s0, s1 = float(score[b, c]), float(score[b, c + 1])
            assert s0 > s1 or (s0 == s1 and int(flat[c]) < int(flat[c + 1])), (b, c, s0, s1, int(flat[c]), int(flat[c + 1]))
            ties += s0 == s1
        # 4. the running beams are exactly the first K reported continuations whose token is no EOS id
        keep = [c for c in range(C) if int(tok[b, c]) not in (eos or ())][:K]
        assert len(keep) == K
        assert new_run[b].tolist() == [float(score[b, c]) for c in keep]
        assert src[b].tolist() == [int(beam[b, c]) for c in keep] and nxt[b].tolist() == [int(tok[b, c]) for c in keep]
    return ties


def beam_step_host(logits, run_scores, C, eos):
    """One device beam step restated with the torch ops `_beam_search` uses: log_softmax of the raw logits [B*K, V] in fp32,
    + run_scores [B, K], torch.topk of the K*V continuations per batch row. Returns the trace entry (score, beam, token), each
    [B, C], and the next running beams (scores, source beam, token, each [B, K]): the first K continuations, in order, whose
    token is no EOS id. (torch.topk leaves the order of equal scores open; the kernel orders them by beam * V + token.)"""
    B, K = run_scores.shape
    V = logits.shape[-1]
    lp = torch.nn.functional.log_softmax(logits.float(), dim=-1).view(B, K, V) + run_scores.float()[:, :, None]
    score, idx = torch.topk(lp.reshape(B, K * V), k=C)
    beam, tok = idx // V, idx % V
    sel = torch.tensor([[c for c in range(C) if int(tok[b, c]) not in (eos or ())][:K] for b in range(B)])
    return (score, beam, tok), (score.gather(1, sel), beam.gather(1, sel), tok.gather(1, sel))

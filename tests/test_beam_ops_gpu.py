"""GPU: the three beam-search kernels on their own. beam_partial + beam_select on random bf16 logits against an fp64 host
restatement (tests/beam_checks.py: every reported score within delta of the host score of its (beam, token), nothing unreported
beats the C-th reported one by more than delta, the order rule, the running beams are the first K non-EOS ones), and the KV row
gather bit for bit against index_select for identity, all-from-one, cyclic and random maps."""
import pytest
import torch

from beam_checks import check_beam_step

pytestmark = pytest.mark.gpu


def _step(dev, logits, run, eos, C, step=3, cap=5):
    from spider_amd import ops
    B, K = run.shape
    R, V = logits.shape
    lg = logits.to(dev)
    ws = ops.beam_workspace(R, V, C, dev)
    run_d = run.to(dev).clone()
    eos_ids = torch.tensor((eos or []) + [-1] * (8 - len(eos or [])), dtype=torch.int32, device=dev)
    n_eos = torch.tensor([len(eos or [])], dtype=torch.int32, device=dev)
    n_hist = torch.full((R,), step, dtype=torch.int32, device=dev)
    trace = (torch.zeros(cap, B, C, device=dev), torch.zeros(cap, B, C, dtype=torch.int32, device=dev),
             torch.zeros(cap, B, C, dtype=torch.int32, device=dev))
    src = torch.full((B, K), -7, dtype=torch.int32, device=dev)
    nxt = torch.full((R,), -7, dtype=torch.int32, device=dev)
    ops.beam_partial(lg, C, ws)
    ops.beam_select(ws, run_d, eos_ids, n_eos, n_hist, trace, src, nxt, V, C)
    torch.cuda.synchronize()
    for t in trace:     # only the step's slot of the trace is written
        other = torch.cat([t[:step], t[step + 1:]])
        assert not other.any()
    return tuple(t[step].cpu() for t in trace), run_d.cpu(), src.cpu(), nxt.cpu().view(B, K)


@pytest.mark.parametrize("n_eos", [0, 1, 3])
@pytest.mark.parametrize("B,K", [(1, 2), (2, 4), (1, 8)])
@pytest.mark.parametrize("V", [331, 4099, 151936])
def test_partial_and_select_against_fp64(dev, V, B, K, n_eos):
    g = torch.Generator().manual_seed(V + 10 * K + n_eos)
    C = max(2, 1 + n_eos) * K
    logits = (torch.randn(B * K, V, generator=g) * 3.0).bfloat16()
    logits[K - 1] = logits[0]                   # planted exact duplicates: two beams with the same logits (and, below, scores)
    top = logits[0].float().topk(4).indices
    logits[0, (top[1] + 1) % V] = logits[0, top[1]]     # ... and two tokens of one row with the same logit, near the top
    logits[K - 1] = logits[0]
    run = -torch.rand(B, K, generator=g) * 4.0
    run[0, 0] = run[0, K - 1] = 0.0              # the twin beams lead, so their (equal) continuations are among the reported ones
    eos = [int(top[0]), int(logits[B * K - 1].float().argmax()), int((top[1] + 1) % V)][:n_eos]
    eos = sorted(set(eos))
    (score, beam, tok), new_run, src, nxt = _step(dev, logits, run, eos, C)
    ties = check_beam_step(logits.float(), run, eos, score, beam, tok, new_run, src, nxt)
    assert ties > 0, "the planted duplicates did not reach the reported continuations"
    # the step-0 score vector: beam 0 alone is drawn from
    run0 = torch.zeros(B, K)
    run0[:, 1:] = -1e9
    (score, beam, tok), new_run, src, nxt = _step(dev, logits, run0, eos, C, step=0)
    check_beam_step(logits.float(), run0, eos, score, beam, tok, new_run, src, nxt)
    assert not beam.any() and not src.any()


def test_select_rejects_what_the_kernel_does_not_hold(dev):
    from spider_amd import ops
    B, K, V, C = 1, 8, 331, 40
    with pytest.raises(ValueError, match="beam_select"):
        ops.beam_select(ops.beam_workspace(8, V, C, dev), torch.zeros(B, K, device=dev), torch.zeros(8, dtype=torch.int32, device=dev),
                        torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev),
                        (torch.zeros(2, B, C, device=dev), torch.zeros(2, B, C, dtype=torch.int32, device=dev),
                         torch.zeros(2, B, C, dtype=torch.int32, device=dev)),
                        torch.zeros(B, K, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev), V, C)


L, ROWS, NKV, T, D = 2, 8, 2, 64, 128


@pytest.fixture(scope="module")
def kv_ref():
    g = torch.Generator().manual_seed(3)
    return torch.randn(L, ROWS, NKV, T, D, generator=g).bfloat16(), torch.randn(L, ROWS, NKV, T, D, generator=g).bfloat16()


def _maps(K, R):
    g = torch.Generator().manual_seed(K)
    nb = R // K
    return {"identity": torch.arange(K).repeat(nb), "all_from_one": torch.full((R,), K - 1),
            "cyclic": ((torch.arange(K) + 1) % K).repeat(nb), "random": torch.randint(0, K, (R,), generator=g)}


@pytest.mark.parametrize("name", ["identity", "all_from_one", "cyclic", "random"])
@pytest.mark.parametrize("K,R", [(8, 8), (4, 8), (2, 8), (2, 4)])
def test_kv_row_gather_equals_index_select(dev, kv_ref, K, R, name):
    from spider_amd import ops
    k0, v0 = kv_ref
    src = _maps(K, R)[name]
    if name == "random":
        assert src.unique().numel() < R or K == 2      # duplicates
    nb = R // K
    beg = torch.tensor([3, 0, 5, 1][:nb]).repeat_interleave(K)       # equal across a batch row's beams
    end = torch.tensor([T - 7, T, 40, T - 1][:nb]).repeat_interleave(K)
    k, v = k0.to(dev).clone(), v0.to(dev).clone()
    kt, vt = torch.zeros_like(k), torch.zeros_like(v)
    ops.kv_row_gather(k, v, kt, vt, src.to(dev, torch.int32), beg.to(dev, torch.int32), end.to(dev, torch.int32), K)
    torch.cuda.synchronize()
    rows = (torch.arange(R) // K) * K + src
    for got, ref in ((k.cpu(), k0), (v.cpu(), v0)):
        want = ref.clone()
        for r in range(R):
            want[:, r, :, beg[r]:end[r]] = ref[:, rows[r], :, beg[r]:end[r]]     # = index_select on the used slots; the rest stays
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), name

"""CPU: `score_host` (the fp64 definition of LlamaEngine.score) against transformers' LlamaForCausalLM.forward(labels=) on a tiny
configuration -- shift, mask, -100 labels, left padding --, the argument rules of `resolve_score`, the new C-ABI symbol and the
size of the kernel tolerance of logprob_checks.py at the full vocabulary."""
import math

import pytest
import torch

import logprob_checks as lc
from spider_amd import lib as slib
from spider_amd.llm import IGNORE_INDEX, resolve_score, score_host, score_targets


@pytest.fixture(scope="module")
def tiny_hf():
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=331, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=64, attn_implementation="eager")
    return LlamaForCausalLM(cfg).float().eval()


def _ids(B=2, S=21, seed=0):
    return torch.randint(3, 331, (B, S), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("case", ["plain", "ignored", "left_pad"])
def test_score_host_loss_equals_transformers(tiny_hf, case):
    ids = _ids()
    labels, am = ids.clone(), None
    if case == "ignored":
        labels[0, 3:9] = IGNORE_INDEX
        labels[1, -1] = IGNORE_INDEX
    if case == "left_pad":
        am = torch.ones_like(ids)
        am[1, :5] = 0
        labels[am == 0] = IGNORE_INDEX         # HF's loss knows labels only: the pads are ignored through them
    with torch.no_grad():
        out = tiny_hf(input_ids=ids, attention_mask=am, labels=labels)
    got = score_host(out.logits, labels if case != "left_pad" else ids, am)     # left_pad: score_host masks the pads by attention_mask
    n = int((labels[:, 1:] != IGNORE_INDEX).sum())
    print(f"MEASURED score_host vs transformers ({case}): loss {got.loss:.7f} vs {float(out.loss):.7f}, n_tokens {got.n_tokens}")
    assert got.n_tokens == n
    assert abs(got.loss - float(out.loss)) <= 1e-5
    assert abs(got.perplexity - math.exp(got.loss)) <= 1e-12
    # the shift: index t holds log_softmax(logits[t - 1])[labels[t]]; index 0 and ignored positions are masked
    lsm = torch.log_softmax(out.logits.double(), -1)
    tg = score_targets(labels, am)
    assert not bool(got.mask[:, 0].any()) and torch.equal(got.mask, tg != IGNORE_INDEX)
    for b, t in ((0, 1), (1, 7), (1, 20)):
        if bool(got.mask[b, t]):
            assert abs(float(got.token_logprobs[b, t]) - float(lsm[b, t - 1, labels[b, t]])) <= 1e-12
            assert int(got.argmax[b, t]) == int(out.logits[b, t - 1].argmax())
    assert float(got.token_logprobs[~got.mask].abs().max()) == 0.0 and bool((got.argmax[~got.mask] == -1).all())


def test_score_host_fields_and_reference_distribution():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 6, 50, generator=g, dtype=torch.float64) * 3
    y = x + torch.randn(2, 6, 50, generator=g, dtype=torch.float64) * 0.3
    labels = torch.randint(0, 50, (2, 6), generator=g)
    o = score_host(x, labels, logits_ref=y)
    p, q = torch.softmax(x, -1), torch.softmax(y, -1)
    ent = -(p * p.log()).sum(-1)
    kl = (q * (q.log() - p.log())).sum(-1)
    assert float((o.entropy[:, 1:] - ent[:, :-1]).abs().max()) < 1e-12
    assert float((o.kl[:, 1:] - kl[:, :-1]).abs().max()) < 1e-12 and float(o.kl.min()) >= 0.0
    assert abs(o.mean_kl - float(kl[:, :-1].mean())) < 1e-12
    assert abs(o.top1_agree - float((p.argmax(-1) == q.argmax(-1))[:, :-1].double().mean())) < 1e-12
    same = score_host(x, labels, logits_ref=x)
    assert float(same.kl.abs().max()) == 0.0 and same.top1_agree == 1.0
    # ties go to the lower id; a constant row has entropy log V
    c = torch.zeros(1, 2, 8)
    c[0, 0, 3] = c[0, 0, 5] = 2.0
    t = score_host(c, torch.tensor([[1, 3]]))
    assert int(t.argmax[0, 1]) == 3
    u = score_host(torch.full((1, 2, 8), 7.0), torch.tensor([[1, 3]]))
    assert int(u.argmax[0, 1]) == 0 and abs(float(u.entropy[0, 1]) - math.log(8)) < 1e-12
    empty = score_host(x, torch.full((2, 6), IGNORE_INDEX))
    assert empty.n_tokens == 0 and math.isnan(empty.loss)


def test_resolve_score_names_the_argument():
    ids = _ids()
    rs = lambda **kw: resolve_score(331, 64, 2, 32, False, **kw)
    B, S, tg = rs(input_ids=ids)
    assert (B, S) == (2, 21) and torch.equal(tg[:, 1:], ids[:, 1:]) and bool((tg[:, 0] == IGNORE_INDEX).all())
    am = torch.ones_like(ids)
    am[1, :5] = 0
    assert bool((rs(input_ids=ids, attention_mask=am)[2][1, :5] == IGNORE_INDEX).all())
    emb = torch.zeros(2, 21, 64)
    for kw, word in ((dict(), "input_ids"),
                     (dict(input_ids=ids, inputs_embeds=emb), "inputs_embeds"),
                     (dict(input_ids=ids.float()), "input_ids"),
                     (dict(input_ids=ids + 400), "input_ids"),
                     (dict(input_ids=_ids(B=3)), "input_ids"),
                     (dict(input_ids=_ids(S=33)), "input_ids"),
                     (dict(inputs_embeds=emb), "labels"),
                     (dict(inputs_embeds=emb[..., :32], labels=ids), "inputs_embeds"),
                     (dict(input_ids=ids, attention_mask=am[:, :20]), "attention_mask"),
                     (dict(input_ids=ids, attention_mask=am.flip(1)), "attention_mask"),
                     (dict(input_ids=ids, position_ids=torch.zeros(3, 2, 21, dtype=torch.long)), "position_ids"),
                     (dict(input_ids=ids, labels=ids[:, :20]), "labels"),
                     (dict(input_ids=ids, labels=ids + 331), "labels"),
                     (dict(input_ids=ids, labels=ids - 400), "labels")):
        with pytest.raises(ValueError, match=word):
            rs(**kw)
    with pytest.raises(ValueError, match="position_ids"):
        resolve_score(331, 64, 2, 32, True, input_ids=ids, position_ids=torch.zeros(3, 2, 20, dtype=torch.long))
    # a label >= vocab at an ignored position is not read
    lab = ids.clone()
    lab[1, :5] = 100000
    rs(input_ids=ids, attention_mask=am, labels=lab)


def test_symbol_and_host_validation():
    assert len(slib.SIGNATURES["spider_logprob_rows_bf16"][1]) == 14
    lib = slib.load()
    assert lib.spider_abi_version() == 4
    one = 16        # any non-null, 16-byte aligned value: validation happens before a launch
    call = lambda ld, rows, V, ref=None, ld_ref=0, kl=None, ar=None: lib.spider_logprob_rows_bf16(
        one, ld, one, ref, ld_ref, one, one, one, one, kl, ar, rows, V, None)
    for args, word in (((8, 0, 8), b"rows"), ((8, 1, 0), b"V must"), ((8, 1, 9), b"ld must"), ((12, 1, 9), b"ld must"),
                       ((16, 1, 9, one, 12, one, one), b"ld_ref"), ((16, 1, 9, one, 16, None, one), b"together")):
        assert call(*args) == -1
        assert word in lib.spider_last_error(), (args, lib.spider_last_error())
    import spider_amd.torch_ops as T
    assert T.SCORE_OP_NAMES == ("logprob_rows",) and hasattr(torch.ops.spider_hip, "logprob_rows") and len(T.OP_NAMES) == 14


def test_tolerance_at_the_full_vocabulary():
    """the condition of the derivation: TOL_LSE at V = 152064 stays <= 2e-4 (T >= 128 lanes per row), on both logit scales of the GPU test"""
    assert lc.T_LANES >= 128 and lc.eps_sum(152064) == 610 * 2.0 ** -23
    g = torch.Generator().manual_seed(0)
    for scale in (1.0, 8.0):
        x = (torch.randn(1, 152064, generator=g) * scale).bfloat16()
        r = lc.reference(x, torch.tensor([5]))
        print(f"MEASURED logprob_checks tolerance at V = 152064, N(0, {scale:g}^2): lse {float(r['tol_lse']):.3g}  logprob "
              f"{float(r['tol_logprob']):.3g}  entropy {float(r['tol_entropy']):.3g}")
        assert float(r["tol_lse"]) <= 2e-4

"""GPU: ops.logprob_rows (csrc/logprob.hip) against the fp64 reference and the derived tolerances of logprob_checks.py, every output."""
import math

import pytest
import torch

import logprob_checks as lc

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


def _padded(x, ld, dev, seed):
    """x [rows, V] bf16 -> a device buffer [rows, ld] with junk (large values, NaN bit patterns) in the stride gap; (buffer, view)"""
    rows, V = x.shape
    g = torch.Generator().manual_seed(seed)
    buf = (torch.randn(rows, ld, generator=g) * 1e4).bfloat16()
    if ld > V:
        buf[:, V::3] = float("nan")
    buf[:, :V] = x
    buf = buf.to(dev)
    return buf, buf[:, :V]


def _targets(rows, V, seed):
    t = torch.randint(0, V, (rows,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    fixed = [0, V - 1, (V - 1) // 8 * 8, -100]       # first, last, first of the masked tail group, ignored
    t[:min(rows, 4)] = torch.tensor(fixed[:min(rows, 4)], dtype=torch.int32)
    return t


def _run(ops, dev, x, tg, y=None, gap=0, seed=0):
    V = x.shape[1]
    ld = (V + 7) // 8 * 8 + gap
    buf, view = _padded(x, ld, dev, seed)
    rbuf, rview = _padded(y, ld + 8, dev, seed + 1) if y is not None else (None, None)
    keep = buf.clone(), (rbuf.clone() if y is not None else None)
    tgd = tg.to(dev)
    got = ops.logprob_rows(view, tgd, logits_ref=rview)
    # the same through the whole-buffer form (V given) and through the torch custom op
    got2 = ops.logprob_rows(buf, tgd, V, logits_ref=rbuf)
    import spider_amd.torch_ops  # noqa: F401
    got3 = torch.ops.spider_hip.logprob_rows(view, tgd, V, rview)
    names = ("logprob", "lse", "argmax", "entropy") + (("kl", "argmax_ref") if y is not None else ())
    for i, k in enumerate(names):
        assert torch.equal(got[k], got2[k]) and torch.equal(got[k], got3[i]), k
    if y is None:
        assert got3[4].numel() == 0 and got3[5].numel() == 0
    # inputs untouched, the stride gap included (bit patterns: the junk holds NaN)
    assert torch.equal(buf.view(torch.int16), keep[0].view(torch.int16)) and torch.equal(tgd.cpu(), tg)
    if y is not None:
        assert torch.equal(rbuf.view(torch.int16), keep[1].view(torch.int16))
    return got


@pytest.mark.parametrize("V", [1, 7, 8, 9, 331, 1024, 4099])
def test_logprob_rows_sweep(ops, dev, V):
    for rows in (1, 3, 130):
        for scale in (1.0, 8.0):
            g = torch.Generator().manual_seed(1000 * V + rows)
            x = (torch.randn(rows, V, generator=g) * scale).bfloat16()
            y = (x.float() + torch.randn(rows, V, generator=g) * 0.5).bfloat16()
            tg = _targets(rows, V, rows)
            ref = lc.reference(x, tg)
            ref_kl = lc.reference(x, tg, y)
            for gap in (0, 24):
                lc.check(_run(ops, dev, x, tg, gap=gap), ref, f"V={V} rows={rows} scale={scale:g} gap={gap}")
                lc.check(_run(ops, dev, x, tg, y, gap=gap), ref_kl, f"V={V} rows={rows} scale={scale:g} gap={gap} +ref")


@pytest.mark.parametrize("scale", [1.0, 8.0])
def test_logprob_rows_full_vocabulary_row(ops, dev, scale):
    V = 152064
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(1, V, generator=g) * scale).bfloat16()
    y = (x.float() + torch.randn(1, V, generator=g) * 0.5).bfloat16()
    tg = torch.tensor([V - 1], dtype=torch.int32)
    lc.check(_run(ops, dev, x, tg, y), lc.reference(x, tg, y), f"V={V} rows=1 scale={scale:g} +ref")


@pytest.mark.parametrize("V", [9, 331, 4099])
def test_logprob_rows_special_rows(ops, dev, V):
    g = torch.Generator().manual_seed(V)
    x = torch.randn(6, V, generator=g).bfloat16()
    x[0] = 100.0                # a missing max subtraction overflows here ...
    x[1] = -100.0               # ... and underflows to log 0 here
    x[2] = 0.625                # constant: argmax 0, entropy log V
    hi = float(x[3].float().max()) + 1.0
    a, b = V // 3, V - 1        # an exact two-way tie of the maximum, the second in the last (masked) group: the lower id wins
    x[3, a] = x[3, b] = hi
    x[4, V - 1] = 50.0          # the maximum is the row's last element
    tg = torch.tensor([0, V - 1, V // 2, b, -100, 1], dtype=torch.int32)
    ref = lc.reference(x, tg)
    got = _run(ops, dev, x, tg, gap=24)
    lc.check(got, ref, f"special rows V={V}")
    assert got["argmax"].tolist()[:5] == [0, 0, 0, a, V - 1]
    for r in (0, 1, 2):
        assert abs(float(got["entropy"][r]) - math.log(V)) <= float(ref["tol_entropy"][r])
        assert abs(float(got["logprob"][r]) + math.log(V)) <= float(ref["tol_logprob"][r])
    assert float(got["logprob"][4]) == 0.0


@pytest.mark.parametrize("V", [7, 331, 4099])
def test_logprob_rows_kl_identities(ops, dev, V):
    g = torch.Generator().manual_seed(V)
    x = (torch.randn(5, V, generator=g) * 8).bfloat16()
    tg = _targets(5, V, 3)
    same = _run(ops, dev, x, tg, x.clone())
    assert float(same["kl"].abs().max()) == 0.0 and torch.equal(same["argmax"], same["argmax_ref"])      # exactly zero
    # a reference shifted by a constant is the same distribution; quarter steps in [-8, 8] + 16 stay exact in bf16
    q = ((torch.randn(5, V, generator=g) * 4).round() / 4).clamp(-8, 8).bfloat16()
    sh = (q.float() + 16.0).bfloat16()
    assert torch.equal(sh.float() - 16.0, q.float())
    ref = lc.reference(q, tg, sh)
    got = _run(ops, dev, q, tg, sh)
    lc.check(got, ref, f"shifted reference V={V}")
    assert bool((got["kl"].double().cpu().abs() <= ref["tol_kl"]).all())


def test_logprob_rows_rejects(ops, dev):
    x = torch.zeros(4, 331, dtype=BF16, device=dev)
    t = torch.zeros(4, dtype=torch.int32, device=dev)
    buf = torch.zeros(4, 336, dtype=BF16, device=dev)
    for bad, kw, word in ((x, {}, "row stride"), (buf[:, :331], dict(V=332), "V=332"), (buf.float()[:, :331], {}, "dtype"),
                          (buf[:, :331], dict(logits_ref=buf[:2, :331]), "logits_ref")):
        with pytest.raises(ValueError, match=word):
            ops.logprob_rows(bad, t, **kw)
    with pytest.raises(ValueError, match="targets"):
        ops.logprob_rows(buf[:, :331], t[:3])

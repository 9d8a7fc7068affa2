"""CPU: the definition of calibrated MXFP4 (`llm.quantize_mxfp4_gptq`, GPTQ on MX blocks), its proxy loss, the host-side
resolver of LlamaEngine's `calibration` keyword, and the argument validation of the sweep kernel's C entry.

Figures of the correlated case (N, K, T) = (200, 256, 1024), seed 0, measured with this file: relative output error
||X (W - Q)^T|| / ||X W^T|| round to nearest 0.1203, calibrated 0.0274 = 0.228 of it (the bound is 0.5, a factor of two for other
seeds); plain weight error ||W - Q|| / ||W|| 0.118 -> 0.137."""
import pytest
import torch

import gptq_cases as GC
from spider_amd.llm import (dequantize_mxfp4, gptq_factor, gptq_prepare, gptq_proxy_loss, quantize_mxfp4, quantize_mxfp4_gptq,
                            resolve_calibration)


def _w(N, K, seed, std=0.02):
    return (torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) * std).bfloat16().float()


def test_diagonal_hessian_gives_round_to_nearest_bytes():
    W = _w(24, 96, 1)
    W[3, 32:64] = 0.0                       # an all-zero block: scale byte 127, codes 0
    W[5, 0:32] = 0.0
    W[5, 7] = 0.5                           # amax 0.5 -> scale 2^-3 ... and a negative entry below a quarter of the scale: code 8 (-0)
    W[5, 9] = -0.01
    b0, s0 = quantize_mxfp4(W)
    assert int(s0[3, 1]) == 127 and int(GC.codes_of(b0)[5, 9]) == 8
    g = torch.Generator().manual_seed(2)
    for H in (torch.eye(96), torch.diag(torch.rand(96, generator=g) + 0.05), torch.diag(torch.rand(96, generator=g).double() * 1e3 + 1.0)):
        for damp in (0.01, 0.5):
            b, s = quantize_mxfp4_gptq(W, H, damp)
            assert b.dtype == torch.uint8 and s.dtype == torch.uint8 and b.shape == (24, 48) and s.shape == (24, 3)
            assert torch.equal(b, b0) and torch.equal(s, s0)


def test_correlated_inputs_halve_the_output_error():
    W, X, H = GC.correlated_case(200, 256, 1024, 0)
    b, s, _ = GC.definition(200, 256, 1024, 0)
    b0, s0 = quantize_mxfp4(W)
    rtn, cal = GC.out_err(W, X, b0, s0), GC.out_err(W, X, b, s)
    f32 = lambda b, s: dequantize_mxfp4(b, s, torch.float32)
    p_rtn, p_cal = gptq_proxy_loss(W, f32(b0, s0), H), gptq_proxy_loss(W, f32(b, s), H)
    wrel = lambda Q: float((W - Q).norm() / W.norm())
    print(f"output error: round to nearest {rtn:.4f}, calibrated {cal:.4f} = {cal / rtn:.3f} of it; proxy {p_rtn:.5f} -> {p_cal:.5f}; "
          f"weight error {wrel(f32(b0, s0)):.4f} -> {wrel(f32(b, s)):.4f}")
    assert cal <= 0.5 * rtn
    assert p_cal < p_rtn
    assert abs(p_rtn - rtn ** 2) < 1e-9 and abs(p_cal - cal ** 2) < 1e-9        # the proxy IS the squared output error on X
    assert wrel(f32(b, s)) > wrel(f32(b0, s0))                                   # what it costs: the plain weight error goes up


def test_compensation_past_six_scales_saturates_at_code_seven():
    # two strongly correlated inputs: the error of column 0 is pushed into column 1, which held the block's amax just below 6 * scale
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(512, 1, generator=g).double()
    X = torch.cat([x0, x0 + 0.05 * torch.randn(512, 1, generator=g).double(), torch.randn(512, 30, generator=g).double()], 1)
    H = X.t() @ X
    W = torch.zeros(2, 32)
    W[0, 0], W[0, 1] = 0.74, 5.9            # amax 5.9 = 0.7375 * 2^3 -> scale 1; 0.74 rounds DOWN to 0.5, error +0.24
    W[1] = -W[0]
    b0, s0 = quantize_mxfp4(W)
    assert s0.tolist() == [[127], [127]] and GC.codes_of(b0)[:, :2].tolist() == [[1, 7], [9, 15]]
    Wd, Hd = gptq_prepare(W, H, 0.01)
    U = gptq_factor(Hd)
    w1 = Wd[:, 1] - (Wd[:, 0] - torch.tensor([0.5, -0.5], dtype=torch.float64)) / U[0, 0] * U[0, 1]
    assert float(w1[0]) > 6.0 and float(w1[1]) < -6.0, w1      # the construction: compensation moved the weight past 6 * scale
    b, s = quantize_mxfp4_gptq(W, H)
    c = GC.codes_of(b)
    assert s.tolist() == [[127], [127]]                         # the scale was chosen before and does not change
    assert c[:, :2].tolist() == [[1, 7], [9, 15]]               # code 7 with the weight's sign: no wrap into the sign bit or to code 0
    assert torch.equal(dequantize_mxfp4(b, s, torch.float32)[:, 1], torch.tensor([6.0, -6.0]))


def test_dead_input_column_gets_zero_codes_and_does_not_leak():
    W, X, _ = GC.correlated_case(96, 64, 512, 1)
    X = X.clone()
    X[:, 17] = 0.0                          # an input that never fires
    H = X.t() @ X
    W2 = W.clone()
    W2[:, 17] = torch.linspace(-3.0, 3.0, 96)
    (b, s), (b2, s2) = quantize_mxfp4_gptq(W, H), quantize_mxfp4_gptq(W2, H)
    assert torch.equal(GC.codes_of(b)[:, 17], torch.zeros(96, dtype=torch.uint8))
    assert torch.equal(b, b2) and torch.equal(s, s2)            # whatever W holds there reaches no other column and no scale
    assert H[17, 17] == 0 and torch.equal(W[:, 17], GC.correlated_case(96, 64, 512, 1)[0][:, 17])     # (the inputs are not written)


def test_result_is_a_bf16_matrix():
    for N, K, T, seed in ((96, 64, 512, 0), (200, 256, 1024, 0)):
        b, s, _ = GC.definition(N, K, T, seed)
        Q = dequantize_mxfp4(b, s, torch.float32)
        assert torch.equal(Q, Q.bfloat16().float()) and torch.equal(dequantize_mxfp4(b, s).float(), Q)


def test_device_cases_respect_the_near_tie_cap():
    """the seeds of tests/test_gptq_ops_gpu.py: near-tie rows (where an fp32 run may legitimately pick another code) are few"""
    for N, K, T, seed in GC.DEVICE_CASES:
        _, _, tie = GC.definition(N, K, T, seed)
        print(f"({N}, {K}) seed {seed}: {int(tie.sum())} near-tie rows of {N}")
        assert int(tie.sum()) <= GC.NEAR_TIE_CAP * N


def test_definition_validation_names_the_argument():
    W, H = _w(4, 64, 5), torch.eye(64)
    for bad in (W[:, :40], W[0], torch.zeros(4, 64, dtype=torch.int32), torch.zeros(0, 64)):
        with pytest.raises(ValueError, match="W has to be"):
            quantize_mxfp4_gptq(bad, H[:bad.shape[-1], :bad.shape[-1]] if bad.dim() == 2 else H)
    Winf = W.clone()
    Winf[1, 2] = float("inf")
    with pytest.raises(ValueError, match="W: entries"):
        quantize_mxfp4_gptq(Winf, H)
    for bad in (torch.eye(32), torch.ones(64), torch.eye(64).long()):
        with pytest.raises(ValueError, match="H has to be"):
            quantize_mxfp4_gptq(W, bad)
    Hn = H.clone()
    Hn[3, 3] = float("nan")
    with pytest.raises(ValueError, match="H: entries"):
        quantize_mxfp4_gptq(W, Hn)
    Ha = H.clone()
    Ha[1, 2] = 0.3
    with pytest.raises(ValueError, match="H has to be symmetric"):
        quantize_mxfp4_gptq(W, Ha)
    Hneg = H.clone()
    Hneg[4, 4] = -1.0
    with pytest.raises(ValueError, match="H: the diagonal"):
        quantize_mxfp4_gptq(W, Hneg)
    for damp in (0.0, -0.01, float("nan"), float("inf"), None, "0.01", True):
        with pytest.raises(ValueError, match="damp"):
            quantize_mxfp4_gptq(W, H, damp)
    ind = -torch.ones(64, 64) + torch.diag(torch.full((64,), 1.5))      # symmetric, positive diagonal, indefinite
    with pytest.raises(ValueError, match="positive definite"):
        quantize_mxfp4_gptq(W, ind)


def test_calibration_resolver_runs_on_the_host():
    ids = torch.randint(0, 100, (3, 16), generator=torch.Generator().manual_seed(0))
    assert resolve_calibration(None, 100, 64) is None                                   # also with bf16 / bf16: nothing is asked
    r = resolve_calibration(dict(input_ids=ids), 100, 64, "mxfp4", "bf16")
    assert torch.equal(r["input_ids"], ids) and r["attention_mask"] is None and r["damp"] == 0.01 and r["n_tokens"] == 48
    am = torch.ones(3, 16, dtype=torch.long)
    am[0, :5] = 0
    am[2, :1] = 0
    r = resolve_calibration(dict(input_ids=ids.int(), attention_mask=am, damp=0.1), 100, 16, "bf16", "mxfp4")
    assert r["n_tokens"] == 42 and r["damp"] == 0.1 and r["input_ids"].dtype == torch.int64 and torch.equal(r["attention_mask"], am)
    ok = dict(input_ids=ids)
    for wd, hd in (("bf16", "bf16"), ("fp8", "bf16"), ("bf16", "fp8"), ("fp8", "fp8")):
        with pytest.raises(ValueError, match="mxfp4"):
            resolve_calibration(ok, 100, 64, wd, hd)
    for bad, word in ((ids, "dict"), ({}, "input_ids"), (dict(input_ids=ids.float()), "input_ids"), (dict(input_ids=ids[0]), "input_ids"),
                      (dict(input_ids=ids[:0]), "input_ids"), (dict(input_ids=ids + 100), "input_ids"), (dict(input_ids=ids - 100), "input_ids"),
                      (dict(input_ids=ids, attention_mask=am[:, :8]), "attention_mask"),
                      (dict(input_ids=ids, attention_mask=am.flip(1)), "attention_mask"),
                      (dict(input_ids=ids, attention_mask=torch.zeros(3, 16)), "attention_mask"),
                      (dict(input_ids=ids, damp=0), "damp"), (dict(input_ids=ids, damp="x"), "damp"),
                      (dict(input_ids=ids, dampen=0.1), "dampen")):
        with pytest.raises(ValueError, match=word):
            resolve_calibration(bad, 100, 64, "mxfp4", "mxfp4")
    with pytest.raises(ValueError, match="max_len"):
        resolve_calibration(ok, 100, 15, "mxfp4", "bf16")


def test_sweep_entry_validates_on_the_host():
    from spider_amd import lib as slib, ops
    assert len(slib.SIGNATURES["spider_gptq_mxfp4_sweep_f32"][1]) == 10 and callable(ops.gptq_mxfp4) and callable(ops.gptq_mxfp4_sweep)
    lib = slib.load()
    assert lib.spider_abi_version() == 4
    one = 16                                # any non-null, 16-byte-aligned value: validation fails before a launch
    call = lambda *p, N=8, K=64, j0=0, nb=1: lib.spider_gptq_mxfp4_sweep_f32(*(p or (one,) * 5), N, K, j0, nb, None)
    for i in range(5):
        assert call(*[None if k == i else one for k in range(5)]) == -1 and b"null" in lib.spider_last_error()
    for kw, word in ((dict(N=0), b"N must"), (dict(K=48), b"multiple of 32"), (dict(K=0), b"multiple of 32"), (dict(nb=0), b"1..4"),
                     (dict(nb=5), b"1..4"), (dict(j0=16), b"start at a block"), (dict(j0=-32), b"start at a block"),
                     (dict(j0=32, nb=2), b"within K"), (dict(j0=64), b"within K")):
        assert call(**kw) == -1, kw
        assert word in lib.spider_last_error(), (kw, lib.spider_last_error())
    assert call(one, 8, one, one, one) == -1 and b"aligned" in lib.spider_last_error()
    assert call(one, one, 24, one, one) == -1 and b"aligned" in lib.spider_last_error()
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.gptq_mxfp4(torch.zeros(4, 32), torch.eye(32))


def test_custom_op_registered_with_schema_and_fake_impl():
    import spider_amd.torch_ops as T
    assert T.GPTQ_OP_NAMES == ("gptq_mxfp4",)
    assert torch.ops.spider_hip.gptq_mxfp4.default._schema.name == "spider_hip::gptq_mxfp4"
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        b, s = torch.ops.spider_hip.gptq_mxfp4(torch.empty(40, 96, dtype=torch.bfloat16, device="cuda"),
                                               torch.empty(96, 96, dtype=torch.float64, device="cuda"), 0.02)
        assert tuple(b.shape) == (40, 48) and tuple(s.shape) == (40, 3) and b.dtype == torch.uint8 and s.dtype == torch.uint8

"""Host-side proof of tests/attn_checks.py and of the cases test_attention_matrix_gpu.py runs (no GPU):
  (a) on every case the 16-bit model of a correct kernel (attn_model16) stays within HALF the case's tolerance of attn_ref64, so the
      reference alone fits and half the tolerance is left for a kernel's summation order;
  (b) on the random-input cases of groups 2 .. 5, moving the visibility rule by one key at any boundary it has puts at least one
      element of attn_ref64 out of the case's tolerance: a mask that is one key off cannot pass;
  (c) on the count variant every such move changes the exact answer by at least 4 times its 2-ulp bound in some element;
and the pure-Python parts: visible() against a double loop, varlen_tiles() against the segment list."""
import pytest
import torch

import attn_checks as ac

N_CASES, cases = ac.N_CASES, ac.cases


def model_within_half(case):
    ref = ac.ref_of(case)
    B = case.q.shape[0]
    got = torch.stack([ac.attn_model16(case.q[b], case.k[b], case.v[b], case.vis[b], case.scale, case.dtype) for b in range(B)])
    worst = ac.err_over_tol(got, ref, ac.bound_of(case, ref))
    print(f"ATTN_MODEL16 group={6 if case.count else case.group} case={case.name} err/tol={worst:.4f}")
    assert worst <= 0.5, f"{case.name}: the 16-bit model alone uses {worst:.3f} of the tolerance"
    return worst


# ---------------------------------------------------------------------------------------------- the helper itself
@pytest.mark.parametrize("Lq,Lk,N,causal,kv_off,kv_beg", [(5, 7, 7, False, 0, 0), (5, 7, 9, True, 2, 1), (6, 6, 6, True, -2, 0),
                                                          (4, 9, 9, True, 3, 4), (3, 5, 8, False, 0, 5)])
def test_visible_flash_is_the_abi_rule(Lq, Lk, N, causal, kv_off, kv_beg):
    vis = ac.visible("flash", Lq, Lk, N, causal, kv_off, kv_beg)
    assert vis.dtype == torch.bool and tuple(vis.shape) == (Lq, N)
    for i in range(Lq):
        for j in range(N):
            assert bool(vis[i, j]) == (j < Lk and j >= kv_beg and (not causal or j <= i + kv_off)), (i, j)


def test_visible_varlen_and_decode_and_tiles():
    from spider_amd import ops
    cu = [0, 1, 4, 4, 9]
    vis = ac.visible("varlen", 9, 9, cu=cu)
    seg = [next(s for s in range(len(cu) - 1) if cu[s] <= r < cu[s + 1]) for r in range(9)]
    for i in range(9):
        for j in range(9):
            assert bool(vis[i, j]) == (seg[i] == seg[j]), (i, j)
    vis = ac.visible("decode", 1, 12, 12, kv_beg=3, kv_end=10)
    assert vis[0].tolist() == [3 <= j < 10 for j in range(12)]
    # varlen_tiles against the segment list of group 4: every query row in exactly one tile, tiles of at most 128 rows that stay
    # inside their segment, and each tile's key range is its segment
    cu = ac.varlen_case(64, ac.BF).par["cu"]
    seen = torch.zeros(cu[-1], dtype=torch.int32)
    for q0, qn, k0, kn in ops.varlen_tiles(cu, "cpu").tolist():
        assert 1 <= qn <= 128
        seen[q0:q0 + qn] += 1
        s = next(s for s in range(len(cu) - 1) if cu[s] <= q0 < cu[s + 1])
        assert (k0, k0 + kn) == (cu[s], cu[s + 1]) and q0 + qn <= cu[s + 1]
    assert bool((seen == 1).all())


def test_reference_conventions():
    """GQA head mapping, zeros for a row that sees nothing, junk in invisible slots ignored, count inputs exact"""
    q, k, v = ac.rnd(3, 4, 8, seed=1), ac.rnd(5, 2, 8, seed=2), ac.rnd(5, 2, 8, seed=3)
    vis = ac.visible("flash", 3, 5, 5, True, -1, 0)            # row 0 sees nothing
    ref = ac.attn_ref64(q, k, v, vis, 0.3)
    assert float(ref[0].abs().max()) == 0.0
    for h in range(4):
        for i in (1, 2):
            s = (k[:i, h // 2].double() @ q[i, h].double()) * 0.3
            want = torch.softmax(s, 0) @ v[:i, h // 2].double()
            assert float((ref[i, h] - want).abs().max()) < 1e-12
    k2, v2 = k.clone(), v.clone()
    k2[3:], v2[3:] = ac.JUNK, -ac.JUNK                          # keys 3, 4 are never visible (j <= i - 1 <= 1)
    assert torch.equal(ac.attn_ref64(q, k2, v2, vis, 0.3), ref)
    qc, kc, vc = ac.count_inputs(40, 16, ac.F16, Lq=40, Hq=2, Hkv=1)
    vis = ac.visible("flash", 40, 40, 40, True, -3, 2)
    exact = ac.count_ref(vis, 16)
    assert float((ac.attn_ref64(qc, kc, vc, vis, 0.25) - exact[:, None]).abs().max()) < 1e-15
    assert float(exact[:5].abs().max()) == 0.0 and abs(float(exact[39].sum()) - 1.0) < 1e-15


# ---------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("mode", ac.SWEEP_MODES)
@pytest.mark.parametrize("dtype", [ac.BF, ac.F16], ids=["bf16", "f16"])
def test_model16_fits_half_tolerance_head_dim_sweep(mode, dtype):
    for d in ac.SWEEP_D:
        model_within_half(ac.sweep_case(d, dtype, mode))


@pytest.mark.parametrize("count", [False, True], ids=["random", "count"])
@pytest.mark.parametrize("idx", range(N_CASES))
def test_model16_fits_half_tolerance(idx, count):
    model_within_half(cases(count)[idx])


# ---------------------------------------------------------------------------------------------- (b), (c)
@pytest.mark.parametrize("count", [False, True], ids=["random", "count"])
@pytest.mark.parametrize("idx", range(N_CASES))
def test_one_key_off_is_out_of_tolerance(idx, count):
    case = cases(count)[idx]
    ref = ac.ref_of(case)
    moves = ac.perturbations(case)
    labels = " ".join(label for label, *_ in moves)
    for boundary in {"flash": ("kv_beg", "kv_off"), "cache": ("kv_beg", "kv_off"), "decode": ("kv_beg", "kv_end"), "varlen": ("start", "end")}[case.kind]:
        assert boundary in labels, f"{case.name}: no effective move of {boundary}"
    for label, b, rows, vis in moves:
        moved = ac.attn_ref64(case.q[b][rows], case.k[b], case.v[b], vis, case.scale)
        base = ref[b][rows]
        if count:      # the exact answer of the unmoved rule, restated by the plain reference
            assert float((ac.attn_ref64(case.q[b][rows], case.k[b], case.v[b], case.vis[b][rows], case.scale) - base).abs().max()) < 1e-14
        diff = (moved - base).abs()
        out = (diff > 0) & (diff >= 4 * ac.bound_of(case, base)) if count else diff > ac.bound_of(case, base)
        assert bool(out.any()), f"{case.name}: {label} stays inside {'4 x ' if count else ''}the bound"

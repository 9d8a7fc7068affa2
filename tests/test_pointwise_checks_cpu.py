"""CPU tests of tests/pointwise_checks.py: the case tables, inputs and derived bounds of the pointwise / plumbing / small-conv GPU
tests are shown to be consistent, and to bite, before a GPU sees them.

Every kernel of the family is replayed in plain torch fp32 following the arithmetic and the rounding points its source documents
(csrc/unet_ops.hip, embed_kernel in csrc/llm_decode.hip, the activations of csrc/common.hpp). Two things are asserted:

* every case of the GPU tables, the large ones included, passes check() on the replay (none was too slow on the CPU to need a
  smaller stand-in);
* each seeded mutant of a replay -- the slips such kernels really make: a swapped half, a missing rounding, a wrong stride, a dropped
  tail or grid-stride trip, an off-by-one at a border -- is rejected by at least one case of its kernel's table. `mut` names the
  mutant inside each replay.
"""
import math

import pytest
import torch

import pointwise_checks as pc
from pointwise_checks import FILL, SWEEP

F32 = torch.float32
DT_IDS = [pc.name(d) for d in pc.DTYPES]


def caught(runs):
    """True if at least one of the callables raises AssertionError (a check rejected the mutant's output)"""
    for run in runs:
        try:
            run()
        except AssertionError:
            return True
    return False


# ------------------------------------------------------------------------------------------------------------------- activations
def sigmoid_rcp(y):
    return 1.0 / (1.0 + torch.exp(-y))


def erf_fast(x):
    ax = x.abs()
    t = 1.0 / (0.3275911 * ax + 1.0)
    p = 1.061405429 * t - 1.453152027
    p = p * t + 1.421413741
    p = p * t - 0.284496736
    p = p * t + 0.254829592
    return torch.copysign(1.0 - p * t * torch.exp(-ax * ax), x)


def act_f32(kind, x, param=0.0):
    if kind == "silu":
        return x * sigmoid_rcp(x)
    if kind == "gelu":
        return 0.5 * x * (1.0 + erf_fast(x * 0.70710678118654752))
    if kind == "quick_gelu":
        return x * sigmoid_rcp(torch.tensor(1.702, dtype=F32) * x)
    if kind == "tanh":
        return torch.tanh(x)
    if kind == "relu":
        return x.clamp_min(0)
    if kind == "leaky_relu":
        return torch.where(x > 0, x, x * torch.tensor(param, dtype=F32))
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------------------------- vector elementwise
def spoil(out, mut):
    """the output-side mutants of a vectorised grid-stride kernel, on a flat 16-bit result"""
    out = out.clone()
    if mut == "last_vector":
        out[-8:] = FILL
    elif mut == "trip2":
        out[SWEEP * 8:] = FILL
    elif mut == "halves":
        out = out.view(-1, 2).flip(1).reshape(-1)
    return out


def emu_vec(op, n, dt, mut=None):
    inp = pc.vec_inputs(n, dt)
    a, b = inp["a"].float(), inp["b"].float()
    if op[0] == "split_hilo":
        x = inp["x32"]
        hi = x.to(dt)
        return spoil(hi, mut), spoil((x - hi.float()).to(dt), mut)
    if op[0] == "act":
        y = act_f32(op[1], a, op[2])
    elif op[0] == "add":
        y = a + b
    elif op[0] == "add_scaled":
        s = torch.tensor(op[1], dtype=F32)
        y = a + b * s if mut == "scale_b_only" else (a + b) * s
    elif op[0] == "axpby":
        y = torch.tensor(op[1], dtype=F32) * a + torch.tensor(op[2], dtype=F32) * b
    return spoil(y.to(dt), mut)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", pc.VEC_OPS, ids=pc.op_id)
def test_vec_emulation_passes(op, dt):
    for n in pc.VEC_N:
        pc.vec_verify(op, n, dt, pc.vec_inputs(n, dt), emu_vec(op, n, dt))


@pytest.mark.parametrize("op", pc.VEC_OPS, ids=pc.op_id)
@pytest.mark.parametrize("mut", ["last_vector", "halves"])
def test_vec_mutants_small(op, mut):
    for dt in pc.DTYPES:
        assert caught(lambda n=n: pc.vec_verify(op, n, dt, pc.vec_inputs(n, dt), emu_vec(op, n, dt, mut)) for n in pc.VEC_N[:2]), (op, mut, dt)


@pytest.mark.parametrize("op", pc.VEC_OPS, ids=pc.op_id)
def test_vec_mutant_second_trip(op):
    """only the largest size reaches the second grid sweep: the two small ones must NOT notice, the large one must"""
    dt = torch.bfloat16
    for n in pc.VEC_N[:2]:
        pc.vec_verify(op, n, dt, pc.vec_inputs(n, dt), emu_vec(op, n, dt, "trip2"))
    n = pc.VEC_N[2]
    assert caught([lambda: pc.vec_verify(op, n, dt, pc.vec_inputs(n, dt), emu_vec(op, n, dt, "trip2"))])


@pytest.mark.parametrize("scale", [1 / 3, 0.5])
def test_add_scaled_mutant(scale):
    op = ("add_scaled", scale)
    for dt in pc.DTYPES:
        assert caught(lambda n=n: pc.vec_verify(op, n, dt, pc.vec_inputs(n, dt), emu_vec(op, n, dt, "scale_b_only")) for n in pc.VEC_N[:2])


# ------------------------------------------------------------------------------------------------------------------- geglu / swiglu
def emu_glu(kind, M, inner, dt, mut=None):
    x = pc.glu_inputs(M, inner, dt).float()
    if mut == "row_stride":         # row m read from m * inner instead of m * 2 * inner
        flat = x.reshape(-1)
        idx = torch.arange(M).view(M, 1) * inner + torch.arange(2 * inner).view(1, -1)
        x = flat[idx]
    a, b = x[:, :inner], x[:, inner:]
    if mut in ("halves", "act_on_wrong_half"):
        a, b = b, a
    lin, gate = (a, b) if kind == "geglu" else (b, a)
    f = act_f32("gelu" if kind == "geglu" else "silu", gate)
    if mut != "no_mid_rounding":
        f = f.to(dt).float()
    return (lin * f).to(dt)


GLU_MUTANTS = ["halves", "act_on_wrong_half", "no_mid_rounding", "row_stride"]


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["geglu", "swiglu"])
def test_glu_emulation_passes(kind, dt):
    for M, inner in pc.GLU_CASES:
        pc.glu_verify(kind, M, inner, dt, pc.glu_inputs(M, inner, dt), emu_glu(kind, M, inner, dt))


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["geglu", "swiglu"])
@pytest.mark.parametrize("mut", GLU_MUTANTS)
def test_glu_mutants(mut, kind, dt):
    assert caught(lambda M=M, inner=inner: pc.glu_verify(kind, M, inner, dt, pc.glu_inputs(M, inner, dt), emu_glu(kind, M, inner, dt, mut))
                  for M, inner in pc.GLU_CASES[:3])


def test_glu_second_trip():
    M, inner = pc.GLU_CASES[3]
    out = emu_glu("geglu", M, inner, torch.bfloat16).reshape(-1)
    out[SWEEP * 8:] = FILL
    assert caught([lambda: pc.glu_verify("geglu", M, inner, torch.bfloat16, pc.glu_inputs(M, inner, torch.bfloat16), out.view(M, inner))])


# ------------------------------------------------------------------------------------------------------------------- concat, embed
def emu_concat(case, dt, mut=None):
    a, b = pc.concat_inputs(*case, dt)
    rows, C1, C2 = case
    out = torch.cat([a, b], dim=-1)
    r = torch.arange(rows).view(rows, 1)
    if mut == "b_stride_C1":
        out[:, C1:] = b.reshape(-1)[(r * C1 + torch.arange(C2).view(1, -1)) % b.numel()]
    elif mut == "boundary_source":      # the first vector behind the seam still taken from a
        out[:, C1:C1 + 8] = a.reshape(-1)[(r * C1 + C1 + torch.arange(8).view(1, -1)) % a.numel()]
    elif mut == "trip2":
        out.view(-1)[SWEEP * 8:] = FILL
    return out


@pytest.mark.parametrize("dt", pc.DTYPES + (F32,), ids=DT_IDS + ["f32"])
def test_concat_emulation_passes(dt):
    for case in (pc.CONCAT32_CASES if dt == F32 else pc.CONCAT_CASES):
        pc.concat_verify(case, dt, pc.concat_inputs(*case, dt), emu_concat(case, dt))


@pytest.mark.parametrize("mut", ["b_stride_C1", "boundary_source", "trip2"])
def test_concat_mutants(mut):
    for dt in pc.DTYPES:
        assert caught(lambda c=c: pc.concat_verify(c, dt, pc.concat_inputs(*c, dt), emu_concat(c, dt, mut)) for c in pc.CONCAT_CASES)
    if mut != "trip2":
        assert caught(lambda c=c: pc.concat_verify(c, F32, pc.concat_inputs(*c, F32), emu_concat(c, F32, mut)) for c in pc.CONCAT32_CASES)


def emu_embed(case, dt, mut=None):
    table, ids = pc.embed_inputs(*case, dt)
    Vn, H = table.shape
    if mut == "no_clamp":
        idx = (ids.long().view(-1, 1) * H + torch.arange(H).view(1, -1)) % table.numel()
        return table.reshape(-1)[idx]
    out = table[ids.long().clamp(0, Vn - 1)].clone()
    if mut == "vec256_up":
        out[:, 2048:] = FILL
    return out


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_embed_emulation_and_mutants(dt):
    for case in pc.EMBED_CASES:
        pc.embed_verify(case, dt, pc.embed_inputs(*case, dt), emu_embed(case, dt))
    for mut in ("no_clamp", "vec256_up"):
        assert caught(lambda c=c: pc.embed_verify(c, dt, pc.embed_inputs(*c, dt), emu_embed(c, dt, mut)) for c in pc.EMBED_CASES), mut


# ------------------------------------------------------------------------------------------------------------------- short reductions
def emu_mean(case, dt, mut=None):
    x = pc.mean_inputs(*case, dt).float()
    B, T, Cn = case
    if mut == "batch_stride":       # batch b starts one row late per batch before it
        idx = ((torch.arange(B).view(B, 1, 1) * (T + 1) + torch.arange(T).view(1, T, 1)) * Cn + torch.arange(Cn).view(1, 1, Cn)) % x.numel()
        x = x.reshape(-1)[idx]
    s = torch.zeros(B, Cn)
    for t in range(T):
        s = s + x[:, t]
    return (s / (T - 1 if mut == "div_T_minus_1" else T)).to(dt)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_mean_tokens_emulation_and_mutants(dt):
    for case in pc.MEAN_CASES:
        pc.mean_verify(case, dt, pc.mean_inputs(*case, dt), emu_mean(case, dt))
    for mut in ("div_T_minus_1", "batch_stride"):
        assert caught(lambda c=c: pc.mean_verify(c, dt, pc.mean_inputs(*c, dt), emu_mean(c, dt, mut)) for c in pc.MEAN_CASES), mut


def emu_moe(case, dt, mut=None):
    xs, logits = pc.moe_inputs(*case, dt)
    E, B = len(xs), logits.shape[0]
    l = logits.float()
    if mut == "prev_row":
        l = torch.roll(l, 1, 0)
    r = 1.0 / (1.0 + torch.exp(-l))
    rs = torch.zeros(B)
    for e in range(E + 1 if mut == "col_E" else E):
        rs = rs + r[:, e]
    acc = torch.zeros(B, xs[0].numel() // B)
    for e in range(E):
        w16 = (r[:, e] / rs).to(dt).float().view(B, 1)
        acc = acc + (xs[e].float().reshape(B, -1) * w16).to(dt).float()
    return acc.to(dt).view(xs[0].shape)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_moe_combine_emulation_and_mutants(dt):
    for case in pc.MOE_CASES:
        pc.moe_verify(case, dt, pc.moe_inputs(*case, dt), emu_moe(case, dt))
    for mut in ("col_E", "prev_row"):
        assert caught(lambda c=c: pc.moe_verify(c, dt, pc.moe_inputs(*c, dt), emu_moe(c, dt, mut)) for c in pc.MOE_CASES[:6]), mut


def emu_l2(case, dt, mut=None):
    x = pc.l2_inputs(*case, dt).float()
    ss = (x * x).sum(1, keepdim=True)
    eps = torch.tensor(pc.L2_EPS, dtype=F32)
    inv = 1.0 / torch.sqrt(torch.maximum(ss, eps)) if mut == "eps_on_square" else 1.0 / torch.maximum(torch.sqrt(ss), eps)
    return (x * inv).to(dt)


def test_l2_normalize_emulation_and_mutant():
    for dt in pc.DTYPES:
        for case in pc.L2_CASES:
            pc.l2_verify(case, dt, pc.l2_inputs(*case, dt), emu_l2(case, dt))
    dt = torch.bfloat16             # the row of 2^-60 values exists in the bf16 table only
    for case in pc.L2_CASES:        # every bf16 case carries that row, so every one catches the mutant
        assert caught([lambda: pc.l2_verify(case, dt, pc.l2_inputs(*case, dt), emu_l2(case, dt, "eps_on_square"))]), case


def emu_softmax(case, scale, dt, mut=None):
    rows, n, nv = case
    x = pc.softmax_inputs(*case)
    s = torch.tensor(scale, dtype=F32)
    m = (x if mut == "pad_in_max" else x[:, :nv]).max(1, keepdim=True).values * s
    z = (x - m) if mut == "scale_on_m_only" else (x * s - m)
    e = torch.exp(z)
    tot = (e if mut == "pad_in_sum" else e[:, :nv]).sum(1, keepdim=True)
    out = (e * (1.0 / tot)).to(dt)
    out[:, nv:] = FILL if mut == "pad_not_zeroed" else 0.0
    return out


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("scale", pc.SOFTMAX_SCALES)
def test_softmax_rows_emulation_and_mutants(scale, dt):
    for case in pc.SOFTMAX_CASES:
        pc.softmax_verify(case, scale, dt, pc.softmax_inputs(*case), emu_softmax(case, scale, dt))
    for mut in ("pad_in_max", "pad_in_sum", "pad_not_zeroed", "scale_on_m_only"):
        assert caught(lambda c=c: pc.softmax_verify(c, scale, dt, pc.softmax_inputs(*c), emu_softmax(c, scale, dt, mut))
                      for c in pc.SOFTMAX_CASES), mut


# ------------------------------------------------------------------------------------------------------------------- pack_keep_bits
def emu_pack(case, mut=None):
    n, nv = case
    u = pc.pack_inputs(n)
    nw = (n + 63) // 64
    idx = torch.arange(nw * 64)
    up = torch.cat([u, torch.ones(nw * 64 - n)])
    keep = (idx < n) & (up <= pc.PACK_THR if mut == "le" else up < pc.PACK_THR)
    if mut != "ignore_n_valid":
        keep &= idx < nv
    bits = keep.view(nw, 64)
    if mut == "reversed":
        bits = bits.flip(1)
    return (bits.long() << torch.arange(64)).sum(1)


def test_pack_keep_bits_emulation_and_mutants():
    for case in pc.pack_cases():
        pc.pack_verify(case, pc.pack_inputs(case[0]), emu_pack(case))
    for mut in ("le", "ignore_n_valid", "reversed"):
        assert caught(lambda c=c: pc.pack_verify(c, pc.pack_inputs(c[0]), emu_pack(c, mut)) for c in pc.pack_cases()), mut


# ------------------------------------------------------------------------------------------------------------------- latent plumbing
def emu_latent(case, reps, scale, dt, mut=None):
    B, Cn, H, W = case
    lat = pc.map_input("lat", *case)
    v = (lat * torch.tensor(scale, dtype=F32)).to(dt)
    v = v.reshape(B, H, W, Cn) if mut == "index_order" else v.permute(0, 2, 3, 1)
    out = v.unsqueeze(0).expand(reps, B, H, W, Cn).reshape(reps * B, H, W, Cn).clone()
    if mut == "replica0" and reps > 1:
        out[B:] = FILL
    return out


@pytest.mark.parametrize("dt", pc.DTYPES + (F32,), ids=DT_IDS + ["f32"])
def test_latent_to_nhwc_emulation_and_mutants(dt):
    runs = {"index_order": [], "replica0": []}
    for case in pc.MAPS:
        for reps in pc.REPS:
            for scale in pc.LATENT_SCALES:
                lat = pc.map_input("lat", *case)
                pc.latent_verify(case, reps, scale, dt, lat, emu_latent(case, reps, scale, dt))
                for mut in runs:
                    runs[mut].append(lambda a=(case, reps, scale), mut=mut: pc.latent_verify(*a, dt, pc.map_input("lat", *a[0]), emu_latent(*a, dt, mut)))
    for mut in runs:
        assert caught(runs[mut]), mut


def emu_cfg(case, mut=None):
    B, Cn, H, W = case
    e2 = pc.map_input("cfg", 2 * B, H, W, Cn)
    eu, ec = (e2[B:], e2[:B]) if mut == "swapped" else (e2[:B], e2[B:])
    v = eu + torch.tensor(pc.GUIDANCE, dtype=F32) * (ec - eu)
    return v.reshape(B, Cn, H, W) if mut == "index_order" else v.permute(0, 3, 1, 2)


def emu_lincomb(case, coefs, mut=None):
    xs = [pc.map_input(f"lin{j}", *case) for j in range(len(coefs))]
    a = torch.zeros_like(xs[0])
    for c, x in zip(coefs, xs):
        a = a + torch.tensor(c, dtype=F32) * x
    return a


def emu_nchw(case, aff, mut=None):
    B, Cn, H, W = case
    mul, add, clamp = aff
    v = pc.nchw_input(case) * torch.tensor(mul, dtype=F32) + torch.tensor(add, dtype=F32)
    if clamp:
        v = v.clamp(0, 1)
    return v.reshape(B, Cn, H, W) if mut == "index_order" else v.permute(0, 3, 1, 2)


def test_cfg_lincomb_nchw_emulation_and_mutants():
    for case in pc.MAPS:
        B, Cn, H, W = case
        pc.cfg_verify(case, pc.map_input("cfg", 2 * B, H, W, Cn), emu_cfg(case))
        for coefs in pc.LINCOMB_COEFS:
            pc.lincomb_verify(case, coefs, [pc.map_input(f"lin{j}", *case) for j in range(len(coefs))], emu_lincomb(case, coefs))
        for aff in pc.NCHW_AFFINES:
            pc.nchw_verify(case, aff, pc.nchw_input(case), emu_nchw(case, aff))
    small = pc.MAPS[:3]
    for mut in ("swapped", "index_order"):
        assert caught(lambda c=c: pc.cfg_verify(c, pc.map_input("cfg", 2 * c[0], c[2], c[3], c[1]), emu_cfg(c, mut)) for c in small), mut
    for aff in pc.NCHW_AFFINES:
        assert caught(lambda c=c: pc.nchw_verify(c, aff, pc.nchw_input(c), emu_nchw(c, aff, "index_order")) for c in small), aff


# ------------------------------------------------------------------------------------------------------------------- conv_transpose1d
def c_rem(a, b):
    """C's %: the sign of the dividend"""
    return int(math.fmod(a, b))


def emu_ct1d(case, dt, use_bias, mut=None):
    L, Cin, Cout, k, stride, pad = case
    x, w, bias, taps = pc.ct1d_inputs(case, dt)
    B = x.shape[0]
    cols = (x.float().reshape(-1, Cin) @ taps.float().T).reshape(-1)         # [B, L, k, Cout] fp32
    L_out = (L - 1) * stride - 2 * pad + k
    out = torch.zeros(B, L_out, Cout)
    co = torch.arange(Cout)
    for b in range(B):
        for t in range(L_out):
            v = torch.zeros(Cout)
            j = c_rem(t - pad, stride) if mut == "tap_phase" else (t + pad) % stride
            while j < k:
                num = t + pad - j
                i = int(num / stride)                                       # C division truncates towards zero
                if not (num < 0 or (i >= L and mut != "no_clip")):
                    v = v + cols[(((b * L + i) * k + j) * Cout + co) % cols.numel()]
                    if use_bias and mut == "bias_per_tap":
                        v = v + bias.float()
                j += stride
            if use_bias and mut != "bias_per_tap":
                v = v + bias.float()
            out[b, t] = v
    return out.to(dt)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_conv_transpose1d_emulation_and_mutants(dt):
    for case in pc.CT1D_CASES:
        for use_bias in (True, False):
            pc.ct1d_verify(case, dt, pc.ct1d_inputs(case, dt), use_bias, emu_ct1d(case, dt, use_bias))
    for mut in ("tap_phase", "no_clip", "bias_per_tap"):
        assert caught(lambda c=c: pc.ct1d_verify(c, dt, pc.ct1d_inputs(c, dt), True, emu_ct1d(c, dt, True, mut)) for c in pc.CT1D_CASES), mut


# ------------------------------------------------------------------------------------------------------------------- small convs
def gather_taps(x, ks, mut=None):
    """x [B, H, W, Cin] fp32 -> [B H W, ks ks, Cin]: the input value under every tap, zero outside the image"""
    B, H, W, Cin = x.shape
    pad = ks // 2 - (1 if mut == "pad_off_by_one" else 0)
    flat = x.reshape(-1, Cin)
    pix = torch.arange(B * H * W)
    ox, oy, b = pix % W, (pix // W) % H, pix // (W * H)
    out = torch.zeros(B * H * W, ks * ks, Cin)
    for ky in range(ks):
        for kx in range(ks):
            dy, dx = (kx, ky) if mut == "taps_transposed" else (ky, kx)
            iy, ix = oy + dy - pad, ox + dx - pad
            idx = (b * H + iy) * W + ix
            ok = (iy >= 0) & (iy < H)
            ok &= ((idx >= 0) & (idx < flat.shape[0])) if mut == "bleed" else ((ix >= 0) & (ix < W))      # bleed: no column check
            out[:, ky * ks + kx] = torch.where(ok.view(-1, 1), flat[idx.clamp(0, flat.shape[0] - 1)], torch.zeros(()))
    return out


def emu_conv_bias(case, bias, mut):
    if not case[6]:
        return torch.zeros(case[4])
    return (torch.roll(bias, -1) if mut == "bias_next" else bias).float()


def emu_cin(case, dt, f32in, mut=None):
    """conv_small_cin_kernel: acc = bias, then += x w over (ky, kx, c) in that order; -> (y16, y32)"""
    x, w, bias = pc.conv_inputs(case, dt)
    B, H, W, Cin, Cout, ks, _ = case
    xv = gather_taps(x if f32in else x.to(dt).float(), ks, mut)
    wf = w.float().reshape(Cout, ks * ks, Cin)
    acc = emu_conv_bias(case, bias, mut).view(1, Cout).expand(B * H * W, Cout).clone()
    for tap in range(ks * ks):
        for c in range(Cin):
            acc = acc + xv[:, tap, c:c + 1] * wf[:, tap, c].view(1, Cout)
    if mut == "trip2":
        acc.view(-1, 8)[512 * 256:] = FILL
    acc = acc.view(B, H, W, Cout)
    return acc.to(dt), acc


def emu_cout(case, dt, f32in, mut=None):
    """conv_small_cout_kernel: lane l sums its 8-channel chunks l, l + 64, ..; wave_sum; + bias; -> (y16, y32)"""
    x, w, bias = pc.conv_inputs(case, dt)
    B, H, W, Cin, Cout, ks, _ = case
    cvn = Cin // 8
    xv = gather_taps(x if f32in else x.to(dt).float(), ks, mut).reshape(B * H * W, 1, ks * ks * cvn, 8)
    wf = w.float().reshape(1, Cout, ks * ks * cvn, 8)
    ch = (xv * wf).sum(-1)                                    # [pixels, Cout, chunks]
    nch = ch.shape[-1]
    trips = (nch + 63) // 64
    ch = torch.cat([ch, torch.zeros(*ch.shape[:-1], trips * 64 - nch)], dim=-1).view(*ch.shape[:-1], trips, 64)
    lanes = ch[..., 0, :].clone()
    for k in range(1, 1 if mut == "drop_chunks" else trips):
        lanes = lanes + ch[..., k, :]
    acc = lanes.sum(-1) + emu_conv_bias(case, bias, mut).view(1, Cout)
    if mut == "trip2":
        acc[2048 * 4:] = FILL
    acc = acc.view(B, H, W, Cout)
    return acc.to(dt), acc


CONV_MUTANTS = ["taps_transposed", "pad_off_by_one", "bleed", "bias_next", "trip2"]


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("f32in", [False, True])
def test_conv_small_cin_emulation_and_mutants(f32in, dt):
    what = "conv2d_small_cin" + ("_f32in" if f32in else "")
    for case in pc.cin_cases():
        y16, y32 = emu_cin(case, dt, f32in)
        pc.conv_verify(what, case, dt, f32in, y16, y32 if f32in else None)
    for mut in CONV_MUTANTS:
        assert caught(lambda c=c: pc.conv_verify(what, c, dt, f32in, emu_cin(c, dt, f32in, mut)[0]) for c in pc.cin_cases()), mut
    # the fp32 twin ties the 16-bit output down to the bit
    case = pc.cin_cases()[-1]
    y16, y32 = emu_cin(case, dt, True)
    assert caught([lambda: pc.conv_verify(what, case, dt, True, y16, y32 * (1 + 2.0 ** -12))])


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("f32in", [False, True])
def test_conv_small_cout_emulation_and_mutants(f32in, dt):
    what = "conv2d_small_cout" + ("_f32in" if f32in else "")
    for case in pc.cout_cases():
        y16, y32 = emu_cout(case, dt, f32in)
        pc.conv_verify(what, case, dt, f32in, None if f32in else y16, y32)
    for mut in CONV_MUTANTS + ["drop_chunks"]:
        assert caught(lambda c=c: pc.conv_verify(what, c, dt, f32in, None, emu_cout(c, dt, f32in, mut)[1]) for c in pc.cout_cases()), mut

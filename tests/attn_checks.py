"""Shared by the attention parity tests (test_attention_matrix_gpu.py on the device, test_attention_checks_cpu.py on the host): the
visibility rule of the attention ABI restated in plain torch, an fp64 reference, a model of the error a correct 16-bit kernel is
allowed, the exact "count" inputs, and the list of cases both files walk. Everything here is host code on CPU tensors.

Layout of a case (logical, the GPU test permutes into what each op takes): q [B, Lq, Hq, d], k / v [B, N, Hkv, d] with N >= Lk
slots, vis = one bool [Lq, N] per batch row. Slots no correct kernel may read (below kv_beg, at or past Lk / kv_end) hold +-3e4."""
import functools
import math

import torch

BF, F16 = torch.bfloat16, torch.float16
JUNK = 3.0e4

# (atol, rtol) of the project's tests: test_attention / test_attention_short_sequences / test_attn_decode / test_attn_decode_fused
TOL_FLASH = {BF: (1.5e-2, 1.5e-2), F16: (3e-3, 3e-3)}
TOL_DECODE = (1e-2, 1e-2)
TOL_FUSED_VS_UNFUSED = (4e-3, 1e-2)
# count variant: 2 ulp of the output type relative to the exact value. Exact integer sums, one fp32 reciprocal or division, one
# fp32 multiply and one rounding to 16 bits stay inside 1 ulp; the second is margin for the division form of the decode kernels.
COUNT_RTOL = {BF: 2.0 ** -7, F16: 2.0 ** -10}


def rnd(*shape, seed=0, scale=1.0, dtype=BF):
    """the rnd() recipe of test_hip_ops.py (seeded randn, rounded to bf16), then the case's 16-bit type"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(dtype)


def junk(*shape, seed=0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randint(0, 2, shape, generator=g).float() * 2 - 1) * JUNK).to(dtype)


# ---------------------------------------------------------------------------------------------- the visibility rule
def visible(op_kind, Lq, Lk, n_slots=None, causal=False, kv_off=0, kv_beg=0, kv_end=None, cu=None):
    """bool [Lq, n_slots] of one batch row: may query i see key slot j? (the ABI comment of attn_flash.hip / llm_decode.hip)
      'flash'  (attention, attention_cache): j < Lk and j >= kv_beg; causal adds j <= i + kv_off
      'varlen' (attention_varlen): i and j lie in the same cu_seqlens segment (Lq == Lk == cu[-1])
      'decode' (attn_decode, attn_decode_fused): kv_beg <= j < kv_end (Lq == 1)"""
    n = Lk if n_slots is None else n_slots
    i, j = torch.arange(Lq)[:, None], torch.arange(n)[None]
    if op_kind == "flash":
        vis = ((j < Lk) & (j >= kv_beg)).expand(Lq, n)
        return (vis & (j <= i + kv_off) if causal else vis).clone()
    if op_kind == "varlen":
        seg = torch.bucketize(torch.arange(n), torch.tensor(list(cu[1:])), right=True)
        return seg[:Lq, None] == seg[None]
    if op_kind == "decode":
        return ((j >= kv_beg) & (j < kv_end) & (j < n)).expand(Lq, n).clone()
    raise ValueError(op_kind)


# ---------------------------------------------------------------------------------------------- references
def _attn(q, k, v, vis, scale, dtype):
    Hq, Hkv = q.shape[1], k.shape[1]
    hk = torch.arange(Hq) // (Hq // Hkv)
    qd, kd, vd = q.double().transpose(0, 1), k.double().transpose(0, 1)[hk], v.double().transpose(0, 1)[hk]
    s = (qd @ kd.transpose(1, 2) * scale).masked_fill(~vis[None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = p.sum(-1, keepdim=True)
    if dtype is not None:
        p = p.to(dtype).double()
    o = p @ vd
    o = torch.where(l > 0, o / l.clamp(min=1e-300), torch.zeros_like(o))
    if dtype is not None:
        o = o.to(dtype).double()
    return o.transpose(0, 1)


def attn_ref64(q, k, v, vis, scale):
    """Plain fp64 softmax attention of one batch row on the (16-bit-rounded) inputs as given: q [Lq, Hq, d], k / v [N, Hkv, d],
    vis bool [Lq, N] -> fp64 [Lq, Hq, d]. GQA: query head hq reads kv head hq // (Hq // Hkv). A row with no visible key is 0."""
    return _attn(q, k, v, vis, scale, None)


def attn_model16(q, k, v, vis, scale, dtype):
    """attn_ref64 with the unnormalised probabilities exp(s - max) rounded to `dtype` before the PV product (what the MFMA of a
    flash kernel multiplies) and the output rounded to `dtype`: the error a correct 16-bit kernel is allowed."""
    return _attn(q, k, v, vis, scale, dtype)


def count_inputs(Lk, d, dtype, Lq=1, Hq=1, Hkv=1, seed=0):
    """q = 0 [Lq, Hq, d], k random [Lk, Hkv, d], v[j, :, c] = 1 if j % d == c else 0. Every score is exactly 0 and every visible
    probability exactly 1, all sums are small integers (exact in fp32): out[i, c] = |{visible j : j % d == c}| / n_i."""
    v = torch.zeros(Lk, Hkv, d, dtype=dtype)
    v[torch.arange(Lk), :, torch.arange(Lk) % d] = 1
    return torch.zeros(Lq, Hq, d, dtype=dtype), rnd(Lk, Hkv, d, seed=seed, dtype=dtype), v


def count_ref(vis, d):
    """the exact answer of the count inputs for one batch row: fp64 [Lq, d] (the same for every head)"""
    N = vis.shape[1]
    onehot = torch.zeros(N, d, dtype=torch.float64)
    onehot[torch.arange(N), torch.arange(N) % d] = 1
    n = vis.sum(-1, keepdim=True).double()
    return torch.where(n > 0, (vis.double() @ onehot) / n.clamp(min=1), torch.zeros(1, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, group, kind, dtype, q, k, v, vis, tol, count=False, **par):
        self.name, self.group, self.kind, self.dtype, self.count = name, group, kind, dtype, count
        self.q, self.k, self.v, self.vis, self.tol, self.par = q, k, v, vis, tol, par
        self.d = q.shape[-1]
        self.scale = 1.0 / math.sqrt(self.d)

    def __repr__(self):
        return self.name


_REF = {}


def ref_of(case):
    """fp64 [B, Lq, Hq, d], computed once per case name and shared; callers must not write into it"""
    if case.name not in _REF:
        B, Lq, Hq, d = case.q.shape
        if case.count:
            r = torch.stack([count_ref(case.vis[b], d)[:, None].expand(Lq, Hq, d) for b in range(B)])
        else:
            r = torch.stack([attn_ref64(case.q[b], case.k[b], case.v[b], case.vis[b], case.scale) for b in range(B)])
        _REF[case.name] = r
    return _REF[case.name]


def bound_of(case, ref, tol=None):
    """elementwise allowed |got - ref|"""
    if case.count:
        return COUNT_RTOL[case.dtype] * ref.abs()
    atol, rtol = tol or case.tol
    return atol + rtol * ref.abs()


def err_over_tol(got, ref, bound):
    """max over elements of |got - ref| / bound (0 / 0 = 0: an exact zero where exactly zero is demanded)"""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    return float(ratio.max())


def check(got, case, what="", ref=None, tol=None):
    """got [B, Lq, Hq, d] (CPU, any float type) against the case's reference: finite everywhere, every element within the bound
    (exactly 0 where the reference is exactly 0 in the count variant). Prints the worst err / tol before asserting; returns it."""
    ref = ref_of(case) if ref is None else ref
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    assert bool(torch.isfinite(got.float()).all()), f"{case.name} {what}: output not finite"
    for b, vis in enumerate(case.vis):      # a query row that sees no key (left padding, kv_off < 0) is exactly 0, not merely small
        dead = ~vis.any(-1)
        assert not bool(got[b, dead].float().abs().any()), f"{case.name} {what}: fully masked rows of batch row {b} are not exactly 0"
    worst = err_over_tol(got, ref, bound_of(case, ref, tol))
    print(f"ATTN_MATRIX group={6 if case.count else case.group} case={case.name} {what} err/tol={worst:.4f}")
    assert worst <= 1.0, f"{case.name} {what}: worst err / tol = {worst:.4g}"
    return worst


def _fill(dtype, count, B, N, Hkv, d, Lq, Hq, seed, scale=1.0):
    """q, k, v of a case before the junk slots are written"""
    if count:
        qs, ks, vs = zip(*[count_inputs(N, d, dtype, Lq, Hq, Hkv, seed=seed + 10 * b) for b in range(B)])
        return torch.stack(qs), torch.stack(ks), torch.stack(vs)
    return (rnd(B, Lq, Hq, d, seed=seed + 1, scale=scale, dtype=dtype), rnd(B, N, Hkv, d, seed=seed + 2, scale=scale, dtype=dtype),
            rnd(B, N, Hkv, d, seed=seed + 3, scale=scale, dtype=dtype))


def _junk_outside(k, v, lo, hi, seed):
    """slots outside [lo[b], hi[b]) of batch row b hold +-3e4"""
    B, N = k.shape[:2]
    jk, jv = junk(*k.shape, seed=seed + 7, dtype=k.dtype), junk(*v.shape, seed=seed + 8, dtype=v.dtype)
    for b in range(B):
        out = torch.ones(N, dtype=torch.bool)
        out[lo[b]:hi[b]] = False
        k[b, out], v[b, out] = jk[b, out], jv[b, out]


def _tag(dtype, count):
    return ("f16" if dtype == F16 else "bf16") + ("-count" if count else "")


def flash_case(name, group, dtype, B, Hq, Hkv, Lq, Lk, d, causal=False, kv_off=None, kv_beg=None, n_slots=None, count=False,
               kind="flash", seed=0):
    """ops.attention (kind 'flash': n_slots == Lk) or ops.attention_cache (kind 'cache': caches of n_slots = T_max slots)"""
    N = n_slots or Lk
    off = Lk - Lq if kv_off is None else kv_off
    beg = [0] * B if kv_beg is None else list(kv_beg)
    q, k, v = _fill(dtype, count, B, N, Hkv, d, Lq, Hq, seed)
    _junk_outside(k, v, beg, [Lk] * B, seed)
    vis = [visible("flash", Lq, Lk, N, causal, off, beg[b]) for b in range(B)]
    tol = TOL_FLASH[dtype]
    return Case(f"{name}-{_tag(dtype, count)}", group, kind, dtype, q, k, v, vis, tol, count, Lk=Lk, causal=causal, kv_off=kv_off,
                off=off, kv_beg=kv_beg, beg=beg)


SWEEP_D = list(range(8, 161, 8))
SWEEP_MODES = ("ragged", "tiles", "masked")


def sweep_case(d, dtype, mode):
    """group 1: ops.attention over every head dim of the ABI"""
    if mode == "ragged":      # plain flash kernel, partial last key tile
        return flash_case(f"sweep-ragged-d{d}", 1, dtype, 1, 2, 2, 70, 150, d, seed=100 + d)
    if mode == "tiles":       # whole 64-key tiles: pipelined for d <= 96 (KQ = 3 for d <= 48), ragged second query tile
        return flash_case(f"sweep-tiles-d{d}", 1, dtype, 1, 2, 2, 200, 192, d, seed=300 + d)
    return flash_case(f"sweep-masked-d{d}", 1, dtype, 2, 4, 2, 150, 150, d, causal=True, kv_beg=[0, 70], seed=500 + d)


PREFILL_BEG = [0, 1, 63, 64, 65, 127, 128, 129, 255, 299]
PREFILL = [(128, BF), (64, BF), (128, F16)]


def prefill_case(d, dtype, count=False):
    """group 2: attention_cache as LlamaEngine._prefill calls it (Lk = S, causal, kv_off = 0, left padding per row)"""
    return flash_case(f"prefill-d{d}", 2, dtype, len(PREFILL_BEG), 4, 2, 300, 300, d, causal=True, kv_off=0, kv_beg=PREFILL_BEG,
                      n_slots=320, count=count, kind="cache", seed=700 + d)


KVOFF = [(70, 300, None, None), (130, 194, 64, None), (128, 191, 63, None), (100, 300, 37, None), (70, 70, -5, None),
         (130, 194, 64, (0, 66))]
KVOFF_D = (128, 80)


def kvoff_case(d, Lq, Lk, kv_off, kv_beg, count=False):
    """group 3: ops.attention, causal with Lq != Lk"""
    B = 1 if kv_beg is None else len(kv_beg)
    name = f"kvoff-d{d}-{Lq}x{Lk}-off{'dflt' if kv_off is None else kv_off}" + ("" if kv_beg is None else "-beg" + "_".join(map(str, kv_beg)))
    return flash_case(name, 3, BF, B, 4, 2, Lq, Lk, d, causal=True, kv_off=kv_off, kv_beg=kv_beg, count=count, seed=900 + d + Lq)


VARLEN_SEGS = [1, 63, 64, 65, 127, 128, 129, 300, 2]
VARLEN = [(d, dt) for d in (64, 80, 128) for dt in (BF, F16)]


def varlen_case(d, dtype, count=False):
    """group 4: attention_varlen over packed segments"""
    cu = [0]
    for n in VARLEN_SEGS:
        cu.append(cu[-1] + n)
    T = cu[-1]
    Hq, Hkv = (4, 2) if d == 128 else (3, 3)
    q, k, v = _fill(dtype, count, 1, T, Hkv, d, T, Hq, 1100 + d)
    return Case(f"varlen-d{d}-{_tag(dtype, count)}", 4, "varlen", dtype, q, k, v, [visible("varlen", T, T, cu=cu)], TOL_FLASH[dtype],
                count, cu=cu)


# name, (n_q, n_kv), kv_beg per row, kv_end per row, nsplit, T_max. kv_end counts the newest token (the one attn_decode_fused appends).
# T_max = 800 with nsplit 8 makes attn_decode_fused take its 8-wave form (T_max / nsplit >= 96), the others the 4-wave form.
DECODE = [("len1", (28, 4), [5], [6], 8, 9), ("len7", (32, 8), [0], [7], 8, 10), ("len9", (8, 8), [5], [14], 8, 17),
          ("len300", (4, 2), [0], [300], 8, 800), ("len1537", (7, 1), [5], [1542], 64, 1545),
          ("nearempty", (28, 4), [297], [300], 8, 800), ("rows3", (32, 8), [0, 17, 63], [130, 97, 64], 8, 133)]


def decode_case(name, count=False):
    """group 5: attn_decode / attn_decode_fused, d = 128, bf16"""
    _, (n_q, n_kv), beg, end, nsplit, T_max = next(c for c in DECODE if c[0] == name)
    B, d = len(beg), 128
    q, k, v = _fill(BF, count, B, T_max, n_kv, d, 1, n_q, 1300 + T_max + n_q)
    _junk_outside(k, v, beg, end, 1300 + T_max)
    # One query row per head: a junk key of random signs scores +-huge, and at -huge a stray read of it would weigh nothing. So the
    # junk keys of a kv head are aligned with its first query head (score = +3e4 * sum |q| * scale): a stray read always shows.
    for b in range(B):
        outside = torch.ones(T_max, dtype=torch.bool)
        outside[beg[b]:end[b]] = False
        sgn = torch.where(q[b, 0, ::n_q // n_kv].float() < 0, -1.0, 1.0)                    # [n_kv, d]
        k[b, outside] = (JUNK * sgn).to(BF)
        # and one key among 1537 random ones weighs too little to be missed: the first and the last visible key lean towards the
        # same query head (score about 0.75 * sum |q| * scale = 7), so both ends of [kv_beg, kv_end) carry weight at any length
        if not count:
            k[b, beg[b]] = k[b, end[b] - 1] = (0.75 * sgn).to(BF)
    vis =[visible("decode", 1, T_max, T_max, kv_beg=beg[b], kv_end=end[b]) for b in range(B)]
    return Case(f"decode-{name}-{_tag(BF, count)}", 5, "decode", BF, q, k, v, vis, TOL_DECODE, count, beg=beg, end=end, nsplit=nsplit)


N_CASES = len(PREFILL) + len(KVOFF_D) * len(KVOFF) + len(VARLEN) + len(DECODE)


@functools.lru_cache(maxsize=None)
def cases(count=False):
    """the cases of groups 2 .. 5 (their count variants are group 6), built once; N_CASES of them, decode last"""
    cs = [prefill_case(d, dt, count) for d, dt in PREFILL]
    cs += [kvoff_case(d, *c, count=count) for d in KVOFF_D for c in KVOFF]
    cs += [varlen_case(d, dt, count) for d, dt in VARLEN]
    cs += [decode_case(c[0], count) for c in DECODE]
    assert len(cs) == N_CASES
    return cs


# ---------------------------------------------------------------------------------------------- one-key perturbations
def perturbations(case):
    """The visibility rule moved by one key at each boundary it has: yields (label, batch row b, query rows (slice), vis of those
    rows). kv_beg +- 1, kv_off +- 1 (causal), kv_end +- 1 (decode), first / last key of each segment +- 1 (varlen). A move that
    another clause of the rule absorbs (kv_beg = 0 - 1, a key past the diagonal, ...) changes nothing and is not yielded."""
    out = []
    B, Lq = case.q.shape[:2]
    N = case.k.shape[1]
    p = case.par
    if case.kind in ("flash", "cache"):
        for b in range(B):
            moves = [("kv_beg", dict(kv_beg=p["beg"][b] + s)) for s in (-1, 1)]
            if p["causal"]:
                moves += [("kv_off", dict(kv_off=p["off"] + s)) for s in (-1, 1)]
            for what, kw in moves:
                args = dict(causal=p["causal"], kv_off=p["off"], kv_beg=p["beg"][b])
                args.update(kw)
                out.append((f"b{b} {what}={kw[what]}", b, slice(0, Lq), visible("flash", Lq, p["Lk"], N, **args)))
    elif case.kind == "decode":
        for b in range(B):
            for s in (-1, 1):
                out.append((f"b{b} kv_beg{s:+d}", b, slice(0, 1), visible("decode", 1, N, N, kv_beg=p["beg"][b] + s, kv_end=p["end"][b])))
                out.append((f"b{b} kv_end{s:+d}", b, slice(0, 1), visible("decode", 1, N, N, kv_beg=p["beg"][b], kv_end=p["end"][b] + s)))
    else:
        cu = p["cu"]
        j = torch.arange(N)[None]
        for a, e in zip(cu[:-1], cu[1:]):
            for what, lo, hi in (("start-1", a - 1, e), ("start+1", a + 1, e), ("end-1", a, e - 1), ("end+1", a, e + 1)):
                out.append((f"seg[{a},{e}) {what}", 0, slice(a, e), ((j >= lo) & (j < hi)).expand(e - a, N).clone()))
    return [(label, b, rows, vis) for label, b, rows, vis in out if not torch.equal(vis, case.vis[b][rows])]

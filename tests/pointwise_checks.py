"""fp64 restatements and DERIVED elementwise bounds for the pointwise, plumbing and small-conv entry points of csrc/unet_ops.hip
(ops.act, add, add_scaled, axpby, split_hilo, geglu, swiglu, concat_channels(_f32), mean_tokens, moe_combine, l2_normalize,
softmax_rows, pack_keep_bits, latent_to_nhwc(_f32), cfg_combine, lincomb, nhwc_to_nchw, conv_transpose1d, conv2d_small_cin(_f32in),
conv2d_small_cout(_f32in)) and the embedding gather of csrc/llm_decode.hip. Companion of gemm_checks.py / norm_checks.py, whose
U, ETA, rnd_err, acc_c, act64, LIP, conv_base, pre_gemm, finish and finish_glu it reuses.

The reference runs on exactly the values the kernel reads: 16-bit inputs after their rounding, fp32 inputs as they are, host scalars
(scale, alpha, beta, guidance, coefficients, leaky slope) after their conversion to fp32 (f32v). This module also holds the case
tables and the seeded inputs, so the CPU self-test (test_pointwise_checks_cpu.py, torch-fp32 emulations and mutants) and the GPU
tests (test_pointwise_ops_gpu.py, test_small_conv_gpu.py) check the same cases with the same bounds.

Notation: e = 2^-24 (one fp32 rounding, relative), u / eta = gemm_checks.U / ETA of the 16-bit format, r() = one correct rounding to
it. check() takes the bound t on the kernel's fp32 value; for a 16-bit output the tolerance is t + rnd_err(|ref| + t): one correct
rounding of a value within t of the reference (norm_checks.bound). Every element has to be inside; there is no outlier allowance.

Bit copies          concat_channels(_f32), embed, the permutation of latent_to_nhwc* (scale 1) and nhwc_to_nchw (mul 1, add 0):
                    torch.equal.
One fp32 operation  add, the scale product of latent_to_nhwc*, relu (fmaxf), leaky_relu (x > 0 ? x : x * slope), split_hilo: a
                    deterministic function of IEEE operations -> torch.equal against the same operation in torch fp32 on the CPU,
                    then .to(dtype). split_hilo: hi == r(x), lo == r(x - hi), and |hi + lo - x| <= max(u^2 |x|, eta) (what the
                    rounding of the remainder |x - hi| <= u |x| loses).
Two or three fp32 operations the compiler may contract into an fma
                    add_scaled (a + b) s; axpby alpha a + beta b; cfg_combine eu + g (ec - eu); lincomb sum c_j x_j; nhwc_to_nchw
                    x mul + add (clamping is 1-Lipschitz). Each operation rounds a value of at most sum |terms| once, contraction
                    only removes roundings:  t = 4 e sum |terms|.
Activations         t = delta_kind(x), the fp32 evaluation error of the device function in csrc/common.hpp (+ ACT_TOL[kind], the
                    one measured term, NOTEBOOK.md):
    silu_f          x * rcp(1 + __expf(-x)). __expf(y) = v_exp_f32(y * log2(e)): the constant and the product each round the
                    argument once (relative e), which the exponential turns into a relative 2 e |y|; v_exp_f32 itself is 1 ulp
                    = 2 e. s = 1 / (1 + E) inherits (1 - s) of E's relative error; the sum rounds once (e), rcp is 1 ulp (2 e),
                    the product rounds once (e):   delta = |silu(x)| e ((1 - s) (2 |x| + 2) + 4) + |x| 2^-126.
                    The last term: below fp32's smallest normal number 2^-126 the sigmoid flushes to zero (expf overflows to inf
                    beyond x = -88.7 and rcp(inf) = 0; rcp does not return subnormals).
    quick_gelu_f    the same with y = 1.702 x: the constant and one more product make it 4 roundings of the argument.
    gelu_erf_f      0.5 x (1 + erf_fast(x / sqrt 2)): Abramowitz-Stegun 7.1.26 with |erf error| <= 1.5e-7 (cited in common.hpp),
                    evaluated in fp32: rcp (2 e), four fmas on values below 1.5 (6 e), __expf(-z^2) whose relative (2 z^2 + 2) e
                    meets z^2 exp(-z^2) <= 0.37 (3 e), two products and the subtraction from 1 (3 e), the rounding of the argument
                    (|d erf / dz| |z| e <= 0.5 e): 16 e absolute with margin. Times |x| / 2, plus 4 e |gelu(x)| for (1 + erf), the
                    product and 0.5 x.
    tanhf           the library's bound of 2 ulp = 4 e |tanh x|.
    geglu / swiglu  gemm_checks.finish_glu with pre.t = 0 -- the product rule over r(gelu(g)) (geglu) / r(silu(a)) (swiglu) -- plus
                    gain * delta_kind(gate). The product of two 16-bit values is exact in fp32, so the output must ALSO be r(lin * h)
                    for a 16-bit h that is a correct rounding of a value within delta_kind of act(gate): glu_exact_ok() checks
                    that, and it is what tells a kernel that skips the intermediate rounding from one that does it.
Short reductions
    mean_tokens     sequential fp32 sum of T terms, every partial sum <= sum |x|: T e sum |x|; divided by T; the division rounds
                    once more:   t = (T + 1) e sum |x| / T.
    l2_normalize    S = sum x^2 in fp32: dS = acc_c(n) sqrt(sum x^4) + 4 e S (any order; the products and the all-positive
                    partial sums), sqrtf, 1 / max(., eps) and the product round once each:
                    t = |ref| (dS / (2 S) + 3 e)   (S = 0: the row is zero and stays zero).
    softmax_rows    the max is exact. z_i = s x_i - fl(s max): two products and a subtraction, or an fma: dz = e (|s x_i| + |m| +
                    |z_i|). E_i = __expf(z_i): relative eps_i = dz + (2 |z_i| + 2) e. The sum of n_valid positive terms:
                    acc_c(n_valid) relative, plus the p-weighted mean of the eps_j; 1 / sum and the product round once each:
                    t = p_i (eps_i + sum_j p_j eps_j + acc_c(n_valid) + 2 e) + 2^-126   (the flush of E_i below 2^-126; sum >= 1).
    moe_combine     r_e = 1 / (1 + __expf(-l_e)): eps_e = (1 - r_e) (2 |l_e| + 2) e + 2 e. S = sum r_e: E sequential adds.
                    w_e = r_e / S: rho_e = eps_e + sum_j w_j eps_j + (E + 1) e. h_e = r(w_e): t_w = w_e rho_e + rnd_err(w_e + ..).
                    x_e h_e is exact in fp32 and rounded to the 16-bit format: |x_e| t_w + rnd_err(|x_e| (w_e + t_w)). The fp32
                    sum of E such terms: E e sum |x_e w_e|. The last rounding is check()'s.
Small convolutions  gemm_checks.conv_base -> pre_gemm -> finish: K = ks^2 Cin products accumulated in fp32 (conv2d_small_cin: in
                    (ky, kx, c) order behind the bias; conv2d_small_cout: 64 per-lane partial sums, then wave_sum, then the bias --
                    acc_c(K) holds for any order). fp32 outputs are held to tol32, 16-bit outputs to the rounding of such a value,
                    and where both exist the 16-bit output has to be r(fp32 output) exactly.
conv_transpose1d    cols = fp32-output GEMM over K = Cin (tol32 of gemm_checks per entry), summed over the <= ceil(k / stride)
                    taps that land on an output position, plus the bias: the taps' bounds add, and the (taps + 1) fp32 additions
                    round partial sums of at most sum |terms|.
"""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

import gemm_checks as gc
from gemm_checks import ETA, U, Pre, acc_c, act64, conv_base, finish, finish_glu, pre_gemm, rnd_err

E32 = 2.0 ** -24
TINY32 = 2.0 ** -126                  # fp32's smallest normal number
AS_ERF_ERR = 1.5e-7                   # Abramowitz-Stegun 7.1.26, as cited at erf_fast in csrc/common.hpp
V = 8                                 # elements per 16-byte vector
SWEEP = 2048 * 256                    # threads of one grid sweep: grid_for() caps a launch at 2048 blocks of 256
FILL = 768.0                          # sentinel of guard elements and of outputs an emulation leaves unwritten (exact in bf16 and f16)
DTYPES = (torch.bfloat16, torch.float16)
# the device activations' own error beyond delta_kind, per kind: 4 x the largest measured excess (NOTEBOOK.md, "Pointwise, plumbing
# and small-conv kernels"). No kind exceeded its derived bound, so every entry is 4 x 0.
ACT_TOL = {"silu": 0.0, "gelu": 0.0, "quick_gelu": 0.0, "tanh": 0.0}
LOG = []                              # one record per check(): the figures, appended before the assertion


def name(dt):
    return str(dt).replace("torch.", "")


def f32v(v) -> float:
    """a host scalar as the kernel reads it: converted to fp32"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def specials(dt):
    v = [0.0, -0.0, 1.0, -1.0, 10.0, -10.0, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0]
    if dt == torch.float16:
        v += [2.0 ** -14, -(2.0 ** -14), 2.0 ** -20, -3 * 2.0 ** -24]      # smallest normal, subnormals
    return torch.tensor(v)


def with_specials(x, dt):
    sp = specials(dt)
    k = min(x.numel(), sp.numel())
    x.view(-1)[:k] = sp[:k]
    return x


# ------------------------------------------------------------------------------------------------------------------- checks
def check(what, got, ref, t, dt, fp32_out=False, act=None, gain=1.0):
    """every element of `got` within the bound (module docstring); figures to LOG and stdout before the assertion"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    assert bool(torch.isfinite(ref).all()), f"{what}: non-finite reference (a mistake of the test's inputs)"
    t = torch.as_tensor(t, dtype=torch.float64).expand(ref.shape)
    derived = t if fp32_out else t + rnd_err(ref.abs() + t, dt)
    tol = derived + (gain * ACT_TOL[act] if act is not None else 0.0)
    err = (got - ref).abs()
    ratio = float((err / derived.clamp_min(1e-300)).max()) if err.numel() else 0.0
    rec = {"what": what, "kernel": what.split(" ")[0], "dtype": name(dt), "out": "f32" if fp32_out else "16", "ratio": ratio, "act": act}
    if act is not None:
        exc = (err - derived) / torch.as_tensor(gain, dtype=torch.float64).expand(ref.shape).clamp_min(1e-300)
        rec["act_excess"] = float(exc.max())
    LOG.append(rec)
    print(f"[pointwise_checks] {what} {rec['dtype']} out={rec['out']}: max err / tol = {ratio:.3f}")
    bad = ~(err <= tol)
    n_bad = int(bad.sum())
    assert n_bad == 0, (f"{what}: {n_bad} / {bad.numel()} elements outside the derived bound, worst err / tol = {ratio:.3f} "
                        f"(max err {float(err.max()):.4g}, first at {int(bad.reshape(-1).nonzero()[0])})")


def check_equal(what, got, want, dt=None):
    got = got.detach().cpu().reshape(want.shape)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype}, expected {want.dtype}"
    if got.dtype.is_floating_point:
        assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    same = torch.equal(got, want)
    LOG.append({"what": what, "kernel": what.split(" ")[0], "dtype": name(dt if dt is not None else want.dtype), "out": "exact",
                "ratio": 0.0 if same else float("inf"), "act": None})
    if not same:
        bad = (got != want).reshape(-1)
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} elements differ from the exact result, first at {int(bad.nonzero()[0])}")


def guarded(shape, dtype, device="cpu"):
    """(buffer, contiguous view of `shape` in its middle): 64 FILL elements on each side of the view"""
    n = math.prod(shape)
    buf = torch.full((n + 128,), FILL, dtype=dtype, device=device)
    return buf, buf[64:64 + n].view(shape)


def assert_guards(what, buf):
    b = buf.detach().cpu().float()
    assert bool((b[:64] == FILL).all()), f"{what}: wrote in front of the output"
    assert bool((b[-64:] == FILL).all()), f"{what}: wrote behind the output"


def into(what, shape, dtype, dev, call):
    """run call(out=view into a guarded buffer); the guards must be untouched; -> the result on the CPU"""
    buf, view = guarded(tuple(shape), dtype, dev)
    call(view)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    assert_guards(what, buf)
    return view.cpu()


def untouched(buf):
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return bool((buf.cpu().float() == FILL).all())


def act_delta(kind, x, ref):
    """fp32 evaluation error of the device activation at x (fp64), ref = act64(kind, x): module docstring"""
    if kind in ("silu", "quick_gelu"):
        k, nz = (1.0, 2.0) if kind == "silu" else (f32v(1.702), 4.0)
        y = k * x
        s = torch.sigmoid(y)
        return ref.abs() * E32 * ((1 - s) * (nz * y.abs() + 2) + 4) + x.abs() * TINY32
    if kind == "gelu":
        return x.abs() / 2 * (AS_ERF_ERR + 16 * E32) + 4 * E32 * ref.abs()
    if kind == "tanh":
        return 4 * E32 * ref.abs()
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------------------------- vector elementwise
VEC_OPS = [("act", "silu", 0.0), ("act", "gelu", 0.0), ("act", "quick_gelu", 0.0), ("act", "tanh", 0.0), ("act", "relu", 0.0),
           ("act", "leaky_relu", 0.1), ("act", "leaky_relu", 0.01), ("add",), ("add_scaled", 1 / 3), ("add_scaled", 0.5),
           ("axpby", 0.1, 0.9), ("axpby", -1.5, 2.0), ("split_hilo",)]
VEC_N = [V, 257 * V, (SWEEP + 3) * V]          # one thread; one live thread in block 2; three vectors in the second grid sweep


def op_id(op):
    return "-".join(str(round(p, 3)) if isinstance(p, float) else str(p) for p in op)


@functools.lru_cache(maxsize=None)
def vec_inputs(n, dt):
    g = gen("vec", n)
    a32 = with_specials(torch.randn(n, generator=g) * 2, dt)
    b32 = torch.randn(n, generator=g) * 2
    return {"a": a32.to(dt), "b": b32.to(dt), "x32": a32}


def vec_verify(op, n, dt, inp, out):
    what = f"{op_id(op)} n={n}"
    a, b = inp["a"], inp["b"]
    a64, b64 = a.double(), b.double()
    if op[0] == "act":
        kind, param = op[1], op[2]
        if kind == "relu":
            return check_equal(what, out, a.float().clamp_min(0).to(dt), dt)
        if kind == "leaky_relu":
            af = a.float()
            return check_equal(what, out, torch.where(af > 0, af, af * torch.tensor(param, dtype=torch.float32)).to(dt), dt)
        ref = act64(kind, a64)
        return check(what, out, ref, act_delta(kind, a64, ref), dt, act=kind)
    if op[0] == "add":
        return check_equal(what, out, (a.float() + b.float()).to(dt), dt)
    if op[0] == "add_scaled":
        s = f32v(op[1])
        return check(what, out, (a64 + b64) * s, 4 * E32 * (a64.abs() + b64.abs()) * abs(s), dt)
    if op[0] == "axpby":
        al, be = f32v(op[1]), f32v(op[2])
        return check(what, out, al * a64 + be * b64, 4 * E32 * ((al * a64).abs() + (be * b64).abs()), dt)
    if op[0] == "split_hilo":
        x, (hi, lo) = inp["x32"], out
        want_hi = x.to(dt)
        check_equal(what + " hi", hi, want_hi, dt)
        check_equal(what + " lo", lo, (x - want_hi.float()).to(dt), dt)
        x64 = x.double()
        s = hi.detach().cpu().double() + lo.detach().cpu().double()
        bad = ~((s - x64).abs() <= (U[dt] ** 2 * x64.abs()).clamp_min(ETA[dt]))
        assert not bool(bad.any()), f"{what}: hi + lo is further than max(u^2 |x|, eta) from x at {int(bad.sum())} elements"
        return None
    raise ValueError(op)


# ------------------------------------------------------------------------------------------------------------------- geglu / swiglu
GLU_CASES = [(1, 8), (3, 24), (5, 1048), (2049, 2048)]        # the last: 524,544 vectors, second grid sweep


@functools.lru_cache(maxsize=None)
def glu_inputs(M, inner, dt):
    return with_specials(torch.randn(M, 2 * inner, generator=gen("glu", M, inner)) * 2, dt).to(dt)


def glu_exact_ok(lin, fx, delta, got, dt):
    """got == r(lin * h) for some 16-bit h that is a correct rounding of a value within delta of fx"""
    # where 2 delta is below the spacing of the format at fx (> rnd_err(fx)) the interval holds at most one 16-bit number, so the
    # three roundings below are all the h there can be; elsewhere (gelu far below zero: |fx| << delta) the element is left to check()
    ok = ~(2 * delta < rnd_err(fx, dt))
    for h in ((fx - delta).to(dt), fx.to(dt), (fx + delta).to(dt)):
        ok |= (lin * h.double()).to(dt) == got
    return ok


def glu_verify(kind, M, inner, dt, x, out):
    what = f"{kind} M={M} inner={inner}"
    x64 = x.double()
    R = finish_glu(Pre(x64, torch.zeros_like(x64), 1), dt, kind)
    act = gc.GLU_KIND[kind]
    a, b = x64[:, :inner], x64[:, inner:]
    lin, gate = (a, b) if kind == "geglu" else (b, a)
    fx = act64(act, gate)
    delta = act_delta(act, gate, fx)
    check(what, out, R.ref, R.tol32 + R.gain * delta, dt, act=act, gain=R.gain)
    got = out.detach().cpu().reshape(M, inner)
    ok = glu_exact_ok(lin, fx, delta + ACT_TOL[act], got, dt)
    assert bool(ok.all()), (f"{what}: {int((~ok).sum())} outputs are not r(lin * h) for any 16-bit rounding h of the activation "
                            "(the intermediate rounding is missing or misplaced)")


# ------------------------------------------------------------------------------------------------------------------- concat, embed
CONCAT_CASES = [(1, 8, 8), (7, 8, 24), (7, 24, 8), (3, 320, 640), (4100, 640, 384)]     # the last: 524,800 vectors
CONCAT32_CASES = [(5, 4, 12), (3, 320, 320)]


@functools.lru_cache(maxsize=None)
def concat_inputs(rows, C1, C2, dt):
    g = gen("concat", rows, C1, C2)
    return torch.randn(rows, C1, generator=g).to(dt), (torch.randn(rows, C2, generator=g) + 4).to(dt)


def concat_verify(case, dt, inp, out):
    check_equal(f"concat_channels{'_f32' if dt == torch.float32 else ''} {case}", out, torch.cat(inp, dim=-1), dt)


EMBED_CASES = [(1, 8, 1), (5, 2048, 11), (3, 2056, 7)]          # (rows, H, V); 2056 = 257 vectors per row


@functools.lru_cache(maxsize=None)
def embed_inputs(rows, H, Vn, dt):
    table = torch.randn(Vn, H, generator=gen("embed", rows, H, Vn)).to(dt)
    ids = torch.tensor([-1, 2 ** 31 - 1, Vn, Vn + 5, 0, Vn - 1, Vn // 2], dtype=torch.int32)      # clamped to rows 0 and V - 1
    ids = ids.repeat(rows // ids.numel() + 1)[:rows]
    return table, ids.contiguous()


def embed_verify(case, dt, inp, out):
    table, ids = inp
    check_equal(f"embed {case}", out, table[ids.long().clamp(0, table.shape[0] - 1)], dt)


# ------------------------------------------------------------------------------------------------------------------- short reductions
MEAN_CASES = [(1, 1, 1), (2, 7, 3), (3, 77, 1280), (2, 2, 262147)]       # the last: B C = SWEEP + 6


@functools.lru_cache(maxsize=None)
def mean_inputs(B, T, Cn, dt):
    g = gen("mean", B, T, Cn)
    return (torch.randn(B, T, Cn, generator=g) + torch.arange(B).view(B, 1, 1) * 3.0).to(dt)      # batches differ by their mean


def mean_verify(case, dt, x, out):
    x64, T = x.double(), x.shape[1]
    check(f"mean_tokens {case}", out, x64.mean(1), (T + 1) * E32 * x64.abs().sum(1) / T, dt)


# (E, B, per-batch shape): ld = E + 3, the unused columns hold +30
MOE_CASES = [(E, B, (5, 13)) for E in (1, 2, 8) for B in (1, 3)] + [(2, 3, (174763,))]      # the last: B per_batch = SWEEP + 1


@functools.lru_cache(maxsize=None)
def moe_inputs(E, B, shape, dt):
    g = gen("moe", E, B, shape)
    xs = tuple((torch.randn(B, *shape, generator=g) * (1 + e)).to(dt) for e in range(E))
    logits = torch.full((B, E + 3), 30.0)
    logits[:, :E] = torch.rand(B, E, generator=g) * 12 - 6
    return xs, logits.to(dt)


def moe_verify(case, dt, inp, out):
    xs, logits = inp
    E, B = len(xs), logits.shape[0]
    l = logits.double()[:, :E]
    r = torch.sigmoid(l)
    eps = (1 - r) * (2 * l.abs() + 2) * E32 + 2 * E32
    w = r / r.sum(1, keepdim=True)
    rho = eps + (w * eps).sum(1, keepdim=True) + (E + 1) * E32
    t_w = w * rho + rnd_err(w + w * rho, dt)
    ref, t, mag = 0.0, 0.0, 0.0
    for e in range(E):
        x = xs[e].double().reshape(B, -1).abs()
        we, te = w[:, e:e + 1], t_w[:, e:e + 1]
        ref = ref + xs[e].double().reshape(B, -1) * we
        t = t + x * te + rnd_err(x * (we + te), dt)
        mag = mag + x * we
    check(f"moe_combine {case}", out, ref, t + E * E32 * mag, dt)


L2_CASES = [(1, 1), (2, 7), (3, 256), (3, 257), (2, 8192)]
L2_EPS = 1e-12


@functools.lru_cache(maxsize=None)
def l2_inputs(rows, n, dt):
    """the table's rows, then a zero row and (bf16 only: it would flush to zero in f16) a row of 2^-60 for the eps clamp"""
    x = torch.randn(rows, n, generator=gen("l2", rows, n)) * 2
    extra = [torch.zeros(1, n)] + ([torch.full((1, n), 2.0 ** -60)] if dt == torch.bfloat16 else [])
    return torch.cat([x] + extra).to(dt)


def l2_verify(case, dt, x, out):
    x64, n = x.double(), x.shape[1]
    S = (x64 * x64).sum(1, keepdim=True)
    ref = x64 / S.sqrt().clamp_min(f32v(L2_EPS))
    dS = acc_c(n) * (x64 ** 4).sum(1, keepdim=True).sqrt() + 4 * E32 * S
    check(f"l2_normalize {case}", out, ref, ref.abs() * (dS / (2 * S).clamp_min(1e-300) + 3 * E32), dt)
    zero = (x64 == 0).all(1)
    assert bool((out.detach().cpu().float()[zero] == 0).all()), f"l2_normalize {case}: a zero row does not stay zero"


SOFTMAX_CASES = [(1, 1, 1), (2, 8, 5), (3, 256, 256), (3, 264, 257), (37, 1000, 1000), (2, 4096, 4090)]      # (rows, n, n_valid)
SOFTMAX_SCALES = [0.3, 512 ** -0.5]
PAD32 = 3e38


@functools.lru_cache(maxsize=None)
def softmax_inputs(rows, n, nv):
    """fp32 [rows, n]: rows of three kinds (randn * 5; all equal; a spike of 1e4 among zeros), the padding columns hold 3e38"""
    g = gen("softmax", rows, n, nv)
    x = torch.full((rows, n), PAD32)
    for r in range(rows):
        kind = (r + n) % 3
        if kind == 0:
            x[r, :nv] = torch.randn(nv, generator=g) * 5
        elif kind == 1:
            x[r, :nv] = 2.5
        else:
            x[r, :nv] = 0.0
            x[r, (7 * r) % nv] = 1e4
    return x


def softmax_verify(case, scale, dt, x, out):
    rows, n, nv = case
    what = f"softmax_rows {case} scale={scale:.3g}"
    got = out.detach().cpu()
    assert bool((got[:, nv:].float() == 0).all()) and bool(torch.isfinite(got.float()).all()), f"{what}: padding columns are not exactly zero"
    s = f32v(scale)
    sx = s * x[:, :nv].double()
    m = sx.max(1, keepdim=True).values
    z = sx - m
    p = torch.softmax(z, dim=1)
    eps = E32 * (sx.abs() + m.abs() + z.abs()) + (2 * z.abs() + 2) * E32
    t = p * (eps + (p * eps).sum(1, keepdim=True) + acc_c(nv) + 2 * E32) + TINY32
    check(what, got[:, :nv], p, t, dt)


# ------------------------------------------------------------------------------------------------------------------- pack_keep_bits
PACK_N = [1, 63, 64, 65, 256, 257, 1000]
PACK_THR = 0.5


def pack_cases():
    return [(n, nv) for n in PACK_N for nv in sorted({0, 1, n - 1, n, n + 7})]


@functools.lru_cache(maxsize=None)
def pack_inputs(n):
    u = torch.rand(n, generator=gen("pack", n))
    u[::5] = PACK_THR                       # exactly at the threshold: the comparison is strict, these are not kept
    return u


def pack_verify(case, u, words):
    n, nv = case
    got = [int(w) & (2 ** 64 - 1) for w in words.detach().cpu().tolist()]
    want = [0] * ((n + 63) // 64)
    for j in range(min(n, nv)):
        if float(u[j]) < PACK_THR:
            want[j // 64] |= 1 << (j % 64)
    LOG.append({"what": f"pack_keep_bits {case}", "kernel": "pack_keep_bits", "dtype": "-", "out": "exact",
                "ratio": 0.0 if got == want else float("inf"), "act": None})
    assert got == want, f"pack_keep_bits {case}: words differ: got {[hex(w) for w in got]}, want {[hex(w) for w in want]}"


# ------------------------------------------------------------------------------------------------------------------- latent plumbing
MAPS = [(1, 3, 1, 1), (2, 4, 3, 5), (1, 16, 7, 2), (1, 4, 363, 363)]         # (B, C, H, W), non-square; the last: 527,076 elements
REPS = [1, 2, 3]
LATENT_SCALES = [1.0, 0.7071]
GUIDANCE = 7.5
LINCOMB_COEFS = [(1.5,), (-0.75, 2.0), (0.3, -1.1, 0.0, 2.5, -0.01, 1.0)]
NCHW_AFFINES = [(1.0, 0.0, False), (0.5, 0.5, False), (0.5, 0.5, True)]


@functools.lru_cache(maxsize=None)
def map_input(tag, *shape):
    return torch.randn(*shape, generator=gen("map", tag, shape))


def latent_verify(case, reps, scale, dt, lat, out):
    """dt = torch.float32: latent_to_nhwc_f32"""
    B, Cn, H, W = case
    v = (lat * torch.tensor(scale, dtype=torch.float32)).permute(0, 2, 3, 1).contiguous().to(dt)
    check_equal(f"latent_to_nhwc{'_f32' if dt == torch.float32 else ''} {case} reps={reps} scale={scale}", out,
                v.unsqueeze(0).expand(reps, B, H, W, Cn).reshape(reps * B, H, W, Cn), dt)


def cfg_verify(case, e2, out):
    B = e2.shape[0] // 2
    eu, ec, g = e2[:B].double(), e2[B:].double(), f32v(GUIDANCE)
    check(f"cfg_combine {case}", out, (eu + g * (ec - eu)).permute(0, 3, 1, 2), (4 * E32 * (eu.abs() + g * (ec.abs() + eu.abs()))).permute(0, 3, 1, 2),
          torch.float32, fp32_out=True)


def lincomb_verify(case, coefs, xs, out):
    terms = [f32v(c) * x.double() for c, x in zip(coefs, xs)]
    check(f"lincomb {case} n={len(coefs)}", out, sum(terms), 4 * E32 * sum(t.abs() for t in terms), torch.float32, fp32_out=True)


def nchw_input(case):
    """fp32 NHWC; the first values are chosen so that x * 0.5 + 0.5 lands exactly on 0 and 1 and beyond both"""
    B, Cn, H, W = case
    x = map_input("nchw", B, H, W, Cn).clone()
    sp = torch.tensor([-1.0, 1.0, -3.0, 3.0])
    x.view(-1)[:min(x.numel(), 4)] = sp[:min(x.numel(), 4)]
    return x


def nchw_verify(case, aff, x, out):
    mul, add, clamp = aff
    what = f"nhwc_to_nchw {case} {aff}"
    if mul == 1.0 and add == 0.0 and not clamp:
        return check_equal(what, out, x.permute(0, 3, 1, 2).contiguous())
    m, a = f32v(mul), f32v(add)
    ref = x.double() * m + a
    t = 4 * E32 * ((x.double() * m).abs() + abs(a))
    if clamp:
        ref = ref.clamp(0, 1)
        got = out.detach().cpu()
        assert bool(((got >= 0) & (got <= 1)).all()), f"{what}: values outside [0, 1]"
    check(what, out, ref.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2), torch.float32, fp32_out=True)


# ------------------------------------------------------------------------------------------------------------------- conv_transpose1d
CT1D_CASES = [(5, 8, 4, 7, 2, 3), (6, 8, 8, 3, 2, 0), (4, 8, 4, 2, 3, 0), (9, 16, 8, 3, 1, 1), (1, 8, 4, 4, 2, 1),
              (4, 8, 4, 5, 3, 1)]     # (L, Cin, Cout, k, stride, pad); the last: 2 pad is no multiple of the stride
CT1D_B = 2


@functools.lru_cache(maxsize=None)
def ct1d_inputs(case, dt):
    L, Cin, Cout, k, stride, pad = case
    g = gen("ct1d", case)
    x = torch.randn(CT1D_B, L, Cin, generator=g).to(dt)
    w = (torch.randn(Cin, Cout, k, generator=g) * Cin ** -0.5).to(dt)             # nn.ConvTranspose1d layout
    bias = (torch.randn(Cout, generator=g) + 2).to(dt)
    return x, w, bias, w.permute(2, 1, 0).reshape(k * Cout, Cin).contiguous()    # row j * Cout + o = w[:, o, j]


def ct1d_verify(case, dt, inp, use_bias, out):
    L, Cin, Cout, k, stride, pad = case
    x, w, bias, _ = inp
    x64, w64 = x.double(), w.double()
    ref = F.conv_transpose1d(x64.transpose(1, 2), w64, bias.double() if use_bias else None, stride=stride, padding=pad).transpose(1, 2)
    # per-entry tol32 of the cols GEMM, and |cols|, pushed through the same overlap-add
    cols = torch.einsum("bic,coj->bijo", x64, w64)
    tq = acc_c(Cin) * torch.einsum("bic,coj->bijo", x64 * x64, w64 * w64).sqrt()
    L_out = ref.shape[1]
    t, mag = torch.zeros_like(ref), torch.zeros_like(ref)
    for i in range(L):
        for j in range(k):
            p = i * stride - pad + j
            if 0 <= p < L_out:
                t[:, p] += tq[:, i, j]
                mag[:, p] += cols[:, i, j].abs()
    if use_bias:
        mag = mag + bias.double().abs()
    ntap = -(-k // stride)
    check(f"conv_transpose1d {case} bias={use_bias}", out, ref, t + (ntap + 1) * E32 * mag, dt)


# ------------------------------------------------------------------------------------------------------------------- small convs
CONV_MAPS_CIN = [(1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 3, 7)]          # (B, H, W)


def cin_cases():
    """(B, H, W, Cin, Cout, ks, bias)"""
    c = [(B, H, W, Cin, Cout, ks, bias) for Cin in (1, 3, 4, 8) for ks in (1, 3) for Cout in (8, 24) for (B, H, W) in CONV_MAPS_CIN
         for bias in (True, False)]
    c.append((2, 64, 64, 4, 136, 3, True))          # 139,264 threads: past the 512-block cap
    c.append((2, 3, 5, 8, 232, 3, True))            # stages 66,816 B of weights: just over 64 KiB of LDS
    return c


CIN_LDS_CASE = (2, 3, 5, 8, 232, 3, True)
CONV_MAPS_COUT = [(1, 1, 1), (1, 3, 3), (2, 5, 3)]


def cout_cases():
    """(B, H, W, Cin, Cout, ks, bias); lane chunks ks^2 Cin / 8 = 1, 63, 64, 72 against the 64 lanes"""
    c = []
    for i, Cout in enumerate((1, 2, 3, 4, 5, 8)):
        for j, (Cin, ks) in enumerate(((8, 1), (56, 3), (512, 1), (64, 3))):
            for k, (B, H, W) in enumerate(CONV_MAPS_COUT):
                c.append((B, H, W, Cin, Cout, ks, (i + j + k) % 2 == 0))
    c.append((1, 91, 91, 8, 3, 3, True))            # 8281 pixels: past the 2048 x 4 cap
    c.append((1, 3, 3, 456, 8, 3, True))            # stages 65,664 B of weights
    return c


COUT_LDS_CASE = (1, 3, 3, 456, 8, 3, True)


@functools.lru_cache(maxsize=None)
def conv_inputs(case, dt):
    """(x fp32 NHWC, w, bias): x is what the _f32in forms read; the 16-bit forms read x.to(dt). The images of a batch differ
    strongly (the second is 8 times larger and of the other sign), so a tap that bleeds across an image border shows."""
    B, H, W, Cin, Cout, ks, _ = case
    g = gen("conv", case)
    x = torch.randn(B, H, W, Cin, generator=g) * torch.tensor([1.0, -8.0])[:B].view(B, 1, 1, 1)
    w = (torch.randn(Cout, ks, ks, Cin, generator=g) * (ks * ks * Cin) ** -0.5).to(dt)
    bias = (torch.randn(Cout, generator=g) + torch.arange(Cout) % 3).to(dt)       # neighbouring channels differ
    return x, w, bias


@functools.lru_cache(maxsize=None)
def conv_ref(case, dt, f32in):
    x, w, bias = conv_inputs(case, dt)
    ks = case[5]
    xin = x if f32in else x.to(dt)
    base, (B, Ho, Wo) = conv_base(xin, w, 1, (ks // 2, ks // 2))
    R = finish(pre_gemm(base, bias if case[6] else None), dt)
    shape = (B, Ho, Wo, w.shape[0])
    return R.ref.reshape(shape), R.tol32.reshape(shape)


def conv_verify(what, case, dt, f32in, y16=None, y32=None):
    ref, t = conv_ref(case, dt, f32in)
    what = f"{what} {case}"
    if y32 is not None:
        check(what, y32, ref, t, dt, fp32_out=True)
    if y16 is not None:
        check(what, y16, ref, t, dt)
    if y16 is not None and y32 is not None:
        check_equal(what + " 16 == r(f32)", y16, y32.detach().cpu().to(dt), dt)


def summary():
    """largest err / bound per (kernel, dtype, out) of everything checked so far"""
    best = {}
    for r in LOG:
        k = (r["kernel"], r["dtype"], r["out"])
        best[k] = max(best.get(k, 0.0), r["ratio"])
    exc = {}
    for r in LOG:
        if r.get("act") is not None and "act_excess" in r:
            k = (r["act"], r["dtype"])
            exc[k] = max(exc.get(k, -float("inf")), r["act_excess"])
    return best, exc

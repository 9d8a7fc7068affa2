"""fp64 restatements of the bf16 decode projections of csrc/llm_decode.hip (gemv, gemv_swiglu, gemv_fm, gemv_swiglu_fm, the lm_head
arg-max entry points, rmsnorm) with DERIVED elementwise bounds, a mirror of their dispatch (route) and the case table of
tests/test_gemv_routes_gpu.py. Built on tests/gemm_checks.py: the product, the accumulation term c = acc_c(K) = 8 sqrt(K) 2^-24 with
q = sqrt(x^2 @ (W^2)^T), the epilogue chains (finish, finish_glu) and check() are imported, not copied.

Operands are drawn as there: randn, pre-rounded to bf16, weights scaled by K^-0.5 (the random-walk bound needs zero-mean operands).
Every element has to be inside its bound; there is no outlier allowance and no fitted term.

  plain / + bias / + bias + res   finish(Pre(p + bias, c sqrt(q2 + bias^2), K), bf16, res=res): the epilogue rounds to bf16 before the
                                  bf16 residual is added (gemv_kernel, skinny_gemm_kernel, skinny_fm_kernel: the same three lines)
  gate/up                         finish_glu(pre, bf16, "swiglu"): bf16(bf16(silu(bf16 g)) * bf16(u))
  fused RMSNorm (norm_w)          the kernel stages bf16(bf16(x rs) w) (norm_vec, wq_common.hpp); the reference is fp64 throughout,
                                  xn = x rsqrt(mean x^2 + eps) w. Two independent roundings per element, each <= u |xn_k|: variance
                                  <= 2 (u xn_k)^2 / 3, six standard deviations = 6 u sqrt(2/3) sqrt(xn^2 @ (W^2)^T); the fp32 sum of
                                  squares and rsqrtf add (c/2 + 2^-22) |ref|; the accumulation adds c q
  folded RMSNorm (norm_eps)       the product against bf16(W norm_w) (ops.repack_fm16) times rs: c q rs + (c/2 + 2^-22) |ref|
  rmsnorm                         y = bf16(bf16(h rs) w): (2u + u^2) |ref| + (c(H)/2 + 2^-22) |ref|; with res, h = bf16(x + res)
  lm_head                         logits: the plain bound; the id: the lowest-index arg-max of the kernel's own logits AND the fp64
                                  arg-max, on cases with a planted winner per sequence whose margin is asserted on the reference
"""
import math
from collections import namedtuple
from functools import lru_cache

import torch

from gemm_checks import LOG, U, Pre, Ref, acc_c, bound, check, finish, finish_glu, matmul64, rnd_err  # noqa: F401  (re-exported)

BF = torch.bfloat16
E_RS = 2.0 ** -22                 # rsqrtf (1 ulp) with the division and the add in front of it
SIX_SIGMA_2R = 6.0 * U[BF] * math.sqrt(2.0 / 3.0)
EPS = 1e-6
XLDS_MAX = 64 * 1024              # gemv_dispatch: xlds_max (SPIDER_GEMV_XLDS_MAX unset)
R2_BYTES = 48 << 20               # gemv_dispatch: rows per wave = 2 from this many weight bytes on


# ================================================================================================ operands
def draw(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


@lru_cache(maxsize=8)
def weights(N, K, seed=1):
    """W [N, K] (K^-0.5), bias [N], norm_w [K] = 1 + 0.1 randn; shared by the tests of one shape and left unchanged"""
    return draw(seed, N, K, scale=K ** -0.5), draw(seed + 1, N), (1 + 0.1 * draw(seed + 2, K).float()).to(BF)


@lru_cache(maxsize=8)
def acts(K, N, scale=1.0, seed=11):
    """x [16, K] * scale and res [16, N]: a case of B rows takes the first B"""
    return draw(seed, 16, K, scale=scale), draw(seed + 1, 16, N)


# ================================================================================================ references
def rs64(x, eps):
    x = x.double()
    return ((x * x).mean(-1, keepdim=True) + eps).rsqrt()


def pre_plain(x, W, bias=None) -> Pre:
    b = matmul64(x, W)
    p, q2 = b.p, b.q2
    if bias is not None:
        p, q2 = p + bias.double(), q2 + bias.double() ** 2
    return Pre(p, acc_c(b.K) * q2.sqrt(), b.K)


def pre_norm(x, W, norm_w, eps) -> Pre:
    """row-major fused RMSNorm: the staged activations carry two bf16 roundings (module docstring)"""
    xn = x.double() * rs64(x, eps) * norm_w.double()
    b = matmul64(xn, W)
    q = b.q2.sqrt()
    c = acc_c(b.K)
    return Pre(b.p, SIX_SIGMA_2R * q + (c / 2 + E_RS) * b.p.abs() + c * q, b.K)


def fold_weight(W, norm_w):
    """bf16(W * norm_w) exactly as ops.repack_fm16 forms it"""
    return (W.float() * norm_w.float()[None, :]).to(W.dtype)


def pre_fold(x, W, norm_w, eps, bias=None) -> Pre:
    """fragment-major folded RMSNorm: (x @ bf16(W norm_w)^T) rs, bias added to the scaled value"""
    b = matmul64(x, fold_weight(W, norm_w))
    rs = rs64(x, eps)
    c = acc_c(b.K)
    core = b.p * rs
    q2 = b.q2 * rs * rs
    p = core
    if bias is not None:
        p, q2 = core + bias.double(), q2 + bias.double() ** 2
    return Pre(p, c * q2.sqrt() + (c / 2 + E_RS) * core.abs(), b.K)


def ref_gemv(x, W, bias=None, res=None, norm_w=None, eps=EPS, fold=False) -> Ref:
    if norm_w is None:
        pre = pre_plain(x, W, bias)
    elif fold:
        pre = pre_fold(x, W, norm_w, eps, bias)
    else:
        assert bias is None
        pre = pre_norm(x, W, norm_w, eps)
    return finish(pre, BF, res=res)


def ref_swiglu(x, Wgu, norm_w=None, eps=EPS, fold=False) -> Ref:
    if norm_w is None:
        pre = pre_plain(x, Wgu)
    elif fold:
        pre = pre_fold(x, Wgu, norm_w, eps)
    else:
        pre = pre_norm(x, Wgu, norm_w, eps)
    return finish_glu(pre, BF, "swiglu")


def add_bf16(x, res):
    """bf16(x + res) as `residual + hidden_states` forms it: the fp32 sum of two bf16 numbers, rounded once"""
    return (x.float() + res.float()).to(BF)


def ref_rmsnorm(h, w, eps) -> Ref:
    """h: the bf16 tensor the norm sees (add_bf16 of x and res where a residual is given)"""
    H = h.shape[-1]
    ref = h.double() * rs64(h, eps) * w.double()
    u = U[BF]
    return Ref(ref, (u + u * u + acc_c(H) / 2 + E_RS) * ref.abs())      # bound() adds the last rounding's u |ref|


# ================================================================================================ lm_head: planted winners
def lm_rows_per_block(V):
    nparts = min(max((V + 63) // 64, 1), 2048)          # spider_lm_head_nparts
    return nparts, (V + nparts - 1) // nparts           # lmhead_partial_kernel: rows_per_block


def winner_rows(V, B, fm=False):
    """distinct rows, one per sequence, the edges first: row 0, row V - 1, the last row of a block, the first row of the last partly
    filled block, an odd row of a block (row-major: of an odd rows_per_block where V gives one); then seeded rows"""
    if fm:
        per, nblk = 16, (V + 15) // 16
    else:
        nparts, per = lm_rows_per_block(V)
        nblk = (V + per - 1) // per
    odd = max(min(3, nblk - 2), 0) * per + min((per // 2) | 1, per - 1)       # an odd offset inside an inner block
    first = [0, V - 1, per - 1, (nblk - 1) * per, odd]
    g = torch.Generator().manual_seed(V + B)
    rows = []
    for r in first + torch.randperm(V, generator=g)[:2 * B + 8].tolist():
        if 0 <= r < V and r not in rows:
            rows.append(r)
    return rows[:B]


def plant(W, x_eff, d, rows, gain):
    """W[rows[b]] += alpha d_b / |d_b| with alpha = gain |d_b| / (x_eff_b . d_b): the logit of sequence b's winner rises by `gain`
    (x_eff: what the row is multiplied with, d: the direction, x_b itself in the plain form); re-rounded to bf16"""
    W = W.clone()
    x_eff, d = x_eff.double(), d.double()
    for b, r in enumerate(rows):
        W[r] = (W[r].double() + gain * d[b] / float(x_eff[b] @ d[b])).to(W.dtype)
    return W


def margins(R: Ref, rows):
    """per sequence: (ref - tol)[winner] - max over the other rows of (ref + tol); positive = the arg-max is resolved"""
    tol = bound(R, BF, False)
    lo, hi = R.ref - tol, R.ref + tol
    out = []
    for b, r in enumerate(rows):
        others = hi[b].clone()
        others[r] = -math.inf
        out.append(float(lo[b, r] - others.max()))
    return out


@lru_cache(maxsize=4)
def lm_case(V, K, B, norm, fm, xscale=1.0):
    """-> (W with the winners planted, x, norm_w, winner rows, Ref of the logits); the margin is asserted on the reference alone"""
    W0, _, nw = weights(V, K, seed=5)
    x = acts(K, 1, xscale)[0][:B]
    rows = winner_rows(V, B, fm)
    x64 = x.double()
    xn = x64 * rs64(x, EPS) * nw.double()
    if not norm:
        W = plant(W0, x64, x64, rows, 12.0 * xscale)
        R = ref_gemv(x, W)
    elif fm:
        # the kernel multiplies x with bf16(W norm_w): plant along x / norm_w so that the folded row points along x
        W = plant(W0, xn, x64 / nw.double(), rows, 12.0)
        R = ref_gemv(x, W, norm_w=nw, fold=True)
    else:
        W = plant(W0, xn, xn, rows, 12.0)
        R = ref_gemv(x, W, norm_w=nw)
    m = margins(R, rows)
    assert min(m) > 0, f"lm_head V={V} K={K} B={B} norm={norm} fm={fm}: planted winner not resolved, margins {m}"
    assert R.ref.argmax(-1).tolist() == rows
    return W, x, nw, rows, R


# ================================================================================================ the dispatch, restated
def staging(NB, NWB, K, norm):
    """which of the three straight-line forms of stage_rows_branchfree (wq_common.hpp) a row takes, and whether it loops"""
    cap = 6 if NWB == 8 else 4                          # stage_cap(nwb)
    nt, nv = NWB * 64, K // 8
    if not norm:                                        # "if (!norm_w)": one batch of CAP vectors per thread, then the loop
        return "plain-1" if nv <= cap * nt else "plain-loop"
    if nv <= (cap // 2) * nt:                           # "else if (nv <= CH * NT)": the row fits the registers
        return "norm-regs"
    return "norm-loop"                                  # "else": sum of squares in batches of CAP, normalise in batches of CH


def route(entry, B, N, K, norm, sched=1, proc=False):
    """The instantiation a call launches, restated from csrc/llm_decode.hip (environment knobs unset). A mirror, not a probe:
    it exists so that the CPU test can assert that the case table reaches every instantiation it is meant to.
    -> ("gemv_kernel", NB, R, GU, XLDS, NWB, SCHED) | ("skinny_gemm_kernel", GU, NW) | ("skinny_fm_kernel", MODE, NW, NORM, PROC)
       | ("lmhead_partial_kernel", NB, R, PROC); ValueError where the library refuses the call"""
    if entry in ("gemv_fm", "gemv_swiglu_fm", "lm_head_argmax_fm"):
        # spider_gemv_fm_bf16 / _swiglu_fm / lm_head_argmax_fm: "B >= 1 && B <= 16 && ... K % 64 == 0"
        if not (1 <= B <= 16 and N > 0 and K > 0 and K % 64 == 0):
            raise ValueError("fm: 1 <= B <= 16, K a positive multiple of 64")
        if entry == "gemv_swiglu_fm" and N % 16:        # spider_gemv_swiglu_fm_bf16: "I % 16 == 0"
            raise ValueError("gemv_swiglu_fm: I a multiple of 16")
        mode = {"gemv_fm": 0, "gemv_swiglu_fm": 1, "lm_head_argmax_fm": 2}[entry]
        # "if (fold_rmsnorm) skinny_fm_kernel<MODE, 8, true> ... else skinny_fm_kernel<MODE, 8, false>"; _proc: <2, 8, NORM, true>
        return ("skinny_fm_kernel", mode, 8, bool(norm), bool(proc))
    if entry == "lm_head_argmax":
        # spider_lm_head_argmax_bf16: "B >= 1 && B <= 8", "K % 8 == 0 && (size_t)B * K * 2 <= 64 * 1024"
        if not (1 <= B <= 8 and N > 0 and K > 0 and K % 8 == 0 and B * K * 2 <= 64 * 1024):
            raise ValueError("lm_head_argmax: batch must be 1..8, B*K*2 <= 64 KiB")
        return ("lmhead_partial_kernel", B, 2, bool(proc))          # LMHEAD_LAUNCH(NB_): lmhead_partial_kernel<NB_, 2>
    gu = {"gemv": False, "gemv_swiglu": True}[entry]
    if not (N > 0 and K > 0 and K % 8 == 0):            # spider_gemv_bf16: "N > 0 && K > 0 && K % 8 == 0"
        raise ValueError("gemv: K must be a positive multiple of 8")
    # gemv_batch: "if (B >= mfma_min_b && B <= 16 && K % 64 == 0 && norm_w == nullptr)", mfma_min_b = 5
    if 5 <= B <= 16 and K % 64 == 0 and not norm:
        return ("skinny_gemm_kernel", gu, 8)            # "skinny_gemm_kernel<GU, 8><<<(N + 15) / 16, 512"
    if not 1 <= B <= 8:                                 # gemv_batch: "switch (B) ... default: batch must be 1..8"
        raise ValueError("gemv: batch must be 1..8")
    NB = B
    # gemv_dispatch: "xlds = (size_t)NB * K * 2 <= xlds_max || norm_w != nullptr"
    xlds = NB * K * 2 <= XLDS_MAX or norm
    # gemv_dispatch: "SPIDER_CHECK((size_t)NB * K * 2 <= 64 * 1024 || norm_w == nullptr, ...)"
    if norm and NB * K * 2 > 64 * 1024:
        raise ValueError("gemv: fused RMSNorm needs batch*K*2 <= 64 KiB")
    R = 1 if gu else 2                                  # "int R = GU ? 1 : 2;"
    if not gu and N * K * 2 < R2_BYTES:                 # "if (!GU && (size_t)N * K * 2 < (size_t)48 << 20) R = 1;"
        R = 1
    wide8 = (not gu) and K >= 8192 and NB == 1          # "wide8 = ... (!GU && K >= 8192 && NB == 1)"
    s = 0 if not sched else (1 if K <= 4096 else 2)     # "sched = !(hoist && gemv_sched()) ? 0 : (K <= 4096 ? 1 : 2)"
    row = (not gu) and R * NB <= 2 and xlds             # GEMV_LAUNCH: "ROW_ = !GU_ && R_ * NB_ <= 2 && XL_"
    if wide8:                                           # GEMV_LAUNCH: "if (wide8) { if (sched) <.., 8, 2> else <.., 8> }"
        return ("gemv_kernel", NB, R, gu, xlds, 8, 2 if s else 0)
    if s == 1 and row:                                  # "else if (sched == 1 && ROW_) <.., 4, 1>"
        return ("gemv_kernel", NB, R, gu, xlds, 4, 1)
    return ("gemv_kernel", NB, R, gu, xlds, 4, 2 if s else 0)       # "else if (sched) <.., 4, 2> else <.., 4>"


# ================================================================================================ the case table
Case = namedtuple("Case", "group entry B N K norm route")


def _gk(NB, R, GU, XLDS, NWB, SCHED):
    return ("gemv_kernel", NB, R, GU, XLDS, NWB, SCHED)


def _table():
    t = []
    add = lambda *a: t.append(Case(*a))

    def fma(group, entry, B, N, K, rt):
        """a gemv_kernel case: without norm_w and, where the library takes it (B*K*2 <= 64 KiB: the activations are in LDS either
        way, so the instantiation is the same), with norm_w"""
        add(group, entry, B, N, K, False, rt)
        if B * K * 2 <= 64 * 1024:
            assert rt[4] is True
            add(group, entry, B, N, K, True, rt)
    # rows: NB = 5..8 on the FMA kernel (K % 64 != 0, or the fused norm)
    for B in (5, 6, 7, 8):
        fma("rows", "gemv", B, 37, 1032, _gk(B, 1, False, True, 4, 2))
        fma("rows", "gemv_swiglu", B, 20, 1032, _gk(B, 1, True, True, 4, 2))
    # activations through L2
    for B, K in ((2, 18944), (4, 8200), (8, 4104)):
        fma("xl2", "gemv", B, 37, K, _gk(B, 1, False, False, 4, 2))
        fma("xl2", "gemv_swiglu", B, 20, K, _gk(B, 1, True, False, 4, 2))
    fma("xl2", "gemv", 4, 37, 8192, _gk(4, 1, False, True, 4, 2))                   # exactly 64 KiB, with and without the fused norm
    # two rows per wave: the only large weights
    for N in (6145, 6144):
        fma("r2", "gemv", 1, N, 4096, _gk(1, 2, False, True, 4, 1))
        fma("r2", "gemv", 2, N, 4096, _gk(2, 2, False, True, 4, 2))
    fma("r2", "gemv", 1, 1329, 18944, _gk(1, 2, False, True, 8, 2))
    fma("r2", "gemv", 2, 1329, 18944, _gk(2, 2, False, False, 4, 2))
    # staging batches (REQUIRED_STAGING names the form each is there for)
    fma("stage", "gemv", 2, 37, 8200, _gk(2, 1, False, True, 4, 2))
    fma("stage", "gemv", 3, 37, 8200, _gk(3, 1, False, True, 4, 2))
    fma("stage", "gemv_swiglu", 1, 20, 8200, _gk(1, 1, True, True, 4, 2))
    fma("stage", "gemv", 2, 37, 4104, _gk(2, 1, False, True, 4, 2))
    fma("stage", "gemv", 1, 37, 12288, _gk(1, 1, False, True, 8, 2))
    fma("stage", "gemv", 1, 37, 12296, _gk(1, 1, False, True, 8, 2))
    fma("stage", "gemv", 1, 37, 24584, _gk(1, 1, False, True, 8, 2))
    # row-major MFMA
    for B in (5, 9, 13, 16):
        for K in (64, 576, 832, 3648):
            for N in (7, 130):
                add("mfma", "gemv", B, N, K, False, ("skinny_gemm_kernel", False, 8))
            for I in (23, 64):
                add("mfma", "gemv_swiglu", B, I, K, False, ("skinny_gemm_kernel", True, 8))
    # fragment-major MFMA
    for B in (1, 2, 3, 4, 7, 8, 9, 15, 16):
        for K in (64, 576, 832, 3648):
            for norm in (False, True):
                for N in (7, 130):
                    add("fm", "gemv_fm", B, N, K, norm, ("skinny_fm_kernel", 0, 8, norm, False))
                for I in (16, 48):
                    add("fm", "gemv_swiglu_fm", B, I, K, norm, ("skinny_fm_kernel", 1, 8, norm, False))
    # lm_head
    for B in range(1, 9):
        for norm in (False, True):
            add("lm", "lm_head_argmax", B, 333, 1032, norm, ("lmhead_partial_kernel", B, 2, False))
    for B in (1, 5):
        add("lm", "lm_head_argmax", B, 131073, 64, False, ("lmhead_partial_kernel", B, 2, False))
    for B in (1, 2, 7, 16):
        for V, K in ((333, 576), (33000, 128)):
            for norm in (False, True):
                add("lm_fm", "lm_head_argmax_fm", B, V, K, norm, ("skinny_fm_kernel", 2, 8, norm, False))
    return t


TABLE = _table()

# what the table is there to reach (tests/test_gemv_checks_cpu.py asserts it through route())
REQUIRED = (
    [_gk(B, 1, gu, True, 4, 2) for B in (5, 6, 7, 8) for gu in (False, True)] +
    [_gk(B, 1, gu, False, 4, 2) for B in (2, 4, 8) for gu in (False, True)] +
    [_gk(1, 2, False, True, 4, 1), _gk(2, 2, False, True, 4, 2), _gk(1, 2, False, True, 8, 2), _gk(2, 2, False, False, 4, 2)] +
    [_gk(2, 1, False, True, 4, 2), _gk(3, 1, False, True, 4, 2), _gk(1, 1, True, True, 4, 2), _gk(1, 1, False, True, 8, 2)] +
    [("skinny_gemm_kernel", gu, 8) for gu in (False, True)] +
    [("skinny_fm_kernel", m, 8, n, False) for m in (0, 1, 2) for n in (False, True)] +
    [("lmhead_partial_kernel", B, 2, False) for B in range(1, 9)]
)
# (NB, NWB, K, norm) -> form of stage_rows_branchfree, for the "staging batches" cases
REQUIRED_STAGING = {
    (2, 4, 8200, False): "plain-loop", (3, 4, 8200, False): "plain-loop", (1, 4, 8200, False): "plain-loop",
    (2, 4, 4104, True): "norm-loop", (3, 4, 8200, True): "norm-loop",
    (1, 8, 12288, True): "norm-regs", (1, 8, 12296, True): "norm-loop", (1, 8, 24584, False): "plain-loop",
}


def cases(group, **kw):
    return [c for c in TABLE if c.group == group and all(getattr(c, k) == v for k, v in kw.items())]

"""Torch-tensor front end of the C ABI (spider_amd/lib.py -> libspider_hip.so).

PyTorch is used here only for device memory and streams: every function checks shapes/dtypes on the
host, passes raw device pointers + sizes to the HIP library and enqueues on torch's current stream
(so the calls can be captured by ``torch.cuda.graph``). Nothing falls back to torch math.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import lib as _lib

BF16 = torch.bfloat16
ACT = {None: 0, "none": 0, "silu": 1, "gelu": 2, "quick_gelu": 3, "geglu": 4, "leaky_relu": 5, "relu": 6, "tanh": 7, "swiglu": 8,
       "geglu_exact": 9}       # 9: GEGLU with ONE final rounding (precise mode; 4 rounds value, gate and gelu(gate) like an f16 module)
GLU_ACTS = ("geglu", "swiglu", "geglu_exact")


def _stream() -> int:
    """torch's current stream on the CURRENT device: the kernels are launched on that device, so every tensor handed to
    the library must live there (`_chk` enforces it; engines on another GPU run under `torch.cuda.device(...)`)."""
    return torch.cuda.current_stream().cuda_stream


_WS = {}
WS_BYTES = 64 << 20
WS_TAIL = 4096        # zero-initialised bytes behind the workspace: arrival counters of the streaming conv's in-launch combine


import threading as _threading


class _ScopeStack(_threading.local):       # per host thread: two threads may enqueue on two streams at once (bench.py)
    def __init__(self):
        self.names = ["default"]


_WS_SCOPE = _ScopeStack()


class workspace_scope:
    """`with ops.workspace_scope("llm"): ...` -- calls (and graph captures) inside the block use a split-K workspace of their own.
    Reuse of a workspace is stream-ordered, so work that runs on two streams AT ONCE must not share one: bench.py's two-stream
    schedule puts the LLM pass and the diffusion decoder in different scopes. A captured graph keeps the
    workspace of the scope it was captured in. The same holds for the WS_TAIL bytes behind a workspace (arrival counters of the
    streaming conv's in-launch split-K combine: zero whenever no launch of that scope is in flight; two launches that overlapped on
    one workspace would mix their tickets and their partial slabs)."""

    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        _WS_SCOPE.names.append(self.name)
        return self

    def __exit__(self, *exc):
        _WS_SCOPE.names.pop()
        return False


def _workspace(device) -> torch.Tensor:
    """Per-(device, scope) fp32 split-K workspace (stream-ordered reuse; allocated on first use, outside any graph capture:
    engines run an eager warm-up pass before they capture)."""
    key = (device.type, device.index, _WS_SCOPE.names[-1])
    if key not in _WS:
        _WS[key] = torch.zeros((WS_BYTES + WS_TAIL) // 4, dtype=torch.float32, device=device)
    return _WS[key]


F16 = torch.float16


def _h16(t: torch.Tensor):
    """(dtype, entry-point suffix) of a diffusion-side operand: the UNet / VAE / text-encoder operators exist as bf16 and as
    IEEE-half (f16, the reference's torch_dtype) instantiations; every 16-bit operand of one call must share the dtype."""
    if t.dtype == BF16:
        return BF16, "bf16"
    if t.dtype == F16:
        return F16, "f16"
    raise ValueError(f"expected a bfloat16 or float16 tensor, got {t.dtype}")


# ---- tile-major weight copies for the weight-streaming GEMMs / convs (include/spider_hip.h: w_tiled) ----
# An engine marks its long-lived weight tensors with mark_weight(); a GEMM / conv call with at most WTILED_MAX_M output rows then
# runs on the tile-major copy [ceil(N/64)][ceil(K/64)][64][64] of that weight (one contiguous 8 KiB read per K tile of 64 rows
# instead of 64 strided 128-byte pieces), built on first use -- outside graph capture: engines run one eager warm-up pass before
# they capture -- and kept for the life of the tensor object. Unmarked tensors (activations passed as the W operand, slices)
# always take the row-major path, so a recycled allocation can never meet a stale copy.
import os as _os

WTILED_MAX_M = int(_os.environ.get("SPIDER_WTILED_MAX_M", "512"))


def mark_weight(t: torch.Tensor) -> torch.Tensor:
    """Mark a long-lived weight: calls may then run on layout copies of it (tile-major `_tiled`, fragment-major `_wsfm`), built on
    first use and rebuilt when the tag (`t._version`, `t.data_ptr()`) changes. That tag sees only in-place operations on the tensor
    itself (`t.mul_()`, `t.copy_()`) and a new storage (`t.data = ...`). A write through a view that torch does not version --
    `t.data.mul_()`, a raw pointer -- leaves `_version` and `data_ptr()` as they were and is NOT tracked: the
    copy stays stale. No engine writes its weights that way; code that must should drop `t._spider_tiled` / `t._spider_fm` itself."""
    t._spider_weight = True
    return t


def tile_weight64(W2: torch.Tensor) -> torch.Tensor:
    """[N, K] 16-bit -> tile-major [ceil(N/64), ceil(K/64), 64, 64], zero-padded (pure data movement)."""
    N, K = W2.shape
    Np, Kp = (N + 63) // 64 * 64, (K + 63) // 64 * 64
    if (Np, Kp) != (N, K):
        Wp = torch.zeros(Np, Kp, dtype=W2.dtype, device=W2.device)
        Wp[:N, :K] = W2
        W2 = Wp
    return W2.view(Np // 64, 64, Kp // 64, 64).permute(0, 2, 1, 3).contiguous()


def _tiled(W: torch.Tensor, M: int):
    """the tile-major copy of a marked weight when the problem is weight-streaming (M <= WTILED_MAX_M), else None"""
    if M > WTILED_MAX_M or not getattr(W, "_spider_weight", False):
        return None
    t = getattr(W, "_spider_tiled", None)
    tag = (W._version, W.data_ptr())           # an in-place update of the weight (copy_, merge) invalidates the copy
    if t is None or getattr(W, "_spider_tiled_tag", None) != tag:
        if torch.cuda.is_current_stream_capturing():
            if t is not None:
                raise RuntimeError("a marked weight was modified in place and is first used again under stream capture: call "
                                   "ops.prebuild_tiled() (or run one eager pass) before capturing")
            return None
        t = tile_weight64(W.reshape(W.shape[0], -1))
        W._spider_tiled, W._spider_tiled_tag = t, tag
    return t


def prebuild_tiled(weights, max_rows: int = 64 << 20) -> int:
    """Build the tile-major copies of every marked weight in `weights` now (engine constructors: no lazy first-use build, nothing
    left for a stream capture to miss). Returns the bytes the copies occupy (INTEGRATION.md states them per model)."""
    n = 0
    for W in weights:
        if getattr(W, "_spider_weight", False) and W.ndim >= 2 and W.numel() <= max_rows:
            t = _tiled(W, 1)
            n += 0 if t is None else t.numel() * t.element_size()
    return n


# ---- fragment-major conv weights for the weight-stationary streaming kernel (csrc/gemm.hip: wstream_kernel, w_tiled == 2) ----
WS_ENABLE = _os.environ.get("SPIDER_WS", "1") != "0"      # tuning aid: 0 = the tile kernels serve every conv
WS_INLAUNCH = _os.environ.get("SPIDER_WS_INLAUNCH", "1") != "0"
WS_MAX_M = int(_os.environ.get("SPIDER_WS_MAX_M", "128"))   # output pixels up to which the streaming kernel is used (it exists up to 512)


def set_ws_inlaunch(on: bool) -> bool:
    """Switch the split-K combine form of the streaming conv at run time (library + this module's mirror of it, which decides whether
    the producer-statistics entry point is used): True = inside the launch, False = partial slabs + reduce kernel. -> previous form.
    Both forms sum the slabs in split order (bit-identical outputs); tests compare them in one process."""
    global WS_INLAUNCH
    prev = WS_INLAUNCH
    _lib.load().spider_set_ws_inlaunch(int(bool(on)))
    WS_INLAUNCH = bool(on)
    return prev


def repack_fm_conv(W: torch.Tensor) -> torch.Tensor:
    """W [Cout, 3, 3, Cin] 16-bit (OHWI, Cin % 32 == 0) -> [ceil(Cout / 32) * 2, (Cin / 32) * 9, 64, 8]: per group of 16 output
    channels and per (32-channel block cb, tap) one 1 KiB piece whose lane 16 g + r holds W[16 rg + r, tap, 32 cb + 8 g : + 8] --
    the A fragment of mfma_f32_16x16x32; the 9 taps of a channel block are contiguous. Output channels are zero-padded to a
    multiple of 32 (one 2-tile strip per block). Pure data movement, once per weight."""
    N, kh, kw, Cin = W.shape
    assert kh == 3 and kw == 3 and Cin % 32 == 0
    Np = (N + 31) // 32 * 32
    if Np != N:
        W = torch.cat([W, torch.zeros(Np - N, kh, kw, Cin, dtype=W.dtype, device=W.device)], 0)
    # [rg, r, tap, cb, g, e] -> [rg, cb, tap, g, r, e]
    return W.reshape(Np // 16, 16, 9, Cin // 32, 4, 8).permute(0, 3, 2, 4, 1, 5).contiguous().view(Np // 16, (Cin // 32) * 9, 64, 8)


def _ws_eligible(B, Hin, Win, Cin, Cout, kh, kw, stride, pad, dil, up_size, Ho, Wo, act) -> bool:
    """mirror of csrc/gemm.hip:ws_eligible -- 3 x 3 / stride 1 / pad 1 convs with <= 512 output pixels (and an input that fits the
    LDS slab of the kernel's row-group form)"""
    if not WS_ENABLE or (kh, kw) != (3, 3) or stride != 1 or dil != 1 or tuple(pad) != (1, 1) or Cin % 32 or Cout % 4 or act:
        return False
    M, rows = B * Ho * Wo, B * Hin * Win
    if M > WS_MAX_M:
        return False
    if M <= 128:
        return rows <= 128 and up_size is None
    return M <= 512 and rows <= 512


def _wsfm(W: torch.Tensor):
    """the fragment-major copy of a marked conv weight (built on first use, outside stream capture), or None"""
    if not getattr(W, "_spider_weight", False):
        return None
    t = getattr(W, "_spider_fm", None)
    tag = (W._version, W.data_ptr())
    if t is None or getattr(W, "_spider_fm_tag", None) != tag:
        if torch.cuda.is_current_stream_capturing():
            if t is not None:
                raise RuntimeError("a marked weight was modified in place and is first used again under stream capture")
            return None
        t = repack_fm_conv(W)
        W._spider_fm, W._spider_fm_tag = t, tag
    return t


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype, name: str, contiguous: bool = True):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA/HIP tensor (the HIP path has no CPU fallback)")
    if t.device.index != torch.cuda.current_device():
        raise ValueError(f"{name}: tensor lives on {t.device} but the current device is cuda:{torch.cuda.current_device()} "
                         "(kernels launch on the current device: wrap the call in torch.cuda.device(...))")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")


# --------------------------------------------------------------------------- LLM decode
def embed(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """Row gather of 16-bit rows (a copy of bit patterns: one kernel serves bf16 and f16 tables)."""
    dt, _ = _h16(table)
    _chk(table, dt, "table"); _chk(ids, torch.int32, "ids")
    V, H = table.shape
    out = torch.empty(*ids.shape, H, dtype=dt, device=table.device)
    _lib.call("spider_embed_bf16", _p(table), _p(ids), _p(out), ids.numel(), H, V, _stream())
    return out


def rmsnorm(x, w, eps, res=None, res_out=None, out=None):
    _chk(x, BF16, "x"); _chk(w, BF16, "w")
    H = x.shape[-1]
    rows = x.numel() // H
    if out is None:
        out = torch.empty_like(x)
    if res is not None:
        _chk(res, BF16, "res")
    _lib.call("spider_rmsnorm_bf16", _p(x), _p(res), _p(w), _p(out), _p(res_out), rows, H, float(eps), _stream())
    return out


def decode_advance(next_ids, cur_ids, pos, slot, kv_end, hist=None, n_hist=None):
    """End of a decode step in one launch: cur_ids <- next_ids; pos, slot, kv_end += 1; hist[b, n_hist[b]++] = next_ids[b]."""
    for t, n in ((next_ids, "next_ids"), (cur_ids, "cur_ids"), (pos, "pos"), (slot, "slot"), (kv_end, "kv_end")):
        _chk(t, torch.int32, n)
    B = next_ids.numel()
    assert cur_ids.numel() == B and pos.numel() == B and slot.numel() == B and kv_end.numel() == B
    cap = 0
    if hist is not None:
        _chk(hist, torch.int32, "hist"); _chk(n_hist, torch.int32, "n_hist")
        assert hist.dim() == 2 and hist.shape[0] == B and n_hist.numel() == B
        cap = hist.shape[1]
    _lib.call("spider_decode_advance_i32", _p(next_ids), _p(cur_ids), _p(pos), _p(slot), _p(kv_end), _p(hist), _p(n_hist), cap, B, _stream())


def gemv(W, x, bias=None, res=None, norm_w=None, eps=0.0, out=None):
    """out[b,n] = sum_k xin[b,k] W[n,k] (+bias) (+res); xin = rmsnorm(x)*norm_w if norm_w is given. 1 <= B <= 8."""
    _chk(W, BF16, "W"); _chk(x, BF16, "x")
    N, K = W.shape
    B = x.numel() // K
    if out is None:
        out = torch.empty(B, N, dtype=BF16, device=x.device)
    _lib.call("spider_gemv_bf16", _p(W), _p(x), _p(out), _p(bias), _p(res), _p(norm_w), float(eps), B, N, K, _stream())
    return out


def gemv_swiglu(W_gate_up, x, norm_w=None, eps=0.0, out=None):
    _chk(W_gate_up, BF16, "W_gate_up"); _chk(x, BF16, "x")
    I2, K = W_gate_up.shape
    I = I2 // 2
    B = x.numel() // K
    if out is None:
        out = torch.empty(B, I, dtype=BF16, device=x.device)
    _lib.call("spider_gemv_swiglu_bf16", _p(W_gate_up), _p(x), _p(out), _p(norm_w), float(eps), B, I, K, _stream())
    return out


def _wq_plain(sym, chk, Wq, scale, x, bias, res, norm_w, eps, out, name):
    """the body of gemv_w8 / gemv_w4: chk = the format's checker (-> K, B), sym = its kernel"""
    K, B = chk(Wq, scale, x, name)
    N = Wq.shape[0]
    for t, n, cnt in ((bias, "bias", N), (res, "res", B * N), (norm_w, "norm_w", K)):
        if t is not None:
            _chk(t, BF16, n)
            assert t.numel() == cnt, f"{n}: expected {cnt} elements"
    if out is None:
        out = torch.empty(B, N, dtype=BF16, device=x.device)
    _chk(out, BF16, "out")
    assert out.numel() == B * N
    _lib.call(sym, _p(Wq), _p(scale), _p(x), _p(out), _p(bias), _p(res), _p(norm_w), float(eps), B, N, K, _stream())
    return out


def _wq_swiglu(sym, chk, Wq_gate_up, scale, x, norm_w, eps, out, name):
    """the body of gemv_swiglu_w8 / gemv_swiglu_w4"""
    K, B = chk(Wq_gate_up, scale, x, name)
    I = Wq_gate_up.shape[0] // 2
    assert Wq_gate_up.shape[0] == 2 * I
    if norm_w is not None:
        _chk(norm_w, BF16, "norm_w")
        assert norm_w.numel() == K
    if out is None:
        out = torch.empty(B, I, dtype=BF16, device=x.device)
    _chk(out, BF16, "out")
    assert out.numel() == B * I
    _lib.call(sym, _p(Wq_gate_up), _p(scale), _p(x), _p(out), _p(norm_w), float(eps), B, I, K, _stream())
    return out


FP8 = torch.float8_e4m3fn      # OCP e4m3fn (448 = 0x7e), the FP8 of gfx950 -- not MI300's e4m3fnuz
W8_LDS_MAX_DEFAULT = 160 * 1024 - 256  # bytes of staged activations per block (csrc/wq_common.hpp: WQ_LDS_HW_LIMIT)
W8_MAX_ROWS = 4                # rows the weight-only FP8 GEMVs exist for
W8_LDS_MAX = min(int(_os.environ.get("SPIDER_W8_LDS_MAX", "0")) or W8_LDS_MAX_DEFAULT, 160 * 1024 - 256)   # mirror of csrc/wq_common.hpp: wq_lds_max<8>


def w8_norm_fits(B: int, K: int) -> bool:
    """True when gemv_w8 / gemv_swiglu_w8 can fuse the RMSNorm for B rows of K: the staged activations (rows padded to whole
    1024-element chunks) fit the kernel's LDS budget (csrc/wq_common.hpp: wq_lds_bytes<8> against wq_lds_max<8>)"""
    return B * ((K + 1023) // 1024) * 2048 <= W8_LDS_MAX


def _chk_w8(Wq, scale, x, name):
    _chk(Wq, FP8, name); _chk(scale, torch.float32, "scale"); _chk(x, BF16, "x")
    if Wq.dim() != 2 or scale.numel() != Wq.shape[0]:
        raise ValueError(f"{name}: expected a [N, K] weight with one scale per row, got {tuple(Wq.shape)} and {scale.numel()} scales")
    K = Wq.shape[1]
    if x.shape[-1] != K:
        raise ValueError(f"{name}: x[..., {x.shape[-1]}] vs {name}[{Wq.shape[0]}, {K}]")
    return K, x.numel() // K


def gemv_w8(Wq, scale, x, bias=None, res=None, norm_w=None, eps=0.0, out=None):
    """`gemv` on weight-only FP8: Wq [N, K] float8_e4m3fn, scale [N] fp32 per weight row (llm.quantize_fp8_rows);
    out[b,n] = scale[n] * sum_k xin[b,k] f32(Wq[n,k]) (+bias) (+res), the fp32 sum scaled once after the reduction. 1 <= B <= 4,
    K % 16 == 0."""
    return _wq_plain("spider_gemv_w8", _chk_w8, Wq, scale, x, bias, res, norm_w, eps, out, "Wq")


def gemv_swiglu_w8(Wq_gate_up, scale, x, norm_w=None, eps=0.0, out=None):
    """`gemv_swiglu` on weight-only FP8: Wq_gate_up [2 I, K] = [gate rows | up rows], scale [2 I]. 1 <= B <= 4, K % 16 == 0."""
    return _wq_swiglu("spider_gemv_swiglu_w8", _chk_w8, Wq_gate_up, scale, x, norm_w, eps, out, "Wq_gate_up")


W4_LDS_MAX_DEFAULT = 160 * 1024 - 256  # bytes of staged activations per block (csrc/wq_common.hpp: WQ_LDS_HW_LIMIT)
W4_MAX_ROWS = 4                # rows the weight-only MXFP4 GEMVs exist for
W4_LDS_MAX = min(int(_os.environ.get("SPIDER_W4_LDS_MAX", "0")) or W4_LDS_MAX_DEFAULT, 160 * 1024 - 256)   # mirror of csrc/wq_common.hpp: wq_lds_max<4>


def w4_norm_fits(B: int, K: int) -> bool:
    """True when gemv_w4 / gemv_swiglu_w4 can fuse the RMSNorm for B rows of K: the staged activations (rows padded to whole
    2048-element chunks) fit the kernel's LDS budget (csrc/wq_common.hpp: wq_lds_bytes<4> against wq_lds_max<4>)"""
    return B * ((K + 2047) // 2048) * 4096 <= W4_LDS_MAX


def _chk_w4(blocks, scales, x, name):
    _chk(blocks, torch.uint8, name); _chk(scales, torch.uint8, "scales"); _chk(x, BF16, "x")
    if blocks.dim() != 2 or blocks.shape[1] % 16 or scales.dim() != 2 or tuple(scales.shape) != (blocks.shape[0], blocks.shape[1] // 16):
        raise ValueError(f"{name}: expected [N, K / 2] bytes (K % 32 == 0) with scales [N, K / 32], got {tuple(blocks.shape)} and "
                         f"{tuple(scales.shape)}")
    K = blocks.shape[1] * 2
    if x.shape[-1] != K:
        raise ValueError(f"{name}: x[..., {x.shape[-1]}] vs {name}[{blocks.shape[0]}, {K} / 2]")
    B = x.numel() // K
    if not 1 <= B <= W4_MAX_ROWS:
        raise ValueError(f"{name}: {B} rows of x, the MXFP4 GEMVs exist for 1..{W4_MAX_ROWS}")
    return K, B


def gemv_w4(blocks, scales, x, bias=None, res=None, norm_w=None, eps=0.0, out=None):
    """`gemv` on weight-only MXFP4 (llm.quantize_mxfp4): blocks [N, K / 2] uint8, two e2m1 codes per byte, low nibble first;
    scales [N, K / 32] uint8, E8M0, bytes 1..254. out[b,n] = sum_k xin[b,k] W_eff[n,k] (+bias) (+res) with
    W_eff[n,k] = e2m1(code) * 2^(scales[n, k / 32] - 127), the scale applied inside the conversion. 1 <= B <= 4, K % 32 == 0."""
    return _wq_plain("spider_gemv_w4", _chk_w4, blocks, scales, x, bias, res, norm_w, eps, out, "blocks")


def gemv_swiglu_w4(blocks_gate_up, scales, x, norm_w=None, eps=0.0, out=None):
    """`gemv_swiglu` on weight-only MXFP4: blocks_gate_up [2 I, K / 2] = [gate rows | up rows], scales [2 I, K / 32].
    1 <= B <= 4, K % 32 == 0."""
    return _wq_swiglu("spider_gemv_swiglu_w4", _chk_w4, blocks_gate_up, scales, x, norm_w, eps, out, "blocks_gate_up")


def repack_fm16(W: torch.Tensor, norm_w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W [N, K] bf16 (K % 64 == 0); with norm_w [K] the copy holds bf16(W * norm_w) for the kernels' fold_rmsnorm form.
    W -> fragment-major copy [ceil(N/16), K/64, 2, 64, 8] for the *_fm kernels: piece (rg, kb, sx)
    holds, at lane 16 g + r, W[16 rg + r, 64 kb + 32 sx + 8 g : + 8]. Pure data movement, done once when an engine loads its
    weights (like the OIHW -> OHWI conv repack); rows are zero-padded to a multiple of 16."""
    dt, _ = _h16(W)
    _chk(W, dt, "W")
    N, K = W.shape
    assert K % 64 == 0, "repack_fm16: K must be a multiple of 64"
    if norm_w is not None:
        W = (W.float() * norm_w.float()[None, :]).to(dt)
    NG = (N + 15) // 16
    if NG * 16 != N:
        W = torch.cat([W, torch.zeros(NG * 16 - N, K, dtype=dt, device=W.device)], 0)
    # [rg, r, kb, sx, g, e] -> [rg, kb, sx, g, r, e]
    return W.view(NG, 16, K // 64, 2, 4, 8).permute(0, 2, 3, 4, 1, 5).contiguous().view(NG, K // 64, 2, 64, 8)


def gemv_fm(Wfm, x, N, bias=None, res=None, out=None, norm_eps=None):
    """out[b, n] = sum_k x[b, k] W[n, k] (+bias) (+res) on the fragment-major copy Wfm = repack_fm16(W); 1 <= B <= 16.
    norm_eps: RMSNorm folded in -- Wfm = repack_fm16(W, norm_w), x un-normalised."""
    _chk(Wfm, BF16, "Wfm"); _chk(x, BF16, "x")
    K = Wfm.shape[1] * 64
    B = x.numel() // K
    assert x.shape[-1] == K and Wfm.shape[0] == (N + 15) // 16
    if out is None:
        out = torch.empty(B, N, dtype=BF16, device=x.device)
    _lib.call("spider_gemv_fm_bf16", _p(Wfm), _p(x), _p(out), _p(bias), _p(res), B, N, K, int(norm_eps is not None),
              float(norm_eps or 0.0), _stream())
    return out


def gemv_swiglu_fm(Wfm_gate_up, x, out=None, norm_eps=None):
    """out = silu(x @ Wg^T) * (x @ Wu^T) on repack_fm16(cat([Wg, Wu])); I % 16 == 0."""
    _chk(Wfm_gate_up, BF16, "Wfm_gate_up"); _chk(x, BF16, "x")
    K = Wfm_gate_up.shape[1] * 64
    I = Wfm_gate_up.shape[0] * 16 // 2
    B = x.numel() // K
    assert x.shape[-1] == K and I % 16 == 0
    if out is None:
        out = torch.empty(B, I, dtype=BF16, device=x.device)
    _lib.call("spider_gemv_swiglu_fm_bf16", _p(Wfm_gate_up), _p(x), _p(out), B, I, K, int(norm_eps is not None), float(norm_eps or 0.0),
              _stream())
    return out


QFM_MAX_ROWS = 16              # rows the fragment-major weight-only GEMVs exist for (one 16-wide MFMA tile)


def _pad_rows(t: torch.Tensor, rows: int, fill: int) -> torch.Tensor:
    if t.shape[0] == rows:
        return t
    return torch.cat([t, torch.full((rows - t.shape[0],) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)], 0)


def repack_fm_w4(blocks: torch.Tensor, scales: torch.Tensor):
    """MXFP4 weights in the public layout (blocks [N, K / 2] uint8, scales [N, K / 32] uint8; K % 128 == 0) -> the fragment-major
    copies (qfm [NG, K / 128, 64, 16], efm [NG, K / 128, 16, 4]) of the *_fm_w4 kernels, NG = ceil(N / 16). In piece (rg, kb) byte
    4 sx + j of lane 16 g + r is blocks[16 rg + r, (128 kb + 32 sx + 8 g) / 2 + j] -- dword sx of a lane holds
    W[16 rg + r][128 kb + 32 sx + 8 g .. + 7], its A fragment of MFMA sub-step sx -- and efm byte (r, sx) is scales[16 rg + r, 4 kb + sx].
    Rows are padded to a multiple of 16 with nibble code 0 and scale byte 127. Pure data movement, on whichever device the bytes are."""
    if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8 or blocks.dim() != 2 or scales.dim() != 2:
        raise ValueError("repack_fm_w4: expected uint8 blocks [N, K / 2] and scales [N, K / 32]")
    N, K = blocks.shape[0], blocks.shape[1] * 2
    if K % 128 or N < 1 or tuple(scales.shape) != (N, K // 32):
        raise ValueError(f"repack_fm_w4: K must be a multiple of 128 with scales [N, K / 32], got blocks {tuple(blocks.shape)} and "
                         f"scales {tuple(scales.shape)}")
    NG = (N + 15) // 16
    b, s = _pad_rows(blocks, NG * 16, 0), _pad_rows(scales, NG * 16, 127)
    # [rg, r, kb, sx, g, j] -> [rg, kb, g, r, sx, j];  [rg, r, kb, sx] -> [rg, kb, r, sx]
    qfm = b.view(NG, 16, K // 128, 4, 4, 4).permute(0, 2, 4, 1, 3, 5).contiguous().view(NG, K // 128, 64, 16)
    efm = s.view(NG, 16, K // 128, 4).permute(0, 2, 1, 3).contiguous()
    return qfm, efm


def unpack_fm_w4(qfm: torch.Tensor, efm: torch.Tensor, N: int):
    """the exact inverse of repack_fm_w4: (blocks [N, K / 2], scales [N, K / 32])"""
    NG, KB = qfm.shape[0], qfm.shape[1]
    if tuple(qfm.shape[2:]) != (64, 16) or tuple(efm.shape) != (NG, KB, 16, 4) or NG != (N + 15) // 16:
        raise ValueError(f"unpack_fm_w4: qfm {tuple(qfm.shape)} / efm {tuple(efm.shape)} are no fragment-major copy of {N} rows")
    b = qfm.view(NG, KB, 4, 16, 4, 4).permute(0, 3, 1, 4, 2, 5).contiguous().view(NG * 16, KB * 64)
    s = efm.permute(0, 2, 1, 3).contiguous().view(NG * 16, KB * 4)
    return b[:N].contiguous(), s[:N].contiguous()


def repack_fm_w8(q: torch.Tensor) -> torch.Tensor:
    """FP8 weights q [N, K] float8_e4m3fn (K % 64 == 0) -> the fragment-major copy qfm uint8 [NG, K / 64, 64, 16] of the *_fm_w8
    kernels: in piece (rg, kb) byte 8 sx + e of lane 16 g + r is q[16 rg + r, 64 kb + 32 sx + 8 g + e]. Rows are padded to a multiple
    of 16 with zero bytes; the per-row scale of llm.quantize_fp8_rows is used as it is."""
    if q.dtype != FP8 or q.dim() != 2:
        raise ValueError("repack_fm_w8: expected a float8_e4m3fn weight [N, K]")
    N, K = q.shape
    if K % 64 or N < 1:
        raise ValueError(f"repack_fm_w8: K must be a multiple of 64, got {tuple(q.shape)}")
    NG = (N + 15) // 16
    b = _pad_rows(q.contiguous().view(torch.uint8), NG * 16, 0)
    # [rg, r, kb, sx, g, e] -> [rg, kb, g, r, sx, e]
    return b.view(NG, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous().view(NG, K // 64, 64, 16)


def unpack_fm_w8(qfm: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """the exact inverse of repack_fm_w8: q [N, K] float8_e4m3fn"""
    NG = (N + 15) // 16
    if K % 64 or tuple(qfm.shape) != (NG, K // 64, 64, 16):
        raise ValueError(f"unpack_fm_w8: qfm {tuple(qfm.shape)} is no fragment-major copy of [{N}, {K}]")
    b = qfm.view(NG, K // 64, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).contiguous().view(NG * 16, K)
    return b[:N].contiguous().view(FP8)


def _chk_qfm(qfm, sc, x, rows, name, fmt):
    """shapes of a fragment-major weight-only call: -> (K, B). rows = weight rows of the copy (N, or 2 I); fmt 4 / 8"""
    _chk(qfm, torch.uint8, name); _chk(x, BF16, "x")
    kp = 128 if fmt == 4 else 64
    if qfm.dim() != 4 or tuple(qfm.shape[2:]) != (64, 16) or rows < 1 or qfm.shape[0] != (rows + 15) // 16:
        raise ValueError(f"{name}: expected [ceil(rows / 16), K / {kp}, 64, 16] bytes for {rows} weight rows, got {tuple(qfm.shape)}")
    K = qfm.shape[1] * kp
    if fmt == 4:
        _chk(sc, torch.uint8, "efm")
        if tuple(sc.shape) != (qfm.shape[0], qfm.shape[1], 16, 4):
            raise ValueError(f"{name}: expected efm {(qfm.shape[0], qfm.shape[1], 16, 4)}, got {tuple(sc.shape)}")
    else:
        _chk(sc, torch.float32, "scale")
        if sc.numel() != rows:
            raise ValueError(f"{name}: expected one scale per weight row ({rows}), got {sc.numel()}")
    if K == 0 or x.shape[-1] != K:
        raise ValueError(f"{name}: x[..., {x.shape[-1]}] vs K = {K}")
    B = x.numel() // K
    if not 1 <= B <= QFM_MAX_ROWS:
        raise ValueError(f"{name}: {B} rows of x, the fragment-major weight-only GEMVs exist for 1..{QFM_MAX_ROWS}")
    return K, B


def _qfm_plain(sym, qfm, sc, x, N, bias, res, out, name, fmt):
    K, B = _chk_qfm(qfm, sc, x, N, name, fmt)
    for t, n, cnt in ((bias, "bias", N), (res, "res", B * N)):
        if t is not None:
            _chk(t, BF16, n)
            assert t.numel() == cnt, f"{n}: expected {cnt} elements"
    if out is None:
        out = torch.empty(B, N, dtype=BF16, device=x.device)
    _chk(out, BF16, "out")
    assert out.numel() == B * N
    _lib.call(sym, _p(qfm), _p(sc), _p(x), _p(out), _p(bias), _p(res), B, N, K, _stream())
    return out


def _qfm_swiglu(sym, qfm, sc, x, out, name, fmt):
    I = qfm.shape[0] * 16 // 2 if qfm.dim() == 4 else 0
    if I < 1 or I % 16:
        raise ValueError(f"{name}: the copy must hold [gate rows | up rows] with I a multiple of 16, got {tuple(qfm.shape)}")
    K, B = _chk_qfm(qfm, sc, x, 2 * I, name, fmt)
    if out is None:
        out = torch.empty(B, I, dtype=BF16, device=x.device)
    _chk(out, BF16, "out")
    assert out.numel() == B * I
    _lib.call(sym, _p(qfm), _p(sc), _p(x), _p(out), B, I, K, _stream())
    return out


def gemv_fm_w4(qfm, efm, x, N, bias=None, res=None, out=None):
    """`gemv_w4` on the fragment-major copy (qfm, efm) = repack_fm_w4(blocks, scales): out[b, n] = sum_k x[b, k] W_eff[n, k] (+bias)
    (+res) on the matrix cores, 1 <= B <= 16, K % 128 == 0. No fused RMSNorm: x is used as it is."""
    return _qfm_plain("spider_gemv_fm_w4", qfm, efm, x, N, bias, res, out, "qfm", 4)


def gemv_swiglu_fm_w4(qfm, efm, x, out=None):
    """`gemv_swiglu_w4` on repack_fm_w4 of [gate rows | up rows] (I % 16 == 0); 1 <= B <= 16."""
    return _qfm_swiglu("spider_gemv_swiglu_fm_w4", qfm, efm, x, out, "qfm_gate_up", 4)


def gemv_fm_w8(qfm, scale, x, N, bias=None, res=None, out=None):
    """`gemv_w8` on the fragment-major copy qfm = repack_fm_w8(Wq) with the per-row scale [N] fp32 as it is:
    out[b, n] = scale[n] * sum_k x[b, k] f32(Wq[n, k]) (+bias) (+res) on the matrix cores, 1 <= B <= 16, K % 64 == 0."""
    return _qfm_plain("spider_gemv_fm_w8", qfm, scale, x, N, bias, res, out, "qfm", 8)


def gemv_swiglu_fm_w8(qfm, scale, x, out=None):
    """`gemv_swiglu_w8` on repack_fm_w8 of [gate rows | up rows] (I % 16 == 0), scale [2 I]; 1 <= B <= 16."""
    return _qfm_swiglu("spider_gemv_swiglu_fm_w8", qfm, scale, x, out, "qfm_gate_up", 8)


def _lm_head_bufs(x, B, V, out_ids, ws):
    """ids and workspaces of the bf16 lm_head_argmax* calls, allocated where missing -> (out_ids, ws, entries a workspace needs)"""
    n = B * lm_head_nparts(V)
    if ws is None:
        ws = (torch.empty(n, dtype=torch.float32, device=x.device), torch.empty(n, dtype=torch.int32, device=x.device))
    if out_ids is None:
        out_ids = torch.empty(B, dtype=torch.int32, device=x.device)
    return out_ids, ws, n


def lm_head_argmax_fm(Wfm, x, V, out_ids=None, logits=None, ws=None, norm_eps=None):
    """Greedy argmax of x @ W^T on the fragment-major lm_head copy; 1 <= B <= 16. x normalised, or (norm_eps given, Wfm =
    repack_fm16(W, norm_w)) the un-normalised last hidden state."""
    _chk(Wfm, BF16, "Wfm"); _chk(x, BF16, "x")
    K = Wfm.shape[1] * 64
    B = x.numel() // K
    out_ids, ws, n = _lm_head_bufs(x, B, V, out_ids, ws)
    assert ws[0].numel() >= n and ws[1].numel() >= n
    _lib.call("spider_lm_head_argmax_fm_bf16", _p(Wfm), _p(x), _p(out_ids), _p(logits), _p(ws[0]), _p(ws[1]), B, V, K,
              int(norm_eps is not None), float(norm_eps or 0.0), _stream())
    return out_ids


def lm_head_nparts(V: int) -> int:
    return _lib.load().spider_lm_head_nparts(V)


def lm_head_argmax(W, x, norm_w=None, eps=0.0, out_ids=None, logits=None, ws=None):
    _chk(W, BF16, "W"); _chk(x, BF16, "x")
    V, K = W.shape
    B = x.numel() // K
    out_ids, ws, _ = _lm_head_bufs(x, B, V, out_ids, ws)
    _lib.call("spider_lm_head_argmax_bf16", _p(W), _p(x), _p(norm_w), float(eps), _p(out_ids), _p(logits),
              _p(ws[0]), _p(ws[1]), B, V, K, _stream())
    return out_ids


def bitmap_words(V: int) -> int:
    return (V + 31) // 32


def _proc_args(proc: dict, B: int, V: int):
    """The logits-processor buffers of the *_proc lm_head forms: seen / ban int32 [B, ceil(V/32)] (uint32 bit patterns), penalty
    float32 [1], min_new / n_eos int32 [1], eos_ids int32 [8], n_hist int32 [B]."""
    W = bitmap_words(V)
    for k in ("seen", "ban"):
        _chk(proc[k], torch.int32, k)
        assert proc[k].numel() == B * W, f"{k}: expected [{B}, {W}] words"
    _chk(proc["penalty"], torch.float32, "penalty")
    for k, n in (("min_new", 1), ("n_eos", 1), ("eos_ids", 8), ("n_hist", B)):
        _chk(proc[k], torch.int32, k)
        assert proc[k].numel() >= n, f"{k}: expected at least {n} entries"
    return tuple(_p(proc[k]) for k in ("seen", "ban", "penalty", "min_new", "eos_ids", "n_eos", "n_hist"))


def lm_head_argmax_proc(W, x, proc: dict, norm_w=None, eps=0.0, out_ids=None, logits=None, ws=None):
    """lm_head_argmax with HF's logits processors in the arg-max epilogue (repetition penalty on the ids of proc['seen'], -inf on
    the ids of proc['ban'] and on the EOS ids while n_hist < min_new); `logits` stay the raw logits. 1 <= B <= 8."""
    _chk(W, BF16, "W"); _chk(x, BF16, "x")
    V, K = W.shape
    B = x.numel() // K
    out_ids, ws, n = _lm_head_bufs(x, B, V, out_ids, ws)
    assert ws[0].numel() >= n and ws[1].numel() >= n
    if logits is not None:
        assert logits.numel() == B * V
    _lib.call("spider_lm_head_argmax_proc_bf16", _p(W), _p(x), _p(norm_w), float(eps), _p(out_ids), _p(logits),
              _p(ws[0]), _p(ws[1]), *_proc_args(proc, B, V), B, V, K, _stream())
    return out_ids


def lm_head_argmax_fm_proc(Wfm, x, V, proc: dict, out_ids=None, logits=None, ws=None, norm_eps=None):
    """lm_head_argmax_fm with the logits processors of lm_head_argmax_proc; 1 <= B <= 16."""
    _chk(Wfm, BF16, "Wfm"); _chk(x, BF16, "x")
    K = Wfm.shape[1] * 64
    B = x.numel() // K
    assert x.shape[-1] == K and Wfm.shape[0] == (V + 15) // 16
    out_ids, ws, n = _lm_head_bufs(x, B, V, out_ids, ws)
    assert ws[0].numel() >= n and ws[1].numel() >= n
    if logits is not None:
        assert logits.numel() == B * V
    _lib.call("spider_lm_head_argmax_fm_proc_bf16", _p(Wfm), _p(x), _p(out_ids), _p(logits), _p(ws[0]), _p(ws[1]),
              *_proc_args(proc, B, V), B, V, K, int(norm_eps is not None), float(norm_eps or 0.0), _stream())
    return out_ids


LM_HEAD_Q_MAX_ROWS = 4         # rows the weight-only lm_head kernels exist for (csrc/lm_head_wq.hip)


def _lm_head_q_bufs(name, x, B, V, K, norm_w, out_ids, logits, ws):
    """rows, norm, ids, logits and workspaces of the lm_head_argmax*_w8 / _w4 calls, checked and allocated where missing"""
    if not 1 <= B <= LM_HEAD_Q_MAX_ROWS:
        raise ValueError(f"{name}: {B} rows of x, the weight-only lm_head kernels exist for 1..{LM_HEAD_Q_MAX_ROWS}")
    if norm_w is not None:
        _chk(norm_w, BF16, "norm_w")
        if norm_w.numel() != K:
            raise ValueError(f"{name}: norm_w has {norm_w.numel()} elements, K is {K}")
    npart = lm_head_nparts(V)
    if ws is None:
        ws = (torch.empty(B * npart, dtype=torch.float32, device=x.device), torch.empty(B * npart, dtype=torch.int32, device=x.device))
    _chk(ws[0], torch.float32, "ws[0]"); _chk(ws[1], torch.int32, "ws[1]")
    if ws[0].numel() < B * npart or ws[1].numel() < B * npart:
        raise ValueError(f"{name}: the workspaces need {B * npart} entries each")
    if logits is not None:
        _chk(logits, BF16, "logits")
        if logits.numel() != B * V:
            raise ValueError(f"{name}: logits has {logits.numel()} elements, expected [{B}, {V}]")
    if out_ids is None:
        out_ids = torch.empty(B, dtype=torch.int32, device=x.device)
    _chk(out_ids, torch.int32, "out_ids")
    if out_ids.numel() < B:
        raise ValueError(f"{name}: out_ids needs {B} entries")
    return out_ids, ws


def _lm_head_q(sym, q, scale, x, proc, norm_w, eps, out_ids, logits, ws):
    """the body of lm_head_argmax[_proc]_w8 / _w4: sym = the kernel, "spider_" + the wrapper's name; proc None: the plain form"""
    if sym.endswith("_w8"):
        K, B = _chk_w8(q, scale, x, "q")
        if K % 16:
            raise ValueError(f"q: K = {K} has to be a multiple of 16 (16 e4m3 weights per 16-byte load)")
    else:
        K, B = _chk_w4(q, scale, x, "blocks")
    V = q.shape[0]
    out_ids, ws = _lm_head_q_bufs(sym[len("spider_"):], x, B, V, K, norm_w, out_ids, logits, ws)
    _lib.call(sym, _p(q), _p(scale), _p(x), _p(norm_w), float(eps), _p(out_ids), _p(logits), _p(ws[0]), _p(ws[1]),
              *(() if proc is None else _proc_args(proc, B, V)), B, V, K, _stream())
    return out_ids


def lm_head_argmax_w8(q, scale, x, norm_w=None, eps=0.0, out_ids=None, logits=None, ws=None):
    """`lm_head_argmax` on a weight-only FP8 head (llm.quantize_fp8_rows): q [V, K] float8_e4m3fn, scale [V] fp32; the fp32 sum is
    scaled once after the reduction. 1 <= B <= 4, K % 16 == 0; the fused norm needs w8_norm_fits(B, K)."""
    return _lm_head_q("spider_lm_head_argmax_w8", q, scale, x, None, norm_w, eps, out_ids, logits, ws)


def lm_head_argmax_proc_w8(q, scale, x, proc: dict, norm_w=None, eps=0.0, out_ids=None, logits=None, ws=None):
    """lm_head_argmax_w8 with the logits processors of lm_head_argmax_proc in the arg-max epilogue; `logits` stay raw."""
    return _lm_head_q("spider_lm_head_argmax_proc_w8", q, scale, x, proc, norm_w, eps, out_ids, logits, ws)


def lm_head_argmax_w4(blocks, scales, x, norm_w=None, eps=0.0, out_ids=None, logits=None, ws=None):
    """`lm_head_argmax` on a weight-only MXFP4 head (llm.quantize_mxfp4): blocks [V, K / 2] uint8, scales [V, K / 32] uint8 (E8M0,
    bytes 1..254), the block scale applied inside the conversion. 1 <= B <= 4, K % 32 == 0; the fused norm needs
    w4_norm_fits(B, K)."""
    return _lm_head_q("spider_lm_head_argmax_w4", blocks, scales, x, None, norm_w, eps, out_ids, logits, ws)


def lm_head_argmax_proc_w4(blocks, scales, x, proc: dict, norm_w=None, eps=0.0, out_ids=None, logits=None, ws=None):
    """lm_head_argmax_w4 with the logits processors of lm_head_argmax_proc in the arg-max epilogue; `logits` stay raw."""
    return _lm_head_q("spider_lm_head_argmax_proc_w4", blocks, scales, x, proc, norm_w, eps, out_ids, logits, ws)


def decode_advance_seen(next_ids, cur_ids, pos, slot, kv_end, seen, V, hist=None, n_hist=None):
    """decode_advance, and bit next_ids[b] of seen [B, ceil(V/32)] is set (the processed greedy path's token set)."""
    for t, n in ((next_ids, "next_ids"), (cur_ids, "cur_ids"), (pos, "pos"), (slot, "slot"), (kv_end, "kv_end"), (seen, "seen")):
        _chk(t, torch.int32, n)
    B = next_ids.numel()
    assert cur_ids.numel() == B and pos.numel() == B and slot.numel() == B and kv_end.numel() == B
    assert seen.numel() == B * bitmap_words(V)
    cap = 0
    if hist is not None:
        _chk(hist, torch.int32, "hist"); _chk(n_hist, torch.int32, "n_hist")
        assert hist.dim() == 2 and hist.shape[0] == B and n_hist.numel() == B
        cap = hist.shape[1]
    _lib.call("spider_decode_advance_seen_i32", _p(next_ids), _p(cur_ids), _p(pos), _p(slot), _p(kv_end), _p(hist), _p(n_hist),
              _p(seen), V, cap, B, _stream())


def _ngram_args(ng: dict, hist, n_hist, B: int, V: int):
    """The buffers of the n-gram ban: ng = dict(prompt_ids int32 [B, pcap], n_prompt int32 [1], ngram int32 [1], ban / ban_step
    int32 [B, ceil(V/32)] (uint32 bit patterns, two buffers)); hist int32 [B, cap], n_hist int32 [B]."""
    W = bitmap_words(V)
    for k in ("prompt_ids", "n_prompt", "ngram", "ban", "ban_step"):
        _chk(ng[k], torch.int32, k)
    _chk(hist, torch.int32, "hist"); _chk(n_hist, torch.int32, "n_hist")
    assert ng["prompt_ids"].dim() == 2 and ng["prompt_ids"].shape[0] == B and ng["prompt_ids"].shape[1] > 0
    assert hist.dim() == 2 and hist.shape[0] == B and hist.shape[1] > 0 and n_hist.numel() == B
    assert ng["n_prompt"].numel() >= 1 and ng["ngram"].numel() >= 1
    assert ng["ban"].numel() == B * W and ng["ban_step"].numel() == B * W, f"ban / ban_step: expected [{B}, {W}] words"
    assert ng["ban"].data_ptr() != ng["ban_step"].data_ptr(), "ban_step must not alias ban"


def ngram_ban(ng: dict, hist, n_hist, V):
    """no_repeat_ngram_size: ng['ban_step'] = ng['ban'] | the tokens that would complete an n-gram (n = ng['ngram'][0]) already in
    the row's sequence prompt_ids[b, :n_prompt[0]] ++ hist[b, :n_hist[b]] (buffers: `_ngram_args`)."""
    B = n_hist.numel()
    _ngram_args(ng, hist, n_hist, B, V)
    _lib.call("spider_ngram_ban_i32", _p(ng["prompt_ids"]), _p(ng["n_prompt"]), ng["prompt_ids"].shape[1], _p(hist), _p(n_hist),
              hist.shape[1], _p(ng["ngram"]), _p(ng["ban"]), _p(ng["ban_step"]), V, B, _stream())
    return ng["ban_step"]


def decode_advance_seen_ngram(next_ids, cur_ids, pos, slot, kv_end, seen, V, hist, n_hist, ng: dict):
    """decode_advance_seen and, in the same launch, ngram_ban on the advanced state: ng['ban_step'] is the ban bitmap of the next
    step (the token just chosen is the last element of the row's sequence)."""
    for t, n in ((next_ids, "next_ids"), (cur_ids, "cur_ids"), (pos, "pos"), (slot, "slot"), (kv_end, "kv_end"), (seen, "seen")):
        _chk(t, torch.int32, n)
    B = next_ids.numel()
    assert cur_ids.numel() == B and pos.numel() == B and slot.numel() == B and kv_end.numel() == B
    assert seen.numel() == B * bitmap_words(V)
    _ngram_args(ng, hist, n_hist, B, V)
    _lib.call("spider_decode_advance_seen_ngram_i32", _p(next_ids), _p(cur_ids), _p(pos), _p(slot), _p(kv_end), _p(hist), _p(n_hist),
              _p(seen), _p(ng["prompt_ids"]), _p(ng["n_prompt"]), ng["prompt_ids"].shape[1], _p(ng["ngram"]), _p(ng["ban"]),
              _p(ng["ban_step"]), V, hist.shape[1], B, _stream())


def token_bitmap_set(ids, bitmap, V):
    """bitmap [B, ceil(V/32)] |= the bits of ids [B, n] (int32); ids outside [0, V) are ignored."""
    _chk(ids, torch.int32, "ids"); _chk(bitmap, torch.int32, "bitmap")
    B = bitmap.shape[0]
    assert bitmap.dim() == 2 and bitmap.shape[1] == bitmap_words(V) and ids.numel() % B == 0
    n = ids.numel() // B
    if n:
        _lib.call("spider_token_bitmap_set_i32", _p(ids), _p(bitmap), B, n, V, _stream())


BEAM_SLICE = 4096       # tokens per block of beam_partial (beam_search.hip)
BEAM_MAX_C = 32


def beam_nslices(V: int) -> int:
    return (V + BEAM_SLICE - 1) // BEAM_SLICE


def beam_workspace(rows: int, V: int, C: int, device):
    """(ws_ms [rows, nslice, 2] f32, ws_val [rows, nslice, C] f32, ws_tok [rows, nslice, C] i32) of beam_partial / beam_select"""
    ns = beam_nslices(V)
    return (torch.empty(rows, ns, 2, dtype=torch.float32, device=device), torch.empty(rows, ns, C, dtype=torch.float32, device=device),
            torch.empty(rows, ns, C, dtype=torch.int32, device=device))


def beam_partial(logits, C, ws):
    """Per row of raw bf16 logits [rows, V] and slice of 4096 tokens: the online-softmax pair and the slice's C best (logit, token)."""
    _chk(logits, BF16, "logits")
    rows, V = logits.shape
    ns = beam_nslices(V)
    _chk(ws[0], torch.float32, "ws_ms"); _chk(ws[1], torch.float32, "ws_val"); _chk(ws[2], torch.int32, "ws_tok")
    assert ws[0].numel() == rows * ns * 2 and ws[1].numel() == rows * ns * C and ws[2].numel() == rows * ns * C
    _lib.call("spider_beam_partial_bf16", _p(logits), _p(ws[0]), _p(ws[1]), _p(ws[2]), rows, V, C, ns, _stream())


def beam_select(ws, run_scores, eos_ids, n_eos, n_hist, trace, src_beam, next_ids, V, C):
    """One beam-search selection per batch row from beam_partial's workspace: run_scores [B, K] f32 (updated in place), the C best
    continuations (score descending, then beam * V + token ascending) written to trace = (score f32, beam i32, token i32), each
    [cap, B, C], at step n_hist[b * K]; the first K non-EOS of them -> run_scores, src_beam [B, K], next_ids [B * K]."""
    _chk(run_scores, torch.float32, "run_scores"); _chk(eos_ids, torch.int32, "eos_ids"); _chk(n_eos, torch.int32, "n_eos")
    _chk(n_hist, torch.int32, "n_hist"); _chk(src_beam, torch.int32, "src_beam"); _chk(next_ids, torch.int32, "next_ids")
    _chk(trace[0], torch.float32, "trace_score"); _chk(trace[1], torch.int32, "trace_beam"); _chk(trace[2], torch.int32, "trace_tok")
    B, K = run_scores.shape
    ns = beam_nslices(V)
    if not (1 <= K <= 8 and K <= C <= BEAM_MAX_C and V >= C):
        raise ValueError(f"beam_select: needs K <= 8 and K <= C <= {BEAM_MAX_C} <= V (K={K}, C={C}, V={V})")
    assert ws[0].numel() == B * K * ns * 2 and ws[1].numel() == B * K * ns * C and ws[2].numel() == B * K * ns * C
    assert eos_ids.numel() >= 8 and n_eos.numel() == 1 and n_hist.numel() == B * K
    assert src_beam.numel() == B * K and next_ids.numel() == B * K
    cap = trace[0].shape[0]
    for t in trace:
        assert tuple(t.shape) == (cap, B, C)
    _lib.call("spider_beam_select_f32", _p(ws[0]), _p(ws[1]), _p(ws[2]), _p(run_scores), _p(eos_ids), _p(n_eos), _p(n_hist),
              _p(trace[0]), _p(trace[1]), _p(trace[2]), cap, _p(src_beam), _p(next_ids), B, K, V, C, ns, _stream())


def kv_row_gather(k_cache, v_cache, k_tmp, v_tmp, src_beam, kv_beg, kv_end, K):
    """Caches [layers, rows_alloc, n_kv, T, d]: row r <- old row (r // K) * K + src_beam[r] over slots [kv_beg[r], kv_end[r]) for
    the R = src_beam.numel() first rows, correct for any map (through k_tmp / v_tmp); K = R: src_beam is an absolute row map."""
    for t, n in ((k_cache, "k_cache"), (v_cache, "v_cache"), (k_tmp, "k_tmp"), (v_tmp, "v_tmp")):
        _chk(t, BF16, n)
        assert t.shape == k_cache.shape and t.dim() == 5
    _chk(src_beam, torch.int32, "src_beam"); _chk(kv_beg, torch.int32, "kv_beg"); _chk(kv_end, torch.int32, "kv_end")
    L, RA, n_kv, T, d = k_cache.shape
    R = src_beam.numel()
    assert kv_beg.numel() == R and kv_end.numel() == R and R <= RA and R % K == 0
    _lib.call("spider_kv_row_gather_bf16", _p(k_cache), _p(v_cache), _p(k_tmp), _p(v_tmp), _p(src_beam), _p(kv_beg), _p(kv_end),
              K, R, L, RA, n_kv, T, d, _stream())


SAMPLE_MAX_K = 64       # top_k limit of the sampling kernels (sample.hip) = stride of their candidate lists


def sample_state(rows: int, V: int, device) -> dict:
    """Parameters, workspace and outputs of sample_partial / sample_select for `rows` rows. The parameters (temperature, top_p
    float [1]; top_k, row0 int [1]; seed int32 [2] = the uint32 words (low, high)) are read by the kernels when they run."""
    ns = beam_nslices(V)
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)
    return dict(temperature=f32(1).fill_(1.0), top_p=f32(1).fill_(1.0), top_k=i32(1).fill_(1), seed=i32(2), row0=i32(1),
                ws_val=f32(rows, ns, SAMPLE_MAX_K), ws_tok=i32(rows, ns, SAMPLE_MAX_K), cand_tok=i32(rows, SAMPLE_MAX_K),
                cand_p=f32(rows, SAMPLE_MAX_K), n_keep=i32(rows), u=f32(rows))


def sample_set_params(sm: dict, temperature: float, top_k: int, top_p: float, seed: int, row0: int = 0):
    """this request's values into the state's parameter buffers (stream-ordered copies)"""
    if not (1 <= int(top_k) <= SAMPLE_MAX_K):
        raise ValueError(f"top_k has to be in [1, {SAMPLE_MAX_K}], but is {top_k}")
    sm["temperature"].fill_(float(temperature))
    sm["top_p"].fill_(float(top_p))
    sm["top_k"].fill_(int(top_k))
    sm["row0"].fill_(int(row0))
    words = [(int(seed) >> s) & 0xFFFFFFFF for s in (0, 32)]
    sm["seed"].copy_(torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32))


def sample_partial(logits, sm: dict, proc: Optional[dict] = None):
    """Per row of raw bf16 logits [rows, V] and slice of 4096 tokens: the slice's top_k best (value, token) of the PROCESSED logits
    (proc = the buffers of lm_head_argmax_proc; None: the raw logits) into sm['ws_val'] / sm['ws_tok']."""
    _chk(logits, BF16, "logits")
    rows, V = logits.shape
    ns = beam_nslices(V)
    _chk(sm["ws_val"], torch.float32, "ws_val"); _chk(sm["ws_tok"], torch.int32, "ws_tok"); _chk(sm["top_k"], torch.int32, "top_k")
    assert sm["ws_val"].numel() == rows * ns * SAMPLE_MAX_K and sm["ws_tok"].numel() == rows * ns * SAMPLE_MAX_K
    pargs = _proc_args(proc, rows, V) if proc is not None else (None,) * 7
    _lib.call("spider_sample_partial_bf16", _p(logits), *pargs, _p(sm["top_k"]), _p(sm["ws_val"]), _p(sm["ws_tok"]), rows, V, ns,
              _stream())


def sample_select(sm: dict, n_hist, next_ids, V: int):
    """One draw per row from sample_partial's workspace (csrc/sample.hip, `sample_token_host` of llm.py is its host restatement):
    next_ids [rows]; sm['cand_tok'] / sm['cand_p'] [rows, 64] = the ranked candidates and their unnormalised probabilities,
    sm['n_keep'] [rows] = the size of the nucleus, sm['u'] [rows] = the uniform of (seed, row0 + row, n_hist[row])."""
    _chk(n_hist, torch.int32, "n_hist"); _chk(next_ids, torch.int32, "next_ids")
    rows = next_ids.numel()
    ns = beam_nslices(V)
    for k, dt, n in (("temperature", torch.float32, 1), ("top_p", torch.float32, 1), ("top_k", torch.int32, 1), ("seed", torch.int32, 2),
                     ("row0", torch.int32, 1), ("ws_val", torch.float32, rows * ns * SAMPLE_MAX_K),
                     ("ws_tok", torch.int32, rows * ns * SAMPLE_MAX_K), ("cand_tok", torch.int32, rows * SAMPLE_MAX_K),
                     ("cand_p", torch.float32, rows * SAMPLE_MAX_K), ("n_keep", torch.int32, rows), ("u", torch.float32, rows)):
        _chk(sm[k], dt, k)
        assert sm[k].numel() == n, f"{k}: expected {n} entries"
    assert n_hist.numel() == rows
    _lib.call("spider_sample_select_f32", _p(sm["ws_val"]), _p(sm["ws_tok"]), _p(sm["temperature"]), _p(sm["top_p"]), _p(sm["top_k"]),
              _p(sm["seed"]), _p(sm["row0"]), _p(n_hist), _p(next_ids), _p(sm["cand_tok"]), _p(sm["cand_p"]), _p(sm["n_keep"]),
              _p(sm["u"]), rows, V, ns, _stream())


def _rows_ld(t, name):
    """(rows, ld, width) of a 2-D bf16 tensor of unit column stride: a contiguous [rows, ld] tensor or a column slice of one"""
    _chk(t, BF16, name, contiguous=False)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.stride(0) % 8:
        raise ValueError(f"{name}: expected a 2-D tensor [rows, width] with unit column stride and a row stride that is a multiple of 8 "
                         f"(pad the rows: the kernel reads whole 16-byte groups), got shape {tuple(t.shape)} strides {t.stride()}")
    return t.shape[0], t.stride(0), t.shape[1]


def logprob_rows(logits, targets, V: Optional[int] = None, logits_ref=None) -> dict:
    """Teacher-forced scoring of logits rows in one pass (csrc/logprob.hip; `llm.score_host` is the definition): replaces
    `logits.float()` -> `log_softmax` -> `gather` / ForCausalLMLoss per row. logits bf16 [rows, ld] with the first V columns valid
    (default: all; ld = the row stride, a multiple of 8 -- a column slice `buf[:, :V]` of a padded buffer works as well); targets
    int32 [rows], ids outside [0, V) (HF's ignore_index -100) score 0. Returns fp32 / int32 [rows] tensors: logprob, lse, argmax
    (lowest id among the maxima), entropy; with logits_ref (same layout rules, its own stride) also kl = KL(softmax(ref) ||
    softmax(logits)) and argmax_ref. The inputs are not written."""
    rows, ld, width = _rows_ld(logits, "logits")
    V = width if V is None else int(V)
    if not 1 <= V <= width:
        raise ValueError(f"V={V} must be in [1, {width}] (the width of logits)")
    _chk(targets, torch.int32, "targets")
    if targets.numel() != rows:
        raise ValueError(f"targets: expected {rows} entries, got {targets.numel()}")
    dv = logits.device
    f32 = lambda: torch.empty(rows, dtype=torch.float32, device=dv)
    i32 = lambda: torch.empty(rows, dtype=torch.int32, device=dv)
    out = dict(logprob=f32(), lse=f32(), argmax=i32(), entropy=f32())
    ld_ref = 0
    if logits_ref is not None:
        rrows, ld_ref, rwidth = _rows_ld(logits_ref, "logits_ref")
        if rrows != rows or rwidth < V:
            raise ValueError(f"logits_ref: expected [{rows}, >= {V}], got {tuple(logits_ref.shape)}")
        out["kl"], out["argmax_ref"] = f32(), i32()
    _lib.call("spider_logprob_rows_bf16", _p(logits), ld, _p(targets), _p(logits_ref), ld_ref, _p(out["logprob"]), _p(out["lse"]),
              _p(out["argmax"]), _p(out["entropy"]), _p(out.get("kl")), _p(out.get("argmax_ref")), rows, V, _stream())
    return out


GPTQ_MAX_GROUP_BLOCKS = 4     # MX blocks per launch of the sweep kernel (its LDS holds a [128, 128] fp32 block of U)
GPTQ_GROUP_BLOCKS = 4         # the driver's default group width
_GPTQ_DEVICE_LINALG = {}      # device index -> does this torch build factor fp64 matrices on the device


def gptq_factor_where(device) -> str:
    """"device" when this torch build runs cholesky / cholesky_inverse in fp64 on `device` (probed once on a 2 x 2 matrix), else
    "host": where `gptq_mxfp4` computes the factor U"""
    key = torch.device(device).index or 0
    if key not in _GPTQ_DEVICE_LINALG:
        try:
            a = torch.eye(2, dtype=torch.float64, device=device) * 2.0
            L = torch.linalg.cholesky(a)
            ok = bool(torch.isfinite(torch.linalg.cholesky(torch.cholesky_inverse(L), upper=True)).all())
        except RuntimeError:
            ok = False
        _GPTQ_DEVICE_LINALG[key] = ok
    return "device" if _GPTQ_DEVICE_LINALG[key] else "host"


def gptq_mxfp4_sweep(Wt, U, blocks, scales, Et, j0: int, nblocks: int):
    """One launch of csrc/gptq.hip: quantise the MX blocks of columns [j0, j0 + 32 nblocks) of every row of the K-major working
    copy Wt [K, N] fp32 with the group's diagonal block of U [K, K] fp32; writes blocks [N, K / 2], scales [N, K / 32] and the
    first 32 nblocks rows of Et [>= 32 nblocks, N] fp32 (E transposed). The columns behind the group are the caller's."""
    _chk(Wt, torch.float32, "Wt"); _chk(U, torch.float32, "U"); _chk(Et, torch.float32, "Et")
    _chk(blocks, torch.uint8, "blocks"); _chk(scales, torch.uint8, "scales")
    if Wt.dim() != 2 or Wt.shape[0] % 32 or Wt.shape[0] < 32 or Wt.shape[1] < 1:
        raise ValueError(f"Wt: expected a K-major working copy [K, N] with K % 32 == 0, got {tuple(Wt.shape)}")
    K, N = Wt.shape
    if tuple(U.shape) != (K, K) or tuple(blocks.shape) != (N, K // 2) or tuple(scales.shape) != (N, K // 32):
        raise ValueError(f"expected U [{K}, {K}], blocks [{N}, {K // 2}] and scales [{N}, {K // 32}], got {tuple(U.shape)}, "
                         f"{tuple(blocks.shape)} and {tuple(scales.shape)}")
    if not 1 <= nblocks <= GPTQ_MAX_GROUP_BLOCKS or j0 < 0 or j0 % 32 or j0 + 32 * nblocks > K:
        raise ValueError(f"group [{j0}, {j0} + 32 * {nblocks}) has to hold 1..{GPTQ_MAX_GROUP_BLOCKS} whole MX blocks within K = {K}")
    if Et.dim() != 2 or Et.shape[1] != N or Et.shape[0] < 32 * nblocks:
        raise ValueError(f"Et: expected [>= {32 * nblocks}, {N}], got {tuple(Et.shape)}")
    _lib.call("spider_gptq_mxfp4_sweep_f32", _p(Wt), _p(U), _p(blocks), _p(scales), _p(Et), N, K, j0, nblocks, _stream())


def gptq_mxfp4(W, H, damp: float = 0.01, group_blocks: Optional[int] = None, timing: Optional[dict] = None):
    """`llm.quantize_mxfp4_gptq(W, H, damp)` on the device: W [N, K] (any float dtype) and H [K, K] on the current HIP device ->
    (blocks uint8 [N, K / 2], scales uint8 [N, K / 32]) on the device, in `quantize_mxfp4`'s layout.
    Validation, dead inputs and damping are the definition's (`llm.gptq_prepare`, fp64, on the device). The factor U comes from
    `llm.gptq_factor` in fp64 -- on the device when this torch build provides the fp64 factorisations there, else on the host
    (`gptq_factor_where`) -- and is rounded to fp32 once. The sweep then runs in fp32: one launch of csrc/gptq.hip per group of
    `group_blocks` MX blocks (default GPTQ_GROUP_BLOCKS; a narrower tail group when K / 32 is no multiple), and between launches
    the columns behind the group take Wt[behind] -= U[group, behind]^T Et as one true-fp32 `addmm_` (TF32 off). The bytes equal
    the definition's except where fp32 rounding decides a tie (a weight within ~1e-6 relative of a rounding midpoint, an amax
    within that of a binade's 0.75); group_blocks changes the fp32 summation order of the compensation and nothing else.
    timing: a dict that receives the seconds spent in prepare / factor / sweep (each behind a device synchronisation)."""
    from .llm import gptq_factor, gptq_prepare
    import time
    if not isinstance(W, torch.Tensor) or not W.is_cuda:
        raise ValueError("W: expected a CUDA/HIP tensor (the HIP path has no CPU fallback)")
    if W.device.index != torch.cuda.current_device():
        raise ValueError(f"W: tensor lives on {W.device} but the current device is cuda:{torch.cuda.current_device()}")
    gb = GPTQ_GROUP_BLOCKS if group_blocks is None else int(group_blocks)
    if not 1 <= gb <= GPTQ_MAX_GROUP_BLOCKS:
        raise ValueError(f"group_blocks={group_blocks} has to be in 1..{GPTQ_MAX_GROUP_BLOCKS}")
    dv = W.device

    def lap(name, t0):
        if timing is not None:
            torch.cuda.synchronize(dv)
            timing[name] = timing.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()
    t = time.perf_counter()
    Wd, Hd = gptq_prepare(W, H, damp, who="gptq_mxfp4")
    t = lap("prepare", t)
    where = gptq_factor_where(dv)
    U = (gptq_factor(Hd, who="gptq_mxfp4") if where == "device" else gptq_factor(Hd.cpu(), who="gptq_mxfp4").to(dv)).float().contiguous()
    del Hd
    if timing is not None:
        timing["factor_where"] = where
    t = lap("factor", t)
    N, K = Wd.shape
    Wt = Wd.t().to(torch.float32).contiguous()          # the K-major working copy [K, N]
    del Wd
    blocks = torch.empty(N, K // 2, dtype=torch.uint8, device=dv)
    scales = torch.empty(N, K // 32, dtype=torch.uint8, device=dv)
    Et = torch.empty(32 * gb, N, dtype=torch.float32, device=dv)
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        for j0 in range(0, K, 32 * gb):
            nb = min(gb, (K - j0) // 32)
            j1 = j0 + 32 * nb
            gptq_mxfp4_sweep(Wt, U, blocks, scales, Et, j0, nb)
            if j1 < K:
                Wt[j1:].addmm_(U[j0:j1, j1:].t(), Et[:32 * nb], alpha=-1.0)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
    lap("sweep", t)
    return blocks, scales


def rope_kv_append(qkv, pos, slot, cos_sin, q_out, k_cache, v_cache, B, S, n_q, n_kv, d, mrope_section=None):
    """pos [B*S] int32, or [3, B*S] with mrope_section=(t, h, w) rotary pairs per component (Qwen2.5-Omni: 16, 24, 24)."""
    _chk(qkv, BF16, "qkv"); _chk(pos, torch.int32, "pos"); _chk(slot, torch.int32, "slot")
    _chk(cos_sin, torch.float32, "cos_sin"); _chk(q_out, BF16, "q_out")
    _chk(k_cache, BF16, "k_cache"); _chk(v_cache, BF16, "v_cache")
    T_max = k_cache.shape[2]
    sec_t, sec_h = (mrope_section[0], mrope_section[1]) if mrope_section is not None else (0, 0)
    assert qkv.numel() == B * S * (n_q + 2 * n_kv) * d and slot.numel() == B * S
    assert pos.numel() == (3 if mrope_section is not None else 1) * B * S
    assert mrope_section is None or sum(mrope_section) == d // 2
    assert k_cache.shape[0] >= B and k_cache.shape[1] == n_kv and k_cache.shape[3] == d
    assert cos_sin.shape[1] == d
    _lib.call("spider_rope_kv_append_mrope_bf16", _p(qkv), _p(pos), _p(slot), _p(cos_sin), _p(q_out), _p(k_cache),
              _p(v_cache), B, S, n_q, n_kv, d, T_max, sec_t, sec_h, _stream())
    return q_out


def attn_decode(q, k_cache, v_cache, kv_end, kv_beg=None, nsplit=1, ws=None, out=None, scale=None):
    _chk(q, BF16, "q"); _chk(k_cache, BF16, "k_cache"); _chk(v_cache, BF16, "v_cache"); _chk(kv_end, torch.int32, "kv_end")
    B, n_q, d = q.shape
    n_kv, T_max = k_cache.shape[1], k_cache.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if out is None:
        out = torch.empty(B, n_q * d, dtype=BF16, device=q.device)
    if nsplit > 1 and ws is None:
        ws = (torch.empty(B * n_q * nsplit * d, dtype=torch.float32, device=q.device),
              torch.empty(B * n_q * nsplit * 2, dtype=torch.float32, device=q.device))
    _lib.call("spider_attn_decode_bf16", _p(q), _p(k_cache), _p(v_cache), _p(kv_beg), _p(kv_end), _p(out),
              _p(ws[0]) if ws else None, _p(ws[1]) if ws else None, B, n_q, n_kv, d, T_max, float(scale), nsplit, _stream())
    return out


def attn_decode_fused(qkv, pos, cos_sin, k_cache, v_cache, kv_end, kv_beg, counters, n_q, nsplit, ws, out, scale=None):
    """RoPE + KV append + split-KV decode attention + combine in one launch. kv_end includes the current token."""
    _chk(qkv, BF16, "qkv"); _chk(pos, torch.int32, "pos"); _chk(cos_sin, torch.float32, "cos_sin")
    _chk(k_cache, BF16, "k_cache"); _chk(v_cache, BF16, "v_cache"); _chk(kv_end, torch.int32, "kv_end")
    _chk(counters, torch.int32, "counters"); _chk(out, BF16, "out")
    B = kv_end.numel()
    n_kv, T_max, d = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    assert qkv.numel() == B * (n_q + 2 * n_kv) * d and counters.numel() >= B * n_kv and cos_sin.shape[1] == d
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    _lib.call("spider_attn_decode_fused_bf16", _p(qkv), _p(pos), _p(cos_sin), _p(k_cache), _p(v_cache), _p(kv_beg), _p(kv_end),
              _p(out), _p(ws[0]) if ws else None, _p(ws[1]) if ws else None, _p(counters), B, n_q, n_kv, d, T_max,
              float(scale), nsplit, _stream())
    return out


# --------------------------------------------------------------------------- prompt-lookup decoding (csrc/spec_decode.hip)
SPEC_MAX_ROWS = 8       # rows per sequence of a verify step (the decode graph's 8 rows)
SPEC_MAX_NGRAM = 8      # largest max_matching_ngram_size the draft kernel compares


def attn_verify(q, k_cache, v_cache, kv_end, R, kv_beg=None, nsplit=1, ws=None, out=None, scale=None):
    """attn_decode for R consecutive query rows per sequence: q [B * R, n_q, d] (rotated by rope_kv_append with S = R, which also
    appended the R new K / V rows), kv_end / kv_beg [B]; row r of sequence b sees the slots kv_beg[b] <= j < kv_end[b] + r.
    Returns out [B * R, n_q * d]."""
    _chk(q, BF16, "q"); _chk(k_cache, BF16, "k_cache"); _chk(v_cache, BF16, "v_cache"); _chk(kv_end, torch.int32, "kv_end")
    rows, n_q, d = q.shape
    B = kv_end.numel()
    n_kv, T_max = k_cache.shape[1], k_cache.shape[2]
    if not (isinstance(R, int) and 1 <= R <= SPEC_MAX_ROWS) or rows != B * R:
        raise ValueError(f"attn_verify: R has to be 1 ... {SPEC_MAX_ROWS} with q [B * R, n_q, d]; got R={R}, {rows} rows, B={B}")
    assert k_cache.shape[0] >= B and v_cache.shape == k_cache.shape and k_cache.shape[3] == d
    if kv_beg is not None:
        _chk(kv_beg, torch.int32, "kv_beg")
        assert kv_beg.numel() == B
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if out is None:
        out = torch.empty(rows, n_q * d, dtype=BF16, device=q.device)
    else:
        _chk(out, BF16, "out")
        assert out.numel() == rows * n_q * d
    if nsplit > 1:
        if ws is None:
            ws = (torch.empty(rows * n_q * nsplit * d, dtype=torch.float32, device=q.device),
                  torch.empty(rows * n_q * nsplit * 2, dtype=torch.float32, device=q.device))
        assert ws[0].numel() >= rows * n_q * nsplit * d and ws[1].numel() >= rows * n_q * nsplit * 2, "attn_verify: workspace too small"
    _lib.call("spider_attn_verify_bf16", _p(q), _p(k_cache), _p(v_cache), _p(kv_beg), _p(kv_end), _p(out),
              _p(ws[0]) if ws else None, _p(ws[1]) if ws else None, B, R, n_q, n_kv, d, T_max, float(scale), nsplit, _stream())
    return out


def _spec_args(sp: dict, hist, n_hist, advance: bool):
    """The buffers of a prompt-lookup step: sp = dict(prompt_ids int32 [B, pcap], n_prompt [B], ngram [1], k_draft [1], ids / pos /
    slot [B * R], n_draft [B]; with `advance` also lm_out [B * R], kv_end [B] and counters int64 [B, 3]); hist int32 [B, cap],
    n_hist [B]. Returns (B, R)."""
    for k in ("prompt_ids", "n_prompt", "ngram", "k_draft", "ids", "pos", "slot", "n_draft") + (("lm_out", "kv_end") if advance else ()):
        _chk(sp[k], torch.int32, k)
    _chk(hist, torch.int32, "hist"); _chk(n_hist, torch.int32, "n_hist")
    B = n_hist.numel()
    assert hist.dim() == 2 and hist.shape[0] == B and hist.shape[1] > 0
    assert sp["prompt_ids"].dim() == 2 and sp["prompt_ids"].shape[0] == B and sp["prompt_ids"].shape[1] > 0
    assert sp["n_prompt"].numel() == B and sp["n_draft"].numel() == B and sp["ngram"].numel() >= 1 and sp["k_draft"].numel() >= 1
    rows = sp["ids"].numel()
    R = rows // B
    if rows != B * R or not 1 <= R <= SPEC_MAX_ROWS:
        raise ValueError(f"prompt lookup: ids has to hold 1 ... {SPEC_MAX_ROWS} rows for each of the {B} sequences, got {rows}")
    assert sp["pos"].numel() == rows and sp["slot"].numel() == rows
    if advance:
        _chk(sp["counters"], torch.int64, "counters")
        assert sp["lm_out"].numel() == rows and sp["kv_end"].numel() == B and sp["counters"].numel() == B * 3
    return B, R


def prompt_lookup_draft(sp: dict, hist, n_hist):
    """Draft the rows 1 ... R - 1 of a verify step from the sequence prompt_ids[b, :n_prompt[b]] ++ hist[b, :n_hist[b]]
    (`llm.prompt_lookup_draft_host` is the definition; buffers: `_spec_args`); row 0 of ids / pos / slot is the caller's."""
    B, R = _spec_args(sp, hist, n_hist, False)
    _lib.call("spider_prompt_lookup_draft_i32", _p(sp["prompt_ids"]), _p(sp["n_prompt"]), sp["prompt_ids"].shape[1], _p(hist),
              _p(n_hist), hist.shape[1], _p(sp["ngram"]), _p(sp["k_draft"]), _p(sp["ids"]), _p(sp["pos"]), _p(sp["slot"]),
              _p(sp["n_draft"]), R, B, _stream())


def spec_advance_draft(sp: dict, hist, n_hist):
    """Close a verify step (accept the drafts sp['lm_out'] agrees with -- `llm.spec_accept_host` --, append them to hist, advance
    the cursors, count) and draft the next one, in one launch."""
    B, R = _spec_args(sp, hist, n_hist, True)
    _lib.call("spider_spec_advance_draft_i32", _p(sp["lm_out"]), _p(sp["ids"]), _p(sp["pos"]), _p(sp["slot"]), _p(sp["kv_end"]),
              _p(sp["n_draft"]), _p(hist), _p(n_hist), hist.shape[1], _p(sp["prompt_ids"]), _p(sp["n_prompt"]),
              sp["prompt_ids"].shape[1], _p(sp["ngram"]), _p(sp["k_draft"]), _p(sp["counters"]), R, B, _stream())


# --------------------------------------------------------------------------- assisted decoding (csrc/spec_assist.hip)
def _assist_rows(ids, pos, slot, what: str, B: int):
    """rows per sequence of three int32 cursor buffers [B * R]"""
    _chk(ids, torch.int32, what + " ids"); _chk(pos, torch.int32, what + " pos"); _chk(slot, torch.int32, what + " slot")
    rows = ids.numel()
    R = rows // B
    if rows != B * R or not 1 <= R <= SPEC_MAX_ROWS or pos.numel() != rows or slot.numel() != rows:
        raise ValueError(f"assisted decoding: the {what} ids / pos / slot have to hold 1 ... {SPEC_MAX_ROWS} rows for each of the {B} "
                         f"sequences, got {rows} / {pos.numel()} / {slot.numel()}")
    return R


def spec_assist_push(src: dict, src_row: int, tgt: dict, j: int, dst: dict, draft_vocab: int):
    """Behind a draft step: the arg-max of row `src_row` of src = dict(out, pos, slot [B * Rs]) is draft number j. It becomes row j of
    the verify step tgt = dict(ids, pos, slot [B * R]) one position and slot behind its source row, and the draft engine's next single
    row dst = dict(ids, pos, slot, kv_end [B]) with ids at or above draft_vocab replaced by 0 (`llm.assisted_round_host` is the
    definition). dst may hold src's own buffers."""
    _chk(dst["kv_end"], torch.int32, "dst kv_end")
    B = dst["kv_end"].numel()
    Rs = _assist_rows(src["out"], src["pos"], src["slot"], "source", B)
    R = _assist_rows(tgt["ids"], tgt["pos"], tgt["slot"], "target", B)
    if _assist_rows(dst["ids"], dst["pos"], dst["slot"], "draft", B) != 1:
        raise ValueError("spec_assist_push: the draft's next step has one row per sequence")
    if not (0 <= src_row < Rs and 1 <= j < R):
        raise ValueError(f"spec_assist_push: source row {src_row} of {Rs}, draft row {j} of {R}")
    _lib.call("spider_spec_assist_push_i32", _p(src["out"]), _p(src["pos"]), _p(src["slot"]), Rs, int(src_row), _p(tgt["ids"]),
              _p(tgt["pos"]), _p(tgt["slot"]), R, int(j), _p(dst["ids"]), _p(dst["pos"]), _p(dst["slot"]), _p(dst["kv_end"]),
              int(draft_vocab), B, _stream())


def spec_assist_advance(sp: dict, hist, n_hist, catch_up: dict, draft_vocab: int):
    """Close the verify step of an assisted round: sp = dict(lm_out, ids, pos, slot [B * R], kv_end, n_draft [B], counters int64
    [B, 3]) as for spec_advance_draft (accept by `llm.spec_accept_host`, append to hist, advance row 0, count), and write the draft
    engine's next catch-up rows catch_up = dict(ids, pos, slot [B * 2], kv_end [B]) (`llm.assisted_round_host`)."""
    for k in ("lm_out", "kv_end", "n_draft"):
        _chk(sp[k], torch.int32, k)
    _chk(hist, torch.int32, "hist"); _chk(n_hist, torch.int32, "n_hist"); _chk(sp["counters"], torch.int64, "counters")
    _chk(catch_up["kv_end"], torch.int32, "catch_up kv_end")
    B = n_hist.numel()
    R = _assist_rows(sp["ids"], sp["pos"], sp["slot"], "target", B)
    if R < 2 or _assist_rows(catch_up["ids"], catch_up["pos"], catch_up["slot"], "catch-up", B) != 2:
        raise ValueError("spec_assist_advance: the verify step has 2 ... 8 rows per sequence, the draft's catch-up step two")
    assert hist.dim() == 2 and hist.shape[0] == B and hist.shape[1] > 0
    assert sp["lm_out"].numel() == B * R and sp["kv_end"].numel() == B and sp["n_draft"].numel() == B and sp["counters"].numel() == B * 3
    assert catch_up["kv_end"].numel() == B
    _lib.call("spider_spec_assist_advance_i32", _p(sp["lm_out"]), _p(sp["ids"]), _p(sp["pos"]), _p(sp["slot"]), _p(sp["kv_end"]),
              _p(sp["n_draft"]), _p(hist), _p(n_hist), hist.shape[1], _p(sp["counters"]), R, _p(catch_up["ids"]), _p(catch_up["pos"]),
              _p(catch_up["slot"]), _p(catch_up["kv_end"]), int(draft_vocab), B, _stream())


# --------------------------------------------------------------------------- GEMM / conv / attention
def gemm(A, W, bias=None, res=None, rowbias=None, rows_per_group=0, act=None, out_scale=1.0, out=None, out_f32=False,
         res32=None, want32=False):
    """C = act(A @ W^T + bias + rowbias[row // rows_per_group]) (+ res) * out_scale.  A [..., K], W [N, K].
    fp32 residual stream: res32 (fp32, shape of C) replaces `res` and is added to the unrounded result; want32=True returns
    (C, C32) with C32 the fp32 value that C rounds."""
    dt, sfx = _h16(A)
    _chk(A, dt, "A"); _chk(W, dt, "W")
    N, K = W.shape
    assert A.shape[-1] == K, f"gemm: A[..., {A.shape[-1]}] vs W[{N},{K}]"
    M = A.numel() // K
    # GEGLU epilogue: W = [value rows | gate rows]; SwiGLU epilogue (LlamaMLP): W = [gate rows | up rows]; the output has N/2 columns
    n_out = N // 2 if act in GLU_ACTS else N
    if out is None:
        out = torch.empty(*A.shape[:-1], n_out, dtype=torch.float32 if out_f32 else dt, device=A.device)
    c16, c32 = (None, out) if out.dtype == torch.float32 else (out, None)
    wt = _tiled(W, M)
    o32 = torch.empty(out.shape, dtype=torch.float32, device=A.device) if want32 else None
    if res32 is not None:
        _chk(res32, torch.float32, "res32")
    _lib.call(f"spider_gemm_{sfx}", _p(A), _p(W if wt is None else wt), _p(c16), _p(c32), _p(bias), _p(res), _p(rowbias), rows_per_group,
              M, N, K, K, n_out, ACT[act], float(out_scale), int(wt is not None), _p(res32), _p(o32), _p(_workspace(A.device)), WS_BYTES,
              _stream())
    return (out, o32) if want32 else out


def fold_layernorm(W, gamma, beta, bias=None):
    """One-time parameter folding for gemm_ln (done when an engine loads its weights, like the OIHW -> OHWI repack):
    LayerNorm(x) @ W^T + bias == rstd * (x @ Wf^T - mean * colsum) + colbias with
    Wf = W * gamma (bf16), colsum = Wf.sum(1) (fp32, of the ROUNDED Wf so that the mean term cancels exactly),
    colbias = W @ beta + bias (fp32). Returns (Wf, colsum, colbias)."""
    W32 = W.float()
    Wf = (W32 * gamma.float()[None, :]).to(W.dtype).contiguous()
    colsum = Wf.float().sum(1).contiguous()
    colbias = (W32 @ beta.float())
    if bias is not None:
        colbias = colbias + bias.float()
    return Wf, colsum, colbias.contiguous()


def gemm_ln(A, Wf, colsum, colbias, res=None, act=None, eps=1e-5, out=None):
    """LayerNorm(A) @ W^T + bias (+ res) in one launch; (Wf, colsum, colbias) = fold_layernorm(W, gamma, beta, bias).
    act: None or "geglu". A [..., K] bf16 contiguous rows."""
    dt, sfx = _h16(A)
    _chk(A, dt, "A"); _chk(Wf, dt, "Wf"); _chk(colsum, torch.float32, "colsum"); _chk(colbias, torch.float32, "colbias")
    N, K = Wf.shape
    assert A.shape[-1] == K and colsum.numel() == N and colbias.numel() == N, "gemm_ln: shape mismatch"
    assert act in (None, "geglu", "geglu_exact"), "gemm_ln: only the plain and GEGLU epilogues exist"
    M = A.numel() // K
    n_out = N // 2 if act in GLU_ACTS else N
    if out is None:
        out = torch.empty(*A.shape[:-1], n_out, dtype=dt, device=A.device)
    if res is not None:
        _chk(res, dt, "res")
    wt = _tiled(Wf, M)
    _lib.call(f"spider_gemm_ln_{sfx}", _p(A), _p(Wf if wt is None else wt), _p(out), _p(colsum), _p(colbias), _p(res), M, N, K, n_out,
              ACT[act], float(eps), int(wt is not None), _p(_workspace(A.device)), WS_BYTES, _stream())
    return out


XATTN_LP = 80     # keys per head in the folded cross-attention operands (77 text tokens padded to a multiple of 16)


def xattn_fused(x, mq_fm, mo_fm, colsum, colbias, bias_o, B2, heads, n_keys, eps=1e-5, out=None, x32=None, want32=False):
    """x + to_out(softmax(to_q(LayerNorm(x)) K^T / sqrt(d)) V) with the prompt's K / V folded into mq_fm / mo_fm (see
    include/spider_hip.h, spider_xattn_fused_bf16, and UNetEngine.prepare). x [B2, n_tok, C] or [B2 * n_tok, C] bf16."""
    dt, sfx = _h16(x)
    _chk(x, dt, "x"); _chk(mq_fm, dt, "mq_fm"); _chk(mo_fm, dt, "mo_fm")
    _chk(colsum, torch.float32, "colsum"); _chk(colbias, torch.float32, "colbias"); _chk(bias_o, dt, "bias_o")
    C = x.shape[-1]
    n_tok = x.numel() // (C * B2)
    if out is None:
        out = torch.empty_like(x)
    o32 = torch.empty(out.shape, dtype=torch.float32, device=x.device) if want32 else None
    if x32 is not None:
        _chk(x32, torch.float32, "x32")
    _lib.call(f"spider_xattn_fused_{sfx}", _p(x), _p(mq_fm), _p(mo_fm), _p(colsum), _p(colbias), _p(bias_o), _p(out), B2, n_tok, C,
              heads, n_keys, float(eps), _p(x32), _p(o32), _stream())
    return (out, o32) if want32 else out


def conv2d(x, w, bias=None, res=None, rowbias=None, stride=1, pad=None, ups=False, out_scale=1.0, out=None, res32=None, want32=False,
           gn_groups=None):
    """NHWC conv. x [B,H,W,Cin] bf16, w [Cout,ks,ks,Cin] bf16 -> [B,Ho,Wo,Cout]. res32 / want32: fp32 residual stream as in gemm().
    gn_groups: see conv_ex (GroupNorm partial statistics of the output as the last element of the result)."""
    if gn_groups and not ups:
        ks_ = w.shape[1]
        pd = ks_ // 2 if pad is None else pad
        return conv_ex(x, w, bias=bias, res=res, rowbias=rowbias, stride=stride, pad=(pd, pd), out_scale=out_scale, out=out,
                       res32=res32, want32=want32, gn_groups=gn_groups)
    dt, sfx = _h16(x)
    _chk(x, dt, "x"); _chk(w, dt, "w")
    B, H, Wd, Cin = x.shape
    Cout, ks = w.shape[0], w.shape[1]
    if pad is None:
        pad = ks // 2
    if ks == 3 and stride == 1 and pad == 1 and WS_ENABLE and B * H * Wd * (4 if ups else 1) <= WS_MAX_M and getattr(w, "_spider_weight", False):
        # weight-bound maps (<= 512 output pixels): the general entry point picks the weight-stationary streaming kernel
        return conv_ex(x, w, bias=bias, res=res, rowbias=rowbias, stride=1, pad=(1, 1), up_size=(2 * H, 2 * Wd) if ups else None,
                       out_scale=out_scale, out=out, res32=res32, want32=want32)
    Hs, Ws = (H * 2, Wd * 2) if ups else (H, Wd)
    Ho, Wo = (Hs + 2 * pad - ks) // stride + 1, (Ws + 2 * pad - ks) // stride + 1
    if out is None:
        out = torch.empty(B, Ho, Wo, Cout, dtype=dt, device=x.device)
    wt = _tiled(w, B * Ho * Wo)
    o32 = torch.empty(out.shape, dtype=torch.float32, device=x.device) if want32 else None
    if res32 is not None:
        _chk(res32, torch.float32, "res32")
    _lib.call(f"spider_conv2d_nhwc_{sfx}", _p(x), _p(w if wt is None else wt), _p(out), _p(bias), _p(res), _p(rowbias), B, H, Wd, Cin, Cout,
              ks, stride, pad, int(ups), float(out_scale), int(wt is not None), _p(res32), _p(o32), _p(_workspace(x.device)), WS_BYTES,
              _stream())
    return (out, o32) if want32 else out


class GnPartial:
    """GroupNorm partial statistics of a [B, HW, C] tensor: t [B, nchunk, G, 2] fp32 = (sum, sum of squares) per pixel chunk and group
    (include/spider_hip.h: spider_conv_nhwc_gn). Produced by `conv_ex(..., gn_groups=G)` for its own output, consumed by
    `groupnorm(..., partial=...)` and `gemm_gn_in`."""
    __slots__ = ("t", "nchunk", "groups")

    def __init__(self, t, nchunk, groups):
        self.t, self.nchunk, self.groups = t, nchunk, groups


def groupnorm_stats(x, groups: int, nchunk: int) -> GnPartial:
    """pass 1 of GroupNorm alone (x [B, ..., C] NHWC) with `nchunk` pixel chunks per image"""
    dt, sfx = _h16(x)
    _chk(x, dt, "x")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    part = torch.empty(B, nchunk, groups, 2, dtype=torch.float32, device=x.device)
    _lib.call(f"spider_groupnorm_stats_nhwc_{sfx}", _p(x), _p(part), B, HW, C, groups, nchunk, _stream())
    return GnPartial(part, nchunk, groups)


def conv_ex(x, w, bias=None, res=None, rowbias=None, stride=1, pad=(0, 0), dil=1, up_size=None, act=None, act_param=0.0,
            out_scale=1.0, out=None, res32=None, want32=False, gn_groups=None):
    """General NHWC conv. x [B,H,W,Cin] bf16, w [Cout,kh,kw,Cin] bf16 -> [B,Ho,Wo,Cout]. up_size=(uh,uw): x is read through
    a nearest upsample to that size (each in (in, 2*in]) before the conv. res32 / want32: fp32 residual stream as in gemm().
    gn_groups=G: also return the GroupNorm partial statistics of the OUTPUT as the last element of the result (a GnPartial):
    written by the conv's own epilogue / split-K reduce where that kernel can, else by one statistics pass -- either way the
    consumer GroupNorm needs none of its own. None is returned in their place when the map is not a multiple of the chunk rows."""
    dt, sfx = _h16(x)
    _chk(x, dt, "x"); _chk(w, dt, "w")
    B, H, Wd, Cin = x.shape
    Cout, kh, kw = w.shape[0], w.shape[1], w.shape[2]
    assert w.shape[3] == Cin, f"conv: x has {Cin} channels, w expects {w.shape[3]}"
    Hs, Ws = up_size if up_size is not None else (H, Wd)
    Ho = (Hs + 2 * pad[0] - dil * (kh - 1) - 1) // stride + 1
    Wo = (Ws + 2 * pad[1] - dil * (kw - 1) - 1) // stride + 1
    if out is None:
        out = torch.empty(B, Ho, Wo, Cout, dtype=dt, device=x.device)
    uh, uw = up_size if up_size is not None else (0, 0)
    wt, wmode = None, 0
    if _ws_eligible(B, H, Wd, Cin, Cout, kh, kw, stride, pad, dil, up_size, Ho, Wo, act):
        wt = _wsfm(w)
        wmode = 2 if wt is not None else 0
    if wt is None:
        wt = _tiled(w, B * Ho * Wo)
        wmode = int(wt is not None)
    o32 = torch.empty(out.shape, dtype=torch.float32, device=x.device) if want32 else None
    if res32 is not None:
        _chk(res32, torch.float32, "res32")
    args = (_p(x), _p(w if wt is None else wt), _p(out), _p(bias), _p(res), _p(rowbias), B, H, Wd, Cin,
            Cout, kh, kw, stride, pad[0], pad[1], dil, uh, uw, ACT[act], float(act_param), float(out_scale), wmode,
            _p(res32), _p(o32), _p(_workspace(x.device)), WS_BYTES, _stream())
    part = None
    HWo = Ho * Wo
    # (every block of the consuming GroupNorm reduces the partials of its image: beyond ~256 chunks -- the UNet3D's temporal norms
    # over 16 frames x 2880 pixels would be 720 -- that prologue costs more than the statistics pass it replaces: measured +0.8 %)
    # (the streaming conv combines its K splits inside the launch and leaves no statistics: on its small maps the consumer's
    # one-launch GroupNorm is cheaper than a reduce kernel that would make them)
    if gn_groups and GN_PRODUCER and HWo % 16 == 0 and HWo <= 16384 and not (wmode == 2 and WS_INLAUNCH):
        buf = torch.empty(B * (HWo // 16) * gn_groups * 2, dtype=torch.float32, device=x.device)
        produced = C.c_int(0)
        _lib.call(f"spider_conv_nhwc_gn_{sfx}", *args, _p(buf), int(gn_groups), C.byref(produced))
        cr = produced.value          # rows per chunk the producing kernel used (64: conv epilogue, 16: split-K reduce), 0: none
        if not cr:                   # this shape's kernel cannot write them: one statistics pass (what the GroupNorm would have run)
            cr = 64 if HWo % 64 == 0 and HWo >= 1024 else 16
            _lib.call(f"spider_groupnorm_stats_nhwc_{sfx}", _p(out), _p(buf), B, HWo, Cout, int(gn_groups), HWo // cr, _stream())
        nchunk = HWo // cr
        part = GnPartial(buf[:B * nchunk * gn_groups * 2].view(B, nchunk, gn_groups, 2), nchunk, gn_groups)
    else:
        _lib.call(f"spider_conv_nhwc_ex_{sfx}", *args)
    if gn_groups:         # part is None where no statistics were made: the consumer runs its own pass
        return (out, o32, part) if want32 else (out, part)
    return (out, o32) if want32 else out


GN_PRODUCER = _os.environ.get("SPIDER_GN_PRODUCER", "1") != "0"     # tuning aid: 0 = every GroupNorm runs its own statistics pass


def gemm_gn_in(A, W, part: GnPartial, gamma, beta, HW: int, eps: float, bias=None, want32=False):
    """C = GroupNorm(A) @ W^T + bias with the normalisation applied inside the GEMM (Transformer2DModel.norm + proj_in in one launch).
    A [B, HW, K] un-normalised, part = its partial statistics."""
    dt, sfx = _h16(A)
    _chk(A, dt, "A"); _chk(W, dt, "W")
    N, K = W.shape
    M = A.numel() // K
    out = torch.empty(*A.shape[:-1], N, dtype=dt, device=A.device)
    o32 = torch.empty(out.shape, dtype=torch.float32, device=A.device) if want32 else None
    wt = _tiled(W, M)
    _lib.call(f"spider_gemm_gn_in_{sfx}", _p(A), _p(W if wt is None else wt), _p(out), _p(bias), M, N, K, N, int(wt is not None),
              _p(part.t), part.nchunk, _p(gamma), _p(beta), part.groups, float(eps), HW, _p(o32), _stream())
    return (out, o32) if want32 else out


def conv1d(x, w, bias=None, res=None, pad=0, dil=1, act=None, act_param=0.0, out=None):
    """x [B,L,Cin] bf16, w [Cout,k,Cin] bf16 (nn.Conv1d weight permuted to O,K,I) -> [B,Lo,Cout]."""
    B, L, Cin = x.shape
    y = conv_ex(x.view(B, 1, L, Cin), w.view(w.shape[0], 1, w.shape[1], Cin), bias=bias,
                res=None if res is None else res.view(B, 1, res.shape[1], res.shape[2]), pad=(0, pad), dil=dil, act=act,
                act_param=act_param, out=None if out is None else out.view(B, 1, out.shape[1], out.shape[2]))
    return y.view(B, y.shape[2], y.shape[3])


def conv_transpose1d(x, w_taps, bias, k: int, stride: int, pad: int):
    """nn.ConvTranspose1d. x [B,L,Cin] bf16; w_taps [k*Cout, Cin] bf16 with row j*Cout+o = weight[:, o, j]
    -> [B, (L-1)*stride - 2*pad + k, Cout]. Per-tap GEMM (fp32) + overlap-add."""
    B, L, Cin = x.shape
    Cout = w_taps.shape[0] // k
    cols = gemm(x, w_taps, out_f32=True)                      # [B, L, k*Cout] fp32
    dt, sfx = _h16(x)
    out = torch.empty(B, (L - 1) * stride - 2 * pad + k, Cout, dtype=dt, device=x.device)
    _lib.call(f"spider_col2im1d_f32_{sfx}", _p(cols), _p(bias), _p(out), B, L, k, stride, pad, Cout, _stream())
    return out


def attention(q, k, v, n_heads, n_kv_heads=None, scale=None, causal=False, kv_off=None, kv_beg=None,
              keep_bits=None, blk=0, q_off=0, out=None):
    """q [B,Lq,Hq*d], k/v [B,Lk,Hkv*d] (last dim contiguous; batch/row strides free) -> [B,Lq,Hq*d]."""
    dt, sfx = _h16(q)
    _chk(q, dt, "q", False); _chk(k, dt, "k", False); _chk(v, dt, "v", False)
    B, Lq, Cq = q.shape
    Lk = k.shape[1]
    Hq = n_heads
    Hkv = n_kv_heads or n_heads
    d = Cq // Hq
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if kv_off is None:
        kv_off = Lk - Lq
    if out is None:
        out = torch.empty(B, Lq, Cq, dtype=dt, device=q.device)
    _lib.call(f"spider_attn_{sfx}", _p(q), _p(k), _p(v), _p(out),
              q.stride(0), d, q.stride(1), k.stride(0), d, k.stride(1), v.stride(0), d, v.stride(1),
              out.stride(0), d, out.stride(1),
              B, Hq, Hkv, Lq, Lk, d, float(scale), int(causal), int(kv_off), _p(kv_beg), _p(keep_bits), blk, q_off,
              _stream())
    return out


def story_key_lists(keep_bits, n_keys: int, N: int, img0: int, n_lists: int, q_img0: int):
    """Visible-key lists of the consistent self-attention: list l (query image img0 + l) = keys whose keep bit is set or that lie in
    the image's own block of N tokens. Returns (key_idx int32 [n_lists * stride], tiles int32 [n_lists * ceil(N/128), 4])."""
    _chk(keep_bits, torch.int64, "keep_bits")
    assert keep_bits.numel() * 64 >= n_keys
    stride = (n_keys + 63) // 64 * 64
    key_idx = torch.empty(n_lists * stride, dtype=torch.int32, device=keep_bits.device)
    tiles = torch.empty(n_lists * ((N + 127) // 128), 4, dtype=torch.int32, device=keep_bits.device)
    _lib.call("spider_story_key_lists_i32", _p(keep_bits), n_keys, N, img0, n_lists, q_img0, stride, _p(key_idx), _p(tiles), _stream())
    return key_idx, tiles


def attention_keylist(q, k, v, n_heads, key_idx, tiles, scale=None, out=None):
    """Consistent self-attention over visible-key lists (story_key_lists): q [B,Lq,H*64], k / v [B,Lk,H*64]."""
    dt, sfx = _h16(q)
    _chk(q, dt, "q", False); _chk(k, dt, "k", False); _chk(v, dt, "v", False)
    _chk(key_idx, torch.int32, "key_idx"); _chk(tiles, torch.int32, "tiles")
    B, Lq, Cq = q.shape
    Lk, d = k.shape[1], Cq // n_heads
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1 and tiles.dim() == 2 and tiles.shape[1] == 4
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if out is None:
        out = torch.empty(B, Lq, Cq, dtype=dt, device=q.device)
    _lib.call(f"spider_attn_keylist_{sfx}", _p(q), _p(k), _p(v), _p(out),
              q.stride(0), d, q.stride(1), k.stride(0), d, k.stride(1), v.stride(0), d, v.stride(1),
              out.stride(0), d, out.stride(1), B, n_heads, n_heads, Lq, Lk, d, float(scale),
              _p(key_idx), key_idx.numel(), _p(tiles), tiles.shape[0], _stream())
    return out


def varlen_tiles(cu_seqlens, device) -> torch.Tensor:
    """cu_seqlens (python ints / tensor, [n_seg + 1]) -> int32 [n_tiles, 4] records {q_start, q_len <= 128, k_start, k_len}
    for attention_varlen: every segment is cut into query tiles of at most 128 rows that all see the whole segment."""
    cu = [int(v) for v in (cu_seqlens.tolist() if hasattr(cu_seqlens, "tolist") else cu_seqlens)]
    rec = []
    for a, b in zip(cu[:-1], cu[1:]):
        if b < a:
            raise ValueError("cu_seqlens must be non-decreasing")
        for q0 in range(a, b, 128):
            rec.append((q0, min(128, b - q0), a, b - a))
    if not rec:
        raise ValueError("cu_seqlens describes no rows")
    return torch.tensor(rec, dtype=torch.int32, device=device)


def attention_varlen(q, k, v, n_heads, tiles, n_kv_heads=None, scale=None, out=None):
    """Packed segments: q [T,Hq*d], k/v [T,Hkv*d] (last dim contiguous, row stride free); tiles from varlen_tiles()."""
    dt, sfx = _h16(q)
    _chk(q, dt, "q", False); _chk(k, dt, "k", False); _chk(v, dt, "v", False)
    T, Cq = q.shape
    Hq, Hkv = n_heads, (n_kv_heads or n_heads)
    d = Cq // Hq
    assert q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1 and k.shape[0] == T and v.shape[0] == T
    assert tiles.dtype == torch.int32 and tiles.dim() == 2 and tiles.shape[1] == 4 and tiles.is_contiguous()
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if out is None:
        out = torch.empty(T, Cq, dtype=dt, device=q.device)
    _lib.call(f"spider_attn_varlen_{sfx}", _p(q), _p(k), _p(v), _p(out), q.stride(0), k.stride(0), v.stride(0), out.stride(0),
              T, Hq, Hkv, d, float(scale), _p(tiles), tiles.shape[0], _stream())
    return out


def rope_rows_(x, cos_sin, n_heads):
    """In-place half-rotation RoPE. x [T, n_heads*d] bf16 view (row stride free), cos_sin [T, d] fp32 = [cos | sin]."""
    _chk(x, BF16, "x", False); _chk(cos_sin, torch.float32, "cos_sin")
    T, Cx = x.shape
    d = Cx // n_heads
    assert x.stride(1) == 1 and tuple(cos_sin.shape) == (T, d)
    _lib.call("spider_rope_rows_bf16", _p(x), _p(cos_sin), x.stride(0), T, n_heads, d, _stream())
    return x


def attention_cache(q, k_cache, v_cache, Lk, scale=None, causal=True, kv_off=None, kv_beg=None, out=None):
    """Prefill attention against the KV cache. q [B,S,n_q,d]; caches [B,n_kv,T_max,d]; keys [0, Lk)."""
    dt, sfx = _h16(q)
    _chk(q, dt, "q"); _chk(k_cache, dt, "k_cache"); _chk(v_cache, dt, "v_cache")
    B, S, n_q, d = q.shape
    n_kv, T_max = k_cache.shape[1], k_cache.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if kv_off is None:
        kv_off = Lk - S
    if out is None:
        out = torch.empty(B, S, n_q * d, dtype=dt, device=q.device)
    _lib.call(f"spider_attn_{sfx}", _p(q), _p(k_cache), _p(v_cache), _p(out),
              S * n_q * d, d, n_q * d, n_kv * T_max * d, T_max * d, d, n_kv * T_max * d, T_max * d, d,
              S * n_q * d, d, n_q * d,
              B, n_q, n_kv, S, Lk, d, float(scale), int(causal), int(kv_off), _p(kv_beg), None, 0, 0, _stream())
    return out


# --------------------------------------------------------------------------- "precise" fp32-operand forms (ABI v4)
# The A operand (or the NHWC image) is an fp32 tensor -- the master of the residual stream, or a GroupNorm output kept in fp32 -- and
# is split into hi / lo 16-bit halves inside the kernel (two MFMAs per K step): include/spider_hip.h, DESIGN.md section 4. The
# 16-bit format of the call is that of W.
# "Split once, doubled K": above A32_DUP_MIN_FLOP the operand is written ONCE in the operand-split form [round16(v) | round16(v -
# round16(v))] ([M, 2K]; v = the fp32 tensor, its LayerNorm or its GroupNorm) and the 16-bit tile kernels run over it against the
# weight repeated along K ([W | W], built once per marked weight): the same hi . W + lo . W sum in the fp32 accumulator as the a32
# kernels form with two MFMAs per K step on register-staged tiles, at the speed of the LDS-DMA / 256^2 kernels and with all of their
# epilogues (GEGLU, rowbias, res32 / c32d, GroupNorm statistics).
A32_DUP_MIN_FLOP = float(_os.environ.get("SPIDER_A32_DUP_GF", "4")) * 1e9
A32_DUP_MIN_M = int(_os.environ.get("SPIDER_A32_DUP_MIN_M", "0"))      # rows below which the a32 kernels keep the call ([W | W] doubles the weight bytes)


def _dup_ok(M: int, N: int, K: int) -> bool:
    return 2.0 * M * N * K >= A32_DUP_MIN_FLOP and M >= A32_DUP_MIN_M and K % 8 == 0


def _wdup(W: torch.Tensor):
    """[W | W] along the last axis of a marked weight ([N, K] -> [N, 2K]; OHWI [Cout, kh, kw, Cin] -> [Cout, kh, kw, 2 Cin]), built on
    first use outside stream capture and kept with the tensor; None for unmarked tensors (slices, activations as W)."""
    if not getattr(W, "_spider_weight", False):
        return None
    t = getattr(W, "_spider_dup", None)
    tag = (W._version, W.data_ptr())
    if t is None or getattr(W, "_spider_dup_tag", None) != tag:
        if torch.cuda.is_current_stream_capturing():
            if t is not None:
                raise RuntimeError("a marked weight was modified in place and is first used again under stream capture")
            return None
        t = mark_weight(torch.cat([W, W], -1).contiguous())
        W._spider_dup, W._spider_dup_tag = t, tag
    return t


dup_weight = _wdup


def row_split(x32, dtype, gamma=None, beta=None, eps=1e-5):
    """x32 [..., K] fp32 -> [..., 2K] 16-bit = [hi | lo] of x32 itself (gamma None) or of LayerNorm(x32) * gamma + beta (fp32 statistics)"""
    _chk(x32, torch.float32, "x32")
    K = x32.shape[-1]
    y = torch.empty(*x32.shape[:-1], 2 * K, dtype=dtype, device=x32.device)
    _, sfx = _h16(y)
    if gamma is not None:
        _chk(gamma, dtype, "gamma")
    if beta is not None:
        _chk(beta, dtype, "beta")
    _lib.call(f"spider_row_split_f32_{sfx}", _p(x32), _p(gamma), _p(beta), _p(y), x32.numel() // K, K, float(eps), _stream())
    return y


def groupnorm_f32in_split(x32, gamma, beta, groups=32, eps=1e-5, silu=False, partial: Optional["GnPartial"] = None):
    """GroupNorm (+ SiLU) of the fp32 tensor x32 [B, ..., C] in the operand-split form [B, ..., 2C]"""
    dt, sfx = _h16(gamma)
    _chk(x32, torch.float32, "x32"); _chk(gamma, dt, "gamma"); _chk(beta, dt, "beta")
    B, Cn = x32.shape[0], x32.shape[-1]
    HW = x32.numel() // (B * Cn)
    y = torch.empty(*x32.shape[:-1], 2 * Cn, dtype=dt, device=x32.device)
    ws, pt, nch = None, None, 0
    if partial is not None:
        assert partial.groups == groups and tuple(partial.t.shape) == (B, partial.nchunk, groups, 2)
        pt, nch = partial.t, partial.nchunk
    else:
        ws = torch.empty(B * groupnorm_nchunk(HW) * groups * 2, dtype=torch.float32, device=x32.device)
    _lib.call(f"spider_groupnorm_f32in_split_nhwc_{sfx}", _p(x32), _p(pt), nch, _p(gamma), _p(beta), _p(y), _p(ws), B, HW, Cn, groups,
              float(eps), int(silu), _stream())
    return y


def gemm_a32(A32, W, bias=None, res=None, out_scale=1.0, res32=None, want32=False):
    dt, sfx = _h16(W)
    if _dup_ok(A32.numel() // W.shape[1], W.shape[0], W.shape[1]):
        W2 = _wdup(W)
        if W2 is not None:
            return gemm(row_split(A32, dt), W2, bias=bias, res=res, out_scale=out_scale, res32=res32, want32=want32)
    _chk(A32, torch.float32, "A32"); _chk(W, dt, "W")
    N, K = W.shape
    assert A32.shape[-1] == K, f"gemm_a32: A[..., {A32.shape[-1]}] vs W[{N},{K}]"
    M = A32.numel() // K
    out = torch.empty(*A32.shape[:-1], N, dtype=dt, device=A32.device)
    o32 = torch.empty(out.shape, dtype=torch.float32, device=A32.device) if want32 else None
    if res32 is not None:
        _chk(res32, torch.float32, "res32")
    wt = _tiled(W, M)
    _lib.call(f"spider_gemm_a32_{sfx}", _p(A32), _p(W if wt is None else wt), _p(out), _p(bias), _p(res), M, N, K, K, N, float(out_scale),
              int(wt is not None), _p(res32), _p(o32), _p(_workspace(A32.device)), WS_BYTES, _stream())
    return (out, o32) if want32 else out


def fold_layernorm_exact(W, gamma, beta, bias=None):
    """parameters of gemm_ln_a32 (once per layer): (W itself, gamma, colsum = sum_k gamma_k W[n,k] in fp32, colbias = W @ beta + bias)"""
    W32 = W.float()
    colsum = (W32 * gamma.float()[None, :]).sum(1).contiguous()
    colbias = W32 @ beta.float()
    if bias is not None:
        colbias = colbias + bias.float()
    return (W, gamma.to(W.dtype).contiguous(), colsum, colbias.contiguous(), beta.to(W.dtype).contiguous(),
            None if bias is None else bias.to(W.dtype).contiguous())


def gemm_ln_a32(A32, W, gamma, colsum, colbias, beta=None, bias=None, act=None, eps=1e-5):
    """LayerNorm(A32) @ W^T + bias (+ GEGLU) on the fp32 rows A32 [..., K]: statistics in fp32, gamma applied to A before the hi / lo
    split, W exact (no re-rounded W * gamma). (W, gamma, colsum, colbias, beta, bias) = fold_layernorm_exact(W, gamma, beta, bias);
    beta / bias (the LayerNorm's shift and the projection's bias as 16-bit vectors) serve the split-once route of large calls, which
    applies the LayerNorm exactly as written -- (x - mean) rstd gamma + beta in fp32 -- before the split."""
    dt, sfx = _h16(W)
    if beta is not None and _dup_ok(A32.numel() // W.shape[1], W.shape[0], W.shape[1]):
        W2 = _wdup(W)
        if W2 is not None:
            return gemm(row_split(A32, dt, gamma, beta, eps), W2, bias=bias, act=act)
    _chk(A32, torch.float32, "A32"); _chk(W, dt, "W"); _chk(gamma, dt, "gamma")
    _chk(colsum, torch.float32, "colsum"); _chk(colbias, torch.float32, "colbias")
    N, K = W.shape
    assert A32.shape[-1] == K and colsum.numel() == N and colbias.numel() == N and gamma.numel() == K
    assert act in (None, "geglu", "geglu_exact")
    M = A32.numel() // K
    n_out = N // 2 if act in GLU_ACTS else N
    out = torch.empty(*A32.shape[:-1], n_out, dtype=dt, device=A32.device)
    wt = _tiled(W, M)
    _lib.call(f"spider_gemm_ln_a32_{sfx}", _p(A32), _p(W if wt is None else wt), _p(out), _p(gamma), _p(colsum), _p(colbias), M, N, K, n_out,
              ACT[act], float(eps), int(wt is not None), _stream())
    return out


def gemm_gn_in_a32(A32, W, part: "GnPartial", gamma, beta, HW: int, eps: float, bias=None, want32=False):
    """GroupNorm(A32) @ W^T + bias with A32 [B, HW, K] fp32, normalised in fp32 inside the GEMM and split hi / lo"""
    dt, sfx = _h16(W)
    _chk(A32, torch.float32, "A32"); _chk(W, dt, "W")
    N, K = W.shape
    M = A32.numel() // K
    if _dup_ok(M, N, K):
        W2 = _wdup(W)
        if W2 is not None:
            return gemm(groupnorm_f32in_split(A32, gamma, beta, part.groups, eps, False, partial=part), W2, bias=bias, want32=want32)
    out = torch.empty(*A32.shape[:-1], N, dtype=dt, device=A32.device)
    o32 = torch.empty(out.shape, dtype=torch.float32, device=A32.device) if want32 else None
    wt = _tiled(W, M)
    _lib.call(f"spider_gemm_gn_in_a32_{sfx}", _p(A32), _p(W if wt is None else wt), _p(out), _p(bias), M, N, K, N, int(wt is not None),
              _p(part.t), part.nchunk, _p(gamma), _p(beta), part.groups, float(eps), HW, _p(o32), _stream())
    return (out, o32) if want32 else out


def conv_a32(x32, w, bias=None, res=None, rowbias=None, stride=1, pad=(0, 0), dil=1, up_size=None, out_scale=1.0, res32=None, want32=False):
    """NHWC conv with the fp32 image x32 [B,H,W,Cin] as the A operand; w [Cout,kh,kw,Cin] 16-bit -> [B,Ho,Wo,Cout] 16-bit (+ fp32)."""
    dt, sfx = _h16(w)
    _chk(x32, torch.float32, "x32"); _chk(w, dt, "w")
    B, H, Wd, Cin = x32.shape
    Cout, kh, kw = w.shape[0], w.shape[1], w.shape[2]
    assert w.shape[3] == Cin, f"conv_a32: x has {Cin} channels, w expects {w.shape[3]}"
    Hs, Ws = up_size if up_size is not None else (H, Wd)
    Ho = (Hs + 2 * pad[0] - dil * (kh - 1) - 1) // stride + 1
    Wo = (Ws + 2 * pad[1] - dil * (kw - 1) - 1) // stride + 1
    if _dup_ok(B * Ho * Wo, Cout, kh * kw * Cin) and Cin % 8 == 0:
        # large conv (the UNet's samplers, shortcuts and every conv of the video UNet): the in-kernel hi / lo split lives on the
        # register-staged tiles, 4-5x slower than the LDS-DMA / 256^2 kernels at this size -- split once into [hi | lo] channels and run
        # the fast conv over 2 Cin channels against [W | W]
        w2 = _wdup(w)
        if w2 is not None:
            return conv_ex(row_split(x32, dt), w2, bias=bias, res=res, rowbias=rowbias, stride=stride, pad=pad, dil=dil, up_size=up_size,
                           out_scale=out_scale, res32=res32, want32=want32)
    if 2.0 * B * Ho * Wo * Cout * kh * kw * Cin >= A32_SPLIT_MIN_FLOP and x32.numel() % 8 == 0 and rowbias is None and res is None and out_scale == 1.0:
        # (unmarked weight: no [W | W] copy is kept) split once, run the fast conv on each half, sum in fp32
        hi, lo = split_hilo(x32, dt)
        kw_ = dict(stride=stride, pad=pad, dil=dil, up_size=up_size)
        _, y32 = conv_ex(hi, w, bias=bias, res32=res32, want32=True, **kw_)
        r = conv_ex(lo, w, res32=y32, want32=True, **kw_)
        return r if want32 else r[0]
    out = torch.empty(B, Ho, Wo, Cout, dtype=dt, device=x32.device)
    o32 = torch.empty(out.shape, dtype=torch.float32, device=x32.device) if want32 else None
    if res32 is not None:
        _chk(res32, torch.float32, "res32")
    uh, uw = up_size if up_size is not None else (0, 0)
    wt = _tiled(w, B * Ho * Wo)
    _lib.call(f"spider_conv_nhwc_a32_{sfx}", _p(x32), _p(w if wt is None else wt), _p(out), _p(bias), _p(res), _p(rowbias), B, H, Wd, Cin,
              Cout, kh, kw, stride, pad[0], pad[1], dil, uh, uw, float(out_scale), int(wt is not None), _p(res32), _p(o32),
              _p(_workspace(x32.device)), WS_BYTES, _stream())
    return (out, o32) if want32 else out


A32_SPLIT_MIN_FLOP = float(_os.environ.get("SPIDER_A32_SPLIT_GF", "4")) * 1e9      # conv_a32 above this: split pass + two fast convs


def split_hilo(x32, dtype):
    """fp32 tensor -> (hi, lo) 16-bit tensors with hi + lo == x to ~22 bits"""
    _chk(x32, torch.float32, "x32")
    hi = torch.empty(x32.shape, dtype=dtype, device=x32.device)
    lo = torch.empty_like(hi)
    _, sfx = _h16(hi)
    _lib.call(f"spider_split_hilo_f32_{sfx}", _p(x32), _p(hi), _p(lo), x32.numel(), _stream())
    return hi, lo


def groupnorm_f32in(x32, gamma, beta, groups=32, eps=1e-5, silu=False, partial: Optional["GnPartial"] = None, want16=True, want32=False):
    """GroupNorm (+ SiLU) of the fp32 tensor x32 [B, ..., C]; returns the 16-bit result (rounded once), the fp32 result, or both."""
    dt, sfx = _h16(gamma)
    _chk(x32, torch.float32, "x32"); _chk(gamma, dt, "gamma"); _chk(beta, dt, "beta")
    B, Cn = x32.shape[0], x32.shape[-1]
    HW = x32.numel() // (B * Cn)
    y = torch.empty(x32.shape, dtype=dt, device=x32.device) if want16 else None
    y32 = torch.empty_like(x32) if want32 else None
    ws, pt, nch = None, None, 0
    if partial is not None:
        assert partial.groups == groups and tuple(partial.t.shape) == (B, partial.nchunk, groups, 2)
        pt, nch = partial.t, partial.nchunk
    else:
        ws = torch.empty(B * groupnorm_nchunk(HW) * groups * 2, dtype=torch.float32, device=x32.device)
    _lib.call(f"spider_groupnorm_f32in_nhwc_{sfx}", _p(x32), _p(pt), nch, _p(gamma), _p(beta), _p(y), _p(y32), _p(ws), B, HW, Cn, groups,
              float(eps), int(silu), _stream())
    return (y, y32) if (want16 and want32) else (y if want16 else y32)


def conv2d_small_cin_f32in(x32, w, bias=None, want32=False):
    dt, sfx = _h16(w)
    _chk(x32, torch.float32, "x32"); _chk(w, dt, "w")
    B, H, Wd, Cin = x32.shape
    Cout, ks = w.shape[0], w.shape[1]
    out = torch.empty(B, H, Wd, Cout, dtype=dt, device=x32.device)
    o32 = torch.empty(out.shape, dtype=torch.float32, device=x32.device) if want32 else None
    _lib.call(f"spider_conv2d_small_cin_f32in_{sfx}", _p(x32), _p(w), _p(bias), _p(out), _p(o32), B, H, Wd, Cin, Cout, ks, _stream())
    return (out, o32) if want32 else out


def conv2d_small_cout_f32in(x32, w, bias=None):
    dt, sfx = _h16(w)
    _chk(x32, torch.float32, "x32"); _chk(w, dt, "w")
    B, H, Wd, Cin = x32.shape
    Cout, ks = w.shape[0], w.shape[1]
    out = torch.empty(B, H, Wd, Cout, dtype=torch.float32, device=x32.device)
    _lib.call(f"spider_conv2d_small_cout_f32in_{sfx}", _p(x32), _p(w), _p(bias), _p(out), B, H, Wd, Cin, Cout, ks, _stream())
    return out


def latent_to_nhwc_f32(lat, reps=1, scale=1.0):
    """fp32 NCHW [B,C,H,W] -> fp32 NHWC [reps*B,H,W,C]"""
    _chk(lat, torch.float32, "lat")
    B, Cn, H, Wd = lat.shape
    out = torch.empty(reps * B, H, Wd, Cn, dtype=torch.float32, device=lat.device)
    _lib.call("spider_latent_to_nhwc_f32", _p(lat), _p(out), B, Cn, H * Wd, reps, float(scale), _stream())
    return out


def concat_channels_f32(a32, b32):
    """channel concat of two fp32 NHWC tensors: a copy of bit patterns, done by the 16-bit concat kernel on the 2-halves-per-float view"""
    _chk(a32, torch.float32, "a32"); _chk(b32, torch.float32, "b32")
    C1, C2 = a32.shape[-1], b32.shape[-1]
    out = torch.empty(*a32.shape[:-1], C1 + C2, dtype=torch.float32, device=a32.device)
    rows = a32.numel() // C1
    assert b32.numel() // C2 == rows
    _lib.call("spider_concat_channels_bf16", _p(a32), _p(b32), _p(out), rows, 2 * C1, 2 * C2, _stream())
    return out


# --------------------------------------------------------------------------- UNet elementwise
def groupnorm_nchunk(HW: int) -> int:
    return _lib.load().spider_groupnorm_nchunk(HW)


def groupnorm(x, gamma, beta, groups=32, eps=1e-5, silu=False, out=None, ws=None, partial: Optional["GnPartial"] = None):
    """x [B, ..., C] NHWC bf16."""
    dt, sfx = _h16(x)
    _chk(x, dt, "x"); _chk(gamma, dt, "gamma"); _chk(beta, dt, "beta")
    B, Cn = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cn)
    if out is None:
        out = torch.empty_like(x)
    if partial is not None:      # statistics from the producer of x (conv_ex(..., gn_groups=...)): the apply pass alone
        assert partial.groups == groups and tuple(partial.t.shape) == (B, partial.nchunk, groups, 2)
        _lib.call(f"spider_groupnorm_apply_nhwc_{sfx}", _p(x), _p(partial.t), partial.nchunk, _p(gamma), _p(beta), _p(out), B, HW, Cn,
                  groups, float(eps), int(silu), _stream())
        return out
    if ws is None:
        ws = torch.empty(B * groupnorm_nchunk(HW) * groups * 2, dtype=torch.float32, device=x.device)
    _lib.call(f"spider_groupnorm_nhwc_{sfx}", _p(x), _p(gamma), _p(beta), _p(out), _p(ws), B, HW, Cn, groups, float(eps),
              int(silu), _stream())
    return out


def groupnorm_cat(x1, x2, gamma, beta, groups=32, eps=1e-5, silu=False, ws=None):
    """GroupNorm(+SiLU) of cat([x1, x2], channel) without a concat launch; returns (normalised, concatenated input)."""
    dt, sfx = _h16(x1)
    _chk(x1, dt, "x1"); _chk(x2, dt, "x2"); _chk(gamma, dt, "gamma"); _chk(beta, dt, "beta")
    B, C1, C2 = x1.shape[0], x1.shape[-1], x2.shape[-1]
    HW = x1.numel() // (B * C1)
    assert x2.shape[:-1] == x1.shape[:-1] and gamma.numel() == C1 + C2, "groupnorm_cat: sources must share [B, ..., *]"
    out = torch.empty(*x1.shape[:-1], C1 + C2, dtype=dt, device=x1.device)
    cat = torch.empty_like(out)
    if ws is None:
        ws = torch.empty(B * groupnorm_nchunk(HW) * groups * 2, dtype=torch.float32, device=x1.device)
    _lib.call(f"spider_groupnorm_cat_nhwc_{sfx}", _p(x1), _p(x2), _p(gamma), _p(beta), _p(out), _p(cat), _p(ws), B, HW, C1, C2,
              groups, float(eps), int(silu), _stream())
    return out, cat


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    dt, sfx = _h16(x)
    _chk(x, dt, "x"); _chk(gamma, dt, "gamma"); _chk(beta, dt, "beta")
    Cn = x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    _lib.call(f"spider_layernorm_{sfx}", _p(x), _p(gamma), _p(beta), _p(out), x.numel() // Cn, Cn, float(eps), _stream())
    return out


def geglu(x, out=None):
    dt, sfx = _h16(x)
    _chk(x, dt, "x")
    inner = x.shape[-1] // 2
    M = x.numel() // (2 * inner)
    if out is None:
        out = torch.empty(*x.shape[:-1], inner, dtype=dt, device=x.device)
    _lib.call(f"spider_geglu_{sfx}", _p(x), _p(out), M, inner, _stream())
    return out


def swiglu(x, out=None):
    dt, sfx = _h16(x)
    _chk(x, dt, "x")
    inner = x.shape[-1] // 2
    M = x.numel() // (2 * inner)
    if out is None:
        out = torch.empty(*x.shape[:-1], inner, dtype=dt, device=x.device)
    _lib.call(f"spider_swiglu_{sfx}", _p(x), _p(out), M, inner, _stream())
    return out


def concat_channels(a, b, out=None):
    dt, sfx = _h16(a)
    _chk(a, dt, "a"); _chk(b, dt, "b")
    C1, C2 = a.shape[-1], b.shape[-1]
    rows = a.numel() // C1
    assert b.numel() // C2 == rows
    if out is None:
        out = torch.empty(*a.shape[:-1], C1 + C2, dtype=dt, device=a.device)
    _lib.call(f"spider_concat_channels_{sfx}", _p(a), _p(b), _p(out), rows, C1, C2, _stream())
    return out


def act(x, kind: str, param: float = 0.0, out=None):
    dt, sfx = _h16(x)
    _chk(x, dt, "x")
    if out is None:
        out = torch.empty_like(x)
    _lib.call(f"spider_act_ex_{sfx}", _p(x), _p(out), x.numel(), ACT[kind], float(param), _stream())
    return out


def add_scaled(a, b, scale: float, out=None):
    """bf16((a + b) * scale)"""
    dt, sfx = _h16(a)
    _chk(a, dt, "a"); _chk(b, dt, "b")
    if out is None:
        out = torch.empty_like(a)
    _lib.call(f"spider_add_scaled_{sfx}", _p(a), _p(b), _p(out), a.numel(), float(scale), _stream())
    return out


def axpby(a, b, alpha: float, beta: float, out=None):
    """bf16(alpha * a + beta * b)"""
    dt, sfx = _h16(a)
    _chk(a, dt, "a"); _chk(b, dt, "b")
    assert a.shape == b.shape, (a.shape, b.shape)
    if out is None:
        out = torch.empty_like(a)
    _lib.call(f"spider_axpby_{sfx}", _p(a), _p(b), _p(out), a.numel(), float(alpha), float(beta), _stream())
    return out


def mean_tokens(x, out=None):
    """x [B,T,C] bf16 -> [B,C] mean over T"""
    dt, sfx = _h16(x)
    _chk(x, dt, "x")
    B, T, Cn = x.shape
    if out is None:
        out = torch.empty(B, Cn, dtype=dt, device=x.device)
    _lib.call(f"spider_mean_tokens_{sfx}", _p(x), _p(out), B, T, Cn, _stream())
    return out


def moe_combine(xs, logits, out=None):
    """xs: list of E tensors [B, ...] bf16; logits [B, ld >= E] bf16 (first E columns used) -> sum_e r_e * xs[e] with
    r = sigmoid(logits) / sum(sigmoid(logits))."""
    for t in xs:
        dt, sfx = _h16(t)
        _chk(t, dt, "expert output")
    _chk(logits, dt, "logits")
    B, ld = logits.shape
    E = len(xs)
    assert ld >= E and all(t.shape == xs[0].shape for t in xs) and xs[0].shape[0] == B
    if out is None:
        out = torch.empty_like(xs[0])
    ptrs = (C.c_void_p * E)(*[t.data_ptr() for t in xs])
    _lib.call(f"spider_moe_combine_{sfx}", ptrs, E, _p(logits), ld, _p(out), B, xs[0].numel() // B, _stream())
    return out


def l2_normalize(x, eps: float = 1e-12, out=None):
    """rows of x [..., n] divided by max(L2 norm, eps) (torch.nn.functional.normalize)."""
    dt, sfx = _h16(x)
    _chk(x, dt, "x")
    if out is None:
        out = torch.empty_like(x)
    n = x.shape[-1]
    _lib.call(f"spider_l2_normalize_rows_{sfx}", _p(x), _p(out), x.numel() // n, n, float(eps), _stream())
    return out


def add(a, b, out=None):
    dt, sfx = _h16(a)
    _chk(a, dt, "a"); _chk(b, dt, "b")
    if out is None:
        out = torch.empty_like(a)
    _lib.call(f"spider_add_{sfx}", _p(a), _p(b), _p(out), a.numel(), _stream())
    return out


def conv2d_small_cin(x, w, bias=None, out=None):
    dt, sfx = _h16(x)
    _chk(x, dt, "x"); _chk(w, dt, "w")
    B, H, Wd, Cin = x.shape
    Cout, ks = w.shape[0], w.shape[1]
    if out is None:
        out = torch.empty(B, H, Wd, Cout, dtype=dt, device=x.device)
    _lib.call(f"spider_conv2d_small_cin_{sfx}", _p(x), _p(w), _p(bias), _p(out), B, H, Wd, Cin, Cout, ks, _stream())
    return out


def conv2d_small_cout(x, w, bias=None, out_f32=True, out=None):
    dt, sfx = _h16(x)
    _chk(x, dt, "x"); _chk(w, dt, "w")
    B, H, Wd, Cin = x.shape
    Cout, ks = w.shape[0], w.shape[1]
    if out is None:
        out = torch.empty(B, H, Wd, Cout, dtype=torch.float32 if out_f32 else dt, device=x.device)
    y32, y16 = (out, None) if out.dtype == torch.float32 else (None, out)
    _lib.call(f"spider_conv2d_small_cout_{sfx}", _p(x), _p(w), _p(bias), _p(y32), _p(y16), B, H, Wd, Cin, Cout, ks, _stream())
    return out


def latent_to_nhwc(lat, reps=1, scale=1.0, out=None, dtype=BF16):
    """fp32 NCHW [B,C,H,W] -> 16-bit (dtype, or out's) NHWC [reps*B,H,W,C]."""
    _chk(lat, torch.float32, "lat")
    B, Cn, H, Wd = lat.shape
    if out is None:
        out = torch.empty(reps * B, H, Wd, Cn, dtype=dtype, device=lat.device)
    _, sfx = _h16(out)
    _lib.call(f"spider_latent_to_nhwc_{sfx}", _p(lat), _p(out), B, Cn, H * Wd, reps, float(scale), _stream())
    return out


def cfg_combine(eps2, guidance, out=None):
    """eps2 fp32 NHWC [2*B,H,W,C] (uncond first) -> fp32 NCHW [B,C,H,W]."""
    _chk(eps2, torch.float32, "eps2")
    B2, H, Wd, Cn = eps2.shape
    B = B2 // 2
    if out is None:
        out = torch.empty(B, Cn, H, Wd, dtype=torch.float32, device=eps2.device)
    _lib.call("spider_cfg_combine_f32", _p(eps2), _p(out), B, Cn, H * Wd, float(guidance), _stream())
    return out


def lincomb(tensors, coefs, out=None):
    n = len(tensors)
    for t in tensors:
        _chk(t, torch.float32, "lincomb input")
    if out is None:
        out = torch.empty_like(tensors[0])
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
    cf = (C.c_float * n)(*[float(c) for c in coefs])
    _lib.call("spider_lincomb_f32", ptrs, cf, n, _p(out), out.numel(), _stream())
    return out


def nhwc_to_nchw(x, mul=1.0, add_=0.0, clamp01=False, out=None):
    _chk(x, torch.float32, "x")
    B, H, Wd, Cn = x.shape
    if out is None:
        out = torch.empty(B, Cn, H, Wd, dtype=torch.float32, device=x.device)
    _lib.call("spider_nhwc_to_nchw_f32", _p(x), _p(out), B, Cn, H * Wd, float(mul), float(add_), int(clamp01), _stream())
    return out


def softmax_rows(x, scale=1.0, n_valid=None, out=None, dtype=BF16):
    """fp32 [rows, n] -> 16-bit softmax(scale * x) per row over the first n_valid (default n) columns; the rest -> 0."""
    _chk(x, torch.float32, "x")
    n = x.shape[-1]
    if out is None:
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _, sfx = _h16(out)
    _lib.call(f"spider_softmax_rows_f32_{sfx}", _p(x), _p(out), x.numel() // n, n, n if n_valid is None else n_valid, float(scale),
              _stream())
    return out


def pack_keep_bits(u: torch.Tensor, thr: float, n_valid: int) -> torch.Tensor:
    """u [n] fp32 uniforms on the device -> int64 [ceil(n / 64)] bit words: bit j = (u[j] < thr) for j < n_valid (keep vector of
    StoryDiffusion's consistent self-attention, layout of spider_attn_bf16's keep_bits). No host synchronisation."""
    _chk(u, torch.float32, "u")
    n = u.numel()
    words = torch.empty((n + 63) // 64, dtype=torch.int64, device=u.device)
    _lib.call("spider_pack_keep_bits_f32", _p(u), _p(words), n, int(n_valid), float(thr), _stream())
    return words


# --------------------------------------------------------------------------- safety checker around the CLIP ViT (csrc/safety.hip)
RESIZE_PRECISION_BITS = 22      # Pillow's 8-bit resampler: taps are round(w * 2^22), accumulated in int32


def bicubic_taps(in_size: int, out_size: int, first: int = 0, count: Optional[int] = None):
    """Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc` (Resample.c) for the antialiased BICUBIC filter (a = -0.5, support
    2 * max(scale, 1), taps normalised to sum 1, then round(w * 2^22) away from zero), for output indices [first, first + count).
    -> (bounds int32 [count, 2] = (first input index, tap count), taps int32 [count, ks]). A pass whose size does not change is the
    identity in Pillow (ImagingResample skips it): one tap of weight 2^22. Host arithmetic in double, as in C."""
    import numpy as np
    count = out_size - first if count is None else count
    one = 1 << RESIZE_PRECISION_BITS
    if in_size == out_size:
        bounds = np.stack([np.arange(first, first + count), np.ones(count, dtype=np.int64)], 1).astype(np.int32)
        return bounds, np.full((count, 1), one, dtype=np.int32)

    def cubic(x):
        x = abs(x)
        if x < 1.0:
            return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * -0.5
        return 0.0

    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    ks = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((count, 2), dtype=np.int32)
    taps = np.zeros((count, ks), dtype=np.int32)
    ss = 1.0 / fscale
    for j in range(count):
        center = (first + j + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [cubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = sum(w)
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[j] = (xmin, xmax)
        taps[j, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= in_size).all() and (bounds[:, 1] <= ks).all()
    return bounds, taps


def clip_resize_geometry(H: int, W: int, size: int, crop: int):
    """(Hr, Wr, top, left) of CLIPImageProcessor: shortest edge -> `size`, long edge int(size * long / short) (transformers'
    get_resize_output_image_size), centre crop top = (Hr - crop) // 2, left = (Wr - crop) // 2."""
    if H <= W:
        Hr, Wr = size, int(size * W / H)
    else:
        Hr, Wr = int(size * H / W), size
    if crop > min(Hr, Wr):
        raise NotImplementedError(f"crop_size {crop} larger than the resized image {Hr}x{Wr}: the padded centre crop is not implemented")
    return Hr, Wr, (Hr - crop) // 2, (Wr - crop) // 2


_CLIP_TABLES = {}


def clip_preprocess_tables(H: int, W: int, size: int, crop: int, mean, std, device) -> dict:
    """Device-resident tap tables + normalisation constants of spider_clip_preprocess for one image shape (built once per shape on
    the host, outside stream capture: engines run an eager pass before they capture)."""
    device = torch.device(device)
    key = (H, W, size, crop, tuple(float(m) for m in mean), tuple(float(s) for s in std), device.type, device.index)
    t = _CLIP_TABLES.get(key)
    if t is None:
        Hr, Wr, top, left = clip_resize_geometry(H, W, size, crop)
        xb, xt = bicubic_taps(W, Wr, left, crop)
        yb, yt = bicubic_taps(H, Hr, top, crop)
        dv = lambda a, dt: torch.as_tensor(a, dtype=dt).contiguous().to(device)
        t = dict(xb=dv(xb, torch.int32), xt=dv(xt, torch.int32), yb=dv(yb, torch.int32), yt=dv(yt, torch.int32),
                 norm=dv(list(mean) + list(std), torch.float32), H=H, W=W, crop=crop, ks_x=xt.shape[1], ks_y=yt.shape[1])
        _CLIP_TABLES[key] = t
    return t


def clip_preprocess(images, tables: dict, patch: int, dtype=BF16, out=None):
    """images [B,3,H,W] fp32 in [0,1] (VAEDecoderEngine.decode's buffer) -> patch rows [B * (crop/patch)^2, Kp] of `dtype`,
    Kp = 3 patch^2 rounded up to a multiple of 8, pad columns zero: numpy_to_pil + CLIPImageProcessor (Pillow BICUBIC) on the device."""
    _chk(images, torch.float32, "images")
    B, Cn, H, W = images.shape
    if Cn != 3 or (H, W) != (tables["H"], tables["W"]):
        raise ValueError(f"clip_preprocess: images {tuple(images.shape)} do not match the tables' [B,3,{tables['H']},{tables['W']}]")
    crop = tables["crop"]
    Kp = (3 * patch * patch + 7) // 8 * 8
    if out is None:
        out = torch.empty(B * (crop // patch) ** 2, Kp, dtype=dtype, device=images.device)
    _, sfx = _h16(out)
    tmp = torch.empty(B * 3 * H * crop, dtype=torch.uint8, device=images.device)
    _lib.call("spider_clip_preprocess", _p(images), _p(tmp), _p(out), _p(tables["xb"]), _p(tables["xt"]), tables["ks_x"], _p(tables["yb"]),
              _p(tables["yt"]), tables["ks_y"], _p(tables["norm"]), B, H, W, crop, patch, Kp, int(sfx == "f16"), _stream())
    return out


def safety_decide(image_embeds, concept_embeds, special_care_embeds, thr_concept, thr_special, scores=None, flags=None):
    """-> (scores fp32 [B, n_special + n_concept] (special-care first), flags int32 [B]); see spider_safety_decide."""
    dt, sfx = _h16(image_embeds)
    _chk(image_embeds, dt, "image_embeds"); _chk(concept_embeds, dt, "concept_embeds"); _chk(special_care_embeds, dt, "special_care_embeds")
    _chk(thr_concept, torch.float32, "thr_concept"); _chk(thr_special, torch.float32, "thr_special")
    B, D = image_embeds.shape
    n_c, n_s = concept_embeds.shape[0], special_care_embeds.shape[0]
    assert concept_embeds.shape[1] == D and (n_s == 0 or special_care_embeds.shape[1] == D)
    assert thr_concept.numel() == n_c and thr_special.numel() == n_s
    if scores is None:
        scores = torch.empty(B, n_s + n_c, dtype=torch.float32, device=image_embeds.device)
    if flags is None:
        flags = torch.empty(B, dtype=torch.int32, device=image_embeds.device)
    _lib.call("spider_safety_decide", _p(image_embeds), _p(concept_embeds), _p(special_care_embeds) if n_s else None, _p(thr_concept),
              _p(thr_special) if n_s else None, _p(scores), _p(flags), B, D, n_c, n_s, int(sfx == "f16"), _stream())
    return scores, flags


def image_blackout_(images, flags):
    """images [B, ...] fp32, flags [B] int32 on the device: flagged images become zeros IN PLACE. -> images"""
    _chk(images, torch.float32, "images"); _chk(flags, torch.int32, "flags")
    B = images.shape[0]
    assert flags.numel() == B
    _lib.call("spider_image_blackout_f32", _p(images), _p(flags), B, images.numel() // B, _stream())
    return images


# --------------------------------------------------------------------------- Whisper log-mel features (csrc/audio_features.hip)
def logmel(waves, lengths, tables: dict, out=None, mask=None, offsets=None, lengths_dev=None):
    """Packed fp32 waveforms -> (input_features [B, mel, cap] fp32, attention_mask [B, cap] int32), both written completely: what
    WhisperFeatureExtractor returns for clips padded to n_samples (spider_amd/audio_features.py states the feature).
    waves: 1-D fp32 on the device, the clips one behind the other; lengths: samples per clip ON THE HOST (they size the grid: only
    frames whose window reaches the clip are computed); tables: audio_features.logmel_tables(cfg, device). offsets / lengths_dev:
    the int32 device arrays the kernel reads; built here from `lengths` (clip b starts where clip b - 1 ends) when not given --
    pass them to keep host -> device copies out of a graph capture. Two launches on the current stream, no synchronisation."""
    _chk(waves, torch.float32, "waves")
    dv = waves.device
    lens = [min(max(int(n), 0), tables["n_samples"]) for n in lengths]
    B, mel, cap, hop, n_fft = len(lens), tables["mel"], tables["cap"], tables["hop"], tables["n_fft"]
    if B == 0:
        raise ValueError("logmel: no clips")
    if (offsets is None) != (lengths_dev is None):
        raise ValueError("logmel: pass offsets and lengths_dev together")
    if offsets is None:
        offs = [0]
        for n in lens[:-1]:
            offs.append(offs[-1] + n)
        if offs[-1] + lens[-1] > waves.numel():
            raise ValueError(f"logmel: the clips hold {offs[-1] + lens[-1]} samples, waves has {waves.numel()}")
        meta = torch.tensor([offs, lens], dtype=torch.int32).to(dv)
        offsets, lengths_dev = meta[0], meta[1]
    _chk(offsets, torch.int32, "offsets"); _chk(lengths_dev, torch.int32, "lengths_dev")
    assert offsets.numel() == B and lengths_dev.numel() == B
    _chk(tables["table"], torch.float32, "table"); _chk(tables["fb"], torch.float32, "fb")
    ldt = tables["table"].shape[1]
    assert tuple(tables["table"].shape) == (n_fft, 64 * ((n_fft // 2 + 32) // 32)) and tuple(tables["fb"].shape) == (n_fft // 2 + 1, mel)
    if out is None:
        out = torch.empty(B, mel, cap, dtype=torch.float32, device=dv)
    if mask is None:
        mask = torch.empty(B, cap, dtype=torch.int32, device=dv)
    _chk(out, torch.float32, "out"); _chk(mask, torch.int32, "mask")
    assert tuple(out.shape) == (B, mel, cap) and tuple(mask.shape) == (B, cap)
    tf = _lib.load().spider_logmel_tile_frames()
    frames = min(cap, -(-(max(lens) + n_fft // 2) // hop))          # frames of the longest clip whose window reaches it
    max_tiles = max(1, -(-frames // tf))
    tile_max = torch.empty(B, max_tiles, dtype=torch.float32, device=dv)
    _lib.call("spider_logmel_f32", _p(waves), _p(offsets), _p(lengths_dev), _p(tables["table"]), _p(tables["fb"]), _p(out), _p(mask),
              _p(tile_max), B, tables["n_samples"], n_fft, hop, mel, cap, ldt, max_tiles, _stream())
    return out, mask


# --------------------------------------------------------------------------- Qwen2-VL image patch rows (csrc/image_features.hip)
def qwen_smart_resize(height: int, width: int, factor: int = 28, min_pixels: int = 56 * 56, max_pixels: int = 14 * 14 * 4 * 1280):
    """transformers' `smart_resize` of Qwen2-VL to the letter: both sides multiples of `factor` (Python's round: half to even), the
    area within [min_pixels, max_pixels] (floor on the way down, ceil on the way up), ValueError beyond an aspect ratio of 200."""
    if max(height, width) / min(height, width) > 200:
        raise ValueError(f"absolute aspect ratio must be smaller than 200, got {max(height, width) / min(height, width)}")
    h_bar = round(height / factor) * factor
    w_bar = round(width / factor) * factor
    if h_bar * w_bar > max_pixels:
        beta = math.sqrt((height * width) / max_pixels)
        h_bar = max(factor, math.floor(height / beta / factor) * factor)
        w_bar = max(factor, math.floor(width / beta / factor) * factor)
    elif h_bar * w_bar < min_pixels:
        beta = math.sqrt(min_pixels / (height * width))
        h_bar = math.ceil(height * beta / factor) * factor
        w_bar = math.ceil(width * beta / factor) * factor
    return h_bar, w_bar


QWEN_DESC_WORDS = 16      # int64 words per image record of spider_qwen_image_patches (include/spider_hip.h lists the fields)
_QWEN_TABLES = {}


def qwen_image_tables(sizes, cfg, device) -> dict:
    """What spider_qwen_image_patches reads for a batch of images of these `sizes` ((H, W), ...) under `cfg`
    (image_features.ImagePatchConfig), built once per (sizes, cfg, device) on the host and cached -- outside stream capture, like
    clip_preprocess_tables: per image the Pillow tap tables of both passes (bicubic_taps) in one int32 buffer and an int64 record
    {input offset, H, W, Ho, Wo, table offsets and tap counts, first output row, offset into the 8-bit intermediate, the input rows the
    vertical pass reads}; and the [3, 256] lookup table of (v * rescale_factor - mean) / std, computed as transformers' numpy `rescale`
    and `normalize` compute it (double product rounded to fp32, then fp32 subtract and divide) and cast once per output format."""
    import numpy as np
    device = torch.device(device)
    sizes = tuple((int(h), int(w)) for h, w in sizes)
    if not sizes:
        raise ValueError("qwen_image_tables: no images")
    key = (sizes, cfg, device.type, device.index)
    t = _QWEN_TABLES.get(key)
    if t is not None:
        return t
    P, m, Tp = cfg.patch_size, cfg.merge_size, cfg.temporal_patch_size
    S = P * m
    if (P * P) % 4 or S % 4 or (3 * Tp * P * P) % 8:
        raise NotImplementedError(f"patch_size {P} / merge_size {m} / temporal_patch_size {Tp}: patch_size^2 and patch_size * merge_size "
                                  "must be multiples of 4 and a patch row a multiple of 8 elements")
    desc = np.zeros((len(sizes), QWEN_DESC_WORDS), dtype=np.int64)
    tabs, grid = [], []
    n_tab = in_off = tmp_off = row0 = max_h = max_tiles = 0

    def put(a):
        nonlocal n_tab
        at = n_tab
        tabs.append(np.ascontiguousarray(a, dtype=np.int32).reshape(-1))
        n_tab += tabs[-1].size
        return at

    for i, (H, W) in enumerate(sizes):
        if H < 1 or W < 1:
            raise ValueError(f"qwen_image_tables: image {i} is {H}x{W}")
        Ho, Wo = qwen_smart_resize(H, W, S, cfg.min_pixels, cfg.max_pixels)
        xb, xt = bicubic_taps(W, Wo)
        yb, yt = bicubic_taps(H, Ho)
        y_first, y_end = int(yb[:, 0].min()), int((yb[:, 0] + yb[:, 1]).max())
        y_count = y_end - y_first
        desc[i] = (in_off, H, W, Ho, Wo, put(xb), put(xt), xt.shape[1], put(yb), put(yt), yt.shape[1], row0, tmp_off, y_first, y_count, 0)
        grid.append((1, Ho // P, Wo // P))
        in_off += H * W * 3
        tmp_off += 3 * y_count * Wo                          # a multiple of 4: Wo is one of patch_size * merge_size
        row0 += (Ho // P) * (Wo // P)
        max_h = max(max_h, y_count * (Wo // 4))
        max_tiles = max(max_tiles, (Ho // S) * (Wo // S))
    if len(cfg.image_mean) != 3 or len(cfg.image_std) != 3:
        raise NotImplementedError("image_mean / image_std must hold 3 values")
    x = (np.arange(256, dtype=np.uint8).astype(np.float64) * cfg.rescale_factor).astype(np.float32)      # transformers' rescale
    lut = ((x[:, None] - np.array(cfg.image_mean, dtype=np.float32)) / np.array(cfg.image_std, dtype=np.float32)).T      # and normalize
    lut = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32))
    lut_bf16 = (lut.to(BF16).view(torch.int16).to(torch.int32) & 0xffff).contiguous()      # round to nearest even, once
    t = dict(desc=torch.from_numpy(desc).to(device), tabs=torch.from_numpy(np.concatenate(tabs)).to(device),
             lut={BF16: lut_bf16.to(device), torch.float32: lut.view(torch.int32).contiguous().to(device)}, sizes=sizes, grid=grid,
             rows=row0, cols=3 * Tp * P * P, in_bytes=in_off, tmp_bytes=tmp_off, max_h_items=max_h, max_tiles=max_tiles,
             patch=P, merge=m, temporal=Tp)
    _QWEN_TABLES[key] = t
    return t


def qwen_image_patches(packed_u8, tables: dict, dtype=BF16, out=None):
    """packed uint8 RGB images (interleaved HWC, one behind the other, on the device) -> pixel_values [rows, 3 Tp P^2] of `dtype`
    (bf16, or fp32 with the host processor's bits): Qwen2VLImageProcessorPil on the device. tables: qwen_image_tables of the images'
    sizes. Two launches on the current stream whatever the number of images, every element of `out` written."""
    _chk(packed_u8, torch.uint8, "packed_u8")
    if dtype not in tables["lut"]:
        raise ValueError(f"qwen_image_patches: dtype must be torch.bfloat16 or torch.float32, got {dtype}")
    if packed_u8.numel() != tables["in_bytes"]:
        raise ValueError(f"qwen_image_patches: the images of sizes {tables['sizes']} hold {tables['in_bytes']} bytes, "
                         f"packed_u8 has {packed_u8.numel()}")
    dv = packed_u8.device
    if out is None:
        out = torch.empty(tables["rows"], tables["cols"], dtype=dtype, device=dv)
    _chk(out, dtype, "out")
    if tuple(out.shape) != (tables["rows"], tables["cols"]):
        raise ValueError(f"qwen_image_patches: out must be [{tables['rows']}, {tables['cols']}], got {tuple(out.shape)}")
    lut = tables["lut"][dtype]
    _chk(tables["desc"], torch.int64, "desc"); _chk(tables["tabs"], torch.int32, "tabs"); _chk(lut, torch.int32, "lut")
    assert tuple(tables["desc"].shape) == (len(tables["sizes"]), QWEN_DESC_WORDS) and lut.numel() == 3 * 256
    tmp = torch.empty(max(tables["tmp_bytes"], 4), dtype=torch.uint8, device=dv)
    _lib.call("spider_qwen_image_patches", _p(packed_u8), _p(tables["desc"]), _p(tables["tabs"]), _p(lut), _p(tmp), _p(out),
              len(tables["sizes"]), tables["patch"], tables["merge"], tables["temporal"], tables["max_h_items"], tables["max_tiles"],
              int(dtype == torch.float32), _stream())
    return out

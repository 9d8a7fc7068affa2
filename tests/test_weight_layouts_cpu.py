"""Host side of the marked-weight routes (spider_amd/ops.py), checked without a GPU:

* `tile_weight64` against the address formula the kernels use (csrc/gemm.hip: w_row_byte / w_tile_step): element
  ((n >> 6) * nk + (k >> 6)) * 4096 + (n & 63) * 64 + (k & 63) of the copy is W[n, k], nk = ceil(K / 64), every other element zero;
* `repack_fm_conv` against its docstring (piece (rg, cb * 9 + tap), lane 16 g + r = W[16 rg + r, tap, 32 cb + 8 g : + 8]);
* the cache lifecycle of `_tiled` / `_wsfm` / `prebuild_tiled`: when a copy is built, reused, rebuilt, refused under stream capture.

`_tiled` asks torch whether the current stream is capturing, which raises without a device: every case sets the answer it needs.
"""
import pytest
import torch

from spider_amd import ops

DTS = [torch.float16, torch.bfloat16]


def _w(*shape, seed=0, dt=torch.float16):
    """distinct, non-zero 16-bit values (a zero weight could hide in the padding)"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(*shape, generator=g)
    return (w + torch.where(w >= 0, 0.5, -0.5)).to(dt)


@pytest.fixture
def capturing(monkeypatch):
    """state['on'] is what torch.cuda.is_current_stream_capturing() answers"""
    state = {"on": False}
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["on"])
    return state


def _expect_tiled(W2):
    """the copy written out from the device's address formula, one element at a time (index arithmetic only)"""
    N, K = W2.shape
    nt, nk = (N + 63) // 64, (K + 63) // 64
    n = torch.arange(N)[:, None].expand(N, K)
    k = torch.arange(K)[None, :].expand(N, K)
    idx = ((n >> 6) * nk + (k >> 6)) * 4096 + (n & 63) * 64 + (k & 63)
    flat = torch.zeros(nt * nk * 4096, dtype=W2.dtype)
    flat[idx.reshape(-1)] = W2.reshape(-1)
    return flat, idx


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(64, 64), (130, 72), (1, 8), (63, 4104), (320, 3, 3, 320), (2 * 132, 1032)],
                         ids=["64x64", "130x72", "1x8", "63x4104", "conv320x3x3x320", "glu264x1032"])
def test_tile_weight64_matches_the_device_address_formula(shape, dt):
    W = _w(*shape, seed=sum(shape), dt=dt)
    W2 = W.reshape(W.shape[0], -1)                   # what _tiled hands to the packer (OHWI conv weights: K = kh * kw * Cin)
    N, K = W2.shape
    t = ops.tile_weight64(W2)
    nt, nk = (N + 63) // 64, (K + 63) // 64
    assert t.dtype == dt and t.is_contiguous()
    assert t.numel() * t.element_size() == nt * nk * 8192
    flat = t.reshape(-1)
    want, idx = _expect_tiled(W2)
    assert idx.unique().numel() == N * K             # the formula is injective: no two elements share a slot
    assert torch.equal(flat[idx.reshape(-1)], W2.reshape(-1)), "W[n, k] is not where w_row_byte / w_tile_step read it"
    assert torch.equal(flat, want), "elements outside the image of W must be zero (they replace the row-major bounds mask)"
    assert int((flat != 0).sum()) == N * K


def test_tile_weight64_of_a_conv_weight_is_built_by_tiled_from_the_flattened_taps(capturing):
    W = ops.mark_weight(_w(320, 3, 3, 320, seed=3))
    t = ops._tiled(W, 512)
    assert tuple(t.shape) == (5, 45, 64, 64)
    # row n, tap (ky, kx), channel c sits at k = (ky * 3 + kx) * 320 + c: TapWalk::wtile = tap * (Cin / 64) + c / 64
    for n, ky, kx, c in [(0, 0, 0, 0), (65, 1, 2, 70), (319, 2, 2, 319), (128, 0, 1, 64)]:
        k = (ky * 3 + kx) * 320 + c
        assert (k >> 6) == (ky * 3 + kx) * (320 >> 6) + (c >> 6)
        assert t[n >> 6, k >> 6, n & 63, k & 63] == W[n, ky, kx, c]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("Cout", [32, 48, 80])
@pytest.mark.parametrize("Cin", [32, 96])
def test_repack_fm_conv_matches_its_docstring(Cout, Cin, dt):
    W = _w(Cout, 3, 3, Cin, seed=Cout + Cin, dt=dt)
    t = ops.repack_fm_conv(W)
    Np = (Cout + 31) // 32 * 32
    assert tuple(t.shape) == (Np // 16, (Cin // 32) * 9, 64, 8) and t.dtype == dt and t.is_contiguous()
    Wt = W.reshape(Cout, 9, Cin)
    want = torch.zeros_like(t)
    for rg in range(Np // 16):
        for cb in range(Cin // 32):
            for tap in range(9):
                for g in range(4):
                    for r in range(16):
                        if 16 * rg + r < Cout:
                            want[rg, cb * 9 + tap, 16 * g + r] = Wt[16 * rg + r, tap, 32 * cb + 8 * g: 32 * cb + 8 * g + 8]
    assert torch.equal(t, want)
    assert int((t != 0).sum()) == W.numel()          # pad rows are zero, nothing is duplicated


# ------------------------------------------------------------------------------------------------ cache lifecycle
def _copy_of(W):
    return ops.tile_weight64(W.reshape(W.shape[0], -1))


BUILDERS = [("_tiled", lambda W: ops._tiled(W, 64), "_spider_tiled", _copy_of, (96, 72)),
            ("_wsfm", lambda W: ops._wsfm(W), "_spider_fm", lambda W: ops.repack_fm_conv(W), (48, 3, 3, 32))]


@pytest.fixture(params=BUILDERS, ids=[b[0] for b in BUILDERS])
def builder(request):
    return request.param


def test_unmarked_tensor_has_no_copy(builder, capturing):
    _, build, attr, _, shape = builder
    W = _w(*shape)
    assert build(W) is None and not hasattr(W, attr)


def test_rows_above_the_threshold_take_the_row_major_route(capturing):
    W = ops.mark_weight(_w(96, 72))
    assert ops._tiled(W, ops.WTILED_MAX_M + 1) is None
    assert not hasattr(W, "_spider_tiled") and not hasattr(W, "_spider_tiled_tag")
    assert ops._tiled(W, ops.WTILED_MAX_M) is not None


def test_copy_is_built_once_and_reused(builder, capturing):
    _, build, attr, fresh, shape = builder
    W = ops.mark_weight(_w(*shape))
    t = build(W)
    assert t is not None and getattr(W, attr) is t and torch.equal(t, fresh(W))
    assert build(W) is t
    capturing["on"] = True                           # an up-to-date copy is served under capture as well
    assert build(W) is t


@pytest.mark.parametrize("update", ["mul_", "copy_", "data"])
def test_in_place_update_rebuilds_the_copy(builder, capturing, update):
    _, build, attr, fresh, shape = builder
    W = ops.mark_weight(_w(*shape, seed=1))
    other = _w(*shape, seed=2)
    t0 = build(W)
    if update == "mul_":
        W.mul_(2)
    elif update == "copy_":
        W.copy_(other)
    else:
        W.data = other                               # a new storage under the same tensor object: data_ptr changes
    t1 = build(W)
    assert t1 is not t0 and getattr(W, attr) is t1
    assert torch.equal(t1, fresh(W)), "the copy served after an update must be the copy of the updated weight"
    assert not torch.equal(t1, t0)
    assert build(W) is t1


def test_first_use_under_capture_builds_nothing(builder, capturing):
    _, build, attr, _, shape = builder
    W = ops.mark_weight(_w(*shape))
    capturing["on"] = True
    assert build(W) is None                          # the call falls back to the row-major operand it was given
    assert not hasattr(W, attr) and not hasattr(W, attr + "_tag")
    capturing["on"] = False
    assert build(W) is not None


def test_stale_copy_under_capture_raises(builder, capturing):
    _, build, attr, _, shape = builder
    W = ops.mark_weight(_w(*shape))
    t0 = build(W)
    W.mul_(2)
    capturing["on"] = True
    with pytest.raises(RuntimeError, match="modified in place"):
        build(W)
    assert getattr(W, attr) is t0                    # nothing was replaced by the refused call
    capturing["on"] = False
    assert build(W) is not t0


def test_prebuild_tiled_counts_bytes_and_leaves_nothing_for_a_capture(capturing):
    lin = ops.mark_weight(_w(130, 72, seed=1))                 # 3 x 2 tiles
    conv = ops.mark_weight(_w(40, 3, 3, 32, seed=2))           # [40, 288]: 1 x 5 tiles
    glu = ops.mark_weight(_w(2 * 132, 1032, seed=3))           # 5 x 17 tiles
    unmarked = _w(64, 64, seed=4)
    vec = ops.mark_weight(_w(64, seed=5))                      # a marked bias: 1-D tensors have no copy
    n = ops.prebuild_tiled([lin, conv, unmarked, vec, glu])
    assert n == (3 * 2 + 1 * 5 + 5 * 17) * 8192
    assert not hasattr(unmarked, "_spider_tiled") and not hasattr(vec, "_spider_tiled")
    capturing["on"] = True
    for W in (lin, conv, glu):
        t = ops._tiled(W, 1)
        assert t is W._spider_tiled and torch.equal(t, _copy_of(W))
    assert ops.prebuild_tiled([lin, conv, glu]) == n           # a second pass rebuilds nothing, even under capture
    assert ops.prebuild_tiled([lin], max_rows=lin.numel() - 1) == 0


def test_writes_through_dot_data_are_not_tracked(capturing):
    """torch does not bump `_version` for an in-place operation on `W.data`, and the storage stays where it is: the tag
    (version, data_ptr) cannot see such a write. As long as that is so, mark_weight's docstring has to say it; on a torch that
    does version the write, the copy has to follow it."""
    W = ops.mark_weight(_w(96, 72))
    t0 = ops._tiled(W, 64)
    v = W._version
    W.data.mul_(2)
    t1 = ops._tiled(W, 64)
    if W._version == v:                              # untracked: the limit has to be stated where weights are marked
        assert t1 is t0
        assert "sees only in-place operations on the tensor" in " ".join(ops.mark_weight.__doc__.split())
        assert "NOT tracked" in ops.mark_weight.__doc__
    else:                                            # a torch that versions it: then the copy has to follow
        assert torch.equal(t1, _copy_of(W))

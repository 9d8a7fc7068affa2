"""fp64 parity of the pointwise and plumbing kernels of csrc/unet_ops.hip and of the embedding gather, at the edges: one thread, one
live thread in the second block, the second trip of the grid-stride loop, odd shapes, bf16 AND f16, every element against the bound
derived in tests/pointwise_checks.py (which also holds the case tables; tests/test_pointwise_checks_cpu.py shows that they bite).
Where a wrapper takes `out=`, it writes into the middle of a sentinel-filled buffer whose guards must survive."""
import pytest
import torch

import pointwise_checks as pc

pytestmark = pytest.mark.gpu

DT_IDS = [pc.name(d) for d in pc.DTYPES]
F32 = torch.float32


@pytest.fixture(scope="module")
def ops(dev):
    from spider_amd import ops as o
    return o


@pytest.fixture(scope="module")
def err():
    from spider_amd.lib import SpiderHipError
    return SpiderHipError


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    best, exc = pc.summary()
    for k in sorted(best):
        print(f"[pointwise summary] {k[0]} {k[1]} out={k[2]}: largest err / bound = {best[k]:.3f}")
    for k in sorted(exc):
        print(f"[pointwise summary] activation {k[0]} {k[1]}: largest excess over the derived bound = {exc[k]:.3e}")


# ------------------------------------------------------------------------------------------------------------------- vector elementwise
def run_vec(ops, dev, op, n, dt):
    inp = pc.vec_inputs(n, dt)
    a, b = inp["a"].to(dev), inp["b"].to(dev)
    if op[0] == "split_hilo":
        hi, lo = ops.split_hilo(inp["x32"].to(dev), dt)
        return hi.cpu(), lo.cpu()
    call = {"act": lambda o: ops.act(a, op[1], op[2] if len(op) > 2 else 0.0, out=o),
            "add": lambda o: ops.add(a, b, out=o),
            "add_scaled": lambda o: ops.add_scaled(a, b, op[1], out=o),
            "axpby": lambda o: ops.axpby(a, b, op[1], op[2], out=o)}[op[0]]
    return pc.into(pc.op_id(op), (n,), dt, dev, call)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("op", pc.VEC_OPS, ids=pc.op_id)
def test_vector_elementwise(ops, dev, op, dt):
    for n in pc.VEC_N:
        pc.vec_verify(op, n, dt, pc.vec_inputs(n, dt), run_vec(ops, dev, op, n, dt))


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_vector_elementwise_rejects(ops, dev, err, dt):
    for n in (12, 0):
        a = torch.ones(n, dtype=dt, device=dev)
        buf, _ = pc.guarded((16,), dt, dev)
        out = buf[64:64 + n]
        for call in (lambda: ops.act(a, "silu", out=out), lambda: ops.add(a, a, out=out), lambda: ops.add_scaled(a, a, 0.5, out=out),
                     lambda: ops.axpby(a, a, 1.0, 1.0, out=out), lambda: ops.split_hilo(torch.ones(n, device=dev), dt)):
            with pytest.raises(err):
                call()
        assert pc.untouched(buf), "a rejected call wrote to its output"


# ------------------------------------------------------------------------------------------------------------------- geglu / swiglu
@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kind", ["geglu", "swiglu"])
@pytest.mark.parametrize("case", pc.GLU_CASES, ids=str)
def test_glu(ops, dev, case, kind, dt):
    M, inner = case
    x = pc.glu_inputs(M, inner, dt)
    out = pc.into(kind, (M, inner), dt, dev, lambda o: getattr(ops, kind)(x.to(dev), out=o))
    pc.glu_verify(kind, M, inner, dt, x, out)


def test_glu_rejects(ops, dev, err):
    x = torch.ones(2, 24, dtype=torch.bfloat16, device=dev)       # inner = 12
    for fn in (ops.geglu, ops.swiglu):
        with pytest.raises(err):
            fn(x)


# ------------------------------------------------------------------------------------------------------------------- concat, embed
@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_concat_channels(ops, dev, err, dt):
    for case in pc.CONCAT_CASES:
        rows, C1, C2 = case
        a, b = pc.concat_inputs(*case, dt)
        out = pc.into("concat_channels", (rows, C1 + C2), dt, dev, lambda o: ops.concat_channels(a.to(dev), b.to(dev), out=o))
        pc.concat_verify(case, dt, (a, b), out)
    with pytest.raises(err):
        ops.concat_channels(torch.ones(3, 4, dtype=dt, device=dev), torch.ones(3, 8, dtype=dt, device=dev))


def test_concat_channels_f32(ops, dev):
    for case in pc.CONCAT32_CASES:
        a, b = pc.concat_inputs(*case, F32)
        pc.concat_verify(case, F32, (a, b), ops.concat_channels_f32(a.to(dev), b.to(dev)).cpu())


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_embed(ops, dev, err, dt):
    for case in pc.EMBED_CASES:
        table, ids = pc.embed_inputs(*case, dt)
        pc.embed_verify(case, dt, (table, ids), ops.embed(table.to(dev), ids.to(dev)).cpu())
    with pytest.raises(err):
        ops.embed(torch.ones(4, 12, dtype=dt, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------------------------------------------------------- short reductions
@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_mean_tokens(ops, dev, dt):
    for case in pc.MEAN_CASES:
        x = pc.mean_inputs(*case, dt)
        out = pc.into("mean_tokens", (case[0], case[2]), dt, dev, lambda o: ops.mean_tokens(x.to(dev), out=o))
        pc.mean_verify(case, dt, x, out)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_moe_combine(ops, dev, err, dt):
    for case in pc.MOE_CASES:
        xs, logits = pc.moe_inputs(*case, dt)
        out = pc.into("moe_combine", xs[0].shape, dt, dev, lambda o: ops.moe_combine([t.to(dev) for t in xs], logits.to(dev), out=o))
        pc.moe_verify(case, dt, (xs, logits), out)
    x = torch.ones(2, 8, dtype=dt, device=dev)
    with pytest.raises(err):
        ops.moe_combine([x] * 9, torch.zeros(2, 12, dtype=dt, device=dev))
    with pytest.raises((err, AssertionError)):          # the wrapper's own assertion stands in front of the library's check
        ops.moe_combine([x] * 4, torch.zeros(2, 3, dtype=dt, device=dev))
    from spider_amd import lib
    import ctypes
    lg, y = torch.zeros(2, 3, dtype=dt, device=dev), torch.empty_like(x)
    with pytest.raises(err):
        lib.call(f"spider_moe_combine_{'f16' if dt == torch.float16 else 'bf16'}", (ctypes.c_void_p * 4)(*[x.data_ptr()] * 4), 4, lg.data_ptr(), 3,
                 y.data_ptr(), 2, 8, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
def test_l2_normalize(ops, dev, err, dt):
    for case in pc.L2_CASES:
        x = pc.l2_inputs(*case, dt)
        out = pc.into("l2_normalize", x.shape, dt, dev, lambda o: ops.l2_normalize(x.to(dev), pc.L2_EPS, out=o))
        pc.l2_verify(case, dt, x, out)
    with pytest.raises(err):
        ops.l2_normalize(torch.ones(2, 8193, dtype=dt, device=dev))


@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("scale", pc.SOFTMAX_SCALES, ids=["0.3", "512^-0.5"])
def test_softmax_rows(ops, dev, scale, dt):
    for case in pc.SOFTMAX_CASES:
        rows, n, nv = case
        x = pc.softmax_inputs(*case)
        out = pc.into("softmax_rows", (rows, n), dt, dev, lambda o: ops.softmax_rows(x.to(dev), scale, n_valid=nv, out=o))
        pc.softmax_verify(case, scale, dt, x, out)


def test_softmax_rows_rejects(ops, dev, err):
    x = torch.zeros(2, 8, device=dev)
    for kw in ({"n_valid": 0}, {"n_valid": 9}, {"scale": 0.0}):
        with pytest.raises(err):
            ops.softmax_rows(x, **kw)


def test_pack_keep_bits(ops, dev):
    for case in pc.pack_cases():
        u = pc.pack_inputs(case[0])
        pc.pack_verify(case, u, ops.pack_keep_bits(u.to(dev), pc.PACK_THR, case[1]).cpu())


# ------------------------------------------------------------------------------------------------------------------- latent plumbing
@pytest.mark.parametrize("dt", pc.DTYPES + (F32,), ids=DT_IDS + ["f32"])
def test_latent_to_nhwc(ops, dev, dt):
    for case in pc.MAPS:
        B, Cn, H, W = case
        lat = pc.map_input("lat", *case)
        for reps in pc.REPS:
            for scale in pc.LATENT_SCALES:
                if dt == F32:
                    out = ops.latent_to_nhwc_f32(lat.to(dev), reps, scale).cpu()
                else:
                    out = pc.into("latent_to_nhwc", (reps * B, H, W, Cn), dt, dev, lambda o: ops.latent_to_nhwc(lat.to(dev), reps, scale, out=o))
                pc.latent_verify(case, reps, scale, dt, lat, out)


def test_cfg_lincomb_nhwc_to_nchw(ops, dev, err):
    for case in pc.MAPS:
        B, Cn, H, W = case
        e2 = pc.map_input("cfg", 2 * B, H, W, Cn)
        pc.cfg_verify(case, e2, pc.into("cfg_combine", case, F32, dev, lambda o: ops.cfg_combine(e2.to(dev), pc.GUIDANCE, out=o)))
        for coefs in pc.LINCOMB_COEFS:
            xs = [pc.map_input(f"lin{j}", *case) for j in range(len(coefs))]
            pc.lincomb_verify(case, coefs, xs, pc.into("lincomb", case, F32, dev, lambda o: ops.lincomb([x.to(dev) for x in xs], coefs, out=o)))
        for aff in pc.NCHW_AFFINES:
            x = pc.nchw_input(case)
            pc.nchw_verify(case, aff, x, pc.into("nhwc_to_nchw", case, F32, dev, lambda o: ops.nhwc_to_nchw(x.to(dev), aff[0], aff[1], aff[2], out=o)))
    x = torch.ones(8, device=dev)
    with pytest.raises(err):
        ops.lincomb([x] * 7, [1.0] * 7)


# ------------------------------------------------------------------------------------------------------------------- conv_transpose1d
@pytest.mark.parametrize("dt", pc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", pc.CT1D_CASES, ids=str)
def test_conv_transpose1d_edges(ops, dev, case, dt):
    L, Cin, Cout, k, stride, pad = case
    x, w, bias, taps = pc.ct1d_inputs(case, dt)
    for use_bias in (True, False):
        y = ops.conv_transpose1d(x.to(dev), taps.to(dev), bias.to(dev) if use_bias else None, k, stride, pad)
        pc.ct1d_verify(case, dt, (x, w, bias, taps), use_bias, y.cpu())

"""CPU: the launch sequence of LlamaEngine._decode_step, pinned. The real method runs on a fake engine whose weights and state buffers
are named sentinels, with `llm.ops` replaced by a recorder: every call is logged as op(tensor names, scalars, non-None keywords) and
returns its `out`. The expected sequences below are written out by hand, one per weight route and norm mode, and `want_routes`
restates which engine settings and row count take which; neither reads the table in spider_amd/llm.py. No GPU, no library load."""
import itertools
import types

import pytest

from spider_amd import llm as L
from spider_amd import ops as real_ops

EPS, VOCAB, N_Q, N_KV, QKV_ROWS, NSPLIT = 1e-6, 1000, 4, 2, 1024, 7
STEP_METHODS = ("_lm_head_step", "_sample_step", "_beam_step", "_decode_route")     # (whichever of them the class has)
SUFFIXES = ("", "_fm", "_q8", "_s8", "_q4", "_e4", "_q8fm", "_q4fm", "_e4fm")


class T:
    """a named stand-in for a tensor; indexing names the part, copy_ is logged like a launch"""
    def __init__(self, name, log=None, shape=None):
        self.name, self.log, self.shape = name, log, shape

    def __getitem__(self, i):
        return T(f"{self.name}[{i}]", self.log)

    def copy_(self, src):
        self.log.append(f"copy_({self.name}, {_fmt(src)})")


class D(dict):
    """a named dict (proc, sample, beam, lookup ... states), logged by its name"""
    def __init__(self, name, log, keys):
        super().__init__({k: T(f"{name}.{k}", log) for k in keys})
        self.name = name


def _fmt(v):
    if isinstance(v, (T, D)):
        return v.name
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(_fmt(x) for x in v) + ")"
    return repr(v)


class Recorder:
    """stands in for spider_amd.ops: constants and the two LDS-budget predicates are the real module's, every other name is a logged call"""
    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        if name.isupper() or name in ("w8_norm_fits", "w4_norm_fits"):
            return getattr(real_ops, name)
        assert hasattr(real_ops, name), f"ops.{name} does not exist"

        def call(*a, **kw):
            kws = [f"{k}={_fmt(v)}" for k, v in sorted(kw.items()) if v is not None]
            self.log.append(f"{name}({', '.join([_fmt(x) for x in a] + kws)})")
            return T("embed", self.log) if name == "embed" else kw.get("out")
        return call


def make(monkeypatch, weight_dtype="bf16", lm_head_dtype="bf16", bws=False, fm_batch=False, hidden=256, head_dim=128, **over):
    rec = Recorder()
    monkeypatch.setattr(L, "ops", rec)
    t = lambda n, **kw: T(n, rec.log, **kw)
    eng = types.SimpleNamespace()
    for name, v in vars(L.LlamaEngine).items():
        if name.isupper():
            setattr(eng, name, v)       # the class constants
        elif name in STEP_METHODS:
            setattr(eng, name, types.MethodType(v, eng))
    eng.FM_MIN_BATCH = 2        # (the class reads it from the environment)
    for k, v in over.items():
        setattr(eng, k, v)
    eng.cfg = types.SimpleNamespace(hidden=hidden, vocab=VOCAB, n_q=N_Q, n_kv=N_KV, head_dim=head_dim, eps=EPS, layers=1)
    eng.weight_dtype, eng.lm_head_dtype, eng.batched_weight_stream, eng.fm_batch = weight_dtype, lm_head_dtype, bws, fm_batch
    lw = {m + s: t(m + s) for m in ("w_qkv", "w_o", "w_gu", "w_down") for s in SUFFIXES}
    lw["w_qkv"].shape = (QKV_ROWS, hidden)
    lw.update(b_qkv=t("b_qkv"), ln1=t("ln1"), ln2=t("ln2"))
    eng.layers = [lw]
    for a in ("embed_w", "norm", "cos_sin", "lm_head", "lm_head_fm", "lm_head_q8", "lm_head_s8", "lm_head_q4", "lm_head_e4"):
        setattr(eng, a, t(a))
    return eng, rec


def state(rec, B, **extra):
    t = lambda n: T(n, rec.log)
    st = {k: t(k) for k in ("cur_ids", "next_ids", "pos", "slot", "kv_end", "kv_beg", "qkv", "q", "attn", "h1", "act", "xn", "attn_cnt",
                            "hist", "n_hist")}
    st.update(B=B, nsplit=NSPLIT, embeds_in=None, h2=[t("h2[0]"), t("h2[1]")], attn_ws=(t("attn_ws0"), t("attn_ws1")),
              lm_ws=(t("lm_ws0"), t("lm_ws1")), kv=(t("k_cache"), t("v_cache")))
    st.update(extra)
    return st


def run(eng, rec, st):
    del rec.log[:]
    L.LlamaEngine._decode_step(eng, st)
    return list(rec.log)


# ---------------------------------------------------------------------------------------------- the expected sequences, by hand
EMBED = ["embed(embed_w, cur_ids)"]
ATTN = {
    "fused": ["attn_decode_fused(qkv, pos, cos_sin, k_cache[0], v_cache[0], kv_end, kv_beg, attn_cnt, 4, 7, (attn_ws0, attn_ws1), attn)"],
    "split": ["rope_kv_append(qkv, pos, slot, cos_sin, q, k_cache[0], v_cache[0], {B}, 1, 4, 2, 64)",
              "attn_decode(q, k_cache[0], v_cache[0], kv_end, kv_beg=kv_beg, nsplit=7, out=attn, ws=(attn_ws0, attn_ws1))"],
    "verify": ["rope_kv_append(qkv, pos, slot, cos_sin, q, k_cache[0], v_cache[0], 1, {B}, 4, 2, 128)",
               "attn_verify(q, k_cache[0], v_cache[0], kv_end, {B}, kv_beg=kv_beg, nsplit=7, out=attn, ws=(attn_ws0, attn_ws1))"],
}
# (front of the attention, behind it); {H} = hidden
LAYER = {
    ("bf16", "arg"): (
        ["gemv(w_qkv, embed, bias=b_qkv, eps=1e-06, norm_w=ln1, out=qkv)"],
        ["gemv(w_o, attn, out=h1, res=embed)",
         "gemv_swiglu(w_gu, h1, eps=1e-06, norm_w=ln2, out=act)",
         "gemv(w_down, act, out=h2[0], res=h1)"]),
    ("bf16", "launch"): (
        ["rmsnorm(embed, ln1, 1e-06, out=xn)",
         "gemv(w_qkv, xn, bias=b_qkv, out=qkv)"],
        ["gemv(w_o, attn, out=h1, res=embed)",
         "rmsnorm(h1, ln2, 1e-06, out=xn)",
         "gemv_swiglu(w_gu, xn, out=act)",
         "gemv(w_down, act, out=h2[0], res=h1)"]),
    ("bf16_fm", "folded"): (
        ["gemv_fm(w_qkv_fm, embed, 1024, bias=b_qkv, norm_eps=1e-06, out=qkv)"],
        ["gemv_fm(w_o_fm, attn, {H}, out=h1, res=embed)",
         "gemv_swiglu_fm(w_gu_fm, h1, norm_eps=1e-06, out=act)",
         "gemv_fm(w_down_fm, act, {H}, out=h2[0], res=h1)"]),
    ("fp8", "arg"): (
        ["gemv_w8(w_qkv_q8, w_qkv_s8, embed, bias=b_qkv, eps=1e-06, norm_w=ln1, out=qkv)"],
        ["gemv_w8(w_o_q8, w_o_s8, attn, out=h1, res=embed)",
         "gemv_swiglu_w8(w_gu_q8, w_gu_s8, h1, eps=1e-06, norm_w=ln2, out=act)",
         "gemv_w8(w_down_q8, w_down_s8, act, out=h2[0], res=h1)"]),
    ("fp8", "launch"): (
        ["rmsnorm(embed, ln1, 1e-06, out=xn)",
         "gemv_w8(w_qkv_q8, w_qkv_s8, xn, bias=b_qkv, out=qkv)"],
        ["gemv_w8(w_o_q8, w_o_s8, attn, out=h1, res=embed)",
         "rmsnorm(h1, ln2, 1e-06, out=xn)",
         "gemv_swiglu_w8(w_gu_q8, w_gu_s8, xn, out=act)",
         "gemv_w8(w_down_q8, w_down_s8, act, out=h2[0], res=h1)"]),
    ("mxfp4", "arg"): (
        ["gemv_w4(w_qkv_q4, w_qkv_e4, embed, bias=b_qkv, eps=1e-06, norm_w=ln1, out=qkv)"],
        ["gemv_w4(w_o_q4, w_o_e4, attn, out=h1, res=embed)",
         "gemv_swiglu_w4(w_gu_q4, w_gu_e4, h1, eps=1e-06, norm_w=ln2, out=act)",
         "gemv_w4(w_down_q4, w_down_e4, act, out=h2[0], res=h1)"]),
    ("mxfp4", "launch"): (
        ["rmsnorm(embed, ln1, 1e-06, out=xn)",
         "gemv_w4(w_qkv_q4, w_qkv_e4, xn, bias=b_qkv, out=qkv)"],
        ["gemv_w4(w_o_q4, w_o_e4, attn, out=h1, res=embed)",
         "rmsnorm(h1, ln2, 1e-06, out=xn)",
         "gemv_swiglu_w4(w_gu_q4, w_gu_e4, xn, out=act)",
         "gemv_w4(w_down_q4, w_down_e4, act, out=h2[0], res=h1)"]),
    ("fp8_fm", "launch"): (
        ["rmsnorm(embed, ln1, 1e-06, out=xn)",
         "gemv_fm_w8(w_qkv_q8fm, w_qkv_s8, xn, 1024, bias=b_qkv, out=qkv)"],
        ["gemv_fm_w8(w_o_q8fm, w_o_s8, attn, {H}, out=h1, res=embed)",
         "rmsnorm(h1, ln2, 1e-06, out=xn)",
         "gemv_swiglu_fm_w8(w_gu_q8fm, w_gu_s8, xn, out=act)",
         "gemv_fm_w8(w_down_q8fm, w_down_s8, act, {H}, out=h2[0], res=h1)"]),
    ("mxfp4_fm", "launch"): (
        ["rmsnorm(embed, ln1, 1e-06, out=xn)",
         "gemv_fm_w4(w_qkv_q4fm, w_qkv_e4fm, xn, 1024, bias=b_qkv, out=qkv)"],
        ["gemv_fm_w4(w_o_q4fm, w_o_e4fm, attn, {H}, out=h1, res=embed)",
         "rmsnorm(h1, ln2, 1e-06, out=xn)",
         "gemv_swiglu_fm_w4(w_gu_q4fm, w_gu_e4fm, xn, out=act)",
         "gemv_fm_w4(w_down_q4fm, w_down_e4fm, act, {H}, out=h2[0], res=h1)"]),
}
# the greedy head (other ids buffers, logits and processors are spelled out in the cases further down)
HEAD = {
    ("bf16", "arg"): ["lm_head_argmax(lm_head, h2[0], eps=1e-06, norm_w=norm, out_ids=next_ids, ws=(lm_ws0, lm_ws1))"],
    ("bf16_fm", "folded"): ["lm_head_argmax_fm(lm_head_fm, h2[0], 1000, norm_eps=1e-06, out_ids=next_ids, ws=(lm_ws0, lm_ws1))"],
    ("fp8", "arg"): ["lm_head_argmax_w8(lm_head_q8, lm_head_s8, h2[0], eps=1e-06, norm_w=norm, out_ids=next_ids, ws=(lm_ws0, lm_ws1))"],
    ("fp8", "launch"): ["rmsnorm(h2[0], norm, 1e-06, out=xn)",
                        "lm_head_argmax_w8(lm_head_q8, lm_head_s8, xn, eps=1e-06, out_ids=next_ids, ws=(lm_ws0, lm_ws1))"],
    ("mxfp4", "arg"): ["lm_head_argmax_w4(lm_head_q4, lm_head_e4, h2[0], eps=1e-06, norm_w=norm, out_ids=next_ids, ws=(lm_ws0, lm_ws1))"],
    ("mxfp4", "launch"): ["rmsnorm(h2[0], norm, 1e-06, out=xn)",
                          "lm_head_argmax_w4(lm_head_q4, lm_head_e4, xn, eps=1e-06, out_ids=next_ids, ws=(lm_ws0, lm_ws1))"],
}
ADVANCE = ["decode_advance(next_ids, cur_ids, pos, slot, kv_end, hist, n_hist)"]


def layer_seq(route, hidden, attn="fused", B=1):
    front, back = LAYER[route]
    return [s.format(H=hidden, B=B) for s in front + ATTN[attn] + back]


def want_routes(e, B):
    """which (route, norm mode) the layers and the head of a B-row step take, restated from the engine's documentation: the
    quantised row-major stream inside its row range; above it the quantised fragment-major stream of a batched_weight_stream
    engine; else bf16, fragment-major from FM_MIN_BATCH rows of an engine that has the copies. The row-major kernels take the
    norm as an argument up to 4 rows (the quantised ones while the rows fit their LDS budget), the bf16 fragment-major copies
    carry it, everything else runs it as a launch. The head: its own quantised stream inside its row range, else the bf16 route."""
    H = e.cfg.hidden
    bf16_fm = e.fm_batch and B >= e.FM_MIN_BATCH
    fits = {"fp8": real_ops.w8_norm_fits, "mxfp4": real_ops.w4_norm_fits}
    rows = {"fp8": min(e.FP8_MAX_ROWS, real_ops.W8_MAX_ROWS), "mxfp4": min(e.MXFP4_MAX_ROWS, real_ops.W4_MAX_ROWS)}
    fm_rows = {"fp8": min(e.FP8_FM_MAX_ROWS, real_ops.QFM_MAX_ROWS), "mxfp4": min(e.MXFP4_FM_MAX_ROWS, real_ops.QFM_MAX_ROWS)}
    head_rows = {"fp8": min(e.LM_HEAD_FP8_MAX_ROWS, real_ops.LM_HEAD_Q_MAX_ROWS),
                 "mxfp4": min(e.LM_HEAD_MXFP4_MAX_ROWS, real_ops.LM_HEAD_Q_MAX_ROWS)}
    bf16 = ("bf16_fm", "folded") if bf16_fm else ("bf16", "arg" if B <= 4 else "launch")
    wd, hd = e.weight_dtype, e.lm_head_dtype
    layer = head = bf16
    if wd != "bf16" and B <= rows[wd]:
        layer = (wd, "arg" if fits[wd](B, H) else "launch")
    elif wd != "bf16" and e.batched_weight_stream and B <= fm_rows[wd]:
        layer = (wd + "_fm", "launch")
    if hd != "bf16" and B <= head_rows[hd]:
        head = (hd, "arg" if fits[hd](B, H) else "launch")
    elif not bf16_fm:
        head = ("bf16", "arg")      # (the row-major lm_head takes the norm as an argument at every row count)
    return layer, head


# ---------------------------------------------------------------------------------------------- the grid
FORCED = dict(FP8_MAX_ROWS=4, MXFP4_MAX_ROWS=4, LM_HEAD_FP8_MAX_ROWS=4, LM_HEAD_MXFP4_MAX_ROWS=4)
DTYPES = ("bf16", "fp8", "mxfp4")


def test_the_large_hidden_size_splits_rows_3_and_4():
    for fits in (real_ops.w8_norm_fits, real_ops.w4_norm_fits):
        assert fits(3, 20480) and not fits(4, 20480) and fits(4, 256)
        assert not any(fits(3, h) and not fits(4, h) for h in range(2048, 20480, 2048)), "20480 is the smallest such multiple of 2048"


@pytest.mark.parametrize("hidden, over", [(256, {}), (20480, FORCED)], ids=["h256", "h20480-forced4"])
@pytest.mark.parametrize("weight_dtype", DTYPES)
@pytest.mark.parametrize("lm_head_dtype", DTYPES)
def test_greedy_step_over_the_grid(monkeypatch, weight_dtype, lm_head_dtype, hidden, over):
    seen = set()
    for bws, fm_batch, B in itertools.product((False, True), (False, True), range(1, 9)):
        eng, rec = make(monkeypatch, weight_dtype, lm_head_dtype, bws, fm_batch, hidden, **over)
        layer, head = want_routes(eng, B)
        got = run(eng, rec, state(rec, B))
        assert got == EMBED + layer_seq(layer, hidden) + HEAD[head] + ADVANCE, (bws, fm_batch, B, layer, head, got)
        seen.add((layer, head))
    # the grid reaches what it is meant to reach
    routes = {l for l, _ in seen}
    assert {("bf16", "launch"), ("bf16_fm", "folded")} <= routes
    if weight_dtype == "bf16":
        assert ("bf16", "arg") in routes
    else:
        assert {(weight_dtype, "arg"), (weight_dtype + "_fm", "launch")} <= routes
        assert ((weight_dtype, "launch") in routes) == (hidden == 20480)
    heads = {h for _, h in seen}
    assert {("bf16", "arg"), ("bf16_fm", "folded")} <= heads
    if lm_head_dtype != "bf16":
        assert (lm_head_dtype, "arg") in heads and ((lm_head_dtype, "launch") in heads) == (hidden == 20480)


def test_every_written_sequence_is_reached(monkeypatch):
    seen_l, seen_h = set(), set()
    for hidden, over in ((256, {}), (20480, FORCED)):
        for wd, hd, bws, fmb, B in itertools.product(DTYPES, DTYPES, (False, True), (False, True), range(1, 9)):
            eng, _ = make(monkeypatch, wd, hd, bws, fmb, hidden, **over)
            layer, head = want_routes(eng, B)
            seen_l.add(layer); seen_h.add(head)
    assert seen_l == set(LAYER) and seen_h == set(HEAD)


# ---------------------------------------------------------------------------------------------- the order of the arms, as it is today
def test_mxfp4_at_4_rows_with_fm_copies_streams_the_layers_and_takes_the_fragment_major_head(monkeypatch):
    eng, rec = make(monkeypatch, "mxfp4", "bf16", fm_batch=True)
    assert eng.MXFP4_MAX_ROWS == 4
    got = run(eng, rec, state(rec, 4))
    assert got == EMBED + layer_seq(("mxfp4", "arg"), 256) + HEAD[("bf16_fm", "folded")] + ADVANCE


def test_an_instance_override_after_construction_changes_the_next_step(monkeypatch):
    eng, rec = make(monkeypatch, "mxfp4", "mxfp4", fm_batch=True)
    st = state(rec, 3)
    assert run(eng, rec, st) == EMBED + layer_seq(("mxfp4", "arg"), 256) + HEAD[("mxfp4", "arg")] + ADVANCE
    eng.MXFP4_MAX_ROWS = 2
    assert run(eng, rec, st) == EMBED + layer_seq(("bf16_fm", "folded"), 256) + HEAD[("mxfp4", "arg")] + ADVANCE
    eng.LM_HEAD_MXFP4_MAX_ROWS = 0
    assert run(eng, rec, st) == EMBED + layer_seq(("bf16_fm", "folded"), 256) + HEAD[("bf16_fm", "folded")] + ADVANCE
    eng.MXFP4_MAX_ROWS = 3
    assert run(eng, rec, st) == EMBED + layer_seq(("mxfp4", "arg"), 256) + HEAD[("bf16_fm", "folded")] + ADVANCE


def test_an_op_wrapped_after_construction_is_the_one_called(monkeypatch):
    eng, rec = make(monkeypatch, "mxfp4", "fp8")
    st = state(rec, 2)
    plain = run(eng, rec, st)
    calls = []
    inner_w4, inner_head = rec.gemv_w4, rec.lm_head_argmax_w8
    rec.gemv_w4 = lambda *a, **kw: (calls.append("gemv_w4"), inner_w4(*a, **kw))[1]
    rec.lm_head_argmax_w8 = lambda *a, **kw: (calls.append("lm_head_argmax_w8"), inner_head(*a, **kw))[1]
    assert run(eng, rec, st) == plain
    assert calls == ["gemv_w4"] * 3 + ["lm_head_argmax_w8"]


# ---------------------------------------------------------------------------------------------- the request kinds, one route each
PROC_KEYS = ("seen", "ban", "penalty", "min_new", "eos_ids", "n_eos", "n_hist")


def test_processed_request(monkeypatch):
    eng, rec = make(monkeypatch, "fp8", "fp8")
    got = run(eng, rec, state(rec, 2, proc=D("proc", rec.log, PROC_KEYS), seen=T("seen")))
    assert got == EMBED + layer_seq(("fp8", "arg"), 256) + [
        "lm_head_argmax_proc_w8(lm_head_q8, lm_head_s8, h2[0], proc, eps=1e-06, norm_w=norm, out_ids=next_ids, ws=(lm_ws0, lm_ws1))",
        "decode_advance_seen(next_ids, cur_ids, pos, slot, kv_end, seen, 1000, hist, n_hist)"]


@pytest.mark.parametrize("lm_head_dtype, fm_batch, head", [
    ("bf16", False, ["lm_head_argmax_proc(lm_head, h2[0], proc, eps=1e-06, logits=logits, norm_w=norm, out_ids=next_ids, ws=(lm_ws0, lm_ws1))"]),
    ("bf16", True, ["lm_head_argmax_fm_proc(lm_head_fm, h2[0], 1000, proc, logits=logits, norm_eps=1e-06, out_ids=next_ids, ws=(lm_ws0, lm_ws1))"]),
    ("mxfp4", True, ["lm_head_argmax_proc_w4(lm_head_q4, lm_head_e4, h2[0], proc, eps=1e-06, logits=logits, norm_w=norm, out_ids=next_ids, "
                     "ws=(lm_ws0, lm_ws1))"]),
])
def test_processed_request_with_logits_on_the_other_heads(monkeypatch, lm_head_dtype, fm_batch, head):
    eng, rec = make(monkeypatch, "bf16", lm_head_dtype, fm_batch=fm_batch)
    got = run(eng, rec, state(rec, 2, proc=D("proc", rec.log, PROC_KEYS), seen=T("seen"), logits=T("logits")))
    layer = ("bf16_fm", "folded") if fm_batch else ("bf16", "arg")
    assert got == EMBED + layer_seq(layer, 256) + head + ["decode_advance_seen(next_ids, cur_ids, pos, slot, kv_end, seen, 1000, hist, n_hist)"]


def test_processed_head_with_the_norm_in_its_own_launch(monkeypatch):
    eng, rec = make(monkeypatch, "bf16", "fp8", hidden=20480, **FORCED)
    got = run(eng, rec, state(rec, 4, proc=D("proc", rec.log, PROC_KEYS), seen=T("seen")))
    assert got == EMBED + layer_seq(("bf16", "arg"), 20480) + [
        "rmsnorm(h2[0], norm, 1e-06, out=xn)",
        "lm_head_argmax_proc_w8(lm_head_q8, lm_head_s8, xn, proc, eps=1e-06, out_ids=next_ids, ws=(lm_ws0, lm_ws1))",
        "decode_advance_seen(next_ids, cur_ids, pos, slot, kv_end, seen, 1000, hist, n_hist)"]


def test_ngram_request(monkeypatch):
    eng, rec = make(monkeypatch, "bf16", "bf16", fm_batch=True)
    st = state(rec, 1, proc=D("proc", rec.log, PROC_KEYS), seen=T("seen"), ngram_bufs=D("ngram_bufs", rec.log, ("ngram",)))
    assert run(eng, rec, st) == EMBED + layer_seq(("bf16", "arg"), 256) + [
        "lm_head_argmax_proc(lm_head, h2[0], proc, eps=1e-06, norm_w=norm, out_ids=next_ids, ws=(lm_ws0, lm_ws1))",
        "decode_advance_seen_ngram(next_ids, cur_ids, pos, slot, kv_end, seen, 1000, hist, n_hist, ngram_bufs)"]


def test_sampling_request(monkeypatch):
    eng, rec = make(monkeypatch, "mxfp4", "mxfp4")
    st = state(rec, 3, sample=D("sample", rec.log, ("lm_ids",)), proc=D("proc", rec.log, PROC_KEYS), seen=T("seen"), logits=T("logits"))
    assert run(eng, rec, st) == EMBED + layer_seq(("mxfp4", "arg"), 256) + [
        "lm_head_argmax_w4(lm_head_q4, lm_head_e4, h2[0], eps=1e-06, logits=logits, norm_w=norm, out_ids=sample.lm_ids, ws=(lm_ws0, lm_ws1))",
        "sample_partial(logits, sample, proc)",
        "sample_select(sample, n_hist, next_ids, 1000)",
        "decode_advance_seen(next_ids, cur_ids, pos, slot, kv_end, seen, 1000, hist, n_hist)"]


def test_beam_request(monkeypatch):
    eng, rec = make(monkeypatch, "fp8", "bf16", bws=True, fm_batch=True)
    bm = D("beam", rec.log, ("lm_ids", "ws", "run", "eos_ids", "n_eos", "trace", "src_beam"))
    bm.update(K=3, C=6, kv_tmp=(T("kv_tmp0"), T("kv_tmp1")))
    st = state(rec, 6, beam=bm, logits=T("logits"))
    assert run(eng, rec, st) == EMBED + layer_seq(("fp8_fm", "launch"), 256) + [
        "lm_head_argmax_fm(lm_head_fm, h2[0], 1000, logits=logits, norm_eps=1e-06, out_ids=beam.lm_ids, ws=(lm_ws0, lm_ws1))",
        "beam_partial(logits, 6, beam.ws)",
        "beam_select(beam.ws, beam.run, beam.eos_ids, beam.n_eos, n_hist, beam.trace, beam.src_beam, next_ids, 1000, 6)",
        "kv_row_gather(k_cache, v_cache, kv_tmp0, kv_tmp1, beam.src_beam, kv_beg, kv_end, 3)",
        "decode_advance(next_ids, cur_ids, pos, slot, kv_end, hist, n_hist)"]


def test_prompt_lookup_request(monkeypatch):
    eng, rec = make(monkeypatch, "mxfp4", "fp8", bws=True, fm_batch=True)
    st = state(rec, 6, lookup=D("lookup", rec.log, ()))
    assert run(eng, rec, st) == EMBED + layer_seq(("mxfp4_fm", "launch"), 256, "verify", 6) + [
        "lm_head_argmax_fm(lm_head_fm, h2[0], 1000, norm_eps=1e-06, out_ids=next_ids, ws=(lm_ws0, lm_ws1))",
        "spec_advance_draft(lookup, hist, n_hist)"]


def test_assisted_request_at_2_rows_and_at_1(monkeypatch):
    eng, rec = make(monkeypatch, "bf16", "fp8", fm_batch=True)
    st = state(rec, 2, assist=D("assist", rec.log, ()))
    assert run(eng, rec, st) == EMBED + layer_seq(("bf16_fm", "folded"), 256, "verify", 2) + HEAD[("fp8", "arg")]
    st = state(rec, 1, assist=D("assist", rec.log, ()))      # the draft engine's single-row step: an ordinary row
    assert run(eng, rec, st) == EMBED + layer_seq(("bf16", "arg"), 256) + HEAD[("fp8", "arg")]


def test_hidden_states_request_and_given_embeddings(monkeypatch):
    eng, rec = make(monkeypatch, "fp8", "bf16")
    st = state(rec, 1, hidden_buf=T("hidden_buf", rec.log), embeds_in=T("embeds_in", rec.log))
    want = [s.replace("embed", "embeds_in") for s in layer_seq(("fp8", "arg"), 256)]
    assert run(eng, rec, st) == ["copy_(hidden_buf[0], embeds_in)"] + want + ["copy_(hidden_buf[1], h2[0])"] + HEAD[("bf16", "arg")] + [
        "rmsnorm(h2[0], norm, 1e-06, out=hidden_buf[1])"] + ADVANCE


def test_head_dim_64_takes_the_two_launch_attention(monkeypatch):
    eng, rec = make(monkeypatch, "bf16", "bf16", head_dim=64)
    assert run(eng, rec, state(rec, 5)) == EMBED + layer_seq(("bf16", "launch"), 256, "split", 5) + HEAD[("bf16", "arg")] + ADVANCE

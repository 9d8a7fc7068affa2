"""Quality of the opt-in quantised weight streams, measured by LlamaEngine.score: one bf16 engine and the weight_dtype="fp8" /
"mxfp4" engines (each without and with the matching lm_head_dtype) on the SAME weights score the same token sequences; the table
is perplexity, delta NLL against bf16, mean KL(bf16 || quantised) per scored token and top-1 agreement with the bf16 engine.

    python scripts/quant_quality.py --path CKPT --tokens FILE [--out FILE]        a checkpoint directory and real token ids
    python scripts/quant_quality.py --shapes qwen25_7b [--out FILE]               true shapes, random weights, random ids

--tokens: a .pt / .npy / .json file holding a [N, S] integer array (or a list of equally long id lists). Without it the ids are
uniform random, and with random weights NOTHING here says anything about text: the synthetic run records how far the formats move
the output distribution of a random network of the true shapes, on the device instead of on toy heads on the host.
--calibrate FILE [--damp D]: also the "mxfp4 (gptq)" rows, without and with the calibrated head: the MXFP4 codes chosen by GPTQ on
the token ids of FILE (same formats; `LlamaEngine(calibration=...)`). FILE "random" draws --seqs sequences of uniform random ids
with another seed than the scored ones. The scored sequences have to be disjoint from the calibration sequences: the rows
measure held-out tokens.
The quantised engines are built one after the other from the bf16 engine's own tensors (a quantised engine is exactly a bf16 model
on W_eff, which is what the scoring pass multiplies), so at most two engines are alive at once."""
import argparse
import json
import sys

import torch

from spider_amd.llm import LlamaEngine, LLMConfig

ap = argparse.ArgumentParser()
ap.add_argument("--path", default=None, help="HF checkpoint directory")
ap.add_argument("--shapes", default=None, choices=("qwen25_7b", "llama3_8b"), help="random weights of these shapes instead of a checkpoint")
ap.add_argument("--tokens", default=None, help="[N, S] token ids (.pt / .npy / .json)")
ap.add_argument("--seqs", type=int, default=4, help="random sequences when --tokens is not given")
ap.add_argument("--len", type=int, default=512, dest="seq_len", help="their length")
ap.add_argument("--layers", type=int, default=None, help="--shapes only: keep this many layers (a quicker synthetic run)")
ap.add_argument("--calibrate", default=None, help='[n, S] token ids to calibrate the "mxfp4 (gptq)" rows on (a file as --tokens, or "random")')
ap.add_argument("--damp", type=float, default=0.01, help="GPTQ damping of --calibrate")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()
if (args.path is None) == (args.shapes is None):
    ap.error("give exactly one of --path and --shapes")

dev = torch.device("cuda:0")
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


def load_tokens(path):
    if path.endswith(".pt"):
        t = torch.load(path)
    elif path.endswith(".npy"):
        import numpy as np
        t = torch.from_numpy(np.load(path))
    else:
        t = torch.tensor(json.load(open(path)))
    return t.to(torch.int64).view(-1, t.shape[-1])


def hf_weights(eng):
    """the bf16 engine's tensors under their checkpoint names (views, no copy beyond the per-layer split)"""
    c = eng.cfg
    qd, kd = c.n_q * c.head_dim, c.n_kv * c.head_dim
    w = {"model.embed_tokens.weight": eng.embed_w, "model.norm.weight": eng.norm}
    if not eng._head_tied:
        w["lm_head.weight"] = eng.lm_head
    for l, lw in enumerate(eng.layers):
        p = f"model.layers.{l}."
        for n, a, b in (("q_proj", 0, qd), ("k_proj", qd, qd + kd), ("v_proj", qd + kd, qd + 2 * kd)):
            w[p + f"self_attn.{n}.weight"] = lw["w_qkv"][a:b]
            if lw["b_qkv"] is not None:
                w[p + f"self_attn.{n}.bias"] = lw["b_qkv"][a:b]
        w[p + "self_attn.o_proj.weight"] = lw["w_o"]
        w[p + "mlp.gate_proj.weight"], w[p + "mlp.up_proj.weight"] = lw["w_gu"][:c.inter], lw["w_gu"][c.inter:]
        w[p + "mlp.down_proj.weight"] = lw["w_down"]
        w[p + "input_layernorm.weight"], w[p + "post_attention_layernorm.weight"] = lw["ln1"], lw["ln2"]
    return w


if args.tokens:
    tokens = load_tokens(args.tokens)
else:
    tokens = None
S = tokens.shape[1] if tokens is not None else args.seq_len
if args.path:
    base = LlamaEngine.from_pretrained(args.path, dev, max_batch=1, max_len=S)
    what = f"checkpoint {args.path}"
else:
    import dataclasses
    cfg = getattr(LLMConfig, args.shapes)()
    if args.layers:
        cfg = dataclasses.replace(cfg, layers=args.layers)
    base = LlamaEngine.random_init(cfg, dev, max_batch=1, max_len=S, seed=0)
    what = f"RANDOM weights N(0, 0.02^2) of the {args.shapes} shapes ({cfg.layers} layers)"
cfg = base.cfg
if tokens is None:
    tokens = torch.randint(0, cfg.vocab, (args.seqs, S), generator=torch.Generator().manual_seed(0))
    what += f"; {args.seqs} sequences of {S} uniform random ids"
else:
    what += f"; {tokens.shape[0]} sequences of {S} ids from {args.tokens}"
if args.path is None or args.tokens is None:
    say("Random weights and random ids say nothing about text: these figures measure how far the number formats move the output "
        "distribution of a network of the true shapes, not the quality of any model.")
cal_tokens = None
if args.calibrate:
    if args.calibrate == "random":
        cal_tokens = torch.randint(0, cfg.vocab, (args.seqs, S), generator=torch.Generator().manual_seed(1))
        what += f"; calibration: {args.seqs} sequences of {S} uniform random ids of another seed"
    else:
        cal_tokens = load_tokens(args.calibrate)
        what += f"; calibration: {cal_tokens.shape[0]} sequences of {cal_tokens.shape[1]} ids from {args.calibrate}"
    scored = {tuple(r) for r in tokens.tolist()}
    if any(tuple(r) in scored for r in cal_tokens.tolist()):
        ap.error("--calibrate: a calibration sequence is also a scored sequence; the gptq rows have to be scored on held-out tokens")
say(what)


def run(eng, other=None):
    """token-weighted totals over the sequences, one per call (max_batch = 1)"""
    nll = kl = agree = 0.0
    n = 0
    for s in range(tokens.shape[0]):
        o = eng.score(input_ids=tokens[s:s + 1], other=other)
        nll += o.loss * o.n_tokens
        n += o.n_tokens
        if other is not None:
            kl += o.mean_kl * o.n_tokens
            agree += o.top1_agree * o.n_tokens
    return nll / n, kl / n, agree / n, n


import math
nll0, _, _, n = run(base)
rows = [("bf16", "bf16", nll0, 0.0, 1.0)]
weights = hf_weights(base)
for wd, hd in (("fp8", "bf16"), ("fp8", "fp8"), ("mxfp4", "bf16"), ("mxfp4", "mxfp4")):
    eng = LlamaEngine(cfg, weights, dev, max_batch=1, max_len=S, weight_dtype=wd, lm_head_dtype=hd)
    nll, kl, agree, _ = run(eng, other=base)
    rows.append((wd, hd, nll, kl, agree))
    say(f"  {wd} / head {hd}: NLL {nll:.5f}  mean KL {kl:.5f}  top-1 agreement {agree:.4f}")
    del eng
    torch.cuda.empty_cache()
if cal_tokens is not None:
    for hd in ("bf16", "mxfp4"):
        eng = LlamaEngine(cfg, weights, dev, max_batch=1, max_len=max(S, cal_tokens.shape[1]), weight_dtype="mxfp4", lm_head_dtype=hd,
                          calibration=dict(input_ids=cal_tokens, damp=args.damp))
        worst = max(eng.calibration["matrices"], key=lambda m: m[3] / m[2])
        nll, kl, agree, _ = run(eng, other=base)
        rows.append(("mxfp4 (gptq)", hd + (" (gptq)" if hd == "mxfp4" else ""), nll, kl, agree))
        say(f"  mxfp4 (gptq) / head {hd}: NLL {nll:.5f}  mean KL {kl:.5f}  top-1 agreement {agree:.4f}   [{eng.calibration['n_tokens']} calibration "
            f"tokens; proxy loss gptq / rtn between {min(m[3] / m[2] for m in eng.calibration['matrices']):.3f} and {worst[3] / worst[2]:.3f} "
            f"(layer {worst[0]} {worst[1]})]")
        del eng
        torch.cuda.empty_cache()
say("")
say(f"{n} scored tokens; KL(bf16 || engine) and top-1 agreement are against the bf16 engine on the same positions")
say("| weight_dtype | lm_head_dtype | perplexity | NLL | delta NLL vs bf16 | mean KL | top-1 agreement |")
say("|---|---|---|---|---|---|---|")
for wd, hd, nll, kl, agree in rows:
    say(f"| {wd} | {hd} | {math.exp(min(nll, 700.0)):.2f} | {nll:.5f} | {nll - nll0:+.5f} | {kl:.5f} | {agree:.4f} |")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
sys.exit(0)

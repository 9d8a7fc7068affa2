"""CPU reference for tests/test_llm_gptq_gpu.py: the definition `llm.quantize_mxfp4_gptq` applied to the test's tiny model through
transformers' LlamaForCausalLM (fp32 arithmetic on the bf16-valued weights), in the order LlamaEngine's calibration pass takes:
per layer qkv (one Hessian), o, gate / up (one Hessian), down, then the lm_head, each matrix on the Hessian of what it sees behind
the matrices already quantised. Prints the mean KL to the unquantised model on the calibration tokens for round-to-nearest MXFP4
and for the calibrated codes, and their ratio -- the figure the test's docstring quotes.

    python scripts/exp/gptq_reference_kl.py [--seed 31] [--std 0.08]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.llama import LlamaCfg, LlamaOracle                                        # noqa: E402
from spider_amd.llm import dequantize_mxfp4, quantize_mxfp4, quantize_mxfp4_gptq      # noqa: E402


def hf_model(ocfg, w):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=ocfg.vocab, hidden_size=ocfg.hidden, intermediate_size=ocfg.inter, num_hidden_layers=ocfg.layers,
                      num_attention_heads=ocfg.n_q, num_key_value_heads=ocfg.n_kv, head_dim=ocfg.head_dim, rms_norm_eps=ocfg.eps,
                      rope_theta=ocfg.rope_theta, max_position_embeddings=ocfg.max_pos, tie_word_embeddings=False, attention_bias=False)
    m = LlamaForCausalLM(cfg).eval().float()
    missing, unexpected = m.load_state_dict({k: v.float() for k, v in w.items()}, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    return m


def mean_kl(ref_logits, logits):
    """KL(ref || model) over the positions that have a next token (what LlamaEngine.score averages)"""
    p = torch.log_softmax(ref_logits[:, :-1].double(), -1)
    q = torch.log_softmax(logits[:, :-1].double(), -1)
    return float((p.exp() * (p - q)).sum(-1).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--std", type=float, default=0.08)
    ap.add_argument("--damp", type=float, default=0.01)
    a = ap.parse_args()
    ocfg = LlamaCfg(256, 2, 2, 1, 128, 512, 512, 10000.0, None, 1e-6, False, 256)
    w = LlamaOracle.random_weights(ocfg, seed=a.seed, std=a.std)
    ids = torch.randint(0, 512, (8, 128), generator=torch.Generator().manual_seed(1000 + a.seed))
    rtn_round = lambda W: dequantize_mxfp4(*quantize_mxfp4(W), dtype=torch.float32)
    with torch.no_grad():
        ref = hf_model(ocfg, w)(input_ids=ids).logits
        # round to nearest: every projection and the head
        proj = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
        w_rtn = {k: (rtn_round(v) if (k.split(".")[-2] in proj or k == "lm_head.weight") else v) for k, v in w.items()}
        kl_rtn = mean_kl(ref, hf_model(ocfg, w_rtn)(input_ids=ids).logits)
        # calibrated, sequentially
        m = hf_model(ocfg, w)

        def hessian_at(module):
            got = []
            h = module.register_forward_pre_hook(lambda mod, args: got.append(args[0].detach()))
            m(input_ids=ids)
            h.remove()
            x = got[0].reshape(-1, got[0].shape[-1]).double()
            return x.t() @ x

        def calibrate(mods):
            H = hessian_at(mods[0])
            W = torch.cat([x.weight.data for x in mods], 0)
            Q = dequantize_mxfp4(*quantize_mxfp4_gptq(W, H, a.damp), dtype=torch.float32)
            o = 0
            for x in mods:
                x.weight.data.copy_(Q[o:o + x.weight.shape[0]])
                o += x.weight.shape[0]
        for layer in m.model.layers:
            at, mlp = layer.self_attn, layer.mlp
            calibrate([at.q_proj, at.k_proj, at.v_proj])
            calibrate([at.o_proj])
            calibrate([mlp.gate_proj, mlp.up_proj])
            calibrate([mlp.down_proj])
        calibrate([m.lm_head])
        kl_cal = mean_kl(ref, m(input_ids=ids).logits)
    print(f"seed {a.seed} std {a.std} damp {a.damp}: mean KL to the unquantised model on the calibration tokens: round to nearest "
          f"{kl_rtn:.5f}, calibrated {kl_cal:.5f}, ratio {kl_cal / kl_rtn:.3f}")


if __name__ == "__main__":
    main()

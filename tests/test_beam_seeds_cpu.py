"""CPU: the models of tests/test_llm_beam_gpu.py tell histories apart, measured with the figure that test asserts. Beam search is
restated on the fp32 oracle (teacher-forced logits, tests/beam_checks.beam_step_host). The GPU test requires, for every final
running beam, relative L2 < BOUND between the engine's logits along the beam's back-pointer chain [N, V] and the oracle's
teacher-forced logits of the same tokens. Here the same chain-wide figure is computed with two final beams' histories swapped --
beam i's chain of logits against the teacher-forced logits of beam j's tokens -- for every pair of final beams of a batch row whose
histories differ: it has to be at least 10 * BOUND, for every configuration and input mode the GPU test uses. Seeds are kept only
where it is (measured on the kept ones: 0.28 .. 1.2)."""
import pytest
import torch

from beam_checks import beam_step_host
from test_llm_beam_gpu import BOUND, CONFIGS, N, S, V


def _teacher(orc, ids_row, am_row, toks):
    """fp32 oracle logits [len(toks), V] that choose toks[0], toks[1], ...: one forward over prompt + toks[:-1]"""
    ids = torch.cat([ids_row, torch.tensor(toks[:-1], dtype=torch.long)])[None]
    am = torch.cat([am_row, torch.ones(len(toks) - 1, dtype=torch.long)])[None]
    lg, _, _ = orc.forward(ids, (am.cumsum(-1) - 1).clamp(min=0), None, am)
    return lg[0, S - 1:]


@pytest.mark.parametrize("mode", ["ids", "embeds"])
@pytest.mark.parametrize("B,K,seed,layers", CONFIGS)
def test_swapping_two_final_beams_histories_moves_the_chain_figure(B, K, seed, layers, mode):
    from oracle.llama import LlamaCfg, LlamaOracle
    ocfg = LlamaCfg(256, layers, 2, 1, 128, 512, V, 10000.0, None, 1e-6, False, 256)
    orc = LlamaOracle(ocfg, LlamaOracle.random_weights(ocfg, seed=seed, std=0.08))
    ids = torch.randint(3, V, (B, S), generator=torch.Generator().manual_seed(100 + seed))     # = _inputs of the GPU test
    am = torch.ones(B, S, dtype=torch.long)
    if mode == "ids":
        for b in range(B):
            ids[b, :2 + b] = 0
            am[b, :2 + b] = 0
    for b in range(B):
        seqs = [[] for _ in range(K)]
        run = torch.zeros(1, K)
        run[:, 1:] = -1e9
        for t in range(N):
            lg = torch.stack([_teacher(orc, ids[b], am[b], seqs[k] + [0])[-1] for k in range(K)])
            _, (run, src, tok) = beam_step_host(lg.bfloat16().float(), run, 2 * K, None)
            seqs = [seqs[int(src[0, k])] + [int(tok[0, k])] for k in range(K)]
        ref = [_teacher(orc, ids[b], am[b], s) for s in seqs]       # [N, V] per final beam
        swapped = [float((ref[i] - ref[j]).norm() / ref[j].norm()) for i in range(K) for j in range(K)
                   if i != j and seqs[i][:-1] != seqs[j][:-1]]
        assert swapped and min(swapped) >= 10 * BOUND, (b, swapped)

// What the kernels behind the lm_head share (llm_decode.hip, beam_search.hip, sample.hip):
//   * HF's deterministic logits processors as the arg-max epilogue applies them (LmProc, lm_proc_flags, lm_proc_apply);
//   * the total order of (fp32 value, index) pairs as 64-bit keys and the block-wide "best C, one per round" selection on them.
#pragma once
#include "common.hpp"

namespace spider {

// HF's deterministic logits processors, applied to the bf16-rounded logit widened to fp32 -- the value transformers hands to its
// processors (generation/logits_process.py: RepetitionPenalty, NoBadWords / SuppressTokens, MinLength / MinNewTokensLength):
//   bit n of seen[b] set:          lv = lv < 0 ? lv * p : lv / p     (fp32, IEEE division)
//   bit n of ban[b] set:           lv = -inf
//   n an EOS id, n_hist[b] < min_new:  lv = -inf
// Every parameter lives in device memory (one captured decode graph serves requests with different values); the bitmaps are
// uint32 [B, words], words = ceil(V / 32), read with per-lane (vector) loads.
struct LmProc {
    const uint32_t* seen;     // [B, words] ids already in the row's sequence (prompt ids of an input_ids call + generated ids)
    const uint32_t* ban;      // [B, words] suppress_tokens / single-token bad_words_ids
    const float* penalty;     // [1]
    const int* min_new;       // [1] EOS is banned while n_hist[b] < min_new
    const int* eos_ids;       // [8]
    const int* n_eos;         // [1] 0 ... 8
    const int* n_hist;        // [B] tokens generated so far
    int words;
};

// bit 0: row n of sequence b is in `seen`; bit 1: it is banned (ban bitmap, or an EOS id before min_new tokens)
__device__ __forceinline__ uint32_t lm_proc_flags(const LmProc& pr, int b, int n) {
    const size_t w = (size_t)b * pr.words + (n >> 5);
    const uint32_t bit = 1u << (n & 31);
    uint32_t f = (pr.seen[w] & bit) ? 1u : 0u;
    if (pr.ban[w] & bit) f |= 2u;
    if (pr.n_hist[b] < pr.min_new[0]) {
        const int ne = min(pr.n_eos[0], 8);
        for (int e = 0; e < ne; ++e)
            if (pr.eos_ids[e] == n) f |= 2u;
    }
    return f;
}

__device__ __forceinline__ float lm_proc_apply(float lv, uint32_t flags, float p) {
    if (flags & 1u) lv = lv < 0.f ? lv * p : __fdiv_rn(lv, p);
    if (flags & 2u) lv = -INFINITY;
    return lv;
}

typedef unsigned long long u64;

// fp32 -> uint32 whose unsigned order is the float order (-inf lowest); -0 was canonicalised to +0 by the caller
__device__ __forceinline__ uint32_t f32_ord(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_f32(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
// larger key = better: value first, then the LOWER index. Key 0 is "nothing" (a real key has a non-zero value half or index half).
__device__ __forceinline__ u64 make_key(float v, uint32_t idx) { return ((u64)f32_ord(v + 0.f) << 32) | (u64)(0xFFFFFFFFu - idx); }
__device__ __forceinline__ float key_value(u64 k) { return ord_f32((uint32_t)(k >> 32)); }
__device__ __forceinline__ uint32_t key_index(u64 k) { return 0xFFFFFFFFu - (uint32_t)k; }

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}
// block of 4 waves; `red` = 4 keys of LDS that nobody touches until the next barrier after this call's
__device__ __forceinline__ u64 block_max_u64(u64 v, u64* red) {
    v = wave_max_u64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = red[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) r = red[i] > r ? red[i] : r;
    return r;
}

// The C best keys of a block of 4 waves in descending order, one per round. scan(limit) = the thread's best key below `limit`
// (keys are unique, so "below the last winner" is "not taken yet"); only the winner's owner scans again. emit(c, key) runs in
// every thread with the round's winner (0 once the keys have run out). `redk` = 2 x 4 keys of LDS.
template <class Scan, class Emit>
__device__ __forceinline__ void block_select_best(int C, u64 (*redk)[4], Scan scan, Emit emit) {
    u64 mine = scan(~0ull);
    for (int c = 0; c < C; ++c) {
        const u64 w = block_max_u64(mine, redk[c & 1]);
        emit(c, w);
        if (w && mine == w) mine = scan(w);
    }
}

}  // namespace spider

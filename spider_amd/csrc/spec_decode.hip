// Prompt-lookup decoding (transformers `generate(prompt_lookup_num_tokens=K)`, PromptLookupCandidateGenerator) for one greedy
// sequence: a decode step carries R = K + 1 rows of the SAME sequence -- the last accepted token and up to K drafted successors --
// through the multi-row weight streams, and keeps the prefix of the drafts the model agrees with. Two kernels are specific to it:
//   spider_attn_verify_bf16         decode attention in which row r of a sequence sees the cache up to its own slot
//   spider_spec_advance_draft_i32   closes a verify step (accept, append, advance) and drafts the rows of the next one
// Everything else of the step is the engine's existing R-row route (GEMVs, rope_kv_append with S = R, lm_head arg-max).
#include "common.hpp"
#include "spec_accept.hpp"
#include <limits.h>

using namespace spider;

// ----------------------------------------------------------------------------------------------
// Verify attention: R consecutive query rows per sequence against one KV cache, GQA-aware, split over the KV length.
// attn_decode_kernel (llm_decode.hip) with one more block index: block = (split, kv head, b * R + r); row r of sequence b reads the
// cache slots kv_beg[b] <= j < kv_end[b] + r (kv_end[b] includes row 0's own token; rope_kv_append with S = R has written the R new
// K / V rows at kv_end[b] - 1 ... kv_end[b] + R - 2 before this launch), so the splits of a row partition the row's own length.
//   q [B * R, n_q, D] bf16;  kc / vc [B, n_kv, T_max, D];  partials and out are indexed by the row b * R + r
// The row's end is clamped to T_max: no block reads past the cache whatever the cursors hold.
// ----------------------------------------------------------------------------------------------
template <int D, int G>
__global__ __launch_bounds__(256) void attn_verify_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc,
                                                          const bf16_t* __restrict__ vc, const int* __restrict__ kv_beg,
                                                          const int* __restrict__ kv_end, float* __restrict__ part_o,
                                                          float* __restrict__ part_ml, bf16_t* __restrict__ out,
                                                          int n_kv, int T_max, float scale, int nsplit, int R) {
    static_assert(D == 128, "verify attention is specialised for head_dim 128");
    const int split = blockIdx.x, hk = blockIdx.y, row = blockIdx.z;
    const int b = row / R, r = row - b * R;
    const int n_q = n_kv * G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane >> 4;        // which of the 4 rows of a wave instruction
    const int dl = (lane & 15) * 8;   // this lane's 8 head-dim elements
    const int beg = max(kv_beg ? kv_beg[b] : 0, 0), end = min(kv_end[b] + r, T_max);
    const int len = max(end - beg, 0);
    const int per = (len + nsplit - 1) / nsplit;
    const int t0 = beg + split * per, t1 = min(end, t0 + per);

    float qf[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(q + ((size_t)row * n_q + hk * G + g) * D + dl);
        const uint32_t aw[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            qf[g][2 * j] = bf16lo_to_f32(aw[j]) * scale;
            qf[g][2 * j + 1] = bf16hi_to_f32(aw[j]) * scale;
        }
    }
    float m[G], l[G], o[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        m[g] = -INFINITY;
        l[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[g][j] = 0.f;
    }
    const bf16_t* kbase = kc + ((size_t)b * n_kv + hk) * (size_t)T_max * D;
    const bf16_t* vbase = vc + ((size_t)b * n_kv + hk) * (size_t)T_max * D;

    // The 16 lanes that share a cache row run the same trip count, and the in-loop shuffles (xor 1..8)
    // never leave that 16-lane group, so row sub-groups may diverge at the tail.
    for (int t = t0 + wave * 4 + sub; t < t1; t += 16) {
        const u32x4 kq = *reinterpret_cast<const u32x4*>(kbase + (size_t)t * D + dl);
        const u32x4 vq = *reinterpret_cast<const u32x4*>(vbase + (size_t)t * D + dl);
        const uint32_t kw[4] = {kq.x, kq.y, kq.z, kq.w};
        const uint32_t vw[4] = {vq.x, vq.y, vq.z, vq.w};
        float kf[8], vf[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kf[2 * j] = bf16lo_to_f32(kw[j]);
            kf[2 * j + 1] = bf16hi_to_f32(kw[j]);
            vf[2 * j] = bf16lo_to_f32(vw[j]);
            vf[2 * j + 1] = bf16hi_to_f32(vw[j]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) s += qf[g][j] * kf[j];
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            s += __shfl_xor(s, 4, 64);
            s += __shfl_xor(s, 8, 64);
            const float mn = fmaxf(m[g], s);
            const float alpha = __expf(m[g] - mn);  // m = -inf on the first row -> 0
            const float p = __expf(s - mn);
            l[g] = l[g] * alpha + p;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[g][j] = o[g][j] * alpha + p * vf[j];
            m[g] = mn;
        }
    }

    // merge the 4 row sub-groups of the wave (lanes differing in bits 4,5), then the 4 waves via LDS
    __shared__ float sm_m[4][G], sm_l[4][G];
    __shared__ float sm_o[4][G][D];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float m2 = __shfl_xor(m[g], off, 64);
            const float l2 = __shfl_xor(l[g], off, 64);
            const float mn = fmaxf(m[g], m2);
            const float a1 = (m[g] == -INFINITY) ? 0.f : __expf(m[g] - mn);
            const float a2 = (m2 == -INFINITY) ? 0.f : __expf(m2 - mn);
            l[g] = l[g] * a1 + l2 * a2;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float o2 = __shfl_xor(o[g][j], off, 64);
                o[g][j] = o[g][j] * a1 + o2 * a2;
            }
            m[g] = mn;
        }
        if (lane < 16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sm_o[wave][g][dl + j] = o[g][j];
            if (lane == 0) { sm_m[wave][g] = m[g]; sm_l[wave][g] = l[g]; }
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < G * D; idx += 256) {
        const int g = idx / D, dd = idx % D;
        float mm = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) mm = fmaxf(mm, sm_m[w][g]);
        float ll = 0.f, oo = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float a = (sm_m[w][g] == -INFINITY) ? 0.f : __expf(sm_m[w][g] - mm);
            ll += sm_l[w][g] * a;
            oo += sm_o[w][g][dd] * a;
        }
        const int hq = hk * G + g;
        if (nsplit == 1) {
            out[((size_t)row * n_q + hq) * D + dd] = f32_to_bf16(ll > 0.f ? oo / ll : 0.f);
        } else {
            const size_t pi = ((size_t)row * n_q + hq) * nsplit + split;
            part_o[pi * D + dd] = oo;
            if (dd == 0) { part_ml[pi * 2] = mm; part_ml[pi * 2 + 1] = ll; }
        }
    }
}

// attn_combine_kernel of llm_decode.hip, unchanged: one block per (row, query head) merges the row's nsplit partials
template <int D>
__global__ __launch_bounds__(256) void attn_verify_combine_kernel(const float* __restrict__ part_o, const float* __restrict__ part_ml,
                                                                  bf16_t* __restrict__ out, int nsplit) {
    static_assert(D == 128, "one wave covers the head dim with 2 elements per lane");
    __shared__ float sm_m[4], sm_l[4], sm_o[4][D];
    const size_t bh = blockIdx.x;  // row * n_q + hq
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float m = -INFINITY, l = 0.f, o0 = 0.f, o1 = 0.f;
    for (int s0 = wave; s0 < nsplit; s0 += 64) {       // 16 independent (m,l) + O loads in flight per wave: 64 splits = ONE round trip
        float2 mlv[16], ovv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int s = s0 + 4 * u;
            const bool ok = s < nsplit;
            const size_t pi = bh * nsplit + (ok ? s : 0);
            mlv[u] = *reinterpret_cast<const float2*>(part_ml + pi * 2);
            ovv[u] = *reinterpret_cast<const float2*>(part_o + pi * D + lane * 2);
            if (!ok) mlv[u] = float2{-INFINITY, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float ms = mlv[u].x, ls = mlv[u].y;
            const float mn = fmaxf(m, ms);
            const float a = (m == -INFINITY) ? 0.f : __expf(m - mn);
            const float bsc = (ms == -INFINITY) ? 0.f : __expf(ms - mn);
            l = l * a + ls * bsc;
            o0 = o0 * a + ovv[u].x * bsc;
            o1 = o1 * a + ovv[u].y * bsc;
            m = mn;
        }
    }
    if (lane == 0) { sm_m[wave] = m; sm_l[wave] = l; }
    sm_o[wave][lane * 2] = o0;
    sm_o[wave][lane * 2 + 1] = o1;
    __syncthreads();
    if (threadIdx.x < D) {
        const int dd = threadIdx.x;
        float mm = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
        float ll = 0.f, oo = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float a = (sm_m[w] == -INFINITY) ? 0.f : __expf(sm_m[w] - mm);
            ll += sm_l[w] * a;
            oo += sm_o[w][dd] * a;
        }
        out[bh * D + dd] = f32_to_bf16(ll > 0.f ? oo / ll : 0.f);
    }
}

// ----------------------------------------------------------------------------------------------
// Accept + draft, one block per sequence (the mould of ngram_ban_kernel<ADVANCE> in llm_decode.hip). Row layout of a sequence's step:
// ids / pos / slot / lm_out [B * R], row b * R is the last accepted token, rows b * R + 1 ... + n_draft[b] its drafted successors.
// ADVANCE (closes a verify step): lm_out[b * R + r] is the model's greedy token BEHIND row r, so
//   a = the largest j <= n_draft[b] with lm_out[i - 1] == ids[i] for all 1 <= i <= j   (drafts the model agrees with)
//   hist[b] gets lm_out[0 .. a] (slots at or past cap are dropped), n_hist += a + 1, kv_end += a + 1, base pos / slot += a + 1,
//   counters[b] += (1, n_draft[b], a)  (int64: steps, drafted, accepted)
// Draft (both forms) over s = prompt_ids[b, :n_prompt[b]] ++ hist[b, :n_hist[b]] of length L, K = k_draft[0] clamped to [0, R - 1],
// N = ngram[0] clamped to [0, SPEC_MAX_N]: for n = min(N, L - 1) ... 1 the EARLIEST window s[i : i + n] == s[L - n :] with
// i + n < L gives the draft s[i + n : min(i + n + K, L)]; the first n that has one wins, else n_draft = 0 (transformers' rule with
// logits_processor = None, no EOS cut and max_length far away). History slots at or past cap were never stored and read as -1.
// The scan runs ONCE for all n: a window of size n that ends in front of position e matches iff the backward match length
//   bm(e) = max { m <= N : s[e - 1 - j] == s[L - 1 - j] for all j < m }   is >= n,
// and the earliest window of size n is the one with the smallest e = i + n. Every thread strides over e in [1, L), keeps its
// smallest e per n, and one LDS atomicMin per n and thread merges them. Two barriers: (inputs read, LDS initialised) -> scanned.
// Then ids[0] = the last accepted token (ADVANCE; the draft-only form leaves row 0 as the caller set it), ids[r] = draft[r - 1]
// for r <= n_draft, ids[r] = ids[0] for the filler rows (their results are never read), pos[r] = pos[0] + r, slot[r] = slot[0] + r.
// Nothing global is written outside the sequence's own rows.
// ----------------------------------------------------------------------------------------------
constexpr int SPEC_THREADS = 1024;
constexpr int SPEC_MAX_R = 8;       // rows per sequence (the decode graph's 8 rows)
constexpr int SPEC_MAX_N = 8;       // largest n-gram the scan compares
template <bool ADVANCE>
__global__ __launch_bounds__(SPEC_THREADS) void spec_draft_kernel(
    const int* __restrict__ prompt_ids, const int* __restrict__ n_prompt, int pcap, int* __restrict__ hist,
    int* __restrict__ n_hist, int cap, const int* __restrict__ ngram, const int* __restrict__ k_draft,
    const int* __restrict__ lm_out, int* __restrict__ ids, int* __restrict__ pos, int* __restrict__ slot,
    int* __restrict__ kv_end, int* __restrict__ n_draft, long long* __restrict__ counters, int R) {
    __shared__ int s_min[SPEC_MAX_N + 1];       // s_min[n]: the smallest e whose window of size n matches the tail
    __shared__ int s_acc[SPEC_MAX_R];           // ADVANCE: the tokens accepted in this step
    const int b = blockIdx.x, tid = threadIdx.x;
    int P = n_prompt[b];
    P = P < 0 ? 0 : (P > pcap ? pcap : P);
    int K = k_draft[0];
    K = K < 0 ? 0 : (K > R - 1 ? R - 1 : K);
    int N = ngram[0];
    N = N < 0 ? 0 : (N > SPEC_MAX_N ? SPEC_MAX_N : N);
    const int nh_old = max(n_hist[b], 0);
    int* const ids_b = ids + (size_t)b * R;
    int* const pos_b = pos + (size_t)b * R;
    int* const slot_b = slot + (size_t)b * R;
    const int pos0 = pos_b[0], slot0 = slot_b[0], id0 = ids_b[0];
    // every thread works the acceptance out for itself from the step's 2 R ints (uniform loads), before anything is overwritten
    int a = 0, last = id0;
    if (ADVANCE) {
        int nd = n_draft[b];
        nd = nd < 0 ? 0 : (nd > K ? K : nd);
        a = spec_accept_len(lm_out + (size_t)b * R, ids_b, nd, R);      // nd <= K <= R - 1
        last = lm_out[(size_t)b * R + a];
        if (tid <= a) s_acc[tid] = lm_out[(size_t)b * R + tid];
        if (tid == 0) {
            counters[(size_t)b * 3] += 1;
            counters[(size_t)b * 3 + 1] += nd;
            counters[(size_t)b * 3 + 2] += a;
        }
    }
    const int adv = ADVANCE ? a + 1 : 0;
    const int nh = nh_old + adv;
    const int L = P + nh;
    if (tid <= SPEC_MAX_N) s_min[tid] = INT_MAX;
    __syncthreads();        // every thread has read the step's inputs; s_acc and s_min are set
    const int* prow = prompt_ids + (size_t)b * pcap;
    const int* hrow = hist + (size_t)b * cap;
    auto tok = [&](int k) -> int {      // element 0 <= k < L of the logical sequence
        if (k < P) return prow[k];
        const int j = k - P;
        if (j >= cap) return -1;
        return (ADVANCE && j >= nh_old) ? s_acc[j - nh_old] : hrow[j];
    };
    if (ADVANCE && tid <= a) {          // the accepted tokens join the history (the scan reads them from s_acc, not from here)
        const int j = nh_old + tid;
        if (j < cap) hist[(size_t)b * cap + j] = s_acc[tid];
    }
    const int nmax = min(N, L - 1);     // <= 0: nothing to match
    if (K > 0 && nmax > 0) {
        int tail[SPEC_MAX_N];
#pragma unroll
        for (int j = 0; j < SPEC_MAX_N; ++j) tail[j] = j < nmax ? tok(L - 1 - j) : 0;
        int best[SPEC_MAX_N];
#pragma unroll
        for (int j = 0; j < SPEC_MAX_N; ++j) best[j] = INT_MAX;
        for (int e = 1 + tid; e < L; e += SPEC_THREADS) {
            bool eq = true;
#pragma unroll
            for (int j = 0; j < SPEC_MAX_N; ++j) {
                eq = eq && j < nmax && j < e && tok(e - 1 - j) == tail[j];
                if (eq) best[j] = min(best[j], e);      // a window of size j + 1 ends in front of e
            }
        }
#pragma unroll
        for (int j = 0; j < SPEC_MAX_N; ++j)
            if (best[j] != INT_MAX) atomicMin(&s_min[j + 1], best[j]);
    }
    __syncthreads();        // scanned
    int e0 = 0, nd_new = 0;
    for (int n = nmax; n >= 1 && nd_new == 0; --n)
        if (K > 0 && s_min[n] != INT_MAX) {
            e0 = s_min[n];
            nd_new = min(K, L - e0);
        }
    if (tid < R) {
        ids_b[tid] = (tid >= 1 && tid <= nd_new) ? tok(e0 + tid - 1) : last;
        pos_b[tid] = pos0 + adv + tid;
        slot_b[tid] = slot0 + adv + tid;
    }
    if (tid == 0) {
        n_draft[b] = nd_new;
        if (ADVANCE) {
            n_hist[b] = nh;
            kv_end[b] += adv;
        }
    }
}

extern "C" {

#define ATTN_VERIFY_LAUNCH(G_)                                                                                  \
    attn_verify_kernel<128, G_><<<grid, 256, 0, (hipStream_t)stream>>>(                                         \
        (const bf16_t*)q, (const bf16_t*)k_cache, (const bf16_t*)v_cache, kv_beg, kv_end, (float*)ws_o,          \
        (float*)ws_ml, (bf16_t*)out, n_kv, T_max, scale, nsplit, R)

// workspace: ws_o >= B*R*n_q*nsplit*d floats, ws_ml >= B*R*n_q*nsplit*2 floats (unused when nsplit == 1)
int spider_attn_verify_bf16(const void* q, const void* k_cache, const void* v_cache, const int* kv_beg, const int* kv_end,
                            void* out, void* ws_o, void* ws_ml, int B, int R, int n_q, int n_kv, int d, int T_max, float scale,
                            int nsplit, void* stream) {
    SPIDER_CHECK(d == 128, "attn_verify: head_dim must be 128");
    SPIDER_CHECK(B > 0 && n_kv > 0 && n_q > 0 && n_q % n_kv == 0 && nsplit >= 1 && T_max > 0, "attn_verify: bad shape");
    SPIDER_CHECK(R >= 1 && R <= SPEC_MAX_R, "attn_verify: rows per sequence must be 1 ... 8");
    SPIDER_CHECK((long)B * R <= 65535 && n_kv <= 65535, "attn_verify: too many rows or kv heads for one grid");
    SPIDER_CHECK(q && k_cache && v_cache && kv_end && out, "attn_verify: q, caches, kv_end and out are required");
    SPIDER_CHECK(nsplit == 1 || (ws_o && ws_ml), "attn_verify: workspace required for nsplit > 1");
    const int G = n_q / n_kv;
    dim3 grid(nsplit, n_kv, B * R);
    switch (G) {
        case 1: ATTN_VERIFY_LAUNCH(1); break;
        case 2: ATTN_VERIFY_LAUNCH(2); break;
        case 3: ATTN_VERIFY_LAUNCH(3); break;
        case 4: ATTN_VERIFY_LAUNCH(4); break;
        case 5: ATTN_VERIFY_LAUNCH(5); break;
        case 6: ATTN_VERIFY_LAUNCH(6); break;
        case 7: ATTN_VERIFY_LAUNCH(7); break;
        case 8: ATTN_VERIFY_LAUNCH(8); break;
        default: spider_set_error("attn_verify: GQA group size must be 1 ... 8"); return -1;
    }
    SPIDER_LAUNCH_OK();
    if (nsplit > 1) {
        attn_verify_combine_kernel<128><<<B * R * n_q, 256, 0, (hipStream_t)stream>>>((const float*)ws_o, (const float*)ws_ml,
                                                                                    (bf16_t*)out, nsplit);
        SPIDER_LAUNCH_OK();
    }
    return 0;
}

static int spec_args_ok(const int* prompt_ids, const int* n_prompt, int pcap, const int* hist, const int* n_hist, int cap,
                        const int* ngram, const int* k_draft, const int* ids, const int* pos, const int* slot, const int* n_draft,
                        int R, int B) {
    SPIDER_CHECK(prompt_ids && n_prompt && pcap > 0 && hist && n_hist && cap > 0 && ngram && k_draft,
                 "prompt_lookup_draft: prompt_ids [B, pcap], n_prompt [B], hist [B, cap], n_hist [B], ngram and k_draft are required");
    SPIDER_CHECK(ids && pos && slot && n_draft, "prompt_lookup_draft: ids, pos, slot [B * R] and n_draft [B] are required");
    SPIDER_CHECK(R >= 1 && R <= SPEC_MAX_R && B > 0, "prompt_lookup_draft: rows per sequence must be 1 ... 8 and B > 0");
    return 0;
}

// draft only: n_draft[b] and rows 1 ... R - 1 of ids, pos[r] = pos[0] + r, slot[r] = slot[0] + r; row 0 stays as the caller set it
int spider_prompt_lookup_draft_i32(const int* prompt_ids, const int* n_prompt, int pcap, const int* hist, const int* n_hist,
                                   int cap, const int* ngram, const int* k_draft, int* ids, int* pos, int* slot, int* n_draft,
                                   int R, int B, void* stream) {
    if (spec_args_ok(prompt_ids, n_prompt, pcap, hist, n_hist, cap, ngram, k_draft, ids, pos, slot, n_draft, R, B)) return -1;
    spec_draft_kernel<false><<<B, SPEC_THREADS, 0, (hipStream_t)stream>>>(prompt_ids, n_prompt, pcap, (int*)hist, (int*)n_hist, cap,
                                                                         ngram, k_draft, nullptr, ids, pos, slot, nullptr, n_draft,
                                                                         nullptr, R);
    SPIDER_LAUNCH_OK();
    return 0;
}

// accept the drafts lm_out agrees with, append, advance, count, then draft the next step's rows -- one launch
int spider_spec_advance_draft_i32(const int* lm_out, int* ids, int* pos, int* slot, int* kv_end, int* n_draft, int* hist,
                                  int* n_hist, int cap, const int* prompt_ids, const int* n_prompt, int pcap, const int* ngram,
                                  const int* k_draft, void* counters, int R, int B, void* stream) {
    if (spec_args_ok(prompt_ids, n_prompt, pcap, hist, n_hist, cap, ngram, k_draft, ids, pos, slot, n_draft, R, B)) return -1;
    SPIDER_CHECK(lm_out && kv_end && counters, "spec_advance_draft: lm_out [B * R], kv_end [B] and counters int64 [B, 3] are required");
    spec_draft_kernel<true><<<B, SPEC_THREADS, 0, (hipStream_t)stream>>>(prompt_ids, n_prompt, pcap, hist, n_hist, cap, ngram,
                                                                        k_draft, lm_out, ids, pos, slot, kv_end, n_draft,
                                                                        (long long*)counters, R);
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // extern "C"

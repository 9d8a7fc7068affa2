// Seeded sampling step on the device (transformers' do_sample=True: logits processors, then TemperatureLogitsWarper,
// TopKLogitsWarper, TopPLogitsWarper, then one multinomial draw), run behind the unchanged decode layer stack and lm_head:
//   sample_partial  grid (vocabulary slices, rows): a slice of a row of raw bf16 logits goes through the logits processors of the
//                   arg-max epilogue (select.hpp) and the slice's top_k best (value, token) are written in key order -- the row's
//                   top_k best are among the union of the slices' top_k best
//   sample_select   one block per row: the row's top_k candidates by (value descending, token ascending) = rank 0 .. top_k - 1, then
//                     y_j = x_j / T,  p_j = expf(y_j - y_0)  (x_j = -inf: p_j = 0),  P = sum p_j in rank order
//                     rank j kept iff the mass before it < top_p * P; n_keep >= 1, S = the kept mass
//                     u = ((philox4x32_10(counter (n, r, 0, 0), key seed)[0] >> 9) + 0.5) * 2^-23,  n = n_hist[row], r = row0 + row
//                     token = first kept rank j with u * S < p_0 + ... + p_j, else rank n_keep - 1
//                   all in fp32, the sums by one thread in rank order. The token depends on (seed, r, n) and the logits only.
// top_k keeps EXACTLY k tokens: where HF's TopKLogitsWarper keeps every token that ties with the k-th value, the lower ids win.
// Every parameter is read from device memory when the kernel runs, so one captured decode graph serves any later request.
#include "common.hpp"
#include "select.hpp"

using namespace spider;

namespace {

constexpr int SAMPLE_SLICE = 4096;      // tokens per block of the partial selection: 256 threads x 2 x 8
constexpr int SAMPLE_MAX_K = 64;        // top_k limit = stride of the candidate lists

__device__ __forceinline__ int clamp_top_k(const int* top_k) {
    const int k = top_k[0];
    return k < 1 ? 1 : (k > SAMPLE_MAX_K ? SAMPLE_MAX_K : k);
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"), first output word
__device__ __forceinline__ uint32_t philox4x32_10_x(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return c0;
}

__global__ __launch_bounds__(256) void sample_partial_kernel(const bf16_t* __restrict__ logits, LmProc pr,
                                                             const int* __restrict__ top_k, float* __restrict__ ws_val,
                                                             int* __restrict__ ws_tok, int V, int nslice) {
    __shared__ u64 redk[2][4];
    const int s = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const bf16_t* row = logits + (size_t)r * V;
    float v[16];
    int t0[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = s * SAMPLE_SLICE + h * (SAMPLE_SLICE / 2) + tid * 8;
        t0[h] = t;
        if (t + 8 <= V && ((((size_t)r * V + t) & 7) == 0)) {        // 16-byte load when the row offset allows it
            const u32x4 q = *reinterpret_cast<const u32x4*>(row + t);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[h * 8 + 2 * j] = bf16lo_to_f32(w[j]);
                v[h * 8 + 2 * j + 1] = bf16hi_to_f32(w[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[h * 8 + j] = (t + j < V) ? bf16_to_f32(row[t + j]) : -INFINITY;
        }
    }
    if (pr.seen) {      // the processors of the arg-max epilogue; t0 is a multiple of 8, so its 8 tokens share one bitmap word
        const float pen = pr.penalty[0];
        const bool no_eos = pr.n_hist[r] < pr.min_new[0];
        const int ne = no_eos ? min(pr.n_eos[0], 8) : 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (t0[h] >= V) continue;
            const size_t w = (size_t)r * pr.words + (t0[h] >> 5);
            const uint32_t sw = pr.seen[w] >> (t0[h] & 31), bw = pr.ban[w] >> (t0[h] & 31);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint32_t fl = ((sw >> j) & 1u) | (((bw >> j) & 1u) << 1);
                for (int e = 0; e < ne; ++e)
                    if (pr.eos_ids[e] == t0[h] + j) fl |= 2u;
                v[h * 8 + j] = lm_proc_apply(v[h * 8 + j], fl, pen);
            }
        }
    }
    auto scan = [&](u64 limit) {
        u64 best = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int t = t0[j >> 3] + (j & 7);
            const u64 k = (t < V) ? make_key(v[j], (uint32_t)t) : 0;
            if (k < limit && k > best) best = k;
        }
        return best;
    };
    float* ov = ws_val + ((size_t)r * nslice + s) * SAMPLE_MAX_K;
    int* ot = ws_tok + ((size_t)r * nslice + s) * SAMPLE_MAX_K;
    block_select_best(clamp_top_k(top_k), redk, scan, [&](int c, u64 w) {
        if (tid == 0) {
            ov[c] = w ? key_value(w) : -INFINITY;
            ot[c] = w ? (int)key_index(w) : -1;        // a slice with fewer than top_k tokens: token -1
        }
    });
}

__global__ __launch_bounds__(256) void sample_select_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_tok,
                                                            const float* __restrict__ temperature, const float* __restrict__ top_p,
                                                            const int* __restrict__ top_k, const uint32_t* __restrict__ seed,
                                                            const int* __restrict__ row0, const int* __restrict__ n_hist,
                                                            int* __restrict__ next_ids, int* __restrict__ cand_tok,
                                                            float* __restrict__ cand_p, int* __restrict__ n_keep_out,
                                                            float* __restrict__ u_out, int V, int nslice) {
    __shared__ u64 redk[2][4];
    __shared__ float c_val[SAMPLE_MAX_K], c_p[SAMPLE_MAX_K];
    __shared__ int c_tok[SAMPLE_MAX_K];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int kk = clamp_top_k(top_k);
    const int E = nslice * SAMPLE_MAX_K;
    const float* bv = ws_val + (size_t)r * E;
    const int* bt = ws_tok + (size_t)r * E;
    auto scan = [&](u64 limit) {
        u64 best = 0;
        for (int e = tid; e < E; e += 256) {
            if ((e & (SAMPLE_MAX_K - 1)) >= kk) continue;       // the slices wrote their first top_k entries only
            const int tok = bt[e];
            if (tok < 0 || tok >= V) continue;
            const u64 key = make_key(bv[e], (uint32_t)tok);
            if (key < limit && key > best) best = key;
        }
        return best;
    };
    block_select_best(kk, redk, scan, [&](int c, u64 w) {
        if (tid == 0) {
            c_val[c] = w ? key_value(w) : -INFINITY;
            c_tok[c] = w ? (int)key_index(w) : -1;      // V < top_k: the ranks past V hold no token and no mass
        }
    });
    __syncthreads();
    if (tid < SAMPLE_MAX_K) {
        float p = 0.f;
        if (tid < kk && c_tok[tid] >= 0 && c_val[tid] != -INFINITY) {
            const float T = temperature[0];
            p = expf(__fdiv_rn(c_val[tid], T) - __fdiv_rn(c_val[0], T));
        }
        c_p[tid] = p;
    }
    __syncthreads();
    if (tid == 0) {
        float P = 0.f;
        for (int j = 0; j < kk; ++j) P += c_p[j];
        const float thr = top_p[0] * P;
        float S = 0.f;
        int nk = 0;
        while (nk < kk && S < thr) S += c_p[nk++];      // p is non-increasing in rank, so the kept ranks are a prefix
        if (nk < 1) nk = 1;                             // a row that is all -inf (P = 0): rank 0
        const uint32_t x = philox4x32_10_x((uint32_t)n_hist[r], (uint32_t)(row0[0] + r), 0u, 0u, seed[0], seed[1]);
        const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-7f;     // 2^-23: 24 significant bits, exact in fp32, inside (0, 1)
        const float target = u * S;
        int pick = nk - 1;
        float cum = 0.f;
        for (int j = 0; j < nk; ++j) {
            cum += c_p[j];
            if (target < cum) {
                pick = j;
                break;
            }
        }
        next_ids[r] = c_tok[pick];
        n_keep_out[r] = nk;
        u_out[r] = u;
    }
    if (tid < SAMPLE_MAX_K) {
        cand_tok[(size_t)r * SAMPLE_MAX_K + tid] = tid < kk ? c_tok[tid] : -1;
        cand_p[(size_t)r * SAMPLE_MAX_K + tid] = c_p[tid];
    }
}

}  // namespace

extern "C" {

int spider_sample_partial_bf16(const void* logits, const void* seen, const void* ban, const float* penalty, const int* min_new,
                               const int* eos_ids, const int* n_eos, const int* n_hist, const int* top_k, float* ws_val,
                               int* ws_tok, int rows, int V, int nslice, void* stream) {
    SPIDER_CHECK(logits && top_k && ws_val && ws_tok, "sample_partial: logits, top_k and the two workspaces required");
    SPIDER_CHECK(rows > 0 && rows <= 64 && V > 0, "sample_partial: 1 <= rows <= 64, V > 0");
    SPIDER_CHECK(((uintptr_t)logits & 15) == 0, "sample_partial: logits must be 16-byte aligned");
    SPIDER_CHECK(nslice == (V + SAMPLE_SLICE - 1) / SAMPLE_SLICE, "sample_partial: nslice must be ceil(V / 4096)");
    SPIDER_CHECK((seen != nullptr) == (ban != nullptr), "sample_partial: seen and ban come together (both null: no processors)");
    SPIDER_CHECK(!seen || (penalty && min_new && eos_ids && n_eos && n_hist),
                 "sample_partial: the bitmaps need penalty, min_new, eos_ids, n_eos and n_hist");
    const LmProc pr{(const uint32_t*)seen, (const uint32_t*)ban, penalty, min_new, eos_ids, n_eos, n_hist, (V + 31) / 32};
    sample_partial_kernel<<<dim3(nslice, rows), 256, 0, (hipStream_t)stream>>>((const bf16_t*)logits, pr, top_k, ws_val, ws_tok, V,
                                                                               nslice);
    SPIDER_LAUNCH_OK();
    return 0;
}

int spider_sample_select_f32(const float* ws_val, const int* ws_tok, const float* temperature, const float* top_p, const int* top_k,
                             const void* seed, const int* row0, const int* n_hist, int* next_ids, int* cand_tok, float* cand_p,
                             int* n_keep, float* u, int rows, int V, int nslice, void* stream) {
    SPIDER_CHECK(ws_val && ws_tok && temperature && top_p && top_k && seed && row0 && n_hist, "sample_select: inputs required");
    SPIDER_CHECK(next_ids && cand_tok && cand_p && n_keep && u, "sample_select: outputs required");
    SPIDER_CHECK(rows > 0 && rows <= 64 && V > 0, "sample_select: 1 <= rows <= 64, V > 0");
    SPIDER_CHECK(nslice == (V + SAMPLE_SLICE - 1) / SAMPLE_SLICE, "sample_select: nslice must be ceil(V / 4096)");
    sample_select_kernel<<<rows, 256, 0, (hipStream_t)stream>>>(ws_val, ws_tok, temperature, top_p, top_k, (const uint32_t*)seed, row0,
                                                                n_hist, next_ids, cand_tok, cand_p, n_keep, u, V, nslice);
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // extern "C"

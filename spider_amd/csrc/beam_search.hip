// Beam search step on the device (transformers GenerationMixin._beam_search: _get_top_k_continuations +
// _get_running_beams_for_next_iteration + the cache reorder), run behind the unchanged decode layer stack and lm_head:
//   beam_partial  grid (vocabulary slices, rows): per slice of a row of raw bf16 logits the online-softmax pair (max, sum exp)
//                 and the slice's C best (logit, token) -- the row's global best C are among the union of the slices' best C
//   beam_select   one block per batch row: lse[k] from the partials, score = run[k] + (logit - lse[k]) in fp32, the C best
//                 continuations of the row's K beams ordered by (score descending, k * V + token ascending), written to the
//                 step's slot of the trace; the first K whose token is no EOS id become the running beams
//   kv_row_copy   cache row b*K + k <- old row b*K + src_beam[b, k] over the slots [kv_beg, kv_end), through a second buffer:
//                 launch 1 copies the moved rows cache -> tmp, launch 2 tmp -> cache. No block reads what another block of its
//                 launch writes, whatever the map (duplicates, cycles); rows that keep their history are skipped by both.
// Orderings are total: the reductions compare 64-bit keys (order-preserving bits of the fp32 value, then the inverted index).
#include "common.hpp"
#include "select.hpp"

using namespace spider;

namespace {

constexpr int BEAM_SLICE = 4096;     // tokens per block of the partial reduction: 256 threads x 2 x 8
constexpr int BEAM_MAX_C = 32;       // continuations kept per batch row
constexpr int BEAM_MAX_K = 8;
constexpr int BEAM_MAX_EOS = 8;

__global__ __launch_bounds__(256) void beam_partial_kernel(const bf16_t* __restrict__ logits, float* __restrict__ ws_ms,
                                                           float* __restrict__ ws_val, int* __restrict__ ws_tok, int V, int C,
                                                           int nslice) {
    __shared__ float redf[4];
    __shared__ u64 redk[2][4];
    const int s = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const bf16_t* row = logits + (size_t)r * V;
    float v[16];
    int t0[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = s * BEAM_SLICE + h * (BEAM_SLICE / 2) + tid * 8;
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
    // online-softmax pair of the slice
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j) m = fmaxf(m, v[j]);
    m = wave_max(m);
    if ((tid & 63) == 0) redf[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    const float ms = (m == -INFINITY) ? 0.f : m;
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) e += expf(v[j] - ms);        // exp(-inf) = 0 for the tokens past V
    e = block_sum<4>(e, redf);
    if (tid == 0) {
        ws_ms[((size_t)r * nslice + s) * 2] = ms;
        ws_ms[((size_t)r * nslice + s) * 2 + 1] = e;
    }
    // the slice's C best, one per round (block_select_best): the winner's owner looks through its 16 values again
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
    float* ov = ws_val + ((size_t)r * nslice + s) * C;
    int* ot = ws_tok + ((size_t)r * nslice + s) * C;
    block_select_best(C, redk, scan, [&](int c, u64 w) {
        if (tid == 0) {
            ov[c] = w ? key_value(w) : -INFINITY;
            ot[c] = w ? (int)key_index(w) : -1;        // a slice with fewer than C tokens: token -1
        }
    });
}

__global__ __launch_bounds__(256) void beam_select_kernel(const float* __restrict__ ws_ms, const float* __restrict__ ws_val,
                                                          const int* __restrict__ ws_tok, float* __restrict__ run,
                                                          const int* __restrict__ eos_ids, const int* __restrict__ n_eos,
                                                          const int* __restrict__ n_hist, float* __restrict__ tr_score,
                                                          int* __restrict__ tr_beam, int* __restrict__ tr_tok, int cap,
                                                          int* __restrict__ src_beam, int* __restrict__ next_ids, int B, int K,
                                                          int V, int C, int nslice) {
    __shared__ float lse[BEAM_MAX_K], runs[BEAM_MAX_K];
    __shared__ u64 redk[2][4];
    __shared__ float c_score[BEAM_MAX_C];
    __shared__ int c_beam[BEAM_MAX_C], c_tok[BEAM_MAX_C];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int k = wv; k < K; k += 4) {       // lse[k] = log sum exp of row b*K + k from its slices' pairs
        const float* ms = ws_ms + (size_t)(b * K + k) * nslice * 2;
        float m = -INFINITY;
        for (int i = lane; i < nslice; i += 64) m = fmaxf(m, ms[2 * i]);
        m = wave_max(m);
        float e = 0.f;
        for (int i = lane; i < nslice; i += 64) e += ms[2 * i + 1] * expf(ms[2 * i] - m);
        e = wave_sum(e);
        if (lane == 0) {
            lse[k] = m + logf(e);
            runs[k] = run[b * K + k];
        }
    }
    __syncthreads();
    const int per = nslice * C, E = K * per;
    const float* bv = ws_val + (size_t)b * E;
    const int* bt = ws_tok + (size_t)b * E;
    // The slices kept their C best by (logit, token); this selection orders by (score, beam * V + token). The two agree while the
    // score is strictly monotone in the logit within a beam. fp32 run + (logit - lse) can round two different bf16 logits of one
    // beam to ONE score only when |run| dwarfs the logits (the -1e9 beams of step 0, which never reach the best C while V >= C):
    // there the token-ascending rule could name a token its slice had dropped for a lower logit. Not reachable otherwise.
    auto scan = [&](u64 limit) {
        u64 best = 0;
        for (int e = tid; e < E; e += 256) {
            const int tok = bt[e];
            if (tok < 0 || tok >= V) continue;
            const int k = e / per;
            const float sc = runs[k] + (bv[e] - lse[k]);
            const u64 key = make_key(sc, (uint32_t)(k * V + tok));
            if (key < limit && key > best) best = key;
        }
        return best;
    };
    block_select_best(C, redk, scan, [&](int c, u64 w) {
        if (tid == 0) {
            const uint32_t flat = key_index(w);
            c_score[c] = w ? key_value(w) : -INFINITY;
            c_beam[c] = w ? (int)(flat / (uint32_t)V) : 0;
            c_tok[c] = w ? (int)(flat % (uint32_t)V) : 0;
        }
    });
    __syncthreads();
    const int step = n_hist[b * K];
    if (tid < C && step >= 0 && step < cap) {
        const size_t o = ((size_t)step * B + b) * C + tid;
        tr_score[o] = c_score[tid];
        tr_beam[o] = c_beam[tid];
        tr_tok[o] = c_tok[tid];
    }
    if (tid == 0) {     // the running beams: the first K continuations, in order, whose token is no EOS id
        int ne = n_eos[0];
        ne = ne < 0 ? 0 : (ne > BEAM_MAX_EOS ? BEAM_MAX_EOS : ne);
        int nk = 0;
        for (int c = 0; c < C && nk < K; ++c) {
            bool fin = false;
            for (int i = 0; i < ne; ++i) fin |= (c_tok[c] == eos_ids[i]);
            if (fin) continue;
            run[b * K + nk] = c_score[c];
            src_beam[b * K + nk] = c_beam[c];
            next_ids[b * K + nk] = c_tok[c];
            ++nk;
        }
        for (; nk < K; ++nk) {      // not reached while C >= (1 + n_eos) * K distinct continuations exist; keeps every index valid
            run[b * K + nk] = -INFINITY;
            src_beam[b * K + nk] = c_beam[0];
            next_ids[b * K + nk] = c_tok[0];
        }
    }
}

// one launch of the two-launch row move. grid (x, R * n_kv, 2 * L). from_tmp = 0: src = cache row of the source beam, dst = tmp
// row r; from_tmp = 1: src = tmp row r, dst = cache row r. Rows whose source is themselves are skipped by both launches.
__global__ __launch_bounds__(256) void kv_row_copy_kernel(const bf16_t* __restrict__ k_src, const bf16_t* __restrict__ v_src,
                                                          bf16_t* __restrict__ k_dst, bf16_t* __restrict__ v_dst,
                                                          const int* __restrict__ src_beam, const int* __restrict__ kv_beg,
                                                          const int* __restrict__ kv_end, int K, int R, int rows_alloc, int n_kv,
                                                          int T, int d, int from_tmp) {
    const int r = blockIdx.y / n_kv, h = blockIdx.y % n_kv, l = blockIdx.z >> 1;
    const int sb = src_beam[r];
    const int s = (r / K) * K + sb;
    if (sb < 0 || sb >= K || s >= R || s == r) return;
    int beg = kv_beg[r], end = kv_end[r];
    beg = beg < 0 ? 0 : beg;
    end = end > T ? T : end;
    if (end <= beg) return;
    const bf16_t* src = (blockIdx.z & 1) ? v_src : k_src;
    bf16_t* dst = (blockIdx.z & 1) ? v_dst : k_dst;
    const size_t row_src = (((size_t)l * rows_alloc + (from_tmp ? r : s)) * n_kv + h) * (size_t)T * d + (size_t)beg * d;
    const size_t row_dst = (((size_t)l * rows_alloc + r) * n_kv + h) * (size_t)T * d + (size_t)beg * d;
    const u32x4* sp = reinterpret_cast<const u32x4*>(src + row_src);
    u32x4* dp = reinterpret_cast<u32x4*>(dst + row_dst);
    const int nvec = (end - beg) * (d / 8);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nvec; i += gridDim.x * 256) dp[i] = sp[i];
}

}  // namespace

extern "C" {

int spider_beam_partial_bf16(const void* logits, float* ws_ms, float* ws_val, int* ws_tok, int rows, int V, int C, int nslice,
                             void* stream) {
    SPIDER_CHECK(logits && ws_ms && ws_val && ws_tok, "beam_partial: logits and the three workspaces required");
    SPIDER_CHECK(rows > 0 && rows <= 64 && V > 0, "beam_partial: 1 <= rows <= 64, V > 0");
    SPIDER_CHECK(((uintptr_t)logits & 15) == 0, "beam_partial: logits must be 16-byte aligned");
    SPIDER_CHECK(C >= 1 && C <= BEAM_MAX_C, "beam_partial: 1 <= C <= 32");
    SPIDER_CHECK(nslice == (V + BEAM_SLICE - 1) / BEAM_SLICE, "beam_partial: nslice must be ceil(V / 4096)");
    beam_partial_kernel<<<dim3(nslice, rows), 256, 0, (hipStream_t)stream>>>((const bf16_t*)logits, ws_ms, ws_val, ws_tok, V, C,
                                                                             nslice);
    SPIDER_LAUNCH_OK();
    return 0;
}

int spider_beam_select_f32(const float* ws_ms, const float* ws_val, const int* ws_tok, float* run_scores, const int* eos_ids,
                           const int* n_eos, const int* n_hist, float* trace_score, int* trace_beam, int* trace_tok, int cap,
                           int* src_beam, int* next_ids, int B, int K, int V, int C, int nslice, void* stream) {
    SPIDER_CHECK(ws_ms && ws_val && ws_tok && run_scores && eos_ids && n_eos && n_hist, "beam_select: inputs required");
    SPIDER_CHECK(trace_score && trace_beam && trace_tok && cap > 0 && src_beam && next_ids, "beam_select: outputs required");
    SPIDER_CHECK(B > 0 && K >= 1 && K <= BEAM_MAX_K && B * K <= 64, "beam_select: 1 <= K <= 8, B * K <= 64");
    SPIDER_CHECK(C >= K && C <= BEAM_MAX_C && V >= C, "beam_select: K <= C <= 32 and V >= C");
    SPIDER_CHECK((long)K * V < (1l << 31), "beam_select: K * V must fit 31 bits");
    SPIDER_CHECK(nslice == (V + BEAM_SLICE - 1) / BEAM_SLICE, "beam_select: nslice must be ceil(V / 4096)");
    beam_select_kernel<<<B, 256, 0, (hipStream_t)stream>>>(ws_ms, ws_val, ws_tok, run_scores, eos_ids, n_eos, n_hist, trace_score,
                                                           trace_beam, trace_tok, cap, src_beam, next_ids, B, K, V, C, nslice);
    SPIDER_LAUNCH_OK();
    return 0;
}

int spider_kv_row_gather_bf16(void* k_cache, void* v_cache, void* k_tmp, void* v_tmp, const int* src_beam, const int* kv_beg,
                              const int* kv_end, int K, int R, int layers, int rows_alloc, int n_kv, int T, int d, void* stream) {
    SPIDER_CHECK(k_cache && v_cache && k_tmp && v_tmp && src_beam && kv_beg && kv_end, "kv_row_gather: buffers required");
    SPIDER_CHECK(k_cache != k_tmp && v_cache != v_tmp && k_cache != v_tmp && v_cache != k_tmp, "kv_row_gather: tmp must not alias the cache");
    SPIDER_CHECK(K >= 1 && R >= K && R % K == 0 && R <= rows_alloc, "kv_row_gather: R = B * K rows within the allocation");
    SPIDER_CHECK(layers > 0 && n_kv > 0 && T > 0 && d > 0 && d % 8 == 0, "kv_row_gather: head_dim must be a multiple of 8");
    SPIDER_CHECK((((uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)k_tmp | (uintptr_t)v_tmp) & 15) == 0, "kv_row_gather: buffers must be 16-byte aligned");
    SPIDER_CHECK((long)R * n_kv <= 65535 && 2l * layers <= 65535, "kv_row_gather: grid too large");
    int gx = (int)(((long)T * (d / 8) + 1023) / 1024);
    gx = gx < 1 ? 1 : (gx > 16 ? 16 : gx);
    const dim3 grid(gx, R * n_kv, 2 * layers);
    kv_row_copy_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_t*)k_cache, (const bf16_t*)v_cache, (bf16_t*)k_tmp,
                                                              (bf16_t*)v_tmp, src_beam, kv_beg, kv_end, K, R, rows_alloc, n_kv, T, d, 0);
    SPIDER_LAUNCH_OK();
    kv_row_copy_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const bf16_t*)k_tmp, (const bf16_t*)v_tmp, (bf16_t*)k_cache,
                                                              (bf16_t*)v_cache, src_beam, kv_beg, kv_end, K, R, rows_alloc, n_kv, T, d, 1);
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // extern "C"

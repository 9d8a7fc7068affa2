// Weight-only FP8 / MXFP4 forms of the row-major lm_head + greedy arg-max (lmhead_partial_kernel of llm_decode.hip), 1..4 sequences
// (gfx950 / CDNA4).
//
//   logit[b, n] = bf16( sum_k xin[b, k] * W_eff[n, k] ),   b < NB <= 4,   n < V
//   FP8   (spider_lm_head_argmax[_proc]_w8): q [V, K] bytes, OCP e4m3fn, K % 16 == 0; scale [V] fp32, one per vocabulary row;
//         W_eff[n, k] = f32(q[n, k]) * scale[n]  (the layout of spider_amd/llm.py: quantize_fp8_rows, as gemv_wq.hip reads it)
//   MXFP4 (spider_lm_head_argmax[_proc]_w4): blocks [V, K / 2] bytes, two e2m1 codes per byte, low nibble first, K % 32 == 0;
//         scales [V, K / 32] bytes, E8M0, 1..254; W_eff[n, k] = e2m1(code) * 2^(scales[n, k / 32] - 127)  (quantize_mxfp4, as
//         gemv_wq.hip reads it)
//   xin   x, or the final RMSNorm in the two-rounding form of lmhead_partial_kernel: bf16(bf16(x * rs) * norm_w), with the sum of
//         squares reduced in that kernel's order
//
// Contract of lmhead_partial_kernel, kept: grid = spider_lm_head_nparts(V) blocks of 4 waves, each block owns a contiguous range of
// vocabulary rows and writes one (value, index) partial per sequence into the [B, nparts] workspace, which the final reduction
// (argmax_final_kernel of wq_common.hpp, the bf16 form's) turns into out_ids. The epilogue is the bf16 kernel's: the logit is rounded
// to bf16, optionally stored RAW to logits [B, V], widened to fp32, passed through lm_proc_flags / lm_proc_apply in the PROC form,
// and kept when lv > best || (lv == best && n < besti): ties and an all -inf row go to the lowest id.
//
// Weight decode: the siblings'. FP8: a lane's 16-byte nontemporal load is 16 weights, v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32 (exact),
// and the row's fp32 scale multiplies the fp32 sum once after the wave reduction. MXFP4: a lane's 16-byte load is 32 weights = one
// MX block with one scale byte, v_cvt_scalef32_pk_bf16_fp4 with the scale uint32(byte) << 23 applied inside the conversion. Both
// meet the activations in v_dot2c_f32_bf16. Activations are staged once per block in LDS, rows padded to whole chunks (1024 / 2048
// elements) and swizzled per chunk (wq_slot of wq_common.hpp) so that every 16-byte LDS read is lane-contiguous; the
// siblings' budget rule decides whether they fit (ops.w8_norm_fits / w4_norm_fits), else x is read through L2 and the fused norm is
// refused. Loads go to clamped addresses (row min(n, V - 1), k min(k, K - 16 / 32)); only the FMAs and the epilogue are predicated.
// Unlike the siblings the weights are decoded one 8-weight piece at a time next to the activations' LDS read, so at most four
// decoded registers are live per row whatever R is.
//
// Bytes in flight: a wave iteration streams R vocabulary rows, U = 2 chunks of each before the first FMA, so a lane has 2 R 16-byte
// weight loads outstanding (K = 3584: the whole MXFP4 row, half of the FP8 row). R = 2 / 4 / 8 are built (SPIDER_LMQ_R selects,
// NB * R <= 64 holds for the per-lane processor flags) and were measured against each other with scripts/exp/lm_head_q_cost.py
// --ops-only (profiles/lm_head_q_cost.txt; [152064, 3584] head, cold weights, us per launch at 1 / 2 / 3 / 4 sequences):
//   FP8    R = 2: 98.1 / 99.1 / 113.4 / 131.0    R = 4: 97.1 / 98.3 / 108.7 / 132.1    R = 8: 108.0 / 108.5 / 144.6 / 177.7
//   MXFP4  R = 2: 57.8 / 69.3 /  87.2 / 110.1    R = 4: 58.9 / 67.5 /  85.8 / 110.2    R = 8:  63.1 /  78.9 / 109.1 / 132.0
//   (the bf16 route of the same process: 187 row-major / 176 / 178 / 179 fragment-major)
// R = 2 and R = 4 are within 5 us of each other either way, R = 8 is slower everywhere (162 - 221 VGPRs from two sequences on, two
// or three waves per SIMD); the default LMQ_R_DEFAULT = 4 is what every other figure of that file was taken with. From three
// sequences on the launch is no longer bound by the weight stream (MXFP4: 3.4 / 2.6 TB/s at 3 / 4 sequences against 4.9 at one).
// Issuing the next group's loads before the current group's reduction was not built or measured.
#include "select.hpp"
#include "wq_common.hpp"

using namespace spider;

extern "C" int spider_lm_head_nparts(int V);     // llm_decode.hip: blocks = partials per sequence

namespace {

#define LMQ_R_DEFAULT 4                          // vocabulary rows per wave iteration

// FMT 8: FP8 bytes + fp32 row scales; FMT 4: MXFP4 nibbles + E8M0 block scale bytes
template <int FMT, int NB, int R, bool PROC, bool XLDS>
__global__ __launch_bounds__(256) void lmq_partial_kernel(const uint8_t* __restrict__ Wq, const void* __restrict__ scale_,
                                                          const bf16_t* __restrict__ x, const bf16_t* __restrict__ norm_w, float eps,
                                                          float* __restrict__ pval, int* __restrict__ pidx,
                                                          bf16_t* __restrict__ logits, int V, int K, LmProc pr) {
    static_assert(FMT == 8 || FMT == 4, "FMT: 8 (FP8) or 4 (MXFP4)");
    static_assert(NB * R <= 64, "one lane per (sequence, row) holds the processor flags");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float red[4];
    __shared__ float bval[4][NB];
    __shared__ int bidx[4][NB];
    constexpr int LW = WQ_LW<FMT>, CHUNK = WQ_CHUNK<FMT>;
    constexpr int NP = LW / 8;                   // 8-weight pieces (one weight word of FP4, two of FP8) = 16-byte LDS reads per load
    constexpr int U = 2;                         // chunks of every row requested before the first FMA
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int KP = (K + CHUNK - 1) & ~(CHUNK - 1);   // LDS row length in elements (whole chunks)
    const size_t row_bytes = FMT == 8 ? (size_t)K : (size_t)(K / 2);
    const float* scale8 = reinterpret_cast<const float*>(scale_);
    const uint8_t* scale4 = reinterpret_cast<const uint8_t*>(scale_);

    // ---- activations: lmhead_partial_kernel's staging (same sum-of-squares order, same two roundings), to swizzled padded rows.
    // The pad past K is never written and never read: a lane's LW weights are wholly inside the row or wholly past it.
    if constexpr (XLDS)
        stage_rows_simple<NB, 4>(x, norm_w, eps, K, KP / 8, reinterpret_cast<u32x4*>(smem), red, [](int i) { return wq_slot<FMT>(i); });
    const bf16_t* xs = reinterpret_cast<const bf16_t*>(smem);

    float best[NB];
    int besti[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { best[b] = -INFINITY; besti[b] = 0x7fffffff; }

    // rows handled by this block: [blockIdx.x * rows_per_block, +rows_per_block), waves interleave groups of R
    const int rows_per_block = (V + gridDim.x - 1) / gridDim.x;
    const int rbeg = blockIdx.x * rows_per_block;
    const int rend = min(V, rbeg + rows_per_block);
    for (int n0 = rbeg + wave * R; n0 < rend; n0 += 4 * R) {       // wave-uniform: every lane reaches the reductions
        float acc[NB][R];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[b][r] = 0.f;
        const uint8_t* wrow[R];
        const uint8_t* srow[R];
        float rscale[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = min(n0 + r, V - 1);
            wrow[r] = Wq + (size_t)n * row_bytes;
            if (FMT == 8) { rscale[r] = scale8[n]; srow[r] = nullptr; }
            else { rscale[r] = 1.f; srow[r] = scale4 + (size_t)n * (K / 32); }
        }
        for (int base = 0; base < K; base += U * CHUNK) {          // uniform trip count
            u32x4 wq[U][R];
            uint32_t sb[U][R];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = base + u * CHUNK + lane * LW;
                const unsigned kc = (unsigned)(k < K ? k : K - LW);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    wq[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[r] + (FMT == 8 ? kc : kc >> 1)));
                    if (FMT == 4) sb[u][r] = srow[r][kc >> 5];
                    else sb[u][r] = 0;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kc = base + u * CHUNK, k = kc + lane * LW;
                if (k < K) {
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        uint32_t xw[NB][4];
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            u32x4 xa;
                            if (XLDS) xa = *reinterpret_cast<const u32x4*>(xs + (size_t)b * KP + kc + p * 512 + lane * 8);
                            else      xa = *reinterpret_cast<const u32x4*>(x + (size_t)b * K + k + p * 8);
                            xw[b][0] = xa.x; xw[b][1] = xa.y; xw[b][2] = xa.z; xw[b][3] = xa.w;
                        }
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const uint32_t ww[4] = {wq[u][r].x, wq[u][r].y, wq[u][r].z, wq[u][r].w};
                            uint32_t wb[4];
                            wq_decode_piece<FMT>(ww, p, sb[u][r], wb);
#pragma unroll
                            for (int b = 0; b < NB; ++b)
#pragma unroll
                                for (int j = 0; j < 4; ++j) acc[b][r] = dot2_bf16(wb[j], xw[b][j], acc[b][r]);
                        }
                    }
                }
            }
        }
        uint32_t pflags = 0;    // PROC: lane b * R + r holds the flags of (sequence b, row n0 + r), loaded per lane
        float pen = 1.f;
        if (PROC) {
            if (lane < NB * R && n0 + lane % R < rend) pflags = lm_proc_flags(pr, lane / R, n0 + lane % R);
            pen = pr.penalty[0];
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float s = wave_sum_valu(acc[b][r]);
                if (FMT == 8) s *= rscale[r];
                const int n = n0 + r;
                const uint32_t fl = PROC ? (uint32_t)__shfl((int)pflags, b * R + r, 64) : 0u;
                if (n < rend) {
                    const bf16_t lb = f32_to_bf16(s);
                    float lv = bf16_to_f32(lb);
                    if (logits && lane == 0) logits[(size_t)b * V + n] = lb;
                    if (PROC) lv = lm_proc_apply(lv, fl, pen);
                    if (lv > best[b] || (lv == best[b] && n < besti[b])) { best[b] = lv; besti[b] = n; }
                }
            }
    }
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) { bval[wave][b] = best[b]; bidx[wave][b] = besti[b]; }
    }
    __syncthreads();
    if (threadIdx.x < NB) {
        const int b = threadIdx.x;
        float bv = bval[0][b];
        int bi = bidx[0][b];
        for (int w = 1; w < 4; ++w) {
            if (bval[w][b] > bv || (bval[w][b] == bv && bidx[w][b] < bi)) { bv = bval[w][b]; bi = bidx[w][b]; }
        }
        pval[(size_t)b * gridDim.x + blockIdx.x] = bv;
        pidx[(size_t)b * gridDim.x + blockIdx.x] = bi;
    }
}

struct LmqArgs {
    const void *q, *scale, *x, *norm_w;
    float eps;
    int* out_ids;
    void *logits, *ws_val, *ws_idx;
    int B, V, K;
    void* stream;
};

template <int FMT, int NB, int R, bool PROC, bool XL>
void lmq_launch(const LmqArgs& a, const LmProc& pr, int nparts, size_t lds) {
    auto* fn = lmq_partial_kernel<FMT, NB, R, PROC, XL>;
    if (XL && lds > WQ_LDS_DEFAULT_LIMIT) {
        static unsigned raised = 0;
        raise_dynamic_lds(fn, (int)WQ_LDS_HW_LIMIT, raised);
    }
    fn<<<nparts, 256, XL ? lds : 0, (hipStream_t)a.stream>>>((const uint8_t*)a.q, a.scale, (const bf16_t*)a.x, (const bf16_t*)a.norm_w,
                                                              a.eps, (float*)a.ws_val, (int*)a.ws_idx, (bf16_t*)a.logits, a.V, a.K, pr);
}

template <int FMT, int NB, bool PROC>
int lmq_dispatch(const LmqArgs& a, const LmProc& pr) {
    // tuning aids, read once: SPIDER_W8_LDS_MAX / SPIDER_W4_LDS_MAX (the siblings' budget of staged activations per block, which
    // ops.w8_norm_fits / w4_norm_fits mirror), SPIDER_LMQ_R (vocabulary rows per wave iteration: 2 / 4 / 8)
    static const int env_r = wq_env("SPIDER_LMQ_R", 0);
    const size_t lds = wq_lds_bytes<FMT>(NB, a.K);
    const bool xlds = lds <= wq_lds_max<FMT>();
    if (!xlds && a.norm_w) return wq_fail(FMT == 8 ? "lm_head_argmax_w8" : "lm_head_argmax_w4", WQ_NORM_RULE<FMT>);
    const int nparts = spider_lm_head_nparts(a.V);
    const int R = (env_r == 2 || env_r == 4 || env_r == 8) ? env_r : LMQ_R_DEFAULT;
    if (!xlds) lmq_launch<FMT, NB, LMQ_R_DEFAULT, PROC, false>(a, pr, nparts, 0);     // activations through L2: one form
    else if (R == 2) lmq_launch<FMT, NB, 2, PROC, true>(a, pr, nparts, lds);
    else if (R == 4) lmq_launch<FMT, NB, 4, PROC, true>(a, pr, nparts, lds);
    else lmq_launch<FMT, NB, 8, PROC, true>(a, pr, nparts, lds);
    SPIDER_LAUNCH_OK();
    argmax_final_kernel<<<a.B, 256, 0, (hipStream_t)a.stream>>>((const float*)a.ws_val, (const int*)a.ws_idx, a.out_ids, nparts);
    SPIDER_LAUNCH_OK();
    return 0;
}

// everything a launch relies on, checked on the host before any launch
template <int FMT>
int lmq_check(const char* who, const LmqArgs& a) {
    if (a.V <= 0 || a.K <= 0 || a.K % WQ_LW<FMT> != 0) return wq_fail(who, WQ_K_RULE<FMT>);
    if (a.B < 1 || a.B > 4) return wq_fail(who, "batch must be 1..4 (more rows take the bf16 lm_head on the dequantised weights)");
    if (!a.q || !a.scale || !a.x || !a.out_ids || !a.ws_val || !a.ws_idx)
        return wq_fail(who, "weights, scales, x, out_ids and both workspaces must not be null");
    return 0;
}

template <int FMT, bool PROC>
int lmq_batch(const LmqArgs& a, const LmProc& pr) {
    switch (a.B) {
        case 1: return lmq_dispatch<FMT, 1, PROC>(a, pr);
        case 2: return lmq_dispatch<FMT, 2, PROC>(a, pr);
        case 3: return lmq_dispatch<FMT, 3, PROC>(a, pr);
        default: return lmq_dispatch<FMT, 4, PROC>(a, pr);
    }
}

int lmq_proc_make(const char* who, LmProc& pr, const void* seen, const void* ban, const float* penalty, const int* min_new,
                  const int* eos_ids, const int* n_eos, const int* n_hist, int V) {
    if (!(seen && ban && penalty && min_new && eos_ids && n_eos && n_hist))
        return wq_fail(who, "seen, ban, penalty, min_new, eos_ids, n_eos and n_hist are required");
    pr = LmProc{(const uint32_t*)seen, (const uint32_t*)ban, penalty, min_new, eos_ids, n_eos, n_hist, (V + 31) / 32};
    return 0;
}

}  // namespace

extern "C" {

int spider_lm_head_argmax_w8(const void* q, const void* scale, const void* x, const void* norm_w, float eps, int* out_ids,
                             void* logits, void* ws_val, void* ws_idx, int B, int V, int K, void* stream) {
    const LmqArgs a{q, scale, x, norm_w, eps, out_ids, logits, ws_val, ws_idx, B, V, K, stream};
    if (lmq_check<8>("lm_head_argmax_w8", a)) return -1;
    return lmq_batch<8, false>(a, LmProc{});
}

int spider_lm_head_argmax_proc_w8(const void* q, const void* scale, const void* x, const void* norm_w, float eps, int* out_ids,
                                  void* logits, void* ws_val, void* ws_idx, const void* seen, const void* ban, const float* penalty,
                                  const int* min_new, const int* eos_ids, const int* n_eos, const int* n_hist, int B, int V, int K,
                                  void* stream) {
    const LmqArgs a{q, scale, x, norm_w, eps, out_ids, logits, ws_val, ws_idx, B, V, K, stream};
    if (lmq_check<8>("lm_head_argmax_proc_w8", a)) return -1;
    LmProc pr;
    if (lmq_proc_make("lm_head_argmax_proc_w8", pr, seen, ban, penalty, min_new, eos_ids, n_eos, n_hist, V)) return -1;
    return lmq_batch<8, true>(a, pr);
}

int spider_lm_head_argmax_w4(const void* blocks, const void* scales, const void* x, const void* norm_w, float eps, int* out_ids,
                             void* logits, void* ws_val, void* ws_idx, int B, int V, int K, void* stream) {
    const LmqArgs a{blocks, scales, x, norm_w, eps, out_ids, logits, ws_val, ws_idx, B, V, K, stream};
    if (lmq_check<4>("lm_head_argmax_w4", a)) return -1;
    return lmq_batch<4, false>(a, LmProc{});
}

int spider_lm_head_argmax_proc_w4(const void* blocks, const void* scales, const void* x, const void* norm_w, float eps, int* out_ids,
                                  void* logits, void* ws_val, void* ws_idx, const void* seen, const void* ban, const float* penalty,
                                  const int* min_new, const int* eos_ids, const int* n_eos, const int* n_hist, int B, int V, int K,
                                  void* stream) {
    const LmqArgs a{blocks, scales, x, norm_w, eps, out_ids, logits, ws_val, ws_idx, B, V, K, stream};
    if (lmq_check<4>("lm_head_argmax_proc_w4", a)) return -1;
    LmProc pr;
    if (lmq_proc_make("lm_head_argmax_proc_w4", pr, seen, ban, penalty, min_new, eos_ids, n_eos, n_hist, V)) return -1;
    return lmq_batch<4, true>(a, pr);
}

}  // extern "C"

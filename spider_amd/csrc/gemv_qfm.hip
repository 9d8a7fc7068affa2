// Weight-only MXFP4 / FP8 forms of the fragment-major skinny MFMA GEMM of llm_decode.hip (skinny_fm_kernel), 1..16 sequences
// (gfx950 / CDNA4): the batched decode steps of a quantised engine, where the row-major gemv_w4 / gemv_w8 are VALU- and LDS-bound.
//
//   out[b, n] = epilogue( sum_k x[b, k] * W_eff[n, k] ),   b < B <= 16
//   MXFP4: qfm [NG, K / 128, 64, 16] bytes + efm [NG, K / 128, 16, 4] bytes (spider_amd.ops.repack_fm_w4), K % 128 == 0.
//          Piece (rg, kb) is 1 KiB = 16 weight rows x 128 weights; lane 16 g + r holds 16 bytes whose dword sx (0..3) is
//          W[16 rg + r][128 kb + 32 sx + 8 g .. + 7] as e2m1 codes, low nibble first: the lane's A fragment of MFMA sub-step sx.
//          efm dword (rg, kb, r) holds the E8M0 bytes of that row's four blocks of 32, byte sx for sub-step sx (one MX block is one
//          sub-step), shared by the row's four g lanes. W_eff = e2m1(code) * 2^(byte - 127), bytes 1..254.
//   FP8:   qfm [NG, K / 64, 64, 16] bytes (spider_amd.ops.repack_fm_w8), K % 64 == 0, + scale [N] fp32 (the public per-row scale).
//          Piece (rg, kb) is 1 KiB = 16 rows x 64 weights; in lane 16 g + r byte 8 sx + e is q[16 rg + r][64 kb + 32 sx + 8 g + e].
//          W_eff = f32(q) * scale[n].
//   epilogue: MODE 0 (+bias) -> bf16 -> (+res -> bf16);  MODE 1: the copy holds [gate groups | up groups] (I % 16 == 0) and
//          out[b, n] = bf16(bf16(silu(bf16(g))) * bf16(u)) -- the contracts of gemv_w4 / gemv_w8, rounding for rounding.
//   No fused RMSNorm: repack_fm16 folds norm_w into the bf16 weights, a quantised matrix cannot carry it; the caller normalises.
//
// What it keeps from skinny_fm_kernel: one row group per block, K split over the block's 8 waves, D pieces in flight per wave, one
// b128 weight load per lane and piece (1 KiB contiguous per wave instruction), the <= 16 activation rows as the B operand in
// natural k order with rows >= B read as zeros through the buffer range, partial tiles summed through LDS by wave 0.
// What differs is the weight decode in front of v_mfma_f32_16x16x32_bf16:
//   MXFP4: four v_cvt_scalef32_pk_bf16_fp4 per sub-step (one per weight byte) with the f32 scale operand uint32(byte) << 23, as in
//          gemv_wq.hip: exact (two significand bits times a power of two).
//   FP8:   four v_cvt_scalef32_pk_bf16_fp8 per sub-step with the scale operand 1.0f, and scale[n] applied to the fp32 accumulators
//          in the epilogue, instead of the row's scale as the conversion's operand. Read from the ISA: either form is one conversion
//          per two weights, so they cost the same VALU work; this one needs no per-lane scale register in the loop, multiplies the
//          finished sum exactly where gemv_w8 does (acc * scale[n]), and does not need the scale to be a power of two.
// Loads past a wave's K range use the all-ones offset of skinny_fm_kernel: weights, activations AND the MXFP4 scale dword read as
// zeros. Scale byte 0 is the operand +0.0f, whose exponent field the conversion reads as 2^-127; the nibbles beside it are code 0, and
// 0 * 2^-127 = 0 meets a zero activation: the sub-step adds +0 to the accumulator. No NaN can arise (only byte 255 is one).
#include "wq_common.hpp"

using namespace spider;

namespace {

// FMT: 4 = MXFP4 (SUB = 4 sub-steps of 32 weights per piece), 8 = FP8 (SUB = 2). MODE 0 / 1 as above. D: pieces in flight per wave.
template <int FMT, int MODE, int NW, int D>
__global__ __launch_bounds__(NW * 64) void qfm_kernel(const uint8_t* __restrict__ qfm, const uint8_t* __restrict__ efm,
                                                      const float* __restrict__ scale, const bf16_t* __restrict__ x,
                                                      bf16_t* __restrict__ out, const bf16_t* __restrict__ bias,
                                                      const bf16_t* __restrict__ res, int B, int N, int K, int NG,
                                                      uint32_t w_bytes, uint32_t e_bytes, uint32_t x_bytes) {
    constexpr bool GATEUP = MODE == 1;
    constexpr int TN = GATEUP ? 2 : 1;
    constexpr int SUB = FMT == 4 ? 4 : 2;
    constexpr int KP = 32 * SUB;                    // weights of one row in a piece
    __shared__ float part[NW][TN][64][4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(qfm), 0, w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t re = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(FMT == 4 ? efm : qfm), 0, FMT == 4 ? e_bytes : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(x), 0, x_bytes, 0x00020000);
    const uint32_t xbase = (uint32_t)r16 * (uint32_t)K * 2u + 16u * g;      // rows >= B lie beyond x_bytes: read as zeros
    const int nkb = K / KP;
    const int kb0 = (wave * nkb) / NW, kb1 = ((wave + 1) * nkb) / NW;
    const int rg = blockIdx.x;

    uint32_t wbase[TN], ebase[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const uint32_t grp = (uint32_t)(t * NG + rg) * (uint32_t)nkb;
        wbase[t] = grp * 1024u + 16u * lane;
        ebase[t] = grp * 64u + 4u * r16;
    }
    f32x4 acc[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 wq[D][TN], xq[D][SUB];
    uint32_t eq[D][TN];
    auto issue = [&](int kb, int s) {
        const uint32_t inv = (uint32_t)((kb1 - 1 - kb) >> 31);              // all ones past this wave's K range: zeros
        const uint32_t kw = (uint32_t)kb * 1024u, ke = (uint32_t)kb * 64u, kx = (uint32_t)kb * (uint32_t)(KP * 2);
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            wq[s][t] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (wbase[t] + kw) | inv, 0, 2));
            if (FMT == 4) eq[s][t] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(re, (ebase[t] + ke) | inv, 0, 0);
        }
#pragma unroll
        for (int sx = 0; sx < SUB; ++sx)
            xq[s][sx] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (xbase + kx + 64u * sx) | inv, 0, 0));
    };
#pragma unroll
    for (int s = 0; s < D; ++s) issue(kb0 + s, s);
    for (int kb = kb0; kb < kb1; kb += D) {
#pragma unroll
        for (int s = 0; s < D; ++s) {
#pragma unroll
            for (int sx = 0; sx < SUB; ++sx) {
                const bf16x8 xf = __builtin_bit_cast(bf16x8, xq[s][sx]);
#pragma unroll
                for (int t = 0; t < TN; ++t) {
                    u32x4 a;
                    if (FMT == 4) {
                        const uint32_t w = wq[s][t][sx];
                        const float sc = e8m0_to_f32((eq[s][t] >> (8 * sx)) & 0xffu);
                        a[0] = fp4x2_to_bf16x2<0>(w, sc); a[1] = fp4x2_to_bf16x2<1>(w, sc); a[2] = fp4x2_to_bf16x2<2>(w, sc); a[3] = fp4x2_to_bf16x2<3>(w, sc);
                    } else {
                        const uint32_t w0 = wq[s][t][2 * sx], w1 = wq[s][t][2 * sx + 1];
                        a[0] = fp8x2_to_bf16x2<false>(w0); a[1] = fp8x2_to_bf16x2<true>(w0); a[2] = fp8x2_to_bf16x2<false>(w1); a[3] = fp8x2_to_bf16x2<true>(w1);
                    }
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), xf, acc[t], 0, 0, 0);
                }
            }
            issue(kb + D + s, s);
            __builtin_amdgcn_sched_barrier(0);      // keep "consume slot s, refill slot s" in this order
        }
    }
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[wave][t][lane][j] = acc[t][j];
    __syncthreads();
    if (wave != 0) return;
    // lane holds D[n = 16 rg + 4 g + j][m = r16]
    const int m = r16;
    if (m >= B) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int nn = 16 * rg + 4 * g + j;
        if (nn >= N) continue;
        float v[TN];
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) a += part[w][t][lane][j];
            v[t] = FMT == 8 ? a * scale[t * N + nn] : a;
        }
        float o;
        if (GATEUP) {
            const float gg = bf16_to_f32(f32_to_bf16(v[0])), uu = bf16_to_f32(f32_to_bf16(v[TN - 1]));
            o = bf16_to_f32(f32_to_bf16(silu_f(gg))) * uu;
        } else {
            o = v[0];
            if (bias) o += bf16_to_f32(bias[nn]);
            if (res) o = bf16_to_f32(f32_to_bf16(o)) + bf16_to_f32(res[(size_t)m * N + nn]);
        }
        out[(size_t)m * N + nn] = f32_to_bf16(o);
    }
}

// everything a launch relies on, checked on the host before any launch. rows = weight rows of the copy (N, or 2 I).
int qfm_check(const char* who, int fmt, const void* qfm, const void* sc, const void* x, const void* out, int B, int N, int K, bool gateup) {
    const int kp = fmt == 4 ? 128 : 64;
    const char* why = nullptr;
    if (N <= 0 || K <= 0 || K % kp != 0) why = fmt == 4 ? "K must be a positive multiple of 128 (one piece is 16 rows x 128 weights)"
                                                        : "K must be a positive multiple of 64 (one piece is 16 rows x 64 weights)";
    else if (B < 1 || B > 16) why = "batch must be 1..16 (the rows are the B operand of one 16-wide MFMA tile)";
    else if (gateup && N % 16 != 0) why = "I must be a multiple of 16";
    else if (!qfm || !sc || !x || !out) why = "weights, scales, x and out must not be null";
    else {
        const size_t groups = (size_t)(gateup ? 2 : 1) * ((N + 15) / 16);
        if (groups * 16 * K / (fmt == 4 ? 2 : 1) >= ((size_t)1 << 32) || (size_t)B * K * 2 >= ((size_t)1 << 32)) why = "weight copy must be < 4 GiB";
    }
    return why ? wq_fail(who, why) : 0;
}

// Pieces in flight per wave: 2, as skinny_fm_kernel keeps two k blocks. Measured against 4 (scripts/exp/qfm_decode_cost.py --ops-only
// under SPIDER_QFM_D, Qwen2.5-7B shapes, 8 rows, us per launch with cold weights, 2 -> 4 pieces): FP8 qkv 9.8 -> 10.1, o 6.6 -> 6.8,
// gate/up 26.7 -> 34.3, down 17.9 -> 19.2; MXFP4 9.3 -> 10.5, 5.9 -> 6.8, 23.1 -> 29.5, 15.7 -> 17.7. Four is slower everywhere
// (registers do not explain it: the FP8 forms stay below 128 VGPRs with four pieces, only the MXFP4 gate/up form does not). Supposed,
// not measured: every piece in flight brings SUB 16-byte activation loads per lane with it (4 KiB per wave instruction set against the
// piece's 1 KiB), and those loads, not the weight bytes, occupy the CU's vector memory path.
template <int FMT, int MODE>
int qfm_launch(const void* qfm, const void* efm, const float* scale, const void* x, void* out, const void* bias, const void* res,
               int B, int N, int K, void* stream) {
    // tuning aid, read once: SPIDER_QFM_D = 2 / 4 pieces in flight for both formats
    static const int env_d = wq_env("SPIDER_QFM_D", 0);
    const int d = (env_d == 2 || env_d == 4) ? env_d : 2;
    const int NG = (N + 15) / 16;
    const size_t groups = (size_t)(MODE == 1 ? 2 : 1) * NG;
    const size_t wb = groups * 16 * (size_t)K / (FMT == 4 ? 2 : 1), eb = FMT == 4 ? groups * 16 * (size_t)(K / 32) : 0, xb = (size_t)B * K * 2;
#define QFM_GO(D_) qfm_kernel<FMT, MODE, 8, D_><<<NG, 512, 0, (hipStream_t)stream>>>((const uint8_t*)qfm, (const uint8_t*)efm, scale, \
        (const bf16_t*)x, (bf16_t*)out, (const bf16_t*)bias, (const bf16_t*)res, B, N, K, NG, (uint32_t)wb, (uint32_t)eb, (uint32_t)xb)
    if (d == 2) QFM_GO(2); else QFM_GO(4);
#undef QFM_GO
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // namespace

extern "C" {

int spider_gemv_fm_w4(const void* qfm, const void* efm, const void* x, void* out, const void* bias, const void* res, int B, int N,
                      int K, void* stream) {
    if (qfm_check("gemv_fm_w4", 4, qfm, efm, x, out, B, N, K, false)) return -1;
    return qfm_launch<4, 0>(qfm, efm, nullptr, x, out, bias, res, B, N, K, stream);
}

int spider_gemv_swiglu_fm_w4(const void* qfm_gate_up, const void* efm, const void* x, void* out, int B, int I, int K, void* stream) {
    if (qfm_check("gemv_swiglu_fm_w4", 4, qfm_gate_up, efm, x, out, B, I, K, true)) return -1;
    return qfm_launch<4, 1>(qfm_gate_up, efm, nullptr, x, out, nullptr, nullptr, B, I, K, stream);
}

int spider_gemv_fm_w8(const void* qfm, const float* scale, const void* x, void* out, const void* bias, const void* res, int B, int N,
                      int K, void* stream) {
    if (qfm_check("gemv_fm_w8", 8, qfm, scale, x, out, B, N, K, false)) return -1;
    return qfm_launch<8, 0>(qfm, nullptr, scale, x, out, bias, res, B, N, K, stream);
}

int spider_gemv_swiglu_fm_w8(const void* qfm_gate_up, const float* scale, const void* x, void* out, int B, int I, int K, void* stream) {
    if (qfm_check("gemv_swiglu_fm_w8", 8, qfm_gate_up, scale, x, out, B, I, K, true)) return -1;
    return qfm_launch<8, 1>(qfm_gate_up, nullptr, scale, x, out, nullptr, nullptr, B, I, K, stream);
}

}  // extern "C"

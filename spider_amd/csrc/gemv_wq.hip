// Weight-only FP8 (OCP e4m3fn) and MXFP4 (OCP Microscaling: e2m1 nibbles, one E8M0 scale per block of 32) siblings of the row-major
// decode GEMVs of llm_decode.hip, 1..4 sequences (gfx950 / CDNA4). One kernel template, FMT = 8 / 4 (wq_common.hpp).
//
//   out[b, n] = epilogue( sum_k xin[b, k] * W_eff[n, k] ),   b < NB <= 4
//   FP8   (spider_gemv[_swiglu]_w8): q [N, K] bytes, OCP e4m3fn (max 448 = 0x7e, 1.0 = 0x38; NOT MI300's fnuz), row-major,
//          K % 16 == 0; scale [N] fp32, one per weight row; W_eff[n, k] = f32(q[n, k]) * scale[n]. A power of two in the engine:
//          float(q) * scale is then a bf16 number, and the launch computes the bf16 GEMV on those weights up to summation order
//          (spider_amd/llm.py: quantize_fp8_rows).
//   MXFP4 (spider_gemv[_swiglu]_w4): blocks [N, K / 2] bytes, row-major: byte j of row n holds weight k = 2 j in its low nibble and
//          k = 2 j + 1 in its high nibble; nibble code c has sign bit 3 and magnitude [0, .5, 1, 1.5, 2, 3, 4, 6][c & 7]; K % 32 == 0;
//          scales [N, K / 32] bytes, row-major, E8M0: W_eff[n, k] = e2m1(code) * 2^(scales[n, k / 32] - 127), bytes 1..254
//          (the layout of spider_amd/llm.py: quantize_mxfp4, which emits 2..252: every non-zero W_eff is a normal bf16 number)
//   xin    x, or RMSNorm(x) * norm_w with the normalised activation rounded to bf16 exactly as gemv_kernel does
//   epilogue: (+bias) -> bf16 -> (+res -> bf16);  GATEUP: the weights hold [gate rows | up rows] (2 N rows, and their scales) and
//          out[b, n] = bf16(bf16(silu(bf16(g))) * bf16(u))
//
// What it keeps from gemv_kernel: each wave owns R output columns and streams their rows with 16-byte
// nontemporal loads; the first U chunks of every row are requested BEFORE the activation prologue, behind the first batch of x
// (stage_rows_branchfree); loads are unconditional on clamped addresses and only the FMAs are predicated; activations are staged
// once per block in LDS.
// What differs: the weight decode in front of v_dot2c_f32_bf16, where every product is exact, the accumulator is fp32 and no
// activation is unpacked.
//   FP8:   a lane's load is 16 weights, 1024 per wave instruction. A weight word (4 bytes) becomes two packed bf16 pairs --
//          v_cvt_pk_f32_fp8 (two values per instruction), then v_cvt_pk_bf16_f32, exact because e4m3 has 3 significand bits: 1 + NB / 2
//          VALU operations per weight. scale[n] multiplies the fp32 sum once, after the wave reduction.
//   MXFP4: a lane's load is 32 weights = exactly one MX block, so one scale byte belongs to one load and a wave instruction covers
//          2048 weights. The f32 scale operand is uint32(byte) << 23 (valid for bytes 1..254) and every weight byte becomes a packed
//          bf16 pair with one v_cvt_scalef32_pk_bf16_fp4: the scale is applied inside the conversion, exactly (two significand bits
//          times a power of two), because it differs from block to block and cannot leave the sum as FP8's per-row scale does:
//          1/2 + NB / 2 VALU operations per weight. Scale loads: one byte load per lane per weight load from the public [N, K / 32]
//          layout (the 64 lanes of a wave read 64 contiguous bytes). A chunk-transposed private layout with one dword per lane for
//          four chunks was not built or measured.
//
// In row order a lane's two (FP8) or four (MXFP4) 16-byte LDS reads would sit 32 / 64 bytes apart from lane to lane and touch a part
// of the banks each (by the bank arithmetic; not measured); the staged copy is swizzled per chunk (wq_slot) so that each read is
// lane-contiguous (64 lanes x 16 bytes = every bank four times, the minimum for a 16-byte read). Rows are padded to whole chunks in
// LDS. The budget is the CU's whole LDS (FP8, the long-K down projection at 2..4 sequences: 76 / 114 / 152 KiB, one or two blocks per
// CU); when the padded copy exceeds it the waves read x through L2 (no fused norm then, as in gemv_kernel).
#include "wq_common.hpp"

using namespace spider;

namespace {

// dispatch defaults (measured: scripts/exp/fp8_decode_cost.py)
// FP8, Qwen2.5-7B shapes, us per launch with cold weights at 1 / 2 / 3 / 4 sequences:
//   gate/up (K = 3584), one -> two columns per wave:      23.8 -> 24.4 | 31.7 -> 28.6 | 40.8 -> 35.4 | 52.5 -> 43.3
//   down (K = 18944), activations through L2 -> in LDS:   (14.1: fits 64 KiB) | 21.1 -> 15.8 | 29.2 -> 17.5 | 32.4 -> 20.3
//   8 waves per block below K = 8192: slower everywhere (gate/up 23.8 -> 27.3 | 31.7 -> 39.7 | 40.8 -> 46.1 | 52.5 -> 55.7)
// MXFP4 takes the same rules. Measured against one / two columns everywhere and 4 / 8 waves everywhere
// (scripts/exp/mxfp4_decode_cost.py --ops-only, Qwen2.5-7B shapes, table in NOTEBOOK.md): nothing beats them by more than 0.5 us per
// launch, one column from two sequences on and 8 waves below K = 8192 lose up to 20 us.
#define WQ_GU_R_MULTI 2                          // output columns per wave of the gate/up form from two sequences on

template <int FMT, int NB, int R, bool GATEUP, bool XLDS, int NWB>
__global__ __launch_bounds__(NWB * 64) void gemv_wq_kernel(const uint8_t* __restrict__ Wq, const void* __restrict__ scale_,
                                                      const bf16_t* __restrict__ x, bf16_t* __restrict__ out,
                                                      const bf16_t* __restrict__ bias, const bf16_t* __restrict__ res,
                                                      const bf16_t* __restrict__ norm_w, float eps, int N, int K) {
    static_assert(FMT == 8 || FMT == 4, "FMT: 8 (FP8) or 4 (MXFP4)");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float red[NWB];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int LW = WQ_LW<FMT>, CHUNK = WQ_CHUNK<FMT>, NP = LW / 8;   // NP: 8-weight pieces = 16-byte LDS reads per load
    constexpr int NR = GATEUP ? 2 * R : R;     // weight rows per wave
    constexpr int U = (NR * NB <= 4) ? 4 : 2;  // chunks in flight per row
    const int KP = (K + CHUNK - 1) & ~(CHUNK - 1);   // LDS row length in elements (whole chunks)
    const float* scale8 = reinterpret_cast<const float*>(scale_);       // FMT 8: [N] row scales
    const uint8_t* scale4 = reinterpret_cast<const uint8_t*>(scale_);   // FMT 4: [N, K / 32] block scales

    const int col0 = (blockIdx.x * NWB + wave) * R;
    const uint8_t* wrow[NR];
    const uint8_t* srow[NR];                   // FMT 4 only
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int n = col0 + r;
        n = n < N ? n : N - 1;
        if constexpr (FMT == 8) {
            wrow[r] = Wq + (size_t)n * K;
            if (GATEUP) wrow[R + r] = Wq + (size_t)(N + n) * K;
        } else {
            wrow[r] = Wq + (size_t)n * (K / 2);
            srow[r] = scale4 + (size_t)n * (K / 32);
            if (GATEUP) {
                wrow[R + r] = Wq + (size_t)(N + n) * (K / 2);
                srow[R + r] = scale4 + (size_t)(N + n) * (K / 32);
            }
        }
    }
    // lane l of chunk u: weights base + CHUNK u + LW l .. + LW - 1 = 16 bytes of the row and (FMT 4) scale byte (that k) / 32
    struct WSet {
        u32x4 q[U][NR];
        uint32_t sc[U][NR];                    // FMT 4 only
    };
    auto load_set = [&](WSet& w, int base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = base + lane * LW + u * CHUNK;
            const unsigned kc = (unsigned)(k < K ? k : K - LW);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                w.q[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[r] + (FMT == 8 ? kc : kc >> 1)));
                if constexpr (FMT == 4) w.sc[u][r] = srow[r][kc >> 5];
            }
        }
    };
    WSet w0;

    if constexpr (!XLDS) load_set(w0, 0);
    else stage_rows_branchfree<NB, NWB>(x, norm_w, eps, K, KP / 8, reinterpret_cast<u32x4*>(smem), red,
                                        [](int i) { return wq_slot<FMT>(i); }, [&]() { load_set(w0, 0); });

    if (col0 >= N) return;      // wave-uniform
    float acc[NB][NR];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[b][r] = 0.f;

    const bf16_t* xs = reinterpret_cast<const bf16_t*>(smem);
    // piece p of the lane's activations for sequence b
    auto load_x = [&](int b, int kc, int k, int p) {
        if (XLDS) return *reinterpret_cast<const u32x4*>(xs + (size_t)b * KP + kc + p * 512 + lane * 8);
        return *reinterpret_cast<const u32x4*>(x + (size_t)b * K + k + p * 8);
    };
    // one set of chunks against the activations; a lane's LW weights are wholly inside the row or wholly past it (K % LW == 0).
    // Every accumulator takes its pieces in k order in both formats; what differs is the schedule the registers were measured with.
    auto fma_set = [&](const WSet& w, int base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kc = base + u * CHUNK, k = kc + lane * LW;
            if (k < K) {
                uint32_t wb[NR][NP][4];
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const uint32_t ww[4] = {w.q[u][r].x, w.q[u][r].y, w.q[u][r].z, w.q[u][r].w};
#pragma unroll
                    for (int p = 0; p < NP; ++p) wq_decode_piece<FMT>(ww, p, FMT == 4 ? w.sc[u][r] : 0u, wb[r][p]);
                }
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    if constexpr (FMT == 8) {      // both reads, then the 8 dot products of each row
                        const u32x4 xa = load_x(b, kc, k, 0), xb = load_x(b, kc, k, 1);
                        const uint32_t xw[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
                        for (int r = 0; r < NR; ++r)
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc[b][r] = dot2_bf16(wb[r][j >> 2][j & 3], xw[j], acc[b][r]);
                    } else {                       // one read at a time
#pragma unroll
                        for (int p = 0; p < NP; ++p) {
                            const u32x4 xa = load_x(b, kc, k, p);
                            const uint32_t xw[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
                            for (int r = 0; r < NR; ++r)
#pragma unroll
                                for (int j = 0; j < 4; ++j) acc[b][r] = dot2_bf16(wb[r][p][j], xw[j], acc[b][r]);
                        }
                    }
                }
            }
        }
    };
    fma_set(w0, 0);
    for (int base = CHUNK * U; base < K; base += CHUNK * U) {     // uniform trip count: the wave reconverges for the reduction
        WSet w;
        load_set(w, base);
        fma_set(w, base);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[b][r] = wave_sum_valu(acc[b][r]);

    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int n = col0 + r;
            if (n < N) {
                // FMT 8: the row scales, applied to the finished sums; FMT 4: the scales are already inside
                float s0 = 1.f, s1 = 1.f;
                if constexpr (FMT == 8) { s0 = scale8[n]; s1 = GATEUP ? scale8[N + n] : 0.f; }
                auto scaled = [](float a, float s) { return FMT == 8 ? a * s : a; };
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    float v;
                    if (GATEUP) {
                        const float g = bf16_to_f32(f32_to_bf16(scaled(acc[b][r], s0)));
                        const float u = bf16_to_f32(f32_to_bf16(scaled(acc[b][R + r], s1)));
                        const float a = bf16_to_f32(f32_to_bf16(silu_f(g)));
                        v = a * u;
                    } else {
                        v = scaled(acc[b][r], s0);
                        if (bias) v += bf16_to_f32(bias[n]);
                        if (res) v = bf16_to_f32(f32_to_bf16(v)) + bf16_to_f32(res[(size_t)b * N + n]);
                    }
                    out[(size_t)b * N + n] = f32_to_bf16(v);
                }
            }
        }
    }
}

struct WqArgs {
    const void *Wq, *scale, *x;
    void* out;
    const void *bias, *res, *norm_w;
    float eps;
    int B, N, K;
    void* stream;
};

template <int FMT, int NB, int R, bool GU, bool XL, int NWB>
void gemv_wq_launch(const WqArgs& a, size_t lds) {
    auto* fn = gemv_wq_kernel<FMT, NB, R, GU, XL, NWB>;
    if (XL && lds > WQ_LDS_DEFAULT_LIMIT) {
        static unsigned raised = 0;
        raise_dynamic_lds(fn, (int)WQ_LDS_HW_LIMIT, raised);
    }
    fn<<<(a.N + NWB * R - 1) / (NWB * R), NWB * 64, XL ? lds : 0, (hipStream_t)a.stream>>>(
        (const uint8_t*)a.Wq, a.scale, (const bf16_t*)a.x, (bf16_t*)a.out, (const bf16_t*)a.bias, (const bf16_t*)a.res,
        (const bf16_t*)a.norm_w, a.eps, a.N, a.K);
}

template <int FMT, int NB, bool GU>
int gemv_wq_dispatch(const char* who, const WqArgs& a) {
    // tuning aids, read once: SPIDER_W8_LDS_MAX / SPIDER_W4_LDS_MAX (bytes of staged activations per block; ops.w8_norm_fits /
    // w4_norm_fits mirror them), SPIDER_W8_NWB / SPIDER_W4_NWB (4 / 8 waves per block), SPIDER_W8_R / SPIDER_W4_R and
    // SPIDER_W8_GU_R / SPIDER_W4_GU_R (output columns per wave of the plain / gate-up form, 1 / 2)
    static const int env_nwb = wq_env(FMT == 8 ? "SPIDER_W8_NWB" : "SPIDER_W4_NWB", 0);
    static const int env_r = wq_env(FMT == 8 ? (GU ? "SPIDER_W8_GU_R" : "SPIDER_W8_R") : (GU ? "SPIDER_W4_GU_R" : "SPIDER_W4_R"), 0);
    const size_t lds = wq_lds_bytes<FMT>(NB, a.K);
    const bool xlds = lds <= wq_lds_max<FMT>();
    if (!xlds && a.norm_w) return wq_fail(who, WQ_NORM_RULE<FMT>);
    // Output columns per wave. A block stages batch * K * 2 bytes of activations for the NWB * R * K weight bytes (FP8; half of
    // that in MXFP4) per column set it streams, at most half of what the same block of the bf16 kernel streams, so from two
    // sequences on the staging is amortised over two columns per wave; one column for single-sequence matrices below 24 Mi
    // weights, where more blocks in flight hide the prologue (gemv_dispatch's rule), and for the single-sequence gate/up form
    // (two weight rows per column already).
    int R = GU ? (NB >= 2 ? WQ_GU_R_MULTI : 1) : ((NB >= 2 || (size_t)a.N * a.K >= ((size_t)24 << 20)) ? 2 : 1);
    if (env_r == 1 || env_r == 2) R = env_r;
    // Waves per block: a function of K alone, so that the plain and the gate/up form of one shape reduce the RMSNorm sum of
    // squares in the same order. 8 waves share one staged copy of a long row (the down projection); for short rows 8 are slower.
    int nwb = a.K >= 8192 ? 8 : 4;
    if (env_nwb == 4 || env_nwb == 8) nwb = env_nwb;
#define WQ_GO(R_, XL_, NWB_) gemv_wq_launch<FMT, NB, R_, GU, XL_, NWB_>(a, lds)
#define WQ_PICK(R_)                                                            \
    do {                                                                       \
        if (xlds) { if (nwb == 8) WQ_GO(R_, true, 8); else WQ_GO(R_, true, 4); } \
        else      { if (nwb == 8) WQ_GO(R_, false, 8); else WQ_GO(R_, false, 4); } \
    } while (0)
    if (R == 1) WQ_PICK(1); else WQ_PICK(2);
#undef WQ_PICK
#undef WQ_GO
    SPIDER_LAUNCH_OK();
    return 0;
}

// everything a launch relies on, checked on the host before any launch; then the batch switch
template <int FMT, bool GU>
int gemv_wq(const char* who, const WqArgs& a) {
    if (a.N <= 0 || a.K <= 0 || a.K % WQ_LW<FMT> != 0) return wq_fail(who, WQ_K_RULE<FMT>);
    if (a.B < 1 || a.B > 4) return wq_fail(who, "batch must be 1..4 (more rows take the bf16 kernels on the dequantised weights)");
    if (!a.Wq || !a.scale || !a.x || !a.out) return wq_fail(who, "weights, scales, x and out must not be null");
    switch (a.B) {
        case 1: return gemv_wq_dispatch<FMT, 1, GU>(who, a);
        case 2: return gemv_wq_dispatch<FMT, 2, GU>(who, a);
        case 3: return gemv_wq_dispatch<FMT, 3, GU>(who, a);
        default: return gemv_wq_dispatch<FMT, 4, GU>(who, a);
    }
}

}  // namespace

extern "C" {

int spider_gemv_w8(const void* Wq, const float* scale, const void* x, void* out, const void* bias, const void* res,
                   const void* norm_w, float eps, int B, int N, int K, void* stream) {
    return gemv_wq<8, false>("gemv_w8", WqArgs{Wq, scale, x, out, bias, res, norm_w, eps, B, N, K, stream});
}

int spider_gemv_swiglu_w8(const void* Wq_gate_up, const float* scale, const void* x, void* out, const void* norm_w, float eps,
                          int B, int I, int K, void* stream) {
    return gemv_wq<8, true>("gemv_swiglu_w8", WqArgs{Wq_gate_up, scale, x, out, nullptr, nullptr, norm_w, eps, B, I, K, stream});
}

int spider_gemv_w4(const void* blocks, const void* scales, const void* x, void* out, const void* bias, const void* res,
                   const void* norm_w, float eps, int B, int N, int K, void* stream) {
    return gemv_wq<4, false>("gemv_w4", WqArgs{blocks, scales, x, out, bias, res, norm_w, eps, B, N, K, stream});
}

int spider_gemv_swiglu_w4(const void* blocks_gate_up, const void* scales, const void* x, void* out, const void* norm_w, float eps,
                          int B, int I, int K, void* stream) {
    return gemv_wq<4, true>("gemv_swiglu_w4", WqArgs{blocks_gate_up, scales, x, out, nullptr, nullptr, norm_w, eps, B, I, K, stream});
}

}  // extern "C"

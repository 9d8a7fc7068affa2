// Weight-only FP8 (OCP e4m3fn) siblings of the row-major decode GEMVs of llm_decode.hip, 1..4 sequences (gfx950 / CDNA4).
//
//   out[b, n] = epilogue( scale[n] * sum_k xin[b, k] * f32(q[n, k]) ),   b < NB <= 4
//   q      [N, K] bytes: OCP e4m3fn (max 448 = 0x7e, 1.0 = 0x38; NOT MI300's fnuz), row-major, K % 16 == 0
//   scale  [N] fp32, one per weight row (a power of two in the engine: float(q) * scale is then a bf16 number, and the
//          launch computes the bf16 GEMV on those weights up to summation order -- spider_amd/llm.py: quantize_fp8_rows)
//   xin    x, or RMSNorm(x) * norm_w with the normalised activation rounded to bf16 exactly as gemv_kernel does
//   epilogue: (+bias) -> bf16 -> (+res -> bf16);  GATEUP: q holds [gate rows | up rows] (2 N rows, 2 N scales) and
//          out[b, n] = bf16(bf16(silu(bf16(g))) * bf16(u))
//
// What it keeps from gemv_kernel: each wave owns R output columns and streams their rows with 16-byte
// nontemporal loads -- 16 weights per lane, 1024 per wave instruction; the first U chunks of every row are requested BEFORE the
// activation prologue, behind the first batch of x (vmcnt retires in order, so the wait for x leaves them in flight); loads are
// unconditional on clamped addresses and only the FMAs are predicated; activations are staged once per block in LDS.
// What differs: a weight word (4 bytes) becomes two packed bf16 pairs -- v_cvt_pk_f32_fp8 (two values per instruction), then
// v_cvt_pk_bf16_f32, exact because e4m3 has 3 significand bits -- and meets the activations in v_dot2c_f32_bf16 as the bf16
// kernel's weights do: every product is exact, the accumulator is fp32, and no activation is unpacked. That is 1 + NB / 2
// VALU operations per weight. scale[n] multiplies the fp32 sum once, after the wave reduction.
//
// A lane's 16 weights meet 16 activations = two 16-byte LDS reads; in row order they would sit 32 bytes apart from lane to lane
// and touch half of the banks each (by the bank arithmetic; not measured). The staged copy is therefore swizzled per 1024-element chunk: the first 8 activations of lane l's 16 sit at vector l of the
// chunk, the second 8 at vector 64 + l, so both reads are lane-contiguous. Rows are padded to whole chunks in LDS.
// The budget is the CU's whole LDS (the long-K down projection at 2..4 sequences: 76 / 114 / 152 KiB, one or two blocks per CU);
// when the padded copy exceeds it the waves read x through L2 (no fused norm then, as in gemv_kernel).
#include "common.hpp"
#include <stdlib.h>

using namespace spider;

namespace {

typedef float f32x2_t __attribute__((ext_vector_type(2)));

constexpr int W8_STAGE_CAP(int nwb) { return nwb == 8 ? 6 : 4; }

// dispatch defaults (measured: scripts/exp/fp8_decode_cost.py)
// Qwen2.5-7B shapes, us per launch with cold weights at 1 / 2 / 3 / 4 sequences:
//   gate/up (K = 3584), one -> two columns per wave:      23.8 -> 24.4 | 31.7 -> 28.6 | 40.8 -> 35.4 | 52.5 -> 43.3
//   down (K = 18944), activations through L2 -> in LDS:   (14.1: fits 64 KiB) | 21.1 -> 15.8 | 29.2 -> 17.5 | 32.4 -> 20.3
//   8 waves per block below K = 8192: slower everywhere (gate/up 23.8 -> 27.3 | 31.7 -> 39.7 | 40.8 -> 46.1 | 52.5 -> 55.7)
#define W8_LDS_BUDGET_BYTES (160 * 1024 - 256)   // staged activations per block: the whole LDS of a CU
#define W8_GU_R_MULTI 2                          // output columns per wave of the gate/up form from two sequences on

// 16-byte vector i of an activation row (elements 8 i .. 8 i + 7) -> its vector slot in the swizzled LDS row
__device__ __forceinline__ int w8_slot(int i) { return (i & ~127) | ((i & 1) << 6) | ((i & 127) >> 1); }

// 4 e4m3 bytes -> two packed bf16 pairs (bytes 0,1 | bytes 2,3), exact
__device__ __forceinline__ void fp8x4_to_bf16x4(uint32_t w, uint32_t& lo, uint32_t& hi) {
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    lo = pack_bf16x2(a[0], a[1]);
    hi = pack_bf16x2(b[0], b[1]);
}

template <int NB, int R, bool GATEUP, bool XLDS, int NWB>
__global__ __launch_bounds__(NWB * 64) void gemv_w8_kernel(const uint8_t* __restrict__ Wq, const float* __restrict__ scale,
                                                      const bf16_t* __restrict__ x, bf16_t* __restrict__ out,
                                                      const bf16_t* __restrict__ bias, const bf16_t* __restrict__ res,
                                                      const bf16_t* __restrict__ norm_w, float eps, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float red[NWB];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int NR = GATEUP ? 2 * R : R;     // weight rows per wave
    constexpr int U = (NR * NB <= 4) ? 4 : 2;  // chunks (of 1024 weights) in flight per row
    const int KP = (K + 1023) & ~1023;         // LDS row length in elements (whole chunks)

    const int col0 = (blockIdx.x * NWB + wave) * R;
    const uint8_t* wrow[NR];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int n = col0 + r;
        n = n < N ? n : N - 1;
        wrow[r] = Wq + (size_t)n * K;
        if (GATEUP) wrow[R + r] = Wq + (size_t)(N + n) * K;
    }
    auto load_set = [&](u32x4 (&wq)[U][NR], int base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = base + lane * 16 + u * 1024;
#pragma unroll
            for (int r = 0; r < NR; ++r)
                wq[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[r] + (unsigned)(k < K ? k : K - 16)));
        }
    };
    u32x4 w0[U][NR];

    // ---- activation prologue (the SCHED 2 staging of gemv_kernel with swizzled slots): branch-free, every load on a clamped
    // index; a vector past the end of the row counts as zero in the sum of squares and is stored to the clamped slot, where every
    // writer has the same value
    if constexpr (!XLDS) {
        load_set(w0, 0);
    } else {
        constexpr int NT = NWB * 64, CAP = W8_STAGE_CAP(NWB), CH = CAP / 2;
        const int nv = K / 8, nvp = KP / 8, t0 = threadIdx.x;
        const u32x4* wv = reinterpret_cast<const u32x4*>(norm_w);
        u32x4 st[CAP];
        auto issue_x = [&](const u32x4* xv, int i0) {
#pragma unroll
            for (int c = 0; c < CAP; ++c) st[c] = xv[min(i0 + c * NT, nv - 1)];
        };
        auto issue_xw = [&](const u32x4* xv, int i0) {
#pragma unroll
            for (int c = 0; c < CH; ++c) st[c] = xv[min(i0 + c * NT, nv - 1)];
#pragma unroll
            for (int c = 0; c < CH; ++c) st[CH + c] = wv[min(i0 + c * NT, nv - 1)];
        };
        auto store_x = [&](u32x4* sv, int i0) {
#pragma unroll
            for (int c = 0; c < CAP; ++c) sv[w8_slot(min(i0 + c * NT, nv - 1))] = st[c];
        };
        auto sumsq = [&](float ss, int i0, int n) {
#pragma unroll
            for (int c = 0; c < CAP; ++c) {
                if (c < n) {
                    const bool in = i0 + c * NT < nv;
                    uint32_t aw[4] = {in ? st[c].x : 0u, in ? st[c].y : 0u, in ? st[c].z : 0u, in ? st[c].w : 0u};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float lo = bf16lo_to_f32(aw[j]), hi = bf16hi_to_f32(aw[j]);
                        ss += lo * lo + hi * hi;
                    }
                }
            }
            return ss;
        };
        auto norm_store = [&](u32x4* sv, int i0, float rs) {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const u32x4 a = st[c], wq = st[CH + c];
                uint32_t aw[4] = {a.x, a.y, a.z, a.w}, ww[4] = {wq.x, wq.y, wq.z, wq.w}, o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float lo = bf16_to_f32(f32_to_bf16(bf16lo_to_f32(aw[j]) * rs)) * bf16lo_to_f32(ww[j]);
                    float hi = bf16_to_f32(f32_to_bf16(bf16hi_to_f32(aw[j]) * rs)) * bf16hi_to_f32(ww[j]);
                    o[j] = pack_bf16x2(lo, hi);
                }
                u32x4 ov;
                ov.x = o[0]; ov.y = o[1]; ov.z = o[2]; ov.w = o[3];
                sv[w8_slot(min(i0 + c * NT, nv - 1))] = ov;
            }
        };
        const u32x4* xv = reinterpret_cast<const u32x4*>(x);
        u32x4* sv = reinterpret_cast<u32x4*>(smem);
        if (!norm_w) {
            issue_x(xv, t0);
            load_set(w0, 0);
            store_x(sv, t0);
            asm volatile("" ::: "memory");   // keeps these stores out of the loop below (gemv_kernel has the reason)
            for (int b = 0; b < NB; ++b)
                for (int i0 = b ? 0 : CAP * NT; i0 < nv; i0 += CAP * NT) {
                    issue_x(xv + (size_t)b * nv, i0 + t0);
                    store_x(sv + (size_t)b * nvp, i0 + t0);
                }
        } else if (nv <= CH * NT) {
            issue_xw(xv, t0);
            load_set(w0, 0);
            for (int b = 0; b < NB; ++b) {
                if (b) issue_xw(xv + (size_t)b * nv, t0);
                const float rs = rsqrtf(block_sum<NWB, true>(sumsq(0.f, t0, CH), red) / (float)K + eps);
                norm_store(sv + (size_t)b * nvp, t0, rs);
            }
        } else {
            load_set(w0, 0);
            for (int b = 0; b < NB; ++b) {
                float ss = 0.f;
                for (int i0 = 0; i0 < nv; i0 += CAP * NT) {
                    issue_x(xv + (size_t)b * nv, i0 + t0);
                    ss = sumsq(ss, i0 + t0, CAP);
                }
                const float rs = rsqrtf(block_sum<NWB, true>(ss, red) / (float)K + eps);
                for (int i0 = 0; i0 < nv; i0 += CH * NT) {
                    issue_xw(xv + (size_t)b * nv, i0 + t0);
                    norm_store(sv + (size_t)b * nvp, i0 + t0, rs);
                }
            }
        }
        __syncthreads();
    }

    if (col0 >= N) return;      // wave-uniform
    float acc[NB][NR];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[b][r] = 0.f;

    const bf16_t* xs = reinterpret_cast<const bf16_t*>(smem);
    // one set of chunks against the activations; a lane's 16 weights are wholly inside the row or wholly past it (K % 16 == 0)
    auto fma_set = [&](const u32x4 (&wq)[U][NR], int base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kc = base + u * 1024, k = kc + lane * 16;
            if (k < K) {
                uint32_t wb[NR][8];
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const uint32_t ww[4] = {wq[u][r].x, wq[u][r].y, wq[u][r].z, wq[u][r].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) fp8x4_to_bf16x4(ww[j], wb[r][2 * j], wb[r][2 * j + 1]);
                }
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    u32x4 xa, xb;
                    if (XLDS) {
                        xa = *reinterpret_cast<const u32x4*>(xs + (size_t)b * KP + kc + lane * 8);
                        xb = *reinterpret_cast<const u32x4*>(xs + (size_t)b * KP + kc + 512 + lane * 8);
                    } else {
                        xa = *reinterpret_cast<const u32x4*>(x + (size_t)b * K + k);
                        xb = *reinterpret_cast<const u32x4*>(x + (size_t)b * K + k + 8);
                    }
                    const uint32_t xw[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
                    for (int r = 0; r < NR; ++r)
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[b][r] = dot2_bf16(wb[r][j], xw[j], acc[b][r]);
                }
            }
        }
    };
    fma_set(w0, 0);
    for (int base = 1024 * U; base < K; base += 1024 * U) {     // uniform trip count: the wave reconverges for the reduction
        u32x4 wq[U][NR];
        load_set(wq, base);
        fma_set(wq, base);
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
                const float s0 = scale[n], s1 = GATEUP ? scale[N + n] : 0.f;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    float v;
                    if (GATEUP) {
                        const float g = bf16_to_f32(f32_to_bf16(acc[b][r] * s0));
                        const float u = bf16_to_f32(f32_to_bf16(acc[b][R + r] * s1));
                        const float a = bf16_to_f32(f32_to_bf16(silu_f(g)));
                        v = a * u;
                    } else {
                        v = acc[b][r] * s0;
                        if (bias) v += bf16_to_f32(bias[n]);
                        if (res) v = bf16_to_f32(f32_to_bf16(v)) + bf16_to_f32(res[(size_t)b * N + n]);
                    }
                    out[(size_t)b * N + n] = f32_to_bf16(v);
                }
            }
        }
    }
}

// Largest staged activation copy per block. Up to 64 KiB (less the block's static LDS) a launch needs no opt-in; beyond it, up to the
// CU's 160 KiB, the kernel's dynamic-LDS limit is raised once per device (raise_dynamic_lds).
constexpr size_t W8_LDS_DEFAULT_LIMIT = 64 * 1024 - 256, W8_LDS_HW_LIMIT = 160 * 1024 - 256;
constexpr size_t W8_LDS_BUDGET = W8_LDS_BUDGET_BYTES;

int w8_env(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

template <int NB, int R, bool GU, bool XL, int NWB>
void gemv_w8_launch(const void* Wq, const float* scale, const void* x, void* out, const void* bias, const void* res,
                    const void* norm_w, float eps, int N, int K, size_t lds, void* stream) {
    auto* fn = gemv_w8_kernel<NB, R, GU, XL, NWB>;
    if (XL && lds > W8_LDS_DEFAULT_LIMIT) {
        static unsigned raised = 0;
        raise_dynamic_lds(fn, (int)W8_LDS_HW_LIMIT, raised);
    }
    fn<<<(N + NWB * R - 1) / (NWB * R), NWB * 64, XL ? lds : 0, (hipStream_t)stream>>>(
        (const uint8_t*)Wq, scale, (const bf16_t*)x, (bf16_t*)out, (const bf16_t*)bias, (const bf16_t*)res, (const bf16_t*)norm_w, eps, N, K);
}

template <int NB, bool GU>
int gemv_w8_dispatch(const void* Wq, const float* scale, const void* x, void* out, const void* bias, const void* res,
                     const void* norm_w, float eps, int N, int K, void* stream) {
    // tuning aids, read once: SPIDER_W8_LDS_MAX (bytes of staged activations per block), SPIDER_W8_NWB (4 / 8 waves per block),
    // SPIDER_W8_R / SPIDER_W8_GU_R (output columns per wave of the plain / gate-up form, 1 / 2)
    static const size_t lds_max = [] { const int v = w8_env("SPIDER_W8_LDS_MAX", 0); return v > 0 ? ((size_t)v < W8_LDS_HW_LIMIT ? (size_t)v : W8_LDS_HW_LIMIT) : W8_LDS_BUDGET; }();
    static const int env_nwb = w8_env("SPIDER_W8_NWB", 0), env_r = w8_env(GU ? "SPIDER_W8_GU_R" : "SPIDER_W8_R", 0);
    const size_t lds = (size_t)NB * ((K + 1023) / 1024) * 2048;      // rows padded to whole chunks
    const bool xlds = lds <= lds_max;
    SPIDER_CHECK(xlds || norm_w == nullptr, "gemv_w8: fused RMSNorm needs the activations in LDS (batch * ceil(K / 1024) * 2 KiB within the budget)");
    // Output columns per wave. A block stages batch * K * 2 bytes of activations for the NWB * R * K weight bytes per column set it
    // streams (half of what the same block of the bf16 kernel streams), so from two sequences on the staging is amortised over two
    // columns per wave; one column for single-sequence matrices below 24 Mi weights, where more blocks in flight hide the prologue
    // (gemv_dispatch's rule), and for the single-sequence gate/up form (two weight rows per column already).
    int R = GU ? (NB >= 2 ? W8_GU_R_MULTI : 1) : ((NB >= 2 || (size_t)N * K >= ((size_t)24 << 20)) ? 2 : 1);
    if (env_r == 1 || env_r == 2) R = env_r;
    // Waves per block: a function of K alone, so that the plain and the gate/up form of one shape reduce the RMSNorm sum of
    // squares in the same order. 8 waves share one staged copy of a long row (the down projection); for short rows 8 are slower.
    int nwb = K >= 8192 ? 8 : 4;
    if (env_nwb == 4 || env_nwb == 8) nwb = env_nwb;
#define W8_GO(R_, XL_, NWB_) gemv_w8_launch<NB, R_, GU, XL_, NWB_>(Wq, scale, x, out, bias, res, norm_w, eps, N, K, lds, stream)
#define W8_PICK(R_)                                                            \
    do {                                                                       \
        if (xlds) { if (nwb == 8) W8_GO(R_, true, 8); else W8_GO(R_, true, 4); } \
        else      { if (nwb == 8) W8_GO(R_, false, 8); else W8_GO(R_, false, 4); } \
    } while (0)
    if (R == 1) W8_PICK(1); else W8_PICK(2);
#undef W8_PICK
#undef W8_GO
    SPIDER_LAUNCH_OK();
    return 0;
}

template <bool GU>
int gemv_w8_batch(const void* Wq, const float* scale, const void* x, void* out, const void* bias, const void* res,
                  const void* norm_w, float eps, int B, int N, int K, void* stream) {
    switch (B) {
        case 1: return gemv_w8_dispatch<1, GU>(Wq, scale, x, out, bias, res, norm_w, eps, N, K, stream);
        case 2: return gemv_w8_dispatch<2, GU>(Wq, scale, x, out, bias, res, norm_w, eps, N, K, stream);
        case 3: return gemv_w8_dispatch<3, GU>(Wq, scale, x, out, bias, res, norm_w, eps, N, K, stream);
        case 4: return gemv_w8_dispatch<4, GU>(Wq, scale, x, out, bias, res, norm_w, eps, N, K, stream);
        default: spider_set_error("gemv_w8: batch must be 1..4 (more rows take the bf16 kernels on the dequantised weights)"); return -1;
    }
}

}  // namespace

extern "C" {

int spider_gemv_w8(const void* Wq, const float* scale, const void* x, void* out, const void* bias, const void* res,
                   const void* norm_w, float eps, int B, int N, int K, void* stream) {
    SPIDER_CHECK(N > 0 && K > 0 && K % 16 == 0, "gemv_w8: K must be a positive multiple of 16");
    return gemv_w8_batch<false>(Wq, scale, x, out, bias, res, norm_w, eps, B, N, K, stream);
}

int spider_gemv_swiglu_w8(const void* Wq_gate_up, const float* scale, const void* x, void* out, const void* norm_w, float eps,
                          int B, int I, int K, void* stream) {
    SPIDER_CHECK(I > 0 && K > 0 && K % 16 == 0, "gemv_swiglu_w8: K must be a positive multiple of 16");
    return gemv_w8_batch<true>(Wq_gate_up, scale, x, out, nullptr, nullptr, norm_w, eps, B, I, K, stream);
}

}  // extern "C"

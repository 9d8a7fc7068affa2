// Weight-only MXFP4 (OCP Microscaling: e2m1 nibbles, one E8M0 scale per block of 32) siblings of the row-major decode GEMVs of
// llm_decode.hip and of gemv_w8.hip, 1..4 sequences (gfx950 / CDNA4).
//
//   out[b, n] = epilogue( sum_k xin[b, k] * W_eff[n, k] ),   b < NB <= 4
//   blocks [N, K / 2] bytes, row-major: byte j of row n holds weight k = 2 j in its low nibble and k = 2 j + 1 in its high nibble;
//          nibble code c has sign bit 3 and magnitude [0, .5, 1, 1.5, 2, 3, 4, 6][c & 7];  K % 32 == 0
//   scales [N, K / 32] bytes, row-major, E8M0: W_eff[n, k] = e2m1(code) * 2^(scales[n, k / 32] - 127), bytes 1..254
//          (the layout of spider_amd/llm.py: quantize_mxfp4, which emits 2..252: every non-zero W_eff is a normal bf16 number)
//   xin    x, or RMSNorm(x) * norm_w with the normalised activation rounded to bf16 exactly as gemv_kernel / gemv_w8_kernel do
//   epilogue: (+bias) -> bf16 -> (+res -> bf16);  GATEUP: blocks / scales hold [gate rows | up rows] (2 N rows) and
//          out[b, n] = bf16(bf16(silu(bf16(g))) * bf16(u))
//
// What it keeps from gemv_w8_kernel: each wave owns R output columns and streams their rows with 16-byte nontemporal loads; the
// first U chunks of every row are requested BEFORE the activation prologue; loads are unconditional on clamped addresses and only
// the FMAs are predicated; activations are staged once per block in LDS, read through L2 when the padded copy does not fit.
// What differs: a lane's 16-byte load is 32 weights = exactly one MX block, so one scale byte belongs to one load and a wave
// instruction covers 2048 weights. The f32 scale operand is uint32(byte) << 23 (valid for bytes 1..254) and every weight byte
// becomes a packed bf16 pair with one v_cvt_scalef32_pk_bf16_fp4: the scale is applied inside the conversion, exactly (two
// significand bits times a power of two), because it differs from block to block and cannot leave the sum as FP8's per-row scale
// does. The pair meets the activations in v_dot2c_f32_bf16: 1/2 + NB / 2 VALU operations per weight.
// Scale loads: one byte load per lane per weight load from the public [N, K / 32] layout (the 64 lanes of a wave read 64
// contiguous bytes). A chunk-transposed private layout with one dword per lane for four chunks was not built or measured.
//
// A lane's 32 weights meet 32 activations = four 16-byte LDS reads, 64 bytes apart from lane to lane in row order. The staged
// copy is swizzled per 2048-element chunk: quarter p (8 activations) of lane l's 32 sits at vector 64 p + l of the chunk, so each of
// the four reads is lane-contiguous (64 lanes x 16 bytes = every bank four times, the minimum for a 16-byte read). Rows are padded
// to whole chunks in LDS: B * ceil(K / 2048) * 4 KiB within the CU's LDS, else the waves read x through L2 (no fused norm then).
#include "common.hpp"
#include <stdio.h>
#include <stdlib.h>

using namespace spider;

namespace {

constexpr int W4_STAGE_CAP(int nwb) { return nwb == 8 ? 6 : 4; }

#define W4_LDS_BUDGET_BYTES (160 * 1024 - 256)   // staged activations per block: the whole LDS of a CU
#define W4_GU_R_MULTI 2                          // output columns per wave of the gate/up form from two sequences on

// 16-byte vector i of an activation row (elements 8 i .. 8 i + 7) -> its vector slot in the swizzled LDS row
__device__ __forceinline__ int w4_slot(int i) { return (i & ~255) | ((i & 3) << 6) | ((i & 255) >> 2); }

// byte `SEL` of w (two e2m1 codes, low nibble first) times the block scale -> a packed bf16 pair, exact
template <int SEL>
__device__ __forceinline__ uint32_t fp4x2_to_bf16x2(uint32_t w, float sc) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, SEL));
}

template <int NB, int R, bool GATEUP, bool XLDS, int NWB>
__global__ __launch_bounds__(NWB * 64) void gemv_w4_kernel(const uint8_t* __restrict__ Wq, const uint8_t* __restrict__ scales,
                                                      const bf16_t* __restrict__ x, bf16_t* __restrict__ out,
                                                      const bf16_t* __restrict__ bias, const bf16_t* __restrict__ res,
                                                      const bf16_t* __restrict__ norm_w, float eps, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float red[NWB];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int NR = GATEUP ? 2 * R : R;     // weight rows per wave
    constexpr int U = (NR * NB <= 4) ? 4 : 2;  // chunks (of 2048 weights) in flight per row
    const int KP = (K + 2047) & ~2047;         // LDS row length in elements (whole chunks)

    const int col0 = (blockIdx.x * NWB + wave) * R;
    const uint8_t* wrow[NR];
    const uint8_t* srow[NR];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int n = col0 + r;
        n = n < N ? n : N - 1;
        wrow[r] = Wq + (size_t)n * (K / 2);
        srow[r] = scales + (size_t)n * (K / 32);
        if (GATEUP) {
            wrow[R + r] = Wq + (size_t)(N + n) * (K / 2);
            srow[R + r] = scales + (size_t)(N + n) * (K / 32);
        }
    }
    // lane l of chunk u: weights base + 2048 u + 32 l .. + 31 = 16 bytes of the row and scale byte (that k) / 32
    auto load_set = [&](u32x4 (&wq)[U][NR], uint32_t (&sc)[U][NR], int base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = base + lane * 32 + u * 2048;
            const unsigned kc = (unsigned)(k < K ? k : K - 32);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                wq[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow[r] + (kc >> 1)));
                sc[u][r] = srow[r][kc >> 5];
            }
        }
    };
    u32x4 w0[U][NR];
    uint32_t s0[U][NR];

    // ---- activation prologue (gemv_w8_kernel's, with this file's slots): branch-free, every load on a clamped index; a vector
    // past the end of the row counts as zero in the sum of squares and is stored to the clamped slot, where every writer has the
    // same value
    if constexpr (!XLDS) {
        load_set(w0, s0, 0);
    } else {
        constexpr int NT = NWB * 64, CAP = W4_STAGE_CAP(NWB), CH = CAP / 2;
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
            for (int c = 0; c < CAP; ++c) sv[w4_slot(min(i0 + c * NT, nv - 1))] = st[c];
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
                sv[w4_slot(min(i0 + c * NT, nv - 1))] = ov;
            }
        };
        const u32x4* xv = reinterpret_cast<const u32x4*>(x);
        u32x4* sv = reinterpret_cast<u32x4*>(smem);
        if (!norm_w) {
            issue_x(xv, t0);
            load_set(w0, s0, 0);
            store_x(sv, t0);
            asm volatile("" ::: "memory");   // keeps these stores out of the loop below (gemv_kernel has the reason)
            for (int b = 0; b < NB; ++b)
                for (int i0 = b ? 0 : CAP * NT; i0 < nv; i0 += CAP * NT) {
                    issue_x(xv + (size_t)b * nv, i0 + t0);
                    store_x(sv + (size_t)b * nvp, i0 + t0);
                }
        } else if (nv <= CH * NT) {
            issue_xw(xv, t0);
            load_set(w0, s0, 0);
            for (int b = 0; b < NB; ++b) {
                if (b) issue_xw(xv + (size_t)b * nv, t0);
                const float rs = rsqrtf(block_sum<NWB, true>(sumsq(0.f, t0, CH), red) / (float)K + eps);
                norm_store(sv + (size_t)b * nvp, t0, rs);
            }
        } else {
            load_set(w0, s0, 0);
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
    // one set of chunks against the activations; a lane's 32 weights are wholly inside the row or wholly past it (K % 32 == 0)
    auto fma_set = [&](const u32x4 (&wq)[U][NR], const uint32_t (&sc)[U][NR], int base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kc = base + u * 2048, k = kc + lane * 32;
            if (k < K) {
                uint32_t wb[NR][16];
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const float s = __builtin_bit_cast(float, sc[u][r] << 23);
                    const uint32_t ww[4] = {wq[u][r].x, wq[u][r].y, wq[u][r].z, wq[u][r].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        wb[r][4 * j + 0] = fp4x2_to_bf16x2<0>(ww[j], s);
                        wb[r][4 * j + 1] = fp4x2_to_bf16x2<1>(ww[j], s);
                        wb[r][4 * j + 2] = fp4x2_to_bf16x2<2>(ww[j], s);
                        wb[r][4 * j + 3] = fp4x2_to_bf16x2<3>(ww[j], s);
                    }
                }
#pragma unroll
                for (int b = 0; b < NB; ++b) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        u32x4 xa;
                        if (XLDS) xa = *reinterpret_cast<const u32x4*>(xs + (size_t)b * KP + kc + p * 512 + lane * 8);
                        else      xa = *reinterpret_cast<const u32x4*>(x + (size_t)b * K + k + p * 8);
                        const uint32_t xw[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
                        for (int r = 0; r < NR; ++r)
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[b][r] = dot2_bf16(wb[r][4 * p + j], xw[j], acc[b][r]);
                    }
                }
            }
        }
    };
    fma_set(w0, s0, 0);
    for (int base = 2048 * U; base < K; base += 2048 * U) {     // uniform trip count: the wave reconverges for the reduction
        u32x4 wq[U][NR];
        uint32_t sc[U][NR];
        load_set(wq, sc, base);
        fma_set(wq, sc, base);
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
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    float v;
                    if (GATEUP) {
                        const float g = bf16_to_f32(f32_to_bf16(acc[b][r]));
                        const float u = bf16_to_f32(f32_to_bf16(acc[b][R + r]));
                        const float a = bf16_to_f32(f32_to_bf16(silu_f(g)));
                        v = a * u;
                    } else {
                        v = acc[b][r];
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
constexpr size_t W4_LDS_DEFAULT_LIMIT = 64 * 1024 - 256, W4_LDS_HW_LIMIT = 160 * 1024 - 256;
constexpr size_t W4_LDS_BUDGET = W4_LDS_BUDGET_BYTES;

int w4_env(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

template <int NB, int R, bool GU, bool XL, int NWB>
void gemv_w4_launch(const void* Wq, const void* scales, const void* x, void* out, const void* bias, const void* res,
                    const void* norm_w, float eps, int N, int K, size_t lds, void* stream) {
    auto* fn = gemv_w4_kernel<NB, R, GU, XL, NWB>;
    if (XL && lds > W4_LDS_DEFAULT_LIMIT) {
        static unsigned raised = 0;
        raise_dynamic_lds(fn, (int)W4_LDS_HW_LIMIT, raised);
    }
    fn<<<(N + NWB * R - 1) / (NWB * R), NWB * 64, XL ? lds : 0, (hipStream_t)stream>>>(
        (const uint8_t*)Wq, (const uint8_t*)scales, (const bf16_t*)x, (bf16_t*)out, (const bf16_t*)bias, (const bf16_t*)res,
        (const bf16_t*)norm_w, eps, N, K);
}

template <int NB, bool GU>
int gemv_w4_dispatch(const void* Wq, const void* scales, const void* x, void* out, const void* bias, const void* res,
                     const void* norm_w, float eps, int N, int K, void* stream) {
    // tuning aids, read once: SPIDER_W4_LDS_MAX (bytes of staged activations per block; ops.w4_norm_fits mirrors it), SPIDER_W4_NWB
    // (4 / 8 waves per block), SPIDER_W4_R / SPIDER_W4_GU_R (output columns per wave of the plain / gate-up form, 1 / 2)
    static const size_t lds_max = [] { const int v = w4_env("SPIDER_W4_LDS_MAX", 0); return v > 0 ? ((size_t)v < W4_LDS_HW_LIMIT ? (size_t)v : W4_LDS_HW_LIMIT) : W4_LDS_BUDGET; }();
    static const int env_nwb = w4_env("SPIDER_W4_NWB", 0), env_r = w4_env(GU ? "SPIDER_W4_GU_R" : "SPIDER_W4_R", 0);
    const size_t lds = (size_t)NB * ((K + 2047) / 2048) * 4096;      // rows padded to whole chunks
    const bool xlds = lds <= lds_max;
    SPIDER_CHECK(xlds || norm_w == nullptr, "gemv_w4: fused RMSNorm needs the activations in LDS (batch * ceil(K / 2048) * 4 KiB within the budget)");
    // Output columns per wave and waves per block: gemv_w8_dispatch's rules. Measured against one / two columns everywhere and 4 / 8
    // waves everywhere (scripts/exp/mxfp4_decode_cost.py --ops-only, Qwen2.5-7B shapes, table in NOTEBOOK.md): nothing beats them
    // by more than 0.5 us per launch, one column from two sequences on and 8 waves below K = 8192 lose up to 20 us.
    // Waves per block are a function of K alone, so that the plain and the gate/up form of one shape reduce the RMSNorm sum of
    // squares in the same order.
    int R = GU ? (NB >= 2 ? W4_GU_R_MULTI : 1) : ((NB >= 2 || (size_t)N * K >= ((size_t)24 << 20)) ? 2 : 1);
    if (env_r == 1 || env_r == 2) R = env_r;
    int nwb = K >= 8192 ? 8 : 4;
    if (env_nwb == 4 || env_nwb == 8) nwb = env_nwb;
#define W4_GO(R_, XL_, NWB_) gemv_w4_launch<NB, R_, GU, XL_, NWB_>(Wq, scales, x, out, bias, res, norm_w, eps, N, K, lds, stream)
#define W4_PICK(R_)                                                            \
    do {                                                                       \
        if (xlds) { if (nwb == 8) W4_GO(R_, true, 8); else W4_GO(R_, true, 4); } \
        else      { if (nwb == 8) W4_GO(R_, false, 8); else W4_GO(R_, false, 4); } \
    } while (0)
    if (R == 1) W4_PICK(1); else W4_PICK(2);
#undef W4_PICK
#undef W4_GO
    SPIDER_LAUNCH_OK();
    return 0;
}

template <bool GU>
int gemv_w4_batch(const void* Wq, const void* scales, const void* x, void* out, const void* bias, const void* res,
                  const void* norm_w, float eps, int B, int N, int K, void* stream) {
    switch (B) {
        case 1: return gemv_w4_dispatch<1, GU>(Wq, scales, x, out, bias, res, norm_w, eps, N, K, stream);
        case 2: return gemv_w4_dispatch<2, GU>(Wq, scales, x, out, bias, res, norm_w, eps, N, K, stream);
        case 3: return gemv_w4_dispatch<3, GU>(Wq, scales, x, out, bias, res, norm_w, eps, N, K, stream);
        default: return gemv_w4_dispatch<4, GU>(Wq, scales, x, out, bias, res, norm_w, eps, N, K, stream);
    }
}

// everything a launch relies on, checked on the host before any launch
int w4_check(const char* who, const void* Wq, const void* scales, const void* x, const void* out, int B, int N, int K) {
    static thread_local char msg[160];
    const char* why = nullptr;
    if (N <= 0 || K <= 0 || K % 32 != 0) why = "K must be a positive multiple of 32 (one E8M0 scale per block of 32 weights)";
    else if (B < 1 || B > 4) why = "batch must be 1..4 (more rows take the bf16 kernels on the dequantised weights)";
    else if (!Wq || !scales || !x || !out) why = "blocks, scales, x and out must not be null";
    if (!why) return 0;
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    spider_set_error(msg);
    return -1;
}

}  // namespace

extern "C" {

int spider_gemv_w4(const void* blocks, const void* scales, const void* x, void* out, const void* bias, const void* res,
                   const void* norm_w, float eps, int B, int N, int K, void* stream) {
    if (w4_check("gemv_w4", blocks, scales, x, out, B, N, K)) return -1;
    return gemv_w4_batch<false>(blocks, scales, x, out, bias, res, norm_w, eps, B, N, K, stream);
}

int spider_gemv_swiglu_w4(const void* blocks_gate_up, const void* scales, const void* x, void* out, const void* norm_w, float eps,
                          int B, int I, int K, void* stream) {
    if (w4_check("gemv_swiglu_w4", blocks_gate_up, scales, x, out, B, I, K)) return -1;
    return gemv_w4_batch<true>(blocks_gate_up, scales, x, out, nullptr, nullptr, norm_w, eps, B, I, K, stream);
}

}  // extern "C"

// Shared device helpers for the spider_hip kernels (gfx950 / CDNA4 only).
// Wavefront = 64 lanes; all bf16 tensors are passed as raw uint16_t bit patterns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spider {

typedef uint16_t bf16_t;

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) short bf16x8;   // MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) short bf16x4;

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;  // 16-byte global/LDS access unit
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

__device__ __forceinline__ float bf16_to_f32(bf16_t v) {
    return __uint_as_float(((uint32_t)v) << 16);
}
__device__ __forceinline__ float bf16lo_to_f32(uint32_t packed) {
    return __uint_as_float(packed << 16);
}
__device__ __forceinline__ float bf16hi_to_f32(uint32_t packed) {
    return __uint_as_float(packed & 0xffff0000u);
}
// round-to-nearest-even f32 -> bf16 through the hardware converter (v_cvt_pk_bf16_f32 on gfx950; NaN stays NaN).
// A software rounding sequence costs ~7 VALU ops per element -- it dominated the flash-attention softmax.
typedef __bf16 hw_bf16x2 __attribute__((ext_vector_type(2)));
typedef float hw_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
    return __builtin_bit_cast(bf16_t, (__bf16)f);
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const hw_f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, hw_bf16x2));
}

// ---- 16-bit storage / operand type of the diffusion-side translation units (gemm, attention, UNet ops, fused cross-attention) ----
// Those files are compiled twice: as bf16 (LLM prefill, towers, CLIP at the BASELINE dtype) and, with -DSPIDER_F16, as IEEE
// half -- the reference's own diffusion dtype (torch_dtype=torch.float16, spider_decoder.py:109,114; base_model.py:211;
// Comic_Generation.py:313). gfx950 runs mfma_f32_*_f16 at the bf16 rate; three more significand bits bring one UNet
// evaluation from 1.5e-2 to 1.6e-3 of the fp32 oracle. The h16_* helpers below are the only place
// the two instantiations differ; entry points are named through SPIDER_FN: spider_gemm -> spider_gemm_bf16 / spider_gemm_f16.
typedef uint16_t h16_t;
typedef bf16x8 h16x8;
typedef bf16x4 h16x4;
#define SPIDER_CAT2_(a, b) a##_##b
#define SPIDER_CAT2(a, b) SPIDER_CAT2_(a, b)
#ifdef SPIDER_F16
#define SPIDER_DT f16
#define SPIDER_DT_NAME "f16"
typedef _Float16 hw_f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 hw_f16x8 __attribute__((ext_vector_type(8)));
constexpr uint32_t H16_ONE = 0x3C00u;   // 1.0
__device__ __forceinline__ float h16_to_f32(h16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
__device__ __forceinline__ float h16lo_to_f32(uint32_t packed) { return (float)__builtin_bit_cast(hw_f16x2, packed)[0]; }
__device__ __forceinline__ float h16hi_to_f32(uint32_t packed) { return (float)__builtin_bit_cast(hw_f16x2, packed)[1]; }
// round-to-nearest-even (v_cvt_f16_f32 / v_cvt_pk_f16_f32); values beyond 65504 become +-inf as in torch.float16
__device__ __forceinline__ h16_t f32_to_h16(float f) { return __builtin_bit_cast(h16_t, (_Float16)f); }
__device__ __forceinline__ uint32_t pack_h16x2(float lo, float hi) {
    const hw_f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, hw_f16x2));
}
__device__ __forceinline__ float dot2_h16(uint32_t a, uint32_t b, float acc) {
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(hw_f16x2, a), __builtin_bit_cast(hw_f16x2, b), acc, false);
}
__device__ __forceinline__ f32x4 mfma_16x16x32_h16(h16x8 a, h16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(hw_f16x8, a), __builtin_bit_cast(hw_f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_32x32x16_h16(h16x8 a, h16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(hw_f16x8, a), __builtin_bit_cast(hw_f16x8, b), c, 0, 0, 0);
}
typedef _Float16 hw_f16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma_16x16x16_h16(h16x4 a, h16x4 b, f32x4 c) {     // K = 16: 4 values per lane
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(hw_f16x4, a), __builtin_bit_cast(hw_f16x4, b), c, 0, 0, 0);
}
#else
#define SPIDER_DT bf16
#define SPIDER_DT_NAME "bf16"
constexpr uint32_t H16_ONE = 0x3F80u;   // 1.0
__device__ __forceinline__ float h16_to_f32(h16_t v) { return bf16_to_f32(v); }
__device__ __forceinline__ float h16lo_to_f32(uint32_t packed) { return bf16lo_to_f32(packed); }
__device__ __forceinline__ float h16hi_to_f32(uint32_t packed) { return bf16hi_to_f32(packed); }
__device__ __forceinline__ h16_t f32_to_h16(float f) { return f32_to_bf16(f); }
__device__ __forceinline__ uint32_t pack_h16x2(float lo, float hi) { return pack_bf16x2(lo, hi); }
__device__ __forceinline__ float dot2_h16(uint32_t a, uint32_t b, float acc) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(hw_bf16x2, a), __builtin_bit_cast(hw_bf16x2, b), acc, false);
}
__device__ __forceinline__ f32x4 mfma_16x16x32_h16(h16x8 a, h16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_32x32x16_h16(h16x8 a, h16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_16x16x16_h16(h16x4 a, h16x4 b, f32x4 c) {     // K = 16: 4 values per lane
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
#endif
#define SPIDER_FN(name) SPIDER_CAT2(name, SPIDER_DT)

// acc += a.lo*b.lo + a.hi*b.hi on packed bf16 pairs (v_dot2c_f32_bf16): no unpacking, 1 VALU op per 2 MACs
__device__ __forceinline__ float dot2_bf16(uint32_t a, uint32_t b, float acc) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(hw_bf16x2, a), __builtin_bit_cast(hw_bf16x2, b), acc, false);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- cross-lane exchanges on the VALU ----
// __shfl_xor compiles to ds_bpermute_b32: a round trip through the LDS pipe (address VGPR, lgkmcnt wait) on the critical path of
// every butterfly step. The forms below fetch the same partner with DPP modifiers / v_permlane*_swap and touch no LDS-pipe
// instruction. Blocks must be one-dimensional with a multiple of 64 threads (the 16 / 32 forms read the lane from threadIdx.x).
// DPP source lanes must be active: call under full exec, or under an exec mask that is uniform per 16-lane row.
//
// Partner read by lane l (row = 16 lanes, i = l & 15; checked on the host by applying the permutations to 0..63):
//   M   instruction(s)                                   source lane                         == l ^ M
//   1   DPP quad_perm:[1,0,3,2]                          (l & ~3) | {1,0,3,2}[l & 3]          yes
//   2   DPP quad_perm:[2,3,0,1]                          (l & ~3) | {2,3,0,1}[l & 3]          yes
//   4   DPP row_half_mirror, then quad_perm:[3,2,1,0]    (l ^ 7) ^ 3: two reflections         yes (7 ^ 3 = 4)
//   8   DPP row_ror:8                                    (l & ~15) | ((i + 8) & 15)           yes (either direction)
//   16  v_permlane16_swap(v, v): rows 0..3 of r0 hold rows 0,0,2,2 of v, those of r1 rows 1,1,3,3
//       partner = (l & 16) ? r0 : r1                                                          yes
//   32  v_permlane32_swap(v, v): r0 = halves 0,0 of v, r1 = halves 1,1;  partner = (l & 32) ? r0 : r1   yes
// For 16 / 32, {r0, r1} is {own, partner} in some order in EVERY lane, so a commutative combine is r0 (op) r1 with no select.
template <int M>
__device__ __forceinline__ uint32_t lane_xor(uint32_t u) {
    static_assert(M == 1 || M == 2 || M == 4 || M == 8 || M == 16 || M == 32, "lane_xor: M must be a power of two below 64");
    if constexpr (M == 1) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0xB1, 0xf, 0xf, true);    // quad_perm:[1,0,3,2]
    } else if constexpr (M == 2) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x4E, 0xf, 0xf, true);    // quad_perm:[2,3,0,1]
    } else if constexpr (M == 4) {
        const int t = __builtin_amdgcn_update_dpp(0, (int)u, 0x141, 0xf, 0xf, true);      // row_half_mirror: i -> i ^ 7
        return (uint32_t)__builtin_amdgcn_update_dpp(0, t, 0x1B, 0xf, 0xf, true);         // quad_perm:[3,2,1,0]: i -> i ^ 3
    } else if constexpr (M == 8) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)u, 0x128, 0xf, 0xf, true);   // row_ror:8
    } else if constexpr (M == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        return (threadIdx.x & 16) ? r[0] : r[1];
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        return (threadIdx.x & 32) ? r[0] : r[1];
    }
}
template <int M>
__device__ __forceinline__ float lane_xor(float v) { return __uint_as_float(lane_xor<M>(__float_as_uint(v))); }
template <int M>
__device__ __forceinline__ int lane_xor(int v) { return (int)lane_xor<M>((uint32_t)v); }
// M = 16 / 32 where only the lanes with (lane & M) == 0 need the partner (the last rounds of a reduction towards lane 0): the
// second result of the swap as it is, no select; the other lanes get their own value back.
template <int M>
__device__ __forceinline__ float lane_xor_lo(float v) {
    static_assert(M == 16 || M == 32, "lane_xor_lo: M must be 16 or 32");
    const uint32_t u = __float_as_uint(v);
    if constexpr (M == 16) return __uint_as_float(__builtin_amdgcn_permlane16_swap(u, u, false, false)[1]);
    else return __uint_as_float(__builtin_amdgcn_permlane32_swap(u, u, false, false)[1]);
}
// v + partner / max(v, partner): the same two operands as `v + __shfl_xor(v, M)`, and IEEE add / max are commutative, so the
// result is bit-identical to the shuffle form in every lane
template <int M>
__device__ __forceinline__ float xor_add(float v) {
    if constexpr (M == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    } else if constexpr (M == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    } else {
        return v + lane_xor<M>(v);
    }
}
template <int M>
__device__ __forceinline__ float xor_max(float v) {
    if constexpr (M == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    } else if constexpr (M == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    } else {
        return fmaxf(v, lane_xor<M>(v));
    }
}
// 64-lane sum / max in the order of wave_sum / wave_max (xor 32, 16, 8, 4, 2, 1): bit-identical to them. Full exec only.
__device__ __forceinline__ float wave_sum_valu(float v) {
    return xor_add<1>(xor_add<2>(xor_add<4>(xor_add<8>(xor_add<16>(xor_add<32>(v))))));
}
__device__ __forceinline__ float wave_max_valu(float v) {
    return xor_max<1>(xor_max<2>(xor_max<4>(xor_max<8>(xor_max<16>(xor_max<32>(v))))));
}
// sum over the 16 lanes of a row in the order xor 1, 2, 4, 8 (the decode attention's score reduction)
__device__ __forceinline__ float row16_sum_valu(float v) { return xor_add<8>(xor_add<4>(xor_add<2>(xor_add<1>(v)))); }

// Block-wide sum for blocks of NW waves; `red` is >= NW floats of LDS. All threads get the result.
// VALU: the wave sums through wave_sum_valu (same order, same bits) instead of six ds_bpermute round trips.
template <int NW, bool VALU = false>
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = VALU ? wave_sum_valu(v) : wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NW; ++i) t += red[i];
    return t;
}

// x * rcp(...) instead of x / (...): an IEEE fp32 division is a ~10-instruction sequence, v_rcp_f32 is 1 ulp
__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
// exact-erf GELU (torch F.gelu default, diffusers GEGLU / CLIP-H / CLAP). erf through Abramowitz-Stegun 7.1.26
// (|error| <= 1.5e-7, two orders below bf16 resolution): branch-free, 2 transcendentals + 7 FMAs, where libdevice's
// erff is a ~50-instruction divergent polynomial -- it was ~25 % of the fused GEGLU GEMM's time.
__device__ __forceinline__ float erf_fast(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = 1.f - p * t * __expf(-ax * ax);
    return copysignf(e, x);
}
__device__ __forceinline__ float gelu_erf_f(float x) { return 0.5f * x * (1.f + erf_fast(x * 0.70710678118654752f)); }
__device__ __forceinline__ float quick_gelu_f(float x) { return x * __builtin_amdgcn_rcpf(1.f + __expf(-1.702f * x)); }

// XCD-aware bijective remap of a linear block id: blocks that share an XCD (id % 8) get a
// contiguous chunk of the logical grid, so neighbouring tiles hit the same L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + idx;
}

}  // namespace spider

// Dynamic LDS above 64 KiB must be enabled per function AND per device (one process may drive engines on several GPUs): raise it
// once for each device the function is launched on. `done_mask` is the caller's static bit mask (bit = device ordinal mod 32).
template <typename F>
inline void raise_dynamic_lds(F* fn, int bytes, unsigned& done_mask) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned bit = 1u << (dev & 31);
    if (!(done_mask & bit)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        done_mask |= bit;
    }
}

// ---- error plumbing shared by the C-ABI translation units ----
extern "C" void spider_set_error(const char* msg);
extern "C" int g_spider_ws_inlaunch;      // capi.cpp: split-K combine form of the streaming conv (spider_set_ws_inlaunch)
#define SPIDER_CHECK(cond, msg)            \
    do {                                   \
        if (!(cond)) {                     \
            spider_set_error(msg);         \
            return -1;                     \
        }                                  \
    } while (0)
#define SPIDER_LAUNCH_OK()                                        \
    do {                                                          \
        hipError_t e__ = hipGetLastError();                       \
        if (e__ != hipSuccess) {                                  \
            spider_set_error(hipGetErrorString(e__));             \
            return -2;                                            \
        }                                                         \
    } while (0)

// What the decode weight streams share (llm_decode.hip: gemv_kernel, lmhead_partial_kernel; gemv_wq.hip, lm_head_wq.hip,
// gemv_qfm.hip): staging the <= 8 activation rows of a block in LDS with the optional fused RMSNorm, the LDS swizzle and the weight
// decode of the two quantised formats, and the host-side budget / env / error helpers of the quantised translation units.
// FMT names a format everywhere: 8 = FP8 (OCP e4m3fn bytes, one fp32 scale per row), 4 = MXFP4 (e2m1 nibbles, one E8M0 byte per 32).
#pragma once
#include "common.hpp"
#include <stdio.h>
#include <stdlib.h>

namespace spider {

// ---- one 16-byte vector (8 bf16) of an activation row ----
// ss + its sum of squares, pair by pair: every kernel that normalises adds in this order
__device__ __forceinline__ float sumsq_vec(float ss, const u32x4 a) {
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float lo = bf16lo_to_f32(aw[j]), hi = bf16hi_to_f32(aw[j]);
        ss += lo * lo + hi * hi;
    }
    return ss;
}
// the two-rounding RMSNorm: bf16(bf16(x * rs) * norm_w)
__device__ __forceinline__ u32x4 norm_vec(const u32x4 a, const u32x4 wq, float rs) {
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, ww[4] = {wq.x, wq.y, wq.z, wq.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float lo = bf16_to_f32(f32_to_bf16(bf16lo_to_f32(aw[j]) * rs)) * bf16lo_to_f32(ww[j]);
        float hi = bf16_to_f32(f32_to_bf16(bf16hi_to_f32(aw[j]) * rs)) * bf16hi_to_f32(ww[j]);
        o[j] = pack_bf16x2(lo, hi);
    }
    u32x4 ov;
    ov.x = o[0]; ov.y = o[1]; ov.z = o[2]; ov.w = o[3];
    return ov;
}

// ---- simple staging: one memory request at a time (gemv_kernel SCHED 0, lmhead_partial_kernel, lmq_partial_kernel) ----
// NB rows of x [NB, K] -> sv[b * ld + slot(i)], i = 16-byte vector of the row; ld = row stride of the LDS copy in vectors. With
// norm_w the row is read twice: a strided sum of squares reduced by block_sum<NWB> (wave_sum's ds_bpermute order), then the
// normalise pass. `red` = NWB floats of LDS. Ends with the block's barrier.
template <int NB, int NWB, class Slot>
__device__ __forceinline__ void stage_rows_simple(const bf16_t* x, const bf16_t* norm_w, float eps, int K, int ld, u32x4* sv,
                                                  float* red, Slot slot) {
    const int nv = K / 8;
    for (int b = 0; b < NB; ++b) {
        const u32x4* xv = reinterpret_cast<const u32x4*>(x + (size_t)b * K);
        u32x4* svb = sv + (size_t)b * ld;
        if (norm_w) {
            float ss = 0.f;
            for (int i = threadIdx.x; i < nv; i += NWB * 64) ss = sumsq_vec(ss, xv[i]);
            const float rs = rsqrtf(block_sum<NWB>(ss, red) / (float)K + eps);
            const u32x4* wv = reinterpret_cast<const u32x4*>(norm_w);
            for (int i = threadIdx.x; i < nv; i += NWB * 64) svb[slot(i)] = norm_vec(xv[i], wv[i], rs);
        } else {
            for (int i = threadIdx.x; i < nv; i += NWB * 64) svb[slot(i)] = xv[i];
        }
    }
    __syncthreads();
}

// ---- branch-free staging: one trip for the prologue (gemv_kernel SCHED 1 / 2, gemv_wq_kernel) ----
// 16-byte vectors a thread keeps in flight while it stages the activations: one batch covers K <= 8192 (plain) or 4096
// (normalised: half of them are norm_w) with 4 waves per block, K <= 24576 with 8 (the down projection asks for 5)
constexpr int stage_cap(int nwb) { return nwb == 8 ? 6 : 4; }

// Same rows, same slots and strides as stage_rows_simple, same arithmetic (the block sum goes through wave_sum_valu: wave_sum's
// order, the same bits). hoist_w() requests the wave's first weight chunks. Every load goes to a clamped index, a vector past the
// end of the row counts as zero in the sum of squares (adding +0 is exact) and is stored, normalised or not, to the clamped slot,
// where every writer has the same value: a load under a per-lane branch would make the compiler drain the queue.
// Three straight-line forms, each with the first batch of row 0 requested BEFORE the weights: vmcnt retires in order, so the wait
// for that batch leaves the weight loads in flight (any later batch or row waits for them too). x stays in registers from the sum
// of squares to the normalise pass when the row fits them; longer rows go on in batches of stage_cap.
template <int NB, int NWB, class Slot, class Hoist>
__device__ __forceinline__ void stage_rows_branchfree(const bf16_t* x, const bf16_t* norm_w, float eps, int K, int ld, u32x4* sv,
                                                      float* red, Slot slot, Hoist hoist_w) {
    constexpr int NT = NWB * 64, CAP = stage_cap(NWB), CH = CAP / 2;
    const int nv = K / 8, t0 = threadIdx.x;
    const u32x4* wv = reinterpret_cast<const u32x4*>(norm_w);
    u32x4 st[CAP];
    auto issue_x = [&](const u32x4* xv, int i0) {     // plain form: CAP vectors of x
#pragma unroll
        for (int c = 0; c < CAP; ++c) st[c] = xv[min(i0 + c * NT, nv - 1)];
    };
    auto issue_xw = [&](const u32x4* xv, int i0) {    // normalised form: CH vectors of x, then the same CH of norm_w
#pragma unroll
        for (int c = 0; c < CH; ++c) st[c] = xv[min(i0 + c * NT, nv - 1)];
#pragma unroll
        for (int c = 0; c < CH; ++c) st[CH + c] = wv[min(i0 + c * NT, nv - 1)];
    };
    auto store_x = [&](u32x4* svb, int i0) {
#pragma unroll
        for (int c = 0; c < CAP; ++c) svb[slot(min(i0 + c * NT, nv - 1))] = st[c];
    };
    auto sumsq = [&](float ss, int i0, int n) {
#pragma unroll
        for (int c = 0; c < CAP; ++c) {
            if (c < n) {
                const bool in = i0 + c * NT < nv;
                u32x4 a;
                a.x = in ? st[c].x : 0u; a.y = in ? st[c].y : 0u; a.z = in ? st[c].z : 0u; a.w = in ? st[c].w : 0u;
                ss = sumsq_vec(ss, a);
            }
        }
        return ss;
    };
    auto norm_store = [&](u32x4* svb, int i0, float rs) {
#pragma unroll
        for (int c = 0; c < CH; ++c) svb[slot(min(i0 + c * NT, nv - 1))] = norm_vec(st[c], st[CH + c], rs);
    };
    const u32x4* xv = reinterpret_cast<const u32x4*>(x);
    if (!norm_w) {
        issue_x(xv, t0);
        hoist_w();
        store_x(sv, t0);
        // keeps these stores out of the loop below: merged with its stores they would sit behind the loop's wait for ALL loads
        asm volatile("" ::: "memory");
        for (int b = 0; b < NB; ++b)
            for (int i0 = b ? 0 : CAP * NT; i0 < nv; i0 += CAP * NT) {
                issue_x(xv + (size_t)b * nv, i0 + t0);
                store_x(sv + (size_t)b * ld, i0 + t0);
            }
    } else if (nv <= CH * NT) {
        // the row fits the registers: x is read once and norm_w is requested with it
        issue_xw(xv, t0);
        hoist_w();
        for (int b = 0; b < NB; ++b) {
            if (b) issue_xw(xv + (size_t)b * nv, t0);
            const float rs = rsqrtf(block_sum<NWB, true>(sumsq(0.f, t0, CH), red) / (float)K + eps);
            norm_store(sv + (size_t)b * ld, t0, rs);
        }
    } else {
        hoist_w();
        for (int b = 0; b < NB; ++b) {
            float ss = 0.f;
            for (int i0 = 0; i0 < nv; i0 += CAP * NT) {
                issue_x(xv + (size_t)b * nv, i0 + t0);
                ss = sumsq(ss, i0 + t0, CAP);
            }
            const float rs = rsqrtf(block_sum<NWB, true>(ss, red) / (float)K + eps);
            for (int i0 = 0; i0 < nv; i0 += CH * NT) {
                issue_xw(xv + (size_t)b * nv, i0 + t0);
                norm_store(sv + (size_t)b * ld, i0 + t0, rs);
            }
        }
    }
    __syncthreads();
}

// ---- the quantised formats ----
template <int FMT> constexpr int WQ_LW = FMT == 8 ? 16 : 32;     // weights per lane per 16-byte load
template <int FMT> constexpr int WQ_CHUNK = 64 * WQ_LW<FMT>;     // weights per wave instruction: 1024 / 2048

// A lane's LW weights meet LW activations = LW / 8 16-byte LDS reads, 2 LW bytes apart from lane to lane in row order. The staged
// copy is therefore swizzled per chunk, rows padded to whole chunks: piece p (8 activations) of lane l's LW sits at vector
// 64 p + l of the chunk, so every read is lane-contiguous. wq_slot: vector i of a row -> its vector slot in the swizzled row.
template <int FMT>
constexpr int wq_slot(int i) {
    constexpr int NP = WQ_LW<FMT> / 8, CV = 64 * NP;
    return (i & ~(CV - 1)) | ((i & (NP - 1)) << 6) | ((i & (CV - 1)) / NP);
}
template <int FMT>
constexpr bool wq_slot_is_bijection() {
    constexpr int CV = WQ_CHUNK<FMT> / 8;
    bool hit[2 * CV] = {};
    for (int i = 0; i < 2 * CV; ++i) {
        const int s = wq_slot<FMT>(i);
        if (s / CV != i / CV || hit[s]) return false;     // stays in its chunk, no slot taken twice
        hit[s] = true;
    }
    return true;
}
static_assert(wq_slot_is_bijection<8>() && wq_slot_is_bijection<4>(), "wq_slot must permute the 128 / 256 vectors of a chunk");

typedef float f32x2_t __attribute__((ext_vector_type(2)));

// 4 e4m3 bytes -> two packed bf16 pairs (bytes 0,1 | bytes 2,3): v_cvt_pk_f32_fp8 + v_cvt_pk_bf16_f32, exact (3 significand bits)
__device__ __forceinline__ void fp8x4_to_bf16x4(uint32_t w, uint32_t& lo, uint32_t& hi) {
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    lo = pack_bf16x2(a[0], a[1]);
    hi = pack_bf16x2(b[0], b[1]);
}
// the low (HI = false) or high two e4m3 bytes of w -> a packed bf16 pair in one v_cvt_scalef32_pk_bf16_fp8 with the scale 1.0
template <bool HI>
__device__ __forceinline__ uint32_t fp8x2_to_bf16x2(uint32_t w) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
}
// byte `SEL` of w (two e2m1 codes, low nibble first) times the block scale -> a packed bf16 pair, exact
template <int SEL>
__device__ __forceinline__ uint32_t fp4x2_to_bf16x2(uint32_t w, float sc) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, SEL));
}
// E8M0 byte 1..254 -> the conversion's f32 scale operand 2^(byte - 127)
__device__ __forceinline__ float e8m0_to_f32(uint32_t byte) { return __builtin_bit_cast(float, byte << 23); }

// piece p (8 weights) of a lane's 16-byte load ww -> four packed bf16 pairs: two weight words of FP8, one of MXFP4 (e8m0 = the
// load's scale byte; FP8's row scale stays outside the sum)
template <int FMT>
__device__ __forceinline__ void wq_decode_piece(const uint32_t (&ww)[4], int p, uint32_t e8m0, uint32_t (&wb)[4]) {
    if constexpr (FMT == 8) {
        fp8x4_to_bf16x4(ww[2 * p], wb[0], wb[1]);
        fp8x4_to_bf16x4(ww[2 * p + 1], wb[2], wb[3]);
    } else {
        const float s = e8m0_to_f32(e8m0);
        wb[0] = fp4x2_to_bf16x2<0>(ww[p], s);
        wb[1] = fp4x2_to_bf16x2<1>(ww[p], s);
        wb[2] = fp4x2_to_bf16x2<2>(ww[p], s);
        wb[3] = fp4x2_to_bf16x2<3>(ww[p], s);
    }
}

// One block per sequence reduces the [nparts] (value, index) partials of the lm_head kernels, ties -> lowest id. Internal linkage:
// each translation unit that launches it gets its own copy and no symbol is exported.
static __global__ __launch_bounds__(256) void argmax_final_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                                  int* __restrict__ out, int nparts) {
    __shared__ float sv[256];
    __shared__ int si[256];
    const int b = blockIdx.x;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < nparts; i += 256) {
        const float v = pval[(size_t)b * nparts + i];
        const int ix = pidx[(size_t)b * nparts + i];
        if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const float v = sv[threadIdx.x + s];
            const int ix = si[threadIdx.x + s];
            if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && ix < si[threadIdx.x])) {
                sv[threadIdx.x] = v;
                si[threadIdx.x] = ix;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[b] = si[0];
}

}  // namespace spider

// ---- host side of the quantised translation units ----
// Largest staged activation copy per block. Up to 64 KiB (less the block's static LDS) a launch needs no opt-in; beyond it, up to
// the CU's 160 KiB, the kernel's dynamic-LDS limit is raised once per device (raise_dynamic_lds). The default budget is the whole
// LDS of a CU. spider_amd/ops.py mirrors these figures (W8_LDS_MAX / W4_LDS_MAX).
constexpr size_t WQ_LDS_DEFAULT_LIMIT = 64 * 1024 - 256, WQ_LDS_HW_LIMIT = 160 * 1024 - 256;

inline int wq_env(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// bytes of LDS for B staged rows of K activations, padded to whole chunks: B * ceil(K / 1024) * 2 KiB, B * ceil(K / 2048) * 4 KiB
template <int FMT>
inline size_t wq_lds_bytes(int B, int K) {
    constexpr int CHUNK = spider::WQ_CHUNK<FMT>;
    return (size_t)B * ((K + CHUNK - 1) / CHUNK) * CHUNK * 2;
}
// the budget wq_lds_bytes is held against: SPIDER_W8_LDS_MAX / SPIDER_W4_LDS_MAX (bytes, read once), else the whole LDS
template <int FMT>
inline size_t wq_lds_max() {
    static const size_t v = [] {
        const int e = wq_env(FMT == 8 ? "SPIDER_W8_LDS_MAX" : "SPIDER_W4_LDS_MAX", 0);
        return e > 0 ? ((size_t)e < WQ_LDS_HW_LIMIT ? (size_t)e : WQ_LDS_HW_LIMIT) : WQ_LDS_HW_LIMIT;
    }();
    return v;
}
template <int FMT>
constexpr const char* WQ_K_RULE = FMT == 8 ? "K must be a positive multiple of 16 (16 e4m3 weights per 16-byte load)"
                                           : "K must be a positive multiple of 32 (one E8M0 scale per block of 32 weights)";
template <int FMT>
constexpr const char* WQ_NORM_RULE =
    FMT == 8 ? "fused RMSNorm needs the activations in LDS (batch * ceil(K / 1024) * 2 KiB within the budget)"
             : "fused RMSNorm needs the activations in LDS (batch * ceil(K / 2048) * 4 KiB within the budget)";

// "<who>: <why>" as the thread's last error; returns -1
inline int wq_fail(const char* who, const char* why) {
    static thread_local char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    spider_set_error(msg);
    return -1;
}

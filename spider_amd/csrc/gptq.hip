// Calibrated MXFP4 (GPTQ on MX blocks; `llm.quantize_mxfp4_gptq` is the definition): the sequential quantise-and-compensate sweep
// over K for one GROUP of C <= 4 consecutive MX blocks (32 C columns), all N rows. One launch:
//   every lane owns ONE row n; the group's diagonal block of U (upper Cholesky factor of H^-1, fp32, [32 C, 32 C], at most
//   64 KiB) sits in LDS and is read as wave-uniform broadcasts;
//   per block b of the group, in order: the row's 32 working weights come into registers; what the earlier blocks of the group
//   owe them is applied pivot by pivot in column order, w_i -= e_p U[p, 32 b + i] (a runtime loop over the pivots with the 32
//   FMAs unrolled; e_p is this lane's own entry of Et, written a block earlier); then amax of the CURRENT weights -> E8M0 exponent
//   by quantize_mxfp4's rule (frexp form on the bits: m > 0.75 <=> fraction > 0x400000; clamp [-125, 125]; byte 127 for an
//   all-zero block), and for i = 0 .. 31 in order
//     a = |w_i| * 2^-e (exact), code = midpoints passed (ties to the even significand; a > 6 saturates at 7), sign bit of w_i,
//     q = +-value * 2^e,  e_i = (w_i - q) / U[i, i]  (IEEE division),  w_i' -= e_i U[i, i'] for the later columns i' of the block.
//   So the compensation crosses the block boundaries inside the group, every weight takes its updates in the definition's order,
//   and the columns behind the group get E U[group, behind] from the caller's fp32 GEMM between launches.
// Only the current block lives in registers: with all 32 C weights of the group resident and every loop unrolled (8128 FMAs at
// C = 4) the compiler delays the updates, keeps thousands of U values live and spills 15 KB per lane; the pivot loop keeps the
// code small and the registers at one block.
// Written: 16 bytes of nibbles per row and block (one store), the scale byte, and E transposed, Et [32 C, N] fp32.
// Memory: the working copy is K-major, Wt [K, N] fp32, so column j of all rows is contiguous: the loads of Wt and the accesses
// of Et are coalesced over the lanes of a wave (256 bytes per wave and column). The nibble stores are 16 bytes per lane at a row
// stride of K / 2 bytes, the layout the decode kernels read. All arithmetic is fp32; plain vector stores, no atomics.
#include "common.hpp"

using namespace spider;

namespace {

constexpr int GQ_THREADS = 64;          // rows per workgroup: one wave, so that N rows spread over N / 64 compute units
constexpr int GQ_MAX_BLOCKS = 4;        // MX blocks per launch: 128 x 128 fp32 of U = 64 KiB of LDS

template <int C>
__global__ __launch_bounds__(GQ_THREADS) void gptq_mxfp4_sweep_kernel(const float* __restrict__ Wt, const float* __restrict__ U,
                                                                      uint8_t* __restrict__ blocks, uint8_t* __restrict__ scales,
                                                                      float* Et, int N, int K, int j0) {
    constexpr int W = 32 * C;
    __shared__ __attribute__((aligned(16))) float Us[W * W];
    const int tid = threadIdx.x;
    // rows j0 .. j0 + W - 1 of U, columns j0 .. j0 + W - 1: W contiguous floats per row, 16-byte pieces (j0 % 32 == 0, K % 32 == 0)
    for (int idx = tid; idx < W * W / 4; idx += GQ_THREADS) {
        const int i = idx / (W / 4), c4 = idx % (W / 4);
        const u32x4 v = *reinterpret_cast<const u32x4*>(U + (size_t)(j0 + i) * K + j0 + 4 * c4);
        *reinterpret_cast<u32x4*>(Us + i * W + 4 * c4) = v;
    }
    __syncthreads();
    const int n = blockIdx.x * GQ_THREADS + tid;
    if (n >= N) return;                 // (no barrier behind this point)
    float* Ecol = Et + n;               // this lane's column of Et: written and read back by this lane alone

#pragma unroll 1
    for (int b = 0; b < C; ++b) {
        float w[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) w[i] = Wt[(size_t)(j0 + 32 * b + i) * N + n];
        // what the earlier blocks of the group owe this one, pivot by pivot in column order (the order of the definition)
#pragma unroll 8
        for (int p = 0; p < 32 * b; ++p) {
            const float err = Ecol[(size_t)p * N];
            const float* row = Us + p * W + 32 * b;
#pragma unroll
            for (int i = 0; i < 32; ++i) w[i] = fmaf(-err, row[i], w[i]);
        }
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < 32; ++i) amax = fmaxf(amax, fabsf(w[i]));
        const uint32_t bits = __float_as_uint(amax);
        const int ex = (int)(bits >> 23);                       // amax >= 0: no sign bit
        int e = ex - 129 + ((bits & 0x7fffffu) > 0x400000u ? 1 : 0);      // frexp exponent (ex - 126) - 3 + (m > 0.75)
        e = ex == 0 ? -125 : min(max(e, -125), 125);            // (a subnormal amax lies below 2^-126: the clamp decides)
        e = amax > 0.f ? e : 0;
        const float s = __uint_as_float((uint32_t)(e + 127) << 23), inv_s = __uint_as_float((uint32_t)(127 - e) << 23);
        const float* diag = Us + (32 * b) * W + 32 * b;         // the block's own 32 x 32 triangle of U
        uint32_t nib[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const float wi = w[i];
            const float a = fabsf(wi) * inv_s;
            const int c = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.0f);
            const float val = c < 4 ? 0.5f * (float)c : (c == 4 ? 2.f : (c == 5 ? 3.f : (c == 6 ? 4.f : 6.f)));
            const uint32_t sign = __float_as_uint(wi) >> 31;
            const float q = __uint_as_float(__float_as_uint(val * s) | (sign << 31));
            const float err = __fdiv_rn(wi - q, diag[i * W + i]);
            Ecol[(size_t)(32 * b + i) * N] = err;
            nib[i >> 3] |= ((uint32_t)c | (sign << 3)) << (4 * (i & 7));
#pragma unroll
            for (int i2 = i + 1; i2 < 32; ++i2) w[i2] = fmaf(-err, diag[i * W + i2], w[i2]);
        }
        const int g = (j0 >> 5) + b;
        const u32x4 out = {nib[0], nib[1], nib[2], nib[3]};
        *reinterpret_cast<u32x4*>(blocks + (size_t)n * (K >> 1) + (size_t)g * 16) = out;
        scales[(size_t)n * (K >> 5) + g] = (uint8_t)(e + 127);
    }
}

}  // namespace

extern "C" {

int spider_gptq_mxfp4_sweep_f32(const float* Wt, const float* U, void* blocks, void* scales, float* Et, int N, int K, int j0,
                                int nblocks, void* stream) {
    SPIDER_CHECK(Wt && U && blocks && scales && Et, "gptq_mxfp4_sweep: null pointer (Wt, U, blocks, scales and Et are required)");
    SPIDER_CHECK(N >= 1, "gptq_mxfp4_sweep: N must be >= 1");
    SPIDER_CHECK(K >= 32 && K % 32 == 0, "gptq_mxfp4_sweep: K must be a positive multiple of 32 (one E8M0 scale per block of 32)");
    SPIDER_CHECK(nblocks >= 1 && nblocks <= GQ_MAX_BLOCKS, "gptq_mxfp4_sweep: a launch takes 1..4 MX blocks");
    SPIDER_CHECK(j0 >= 0 && j0 % 32 == 0 && (long)j0 + 32L * nblocks <= (long)K,
                 "gptq_mxfp4_sweep: the group [j0, j0 + 32 nblocks) must start at a block and end within K");
    SPIDER_CHECK(((uintptr_t)U & 15) == 0 && ((uintptr_t)blocks & 15) == 0, "gptq_mxfp4_sweep: U and blocks must be 16-byte aligned");
    const dim3 grid((unsigned)((N + GQ_THREADS - 1) / GQ_THREADS));
    uint8_t* bl = (uint8_t*)blocks;
    uint8_t* sc = (uint8_t*)scales;
    hipStream_t st = (hipStream_t)stream;
    switch (nblocks) {
        case 1: gptq_mxfp4_sweep_kernel<1><<<grid, GQ_THREADS, 0, st>>>(Wt, U, bl, sc, Et, N, K, j0); break;
        case 2: gptq_mxfp4_sweep_kernel<2><<<grid, GQ_THREADS, 0, st>>>(Wt, U, bl, sc, Et, N, K, j0); break;
        case 3: gptq_mxfp4_sweep_kernel<3><<<grid, GQ_THREADS, 0, st>>>(Wt, U, bl, sc, Et, N, K, j0); break;
        default: gptq_mxfp4_sweep_kernel<4><<<grid, GQ_THREADS, 0, st>>>(Wt, U, bl, sc, Et, N, K, j0); break;
    }
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // extern "C"

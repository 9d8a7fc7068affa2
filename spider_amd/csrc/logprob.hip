// Teacher-forced scoring of rows of bf16 logits (LlamaForCausalLM.forward(labels=...): logits.float() -> log_softmax -> gather,
// ForCausalLMLoss; and the divergence between two models on the same positions). One block of 256 lanes per row, ONE pass over
// the row (two rows with logits_ref), fp32 throughout:
//   x = float(logits[r, :V]),  m = max x,  s = sum exp(x - m),  t = sum exp(x - m) (x - m)
//   lse     = m + log s
//   logprob = x[target] - lse                (target outside [0, V), e.g. HF's ignore_index -100: 0)
//   argmax  = lowest id among the maxima     (the (value, index) order of select.hpp)
//   entropy = -sum p log p = log s - t / s
//   with logits_ref, y = float(logits_ref[r, :V]), p_ref = softmax(y), w = sum exp(y - m_ref) (y - x):
//   kl      = KL(p_ref || p) = w / s_ref - lse_ref + lse,   argmax_ref
// Every lane keeps a running max and the sums relative to it; a group of 8 logits (one 16-byte load) first raises the max to the
// group's, rescales the sums by exp(old - new) (exactly 1 when the max stays), then adds its 8 terms one after the other. Lane
// l takes the groups l, l + 256, ...; the lane states merge by the same rescaling over the VALU cross-lane exchanges of
// common.hpp (xor 32 ... 1), the four wave states through LDS in wave order. A row's result therefore depends on the row alone:
// not on the number of rows in the call, not on its neighbours. The x and the y stream run the same instruction sequence, so
// logits_ref == logits gives lse_ref == lse bit for bit and kl == 0.0 exactly.
// Inputs are FINITE (|x| < 1e37): no inf / NaN handling; the masked tail of the last group carries the most negative bf16, whose
// terms are exact zeros beside a real value, and a lane without a group keeps the empty state (that max, sums 0). exp is v_exp_f32 on (x - m) * log2(e): the rounding of that product moves
// a term by |x - m| 2^-24 relative, which the tolerance of tests/logprob_checks.py carries next to the summation depth
// ceil(V / 256) + 8 + 8.
// A pure stream: 2 bytes per logit (4 with logits_ref), ~12 VALU operations per logit, plain vector stores, no atomics.
#include "common.hpp"
#include "select.hpp"
#include <type_traits>

using namespace spider;

namespace {

constexpr int LP_THREADS = 256;         // lanes per row (the summation depth of the tolerance is derived from it)
constexpr int LP_UNROLL = 4;            // 16-byte loads in flight per lane and stream
constexpr uint32_t LP_NEG_PAIR = 0xFF7FFF7Fu;   // two bf16 of the most negative finite value: masked logits
constexpr float LOG2E = 1.4426950408889634f;

struct RowState {
    float m, s, t;      // running max, sum e, sum e (x - m)
};

__device__ __forceinline__ float lp_exp(float z) { return __builtin_amdgcn_exp2f(z * LOG2E); }

// MASK: the batch behind the last full one -- values at or past V (the tail of the last group, groups past the row) are masked
template <bool MASK>
__device__ __forceinline__ void unpack8(const u32x4 q, int base, int V, float v[8]) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    const float neg = bf16hi_to_f32(LP_NEG_PAIR);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[2 * e] = (!MASK || base + 2 * e < V) ? bf16lo_to_f32(w[e]) : neg;
        v[2 * e + 1] = (!MASK || base + 2 * e + 1 < V) ? bf16hi_to_f32(w[e]) : neg;
    }
}

// One group of 8 values into a lane's state: raise the max to the group's and rescale (the factor is returned for the sum the
// caller keeps beside the state), add the 8 terms in order; W: also w += e (v - xs). The arg-max is kept per group -- a lane's
// record changes a handful of times per row, so the index search sits behind a rarely taken branch; ids ascend within a lane
// and within a group, so '>' and "first equal" keep the lowest id.
template <bool W>
__device__ __forceinline__ float state_add8(RowState& a, float& best, int& bidx, const float v[8], int base, const float* xs, float& w) {
#pragma clang fp contract(off)
    const float gm = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
    if (gm > best) {
        best = gm;
        int e = 7;
#pragma unroll
        for (int i = 6; i >= 0; --i) e = v[i] == gm ? i : e;
        bidx = base + e;
    }
    const float mn = fmaxf(a.m, gm);
    const float d = a.m - mn;
    const float c = lp_exp(d);
    a.t = c * fmaf(d, a.s, a.t);
    a.s = a.s * c;
    a.m = mn;
    if (W) w = w * c;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float z = v[e] - mn;
        const float ex = lp_exp(z);
        a.s = a.s + ex;
        a.t = fmaf(ex, z, a.t);
        if (W) w = fmaf(ex, v[e] - xs[e], w);
    }
    return c;
}

__device__ __forceinline__ RowState state_merge(const RowState a, const RowState b, float& ca, float& cb) {
#pragma clang fp contract(off)
    RowState r;
    r.m = fmaxf(a.m, b.m);
    const float da = a.m - r.m, db = b.m - r.m;
    ca = lp_exp(da);
    cb = lp_exp(db);
    r.s = a.s * ca + b.s * cb;
    r.t = ca * fmaf(da, a.s, a.t) + cb * fmaf(db, b.s, b.t);
    return r;
}

template <int M>
__device__ __forceinline__ void xor_merge(RowState& a, float* w, u64& key) {
#pragma clang fp contract(off)
    RowState b;
    b.m = lane_xor<M>(a.m); b.s = lane_xor<M>(a.s); b.t = lane_xor<M>(a.t);
    float ca, cb;
    const RowState r = state_merge(a, b, ca, cb);
    if (w) {
        const float wb = lane_xor<M>(*w);
        *w = *w * ca + wb * cb;
    }
    a = r;
    const u64 kb = ((u64)lane_xor<M>((uint32_t)(key >> 32)) << 32) | (u64)lane_xor<M>((uint32_t)key);
    key = kb > key ? kb : key;
}

__device__ __forceinline__ void wave_merge(RowState& a, float* w, u64& key) {
    xor_merge<32>(a, w, key); xor_merge<16>(a, w, key); xor_merge<8>(a, w, key);
    xor_merge<4>(a, w, key); xor_merge<2>(a, w, key); xor_merge<1>(a, w, key);
}

struct LpShared {
    RowState st[2][LP_THREADS / 64];
    float w[LP_THREADS / 64];
    u64 key[2][LP_THREADS / 64];
};

template <bool REF>
__global__ __launch_bounds__(LP_THREADS) void logprob_rows_kernel(const bf16_t* __restrict__ logits, int ld,
                                                                  const int* __restrict__ targets,
                                                                  const bf16_t* __restrict__ logits_ref, int ld_ref,
                                                                  float* __restrict__ logprob, float* __restrict__ lse_out,
                                                                  int* __restrict__ argmax, float* __restrict__ entropy,
                                                                  float* __restrict__ kl, int* __restrict__ argmax_ref, int V) {
#pragma clang fp contract(off)
    __shared__ LpShared sh;
    const int r = blockIdx.x, tid = threadIdx.x;
    const bf16_t* row = logits + (size_t)r * ld;
    const bf16_t* rrow = REF ? logits_ref + (size_t)r * ld_ref : nullptr;
    const int ngroups = (V + 7) >> 3;       // the last group may reach past V, never past ld (ld % 8 == 0, ld >= V)
    const float neg = bf16hi_to_f32(LP_NEG_PAIR);
    RowState a{neg, 0.f, 0.f}, b{neg, 0.f, 0.f};
    float w = 0.f;                          // sum e_ref (y - x), relative to b.m
    float bx = neg, by = neg;               // per-lane best value; ids ascend within a lane, so '>' keeps the lowest id
    int ix = 0x7fffffff, iy = 0x7fffffff;

    // Batches of LP_UNROLL groups per lane (lane l: groups gb + l + u * 256). The first nb batches hold full groups for every lane and
    // run unmasked; what is left (< one batch, the ragged last group included) is ONE guarded, masked batch. The loads of batch
    // k + 1 are issued before batch k is summed.
    constexpr int BATCH = LP_THREADS * LP_UNROLL;
    const int nb = (V >> 3) / BATCH;
    u32x4 cx[LP_UNROLL], cy[LP_UNROLL], nx[LP_UNROLL], ny[LP_UNROLL];
    auto load = [&](int k, u32x4* qx, u32x4* qy) {
#pragma unroll
        for (int u = 0; u < LP_UNROLL; ++u) {
            const int g = k * BATCH + u * LP_THREADS + tid;
            const u32x4 fill = {LP_NEG_PAIR, LP_NEG_PAIR, LP_NEG_PAIR, LP_NEG_PAIR};
            const bool ok = k < nb || g < ngroups;      // (uniform for k < nb)
            qx[u] = ok ? *reinterpret_cast<const u32x4*>(row + (size_t)g * 8) : fill;
            if (REF) qy[u] = ok ? *reinterpret_cast<const u32x4*>(rrow + (size_t)g * 8) : fill;
        }
    };
    auto sum = [&](int k, const u32x4* qx, const u32x4* qy, auto masked) {
        constexpr bool MASK = decltype(masked)::value;
#pragma unroll
        for (int u = 0; u < LP_UNROLL; ++u) {
            const int base = (k * BATCH + u * LP_THREADS + tid) * 8;
            // a group past the row is skipped, not summed: under a max that is still the mask value its 8 terms would be exp(0)
            if (MASK && base >= V) continue;
            float x[8], y[8], none = 0.f;
            unpack8<MASK>(qx[u], base, V, x);
            state_add8<false>(a, bx, ix, x, base, nullptr, none);
            if (REF) {
                unpack8<MASK>(qy[u], base, V, y);
                state_add8<true>(b, by, iy, y, base, x, w);
            }
        }
    };
    load(0, cx, cy);
    for (int k = 0; k < nb; ++k) {
        load(k + 1, nx, ny);
        sum(k, cx, cy, std::false_type{});
#pragma unroll
        for (int u = 0; u < LP_UNROLL; ++u) { cx[u] = nx[u]; if (REF) cy[u] = ny[u]; }
    }
    sum(nb, cx, cy, std::true_type{});

    // lanes without a logit hold (neg, id 0x7fffffff): below every real key
    u64 kx = make_key(bx, (uint32_t)ix), ky = make_key(by, (uint32_t)iy);
    wave_merge(a, nullptr, kx);
    if (REF) wave_merge(b, &w, ky);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) {
        sh.st[0][wv] = a; sh.key[0][wv] = kx;
        if (REF) { sh.st[1][wv] = b; sh.w[wv] = w; sh.key[1][wv] = ky; }
    }
    __syncthreads();
    if (tid != 0) return;
    RowState A = sh.st[0][0], B = sh.st[1][0];
    float W = sh.w[0];
    u64 KX = sh.key[0][0], KY = sh.key[1][0];
#pragma unroll
    for (int i = 1; i < LP_THREADS / 64; ++i) {
        float ca, cb;
        A = state_merge(A, sh.st[0][i], ca, cb);
        KX = sh.key[0][i] > KX ? sh.key[0][i] : KX;
        if (REF) {
            B = state_merge(B, sh.st[1][i], ca, cb);
            W = W * ca + sh.w[i] * cb;
            KY = sh.key[1][i] > KY ? sh.key[1][i] : KY;
        }
    }
    const float lse = A.m + logf(A.s);
    const int tg = targets[r];
    logprob[r] = (tg >= 0 && tg < V) ? bf16_to_f32(row[tg]) - lse : 0.f;
    lse_out[r] = lse;
    argmax[r] = (int)key_index(KX);
    entropy[r] = logf(A.s) - A.t / A.s;
    if (REF) {
        const float lse_ref = B.m + logf(B.s);
        kl[r] = (W / B.s - lse_ref) + lse;
        argmax_ref[r] = (int)key_index(KY);
    }
}

}  // namespace

extern "C" {

int spider_logprob_rows_bf16(const void* logits, int ld, const int* targets, const void* logits_ref, int ld_ref, float* logprob,
                             float* lse, int* argmax, float* entropy, float* kl, int* argmax_ref, int rows, int V, void* stream) {
    SPIDER_CHECK(logits && targets && logprob && lse && argmax && entropy, "logprob_rows: logits, targets and the four outputs required");
    SPIDER_CHECK(rows > 0, "logprob_rows: rows must be >= 1");
    SPIDER_CHECK(V >= 1, "logprob_rows: V must be >= 1");
    SPIDER_CHECK(ld >= V && ld % 8 == 0, "logprob_rows: ld must be >= V and a multiple of 8 (16-byte loads)");
    SPIDER_CHECK(((uintptr_t)logits & 15) == 0, "logprob_rows: logits must be 16-byte aligned");
    SPIDER_CHECK((logits_ref != nullptr) == (kl != nullptr) && (logits_ref != nullptr) == (argmax_ref != nullptr),
                 "logprob_rows: logits_ref, kl and argmax_ref come together");
    if (logits_ref) {
        SPIDER_CHECK(ld_ref >= V && ld_ref % 8 == 0, "logprob_rows: ld_ref must be >= V and a multiple of 8 (16-byte loads)");
        SPIDER_CHECK(((uintptr_t)logits_ref & 15) == 0, "logprob_rows: logits_ref must be 16-byte aligned");
        logprob_rows_kernel<true><<<rows, LP_THREADS, 0, (hipStream_t)stream>>>((const bf16_t*)logits, ld, targets,
                                                                                  (const bf16_t*)logits_ref, ld_ref, logprob, lse,
                                                                                  argmax, entropy, kl, argmax_ref, V);
    } else {
        logprob_rows_kernel<false><<<rows, LP_THREADS, 0, (hipStream_t)stream>>>((const bf16_t*)logits, ld, targets, nullptr, 0,
                                                                                   logprob, lse, argmax, entropy, nullptr, nullptr, V);
    }
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // extern "C"

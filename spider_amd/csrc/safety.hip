// Stable Diffusion safety checker, the parts around the CLIP ViT (gfx950): the feature extractor on the VAE's output buffer, the
// concept decision and the black-out of flagged images (spider/models/custom_sd.py:376-384 run_safety_checker, called at :658).
//   spider_clip_preprocess      numpy_to_pil + CLIPImageProcessor: 8-bit quantisation, Pillow's antialiased BICUBIC resize (horizontal
//                               pass, then vertical, each rounded to 8 bits and clipped, 22-bit fixed-point taps as in Pillow's
//                               Resample.c), centre crop, (v/255 - mean)/std, written as the patch rows of the ViT's patch-embedding GEMM
//   spider_safety_decide        StableDiffusionSafetyChecker.forward of diffusers 0.25 after the ViT: fp32 cosine similarities, the
//                               special-care cascade, three-decimal rounding, one flag per image
//   spider_image_blackout_f32   flagged images become zeros in place
// One translation unit for both 16-bit formats: the format is an argument (0 = bf16, 1 = IEEE half), not a second build.
#include "common.hpp"

using namespace spider;

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow: 8-bit pixels, 2 bits of headroom for the negative lobes
constexpr int MAX_CONCEPTS = 64;                // special-care + concepts (the published checker has 3 + 17)

__device__ __forceinline__ float ld16(uint16_t v, int f16) {
    return f16 ? (float)__builtin_bit_cast(_Float16, v) : bf16_to_f32(v);
}
__device__ __forceinline__ uint16_t st16(float v, int f16) {
    return f16 ? __builtin_bit_cast(uint16_t, (_Float16)v) : f32_to_bf16(v);
}
__device__ __forceinline__ float lo16(uint32_t p, int f16) { return ld16((uint16_t)(p & 0xffffu), f16); }
__device__ __forceinline__ float hi16(uint32_t p, int f16) { return ld16((uint16_t)(p >> 16), f16); }

__device__ __forceinline__ int clip8(int acc) {      // Pillow clip8: (acc + half) >> bits, clipped to 0..255 (the caller adds half)
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// (x * 255).round().astype(uint8) of numpy_to_pil: fp32 product, round-half-even
__device__ __forceinline__ int quant8(float x) {
    const float q = rintf(x * 255.f);
    return q >= 255.f ? 255 : (q > 0.f ? (int)q : 0);      // NaN -> 0
}

// Horizontal pass over the crop's columns: tmp[b, c, y, j] = clip8(sum_t quant8(img[b, c, y, xmin_j + t]) * k_j[t]), j in [0, crop).
// bounds [crop, 2] = (xmin, count); taps [crop, ks] int32 (22-bit fixed point, zero beyond count).
__global__ __launch_bounds__(256) void clip_resize_h_kernel(const float* __restrict__ img, uint8_t* __restrict__ tmp,
                                                            const int* __restrict__ bounds, const int* __restrict__ taps, int ks,
                                                            int rows, int W, int crop) {
    const size_t total = (size_t)rows * crop;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int j = (int)(i % crop);
        const size_t row = i / crop;                       // (b, c, y) flattened: rows of W floats
        const int x0 = bounds[2 * j], n = min(bounds[2 * j + 1], ks);
        const float* src = img + row * W;
        const int* k = taps + (size_t)j * ks;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < n; ++t) acc += quant8(src[min(max(x0 + t, 0), W - 1)]) * k[t];
        tmp[i] = (uint8_t)clip8(acc);
    }
}

// Vertical pass over the crop's rows + normalisation + patch rows. rows_out [B * P, Kp], P = (crop / patch)^2, column
// k = (c * patch + dy) * patch + dx for k < 3 patch^2, zero beyond. One thread writes 8 columns (16 bytes).
__global__ __launch_bounds__(256) void clip_resize_v_patch_kernel(const uint8_t* __restrict__ tmp, uint16_t* __restrict__ rows_out,
                                                                  const int* __restrict__ bounds, const int* __restrict__ taps, int ks,
                                                                  const float* __restrict__ norm, int B, int H, int crop, int patch,
                                                                  int Kp, int f16) {
    const int g = crop / patch, P = g * g, K = 3 * patch * patch, K8 = Kp / 8;
    const size_t total = (size_t)B * P * K8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int k8 = (int)(i % K8);
        const size_t bp = i / K8;
        const int p = (int)(bp % P), b = (int)(bp / P);
        const int py = p / g, px = p % g;
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k8 * 8 + e;
            float v = 0.f;
            if (k < K) {
                const int c = k / (patch * patch), r = k % (patch * patch);
                const int y = py * patch + r / patch, x = px * patch + r % patch;
                const int y0 = bounds[2 * y], n = min(bounds[2 * y + 1], ks);
                const int* kk = taps + (size_t)y * ks;
                const uint8_t* col = tmp + ((size_t)(b * 3 + c) * H) * crop + x;
                int acc = 1 << (PRECISION_BITS - 1);
                for (int t = 0; t < n; ++t) acc += (int)col[(size_t)min(max(y0 + t, 0), H - 1) * crop] * kk[t];
                v = ((float)clip8(acc) / 255.f - norm[c]) / norm[3 + c];
            }
            const uint32_t h = st16(v, f16);
            o[e >> 1] = (e & 1) ? (o[e >> 1] | (h << 16)) : h;
        }
        *reinterpret_cast<u32x4*>(rows_out + i * 8) = u32x4{o[0], o[1], o[2], o[3]};
    }
}

// One block of 4 waves per image. Wave w takes rows w, w + 4, ... of [special | concepts]; its 64 lanes stride over D in 16-byte
// pieces and wave-reduce dot, |e|^2 and |c|^2 in fp32. Thread 0 then runs the 20 serial compares.
__global__ __launch_bounds__(256) void safety_decide_kernel(const uint16_t* __restrict__ emb, const uint16_t* __restrict__ concepts,
                                                            const uint16_t* __restrict__ special, const float* __restrict__ thr_c,
                                                            const float* __restrict__ thr_s, float* __restrict__ scores,
                                                            int* __restrict__ flags, int D, int n_c, int n_s, int f16) {
    __shared__ float cosv[MAX_CONCEPTS];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = n_s + n_c;
    const u32x4* e4 = reinterpret_cast<const u32x4*>(emb + (size_t)b * D);
    for (int j = w; j < n; j += 4) {
        const uint16_t* row = j < n_s ? special + (size_t)j * D : concepts + (size_t)(j - n_s) * D;
        const u32x4* c4 = reinterpret_cast<const u32x4*>(row);
        float dot = 0.f, ee = 0.f, cc = 0.f;
        for (int i = lane; i < D / 8; i += 64) {
            const u32x4 ev = e4[i], cv = c4[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float e0 = lo16(ev[q], f16), e1 = hi16(ev[q], f16), c0 = lo16(cv[q], f16), c1 = hi16(cv[q], f16);
                dot = fmaf(e0, c0, dot); dot = fmaf(e1, c1, dot);
                ee = fmaf(e0, e0, ee); ee = fmaf(e1, e1, ee);
                cc = fmaf(c0, c0, cc); cc = fmaf(c1, c1, cc);
            }
        }
        dot = wave_sum(dot); ee = wave_sum(ee); cc = wave_sum(cc);
        // F.normalize on both sides, then the dot: x / max(|x|, 1e-12)
        if (lane == 0) cosv[j] = dot / (fmaxf(sqrtf(ee), 1e-12f) * fmaxf(sqrtf(cc), 1e-12f));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float adj = 0.f;
        int flag = 0;
        float* out = scores + (size_t)b * n;
        for (int j = 0; j < n; ++j) {
            const float thr = j < n_s ? thr_s[j] : thr_c[j - n_s];
            const float s = rintf((cosv[j] - thr + adj) * 1000.f) / 1000.f;      // round(x, 3): half-even on x * 1000
            out[j] = s;
            if (s > 0.f) {
                if (j < n_s) adj = 0.01f;
                else flag = 1;
            }
        }
        flags[b] = flag;
    }
}

// grid (pieces of one image, B): a block of a flagged image writes 256 x 16 bytes of zeros
__global__ __launch_bounds__(256) void image_blackout_kernel(float* __restrict__ img, const int* __restrict__ flags, size_t per_image4) {
    if (flags[blockIdx.y] == 0) return;
    f32x4* p = reinterpret_cast<f32x4*>(img) + (size_t)blockIdx.y * per_image4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per_image4; i += (size_t)gridDim.x * 256) p[i] = f32x4{0.f, 0.f, 0.f, 0.f};
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int grid_for(size_t total, int cap = 4096) {
    const size_t g = (total + 255) / 256;
    return (int)(g > (size_t)cap ? cap : (g ? g : 1));
}

}  // namespace

extern "C" {

int spider_clip_preprocess(const float* images, void* tmp, void* rows, const int* xbounds, const int* xtaps, int ks_x,
                           const int* ybounds, const int* ytaps, int ks_y, const float* norm, int B, int H, int W, int crop, int patch,
                           int Kp, int f16, void* stream) {
    SPIDER_CHECK(images && tmp && rows && xbounds && xtaps && ybounds && ytaps && norm, "clip_preprocess: null pointer");
    SPIDER_CHECK(B > 0 && H > 0 && W > 0 && crop > 0 && patch > 0 && crop % patch == 0, "clip_preprocess: crop must be a multiple of patch");
    SPIDER_CHECK(ks_x >= 1 && ks_x <= 4096 && ks_y >= 1 && ks_y <= 4096, "clip_preprocess: tap count out of range");
    SPIDER_CHECK(Kp % 8 == 0 && Kp >= 3 * patch * patch && Kp < 3 * patch * patch + 8, "clip_preprocess: Kp must be 3 patch^2 rounded up to a multiple of 8 (Kp % 8)");
    SPIDER_CHECK(aligned16(rows), "clip_preprocess: rows must be 16-byte aligned");
    SPIDER_CHECK(f16 == 0 || f16 == 1, "clip_preprocess: format must be 0 (bf16) or 1 (f16)");
    SPIDER_CHECK((size_t)B * 3 * H * (size_t)(W > crop ? W : crop) < ((size_t)1 << 40), "clip_preprocess: image too large");
    const int P = (crop / patch) * (crop / patch);
    clip_resize_h_kernel<<<grid_for((size_t)B * 3 * H * crop), 256, 0, (hipStream_t)stream>>>(images, (uint8_t*)tmp, xbounds, xtaps, ks_x,
                                                                                             B * 3 * H, W, crop);
    SPIDER_LAUNCH_OK();
    clip_resize_v_patch_kernel<<<grid_for((size_t)B * P * (Kp / 8)), 256, 0, (hipStream_t)stream>>>(
        (const uint8_t*)tmp, (uint16_t*)rows, ybounds, ytaps, ks_y, norm, B, H, crop, patch, Kp, f16);
    SPIDER_LAUNCH_OK();
    return 0;
}

int spider_safety_decide(const void* image_embeds, const void* concept_embeds, const void* special_care_embeds, const float* thr_concept,
                         const float* thr_special, float* scores, int* flags, int B, int D, int n_concept, int n_special, int f16,
                         void* stream) {
    SPIDER_CHECK(image_embeds && concept_embeds && thr_concept && scores && flags, "safety_decide: null pointer");
    SPIDER_CHECK(n_special == 0 || (special_care_embeds && thr_special), "safety_decide: null special-care pointer");
    SPIDER_CHECK(B > 0 && D > 0 && D % 8 == 0, "safety_decide: D must be a multiple of 8 (D % 8)");
    SPIDER_CHECK(n_concept >= 1 && n_special >= 0 && n_concept + n_special <= MAX_CONCEPTS, "safety_decide: at most 64 concepts + special-care concepts");
    SPIDER_CHECK(aligned16(image_embeds) && aligned16(concept_embeds) && aligned16(special_care_embeds), "safety_decide: embeddings must be 16-byte aligned");
    SPIDER_CHECK(f16 == 0 || f16 == 1, "safety_decide: format must be 0 (bf16) or 1 (f16)");
    safety_decide_kernel<<<B, 256, 0, (hipStream_t)stream>>>((const uint16_t*)image_embeds, (const uint16_t*)concept_embeds,
                                                              (const uint16_t*)special_care_embeds, thr_concept, thr_special, scores, flags,
                                                              D, n_concept, n_special, f16);
    SPIDER_LAUNCH_OK();
    return 0;
}

int spider_image_blackout_f32(float* images, const int* flags, int B, long per_image, void* stream) {
    SPIDER_CHECK(images && flags, "image_blackout: null pointer");
    SPIDER_CHECK(B > 0 && B <= 65535 && per_image > 0 && per_image % 4 == 0, "image_blackout: C*H*W must be a multiple of 4, B <= 65535");
    SPIDER_CHECK(aligned16(images), "image_blackout: images must be 16-byte aligned");
    const size_t n4 = (size_t)per_image / 4;
    image_blackout_kernel<<<dim3(grid_for(n4, 1024), B), 256, 0, (hipStream_t)stream>>>(images, flags, n4);
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // extern "C"

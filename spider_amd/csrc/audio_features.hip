// Whisper log-mel features of Qwen2.5-Omni's audio input (gfx950): what WhisperFeatureExtractor._torch_extract_fbank_features computes
// for clips padded to n_samples, on the packed waveforms where they lie (spider_amd/audio_features.py states the definition).
//   spider_logmel_f32   two launches on the caller's stream, no host synchronisation:
//     logmel_power_kernel    one block per tile of 32 frames of one clip. The samples the tile's windows cover are fetched once into LDS
//                            (reflect pad at the front, zeros behind the clip, reflect at n_samples: index arithmetic, no padded copy);
//                            frames x windowed-DFT table on the fp32-input MFMA (exact fp32: a k-ordered fmaf chain), re^2 + im^2 in
//                            registers, the power tile in LDS, mel projection on the same MFMA, log10(max(., 1e-10)) stored in HF's
//                            [B, mel, cap] layout, the tile's maximum to tile_max[b, tile]
//     logmel_finish_kernel   clip maximum from the tile maxima (fixed order, no float atomics), max(., clip_max - 8), (. + 4) / 4 in
//                            place, the floor value into every frame whose window holds only padding, the int32 frame mask
// Only frames with signal are computed: the grid's x extent comes from the host-known longest clip; the per-clip counts are read
// from the device arrays. cap, n_fft, hop and mel are runtime arguments: one build serves every configuration.
#include "common.hpp"

using namespace spider;

namespace {

constexpr int TILE_F = 32;            // frames per block = rows of one 32x32x2 MFMA
constexpr int MAX_NFFT = 512, MAX_MEL = 128;

__device__ __forceinline__ f32x16 mfma_32x32x2(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// frames of clip length L (already capped at n_samples) whose window [f hop - n_fft / 2, f hop + n_fft / 2) holds a sample of the clip
__device__ __forceinline__ int frames_with_signal(int L, int n_fft, int hop, int cap) {
    const long n = ((long)L + n_fft / 2 + hop - 1) / hop;
    return (int)(n < cap ? n : cap);
}

// table [n_fft, ldt]: per group g of 32 bins, columns [64 g, 64 g + 32) = w[n] cos(2 pi n k / n_fft), [64 g + 32, 64 g + 64) =
// w[n] sin(.) for k = 32 g + j; bins beyond n_fft / 2 are zero columns. fb [nb, mel] row-major. logspec [B, mel, cap].
// LDS: sig = the tile's samples, sample s at s + (s / hop) padh (padh makes the frame stride odd: the 32 rows of an A fragment fall
// into 32 different banks); pw = power tile [32][pw_ld], pw_ld odd; 4 floats behind it for the block's maximum.
__global__ __launch_bounds__(256) void logmel_power_kernel(const float* __restrict__ wave, const int* __restrict__ offsets,
                                                           const int* __restrict__ lengths, const float* __restrict__ table,
                                                           const float* __restrict__ fb, float* __restrict__ logspec,
                                                           float* __restrict__ tile_max, int n_samples, int n_fft, int hop, int mel,
                                                           int cap, int ldt, int groups, int padh, int sig_floats, int pw_ld, int max_tiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* sig = lds;
    float* pw = lds + sig_floats;
    float* red = pw + TILE_F * pw_ld;                        // 4 floats: the waves' maxima
    const int b = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int L = min(max(lengths[b], 0), n_samples);
    const int nsig = frames_with_signal(L, n_fft, hop, cap);
    const int f0 = tile * TILE_F;
    if (f0 >= nsig) return;                                  // uniform per block
    const float* x = wave + offsets[b];
    const int nb = n_fft / 2 + 1, half = n_fft / 2;

    // the samples under the tile's windows
    const int span = (TILE_F - 1) * hop + n_fft;
    for (int s = tid; s < span; s += 256) {
        long i = (long)f0 * hop + s - half;
        if (i < 0) i = -i;                                   // reflect at the front
        if (i >= n_samples) i = 2L * (n_samples - 1) - i;    // reflect at n_samples
        const float v = (i >= 0 && i < L) ? x[i] : 0.f;      // zeros behind the clip
        sig[s + (s / hop) * padh] = v;
    }
    __syncthreads();

    // frames x table -> power. Wave w takes bin groups w, w + 4, ...: the cos and the sin tile of a group share lane and register.
    const int row = lane & 31, kh = lane >> 5;
    const int a_base = row * (hop + padh);
    for (int g = w; g < groups; g += 4) {
        f32x16 re, im;
#pragma unroll
        for (int r = 0; r < 16; ++r) { re[r] = 0.f; im[r] = 0.f; }
        const float* tb = table + (size_t)kh * ldt + g * 64 + row;
        // n = k + kh; q = n / hop kept incrementally. padh != 0 only for an even hop (>= 2), where a step of 2 wraps at most once;
        // for an odd hop q multiplies padh = 0
        int n = kh, q = n / hop, rem = n - q * hop;
        // 4 steps of k per trip; the 12 loads of the NEXT trip are issued before the 8 MFMAs of this one (a table row pair is an L2
        // round trip: the MFMAs cover it). Steps beyond n_fft load nothing and multiply zeros.
        float a[4], bc[4], bs[4];
        auto fetch = [&](int k) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool live = k + 2 * u < n_fft;
                a[u] = live ? sig[a_base + n + q * padh] : 0.f;
                bc[u] = live ? tb[0] : 0.f;
                bs[u] = live ? tb[32] : 0.f;
                tb += 2 * (size_t)ldt;
                n += 2; rem += 2;
                const bool wrap = rem >= hop;
                rem -= wrap ? hop : 0;
                q += wrap ? 1 : 0;
            }
        };
        fetch(0);
        for (int k = 0; k < n_fft; k += 8) {
            float a0[4], bc0[4], bs0[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a0[u] = a[u]; bc0[u] = bc[u]; bs0[u] = bs[u]; }
            fetch(k + 8);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                re = mfma_32x32x2(a0[u], bc0[u], re);
                im = mfma_32x32x2(a0[u], bs0[u], im);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = (r & 3) + 8 * (r >> 2) + 4 * kh;
            pw[f * pw_ld + g * 32 + row] = fmaf(re[r], re[r], im[r] * im[r]);
        }
    }
    __syncthreads();

    // mel projection, transposed so that a lane's column is a frame: D[m, f] = sum_k fb[k, m] pw[f, k]. Wave w takes mel rows
    // [32 w, 32 w + 32); k runs to nb rounded up to even (bins beyond nb hold zero power, the filter is read as zero there).
    float tmax = -INFINITY;
    if (w * 32 < mel) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const int m_a = w * 32 + row;
        const float* pr = pw + row * pw_ld;
        // 4 steps of k per trip, loads first: the filter rows come from L2. pr[kk] stays inside the row for kk <= nb + 6 only if
        // guarded: columns beyond nb are not read.
        for (int k = 0; k < nb; k += 8) {
            float fa[4], pb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = k + 2 * u + kh;
                const bool live = kk < nb;
                fa[u] = (live && m_a < mel) ? fb[(size_t)kk * mel + m_a] : 0.f;
                pb[u] = live ? pr[kk] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = mfma_32x32x2(fa[u], pb[u], acc);
        }
        const int f = f0 + row;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = w * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (m < mel && f < nsig) {
                // log10 in double, rounded once: log10f is a ulp off at the floor (the fp32 next to 1e-10 must give -10, so that an
                // all-zero clip is -1.5 everywhere as on the host); 16 values per lane
                const float v = (float)log10((double)fmaxf(acc[r], 1e-10f));
                logspec[((size_t)b * mel + m) * cap + f] = v;
                tmax = fmaxf(tmax, v);
            }
        }
    }
    tmax = wave_max(tmax);
    if (lane == 0) red[w] = tmax;
    __syncthreads();
    if (tid == 0) tile_max[(size_t)b * max_tiles + tile] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// grid (pieces, B). Every block reduces its clip's tile maxima itself (at most a few hundred floats), then walks [mel, cap] in
// pieces of 4 frames: computed frames are clamped and scaled in place, the others get the floor value. Row 0's threads write the mask.
__global__ __launch_bounds__(256) void logmel_finish_kernel(const int* __restrict__ lengths, const float* __restrict__ tile_max,
                                                            float* __restrict__ feat, int* __restrict__ mask, int n_samples, int n_fft,
                                                            int hop, int mel, int cap, int max_tiles, int vec) {
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int L = min(max(lengths[b], 0), n_samples);
    const int nsig = min(frames_with_signal(L, n_fft, hop, cap), max_tiles * TILE_F);
    const int nv = (int)min(((long)L + hop - 1) / hop, (long)cap);
    const int ntiles = (nsig + TILE_F - 1) / TILE_F;
    float m = -INFINITY;
    for (int t = tid; t < ntiles; t += 256) m = fmaxf(m, tile_max[(size_t)b * max_tiles + t]);
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    const float cmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float lo = cmax - 8.f;
    const float fl = (fmaxf(lo, -10.f) + 4.f) * 0.25f;       // a frame of padding: log10(1e-10) = -10 under the same clamp
    const int c4 = (cap + 3) / 4;
    const size_t total = (size_t)mel * c4;
    float* out = feat + (size_t)b * mel * cap;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < total; i += (size_t)gridDim.x * 256) {
        const int row = (int)(i / c4), f = (int)(i % c4) * 4;
        float* p = out + (size_t)row * cap + f;
        if (vec) {                                           // cap % 4 == 0 and a 16-byte aligned base
            f32x4 v = {fl, fl, fl, fl};
            if (f < nsig) {
                const f32x4 o = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (f + e < nsig) v[e] = (fmaxf(o[e], lo) + 4.f) * 0.25f;
            }
            *reinterpret_cast<f32x4*>(p) = v;
        } else {
            for (int e = 0; e < 4 && f + e < cap; ++e) p[e] = f + e < nsig ? (fmaxf(p[e], lo) + 4.f) * 0.25f : fl;
        }
        if (row == 0)
            for (int e = 0; e < 4 && f + e < cap; ++e) mask[(size_t)b * cap + f + e] = f + e < nv ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int spider_logmel_tile_frames(void) { return TILE_F; }

int spider_logmel_f32(const float* waves, const int* offsets, const int* lengths, const float* table, const float* fb, float* feat,
                      int* mask, float* tile_max, int B, int n_samples, int n_fft, int hop, int mel, int cap, int ldt, int max_tiles,
                      void* stream) {
    SPIDER_CHECK(waves && offsets && lengths && table && fb && feat && mask && tile_max, "logmel: null pointer");
    SPIDER_CHECK(B > 0 && B <= 65535, "logmel: batch must be 1..65535");
    SPIDER_CHECK(n_fft >= 2 && n_fft <= MAX_NFFT && n_fft % 2 == 0, "logmel: n_fft must be even and at most 512");
    SPIDER_CHECK(mel >= 1 && mel <= MAX_MEL, "logmel: feature_size (mel) must be 1..128");
    SPIDER_CHECK(hop >= 1 && hop <= n_fft, "logmel: hop_length must be 1..n_fft");
    SPIDER_CHECK(n_samples > n_fft / 2 && cap >= 1 && (long)cap * hop <= (long)n_samples, "logmel: cap * hop must not exceed n_samples, n_samples > n_fft / 2");
    const int groups = (n_fft / 2 + 1 + 31) / 32;
    SPIDER_CHECK(ldt == groups * 64, "logmel: table leading dimension must be 64 * ceil((n_fft / 2 + 1) / 32)");
    SPIDER_CHECK(max_tiles >= 1 && max_tiles <= (cap + TILE_F - 1) / TILE_F, "logmel: max_tiles out of range");
    const int padh = (hop & 1) ? 0 : 1;
    const int span = (TILE_F - 1) * hop + n_fft;
    const int sig_floats = (span + (span / hop + 1) * padh + 3) & ~3;
    const int pw_ld = groups * 32 + 1;
    const size_t lds_bytes = (size_t)(sig_floats + TILE_F * pw_ld + 4) * sizeof(float);
    SPIDER_CHECK(lds_bytes <= 64 * 1024 - 64, "logmel: 31 hop + n_fft samples and the power tile do not fit in 64 KiB of LDS (hop too large)");
    hipStream_t s = (hipStream_t)stream;
    logmel_power_kernel<<<dim3(max_tiles, B), 256, lds_bytes, s>>>(waves, offsets, lengths, table, fb, feat, tile_max, n_samples, n_fft,
                                                                   hop, mel, cap, ldt, groups, padh, sig_floats, pw_ld, max_tiles);
    SPIDER_LAUNCH_OK();
    const int vec = (cap % 4 == 0 && ((uintptr_t)feat & 15) == 0) ? 1 : 0;
    const size_t pieces = ((size_t)mel * ((cap + 3) / 4) + 255) / 256;
    logmel_finish_kernel<<<dim3((unsigned)(pieces > 1024 ? 1024 : pieces), B), 256, 0, s>>>(lengths, tile_max, feat, mask, n_samples,
                                                                                             n_fft, hop, mel, cap, max_tiles, vec);
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // extern "C"

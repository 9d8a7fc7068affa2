// Qwen2-VL image processor, the image input of Qwen2.5-Omni (gfx950): a packed batch of uint8 RGB images (interleaved HWC, each its own
// size) -> the patch rows `pixel_values` [sum_i Gh_i Gw_i, 3 Tp P^2] that Qwen2VLImageProcessorPil returns.
//   qwen_resize_h_kernel         Pillow's antialiased BICUBIC, horizontal pass: 22-bit fixed-point taps (built on the host per image size,
//                                ops.bicubic_taps), clip8((sum v tap + 2^21) >> 22), written as planar [3, rows, Wo] bytes per image
//   qwen_resize_v_patch_kernel   vertical pass, 8-bit clip, lookup of the normalised value ([3][256], built on the host by numpy's own
//                                arithmetic and cast once to the output format), one merge block (m P x m P pixels = m^2 consecutive
//                                patch rows) per trip through LDS, written as 16-byte stores: row ((gh/m Gw/m + gw/m) m + mh) m + mw,
//                                column ((c Tp + t) P + dy) P + dx; the Tp copies of a value come from the one LDS word
// Tap counts are run-time values (no cap: 600 -> 28 pixels has 87). One translation unit for both output formats: the format is an
// argument (0 = bf16, 1 = fp32), not a second build.
#include "common.hpp"

using namespace spider;

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow: 8-bit pixels, 2 bits of headroom for the negative lobes

// One record per image, int64 [n, DESC_WORDS]; the *_OFF fields index the int32 table buffer, TMP_OFF the intermediate (bytes).
enum { D_IN_OFF = 0, D_H, D_W, D_HO, D_WO, D_XB_OFF, D_XT_OFF, D_KS_X, D_YB_OFF, D_YT_OFF, D_KS_Y, D_ROW0, D_TMP_OFF, D_Y_FIRST, D_Y_COUNT,
       DESC_WORDS = 16 };

__device__ __forceinline__ int clip8(int acc) {      // Pillow clip8 (the caller has added the rounding half)
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// grid (pieces, images). One thread: 4 consecutive output columns of one input row, all three channels, one 32-bit store per plane.
// Only the input rows [y_first, y_first + y_count) that the vertical pass reads are computed.
__global__ __launch_bounds__(256) void qwen_resize_h_kernel(const uint8_t* __restrict__ img, const long long* __restrict__ desc,
                                                            const int* __restrict__ tabs, uint8_t* __restrict__ tmp) {
    const long long* d = desc + (size_t)blockIdx.y * DESC_WORDS;
    const int W = (int)d[D_W], Wo = (int)d[D_WO], ks = (int)d[D_KS_X], y_first = (int)d[D_Y_FIRST], rows = (int)d[D_Y_COUNT];
    const int* bounds = tabs + d[D_XB_OFF];
    const int* taps = tabs + d[D_XT_OFF];
    const uint8_t* src = img + d[D_IN_OFF];
    uint8_t* dst = tmp + d[D_TMP_OFF];
    const int W4 = Wo >> 2;
    const uint32_t total = (uint32_t)rows * (uint32_t)W4;               // the host checks max_h_items < 2^31: 32-bit divisions
    const size_t plane = (size_t)rows * Wo;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const int j4 = (int)(i % (uint32_t)W4);
        const size_t r = i / (uint32_t)W4;
        const uint8_t* row = src + ((size_t)(y_first + r) * W) * 3;
        uint32_t o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j4 * 4 + e;
            const int x0 = bounds[2 * j], n = min(bounds[2 * j + 1], ks);
            const int* k = taps + (size_t)j * ks;
            int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
            for (int t = 0; t < n; ++t) {
                const uint8_t* p = row + (size_t)min(max(x0 + t, 0), W - 1) * 3;
                const int w = k[t];
                a0 += (int)p[0] * w; a1 += (int)p[1] * w; a2 += (int)p[2] * w;
            }
            o0 |= (uint32_t)clip8(a0) << (8 * e); o1 |= (uint32_t)clip8(a1) << (8 * e); o2 |= (uint32_t)clip8(a2) << (8 * e);
        }
        uint32_t* q = reinterpret_cast<uint32_t*>(dst + r * Wo + (size_t)j4 * 4);      // Wo and every plane are multiples of 4 bytes
        q[0] = o0;
        *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(q) + plane) = o1;
        *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(q) + 2 * plane) = o2;
    }
}

// grid (blocks, images); a block walks the merge blocks (tiles of S x S pixels, S = m P) of its image. Per tile:
//   1. a thread takes 4 consecutive pixels of one tile row and channel (one 32-bit load per tap from the intermediate), clips, looks the
//      output word up and files it in LDS under [patch mh m + mw][c][dy P + dx];
//   2. the tile's m^2 patch rows are one contiguous piece of the output: the block writes it as consecutive 16-byte stores, each built
//      from LDS words (column k of a row: channel k / (Tp P^2), pixel (k % (Tp P^2)) % P^2, so the Tp copies read the same word).
// ELEM = bytes per output element (2: bf16, 4: fp32). P^2 and S are multiples of 4, so 4 consecutive columns are 4 consecutive LDS words.
// CP / CM / CT: patch, merge and temporal patch size as compile-time constants (Qwen2.5-Omni's 14 / 2 / 2: the index arithmetic below is
// some twenty divisions per item, which cost more than everything else when the divisors are run-time values), or 0 = the arguments.
template <int ELEM, int CP, int CM, int CT>
__global__ __launch_bounds__(256) void qwen_resize_v_patch_kernel(const uint8_t* __restrict__ tmp, const long long* __restrict__ desc,
                                                                  const int* __restrict__ tabs, const uint32_t* __restrict__ lut,
                                                                  uint8_t* __restrict__ out, int P_, int m_, int Tp_) {
    const int P = CP ? CP : P_, m = CM ? CM : m_, Tp = CT ? CT : Tp_;
    extern __shared__ __align__(16) uint8_t smem[];
    uint32_t* slut = reinterpret_cast<uint32_t*>(smem);                 // [3][256] output words (bf16 in the low half)
    uint8_t* tile = smem + 3 * 256 * 4;                                 // [m^2][3][P^2] elements
    for (int i = threadIdx.x; i < 3 * 256; i += 256) slut[i] = lut[i];

    const long long* d = desc + (size_t)blockIdx.y * DESC_WORDS;
    const int Ho = (int)d[D_HO], Wo = (int)d[D_WO], ks = (int)d[D_KS_Y], y_first = (int)d[D_Y_FIRST], rows = (int)d[D_Y_COUNT];
    const int* bounds = tabs + d[D_YB_OFF];
    const int* taps = tabs + d[D_YT_OFF];
    const uint8_t* src = tmp + d[D_TMP_OFF];
    const int S = m * P, PP = P * P, S4 = S >> 2;
    const int tiles_w = Wo / S, n_tiles = (Ho / S) * tiles_w;
    const int quads_c = S * S4, quads = 3 * quads_c;                    // 4-pixel pieces per channel / per tile
    const int K = 3 * Tp * PP;                                          // columns of a patch row
    constexpr int EPC = 16 / ELEM;                                      // elements per 16-byte store
    const int chunks_row = K / EPC, chunks = m * m * chunks_row;
    const size_t plane = (size_t)rows * Wo;
    __syncthreads();

    for (int tI = blockIdx.x; tI < n_tiles; tI += gridDim.x) {
        const int Y0 = (tI / tiles_w) * S, X0 = (tI % tiles_w) * S;
        for (int q = threadIdx.x; q < quads; q += 256) {
            const int c = q / quads_c, rem = q % quads_c, ty = rem / S4, s = rem % S4;
            const int y = Y0 + ty;
            const int y0 = bounds[2 * y], n = min(bounds[2 * y + 1], ks);
            const int* k = taps + (size_t)y * ks;
            const uint8_t* col = src + c * plane + X0 + 4 * s;
            int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int t = 0; t < n; ++t) {
                const int yy = min(max(y0 + t - y_first, 0), rows - 1);
                const uint32_t v = *reinterpret_cast<const uint32_t*>(col + (size_t)yy * Wo);
                const int w = k[t];
                a0 += (int)(v & 0xffu) * w; a1 += (int)((v >> 8) & 0xffu) * w; a2 += (int)((v >> 16) & 0xffu) * w; a3 += (int)(v >> 24) * w;
            }
            const int a[4] = {a0, a1, a2, a3};
            const int mh = ty / P, dy = ty % P;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int x = 4 * s + e, mw = x / P, dx = x % P;
                const uint32_t word = slut[c * 256 + clip8(a[e])];
                const int at = ((mh * m + mw) * 3 + c) * PP + dy * P + dx;
                if (ELEM == 2) reinterpret_cast<uint16_t*>(tile)[at] = (uint16_t)word;
                else reinterpret_cast<uint32_t*>(tile)[at] = word;
            }
        }
        __syncthreads();
        uint8_t* dst = out + ((size_t)d[D_ROW0] + (size_t)tI * m * m) * K * ELEM;
        for (int ch = threadIdx.x; ch < chunks; ch += 256) {
            const int mp = ch / chunks_row, k0 = (ch % chunks_row) * EPC;
            u32x4 o;
            if (ELEM == 2) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int kk = k0 + 4 * h, c = kk / (Tp * PP), pix = (kk % (Tp * PP)) % PP;
                    const u32x2 w = *reinterpret_cast<const u32x2*>(tile + (size_t)((mp * 3 + c) * PP + pix) * 2);
                    o[2 * h] = w[0]; o[2 * h + 1] = w[1];
                }
            } else {
                const int c = k0 / (Tp * PP), pix = (k0 % (Tp * PP)) % PP;
                o = *reinterpret_cast<const u32x4*>(tile + (size_t)((mp * 3 + c) * PP + pix) * 4);
            }
            *reinterpret_cast<u32x4*>(dst + (size_t)ch * 16) = o;
        }
        __syncthreads();
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int spider_qwen_image_patches(const void* images, const long long* desc, const int* tabs, const void* lut, void* tmp, void* rows,
                              int n_images, int patch, int merge, int temporal, long max_h_items, int max_tiles, int f32, void* stream) {
    SPIDER_CHECK(images && desc && tabs && lut && tmp && rows, "qwen_image_patches: null pointer");
    SPIDER_CHECK(n_images > 0 && n_images <= 65535, "qwen_image_patches: 1 to 65535 images per call");
    SPIDER_CHECK(patch > 0 && merge > 0 && temporal > 0 && patch <= 64 && merge <= 8 && temporal <= 8, "qwen_image_patches: patch <= 64, merge <= 8, temporal_patch <= 8");
    SPIDER_CHECK((patch * patch) % 4 == 0 && (patch * merge) % 4 == 0, "qwen_image_patches: patch^2 and patch * merge must be multiples of 4");
    SPIDER_CHECK(f32 == 0 || f32 == 1, "qwen_image_patches: format must be 0 (bf16) or 1 (fp32)");
    const int elem = f32 ? 4 : 2;
    SPIDER_CHECK((3 * temporal * patch * patch * elem) % 16 == 0, "qwen_image_patches: a patch row must be a multiple of 16 bytes");
    SPIDER_CHECK(aligned16(rows) && ((uintptr_t)tmp & 3) == 0, "qwen_image_patches: rows must be 16-byte aligned, tmp 4-byte aligned");
    SPIDER_CHECK(max_h_items > 0 && max_tiles > 0, "qwen_image_patches: empty grid");
    SPIDER_CHECK(max_h_items <= 0x7fffffffL, "qwen_image_patches: image too large (rows * Wo / 4 must stay below 2^31)");
    const int lds = 3 * 256 * 4 + merge * merge * 3 * patch * patch * elem;
    SPIDER_CHECK(lds <= 64 * 1024, "qwen_image_patches: merge block too large for LDS");
    constexpr long MAX_BLOCKS = 2048;      // 8 blocks of 256 threads on each of the 256 CUs; the kernels grid-stride beyond
    const long hb = (max_h_items + 255) / 256;
    qwen_resize_h_kernel<<<dim3((unsigned)(hb > MAX_BLOCKS ? MAX_BLOCKS : hb), n_images), 256, 0, (hipStream_t)stream>>>(
        (const uint8_t*)images, desc, tabs, (uint8_t*)tmp);
    SPIDER_LAUNCH_OK();
    const dim3 grid((unsigned)(max_tiles > MAX_BLOCKS ? MAX_BLOCKS : max_tiles), n_images);
    const bool omni = patch == 14 && merge == 2 && temporal == 2;
#define SPIDER_QWEN_V(ELEM, CP, CM, CT)                                                                                                      \
    qwen_resize_v_patch_kernel<ELEM, CP, CM, CT><<<grid, 256, lds, (hipStream_t)stream>>>((const uint8_t*)tmp, desc, tabs, (const uint32_t*)lut, \
                                                                                          (uint8_t*)rows, patch, merge, temporal)
    if (f32) {
        if (omni) SPIDER_QWEN_V(4, 14, 2, 2); else SPIDER_QWEN_V(4, 0, 0, 0);
    } else {
        if (omni) SPIDER_QWEN_V(2, 14, 2, 2); else SPIDER_QWEN_V(2, 0, 0, 0);
    }
#undef SPIDER_QWEN_V
    SPIDER_LAUNCH_OK();
    return 0;
}

}  // extern "C"

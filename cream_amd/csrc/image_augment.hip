// image_augment.hip — RandAugment of the training recipe on the device: per-image chains of op descriptors (struct cream_aug_op) on a
// batch of uint8 RGB images of one size.
//
// Reference: `--aa rand-m9-mstd0.5-inc1` (AutoFormer/supernet_train.py:111) -> timm 0.3.2's RandAugment inside create_transform,
// between RandomHorizontalFlip and ToTensor (lib/datasets.py:189-202).  The host draws every image's ops (autoformer/data.py:
// rand_augment_params); each op is Pillow's operation on a uint8 RGB image, restated here integer for integer:
//   LUT ops      ImageOps.autocontrast (cutoff 0) / equalize (per-channel histograms of the whole image -> 256-entry LUTs),
//                invert, posterize, solarize, timm's solarize_add
//   blend ops    ImageEnhance.Color / Contrast / Brightness / Sharpness = Image.blend(degenerate, image, (float)factor) of
//                libImaging/Blend.c (float32, clipped, truncated); the degenerates: the grey level of libImaging/Convert.c, its
//                mean over the image (ImageStat, in doubles), 0, ImageFilter.SMOOTH (border copied, interior (acc + 6) / 13)
//   affine       Image.transform(size, AFFINE, m, BICUBIC, fillcolor) of libImaging/Geometry.c: the input point of an output
//                pixel centre in doubles, fill outside [0, W) x [0, H), else a 4 x 4 cubic (a = -0.5) along x per row, then
//                along y, in Geometry.c's order of IEEE double operations (this library is built with -ffp-contract=off)
// Byte-exact against a numpy restatement that is pinned against Pillow (tests/test_randaugment_*.py).
//
// One launch per op layer for the whole batch: grid (row tiles of AUG_ROWS rows, B), 256 threads; a workgroup reads its image's op
// once (the branch is per workgroup, never per lane).  The ops that need the whole image (the two histograms, Contrast's mean)
// compute it in every workgroup of that image from the layer's input (L2-resident: 200 KB at 224 x 224), so a layer is one launch
// with no hand-off between workgroups.  Between layers the images are RGBX words (R | G << 8 | B << 16, one aligned load per tap
// of the affine op); the first layer of cream_image_augment_u8 reads and its last layer writes packed HWC bytes, the last layer of
// cream_image_batch_transform_aug ends in the float tail of image_transform.hip (store_normalized4).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "cream_amd.h"
#include "image_common.hpp"

namespace {
constexpr int AUG_ROWS = 16;                        // output rows per workgroup
constexpr int AUG_THREADS = 256;
constexpr int HIST_UNROLL = 8;                      // whole-image passes: pixels per thread and step
constexpr int AUG_MAX_W = 1024;
constexpr int AUG_MAX_H = 4096;                     // whole-image counts and sums stay in int32

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
enum { SRC_RGBX = 0, SRC_HWC = 1 };
enum { DST_RGBX = 0, DST_HWC = 1, DST_TAIL = 2 };

struct Layer {
    const void* src;
    void* dst;
    const cream_aug_op* ops;
    float* out;                                     // DST_TAIL: (B, 3, H, W) fp32
    const cream_image_desc* descs;                  // DST_TAIL: the RandomErasing boxes
    float mean[3], sd[3];
    int n_ops, layer, H, W, src_mode, dst_mode;
};

__device__ __forceinline__ uint32_t load_px(const Layer& a, int64_t i) {
    if (a.src_mode == SRC_HWC) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(a.src) + 3 * i;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    return reinterpret_cast<const uint32_t*>(a.src)[i];
}
__device__ __forceinline__ int ch(uint32_t p, int c) { return (int)((p >> (8 * c)) & 255u); }
__device__ __forceinline__ uint32_t pack(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }

// libImaging/Convert.c rgb2l
__device__ __forceinline__ int grey(uint32_t p) { return (19595 * ch(p, 0) + 38470 * ch(p, 1) + 7471 * ch(p, 2) + 0x8000) >> 16; }

// libImaging/Blend.c: in1 + alpha * (in2 - in1) in float32, 0 / 255 at the ends, truncated between (for 0 <= alpha <= 1 the clip
// never acts: the same bytes as Blend.c's unclipped branch)
__device__ __forceinline__ int blend(int deg, int v, float f) {
    const float t = (float)deg + f * (float)(v - deg);
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// libImaging/Geometry.c BICUBIC: integer taps (the x pass: p2..p4 exact integers) and double taps (the y pass)
__device__ __forceinline__ double cubic_i(int v1, int v2, int v3, int v4, double d) {
    const double p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}
__device__ __forceinline__ double cubic_d(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}
__device__ __forceinline__ int clip_d(double v) { return v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (int)v); }

__device__ uint32_t affine_px(const Layer& a, int64_t base, int x, int y, const cream_aug_op& op) {
    const int W = a.W, H = a.H;
    const double xo = x + 0.5, yo = y + 0.5;
    double xin = op.m[0] * xo + op.m[1] * yo + op.m[2];
    double yin = op.m[3] * xo + op.m[4] * yo + op.m[5];
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return op.fill & 0xFFFFFFu;     // (NaN: outside)
    xin -= 0.5;
    yin -= 0.5;
    const int xi = (int)floor(xin), yi = (int)floor(yin);
    const double dx = xin - xi, dy = yin - yi;
    int cols[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cols[k] = min(max(xi - 1 + k, 0), W - 1);
    // rows outside the image: Geometry.c clamps the first and repeats the previous row's value for the other three, which is the
    // clamped row again (the first tap row is >= -2, so only y - 1 + 1 = -1 can lie above the image)
    double v[4][3];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t row = base + (int64_t)min(max(yi - 1 + r, 0), H - 1) * W;
        const uint32_t p0 = load_px(a, row + cols[0]), p1 = load_px(a, row + cols[1]), p2 = load_px(a, row + cols[2]),
                       p3 = load_px(a, row + cols[3]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[r][c] = cubic_i(ch(p0, c), ch(p1, c), ch(p2, c), ch(p3, c), dx);
    }
    int o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = clip_d(cubic_d(v[0][c], v[1][c], v[2][c], v[3][c], dy));
    return pack(o[0], o[1], o[2]);
}

// exclusive prefix sum over the 256 threads of the workgroup (4 waves of 64)
__device__ int block_exclusive_scan(int v, int* wave_tot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) wave_tot[w] = x;
    __syncthreads();
    int add = 0;
    for (int i = 0; i < w; ++i) add += wave_tot[i];
    __syncthreads();
    return x + add - v;
}

__global__ __launch_bounds__(AUG_THREADS) void image_augment_kernel(Layer a)
{
    __shared__ int hist[768];                       // per-channel histograms of the layer's input image
    __shared__ int lut[768];                        // AutoContrast / Equalize
    __shared__ int misc[16];                        // lo[3], hi[3], distinct[3]; scan scratch
    __shared__ unsigned long long grey_sum;
    const int b = blockIdx.y, H = a.H, W = a.W, tid = threadIdx.x;
    const cream_aug_op op = a.ops[(int64_t)b * a.n_ops + a.layer];
    const int kind = op.kind;
    const int64_t base = (int64_t)b * H * W, npx = (int64_t)H * W;
    int degen = 0;                                  // Contrast: the grey mean
    if (kind == CREAM_AUG_AUTOCONTRAST || kind == CREAM_AUG_EQUALIZE) {
        for (int i = tid; i < 768; i += AUG_THREADS) hist[i] = 0;
        if (tid < 3) { misc[tid] = 256; misc[3 + tid] = -1; misc[6 + tid] = 0; }
        __syncthreads();
        for (int64_t i0 = tid; i0 < npx; i0 += HIST_UNROLL * AUG_THREADS) {     // the loads of a step in flight together
            uint32_t p[HIST_UNROLL];
#pragma unroll
            for (int u = 0; u < HIST_UNROLL; ++u) p[u] = i0 + u * AUG_THREADS < npx ? load_px(a, base + i0 + u * AUG_THREADS) : 0u;
#pragma unroll
            for (int u = 0; u < HIST_UNROLL; ++u)
                if (i0 + u * AUG_THREADS < npx) {
                    atomicAdd(&hist[ch(p[u], 0)], 1);
                    atomicAdd(&hist[256 + ch(p[u], 1)], 1);
                    atomicAdd(&hist[512 + ch(p[u], 2)], 1);
                }
        }
        __syncthreads();
        for (int c = 0; c < 3; ++c)                 // thread tid = bin tid
            if (hist[c * 256 + tid] > 0) {
                atomicMin(&misc[c], tid);
                atomicMax(&misc[3 + c], tid);
                atomicAdd(&misc[6 + c], 1);
            }
        __syncthreads();
        for (int c = 0; c < 3; ++c) {
            const int lo = misc[c], hi = misc[3 + c];
            int l = tid;
            if (kind == CREAM_AUG_AUTOCONTRAST) {
                if (hi > lo) {                       // ImageOps.autocontrast: int(ix * scale + offset), clipped
                    const double scale = 255.0 / (double)(hi - lo);
                    const double offset = (double)(-lo) * scale;
                    l = (int)((double)tid * scale + offset);
                    l = l < 0 ? 0 : (l > 255 ? 255 : l);
                }
            } else {                                 // ImageOps.equalize: step from the histogram without its last bin
                const int h = hist[c * 256 + tid];
                const int before = block_exclusive_scan(h, misc + 10);
                const int step = ((int)npx - hist[c * 256 + hi]) / 255;
                if (misc[6 + c] > 1 && step != 0) l = min(255, (step / 2 + before) / step);
            }
            lut[c * 256 + tid] = l;
        }
        __syncthreads();
    } else if (kind == CREAM_AUG_CONTRAST) {         // int(sum(L) / (W H) + 0.5), the division in double (ImageStat)
        if (tid == 0) grey_sum = 0;
        __syncthreads();
        unsigned long long s = 0;
        for (int64_t i0 = tid; i0 < npx; i0 += HIST_UNROLL * AUG_THREADS) {
            uint32_t p[HIST_UNROLL];
#pragma unroll
            for (int u = 0; u < HIST_UNROLL; ++u) p[u] = i0 + u * AUG_THREADS < npx ? load_px(a, base + i0 + u * AUG_THREADS) : 0u;
#pragma unroll
            for (int u = 0; u < HIST_UNROLL; ++u) s += (unsigned)grey(p[u]);             // (grey(0) == 0)
        }
        atomicAdd(&grey_sum, s);
        __syncthreads();
        degen = (int)((double)grey_sum / (double)npx + 0.5);
    }

    const int y0 = blockIdx.x * AUG_ROWS, y1 = min(H, y0 + AUG_ROWS);
    const int gpr = (W + 3) >> 2;                   // groups of 4 pixels per row
    const float f = op.factor;
    for (int it = tid; it < (y1 - y0) * gpr; it += AUG_THREADS) {
        const int y = y0 + it / gpr, x0 = (it % gpr) * 4;
        uint32_t pin[4];                                         // the group's own pixels, loaded together
        if (a.src_mode == SRC_RGBX && (W & 3) == 0) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint32_t*>(a.src) + base + (int64_t)y * W + x0);
#pragma unroll
            for (int px = 0; px < 4; ++px) pin[px] = v[px];
        } else {
#pragma unroll
            for (int px = 0; px < 4; ++px) pin[px] = x0 + px < W ? load_px(a, base + (int64_t)y * W + x0 + px) : 0u;
        }
        int u8[12];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            const int x = x0 + px;
            uint32_t q = 0;
            if (x < W) {
                const uint32_t p = pin[px];
                int r = ch(p, 0), g = ch(p, 1), bl = ch(p, 2);
                switch (kind) {
                case CREAM_AUG_AUTOCONTRAST:
                case CREAM_AUG_EQUALIZE: r = lut[r]; g = lut[256 + g]; bl = lut[512 + bl]; break;
                case CREAM_AUG_INVERT: r = 255 - r; g = 255 - g; bl = 255 - bl; break;
                case CREAM_AUG_POSTERIZE: {
                    const int mask = ~((1 << (8 - op.arg)) - 1) & 255;
                    r &= mask; g &= mask; bl &= mask;
                    break;
                }
                case CREAM_AUG_SOLARIZE:
                    r = r < op.arg ? r : 255 - r; g = g < op.arg ? g : 255 - g; bl = bl < op.arg ? bl : 255 - bl;
                    break;
                case CREAM_AUG_SOLARIZE_ADD:
                    r = r < 128 ? min(255, r + op.arg) : r; g = g < 128 ? min(255, g + op.arg) : g;
                    bl = bl < 128 ? min(255, bl + op.arg) : bl;
                    break;
                case CREAM_AUG_COLOR: {
                    const int l = grey(p);
                    r = blend(l, r, f); g = blend(l, g, f); bl = blend(l, bl, f);
                    break;
                }
                case CREAM_AUG_CONTRAST: r = blend(degen, r, f); g = blend(degen, g, f); bl = blend(degen, bl, f); break;
                case CREAM_AUG_BRIGHTNESS: r = blend(0, r, f); g = blend(0, g, f); bl = blend(0, bl, f); break;
                case CREAM_AUG_SHARPNESS: {
                    int s[3] = {r, g, bl};                       // ImageFilter.SMOOTH: the border is copied
                    if (x > 0 && y > 0 && x < W - 1 && y < H - 1) {
                        int acc[3] = {4 * r, 4 * g, 4 * bl};
                        for (int dy = -1; dy <= 1; ++dy)
                            for (int dx = -1; dx <= 1; ++dx) {
                                const uint32_t n = load_px(a, base + (int64_t)(y + dy) * W + x + dx);
                                acc[0] += ch(n, 0); acc[1] += ch(n, 1); acc[2] += ch(n, 2);
                            }
                        for (int c = 0; c < 3; ++c) s[c] = (acc[c] + 6) / 13;
                    }
                    r = blend(s[0], r, f); g = blend(s[1], g, f); bl = blend(s[2], bl, f);
                    break;
                }
                case CREAM_AUG_AFFINE: {
                    const uint32_t o = affine_px(a, base, x, y, op);
                    r = ch(o, 0); g = ch(o, 1); bl = ch(o, 2);
                    break;
                }
                default: break;                                  // CREAM_AUG_NONE
                }
                q = pack(r, g, bl);
                u8[3 * px] = r; u8[3 * px + 1] = g; u8[3 * px + 2] = bl;
            } else {
                u8[3 * px] = u8[3 * px + 1] = u8[3 * px + 2] = 0;
            }
            if (x < W) {
                if (a.dst_mode == DST_RGBX) {
                    reinterpret_cast<uint32_t*>(a.dst)[base + (int64_t)y * W + x] = q;
                } else if (a.dst_mode == DST_HWC) {
                    uint8_t* o = reinterpret_cast<uint8_t*>(a.dst) + 3 * (base + (int64_t)y * W + x);
                    o[0] = (uint8_t)u8[3 * px]; o[1] = (uint8_t)u8[3 * px + 1]; o[2] = (uint8_t)u8[3 * px + 2];
                }
            }
        }
        if (a.dst_mode == DST_TAIL)                                  // W % 4 == 0 here: four whole pixels
            cream_image::store_normalized4(a.out + (int64_t)b * 3 * npx + (int64_t)y * W, npx, x0, y, false, u8, a.mean, a.sd,
                                           a.descs[b]);
    }
}

int launch_layers(Layer a, const void* src, int src_mode, void* dst, int dst_mode, void* buf0, void* buf1, int n, int B,
                  hipStream_t st)
{
    const dim3 grid((a.H + AUG_ROWS - 1) / AUG_ROWS, B);
    for (int k = 0; k < n; ++k) {
        a.layer = k;
        a.src = k == 0 ? src : (k % 2 == 1 ? buf0 : buf1);
        a.src_mode = k == 0 ? src_mode : SRC_RGBX;
        a.dst = k == n - 1 ? dst : (k % 2 == 0 ? buf0 : buf1);
        a.dst_mode = k == n - 1 ? dst_mode : DST_RGBX;
        hipLaunchKernelGGL(image_augment_kernel, grid, dim3(AUG_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) return CREAM_ERR_LAUNCH;
    }
    return CREAM_OK;
}

int64_t image_bytes(int B, int H, int W) { return ((int64_t)B * H * W * 4 + 15) & ~(int64_t)15; }
}  // namespace

namespace cream_image {
int check_aug_ops(const cream_aug_op* ops, int64_t count) {
    for (int64_t i = 0; i < count; ++i) {
        const cream_aug_op& o = ops[i];
        if (o.kind < CREAM_AUG_NONE || o.kind > CREAM_AUG_AFFINE) return CREAM_ERR_BAD_ARG;
        if (o.kind == CREAM_AUG_POSTERIZE && (o.arg < 0 || o.arg > 8)) return CREAM_ERR_BAD_ARG;
        if (o.kind == CREAM_AUG_SOLARIZE && (o.arg < 0 || o.arg > 256)) return CREAM_ERR_BAD_ARG;
        if (o.kind == CREAM_AUG_SOLARIZE_ADD && (o.arg < 0 || o.arg > 255)) return CREAM_ERR_BAD_ARG;
        if (!isfinite(o.factor)) return CREAM_ERR_BAD_ARG;
        for (int j = 0; j < 6; ++j)
            if (!isfinite(o.m[j])) return CREAM_ERR_BAD_ARG;
    }
    return CREAM_OK;
}

int launch_aug_tail(float* out, uint32_t* img, uint32_t* img2, const cream_aug_op* ops_dev, int ops_per_image, int B, int H, int W,
                    const cream_image_desc* descs_dev, const float* mean, const float* stdev, hipStream_t st) {
    Layer a{};
    a.ops = ops_dev;
    a.out = out;
    a.descs = descs_dev;
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.sd[c] = stdev[c]; }
    a.n_ops = ops_per_image;
    a.H = H;
    a.W = W;
    // layer k reads img (k even) / img2 (k odd); the last one writes the float tail
    return launch_layers(a, img, SRC_RGBX, nullptr, DST_TAIL, img2, img, ops_per_image, B, st);
}
}  // namespace cream_image

extern "C" int64_t cream_image_augment_workspace(int B, int H, int W, int ops_per_image)
{
    if (B < 0 || H <= 0 || W <= 0 || W > AUG_MAX_W || H > AUG_MAX_H || ops_per_image < 0 || ops_per_image > CREAM_AUG_MAX_OPS)
        return CREAM_ERR_BAD_ARG;
    return (ops_per_image <= 1 ? 0 : ops_per_image == 2 ? 1 : 2) * image_bytes(B, H, W);
}

extern "C" int cream_image_augment_u8(uint8_t* dst, const uint8_t* src, int B, int H, int W, const cream_aug_op* ops,
                                      const cream_aug_op* ops_dev, int ops_per_image, void* workspace, int64_t workspace_bytes,
                                      void* stream)
{
    const int64_t need = cream_image_augment_workspace(B, H, W, ops_per_image);
    if (need < 0) return (int)need;
    if (B == 0 || ops_per_image == 0) return CREAM_OK;
    if (!dst || !src || !ops || !ops_dev || dst == src || ((uintptr_t)ops_dev) % 8) return CREAM_ERR_BAD_ARG;
    if (need > 0 && (!workspace || workspace_bytes < need || ((uintptr_t)workspace) % 16)) return CREAM_ERR_BAD_ARG;
    const int rc = cream_image::check_aug_ops(ops, (int64_t)B * ops_per_image);
    if (rc != CREAM_OK) return rc;
    Layer a{};
    a.ops = ops_dev;
    a.n_ops = ops_per_image;
    a.H = H;
    a.W = W;
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    void* buf0 = ops_per_image >= 2 ? ws : nullptr;
    void* buf1 = ops_per_image >= 3 ? ws + image_bytes(B, H, W) : nullptr;
    return launch_layers(a, src, SRC_HWC, dst, DST_HWC, buf0, buf1, ops_per_image, B, (hipStream_t)stream);
}

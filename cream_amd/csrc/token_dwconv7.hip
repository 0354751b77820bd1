// token_dwconv7.hip — depthwise 7 x 7 convolution (stride 1, zero padding 3) on the TOKEN layout (B, Hs*Ws, C), with an optional
// fused residual r in {0, 1}.
//
// Mini-Swin with is_transform_FFN runs LayerNorm -> x + depthwise 7 x 7 Conv2d(x) between the attention and the MLP of every
// block repeat (MiniViT/Mini-Swin/models/swin_transformer_minivit.py:273-281, :328-332) and transposes the token stream to NCHW
// and back for it.  The 3 x 3 kernels of token_dwconv.hip keep all taps of 8 channels in registers and fetch every neighbour
// from L1 / L2; with 49 taps that spills, so this file stages tiles in LDS instead.
//
//     y[b, i, j, c]   = bias[c] + sum_{di, dj < 7} w[c, di, dj] x[b, i + di - 3, j + dj - 3, c]     (+ x[b, i, j, c] if r)
//     dx[b, i, j, c]  = sum_{di, dj} w[c, di, dj] dy[b, i - di + 3, j - dj + 3, c]                  (+ dy[b, i, j, c] if r)
//     dw[c, di, dj]   = sum_{b, i, j} dy[b, i, j, c] x[b, i + di - 3, j + dj - 3, c],   dbias[c] = sum dy[b, i, j, c]
//
// Work item: one tile of up to 14 x 14 tokens of one image times a chunk of 32 channels.  The 256 threads stage the tile plus a
// 3-token halo (up to 20 x 20 positions x 32 channels, fp32, 51 200 B; zeros outside the map) in LDS with 16-byte accesses along
// C.  Then thread = (channel = tid % 32, group = tid / 32): a lane owns ONE channel and keeps its 49 taps in registers, so the 32
// lanes of a half-wave read 32 consecutive LDS banks.  The 8 groups share the tile's strips: a strip is 7 horizontally adjacent
// outputs of one row; for each of the 7 tap rows the thread reads the 13 inputs under the strip once and uses each for up to 7
// outputs (91 LDS reads for 343 products).  The gradient launch stages dy's tile (25 088 B more) next to x's and walks the same
// strips with 49 + 1 accumulators in place of the taps.
//
// Arithmetic: fp32 throughout, products and additions separate (-ffp-contract=off).  I/O is bf16 (round to nearest even on the
// store) or fp32.  The order is fixed:
//     y, dx   the bias (y) or nothing (dx), then the 49 products in row-major order of the INPUT offset (di - 3, dj - 3) — for
//             dx that is tap (6 - di, 6 - dj) at offset (di - 3, dj - 3) — then the residual.  An out-of-map tap multiplies a
//             staged zero: it adds +-0.
//     dbias   per thread: its strips in ascending order (tiles ascending, strips ascending within a tile, left to right within
//             a strip); then the 8 groups of the workgroup in ascending order through LDS; then the caller's sum of partials.
//     dw      per thread and tap: the same chain of its strips, one product per output of the strip, left to right; then
//             groups and partials as for dbias.  Positions of a strip beyond the tile hold dy = 0 and add +-0.
// No atomics: one partial [dw (C, 49) | dbias (C)] per blockIdx.x of the gradient launch, every entry written exactly once (by
// the workgroup whose blockIdx.y owns the channel).
//
// Launch shape: grid (X, ceil(C / 32)).  blockIdx.y is the channel chunk — fixed for a workgroup, so taps and gradient
// accumulators stay in registers across tiles — and blockIdx.x strides over the B * ceil(Hs / 14) * ceil(Ws / 14) tiles, with
// X = min(tiles, 2 cu_count() / chunks): persistent, two workgroups per CU (2 x 76 288 B of LDS in the gradient launch).  Maps
// smaller than a tile stage and walk only what they have (a 7 x 7 map is 7 strips, one per group), and their many channel chunks
// and images fill the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cream_amd.h"
#include "cu_budget.hpp"

namespace {

using cream::cu_count;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 hwbf16x2 __attribute__((ext_vector_type(2)));

constexpr int THREADS = 256, CCH = 32, GROUPS = THREADS / CCH;      // channels per chunk, strip groups per workgroup
constexpr int K = 7, R = 3, T = K * K;
constexpr int TILE = 14, STRIP = 7;                                  // outputs per tile edge, outputs per strip
constexpr int SW = TILE + 2 * R;                                     // staged positions per tile edge, halo included
constexpr int XS_FLOATS = SW * SW * CCH, DY_FLOATS = TILE * TILE * CCH;
constexpr int PER_CU = 2;
static_assert(TILE % STRIP == 0 && GROUPS * (T + 1) * CCH <= XS_FLOATS, "the partial reduction reuses the x tile");

struct Args {
    const void* x;        // what the stencil reads (x in the forward, dy for dx) / the x of the gradient launch
    const void* dy;       // gradient launch only
    const float* w;       // (C, 49)
    const float* bias;    // (C) or nullptr
    void* y;              // what the stencil writes
    float* part;          // (gridDim.x, 50 C)
    int B, Hs, Ws, C, nti, ntj, tiles, flip, residual;
};

struct Tile { int b, i0, j0, th, tw, ncb; };          // image, origin, extent, strips per row

__device__ __forceinline__ Tile tile_of(const Args& a, int t) {
    Tile s;
    const int tj = t % a.ntj, rest = t / a.ntj, ti = rest % a.nti;
    s.b = rest / a.nti;
    s.i0 = ti * TILE; s.j0 = tj * TILE;
    s.th = min(TILE, a.Hs - s.i0); s.tw = min(TILE, a.Ws - s.j0);
    s.ncb = (s.tw + STRIP - 1) / STRIP;
    return s;
}

// Stages rows x cols positions, position (r, q) = map token (i0 + r, j0 + q) of image b, channels c0 .. c0 + 31, as fp32 at
// lds[(r * ldw + q) * 32 + channel]; zeros where the token is outside [0, ilim) x [jlo, jlim) or the channel is past C.
// 8 threads per position, 4 channels each.  Every load is from a clamped, valid address, so none is conditional.
template <bool BF16> __device__ __forceinline__ void stage(float* lds, int ldw, const void* src, const Args& a, int b, int i0, int j0,
                                                           int rows, int cols, int ilim, int jlim, int c0) {
    const int k = threadIdx.x & 7, ch = c0 + 4 * k;
    const bool ch_ok = ch < a.C;
    const int chc = ch_ok ? ch : c0;
    const int n = rows * cols;
#pragma unroll 4
    for (int p = threadIdx.x >> 3; p < n; p += THREADS / 8) {
        const int r = p / cols, q = p - r * cols, i = i0 + r, j = j0 + q;
        const bool ok = ch_ok && i >= 0 && i < ilim && j >= 0 && j < jlim;
        const int ic = min(max(i, 0), a.Hs - 1), jc = min(max(j, 0), a.Ws - 1);
        const int64_t off = (((int64_t)b * a.Hs + ic) * a.Ws + jc) * a.C + chc;
        f32x4 v;
        if constexpr (BF16) {
            const u32x2 u = *(const u32x2*)((const uint16_t*)src + off);
            v = f32x4{__uint_as_float(u[0] << 16), __uint_as_float(u[0] & 0xffff0000u), __uint_as_float(u[1] << 16),
                      __uint_as_float(u[1] & 0xffff0000u)};
        } else {
            v = *(const f32x4*)((const float*)src + off);
        }
        *(f32x4*)(lds + (r * ldw + q) * CCH + 4 * k) = ok ? v : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

template <bool BF16> __device__ __forceinline__ void store_one(void* base, int64_t off, float v) {
    if constexpr (BF16)                                 // round to nearest even (v_cvt_pk_bf16_f32)
        ((uint16_t*)base)[off] = (uint16_t)__builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2{v, 0.0f}), hwbf16x2));
    else
        ((float*)base)[off] = v;
}

// y = bias + stencil(x) (+ x) with the taps as they are (flip == 0) or reversed (flip != 0: dx from dy)
template <bool BF16> __global__ __launch_bounds__(THREADS) void token_dwconv7_stencil_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds7[];
    float* xs = lds7;
    const int c = threadIdx.x % CCH, g = threadIdx.x / CCH, c0 = blockIdx.y * CCH;
    const bool ch_ok = c0 + c < a.C;

    float tap[T];
#pragma unroll
    for (int t = 0; t < T; ++t) tap[t] = ch_ok ? a.w[(int64_t)(c0 + c) * T + (a.flip ? T - 1 - t : t)] : 0.0f;
    const float bv = (ch_ok && a.bias) ? a.bias[c0 + c] : 0.0f;

    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const Tile s = tile_of(a, t);
        __syncthreads();                                // the previous tile's reads are done
        stage<BF16>(xs, SW, a.x, a, s.b, s.i0 - R, s.j0 - R, s.th + 2 * R, s.ncb * STRIP + 2 * R, a.Hs, a.Ws, c0);
        __syncthreads();
        for (int u = g; u < s.th * s.ncb; u += GROUPS) {
            const int row = u / s.ncb, q0 = (u - row * s.ncb) * STRIP;
            float acc[STRIP], ctr[STRIP];
#pragma unroll
            for (int o = 0; o < STRIP; ++o) acc[o] = bv;
#pragma unroll
            for (int di = 0; di < K; ++di) {
                const float* p = xs + ((row + di) * SW + q0) * CCH + c;
                float v[STRIP + K - 1];
#pragma unroll
                for (int q = 0; q < STRIP + K - 1; ++q) v[q] = p[q * CCH];
#pragma unroll
                for (int o = 0; o < STRIP; ++o) {
#pragma unroll
                    for (int dj = 0; dj < K; ++dj) {
                        const float pr = tap[di * K + dj] * v[o + dj];
                        acc[o] = acc[o] + pr;
                    }
                }
                if (di == R) {
#pragma unroll
                    for (int o = 0; o < STRIP; ++o) ctr[o] = v[o + R];
                }
            }
            const int64_t tok = ((int64_t)s.b * a.Hs + s.i0 + row) * a.Ws + s.j0 + q0;
#pragma unroll
            for (int o = 0; o < STRIP; ++o) {
                if (ch_ok && q0 + o < s.tw) store_one<BF16>(a.y, (tok + o) * a.C + c0 + c, a.residual ? acc[o] + ctr[o] : acc[o]);
            }
        }
    }
}

// one partial [dw (C, 49) | dbias (C)] per blockIdx.x
template <bool BF16> __global__ __launch_bounds__(THREADS) void token_dwconv7_wgrad_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds7[];
    float* xs = lds7;
    float* gs = lds7 + XS_FLOATS;
    const int c = threadIdx.x % CCH, g = threadIdx.x / CCH, c0 = blockIdx.y * CCH;

    float dw[T], db = 0.0f;
#pragma unroll
    for (int t = 0; t < T; ++t) dw[t] = 0.0f;

    for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
        const Tile s = tile_of(a, t);
        __syncthreads();
        stage<BF16>(xs, SW, a.x, a, s.b, s.i0 - R, s.j0 - R, s.th + 2 * R, s.ncb * STRIP + 2 * R, a.Hs, a.Ws, c0);
        stage<BF16>(gs, TILE, a.dy, a, s.b, s.i0, s.j0, s.th, s.ncb * STRIP, a.Hs, s.j0 + s.tw, c0);      // zeros past the tile
        __syncthreads();
        for (int u = g; u < s.th * s.ncb; u += GROUPS) {
            const int row = u / s.ncb, q0 = (u - row * s.ncb) * STRIP;
            float gy[STRIP];
#pragma unroll
            for (int o = 0; o < STRIP; ++o) {
                gy[o] = gs[(row * TILE + q0 + o) * CCH + c];
                db = db + gy[o];
            }
#pragma unroll
            for (int di = 0; di < K; ++di) {
                const float* p = xs + ((row + di) * SW + q0) * CCH + c;
                float v[STRIP + K - 1];
#pragma unroll
                for (int q = 0; q < STRIP + K - 1; ++q) v[q] = p[q * CCH];
#pragma unroll
                for (int dj = 0; dj < K; ++dj) {
#pragma unroll
                    for (int o = 0; o < STRIP; ++o) {
                        const float pr = gy[o] * v[o + dj];
                        dw[di * K + dj] = dw[di * K + dj] + pr;
                    }
                }
            }
        }
    }

    // the workgroup's groups, in ascending order: red[group][tap | dbias][channel] over the x tile
    __syncthreads();
    float* red = lds7;
#pragma unroll
    for (int t = 0; t < T; ++t) red[(g * (T + 1) + t) * CCH + c] = dw[t];
    red[(g * (T + 1) + T) * CCH + c] = db;
    __syncthreads();
    float* out = a.part + (int64_t)blockIdx.x * (T + 1) * a.C;
    for (int idx = threadIdx.x; idx < (T + 1) * CCH; idx += THREADS) {
        const int cl = idx < T * CCH ? idx / T : idx - T * CCH, t = idx < T * CCH ? idx - cl * T : T;
        if (c0 + cl < a.C) {
            float sum = 0.0f;
#pragma unroll
            for (int gg = 0; gg < GROUPS; ++gg) sum = sum + red[(gg * (T + 1) + t) * CCH + cl];
            out[t < T ? (int64_t)(c0 + cl) * T + t : (int64_t)T * a.C + c0 + cl] = sum;
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_shape(const cream_token_dwconv7_desc* d) {
    if (!d) return CREAM_ERR_BAD_ARG;
    if (d->B < 1 || d->Hs < 1 || d->Ws < 1 || d->C < 8 || d->C % 8) return CREAM_ERR_BAD_ARG;
    if (d->residual != 0 && d->residual != 1) return CREAM_ERR_BAD_ARG;
    if (d->dtype != CREAM_BF16 && d->dtype != CREAM_F32) return CREAM_ERR_BAD_DTYPE;
    if ((int64_t)d->B * d->Hs * d->Ws > (int64_t)1 << 30 || (int64_t)d->Hs * d->Ws > (int64_t)1 << 30) return CREAM_ERR_TOO_LARGE;
    return CREAM_OK;
}

int check(const cream_token_dwconv7_desc* d, bool bwd) {
    if (!d || !d->x || !d->w) return CREAM_ERR_BAD_ARG;
    if (const int rc = check_shape(d)) return rc;
    if (!aligned16(d->x) || !aligned16(d->w) || ((uintptr_t)d->bias & 3)) return CREAM_ERR_BAD_ARG;
    if (!bwd) {
        if (!d->y || !aligned16(d->y)) return CREAM_ERR_BAD_ARG;
    } else {
        if (!d->dy || !d->dx || !d->part || d->part_blocks < 1) return CREAM_ERR_BAD_ARG;
        if (!aligned16(d->dy) || !aligned16(d->dx) || !aligned16(d->part)) return CREAM_ERR_BAD_ARG;
    }
    return CREAM_OK;
}

Args to_args(const cream_token_dwconv7_desc* d) {
    Args a{};
    a.w = d->w;
    a.B = d->B; a.Hs = d->Hs; a.Ws = d->Ws; a.C = d->C;
    a.nti = (d->Hs + TILE - 1) / TILE; a.ntj = (d->Ws + TILE - 1) / TILE;
    a.tiles = d->B * a.nti * a.ntj;
    a.residual = d->residual;
    return a;
}

dim3 grid_for(const Args& a) {
    const int chunks = (a.C + CCH - 1) / CCH;
    int cap = cu_count() * PER_CU / chunks;
    if (cap < 1) cap = 1;
    return dim3((unsigned)(a.tiles < cap ? a.tiles : cap), (unsigned)chunks);
}

template <typename Kern> int launch(Kern kern, dim3 grid, int lds_bytes, const Args& a, hipStream_t st) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess)
        return CREAM_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), (size_t)lds_bytes, st, a);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int stencil(const Args& a, bool bf16, hipStream_t st) {
    constexpr int lds = XS_FLOATS * 4;
    return bf16 ? launch(token_dwconv7_stencil_kernel<true>, grid_for(a), lds, a, st)
                : launch(token_dwconv7_stencil_kernel<false>, grid_for(a), lds, a, st);
}

}  // namespace

extern "C" {

int cream_token_dwconv7_part_size(int C)
{
    if (C < 8 || C % 8) return CREAM_ERR_BAD_ARG;
    return (T + 1) * C;
}

int cream_token_dwconv7_blocks(const cream_token_dwconv7_desc* d)
{
    const int rc = check_shape(d);
    if (rc) return rc;
    return (int)grid_for(to_args(d)).x;
}

int cream_token_dwconv7_fwd(const cream_token_dwconv7_desc* d, void* stream)
{
    const int rc = check(d, false);
    if (rc) return rc;
    Args a = to_args(d);
    a.x = d->x; a.bias = d->bias; a.y = d->y; a.flip = 0;
    return stencil(a, d->dtype == CREAM_BF16, (hipStream_t)stream);
}

int cream_token_dwconv7_bwd(const cream_token_dwconv7_desc* d, void* stream)
{
    const int rc = check(d, true);
    if (rc) return rc;
    Args a = to_args(d);
    const dim3 grid = grid_for(a);
    if (d->part_blocks != (int)grid.x) return CREAM_ERR_BAD_ARG;
    const bool bf16 = d->dtype == CREAM_BF16;
    a.x = d->dy; a.bias = nullptr; a.y = d->dx; a.flip = 1;                      // dx: the flipped stencil on dy
    if (const int rc2 = stencil(a, bf16, (hipStream_t)stream)) return rc2;
    a.x = d->x; a.dy = d->dy; a.part = d->part;
    constexpr int lds = (XS_FLOATS + DY_FLOATS) * 4;
    return bf16 ? launch(token_dwconv7_wgrad_kernel<true>, grid, lds, a, (hipStream_t)stream)
                : launch(token_dwconv7_wgrad_kernel<false>, grid, lds, a, (hipStream_t)stream);
}

}  // extern "C"

// token_dwconv.hip — depthwise K x K convolution (stride 1, zero padding K / 2) on the TOKEN layout (B, Hs*Ws, C).
//
// TinyViT runs a depthwise 3 x 3 Conv2d_BN between the attention and the MLP of every block (TinyViT/models/tiny_vit.py:333-335,
// :374-376) and transposes the token stream to NCHW and back for it.  On the token layout the channel axis is the fast one, so
// the convolution is a stencil over rows of C values: a thread owns VEC consecutive channels, keeps their K*K taps in registers
// and walks over tokens; every access is one 16-byte (bf16, VEC = 8) or two 16-byte (fp32) accesses along C.
//
//     y[b, i, j, c]   = bias[c] + sum_{di, dj} w[c, di, dj] x[b, i + di - R, j + dj - R, c]          R = K / 2
//     dx[b, i, j, c]  = sum_{di, dj} w[c, di, dj] dy[b, i - di + R, j - dj + R, c]                   (the same stencil, taps flipped)
//     dw[c, di, dj]   = sum_{b, i, j} dy[b, i, j, c] x[b, i + di - R, j + dj - R, c],   dbias[c] = sum dy[b, i, j, c]
//
// Arithmetic: fp32 throughout, products and additions separate (-ffp-contract=off), in the fixed order bias, then the taps in
// row-major (di, dj) order; out-of-map taps add nothing.  I/O is bf16 (round to nearest even on the store) or fp32.
// No atomics: dw and dbias come as one partial per workgroup of the gradient launch, [dw (C, K*K) | dbias (C)] fp32, every
// entry written by exactly one workgroup — a thread's chain over its tokens, then the workgroup's token slots in ascending order
// through LDS; the caller sums the partials over the first axis.
//
// Launch shape.  CV = C / VEC channel vectors.  A workgroup of 256 threads covers CVB = min(CV, 256) channel vectors
// (blockIdx.y picks the chunk when CV > 256) times TPB = 256 / CVB token slots; thread = slot * CVB + vector, so a wave reads
// consecutive channels of one token, then the next token.  blockIdx.x strides over the tokens.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cream_amd.h"
#include "cu_budget.hpp"

namespace {

using cream::cu_count;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 hwbf16x2 __attribute__((ext_vector_type(2)));

constexpr int THREADS = 256;

struct Args {
    const void* x;        // what the stencil reads (x in the forward, dy for dx) / the x of the gradient launch
    const void* dy;       // gradient launch only
    const float* w;       // (C, K*K)
    const float* bias;    // (C) or nullptr
    void* y;              // what the stencil writes
    float* part;          // (gridDim.x, (K*K + 1) C)
    int64_t tokens;       // B * Hs * Ws
    int Hs, Ws, C, CV, CVB, TPB, flip;
};

// VEC consecutive elements at element offset `off` of a bf16 or fp32 array, as fp32
template <int VEC, bool BF16> __device__ __forceinline__ void load_vec(float (&v)[VEC], const void* base, int64_t off) {
    if constexpr (BF16) {
        const uint16_t* p = (const uint16_t*)base + off;
        if constexpr (VEC == 8) {
            const u32x4 r = *(const u32x4*)p;
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(r[i] << 16); v[2 * i + 1] = __uint_as_float(r[i] & 0xffff0000u); }
        } else {
            const u32x2 r = *(const u32x2*)p;
#pragma unroll
            for (int i = 0; i < 2; ++i) { v[2 * i] = __uint_as_float(r[i] << 16); v[2 * i + 1] = __uint_as_float(r[i] & 0xffff0000u); }
        }
    } else {
        const float* p = (const float*)base + off;
#pragma unroll
        for (int i = 0; i < VEC / 4; ++i) {
            const f32x4 r = *(const f32x4*)(p + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * i + e] = r[e];
        }
    }
}

template <int VEC, bool BF16> __device__ __forceinline__ void store_vec(void* base, int64_t off, const float (&v)[VEC]) {
    if constexpr (BF16) {
        uint16_t* p = (uint16_t*)base + off;
        uint32_t r[VEC / 2];
#pragma unroll
        for (int i = 0; i < VEC / 2; ++i)         // round to nearest even (v_cvt_pk_bf16_f32)
            r[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2{v[2 * i], v[2 * i + 1]}), hwbf16x2));
        if constexpr (VEC == 8) *(u32x4*)p = u32x4{r[0], r[1], r[2], r[3]};
        else *(u32x2*)p = u32x2{r[0], r[1]};
    } else {
        float* p = (float*)base + off;
#pragma unroll
        for (int i = 0; i < VEC / 4; ++i) *(f32x4*)(p + 4 * i) = f32x4{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]};
    }
}

// y = bias + stencil(x) with the taps as they are (flip == 0) or reversed (flip != 0: dx from dy)
template <int K, int VEC, bool BF16> __global__ __launch_bounds__(THREADS) void token_dwconv_stencil_kernel(const Args a) {
    constexpr int T = K * K, R = K / 2;
    const int cvl = threadIdx.x % a.CVB, slot = threadIdx.x / a.CVB;
    const int cv = blockIdx.y * a.CVB + cvl;
    if (slot >= a.TPB || cv >= a.CV) return;
    const int c0 = cv * VEC;

    float tap[T][VEC], bv[VEC];
    {
        float flat[T * VEC];                          // w[c0 .. c0 + VEC - 1][0 .. T - 1]: contiguous, 16-byte aligned
        const f32x4* wp = (const f32x4*)(a.w + (int64_t)c0 * T);
#pragma unroll
        for (int i = 0; i < T * VEC / 4; ++i) {
            const f32x4 r = wp[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) flat[4 * i + e] = r[e];
        }
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int e = 0; e < VEC; ++e) tap[t][e] = a.flip ? flat[e * T + T - 1 - t] : flat[e * T + t];
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) bv[e] = a.bias ? a.bias[c0 + e] : 0.0f;

    const int L = a.Hs * a.Ws;
    for (int64_t tok = (int64_t)blockIdx.x * a.TPB + slot; tok < a.tokens; tok += (int64_t)gridDim.x * a.TPB) {
        const int n = (int)(tok % L), i = n / a.Ws, j = n - i * a.Ws;
        float acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = bv[e];
#pragma unroll
        for (int di = 0; di < K; ++di) {
            const int ii = i + di - R;
            const bool row_ok = ii >= 0 && ii < a.Hs;
#pragma unroll
            for (int dj = 0; dj < K; ++dj) {
                const int jj = j + dj - R;
                const bool ok = row_ok && jj >= 0 && jj < a.Ws;
                // an out-of-map tap reads the token itself (always in bounds) and adds nothing
                const int64_t src = ok ? tok + (int64_t)(di - R) * a.Ws + (dj - R) : tok;
                float v[VEC];
                load_vec<VEC, BF16>(v, a.x, src * a.C + c0);
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float p = tap[di * K + dj][e] * v[e];
                    acc[e] = ok ? acc[e] + p : acc[e];
                }
            }
        }
        store_vec<VEC, BF16>(a.y, tok * a.C + c0, acc);
    }
}

// one partial [dw (C, T) | dbias (C)] per blockIdx.x
template <int K, int VEC, bool BF16> __global__ __launch_bounds__(THREADS) void token_dwconv_wgrad_kernel(const Args a) {
    constexpr int T = K * K, R = K / 2;
    __shared__ float red[THREADS * VEC];
    const int cvl = threadIdx.x % a.CVB, slot = threadIdx.x / a.CVB;
    const int cv = blockIdx.y * a.CVB + cvl;
    const bool active = slot < a.TPB && cv < a.CV;
    const int c0 = cv * VEC;

    float dw[T + 1][VEC];                             // row T: dbias
#pragma unroll
    for (int t = 0; t <= T; ++t)
#pragma unroll
        for (int e = 0; e < VEC; ++e) dw[t][e] = 0.0f;

    if (active) {
        const int L = a.Hs * a.Ws;
        for (int64_t tok = (int64_t)blockIdx.x * a.TPB + slot; tok < a.tokens; tok += (int64_t)gridDim.x * a.TPB) {
            const int n = (int)(tok % L), i = n / a.Ws, j = n - i * a.Ws;
            float g[VEC];
            load_vec<VEC, BF16>(g, a.dy, tok * a.C + c0);
#pragma unroll
            for (int e = 0; e < VEC; ++e) dw[T][e] = dw[T][e] + g[e];
#pragma unroll
            for (int di = 0; di < K; ++di) {
                const int ii = i + di - R;
                const bool row_ok = ii >= 0 && ii < a.Hs;
#pragma unroll
                for (int dj = 0; dj < K; ++dj) {
                    const int jj = j + dj - R;
                    const bool ok = row_ok && jj >= 0 && jj < a.Ws;
                    const int64_t src = ok ? tok + (int64_t)(di - R) * a.Ws + (dj - R) : tok;
                    float v[VEC];
                    load_vec<VEC, BF16>(v, a.x, src * a.C + c0);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const float p = g[e] * v[e];
                        dw[di * K + dj][e] = ok ? dw[di * K + dj][e] + p : dw[di * K + dj][e];
                    }
                }
            }
        }
    }

    // the workgroup's token slots, in ascending order, one tap (or dbias) per round
    float* out = a.part + (int64_t)blockIdx.x * (T + 1) * a.C;
#pragma unroll
    for (int t = 0; t <= T; ++t) {
        if (active) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) red[threadIdx.x * VEC + e] = dw[t][e];
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < a.CVB * VEC; idx += THREADS) {
            const int cl = idx / VEC, e = idx - cl * VEC, cvx = blockIdx.y * a.CVB + cl;
            if (cvx < a.CV) {
                float s = 0.0f;
                for (int sl = 0; sl < a.TPB; ++sl) s = s + red[(sl * a.CVB + cl) * VEC + e];
                const int c = cvx * VEC + e;
                out[t < T ? (int64_t)c * T + t : (int64_t)T * a.C + c] = s;
            }
        }
        __syncthreads();
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
constexpr int VEC_BF16 = 8, VEC_F32 = 4;             // channels per thread: one 16-byte access either way

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_shape(const cream_token_dwconv3_desc* d) {
    if (!d) return CREAM_ERR_BAD_ARG;
    if (d->B < 1 || d->Hs < 1 || d->Ws < 1 || d->C < 8 || d->C % 8) return CREAM_ERR_BAD_ARG;
    if (d->dtype != CREAM_BF16 && d->dtype != CREAM_F32) return CREAM_ERR_BAD_DTYPE;
    if ((int64_t)d->B * d->Hs * d->Ws > (int64_t)1 << 30 || (int64_t)d->Hs * d->Ws > (int64_t)1 << 30) return CREAM_ERR_TOO_LARGE;
    return CREAM_OK;
}

int check(const cream_token_dwconv3_desc* d, bool bwd) {
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

Args to_args(const cream_token_dwconv3_desc* d) {
    Args a{};
    const int vec = d->dtype == CREAM_BF16 ? VEC_BF16 : VEC_F32;
    a.w = d->w;
    a.tokens = (int64_t)d->B * d->Hs * d->Ws;
    a.Hs = d->Hs; a.Ws = d->Ws; a.C = d->C;
    a.CV = d->C / vec;
    a.CVB = a.CV < THREADS ? a.CV : THREADS;
    a.TPB = THREADS / a.CVB;
    return a;
}

dim3 grid_for(const Args& a, int blocks_per_cu) {
    const int64_t need = (a.tokens + a.TPB - 1) / a.TPB, cap = (int64_t)cu_count() * blocks_per_cu;
    return dim3((unsigned)(need < cap ? need : cap), (unsigned)((a.CV + a.CVB - 1) / a.CVB));
}

constexpr int FWD_PER_CU = 8, WGRAD_PER_CU = 2;      // the gradient launch writes one partial per workgroup: fewer, longer chains

template <typename Kern> int launch(Kern kern, dim3 grid, const Args& a, hipStream_t st) {
    hipLaunchKernelGGL(kern, grid, dim3(THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int stencil(const Args& a, bool bf16, hipStream_t st) {
    const dim3 grid = grid_for(a, FWD_PER_CU);
    return bf16 ? launch(token_dwconv_stencil_kernel<3, VEC_BF16, true>, grid, a, st)
                : launch(token_dwconv_stencil_kernel<3, VEC_F32, false>, grid, a, st);
}

}  // namespace

extern "C" {

int cream_token_dwconv3_part_size(int C)
{
    if (C < 8 || C % 8) return CREAM_ERR_BAD_ARG;
    return 10 * C;
}

int cream_token_dwconv3_blocks(const cream_token_dwconv3_desc* d)
{
    const int rc = check_shape(d);
    if (rc) return rc;
    return (int)grid_for(to_args(d), WGRAD_PER_CU).x;
}

int cream_token_dwconv3_fwd(const cream_token_dwconv3_desc* d, void* stream)
{
    const int rc = check(d, false);
    if (rc) return rc;
    Args a = to_args(d);
    a.x = d->x; a.bias = d->bias; a.y = d->y; a.flip = 0;
    return stencil(a, d->dtype == CREAM_BF16, (hipStream_t)stream);
}

int cream_token_dwconv3_bwd(const cream_token_dwconv3_desc* d, void* stream)
{
    const int rc = check(d, true);
    if (rc) return rc;
    Args a = to_args(d);
    const dim3 grid = grid_for(a, WGRAD_PER_CU);
    if (d->part_blocks != (int)grid.x) return CREAM_ERR_BAD_ARG;
    const bool bf16 = d->dtype == CREAM_BF16;
    a.x = d->dy; a.bias = nullptr; a.y = d->dx; a.flip = 1;                      // dx: the flipped stencil on dy
    if (const int rc2 = stencil(a, bf16, (hipStream_t)stream)) return rc2;
    a.x = d->x; a.dy = d->dy; a.part = d->part;
    return bf16 ? launch(token_dwconv_wgrad_kernel<3, VEC_BF16, true>, grid, a, (hipStream_t)stream)
                : launch(token_dwconv_wgrad_kernel<3, VEC_F32, false>, grid, a, (hipStream_t)stream);
}

}  // extern "C"

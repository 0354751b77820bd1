// cga_attn.hip — EfficientViT's cascaded group attention (EfficientViT/classification/model/efficientvit.py:159-180), one
// launch for every window of the map, BatchNorm folded (inference).
//
// The heads of a CascadedGroupAttention run in sequence: head i projects  feat_in_i = feat_{i-1} + x_i  (x_i: its Cg = C / h
// input channels) with a 1 x 1 convolution into q (16), k (16) and v (Cg), passes q through a k_i x k_i depthwise convolution
// inside the window (zero padding), and  feat_i = softmax(scale q' k^T + ab_i) v  is both a slice of the output and the next
// head's input.  A window has N = w^2 <= 64 tokens, so one workgroup keeps the whole cascade of a window in LDS and registers:
// x is read once, the output written once, nothing else touches memory but the (L2-resident) weights.
//
// Work split.  The window is padded to MT = ceil(N / 16) tiles of 16 tokens and the workgroup has MT waves (64 threads for the
// 16-token windows, 256 for the 49- and 64-token ones).  Per head:
//   A  projection   [q | k | v] = feat_in W^T + b on v_mfma_f32_16x16x32_bf16; a wave takes 16-wide output-channel tiles and
//                   keeps the weight fragments of its tile in registers (read straight from global: the (oc, c) layout of
//                   the folded convolution weight IS the operand layout).  q and k land token-major, v channel-major, each with
//                   8-byte LDS stores: the q / k tiles are computed as W X^T, the v tiles as X W^T — the same fragments, swapped.
//   B  q' = dwconv(q) + bias on the VALU, one (token, channel) per thread and step, taps staged in LDS.
//   C  wave t owns query tile t: S^T = K Q'^T on v_mfma_f32_16x16x16_bf16 (the contraction is key_dim = 16), so a lane holds
//      16 keys of ONE query (4 per key tile) and the softmax needs two shuffles; P^T goes back in as the B operand of
//      v_mfma_f32_16x16x32_bf16 with the contraction enumerated in the accumulator's order (keys 16 t + 4 (lane >> 4) + r of
//      two key tiles), which V^T supplies with two 8-byte LDS reads — no LDS round trip for P.  The lane then holds
//      feat_i[query][4 consecutive channels]: one 8-byte store to the output, and  bf16(feat_i + x_{i+1})  into the next
//      head's input tile.
//
// Rounding points (tests/cga_ref.py `kernel_model` restates them): feat_in = bf16(feat_{i-1} + x_i), both terms bf16;
// q, k, v = bf16(fp32 accumulation + bias); q' = bf16(fp32 taps + bias); logits scale q'k + ab, softmax and the row sum in
// fp32; P = bf16(exp(l - max)) unnormalised; feat = bf16(fp32 accumulation / row sum).  The stored (pre-ReLU) bf16 feat_i is
// the value head i + 1 reads.  Pad keys (m >= N) are excluded from the softmax; pad queries are never stored.
//
// Operands: the weights (h, 32 + Cg, KP) bf16 with KP = Cg rounded up to 32 and zero columns past Cg; biases, taps and the
// expanded attention bias fp32.  No atomics, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_common.hpp"
#include "cream_amd.h"

namespace {

using namespace cream;

constexpr int KD = 16;            // key_dim
constexpr int QPI = 20;           // pitch (elements) of the token-major q / q' / k tiles
constexpr int VPI = 72;           // pitch of the channel-major v tile (64 tokens + 8)
constexpr int MAXK = 7;

struct Args {
    const short* x;
    int64_t xsb, xsy, xsx;
    const short* wqkv;
    const float* bqkv;
    const float* dw;
    const float* dwb;
    const float* ab;
    short* out;
    int Hs, Ws, w, h, Cg, relu, nwx, nwy;
    int ks4;              // k_i in bits 4 i .. 4 i + 3
    float scale;
};

__device__ __forceinline__ f32x4v mma32(bf16x8 a, bf16x8 b, f32x4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(hwbf16x8, a), __builtin_bit_cast(hwbf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4v mma16(bf16x4 a, bf16x4 b, f32x4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x4 ld4(const short* p) { return __builtin_bit_cast(bf16x4, *reinterpret_cast<const u32x2v*>(p)); }
__device__ __forceinline__ bf16x8 ld8(const short* p) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(p)); }
__device__ __forceinline__ void st4(short* p, float a, float b, float c, float d) {
    *reinterpret_cast<u32x2v*>(p) = u32x2v{f2bf_pair(a, b), f2bf_pair(c, d)};
}

// KS: 32-deep contraction steps of the projection, KP = 32 KS >= Cg
template <int KS>
__global__ __launch_bounds__(256) void cga_attn_kernel(const Args a)
{
    constexpr int KP = 32 * KS, XPI = KP + 8;
    __shared__ __attribute__((aligned(16))) short XF[64 * XPI];        // feat_in, token-major, zero past Cg and past N
    __shared__ __attribute__((aligned(16))) short QS[64 * QPI];        // q
    __shared__ __attribute__((aligned(16))) short QC[64 * QPI];        // q' (after the depthwise convolution)
    __shared__ __attribute__((aligned(16))) short KT[64 * QPI];        // k
    __shared__ __attribute__((aligned(16))) short VT[KP * VPI];        // v, channel-major
    __shared__ float TAPS[KD * MAXK * MAXK];

    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
    const int li = lane & 15, q4 = lane >> 4;
    const int w = a.w, N = w * w, MT = (N + 15) >> 4;                  // nw == MT
    const int Cg = a.Cg, C = a.h * Cg, CT = 2 + (Cg >> 4);
    int bid = blockIdx.x;
    const int wx = bid % a.nwx;
    bid /= a.nwx;
    const int wy = bid % a.nwy, b = bid / a.nwy;
    const short* xw = a.x + b * a.xsb + (int64_t)(wy * w) * a.xsy + (int64_t)(wx * w) * a.xsx;
    short* ow = a.out + (((int64_t)b * a.Hs + wy * w) * a.Ws + wx * w) * C;

    // feat_in of head 0: x's first Cg channels; zero rows past N and zero columns past Cg, which stay zero
    for (int idx = tid; idx < MT * 16 * (KP / 8); idx += nthr) {
        const int n = idx / (KP / 8), c = (idx - n * (KP / 8)) * 8;
        u32x4v v = u32x4v{0u, 0u, 0u, 0u};
        if (n < N && c < Cg) v = *reinterpret_cast<const u32x4v*>(xw + (n / w) * a.xsy + (n % w) * a.xsx + c);
        *reinterpret_cast<u32x4v*>(XF + n * XPI + c) = v;
    }
    __syncthreads();

    int tap_off = 0;
    for (int i = 0; i < a.h; ++i) {
        const int k = (a.ks4 >> (4 * i)) & 15, R = k >> 1;
        // ---- A: projection -----------------------------------------------------------------------------------------------
        {
            const short* W = a.wqkv + (int64_t)i * (32 + Cg) * KP;
            const float* bq = a.bqkv + i * (32 + Cg);
            for (int ct = wave; ct < CT; ct += nw) {
                bf16x8 wf[KS];
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) wf[kk] = ld8(W + (ct * 16 + li) * KP + kk * 32 + 8 * q4);
                for (int mt = 0; mt < MT; ++mt) {
                    const short* xr = XF + (mt * 16 + li) * XPI + 8 * q4;
                    f32x4v acc = f32x4v{0.f, 0.f, 0.f, 0.f};
                    if (ct < 2) {                                      // rows = 4 output channels, column = token li
#pragma unroll
                        for (int kk = 0; kk < KS; ++kk) acc = mma32(wf[kk], ld8(xr + kk * 32), acc);
                        const f32x4v bb = *reinterpret_cast<const f32x4v*>(bq + ct * 16 + 4 * q4);
                        st4((ct == 0 ? QS : KT) + (mt * 16 + li) * QPI + 4 * q4, acc[0] + bb[0], acc[1] + bb[1], acc[2] + bb[2],
                            acc[3] + bb[3]);
                    } else {                                           // rows = 4 tokens, column = output channel li
#pragma unroll
                        for (int kk = 0; kk < KS; ++kk) acc = mma32(ld8(xr + kk * 32), wf[kk], acc);
                        const int d = (ct - 2) * 16 + li;
                        const float bb = bq[32 + d];
                        st4(VT + d * VPI + mt * 16 + 4 * q4, acc[0] + bb, acc[1] + bb, acc[2] + bb, acc[3] + bb);
                    }
                }
            }
            for (int idx = tid; idx < KD * k * k; idx += nthr) TAPS[idx] = a.dw[tap_off + idx];
        }
        __syncthreads();
        // ---- B: q' = depthwise k x k convolution of q inside the window, zero padding ---------------------------------------
        for (int idx = tid; idx < MT * 16 * KD; idx += nthr) {
            const int c = idx & 15, n = idx >> 4;
            float r = 0.f;
            if (n < N) {
                const int y0 = n / w, x0 = n - y0 * w;
                float acc = 0.f;
                for (int dy = -R; dy <= R; ++dy) {
                    const int yy = y0 + dy;
                    if (yy < 0 || yy >= w) continue;
                    for (int dx = -R; dx <= R; ++dx) {
                        const int xx = x0 + dx;
                        if (xx < 0 || xx >= w) continue;
                        acc += TAPS[(c * k + dy + R) * k + dx + R] * bf2f(QS[(yy * w + xx) * QPI + c]);
                    }
                }
                r = acc + a.dwb[i * KD + c];
            }
            QC[n * QPI + c] = f2bf(r);
        }
        __syncthreads();
        // ---- C: attention of query tile `wave` ----------------------------------------------------------------------------------
        {
            const int nq = wave * 16 + li;                             // this lane's query
            const int nqc = nq < N ? nq : N - 1;                       // a pad query computes a copy of the last row, never stored
            const bf16x4 qf = ld4(QC + nqc * QPI + 4 * q4);
            const float* abr = a.ab + ((int64_t)i * N + nqc) * N;
            float p[4][4];
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f32x4v s = f32x4v{0.f, 0.f, 0.f, 0.f};
                if (t < MT) s = mma16(ld4(KT + (t * 16 + li) * QPI + 4 * q4), qf, s);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = t * 16 + 4 * q4 + r;                 // the key of accumulator register r
                    p[t][r] = m < N ? s[r] * a.scale + abr[m] : -INFINITY;
                    mx = fmaxf(mx, p[t][r]);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[t][r] = t * 16 + 4 * q4 + r < N ? __expf(p[t][r] - mx) : 0.f;
                    sum += p[t][r];
                }
            sum += __shfl_xor(sum, 16);
            sum += __shfl_xor(sum, 32);
            bf16x8 pf[2];
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                const u32x4v u = u32x4v{f2bf_pair(p[2 * pp][0], p[2 * pp][1]), f2bf_pair(p[2 * pp][2], p[2 * pp][3]),
                                        f2bf_pair(p[2 * pp + 1][0], p[2 * pp + 1][1]), f2bf_pair(p[2 * pp + 1][2], p[2 * pp + 1][3])};
                pf[pp] = __builtin_bit_cast(bf16x8, u);
            }
            const bool more = i + 1 < a.h;
            const short* xq = xw + (nqc / w) * a.xsy + (nqc % w) * a.xsx + (i + 1) * Cg;
            short* oq = ow + ((int64_t)(nqc / w) * a.Ws + nqc % w) * C + i * Cg;
            for (int dt = 0; dt < (Cg >> 4); ++dt) {
                const short* vr = VT + (dt * 16 + li) * VPI + 4 * q4;
                f32x4v acc = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) {
                    if (2 * pp < MT) {
                        const u32x2v lo = *reinterpret_cast<const u32x2v*>(vr + 32 * pp);
                        u32x2v hi = u32x2v{0u, 0u};
                        if (2 * pp + 1 < MT) hi = *reinterpret_cast<const u32x2v*>(vr + 32 * pp + 16);
                        acc = mma32(__builtin_bit_cast(bf16x8, (u32x4v{lo[0], lo[1], hi[0], hi[1]})), pf[pp], acc);
                    }
                }
                // this lane: feat_i[nq][dt * 16 + 4 q4 + r]
                if (nq < N) {
                    const int d = dt * 16 + 4 * q4;
                    float f[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) f[r] = bf2f(f2bf(acc[r] / sum));
                    if (a.relu) st4(oq + d, fmaxf(f[0], 0.f), fmaxf(f[1], 0.f), fmaxf(f[2], 0.f), fmaxf(f[3], 0.f));
                    else st4(oq + d, f[0], f[1], f[2], f[3]);
                    if (more) {
                        const bf16x4 xv = ld4(xq + d);
                        st4(XF + nq * XPI + d, f[0] + bf2f(xv[0]), f[1] + bf2f(xv[1]), f[2] + bf2f(xv[2]), f[3] + bf2f(xv[3]));
                    }
                }
            }
        }
        tap_off += KD * k * k;
        __syncthreads();
    }
}

bool cg_ok(int Cg) { return Cg >= 16 && Cg <= 112 && Cg % 16 == 0; }
bool aligned(const void* p, uintptr_t n) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

int check(const cream_cga_desc* d)
{
    if (!d) return CREAM_ERR_BAD_ARG;
    if (!cg_ok(d->Cg) || d->h < 1 || d->h > 4 || d->w < 1 || d->w > 8) return CREAM_ERR_BAD_ARG;
    if (d->B < 1 || d->Hs < 1 || d->Ws < 1 || d->Hs % d->w || d->Ws % d->w) return CREAM_ERR_BAD_ARG;
    for (int i = 0; i < d->h; ++i)
        if (d->ks[i] != 1 && d->ks[i] != 3 && d->ks[i] != 5 && d->ks[i] != 7) return CREAM_ERR_BAD_ARG;
    if (!aligned(d->x, 16) || !aligned(d->wqkv, 16) || !aligned(d->out, 16)) return CREAM_ERR_BAD_ARG;
    if (!aligned(d->bqkv, 16) || !aligned(d->dw, 4) || !aligned(d->dwb, 4) || !aligned(d->ab, 4)) return CREAM_ERR_BAD_ARG;
    if (d->xsb < 0 || d->xsy < 0 || d->xsx < 0 || d->xsb % 8 || d->xsy % 8 || d->xsx % 8) return CREAM_ERR_BAD_ARG;
    if (d->xsx < (int64_t)d->h * d->Cg) return CREAM_ERR_BAD_ARG;                       // tokens would overlap
    if ((int64_t)d->B * (d->Hs / d->w) * (d->Ws / d->w) > 0x7fffffffLL) return CREAM_ERR_TOO_LARGE;
    return CREAM_OK;
}

}  // namespace

extern "C" {

int cream_cga_attn_check(const cream_cga_desc* d) { return check(d); }

int cream_cga_attn_fwd(const cream_cga_desc* d, void* stream)
{
    const int rc = check(d);
    if (rc) return rc;
    Args a{};
    a.x = static_cast<const short*>(d->x);
    a.xsb = d->xsb; a.xsy = d->xsy; a.xsx = d->xsx;
    a.wqkv = static_cast<const short*>(d->wqkv);
    a.bqkv = d->bqkv; a.dw = d->dw; a.dwb = d->dwb; a.ab = d->ab;
    a.out = static_cast<short*>(d->out);
    a.Hs = d->Hs; a.Ws = d->Ws; a.w = d->w; a.h = d->h; a.Cg = d->Cg; a.relu = d->relu != 0;
    a.nwx = d->Ws / d->w; a.nwy = d->Hs / d->w;
    for (int i = 0; i < d->h; ++i) a.ks4 |= d->ks[i] << (4 * i);
    a.scale = d->scale;
    const dim3 grid((unsigned)(d->B * a.nwy * a.nwx)), block(64 * ((d->w * d->w + 15) / 16));
    hipStream_t st = (hipStream_t)stream;
    switch ((d->Cg + 31) / 32) {
        case 1: hipLaunchKernelGGL(cga_attn_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(cga_attn_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(cga_attn_kernel<3>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(cga_attn_kernel<4>, grid, block, 0, st, a); break;
    }
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

}  // extern "C"

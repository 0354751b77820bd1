// evit_ffn.hip — EfficientViT's depthwise 3 x 3 + FFN pair on the token layout, BatchNorm folded (inference), and the
// pointwise convolution with a residual that the mixer's `proj` needs.
//
// Every EfficientViTBlock (EfficientViT/classification/model/efficientvit.py:250-282) is  dw0 -> ffn0 -> mixer -> dw1 -> ffn1,
// each a Residual; in eval mode every Conv2d_BN is a convolution with a bias, so a dw + FFN pair is
//     y1 = x + dw3x3(x) + bd                       (zero padding outside the map)
//     y2 = y1 + W2 relu(W1 y1 + b1) + b2
// cream_evit_dwffn_fwd computes it in one launch: x (B, H, W, C) is read once (plus the halo rows, which the caches serve),
// y2 written once; y1 and the Ch-wide hidden activation stay in registers and LDS.
// cream_evit_pw_residual_fwd is the second product alone:  out = res + W a + b.
//
// Work split.  The B H W tokens are numbered b (H W) + y W + x and a workgroup of four waves owns 64 consecutive ones,
// whatever the map: row strips with their halo on 14 x 14, one image and part of the next on 7 x 7, four images on 4 x 4.
// Every product is computed "swapped" on v_mfma_f32_16x16x32_bf16, D = W X^T: the A operand is a weight fragment (16 rows of
// the (oc, c) convolution weight, which IS the operand layout), the B operand 16 tokens of an LDS tile, and a lane holds
// 4 consecutive output channels of ONE token.
//   0  y1: wave v owns the 16-channel tiles v, v + 4, ..; a lane computes the nine taps of its 4 channels for its token in
//      each of the four token tiles straight from global memory (8-byte loads; the image a token belongs to and the border
//      decide which taps exist, so a halo never crosses into a neighbouring image or a buffer's padding).  The fp32 y1 IS the
//      output accumulator of that lane; bf16(y1) goes to the LDS tile Y1 (64 tokens x KP, zero past C).
//   1  per chunk of 64 hidden channels: wave v computes hidden tile v of the chunk, relu(W1 Y1^T + b1) for the 64 tokens, and
//      stores it bf16 into the LDS tile HS (two buffers, so one barrier per chunk).
//   2  acc += W2[:, chunk] HS^T for the wave's channel tiles.
//   3  the bf16 result goes through the Y1 tile so that the 64 x C output — one contiguous block — is written with 16-byte
//      stores.
// The weights are NOT staged in LDS: within a workgroup every weight element is used by exactly one wave (the waves split the
// hidden rows in 1 and the output rows in 2), so LDS would add a copy and save no traffic; the fragments go from L2 to
// registers and are reused across the four token tiles.
//
// Rounding points (tests/evit_ffn_ref.py `kernel_model` restates them): x bf16; the nine taps, the bias and y1 in fp32; the
// first product's operand is bf16(y1); the hidden is accumulated in fp32, + b1, ReLU, then bf16; the second product is
// accumulated in fp32 ON TOP of the fp32 y1; out = bf16(that + b2).  pw_residual: out = bf16(fp32(res) + b + fp32 products).
// No atomics, no scratch, nothing of activation size but the output is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_common.hpp"
#include "cream_amd.h"

namespace {

using namespace cream;

constexpr int TM = 64;            // tokens of a workgroup
constexpr int HC = 64;            // hidden channels of a chunk
constexpr int HPI = HC + 8;       // pitch (elements) of the hidden tile

struct DwArgs {
    const short* x;
    int64_t xsb, xsy, xsx;
    const float* taps;
    const float* dwb;
    const short* w1;
    const float* b1;
    const short* w2;
    const float* b2;
    short* out;
    int H, W, C, Ch, KP, T;
};

struct PwArgs {
    const short* a;
    int64_t asb, asy, asx;
    const short* res;
    int64_t rsb, rsy, rsx;
    const short* w;
    const float* b;
    short* out;
    int H, W, Cin, Cout, KP, T;
};

__device__ __forceinline__ f32x4v mma32(bf16x8 a, bf16x8 b, f32x4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(hwbf16x8, a), __builtin_bit_cast(hwbf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ bf16x4 ld4(const short* p) { return __builtin_bit_cast(bf16x4, *reinterpret_cast<const u32x2v*>(p)); }
__device__ __forceinline__ bf16x8 ld8(const short* p) { return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4v*>(p)); }
__device__ __forceinline__ void st4(short* p, float a, float b, float c, float d) {
    *reinterpret_cast<u32x2v*>(p) = u32x2v{f2bf_pair(a, b), f2bf_pair(c, d)};
}

// the 64 x C bf16 tile in LDS (pitch PI) -> out rows t0 .. t0 + 63 (those below T), 16 bytes per thread and step
__device__ __forceinline__ void store_tile(const short* tile, int PI, short* out, int C, int t0, int T, int tid)
{
    const int c8 = C >> 3;
    int live = T - t0;
    live = live < TM ? live : TM;
    short* o = out + (int64_t)t0 * C;
    for (int idx = tid; idx < live * c8; idx += 256) {
        const int n = idx / c8, c = (idx - n * c8) * 8;
        *reinterpret_cast<u32x4v*>(o + (int64_t)n * C + c) = *reinterpret_cast<const u32x4v*>(tile + n * PI + c);
    }
}

// KS2: the channel axis in steps of 64 (KPL = 64 KS2 >= C); a wave owns up to KS2 channel tiles of 16
template <int KS2>
__global__ __launch_bounds__(256) void evit_dwffn_kernel(const DwArgs a)
{
    constexpr int KPL = 64 * KS2, PI = KPL + 8, NTW = KS2;
    __shared__ __attribute__((aligned(16))) short Y1[TM * PI];         // bf16(y1), token-major, zero past C
    __shared__ __attribute__((aligned(16))) short HS[2 * TM * HPI];    // the hidden chunk, token-major, two buffers

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q4 = lane >> 4;
    const int C = a.C, Ch = a.Ch, KP = a.KP, nt = C >> 4, ks = KP >> 5, H = a.H, W = a.W;
    const int t0 = blockIdx.x * TM;

    // the columns C .. KPL of Y1 are contraction padding: zero
    {
        const int z8 = (KPL - C) >> 3;
        for (int idx = tid; idx < TM * z8; idx += 256) {
            const int n = idx / z8, c = C + (idx - n * z8) * 8;
            *reinterpret_cast<u32x4v*>(Y1 + n * PI + c) = u32x4v{0u, 0u, 0u, 0u};
        }
    }

    // ---- 0: y1 = x + dw3x3(x) + bd in the accumulator layout --------------------------------------------------------------
    f32x4v acc[NTW][4];
    {
        const short* xc[4];       // this lane's token in token tile mt (a token past T computes a copy of the last one)
        int ok[4];                // bit k: tap k = 3 (dy + 1) + dx + 1 lies inside the token's own image
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            int t = t0 + mt * 16 + li;
            t = t < a.T ? t : a.T - 1;
            const int b = t / (H * W), r = t - b * (H * W), y = r / W, x = r - y * W;
            xc[mt] = a.x + b * a.xsb + y * a.xsy + x * a.xsx;
            int m = 0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
                m |= (yy >= 0 && yy < H && xx >= 0 && xx < W) ? 1 << k : 0;
            }
            ok[mt] = m;
        }
#pragma unroll
        for (int c = 0; c < NTW; ++c) {
            const int ct = wave + 4 * c;
            if (ct < nt) {
                const int ch = ct * 16 + 4 * q4;
                f32x4v tp[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) tp[k] = *reinterpret_cast<const f32x4v*>(a.taps + k * C + ch);
                const f32x4v bd = *reinterpret_cast<const f32x4v*>(a.dwb + ch);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    f32x4v s = f32x4v{0.f, 0.f, 0.f, 0.f};
                    f32x4v ctr = s;
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        if ((ok[mt] >> k) & 1) {
                            const bf16x4 v = ld4(xc[mt] + (k / 3 - 1) * a.xsy + (k % 3 - 1) * a.xsx + ch);
#pragma unroll
                            for (int r = 0; r < 4; ++r) s[r] += tp[k][r] * bf2f(v[r]);
                            if (k == 4) ctr = f32x4v{bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])};
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) s[r] = ctr[r] + (s[r] + bd[r]);
                    acc[c][mt] = s;
                    st4(Y1 + (mt * 16 + li) * PI + ch, s[0], s[1], s[2], s[3]);
                }
            } else {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[c][mt] = f32x4v{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    __syncthreads();

    // ---- 1, 2: the hidden activation in chunks of 64 channels -----------------------------------------------------------------
    int buf = 0;
    for (int h0 = 0; h0 < Ch; h0 += HC, buf ^= 1) {
        const int hv = Ch - h0 < HC ? Ch - h0 : HC;                    // 64, or 32 in the last chunk
        short* hs = HS + buf * (TM * HPI);
        if (wave * 16 < hv) {
            const short* wr = a.w1 + (int64_t)(h0 + wave * 16 + li) * KP + 8 * q4;
            bf16x8 wf[2 * KS2];
#pragma unroll
            for (int kk = 0; kk < 2 * KS2; ++kk)
                if (kk < ks) wf[kk] = ld8(wr + kk * 32);
            const f32x4v bb = *reinterpret_cast<const f32x4v*>(a.b1 + h0 + wave * 16 + 4 * q4);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const short* yr = Y1 + (mt * 16 + li) * PI + 8 * q4;
                f32x4v h = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 2 * KS2; ++kk)
                    if (kk < ks) h = mma32(wf[kk], ld8(yr + kk * 32), h);
                st4(hs + (mt * 16 + li) * HPI + wave * 16 + 4 * q4, fmaxf(h[0] + bb[0], 0.f), fmaxf(h[1] + bb[1], 0.f),
                    fmaxf(h[2] + bb[2], 0.f), fmaxf(h[3] + bb[3], 0.f));
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NTW; ++c) {
            const int ct = wave + 4 * c;
            if (ct < nt) {
                const short* wr = a.w2 + (int64_t)(ct * 16 + li) * Ch + h0 + 8 * q4;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    if (kk * 32 < hv) {
                        const bf16x8 wf = ld8(wr + kk * 32);
#pragma unroll
                        for (int mt = 0; mt < 4; ++mt)
                            acc[c][mt] = mma32(wf, ld8(hs + (mt * 16 + li) * HPI + kk * 32 + 8 * q4), acc[c][mt]);
                    }
                }
            }
        }
    }

    // ---- 3: + b2, bf16, through the Y1 tile to the output ---------------------------------------------------------------------
    // every wave has passed the last chunk's barrier, so Y1 is no longer read
#pragma unroll
    for (int c = 0; c < NTW; ++c) {
        const int ct = wave + 4 * c;
        if (ct < nt) {
            const int ch = ct * 16 + 4 * q4;
            const f32x4v bb = *reinterpret_cast<const f32x4v*>(a.b2 + ch);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                st4(Y1 + (mt * 16 + li) * PI + ch, acc[c][mt][0] + bb[0], acc[c][mt][1] + bb[1], acc[c][mt][2] + bb[2],
                    acc[c][mt][3] + bb[3]);
        }
    }
    __syncthreads();
    store_tile(Y1, PI, a.out, C, t0, a.T, tid);
}

// KS2: max(Cin, Cout) in steps of 64
template <int KS2>
__global__ __launch_bounds__(256) void evit_pw_kernel(const PwArgs a)
{
    constexpr int KPL = 64 * KS2, PI = KPL + 8, NTW = KS2;
    __shared__ __attribute__((aligned(16))) short AT[TM * PI];         // a, token-major, zero past Cin; then the result

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, q4 = lane >> 4;
    const int Cin = a.Cin, Cout = a.Cout, KP = a.KP, nt = Cout >> 4, ks = KP >> 5, H = a.H, W = a.W;
    const int t0 = blockIdx.x * TM;

    // the tile of a: 16 bytes per thread and step, zero past Cin (a token past T reads a copy of the last one)
    {
        const int k8 = KPL >> 3;
        for (int idx = tid; idx < TM * k8; idx += 256) {
            const int n = idx / k8, c = (idx - n * k8) * 8;
            u32x4v v = u32x4v{0u, 0u, 0u, 0u};
            if (c < Cin) {
                int t = t0 + n;
                t = t < a.T ? t : a.T - 1;
                const int b = t / (H * W), r = t - b * (H * W), y = r / W, x = r - y * W;
                v = *reinterpret_cast<const u32x4v*>(a.a + b * a.asb + y * a.asy + x * a.asx + c);
            }
            *reinterpret_cast<u32x4v*>(AT + n * PI + c) = v;
        }
    }

    // the accumulators start from res + b
    f32x4v acc[NTW][4];
    {
        const short* rc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            int t = t0 + mt * 16 + li;
            t = t < a.T ? t : a.T - 1;
            const int b = t / (H * W), r = t - b * (H * W), y = r / W, x = r - y * W;
            rc[mt] = a.res + b * a.rsb + y * a.rsy + x * a.rsx;
        }
#pragma unroll
        for (int c = 0; c < NTW; ++c) {
            const int ct = wave + 4 * c;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[c][mt] = f32x4v{0.f, 0.f, 0.f, 0.f};
            if (ct < nt) {
                const int ch = ct * 16 + 4 * q4;
                const f32x4v bb = *reinterpret_cast<const f32x4v*>(a.b + ch);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const bf16x4 v = ld4(rc[mt] + ch);
                    acc[c][mt] = f32x4v{bf2f(v[0]) + bb[0], bf2f(v[1]) + bb[1], bf2f(v[2]) + bb[2], bf2f(v[3]) + bb[3]};
                }
            }
        }
    }
    __syncthreads();

#pragma unroll
    for (int c = 0; c < NTW; ++c) {
        const int ct = wave + 4 * c;
        if (ct < nt) {
            const short* wr = a.w + (int64_t)(ct * 16 + li) * KP + 8 * q4;
#pragma unroll
            for (int kk = 0; kk < 2 * KS2; ++kk) {
                if (kk < ks) {
                    const bf16x8 wf = ld8(wr + kk * 32);
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
                        acc[c][mt] = mma32(wf, ld8(AT + (mt * 16 + li) * PI + kk * 32 + 8 * q4), acc[c][mt]);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NTW; ++c) {
        const int ct = wave + 4 * c;
        if (ct < nt) {
            const int ch = ct * 16 + 4 * q4;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                st4(AT + (mt * 16 + li) * PI + ch, acc[c][mt][0], acc[c][mt][1], acc[c][mt][2], acc[c][mt][3]);
        }
    }
    __syncthreads();
    store_tile(AT, PI, a.out, Cout, t0, a.T, tid);
}

bool aligned(const void* p, uintptr_t n) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// the rules of a strided (B, H, W, C) bf16 view: channel stride 1, the others non-negative multiples of 8, tokens apart
int view_check(int64_t sb, int64_t sy, int64_t sx, int64_t sc, int C)
{
    if (sc != 1) return CREAM_ERR_CHANNEL_STRIDE;
    if (sb < 0 || sy < 0 || sx < 0 || sb % 8 || sy % 8 || sx % 8 || sx < C) return CREAM_ERR_BAD_STRIDE;
    return CREAM_OK;
}

int map_check(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1) return CREAM_ERR_BAD_SHAPE;
    if ((int64_t)B * H * W > 0x7fffffffLL - TM) return CREAM_ERR_TOO_LARGE;
    return CREAM_OK;
}

int dw_check(const cream_evit_dwffn_desc* d)
{
    if (!d) return CREAM_ERR_BAD_ARG;
    if (d->C < 16 || d->C > 384 || d->C % 16 || d->Ch < 32 || d->Ch > 768 || d->Ch % 32) return CREAM_ERR_BAD_SHAPE;
    if (int rc = map_check(d->B, d->H, d->W)) return rc;
    if (!aligned(d->x, 16) || !aligned(d->w1, 16) || !aligned(d->w2, 16) || !aligned(d->out, 16)) return CREAM_ERR_BAD_ARG;
    if (!aligned(d->taps, 16) || !aligned(d->dwb, 16) || !aligned(d->b1, 16) || !aligned(d->b2, 16)) return CREAM_ERR_BAD_ARG;
    return view_check(d->xsb, d->xsy, d->xsx, d->xsc, d->C);
}

int pw_check(const cream_evit_pw_desc* d)
{
    if (!d) return CREAM_ERR_BAD_ARG;
    if (d->Cin < 16 || d->Cin > 384 || d->Cin % 16 || d->Cout < 16 || d->Cout > 384 || d->Cout % 16) return CREAM_ERR_BAD_SHAPE;
    if (int rc = map_check(d->B, d->H, d->W)) return rc;
    if (!aligned(d->a, 16) || !aligned(d->res, 16) || !aligned(d->w, 16) || !aligned(d->b, 16) || !aligned(d->out, 16))
        return CREAM_ERR_BAD_ARG;
    if (int rc = view_check(d->asb, d->asy, d->asx, d->asc, d->Cin)) return rc;
    return view_check(d->rsb, d->rsy, d->rsx, d->rsc, d->Cout);
}

}  // namespace

extern "C" {

int cream_evit_dwffn_check(const cream_evit_dwffn_desc* d) { return dw_check(d); }

int cream_evit_dwffn_fwd(const cream_evit_dwffn_desc* d, void* stream)
{
    const int rc = dw_check(d);
    if (rc) return rc;
    DwArgs a{};
    a.x = static_cast<const short*>(d->x);
    a.xsb = d->xsb; a.xsy = d->xsy; a.xsx = d->xsx;
    a.taps = d->taps; a.dwb = d->dwb;
    a.w1 = static_cast<const short*>(d->w1); a.b1 = d->b1;
    a.w2 = static_cast<const short*>(d->w2); a.b2 = d->b2;
    a.out = static_cast<short*>(d->out);
    a.H = d->H; a.W = d->W; a.C = d->C; a.Ch = d->Ch; a.KP = (d->C + 31) / 32 * 32;
    a.T = d->B * d->H * d->W;
    const dim3 grid((unsigned)((a.T + TM - 1) / TM)), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch ((d->C + 63) / 64) {
        case 1: hipLaunchKernelGGL(evit_dwffn_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(evit_dwffn_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(evit_dwffn_kernel<3>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(evit_dwffn_kernel<4>, grid, block, 0, st, a); break;
        case 5: hipLaunchKernelGGL(evit_dwffn_kernel<5>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(evit_dwffn_kernel<6>, grid, block, 0, st, a); break;
    }
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int cream_evit_pw_residual_check(const cream_evit_pw_desc* d) { return pw_check(d); }

int cream_evit_pw_residual_fwd(const cream_evit_pw_desc* d, void* stream)
{
    const int rc = pw_check(d);
    if (rc) return rc;
    PwArgs a{};
    a.a = static_cast<const short*>(d->a);
    a.asb = d->asb; a.asy = d->asy; a.asx = d->asx;
    a.res = static_cast<const short*>(d->res);
    a.rsb = d->rsb; a.rsy = d->rsy; a.rsx = d->rsx;
    a.w = static_cast<const short*>(d->w); a.b = d->b;
    a.out = static_cast<short*>(d->out);
    a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout; a.KP = (d->Cin + 31) / 32 * 32;
    a.T = d->B * d->H * d->W;
    const dim3 grid((unsigned)((a.T + TM - 1) / TM)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const int cm = d->Cin > d->Cout ? d->Cin : d->Cout;
    switch ((cm + 63) / 64) {
        case 1: hipLaunchKernelGGL(evit_pw_kernel<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(evit_pw_kernel<2>, grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL(evit_pw_kernel<3>, grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL(evit_pw_kernel<4>, grid, block, 0, st, a); break;
        case 5: hipLaunchKernelGGL(evit_pw_kernel<5>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(evit_pw_kernel<6>, grid, block, 0, st, a); break;
    }
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

}  // extern "C"

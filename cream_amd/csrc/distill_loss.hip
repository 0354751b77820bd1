// distill_loss.hip — the two relation losses of the Mini-Swin distillation step (MiniViT/Mini-Swin/main.py:39-57 and :66-77),
// each with its input gradient in the same pass, for gfx950 (MI355X).  Both reduce an N^2-sized intermediate that never has to
// exist in HBM.
//
// 1. Relation loss.  Per window of N = w*w <= 64 tokens, per channel group g of Ar and per ordered pair (i, j) of {q, k, v}:
//        A_s = X_i X_j^T / sqrt(Cs/Ar)   (student)        A_t = Y_i Y_j^T / sqrt(Ct/Ar)   (teacher)       both N x N
//        loss += sum_rows -softmax(A_t) . log_softmax(A_s) = sum_rows (lse(A_s) - softmax(A_t) . A_s)
//    and, with G_ij = softmax(A_s) - softmax(A_t):  dX_i += s G_ij X_j,  dX_j += s G_ij^T X_i,  s = coef / sqrt(Cs/Ar).
//    Each side is addressed through its own window geometry (cream_window_attn's: local token (iy, ix) of window (wy, wx) is map
//    token ((wy w + iy + shift) mod Hs, (wx w + ix + shift) mod Ws)), so the student can be the packed projection of the
//    unshifted map and the teacher a batch of partitioned windows, or the other way round.
//    One workgroup (4 waves) per (window, group) item of a persistent grid.  Phase 1: the 18 units (pair, 32-query tile) go
//    round the waves; a unit streams the contraction depth from global memory in steps of 32 channels (swapped product of
//    attn_common.hpp: a lane holds 32 keys of ONE own query, both key tiles of both sides in registers), does the two row
//    softmaxes in registers and leaves G_ij as bf16 in LDS, row-major and transposed.  Phase 2: per 32-channel chunk the
//    workgroup stages X_q^T, X_k^T, X_v^T in LDS and every (target a, token tile) unit contracts its six terms
//    sum_b (G_ab + G_ba^T) X_b over the 3 x 64 tokens into one accumulator tile, which is stored once as bf16.
// 2. Hidden relation loss.  S^ = normalize(S), T^ = normalize(T) row-wise (x / max(|x|, 1e-12), norms in fp32),
//        D = S^ S^^T - T^ T^^T  (L x L per image),  loss = coef sum D^2,  dS^_i = 4 coef sum_j D_ij S^_j  (D is symmetric),
//        dS = (g - S^ (S^ . g)) / max(|S|, 1e-12).
//    Three launches: rows -> bf16 unit rows (zero-padded to a multiple of 32 channels) and 1 / max(|x|, eps);  the tile kernel:
//    one workgroup per (image, 64-row tile, 128-channel chunk) walks the 64-column tiles, forms D on the matrix cores (the
//    teacher's product enters the same accumulator with a negated operand), adds D^2 (chunk 0 only) and contracts the bf16 D
//    tile from LDS with the staged S^_j^T into g;  the row epilogue applies the normalisation's backward in fp32 and writes the
//    gradient once in the input's dtype.  The scratch is O(L C); the (L, L) matrix stays on chip.
// No atomics anywhere: every workgroup writes one fp32 partial of the loss (summed in a fixed order inside the workgroup), the
// caller sums the partials; every gradient element has one writer.  Reruns are bit-identical.
#include <hip/hip_runtime.h>
#include <hip/hip_bfloat16.h>
#include <math.h>
#include <stdint.h>

#include "attn_lane.hpp"
#include "cream_amd.h"
#include "cu_budget.hpp"

namespace {
using namespace cream;

constexpr int GP = 64;                 // pitch (bf16) of the G matrices: 64 x 64, read once per chunk and unit
constexpr int XP = 72;                 // pitch (bf16) of the transposed [32 channels][64 tokens] chunks
constexpr int DP = 72;                 // pitch (bf16) of the hidden kernel's D tile and S^_j^T chunk

__device__ __forceinline__ float xor32(float v) { return __shfl_xor(v, 32); }

// sum of the workgroup's 256 per-thread values in a fixed order (thread 0 walks them); `red` = 256 floats of LDS
__device__ __forceinline__ void block_partial(float* red, float v, float* dst, float mul) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < 256; ++i) s += red[i];
        *dst = s * mul;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// relation loss
// ---------------------------------------------------------------------------------------------------------------------------
struct Side {
    const short* x[3];
    int64_t sb, sn;
    int Hs, Ws, w, shift, nWx, nW, d;
    float scale;                       // 1 / sqrt(d)
};
struct RArgs {
    Side s, t;
    int N, items, Ar, want_grad;
    float coef;
    float* part;
    short* dx[3];
    int64_t dsb, dsn;
};
struct RLds {
    int off, g, gt, xt, total;         // off: 3 x 64 int64 (student, teacher, gradient offsets); red shares xt
    __host__ __device__ RLds(bool grad) {
        off = 0;
        g = off + 3 * 64 * 8;
        gt = g + (grad ? 9 * 64 * GP * 2 : 0);
        xt = gt + (grad ? 9 * 64 * GP * 2 : 0);
        total = xt + (grad ? 3 * 32 * XP * 2 : 1024);
    }
};

__device__ __forceinline__ int64_t window_token(const Side& sd, int64_t sb, int64_t sn, int win, int i) {
    const int iy = i / sd.w, ix = i - iy * sd.w;
    const int b = win / sd.nW, wi = win - b * sd.nW;
    const int wy = wi / sd.nWx, wx = wi - wy * sd.nWx;
    const int y = (wy * sd.w + iy + sd.shift) % sd.Hs, x = (wx * sd.w + ix + sd.shift) % sd.Ws;
    return (int64_t)b * sb + (int64_t)(y * sd.Ws + x) * sn;
}

// both 32-key tiles of A^T (keys x own queries) of one side for pair (i, j): the contraction streamed from global memory
__device__ __forceinline__ void pair_logits(f32x16 (&acc)[2], const Side& sd, const int64_t* off, int i, int j, int qt, int lane) {
    const int c32 = lane & 31, g = lane >> 5;
    const short* own = sd.x[i] + off[qt * 32 + c32] + g * 8;
    const short* k0 = sd.x[j] + off[c32] + g * 8;
    const short* k1 = sd.x[j] + off[32 + c32] + g * 8;
    acc[0] = f32x16{};
    acc[1] = f32x16{};
    for (int kk = 0; kk < sd.d; kk += 32) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const F b = TT::load(own + kk + ks * 16);
            acc[0] = TT::mma(TT::load(k0 + kk + ks * 16), b, acc[0]);
            acc[1] = TT::mma(TT::load(k1 + kk + ks * 16), b, acc[1]);
        }
    }
}

// max and log-sum-exp pieces of this lane's query row: 32 keys here, the other 32 in lane ^ 32
__device__ __forceinline__ void row_softmax(float (&p)[32], float& lse, const f32x16 (&acc)[2], float scale, int N, int g) {
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const int j = (e >> 4) * 32 + acc_row(e & 15, g);
        p[e] = acc[e >> 4][e & 15] * scale;
        if (j < N) m = fmaxf(m, p[e]);
    }
    m = fmaxf(m, xor32(m));
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
        const int j = (e >> 4) * 32 + acc_row(e & 15, g);
        p[e] = j < N ? expf(p[e] - m) : 0.f;
        sum += p[e];
    }
    sum += xor32(sum);
    const float inv = 1.f / sum;
#pragma unroll
    for (int e = 0; e < 32; ++e) p[e] *= inv;
    lse = m + logf(sum);
}

__global__ __launch_bounds__(256) void relation_loss_kernel(const RArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const RLds L(a.want_grad != 0);
    int64_t* off = reinterpret_cast<int64_t*>(smem + L.off);
    short* G = reinterpret_cast<short*>(smem + L.g);
    short* GT = reinterpret_cast<short*>(smem + L.gt);
    short* XT = reinterpret_cast<short*>(smem + L.xt);
    float loss = 0.f;

    for (int item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int win = item / a.Ar, grp = item - win * a.Ar;
        __syncthreads();                               // the previous item's readers are done
        if (threadIdx.x < 192) {
            const int which = threadIdx.x >> 6;
            const int i = min((int)threadIdx.x & 63, a.N - 1);      // padded tokens repeat the last real one (finite, masked)
            const Side& sd = which == 1 ? a.t : a.s;
            off[threadIdx.x] = window_token(sd, which == 2 ? a.dsb : sd.sb, which == 2 ? a.dsn : sd.sn, win, i) + (int64_t)grp * sd.d;
        }
        __syncthreads();

        // ---- phase 1: the nine pairs' losses, and G = softmax(A_s) - softmax(A_t) into LDS
        for (int u = wave; u < 18; u += 4) {
            const int p = u >> 1, qt = u & 1, pi = p / 3, pj = p - 3 * pi;
            const int q = qt * 32 + c32;
            f32x16 acc[2];
            float ps[32], pt[32], lse_s, lse_t;
            pair_logits(acc, a.t, off + 64, pi, pj, qt, lane);
            row_softmax(pt, lse_t, acc, a.t.scale, a.N, g);
            pair_logits(acc, a.s, off, pi, pj, qt, lane);
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < 32; ++e) {
                const int j = (e >> 4) * 32 + acc_row(e & 15, g);
                if (j < a.N) dot += pt[e] * (acc[e >> 4][e & 15] * a.s.scale);
            }
            row_softmax(ps, lse_s, acc, a.s.scale, a.N, g);
            dot += xor32(dot);
            if (g == 0 && q < a.N) loss += lse_s - dot;            // sum_j pt = 1
            if (a.want_grad) {
                short* gp = G + (p * 64 + q) * GP;
                short* gtp = GT + p * 64 * GP + q;
#pragma unroll
                for (int e = 0; e < 32; ++e) ps[e] = q < a.N ? ps[e] - pt[e] : 0.f;     // exactly 0 at padded keys
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const int e = t * 16 + 4 * r4, j0 = t * 32 + 8 * r4 + 4 * g;
                        *reinterpret_cast<u32x2v*>(gp + j0) = u32x2v{f2bf_pair(ps[e], ps[e + 1]), f2bf_pair(ps[e + 2], ps[e + 3])};
#pragma unroll
                        for (int x = 0; x < 4; ++x) gtp[(j0 + x) * GP] = f2bf(ps[e + x]);
                    }
            }
        }
        if (!a.want_grad) continue;

        // ---- phase 2: dX_a = s sum_b (G_ab + G_ba^T) X_b, 32 channels at a time
        const float mul = a.coef * a.s.scale;
        for (int c = 0; c < a.s.d; c += 32) {
            __syncthreads();                           // G is complete / the previous chunk's readers are done
            for (int idx = threadIdx.x; idx < 3 * 64 * 4; idx += 256) {
                const int b = idx >> 8, tok = (idx >> 2) & 63, cc = idx & 3;
                const F x = TT::load(a.s.x[b] + off[tok] + c + cc * 8);
                short* dst = XT + (b * 32 + cc * 8) * XP + tok;
#pragma unroll
                for (int e = 0; e < 8; ++e) dst[e * XP] = x[e];
            }
            __syncthreads();
            for (int u = wave; u < 6; u += 4) {
                const int ta = u >> 1, tt = u & 1;
                const int tok = tt * 32 + c32;
                f32x16 acc = {};
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const short* xr = XT + (b * 32 + c32) * XP + g * 8;
                    const short* g1 = G + ((ta * 3 + b) * 64 + tok) * GP + g * 8;       // G_ab[tok][tok']
                    const short* g2 = GT + ((b * 3 + ta) * 64 + tok) * GP + g * 8;      // G_ba[tok'][tok]
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        const F xa = TT::load(xr + ks * 16);
                        acc = TT::mma(xa, TT::load(g1 + ks * 16), acc);
                        acc = TT::mma(xa, TT::load(g2 + ks * 16), acc);
                    }
                }
                if (tok < a.N) {
                    short* op = a.dx[ta] + off[128 + tok] + c;
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4)
                        *reinterpret_cast<u32x2v*>(op + 8 * r4 + 4 * g) =
                            u32x2v{f2bf_pair(acc[4 * r4] * mul, acc[4 * r4 + 1] * mul), f2bf_pair(acc[4 * r4 + 2] * mul, acc[4 * r4 + 3] * mul)};
                }
            }
        }
    }
    block_partial(reinterpret_cast<float*>(XT), loss, a.part + blockIdx.x, a.coef);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

int64_t side_windows(const cream_relation_side* s) { return (int64_t)s->B * (s->Hs / s->w) * (s->Ws / s->w); }

int check_side(const cream_relation_side* s, int Ar, bool shape_only) {
    if (s->B < 0 || s->C < 1 || Ar < 1 || s->C % Ar || (s->C / Ar) % 32) return CREAM_ERR_BAD_ARG;
    if (s->w < 1 || s->w * s->w > 64 || s->Hs < s->w || s->Ws < s->w || s->Hs % s->w || s->Ws % s->w) return CREAM_ERR_BAD_ARG;
    if (s->shift < 0 || s->shift >= s->w) return CREAM_ERR_BAD_ARG;
    if ((int64_t)s->B * s->Hs * s->Ws > (int64_t)1 << 30) return CREAM_ERR_TOO_LARGE;
    if (shape_only) return CREAM_OK;
    if (!s->q || !s->k || !s->v || !aligned16(s->q) || !aligned16(s->k) || !aligned16(s->v)) return CREAM_ERR_BAD_ARG;
    if (s->sb < 0 || s->sn < s->C || s->sb % 8 || s->sn % 8) return CREAM_ERR_BAD_ARG;
    return CREAM_OK;
}
int relation_check_shape(const cream_relation_desc* d) {
    if (!d) return CREAM_ERR_BAD_ARG;
    if (const int rc = check_side(&d->s, d->Ar, true)) return rc;
    if (const int rc = check_side(&d->t, d->Ar, true)) return rc;
    if (d->s.w != d->t.w || side_windows(&d->s) != side_windows(&d->t)) return CREAM_ERR_BAD_ARG;
    if (side_windows(&d->s) * d->Ar > (int64_t)1 << 30) return CREAM_ERR_TOO_LARGE;
    return CREAM_OK;
}
int relation_check(const cream_relation_desc* d) {
    if (const int rc = relation_check_shape(d)) return rc;
    if (const int rc = check_side(&d->s, d->Ar, false)) return rc;
    if (const int rc = check_side(&d->t, d->Ar, false)) return rc;
    if (!d->part || !aligned4(d->part) || d->part_blocks < 1 || !(d->coef == d->coef)) return CREAM_ERR_BAD_ARG;
    if (d->want_grad) {
        if (!d->dq || !d->dk || !d->dv || !aligned8(d->dq) || !aligned8(d->dk) || !aligned8(d->dv)) return CREAM_ERR_BAD_ARG;
        if (d->dsb < 0 || d->dsn < d->s.C || d->dsb % 4 || d->dsn % 4) return CREAM_ERR_BAD_ARG;
    }
    return CREAM_OK;
}
int relation_grid(const cream_relation_desc* d) {
    const int64_t items = side_windows(&d->s) * d->Ar;
    const int64_t cap = (int64_t)cu_count() * (d->want_grad ? 1 : 4);
    return (int)(items < cap ? items : cap);
}
Side to_side(const cream_relation_side* s, int Ar) {
    Side o{};
    o.x[0] = (const short*)s->q; o.x[1] = (const short*)s->k; o.x[2] = (const short*)s->v;
    o.sb = s->sb; o.sn = s->sn;
    o.Hs = s->Hs; o.Ws = s->Ws; o.w = s->w; o.shift = s->shift;
    o.nWx = s->Ws / s->w; o.nW = (s->Hs / s->w) * o.nWx; o.d = s->C / Ar;
    o.scale = (float)(1.0 / sqrt((double)o.d));
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------------
// hidden relation loss
// ---------------------------------------------------------------------------------------------------------------------------
constexpr float NORM_EPS = 1e-12f;
constexpr int HCH = 128;               // channels of g per workgroup of the tile kernel

__device__ __forceinline__ float load_elem(const void* p, int64_t i, int bf16) {
    return bf16 ? bf2f(reinterpret_cast<const short*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
}

// one wave per row: unit row as bf16 (zero-padded to Cp channels) and 1 / max(|x|, eps)
__global__ __launch_bounds__(256) void hidden_rows_kernel(const void* x, int bf16, int64_t rows, int C, int Cp, short* xn, float* rinv) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = load_elem(x, row * C + c, bf16);
        ss += v * v;
    }
    const float ri = 1.f / fmaxf(sqrtf(wave_sum(ss)), NORM_EPS);
    for (int c = lane; c < Cp; c += 64) xn[row * Cp + c] = c < C ? f2bf(load_elem(x, row * C + c, bf16) * ri) : (short)0;
    if (lane == 0) rinv[row] = ri;
}

struct HArgs {
    const short *sn, *tn;              // (B, L, Csp), (B, L, Ctp) unit rows
    float* g;                          // (B, L, Csp) fp32: sum_j D_ij S^_j
    float* part;                       // (B * tiles)
    int B, L, Csp, Ctp, tiles, chunks, want_grad;
    float coef;
};

__device__ __forceinline__ F negated(F x) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (short)(x[e] ^ (short)0x8000);
    return x;
}

__global__ __launch_bounds__(256) void hidden_tiles_kernel(const HArgs a) {
    __shared__ __attribute__((aligned(16))) short Dl[64 * DP];
    __shared__ __attribute__((aligned(16))) short SjT[HCH * DP];
    __shared__ float red[256];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const int chunk = blockIdx.x % a.chunks, it = (blockIdx.x / a.chunks) % a.tiles, b = blockIdx.x / (a.chunks * a.tiles);
    const int ri = wave >> 1, cj = wave & 1;
    const int c0 = chunk * HCH, cw = min(HCH, a.Csp - c0);              // a multiple of 32
    const short* sb = a.sn + (int64_t)b * a.L * a.Csp;
    const short* tb = a.tn + (int64_t)b * a.L * a.Ctp;
    const int i = it * 64 + ri * 32 + c32;                              // this lane's row of D
    const int ic = min(i, a.L - 1);
    const short* si = sb + (int64_t)ic * a.Csp + g * 8;
    const short* ti = tb + (int64_t)ic * a.Ctp + g * 8;
    float sq = 0.f;
    f32x16 acc[2] = {f32x16{}, f32x16{}};                               // g^T tiles: channels c0 + 32 wave.., rows 0..31 | 32..63

    for (int jt = 0; jt < a.tiles; ++jt) {
        const int jr = min(jt * 64 + cj * 32 + c32, a.L - 1);
        const short* sj = sb + (int64_t)jr * a.Csp + g * 8;
        const short* tj = tb + (int64_t)jr * a.Ctp + g * 8;
        f32x16 d = {};
        for (int k = 0; k < a.Csp; k += 16) d = TT::mma(TT::load(sj + k), TT::load(si + k), d);
        for (int k = 0; k < a.Ctp; k += 16) d = TT::mma(TT::load(tj + k), negated(TT::load(ti + k)), d);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jt * 64 + cj * 32 + acc_row(r, g);
            d[r] = (i < a.L && j < a.L) ? d[r] : 0.f;
            sq += d[r] * d[r];
        }
        if (!a.want_grad) continue;
        __syncthreads();                                                // the previous tile's readers are done
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
            *reinterpret_cast<u32x2v*>(Dl + (ri * 32 + c32) * DP + cj * 32 + 8 * r4 + 4 * g) =
                u32x2v{f2bf_pair(d[4 * r4], d[4 * r4 + 1]), f2bf_pair(d[4 * r4 + 2], d[4 * r4 + 3])};
        for (int idx = threadIdx.x; idx < 64 * (cw / 8); idx += 256) {
            const int row = idx / (cw / 8), cc = idx - row * (cw / 8);
            const F x = TT::load(sb + (int64_t)min(jt * 64 + row, a.L - 1) * a.Csp + c0 + cc * 8);
            short* dst = SjT + cc * 8 * DP + row;
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[e * DP] = x[e];
        }
        __syncthreads();
        if (wave * 32 < cw) {
            const short* xr = SjT + (wave * 32 + c32) * DP + g * 8;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const F xa = TT::load(xr + ks * 16);
                acc[0] = TT::mma(xa, TT::load(Dl + c32 * DP + g * 8 + ks * 16), acc[0]);
                acc[1] = TT::mma(xa, TT::load(Dl + (32 + c32) * DP + g * 8 + ks * 16), acc[1]);
            }
        }
    }
    if (a.want_grad && wave * 32 < cw) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int row = it * 64 + t * 32 + c32;
            if (row < a.L) {
                float* op = a.g + ((int64_t)b * a.L + row) * a.Csp + c0 + wave * 32;
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4)
                    *reinterpret_cast<f32x4v*>(op + 8 * r4 + 4 * g) =
                        f32x4v{acc[t][4 * r4], acc[t][4 * r4 + 1], acc[t][4 * r4 + 2], acc[t][4 * r4 + 3]};
            }
        }
    }
    if (chunk == 0) block_partial(red, sq, a.part + (int64_t)b * a.tiles + it, a.coef);
}

// one wave per row: dS = 4 coef (g - S^ (S^ . g)) / max(|S|, eps), S^ from the input in fp32; no projection where the norm is clamped
__global__ __launch_bounds__(256) void hidden_epilogue_kernel(const void* x, int bf16, int64_t rows, int C, int Cp, const float* gsum,
                                                              const float* rinv, float coef4, void* dx) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float ri = rinv[row];
    const bool clamped = ri >= 1.f / NORM_EPS;
    float dot = 0.f;
    for (int c = lane; c < C; c += 64) dot += load_elem(x, row * C + c, bf16) * ri * gsum[row * Cp + c];
    dot = clamped ? 0.f : wave_sum(dot);
    for (int c = lane; c < C; c += 64) {
        const float v = coef4 * (gsum[row * Cp + c] - load_elem(x, row * C + c, bf16) * ri * dot) * ri;
        if (bf16) reinterpret_cast<short*>(dx)[row * C + c] = f2bf(v);
        else reinterpret_cast<float*>(dx)[row * C + c] = v;
    }
}

int pad32(int c) { return (c + 31) / 32 * 32; }

int hidden_check(const cream_hidden_relation_desc* d) {
    if (!d) return CREAM_ERR_BAD_ARG;
    if (d->B < 0 || d->L < 1 || d->Cs < 1 || d->Ct < 1) return CREAM_ERR_BAD_ARG;
    if (d->s_dtype != CREAM_F32 && d->s_dtype != CREAM_BF16) return CREAM_ERR_BAD_DTYPE;
    if (d->t_dtype != CREAM_F32 && d->t_dtype != CREAM_BF16) return CREAM_ERR_BAD_DTYPE;
    if ((int64_t)d->B * d->L > (int64_t)1 << 30 || d->Cs > 8192 || d->Ct > 8192) return CREAM_ERR_TOO_LARGE;
    if (!d->s || !d->t || !d->sn || !d->tn || !d->s_rinv || !d->t_rinv || !d->part) return CREAM_ERR_BAD_ARG;
    if (!aligned4(d->s) || !aligned4(d->t) || !aligned16(d->sn) || !aligned16(d->tn) || !aligned4(d->s_rinv) || !aligned4(d->t_rinv) ||
        !aligned4(d->part))
        return CREAM_ERR_BAD_ARG;
    if (d->want_grad && (!d->g || !d->ds || !aligned16(d->g) || !aligned4(d->ds))) return CREAM_ERR_BAD_ARG;
    return CREAM_OK;
}

}  // namespace

extern "C" {

int cream_relation_loss_check(const cream_relation_desc* d) { return relation_check(d); }

int cream_relation_loss_blocks(const cream_relation_desc* d)
{
    const int rc = relation_check_shape(d);
    if (rc) return rc;
    if (side_windows(&d->s) == 0) return 0;
    return relation_grid(d);
}

int cream_relation_loss(const cream_relation_desc* d, void* stream)
{
    const int rc = relation_check(d);
    if (rc) return rc;
    if (side_windows(&d->s) == 0) return CREAM_OK;
    const int blocks = relation_grid(d);
    if (d->part_blocks != blocks) return CREAM_ERR_BAD_ARG;
    RArgs a{};
    a.s = to_side(&d->s, d->Ar);
    a.t = to_side(&d->t, d->Ar);
    a.N = d->s.w * d->s.w;
    a.items = (int)(side_windows(&d->s) * d->Ar);
    a.Ar = d->Ar;
    a.want_grad = d->want_grad != 0;
    a.coef = d->coef;
    a.part = d->part;
    a.dx[0] = (short*)d->dq; a.dx[1] = (short*)d->dk; a.dx[2] = (short*)d->dv;
    a.dsb = d->dsb; a.dsn = d->dsn;
    const int lds = RLds(a.want_grad != 0).total;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(relation_loss_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
        return CREAM_ERR_LAUNCH;
    hipLaunchKernelGGL(relation_loss_kernel, dim3(blocks), dim3(256), (size_t)lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int cream_hidden_relation_check(const cream_hidden_relation_desc* d) { return hidden_check(d); }

int cream_hidden_relation_padded(int C) { return C < 1 ? CREAM_ERR_BAD_ARG : pad32(C); }

int cream_hidden_relation_parts(int B, int L) { return (B < 0 || L < 1) ? CREAM_ERR_BAD_ARG : B * ((L + 63) / 64); }

int cream_hidden_relation_loss(const cream_hidden_relation_desc* d, void* stream)
{
    const int rc = hidden_check(d);
    if (rc) return rc;
    if (d->B == 0) return CREAM_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rows = (int64_t)d->B * d->L;
    const int Csp = pad32(d->Cs), Ctp = pad32(d->Ct);
    const int rb = (int)((rows + 3) / 4);
    hipLaunchKernelGGL(hidden_rows_kernel, dim3(rb), dim3(256), 0, st, d->s, d->s_dtype == CREAM_BF16, rows, d->Cs, Csp, (short*)d->sn,
                       d->s_rinv);
    hipLaunchKernelGGL(hidden_rows_kernel, dim3(rb), dim3(256), 0, st, d->t, d->t_dtype == CREAM_BF16, rows, d->Ct, Ctp, (short*)d->tn,
                       d->t_rinv);
    HArgs a{};
    a.sn = (const short*)d->sn; a.tn = (const short*)d->tn;
    a.g = d->g; a.part = d->part;
    a.B = d->B; a.L = d->L; a.Csp = Csp; a.Ctp = Ctp;
    a.tiles = (d->L + 63) / 64;
    a.want_grad = d->want_grad != 0;
    a.chunks = a.want_grad ? (Csp + HCH - 1) / HCH : 1;
    a.coef = d->coef;
    const int64_t blocks = (int64_t)d->B * a.tiles * a.chunks;
    if (blocks > (int64_t)1 << 30) return CREAM_ERR_TOO_LARGE;
    hipLaunchKernelGGL(hidden_tiles_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    if (a.want_grad)
        hipLaunchKernelGGL(hidden_epilogue_kernel, dim3(rb), dim3(256), 0, st, d->s, d->s_dtype == CREAM_BF16, rows, d->Cs, Csp, d->g,
                           d->s_rinv, 4.f * d->coef, d->ds);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

}  // extern "C"

// window_attn_mix_large.hip — fused (shifted-)window attention of Mini-Swin WITH the head-mixing linears for windows of 9x9 ..
// 12x12 tokens (64 < N = w*w <= 144), forward and backward, for gfx950 (MI355X): what Mini-Swin-B at 384 (window 12, heads
// 4 / 8 / 16) computes between the qkv and proj linears.  Heads of 32, 1 <= H <= 16, proj_l and proj_w always present.
//
// Semantics, geometry and the backward are those of window_attn.hip:5-39, word for word: S_h = (s q_h).k_h + T[rel, h],
// S'_o = sum_h Wl[o,h] S_h + bl[o] (+ mask in {0, -100}), P = softmax, P'_o = sum_h Ww[o,h] P_h + bw[o], O = P' v; keys past N are
// masked AFTER the first mix and get bw never; the kernels read the packed projection of the UNSHIFTED, UNPARTITIONED map, shift
// and mask_shift are two arguments, nothing is read from an (N, N) matrix.
//
// Shape of the kernels: the work item, the head slots and the exchange of window_attn.hip (a work item is (window, 32-query tile)
// with ALL heads, 4 waves, wave v owns heads v, v + 4, ... (HPW head slots), tiles go through X[h][4][64 lanes][4] fp32 of
// attn_lane.hpp and are mixed on the VALU), with the softmax of window_attn_large.hip: a key row is 3 to 5 tiles, too many to keep
// the mixed logits of every head slot in registers, so the forward makes TWO PASSES over the key tiles.  Pass 1: S tile,
// exchange, mix with Wl, mask, running (max, sum) per own (head, query).  Pass 2: the same again, P = exp(S' - lse), exchange,
// mix with Ww, P' v.  K and V of all heads do not fit in LDS (160 tokens x 16 heads x 64 B x 2), so key tiles stream from
// global memory (L2) per tile, as in window_attn.hip.
//
// Backward, two launches:
//   launch Q (lanes own queries).  Pass A: P and dP = Ww^T (dO . v) tile by tile, delta = sum_j P dP (written out for launch K),
//   d Ww, d bw.  Pass B: the same tiles again, dS' = P (dP - delta), dS = Wl^T dS', dq, d bl, d Wl, and d table gathered from the
//   exchanged dS tiles (thread u, u + 256, u + 512 walks the (i, j) pairs of this (query tile, key tile) at offset u in ascending i).
//   launch K (lanes own keys): dk, dv from lse and delta, the loop of window_attn.hip over 3 to 5 query tiles.
// The grids are persistent (sized from cu_count()); a workgroup of launch Q keeps its share of d table | d Wl | d Ww | d bl | d bw
// in LDS, every entry with one owning thread and a fixed order of items, and writes ONE partial at the end; the caller sums the
// partials.  No global atomics.  lse, delta and the parameter gradients never leave fp32.
//
// LDS at w = 12, H = 16 (bytes): X 65,536, the four waves' staging tiles 10,240, the table 33,856, geometry 2,560; launch Q adds
// its partial, 36,032 (148,224 in all), launch K the window's lse and delta rows, 2 x 10,240 (132,672); the forward has 112,192.
// One workgroup per CU from 5 heads on (registers).  32 heads (the last stage of the 384 model, one window per image) are NOT covered: X
// alone would be 128 KB next to a 68 KB table; the argument check refuses H > 16.
// Code object (gfx950, hipcc -O3, from the kernels' metadata; profiles/NOTES_window_attention_mix_large.md has the listing):
// per head-slot count HPW = ceil(H / 4); every kernel 1 wave per SIMD from HPW = 2 on, LDS dynamic):
//     HPW                                   1                 2                  3                  4
//     fwd     VGPR + AGPR, scratch B/lane   129 +  32,   0    210 +  48,   0     210 +  64,   0     253 +  80,   0
//     bwd_q                                 159 +  32,   0    256 + 136,   0     256 + 205,   0     256 + 256, 404
//     bwd_kv                                151 +  48,   0    256 + 112,   0     256 + 196,   0     256 + 256, 288
// No scratch in the forward.  The backward spills at 13 to 16 heads only (108 and 71 VGPRs): five live tiles per head slot in
// pass B of launch Q (S, dS' / P, dP, dS, dq) and in launch K.  bwd_q at HPW = 2 and 3 spills 4 and 13 VGPRs into AGPR lanes, not
// to memory.  SGPR spills (to VGPR lanes) 36 to 554.
#include <hip/hip_runtime.h>
#include <hip/hip_bfloat16.h>
#include <math.h>
#include <stdint.h>

#include "attn_lane.hpp"
#include "cream_amd.h"
#include "cu_budget.hpp"

namespace {
using namespace cream;

constexpr float LOG2E = 1.4426950408889634f;
constexpr int KP = 40;                 // pitch (bf16) of staged row-major [32][32] tiles (rows 8-byte aligned for the transposing read)
constexpr int WMIN = 9, WMAX = 12;
constexpr int MAXH = 16;               // X = 4 KB per head, HPW <= 4 head slots of registers

struct Args {
    const short *q, *k, *v;
    int64_t sb, sn, sh;
    short* out;                        // (B, L, H, 32)
    float* lse;                        // (B nW, H, NP) of the mixed, masked logits
    const float *tab, *wl, *bl, *ww, *bw;
    int B, H, Hs, Ws, w, shift, ms;
    float scale;
    const short* dout;                 // (B, L, H, 32)
    short *dq, *dk, *dv;
    int64_t dsb, dsn, dsh;
    float* delta;                      // (B nW, H, NP)
    float* part;                       // (grid of launch Q, psize) partials
    int N, NT, NP, NU, nWx, nW, nwin, L, psize;
};

// ---- LDS carve-up (bytes), per launch --------------------------------------------------------------------------------------------
enum Kind { FWD = 0, BWD_Q = 1, BWD_K = 2 };
struct Lds {
    int x, st, tl, geo, acc, lse, dl, total;
    __host__ __device__ Lds(int H, int NP, int NU, int psize, int kind) {
        x = 0;
        st = x + H * 4096;                             // X[h][4][64][4] fp32
        tl = st + 4 * 32 * KP * 2;                     // 4 waves x [32][KP] bf16
        geo = tl + ((NU * H * 4 + 15) & ~15);          // the bias table [u][h] fp32
        acc = geo + 4 * NP * 4;                        // tok | reg | cyx | kc, NP ints each
        lse = acc + (kind == BWD_Q ? (psize * 4 + 15) & ~15 : 0);   // the workgroup's parameter-gradient partial (launch Q)
        dl = lse + (kind == BWD_K ? H * NP * 4 : 0);   // [H][NP] fp32 each (launch K)
        total = dl + (kind == BWD_K ? H * NP * 4 : 0);
    }
};
struct Geo { const int *tok, *reg, *cyx, *kc; };

// tile^T (rows = the 32 tokens of tile t, column = own token) = A rows (global, 32 wide, through the token table) . own^T
__device__ __forceinline__ f32x16 stream_tile(const short* base, int64_t rs, const int* tok, int t, float a_scale, bool scale_a,
                                              const F (&own)[2], int lane) {
    const int c32 = lane & 31, g = lane >> 5;
    const short* rp = base + (int64_t)tok[t * 32 + c32] * rs + g * 8;
    f32x16 s = {};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        F aop = TT::load(rp + ks * 16);
        if (scale_a) aop = scaled(aop, a_scale);
        s = TT::mma(aop, own[ks], s);
    }
    return s;
}
// this wave's private copy of the [32][32] tile t of global rows (for the transposing read), optionally scaled
__device__ __forceinline__ void stage_tile(short* dst, const short* base, int64_t rs, const int* tok, int t, float a_scale,
                                           bool scale_a, int lane) {
    wave_lds_fence();                                  // earlier reads of the buffer by this wave are done
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int row = it * 16 + (lane >> 2), cc = lane & 3;
        F x = TT::load(base + (int64_t)tok[t * 32 + row] * rs + cc * 8);
        if (scale_a) x = scaled(x, a_scale);
        *reinterpret_cast<F*>(dst + row * KP + cc * 8) = x;
    }
    wave_lds_fence();
}
// acc^T (32 x own tokens) += tile^T (32 x 32 streamed) . p (32 streamed x own), p in accumulator layout
__device__ __forceinline__ void rows_product(f32x16& acc, const short* tile, const f32x16& p, int lane) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) acc = TT::mma(load_perm_tr<KP>(tile, 0, s2, lane), TT::from_acc(p, s2), acc);
}

// the lanes' shares of a weight gradient, summed over the wave in a fixed butterfly, into the workgroup's LDS partial
// acc[row h][column own head] — lane 0 of the wave that owns the column is the only writer of the entry
template <int HPW>
__device__ __forceinline__ void cross_accum(float* acc, float (&cross)[4 * HPW][HPW], int H, int wave, int lane) {
#pragma unroll
    for (int h = 0; h < 4 * HPW; ++h)
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const float v = wave_sum(cross[h][s]);
            const int o = wave + 4 * s;
            if (h < H && o < H && lane == 0) acc[h * H + o] += v;
            cross[h][s] = 0.f;
        }
}

// ---- geometry of one window: token offsets, mask regions and coordinates of its NP (padded) local tokens -----------------------
__device__ __forceinline__ void setup_window(int* geo, const Args& a, int win) {
    __syncthreads();                                   // the previous item's readers are done
    if ((int)threadIdx.x < a.NP) {
        const int i = min((int)threadIdx.x, a.N - 1);   // padded tokens repeat the last real one (finite data, never used)
        const int iy = i / a.w, ix = i - iy * a.w;
        const int wi = win % a.nW;
        const int wy = wi / a.nWx, wx = wi - wy * a.nWx;
        const int fy = wy * a.w + iy, fx = wx * a.w + ix;                                  // position in the shifted frame
        const int y = (fy + a.shift) % a.Hs, x = (fx + a.shift) % a.Ws;                    // position in the map
        geo[threadIdx.x] = y * a.Ws + x;
        const int ry = fy < a.Hs - a.w ? 0 : (fy < a.Hs - a.ms ? 1 : 2);
        const int rx = fx < a.Ws - a.w ? 0 : (fx < a.Ws - a.ms ? 1 : 2);
        geo[a.NP + threadIdx.x] = a.ms > 0 ? ry * 3 + rx : 0;
        geo[2 * a.NP + threadIdx.x] = iy | (ix << 8);
        geo[3 * a.NP + threadIdx.x] = iy * (2 * a.w - 1) + ix;
    }
    __syncthreads();
}

// S tiles (+ table bias) of this wave's heads for key tile t, lanes own queries.  rel[r] = table row of (own query, key r).
template <int HPW>
__device__ __forceinline__ void own_scores(f32x16 (&S)[HPW], const Args& a, const short* qp, const short* kp, const float* tl,
                                           const Geo& G, int qtok, int t, const int (&rel)[16], int wave, int lane) {
    const int g = lane >> 5;
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const int h = wave + 4 * s;
        S[s] = f32x16{};
        if (h < a.H) {
            const short* row = qp + (int64_t)qtok * a.sn + (int64_t)h * a.sh + g * 8;
            F qs[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) qs[ks] = scaled(TT::load(row + ks * 16), a.scale);
            S[s] = stream_tile(kp + (int64_t)h * a.sh, a.sn, G.tok, t, 1.f, false, qs, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) S[s][r] += tl[rel[r] * a.H + h];
        }
    }
}
// dP' tiles of this wave's heads for key tile t: dO (own query) . v (keys of tile t)
template <int HPW>
__device__ __forceinline__ void own_dpp(f32x16 (&T)[HPW], const Args& a, const short* dop, int64_t dos, const short* vp, const Geo& G,
                                        int qtok, int t, int wave, int lane) {
    const int g = lane >> 5;
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const int o = wave + 4 * s;
        T[s] = f32x16{};
        if (o < a.H) {
            const short* row = dop + (int64_t)qtok * dos + o * 32 + g * 8;
            F df[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) df[ks] = TT::load(row + ks * 16);
            T[s] = stream_tile(vp + (int64_t)o * a.sh, a.sn, G.tok, t, 1.f, false, df, lane);
        }
    }
}
// the two lanes of a query merge their (max, sum) pairs, lane group 0 first in both, so that both hold the same bits
__device__ __forceinline__ float pair_lse(float m, float l, float mx, float lx, int g) {
    const float m0 = g == 0 ? m : mx, l0 = g == 0 ? l : lx, m1 = g == 0 ? mx : m, l1 = g == 0 ? lx : l;
    const float mm = fmaxf(m0, m1);
    const float ll = l0 * __builtin_amdgcn_exp2f((m0 - mm) * LOG2E) + l1 * __builtin_amdgcn_exp2f((m1 - mm) * LOG2E);
    return mm + __logf(ll);
}

struct Ctx {
    float *X, *tl, *acc, *lse_s, *dl_s;
    short* st;
    int* geo;
    Geo G;
};
__device__ __forceinline__ Ctx carve(unsigned char* smem, const Args& a, int kind, int wave) {
    const Lds L(a.H, a.NP, a.NU, a.psize, kind);
    Ctx c;
    c.X = reinterpret_cast<float*>(smem + L.x);
    c.st = reinterpret_cast<short*>(smem + L.st) + wave * 32 * KP;
    c.tl = reinterpret_cast<float*>(smem + L.tl);
    c.geo = reinterpret_cast<int*>(smem + L.geo);
    c.acc = reinterpret_cast<float*>(smem + L.acc);
    c.lse_s = reinterpret_cast<float*>(smem + L.lse);
    c.dl_s = reinterpret_cast<float*>(smem + L.dl);
    c.G = Geo{c.geo, c.geo + a.NP, c.geo + 2 * a.NP, c.geo + 3 * a.NP};
    return c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------
template <int HPW>
__global__ __launch_bounds__(256) void window_attn_mix_large_fwd_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, FWD, wave);
    for (int i = threadIdx.x; i < a.NU * a.H; i += 256) c.tl[i] = a.tab[i];
    const int relc = 2 * a.w * (a.w - 1);

    for (int item = blockIdx.x; item < a.nwin * a.NT; item += gridDim.x) {
        const int win = item / a.NT, qt = item - win * a.NT, b = win / a.nW;
        setup_window(c.geo, a, win);
        const int qi = qt * 32 + c32;
        const bool qok = qi < a.N;
        const int qtok = c.G.tok[qi], qreg = c.G.reg[qi], qkc = c.G.kc[qi] + relc;
        const short* qp = a.q + (int64_t)b * a.sb;
        const short* kp = a.k + (int64_t)b * a.sb;
        const short* vp = a.v + (int64_t)b * a.sb;

        float bl[HPW], bw[HPW], m[HPW], l[HPW];
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = min(wave + 4 * s, a.H - 1);
            bl[s] = a.bl[o];
            bw[s] = a.bw[o];
            m[s] = -INFINITY;
            l[s] = 0.f;
        }
        f32x16 S[HPW];
        // ---- pass 1: the log-sum-exp of the mixed, masked logits (tile 0 has 16 real keys for both lane groups: m is finite after it)
#pragma unroll 1
        for (int t = 0; t < a.NT; ++t) {
            int rel[16];
            float mk[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = t * 32 + acc_row(r, g);
                rel[r] = qkc - c.G.kc[j];
                mk[r] = j >= a.N ? -INFINITY : (c.G.reg[j] != qreg ? -100.f : 0.f);      // padding keys: masked AFTER proj_l
            }
            own_scores<HPW>(S, a, qp, kp, c.tl, c.G, qtok, t, rel, wave, lane);
            xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
            xchg_mix<HPW, false>(c.X, S, a.wl, a.H, wave, lane);
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                float mn = m[s];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    S[s][r] = S[s][r] + bl[s] + mk[r];
                    mn = fmaxf(mn, S[s][r]);
                }
                float sum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f((S[s][r] - mn) * LOG2E);
                l[s] = l[s] * __builtin_amdgcn_exp2f((m[s] - mn) * LOG2E) + sum;
                m[s] = mn;
            }
        }
        float lse[HPW];
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const float mx = __shfl_xor(m[s], 32), lx = __shfl_xor(l[s], 32);
            lse[s] = pair_lse(m[s], l[s], mx, lx, g);
            const int o = wave + 4 * s;
            if (o < a.H && g == 0) a.lse[((int64_t)win * a.H + o) * a.NP + qi] = lse[s];
        }
        // ---- pass 2: P = exp(S' - lse), P' = proj_w(P), O = P' V -----------------------------------------------------------------
        f32x16 O[HPW];
#pragma unroll
        for (int s = 0; s < HPW; ++s) O[s] = f32x16{};
#pragma unroll 1
        for (int t = 0; t < a.NT; ++t) {
            int rel[16];
            float mk[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = t * 32 + acc_row(r, g);
                rel[r] = qkc - c.G.kc[j];
                mk[r] = j >= a.N ? -INFINITY : (c.G.reg[j] != qreg ? -100.f : 0.f);
            }
            own_scores<HPW>(S, a, qp, kp, c.tl, c.G, qtok, t, rel, wave, lane);
            xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
            xchg_mix<HPW, false>(c.X, S, a.wl, a.H, wave, lane);
#pragma unroll
            for (int s = 0; s < HPW; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r) S[s][r] = __builtin_amdgcn_exp2f((S[s][r] + bl[s] + mk[r] - lse[s]) * LOG2E);
            xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
            xchg_mix<HPW, false>(c.X, S, a.ww, a.H, wave, lane);
#pragma unroll
            for (int s = 0; s < HPW; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r) S[s][r] += t * 32 + acc_row(r, g) < a.N ? bw[s] : 0.f;
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int o = wave + 4 * s;
                if (o < a.H) {
                    stage_tile(c.st, vp + (int64_t)o * a.sh, a.sn, c.G.tok, t, 1.f, false, lane);
                    rows_product(O[s], c.st, S[s], lane);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = wave + 4 * s;
            if (o < a.H && qok) store_row(a.out + (((int64_t)b * a.L + qtok) * a.H + o) * 32, O[s], g, 1.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own queries (launch Q): delta, dq, and the workgroup's partial of dT | dWl | dWw | dbl | dbw
// ---------------------------------------------------------------------------------------------------------------------------
template <int HPW>
__global__ __launch_bounds__(256) void window_attn_mix_large_bwd_q_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, BWD_Q, wave);
    for (int i = threadIdx.x; i < a.NU * a.H; i += 256) c.tl[i] = a.tab[i];
    for (int i = threadIdx.x; i < a.psize; i += 256) c.acc[i] = 0.f;
    float* acc_t = c.acc;                              // [NU][H]
    float* acc_wl = acc_t + a.NU * a.H;                // [H][H]
    float* acc_ww = acc_wl + a.H * a.H;                // [H][H]
    float* acc_bl = acc_ww + a.H * a.H;                // [H]
    float* acc_bw = acc_bl + a.H;                      // [H]
    const int relc = 2 * a.w * (a.w - 1);
    const int W2 = 2 * a.w - 1;
    const int64_t dos = (int64_t)a.H * 32;

    for (int item = blockIdx.x; item < a.nwin * a.NT; item += gridDim.x) {
        const int win = item / a.NT, qt = item - win * a.NT, b = win / a.nW;
        setup_window(c.geo, a, win);
        const int qi = qt * 32 + c32;
        const bool qok = qi < a.N;
        const int qtok = c.G.tok[qi], qreg = c.G.reg[qi], qkc = c.G.kc[qi] + relc;
        const short* qp = a.q + (int64_t)b * a.sb;
        const short* kp = a.k + (int64_t)b * a.sb;
        const short* vp = a.v + (int64_t)b * a.sb;
        const short* dop = a.dout + (int64_t)b * a.L * dos;

        float bl[HPW], lse[HPW], dbw[HPW], dbl[HPW], dl[HPW];
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = min(wave + 4 * s, a.H - 1);
            bl[s] = a.bl[o];
            lse[s] = a.lse[((int64_t)win * a.H + o) * a.NP + qi];
            dbw[s] = 0.f; dbl[s] = 0.f;
        }
        float cross[4 * HPW][HPW];
#pragma unroll
        for (int h = 0; h < 4 * HPW; ++h)
#pragma unroll
            for (int s = 0; s < HPW; ++s) cross[h][s] = 0.f;
        f32x16 P[HPW], S[HPW], T[HPW], U[HPW];

        // ---- pass A: delta = sum_j P dP over the key tiles; dWw, dbw ------------------------------------------------------------
        float d0[HPW], d1[HPW];
#pragma unroll
        for (int s = 0; s < HPW; ++s) { d0[s] = 0.f; d1[s] = 0.f; }
#pragma unroll 1
        for (int t = 0; t < a.NT; ++t) {
            int rel[16];
            float mk[16];
            bool ok[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = t * 32 + acc_row(r, g);
                rel[r] = qkc - c.G.kc[j];
                mk[r] = c.G.reg[j] != qreg ? -100.f : 0.f;
                ok[r] = qok && j < a.N;
            }
            own_scores<HPW>(S, a, qp, kp, c.tl, c.G, qtok, t, rel, wave, lane);
            xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
            xchg_mix<HPW, false>(c.X, S, a.wl, a.H, wave, lane);
#pragma unroll
            for (int s = 0; s < HPW; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    P[s][r] = ok[r] ? __builtin_amdgcn_exp2f((S[s][r] + bl[s] + mk[r] - lse[s]) * LOG2E) : 0.f;
            own_dpp<HPW>(T, a, dop, dos, vp, c.G, qtok, t, wave, lane);
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                float x0 = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) x0 += ok[r] ? T[s][r] : 0.f;
                dbw[s] += x0;
            }
            xchg_put<HPW>(c.X, T, 0, a.H, wave, lane);
            xchg_mix<HPW, true, true>(c.X, U, a.ww, a.H, wave, lane, P, cross);                       // dP; dWw[o][h] += dP'_o P_h
#pragma unroll
            for (int s = 0; s < HPW; ++s)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    d0[s] = __builtin_fmaf(P[s][r], U[s][r], d0[s]);
                    d1[s] = __builtin_fmaf(P[s][r + 1], U[s][r + 1], d1[s]);
                }
        }
        cross_accum<HPW>(acc_ww, cross, a.H, wave, lane);
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            float d = d0[s] + d1[s];
            d += __shfl_xor(d, 32);
            dl[s] = d;
            const int o = wave + 4 * s;
            if (o < a.H && g == 0) a.delta[((int64_t)win * a.H + o) * a.NP + qi] = d;
        }
        // ---- pass B: dS' = P (dP - delta), dS = proj_l^T dS', dWl, dbl, dq, dT ----------------------------------------------------
        f32x16 dq[HPW];
#pragma unroll
        for (int s = 0; s < HPW; ++s) dq[s] = f32x16{};
#pragma unroll 1
        for (int t = 0; t < a.NT; ++t) {
            {
                int rel[16];
                float mk[16];
                bool ok[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = t * 32 + acc_row(r, g);
                    rel[r] = qkc - c.G.kc[j];
                    mk[r] = c.G.reg[j] != qreg ? -100.f : 0.f;
                    ok[r] = qok && j < a.N;
                }
                own_scores<HPW>(S, a, qp, kp, c.tl, c.G, qtok, t, rel, wave, lane);
                xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
                xchg_mix<HPW, false>(c.X, U, a.wl, a.H, wave, lane);
#pragma unroll
                for (int s = 0; s < HPW; ++s)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        P[s][r] = ok[r] ? __builtin_amdgcn_exp2f((U[s][r] + bl[s] + mk[r] - lse[s]) * LOG2E) : 0.f;
            }
            own_dpp<HPW>(T, a, dop, dos, vp, c.G, qtok, t, wave, lane);
            xchg_put<HPW>(c.X, T, 0, a.H, wave, lane);
            xchg_mix<HPW, true>(c.X, U, a.ww, a.H, wave, lane);                                       // dP
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                float sum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    P[s][r] = P[s][r] * (U[s][r] - dl[s]);                                            // dS'
                    sum += P[s][r];
                }
                dbl[s] += sum;
            }
            xchg_put<HPW>(c.X, P, 0, a.H, wave, lane);
            xchg_mix<HPW, true, true>(c.X, U, a.wl, a.H, wave, lane, S, cross);                       // dS; dWl[o][h] += dS'_o S_h
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int h = wave + 4 * s;
                if (h < a.H) {
                    stage_tile(c.st, kp + (int64_t)h * a.sh, a.sn, c.G.tok, t, 1.f, false, lane);
                    rows_product(dq[s], c.st, U[s], lane);
                }
            }
            // dT[u][h] += the dS_h[i][j] of this (query tile, key tile) at offset u, i ascending: thread u, u + 256, u + 512
            xchg_put<HPW>(c.X, U, 0, a.H, wave, lane);
            for (int u = threadIdx.x; u < a.NU; u += 256) {
                const int uy = u / W2;
                const int dy = uy - (a.w - 1), dx = u - uy * W2 - (a.w - 1);
                const int off = dy * a.w + dx;                                  // i - j
                const int lo = max(max(qt * 32, t * 32 + off), 0), hi = min(min(qt * 32 + 32, t * 32 + 32 + off), a.N);
                if (lo >= hi) continue;
                const int y0 = max(max(0, dy), lo / a.w), y1 = min(min(a.w, a.w + dy), (hi - 1) / a.w + 1);
                const int x0 = max(0, dx), x1 = min(a.w, a.w + dx);
                float* ap = acc_t + u * a.H;
                for (int iy = y0; iy < y1; ++iy) {
                    const int r0 = iy * a.w;
                    for (int i = max(r0 + x0, lo); i < min(r0 + x1, hi); ++i) {
                        const int ii = i & 31, jl = (i - off) & 31;
                        const float* xp = c.X + ((jl >> 3) * 64 + ii + 32 * ((jl >> 2) & 1)) * 4 + (jl & 3);
                        for (int x = 0; x < a.H; ++x) ap[x] += xp[x * 1024];
                    }
                }
            }
        }
        cross_accum<HPW>(acc_wl, cross, a.H, wave, lane);
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const float vl = wave_sum(dbl[s]), vw = wave_sum(dbw[s]);
            const int o = wave + 4 * s;
            if (o < a.H && lane == 0) { acc_bl[o] += vl; acc_bw[o] += vw; }
        }
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int h = wave + 4 * s;
            if (h < a.H && qok) store_row(a.dq + (int64_t)b * a.dsb + (int64_t)qtok * a.dsn + (int64_t)h * a.dsh, dq[s], g, a.scale);
        }
    }
    __syncthreads();
    float* part = a.part + (int64_t)blockIdx.x * a.psize;
    for (int i = threadIdx.x; i < a.psize; i += 256) part[i] = c.acc[i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own keys (launch K): dk, dv.  Streams the window's query tiles; lse and delta of its queries through LDS.
// ---------------------------------------------------------------------------------------------------------------------------
template <int HPW>
__global__ __launch_bounds__(256) void window_attn_mix_large_bwd_kv_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, BWD_K, wave);
    for (int i = threadIdx.x; i < a.NU * a.H; i += 256) c.tl[i] = a.tab[i];
    const int relc = 2 * a.w * (a.w - 1);
    const int64_t dos = (int64_t)a.H * 32;

    for (int item = blockIdx.x; item < a.nwin * a.NT; item += gridDim.x) {
        const int win = item / a.NT, kt = item - win * a.NT, b = win / a.nW;
        setup_window(c.geo, a, win);
        for (int i = threadIdx.x; i < a.H * a.NP; i += 256) {
            c.lse_s[i] = a.lse[(int64_t)win * a.H * a.NP + i];
            c.dl_s[i] = a.delta[(int64_t)win * a.H * a.NP + i];
        }
        __syncthreads();
        const int kj = kt * 32 + c32;
        const bool kok = kj < a.N;
        const int ktok = c.G.tok[kj], kreg = c.G.reg[kj], kkc = relc - c.G.kc[kj];
        const short* qp = a.q + (int64_t)b * a.sb;
        const short* kp = a.k + (int64_t)b * a.sb;
        const short* vp = a.v + (int64_t)b * a.sb;
        const short* dop = a.dout + (int64_t)b * a.L * dos;

        float bl[HPW], bw[HPW];
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = min(wave + 4 * s, a.H - 1);
            bl[s] = a.bl[o];
            bw[s] = a.bw[o];
        }
        f32x16 dk[HPW], dv[HPW];
#pragma unroll
        for (int s = 0; s < HPW; ++s) { dk[s] = f32x16{}; dv[s] = f32x16{}; }
        f32x16 S[HPW], P[HPW], T[HPW];
#pragma unroll 1
        for (int t = 0; t < a.NT; ++t) {
            bool ok[16];
            float mk[16];
            int rel[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = t * 32 + acc_row(r, g);
                ok[r] = kok && i < a.N;
                mk[r] = c.G.reg[i] != kreg ? -100.f : 0.f;
                rel[r] = c.G.kc[i] + kkc;
            }
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int h = wave + 4 * s;
                S[s] = f32x16{};
                if (h < a.H) {
                    const short* row = kp + (int64_t)ktok * a.sn + (int64_t)h * a.sh + g * 8;
                    F kf[2];
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) kf[ks] = TT::load(row + ks * 16);
                    S[s] = stream_tile(qp + (int64_t)h * a.sh, a.sn, c.G.tok, t, a.scale, true, kf, lane);
#pragma unroll
                    for (int r = 0; r < 16; ++r) S[s][r] += c.tl[rel[r] * a.H + h];
                }
            }
            xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
            xchg_mix<HPW, false>(c.X, S, a.wl, a.H, wave, lane);
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int o = min(wave + 4 * s, a.H - 1);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    P[s][r] = ok[r] ? __builtin_amdgcn_exp2f((S[s][r] + bl[s] + mk[r] - c.lse_s[o * a.NP + t * 32 + acc_row(r, g)]) * LOG2E)
                                    : 0.f;
            }
            xchg_put<HPW>(c.X, P, 0, a.H, wave, lane);
            xchg_mix<HPW, false>(c.X, S, a.ww, a.H, wave, lane);                              // P'
#pragma unroll
            for (int s = 0; s < HPW; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r) S[s][r] += ok[r] ? bw[s] : 0.f;
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int o = wave + 4 * s;
                T[s] = f32x16{};
                __builtin_amdgcn_sched_barrier(0);     // one head slot at a time: hoisting every slot's loads costs the registers
                if (o < a.H) {
                    stage_tile(c.st, dop + o * 32, dos, c.G.tok, t, 1.f, false, lane);
                    rows_product(dv[s], c.st, S[s], lane);                                // dv_o^T += dO_o^T P'_o^T
                    const short* row = vp + (int64_t)ktok * a.sn + (int64_t)o * a.sh + g * 8;
                    F vf[2];
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) vf[ks] = TT::load(row + ks * 16);
                    T[s] = stream_tile(dop + o * 32, dos, c.G.tok, t, 1.f, false, vf, lane);   // dP'_o
                }
            }
            xchg_put<HPW>(c.X, T, 0, a.H, wave, lane);
            xchg_mix<HPW, true>(c.X, T, a.ww, a.H, wave, lane);                               // dP
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int o = min(wave + 4 * s, a.H - 1);
#pragma unroll
                for (int r = 0; r < 16; ++r) T[s][r] = P[s][r] * (T[s][r] - c.dl_s[o * a.NP + t * 32 + acc_row(r, g)]);   // dS'
            }
            xchg_put<HPW>(c.X, T, 0, a.H, wave, lane);
            xchg_mix<HPW, true>(c.X, T, a.wl, a.H, wave, lane);                               // dS
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int h = wave + 4 * s;
                __builtin_amdgcn_sched_barrier(0);
                if (h < a.H) {
                    stage_tile(c.st, qp + (int64_t)h * a.sh, a.sn, c.G.tok, t, a.scale, true, lane);
                    rows_product(dk[s], c.st, T[s], lane);                                // dk_h^T += (s q_h)^T dS_h^T
                }
            }
        }
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int h = wave + 4 * s;
            if (h < a.H && kok) {
                store_row(a.dk + (int64_t)b * a.dsb + (int64_t)ktok * a.dsn + (int64_t)h * a.dsh, dk[s], g, 1.f);
                store_row(a.dv + (int64_t)b * a.dsb + (int64_t)ktok * a.dsn + (int64_t)h * a.dsh, dv[s], g, 1.f);
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int lds_of(const Args& a, int kind) { return Lds(a.H, a.NP, a.NU, a.psize, kind).total; }
// two workgroups per CU only where both LDS and registers admit them: from 5 heads on (two head slots) every kernel needs more
// than half of the register file (the listing in the header), so a second workgroup could not be resident
int grid_for(const Args& a, int lds) {
    const int per_cu = (lds <= 80 * 1024 && a.H <= 4) ? 2 : 1;
    const int items = a.nwin * a.NT, cap = cu_count() * per_cu;
    return items < cap ? items : cap;
}
template <typename K> int launch(K kern, const Args& a, int blocks, int lds, hipStream_t st) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return CREAM_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), (size_t)lds, st, a);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}
template <int HPW> int run(const Args& a, bool bwd, hipStream_t st) {
    if (!bwd) return launch(window_attn_mix_large_fwd_kernel<HPW>, a, grid_for(a, lds_of(a, FWD)), lds_of(a, FWD), st);
    const int rc = launch(window_attn_mix_large_bwd_q_kernel<HPW>, a, grid_for(a, lds_of(a, BWD_Q)), lds_of(a, BWD_Q), st);
    if (rc) return rc;
    return launch(window_attn_mix_large_bwd_kv_kernel<HPW>, a, grid_for(a, lds_of(a, BWD_K)), lds_of(a, BWD_K), st);
}
int dispatch(const Args& a, bool bwd, hipStream_t st) {
    switch ((a.H + 3) / 4) {
        case 1: return run<1>(a, bwd, st);
        case 2: return run<2>(a, bwd, st);
        case 3: return run<3>(a, bwd, st);
        default: return run<4>(a, bwd, st);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

int psize_of(int H, int w) { return (2 * w - 1) * (2 * w - 1) * H + 2 * H * H + 2 * H; }

// the shape alone (what sizes the grid and the partials)
int check_shape(const cream_window_attn_mix_large_desc* d) {
    if (!d) return CREAM_ERR_BAD_ARG;
    if (!(d->wl && d->bl && d->ww && d->bw)) return CREAM_ERR_BAD_ARG;
    if (d->head_dim != 32 || d->B < 0 || d->H < 1 || d->H > MAXH) return CREAM_ERR_BAD_ARG;
    if (d->w < WMIN || d->w > WMAX || d->Hs < d->w || d->Ws < d->w || d->Hs % d->w || d->Ws % d->w) return CREAM_ERR_BAD_ARG;
    if (d->shift < 0 || d->shift >= d->w || d->mask_shift < 0 || d->mask_shift >= d->w) return CREAM_ERR_BAD_ARG;
    if ((int64_t)d->B * d->Hs * d->Ws > (int64_t)1 << 30) return CREAM_ERR_TOO_LARGE;
    return CREAM_OK;
}

int check(const cream_window_attn_mix_large_desc* d, bool bwd) {
    if (!d || !d->q || !d->k || !d->v || !d->lse || !d->table || (!bwd && !d->out)) return CREAM_ERR_BAD_ARG;
    if (const int rc = check_shape(d)) return rc;
    if (d->sn % 8 || d->sh % 8 || d->sb % 8 || !aligned16(d->q) || !aligned16(d->k) || !aligned16(d->v) || (!bwd && !aligned8(d->out)))
        return CREAM_ERR_BAD_ARG;
    if (!aligned4(d->lse) || !aligned4(d->table) || !(aligned4(d->wl) && aligned4(d->bl) && aligned4(d->ww) && aligned4(d->bw)))
        return CREAM_ERR_BAD_ARG;
    if (bwd) {
        if (!d->dout || !d->dq || !d->dk || !d->dv || !d->delta || !d->part || d->part_blocks < 1) return CREAM_ERR_BAD_ARG;
        if (d->dsn % 4 || d->dsh % 4 || d->dsb % 4 || !aligned16(d->dout)) return CREAM_ERR_BAD_ARG;
        if (!aligned8(d->dq) || !aligned8(d->dk) || !aligned8(d->dv) || !aligned4(d->delta) || !aligned4(d->part)) return CREAM_ERR_BAD_ARG;
    }
    return CREAM_OK;
}

Args to_args(const cream_window_attn_mix_large_desc* d) {
    Args a{};
    a.q = (const short*)d->q; a.k = (const short*)d->k; a.v = (const short*)d->v;
    a.sb = d->sb; a.sn = d->sn; a.sh = d->sh;
    a.out = (short*)d->out; a.lse = d->lse;
    a.tab = d->table; a.wl = d->wl; a.bl = d->bl; a.ww = d->ww; a.bw = d->bw;
    a.B = d->B; a.H = d->H; a.Hs = d->Hs; a.Ws = d->Ws; a.w = d->w; a.shift = d->shift; a.ms = d->mask_shift; a.scale = d->scale;
    a.dout = (const short*)d->dout;
    a.dq = (short*)d->dq; a.dk = (short*)d->dk; a.dv = (short*)d->dv;
    a.dsb = d->dsb; a.dsn = d->dsn; a.dsh = d->dsh;
    a.delta = d->delta; a.part = d->part;
    a.N = d->w * d->w; a.NT = (a.N + 31) / 32; a.NP = a.NT * 32; a.NU = (2 * d->w - 1) * (2 * d->w - 1);
    a.nWx = d->Ws / d->w; a.nW = (d->Hs / d->w) * a.nWx; a.nwin = d->B * a.nW; a.L = d->Hs * d->Ws;
    a.psize = psize_of(d->H, d->w);
    return a;
}

}  // namespace

extern "C" {

int cream_window_attn_mix_large_check(const cream_window_attn_mix_large_desc* d, int backward) { return check(d, backward != 0); }

int cream_window_attn_mix_large_part_size(int H, int w)
{
    if (H < 1 || H > MAXH || w < WMIN || w > WMAX) return CREAM_ERR_BAD_ARG;
    return psize_of(H, w);
}

int cream_window_attn_mix_large_blocks(const cream_window_attn_mix_large_desc* d)
{
    const int rc = check_shape(d);
    if (rc) return rc;
    const Args a = to_args(d);
    if (a.nwin == 0) return 0;
    return grid_for(a, lds_of(a, BWD_Q));
}

int cream_window_attn_mix_large_fwd(const cream_window_attn_mix_large_desc* d, void* stream)
{
    const int rc = check(d, false);
    if (rc) return rc;
    if (d->B == 0) return CREAM_OK;
    return dispatch(to_args(d), false, (hipStream_t)stream);
}

int cream_window_attn_mix_large_bwd(const cream_window_attn_mix_large_desc* d, void* stream)
{
    const int rc = check(d, true);
    if (rc) return rc;
    if (d->B == 0) return CREAM_OK;
    const Args a = to_args(d);
    if (d->part_blocks != grid_for(a, lds_of(a, BWD_Q))) return CREAM_ERR_BAD_ARG;
    return dispatch(a, true, (hipStream_t)stream);
}

}  // extern "C"

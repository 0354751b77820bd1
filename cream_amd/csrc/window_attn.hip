// window_attn.hip — fused (shifted-)window attention of Swin / Mini-Swin, forward and backward, for gfx950 (MI355X):
// relative-position bias TABLE, the two head-mixing linears of MiniViT (proj_l before the softmax, proj_w after it, both with
// bias), the -100 shift mask, and the whole window geometry (cyclic shift, partition, reverse) in the addressing.
//
// Reference semantics (MiniViT/Mini-Swin/models/swin_transformer_minivit.py:109-147 and :284-323), per window of N = w*w tokens,
// H heads of 32, s = scale, T = relative_position_bias_table ((2w-1)^2, H), Wl, bl = proj_l, Ww, bw = proj_w ([out][in] fp32):
//     S_h[i,j]  = (s q_h,i).k_h,j + T[rel(i,j), h]
//     S'_o      = sum_h Wl[o,h] S_h + bl[o]   (+ mask[i,j] in {0, -100})
//     P_o       = softmax_j(S'_o)
//     P'_o      = sum_h Ww[o,h] P_h + bw[o]
//     O_o,i     = sum_j P'_o[i,j] v_o,j
// Without the head transforms (wl == NULL) the mixes are the identity and the heads are independent.
//
// Geometry.  The kernels read the packed projection of the UNSHIFTED, UNPARTITIONED map and write the output in the same token
// order: local token (iy, ix) of window (wy, wx) is map token ((wy w + iy + shift) mod Hs, (wx w + ix + shift) mod Ws) — what
// roll(-shift), window_partition, window_reverse and roll(+shift) amount to.  rel(i,j) = (iy-jy+w-1)(2w-1) + (ix-jx+w-1), and the
// mask compares the region ids of the two tokens' positions in the shifted frame, three slices per axis: [0, Hs-w),
// [Hs-w, Hs-m), [Hs-m, Hs) with m = mask_shift.  (The reference applies a block's mask whether or not the repeat rolls the map,
// so the roll and the mask are separate arguments.)  Nothing is read from an (N, N) index or mask matrix.
//
// Shape of the kernels (all heads in one workgroup and the head exchange of attn_lane.hpp, as in mini_attn.hip, with whole key
// rows on chip).  N <= 64, so a window's keys are at most two 32-wide tiles.  A work item is (window, 32-query tile) with ALL heads; one workgroup = 4 waves, wave w owns heads w, w+4, ...
// (HPW head slots).  A wave computes the 32 x 32 tiles of its heads with the swapped product of attn_common.hpp (a lane holds 16
// keys of ONE own query), the waves exchange tiles through the fp32 LDS buffer X[h][4][64 lanes][4] and every wave mixes the
// tiles of all heads into those of its own heads on the VALU.  Both key tiles of the mixed logits stay in registers, so the
// softmax needs no second pass over the keys.  Without head transforms HPW = 1 and the kernels loop over groups of four heads.
// Keys past N are masked AFTER the first mix (the mixing weights may be negative); their P is exactly 0 before proj_w, and bw is
// added to real keys only.
//
// Backward, with dP'_o[i,j] = dO_o,i . v_o,j:
//     dP_h = sum_o Ww[o,h] dP'_o      delta_h[i] = sum_j P_h dP_h       dS'_h = P_h (dP_h - delta_h)
//     dS_h = sum_o Wl[o,h] dS'_o      dT[u,h] = sum_{rel(i,j)=u} dS_h[i,j]
//     dq_h = s dS_h k_h    dk_h = dS_h^T (s q_h)    dv_o = P'_o^T dO_o
//     dWl[o,h] = sum dS'_o S_h   dbl[o] = sum dS'_o   dWw[o,h] = sum dP'_o P_h   dbw[o] = sum dP'_o   (real (i,j) only)
//   launch Q (lanes own queries): delta (in registers, written out for launch K), dq, and the parameter gradients;
//   launch K (lanes own keys): dk, dv from lse and delta.
// The grids are persistent (sized from cu_count()): a workgroup keeps its share of dT, dWl, dbl, dWw, dbw in LDS, every entry
// with one owning thread and a fixed order of items, and writes ONE partial at the end; the caller sums the partials.  dT is a
// gather from the exchanged dS tiles (thread u walks the (i, j) pairs at offset u), not a scatter.  No global atomics.
#include <hip/hip_runtime.h>
#include <hip/hip_bfloat16.h>
#include <stdint.h>

#include "attn_lane.hpp"
#include "cream_amd.h"
#include "cu_budget.hpp"

namespace {
using namespace cream;

constexpr float LOG2E = 1.4426950408889634f;
constexpr int KP = 40;                 // pitch (bf16) of staged row-major [32][32] tiles (rows 8-byte aligned for the transposing read)
constexpr int MAXH = 32;               // without head transforms
constexpr int MAXH_MIXED = 16;         // with head transforms: X = 4 KB per head, HPW <= 4 head slots of registers

struct Args {
    const short *q, *k, *v;
    int64_t sb, sn, sh;
    short* out;                        // (B, L, H, 32)
    float* lse;                        // (B nW, H, 64) of the mixed, masked logits
    const float *tab, *wl, *bl, *ww, *bw;
    int B, H, Hs, Ws, w, shift, ms;
    float scale;
    const short* dout;                 // (B, L, H, 32)
    short *dq, *dk, *dv;
    int64_t dsb, dsn, dsh;
    float* delta;                      // (B nW, H, 64)
    float* part;                       // (grid, psize) partials of launch Q
    int N, NT, NU, nWx, nW, nwin, L, psize;
};

// ---- LDS carve-up (bytes), the same for every launch ---------------------------------------------------------------------------
struct Lds {
    int x, st, tl, acc, geo, lse, dl, total;
    __host__ __device__ Lds(int H, bool mix, int NU, int psize) {
        x = 0;
        st = x + (mix ? H : 4) * 4096;                 // X[h][4][64][4] fp32
        tl = st + 4 * 32 * KP * 2;                     // 4 waves x [32][KP] bf16
        acc = tl + ((NU * H * 4 + 15) & ~15);          // the bias table [u][h] fp32
        geo = acc + ((psize * 4 + 15) & ~15);          // the workgroup's parameter-gradient partial (launch Q)
        lse = geo + 4 * 64 * 4;                        // tok | reg | cyx | kc, 64 ints each
        dl = lse + H * 64 * 4;                         // [H][64] fp32 each (launch K)
        total = dl + H * 64 * 4;
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
    for (int s2 = 0; s2 < 2; ++s2) acc = TT::mma(load_perm_tr(tile, KP, 0, s2, lane), TT::from_acc(p, s2), acc);
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

// ---- geometry of one window: token offsets, mask regions and coordinates of its 64 (padded) local tokens ----------------------
__device__ __forceinline__ void setup_window(int* geo, const Args& a, int win) {
    __syncthreads();                                   // the previous item's readers are done
    if (threadIdx.x < 64) {
        const int i = min((int)threadIdx.x, a.N - 1);   // padded tokens repeat the last real one (finite data, never used)
        const int iy = i / a.w, ix = i - iy * a.w;
        const int wi = win % a.nW;
        const int wy = wi / a.nWx, wx = wi - wy * a.nWx;
        const int fy = wy * a.w + iy, fx = wx * a.w + ix;                                  // position in the shifted frame
        const int y = (fy + a.shift) % a.Hs, x = (fx + a.shift) % a.Ws;                    // position in the map
        geo[threadIdx.x] = y * a.Ws + x;
        const int ry = fy < a.Hs - a.w ? 0 : (fy < a.Hs - a.ms ? 1 : 2);
        const int rx = fx < a.Ws - a.w ? 0 : (fx < a.Ws - a.ms ? 1 : 2);
        geo[64 + threadIdx.x] = a.ms > 0 ? ry * 3 + rx : 0;
        geo[128 + threadIdx.x] = iy | (ix << 8);
        geo[192 + threadIdx.x] = iy * (2 * a.w - 1) + ix;
    }
    __syncthreads();
}

// S tiles (+ table bias) of this wave's heads for key tile t, lanes own queries.  rel[r] = table row of (own query, key r).
template <int HPW>
__device__ __forceinline__ void own_scores(f32x16 (&S)[HPW], const Args& a, const short* qp, const short* kp, const float* tl,
                                           const Geo& G, int qtok, int t, int hb, const int (&rel)[16], int wave, int lane) {
    const int g = lane >> 5;
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const int h = hb + wave + 4 * s;
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

struct Ctx {
    float *X, *tl, *acc, *lse_s, *dl_s;
    short* st;
    int* geo;
    Geo G;
};
__device__ __forceinline__ Ctx carve(unsigned char* smem, const Args& a, bool mix, int wave) {
    const Lds L(a.H, mix, a.NU, a.psize);
    Ctx c;
    c.X = reinterpret_cast<float*>(smem + L.x);
    c.st = reinterpret_cast<short*>(smem + L.st) + wave * 32 * KP;
    c.tl = reinterpret_cast<float*>(smem + L.tl);
    c.acc = reinterpret_cast<float*>(smem + L.acc);
    c.geo = reinterpret_cast<int*>(smem + L.geo);
    c.lse_s = reinterpret_cast<float*>(smem + L.lse);
    c.dl_s = reinterpret_cast<float*>(smem + L.dl);
    c.G = Geo{c.geo, c.geo + 64, c.geo + 128, c.geo + 192};
    return c;
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------
template <int HPW, bool MIX>
__global__ __launch_bounds__(256) void window_attn_fwd_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, MIX, wave);
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

        for (int hb = 0; hb < (MIX ? 1 : a.H); hb += 4) {
            float bl[HPW], bw[HPW];
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int o = min(hb + wave + 4 * s, a.H - 1);
                bl[s] = MIX ? a.bl[o] : 0.f;
                bw[s] = MIX ? a.bw[o] : 0.f;
            }
            f32x16 Sp[2][HPW], S[HPW];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t < a.NT) {
                    int rel[16];
                    float mk[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int j = t * 32 + acc_row(r, g);
                        rel[r] = qkc - c.G.kc[j];
                        mk[r] = j >= a.N ? -INFINITY : (c.G.reg[j] != qreg ? -100.f : 0.f);
                    }
                    own_scores<HPW>(S, a, qp, kp, c.tl, c.G, qtok, t, hb, rel, wave, lane);
                    if constexpr (MIX) {
                        xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
                        xchg_mix<HPW, false>(c.X, S, a.wl, a.H, wave, lane);
                    }
#pragma unroll
                    for (int s = 0; s < HPW; ++s)
#pragma unroll
                        for (int r = 0; r < 16; ++r) Sp[t][s][r] = S[s][r] + bl[s] + mk[r];      // padding keys: masked AFTER proj_l
                } else {
#pragma unroll
                    for (int s = 0; s < HPW; ++s)
#pragma unroll
                        for (int r = 0; r < 16; ++r) Sp[t][s][r] = -INFINITY;
                }
            }
            // ---- softmax over the whole key row (two tiles x two lane groups) ----------------------------------------------
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                float m = -INFINITY;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) m = fmaxf(m, Sp[t][s][r]);
                m = fmaxf(m, __shfl_xor(m, 32));                                           // finite: key 0 is real
                float l = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        Sp[t][s][r] = __builtin_amdgcn_exp2f((Sp[t][s][r] - m) * LOG2E);
                        l += Sp[t][s][r];
                    }
                l += __shfl_xor(l, 32);
                const float inv = 1.f / l;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) Sp[t][s][r] *= inv;
                const int o = hb + wave + 4 * s;
                if (o < a.H && g == 0) a.lse[((int64_t)win * a.H + o) * 64 + qi] = m + __logf(l);
            }
            // ---- P' = proj_w(P), O = P' V -----------------------------------------------------------------------------------
            f32x16 O[HPW];
#pragma unroll
            for (int s = 0; s < HPW; ++s) O[s] = f32x16{};
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t < a.NT) {
#pragma unroll
                    for (int s = 0; s < HPW; ++s) S[s] = Sp[t][s];
                    if constexpr (MIX) {
                        xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
                        xchg_mix<HPW, false>(c.X, S, a.ww, a.H, wave, lane);
#pragma unroll
                        for (int s = 0; s < HPW; ++s)
#pragma unroll
                            for (int r = 0; r < 16; ++r) S[s][r] += t * 32 + acc_row(r, g) < a.N ? bw[s] : 0.f;
                    }
#pragma unroll
                    for (int s = 0; s < HPW; ++s) {
                        const int o = hb + wave + 4 * s;
                        if (o < a.H) {
                            stage_tile(c.st, vp + (int64_t)o * a.sh, a.sn, c.G.tok, t, 1.f, false, lane);
                            rows_product(O[s], c.st, S[s], lane);
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int o = hb + wave + 4 * s;
                if (o < a.H && qok) store_row(a.out + (((int64_t)b * a.L + qtok) * a.H + o) * 32, O[s], g, 1.f);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own queries (launch Q): delta, dq, and the workgroup's partial of dT | dWl | dWw | dbl | dbw
// ---------------------------------------------------------------------------------------------------------------------------
template <int HPW, bool MIX>
__global__ __launch_bounds__(256) void window_attn_bwd_q_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, MIX, wave);
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

        for (int hb = 0; hb < (MIX ? 1 : a.H); hb += 4) {
            float bl[HPW], lse[HPW], dbw[HPW], dbl[HPW];
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int o = min(hb + wave + 4 * s, a.H - 1);
                bl[s] = MIX ? a.bl[o] : 0.f;
                lse[s] = a.lse[((int64_t)win * a.H + o) * 64 + qi];
                dbw[s] = 0.f; dbl[s] = 0.f;
            }
            float cross[4 * HPW][HPW];
#pragma unroll
            for (int h = 0; h < 4 * HPW; ++h)
#pragma unroll
                for (int s = 0; s < HPW; ++s) cross[h][s] = 0.f;
            f32x16 P[2][HPW], D[2][HPW], S[HPW], U[HPW];

            // ---- phase 1: P of the whole key row ---------------------------------------------------------------------------
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t < a.NT) {
                    int rel[16];
                    float mk[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int j = t * 32 + acc_row(r, g);
                        rel[r] = qkc - c.G.kc[j];
                        mk[r] = c.G.reg[j] != qreg ? -100.f : 0.f;
                    }
                    own_scores<HPW>(S, a, qp, kp, c.tl, c.G, qtok, t, hb, rel, wave, lane);
                    if constexpr (MIX) {
                        xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
                        xchg_mix<HPW, false>(c.X, S, a.wl, a.H, wave, lane);
                    }
#pragma unroll
                    for (int s = 0; s < HPW; ++s)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            P[t][s][r] = (qok && t * 32 + acc_row(r, g) < a.N)
                                             ? __builtin_amdgcn_exp2f((S[s][r] + bl[s] + mk[r] - lse[s]) * LOG2E) : 0.f;
                } else {
#pragma unroll
                    for (int s = 0; s < HPW; ++s) { P[t][s] = f32x16{}; D[t][s] = f32x16{}; }
                }
            }
            // ---- phase 2: dP' = dO . v of the own heads, dP = proj_w^T dP', dWw, dbw ------------------------------------------
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t < a.NT) {
#pragma unroll
                    for (int s = 0; s < HPW; ++s) {
                        const int o = hb + wave + 4 * s;
                        S[s] = f32x16{};
                        if (o < a.H) {
                            const short* row = dop + (int64_t)qtok * dos + o * 32 + g * 8;
                            F df[2];
#pragma unroll
                            for (int ks = 0; ks < 2; ++ks) df[ks] = TT::load(row + ks * 16);
                            S[s] = stream_tile(vp + (int64_t)o * a.sh, a.sn, c.G.tok, t, 1.f, false, df, lane);
                        }
                    }
                    if constexpr (MIX) {
#pragma unroll
                        for (int s = 0; s < HPW; ++s) {
                            float d0 = 0.f;
#pragma unroll
                            for (int r = 0; r < 16; ++r) d0 += (qok && t * 32 + acc_row(r, g) < a.N) ? S[s][r] : 0.f;
                            dbw[s] += d0;
                        }
                        xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
                        xchg_mix<HPW, true, true>(c.X, U, a.ww, a.H, wave, lane, P[t], cross);             // dWw[o][h] += dP'_o P_h
                    }
#pragma unroll
                    for (int s = 0; s < HPW; ++s) D[t][s] = MIX ? U[s] : S[s];
                }
            }
            if constexpr (MIX) cross_accum<HPW>(acc_ww, cross, a.H, wave, lane);
            // ---- delta, dS' ------------------------------------------------------------------------------------------------
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                float d0 = 0.f, d1 = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        d0 = __builtin_fmaf(P[t][s][r], D[t][s][r], d0);
                        d1 = __builtin_fmaf(P[t][s][r + 1], D[t][s][r + 1], d1);
                    }
                float dl = d0 + d1;
                dl += __shfl_xor(dl, 32);
                const int o = hb + wave + 4 * s;
                if (o < a.H && g == 0) a.delta[((int64_t)win * a.H + o) * 64 + qi] = dl;
                float sum = 0.f;
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        D[t][s][r] = P[t][s][r] * (D[t][s][r] - dl);
                        sum += D[t][s][r];
                    }
                dbl[s] += sum;
            }
            // ---- phase 3: dS = proj_l^T dS', dWl, dq, dT --------------------------------------------------------------------
            f32x16 dq[HPW];
#pragma unroll
            for (int s = 0; s < HPW; ++s) dq[s] = f32x16{};
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (t < a.NT) {
                    if constexpr (MIX) {
                        int rel[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) rel[r] = qkc - c.G.kc[t * 32 + acc_row(r, g)];
                        own_scores<HPW>(S, a, qp, kp, c.tl, c.G, qtok, t, hb, rel, wave, lane);
#pragma unroll
                        for (int s = 0; s < HPW; ++s) U[s] = D[t][s];
                        xchg_put<HPW>(c.X, U, 0, a.H, wave, lane);
                        xchg_mix<HPW, true, true>(c.X, U, a.wl, a.H, wave, lane, S, cross);          // dWl[o][h] += dS'_o S_h
                    } else {
#pragma unroll
                        for (int s = 0; s < HPW; ++s) U[s] = D[t][s];
                    }
#pragma unroll
                    for (int s = 0; s < HPW; ++s) {
                        const int h = hb + wave + 4 * s;
                        if (h < a.H) {
                            stage_tile(c.st, kp + (int64_t)h * a.sh, a.sn, c.G.tok, t, 1.f, false, lane);
                            rows_product(dq[s], c.st, U[s], lane);
                        }
                    }
                    // dT[u][h] += sum of dS_h[i][j] over the pairs of this (query tile, key tile) at offset u: thread u
                    xchg_put<HPW>(c.X, U, hb, a.H, wave, lane);
                    if ((int)threadIdx.x < a.NU) {
                        const int u = threadIdx.x;
                        const int dy = u / W2 - (a.w - 1), dx = u - (u / W2) * W2 - (a.w - 1);
                        const int hx = MIX ? a.H : min(4, a.H - hb);
                        for (int iy = max(0, dy); iy < min(a.w, a.w + dy); ++iy)
                            for (int ix = max(0, dx); ix < min(a.w, a.w + dx); ++ix) {
                                const int i = iy * a.w + ix, j = i - (dy * a.w + dx);
                                if ((i >> 5) != qt || (j >> 5) != t) continue;
                                const int ii = i & 31, jl = j & 31;
                                const float* xp = c.X + ((jl >> 3) * 64 + ii + 32 * ((jl >> 2) & 1)) * 4 + (jl & 3);
                                float* ap = acc_t + u * a.H + hb;
                                for (int x = 0; x < hx; ++x) ap[x] += xp[x * 1024];
                            }
                    }
                }
            }
            if constexpr (MIX) {
                cross_accum<HPW>(acc_wl, cross, a.H, wave, lane);
#pragma unroll
                for (int s = 0; s < HPW; ++s) {
                    const float vl = wave_sum(dbl[s]), vw = wave_sum(dbw[s]);
                    const int o = wave + 4 * s;
                    if (o < a.H && lane == 0) { acc_bl[o] += vl; acc_bw[o] += vw; }
                }
            }
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int h = hb + wave + 4 * s;
                if (h < a.H && qok) store_row(a.dq + (int64_t)b * a.dsb + (int64_t)qtok * a.dsn + (int64_t)h * a.dsh, dq[s], g, a.scale);
            }
        }
    }
    __syncthreads();
    float* part = a.part + (int64_t)blockIdx.x * a.psize;
    for (int i = threadIdx.x; i < a.psize; i += 256) part[i] = c.acc[i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own keys (launch K): dk, dv.  Streams the window's query tiles; lse and delta of its queries through LDS.
// ---------------------------------------------------------------------------------------------------------------------------
template <int HPW, bool MIX>
__global__ __launch_bounds__(256) void window_attn_bwd_kv_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, MIX, wave);
    for (int i = threadIdx.x; i < a.NU * a.H; i += 256) c.tl[i] = a.tab[i];
    const int relc = 2 * a.w * (a.w - 1);
    const int64_t dos = (int64_t)a.H * 32;

    for (int item = blockIdx.x; item < a.nwin * a.NT; item += gridDim.x) {
        const int win = item / a.NT, kt = item - win * a.NT, b = win / a.nW;
        setup_window(c.geo, a, win);
        for (int i = threadIdx.x; i < a.H * 64; i += 256) {
            c.lse_s[i] = a.lse[(int64_t)win * a.H * 64 + i];
            c.dl_s[i] = a.delta[(int64_t)win * a.H * 64 + i];
        }
        __syncthreads();
        const int kj = kt * 32 + c32;
        const bool kok = kj < a.N;
        const int ktok = c.G.tok[kj], kreg = c.G.reg[kj], kkc = relc - c.G.kc[kj];
        const short* qp = a.q + (int64_t)b * a.sb;
        const short* kp = a.k + (int64_t)b * a.sb;
        const short* vp = a.v + (int64_t)b * a.sb;
        const short* dop = a.dout + (int64_t)b * a.L * dos;

        for (int hb = 0; hb < (MIX ? 1 : a.H); hb += 4) {
            float bl[HPW], bw[HPW];
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int o = min(hb + wave + 4 * s, a.H - 1);
                bl[s] = MIX ? a.bl[o] : 0.f;
                bw[s] = MIX ? a.bw[o] : 0.f;
            }
            f32x16 dk[HPW], dv[HPW];
#pragma unroll
            for (int s = 0; s < HPW; ++s) { dk[s] = f32x16{}; dv[s] = f32x16{}; }
            f32x16 S[HPW], P[HPW], T[HPW];
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
                    const int h = hb + wave + 4 * s;
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
                if constexpr (MIX) {
                    xchg_put<HPW>(c.X, S, 0, a.H, wave, lane);
                    xchg_mix<HPW, false>(c.X, S, a.wl, a.H, wave, lane);
                }
#pragma unroll
                for (int s = 0; s < HPW; ++s) {
                    const int o = min(hb + wave + 4 * s, a.H - 1);
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        P[s][r] = ok[r] ? __builtin_amdgcn_exp2f((S[s][r] + bl[s] + mk[r] - c.lse_s[o * 64 + t * 32 + acc_row(r, g)]) * LOG2E)
                                        : 0.f;
                }
#pragma unroll
                for (int s = 0; s < HPW; ++s) S[s] = P[s];
                if constexpr (MIX) {
                    xchg_put<HPW>(c.X, P, 0, a.H, wave, lane);
                    xchg_mix<HPW, false>(c.X, S, a.ww, a.H, wave, lane);                          // P'
#pragma unroll
                    for (int s = 0; s < HPW; ++s)
#pragma unroll
                        for (int r = 0; r < 16; ++r) S[s][r] += ok[r] ? bw[s] : 0.f;
                }
#pragma unroll
                for (int s = 0; s < HPW; ++s) {
                    const int o = hb + wave + 4 * s;
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
                if constexpr (MIX) {
                    xchg_put<HPW>(c.X, T, 0, a.H, wave, lane);
                    xchg_mix<HPW, true>(c.X, T, a.ww, a.H, wave, lane);                           // dP
                }
#pragma unroll
                for (int s = 0; s < HPW; ++s) {
                    const int o = min(hb + wave + 4 * s, a.H - 1);
#pragma unroll
                    for (int r = 0; r < 16; ++r) T[s][r] = P[s][r] * (T[s][r] - c.dl_s[o * 64 + t * 32 + acc_row(r, g)]);   // dS'
                }
                if constexpr (MIX) {
                    xchg_put<HPW>(c.X, T, 0, a.H, wave, lane);
                    xchg_mix<HPW, true>(c.X, T, a.wl, a.H, wave, lane);                           // dS
                }
#pragma unroll
                for (int s = 0; s < HPW; ++s) {
                    const int h = hb + wave + 4 * s;
                    __builtin_amdgcn_sched_barrier(0);
                    if (h < a.H) {
                        stage_tile(c.st, qp + (int64_t)h * a.sh, a.sn, c.G.tok, t, a.scale, true, lane);
                        rows_product(dk[s], c.st, T[s], lane);                                // dk_h^T += (s q_h)^T dS_h^T
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int h = hb + wave + 4 * s;
                if (h < a.H && kok) {
                    store_row(a.dk + (int64_t)b * a.dsb + (int64_t)ktok * a.dsn + (int64_t)h * a.dsh, dk[s], g, 1.f);
                    store_row(a.dv + (int64_t)b * a.dsb + (int64_t)ktok * a.dsn + (int64_t)h * a.dsh, dv[s], g, 1.f);
                }
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
int grid_for(const Args& a, int lds) {
    const int per_cu = lds <= 80 * 1024 ? 2 : 1;
    const int items = a.nwin * a.NT, cap = cu_count() * per_cu;
    return items < cap ? items : cap;
}
template <typename K> int launch(K kern, const Args& a, int blocks, int lds, hipStream_t st) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return CREAM_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), (size_t)lds, st, a);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}
template <int HPW, bool MIX> int run(const Args& a, bool bwd, hipStream_t st) {
    const int lds = Lds(a.H, MIX, a.NU, a.psize).total;
    const int blocks = grid_for(a, lds);
    if (!bwd) return launch(window_attn_fwd_kernel<HPW, MIX>, a, blocks, lds, st);
    const int rc = launch(window_attn_bwd_q_kernel<HPW, MIX>, a, blocks, lds, st);
    if (rc) return rc;
    return launch(window_attn_bwd_kv_kernel<HPW, MIX>, a, blocks, lds, st);
}
int dispatch(const Args& a, bool bwd, hipStream_t st) {
    if (!a.wl) return run<1, false>(a, bwd, st);
    switch ((a.H + 3) / 4) {
        case 1: return run<1, true>(a, bwd, st);
        case 2: return run<2, true>(a, bwd, st);
        case 3: return run<3, true>(a, bwd, st);
        default: return run<4, true>(a, bwd, st);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

int psize_of(int H, int w, bool mix) { return (2 * w - 1) * (2 * w - 1) * H + (mix ? 2 * H * H + 2 * H : 0); }

// the shape alone (what sizes the grid and the partials)
int check_shape(const cream_window_attn_desc* d) {
    if (!d) return CREAM_ERR_BAD_ARG;
    const bool mix = d->wl || d->bl || d->ww || d->bw;
    if (mix && !(d->wl && d->bl && d->ww && d->bw)) return CREAM_ERR_BAD_ARG;
    if (d->head_dim != 32 || d->B < 0 || d->H < 1 || d->H > (mix ? MAXH_MIXED : MAXH)) return CREAM_ERR_BAD_ARG;
    if (d->w < 1 || d->w * d->w > 64 || d->Hs < d->w || d->Ws < d->w || d->Hs % d->w || d->Ws % d->w) return CREAM_ERR_BAD_ARG;
    if (d->shift < 0 || d->shift >= d->w || d->mask_shift < 0 || d->mask_shift >= d->w) return CREAM_ERR_BAD_ARG;
    if ((int64_t)d->B * d->Hs * d->Ws > (int64_t)1 << 30) return CREAM_ERR_TOO_LARGE;
    return CREAM_OK;
}

int check(const cream_window_attn_desc* d, bool bwd) {
    if (!d || !d->q || !d->k || !d->v || !d->lse || !d->table || (!bwd && !d->out)) return CREAM_ERR_BAD_ARG;
    if (const int rc = check_shape(d)) return rc;
    const bool mix = d->wl != nullptr;
    if (d->sn % 8 || d->sh % 8 || d->sb % 8 || !aligned16(d->q) || !aligned16(d->k) || !aligned16(d->v) || (!bwd && !aligned8(d->out)))
        return CREAM_ERR_BAD_ARG;
    if (!aligned4(d->lse) || !aligned4(d->table) || (mix && !(aligned4(d->wl) && aligned4(d->bl) && aligned4(d->ww) && aligned4(d->bw))))
        return CREAM_ERR_BAD_ARG;
    if (bwd) {
        if (!d->dout || !d->dq || !d->dk || !d->dv || !d->delta || !d->part || d->part_blocks < 1) return CREAM_ERR_BAD_ARG;
        if (d->dsn % 4 || d->dsh % 4 || d->dsb % 4 || !aligned16(d->dout)) return CREAM_ERR_BAD_ARG;
        if (!aligned8(d->dq) || !aligned8(d->dk) || !aligned8(d->dv) || !aligned4(d->delta) || !aligned4(d->part)) return CREAM_ERR_BAD_ARG;
    }
    return CREAM_OK;
}

Args to_args(const cream_window_attn_desc* d) {
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
    a.N = d->w * d->w; a.NT = (a.N + 31) / 32; a.NU = (2 * d->w - 1) * (2 * d->w - 1);
    a.nWx = d->Ws / d->w; a.nW = (d->Hs / d->w) * a.nWx; a.nwin = d->B * a.nW; a.L = d->Hs * d->Ws;
    a.psize = psize_of(d->H, d->w, d->wl != nullptr);
    return a;
}

}  // namespace

extern "C" {

int cream_window_attn_check(const cream_window_attn_desc* d, int backward) { return check(d, backward != 0); }

int cream_window_attn_part_size(int H, int w, int mixed)
{
    if (H < 1 || H > MAXH || w < 1 || w * w > 64) return CREAM_ERR_BAD_ARG;
    return psize_of(H, w, mixed != 0);
}

int cream_window_attn_blocks(const cream_window_attn_desc* d)
{
    const int rc = check_shape(d);
    if (rc) return rc;
    const Args a = to_args(d);
    if (a.nwin == 0) return 0;
    return grid_for(a, Lds(a.H, a.wl != nullptr, a.NU, a.psize).total);
}

int cream_window_attn_fwd(const cream_window_attn_desc* d, void* stream)
{
    const int rc = check(d, false);
    if (rc) return rc;
    if (d->B == 0) return CREAM_OK;
    return dispatch(to_args(d), false, (hipStream_t)stream);
}

int cream_window_attn_bwd(const cream_window_attn_desc* d, void* stream)
{
    const int rc = check(d, true);
    if (rc) return rc;
    if (d->B == 0) return CREAM_OK;
    const Args a = to_args(d);
    if (d->part_blocks != grid_for(a, Lds(a.H, a.wl != nullptr, a.NU, a.psize).total)) return CREAM_ERR_BAD_ARG;
    return dispatch(a, true, (hipStream_t)stream);
}

}  // extern "C"

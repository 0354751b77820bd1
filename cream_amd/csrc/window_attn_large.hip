// window_attn_large.hip — fused (shifted-)window attention for windows of 9x9 .. 14x14 tokens (64 < N = w*w <= 196), forward and
// backward, for gfx950 (MI355X): what AutoFormerV2 / S3 (and Swin at window 12, TinyViT at 14) computes between the qkv and proj
// linears.  Heads of 32, 1 <= H <= 32 independent heads, no head transforms.
//
// Reference semantics (AutoFormerV2/model/SSS.py:106-137 inside :205-243), per window of N tokens, s = scale,
// T = relative_position_bias_table ((2w-1)^2, H) fp32:
//     S_h[i,j] = (s q_h,i).k_h,j + T[rel(i,j), h] (+ mask[i,j] in {0, -100})      P_h = softmax_j(S_h)      O_h,i = sum_j P_h[i,j] v_h,j
//
// The tile format, the lane's products, logit, log-sum-exp and P, and the host's descriptor check are window_attn_rows.hpp, shared
// with window_attn_xl.hip (15x15 .. 32x32); this file has what is this family's own: the head's K and V resident in LDS, the
// shift's geometry, the loops.  The tile bodies of the backward are the same text in both files (window_attn_rows.hpp says why).
//
// Geometry: the conventions of window_attn.hip:14-19.  The kernels read the packed projection of the UNSHIFTED, UNPARTITIONED map
// and write the output in the same token order: local token (iy, ix) of window (wy, wx) is map token
// ((wy w + iy + shift) mod Hs, (wx w + ix + shift) mod Ws); rel(i,j) = (iy-jy+w-1)(2w-1) + (ix-jx+w-1); the mask compares the region
// ids of the two positions in the shifted frame, three slices per axis with m = mask_shift.
//
// Shape of the kernels.  The heads are independent, so a work item is ONE (window, head) and a workgroup (4 waves) serves ONE head
// for its whole life: workgroup b has head b mod H and walks the windows b / H, b / H + G / H, ...  (G = the persistent grid, a
// multiple of H).  Per item the workgroup stages the head's two row operands — K and V (forward, launch Q) or s q and dO (launch
// K) — once into LDS as [NP][40] bf16 (NP = N padded to the 32-key tile, padded rows zero), and wave v then owns the 32-token
// tiles v and v + 4 (at most 7 tiles), one token per lane, with the swapped product of attn_common.hpp: tiles of the streamed
// side come from LDS, row-wise for q k^T and dO v^T and through the transposing read of attn_lane.hpp for P v, dS k, dO^T P
// and q^T dS.  Waves never exchange anything in the forward and in launch K.
//
// Softmax: TWO PASSES over the LDS-resident keys, not an online softmax.  Pass 1 forms the S tiles and keeps a running (max,
// sum) per lane (no O to rescale), pass 2 forms them again and multiplies P = exp(S - lse) into V.  The second q k^T costs 2 of
// the 6 MFMAs per tile pair and reads only LDS; in exchange no 7-tile row of logits (112 registers) and no rescaling of O is
// kept, the forward holds one S tile and one O tile, and the backward's P = exp(S - lse) is the forward's P bit for bit.  Keys past N have
// S = -inf in pass 1 and P = 0 in pass 2: they contribute exactly 0.
//
// Backward, with dP[i,j] = dO_i . v_j:   delta[i] = sum_j P dP    dS = P (dP - delta)    dT[u,h] = sum_{rel(i,j)=u} dS_h[i,j]
//                                        dq = s dS k              dk = dS^T (s q)       dv = P^T dO
//   launch Q (lanes own queries): delta (pass A, written out for launch K), then dq and dT (pass B);
//   launch K (lanes own keys): dk, dv from lse and delta.
// dT: a workgroup owns one head, so its share of dT is ONE column, (2w-1)^2 fp32 = 2.9 KB at w = 14, whatever H is (the
// all-heads share of window_attn.hip would be 93 KB at H = 32 next to a table of the same size).  In pass B the waves put the dS
// tiles of all query tiles against key tile t into X[8][4 KB]; thread u (and u + 256, u + 512) then walks the queries
// i = j + off(u), j in tile t, in ascending order and adds the sum onto acc[u]: one owner per entry, a fixed order of items, no
// atomics.  At the end the workgroup writes its column into part[b / H][u, h]; the caller sums the (G / H) partials.
//
// Budgets at w = 14 (NP = 224): operands 2 x 17,920 B, table column and dT column 2 x 2,916 B, geometry 3,584 B, lse/delta rows
// 1,792 B, X 32 KB (launch Q only): 46.3 KB for the forward and launch K (3 workgroups per CU), 78.3 KB for launch Q (2 per CU).
// Code object (gfx950, hipcc -O3, from the kernels' metadata; profiles/NOTES_window_attention_large.md has the listing):
//     window_attn_large_fwd_kernel      VGPR 104, AGPR 16, SGPR 103, scratch 0, no VGPR or SGPR spills, 4 waves/SIMD by registers
//     window_attn_large_bwd_q_kernel    VGPR 163, AGPR 48, SGPR 106, scratch 0, no VGPR spills, 43 SGPRs spilled to VGPR lanes, 2
//     window_attn_large_bwd_kv_kernel   VGPR 144, AGPR 32, SGPR  91, scratch 0, no VGPR or SGPR spills, 2
// LDS is dynamic (the figures above).  With 256-thread workgroups a CU holds 3 / 2 / 3 workgroups by LDS = 3 / 2 / 3 waves per
// SIMD, so launch K's registers (2) are the one place where the register file, not LDS, is the bound.
#include <hip/hip_runtime.h>
#include <hip/hip_bfloat16.h>
#include <stdint.h>

#include "window_attn_rows.hpp"

namespace {
using namespace cream;

constexpr int WMIN = 9, WMAX = 14;
constexpr int XT = 8;                  // X tiles of launch Q: query tiles wave + 4 round, round = 0, 1

struct Args {
    const short *q, *k, *v;
    int64_t sb, sn, sh;
    short* out;                        // (B, L, H, 32)
    float* lse;                        // (B nW, H, NP)
    const float* tab;
    int B, H, Hs, Ws, w, shift, ms;
    float scale;
    const short* dout;                 // (B, L, H, 32)
    short *dq, *dk, *dv;
    int64_t dsb, dsn, dsh;
    float* delta;                      // (B nW, H, NP)
    float* part;                       // (G / H, NU, H) partials of launch Q
    int N, NT, NP, NU, nWx, nW, nwin, L;
};

// ---- LDS carve-up (bytes) ------------------------------------------------------------------------------------------------------
struct Lds {
    int ra, rb, tl, acc, geo, lse, dl, x, total;
    __host__ __device__ Lds(int NP, int NU, bool with_x) {
        ra = 0;
        rb = ra + NP * KP * 2;                         // [NP][KP] bf16: K | s q
        tl = rb + NP * KP * 2;                         // [NP][KP] bf16: V | dO
        acc = tl + ((NU * 4 + 15) & ~15);              // this head's column of the bias table
        geo = acc + ((NU * 4 + 15) & ~15);             // this head's column of dT (launch Q)
        lse = geo + 4 * NP * 4;                        // tok | reg | (unused) | kc, NP ints each
        dl = lse + NP * 4;                             // lse and delta rows of the window (launch K)
        x = dl + NP * 4;
        total = x + (with_x ? XT * 4096 : 0);          // X[qt][4][64][4] fp32 (launch Q)
    }
};
struct Ctx {
    short *ra, *rb;
    float *tl, *acc, *lse_s, *dl_s, *X;
    const int *tok, *reg, *kc;
    int* geo;
};
__device__ __forceinline__ Ctx carve(unsigned char* smem, const Args& a, bool with_x) {
    const Lds L(a.NP, a.NU, with_x);
    Ctx c;
    c.ra = reinterpret_cast<short*>(smem + L.ra);
    c.rb = reinterpret_cast<short*>(smem + L.rb);
    c.tl = reinterpret_cast<float*>(smem + L.tl);
    c.acc = reinterpret_cast<float*>(smem + L.acc);
    c.geo = reinterpret_cast<int*>(smem + L.geo);
    c.lse_s = reinterpret_cast<float*>(smem + L.lse);
    c.dl_s = reinterpret_cast<float*>(smem + L.dl);
    c.X = reinterpret_cast<float*>(smem + L.x);
    c.tok = c.geo; c.reg = c.geo + a.NP; c.kc = c.geo + 3 * a.NP;
    return c;
}

// ---- geometry of one window: token offsets, mask regions and table coordinates of its NP (padded) local tokens ------------------
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
        geo[3 * a.NP + threadIdx.x] = iy * (2 * a.w - 1) + ix;
    }
    __syncthreads();
}
// the workgroup's copy of the window's rows of one head: dst[NP][KP] = base[tok[row] * rs + 0..31] (optionally scaled), rows
// past N zero
__device__ __forceinline__ void stage_rows(short* dst, const short* base, int64_t rs, const int* tok, const Args& a, bool scale_a) {
    for (int idx = threadIdx.x; idx < a.NP * 4; idx += 256) {
        const int row = idx >> 2, cc = idx & 3;
        F x = TT::zero();
        if (row < a.N) {
            x = TT::load(base + (int64_t)tok[row] * rs + cc * 8);
            if (scale_a) x = scaled(x, a.scale);
        }
        *reinterpret_cast<F*>(dst + row * KP + cc * 8) = x;
    }
}
// the 32 staged rows of tile t
__device__ __forceinline__ const short* tile_of(const short* rows, int t) { return rows + t * 32 * KP; }

// ---------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_attn_large_fwd_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, false);
    const int h = blockIdx.x % a.H, wl0 = blockIdx.x / a.H, wls = gridDim.x / a.H;
    for (int i = threadIdx.x; i < a.NU; i += 256) c.tl[i] = a.tab[i * a.H + h];
    const int relc = 2 * a.w * (a.w - 1);

    for (int win = wl0; win < a.nwin; win += wls) {
        const int b = win / a.nW;
        setup_window(c.geo, a, win);
        stage_rows(c.ra, a.k + (int64_t)b * a.sb + (int64_t)h * a.sh, a.sn, c.tok, a, false);
        stage_rows(c.rb, a.v + (int64_t)b * a.sb + (int64_t)h * a.sh, a.sn, c.tok, a, false);
        __syncthreads();
        for (int qt = wave; qt < a.NT; qt += 4) {
            const int qi = qt * 32 + c32;
            const int qtok = c.tok[qi], qreg = c.reg[qi], qkc = c.kc[qi] + relc;
            F qs[2];
            load_own(qs, a.q + (int64_t)b * a.sb + (int64_t)qtok * a.sn + (int64_t)h * a.sh, g, a.scale, true);
            // ---- pass 1: the row's log-sum-exp (tile 0 has 16 real keys for both lane groups, so m is finite after it) ----------
            float m = -INFINITY, l = 0.f;
            for (int t = 0; t < a.NT; ++t) {
                f32x16 S = lds_tile(c.ra, qs, lane, t * 32);
                add_bias<true>(S, c.tl, c.kc, c.reg, t, qkc, qreg, a.N, g);
                const float mn = fmaxf(m, tile_max(S));
                float sum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f((S[r] - mn) * LOG2E);
                l = l * __builtin_amdgcn_exp2f((m - mn) * LOG2E) + sum;
                m = mn;
            }
            const float mx = __shfl_xor(m, 32), lx = __shfl_xor(l, 32);
            const float lse = pair_lse(m, l, mx, lx, g);
            if (g == 0) a.lse[((int64_t)win * a.H + h) * a.NP + qi] = lse;
            // ---- pass 2: O = P V with P = exp(S - lse) ---------------------------------------------------------------------------
            f32x16 O = {};
            for (int t = 0; t < a.NT; ++t) {
                f32x16 S = lds_tile(c.ra, qs, lane, t * 32);
                add_bias<true>(S, c.tl, c.kc, c.reg, t, qkc, qreg, a.N, g);
                p_tile(S, lse);
                rows_product(O, tile_of(c.rb, t), S, lane);
            }
            if (qi < a.N) store_row(a.out + (((int64_t)b * a.L + qtok) * a.H + h) * 32, O, g, 1.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own queries (launch Q): delta, dq, and the workgroup's column of dT
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_attn_large_bwd_q_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, true);
    const int h = blockIdx.x % a.H, wl0 = blockIdx.x / a.H, wls = gridDim.x / a.H;
    for (int i = threadIdx.x; i < a.NU; i += 256) { c.tl[i] = a.tab[i * a.H + h]; c.acc[i] = 0.f; }
    const int relc = 2 * a.w * (a.w - 1);
    const int W2 = 2 * a.w - 1;
    const int64_t dos = (int64_t)a.H * 32;

    for (int win = wl0; win < a.nwin; win += wls) {
        const int b = win / a.nW;
        setup_window(c.geo, a, win);
        stage_rows(c.ra, a.k + (int64_t)b * a.sb + (int64_t)h * a.sh, a.sn, c.tok, a, false);
        stage_rows(c.rb, a.v + (int64_t)b * a.sb + (int64_t)h * a.sh, a.sn, c.tok, a, false);
        __syncthreads();
        F qs[2][2], dof[2][2];
        float lse[2], dl[2];
        int qkc[2], qreg[2];
        // ---- pass A: delta of the wave's query tiles ---------------------------------------------------------------------------
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
            const int qt = wave + 4 * rd;
            lse[rd] = 0.f; dl[rd] = 0.f; qkc[rd] = relc; qreg[rd] = 0;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) { qs[rd][ks] = TT::zero(); dof[rd][ks] = TT::zero(); }
            if (qt < a.NT) {
                const int qi = qt * 32 + c32;
                const int qtok = c.tok[qi];
                qreg[rd] = c.reg[qi]; qkc[rd] = c.kc[qi] + relc;
                load_own(qs[rd], a.q + (int64_t)b * a.sb + (int64_t)qtok * a.sn + (int64_t)h * a.sh, g, a.scale, true);
                load_own(dof[rd], a.dout + ((int64_t)b * a.L + qtok) * dos + h * 32, g, 1.f, false);
                lse[rd] = a.lse[((int64_t)win * a.H + h) * a.NP + qi];
                float d0 = 0.f, d1 = 0.f;
                for (int t = 0; t < a.NT; ++t) {
                    f32x16 S = lds_tile(c.ra, qs[rd], lane, t * 32);
                    add_bias<true>(S, c.tl, c.kc, c.reg, t, qkc[rd], qreg[rd], a.N, g);
                    const f32x16 D = lds_tile(c.rb, dof[rd], lane, t * 32);
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        d0 = __builtin_fmaf(qi < a.N ? __builtin_amdgcn_exp2f((S[r] - lse[rd]) * LOG2E) : 0.f, D[r], d0);
                        d1 = __builtin_fmaf(qi < a.N ? __builtin_amdgcn_exp2f((S[r + 1] - lse[rd]) * LOG2E) : 0.f, D[r + 1], d1);
                    }
                }
                float d = d0 + d1;
                d += __shfl_xor(d, 32);
                dl[rd] = d;
                if (g == 0) a.delta[((int64_t)win * a.H + h) * a.NP + qi] = d;
            }
        }
        // ---- pass B: dS tile by tile; dq; the dS tiles of all query tiles against key tile t go through X for dT ---------------------
        f32x16 dq[2];
        dq[0] = f32x16{}; dq[1] = f32x16{};
        for (int t = 0; t < a.NT; ++t) {
#pragma unroll
            for (int rd = 0; rd < 2; ++rd) {
                const int qt = wave + 4 * rd;
                f32x16 U[1];
                U[0] = f32x16{};
                if (qt < a.NT) {
                    const bool qok = qt * 32 + c32 < a.N;
                    f32x16 S = lds_tile(c.ra, qs[rd], lane, t * 32);
                    add_bias<true>(S, c.tl, c.kc, c.reg, t, qkc[rd], qreg[rd], a.N, g);
                    const f32x16 D = lds_tile(c.rb, dof[rd], lane, t * 32);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float p = qok ? __builtin_amdgcn_exp2f((S[r] - lse[rd]) * LOG2E) : 0.f;
                        U[0][r] = p * (D[r] - dl[rd]);
                    }
                    rows_product(dq[rd], tile_of(c.ra, t), U[0], lane);
                }
                xchg_put<1>(c.X + rd * 4 * 1024, U, 0, 4, wave, lane);         // tile qt = wave + 4 rd; barriers on both sides
            }
            // dT[u] += sum over the pairs (i, j) at offset u with j in key tile t, i ascending: thread u, u + 256, u + 512
            for (int u = threadIdx.x; u < a.NU; u += 256) {
                const int uy = u / W2;
                const int dy = uy - (a.w - 1), dx = u - uy * W2 - (a.w - 1);
                const int off = dy * a.w + dx;                                  // i - j
                const int lo = max(0, t * 32 + off), hi = min(a.N, t * 32 + 32 + off);
                if (lo >= hi) continue;
                const int y0 = max(max(0, dy), lo / a.w), y1 = min(min(a.w, a.w + dy), (hi - 1) / a.w + 1);
                const int x0 = max(0, dx), x1 = min(a.w, a.w + dx);
                float sum = 0.f;
                for (int iy = y0; iy < y1; ++iy) {
                    const int r0 = iy * a.w;
                    for (int i = max(r0 + x0, lo); i < min(r0 + x1, hi); ++i) {
                        const int ii = i & 31, jl = (i - off) & 31;
                        sum += c.X[(i >> 5) * 1024 + ((jl >> 3) * 64 + ii + 32 * ((jl >> 2) & 1)) * 4 + (jl & 3)];
                    }
                }
                c.acc[u] += sum;
            }
        }
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
            const int qt = wave + 4 * rd, qi = qt * 32 + c32;
            if (qt < a.NT && qi < a.N)
                store_row(a.dq + (int64_t)b * a.dsb + (int64_t)c.tok[qi] * a.dsn + (int64_t)h * a.dsh, dq[rd], g, a.scale);
        }
    }
    __syncthreads();
    float* part = a.part + (int64_t)wl0 * a.NU * a.H;
    for (int i = threadIdx.x; i < a.NU; i += 256) part[i * a.H + h] = c.acc[i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own keys (launch K): dk, dv.  s q and dO of the window's queries staged; their lse and delta through LDS.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_attn_large_bwd_kv_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, false);
    const int h = blockIdx.x % a.H, wl0 = blockIdx.x / a.H, wls = gridDim.x / a.H;
    for (int i = threadIdx.x; i < a.NU; i += 256) c.tl[i] = a.tab[i * a.H + h];
    const int relc = 2 * a.w * (a.w - 1);
    const int64_t dos = (int64_t)a.H * 32;

    for (int win = wl0; win < a.nwin; win += wls) {
        const int b = win / a.nW;
        setup_window(c.geo, a, win);
        stage_rows(c.ra, a.q + (int64_t)b * a.sb + (int64_t)h * a.sh, a.sn, c.tok, a, true);
        stage_rows(c.rb, a.dout + (int64_t)b * a.L * dos + h * 32, dos, c.tok, a, false);
        for (int i = threadIdx.x; i < a.NP; i += 256) {
            c.lse_s[i] = a.lse[((int64_t)win * a.H + h) * a.NP + i];
            c.dl_s[i] = a.delta[((int64_t)win * a.H + h) * a.NP + i];
        }
        __syncthreads();
        for (int kt = wave; kt < a.NT; kt += 4) {
            const int kj = kt * 32 + c32;
            const bool kok = kj < a.N;
            const int ktok = c.tok[kj], kreg = c.reg[kj], kkc = relc - c.kc[kj];
            F kf[2], vf[2];
            load_own(kf, a.k + (int64_t)b * a.sb + (int64_t)ktok * a.sn + (int64_t)h * a.sh, g, 1.f, false);
            load_own(vf, a.v + (int64_t)b * a.sb + (int64_t)ktok * a.sn + (int64_t)h * a.sh, g, 1.f, false);
            f32x16 dk = {}, dv = {};
            for (int t = 0; t < a.NT; ++t) {
                f32x16 P = lds_tile(c.ra, kf, lane, t * 32);                   // rows: queries of tile t, column: own key
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = t * 32 + acc_row(r, g);
                    const float s = P[r] + c.tl[c.kc[i] + kkc] + (c.reg[i] != kreg ? -100.f : 0.f);
                    P[r] = (kok && i < a.N) ? __builtin_amdgcn_exp2f((s - c.lse_s[i]) * LOG2E) : 0.f;
                }
                rows_product(dv, tile_of(c.rb, t), P, lane);                    // dv^T += dO^T P
                f32x16 D = lds_tile(c.rb, vf, lane, t * 32);                    // dP
#pragma unroll
                for (int r = 0; r < 16; ++r) D[r] = P[r] * (D[r] - c.dl_s[t * 32 + acc_row(r, g)]);
                rows_product(dk, tile_of(c.ra, t), D, lane);                    // dk^T += (s q)^T dS
            }
            if (kok) {
                store_row(a.dk + (int64_t)b * a.dsb + (int64_t)ktok * a.dsn + (int64_t)h * a.dsh, dk, g, 1.f);
                store_row(a.dv + (int64_t)b * a.dsb + (int64_t)ktok * a.dsn + (int64_t)h * a.dsh, dv, g, 1.f);
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
Args to_args(const cream_window_attn_large_desc* d) {
    Args a{};
    a.q = (const short*)d->q; a.k = (const short*)d->k; a.v = (const short*)d->v;
    a.sb = d->sb; a.sn = d->sn; a.sh = d->sh;
    a.out = (short*)d->out; a.lse = d->lse;
    a.tab = d->table;
    a.B = d->B; a.H = d->H; a.Hs = d->Hs; a.Ws = d->Ws; a.w = d->w; a.shift = d->shift; a.ms = d->mask_shift; a.scale = d->scale;
    a.dout = (const short*)d->dout;
    a.dq = (short*)d->dq; a.dk = (short*)d->dk; a.dv = (short*)d->dv;
    a.dsb = d->dsb; a.dsn = d->dsn; a.dsh = d->dsh;
    a.delta = d->delta; a.part = d->part;
    a.N = d->w * d->w; a.NT = (a.N + 31) / 32; a.NP = a.NT * 32; a.NU = (2 * d->w - 1) * (2 * d->w - 1);
    a.nWx = d->Ws / d->w; a.nW = (d->Hs / d->w) * a.nWx; a.nwin = d->B * a.nW; a.L = d->Hs * d->Ws;
    return a;
}

// window lanes per head of the persistent grids
int lanes_of(const Args& a) { return lanes_for(Lds(a.NP, a.NU, true).total, a.nwin, a.H); }

// the argument check, then the launches
int run(const cream_window_attn_large_desc* d, bool bwd, void* stream) {
    if (const int rc = check(d, bwd, WMIN, WMAX, true)) return rc;
    if (d->B == 0) return CREAM_OK;
    const Args a = to_args(d);
    const int lanes = lanes_of(a), lds = Lds(a.NP, a.NU, false).total, ldsq = Lds(a.NP, a.NU, true).total;
    const hipStream_t st = (hipStream_t)stream;
    if (!bwd) return launch(window_attn_large_fwd_kernel, a, lanes * a.H, lds, st);
    if (d->part_blocks != lanes) return CREAM_ERR_BAD_ARG;
    if (const int rc = launch(window_attn_large_bwd_q_kernel, a, lanes * a.H, ldsq, st)) return rc;
    return launch(window_attn_large_bwd_kv_kernel, a, lanes * a.H, lds, st);
}

}  // namespace

extern "C" {

int cream_window_attn_large_check(const cream_window_attn_large_desc* d, int backward) { return check(d, backward != 0, WMIN, WMAX, true); }
int cream_window_attn_large_part_size(int H, int w) { return part_size(H, w, WMIN, WMAX); }
int cream_window_attn_large_blocks(const cream_window_attn_large_desc* d)
{
    const int rc = check_shape(d, WMIN, WMAX, true);
    return rc ? rc : d->B == 0 ? 0 : lanes_of(to_args(d));
}
int cream_window_attn_large_fwd(const cream_window_attn_large_desc* d, void* stream) { return run(d, false, stream); }
int cream_window_attn_large_bwd(const cream_window_attn_large_desc* d, void* stream) { return run(d, true, stream); }

}  // extern "C"

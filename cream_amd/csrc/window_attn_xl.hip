// window_attn_xl.hip — fused window attention for windows of 15x15 .. 32x32 tokens (225 <= N = w*w <= 1024), forward and
// backward, for gfx950 (MI355X): what TinyViT-21M at 384 and 512 (TinyViT/models/tiny_vit.py:216-286 inside :289-383, windows of
// 16, 24 and 32) computes between the qkv and proj linears.  Heads of 32, 1 <= H <= 32 independent heads, no shift, no mask.
//
// Semantics per window of N tokens, s = scale, T = the ((2w-1)^2, H) fp32 relative-position table:
//     S_h[i,j] = (s q_h,i).k_h,j + T[rel(i,j), h]      P_h = softmax_j(S_h)      O_h,i = sum_j P_h[i,j] v_h,j
// The tile format, the lane's products, logit, log-sum-exp and P, and the host's descriptor check are window_attn_rows.hpp, shared
// with window_attn_large.hip (9x9 .. 14x14); this file has what is this family's own: the chunked, double-buffered stream, the
// candidate set of dT, the loops.  The tile bodies of the backward are the same text in both files (window_attn_rows.hpp says why).
// Geometry: that of window_attn_large.hip's header with shift = mask_shift = 0.  The kernels read the packed projection of the
// UNPARTITIONED map and write the output in the same token order: local token (iy, ix) of window (wy, wx) is map token
// (wy w + iy, wx w + ix); rel(i,j) = (iy-jy+w-1)(2w-1) + (ix-jx+w-1).
//
// Shape of the kernels.  window_attn_large.hip keeps K and V of a head resident in LDS; at NP = 1024 that would be 160 KB.  Here
// the streamed side goes through LDS in CHUNKS of two 32-row tiles (64 rows x 2 operands x 80 B = 10 KB), double-buffered: while
// the waves work on chunk c, every thread holds its 16-byte piece of each operand of chunk c + 1 in registers (one global load
// per operand, issued before the products) and puts it into the other buffer afterwards; one barrier per chunk.  A work item is
// ONE (window, head, block of 128 own tokens): wave v owns the 32-token tile 4 block + v, one token per lane, with the swapped
// product of attn_common.hpp and the transposing read of attn_lane.hpp.  A workgroup (4 waves) serves ONE head for its whole
// life: workgroup b has head b mod H and walks the items b / H, b / H + G / H, ... of that head (G = the persistent grid, a
// multiple of H), so that its share of the table and of dT is one column.  Waves exchange nothing in the forward and in launch K.
//
// Softmax: TWO PASSES over the streamed keys, as in window_attn_large.hip.  Pass 1 streams K alone and keeps a running (max, sum) per lane,
// pass 2 streams K and V and multiplies P = exp(S - lse) into V; the backward's P = exp(S - lse) is then the forward's P bit for
// bit, and no O is rescaled.  The second stream of K is LDS and L2 traffic (a head's K of one window is at most 64 KB and is
// read by the 8 items of the window), not HBM.  Keys past N are staged as zero rows and have S = -inf in pass 1 and P = 0 in
// pass 2 and in the backward: they contribute exactly 0.
//
// Backward, with dP[i,j] = dO_i . v_j:   delta[i] = sum_j P dP    dS = P (dP - delta)    dT[u,h] = sum_{rel(i,j)=u} dS_h[i,j]
//                                        dq = s dS k              dk = dS^T (s q)       dv = P^T dO
//   launch Q (lanes own queries; K and V streamed twice): delta (pass A, written out for launch K), then dq and dT (pass B);
//   launch K (lanes own keys; s q and dO streamed, lse and delta rows of the window in LDS): dk, dv.
// dT: in pass B the four waves put their dS tiles against key tile t into X[4][4 KB].  The offsets i - j of the 128 x 32 pairs lie
// in a band of at most 159 values, and an offset has at most two (dy, dx): 318 candidate entries u, one per thread and round.
// The thread walks the queries i = j + off(u) of the block in ascending order and adds the sum onto acc[u] in LDS: one owner per
// entry and step, a fixed order of items and tiles, no atomics.  At the end the workgroup writes its column into
// part[b / H][u, h]; the caller sums the (G / H) partials in a fixed order.
//
// Budgets at w = 32 (NP = 1024, NU = 3969): chunks 20,480 B, table column 15,888 B, geometry 8,192 B; + lse/delta rows 8,192 B in
// launch K; + dT column 15,888 B and X 16,384 B in launch Q: 44,560 B forward (3 workgroups per CU), 52,752 B launch K (3),
// 76,832 B launch Q (2).  At w = 16: 26,384 / 28,432 / 46,624 B.
// Code object (gfx950, hipcc -O3, from the kernels' metadata; profiles/NOTES_window_attention_xl.md has the listing):
//     window_attn_xl_fwd_kernel      VGPR  86, AGPR 32, SGPR  96, scratch 0, no VGPR or SGPR spills, 4 waves/SIMD by registers
//     window_attn_xl_bwd_q_kernel    VGPR 131, AGPR 32, SGPR 106, scratch 0, no VGPR spills, 42 SGPRs spilled to VGPR lanes, 3
//     window_attn_xl_bwd_kv_kernel   VGPR 100, AGPR 48, SGPR 104, scratch 0, no VGPR or SGPR spills, 3
// LDS is dynamic (the figures above).  A 256-thread workgroup is one wave per SIMD, so the registers allow 4 / 3 / 3 workgroups
// per CU and LDS allows 3 / 2 / 3 at w = 32 (6 / 3 / 5 at w = 16, where the registers bind): achieved occupancy at w = 32 is
// 3 / 2 / 3 workgroups per CU, bound by LDS — in launch Q by the two fp32 columns of 3969 entries (31 KB) and X (16 KB) — with
// launch K at the point where both limits meet.
#include <hip/hip_runtime.h>
#include <hip/hip_bfloat16.h>
#include <stdint.h>

#include "window_attn_rows.hpp"

namespace {
using namespace cream;

constexpr int WMIN = 15, WMAX = 32;
constexpr int CT = 2;                  // 32-row tiles per streamed chunk
constexpr int CR = CT * 32;            // rows per chunk: 256 threads x one 16-byte piece per operand
constexpr int BUF = CR * KP;           // bf16 per operand buffer

struct Args {
    const short *q, *k, *v;
    int64_t sb, sn, sh;
    short* out;                        // (B, L, H, 32)
    float* lse;                        // (B nW, H, NP)
    const float* tab;
    int B, H, Hs, Ws, w;
    float scale;
    const short* dout;                 // (B, L, H, 32)
    short *dq, *dk, *dv;
    int64_t dsb, dsn, dsh;
    float* delta;                      // (B nW, H, NP)
    float* part;                       // (G / H, NU, H) partials of launch Q
    int N, NT, NP, NU, NC, NB, nWx, nW, nwin, nitems, L;
};

// ---- LDS carve-up (bytes) ------------------------------------------------------------------------------------------------------
enum Mode { FWD = 0, BQ = 1, BK = 2 };
struct Lds {
    int buf, tl, geo, acc, x, lse, total;
    __host__ __device__ Lds(int NP, int NU, int mode) {
        buf = 0;                                       // [2 buffers][2 operands][CR][KP] bf16
        tl = buf + 4 * BUF * 2;                        // this head's column of the bias table
        geo = tl + ((NU * 4 + 15) & ~15);              // tok | kc, NP ints each
        acc = geo + 2 * NP * 4;                        // this head's column of dT (launch Q)
        x = acc + (mode == BQ ? ((NU * 4 + 15) & ~15) : 0);
        lse = x + (mode == BQ ? 4 * 4096 : 0);         // X[4][4][64][4] fp32 (launch Q)
        total = lse + (mode == BK ? 2 * NP * 4 : 0);   // lse and delta rows of the window (launch K)
    }
};
struct Ctx {
    short* buf;
    float *tl, *acc, *X, *lse_s, *dl_s;
    int *tok, *kc;
};
__device__ __forceinline__ Ctx carve(unsigned char* smem, const Args& a, int mode) {
    const Lds L(a.NP, a.NU, mode);
    Ctx c;
    c.buf = reinterpret_cast<short*>(smem + L.buf);
    c.tl = reinterpret_cast<float*>(smem + L.tl);
    c.tok = reinterpret_cast<int*>(smem + L.geo);
    c.kc = c.tok + a.NP;
    c.acc = reinterpret_cast<float*>(smem + L.acc);
    c.X = reinterpret_cast<float*>(smem + L.x);
    c.lse_s = reinterpret_cast<float*>(smem + L.lse);
    c.dl_s = c.lse_s + a.NP;
    return c;
}
__device__ __forceinline__ short* buf_of(const Ctx& c, int which, int operand) { return c.buf + (which * 2 + operand) * BUF; }

// ---- geometry of one window: token offsets and table coordinates of its NP (padded) local tokens ---------------------------------
__device__ __forceinline__ void setup_window(const Ctx& c, const Args& a, int win) {
    __syncthreads();                                   // the previous item's readers are done
    const int wi = win % a.nW;
    const int wy = wi / a.nWx, wx = wi - wy * a.nWx;
    for (int t = threadIdx.x; t < a.NP; t += 256) {
        const int i = min(t, a.N - 1);                 // padded tokens repeat the last real one (finite data, never used)
        const int iy = i / a.w, ix = i - iy * a.w;
        c.tok[t] = (wy * a.w + iy) * a.Ws + wx * a.w + ix;
        c.kc[t] = iy * (2 * a.w - 1) + ix;
    }
    __syncthreads();
}

// ---- the stream: this thread's 16-byte pieces of chunk `ch` of one or two row operands, rows past N zero ------------------------
struct Piece { F a, b; };
template <bool BOTH>
__device__ __forceinline__ Piece fetch(const short* pa, int64_t rsa, const short* pb, int64_t rsb, const Ctx& c, const Args& a, int ch,
                                       bool scale_a) {
    const int row = ch * CR + ((int)threadIdx.x >> 2), cc = threadIdx.x & 3;
    Piece p;
    p.a = TT::zero(); p.b = TT::zero();
    if (row < a.N) {
        const int tok = c.tok[row];
        p.a = TT::load(pa + (int64_t)tok * rsa + cc * 8);
        if (scale_a) p.a = scaled(p.a, a.scale);
        if constexpr (BOTH) p.b = TT::load(pb + (int64_t)tok * rsb + cc * 8);
    }
    return p;
}
template <bool BOTH> __device__ __forceinline__ void put(const Ctx& c, int which, const Piece& p) {
    const int off = ((int)threadIdx.x >> 2) * KP + (threadIdx.x & 3) * 8;
    *reinterpret_cast<F*>(buf_of(c, which, 0) + off) = p.a;
    if constexpr (BOTH) *reinterpret_cast<F*>(buf_of(c, which, 1) + off) = p.b;
}
// One pass over the NC chunks of (pa, pb): body(t, rows_a, rows_b) once per key tile t, with the tile's rows in LDS.  Every thread
// of the workgroup calls this (the barriers), whether its wave has work or not.  Buffer (c + 1) & 1 was last read in iteration
// c - 1, which ended in a barrier; the pass itself ends in one, so passes follow each other without another.
template <bool BOTH, typename Body>
__device__ __forceinline__ void stream(const short* pa, int64_t rsa, const short* pb, int64_t rsb, const Ctx& c, const Args& a,
                                       bool scale_a, Body body) {
    Piece p = fetch<BOTH>(pa, rsa, pb, rsb, c, a, 0, scale_a);
    put<BOTH>(c, 0, p);
    __syncthreads();
    for (int ch = 0; ch < a.NC; ++ch) {
        const bool more = ch + 1 < a.NC;
        if (more) p = fetch<BOTH>(pa, rsa, pb, rsb, c, a, ch + 1, scale_a);
        const short *ra = buf_of(c, ch & 1, 0), *rb = buf_of(c, ch & 1, 1);
#pragma unroll
        for (int tt = 0; tt < CT; ++tt)
            if (ch * CT + tt < a.NT) body(ch * CT + tt, ra + tt * 32 * KP, rb + tt * 32 * KP);
        if (more) put<BOTH>(c, (ch + 1) & 1, p);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_attn_xl_fwd_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, FWD);
    const int h = blockIdx.x % a.H, wl0 = blockIdx.x / a.H, wls = gridDim.x / a.H;
    for (int i = threadIdx.x; i < a.NU; i += 256) c.tl[i] = a.tab[i * a.H + h];
    const int relc = 2 * a.w * (a.w - 1);

    for (int item = wl0; item < a.nitems; item += wls) {
        const int win = item / a.NB, qt = (item - win * a.NB) * 4 + wave;
        const int b = win / a.nW;
        const bool active = qt < a.NT;                 // wave-uniform
        setup_window(c, a, win);
        const int qi = active ? qt * 32 + c32 : 0;
        const int qtok = c.tok[qi], qkc = c.kc[qi] + relc;
        const short* kb = a.k + (int64_t)b * a.sb + (int64_t)h * a.sh;
        const short* vb = a.v + (int64_t)b * a.sb + (int64_t)h * a.sh;
        F qs[2];
        load_own(qs, a.q + (int64_t)b * a.sb + (int64_t)qtok * a.sn + (int64_t)h * a.sh, g, a.scale, true);
        // ---- pass 1: the row's log-sum-exp (tile 0 has only real keys, so m is finite after it) --------------------------------
        float m = -INFINITY, l = 0.f;
        stream<false>(kb, a.sn, kb, a.sn, c, a, false, [&](int t, const short* rk, const short*) {
            if (!active) return;
            f32x16 S = lds_tile(rk, qs, lane);
            add_bias<false>(S, c.tl, c.kc, nullptr, t, qkc, 0, a.N, g);
            const float mn = fmaxf(m, tile_max(S));
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) sum += __builtin_amdgcn_exp2f((S[r] - mn) * LOG2E);
            l = l * __builtin_amdgcn_exp2f((m - mn) * LOG2E) + sum;
            m = mn;
        });
        float lse = 0.f;
        if (active) {
            const float mx = __shfl_xor(m, 32), lx = __shfl_xor(l, 32);
            lse = pair_lse(m, l, mx, lx, g);
            if (g == 0) a.lse[((int64_t)win * a.H + h) * a.NP + qi] = lse;
        }
        // ---- pass 2: O = P V with P = exp(S - lse) -------------------------------------------------------------------------------
        f32x16 O = {};
        stream<true>(kb, a.sn, vb, a.sn, c, a, false, [&](int t, const short* rk, const short* rv) {
            if (!active) return;
            f32x16 S = lds_tile(rk, qs, lane);
            add_bias<false>(S, c.tl, c.kc, nullptr, t, qkc, 0, a.N, g);
            p_tile(S, lse);
            rows_product(O, rv, S, lane);
        });
        if (active && qi < a.N) store_row(a.out + (((int64_t)b * a.L + qtok) * a.H + h) * 32, O, g, 1.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own queries (launch Q): delta, dq, and the workgroup's column of dT
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_attn_xl_bwd_q_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, BQ);
    const int h = blockIdx.x % a.H, wl0 = blockIdx.x / a.H, wls = gridDim.x / a.H;
    for (int i = threadIdx.x; i < a.NU; i += 256) { c.tl[i] = a.tab[i * a.H + h]; c.acc[i] = 0.f; }
    const int relc = 2 * a.w * (a.w - 1);
    const int W2 = 2 * a.w - 1;
    const int64_t dos = (int64_t)a.H * 32;

    for (int item = wl0; item < a.nitems; item += wls) {
        const int win = item / a.NB, q0 = (item - win * a.NB) * 128, qt = (q0 >> 5) + wave;
        const int q1 = min(a.N, q0 + 128);             // the block's real queries: [q0, q1)
        const int b = win / a.nW;
        const bool active = qt < a.NT;                 // wave-uniform
        setup_window(c, a, win);
        const int qi = active ? qt * 32 + c32 : 0;
        const bool qok = active && qi < a.N;
        const int qtok = c.tok[qi], qkc = c.kc[qi] + relc;
        const short* kb = a.k + (int64_t)b * a.sb + (int64_t)h * a.sh;
        const short* vb = a.v + (int64_t)b * a.sb + (int64_t)h * a.sh;
        F qs[2], dof[2];
        load_own(qs, a.q + (int64_t)b * a.sb + (int64_t)qtok * a.sn + (int64_t)h * a.sh, g, a.scale, true);
        load_own(dof, a.dout + ((int64_t)b * a.L + qtok) * dos + h * 32, g, 1.f, false);
        const float lse = a.lse[((int64_t)win * a.H + h) * a.NP + qi];
        // ---- pass A: delta of the wave's query tile ------------------------------------------------------------------------------
        float d0 = 0.f, d1 = 0.f;
        stream<true>(kb, a.sn, vb, a.sn, c, a, false, [&](int t, const short* rk, const short* rv) {
            if (!active) return;
            f32x16 S = lds_tile(rk, qs, lane);
            add_bias<false>(S, c.tl, c.kc, nullptr, t, qkc, 0, a.N, g);
            const f32x16 D = lds_tile(rv, dof, lane);
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                d0 = __builtin_fmaf(qok ? __builtin_amdgcn_exp2f((S[r] - lse) * LOG2E) : 0.f, D[r], d0);
                d1 = __builtin_fmaf(qok ? __builtin_amdgcn_exp2f((S[r + 1] - lse) * LOG2E) : 0.f, D[r + 1], d1);
            }
        });
        float dl = d0 + d1;
        dl += __shfl_xor(dl, 32);
        if (active && g == 0) a.delta[((int64_t)win * a.H + h) * a.NP + qi] = dl;
        // ---- pass B: dS tile by tile; dq; the dS tiles of the four query tiles against key tile t go through X for dT ----------------
        f32x16 dq = {};
        stream<true>(kb, a.sn, vb, a.sn, c, a, false, [&](int t, const short* rk, const short* rv) {
            f32x16 U[1];
            U[0] = f32x16{};
            if (active) {
                f32x16 S = lds_tile(rk, qs, lane);
                add_bias<false>(S, c.tl, c.kc, nullptr, t, qkc, 0, a.N, g);
                const f32x16 D = lds_tile(rv, dof, lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = qok ? __builtin_amdgcn_exp2f((S[r] - lse) * LOG2E) : 0.f;
                    U[0][r] = p * (D[r] - dl);
                }
                rows_product(dq, rk, U[0], lane);
            }
            xchg_put<1>(c.X, U, 0, 4, wave, lane);     // X[wave] = the tile of query tile q0 / 32 + wave; barriers on both sides
            // dT[u] += sum over the pairs (i, j) at offset u with j in key tile t and i in [q0, q1), i ascending.  The offsets
            // off = i - j of such pairs: [q0 - 32 t - 31, q1 - 1 - 32 t]; off = dy w + dx has the two readings dx in [0, w) and
            // dx in (-w, 0): candidate cd = 2 (off - offlo) + reading, one thread each.
            const int offlo = q0 - 32 * t - 31, ncand = 2 * (q1 - q0 + 31);
            for (int cd = threadIdx.x; cd < ncand; cd += 256) {
                const int off = offlo + (cd >> 1);
                int dy = off >= 0 ? off / a.w : -((a.w - 1 - off) / a.w);          // floor
                int dx = off - dy * a.w;                                          // [0, w)
                if (cd & 1) { dy += 1; dx -= a.w; }
                if (dy <= -a.w || dy >= a.w || dx <= -a.w) continue;
                const int u = (dy + a.w - 1) * W2 + dx + a.w - 1;
                const int lo = max(q0, t * 32 + off), hi = min(q1, t * 32 + 32 + off);
                if (lo >= hi) continue;
                const int y0 = max(max(0, dy), lo / a.w), y1 = min(min(a.w, a.w + dy), (hi - 1) / a.w + 1);
                const int x0 = max(0, dx), x1 = min(a.w, a.w + dx);
                float sum = 0.f;
                for (int iy = y0; iy < y1; ++iy) {
                    const int r0 = iy * a.w;
                    for (int i = max(r0 + x0, lo); i < min(r0 + x1, hi); ++i) {
                        const int ii = i - q0, jl = (i - off) & 31;
                        sum += c.X[(ii >> 5) * 1024 + ((jl >> 3) * 64 + (ii & 31) + 32 * ((jl >> 2) & 1)) * 4 + (jl & 3)];
                    }
                }
                c.acc[u] += sum;
            }
        });
        if (qok) store_row(a.dq + (int64_t)b * a.dsb + (int64_t)qtok * a.dsn + (int64_t)h * a.dsh, dq, g, a.scale);
    }
    __syncthreads();
    float* part = a.part + (int64_t)wl0 * a.NU * a.H;
    for (int i = threadIdx.x; i < a.NU; i += 256) part[i * a.H + h] = c.acc[i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own keys (launch K): dk, dv.  s q and dO of the window's queries streamed; their lse and delta rows in LDS.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_attn_xl_bwd_kv_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const Ctx c = carve(smem, a, BK);
    const int h = blockIdx.x % a.H, wl0 = blockIdx.x / a.H, wls = gridDim.x / a.H;
    for (int i = threadIdx.x; i < a.NU; i += 256) c.tl[i] = a.tab[i * a.H + h];
    const int relc = 2 * a.w * (a.w - 1);
    const int64_t dos = (int64_t)a.H * 32;

    for (int item = wl0; item < a.nitems; item += wls) {
        const int win = item / a.NB, kt = (item - win * a.NB) * 4 + wave;
        const int b = win / a.nW;
        const bool active = kt < a.NT;                 // wave-uniform
        setup_window(c, a, win);
        for (int i = threadIdx.x; i < a.NP; i += 256) {
            c.lse_s[i] = a.lse[((int64_t)win * a.H + h) * a.NP + i];
            c.dl_s[i] = a.delta[((int64_t)win * a.H + h) * a.NP + i];
        }                                              // visible after the stream's first barrier
        const int kj = active ? kt * 32 + c32 : 0;
        const bool kok = active && kj < a.N;
        const int ktok = c.tok[kj], kkc = relc - c.kc[kj];
        F kf[2], vf[2];
        load_own(kf, a.k + (int64_t)b * a.sb + (int64_t)ktok * a.sn + (int64_t)h * a.sh, g, 1.f, false);
        load_own(vf, a.v + (int64_t)b * a.sb + (int64_t)ktok * a.sn + (int64_t)h * a.sh, g, 1.f, false);
        f32x16 dk = {}, dv = {};
        stream<true>(a.q + (int64_t)b * a.sb + (int64_t)h * a.sh, a.sn, a.dout + (int64_t)b * a.L * dos + h * 32, dos, c, a, true,
                     [&](int t, const short* rq, const short* rdo) {
            if (!active) return;
            f32x16 P = lds_tile(rq, kf, lane);                                 // rows: queries of tile t, column: own key
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = t * 32 + acc_row(r, g);
                const float s = P[r] + c.tl[c.kc[i] + kkc];
                P[r] = (kok && i < a.N) ? __builtin_amdgcn_exp2f((s - c.lse_s[i]) * LOG2E) : 0.f;
            }
            rows_product(dv, rdo, P, lane);                                    // dv^T += dO^T P
            f32x16 D = lds_tile(rdo, vf, lane);                                // dP
#pragma unroll
            for (int r = 0; r < 16; ++r) D[r] = P[r] * (D[r] - c.dl_s[t * 32 + acc_row(r, g)]);
            rows_product(dk, rq, D, lane);                                     // dk^T += (s q)^T dS
        });
        if (kok) {
            store_row(a.dk + (int64_t)b * a.dsb + (int64_t)ktok * a.dsn + (int64_t)h * a.dsh, dk, g, 1.f);
            store_row(a.dv + (int64_t)b * a.dsb + (int64_t)ktok * a.dsn + (int64_t)h * a.dsh, dv, g, 1.f);
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
Args to_args(const cream_window_attn_xl_desc* d) {
    Args a{};
    a.q = (const short*)d->q; a.k = (const short*)d->k; a.v = (const short*)d->v;
    a.sb = d->sb; a.sn = d->sn; a.sh = d->sh;
    a.out = (short*)d->out; a.lse = d->lse;
    a.tab = d->table;
    a.B = d->B; a.H = d->H; a.Hs = d->Hs; a.Ws = d->Ws; a.w = d->w; a.scale = d->scale;
    a.dout = (const short*)d->dout;
    a.dq = (short*)d->dq; a.dk = (short*)d->dk; a.dv = (short*)d->dv;
    a.dsb = d->dsb; a.dsn = d->dsn; a.dsh = d->dsh;
    a.delta = d->delta; a.part = d->part;
    a.N = d->w * d->w; a.NT = (a.N + 31) / 32; a.NP = a.NT * 32; a.NU = (2 * d->w - 1) * (2 * d->w - 1);
    a.NC = (a.NT + CT - 1) / CT; a.NB = (a.NT + 3) / 4;
    a.nWx = d->Ws / d->w; a.nW = (d->Hs / d->w) * a.nWx; a.nwin = d->B * a.nW; a.nitems = a.nwin * a.NB; a.L = d->Hs * d->Ws;
    return a;
}

// item lanes per head of the persistent grids
int lanes_of(const Args& a) { return lanes_for(Lds(a.NP, a.NU, BQ).total, a.nitems, a.H); }

// the argument check, then the launches
int run(const cream_window_attn_xl_desc* d, bool bwd, void* stream) {
    if (const int rc = check(d, bwd, WMIN, WMAX, false)) return rc;       // no shifted window is implemented at these sizes
    if (d->B == 0) return CREAM_OK;
    const Args a = to_args(d);
    const int lanes = lanes_of(a);
    const hipStream_t st = (hipStream_t)stream;
    if (!bwd) return launch(window_attn_xl_fwd_kernel, a, lanes * a.H, Lds(a.NP, a.NU, FWD).total, st);
    if (d->part_blocks != lanes) return CREAM_ERR_BAD_ARG;
    if (const int rc = launch(window_attn_xl_bwd_q_kernel, a, lanes * a.H, Lds(a.NP, a.NU, BQ).total, st)) return rc;
    return launch(window_attn_xl_bwd_kv_kernel, a, lanes * a.H, Lds(a.NP, a.NU, BK).total, st);
}

}  // namespace

extern "C" {

int cream_window_attn_xl_check(const cream_window_attn_xl_desc* d, int backward) { return check(d, backward != 0, WMIN, WMAX, false); }
int cream_window_attn_xl_part_size(int H, int w) { return part_size(H, w, WMIN, WMAX); }
int cream_window_attn_xl_blocks(const cream_window_attn_xl_desc* d)
{
    const int rc = check_shape(d, WMIN, WMAX, false);
    return rc ? rc : d->B == 0 ? 0 : lanes_of(to_args(d));
}
int cream_window_attn_xl_fwd(const cream_window_attn_xl_desc* d, void* stream) { return run(d, false, stream); }
int cream_window_attn_xl_bwd(const cream_window_attn_xl_desc* d, void* stream) { return run(d, true, stream); }

}  // extern "C"

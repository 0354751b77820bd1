// irpe_attn_x.hip — the fused iRPE attention of irpe_attn.hip for 32- and 64-wide heads, up to 128 buckets and a key
// padding mask (DETR-with-iRPE's encoder self-attention: d_model 256, 8 heads, (2 * 4 + 1)^2 = 81 buckets on k,
// images of different sizes in one batch), forward and backward, for gfx950 (MI355X).
//
// Same formulas, same launch structure and the same lane / tile conventions as irpe_attn.hip (read its header first):
// one workgroup = 4 waves = 128 tokens of one (b, h), swapped 32 x 32 score tiles, bucket ids as bytes holding 2 * id
// (cream_irpe_bucket_bytes: ids up to 127 fit), lookup rows in LDS, ordered read-modify-write scatter rows, forward with
// a lazy running maximum, backward launch A over queries, launch B over keys, pre-pass for the rpe_q rows, per-(b, h)
// table-gradient products, no global atomics, fixed summation order.  The 64-wide / <= 64-bucket / unmasked kernels of
// irpe_attn.hip are NOT touched by this file: it is a sibling with its own entry points (cream_irpe_attn2_*).  The two share
// their lane-level helpers (bucket ids, scatter-add, operand fragments, output rows) through attn_lane.hpp and nothing else.
//
// What is a template parameter here:
//   D    head_dim 32 | 64.  Row tiles are [32][D] with pitch D + 8 (80 / 144 bytes: 16-byte reads of 8 consecutive rows
//        cover all 32 banks); D / 16 contraction steps per score tile, D / 32 accumulator tiles per output row.
//   NBW  width of every bucket-indexed row, 64 | 128: lookup rows (bf16, pitch NBW + 2: an odd number of words), scatter
//        rows (fp32, pitch NBW + 1), the (D, nb) / (nb, D) tables as MFMA operands and the (B, H, NP, NBW) side buffers.
//        NBW = 128 is instantiated for rpe on k alone (the published DETR recipe, the ratio-2.0 DeiT configurations):
//        the fp32 scatter rows of one workgroup are 66 KB at 128 columns, so launch A with rpe_k takes 112-120 KB (one
//        workgroup per CU) and with a second table nothing fits twice; cream_irpe_attn2_* answer CREAM_ERR_BAD_ARG
//        for q / v above 64 buckets and the callers keep the composed path there.
// What is a run-time operand:
//   key_pad   (B, L) bytes, non-zero = the key takes no part for any query of that image.  Every kernel keeps the
//        image's mask (tail keys j >= L included) as NP bytes in LDS; a lane's 16 partners of a tile are four aligned
//        32-bit reads.  A masked key gets probability exactly 0 (a select, not a large negative logit), so it adds
//        nothing to the log-sum-exp, the value product, the bucket sums or a bucket gradient, and its dk = dv = 0 and
//        dLQ row = 0 exactly, whatever finite or non-finite numbers its k / v rows hold.  Queries at padded positions
//        attend to the real keys like any other query.  Precondition: at least one real key per image (the reference
//        gives NaN otherwise; here the rows of such an image come out NaN / inf without a fault).
//   out / dout strides, so that a sequence-first caller ((L, N, E) tensors) needs no permute copy.
#include <hip/hip_runtime.h>
#include <hip/hip_bfloat16.h>
#include <stdint.h>

#include <type_traits>

#include "attn_lane.hpp"
#include "cream_amd.h"

namespace {
using namespace cream;

constexpr float LOG2E = 1.4426950408889634f;
constexpr int QW = 4;       // waves (32-token tiles) per workgroup
constexpr int MAXNP = 2048;

template <int D_, int NBW_> struct Geo {
    static constexpr int D = D_, NBW = NBW_;
    static constexpr int KS = D / 16;        // contraction steps over the head dimension
    static constexpr int DT = D / 32;        // 32-column accumulator tiles of an output row
    static constexpr int KP = D + 8;         // pitch (bf16) of [32][D] tiles and of [NBW buckets][D] tables
    static constexpr int WP = NBW + 8;       // pitch (bf16) of [D][NBW buckets] tables
    static constexpr int KSB = NBW / 16;     // contraction steps over the buckets
    static constexpr int BT = NBW / 32;      // 32-bucket tiles of a lookup row
    static constexpr int LK = NBW + 1;       // fp32 scatter-add rows
    static constexpr int LB = NBW + 2;       // bf16 lookup rows: 33 / 65 words
    static constexpr int TILE = 32 * KP * 2;                                            // bytes of one [32][D] tile
    static constexpr int TABB = (NBW * KP > D * WP ? NBW * KP : D * WP) * 2;            // bytes of a table in either orientation
    static_assert(4 * TILE >= TABB, "a table fits over the K + V tile area");
};

struct Args {
    const short *q, *k, *v;
    int64_t sb, sn, sh;
    short* out;                       // element (b, n, h, :) at out[b*osb + n*osn + h*D]
    int64_t osb, osn;
    float* lse;                       // (B, H, L)
    short* sv;                        // (B, H, NP, NBW) bucket sums of P (value side), bf16
    const float *wq, *wk, *wv;        // (H', D, nb), (H', D, nb), (H', nb, D) fp32
    int64_t wq_hs, wk_hs, wv_hs;      // head strides (0: shared)
    const float *bq, *bk;             // bias mode: (H', nb) tables, used when wq / wk is null
    int64_t bq_hs, bk_hs;
    const uint8_t *idq, *idk, *idv;         // (NP, NP) query-major
    const uint8_t *idq_t, *idk_t, *idv_t;   // (NP, NP) key-major
    const uint8_t* pad;               // (B, L) key padding mask or null
    int64_t pad_sb;
    int B, H, L, NP, nb;
    float scale;
    int causal;
    uint32_t drop_thr;
    uint32_t drop_seed;
    float drop_scale;
    // backward
    const short* dout;                // element (b, n, h, :) at dout[b*dosb + n*dosn + h*D]
    int64_t dosb, dosn;
    short *dq, *dk, *dv;
    int64_t dsb, dsn, dsh;
    float* delta;                     // (B, H, NP)
    short *lkg, *gg;                  // (B, H, NP, NBW)
    short *dlk, *dlq;                 // (B, H, NP, NBW)
};

// dst[c][r] = src[r][c] for r < R, c < C (src: nrow x ncol fp32, zero outside) as bf16 operand rows of pitch P
template <int R, int C, int P> __device__ __forceinline__ void stage_T(short* dst, const float* src, int nrow, int ncol) {
    for (int i = threadIdx.x; i < R * C; i += 256) {
        const int c = i % C, r = i / C;
        dst[c * P + r] = f2bf((r < nrow && c < ncol) ? src[(int64_t)r * ncol + c] : 0.f);
    }
}
// dst[r][c] = src[r][c]
template <int R, int C, int P> __device__ __forceinline__ void stage_R(short* dst, const float* src, int nrow, int ncol) {
    for (int i = threadIdx.x; i < R * C; i += 256) {
        const int c = i % C, r = i / C;
        dst[r * P + c] = f2bf((r < nrow && c < ncol) ? src[(int64_t)r * ncol + c] : 0.f);
    }
}

// ---- staged tiles ------------------------------------------------------------------------------------
// row-major [32][W] bf16 tile in 16-byte chunks: chunk c = tid + 256 p -> (row c / (W/8), chunk c % (W/8)); W = 32: half the
// threads carry a chunk, W = 128: two chunks per thread
template <int W> struct Rows {
    static constexpr int CPR = W / 8, N = (32 * CPR + 255) / 256;
    u32x4v x[N];
};
template <int W> __device__ __forceinline__ Rows<W> rows_load(const short* base, int64_t rs, int row0, int nrows, bool zero_pad) {
    Rows<W> r;
#pragma unroll
    for (int p = 0; p < Rows<W>::N; ++p) {
        const int c = threadIdx.x + 256 * p;
        const int row = min(c / Rows<W>::CPR, 31), cc = c % Rows<W>::CPR;
        const int j = min(row0 + row, nrows - 1);
        const u32x4v x = *reinterpret_cast<const u32x4v*>(base + (int64_t)j * rs + cc * 8);
        r.x[p] = (!zero_pad || row0 + row < nrows) ? x : u32x4v{0, 0, 0, 0};
    }
    return r;
}
template <int W> __device__ __forceinline__ Rows<W> rows_scaled(Rows<W> r, float s) {
#pragma unroll
    for (int p = 0; p < Rows<W>::N; ++p) r.x[p] = scaled_raw(r.x[p], s);
    return r;
}
// -> [32][P] with 16-byte stores (P * 2 a multiple of 16)
template <int W, int P> __device__ __forceinline__ void rows_store(short* dst, const Rows<W>& r) {
#pragma unroll
    for (int p = 0; p < Rows<W>::N; ++p) {
        const int c = threadIdx.x + 256 * p;
        const int row = c / Rows<W>::CPR, cc = c % Rows<W>::CPR;
        if (row < 32) *reinterpret_cast<u32x4v*>(dst + row * P + cc * 8) = r.x[p];
    }
}
// lookup rows (bf16 [32][W] contiguous in global) -> [32][P], P an odd number of words: 4-byte stores
template <int W, int P> __device__ __forceinline__ void lrows_store(short* dst, const Rows<W>& r) {
#pragma unroll
    for (int p = 0; p < Rows<W>::N; ++p) {
        const int c = threadIdx.x + 256 * p;
        const int row = c / Rows<W>::CPR, cc = c % Rows<W>::CPR;
        if (row < 32) {
            uint32_t* d = reinterpret_cast<uint32_t*>(dst + row * P + cc * 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = r.x[p][i];
        }
    }
}
// transposed: dst[col][row] (table-gradient products)
template <int W, int P> __device__ __forceinline__ void rows_store_T(short* dst, const Rows<W>& r) {
#pragma unroll
    for (int p = 0; p < Rows<W>::N; ++p) {
        const int c = threadIdx.x + 256 * p;
        const int row = c / Rows<W>::CPR, cc = c % Rows<W>::CPR;
        if (row < 32) {
            union { u32x4v v; short e[8]; } u;
            u.v = r.x[p];
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[(cc * 8 + e) * P + row] = u.e[e];
        }
    }
}

// the image's key mask as NP bytes in LDS: 1 = the key takes no part (padded by the caller, or the tail j >= L)
__device__ __forceinline__ void stage_pad(uint8_t* dst, const Args& a, int b) {
    for (int i = threadIdx.x; i < a.NP; i += 256)
        dst[i] = (i >= a.L || (a.pad && a.pad[(int64_t)b * a.pad_sb + i])) ? 1 : 0;
}
// bit r set <=> partner acc_row(r, g) of tile t is masked: partners 8 rr + 4 g + e, e = 0..3, are one aligned 32-bit read
__device__ __forceinline__ uint32_t pad_bits(const uint8_t* padm, int t, int g) {
    uint32_t m = 0;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(padm + t * 32 + 8 * rr + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) m |= ((w >> (8 * e)) & 0xffu) ? (1u << (4 * rr + e)) : 0u;
    }
    return m;
}

// lookups^T (NBW buckets x 32 own rows) = tab(NBW buckets x D) . X^T  ->  scr[row][bucket] (bf16) * mul
template <typename G> __device__ __forceinline__ void lookups_to_lds(short* scr, const short* tab, const F (&xb)[G::KS], float mul, int lane) {
    const int c32 = lane & 31, g = lane >> 5;
    short* row = scr + c32 * G::LB;
#pragma unroll
    for (int bt = 0; bt < G::BT; ++bt) {
        f32x16 acc = {};
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks) acc = TT::mma(TT::load(tab + (c32 + 32 * bt) * G::KP + ks * 16 + g * 8), xb[ks], acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) row[32 * bt + acc_row(r, g)] = f2bf(acc[r] * mul);
    }
}
// bias mode: every row of a [32][LB] block is the head's bias table
template <typename G> __device__ __forceinline__ void bias_rows_to_lds(short* scr, const float* bias, int nb, int lane) {
    const int c32 = lane & 31, g = lane >> 5;
    constexpr int HALF = G::NBW / 2;
    short* row = scr + c32 * G::LB + g * HALF;
#pragma unroll 8
    for (int e = 0; e < HALF; ++e) row[e] = f2bf(g * HALF + e < nb ? bias[g * HALF + e] : 0.f);
}
// S^T tile (rows = streamed tokens, column = own token) with the relative position terms (irpe_attn.hip score_tile)
template <typename G, bool OWN, bool SIDE>
__device__ __forceinline__ f32x16 score_tile(const short* rows, const F (&own)[G::KS], const u32x4v& own_ids,
                                             const u32x4v& side_ids, const short* own_row, const short* side, int lane) {
    const int c32 = lane & 31, g = lane >> 5;
    f32x16 s = {};
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) s = TT::mma(TT::load(rows + c32 * G::KP + ks * 16 + g * 8), own[ks], s);
    if constexpr (OWN) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = add_bf16_at(s[r], own_row, off2_of(own_ids, r));
    }
    if constexpr (SIDE) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = add_bf16_at(s[r], side + acc_row(r, g) * G::LB, off2_of(side_ids, r));
    }
    return s;
}

// rpe_q lookups of a staged key tile, shared by the four waves: wave w < NBW / 32 computes buckets 32 w .. 32 w + 31.
// Ends with a workgroup barrier.
template <typename G>
__device__ __forceinline__ void lq_tile(short* dst, const short* wqT, const short* kb, float scale, int wave, int lane, bool ctx) {
    if (!ctx) return;                                  // bias mode: both tile buffers were filled once
    if (wave < G::BT) {
        const int c32 = lane & 31, g = lane >> 5;
        f32x16 acc = {};
#pragma unroll
        for (int ks = 0; ks < G::KS; ++ks)
            acc = TT::mma(TT::load(wqT + (c32 + 32 * wave) * G::KP + ks * 16 + g * 8), TT::load(kb + c32 * G::KP + ks * 16 + g * 8), acc);
        short* row = dst + c32 * G::LB + 32 * wave;                   // lane = key, rows = buckets
#pragma unroll
        for (int r = 0; r < 16; ++r) row[acc_row(r, g)] = f2bf(acc[r] * scale);
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------
template <typename G, bool HQ, bool HK, bool HV> struct LdsF {
    static constexpr int kbuf = 0;                                       // 2 x [32][KP] bf16
    static constexpr int vbuf = kbuf + 2 * G::TILE;                      // 2 x [32][KP] bf16 (read transposed)
    static constexpr int wkT = 0;                                        // [NBW buckets][KP]: prologue only, over the tile area
    static constexpr int wvT = 0;                                        // [D][WP] (columns = buckets): epilogue only, over the tile area
    static constexpr int wqT = vbuf + 2 * G::TILE;                       // [NBW buckets][KP]: every key tile (lq_tile)
    static constexpr int lk = wqT + (HQ ? G::NBW * G::KP * 2 : 0);       // QW x [32][LB] bf16
    static constexpr int sv = lk + (HK ? QW * 32 * G::LB * 2 : 0);       // QW x [32][LK] fp32
    static constexpr int lq = sv + (HV ? QW * 32 * G::LK * 4 : 0);       // 2 x [32 keys][LB] bf16
    static constexpr int pad = lq + (HQ ? 2 * 32 * G::LB * 2 : 0);       // [NP] bytes
    static constexpr int total = pad + MAXNP;
    static_assert(total <= 160 * 1024, "LDS of a CU");
};

template <typename G, bool HQ, bool HK, bool HV, bool DROP>
__global__ __launch_bounds__(256) void irpe_x_fwd_kernel(const Args a) {
    using L = LdsF<G, HQ, HK, HV>;
    constexpr int D = G::D, KP = G::KP, LBP = G::LB, LKP = G::LK, KS = G::KS, DT = G::DT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NT = a.NP >> 5, QB = (NT + QW - 1) / QW;
    const int lb = xcd_order(blockIdx.x, gridDim.x);
    const int bh = lb / QB, qblk = lb - bh * QB;
    const int b = bh / a.H, h = bh - b * a.H;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const int q0 = qblk * 32 * QW;
    const bool active = qblk * QW + wave < NT;
    const int qi = q0 + wave * 32 + c32;
    const bool qok = active && qi < a.L;

    const int64_t base = (int64_t)b * a.sb + (int64_t)h * a.sh;
    const short* qp = a.q + base;
    const short* kp = a.k + base;
    const short* vp = a.v + base;

    short* kbuf = reinterpret_cast<short*>(smem + L::kbuf);
    short* vbuf = reinterpret_cast<short*>(smem + L::vbuf);
    short* wkT = reinterpret_cast<short*>(smem + L::wkT);
    short* wqT = reinterpret_cast<short*>(smem + L::wqT);
    short* wvT = reinterpret_cast<short*>(smem + L::wvT);
    short* lkw = reinterpret_cast<short*>(smem + L::lk) + wave * 32 * LBP;
    float* svw = reinterpret_cast<float*>(smem + L::sv) + wave * 32 * LKP;
    short* lqs = reinterpret_cast<short*>(smem + L::lq);
    uint8_t* padm = smem + L::pad;

    // ---- prologue: this lane's query row (scaled), tables, key mask, first key tile ----------------
    F qs[KS];
    load_frags<KS>(qs, qp + (int64_t)min(qi, a.L - 1) * a.sn, g);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qs[ks] = scaled(qs[ks], a.scale);
    Rows<D> sk, sv4;
    u32x4v sik = {}, siv = {}, siq = {};
    u32x4v cik = {}, civ = {}, ciq = {};
    sk = rows_load<D>(kp, a.sn, 0, a.L, false);
    sv4 = rows_load<D>(vp, a.sn, 0, a.L, true);
    if constexpr (HK) cik = ids_load(a.idk, a.NP, qi, 0, g);
    if constexpr (HQ) ciq = ids_load(a.idq, a.NP, qi, 0, g);
    if constexpr (HV) civ = ids_load(a.idv, a.NP, qi, 0, g);
    stage_pad(padm, a, b);
    if constexpr (HK) { if (a.wk) stage_T<D, G::NBW, KP>(wkT, a.wk + (int64_t)h * a.wk_hs, D, a.nb); }
    if constexpr (HQ) {
        if (a.wq) stage_T<D, G::NBW, KP>(wqT, a.wq + (int64_t)h * a.wq_hs, D, a.nb);
        else if (wave < 2) bias_rows_to_lds<G>(lqs + wave * 32 * LBP, a.bq + (int64_t)h * a.bq_hs, a.nb, lane);   // both tile buffers
    }
    if constexpr (HV) { for (int i = lane; i < 32 * LKP; i += 64) svw[i] = 0.f; }
    if constexpr (HK) {
        __syncthreads();                               // the rpe_k table lies over the tile area: use it before the first tiles land
        if (active) {
            if (a.wk) lookups_to_lds<G>(lkw, wkT, qs, 1.f, lane);
            else bias_rows_to_lds<G>(lkw, a.bk + (int64_t)h * a.bk_hs, a.nb, lane);
        }
        __syncthreads();
    }
    rows_store<D, KP>(kbuf, sk);
    rows_store<D, KP>(vbuf, sv4);
    __syncthreads();
    if constexpr (HQ) lq_tile<G>(lqs, wqT, kbuf, a.scale, wave, lane, a.wq != nullptr);

    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x16{};
    float m = -INFINITY, lrun = 0.f;
    // one pass, online softmax with a lazy reference maximum (irpe_attn.hip); a tile whose keys are all masked has the maximum
    // -inf, moves nothing and adds exact zeros
    constexpr float RESCALE_T = 8.f;
    for (int t = 0; t < NT; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        const bool more = t + 1 < NT;
        if (more) {
            sk = rows_load<D>(kp, a.sn, (t + 1) * 32, a.L, false);
            sv4 = rows_load<D>(vp, a.sn, (t + 1) * 32, a.L, true);
            if constexpr (HK) sik = ids_load(a.idk, a.NP, qi, t + 1, g);
            if constexpr (HQ) siq = ids_load(a.idq, a.NP, qi, t + 1, g);
            if constexpr (HV) siv = ids_load(a.idv, a.NP, qi, t + 1, g);
        }
        f32x16 s = {};
        if (active) {
            s = score_tile<G, HK, HQ>(kbuf + cur * 32 * KP, qs, cik, ciq, lkw + c32 * LBP, lqs + cur * 32 * LBP, lane);
            uint32_t off = pad_bits(padm, t, g);
            if (a.causal && t * 32 + 31 > q0 + wave * 32) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (t * 32 + acc_row(r, g) > qi) off |= 1u << r;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = ((off >> r) & 1u) ? -INFINITY : s[r];
            float t4[4] = {s[0], s[1], s[2], s[3]};
#pragma unroll
            for (int r = 4; r < 16; ++r) t4[r & 3] = fmaxf(t4[r & 3], s[r]);
            float tm = fmaxf(fmaxf(t4[0], t4[1]), fmaxf(t4[2], t4[3]));
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            const bool grow = tm > m + RESCALE_T;                // (false for a fully masked tile: -inf > x never holds)
            if (__any(grow)) {
                const float alpha = grow ? __builtin_amdgcn_exp2f((m - tm) * LOG2E) : 1.f;     // 0 on a row's first real tile (m = -inf)
                m = grow ? tm : m;
                lrun *= alpha;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
                if constexpr (HV) {
                    float* row = svw + c32 * LKP + (G::NBW / 2) * g;       // this lane's half of the row's bucket sums
#pragma unroll
                    for (int i = 0; i < G::NBW / 2; ++i) row[i] *= alpha;
                    wave_lds_fence();
                }
            }
            const float mLn = (m == -INFINITY ? 0.f : m) * LOG2E;          // no real key seen yet: exp2(-inf - 0) = 0, not NaN
            float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = ((off >> r) & 1u) ? 0.f : __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], LOG2E, -mLn));
                s[r] = p;
                ps[r & 3] += p;
            }
            lrun += (ps[0] + ps[1]) + (ps[2] + ps[3]);
            if constexpr (DROP) {                                // the normaliser above is the undropped sum
                const uint32_t dkey = drop_key(a.drop_seed, bh);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    s[r] = drop_keep(dkey, qi, t * 32 + acc_row(r, g), a.drop_thr) ? s[r] * a.drop_scale : 0.f;
            }
            const short* vb = vbuf + cur * 32 * KP;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const F pb = TT::from_acc(s, s2);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[dt] = TT::mma(load_perm_tr<KP>(vb, dt, s2, lane), pb, o[dt]);
            }
            if constexpr (HV) scatter_add16(svw + c32 * LKP, civ, s, g);
        }
        if (more) {
            rows_store<D, KP>(kbuf + nxt * 32 * KP, sk);
            rows_store<D, KP>(vbuf + nxt * 32 * KP, sv4);
            if constexpr (HK) cik = sik;
            if constexpr (HQ) ciq = siq;
            if constexpr (HV) civ = siv;
            __syncthreads();
            if constexpr (HQ) lq_tile<G>(lqs + nxt * 32 * LBP, wqT, kbuf + nxt * 32 * KP, a.scale, wave, lane, a.wq != nullptr);
        }
    }
    if constexpr (HV) {
        __syncthreads();                               // every wave is done with the tile area: the value table goes over it
        stage_T<G::NBW, D, G::WP>(wvT, a.wv + (int64_t)h * a.wv_hs, a.nb, D);      // Wv (nb x D): dst[d][u]
        __syncthreads();
    }
    if (!active) return;
    float l = lrun + __shfl_xor(lrun, 32);
    const float inv_l = 1.f / l;
    if (qok && g == 0) a.lse[(int64_t)bh * a.L + qi] = m + __logf(l);

    // ---- value-side term: (normalised bucket sums) . Wv;  the bucket sums are kept for backward ------
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= inv_l;
    if constexpr (HV) {
        const float* row = svw + c32 * LKP;
        short* svg = a.sv + ((int64_t)bh * a.NP + qi) * G::NBW;
#pragma unroll
        for (int ks = 0; ks < G::KSB; ++ks) {
            const F sb = srow_frag<LKP>(row, ks, g, inv_l);
            *reinterpret_cast<F*>(svg + ks * 16 + g * 8) = sb;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = TT::mma(TT::load(wvT + (c32 + 32 * dt) * G::WP + ks * 16 + g * 8), sb, o[dt]);
        }
    }
    if (qok) store_row<DT>(a.out + (int64_t)b * a.osb + (int64_t)qi * a.osn + (int64_t)h * D, o, g, 1.f);
}

// ---------------------------------------------------------------------------------------------------
// backward A: lanes own queries — delta, dq, dLK; LK / G rows for launch B
// ---------------------------------------------------------------------------------------------------
template <typename G, bool HQ, bool HK, bool HV> struct LdsA {
    static constexpr int kbuf = 0;                                   // 2 x [32][KP]   K rows
    static constexpr int vbuf = kbuf + 2 * G::TILE;                  // 2 x [32][KP]   V rows
    static constexpr int tile_end = vbuf + 2 * G::TILE;
    static constexpr int tables = (HV ? 2 : (HK ? 1 : 0)) * G::TABB; // Wk^T (slot 0) / Wv (slot 1) are staged over the tile area outside the loop
    static constexpr int stage_end = tile_end > tables ? tile_end : tables;
    static constexpr int lk = stage_end;                             // QW x [32][LB] bf16
    static constexpr int gl = lk + (HK ? QW * 32 * G::LB * 2 : 0);   // QW x [32][LB] bf16
    static constexpr int dlk = gl + (HV ? QW * 32 * G::LB * 2 : 0);  // QW x [32][LK] fp32
    static constexpr int lq = dlk + (HK ? QW * 32 * G::LK * 4 : 0);  // 2 x [32][LB] bf16
    static constexpr int pad = lq + (HQ ? 2 * 32 * G::LB * 2 : 0);   // [NP] bytes
    static constexpr int total = pad + MAXNP;
    static_assert(total <= 160 * 1024, "LDS of a CU");
};

template <typename G, bool HQ, bool HK, bool HV, bool DROP>
__global__ __launch_bounds__(256) void irpe_x_bwd_q_kernel(const Args a) {
    using L = LdsA<G, HQ, HK, HV>;
    constexpr int D = G::D, KP = G::KP, LBP = G::LB, LKP = G::LK, KS = G::KS, DT = G::DT, NBW = G::NBW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NT = a.NP >> 5, QB = (NT + QW - 1) / QW;
    const int lb = xcd_order(blockIdx.x, gridDim.x);
    const int bh = lb / QB, qblk = lb - bh * QB;
    const int b = bh / a.H, h = bh - b * a.H;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const int q0 = qblk * 32 * QW;
    const bool active = qblk * QW + wave < NT;
    const int qi = q0 + wave * 32 + c32;
    const bool qok = active && qi < a.L;
    const int qcl = min(qi, a.L - 1);

    const int64_t base = (int64_t)b * a.sb + (int64_t)h * a.sh;
    const short* kp = a.k + base;
    const short* vp = a.v + base;
    const short* dop = a.dout + (int64_t)b * a.dosb + (int64_t)h * D;
    const short* outp = a.out + (int64_t)b * a.osb + (int64_t)h * D;

    short* kbuf = reinterpret_cast<short*>(smem + L::kbuf);
    short* vbuf = reinterpret_cast<short*>(smem + L::vbuf);
    short* tab0 = reinterpret_cast<short*>(smem);                    // tables staged over the tile area
    short* tab1 = reinterpret_cast<short*>(smem + G::TABB);
    short* lkw = reinterpret_cast<short*>(smem + L::lk) + wave * 32 * LBP;
    short* glw = reinterpret_cast<short*>(smem + L::gl) + wave * 32 * LBP;
    float* dlkw = reinterpret_cast<float*>(smem + L::dlk) + wave * 32 * LKP;
    short* lqs = reinterpret_cast<short*>(smem + L::lq);
    uint8_t* padm = smem + L::pad;

    // ---- prologue ---------------------------------------------------------------------------------
    F qs[KS], dob[KS];
    float delta = 0.f;
    {
        F ob[KS];
        load_frags<KS>(qs, a.q + base + (int64_t)qcl * a.sn, g);
        load_frags<KS>(dob, dop + (int64_t)qcl * a.dosn, g);
        load_frags<KS>(ob, outp + (int64_t)qcl * a.osn, g);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qs[ks] = scaled(qs[ks], a.scale);
#pragma unroll
            for (int e = 0; e < 8; ++e) delta += bf2f(dob[ks][e]) * bf2f(ob[ks][e]);
        }
        delta += __shfl_xor(delta, 32);
        if (!qok) {
            delta = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) dob[ks] = TT::zero();
        }
    }
    if (active && g == 0) a.delta[(int64_t)bh * a.NP + qi] = delta;
    const float lseL = qok ? a.lse[(int64_t)bh * a.L + qi] * LOG2E : INFINITY;

    stage_pad(padm, a, b);
    if constexpr (HK) { if (a.wk) stage_T<D, NBW, KP>(tab0, a.wk + (int64_t)h * a.wk_hs, D, a.nb); }      // [bucket][d]
    if constexpr (HV) stage_R<NBW, D, KP>(tab1, a.wv + (int64_t)h * a.wv_hs, a.nb, D);                    // [bucket][d]
    // rpe_q lookups of the streamed keys: rows of (k * scale) Wq written by the pre-pass into the dlq buffer (irpe_attn.hip)
    const short* lqg = HQ ? a.dlq + (int64_t)bh * a.NP * NBW : nullptr;
    const bool lq_rows = HQ && a.wq != nullptr;
    if constexpr (HQ) {
        if (!a.wq && wave < 2) bias_rows_to_lds<G>(lqs + wave * 32 * LBP, a.bq + (int64_t)h * a.bq_hs, a.nb, lane);
    }
    if constexpr (HK) { for (int i = lane; i < 32 * LKP; i += 64) dlkw[i] = 0.f; }
    __syncthreads();
    if (active) {
        if constexpr (HK) {
            if (a.wk) lookups_to_lds<G>(lkw, tab0, qs, 1.f, lane);
            else bias_rows_to_lds<G>(lkw, a.bk + (int64_t)h * a.bk_hs, a.nb, lane);
            wave_lds_fence();
            lrow_to_global<G::KSB>(a.lkg + ((int64_t)bh * a.NP + qi) * NBW, lkw + c32 * LBP, g);
        }
        if constexpr (HV) {
            lookups_to_lds<G>(glw, tab1, dob, 1.f, lane);
            wave_lds_fence();
            lrow_to_global<G::KSB>(a.gg + ((int64_t)bh * a.NP + qi) * NBW, glw + c32 * LBP, g);
        }
    }
    __syncthreads();                                   // tables consumed: the tile area is free
    struct Stage { Rows<D> k, v; Rows<NBW> lq; u32x4v ik, iv, iq; } st;
    u32x4v cik = {}, ciq = {}, civ = {};
    auto issue = [&](Stage& r, int t) {
        r.k = rows_load<D>(kp, a.sn, t * 32, a.L, false);
        r.v = rows_load<D>(vp, a.sn, t * 32, a.L, true);
        if constexpr (HQ) { if (lq_rows) r.lq = rows_load<NBW>(lqg, NBW, t * 32, a.NP, false); }
        if constexpr (HK) r.ik = ids_load(a.idk, a.NP, qi, t, g);
        if constexpr (HQ) r.iq = ids_load(a.idq, a.NP, qi, t, g);
        if constexpr (HV) r.iv = ids_load(a.idv, a.NP, qi, t, g);
    };
    auto commit = [&](const Stage& r, int t) {
        const int buf = t & 1;
        rows_store<D, KP>(kbuf + buf * 32 * KP, r.k);
        rows_store<D, KP>(vbuf + buf * 32 * KP, r.v);
        if constexpr (HQ) { if (lq_rows) lrows_store<NBW, LBP>(lqs + buf * 32 * LBP, r.lq); }
        if constexpr (HK) cik = r.ik;
        if constexpr (HQ) ciq = r.iq;
        if constexpr (HV) civ = r.iv;
    };
    issue(st, 0);
    commit(st, 0);
    __syncthreads();

    // ---- key tiles ----------------------------------------------------------------------------------
    f32x16 dq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x16{};
    for (int t = 0; t < NT; ++t) {
        const int cur = t & 1;
        if (t + 1 < NT) issue(st, t + 1);
        if (active) {
            f32x16 s = score_tile<G, HK, HQ>(kbuf + cur * 32 * KP, qs, cik, ciq, lkw + c32 * LBP, lqs + cur * 32 * LBP, lane);
            f32x16 dp = {};
            const short* vb = vbuf + cur * 32 * KP;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) dp = TT::mma(TT::load(vb + c32 * KP + ks * 16 + g * 8), dob[ks], dp);
            if constexpr (HV) {
                const short* row = glw + c32 * LBP;
#pragma unroll
                for (int r = 0; r < 16; ++r) dp[r] = add_bf16_at(dp[r], row, off2_of(civ, r));
            }
            const uint32_t off = pad_bits(padm, t, g);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = t * 32 + acc_row(r, g);
                const bool ok = !((off >> r) & 1u) && !(a.causal && key > qi);
                const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], LOG2E, -lseL));
                float dpr = dp[r];                                   // gradient of the DROPPED map -> of the softmax output
                if constexpr (DROP) dpr = drop_keep(drop_key(a.drop_seed, bh), qi, key, a.drop_thr) ? dpr * a.drop_scale : 0.f;
                s[r] = ok ? p * (dpr - delta) : 0.f;                 // a select: whatever a masked key's rows hold
            }
            if constexpr (HK) scatter_add16(dlkw + c32 * LKP, cik, s, g);
            const short* kb = kbuf + cur * 32 * KP;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const F db = TT::from_acc(s, s2);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) dq[dt] = TT::mma(load_perm_tr<KP>(kb, dt, s2, lane), db, dq[dt]);
            }
        }
        if (t + 1 < NT) {
            commit(st, t + 1);
            __syncthreads();
        }
    }

    // ---- dq += dLK Wk^T; bucket gradient rows out -------------------------------------------------
    if constexpr (HK) {
        const bool ctx = a.wk != nullptr;
        if (ctx) {
            __syncthreads();                           // every wave is done with the tile area
            stage_R<D, NBW, G::WP>(tab0, a.wk + (int64_t)h * a.wk_hs, D, a.nb);  // [d][bucket]
            __syncthreads();
        }
        if (active) {
            const float* row = dlkw + c32 * LKP;
            short* dst = a.dlk + ((int64_t)bh * a.NP + qi) * NBW;
#pragma unroll
            for (int ks = 0; ks < G::KSB; ++ks) {
                const F db = srow_frag<LKP>(row, ks, g, 1.f);
                *reinterpret_cast<F*>(dst + ks * 16 + g * 8) = db;
                if (ctx) {
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) dq[dt] = TT::mma(TT::load(tab0 + (c32 + 32 * dt) * G::WP + ks * 16 + g * 8), db, dq[dt]);
                }
            }
        }
    }
    if (qok) store_row<DT>(a.dq + (int64_t)b * a.dsb + (int64_t)qi * a.dsn + (int64_t)h * a.dsh, dq, g, a.scale);
}

// rpe_q lookup rows of every key, (k * scale) Wq as bf16 -> dst (B, H, NP, NBW).  Launched in front of backward A with
// dst = the dlq buffer.  Masked keys get rows too (finite inputs give finite rows; nothing reads them into a result).
template <typename G>
__global__ __launch_bounds__(256) void irpe_x_lq_rows_kernel(const Args a, short* dst) {
    __shared__ __attribute__((aligned(16))) short tab[G::NBW * G::KP];
    __shared__ __attribute__((aligned(16))) short scr[QW * 32 * G::LB];
    const int NT = a.NP >> 5, KB = (NT + QW - 1) / QW;
    const int bh = blockIdx.x / KB, kblk = blockIdx.x - bh * KB;
    const int b = bh / a.H, h = bh - b * a.H;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const int kj = kblk * 32 * QW + wave * 32 + c32;
    stage_T<G::D, G::NBW, G::KP>(tab, a.wq + (int64_t)h * a.wq_hs, G::D, a.nb);      // [bucket][d]
    __syncthreads();
    if (kblk * QW + wave >= NT) return;
    F kf[G::KS];
    load_frags<G::KS>(kf, a.k + (int64_t)b * a.sb + (int64_t)h * a.sh + (int64_t)min(kj, a.L - 1) * a.sn, g);
    short* rows = scr + wave * 32 * G::LB;
    lookups_to_lds<G>(rows, tab, kf, a.scale, lane);
    wave_lds_fence();
    lrow_to_global<G::KSB>(dst + ((int64_t)bh * a.NP + kj) * G::NBW, rows + c32 * G::LB, g);
}

// ---------------------------------------------------------------------------------------------------
// backward B: lanes own keys — dk, dv, dLQ
// ---------------------------------------------------------------------------------------------------
template <typename G, bool HQ, bool HK, bool HV> struct LdsB {
    static constexpr int qbuf = 0;                                   // 2 x [32][KP]   (s q) rows
    static constexpr int dobuf = qbuf + 2 * G::TILE;                 // 2 x [32][KP]   dO rows
    static constexpr int stage_end = dobuf + 2 * G::TILE;            // (>= TABB: Wq is staged over the tile area outside the loop)
    static constexpr int lkt = stage_end;                            // 2 x [32 queries][LB]  rpe_k lookups of the query tile
    static constexpr int gt = lkt + (HK ? 2 * 32 * G::LB * 2 : 0);   // 2 x [32 queries][LB]  value-side lookups of dO
    static constexpr int lqk = gt + (HV ? 2 * 32 * G::LB * 2 : 0);   // QW x [32 keys][LB]    rpe_q lookups (own keys)
    static constexpr int dlq = lqk + (HQ ? QW * 32 * G::LB * 2 : 0); // QW x [32 keys][LK] fp32
    static constexpr int stats = dlq + (HQ ? QW * 32 * G::LK * 4 : 0); // lse*log2e [NP], delta [NP]
    static constexpr int fixed = stats;
    static_assert(fixed + MAXNP * 8 <= 160 * 1024, "LDS of a CU");
};

template <typename G, bool HQ, bool HK, bool HV, bool DROP>
__global__ __launch_bounds__(256) void irpe_x_bwd_kv_kernel(const Args a) {
    using L = LdsB<G, HQ, HK, HV>;
    constexpr int D = G::D, KP = G::KP, LBP = G::LB, LKP = G::LK, KS = G::KS, DT = G::DT, NBW = G::NBW;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NT = a.NP >> 5, KB = (NT + QW - 1) / QW;
    const int lb = xcd_order(blockIdx.x, gridDim.x);
    const int bh = lb / KB, kblk = lb - bh * KB;
    const int b = bh / a.H, h = bh - b * a.H;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const int k0 = kblk * 32 * QW;
    const bool active = kblk * QW + wave < NT;
    const int kj = k0 + wave * 32 + c32;
    const bool kok = active && kj < a.L;
    const int kcl = min(kj, a.L - 1);
    // this lane's key takes part: inside the sequence and not padded.  A masked key keeps p = 0 for every query: dk = dv = 0
    // and a zero dLQ row, exactly.
    const bool kreal = kok && !(a.pad && a.pad[(int64_t)b * a.pad_sb + kcl]);

    const int64_t base = (int64_t)b * a.sb + (int64_t)h * a.sh;
    const short* qp = a.q + base;
    const short* dop = a.dout + (int64_t)b * a.dosb + (int64_t)h * D;
    const short* lkg = a.lkg + (int64_t)bh * a.NP * NBW;
    const short* gg = a.gg + (int64_t)bh * a.NP * NBW;

    short* qbuf = reinterpret_cast<short*>(smem + L::qbuf);
    short* dobuf = reinterpret_cast<short*>(smem + L::dobuf);
    short* tab0 = reinterpret_cast<short*>(smem);
    short* lkt = reinterpret_cast<short*>(smem + L::lkt);
    short* gt = reinterpret_cast<short*>(smem + L::gt);
    short* lqw = reinterpret_cast<short*>(smem + L::lqk) + wave * 32 * LBP;
    float* dlqw = reinterpret_cast<float*>(smem + L::dlq) + wave * 32 * LKP;
    float* lse_s = reinterpret_cast<float*>(smem + L::stats);
    float* delta_s = lse_s + a.NP;

    // ---- prologue ---------------------------------------------------------------------------------
    F kf[KS], vf[KS];
    load_frags<KS>(kf, a.k + base + (int64_t)kcl * a.sn, g);
    load_frags<KS>(vf, a.v + base + (int64_t)kcl * a.sn, g);
    for (int i = threadIdx.x; i < a.NP; i += 256) {
        lse_s[i] = i < a.L ? a.lse[(int64_t)bh * a.L + i] * LOG2E : INFINITY;
        delta_s[i] = a.delta[(int64_t)bh * a.NP + i];
    }
    if constexpr (HQ) {
        if (a.wq) stage_T<D, NBW, KP>(tab0, a.wq + (int64_t)h * a.wq_hs, D, a.nb);      // [bucket][d]
        for (int i = lane; i < 32 * LKP; i += 64) dlqw[i] = 0.f;
        __syncthreads();
        if (active) {
            if (a.wq) {
                // (k Wq) * scale: product first, scale after, rounded once — bit for bit the rows lq_tile (forward) and
                // irpe_x_lq_rows_kernel (launch A) use, also for a scale that is no power of two (bf16(k * scale) Wq is not)
                lookups_to_lds<G>(lqw, tab0, kf, a.scale, lane);
            } else {
                bias_rows_to_lds<G>(lqw, a.bq + (int64_t)h * a.bq_hs, a.nb, lane);
            }
            wave_lds_fence();
        }
    }
    __syncthreads();
    struct Stage { Rows<D> q, dout; Rows<NBW> lk, gl; u32x4v ik, iv, iq; } st;
    u32x4v cik = {}, ciq = {}, civ = {};
    auto issue = [&](Stage& r, int t) {
        r.q = rows_scaled<D>(rows_load<D>(qp, a.sn, t * 32, a.L, false), a.scale);
        r.dout = rows_load<D>(dop, a.dosn, t * 32, a.L, true);
        if constexpr (HK) r.lk = rows_load<NBW>(lkg, NBW, t * 32, a.NP, false);
        if constexpr (HV) r.gl = rows_load<NBW>(gg, NBW, t * 32, a.NP, false);
        if constexpr (HK) r.ik = ids_load(a.idk_t, a.NP, kj, t, g);
        if constexpr (HQ) r.iq = ids_load(a.idq_t, a.NP, kj, t, g);
        if constexpr (HV) r.iv = ids_load(a.idv_t, a.NP, kj, t, g);
    };
    auto commit = [&](const Stage& r, int t) {
        const int buf = t & 1;
        rows_store<D, KP>(qbuf + buf * 32 * KP, r.q);
        rows_store<D, KP>(dobuf + buf * 32 * KP, r.dout);
        if constexpr (HK) lrows_store<NBW, LBP>(lkt + buf * 32 * LBP, r.lk);
        if constexpr (HV) lrows_store<NBW, LBP>(gt + buf * 32 * LBP, r.gl);
        if constexpr (HK) cik = r.ik;
        if constexpr (HQ) ciq = r.iq;
        if constexpr (HV) civ = r.iv;
    };
    issue(st, 0);
    commit(st, 0);
    __syncthreads();

    // ---- query tiles --------------------------------------------------------------------------------
    f32x16 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { dk[dt] = f32x16{}; dv[dt] = f32x16{}; }
    for (int t = 0; t < NT; ++t) {
        const int cur = t & 1;
        if (t + 1 < NT) issue(st, t + 1);
        if (active) {
            // rows = queries of the tile, column = own key: own lookups = rpe_q, side lookups = rpe_k
            f32x16 s = score_tile<G, HQ, HK>(qbuf + cur * 32 * KP, kf, ciq, cik, lqw + c32 * LBP, lkt + cur * 32 * LBP, lane);
            f32x16 dp = {};
            const short* db = dobuf + cur * 32 * KP;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) dp = TT::mma(TT::load(db + c32 * KP + ks * 16 + g * 8), vf[ks], dp);
            if constexpr (HV) {
                const short* side = gt + cur * 32 * LBP;
#pragma unroll
                for (int r = 0; r < 16; ++r) dp[r] = add_bf16_at(dp[r], side + acc_row(r, g) * LBP, off2_of(civ, r));
            }
            f32x16 ds;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const f32x4v ls = *reinterpret_cast<const f32x4v*>(lse_s + t * 32 + 8 * rr + 4 * g);
                const f32x4v dl = *reinterpret_cast<const f32x4v*>(delta_s + t * 32 + 8 * rr + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * rr + e;
                    const bool ok = kreal && !(a.causal && t * 32 + acc_row(r, g) < kj);      // (a query before this lane's key)
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], LOG2E, -ls[e]));
                    float dpr = dp[r], pd = p;
                    if constexpr (DROP) {                                          // dv takes the dropped map, dS the mask on dP
                        const bool keep = drop_keep(drop_key(a.drop_seed, bh), t * 32 + acc_row(r, g), kj, a.drop_thr);
                        dpr = keep ? dpr * a.drop_scale : 0.f;
                        pd = keep ? p * a.drop_scale : 0.f;
                    }
                    s[r] = ok ? pd : 0.f;
                    ds[r] = ok ? p * (dpr - dl[e]) : 0.f;
                }
            }
            if constexpr (HQ) scatter_add16(dlqw + c32 * LKP, ciq, ds, g);
            const short* qb = qbuf + cur * 32 * KP;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const F pb = TT::from_acc(s, s2);
                const F sb = TT::from_acc(ds, s2);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    dv[dt] = TT::mma(load_perm_tr<KP>(db, dt, s2, lane), pb, dv[dt]);
                    dk[dt] = TT::mma(load_perm_tr<KP>(qb, dt, s2, lane), sb, dk[dt]);
                }
            }
        }
        if (t + 1 < NT) {
            commit(st, t + 1);
            __syncthreads();
        }
    }

    // ---- dk += s dLQ Wq^T; bucket gradient rows out ------------------------------------------------
    if constexpr (HQ) {
        const bool ctx = a.wq != nullptr;
        if (ctx) {
            __syncthreads();
            stage_R<D, NBW, G::WP>(tab0, a.wq + (int64_t)h * a.wq_hs, D, a.nb);  // [d][bucket]
            __syncthreads();
        }
        if (active) {
            const float* row = dlqw + c32 * LKP;
            short* dst = a.dlq + ((int64_t)bh * a.NP + kj) * NBW;
#pragma unroll
            for (int ks = 0; ks < G::KSB; ++ks) {
                *reinterpret_cast<F*>(dst + ks * 16 + g * 8) = srow_frag<LKP>(row, ks, g, 1.f);
                if (ctx) {
                    const F db = srow_frag<LKP>(row, ks, g, a.scale);
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) dk[dt] = TT::mma(TT::load(tab0 + (c32 + 32 * dt) * G::WP + ks * 16 + g * 8), db, dk[dt]);
                }
            }
        }
    }
    if (kok) {
        const int64_t off = (int64_t)b * a.dsb + (int64_t)kj * a.dsn + (int64_t)h * a.dsh;
        store_row<DT>(a.dk + off, dk, g, 1.f);
        store_row<DT>(a.dv + off, dv, g, 1.f);
    }
}

// ---------------------------------------------------------------------------------------------------
// table gradients: out[bh][x][y] = mul * sum_i X[b,i,h][x] * Y[b,i,h][y]     (XA x YC per (b,h); XA, YC in 32 | 64 | 128)
// ---------------------------------------------------------------------------------------------------
struct TgArgs {
    const short *x, *y;
    int64_t xsb, xsn, xsh, ysb, ysn, ysh;
    float* out;
    int H, L;
    float mul;
};
constexpr int TGP = 40;      // pitch of the transposed tiles here: rows are read 16 bytes at a time

template <int XA, int YC>
__global__ __launch_bounds__(256) void irpe_x_table_grad_kernel(const TgArgs a) {
    __shared__ __attribute__((aligned(16))) short xt[2][XA * TGP];
    __shared__ __attribute__((aligned(16))) short yt[2][YC * TGP];
    constexpr int TA = XA / 32, TC = YC / 32, NTL = TA * TC, PER = (NTL + 3) / 4;      // 32 x 32 output tiles, PER per wave
    const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const short* xp = a.x + (int64_t)b * a.xsb + (int64_t)h * a.xsh;
    const short* yp = a.y + (int64_t)b * a.ysb + (int64_t)h * a.ysh;
    const int NT = (a.L + 31) >> 5;
    Rows<XA> sx = rows_load<XA>(xp, a.xsn, 0, a.L, true);
    Rows<YC> sy = rows_load<YC>(yp, a.ysn, 0, a.L, true);
    rows_store_T<XA, TGP>(xt[0], sx);
    rows_store_T<YC, TGP>(yt[0], sy);
    __syncthreads();
    f32x16 acc[PER];
#pragma unroll
    for (int p = 0; p < PER; ++p) acc[p] = f32x16{};
    for (int t = 0; t < NT; ++t) {
        const int cur = t & 1;
        if (t + 1 < NT) {
            sx = rows_load<XA>(xp, a.xsn, (t + 1) * 32, a.L, true);
            sy = rows_load<YC>(yp, a.ysn, (t + 1) * 32, a.L, true);
        }
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int tile = wave + 4 * p;
            if (tile < NTL) {
                const int ta = tile % TA, tc = tile / TA;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    acc[p] = TT::mma(TT::load(xt[cur] + (ta * 32 + c32) * TGP + ks * 16 + g * 8),
                                     TT::load(yt[cur] + (tc * 32 + c32) * TGP + ks * 16 + g * 8), acc[p]);
            }
        }
        if (t + 1 < NT) {
            rows_store_T<XA, TGP>(xt[cur ^ 1], sx);
            rows_store_T<YC, TGP>(yt[cur ^ 1], sy);
            __syncthreads();
        }
    }
    float* o = a.out + (int64_t)bh * XA * YC;
#pragma unroll
    for (int p = 0; p < PER; ++p) {
        const int tile = wave + 4 * p;
        if (tile < NTL) {
            const int ta = tile % TA, tc = tile / TA;
#pragma unroll
            for (int r = 0; r < 16; ++r) o[(ta * 32 + acc_row(r, g)) * YC + tc * 32 + c32] = acc[p][r] * a.mul;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------
template <typename K>
int launch(K kern, const Args& a, size_t lds, hipStream_t st) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
        return CREAM_ERR_LAUNCH;
    const int NT = a.NP >> 5, QB = (NT + QW - 1) / QW;
    hipLaunchKernelGGL(kern, dim3(a.B * a.H * QB), dim3(256), lds, st, a);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

template <typename G, bool HQ, bool HK, bool HV> int run_fwd(const Args& a, hipStream_t st) {
    return a.drop_thr ? launch(irpe_x_fwd_kernel<G, HQ, HK, HV, true>, a, LdsF<G, HQ, HK, HV>::total, st)
                      : launch(irpe_x_fwd_kernel<G, HQ, HK, HV, false>, a, LdsF<G, HQ, HK, HV>::total, st);
}
template <typename G, bool HQ, bool HK, bool HV> int run_bwd(const Args& a, hipStream_t st) {
    if (HQ && a.wq) {                                  // rpe_q lookup rows of the keys for launch A, in the buffer launch B fills last
        const int NT = a.NP >> 5, KB = (NT + QW - 1) / QW;
        hipLaunchKernelGGL(irpe_x_lq_rows_kernel<G>, dim3(a.B * a.H * KB), dim3(256), 0, st, a, a.dlq);
        if (hipGetLastError() != hipSuccess) return CREAM_ERR_LAUNCH;
    }
    const size_t ldsb = LdsB<G, HQ, HK, HV>::fixed + (size_t)a.NP * 8;
    int rc = a.drop_thr ? launch(irpe_x_bwd_q_kernel<G, HQ, HK, HV, true>, a, LdsA<G, HQ, HK, HV>::total, st)
                        : launch(irpe_x_bwd_q_kernel<G, HQ, HK, HV, false>, a, LdsA<G, HQ, HK, HV>::total, st);
    if (rc) return rc;
    return a.drop_thr ? launch(irpe_x_bwd_kv_kernel<G, HQ, HK, HV, true>, a, ldsb, st)
                      : launch(irpe_x_bwd_kv_kernel<G, HQ, HK, HV, false>, a, ldsb, st);
}

// every subset of q / k / v at 64 columns; rpe on k alone at 128
template <typename G, bool BWD> int dispatch_terms(const Args& a, hipStream_t st) {
    const int key = ((a.wq || a.bq) ? 4 : 0) | ((a.wk || a.bk) ? 2 : 0) | (a.wv ? 1 : 0);
#define CREAM_X_CASE(K, HQ, HK, HV) \
    case K: return BWD ? run_bwd<G, HQ, HK, HV>(a, st) : run_fwd<G, HQ, HK, HV>(a, st);
    if constexpr (G::NBW == 128) {
        switch (key) {
            CREAM_X_CASE(2, false, true, false)
            default: return CREAM_ERR_BAD_ARG;
        }
    } else {
        switch (key) {
            CREAM_X_CASE(0, false, false, false)
            CREAM_X_CASE(1, false, false, true)
            CREAM_X_CASE(2, false, true, false)
            CREAM_X_CASE(3, false, true, true)
            CREAM_X_CASE(4, true, false, false)
            CREAM_X_CASE(5, true, false, true)
            CREAM_X_CASE(6, true, true, false)
            default: return BWD ? run_bwd<G, true, true, true>(a, st) : run_fwd<G, true, true, true>(a, st);
        }
    }
#undef CREAM_X_CASE
}
template <bool BWD> int dispatch(const Args& a, int head_dim, int row_width, hipStream_t st) {
    if (head_dim == 32) return row_width == 64 ? dispatch_terms<Geo<32, 64>, BWD>(a, st) : dispatch_terms<Geo<32, 128>, BWD>(a, st);
    return row_width == 64 ? dispatch_terms<Geo<64, 64>, BWD>(a, st) : dispatch_terms<Geo<64, 128>, BWD>(a, st);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check(const cream_irpe_attn2_desc* x, bool bwd) {
    if (!x) return CREAM_ERR_BAD_ARG;
    const cream_irpe_attn_desc* d = &x->base;
    if (!d->q || !d->k || !d->v || !d->out || !d->lse) return CREAM_ERR_BAD_ARG;
    if (x->head_dim != 32 && x->head_dim != 64) return CREAM_ERR_BAD_ARG;
    if (x->row_width != 64 && x->row_width != 128) return CREAM_ERR_BAD_ARG;
    if (d->B <= 0 || d->H <= 0 || d->L <= 0 || d->nb <= 0 || d->nb > x->row_width) return CREAM_ERR_BAD_ARG;
    if (d->NP != (d->L + 31) / 32 * 32) return CREAM_ERR_BAD_ARG;
    if (d->NP > MAXNP) return CREAM_ERR_TOO_LARGE;
    if (!(d->dropout_p >= 0.f) || d->dropout_p >= 1.f) return CREAM_ERR_BAD_ARG;
    if (d->sn % 8 || d->sh % 8 || d->sb % 8 || !aligned16(d->q) || !aligned16(d->k) || !aligned16(d->v) || !aligned16(d->out))
        return CREAM_ERR_BAD_ARG;
    if ((x->osb || x->osn) && (x->osb % 8 || x->osn % 8 || x->osn < (int64_t)d->H * x->head_dim)) return CREAM_ERR_BAD_ARG;
    const bool hq = d->wq != nullptr || d->bq != nullptr, hk = d->wk != nullptr || d->bk != nullptr, hv = d->wv != nullptr;
    if ((d->wq && d->bq) || (d->wk && d->bk)) return CREAM_ERR_BAD_ARG;
    if (x->row_width == 128 && (hq || hv || !hk)) return CREAM_ERR_BAD_ARG;      // 128 columns: rpe on k alone
    if ((hq && !d->idq) || (hk && !d->idk) || (hv && (!d->idv || !d->sv))) return CREAM_ERR_BAD_ARG;
    if ((hq && !aligned16(d->idq)) || (hk && !aligned16(d->idk)) || (hv && !aligned16(d->idv))) return CREAM_ERR_BAD_ARG;
    if (bwd) {
        if (!d->dout || !d->dq || !d->dk || !d->dv || !d->delta) return CREAM_ERR_BAD_ARG;
        if (d->dsn % 4 || d->dsh % 4 || d->dsb % 4 || !aligned16(d->dout)) return CREAM_ERR_BAD_ARG;
        if ((x->dosb || x->dosn) && (x->dosb % 8 || x->dosn % 8 || x->dosn < (int64_t)d->H * x->head_dim)) return CREAM_ERR_BAD_ARG;
        if ((hq && (!d->idq_t || !d->dlq)) || (hk && (!d->idk_t || !d->lkg || !d->dlk)) || (hv && (!d->idv_t || !d->gg)))
            return CREAM_ERR_BAD_ARG;
        if ((hq && !aligned16(d->idq_t)) || (hk && !aligned16(d->idk_t)) || (hv && !aligned16(d->idv_t))) return CREAM_ERR_BAD_ARG;
    }
    return CREAM_OK;
}

Args to_args(const cream_irpe_attn2_desc* x) {
    const cream_irpe_attn_desc* d = &x->base;
    Args a{};
    a.q = (const short*)d->q; a.k = (const short*)d->k; a.v = (const short*)d->v;
    a.sb = d->sb; a.sn = d->sn; a.sh = d->sh;
    a.out = (short*)d->out; a.lse = d->lse; a.sv = (short*)d->sv;
    const int64_t row = (int64_t)d->H * x->head_dim;
    a.osn = x->osn ? x->osn : row;       a.osb = (x->osb || x->osn) ? x->osb : row * d->L;
    a.dosn = x->dosn ? x->dosn : row;    a.dosb = (x->dosb || x->dosn) ? x->dosb : row * d->L;
    a.wq = d->wq; a.wk = d->wk; a.wv = d->wv;
    a.wq_hs = d->wq_hs; a.wk_hs = d->wk_hs; a.wv_hs = d->wv_hs;
    a.bq = d->bq; a.bk = d->bk; a.bq_hs = d->bq_hs; a.bk_hs = d->bk_hs;
    a.idq = d->idq; a.idk = d->idk; a.idv = d->idv;
    a.idq_t = d->idq_t; a.idk_t = d->idk_t; a.idv_t = d->idv_t;
    a.pad = x->key_pad; a.pad_sb = x->key_pad_sb;
    a.B = d->B; a.H = d->H; a.L = d->L; a.NP = d->NP; a.nb = d->nb; a.scale = d->scale; a.causal = d->causal;
    a.drop_thr = drop_threshold(d->dropout_p);
    a.drop_seed = d->dropout_seed;
    a.drop_scale = 1.f / (1.f - d->dropout_p);
    a.dout = (const short*)d->dout;
    a.dq = (short*)d->dq; a.dk = (short*)d->dk; a.dv = (short*)d->dv;
    a.dsb = d->dsb; a.dsn = d->dsn; a.dsh = d->dsh;
    a.delta = d->delta; a.lkg = (short*)d->lkg; a.gg = (short*)d->gg; a.dlk = (short*)d->dlk; a.dlq = (short*)d->dlq;
    return a;
}

template <int XA> int table_grad_y(const TgArgs& a, int yc, int BH, hipStream_t st) {
    switch (yc) {
        case 32: hipLaunchKernelGGL((irpe_x_table_grad_kernel<XA, 32>), dim3(BH), dim3(256), 0, st, a); break;
        case 64: hipLaunchKernelGGL((irpe_x_table_grad_kernel<XA, 64>), dim3(BH), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((irpe_x_table_grad_kernel<XA, 128>), dim3(BH), dim3(256), 0, st, a); break;
    }
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

}  // namespace

extern "C" {

int cream_irpe_attn2_check(const cream_irpe_attn2_desc* d, int backward) { return check(d, backward != 0); }

int cream_irpe_attn2_fwd(const cream_irpe_attn2_desc* d, void* stream)
{
    const int rc = check(d, false);
    if (rc) return rc;
    return dispatch<false>(to_args(d), d->head_dim, d->row_width, (hipStream_t)stream);
}

int cream_irpe_attn2_bwd(const cream_irpe_attn2_desc* d, void* stream)
{
    const int rc = check(d, true);
    if (rc) return rc;
    return dispatch<true>(to_args(d), d->head_dim, d->row_width, (hipStream_t)stream);
}

int cream_irpe_table_grad2(float* out, const void* x, int64_t xsb, int64_t xsn, int64_t xsh, int xa, const void* y, int64_t ysb,
                           int64_t ysn, int64_t ysh, int yc, int B, int H, int L, float mul, void* stream)
{
    if (!out || !x || !y || B <= 0 || H <= 0 || L <= 0) return CREAM_ERR_BAD_ARG;
    if ((xa != 32 && xa != 64 && xa != 128) || (yc != 32 && yc != 64 && yc != 128)) return CREAM_ERR_BAD_ARG;
    if (xsn % 8 || xsh % 8 || xsb % 8 || ysn % 8 || ysh % 8 || ysb % 8 || !aligned16(x) || !aligned16(y)) return CREAM_ERR_BAD_ARG;
    TgArgs a{(const short*)x, (const short*)y, xsb, xsn, xsh, ysb, ysn, ysh, out, H, L, mul};
    switch (xa) {
        case 32: return table_grad_y<32>(a, yc, B * H, (hipStream_t)stream);
        case 64: return table_grad_y<64>(a, yc, B * H, (hipStream_t)stream);
        default: return table_grad_y<128>(a, yc, B * H, (hipStream_t)stream);
    }
}

}  // extern "C"

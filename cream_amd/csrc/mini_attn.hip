// mini_attn.hip — fused Mini-DeiT attention with the two head-mixing 1x1 convolutions (conv_l before the softmax,
// conv_w after it) and contextual iRPE on keys, forward and backward, for gfx950 (MI355X).
//
// Reference semantics (MiniViT/Mini-DeiT/mini_vision_transformer.py:84-114), per image, H heads, head_dim 64,
// s = scale, Wl = conv_l.weight[:, :, 0, 0], Ww = conv_w.weight[:, :, 0, 0] (H x H fp32, [out][in]):
//     S_h[i,j]  = (s q_h,i).k_h,j + LK_h[i, idk[i,j]]          LK_h = (s q_h) Wk   (absent without rpe_k)
//     S'_o      = sum_h Wl[o,h] S_h
//     P_o       = softmax_j(S'_o)
//     P'_o      = sum_h Ww[o,h] P_h
//     O_o,i     = sum_j P'_o[i,j] v_o,j
// Both mixes are pointwise in (i, j); only the softmax couples keys.  So a (32 queries x 32 keys) block that carries ALL heads is
// self-contained once the row statistics of S' are known, and nothing of size L^2 leaves the chip.
//
// Shape of the kernels.  One workgroup = 4 waves owns (image, 32 tokens) with all heads; wave w owns heads w, w + 4, w + 8
// (HPW = ceil(H / 4) head slots, a template parameter).  A wave computes the 32 x 32 tile of each of its heads with the
// swapped product of attn_common.hpp (a lane holds 16 partners of ONE own token), then the waves exchange their tiles through
// one fp32 LDS buffer X[h][16][64 lanes] (the accumulator layout itself, 16-byte accesses, no bank conflicts) and every wave
// mixes the tiles of ALL heads into those of its OWN heads on the VALU: 2 H^2 FMAs per (i, j) per mix, with the weights as
// wave-uniform scalars.  (An MFMA with heads as the contraction would need the heads on the lane axis, i.e. a transposing
// exchange for a contraction of at most 12; the VALU form needs no relayout.)  The streamed side (K, V, or q, dO for the
// key-owned launch) comes straight from global memory as the A operand (16 bytes per lane, L2-resident); only the tiles that
// are contracted over their ROWS (P'.V, dS.K, ...) are staged, per wave, for the transposing LDS read.  The exchange
// (xchg_put / xchg_mix) and the bucket-id and scatter-add helpers are in attn_lane.hpp.
//
// Forward: two passes over the keys (pass 1: running max / sum of S' per (o, i); pass 2: P from the final statistics, P', P'.V) —
// conv_w mixes rows normalised by different sums, so a one-pass online softmax would need H^2 cross accumulators.
// Keys past L are masked AFTER conv_l (on S'): -inf in S would meet negative mixing weights.  P' may be negative.
//
// Backward, with dP'_o[i,j] = dO_o,i . v_o,j:
//     dP_h = sum_o Ww[o,h] dP'_o      delta_h[i] = sum_j P_h dP_h       dS'_h = P_h (dP_h - delta_h)
//     dS_h = sum_o Wl[o,h] dS'_o      dLK_h[i,u] = sum_{j: idk[i,j]=u} dS_h[i,j]
//     dq_h = s (dS_h k_h + dLK_h Wk^T)   dk_h = dS_h^T (s q_h)   dv_o = P'_o^T dO_o
//     dWl[o,h] = sum_ij dS'_o S_h        dWw[o,h] = sum_ij dP'_o P_h     dWk = (s q)^T dLK (cream_irpe_table_grad)
//   launch D (lanes own queries): delta, the LK rows for launch K, per-workgroup partials of dWw;
//   launch Q (lanes own queries; one launch per head slot, the fp32 bucket-gradient rows of 4 heads fit in LDS beside the
//             exchange buffer, those of 12 do not): dq, dLK rows, and (slot 0) per-workgroup partials of dWl;
//   launch K (lanes own keys): dk, dv.
// No global atomics: every reduction has a fixed order (the partials are summed by the caller).
#include <hip/hip_runtime.h>
#include <hip/hip_bfloat16.h>
#include <stdint.h>

#include "attn_lane.hpp"
#include "cream_amd.h"

namespace {
using namespace cream;

constexpr float LOG2E = 1.4426950408889634f;
constexpr int KP = 72;      // pitch (bf16) of staged row-major [32][64] tiles
constexpr int LBP = 66;     // pitch (bf16) of lookup rows: 33 words
constexpr int LKP = 65;     // pitch (fp32) of bucket-gradient rows
constexpr int MAXH = 12;

struct Args {
    const short *q, *k, *v;
    int64_t sb, sn, sh;
    short* out;                       // (B, L, H, 64)
    float* lse;                       // (B, H, L) of the MIXED logits S'
    const float* wk;                  // (H', 64, nb) fp32 or null
    int64_t wk_hs;
    const uint8_t *idk, *idk_t;       // (NP, NP) byte bucket matrices (cream_irpe_bucket_bytes), query- / key-major
    const float *wl, *ww;             // (H, H) fp32 [out][in]
    int B, H, L, NP, nb;
    float scale;
    const short* dout;                // (B, L, H, 64)
    short *dq, *dk, *dv;
    int64_t dsb, dsn, dsh;
    float* delta;                     // (B, H, NP)
    short *lkg, *dlk;                 // (B, H, NP, 64) bf16
    float *dwl_part, *dww_part;       // (B * NP / 32, H, H)
    int slot;                         // launch Q: the head slot whose dq / dLK this launch produces
};

__device__ __forceinline__ void load_frags_scaled(F (&f)[4], const short* row, int g, float s) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) f[ks] = scaled(TT::load(row + ks * 16 + g * 8), s);
}
// acc += (bf16 at byte offset off2 of row) as shift + add: attn_lane.hpp's add_bf16_at (v_dot2c) is another instruction sequence,
// and these kernels were measured with this one
__device__ __forceinline__ float add_bf16_at_shift(float acc, const short* row, int off2) {
    const uint32_t x = *reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(row) + off2);
    return acc + __uint_as_float(x << 16);
}

// tile^T (rows = 32 streamed tokens from row0, column = own token) = A rows (global, 64 wide, clamped to the last real row) . own^T
__device__ __forceinline__ f32x16 stream_tile(const short* base, int64_t rs, int row0, int L, float a_scale, bool scale_a,
                                              const F (&own)[4], int lane) {
    const int c32 = lane & 31, g = lane >> 5;
    const short* rp = base + (int64_t)min(row0 + c32, L - 1) * rs + g * 8;
    f32x16 s = {};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        F aop = TT::load(rp + ks * 16);
        if (scale_a) aop = scaled(aop, a_scale);
        s = TT::mma(aop, own[ks], s);
    }
    return s;
}
// this wave's private copy of a [32][64] tile of global rows (for the transposing read), optionally scaled
__device__ __forceinline__ void stage_tile(short* dst, const short* base, int64_t rs, int row0, int L, float a_scale, bool scale_a,
                                           int lane) {
    wave_lds_fence();                                  // earlier reads of the buffer by this wave are done
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = it * 8 + (lane >> 3), cc = lane & 7;
        F x = TT::load(base + (int64_t)min(row0 + row, L - 1) * rs + cc * 8);
        if (scale_a) x = scaled(x, a_scale);
        *reinterpret_cast<F*>(dst + row * KP + cc * 8) = x;
    }
    wave_lds_fence();
}
// acc^T (64 x own tokens, two 32-row halves) += tile^T (64 x 32 streamed) . p (32 streamed x own), p in accumulator layout
__device__ __forceinline__ void rows_product(f32x16 (&acc)[2], const short* tile, const f32x16& p, int lane) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const F pb = TT::from_acc(p, s2);
        acc[0] = TT::mma(load_perm_tr(tile, KP, 0, s2, lane), pb, acc[0]);
        acc[1] = TT::mma(load_perm_tr(tile, KP, 1, s2, lane), pb, acc[1]);
    }
}

// lookups^T (64 buckets x 32 own rows) = Wk^T (buckets x 64 d, read from the fp32 table) . X^T -> rows[own row][bucket] (bf16)
__device__ __forceinline__ void lookups_to_lds(short* rows, const float* wk, int nb, const F (&xb)[4], int lane) {
    const int c32 = lane & 31, g = lane >> 5;
    f32x16 a0 = {}, a1 = {};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        f32x8v x0, x1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float* p = wk + (int64_t)(ks * 16 + g * 8 + e) * nb;
            x0[e] = c32 < nb ? p[c32] : 0.f;
            x1[e] = c32 + 32 < nb ? p[c32 + 32] : 0.f;
        }
        a0 = TT::mma(__builtin_bit_cast(F, __builtin_convertvector(x0, hwbf16x8)), xb[ks], a0);
        a1 = TT::mma(__builtin_bit_cast(F, __builtin_convertvector(x1, hwbf16x8)), xb[ks], a1);
    }
    short* row = rows + c32 * LBP;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        row[acc_row(r, g)] = f2bf(a0[r]);
        row[32 + acc_row(r, g)] = f2bf(a1[r]);
    }
}
// the lanes' shares of a weight gradient -> part[row h][column own head], summed over the wave in a fixed butterfly
template <int HPW>
__device__ __forceinline__ void cross_store(float* part, float (&cross)[4 * HPW][HPW], int H, int wave, int lane) {
#pragma unroll
    for (int h = 0; h < 4 * HPW; ++h)
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            float v = cross[h][s];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);        // (wave_sum of lane_ops.hpp, kept inline: the call form schedules these kernels differently)
            const int o = wave + 4 * s;
            if (h < H && o < H && lane == 0) part[h * H + o] = v;
        }
}

struct Lds {
    static __host__ __device__ int x(int H) { return 0; }
    static __host__ __device__ int lk(int H) { return H * 16 * 64 * 4; }                        // [H][32][LBP] bf16
    static __host__ __device__ int stage(int H) { return lk(H) + H * 32 * LBP * 2; }           // 4 x [32][KP] bf16
    static __host__ __device__ int rows(int H) { return stage(H) + 4 * 32 * KP * 2; }          // 4 x [32][LKP] fp32 | [2][H][32] fp32
    static __host__ __device__ int total(int H) { return rows(H) + 4 * 32 * LKP * 4; }
};

// S tiles of this wave's heads for streamed key tile t (lanes own queries): MFMA + the rpe_k gather from the own lookup rows
template <int HPW, bool HK>
__device__ __forceinline__ void own_scores(f32x16 (&S)[HPW], const Args& a, const short* qp, const short* kp, const short* lk, int qi,
                                           int t, const u32x4v& ids, int wave, int lane) {
    const int c32 = lane & 31, g = lane >> 5;
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const int h = wave + 4 * s;
        S[s] = f32x16{};
        if (h < a.H) {
            F qs[4];
            load_frags_scaled(qs, qp + (int64_t)min(qi, a.L - 1) * a.sn + (int64_t)h * a.sh, g, a.scale);
            S[s] = stream_tile(kp + (int64_t)h * a.sh, a.sn, t * 32, a.L, 1.f, false, qs, lane);
            if constexpr (HK) {
                const short* row = lk + (h * 32 + c32) * LBP;
#pragma unroll
                for (int r = 0; r < 16; ++r) S[s][r] = add_bf16_at_shift(S[s][r], row, off2_of(ids, r));
            }
        }
    }
}
// the rpe_k lookup rows of this wave's heads for its 32 queries (wave-private rows of the shared array)
template <int HPW>
__device__ __forceinline__ void own_lookups(short* lk, const Args& a, const short* qp, int b, int qi, bool to_global, int wave, int lane) {
    const int c32 = lane & 31, g = lane >> 5;
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const int h = wave + 4 * s;
        if (h < a.H) {
            F qs[4];
            load_frags_scaled(qs, qp + (int64_t)min(qi, a.L - 1) * a.sn + (int64_t)h * a.sh, g, a.scale);
            lookups_to_lds(lk + h * 32 * LBP, a.wk + (int64_t)h * a.wk_hs, a.nb, qs, lane);
            wave_lds_fence();
            if (to_global) lrow_to_global<4>(a.lkg + (((int64_t)b * a.H + h) * a.NP + qi) * 64, lk + (h * 32 + c32) * LBP, g);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------------
template <int HPW, bool HK>
__global__ __launch_bounds__(256) void mini_attn_fwd_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NT = a.NP >> 5;
    const int b = blockIdx.x / NT, qt = blockIdx.x - b * NT;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const int qi = qt * 32 + c32;
    const bool qok = qi < a.L;
    float* X = reinterpret_cast<float*>(smem + Lds::x(a.H));
    short* lk = reinterpret_cast<short*>(smem + Lds::lk(a.H));
    short* st = reinterpret_cast<short*>(smem + Lds::stage(a.H)) + wave * 32 * KP;
    const short* qp = a.q + (int64_t)b * a.sb;
    const short* kp = a.k + (int64_t)b * a.sb;
    const short* vp = a.v + (int64_t)b * a.sb;

    if constexpr (HK) own_lookups<HPW>(lk, a, qp, b, qi, false, wave, lane);

    // ---- pass 1: running maximum and sum of the mixed logits per (own head, query) ------------------------------------
    float m[HPW], l[HPW];
#pragma unroll
    for (int s = 0; s < HPW; ++s) { m[s] = -INFINITY; l[s] = 0.f; }
    f32x16 S[HPW], Sp[HPW];
    for (int t = 0; t < NT; ++t) {
        u32x4v ids = {};
        if constexpr (HK) ids = ids_load(a.idk, a.NP, qi, t, g);
        own_scores<HPW, HK>(S, a, qp, kp, lk, qi, t, ids, wave, lane);
        xchg_put<HPW>(X, S, 0, a.H, wave, lane);
        xchg_mix<HPW, false>(X, Sp, a.wl, a.H, wave, lane);
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            float tm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (t * 32 + acc_row(r, g) >= a.L) Sp[s][r] = -INFINITY;          // padding keys: masked AFTER conv_l
                tm = fmaxf(tm, Sp[s][r]);
            }
            const float mn = fmaxf(m[s], tm);
            const float ms = mn == -INFINITY ? 0.f : mn;                          // (a lane that has seen no real key yet)
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) ps += __builtin_amdgcn_exp2f((Sp[s][r] - ms) * LOG2E);
            l[s] = l[s] * __builtin_amdgcn_exp2f((m[s] - ms) * LOG2E) + ps;
            m[s] = mn;
        }
    }
    float lse[HPW];
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const float mo = __shfl_xor(m[s], 32), lo = __shfl_xor(l[s], 32);
        const float mn = fmaxf(m[s], mo);                                          // finite: key 0 exists (lane group 0)
        const float lt = l[s] * __builtin_amdgcn_exp2f((m[s] - mn) * LOG2E) + lo * __builtin_amdgcn_exp2f((mo - mn) * LOG2E);
        lse[s] = mn + __logf(lt);
        const int o = wave + 4 * s;
        if (o < a.H && qok && g == 0) a.lse[((int64_t)b * a.H + o) * a.L + qi] = lse[s];
    }

    // ---- pass 2: P from the final statistics, P' = conv_w(P), O = P' V --------------------------------------------------
    f32x16 O[HPW][2];
#pragma unroll
    for (int s = 0; s < HPW; ++s) { O[s][0] = f32x16{}; O[s][1] = f32x16{}; }
    for (int t = 0; t < NT; ++t) {
        u32x4v ids = {};
        if constexpr (HK) ids = ids_load(a.idk, a.NP, qi, t, g);
        own_scores<HPW, HK>(S, a, qp, kp, lk, qi, t, ids, wave, lane);
        xchg_put<HPW>(X, S, 0, a.H, wave, lane);
        xchg_mix<HPW, false>(X, Sp, a.wl, a.H, wave, lane);
#pragma unroll
        for (int s = 0; s < HPW; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                Sp[s][r] = t * 32 + acc_row(r, g) < a.L ? __builtin_amdgcn_exp2f((Sp[s][r] - lse[s]) * LOG2E) : 0.f;
        xchg_put<HPW>(X, Sp, 0, a.H, wave, lane);
        xchg_mix<HPW, false>(X, S, a.ww, a.H, wave, lane);                         // S now holds P'
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = wave + 4 * s;
            if (o < a.H) {
                stage_tile(st, vp + (int64_t)o * a.sh, a.sn, t * 32, a.L, 1.f, false, lane);
                rows_product(O[s], st, S[s], lane);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const int o = wave + 4 * s;
        if (o < a.H && qok) store_row(a.out + (((int64_t)b * a.L + qi) * a.H + o) * 64, O[s], g, 1.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own queries.  MODE 0 (launch D): delta, LK rows to global, dWw partials.  MODE 1 (launch Q): dq and dLK rows of
// head slot a.slot, dWl partials when a.slot == 0.
// ---------------------------------------------------------------------------------------------------------------------------
template <int HPW, bool HK, int MODE>
__global__ __launch_bounds__(256) void mini_attn_bwd_q_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NT = a.NP >> 5;
    const int b = blockIdx.x / NT, qt = blockIdx.x - b * NT;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const int qi = qt * 32 + c32;
    const bool qok = qi < a.L;
    float* X = reinterpret_cast<float*>(smem + Lds::x(a.H));
    short* lk = reinterpret_cast<short*>(smem + Lds::lk(a.H));
    short* st = reinterpret_cast<short*>(smem + Lds::stage(a.H)) + wave * 32 * KP;
    float* dlr = reinterpret_cast<float*>(smem + Lds::rows(a.H)) + wave * 32 * LKP;
    const short* qp = a.q + (int64_t)b * a.sb;
    const short* kp = a.k + (int64_t)b * a.sb;
    const short* vp = a.v + (int64_t)b * a.sb;
    const short* dop = a.dout + (int64_t)b * a.L * a.H * 64;
    const int64_t dos = (int64_t)a.H * 64;
    const bool with_wl = MODE == 1 && a.slot == 0;

    if constexpr (HK) own_lookups<HPW>(lk, a, qp, b, qi, MODE == 0, wave, lane);
    float lse[HPW], dl[HPW], dacc[HPW];
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const int o = min(wave + 4 * s, a.H - 1);
        lse[s] = a.lse[((int64_t)b * a.H + o) * a.L + min(qi, a.L - 1)];
        dl[s] = MODE == 1 ? a.delta[((int64_t)b * a.H + o) * a.NP + qi] : 0.f;
        dacc[s] = 0.f;
    }
    float cross[4 * HPW][HPW];
#pragma unroll
    for (int h = 0; h < 4 * HPW; ++h)
#pragma unroll
        for (int s = 0; s < HPW; ++s) cross[h][s] = 0.f;
    f32x16 dq[2] = {f32x16{}, f32x16{}};
    if constexpr (MODE == 1 && HK) {
        for (int i = lane; i < 32 * LKP; i += 64) dlr[i] = 0.f;
        wave_lds_fence();
    }

    f32x16 S[HPW], P[HPW], T[HPW], U[HPW];
    for (int t = 0; t < NT; ++t) {
        u32x4v ids = {};
        if constexpr (HK) ids = ids_load(a.idk, a.NP, qi, t, g);
        own_scores<HPW, HK>(S, a, qp, kp, lk, qi, t, ids, wave, lane);
        xchg_put<HPW>(X, S, 0, a.H, wave, lane);
        xchg_mix<HPW, false>(X, P, a.wl, a.H, wave, lane);
#pragma unroll
        for (int s = 0; s < HPW; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                P[s][r] = (qok && t * 32 + acc_row(r, g) < a.L) ? __builtin_amdgcn_exp2f((P[s][r] - lse[s]) * LOG2E) : 0.f;
        // dP'_o = dO_o . v_o of the own heads
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = wave + 4 * s;
            T[s] = f32x16{};
            if (o < a.H) {
                F df[4];
                load_frags(df, dop + (int64_t)min(qi, a.L - 1) * dos + o * 64, g);
                T[s] = stream_tile(vp + (int64_t)o * a.sh, a.sn, t * 32, a.L, 1.f, false, df, lane);
            }
        }
        xchg_put<HPW>(X, T, 0, a.H, wave, lane);
        if constexpr (MODE == 0) xchg_mix<HPW, true, true>(X, U, a.ww, a.H, wave, lane, P, cross);      // dP; dWw[o][h] += dP'_o P_h
        else xchg_mix<HPW, true>(X, U, a.ww, a.H, wave, lane);
        if constexpr (MODE == 0) {
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                float d0 = 0.f, d1 = 0.f;
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    d0 = __builtin_fmaf(P[s][r], U[s][r], d0);
                    d1 = __builtin_fmaf(P[s][r + 1], U[s][r + 1], d1);
                }
                dacc[s] += d0 + d1;
            }
        } else {
#pragma unroll
            for (int s = 0; s < HPW; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r) T[s][r] = P[s][r] * (U[s][r] - dl[s]);                     // dS'
            xchg_put<HPW>(X, T, 0, a.H, wave, lane);
            if (with_wl) xchg_mix<HPW, true, true>(X, U, a.wl, a.H, wave, lane, S, cross);              // dS; dWl[o][h] += dS'_o S_h
            else xchg_mix<HPW, true>(X, U, a.wl, a.H, wave, lane);
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int h = wave + 4 * s;
                if (s == a.slot && h < a.H) {
                    stage_tile(st, kp + (int64_t)h * a.sh, a.sn, t * 32, a.L, 1.f, false, lane);
                    rows_product(dq, st, U[s], lane);
                    if constexpr (HK) scatter_add16(dlr + c32 * LKP, ids, U[s], g);
                }
            }
        }
    }

    float* part = (MODE == 0 ? a.dww_part : a.dwl_part) + (int64_t)blockIdx.x * a.H * a.H;
    if constexpr (MODE == 0) {
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = wave + 4 * s;
            const float d = dacc[s] + __shfl_xor(dacc[s], 32);
            if (o < a.H && g == 0) a.delta[((int64_t)b * a.H + o) * a.NP + qi] = d;
        }
        cross_store<HPW>(part, cross, a.H, wave, lane);
    } else {
        if (with_wl) cross_store<HPW>(part, cross, a.H, wave, lane);
        const int h = wave + 4 * a.slot;
        if (h < a.H) {
            if constexpr (HK) {
                // dq^T += Wk (64 d x buckets) . dLK^T (buckets x queries); the bucket-gradient rows go out for the table gradient
                wave_lds_fence();
                const float* row = dlr + c32 * LKP;
                const float* wk = a.wk + (int64_t)h * a.wk_hs;
                short* dst = a.dlk + (((int64_t)b * a.H + h) * a.NP + qi) * 64;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    f32x8v x, w0, w1;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int u = ks * 16 + g * 8 + e;
                        x[e] = row[u];
                        w0[e] = u < a.nb ? wk[(int64_t)c32 * a.nb + u] : 0.f;
                        w1[e] = u < a.nb ? wk[(int64_t)(c32 + 32) * a.nb + u] : 0.f;
                    }
                    const F xb = __builtin_bit_cast(F, __builtin_convertvector(x, hwbf16x8));
                    *reinterpret_cast<F*>(dst + ks * 16 + g * 8) = xb;
                    dq[0] = TT::mma(__builtin_bit_cast(F, __builtin_convertvector(w0, hwbf16x8)), xb, dq[0]);
                    dq[1] = TT::mma(__builtin_bit_cast(F, __builtin_convertvector(w1, hwbf16x8)), xb, dq[1]);
                }
            }
            if (qok) store_row(a.dq + (int64_t)b * a.dsb + (int64_t)qi * a.dsn + (int64_t)h * a.dsh, dq, g, a.scale);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward, lanes own keys (launch K): dk, dv.  Streams query tiles: q and dO rows from global, the LK rows of launch D and the
// lse / delta of the tile's queries through LDS.
// ---------------------------------------------------------------------------------------------------------------------------
template <int HPW, bool HK>
__global__ __launch_bounds__(256) void mini_attn_bwd_kv_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int NT = a.NP >> 5;
    const int b = blockIdx.x / NT, kt = blockIdx.x - b * NT;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, g = lane >> 5, c32 = lane & 31;
    const int kj = kt * 32 + c32;
    const bool kok = kj < a.L;
    float* X = reinterpret_cast<float*>(smem + Lds::x(a.H));
    short* lk = reinterpret_cast<short*>(smem + Lds::lk(a.H));
    short* st = reinterpret_cast<short*>(smem + Lds::stage(a.H)) + wave * 32 * KP;
    float* lse_s = reinterpret_cast<float*>(smem + Lds::rows(a.H));           // [H][32]
    float* dl_s = lse_s + a.H * 32;                                            // [H][32]
    const short* qp = a.q + (int64_t)b * a.sb;
    const short* kp = a.k + (int64_t)b * a.sb;
    const short* vp = a.v + (int64_t)b * a.sb;
    const short* dop = a.dout + (int64_t)b * a.L * a.H * 64;
    const int64_t dos = (int64_t)a.H * 64;

    f32x16 dk[HPW][2], dv[HPW][2];
#pragma unroll
    for (int s = 0; s < HPW; ++s) { dk[s][0] = f32x16{}; dk[s][1] = f32x16{}; dv[s][0] = f32x16{}; dv[s][1] = f32x16{}; }
    f32x16 S[HPW], P[HPW], T[HPW];
    for (int t = 0; t < NT; ++t) {
        __syncthreads();                               // the previous tile's rows and statistics are no longer read
        if constexpr (HK) {
            for (int idx = threadIdx.x; idx < a.H * 256; idx += 256) {
                const int h = idx >> 8, row = (idx >> 3) & 31, cc = idx & 7;
                const u32x4v x = *reinterpret_cast<const u32x4v*>(a.lkg + (((int64_t)b * a.H + h) * a.NP + t * 32 + row) * 64 + cc * 8);
                uint32_t* d = reinterpret_cast<uint32_t*>(lk + (h * 32 + row) * LBP + cc * 8);
                d[0] = x[0]; d[1] = x[1]; d[2] = x[2]; d[3] = x[3];
            }
        }
        for (int idx = threadIdx.x; idx < a.H * 32; idx += 256) {
            const int h = idx >> 5, i = t * 32 + (idx & 31);
            lse_s[idx] = a.lse[((int64_t)b * a.H + h) * a.L + min(i, a.L - 1)];
            dl_s[idx] = a.delta[((int64_t)b * a.H + h) * a.NP + i];
        }
        __syncthreads();
        u32x4v ids = {};
        if constexpr (HK) ids = ids_load(a.idk_t, a.NP, kj, t, g);
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int h = wave + 4 * s;
            S[s] = f32x16{};
            __builtin_amdgcn_sched_barrier(0);
            if (h < a.H) {
                F kf[4];
                load_frags(kf, kp + (int64_t)min(kj, a.L - 1) * a.sn + (int64_t)h * a.sh, g);
                S[s] = stream_tile(qp + (int64_t)h * a.sh, a.sn, t * 32, a.L, a.scale, true, kf, lane);
                if constexpr (HK) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        S[s][r] = add_bf16_at_shift(S[s][r], lk + (h * 32 + acc_row(r, g)) * LBP, off2_of(ids, r));
                }
            }
        }
        xchg_put<HPW>(X, S, 0, a.H, wave, lane);
        xchg_mix<HPW, false>(X, P, a.wl, a.H, wave, lane);
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = min(wave + 4 * s, a.H - 1);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                P[s][r] = (kok && t * 32 + acc_row(r, g) < a.L)
                              ? __builtin_amdgcn_exp2f((P[s][r] - lse_s[o * 32 + acc_row(r, g)]) * LOG2E) : 0.f;
        }
        xchg_put<HPW>(X, P, 0, a.H, wave, lane);
        xchg_mix<HPW, false>(X, S, a.ww, a.H, wave, lane);                         // P'
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = wave + 4 * s;
            T[s] = f32x16{};
            __builtin_amdgcn_sched_barrier(0);         // one head slot at a time: hoisting every slot's loads costs the registers
            if (o < a.H) {
                stage_tile(st, dop + o * 64, dos, t * 32, a.L, 1.f, false, lane);
                rows_product(dv[s], st, S[s], lane);                                // dv_o^T += dO_o^T P'_o^T
                F vf[4];
                load_frags(vf, vp + (int64_t)min(kj, a.L - 1) * a.sn + (int64_t)o * a.sh, g);
                T[s] = stream_tile(dop + o * 64, dos, t * 32, a.L, 1.f, false, vf, lane);   // dP'_o
            }
        }
        xchg_put<HPW>(X, T, 0, a.H, wave, lane);
        xchg_mix<HPW, true>(X, S, a.ww, a.H, wave, lane);                          // dP
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int o = min(wave + 4 * s, a.H - 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) T[s][r] = P[s][r] * (S[s][r] - dl_s[o * 32 + acc_row(r, g)]);   // dS'
        }
        xchg_put<HPW>(X, T, 0, a.H, wave, lane);
        xchg_mix<HPW, true>(X, S, a.wl, a.H, wave, lane);                          // dS
#pragma unroll
        for (int s = 0; s < HPW; ++s) {
            const int h = wave + 4 * s;
            __builtin_amdgcn_sched_barrier(0);
            if (h < a.H) {
                stage_tile(st, qp + (int64_t)h * a.sh, a.sn, t * 32, a.L, a.scale, true, lane);
                rows_product(dk[s], st, S[s], lane);                                // dk_h^T += (s q_h)^T dS_h^T
            }
        }
    }
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const int h = wave + 4 * s;
        if (h < a.H && kok) {
            store_row(a.dk + (int64_t)b * a.dsb + (int64_t)kj * a.dsn + (int64_t)h * a.dsh, dk[s], g, 1.f);
            store_row(a.dv + (int64_t)b * a.dsb + (int64_t)kj * a.dsn + (int64_t)h * a.dsh, dv[s], g, 1.f);
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------
template <typename K> int launch(K kern, const Args& a, int blocks, hipStream_t st) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return CREAM_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), (size_t)Lds::total(a.H), st, a);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}
template <int HPW, bool HK> int run_fwd(const Args& a, hipStream_t st) {
    return launch(mini_attn_fwd_kernel<HPW, HK>, a, a.B * (a.NP >> 5), st);
}
template <int HPW, bool HK> int run_bwd(Args a, hipStream_t st) {
    const int blocks = a.B * (a.NP >> 5);
    int rc = launch(mini_attn_bwd_q_kernel<HPW, HK, 0>, a, blocks, st);
    for (int slot = 0; slot < HPW && !rc; ++slot) {
        if (4 * slot >= a.H) break;
        a.slot = slot;
        rc = launch(mini_attn_bwd_q_kernel<HPW, HK, 1>, a, blocks, st);
    }
    if (rc) return rc;
    return launch(mini_attn_bwd_kv_kernel<HPW, HK>, a, blocks, st);
}
template <bool BWD> int dispatch(const Args& a, hipStream_t st) {
    const int hpw = (a.H + 3) / 4;
    const bool hk = a.wk != nullptr;
#define MINI_CASE(N)                                                                                     \
    case N:                                                                                              \
        if (BWD) return hk ? run_bwd<N, true>(a, st) : run_bwd<N, false>(a, st);                         \
        return hk ? run_fwd<N, true>(a, st) : run_fwd<N, false>(a, st);
    switch (hpw) {
        MINI_CASE(1)
        MINI_CASE(2)
        default:
        MINI_CASE(3)
    }
#undef MINI_CASE
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

int check(const cream_mini_attn_desc* d, bool bwd) {
    if (!d || !d->q || !d->k || !d->v || !d->lse || (!bwd && !d->out)) return CREAM_ERR_BAD_ARG;
    if (d->head_dim != 64 || d->B <= 0 || d->H <= 0 || d->H > MAXH || d->L <= 0 || d->nb <= 0 || d->nb > 64) return CREAM_ERR_BAD_ARG;
    if (!d->wl || !d->ww) return CREAM_ERR_BAD_ARG;
    if (d->NP != (d->L + 31) / 32 * 32) return CREAM_ERR_BAD_ARG;
    if (d->NP > 2048) return CREAM_ERR_TOO_LARGE;
    if (d->sn % 8 || d->sh % 8 || d->sb % 8 || !aligned16(d->q) || !aligned16(d->k) || !aligned16(d->v) || (!bwd && !aligned16(d->out)))
        return CREAM_ERR_BAD_ARG;
    if (!aligned4(d->lse) || !aligned4(d->wl) || !aligned4(d->ww) || (d->wk && !aligned4(d->wk))) return CREAM_ERR_BAD_ARG;
    if (d->wk && (!d->idk || !aligned16(d->idk))) return CREAM_ERR_BAD_ARG;
    if (bwd) {
        if (!d->dout || !d->dq || !d->dk || !d->dv || !d->delta || !d->dwl_part || !d->dww_part) return CREAM_ERR_BAD_ARG;
        if (d->dsn % 4 || d->dsh % 4 || d->dsb % 4 || !aligned16(d->dout)) return CREAM_ERR_BAD_ARG;
        if (!aligned8(d->dq) || !aligned8(d->dk) || !aligned8(d->dv)) return CREAM_ERR_BAD_ARG;       // rows go out as 8-byte vectors
        if (!aligned4(d->delta) || !aligned4(d->dwl_part) || !aligned4(d->dww_part)) return CREAM_ERR_BAD_ARG;
        if (d->wk && (!d->idk_t || !aligned16(d->idk_t) || !d->lkg || !d->dlk || !aligned16(d->lkg) || !aligned16(d->dlk)))
            return CREAM_ERR_BAD_ARG;
    }
    return CREAM_OK;
}

Args to_args(const cream_mini_attn_desc* d) {
    Args a{};
    a.q = (const short*)d->q; a.k = (const short*)d->k; a.v = (const short*)d->v;
    a.sb = d->sb; a.sn = d->sn; a.sh = d->sh;
    a.out = (short*)d->out; a.lse = d->lse;
    a.wk = d->wk; a.wk_hs = d->wk_hs; a.idk = d->idk; a.idk_t = d->idk_t;
    a.wl = d->wl; a.ww = d->ww;
    a.B = d->B; a.H = d->H; a.L = d->L; a.NP = d->NP; a.nb = d->nb; a.scale = d->scale;
    a.dout = (const short*)d->dout;
    a.dq = (short*)d->dq; a.dk = (short*)d->dk; a.dv = (short*)d->dv;
    a.dsb = d->dsb; a.dsn = d->dsn; a.dsh = d->dsh;
    a.delta = d->delta; a.lkg = (short*)d->lkg; a.dlk = (short*)d->dlk;
    a.dwl_part = d->dwl_part; a.dww_part = d->dww_part;
    return a;
}

}  // namespace

extern "C" {

int cream_mini_attn_fwd(const cream_mini_attn_desc* d, void* stream)
{
    const int rc = check(d, false);
    if (rc) return rc;
    return dispatch<false>(to_args(d), (hipStream_t)stream);
}

int cream_mini_attn_bwd(const cream_mini_attn_desc* d, void* stream)
{
    const int rc = check(d, true);
    if (rc) return rc;
    return dispatch<true>(to_args(d), (hipStream_t)stream);
}

}  // extern "C"

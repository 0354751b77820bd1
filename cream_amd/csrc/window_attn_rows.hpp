// window_attn_rows.hpp — what the two per-head window attention families share (window_attn_large.hip, 9x9 .. 14x14, the
// head's K and V resident in LDS; window_attn_xl.hip, 15x15 .. 32x32, K and V streamed through LDS in chunks): the staged-row
// tile format, [rows][KP = 40] bf16 with one token per row, the arithmetic of one 32 x 32 tile on it, and the host half of
// the descriptor they have in common.  A lane owns ONE token (query or key) and holds its 16 partners acc_row(r, g) of the
// tile, as in attn_lane.hpp.
//
// What belongs here: what one lane does with ONE tile, given pointers and ints (never a family's argument struct): the two
// products, the logit, the tile maximum, the merge of a query's two lanes into the log-sum-exp, and P.  What does not: the
// argument structs (their layout is part of the code objects), the LDS carve-ups, how rows get into LDS (stage_rows in one
// family; fetch, put and stream in the other) and the kernels' loops; those stay with their kernels.
// Everything on the device side is __forceinline__, and tools/device_code_diff.py is the test of what may live here: a kernel's
// code must be what it was with a private copy.  The exp-sum of pass 1, the delta step, the dS tile, launch K's tile and the
// pair walk of dT failed that test (behind a function the compiler orders the operands of their additions, or numbers the
// registers, differently in at least one of the six kernels), so both files still write them out; a change to one of them has
// to be made in both.
#pragma once
#include <math.h>
#include <stdint.h>

#include "attn_lane.hpp"
#include "cream_amd.h"
#include "cu_budget.hpp"

namespace cream {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int KP = 40;                 // pitch (bf16) of the staged rows (16-byte aligned rows, 8-byte aligned for the transposing read)
constexpr int MAXH = 32;

// ---- products on one staged tile (tile_rows = the first of its 32 rows) ----------------------------------------------------------
// tile^T (rows = the 32 staged tokens of the tile, column = own token) = staged rows . own^T.  The resident family passes
// the operand's first row and row0 = 32 t (one row index times the pitch: its address arithmetic), the streaming family
// the tile's first row
__device__ __forceinline__ f32x16 lds_tile(const short* tile_rows, const F (&own)[2], int lane, int row0 = 0) {
    const short* rp = tile_rows + (row0 + (lane & 31)) * KP + (lane >> 5) * 8;
    f32x16 s = {};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) s = TT::mma(TT::load(rp + ks * 16), own[ks], s);
    return s;
}
// acc^T (32 x own tokens) += tile^T (32 x 32 staged tokens) . p (32 staged x own), p in accumulator layout
__device__ __forceinline__ void rows_product(f32x16& acc, const short* tile_rows, const f32x16& p, int lane) {
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) acc = TT::mma(load_perm_tr<KP>(tile_rows, 0, s2, lane), TT::from_acc(p, s2), acc);
}
// this lane's two fragments of its own 32-wide row: load_frags<2> of attn_lane.hpp, then (optionally) scaled()
__device__ __forceinline__ void load_own(F (&f)[2], const short* row, int g, float s, bool scale_it) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        f[ks] = TT::load(row + ks * 16 + g * 8);
        if (scale_it) f[ks] = scaled(f[ks], s);
    }
}
// logits of (own query, keys acc_row(r, g) of tile t): the product + table (+ the -100 of the shift mask where the regions of
// the two tokens differ, MASK); keys past N: -inf.  tl: the head's table column, kc / reg: table coordinate and region per token
template <bool MASK>
__device__ __forceinline__ void add_bias(f32x16& S, const float* tl, const int* kc, const int* reg, int t, int qkc, int qreg, int N, int g) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int j = t * 32 + acc_row(r, g);
        float s = S[r] + tl[qkc - kc[j]];
        if constexpr (MASK) s += reg[j] != qreg ? -100.f : 0.f;
        S[r] = j < N ? s : -INFINITY;
    }
}

// ---- softmax, two passes ---------------------------------------------------------------------------------------------------------
// pass 1: the largest logit of a tile; the caller folds it into its running (max, sum)
__device__ __forceinline__ float tile_max(const f32x16& S) {
    float mt = S[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mt = fmaxf(mt, S[r]);
    return mt;
}
// the two lanes of a query merge their pairs, (m0, l0) of lane group 0 first in both, so that both hold the same bits.
// (mx, lx) = __shfl_xor(m, 32), __shfl_xor(l, 32): the caller shuffles its own variables (the compiler treats a shuffled
// function parameter differently from a shuffled local, and the kernels' code would change)
__device__ __forceinline__ float pair_lse(float m, float l, float mx, float lx, int g) {
    const float m0 = g == 0 ? m : mx, l0 = g == 0 ? l : lx, m1 = g == 0 ? mx : m, l1 = g == 0 ? lx : l;
    const float mm = fmaxf(m0, m1);
    const float ll = l0 * __builtin_amdgcn_exp2f((m0 - mm) * LOG2E) + l1 * __builtin_amdgcn_exp2f((m1 - mm) * LOG2E);
    return mm + __logf(ll);
}
// pass 2 (and the backward): P = exp(S - lse) in place; -inf -> 0
__device__ __forceinline__ void p_tile(f32x16& S, float lse) {
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = __builtin_amdgcn_exp2f((S[r] - lse) * LOG2E);
}

// ---- host: the descriptor both families take (cream_window_attn_large_desc; _xl_desc is the same type) --------------------------
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// the shape alone (what sizes the grid and the partials); without `shifts`, shift and mask_shift must be 0
inline int check_shape(const cream_window_attn_large_desc* d, int wmin, int wmax, bool shifts) {
    if (!d) return CREAM_ERR_BAD_ARG;
    if (d->head_dim != 32 || d->B < 0 || d->H < 1 || d->H > MAXH) return CREAM_ERR_BAD_ARG;
    if (d->w < wmin || d->w > wmax || d->Hs < d->w || d->Ws < d->w || d->Hs % d->w || d->Ws % d->w) return CREAM_ERR_BAD_ARG;
    if (shifts ? (d->shift < 0 || d->shift >= d->w || d->mask_shift < 0 || d->mask_shift >= d->w) : (d->shift != 0 || d->mask_shift != 0))
        return CREAM_ERR_BAD_ARG;
    if ((int64_t)d->B * d->Hs * d->Ws > (int64_t)1 << 30) return CREAM_ERR_TOO_LARGE;
    return CREAM_OK;
}
inline int check(const cream_window_attn_large_desc* d, bool bwd, int wmin, int wmax, bool shifts) {
    if (!d || !d->q || !d->k || !d->v || !d->lse || !d->table || (!bwd && !d->out)) return CREAM_ERR_BAD_ARG;
    if (const int rc = check_shape(d, wmin, wmax, shifts)) return rc;
    if (d->sn % 8 || d->sh % 8 || d->sb % 8 || !aligned16(d->q) || !aligned16(d->k) || !aligned16(d->v) || (!bwd && !aligned8(d->out)))
        return CREAM_ERR_BAD_ARG;
    if (!aligned4(d->lse) || !aligned4(d->table)) return CREAM_ERR_BAD_ARG;
    if (bwd) {
        if (!d->dout || !d->dq || !d->dk || !d->dv || !d->delta || !d->part || d->part_blocks < 1) return CREAM_ERR_BAD_ARG;
        if (d->dsn % 4 || d->dsh % 4 || d->dsb % 4 || !aligned16(d->dout)) return CREAM_ERR_BAD_ARG;
        if (!aligned8(d->dq) || !aligned8(d->dk) || !aligned8(d->dv) || !aligned4(d->delta) || !aligned4(d->part)) return CREAM_ERR_BAD_ARG;
    }
    return CREAM_OK;
}
// floats per partial of d table
inline int part_size(int H, int w, int wmin, int wmax) {
    if (H < 1 || H > MAXH || w < wmin || w > wmax) return CREAM_ERR_BAD_ARG;
    return (2 * w - 1) * (2 * w - 1) * H;
}
// work-item lanes per head of the persistent grids: launch Q's carve-up of `lds` bytes (the largest) sizes all three launches,
// so that one partial count describes the descriptor
inline int lanes_for(int lds, int items, int H) {
    const int per_cu = 160 * 1024 / lds < 4 ? 160 * 1024 / lds : 4;
    const int cap = cu_count() * per_cu / H;
    const int lanes = cap < 1 ? 1 : cap;
    return items < lanes ? items : lanes;
}
template <typename K, typename A> int launch(K kern, const A& a, int blocks, int lds, hipStream_t st) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
        return CREAM_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), (size_t)lds, st, a);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

}  // namespace cream

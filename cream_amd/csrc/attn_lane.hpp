// attn_lane.hpp — the lane-level helpers shared by the bf16 attention kernels that use the swapped product of
// attn_common.hpp, where a lane owns ONE token and holds 16 partners of it per 32 x 32 tile (irpe_attn.hip, irpe_attn_x.hip,
// mini_attn.hip, window_attn.hip, distill_loss.hip, and window_attn_large.hip and window_attn_xl.hip through
// window_attn_rows.hpp, which adds what those two share beyond this file: a pitch and the arithmetic of a tile at that pitch).
//
// What belongs here: what one lane (or one wave, for the head exchange) does with registers and pointers it is handed —
// operand fragments, byte bucket ids, the ordered scatter-add, output rows, the X[h][r4][lane] exchange.  What does not:
// anything that owns an LDS carve-up, a pitch constant, an argument struct or a loop over tiles; those stay with their kernels.
// Everything is __forceinline__, so a kernel's code is what it was with a private copy.
#pragma once
#include "attn_common.hpp"
#include "lane_ops.hpp"

namespace cream {

using TT = Tr<hip_bfloat16>;
using F = TT::frag;

// consecutive logical workgroups (the blocks of one (b,h), which share the streamed side) on one XCD
__device__ __forceinline__ int xcd_order(int bid, int n) {
    if (n & 7) return bid;
    return (bid & 7) * (n >> 3) + (bid >> 3);
}

// ---- operand fragments --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ F scaled(const F x, float s) {
    f32x8v y;
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = bf2f(x[e]) * s;
    return __builtin_bit_cast(F, __builtin_convertvector(y, hwbf16x8));
}
__device__ __forceinline__ u32x4v scaled_raw(const u32x4v x, float s) {
    return __builtin_bit_cast(u32x4v, scaled(__builtin_bit_cast(F, x), s));
}
// this lane's KS operand fragments of its own row (16 KS wide): elements ks*16 + g*8 .. +7
template <int KS> __device__ __forceinline__ void load_frags(F (&f)[KS], const short* row, int g) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) f[ks] = TT::load(row + ks * 16 + g * 8);
}

// A operand of a product that contracts over the 32 streamed tokens of a ROW-major [32][KP] tile (rows = tokens):
// MFMA row = column dt*32 + (lane & 31) of the tile, contraction indices in the permuted order of from_acc
// (acc_row(s2*8 + e, g)): two ds_read_b64_tr_b16 — the transpose happens on the way to the matrix cores, so no
// transposed copy of the tile is staged (8 conflicting 2-byte LDS stores per thread and tile, and 9 KB per buffer).
// The pitch is a compile-time constant here (it folds into the instruction offsets); attn_common.hpp has the run-time form.
template <int KP> __device__ __forceinline__ F load_perm_tr(const short* rows, int dt, int s2, int lane) {
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    const int gi = lane & 15, q = lane >> 4;
    const short* p0 = rows + (16 * s2 + 4 * (q >> 1) + (gi >> 2)) * KP + dt * 32 + 16 * (q & 1) + (gi & 3) * 4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        reinterpret_cast<__attribute__((address_space(3))) s16x4*>(reinterpret_cast<uintptr_t>(p0)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        reinterpret_cast<__attribute__((address_space(3))) s16x4*>(reinterpret_cast<uintptr_t>(p0 + 8 * KP)));
    return F{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// ---- bucket ids ---------------------------------------------------------------------------------------------------------------
// The 16 bucket ids of this lane's (own row, partners acc_row(r, g), r = 0..15) of streamed tile t: ONE 16-byte load from the
// byte matrix straight into registers.  bucket_bytes_kernel stores every 32-byte group of a row in that order (lane group g = 0
// first), so the two lanes of an own row read the two halves of one 32-byte piece and a wave reads 32 such pieces — the access
// pattern the staged id tiles had (round 2-5: a (128 x 32)-byte tile per table, double-buffered in LDS, 27 KB with rpe on q, k
// and v), without the LDS tile, its store and its four reads per lane.
__device__ __forceinline__ u32x4v ids_load(const uint8_t* tab, int NP, int row, int t, int g) {
    return *reinterpret_cast<const u32x4v*>(tab + (int64_t)min(row, NP - 1) * NP + t * 32 + g * 16);
}
// the bytes hold 2 * bucket id (<= 254): the byte offset of the bucket in a bf16 lookup row
__device__ __forceinline__ int off2_of(const u32x4v& w, int r) { return (w[r >> 2] >> (8 * (r & 3))) & 0xffu; }
// acc += (bf16 at byte offset off2 of row): one v_dot2c_f32_bf16 with (x, 0) . (1, 1) instead of shift + add
__device__ __forceinline__ float add_bf16_at(float acc, const short* row, int off2) {
    const uint32_t x = *reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(row) + off2);
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(hwbf16x2, x), __builtin_bit_cast(hwbf16x2, 0x3F803F80u), acc, false);   // (1, 1): a literal — the inline constant 1.0 is not (1, 0) for packed bf16
}

// row[id_r] += val_r for the 16 (bucket id, value) pairs of this lane — without LDS float atomics
// (ds_add_f32 retires a few lanes per clock: the kernels were 6x slower with it, profiles/r02_irpe_attention.md).
// The two lanes that share a row (g = 0 / 1) take turns — the LDS operations of a wave execute in order, so
// the second half adds onto the first half's sums — and each half goes G pairs at a time: G reads,
// duplicates inside the group resolved in registers (the latest earlier match carries the running sum,
// and the last write to an address is the complete one), G writes.
// G = pairs per read-modify-write group.  Same-call A/B at config 4 of the iRPE zoo (tools/probe_irpe_variants.sh, two
// workgroups per CU): 16 / 8 / 4 / 2 -> forward v 413 / 313 / 274 / 274 us, backward k 1,042 / 930 / 870 / 870: with a second
// wave on the SIMD the extra LDS round trips are hidden and the compare / select pairs (G (G - 1) / 2 per group) are not.
template <int G = 4> __device__ __forceinline__ void scatter_add16(float* row, const u32x4v& w, const f32x16& val, int g) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (g == half) {
#pragma unroll
            for (int grp = 0; grp < 16 / G; ++grp) {
                int id[G];
                float sum[G];
#pragma unroll
                for (int v = 0; v < G; ++v) {
                    id[v] = off2_of(w, grp * G + v);
                    sum[v] = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(row) + 2 * id[v]);
                }
#pragma unroll
                for (int v = 0; v < G; ++v) {
                    float base = sum[v];
#pragma unroll
                    for (int u = 0; u < v; ++u) base = (id[u] == id[v]) ? sum[u] : base;
                    sum[v] = base + val[grp * G + v];
                }
#pragma unroll
                for (int v = 0; v < G; ++v) *reinterpret_cast<float*>(reinterpret_cast<char*>(row) + 2 * id[v]) = sum[v];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    }
}

// ---- rows in and out ----------------------------------------------------------------------------------------------------------
// this lane's half of a bf16 lookup row (buckets ks*16 + g*8 .. +7, ks = 0..KS-1) -> global row of 16 KS
template <int KS> __device__ __forceinline__ void lrow_to_global(short* dst, const short* row, int g) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(row + ks * 16 + g * 8);
        *reinterpret_cast<u32x4v*>(dst + ks * 16 + g * 8) = u32x4v{s[0], s[1], s[2], s[3]};
    }
}
// fragment of 8 consecutive values (buckets ks*16 + g*8 ..) of an fp32 scatter-add row of pitch LKP, times mul; columns past a
// pitch below 64 do not exist and read as 0
template <int LKP> __device__ __forceinline__ F srow_frag(const float* row, int ks, int g, float mul) {
    f32x8v x;
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (LKP >= 64 || ks * 16 + g * 8 + e < LKP) ? row[ks * 16 + g * 8 + e] * mul : 0.f;
    return __builtin_bit_cast(F, __builtin_convertvector(x, hwbf16x8));
}
// this lane's share of its own token's output row (o in accumulator layout: columns acc_row(r, g) of each 32-wide tile), times
// mul, as bf16: 32 DT columns from DT accumulator tiles, or 32 from one
template <int DT> __device__ __forceinline__ void store_row(short* op, const f32x16 (&o)[DT], int g, float mul) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int d = dt * 32 + 8 * r4 + 4 * g;
            *reinterpret_cast<u32x2v*>(op + d) = u32x2v{f2bf_pair(o[dt][4 * r4] * mul, o[dt][4 * r4 + 1] * mul),
                                                        f2bf_pair(o[dt][4 * r4 + 2] * mul, o[dt][4 * r4 + 3] * mul)};
        }
}
__device__ __forceinline__ void store_row(short* op, const f32x16& o, int g, float mul) {
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4)
        *reinterpret_cast<u32x2v*>(op + 8 * r4 + 4 * g) =
            u32x2v{f2bf_pair(o[4 * r4] * mul, o[4 * r4 + 1] * mul), f2bf_pair(o[4 * r4 + 2] * mul, o[4 * r4 + 3] * mul)};
}

// ---- the head exchange: X[x][r4][lane] (16 bytes each) holds the tile of head hb + x in the accumulator layout ------------------
// (one fp32 LDS buffer, 4 KB per head: the accumulator layout itself, 16-byte accesses, no bank conflicts).  Wave w puts the
// tiles of its head slots x = w, w + 4, ...; the barriers on both sides make the buffer reusable from call to call.
template <int HPW>
__device__ __forceinline__ void xchg_put(float* X, const f32x16 (&in)[HPW], int hb, int H, int wave, int lane) {
    __syncthreads();                                   // every wave has read the previous contents
#pragma unroll
    for (int s = 0; s < HPW; ++s) {
        const int x = wave + 4 * s;
        if (hb + x < H) {
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4)
                *reinterpret_cast<f32x4v*>(X + ((x * 4 + r4) * 64 + lane) * 4) =
                    f32x4v{in[s][4 * r4], in[s][4 * r4 + 1], in[s][4 * r4 + 2], in[s][4 * r4 + 3]};
        }
    }
    __syncthreads();
}
// out[s] = sum_h W[o_s][h] X[h]  (TRANS: sum_h W[h][o_s] X[h]);  CROSS: cross[h][s] += sum over this lane's 16 elements of
// own[s] * X[h]  (the lane's share of a weight gradient: row h = the exchanged head, column = the own head of slot s)
template <int HPW, bool TRANS, bool CROSS>
__device__ __forceinline__ void xchg_mix(const float* X, f32x16 (&out)[HPW], const float* __restrict__ W, int H, int wave, int lane,
                                         const f32x16 (&own)[HPW], float (&cross)[4 * HPW][HPW]) {
#pragma unroll
    for (int s = 0; s < HPW; ++s) out[s] = f32x16{};
#pragma unroll
    for (int h = 0; h < 4 * HPW; ++h) {
        if (h < H) {
            f32x16 x;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const f32x4v v = *reinterpret_cast<const f32x4v*>(X + ((h * 4 + r4) * 64 + lane) * 4);
                x[4 * r4] = v[0]; x[4 * r4 + 1] = v[1]; x[4 * r4 + 2] = v[2]; x[4 * r4 + 3] = v[3];
            }
#pragma unroll
            for (int s = 0; s < HPW; ++s) {
                const int o = wave + 4 * s;
                if (o < H) {
                    const float w = TRANS ? W[h * H + o] : W[o * H + h];
#pragma unroll
                    for (int r = 0; r < 16; ++r) out[s][r] = __builtin_fmaf(w, x[r], out[s][r]);
                    if constexpr (CROSS) {
                        float c0 = 0.f, c1 = 0.f;
#pragma unroll
                        for (int r = 0; r < 16; r += 2) {
                            c0 = __builtin_fmaf(own[s][r], x[r], c0);
                            c1 = __builtin_fmaf(own[s][r + 1], x[r + 1], c1);
                        }
                        cross[h][s] += c0 + c1;
                    }
                }
            }
        }
    }
}
template <int HPW, bool TRANS>
__device__ __forceinline__ void xchg_mix(const float* X, f32x16 (&out)[HPW], const float* __restrict__ W, int H, int wave, int lane) {
    float dummy[4 * HPW][HPW];
    xchg_mix<HPW, TRANS, false>(X, out, W, H, wave, lane, out, dummy);
}

}  // namespace cream

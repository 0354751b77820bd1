// attn_rpe2d_whole14.hpp — what the three whole-matrix kernels of the AutoFormer geometry (N = 197, 14 x 14 grid,
// max_relative_position 14, bf16) share: attn_rpe2d_fwd2.hpp, attn_rpe2d_bwd1.hpp, attn_rpe2d_bwd2.hpp.  They keep an
// item's matrices WHOLE in LDS ([224][64] bf16 each, XOR-swizzled, fetched by DMA) and read the bucket tables from bf16
// operand images in global memory.  Here: the LDS offsets, the table images, swizzled / transposing LDS reads, the DMA
// helpers, and the bf16 slot <-> bucket shifts and staged row store.
#pragma once
#include "attn_rpe2d_tile.hpp"

namespace {
namespace whole14 {

constexpr int NT = 7, N14 = 197, NP14 = 224, THREADS = 448;
constexpr int MAT_B = NP14 * 128;                    // one [224][64] bf16 matrix
constexpr int OFF_K = 0, OFF_V = MAT_B, OFF_Q = 2 * MAT_B, OFF_D = 3 * MAT_B;
constexpr int OFF_OH = 4 * MAT_B, OH_B = NP14 * 64;
constexpr int OFF_X = OFF_OH + OH_B;
constexpr int SLOT_B = 4608, XT_B = 2048;            // slot = P tile | dS tile | pad  (scratch rows: 72 bf16 = 144 B)
constexpr int OFF_SINK = OFF_X + NT * SLOT_B;        // 1 KB landing zone of the L2 prefetch (never read)
constexpr int LDS_B = OFF_SINK + 1024;
constexpr int SCRP = 72;                             // shift scratch pitch (bf16 elements)
static_assert(LDS_B <= 160 * 1024, "LDS budget");
static_assert(32 * SCRP * 2 <= SLOT_B, "shift scratch fits the wave's exchange slot");

// image layout (bf16 elements): key rows [64 u'][64 d] | key^T [64 d][64 u'] | value rows | value^T,
// u' = bucket of the vertical table (0..31) or 32 + bucket of the horizontal table; rows >= nb are zero
constexpr int IMG_KR = 0, IMG_KT = 4096, IMG_VR = 8192, IMG_VT = 12288, IMG_ELEMS = 16384;

__global__ __launch_bounds__(256) void table_images_kernel(short* img, const float* tkv, const float* tkh, const float* tvv,
                                                           const float* tvh, int ldt, int nb) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * 4096; i += gridDim.x * blockDim.x) {
        const int pair = i >> 12, e = i & 4095, u2 = e >> 6, d = e & 63, u = u2 & 31;
        const float* t = pair == 0 ? (u2 < 32 ? tkv : tkh) : (u2 < 32 ? tvv : tvh);
        const short x = u < nb ? f2bf(t[(int64_t)u * ldt + d]) : (short)0;
        img[pair * 8192 + u2 * 64 + d] = x;                  // rows
        img[pair * 8192 + 4096 + d * 64 + u2] = x;           // transposed
    }
}

__device__ __forceinline__ int swz128(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }

typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ s16x4 lds_tr16(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        reinterpret_cast<__attribute__((address_space(3))) s16x4*>(reinterpret_cast<uintptr_t>(p)));
}
__device__ __forceinline__ bf16x8 tr_pair(const unsigned char* p0, const unsigned char* p1) {
    const s16x4 lo = lds_tr16(p0), hi = lds_tr16(p1);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ bf16x8 lds_b128(const unsigned char* p) {
    union { u32x4v v; bf16x8 f; } u;
    u.v = *reinterpret_cast<const u32x4v*>(p);
    return u.f;
}
__device__ __forceinline__ bf16x8 mk8(const short (&x)[8]) { return bf16x8{x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]}; }
__device__ __forceinline__ f32x16 mma16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

// per-lane LDS offsets (bytes) that do not depend on the tile: computed once per kernel
struct LaneOffs {
    int row[4];        // A / B operand rows of a [32][64] tile: lane = row c32, k-step ks -> 16 bytes
    int ohrow[2];      // the same for a [32][32] one-hot tile
    int tr[2][2];      // ds_read_b64_tr_b16 of a [32][64] tile: [dt][h] (+ 2048 per k-step of 16 tokens)
    int ohtr[2];       // the same for a [32][32] one-hot tile     (+ 1024 per k-step)
    int xr[2];         // the same for an exchange tile            (+ 1024 per k-step)
    int xw[2][2];      // exchange tile write: [st][h], 8 bytes
};
__device__ __forceinline__ LaneOffs lane_offs(int lane) {
    LaneOffs o;
    const int c32 = lane & 31, g = lane >> 5, gi = lane & 15, q4 = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) o.row[ks] = c32 * 128 + (((2 * ks + g) ^ swz128(c32)) << 4);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) o.ohrow[ks] = c32 * 64 + (((2 * ks + g) ^ ((c32 >> 2) & 3)) << 4);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int rh = 4 * g + (gi >> 2) + 8 * h;                  // token row inside a 16-token k-step
        const int inner = 8 * (gi & 1), c0 = 2 * (q4 & 1) + ((gi & 3) >> 1);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) o.tr[dt][h] = rh * 128 + (((4 * dt + c0) ^ swz128(rh)) << 4) + inner;
        o.ohtr[h] = rh * 64 + ((c0 ^ ((rh >> 2) & 3)) << 4) + inner;
        o.xr[h] = rh * 64 + (((4 * (q4 & 1) + (gi & 3)) ^ ((rh >> 1) & 7)) << 3);
#pragma unroll
        for (int st = 0; st < 2; ++st) o.xw[st][h] = c32 * 64 + (((4 * st + 2 * h + g) ^ ((c32 >> 1) & 7)) << 3);
    }
    return o;
}

// workgroup barrier for LDS traffic only: ds operations are retired (lgkmcnt), global loads and the prefetch DMA stay in
// flight across it (__syncthreads() would also drain vmcnt)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// one 1 KB global -> LDS DMA read (16 bytes per lane, LDS destination = wave-uniform `lds_dst` + 16 lane) as INLINE ASM:
// hipcc orders every later ds_read behind a builtin LDS-DMA with s_waitcnt vmcnt(0) (it is a pending LDS write), which
// would drain the prefetch at every step; an asm statement is outside its bookkeeping (cdna_hip_programming.md 5.7).
// Nothing ever reads the destination, so no wait belongs to it; M0 is restored.
__device__ __forceinline__ void prefetch_dma(const short* src, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_dst));
}

// ---- the item's matrices travel global -> LDS by DMA (no register staging) --------------------------------------------
// A register-staged prefetch of the next item does not survive here: with ~230 live registers the compiler waits for every
// prefetched vector at once and parks it in scratch (round-4 builds: the "prefetch" was a load, a wait, a scratch store and
// a scratch reload).  LDS-DMA needs no registers: one wave instruction moves 1 KB = 8 rows x 128 B into a lane-linear image;
// the chunk swizzle of the tile (chunk ^ swz128(row)) is applied to the SOURCE address, rows beyond N come from a zero line.
__device__ __attribute__((aligned(16))) const uint32_t g_zero_line[4] = {0u, 0u, 0u, 0u};
__device__ __forceinline__ void dma_1k(const short* src, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}
// rows [0, 224) of one matrix (row stride rs elements) into the LDS region at byte address lds_base: 28 pieces, 4 per wave
__device__ __forceinline__ void mat_dma(const short* src, int64_t rs, uint32_t lds_base, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int piece = wave + NT * i, row = piece * 8 + (lane >> 3), cc = lane & 7;
        const short* s = row < N14 ? src + (int64_t)row * rs + ((cc ^ swz128(row)) << 3) : reinterpret_cast<const short*>(g_zero_line);
        dma_1k(s, lds_base + piece * 1024);
    }
}
__device__ __forceinline__ void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// one-hot slot rows of the keys (geometry only): OH[j][c] = 1 iff key j sits in slot c
__device__ __forceinline__ void fill_onehot_swz(unsigned char* oh) {
    const RelGeom G{N14, G14, G14, G14};
    for (int i = threadIdx.x; i < NP14 * 4; i += THREADS) {
        const int j = i >> 2, cc = i & 3;
        // keys >= N carry slot 15 (unused by the geometry): the query extension holds -2^15 there, so their
        // probabilities underflow to exactly 0 without a select per score (slot 15 of every gradient stays exactly 0)
        const uint32_t m = (key_mask(j, G) | (j >= N14 ? 1u << 15 : 0u)) >> (8 * cc);
        u32x4v w;
#pragma unroll
        for (int p = 0; p < 4; ++p) w[p] = ((m >> (2 * p)) & 1u) * 0x3F80u + ((m >> (2 * p + 1)) & 1u) * 0x3F800000u;
        *reinterpret_cast<u32x4v*>(oh + j * 64 + ((cc ^ ((j >> 2) & 3)) << 4)) = w;
    }
}

// ---- slot <-> bucket shifts through the wave's bf16 scratch ([32 queries][SCRP]) ---------------------------------
// lookups^T (buckets x queries) of the vertical / horizontal table against this lane's row fragments xb, then the
// window shift of attn_common.hpp (ext_window14) -> slot extension fragments xe[2] (B operand, lane = query).
// `rows` = bf16 image [64 u'][64 d] in global memory.  Rounding the lookups to bf16 before the shift gives the same
// bits as rounding the shifted values (the shift is a permutation); the class-token value is summed in fp32 first.
// one lookup set -> scratch -> window shift (attn_common.hpp: ext_window14).  slot15 = raw bf16 placed in the unused slot 15
// (0, or -2^15 for the key-side extension: padding-key mask)
__device__ __forceinline__ void ext_from_lookups14(bf16x8 (&xe)[2], const f32x16& av, const f32x16& ah, unsigned char* scr, int lane,
                                                   bool tile0, int qr, int qc, short slot15) {
    const int c32 = lane & 31, g = lane >> 5;
    unsigned char* row = scr + c32 * (SCRP * 2);
    // buckets acc_row(4i + e, g) = 8i + 4g + e: four consecutive bf16 per store
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<u32x2v*>(row + (8 * i + 4 * g) * 2) =
            u32x2v{f2bf_pair(av[4 * i], av[4 * i + 1]), f2bf_pair(av[4 * i + 2], av[4 * i + 3])};
        *reinterpret_cast<u32x2v*>(row + (32 + 8 * i + 4 * g) * 2) =
            u32x2v{f2bf_pair(ah[4 * i], ah[4 * i + 1]), f2bf_pair(ah[4 * i + 2], ah[4 * i + 3])};
    }
    if (g == 0) *reinterpret_cast<float*>(row + 128) = av[0] + ah[0];          // bucket 0 of both tables (fp32)
    wave_lds_fence();
    const short cls = f2bf(*reinterpret_cast<const float*>(row + 128));
    if (tile0) {                                                               // class-token query (attn_common.hpp: ext_fix_query0)
        if (c32 == 0 && g == 0) {
            short* r = reinterpret_cast<short*>(row);
#pragma unroll
            for (int u = 0; u < 16; ++u) { r[15 + u] = cls; r[32 + 15 + u] = 0; }
        }
        wave_lds_fence();
    }
    const short* r = reinterpret_cast<const short*>(row);
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
        const short* p = r + (kh == 0 ? 15 - qr : 32 + 15 - qc) + 8 * g;
        short x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = p[e];
        x[6] = g ? (kh == 0 ? cls : (short)0) : x[6];
        x[7] = g ? (kh == 0 ? slot15 : (short)0) : x[7];
        xe[kh] = mk8(x);
    }
    wave_lds_fence();
}

// slot extensions of q (key tables) and of dO (value tables): lookups^T (buckets x queries) of the vertical / horizontal
// table against this lane's row fragments, then the window shifts through the wave's scratch.  `img` = the bf16 images
// in global memory; all 16 row fragments are requested before the first MFMA.  Rounding the lookups to bf16 before the
// shift gives the same bits as rounding the shifted values (the shift is a permutation); the class-token value is
// summed in fp32 first.
struct TabFrags { bf16x8 tk[2][4], tv[2][4]; };       // row fragments of the key / value table images (vertical, horizontal)
__device__ __forceinline__ void load_tab_frags(TabFrags& f, const short* img, int lane) {
    const int c32 = lane & 31, g = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f.tk[t][ks] = *reinterpret_cast<const bf16x8*>(img + IMG_KR + (32 * t + c32) * 64 + ks * 16 + g * 8);
            f.tv[t][ks] = *reinterpret_cast<const bf16x8*>(img + IMG_VR + (32 * t + c32) * 64 + ks * 16 + g * 8);
        }
}
__device__ __forceinline__ void lookups_ext14_pair(bf16x8 (&qe)[2], bf16x8 (&de)[2], const bf16x8 (&qb)[4], const bf16x8 (&dob)[4],
                                                   const TabFrags& tf, unsigned char* scr, int lane, bool tile0, int qr, int qc) {
    const bf16x8 (&tk)[2][4] = tf.tk;
    const bf16x8 (&tv)[2][4] = tf.tv;
    f32x16 kv = {}, kh = {}, vv = {}, vh = {};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        kv = mma16(tk[0][ks], qb[ks], kv);
        kh = mma16(tk[1][ks], qb[ks], kh);
        vv = mma16(tv[0][ks], dob[ks], vv);
        vh = mma16(tv[1][ks], dob[ks], vh);
    }
    ext_from_lookups14(qe, kv, kh, scr, lane, tile0, qr, qc, (short)0xC700);
    ext_from_lookups14(de, vv, vh, scr, lane, tile0, qr, qc, (short)0);
}

// adjoint: slot tile (accumulator: this lane holds slots acc_row(r, g) of its query) -> the 32 bucket values of table g
// (0 vertical / 1 horizontal) of this lane's query as four bf16 operand fragments bk[ks] = buckets 8 ks .. 8 ks + 7
// (attn_common.hpp: slots_to_buckets14; the class-token query's sum is taken in fp32 from the registers)
__device__ __forceinline__ void slots_to_buckets14_bf16(bf16x8 (&bk)[4], unsigned char* scr, const f32x16& x, int lane,
                                                        bool tile0, int qr, int qc) {
    const int c32 = lane & 31, g = lane >> 5;
    unsigned char* rowb = scr + c32 * (SCRP * 2);
    short* row = reinterpret_cast<short*>(rowb);
    {
        // zero pads: lane group 0 writes [0,14) and [28,42), lane group 1 [56,70) and (again) [28,42)
        uint32_t* z = reinterpret_cast<uint32_t*>(rowb + (g ? 112 : 0));
        uint32_t* z2 = reinterpret_cast<uint32_t*>(rowb + 56);
#pragma unroll
        for (int i = 0; i < 7; ++i) { z[i] = 0u; z2[i] = 0u; }
    }
    wave_lds_fence();
    {
        // vertical half: slots c = c0 + 4g, c0 = (r & 3) + 8 (r >> 2), r < 8  -> index 14 + c; slot 14 (c0 = 10, g = 1)
        // is the class-token key slot (index 70), slot 15 is exactly 0
#pragma unroll
        for (int rp = 0; rp < 4; ++rp) {
            const int r0 = 2 * rp, c0 = (r0 & 3) + 8 * (r0 >> 2);
            float lo = x[r0], hi = x[r0 + 1];
            if (c0 == 10) { lo = g ? 0.f : lo; hi = g ? 0.f : hi; }
            *reinterpret_cast<uint32_t*>(rowb + (14 + c0 + 4 * g) * 2) = f2bf_pair(lo, hi);
        }
        if (g) row[70] = f2bf(x[6]);
        // horizontal half: slots 16 + c', r >= 8 -> index 42 + c - 16 (slots 30, 31 are exactly 0 and land in the pad)
#pragma unroll
        for (int rp = 4; rp < 8; ++rp) {
            const int r0 = 2 * rp, c0 = (r0 & 3) + 8 * (r0 >> 2);      // 16,18,24,26
            *reinterpret_cast<uint32_t*>(rowb + (42 - 16 + c0 + 4 * g) * 2) = f2bf_pair(x[r0], x[r0 + 1]);
        }
    }
    wave_lds_fence();
    short b[32];
    {
        const short* p = row + (g ? 28 + qc : qr);
        b[0] = row[70];
#pragma unroll
        for (int u = 1; u < 30; ++u) b[u] = p[u - 1];
        b[30] = 0;
        b[31] = 0;
    }
    if (tile0) {                                    // class-token query: bucket 0 collects every key (row slots + cls slot)
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) sum += x[r];    // slots 0..15 of the vertical half (slot 15 is exactly 0)
        sum += __shfl_xor(sum, 32);
        const bool q0 = c32 == 0;
        const short s16 = f2bf(sum);
#pragma unroll
        for (int u = 0; u < 32; ++u) b[u] = q0 ? (u == 0 ? s16 : (short)0) : b[u];
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        bk[ks] = bf16x8{b[8 * ks], b[8 * ks + 1], b[8 * ks + 2], b[8 * ks + 3], b[8 * ks + 4], b[8 * ks + 5], b[8 * ks + 6], b[8 * ks + 7]};
    wave_lds_fence();                               // the slot is reused by the caller
}

// accumulator tile (lane = token row c32 of this wave's 32-token tile, 64 d-values) -> global rows, COALESCED: the tile goes
// through a wave-private 4 KB LDS stage ([32][128 B], chunks ^ swz128) and leaves as whole 128-byte rows (8 lanes x 16 B
// per row, 8 rows per wave instruction).  Storing straight from the accumulator layout (a lane owns a row, 32 rows at a
// 2.3 KB stride per instruction, 32 bytes each) made the write-back of dq / dk / dv the slowest phase of an item: vmcnt
// retires in order, so the first load consumer behind those stores waited ~20k cycles for them (ablation in
// tools/probes/attn_bwd1_probe: an item 81k -> 52k cycles without the stores).
// The two lane groups of a row hold alternating runs of 4 d-values; one v_permlane32_swap per dword pairs them up into
// 16-byte pieces (cdna_hip_programming.md T21).  `tile_row0` = first token of the tile; rows >= N14 are not written.
__device__ __forceinline__ void store_tile_staged(unsigned char* stage, short* gbase, int64_t rs, int tile_row0,
                                                  const f32x16 (&o)[2], int lane) {
    const int c32 = lane & 31, g = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int k = 0; k < 4; k += 2) {
            uint32_t ax = f2bf_pair(o[dt][4 * k], o[dt][4 * k + 1]), ay = f2bf_pair(o[dt][4 * k + 2], o[dt][4 * k + 3]);
            uint32_t bx = f2bf_pair(o[dt][4 * k + 4], o[dt][4 * k + 5]), by = f2bf_pair(o[dt][4 * k + 6], o[dt][4 * k + 7]);
            const auto rx = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
            const auto ry = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
            // lanes 0-31: [own run k | partner's run k] = d 8k .. 8k+7 (chunk 4 dt + k);  lanes 32-63: chunk 4 dt + k + 1
            *reinterpret_cast<u32x4v*>(stage + c32 * 128 + (((4 * dt + k + g) ^ swz128(c32)) << 4)) = u32x4v{rx[0], ry[0], rx[1], ry[1]};
        }
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = i * 8 + (lane >> 3), cc = lane & 7;
        const u32x4v v = *reinterpret_cast<const u32x4v*>(stage + row * 128 + ((cc ^ swz128(row)) << 4));
        if (tile_row0 + row < N14) *reinterpret_cast<u32x4v*>(gbase + (int64_t)row * rs + cc * 8) = v;
    }
    wave_lds_fence();                               // the stage may be rewritten by the caller
}

}  // namespace whole14
}  // namespace

// attn_rpe2d_tile.hpp — what the kernels of attn_rpe2d.hip share: the argument structs, the phase stamps of the probes,
// and the pieces of the tile-streamed kernels (attn_rpe2d_fwd.hpp, attn_rpe2d_fwd14.hpp, attn_rpe2d_bwd.hpp): bucket
// lookups and slot <-> bucket shifts on 32-query tiles, the streamed operand tiles, table staging, one-hot operands.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bfloat16.h>
#include <stdint.h>

#include "attn_common.hpp"

namespace {
using namespace cream;

constexpr float LOG2E = 1.4426950408889634f;

// Phase timestamps for tools/probes/attn_probe.hip (compiled out of the library).
#ifdef ATTN_PROFILE
__device__ long long* g_attn_prof = nullptr;
#define PROF_DECL long long prof_t[12]; int prof_n = 0;
#define PROF_MARK() do { prof_t[prof_n++] = (long long)__builtin_readcyclecounter(); } while (0)
#define PROF_FLUSH() do { if ((threadIdx.x & 63) == 0 && g_attn_prof) { \
        long long* d_ = g_attn_prof + ((long long)blockIdx.x * 8 + (threadIdx.x >> 6)) * 12; \
        for (int i_ = 0; i_ < 12; ++i_) d_[i_] = i_ < prof_n ? prof_t[i_] : 0; } } while (0)
#else
#define PROF_DECL
#define PROF_MARK() do {} while (0)
#define PROF_FLUSH() do {} while (0)
#endif
#ifdef ATTN_PROFILE_KVLOOP           // sub-phase stamps inside one iteration of the dK/dV tile loop
#define PROF_LOOP(t) do { if ((t) == 3) PROF_MARK(); } while (0)
#else
#define PROF_LOOP(t) do {} while (0)
#endif

struct FwdArgs {
    const void* q; const void* k; const void* v;    // element (b, n, h, :) at b*sb + n*sn + h*sh
    int64_t sb, sn, sh;
    void* out;                                       // (B, N, H, 64) contiguous
    float* lse;                                      // (B, H, N)   log-sum-exp of scaled logits
    void* sp;                                        // (B, H, 64, NP) bucket sums S'^T, dtype T
    const float *tkv, *tkh, *tvv, *tvh;              // (nb, 64) tables, row stride ldt
    int ldt, nb;
    int H, NP;
    RelGeom G;
    float scale;
    int nitems;                                      // B * H (forward: persistent workgroups walk them)
    const void* timg;                                // bf16 operand images of the four tables (cream_attn_rpe2d_table_images) or NULL
    // attention dropout (multihead_super.py:145), DROP instantiations of the tile-streamed kernels only (attn_common.hpp: drop_keep)
    uint32_t drop_thr = 0, drop_seed = 0;            // keep iff hash >= drop_thr; 0: no dropout
    float drop_scale = 1.f;                          // 1 / (1 - p)
};

struct BwdArgs {
    const void* q; const void* k; const void* v;
    int64_t sb, sn, sh;
    void* dq; void* dk; void* dv;                    // same indexing with (dsb, dsn, dsh)
    int64_t dsb, dsn, dsh;
    const void* dout; const void* out;               // (B, N, H, 64) contiguous
    const float* lse;                                // (B, H, N)
    const void* sp;                                  // (B, H, 64, NP) from forward
    void* dlt;                                       // (B, H, 64, NP)  dL'^T            (A -> B)
    void* qe; void* de;                              // (B, H, NP, 32)  slot extensions  (A -> B)
    float* delta;                                    // (B, H, NP)                       (A -> B)
    float* dtab;                                     // (B*H, 4, 32, 64) per-(b,h) table gradients
    const float *tkv, *tkh, *tvv, *tvh;
    int ldt, nb;
    int H, NP;
    RelGeom G;
    float scale;
    int nitems;                                      // B * H (dQ kernel: persistent workgroups walk them)
    int stagger;                                     // one-pass kernel: start offset between the 8 phase groups (x 64 cycles)
    const void* timg;                                // bf16 operand images of the four tables or NULL (then built into dlt)
    uint32_t drop_thr = 0, drop_seed = 0;            // as in FwdArgs: the two-launch backward regenerates the forward's mask
    float drop_scale = 1.f;
};

// ---- pieces shared by forward and backward ---------------------------------------------

template <typename T> __host__ __device__ constexpr int table_pitch() { return sizeof(typename Tr<T>::elem) == 2 ? 72 : 65; }
// bf16: the bucket tables are staged in LDS as operand rows; fp32 (parity mode) reads them from
// global memory (its LDS is full of fp32 tiles)
template <typename T> __host__ __device__ constexpr bool tables_in_lds() { return sizeof(typename Tr<T>::elem) == 2; }

// operand fragments of one row of a row-major (n, 64) matrix (lane = row, steps over d); the
// row pointer is always valid (callers clamp the row index), so the loads are unconditional
// and can be issued a tile ahead of their use
template <typename T>
__device__ __forceinline__ void load_row(typename Tr<T>::frag (&f)[64 / Tr<T>::KI],
                                         const typename Tr<T>::elem* rowp, int g) {
    using TT = Tr<T>;
#pragma unroll
    for (int ks = 0; ks < 64 / TT::KI; ++ks) f[ks] = TT::load(rowp + ks * TT::KI + g * TT::EPL);
}
template <typename T, int NF>
__device__ __forceinline__ void zero_frags(typename Tr<T>::frag (&f)[NF]) {
#pragma unroll
    for (int i = 0; i < NF; ++i) f[i] = Tr<T>::zero();
}

// lookups^T (32 buckets x 32 queries) = table(32 x 64) . X^T for the vertical and horizontal
// table, written to the wave's scratch as row[q][u] / row[q][32 + u].
//   tabR : LDS operand rows [64][tp] (rows 0..31 vertical, 32..63 horizontal)  — bf16 mode
//   tv/th: the fp32 tables in global memory                                    — fp32 mode
template <typename T>
__device__ __forceinline__ void table_lookups(float* scr, const typename Tr<T>::frag (&xb)[64 / Tr<T>::KI],
                                              const typename Tr<T>::elem* tabR, const float* tv, const float* th,
                                              int ldt, int nb, int lane) {
    using TT = Tr<T>;
    constexpr int tp = table_pitch<T>();
    const int u = lane & 31, g = lane >> 5;
    f32x16 av = {}, ah = {};
#pragma unroll
    for (int ks = 0; ks < 64 / TT::KI; ++ks) {
        const int k0 = ks * TT::KI + g * TT::EPL;
        if constexpr (tables_in_lds<T>()) {
            av = TT::mma(TT::load(tabR + u * tp + k0), xb[ks], av);
            ah = TT::mma(TT::load(tabR + (u + 32) * tp + k0), xb[ks], ah);
        } else {
            av = TT::mma(TT::load_f32(tv + (int64_t)u * ldt + k0, u < nb), xb[ks], av);
            ah = TT::mma(TT::load_f32(th + (int64_t)u * ldt + k0, u < nb), xb[ks], ah);
        }
    }
    float* row = scr + (lane & 31) * LP;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        row[acc_row(r, g)] = av[r];
        row[32 + acc_row(r, g)] = ah[r];
    }
}

// extension fragments x_i[slot] (B operand, 32 slots) from the wave's scratch
template <typename T>
__device__ __forceinline__ void build_ext(typename Tr<T>::frag (&xe)[32 / Tr<T>::KI], const float* scr,
                                          int lane, int qi, int qr, int qc, const RelGeom& G) {
    using TT = Tr<T>;
    const int g = lane >> 5;
    const float* row = scr + (lane & 31) * LP;
    const float cls = row[0] + row[32];
#pragma unroll
    for (int ks = 0; ks < 32 / TT::KI; ++ks) {
        if constexpr (TT::EPL == 1) {
            xe[ks] = ext_gather(row, cls, ks * 2 + g, qi, qr, qc, G);
        } else {
            f32x8v x;
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = ext_gather(row, cls, ks * 16 + g * 8 + e, qi, qr, qc, G);
            xe[ks] = __builtin_bit_cast(bf16x8, __builtin_convertvector(x, hwbf16x8));
        }
    }
}

// fast geometry (attn_common.hpp): window reads with immediate offsets; bf16 fragments only
__device__ __forceinline__ void build_ext14(bf16x8 (&xe)[2], float* scr, int lane, bool tile0, int qr, int qc) {
    const int g = lane >> 5;
    float* row = scr + (lane & 31) * LP;
    const float cls = row[0] + row[32];
    if (tile0) {
        ext_fix_query0(row, cls, lane);
        wave_lds_fence();
    }
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
        float x[8];
        ext_window14(x, row, cls, kh, g, qr, qc);
        xe[kh] = __builtin_bit_cast(bf16x8, __builtin_convertvector((f32x8v{x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]}), hwbf16x8));
    }
}

// slot tile (accumulator, lane = query, rows = slots) -> this lane's 32 bucket values of table
// g (0 vertical / 1 horizontal) in `bk`, and the full bucket rows row[q][0..63] in scratch
__device__ __forceinline__ void slots_to_buckets(float (&bk)[32], float* scr, const f32x16& x, int lane, int qi,
                                                 int qr, int qc, const RelGeom& G) {
    const int g = lane >> 5;
    float* row = scr + (lane & 31) * LP;
#pragma unroll
    for (int r = 0; r < 16; ++r) row[acc_row(r, g)] = x[r];
    wave_lds_fence();
#pragma unroll
    for (int u = 0; u < 32; ++u) bk[u] = bucket_from_slots(row, u, g, qi, qr, qc, G);
    wave_lds_fence();
}

// bucket rows^T (64 buckets x NP queries, dtype T) for the second backward launch
template <typename T>
__device__ __forceinline__ void store_buckets_T(typename Tr<T>::elem* dst /* + qi */, int NP,
                                                const float (&bk)[32], int g) {
#pragma unroll
    for (int u = 0; u < 32; ++u) dst[(int64_t)(g * 32 + u) * NP] = Tr<T>::from_f(bk[u]);
}

// acc^T(64 x 32 queries) += Tab^T(64 x 64 buckets) . rows^T  with Tab^T in LDS ([64][tp], columns
// 0..31 vertical / 32..63 horizontal table) and the bucket rows still in registers: lane (q, g)
// holds the 32 buckets of table g of its query, so in contraction step ks lane group g supplies
// the elements (table g, bucket ks*EPL + e) — the order of the contraction index is free as
// long as both operands agree.  No LDS round trip for the bucket rows.
template <typename T>
__device__ __forceinline__ void add_bucket_product(f32x16 (&o)[2], const typename Tr<T>::elem* tabT,
                                                   const float (&bk)[32], int lane) {
    using TT = Tr<T>;
    constexpr int tp = table_pitch<T>();
    const int g = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < 32 / TT::EPL; ++ks) {
        typename TT::frag b;
        if constexpr (TT::EPL == 1) b = bk[ks];
        else {
            f32x8v x;
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = bk[ks * 8 + e];
            b = __builtin_bit_cast(bf16x8, __builtin_convertvector(x, hwbf16x8));
        }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
            o[dt] = TT::mma(TT::load(tabT + ((lane & 31) + 32 * dt) * tp + g * 32 + ks * TT::EPL), b, o[dt]);
    }
}

// ---- streamed operand tiles -----------------------------------------------------------------
// Every operand that all waves of the workgroup read (K, V, Q, dO, ...) is streamed through LDS
// one 32-token tile at a time: full 128-byte lines, each fetched ONCE per workgroup, register
// staged (loads for tile t+1 are in flight while tile t is consumed; written to the other
// half of a double buffer before the single barrier of the iteration).  Reading such rows
// straight from global memory per wave costs 7x the L2 traffic at a quarter line efficiency
// (16 B of each 128-B line per instruction) — measured 36k of 54k cycles in the dK/dV loop.
template <typename T, int ROWS, int COLS> struct TileRegs {
    static constexpr int V = 16 / sizeof(typename Tr<T>::elem), CPR = COLS / V, CH = ROWS * CPR, NI = (CH + 255) / 256;
    u32x4v v[NI];
};

// rows [row0, row0 + ROWS) of a row-major matrix (row stride `rs` elements), zero beyond `nrows`
template <typename T, int ROWS, int COLS>
__device__ __forceinline__ void tile_load(TileRegs<T, ROWS, COLS>& r, const typename Tr<T>::elem* src, int64_t rs,
                                          int row0, int nrows, int col0 = 0) {
    using R = TileRegs<T, ROWS, COLS>;
#pragma unroll
    for (int i = 0; i < R::NI; ++i) {
        const int c = threadIdx.x + i * blockDim.x;
        const int row = c / R::CPR, cc = c - row * R::CPR;
        r.v[i] = (c < R::CH && row0 + row < nrows)
                     ? *reinterpret_cast<const u32x4v*>(src + (int64_t)(row0 + row) * rs + col0 + cc * R::V)
                     : u32x4v{0, 0, 0, 0};
    }
}

// RM: dst_rm[row][col] (pitch prm);  TR: dst_t[col][row] (pitch pt)
template <typename T, int ROWS, int COLS, bool RM, bool TR>
__device__ __forceinline__ void tile_store(const TileRegs<T, ROWS, COLS>& r, typename Tr<T>::elem* dst_rm, int prm,
                                           typename Tr<T>::elem* dst_t, int pt) {
    using R = TileRegs<T, ROWS, COLS>;
    using E = typename Tr<T>::elem;
#pragma unroll
    for (int i = 0; i < R::NI; ++i) {
        const int c = threadIdx.x + i * blockDim.x;
        if (c < R::CH) {
            const int row = c / R::CPR, cc = c - row * R::CPR;
            union { u32x4v v; E e[R::V]; } u;
            u.v = r.v[i];
            if constexpr (RM) {
                if constexpr (sizeof(E) == 2) {
                    E* d = dst_rm + row * prm + cc * R::V;
                    if ((prm * 2) % 16 == 0) *reinterpret_cast<u32x4v*>(d) = u.v;
                    else {                                   // 8-byte aligned rows (pitch 36)
                        *reinterpret_cast<u32x2v*>(d) = u32x2v{u.v[0], u.v[1]};
                        *reinterpret_cast<u32x2v*>(d + 4) = u32x2v{u.v[2], u.v[3]};
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < R::V; ++e) dst_rm[row * prm + cc * R::V + e] = u.e[e];
                }
            }
            if constexpr (TR) {
#pragma unroll
                for (int e = 0; e < R::V; ++e) dst_t[(cc * R::V + e) * pt + row] = u.e[e];
            }
        }
    }
}

// The same with a GROUP of 256 threads (4 waves) owning the tile: thread `tid` (0..255) of the group
// moves chunks tid, tid + 256, ... — every thread of the group has work (no predicate, no
// exec-mask branch); callers pick the group wave-uniformly.
template <typename T, int ROWS, int COLS>
__device__ __forceinline__ void tile_load_g(TileRegs<T, ROWS, COLS>& r, const typename Tr<T>::elem* src, int64_t rs,
                                            int row0, int nrows, int col0, int tid) {
    using R = TileRegs<T, ROWS, COLS>;
    static_assert(R::CH % 256 == 0, "tile must split evenly over a 256-thread group");
#pragma unroll
    for (int i = 0; i < R::NI; ++i) {
        const int c = tid + i * 256;
        const int row = c / R::CPR, cc = c - row * R::CPR;
        const int rr = min(row0 + row, nrows - 1);
        const u32x4v v = *reinterpret_cast<const u32x4v*>(src + (int64_t)rr * rs + col0 + cc * R::V);
        r.v[i] = row0 + row < nrows ? v : u32x4v{0, 0, 0, 0};
    }
}

template <typename T, int ROWS, int COLS, bool RM, bool TR>
__device__ __forceinline__ void tile_store_g(const TileRegs<T, ROWS, COLS>& r, typename Tr<T>::elem* dst_rm, int prm,
                                             typename Tr<T>::elem* dst_t, int pt, int tid) {
    using R = TileRegs<T, ROWS, COLS>;
    using E = typename Tr<T>::elem;
#pragma unroll
    for (int i = 0; i < R::NI; ++i) {
        const int c = tid + i * 256;
        const int row = c / R::CPR, cc = c - row * R::CPR;
        union { u32x4v v; E e[R::V]; } u;
        u.v = r.v[i];
        if constexpr (RM) {
            if constexpr (sizeof(E) == 2) {
                E* d = dst_rm + row * prm + cc * R::V;
                if ((prm * 2) % 16 == 0) *reinterpret_cast<u32x4v*>(d) = u.v;
                else {                                   // 8-byte aligned rows (pitch 36)
                    *reinterpret_cast<u32x2v*>(d) = u32x2v{u.v[0], u.v[1]};
                    *reinterpret_cast<u32x2v*>(d + 4) = u32x2v{u.v[2], u.v[3]};
                }
            } else {
#pragma unroll
                for (int e = 0; e < R::V; ++e) dst_rm[row * prm + cc * R::V + e] = u.e[e];
            }
        }
        if constexpr (TR) {
#pragma unroll
            for (int e = 0; e < R::V; ++e) dst_t[(cc * R::V + e) * pt + row] = u.e[e];
        }
    }
}

// pitches of staged tiles: row-major [32][RMP(cols)], transposed / bucket-row tiles [rows][TPT]
template <typename T> __host__ __device__ constexpr int rm_pitch(int cols) { return sizeof(typename Tr<T>::elem) == 2 ? cols + 8 : cols + 1; }
template <typename T> __host__ __device__ constexpr int t_pitch() { return sizeof(typename Tr<T>::elem) == 2 ? 36 : 33; }

// workgroup-cooperative table staging.  Two phases so that ALL global loads of a workgroup's
// prologue are in flight together (a load -> convert -> store loop pays one L2/HBM round trip per
// iteration: 6-9 dependent round trips were a quarter of the forward kernel):
//   tab_load  : this thread's float4 pieces (4 d-values of one bucket) of a (v, h) table pair
//   tab_store_T: tabT[d][u] = (u < 32 ? tv[u][d] : th[u-32][d]), zero for u >= nb   (transposed)
//   tab_store_R: tabR[u][d] operand rows, rows 0..31 from tv, 32..63 from th
constexpr int TAB_IT = 4;                        // 64 buckets x 16 pieces = 1024 <= 4 x 256 threads
struct TabRegs { f32x4v v[TAB_IT]; };

__device__ __forceinline__ void tab_load(TabRegs& r, const float* tv, const float* th, int ldt, int nb) {
#pragma unroll
    for (int it = 0; it < TAB_IT; ++it) {
        const int i = threadIdx.x + it * blockDim.x;
        const int d4 = (i & 15) * 4, u = (i >> 4) & 63, uu = u & 31;
        const float* t = u < 32 ? tv : th;
        r.v[it] = (i < 1024 && uu < nb) ? *reinterpret_cast<const f32x4v*>(t + (int64_t)uu * ldt + d4) : f32x4v{0, 0, 0, 0};
    }
}
template <typename T>
__device__ __forceinline__ void tab_store_T(const TabRegs& r, typename Tr<T>::elem* tabT) {
    constexpr int tp = table_pitch<T>();
#pragma unroll
    for (int it = 0; it < TAB_IT; ++it) {
        const int i = threadIdx.x + it * blockDim.x;
        if (i < 1024) {
            const int d4 = (i & 15) * 4, u = i >> 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) tabT[(d4 + e) * tp + u] = Tr<T>::from_f(r.v[it][e]);
        }
    }
}
template <typename T>
__device__ __forceinline__ void tab_store_R(const TabRegs& r, typename Tr<T>::elem* tabR) {
    constexpr int tp = table_pitch<T>();
#pragma unroll
    for (int it = 0; it < TAB_IT; ++it) {
        const int i = threadIdx.x + it * blockDim.x;
        if (i < 1024) {
            const int d4 = (i & 15) * 4, u = i >> 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) tabR[u * tp + d4 + e] = Tr<T>::from_f(r.v[it][e]);
        }
    }
}

// ---- one-hot key operands as ready-made bf16 MFMA fragments (fast path) ------------------------
// ohr[j][c]  ([NP][OHP])     : rows = keys, contraction = slots  (S^T += E . X^T)
// oht[c][j]  ([32][NP + 4])  : rows = slots, contraction = keys  (slot sums += E^T . P^T), read
//                              with load_perm like a transposed V tile
// Built once per workgroup from the geometry; the bit-twiddled operands (Tr::onehot_row /
// onehot_perm, ~45 VALU instructions per key tile and wave) disappear from the tile loops.
constexpr int OHP = 40;
__host__ __device__ constexpr int oht_pitch(int NP) { return NP + 4; }
__host__ __device__ constexpr size_t onehot_bytes(int NP) { return (size_t)NP * OHP * 2 + (size_t)32 * oht_pitch(NP) * 2; }

__device__ __forceinline__ void fill_onehot(short* ohr, short* oht, const uint32_t* masks, int NP) {
    // masks[] must be visible (barrier) before this call
    for (int i = threadIdx.x; i < NP * 4; i += blockDim.x) {          // 8 slots of one key
        const int j = i >> 2, cc = i & 3;
        const uint32_t m = masks[j] >> (8 * cc);
        u32x4v w;
#pragma unroll
        for (int p = 0; p < 4; ++p) w[p] = ((m >> (2 * p)) & 1u) * 0x3F80u + ((m >> (2 * p + 1)) & 1u) * 0x3F800000u;
        *reinterpret_cast<u32x4v*>(ohr + j * OHP + cc * 8) = w;
    }
    const int tpo = oht_pitch(NP);
    for (int i = threadIdx.x; i < 32 * (NP >> 3); i += blockDim.x) {  // 8 keys of one slot
        const int c = i / (NP >> 3), j0 = (i - c * (NP >> 3)) * 8;
        const u32x4v lo = *reinterpret_cast<const u32x4v*>(masks + j0);
        const u32x4v hi = *reinterpret_cast<const u32x4v*>(masks + j0 + 4);
        u32x2v w0, w1;
        w0[0] = ((lo[0] >> c) & 1u) * 0x3F80u + ((lo[1] >> c) & 1u) * 0x3F800000u;
        w0[1] = ((lo[2] >> c) & 1u) * 0x3F80u + ((lo[3] >> c) & 1u) * 0x3F800000u;
        w1[0] = ((hi[0] >> c) & 1u) * 0x3F80u + ((hi[1] >> c) & 1u) * 0x3F800000u;
        w1[1] = ((hi[2] >> c) & 1u) * 0x3F80u + ((hi[3] >> c) & 1u) * 0x3F800000u;
        *reinterpret_cast<u32x2v*>(oht + c * tpo + j0) = w0;
        *reinterpret_cast<u32x2v*>(oht + c * tpo + j0 + 4) = w1;
    }
}

template <typename T>
__device__ __forceinline__ void store_ext_rows(typename Tr<T>::elem* dst /* row of 32 */,
                                               const typename Tr<T>::frag (&xe)[32 / Tr<T>::KI], int g) {
    using TT = Tr<T>;
#pragma unroll
    for (int ks = 0; ks < 32 / TT::KI; ++ks) {
        if constexpr (TT::EPL == 1) dst[ks * 2 + g] = xe[ks];
        else *reinterpret_cast<bf16x8*>(dst + ks * TT::KI + g * TT::EPL) = xe[ks];
    }
}

// accumulator tile (lane = row n of the output, 16 x 2 d-values) -> (.., n, h, :) row pointer
template <typename T>
__device__ __forceinline__ void store_rows_64(typename Tr<T>::elem* op, const f32x16 (&o)[2], int g) {
    using TT = Tr<T>;
    using E = typename TT::elem;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int d = dt * 32 + 8 * r4 + 4 * g;
            if constexpr (sizeof(E) == 2) {
                *reinterpret_cast<u32x2v*>(op + d) = u32x2v{f2bf_pair(o[dt][4 * r4], o[dt][4 * r4 + 1]),
                                                            f2bf_pair(o[dt][4 * r4 + 2], o[dt][4 * r4 + 3])};
            } else {
                *reinterpret_cast<f32x4v*>(op + d) =
                    f32x4v{o[dt][4 * r4], o[dt][4 * r4 + 1], o[dt][4 * r4 + 2], o[dt][4 * r4 + 3]};
            }
        }
}

template <typename T> __host__ __device__ constexpr int tabr_rows(int n_tables) { return tables_in_lds<T>() ? 32 * n_tables : 0; }

// bytes of one set of staged tiles
template <typename T> __host__ __device__ constexpr size_t rm_tile_bytes(int cols) { return (size_t)32 * rm_pitch<T>(cols) * sizeof(typename Tr<T>::elem); }
template <typename T> __host__ __device__ constexpr size_t t_tile_bytes() { return (size_t)64 * t_pitch<T>() * sizeof(typename Tr<T>::elem); }

}  // namespace

// l0_mask.hip — TinyCLIP's pruning masks (TinyCLIP/src/open_clip/l0module.py, model.py:40-68, :131-136, :273-282) kept out of
// the activations (gfx950).  With zh = hidden_z (D), zd = heads_z[l] (H), zi = intermediate_z[l] (F) a masked block is the
// dense block on the EFFECTIVE operands
//     Wo' = diag(zh) Wo diag(e(zd))   bo' = zh * bo        W2' = diag(zh) W2 diag(zi)   b2' = zh * b2
// with ln_1 / ln_2 replaced by the masked LayerNorm.  Three kernel groups, all bandwidth kernels at activation (a) or weight
// (b, c) size, one pass, no atomics, fixed summation orders (bit-reproducible, independent of the grid):
//   a. masked LayerNorm forward (+ folded residual add) and backward: statistics over the kept columns (z != 0) only —
//      selected, never multiplied, whatever the dropped columns hold —, exact zeros in the dropped columns of y, of the
//      LayerNorm's part of dx and of the dgamma / dbeta partials; the residual gradient passes through;
//   b. masked operand pack: bf16((W[i,k] r[i]) c[k]) as (rows, cols) and transposed copies, several tensors per launch;
//   c. masked gradient finalisation: G = sum of the split-K partials (the tree of cream_grad_finalize),
//      dst (+)= r (x) c . G,  dr[i] = sum_k G W c,  dc[k or head] = sum_i G W r  — the gradients of the masks at weight size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_common.hpp"
#include "lane_ops.hpp"
#include "cream_amd.h"
#include "cu_budget.hpp"
#include "launch_ev.hpp"

namespace {
using namespace cream;

__device__ __forceinline__ void unpack4(u32x2v v, float (&f)[4]) {
    f[0] = __uint_as_float(v[0] << 16); f[1] = __uint_as_float(v[0] & 0xFFFF0000u);
    f[2] = __uint_as_float(v[1] << 16); f[3] = __uint_as_float(v[1] & 0xFFFF0000u);
}
__device__ __forceinline__ u32x2v pack4(const float (&f)[4]) { return u32x2v{f2bf_pair(f[0], f[1]), f2bf_pair(f[2], f[3])}; }

constexpr int LN_MAXC = 5;          // float4 chunks per lane: E <= 64 * 4 * 5 = 1280 (as csrc/block_ops.hip)

// ---- a. masked LayerNorm forward: one wave per row (the structure of block_ops.hip's ln_fwd_kernel) ------------------------
__global__ __launch_bounds__(256) void ln_fwd_masked_kernel(uint16_t* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
                                                            const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ z, float inv_keep,
                                                            int M, int E, float eps, float* __restrict__ xsum,
                                                            const uint16_t* __restrict__ res, const float* __restrict__ sscale,
                                                            int rows_per_sample) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= M) return;
    const int nch = E >> 2;
    const float* xr = x + (int64_t)row * E;
    f32x4v v[LN_MAXC];
    bool kp[LN_MAXC][4];
    float s = 0.f;
    const float sc = (res && sscale) ? sscale[row / rows_per_sample] : 1.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        v[i] = f32x4v{0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; ++e) kp[i][e] = false;
        if (c < nch) {
            v[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4v*>(xr + 4 * c));
            const f32x4v zv = *reinterpret_cast<const f32x4v*>(z + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) kp[i][e] = zv[e] != 0.f;
            if (res) {
                float r[4];
                unpack4(__builtin_nontemporal_load(reinterpret_cast<const u32x2v*>(res + (int64_t)row * E + 4 * c)), r);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[i][e] += sc * r[e];
                __builtin_nontemporal_store(v[i], reinterpret_cast<f32x4v*>(xsum + (int64_t)row * E + 4 * c));      // every column
            }
        }
        // selected: a dropped column never enters an addition
        s += ((kp[i][0] ? v[i][0] : 0.f) + (kp[i][1] ? v[i][1] : 0.f)) + ((kp[i][2] ? v[i][2] : 0.f) + (kp[i][3] ? v[i][3] : 0.f));
    }
    const float mu = wave_sum(s) * inv_keep;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = kp[i][e] ? v[i][e] - mu : 0.f;
            q += d * d;
        }
    const float rs = rsqrtf(wave_sum(q) * inv_keep + eps);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
    uint16_t* yr = y + (int64_t)row * E;
#pragma unroll
    for (int i = 0; i < LN_MAXC; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            const f32x4v g = *reinterpret_cast<const f32x4v*>(gamma + 4 * c);
            const f32x4v b = *reinterpret_cast<const f32x4v*>(beta + 4 * c);
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = kp[i][e] ? (v[i][e] - mu) * rs * g[e] + b[e] : 0.f;
            *reinterpret_cast<u32x2v*>(yr + 4 * c) = pack4(o);
        }
    }
}

// ---- a. masked LayerNorm backward: grid = P workgroups of 4 waves, wave w of workgroup p walks rows p*4 + w, += 4P, ...
// (the partial layout of block_ops.hip's ln_bwd_kernel: partial[p][0] dgamma, [1] dbeta, [2] column sums of dx_scaled)
template <int MAXC>
__global__ __launch_bounds__(256) void ln_bwd_masked_kernel(float* __restrict__ dx, uint16_t* __restrict__ dxs, float* __restrict__ partial,
                                                            const uint16_t* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ z, float inv_keep,
                                                            const float* __restrict__ dres, const float* __restrict__ sscale,
                                                            int rows_per_sample, int M, int E) {
    __shared__ float red[4][MAXC * 256 + 4];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nch = E >> 2;
    f32x4v g[MAXC], ag[MAXC], ab[MAXC], as[MAXC];
    bool kp[MAXC][4];
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c = lane + 64 * i;
        g[i] = c < nch ? *reinterpret_cast<const f32x4v*>(gamma + 4 * c) : f32x4v{0, 0, 0, 0};
        const f32x4v zv = c < nch ? *reinterpret_cast<const f32x4v*>(z + 4 * c) : f32x4v{0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; ++e) kp[i][e] = zv[e] != 0.f;
        ag[i] = f32x4v{0, 0, 0, 0};
        ab[i] = f32x4v{0, 0, 0, 0};
        as[i] = f32x4v{0, 0, 0, 0};
    }
    const int stride = gridDim.x * 4;
    for (int row = blockIdx.x * 4 + wave; row < M; row += stride) {
        const int64_t ro = (int64_t)__builtin_amdgcn_readfirstlane(row) * E;
        const float mu = mean[row], rs = rstd[row];
        const float sc = sscale ? sscale[row / rows_per_sample] : 1.f;
        float xh[MAXC][4], d[MAXC][4];
        f32x4v xin[MAXC], rin[MAXC];
        u32x2v dyin[MAXC];
        float s1 = 0.f, s2 = 0.f;
        // all three row operands are requested before the reductions (one memory round trip per row, not two)
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const unsigned c = lane + 64 * i;
            if (c < (unsigned)nch) {
                xin[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4v*>(x + ro + 4u * c));
                dyin[i] = *reinterpret_cast<const u32x2v*>(dy + ro + 4u * c);
                rin[i] = dres ? __builtin_nontemporal_load(reinterpret_cast<const f32x4v*>(dres + ro + 4u * c)) : f32x4v{0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const unsigned c = lane + 64 * i;
#pragma unroll
            for (int e = 0; e < 4; ++e) { xh[i][e] = 0.f; d[i][e] = 0.f; }
            if (c < (unsigned)nch) {
                const f32x4v xv = xin[i];
                float dyv[4];
                unpack4(dyin[i], dyv);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (kp[i][e]) {                                   // a dropped column: y is the constant 0, its dy is discarded
                        xh[i][e] = (xv[e] - mu) * rs;
                        ag[i][e] += dyv[e] * xh[i][e];
                        ab[i][e] += dyv[e];
                        const float dg = dyv[e] * g[i][e];
                        d[i][e] = dg;
                        s1 += dg;
                        s2 += dg * xh[i][e];
                    }
                }
            }
        }
        s1 = wave_sum(s1) * inv_keep;
        s2 = wave_sum(s2) * inv_keep;
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const unsigned c = lane + 64 * i;
            if (c < (unsigned)nch) {
                f32x4v r = rin[i];
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (kp[i][e]) r[e] += rs * (d[i][e] - s1 - xh[i][e] * s2);
                    o[e] = r[e] * sc;
                }
                __builtin_nontemporal_store(r, reinterpret_cast<f32x4v*>(dx + ro + 4u * c));
                if (dxs) {
                    const u32x2v pk = pack4(o);
                    *reinterpret_cast<u32x2v*>(dxs + ro + 4u * c) = pk;
                    unpack4(pk, o);                                   // the values as written
#pragma unroll
                    for (int e = 0; e < 4; ++e) as[i][e] += o[e];
                }
            }
        }
    }
#pragma unroll
    for (int which = 0; which < 3; ++which) {
#pragma unroll
        for (int i = 0; i < MAXC; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                red[wave][(i * 64 + lane) * 4 + e] = which == 0 ? ag[i][e] : (which == 1 ? ab[i][e] : as[i][e]);
        __syncthreads();
        float* prow = partial + ((int64_t)blockIdx.x * 3 + which) * E;
#pragma nounroll
        for (unsigned c = threadIdx.x; c < (unsigned)E; c += 256)
            prow[c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        __syncthreads();
    }
}

// ---- job tables (passed by value in the kernel arguments, as cream_grad_finalize does) ---------------------------------------
constexpr int TILE = 64;            // the weight-size kernels walk fixed tiles (pack 64 x 64, finalisation 16 x 64): the tiling, and
constexpr int GROWS = 16;           // with it every summation order, follows from the shapes alone — never from the grid
struct PackJobs {
    cream_mask_pack_job job[CREAM_MAX_MASK_JOBS];
    int first[CREAM_MAX_MASK_JOBS + 1];
    int njobs;
};
struct MaskGradJobs {
    cream_mask_grad_job job[CREAM_MAX_MASK_JOBS];
    int first[CREAM_MAX_MASK_JOBS + 1];           // tiles (first kernel) / reduction blocks (second kernel)
    int njobs;
};

__host__ __device__ __forceinline__ int tiles_of(int n) { return (n + TILE - 1) / TILE; }
__host__ __device__ __forceinline__ int gtiles_of(int rows) { return (rows + GROWS - 1) / GROWS; }

template <typename J>
__device__ __forceinline__ int find_job(const J& jobs, int item) {
    int j = 0;
    while (j + 1 < jobs.njobs && item >= jobs.first[j + 1]) ++j;
    return j;
}

// ---- b. masked operand pack ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_pack_kernel(const PackJobs J) {
    __shared__ __attribute__((aligned(16))) uint16_t tile[TILE][TILE + 8];
    const int cc = threadIdx.x & 15, rq = threadIdx.x >> 4;
    const int total = J.first[J.njobs];
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const int j = find_job(J, t);
        const cream_mask_pack_job& jb = J.job[j];
        const int lt = t - J.first[j], tcn = tiles_of(jb.cols);
        const int r0 = (lt / tcn) * TILE, c0 = (lt % tcn) * TILE;
        const int col = c0 + 4 * cc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int lr = rq + 16 * q, row = r0 + lr;
            u32x2v pk = u32x2v{0, 0};
            if (row < jb.rows && col < jb.cols) {                     // cols % 4 == 0: the whole chunk is inside
                const f32x4v w = *reinterpret_cast<const f32x4v*>(jb.w + (int64_t)row * jb.ld + col);
                const float rv = jb.r ? jb.r[row] : 1.f;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float cv = jb.c ? jb.c[(col + e) / jb.c_group] : 1.f;
                    o[e] = (w[e] * rv) * cv;                          // fp32 products in this order, rounded once
                }
                pk = pack4(o);
                if (jb.mir) *reinterpret_cast<u32x2v*>(reinterpret_cast<uint16_t*>(jb.mir) + (int64_t)row * jb.ld_mir + col) = pk;
            }
            *reinterpret_cast<u32x2v*>(&tile[lr][4 * cc]) = pk;
        }
        __syncthreads();
        if (jb.mir_t) {                                               // (cols, rows): thread = one source column, 16 source rows
            const int lc = threadIdx.x >> 2, seg = threadIdx.x & 3;
            const int k = c0 + lc;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int lr = 16 * seg + 4 * q, rb = r0 + lr;
                if (k < jb.cols && rb < jb.rows) {                    // rows % 4 == 0 with a transposed copy
                    const uint32_t lo = (uint32_t)tile[lr][lc] | ((uint32_t)tile[lr + 1][lc] << 16);
                    const uint32_t hi = (uint32_t)tile[lr + 2][lc] | ((uint32_t)tile[lr + 3][lc] << 16);
                    *reinterpret_cast<u32x2v*>(reinterpret_cast<uint16_t*>(jb.mir_t) + (int64_t)k * jb.ld_mir_t + rb) = u32x2v{lo, hi};
                }
            }
        }
        __syncthreads();
    }
}

// ---- c. masked gradient finalisation --------------------------------------------------------------------------------------------
// the summation tree of cream_grad_finalize (csrc/block_ops.hip: grad_part_lanes / grad_finalize_job), walked by one thread:
// part lane l adds parts l, l + PL, ... in ascending order; the lanes are added in ascending order (PL = 64: 8 groups of 8, then
// the 8 sums)
__host__ __device__ __forceinline__ int part_lanes(int nparts) { return nparts <= 16 ? 4 : (nparts <= 64 ? 16 : 64); }

__device__ __forceinline__ f32x4v load_part(const cream_mask_grad_job& jb, int p, int64_t off) {
    const int64_t idx = (int64_t)p * jb.pstride + off;
    if (jb.src_bf16) {
        float f[4];
        unpack4(*reinterpret_cast<const u32x2v*>(reinterpret_cast<const uint16_t*>(jb.src) + idx), f);
        return f32x4v{f[0], f[1], f[2], f[3]};
    }
    return *reinterpret_cast<const f32x4v*>(reinterpret_cast<const float*>(jb.src) + idx);
}

__device__ __forceinline__ f32x4v part_sum(const cream_mask_grad_job& jb, int64_t off) {
    const int PL = part_lanes(jb.nparts);
    const int groups = PL == 64 ? 8 : 1, per = PL / groups;
    f32x4v total = f32x4v{0, 0, 0, 0};
    for (int gi = 0; gi < groups; ++gi) {
        f32x4v gs = f32x4v{0, 0, 0, 0};
        for (int l = 0; l < per; ++l) {
            f32x4v acc = f32x4v{0, 0, 0, 0};
            int p = gi * per + l;
            for (; p + 3 * PL < jb.nparts; p += 4 * PL) {             // four loads in flight, added in ascending order
                const f32x4v a0 = load_part(jb, p, off), a1 = load_part(jb, p + PL, off);
                const f32x4v a2 = load_part(jb, p + 2 * PL, off), a3 = load_part(jb, p + 3 * PL, off);
                acc += a0; acc += a1; acc += a2; acc += a3;
            }
            for (; p < jb.nparts; p += PL) acc += load_part(jb, p, off);
            gs = l == 0 ? acc : gs + acc;
        }
        total = gi == 0 ? gs : total + gs;
    }
    return total;
}

// workspace of a job: row partials [column tile][row], then column partials [row tile][column]
__host__ __device__ __forceinline__ int64_t ws_rows(const cream_mask_grad_job& jb) { return (int64_t)tiles_of(jb.cols) * jb.rows; }

__global__ __launch_bounds__(256) void mask_grad_tiles_kernel(const MaskGradJobs J) {
    __shared__ float colred[16][TILE];
    const int cc = threadIdx.x & 15, rq = threadIdx.x >> 4;
    const int total = J.first[J.njobs];
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const int j = find_job(J, t);
        const cream_mask_grad_job& jb = J.job[j];
        const int lt = t - J.first[j], tcn = tiles_of(jb.cols);
        const int tr = lt / tcn, tc = lt % tcn;
        const int r0 = tr * GROWS, c0 = tc * TILE;
        const int col = c0 + 4 * cc;
        float cv[4] = {1.f, 1.f, 1.f, 1.f};
        if (jb.c && col < jb.cols) {
#pragma unroll
            for (int e = 0; e < 4; ++e) cv[e] = jb.c[(col + e) / jb.c_group];
        }
        float colacc[4] = {0.f, 0.f, 0.f, 0.f};
        {
            const int row = r0 + rq;
            float rowv = 0.f;
            if (row < jb.rows && col < jb.cols) {
                const f32x4v G = part_sum(jb, (int64_t)row * jb.cols + col);
                const float rv = jb.r ? jb.r[row] : 1.f;
                float* d = jb.dst + (int64_t)row * jb.ld + col;
                f32x4v o = jb.overwrite ? f32x4v{0, 0, 0, 0} : *reinterpret_cast<const f32x4v*>(d);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += (rv * cv[e]) * G[e];
                *reinterpret_cast<f32x4v*>(d) = o;
                const f32x4v w = *reinterpret_cast<const f32x4v*>(jb.w + (int64_t)row * jb.ld_w + col);
                float tv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    tv[e] = G[e] * w[e];
                    colacc[e] = tv[e] * rv;
                }
                rowv = (tv[0] * cv[0] + tv[1] * cv[1]) + (tv[2] * cv[2] + tv[3] * cv[3]);
            }
            // the 16 lanes of a tile row are consecutive lanes of one wave: fixed butterfly
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) rowv += __shfl_xor(rowv, off);
            if (cc == 0 && row < jb.rows && jb.dr_out) jb.ws[(int64_t)tc * jb.rows + row] = rowv;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) colred[rq][4 * cc + e] = colacc[e];
        __syncthreads();
        if (threadIdx.x < TILE && c0 + (int)threadIdx.x < jb.cols && jb.dc_out) {
            float s = colred[0][threadIdx.x];
            for (int q = 1; q < 16; ++q) s += colred[q][threadIdx.x];
            jb.ws[ws_rows(jb) + (int64_t)tr * jb.cols + c0 + threadIdx.x] = s;
        }
        __syncthreads();
    }
}

// second launch: the tile partials in ascending tile order.  Blocks of a job: ceil(rows / 256) for dr, then for dc
// ceil(cols / 256) (c_group 1: a thread per column) or ceil(groups / 4) (c_group 64: a wave per group, fixed butterfly)
__host__ __device__ __forceinline__ int dr_blocks(const cream_mask_grad_job& jb) { return jb.dr_out ? (jb.rows + 255) / 256 : 0; }
__host__ __device__ __forceinline__ int dc_blocks(const cream_mask_grad_job& jb) {
    if (!jb.dc_out) return 0;
    return jb.c_group == 1 ? (jb.cols + 255) / 256 : (jb.cols / jb.c_group + 3) / 4;
}

__global__ __launch_bounds__(256) void mask_grad_reduce_kernel(const MaskGradJobs J) {
    const int total = J.first[J.njobs];
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const int j = find_job(J, t);
        const cream_mask_grad_job& jb = J.job[j];
        int b = t - J.first[j];
        const int trn = gtiles_of(jb.rows), tcn = tiles_of(jb.cols);
        if (b < dr_blocks(jb)) {
            const int i = b * 256 + threadIdx.x;
            if (i < jb.rows) {
                float s = jb.ws[i];
                for (int k = 1; k < tcn; ++k) s += jb.ws[(int64_t)k * jb.rows + i];
                jb.dr_out[i] = jb.dr_accumulate ? jb.dr_out[i] + s : s;
            }
            continue;
        }
        b -= dr_blocks(jb);
        const float* cp = jb.ws + ws_rows(jb);
        if (jb.c_group == 1) {
            const int k = b * 256 + threadIdx.x;
            if (k < jb.cols) {
                float s = cp[k];
                for (int q = 1; q < trn; ++q) s += cp[(int64_t)q * jb.cols + k];
                jb.dc_out[k] = jb.dc_accumulate ? jb.dc_out[k] + s : s;
            }
        } else {                                                      // c_group == 64 == the wave
            const int gidx = b * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
            const bool on = gidx < jb.cols / jb.c_group;
            float s = 0.f;
            if (on) {
                const int k = gidx * 64 + lane;
                s = cp[k];
                for (int q = 1; q < trn; ++q) s += cp[(int64_t)q * jb.cols + k];
            }
            s = wave_sum(s);
            if (on && lane == 0) jb.dc_out[gidx] = jb.dc_accumulate ? jb.dc_out[gidx] + s : s;
        }
    }
}

int ln_masked_args(int M, int E, int n_keep) {
    if (M < 0 || E <= 0 || n_keep <= 0 || n_keep > E) return CREAM_ERR_BAD_ARG;      // (no kept column: nothing to normalise)
    if (E % 4 || E > 64 * 4 * LN_MAXC) return CREAM_ERR_TOO_LARGE;
    return CREAM_OK;
}

int grid_cap(int items, int per_cu) {
    const int cap = cu_count() * per_cu;
    return items < cap ? items : cap;
}

}  // namespace

extern "C" {

int cream_ln_fwd_masked(void* y, float* mean, float* rstd, const float* x, const float* gamma, const float* beta, const float* z,
                        int n_keep, int M, int E, float eps, void* stream)
{
    const int rc = ln_masked_args(M, E, n_keep);
    if (rc != CREAM_OK) return rc;
    if (M == 0) return CREAM_OK;
    if (!y || !mean || !rstd || !x || !gamma || !beta || !z) return CREAM_ERR_BAD_ARG;
    if (((uintptr_t)y | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)z) % 16) return CREAM_ERR_BAD_ARG;
    CREAM_LAUNCH(ln_fwd_masked_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (uint16_t*)y, mean, rstd, x, gamma, beta, z,
                 1.f / (float)n_keep, M, E, eps, (float*)nullptr, (const uint16_t*)nullptr, (const float*)nullptr, 1);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int cream_add_ln_fwd_masked(float* xsum, void* y, float* mean, float* rstd, const float* x, const void* res, const float* sample_scale,
                            int rows_per_sample, const float* gamma, const float* beta, const float* z, int n_keep, int M, int E,
                            float eps, void* stream)
{
    const int rc = ln_masked_args(M, E, n_keep);
    if (rc != CREAM_OK) return rc;
    if (rows_per_sample <= 0) return CREAM_ERR_BAD_ARG;
    if (M == 0) return CREAM_OK;
    if (!xsum || !y || !mean || !rstd || !x || !res || !gamma || !beta || !z) return CREAM_ERR_BAD_ARG;
    if (((uintptr_t)xsum | (uintptr_t)y | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)z) % 16 || (uintptr_t)res % 8)
        return CREAM_ERR_BAD_ARG;
    CREAM_LAUNCH(ln_fwd_masked_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (uint16_t*)y, mean, rstd, x, gamma, beta, z,
                 1.f / (float)n_keep, M, E, eps, xsum, (const uint16_t*)res, sample_scale, rows_per_sample);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int cream_ln_bwd_masked(float* dx, void* dx_scaled, float* partial, const void* dy, const float* x, const float* mean, const float* rstd,
                        const float* gamma, const float* z, int n_keep, const float* dres, const float* sample_scale,
                        int rows_per_sample, int M, int E, void* stream)
{
    const int rc = ln_masked_args(M, E, n_keep);
    if (rc != CREAM_OK) return rc;
    if (M == 0 || rows_per_sample <= 0) return CREAM_ERR_BAD_ARG;
    if (!dx || !partial || !dy || !x || !mean || !rstd || !gamma || !z) return CREAM_ERR_BAD_ARG;
    if (((uintptr_t)dx | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)z | (uintptr_t)dres) % 16 ||
        ((uintptr_t)dx_scaled | (uintptr_t)dy) % 8)
        return CREAM_ERR_BAD_ARG;
    auto kern = E <= 512 ? ln_bwd_masked_kernel<2> : (E <= 768 ? ln_bwd_masked_kernel<3> : ln_bwd_masked_kernel<LN_MAXC>);
    CREAM_LAUNCH(kern, dim3(cream_ln_partials()), dim3(256), 0, (hipStream_t)stream, dx, (uint16_t*)dx_scaled, partial,
                 (const uint16_t*)dy, x, mean, rstd, gamma, z, 1.f / (float)n_keep, dres, sample_scale, rows_per_sample, M, E);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int cream_mask_pack_check(const cream_mask_pack_job* jobs, int njobs)
{
    if (njobs < 0 || njobs > CREAM_MAX_MASK_JOBS) return CREAM_ERR_BAD_ARG;
    if (njobs == 0) return CREAM_OK;
    if (!jobs) return CREAM_ERR_BAD_ARG;
    int64_t tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        const cream_mask_pack_job& b = jobs[j];
        if (!b.w || (!b.mir && !b.mir_t) || b.rows <= 0 || b.cols <= 0 || b.cols % 4 || b.ld % 4 || b.ld < b.cols) return CREAM_ERR_BAD_ARG;
        if (b.c_group != 1 && b.c_group != 64) return CREAM_ERR_BAD_ARG;
        if (b.c && b.cols % b.c_group) return CREAM_ERR_BAD_ARG;
        if ((uintptr_t)b.w % 16 || (uintptr_t)b.r % 4 || (uintptr_t)b.c % 4) return CREAM_ERR_BAD_ARG;
        if (b.mir && (b.ld_mir % 4 || b.ld_mir < b.cols || (uintptr_t)b.mir % 8)) return CREAM_ERR_BAD_ARG;
        if (b.mir_t && (b.rows % 4 || b.ld_mir_t % 4 || b.ld_mir_t < b.rows || (uintptr_t)b.mir_t % 8)) return CREAM_ERR_BAD_ARG;
        tiles += (int64_t)tiles_of(b.rows) * tiles_of(b.cols);
    }
    return tiles > (1 << 24) ? CREAM_ERR_TOO_LARGE : CREAM_OK;
}

int cream_mask_pack(const cream_mask_pack_job* jobs, int njobs, void* stream)
{
    const int rc = cream_mask_pack_check(jobs, njobs);
    if (rc != CREAM_OK || njobs == 0) return rc;
    PackJobs J;
    J.njobs = njobs;
    int tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        J.job[j] = jobs[j];
        J.first[j] = tiles;
        tiles += tiles_of(jobs[j].rows) * tiles_of(jobs[j].cols);
    }
    J.first[njobs] = tiles;
    CREAM_LAUNCH(mask_pack_kernel, dim3(grid_cap(tiles, 8)), dim3(256), 0, (hipStream_t)stream, J);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int64_t cream_mask_grad_ws_floats(int rows, int cols)
{
    if (rows <= 0 || cols <= 0) return 0;
    return (int64_t)tiles_of(cols) * rows + (int64_t)gtiles_of(rows) * cols;
}

int cream_mask_grad_check(const cream_mask_grad_job* jobs, int njobs)
{
    if (njobs < 0 || njobs > CREAM_MAX_MASK_JOBS) return CREAM_ERR_BAD_ARG;
    if (njobs == 0) return CREAM_OK;
    if (!jobs) return CREAM_ERR_BAD_ARG;
    int64_t tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        const cream_mask_grad_job& b = jobs[j];
        if (!b.dst || !b.src || !b.w || b.nparts <= 0 || b.rows <= 0 || b.cols <= 0 || b.cols % 4 || b.ld % 4 || b.ld < b.cols ||
            b.ld_w % 4 || b.ld_w < b.cols || b.pstride % 4 || (b.nparts > 1 && b.pstride < (int64_t)b.rows * b.cols))
            return CREAM_ERR_BAD_ARG;
        if (b.c_group != 1 && b.c_group != 64) return CREAM_ERR_BAD_ARG;
        if ((b.c || b.dc_out) && b.cols % b.c_group) return CREAM_ERR_BAD_ARG;
        if ((b.dr_out || b.dc_out) && !b.ws) return CREAM_ERR_BAD_ARG;
        if (((uintptr_t)b.dst | (uintptr_t)b.w) % 16 || (uintptr_t)b.src % (b.src_bf16 ? 8 : 16)) return CREAM_ERR_BAD_ARG;
        if (((uintptr_t)b.r | (uintptr_t)b.c | (uintptr_t)b.dr_out | (uintptr_t)b.dc_out | (uintptr_t)b.ws) % 4) return CREAM_ERR_BAD_ARG;
        // every output of a launch has one writer: two jobs never share dst, a mask-gradient output or a workspace
        for (int i = 0; i < j; ++i) {
            const cream_mask_grad_job& a = jobs[i];
            const float* outs_a[4] = {a.dr_out, a.dc_out, a.ws, a.dst};
            const float* outs_b[4] = {b.dr_out, b.dc_out, b.ws, b.dst};
            for (const float* pa : outs_a)
                for (const float* pb : outs_b)
                    if (pa && pa == pb) return CREAM_ERR_BAD_ARG;
        }
        if (b.dr_out && b.dr_out == b.dc_out) return CREAM_ERR_BAD_ARG;
        tiles += (int64_t)gtiles_of(b.rows) * tiles_of(b.cols);
    }
    return tiles > (1 << 24) ? CREAM_ERR_TOO_LARGE : CREAM_OK;
}

int cream_mask_grad_finalize(const cream_mask_grad_job* jobs, int njobs, void* stream)
{
    const int rc = cream_mask_grad_check(jobs, njobs);
    if (rc != CREAM_OK || njobs == 0) return rc;
    MaskGradJobs J;
    J.njobs = njobs;
    int tiles = 0;
    for (int j = 0; j < njobs; ++j) {
        J.job[j] = jobs[j];
        J.first[j] = tiles;
        tiles += gtiles_of(jobs[j].rows) * tiles_of(jobs[j].cols);
    }
    J.first[njobs] = tiles;
    hipLaunchKernelGGL(mask_grad_tiles_kernel, dim3(grid_cap(tiles, 8)), dim3(256), 0, (hipStream_t)stream, J);
    if (hipGetLastError() != hipSuccess) return CREAM_ERR_LAUNCH;
    int blocks = 0;
    for (int j = 0; j < njobs; ++j) {
        J.first[j] = blocks;
        blocks += dr_blocks(jobs[j]) + dc_blocks(jobs[j]);
    }
    J.first[njobs] = blocks;
    if (blocks == 0) return CREAM_OK;
    CREAM_LAUNCH(mask_grad_reduce_kernel, dim3(grid_cap(blocks, 8)), dim3(256), 0, (hipStream_t)stream, J);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

}  // extern "C"

// pruned_ops.hip — what a pruned TinyCLIP tower (TinyCLIP/src/open_clip/model.py:139-205, :317-339: prune()) needs beyond the
// dense node's kernels (gfx950).  The tower runs on operands padded with zeros to the GEMM granularity (stream d -> Dp, MLP
// widths F_l -> Fp_l); parameters and gradients keep the compact shapes.  Two kernel groups, both bandwidth kernels:
//   a. compact gradient finalisation: split-K partials on the padded shape, summed on the tree of cream_grad_finalize
//      (grad_tree.hpp), stored into a compact fp32 gradient of any width and alignment;
//   b. pad / unpad of activation rows between (M, d) in the caller's dtype and (M, Dp) fp32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_common.hpp"
#include "cream_amd.h"
#include "grad_tree.hpp"
#include "launch_ev.hpp"

namespace {
using namespace cream;

// ---- a. compact gradient finalisation ---------------------------------------------------------------------------------------
struct CompactJobs {
    cream_grad_compact_job job[CREAM_MAX_COMPACT_JOBS];
    int first_block[CREAM_MAX_COMPACT_JOBS + 1];
    int njobs;
};

__host__ __device__ __forceinline__ int compact_chunk_width(const cream_grad_compact_job& b) { return b.src_bf16 ? 8 : 4; }
__host__ __device__ __forceinline__ int compact_chunks_per_row(const cream_grad_compact_job& b) {
    const int W = compact_chunk_width(b);
    return (b.cols + W - 1) / W;
}

// A chunk = W consecutive source columns of one row, from a multiple of W: the last chunk of a row may reach into the source's
// padding (ld_src % W == 0 and ld_src >= cols keep it inside the row); only its columns < cols are stored.
template <int W>
__device__ __forceinline__ void compact_job(const cream_grad_compact_job& jb, int block_in_job, PartChunk<W>* red) {
    const int CL = 256 / grad_part_lanes(jb.nparts);
    const int cpr = compact_chunks_per_row(jb);
    const int64_t nchunks = (int64_t)jb.rows * cpr;
    const int64_t chunk = (int64_t)block_in_job * CL + threadIdx.x % CL;
    const bool valid = chunk < nchunks;
    const int r = valid ? (int)(chunk / cpr) : 0;
    const int c = valid ? (int)(chunk - (int64_t)r * cpr) * W : 0;
    PartChunk<W> s;
    if (grad_tree_sum<W>(s, jb.src, jb.src_bf16 != 0, jb.nparts, jb.pstride, (int64_t)r * jb.ld_src + c, valid, red)) {
        float* d = jb.dst + (int64_t)r * jb.ld_dst + c;
        const int n = jb.cols - c < W ? jb.cols - c : W;
        if (n == W && ((uintptr_t)d & 15) == 0) {                  // a whole chunk on a 16-byte boundary of dst
            if (jb.overwrite) s.store(d);
            else s.add_into(d);
        } else {
#pragma unroll
            for (int e = 0; e < W; ++e)
                if (e < n) d[e] = jb.overwrite ? s.at(e) : d[e] + s.at(e);
        }
    }
}

__global__ __launch_bounds__(256) void grad_finalize_compact_kernel(const CompactJobs J) {
    __shared__ __attribute__((aligned(16))) char red[256 * sizeof(PartChunk<8>)];
    int j = 0;
    while (j + 1 < J.njobs && (int)blockIdx.x >= J.first_block[j + 1]) ++j;
    const cream_grad_compact_job& jb = J.job[j];
    const int b = (int)blockIdx.x - J.first_block[j];
    if (compact_chunk_width(jb) == 8) compact_job<8>(jb, b, reinterpret_cast<PartChunk<8>*>(red));
    else compact_job<4>(jb, b, reinterpret_cast<PartChunk<4>*>(red));
}

// ---- b. pad / unpad: a thread owns 4 consecutive columns of the padded row -----------------------------------------------------
template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<uint16_t>(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ uint16_t from_f32<uint16_t>(float v) { return (uint16_t)f2bf(v); }

template <typename T>
__global__ __launch_bounds__(256) void pad_cols_kernel(float* __restrict__ out, const T* __restrict__ in, int64_t nchunks, int d, int Dp) {
    const int cpr = Dp >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cpr;
        const int c = (int)(i - r * cpr) * 4;
        const T* src = in + r * d + c;
        f32x4v v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < d ? to_f32<T>(src[e]) : 0.f;
        *reinterpret_cast<f32x4v*>(out + r * Dp + c) = v;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void unpad_cols_kernel(T* __restrict__ out, const float* __restrict__ in, int64_t nchunks, int d, int Dp) {
    const int cpr = (d + 3) >> 2;                                  // only the chunks that hold a kept column
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cpr;
        const int c = (int)(i - r * cpr) * 4;
        const f32x4v v = *reinterpret_cast<const f32x4v*>(in + r * Dp + c);
        T* dst = out + r * d + c;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < d) dst[e] = from_f32<T>(v[e]);
    }
}

int grid_of(int64_t nchunks) {
    const int64_t b = (nchunks + 255) / 256;
    return (int)(b > 8192 ? 8192 : b);
}

int pad_args(const void* padded, const void* compact, int dtype, int M, int d, int Dp) {
    if (M < 0 || d <= 0 || Dp < d || Dp % 4) return CREAM_ERR_BAD_ARG;
    if (dtype != CREAM_F32 && dtype != CREAM_BF16) return CREAM_ERR_BAD_DTYPE;
    if (M == 0) return 1;
    if (!padded || !compact || (uintptr_t)padded % 16 || (uintptr_t)compact % (dtype == CREAM_F32 ? 4 : 2)) return CREAM_ERR_BAD_ARG;
    return CREAM_OK;
}

}  // namespace

extern "C" {

int cream_grad_finalize_compact_check(const cream_grad_compact_job* jobs, int njobs)
{
    if (njobs < 0 || njobs > CREAM_MAX_COMPACT_JOBS) return CREAM_ERR_BAD_ARG;
    if (njobs == 0) return CREAM_OK;
    if (!jobs) return CREAM_ERR_BAD_ARG;
    int64_t blocks = 0;
    for (int j = 0; j < njobs; ++j) {
        const cream_grad_compact_job& b = jobs[j];
        if (!b.dst || !b.src || b.nparts <= 0 || b.rows <= 0 || b.cols <= 0 || b.ld_dst < b.cols || b.ld_src < b.cols)
            return CREAM_ERR_BAD_ARG;
        const int W = compact_chunk_width(b);
        if (b.ld_src % W || b.pstride % W || b.pstride < 0) return CREAM_ERR_BAD_ARG;
        if ((uintptr_t)b.dst % 4 || (uintptr_t)b.src % 16) return CREAM_ERR_BAD_ARG;
        for (int i = 0; i < j; ++i)
            if (jobs[i].dst == b.dst) return CREAM_ERR_BAD_ARG;      // every destination has one writer
        const int CL = 256 / grad_part_lanes(b.nparts);
        blocks += ((int64_t)b.rows * compact_chunks_per_row(b) + CL - 1) / CL;
    }
    return blocks > ((int64_t)1 << 30) ? CREAM_ERR_TOO_LARGE : CREAM_OK;
}

int cream_grad_finalize_compact(const cream_grad_compact_job* jobs, int njobs, void* stream)
{
    const int rc = cream_grad_finalize_compact_check(jobs, njobs);
    if (rc != CREAM_OK || njobs == 0) return rc;
    CompactJobs J;
    J.njobs = njobs;
    int blocks = 0;
    for (int j = 0; j < njobs; ++j) {
        J.job[j] = jobs[j];
        J.first_block[j] = blocks;
        const int CL = 256 / grad_part_lanes(jobs[j].nparts);
        blocks += (int)(((int64_t)jobs[j].rows * compact_chunks_per_row(jobs[j]) + CL - 1) / CL);
    }
    J.first_block[njobs] = blocks;
    CREAM_LAUNCH(grad_finalize_compact_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, J);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int cream_pad_cols(float* out, const void* in, int in_dtype, int M, int d, int Dp, void* stream)
{
    const int rc = pad_args(out, in, in_dtype, M, d, Dp);
    if (rc) return rc < 0 ? rc : CREAM_OK;
    const int64_t nchunks = (int64_t)M * (Dp >> 2);
    if (in_dtype == CREAM_F32)
        hipLaunchKernelGGL(pad_cols_kernel<float>, dim3(grid_of(nchunks)), dim3(256), 0, (hipStream_t)stream, out, (const float*)in, nchunks, d, Dp);
    else
        hipLaunchKernelGGL(pad_cols_kernel<uint16_t>, dim3(grid_of(nchunks)), dim3(256), 0, (hipStream_t)stream, out, (const uint16_t*)in, nchunks, d, Dp);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int cream_unpad_cols(void* out, int out_dtype, const float* in, int M, int d, int Dp, void* stream)
{
    const int rc = pad_args(in, out, out_dtype, M, d, Dp);
    if (rc) return rc < 0 ? rc : CREAM_OK;
    const int64_t nchunks = (int64_t)M * ((d + 3) >> 2);
    if (out_dtype == CREAM_F32)
        hipLaunchKernelGGL(unpad_cols_kernel<float>, dim3(grid_of(nchunks)), dim3(256), 0, (hipStream_t)stream, (float*)out, in, nchunks, d, Dp);
    else
        hipLaunchKernelGGL(unpad_cols_kernel<uint16_t>, dim3(grid_of(nchunks)), dim3(256), 0, (hipStream_t)stream, (uint16_t*)out, in, nchunks, d, Dp);
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

}  // extern "C"

// grad_tree.hpp — the fixed summation tree of the gradient finalisation, shared by cream_grad_finalize (block_ops.hip: rows as
// wide as the destination's) and cream_grad_finalize_compact (pruned_ops.hip: padded source rows, compact destination).
//
// One workgroup of 256 threads = CL consecutive W-element chunks x PL part lanes (CL * PL = 256): part lane l adds parts
// l, l + PL, ... in ascending order, the lanes are combined in ascending order through LDS (PL = 64: 8 groups of 8 lanes, then
// the 8 sums).  The tree of an ELEMENT depends on nparts alone — not on W, on the chunk it sits in or on the grid — so every
// caller that walks it gets the same bits for the same parts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_common.hpp"

namespace cream {

// W = elements per chunk: 4 (fp32 partials, 16-byte loads) or 8 (bf16 partials with cols % 8 == 0: 16-byte loads too —
// at 4 elements a bf16 load is 8 bytes per lane, which the vector memory path serves at 0.54-0.70x the 16-byte rate)
template <int W> struct PartChunk;
template <> struct PartChunk<4> {
    f32x4v v;
    __device__ __forceinline__ void zero() { v = f32x4v{0, 0, 0, 0}; }
    __device__ __forceinline__ void add(const PartChunk& o) { v += o.v; }
    static __device__ __forceinline__ PartChunk load(const void* src, int64_t idx, bool is_bf16) {
        PartChunk c;
        if (is_bf16) {
            const u32x2v r = *reinterpret_cast<const u32x2v*>(reinterpret_cast<const uint16_t*>(src) + idx);
            c.v = f32x4v{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xFFFF0000u), __uint_as_float(r[1] << 16),
                         __uint_as_float(r[1] & 0xFFFF0000u)};
        } else {
            c.v = *reinterpret_cast<const f32x4v*>(reinterpret_cast<const float*>(src) + idx);
        }
        return c;
    }
    __device__ __forceinline__ float at(int e) const { return v[e]; }
    __device__ __forceinline__ void add_into(float* d) const {
        f32x4v o = *reinterpret_cast<f32x4v*>(d);
        o += v;
        *reinterpret_cast<f32x4v*>(d) = o;
    }
    __device__ __forceinline__ void store(float* d) const { *reinterpret_cast<f32x4v*>(d) = v; }
};
template <> struct PartChunk<8> {                                  // bf16 sources only
    f32x4v lo, hi;
    __device__ __forceinline__ void zero() { lo = f32x4v{0, 0, 0, 0}; hi = lo; }
    __device__ __forceinline__ void add(const PartChunk& o) { lo += o.lo; hi += o.hi; }
    static __device__ __forceinline__ PartChunk load(const void* src, int64_t idx, bool) {
        const u32x4v r = *reinterpret_cast<const u32x4v*>(reinterpret_cast<const uint16_t*>(src) + idx);
        PartChunk c;
        c.lo = f32x4v{__uint_as_float(r[0] << 16), __uint_as_float(r[0] & 0xFFFF0000u), __uint_as_float(r[1] << 16),
                      __uint_as_float(r[1] & 0xFFFF0000u)};
        c.hi = f32x4v{__uint_as_float(r[2] << 16), __uint_as_float(r[2] & 0xFFFF0000u), __uint_as_float(r[3] << 16),
                      __uint_as_float(r[3] & 0xFFFF0000u)};
        return c;
    }
    __device__ __forceinline__ float at(int e) const { return e < 4 ? lo[e] : hi[e - 4]; }
    __device__ __forceinline__ void add_into(float* d) const {
        f32x4v o0 = *reinterpret_cast<f32x4v*>(d), o1 = *reinterpret_cast<f32x4v*>(d + 4);
        o0 += lo;
        o1 += hi;
        *reinterpret_cast<f32x4v*>(d) = o0;
        *reinterpret_cast<f32x4v*>(d + 4) = o1;
    }
    __device__ __forceinline__ void store(float* d) const {
        *reinterpret_cast<f32x4v*>(d) = lo;
        *reinterpret_cast<f32x4v*>(d + 4) = hi;
    }
};

// part lanes per chunk: a lane walks its parts four loads at a time, so the dependent chain of a job is nparts / (4 PL)
// round trips — the LayerNorm jobs (1024 slab partials of a few hundred columns) set the kernel's duration at PL = 16
// (16 round trips on 6 workgroups while the chip idles): 64 lanes there
__host__ __device__ __forceinline__ int grad_part_lanes(int nparts) { return nparts <= 16 ? 4 : (nparts <= 64 ? 16 : 64); }

// The tree over the parts of one chunk per (threadIdx.x % CL): the chunk starts `off` elements into part 0, parts are `pstride`
// elements apart.  Every thread of the workgroup calls it (barriers inside); `valid` = the thread's chunk exists.  Returns true
// in the one thread per valid chunk (part lane 0) that then holds the sum in `s`.  red: 256 chunks of LDS.
template <int W>
__device__ __forceinline__ bool grad_tree_sum(PartChunk<W>& s, const void* src, bool bf, int nparts, int64_t pstride, int64_t off,
                                              bool valid, PartChunk<W>* red) {
    const int PL = grad_part_lanes(nparts), CL = 256 / PL;
    const int cl = threadIdx.x % CL, pl = threadIdx.x / CL;
    PartChunk<W> acc;
    acc.zero();
    if (valid) {
        int p = pl;
        for (; p + 3 * PL < nparts; p += 4 * PL) {                 // four loads in flight
            const PartChunk<W> a0 = PartChunk<W>::load(src, (int64_t)p * pstride + off, bf);
            const PartChunk<W> a1 = PartChunk<W>::load(src, (int64_t)(p + PL) * pstride + off, bf);
            const PartChunk<W> a2 = PartChunk<W>::load(src, (int64_t)(p + 2 * PL) * pstride + off, bf);
            const PartChunk<W> a3 = PartChunk<W>::load(src, (int64_t)(p + 3 * PL) * pstride + off, bf);
            acc.add(a0); acc.add(a1); acc.add(a2); acc.add(a3);
        }
        for (; p < nparts; p += PL) acc.add(PartChunk<W>::load(src, (int64_t)p * pstride + off, bf));
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (PL == 64) {                                                // two levels (fixed order): 8 groups of 8 lanes, then the 8 sums
        if (pl < 8) {
            PartChunk<W> g = red[(8 * pl) * CL + cl];
            for (int l = 1; l < 8; ++l) g.add(red[(8 * pl + l) * CL + cl]);
            acc = g;
        }
        __syncthreads();
        if (pl < 8) red[pl * CL + cl] = acc;
        __syncthreads();
    }
    if (pl != 0 || !valid) return false;
    const int nl = PL == 64 ? 8 : PL;
    s = red[cl];
    for (int l = 1; l < nl; ++l) s.add(red[l * CL + cl]);
    return true;
}

}  // namespace cream

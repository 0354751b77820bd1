// sparse_distill.hip — the two kernels of TinyViT's fast pretraining distillation (gfx950), one workgroup per row.
//
// Reference semantics: the teacher's soft labels are stored once as sparse records — per image an int32 augmentation
// seed and the top-k softmax probabilities as int16 index / fp16 value (TinyViT/save_logits.py:135-158) — and the student
// trains on the dense target rebuilt from them (TinyViT/main.py:321-330):
//     minor = (1 - sum_j v_j) / (C - k);   t_c = v_j at c = index_j, minor elsewhere;   loss = SoftTargetCrossEntropy(x, t).
//
// sparse_ce_kernel: loss row and dense logit gradient from the SPARSE target; no B x C target exists anywhere.
//   The closed form the kernel evaluates (tests/test_sparse_distill_ref_cpu.py pins it against the dense formulation):
//     loss = minor * sum_{c not in index} (lse - x_c) + sum_j v_j (lse - x_{index_j}),     lse = max + log sum exp(x - max)
//     dx_c = (exp(x_c - max) / se * st - t_c) * grad_scale,                                st = minor (C - k) + sum_j v_j
//   Every term lse - x_c is non-negative and they are summed as terms (never C * lse - sum x, which cancels).
//   The row is read from HBM ONCE: it stays in LDS in its own element type (64 KB for bf16, 128 KB for fp32 at C = 32768,
//   dynamic LDS raised to 160 KB) for the exp-sum pass and the gradient pass.  Rows of odd length start at the element's
//   own alignment only: the loader takes a scalar head up to the next 16-byte boundary, 16-byte vectors for the body and a
//   scalar tail; the LDS image keeps the row's offset within its 16 bytes, so the vector stores into LDS are aligned too.
//   The k patched classes are marked in an LDS bitmap before the gradient pass: the dense pass skips marked classes, the
//   k owner threads store them — ONE store per address.  An index outside [0, C) is never dereferenced: its entry
//   contributes to `minor` (which is defined on the values alone) and to nothing else.
//
// softmax_topk_kernel: logits -> softmax -> top-k, largest first, straight into the record layout.  The order is defined
//   on the LOGITS (softmax is monotone): larger logit first, equal logits by ascending class index.  Order-preserving 32-bit
//   keys (-0 folded onto +0); a 4 x 8-bit radix select with an LDS histogram finds the k-th largest key and how many of
//   its ties to admit; every thread owns a CONTIGUOUS run of classes, so an exclusive scan of the per-thread tie counts
//   ranks the ties in index order; at most 128 candidates are compacted and rank-sorted on (key descending, index
//   ascending) in LDS.  Values are the fp32 softmax rounded to nearest-even fp16 by integer arithmetic, subnormals kept.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cream_amd.h"
#include "launch_ev.hpp"

namespace {

constexpr int NT = 1024;             // threads per workgroup: B is small (128 rows on 256 CUs), the row is long
constexpr int NW = NT / 64;
constexpr int MAXK = 128, MAXC = 32768;

template <typename TX> __device__ __forceinline__ float to_f32(TX v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<uint16_t>(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

// ONE dynamic LDS block per kernel, as in the other kernels that raise the dynamic limit to 160 KB (with static arrays
// beside it the launch was refused with an invalid-argument error): the small arrays first, the row image behind them at
// a 16-byte boundary
struct CeLds {
    float red[NW];
    uint32_t marked[MAXC / 32];
};
struct TopkLds {
    unsigned long long cand[MAXK], sorted[MAXK];
    float red[NW];
    int wsum[NW], hist[256], rank[MAXK];
    uint32_t sel[2];
    int ncand, reserved;
};
template <typename L> __host__ __device__ constexpr size_t lds_head() { return (sizeof(L) + 15) & ~(size_t)15; }

template <typename TX> struct alignas(16) Vec16 { TX e[16 / sizeof(TX)]; };

// elements by which the row's first element is off a 16-byte boundary: the LDS image starts at the same offset
template <typename TX> __device__ __forceinline__ int row_pad(const TX* x) { return (int)(((uintptr_t)x & 15) / sizeof(TX)); }

// global row -> LDS image (srow[pad + c] = x[c]), returns this thread's maximum
template <typename TX>
__device__ __forceinline__ float load_row(TX* srow, const TX* __restrict__ x, int C, int pad, int tid)
{
    constexpr int VEC = 16 / sizeof(TX);
    const int head = min(C, (VEC - pad) % VEC);
    const int nvec = (C - head) / VEC, tail = head + nvec * VEC;
    float mx = -INFINITY;
    if (tid < head) { const TX v = x[tid]; srow[pad + tid] = v; mx = to_f32(v); }
    for (int i = tid; i < nvec; i += NT) {
        const Vec16<TX> q = *reinterpret_cast<const Vec16<TX>*>(x + head + i * VEC);
        *reinterpret_cast<Vec16<TX>*>(srow + pad + head + i * VEC) = q;
#pragma unroll
        for (int e = 0; e < VEC; ++e) mx = fmaxf(mx, to_f32(q.e[e]));
    }
    const int c = tail + tid;
    if (c < C) { const TX v = x[c]; srow[pad + c] = v; mx = fmaxf(mx, to_f32(v)); }
    return mx;
}

// fixed-order reductions over the workgroup; `red` has NW floats and is free again after the trailing barrier
__device__ __forceinline__ float block_sum(float v, float* red, int tid)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += red[w];
    __syncthreads();
    return s;
}
__device__ __forceinline__ float block_max(float v, float* red, int tid)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float s = -INFINITY;
#pragma unroll
    for (int w = 0; w < NW; ++w) s = fmaxf(s, red[w]);
    __syncthreads();
    return s;
}
// exclusive prefix sum over the threads in thread order
__device__ __forceinline__ int block_scan(int v, int* wsum, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) before += w < wave ? wsum[w] : 0;
    __syncthreads();
    return before + inc - v;
}

// ---- loss rows + dense gradient from sparse targets ---------------------------------------------------------------------
template <typename TX>
__global__ __launch_bounds__(NT) void sparse_ce_kernel(float* __restrict__ loss_rows, float* __restrict__ dlogits,
                                                       const TX* __restrict__ logits, const int16_t* __restrict__ index,
                                                       const uint16_t* __restrict__ value, int C, int k, float gscale)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    CeLds& lds = *reinterpret_cast<CeLds*>(smem);
    float* red = lds.red;
    uint32_t* marked = lds.marked;
    TX* srow = reinterpret_cast<TX*>(smem + lds_head<CeLds>());
    const int row = blockIdx.x, tid = threadIdx.x;
    const TX* x = logits + (int64_t)row * C;
    const int pad = row_pad(x);

    // the sparse entry of this thread (tid < k); the half is widened exactly
    int idx = -1;
    float val = 0.f;
    if (tid < k) {
        idx = index[(int64_t)row * k + tid];
        val = (float)*reinterpret_cast<const _Float16*>(value + (int64_t)row * k + tid);
    }
    const bool valid = idx >= 0 && idx < C;
    for (int i = tid; i < MAXC / 32; i += NT) marked[i] = 0u;

    const float mx = block_max(load_row(srow, x, C, pad, tid), red, tid);         // barrier: row and bitmap are in LDS
    if (valid) atomicOr(&marked[idx >> 5], 1u << (idx & 31));
    float se = 0.f;
    for (int c = tid; c < C; c += NT) se += expf(to_f32(srow[pad + c]) - mx);
    se = block_sum(se, red, tid);                                                 // barrier: the bitmap is complete
    const float sv = block_sum(val, red, tid);
    const float svv = block_sum(valid ? val : 0.f, red, tid);
    const float nvalid = block_sum(valid ? 1.f : 0.f, red, tid);
    const float minor = (1.f - sv) / (float)(C - k);
    const float st = minor * ((float)C - nvalid) + svv;
    const float lse = mx + logf(se), inv = 1.f / se;

    float* d = dlogits + (int64_t)row * C;
    float loss = 0.f;
    for (int c = tid; c < C; c += NT) {
        if (marked[c >> 5] >> (c & 31) & 1u) continue;                            // stored by its owner below
        const float xc = to_f32(srow[pad + c]);
        loss += minor * (lse - xc);
        d[c] = (expf(xc - mx) * inv * st - minor) * gscale;
    }
    if (valid) {
        const float xc = to_f32(srow[pad + idx]);
        loss += val * (lse - xc);
        d[idx] = (expf(xc - mx) * inv * st - val) * gscale;
    }
    loss = block_sum(loss, red, tid);
    if (tid == 0) loss_rows[row] = loss;
}

// ---- softmax -> top-k -> records ------------------------------------------------------------------------------------------
// larger logit <=> larger key; -0 and +0 share a key (they compare equal)
__device__ __forceinline__ uint32_t order_key(float f)
{
    const uint32_t u = __float_as_uint(f + 0.f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// fp32 -> fp16 bits, round to nearest even, subnormals kept, for 0 <= f <= 1 (no overflow, no NaN)
__device__ __forceinline__ uint16_t f32_to_f16_rne(float f)
{
    uint32_t u = __float_as_uint(f);
    if (u < 0x38800000u) {                                                        // below 2^-14: a multiple of 2^-24
        const float m = f + 0.5f;                                                 // one ulp of 0.5f is 2^-24: the add rounds
        return (uint16_t)(__float_as_uint(m) - 0x3F000000u);
    }
    u += 0xC8000FFFu + ((u >> 13) & 1u);                                          // rebias the exponent, round the 13 lost bits
    return (uint16_t)(u >> 13);
}

template <typename TX>
__global__ __launch_bounds__(NT) void softmax_topk_kernel(uint8_t* __restrict__ records, const TX* __restrict__ logits,
                                                          const int32_t* __restrict__ seeds, int C, int k)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TopkLds& lds = *reinterpret_cast<TopkLds*>(smem);
    float* red = lds.red;
    int *wsum = lds.wsum, *hist = lds.hist, *rank = lds.rank;
    uint32_t* sel = lds.sel;                                                      // prefix of the k-th key so far, ties still wanted
    int& ncand = lds.ncand;
    unsigned long long *cand = lds.cand, *sorted = lds.sorted;
    TX* srow = reinterpret_cast<TX*>(smem + lds_head<TopkLds>());
    const int row = blockIdx.x, tid = threadIdx.x;
    const TX* x = logits + (int64_t)row * C;
    const int pad = row_pad(x);

    if (tid < MAXK) { cand[tid] = 0ull; sorted[tid] = 0ull; rank[tid] = 0; }
    if (tid == 0) { sel[0] = 0u; sel[1] = (uint32_t)k; ncand = 0; }
    const float mx = block_max(load_row(srow, x, C, pad, tid), red, tid);
    float se = 0.f;
    for (int c = tid; c < C; c += NT) se += expf(to_f32(srow[pad + c]) - mx);
    se = block_sum(se, red, tid);

    // radix select, most significant byte first: after pass p the top 8 (p + 1) bits of the k-th largest key are known
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = sel[0], want = sel[1];
        const uint32_t himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        for (int c = tid; c < C; c += NT) {
            const uint32_t key = order_key(to_f32(srow[pad + c]));
            if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        // thread t < 256 looks at digit 255 - t: the inclusive scan counts the keys with this digit or a larger one
        const int digit = 255 - tid, h = tid < 256 ? hist[digit & 255] : 0;
        const int above = block_scan(h, wsum, tid);                               // keys with a larger digit
        if (tid < 256 && (uint32_t)above < want && (uint32_t)(above + h) >= want) {
            sel[0] = prefix | ((uint32_t)digit << shift);
            sel[1] = want - (uint32_t)above;
        }
        __syncthreads();
    }
    const uint32_t kth = sel[0];
    const int ties_wanted = (int)sel[1];

    // every thread owns a contiguous run of classes: the scan of the tie counts is in index order
    const int per = (C + NT - 1) / NT, c0 = min(C, tid * per), c1 = min(C, c0 + per);
    int eq = 0;
    for (int c = c0; c < c1; ++c) eq += order_key(to_f32(srow[pad + c])) == kth ? 1 : 0;
    int tie = block_scan(eq, wsum, tid);
    for (int c = c0; c < c1; ++c) {
        const uint32_t key = order_key(to_f32(srow[pad + c]));
        bool take = key > kth;
        if (key == kth) { take = tie < ties_wanted; ++tie; }
        if (take) {
            const int slot = atomicAdd(&ncand, 1);
            if (slot < MAXK) cand[slot] = ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)c;
        }
    }
    __syncthreads();
    // rank sort: the composites are distinct (distinct classes), a larger one comes first; empty slots are 0 and come last
    {
        const int i = tid & (MAXK - 1), part = tid / MAXK;                        // 8 parts of 16 rivals each
        const unsigned long long mine = cand[i];
        int r = 0;
#pragma unroll
        for (int j = 0; j < MAXK / (NT / MAXK); ++j) r += cand[part * (MAXK / (NT / MAXK)) + j] > mine ? 1 : 0;
        if (r) atomicAdd(&rank[i], r);
    }
    __syncthreads();
    if (tid < MAXK && cand[tid] != 0ull) sorted[rank[tid]] = cand[tid];           // ranks of the real entries: 0 .. ncand - 1
    __syncthreads();
    uint8_t* rec = records + (int64_t)row * (4 + 4 * k);
    if (tid == 0) *reinterpret_cast<int32_t*>(rec) = seeds[row];
    if (tid < k) {
        const unsigned long long e = sorted[tid];
        const int c = (int)(~(uint32_t)e);
        const bool ok = e != 0ull && c >= 0 && c < C;                             // always true for finite logits
        const float p = ok ? expf(to_f32(srow[pad + c]) - mx) / se : 0.f;
        reinterpret_cast<int16_t*>(rec + 4)[tid] = (int16_t)(ok ? c : 0);
        reinterpret_cast<uint16_t*>(rec + 4 + 2 * k)[tid] = f32_to_f16_rne(p);
    }
}

// the small arrays, then the row image with up to 16 bytes of leading offset
size_t lds_bytes(size_t head, size_t elem, int C) { return head + (((size_t)C * elem + 16 + 15) & ~(size_t)15); }

template <typename K> bool raise_lds(K kern) { return cream::raise_dynamic_lds(kern, 160 * 1024); }

}  // namespace

extern "C" {

int cream_sparse_ce(float* loss_rows, float* dlogits, const void* logits, const int16_t* index, const void* value, int B, int C,
                    int k, int logits_dtype, float grad_scale, void* stream)
{
    if (B < 0 || C <= 0 || k <= 0) return CREAM_ERR_BAD_ARG;
    if (k > MAXK || C > MAXC) return CREAM_ERR_TOO_LARGE;
    if (k >= C) return CREAM_ERR_BAD_ARG;
    if (!loss_rows || !dlogits || !logits || !index || !value) return CREAM_ERR_BAD_ARG;
    if (logits_dtype != CREAM_BF16 && logits_dtype != CREAM_F32) return CREAM_ERR_BAD_DTYPE;
    const uintptr_t xa = (uintptr_t)logits;
    if ((xa & (logits_dtype == CREAM_BF16 ? 1 : 3)) || ((uintptr_t)loss_rows & 3) || ((uintptr_t)dlogits & 3) ||
        ((uintptr_t)index & 1) || ((uintptr_t)value & 1))
        return CREAM_ERR_BAD_ARG;
    if (B == 0) return CREAM_OK;
    hipStream_t st = (hipStream_t)stream;
    if (logits_dtype == CREAM_BF16) {
        if (!raise_lds(sparse_ce_kernel<uint16_t>)) return CREAM_ERR_LAUNCH;
        hipLaunchKernelGGL(sparse_ce_kernel<uint16_t>, dim3(B), dim3(NT), lds_bytes(lds_head<CeLds>(), 2, C), st, loss_rows, dlogits,
                           (const uint16_t*)logits, index, (const uint16_t*)value, C, k, grad_scale);
    } else {
        if (!raise_lds(sparse_ce_kernel<float>)) return CREAM_ERR_LAUNCH;
        hipLaunchKernelGGL(sparse_ce_kernel<float>, dim3(B), dim3(NT), lds_bytes(lds_head<CeLds>(), 4, C), st, loss_rows, dlogits,
                           (const float*)logits, index, (const uint16_t*)value, C, k, grad_scale);
    }
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

int cream_softmax_topk_records(void* records, const void* logits, const int32_t* seeds, int B, int C, int k, int logits_dtype,
                               void* stream)
{
    if (B < 0 || C <= 0 || k <= 0) return CREAM_ERR_BAD_ARG;
    if (k > MAXK || C > MAXC) return CREAM_ERR_TOO_LARGE;
    if (k > C) return CREAM_ERR_BAD_ARG;
    if (!records || !logits || !seeds) return CREAM_ERR_BAD_ARG;
    if (logits_dtype != CREAM_BF16 && logits_dtype != CREAM_F32) return CREAM_ERR_BAD_DTYPE;
    if (((uintptr_t)logits & (logits_dtype == CREAM_BF16 ? 1 : 3)) || ((uintptr_t)records & 3) || ((uintptr_t)seeds & 3))
        return CREAM_ERR_BAD_ARG;
    if (B == 0) return CREAM_OK;
    hipStream_t st = (hipStream_t)stream;
    if (logits_dtype == CREAM_BF16) {
        if (!raise_lds(softmax_topk_kernel<uint16_t>)) return CREAM_ERR_LAUNCH;
        hipLaunchKernelGGL(softmax_topk_kernel<uint16_t>, dim3(B), dim3(NT), lds_bytes(lds_head<TopkLds>(), 2, C), st, (uint8_t*)records,
                           (const uint16_t*)logits, seeds, C, k);
    } else {
        if (!raise_lds(softmax_topk_kernel<float>)) return CREAM_ERR_LAUNCH;
        hipLaunchKernelGGL(softmax_topk_kernel<float>, dim3(B), dim3(NT), lds_bytes(lds_head<TopkLds>(), 4, C), st, (uint8_t*)records,
                           (const float*)logits, seeds, C, k);
    }
    return hipGetLastError() == hipSuccess ? CREAM_OK : CREAM_ERR_LAUNCH;
}

}  // extern "C"
